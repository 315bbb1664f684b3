"""CPU: the host side of step 2's driver (bridged_gnn_amd.transfer): sklearn's numbers from integer confusion counts and from the
tie-aware rank statistic, against the values the reference's own `test` / `get_each_clf_res` recorded in
tests/golden/transfer_office_a2d.npz (tools/gen_golden_transfer.py) and against sklearn itself; the command line."""
import os

import numpy as np
import pytest

from bridged_gnn_amd import transfer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = "transfer_office_a2d.npz"


def confusion(y, pred, C):
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (y, pred), 1)
    return cm


def rank_counts(score, y):
    """(u2, n_pos, n_neg) as ops.step2_auc counts them"""
    pos, neg = score[y == 1], np.sort(score[y == 0])
    lb, ub = np.searchsorted(neg, pos, "left"), np.searchsorted(neg, pos, "right")
    return int((2 * lb + (ub - lb)).sum()), pos.size, neg.size


def selections(g, pre):
    """the row selections `test` and `get_each_clf_res` score (main_graph_knowledge_transfer.py:82-105, :124-131)"""
    tgt = ~g[pre + "central_mask"]
    return g[pre + "train_mask"], g[pre + "val_mask"] & tgt, g[pre + "test_mask"] & tgt


def test_office_scores_from_counts_match_the_reference(golden):
    g = golden(FIX)
    og = golden("office_a2d_graph.npz")
    y = og["y"]
    train = og["train_mask"] & (y != -1)
    tgt = ~og["central_mask"]
    assert not (og["val_mask"] & ~tgt).any() and not (og["test_mask"] & ~tgt).any()
    sels = (train, og["val_mask"] & tgt, og["test_mask"] & tgt)
    pred = {k: g[f"office/pred_{k}"].astype(np.int64) for k in "sth"}
    cms = [confusion(y[m], pred[k][m], 31) for k, m in zip("shh", sels)]
    for i, cm in enumerate(cms):
        assert abs(transfer.f1_from_counts(cm, "macro") - g["office/test_f1"][i]) <= 1e-12
        assert abs(transfer.f1_from_counts(cm, "micro") - g["office/test_f1_micro"][i]) <= 1e-12
        assert abs(transfer.accuracy_from_counts(cm) - g["office/test_acc"][i]) <= 1e-12
    for i, k in enumerate("sth"):
        cm = confusion(y[sels[2]], pred[k][sels[2]], 31)
        assert abs(transfer.f1_from_counts(cm) - g["office/each_f1"][i]) <= 1e-12


@pytest.mark.parametrize("pre", ["bin/", "bin/tie/"])
def test_binary_scores_and_tie_aware_auc_match_the_reference(golden, pre):
    g = golden(FIX)
    y = g["bin/y"]
    sels = selections(g, "bin/")
    for i, (k, m) in enumerate(zip("shh", sels)):
        lp = g[f"{pre}lp_{k}"]
        top = np.sort(lp, 1)
        assert (top[m, 1] > top[m, 0]).all() or pre == "bin/tie/"         # the plain fixture is tie-free on its scored rows
        cm = confusion(y[m], lp.argmax(1)[m], 2)                          # argmax: the lowest index on a tie, like max(1)[1] here
        assert abs(transfer.f1_from_counts(cm, "macro") - g[pre + "test_f1"][i]) <= 1e-12
        assert abs(transfer.f1_from_counts(cm, "micro") - g[pre + "test_f1_micro"][i]) <= 1e-12
        assert abs(transfer.accuracy_from_counts(cm) - g[pre + "test_acc"][i]) <= 1e-12
        auc = transfer.auc_from_rank_counts(*rank_counts(g[f"{pre}score_{k}"][m], y[m]))
        assert abs(auc - g[pre + "test_auc"][i]) <= 1e-12
    for i, k in enumerate("sth"):
        m = sels[2]
        assert abs(transfer.auc_from_rank_counts(*rank_counts(g[f"{pre}score_{k}"][m], y[m])) - g[pre + "each_auc"][i]) <= 1e-12
        cm = confusion(y[m], g[f"{pre}lp_{k}"].argmax(1)[m], 2)
        assert abs(transfer.f1_from_counts(cm) - g[pre + "each_f1"][i]) <= 1e-12
    if pre == "bin/tie/":
        assert int(g["bin/tie/n_tied"]) > 0


def test_scores_from_random_counts_match_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    for trial in range(40):
        C = int(rng.integers(2, 9))
        n = int(rng.integers(1, 400))
        # labels absent from y_true, from y_pred, or from both
        true_pool = rng.choice(C, size=int(rng.integers(1, C + 1)), replace=False)
        pred_pool = rng.choice(C, size=int(rng.integers(1, C + 1)), replace=False)
        y, p = rng.choice(true_pool, n), rng.choice(pred_pool, n)
        cm = confusion(y, p, C)
        assert abs(transfer.f1_from_counts(cm, "macro") - sk.f1_score(y, p, average="macro")) <= 1e-12
        assert abs(transfer.f1_from_counts(cm, "micro") - sk.f1_score(y, p, average="micro")) <= 1e-12
        assert abs(transfer.accuracy_from_counts(cm) - sk.accuracy_score(y, p)) <= 1e-12
    for trial in range(40):
        n = int(rng.integers(4, 500))
        y = rng.integers(0, 2, n)
        y[:2] = (0, 1)
        score = np.round(rng.random(n), int(rng.integers(1, 4))).astype(np.float32)      # coarse scores: many ties
        assert abs(transfer.auc_from_rank_counts(*rank_counts(score, y)) - sk.roc_auc_score(y, score)) <= 1e-12


def test_auc_of_one_class_raises_like_sklearn():
    with pytest.raises(ValueError, match="Only one class"):
        transfer.auc_from_rank_counts(0, 5, 0)
    with pytest.raises(ValueError, match="Only one class"):
        transfer.auc_from_rank_counts(0, 0, 5)
    with pytest.raises(NotImplementedError):
        transfer.score_from_counts(np.eye(2), "precision")


def test_best_epoch_rule_on_non_monotone_histories():
    """main_graph_knowledge_transfer.py:238 / :374: strictly below the best so far, which starts at 666"""
    sel = transfer.select_best
    assert sel([3.0, 2.0, 2.5, 1.0, 1.5, 0.5, 0.7]) == [0, 1, 3, 5]                  # not 'the last epoch', not every epoch
    assert sel([2.0, 1.0, 1.0, 3.0]) == [0, 1]                                        # a tie keeps the EARLIER epoch ('<', not '<=')
    assert sel([700.0, 666.0, 665.9]) == [2]                                          # the start value 666 has to be beaten
    assert sel([700.0, 900.0]) == [] and sel([]) == []
    assert sel([float("nan"), 2.0, float("nan"), 1.0]) == [1, 3]                      # NaN never wins
    assert sel([0.4], 0.5) == [0] and sel([0.5], 0.5) == []                           # continuing from a running best
    rng = np.random.default_rng(3)
    for _ in range(20):
        v = rng.random(30).astype(np.float32).tolist()
        assert sel(v)[-1] == int(np.argmin(v))


RUN_SH_STEP2 = (
    "--num_layer 2 --hidden_dim 128 --path_data ../data_bridged_graph/twitter_unrelational_bridged_graph.dat --to_undirected",
    "--num_layer 2 --hidden_dim 64 --path_data ../data_bridged_graph/office_amazon2dslr_bridged_graph.dat --to_undirected",
    "--num_layer 2 --hidden_dim 128 --path_data ../data_bridged_graph/office_amazon2webcam_bridged_graph.dat --to_undirected",
    "--num_epoch 300 --num_layer 2 --hidden_dim 64 --path_data ../data_bridged_graph/fb_hamilton2caltech_bridged_graph.dat --to_undirected --no_dtc",
    "--num_epoch 200 --num_layer 2 --hidden_dim 64 --path_data ../data_bridged_graph/fb_howard2simmons_bridged_graph.dat",
)


@pytest.mark.parametrize("line", RUN_SH_STEP2)
def test_parser_accepts_the_references_step2_command_lines(line):
    """the five `python main_graph_knowledge_transfer.py ...` lines of the reference's run.sh, verbatim"""
    a = transfer.build_parser().parse_args(line.split())
    assert a.num_layer == 2 and a.path_data.endswith("_bridged_graph.dat") and a.model_name == "KTGNN" and a.eval_metric == "f1"
    assert a.no_dtc == ("--no_dtc" in line) and a.to_undirected == ("--to_undirected" in line)
    assert a.num_epoch == (int(line.split()[1]) if line.startswith("--num_epoch") else 300) and a.gpu == 0 and not a.save


def test_reference_names_and_defaults():
    import inspect
    sig = inspect.signature(transfer.train_gnn).parameters
    ref = dict(save=False, repeat=3, num_epoch=200, gnn="GCN", seed=None, step_size=100, gamma=0.1, num_layer=2, hidden=64, lr=1e-3, wd=5e-3,
               use_shceduler=True, step=1, Lambda=1., f1_average="macro", metric="f1", noDTC=False)
    assert list(sig)[:3] == ["args", "dataset", "data"] and list(sig)[3:3 + len(ref)] == list(ref)
    assert all(sig[k].default == v for k, v in ref.items())
    assert sig["dropout"].default == 0.5 and sig["verbose"].default is True
    sig = inspect.signature(transfer.train_gnn_noDTC).parameters
    ref = dict(save=False, repeat=3, num_epoch=200, gnn="GCN", seed=None, num_layer=2, hidden=64, lr=1e-3, wd=5e-3, use_scheduler=True, step=1,
               step_size=100, gamma=0.1, metric="f1", f1_average="macro")
    assert list(sig)[3:3 + len(ref)] == list(ref) and all(sig[k].default == v for k, v in ref.items())
    assert list(inspect.signature(transfer.train).parameters)[:6] == ["data", "model", "optimizer", "clip_grad", "gnn", "Lambda"]
    assert list(inspect.signature(transfer.test).parameters) == ["data", "model", "dataset_name", "gnn", "metric", "f1_average"]
    assert list(inspect.signature(transfer.get_each_clf_res).parameters) == ["data", "model", "metric", "f1_average"]
    for name in ("pyg_dataset", "train_noDTC", "test_noDTC", "main"):
        assert hasattr(transfer, name)
    with pytest.raises(NotImplementedError):
        transfer.train_gnn(None, None, None, gnn="GCN")
    with pytest.raises(NotImplementedError):
        transfer.train(None, None, None, gnn="GCN")


def test_step2_entries_are_bound():
    from bridged_gnn_amd import _lib, ops
    for n in ("loss_workspace_bytes", "loss_f32", "loss_bwd_f32", "nll_f32", "nll_bwd_f32", "counts_f32", "auc_count_f32"):
        assert "bgnn_step2_" + n in _lib.SIGNATURES
    assert "bgnn_step2.hip" in _lib._HASHED_SOURCES and _lib.ABI_VERSION == 116
    for n in ("step2_loss", "step2_nll", "step2_counts", "step2_auc"):
        assert callable(getattr(ops, n))
    import torch
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.step2_loss(torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64),
                       torch.ones(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool))
