"""GPU: `train_gnn(graphed=True)` / `train_gnn_noDTC(graphed=True)` -- every epoch one replay of a captured HIP graph -- is the eager
run: against the reference's recorded run, against `graphed=False` under dropout, and in what it leaves behind."""
import os
import types

import numpy as np
import pytest
import torch

from test_gpu_transfer import DEV, FIX, TRAJ_RTOL, build_ktgnn, office_data

pytestmark = pytest.mark.gpu
ARGS = types.SimpleNamespace(dataset_name="office")


def grab_models(monkeypatch):
    """the models the drivers build (they do not return them): `_prime` sees each one first"""
    from bridged_gnn_amd import transfer
    seen, prime0 = [], transfer._prime

    def prime(model, *a, **k):
        seen.append(model)
        return prime0(model, *a, **k)
    monkeypatch.setattr(transfer, "_prime", prime)
    return seen


def run_dtc(data, graphed, hist=None, **kw):
    from bridged_gnn_amd import transfer
    cfg = dict(repeat=1, num_epoch=8, step_size=3, gamma=0.1, gnn="KTGNN", seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)
    cfg.update(kw)
    return transfer.train_gnn(ARGS, transfer.pyg_dataset(data), data, history=hist, graphed=graphed, **cfg)


def run_plain(data, graphed, hist, **kw):
    from bridged_gnn_amd import transfer
    cfg = dict(repeat=1, num_epoch=8, step_size=3, gamma=0.1, gnn="GraphSAGE", seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)
    cfg.update(kw)
    return transfer.train_gnn_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, graphed=graphed, **cfg)


def series(lb):
    return np.array([lb["source&target"], lb["target_hat"], lb["target"], lb["kl"]]).T


def test_graphed_train_gnn_follows_the_references_recorded_run(golden):
    """`test_train_gnn_follows_the_references_recorded_run` with graphed=True: the same fixture, yardsticks (|run32 - run64| per series)
    and bars (4x; an F1 series whose yardstick is 0 must be equal), the best epoch equal to the fp64 run's."""
    from bridged_gnn_amd import transfer
    g = golden(FIX)
    data = office_data(golden)
    hist = {}
    lb, each = transfer.train_gnn(types.SimpleNamespace(dataset_name="office_amazon2dslr"), transfer.pyg_dataset(data), data, save=False,
                                  repeat=1, num_epoch=20, step_size=100, gamma=0.1, gnn="KTGNN", seed=0, num_layer=2, hidden=64, lr=1e-3,
                                  wd=5e-3, use_shceduler=True, step=1, Lambda=1., metric="f1", f1_average="macro", dropout=0.0,
                                  verbose=False, history=hist, graphed=True)
    got = series(lb)
    r64, r32 = g["run64/loss"], g["run32/loss"]
    yard = np.abs(r32 - r64).max(0)
    dev = np.abs(got - r64).max(0)
    print("loss yardstick", yard, "measured", dev, "bar", 4 * yard)
    f_got = np.concatenate([np.array(hist["eval_res"]), np.array([each["source&target"], each["target"], each["target_hat"]]).T], axis=1)
    f64 = np.concatenate([g["run64/eval_res"], g["run64/eval_res_each"]], axis=1)
    f32 = np.concatenate([g["run32/eval_res"], g["run32/eval_res_each"]], axis=1)
    f_yard = np.abs(f32 - f64).max(0)
    f_dev = np.abs(f_got - f64).max(0)
    print("f1 yardstick", f_yard, "measured", f_dev, "bar", 4 * f_yard)
    print("best epoch", hist["best_epoch"], int(g["run64/best_epoch"]))
    assert (dev <= 4 * yard).all()
    assert (f_dev <= 4 * f_yard).all()
    assert hist["best_epoch"] == int(g["run64/best_epoch"])


def test_graphed_dropout_run_equals_the_eager_run(golden):
    data = office_data(golden)
    he, hg = {}, {}
    lb_e, each_e = run_dtc(data, False, he)
    lb_g, each_g = run_dtc(data, True, hg)
    e, g = series(lb_e), series(lb_g)
    print("KTGNN dropout run, max rel dev per series", (np.abs(g - e) / np.abs(e)).max(0))
    assert g.shape == (8, 4) and np.allclose(g, e, rtol=TRAJ_RTOL), (g, e)
    assert hg["eval_res"] == he["eval_res"] and each_g == each_e
    assert hg["best_epoch"] == he["best_epoch"] and hg["best_acc"] == pytest.approx(he["best_acc"], rel=TRAJ_RTOL)


def test_graphed_noDTC_dropout_run_equals_the_eager_run(golden):
    data = office_data(golden)
    he, hg = {}, {}
    assert run_plain(data, False, he) is None and run_plain(data, True, hg) is None
    e, g = np.array(he["loss_train"]), np.array(hg["loss_train"])
    print("GraphSAGE dropout run, max rel dev", (np.abs(g - e) / np.abs(e)).max())
    assert g.shape == (8,) and np.allclose(g, e, rtol=TRAJ_RTOL), (g, e)
    assert hg["eval_res"] == he["eval_res"] and hg["best_epoch"] == he["best_epoch"]


def test_replayed_dropout_masks_are_the_eager_masks(golden):
    """frozen weights (lr = 0, wd = 0): the training loss of epoch k depends on that epoch's dropout masks alone, so the two modes must
    give the same bits, epoch by epoch, for KTGNN and for GraphSAGE"""
    data = office_data(golden)
    lb_e, _ = run_dtc(data, False, {}, lr=0.0, wd=0.0)
    lb_g, _ = run_dtc(data, True, {}, lr=0.0, wd=0.0)
    assert lb_g == lb_e
    assert len(set(lb_e["source&target"])) == 8                         # (the masks differ from epoch to epoch: the comparison says something)
    he, hg = {}, {}
    run_plain(data, False, he, lr=0.0, wd=0.0)
    run_plain(data, True, hg, lr=0.0, wd=0.0)
    assert hg["loss_train"] == he["loss_train"] and len(set(he["loss_train"])) == 8
    assert hg["eval_res"] == he["eval_res"]


@pytest.mark.parametrize("dtc", [True, False])
def test_warm_up_and_capture_leave_no_trace(golden, monkeypatch, dtc):
    """0 epochs: the model's state_dict and both generators after graphed=True equal those of the eager twin"""
    data = office_data(golden)
    seen = grab_models(monkeypatch)
    run = (lambda gr: run_dtc(data, gr, {}, num_epoch=0)) if dtc else (lambda gr: run_plain(data, gr, {}, num_epoch=0))
    states = []
    for graphed in (False, True):
        run(graphed)
        states.append(({k: v.clone() for k, v in seen[-1].state_dict().items()}, torch.get_rng_state(), torch.cuda.get_rng_state(DEV)))
    (sd_e, rng_e, dev_e), (sd_g, rng_g, dev_g) = states
    assert len(seen) == 2 and sorted(sd_e) == sorted(sd_g)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert torch.equal(rng_e, rng_g) and torch.equal(dev_e, dev_g)
    # and the generator ends where the eager loop leaves it after real epochs too
    run_e = (lambda gr: run_dtc(data, gr, {}, num_epoch=3)) if dtc else (lambda gr: run_plain(data, gr, {}, num_epoch=3))
    ends = []
    for graphed in (False, True):
        run_e(graphed)
        ends.append(torch.get_rng_state())
    assert torch.equal(ends[0], ends[1])


def test_trained_weights_are_what_an_eager_eval_sees(golden, monkeypatch):
    from bridged_gnn_amd import transfer
    data = office_data(golden)
    seen = grab_models(monkeypatch)
    hist = {}
    _, each = run_dtc(data, True, hist, num_epoch=5)
    model = seen[-1]
    last_each = [each["source&target"][-1], each["target"][-1], each["target_hat"][-1]]
    # the trained model itself: its packed / folded weight copies were dropped after the last replay
    assert transfer.test(data, model, "office", gnn="KTGNN") == hist["eval_res"][-1]
    assert transfer.get_each_clf_res(data, model) == last_each
    assert all(p.grad is None for p in model.parameters())
    fresh = build_ktgnn(data, 31, 64, 0.5)
    fresh.load_state_dict(model.state_dict())
    assert transfer.test(data, fresh, "office", gnn="KTGNN") == hist["eval_res"][-1]
    assert transfer.get_each_clf_res(data, fresh) == last_each
    assert int(model.state_dict()["bns.0.num_batches_tracked"]) == 5
    # GraphSAGE
    hist = {}
    run_plain(data, True, hist, num_epoch=5)
    assert transfer.test_noDTC(data, seen[-1]) == hist["eval_res"][-1]


@pytest.mark.parametrize("dtc", [True, False])
def test_replayed_epochs_do_not_wait_for_the_device(golden, monkeypatch, dtc):
    from bridged_gnn_amd import transfer
    data = office_data(golden)
    calls = {"sync": 0, "epochs": 0}
    replay0, drain0 = transfer._GraphedEpoch.replay, transfer._History.drain
    names = ("item", "tolist", "cpu", "numpy", "__bool__", "__int__", "__float__", "nonzero")
    orig = {n: getattr(torch.Tensor, n) for n in names}

    def counted(n):
        def f(self, *a, **k):
            if calls["epochs"] and self.is_cuda:
                calls["sync"] += 1
            return orig[n](self, *a, **k)
        return f

    def replay(self):
        if calls["epochs"] == 0:
            torch.cuda.set_sync_debug_mode("error")     # from the first replay on a synchronising torch call raises
            for n in names:
                monkeypatch.setattr(torch.Tensor, n, counted(n))
            monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.__setitem__("sync", calls["sync"] + 1))
        calls["epochs"] += 1
        return replay0(self)

    def drain(self):
        torch.cuda.set_sync_debug_mode("default")       # the loop is over: the history is read once
        calls["replays"] = calls.get("replays", 0) + calls["epochs"]
        calls["epochs"] = 0
        return drain0(self)
    monkeypatch.setattr(transfer._GraphedEpoch, "replay", replay)
    monkeypatch.setattr(transfer._History, "drain", drain)
    try:
        hist = {}
        (run_dtc if dtc else run_plain)(data, True, hist, num_epoch=6, step_size=2)
        seen = calls["sync"]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert seen == 0 and calls["replays"] == 6 and len(hist["eval_res"]) == 6 and hist["best_epoch"] is not None


def test_save_writes_the_best_epochs_parameters(golden, tmp_path):
    from bridged_gnn_amd import transfer
    data = office_data(golden)
    hist = {}
    run_dtc(data, True, hist, num_epoch=4, save=True, ckpt_dir=str(tmp_path))
    path = os.path.join(str(tmp_path), "model_KTGNN_office_best.ckpt")
    fresh = build_ktgnn(data, 31, 64, 0.5)
    fresh.load_state_dict(torch.load(path))
    assert transfer.test(data, fresh, "office", gnn="KTGNN") == hist["eval_res"][hist["best_epoch"]]
    hist = {}
    run_plain(data, True, hist, num_epoch=4, save=True, ckpt_dir=str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "model_GraphSAGE_office_share_best.ckpt"))


def test_verbose_and_repeat(golden, capsys):
    data = office_data(golden)
    he, hg = {}, {}
    lb_e, _ = run_dtc(data, False, he, num_epoch=3, repeat=2, seed=None)
    lb_g, _ = run_dtc(data, True, hg, num_epoch=3, repeat=2, seed=None)             # one capture per repeat
    assert series(lb_g).shape == (6, 4) and np.allclose(series(lb_g), series(lb_e), rtol=TRAJ_RTOL)
    assert len(hg["final_acc"]["test"]) == 2 and hg["final_acc"] == pytest.approx(he["final_acc"])
    capsys.readouterr()
    lb_v, _ = run_dtc(data, True, {}, num_epoch=3, verbose=True)                      # every=1: each epoch is read as it is written
    out = capsys.readouterr().out
    assert out.count("Epoch: 00") == 3 and out.count("Loss_clf:") == 3
    assert np.allclose(series(lb_v), series(lb_e)[:3], rtol=TRAJ_RTOL)


def test_auc_metric_on_the_binary_fixture(golden):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.data import Data
    g = golden(FIX)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    data = Data(x=dev(g["bin/x"]), edge_index=dev(g["bin/edge_index"]), y=dev(g["bin/y"]),
                **{k: dev(g["bin/" + k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    res = {}
    for graphed in (False, True):
        hist = {}
        lb, _ = transfer.train_gnn(types.SimpleNamespace(dataset_name="bin"), transfer.pyg_dataset(data), data, repeat=1, num_epoch=6, step_size=3,
                                   gnn="KTGNN", seed=0, num_layer=2, hidden=32, dropout=0.0, metric="auc", verbose=False, history=hist,
                                   graphed=graphed)
        res[graphed] = (series(lb), np.array(hist["eval_res"]))
    print("auc eager", res[False][1][-1], "graphed", res[True][1][-1], "max dev", np.abs(res[True][1] - res[False][1]).max())
    assert res[True][1].shape == (6, 3) and ((res[True][1] >= 0) & (res[True][1] <= 1)).all()
    assert np.allclose(res[True][0], res[False][0], rtol=TRAJ_RTOL)
    with pytest.raises(ValueError, match="binary"):
        run_dtc(office_data(golden), True, {}, num_epoch=1, metric="auc")


@pytest.mark.parametrize("extra", [["--to_undirected"], ["--to_undirected", "--no_dtc"]])
def test_main_runs_graphed_from_a_saved_bridged_graph(golden, tmp_path, extra, capsys):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.data import Data, save_bridged_graph
    og = golden("office_a2d_graph.npz")
    d = Data(x=torch.from_numpy(og["x"]), edge_index=torch.from_numpy(og["edge_index"]).long(), y=torch.from_numpy(og["y"]).long(),
             **{k: torch.from_numpy(og[k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    path = str(tmp_path / "office_amazon2dslr_bridged_graph.dat")
    save_bridged_graph(d, path)
    words = ["--num_layer", "2", "--hidden_dim", "64", "--num_epoch", "3", "--dataset_name", "office_amazon2dslr", "--path_data", path] + extra
    res = transfer.main(words + ["--graphed"])
    out = capsys.readouterr().out
    assert out.count("Epoch: 00") == 3 and "[Best Score]" in out and "[Run-1 score]" in out
    if "--no_dtc" in extra:
        assert res is None
    else:
        lb, each = res
        assert len(lb["source&target"]) == 3 and all(np.isfinite(lb[k]).all() for k in lb) and len(each["target_hat"]) == 3
        lb_e, each_e = transfer.main(words, verbose=False)
        assert np.allclose(series(lb), series(lb_e), rtol=TRAJ_RTOL) and each == each_e
