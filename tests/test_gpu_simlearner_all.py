"""GPU: the Cartesian evaluation of the v2 similarity learner (eval_mode='all') -- the product count pass ops.pair_mlp_count
against an fp64 restatement over the enumerated product and against the list pass ops.pair_mlp_eval, a product of more than 2^31
pairs, the reference's own eval_adv_v2(eval_mode='all') on office A->D (tools/gen_golden_simlearner_all.py), main_adv_v2 end to
end, and eval_mode='sampling' unchanged.

Bound of every count comparison: an fp32 evaluation may put a pair on the other side of p > 0.5 only if its fp64 logit lies
inside the near band |logit| < 1e-4 (the cases are built so that fp32's logit error is far below that, see count_case), so each
of the four counts may differ from fp64 by at most the number of near-band pairs of the case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_simlearner_all_host import COUNT_CASES, FIX_ALL, NEAR, NEAR_CAP, count_case, restate_counts, restate_logits
from test_simlearner_host import FIX, office, seeded_model

pytestmark = pytest.mark.gpu

BIG_M = 46500                # 46500^2 = 2 162 250 000 pairs > 2^31
BIG_TIME_LIMIT = 240         # seconds for the child process of the big product (import, tables, one count call, 192 tiny ones)


def _dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _count(c):
    from bridged_gnn_amd import ops
    return ops.pair_mlp_count(c["A"], c["B"], c["rows1"], c["rows2"], c["lab1"], c["lab2"], c["scale2"], c["shift2"], c["w2"], c["b2"])


@pytest.mark.parametrize("case", COUNT_CASES, ids=lambda c: f"m{c[3]}x{c[4]}_{c[5]}")
def test_product_count_matches_fp64_restatement(case):
    c = count_case(*case, dev=_dev())
    m = case[3] * case[4]
    got = _count(c)
    again = _count(c)
    assert got.dtype == torch.int64 and got.shape == (4,)
    assert torch.equal(got, again), "two calls differ"
    got = got.cpu()
    assert int(got.sum()) == m, "TP + FP + FN + TN != m1 * m2"
    ref, near = restate_counts(c)
    print(f"m1 x m2 = {case[3]} x {case[4]}: got {got.tolist()} fp64 {ref.tolist()} near band {near}")
    assert near <= NEAR_CAP * m
    assert int((got - ref).abs().max()) <= near, f"counts {got.tolist()} vs fp64 {ref.tolist()} differ by more than the near band {near}"


@pytest.mark.parametrize("case", COUNT_CASES[:4] + COUNT_CASES[5:7], ids=lambda c: f"m{c[3]}x{c[4]}_{c[5]}")
def test_product_count_against_list_pass(case):
    """ops.pair_mlp_count against ops.pair_mlp_eval on the materialised list of the same product.  The product pass does NOT keep
    the list pass's arithmetic order (it folds BN2 into the staged tables and sums the 128 columns in ascending order, where the
    list pass forms fma(a + b, scale2, shift2) and adds 16 lane partials of 8 columns), so the counts are held to the same
    near-band bound as against fp64, not to equality.  Both use the predicate 1 / (1 + expf(-logit)) > 0.5f."""
    from bridged_gnn_amd import ops
    c = count_case(*case, dev=_dev())
    m1, m2 = case[3], case[4]
    got = _count(c).cpu()
    idx1 = c["rows1"].repeat_interleave(m2).contiguous()
    idx2 = c["rows2"].repeat(m1).contiguous()
    y = (c["lab1"][idx1] == c["lab2"][idx2]).to(torch.uint8)
    A, B = c["A"].contiguous(), c["B"].contiguous()
    _, cnt = ops.pair_mlp_eval(A, B, idx1, idx2, c["scale2"], c["shift2"], c["w2"], c["b2"], y)
    tp, fp, fn = (int(v) for v in cnt.tolist())
    lst = torch.tensor([tp, fp, fn, m1 * m2 - tp - fp - fn])
    near = int((restate_logits(c).abs() < NEAR).sum().item())
    print(f"m1 x m2 = {m1} x {m2}: product {got.tolist()} list {lst.tolist()} near band {near}")
    assert int((got - lst).abs().max()) <= near


def _big_child():
    """Child process of test_product_of_more_than_2_31_pairs: one JSON line with the big product's counts and the per-pair decisions
    of the 16 x 12 distinct (row1, row2) pairs, each from the same kernel on a 1 x 1 product."""
    from bridged_gnn_amd import ops
    dev = torch.device("cuda:0")
    c = count_case(77, 16, 12, BIG_M, BIG_M, rows="repeat", dev=dev)
    args = (c["lab1"], c["lab2"], c["scale2"], c["shift2"], c["w2"], c["b2"])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    big = ops.pair_mlp_count(c["A"], c["B"], c["rows1"], c["rows2"], *args)
    b.record()
    big2 = ops.pair_mlp_count(c["A"], c["B"], c["rows1"], c["rows2"], *args)
    torch.cuda.synchronize()
    singles = []
    for i in range(16):
        for j in range(12):
            singles.append(ops.pair_mlp_count(c["A"], c["B"], torch.tensor([i], device=dev), torch.tensor([j], device=dev), *args))
    singles = torch.stack(singles).cpu().reshape(16, 12, 4)
    c1 = torch.bincount(c["rows1"].cpu(), minlength=16)
    c2 = torch.bincount(c["rows2"].cpu(), minlength=12)
    want = (singles * (c1[:, None] * c2[None, :])[:, :, None]).sum((0, 1))
    print(json.dumps({"big": big.tolist(), "again": big2.tolist(), "want": want.tolist(), "ms": a.elapsed_time(b)}))


def test_product_of_more_than_2_31_pairs():
    """46500 x 46500 rows drawn from a 16-row and a 12-row table: the tile ids and the counts pass 2^31.  The kernel's decision on a
    pair depends on the two rows only (every pair sums its 128 columns in the same order wherever it sits in a tile), so the big
    counts must EQUAL the 16 x 12 single-pair decisions weighted by the rows' multiplicities.  Runs in a child process under its
    own time limit."""
    assert BIG_M * BIG_M > 2 ** 31
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--big-child"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=BIG_TIME_LIMIT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("big product:", out)
    assert sum(out["big"]) == BIG_M * BIG_M
    assert out["big"] == out["again"] == out["want"]
    assert min(out["big"]) > 0


def _fixture_model(f, ds, dt, dev):
    from bridged_gnn_amd import simlearner as SL
    model = SL.Adversarial_Learner_v2(ds, dt, dim_hidden=int(f["hidden"]), num_layer=2, use_norm=True, source_clf=True,
                                      norm_mode="None", norm_scale=1., sim_mode="mlp", backbone="mlp", dropout=False)
    assert list(model.state_dict().keys()) == list(f["keys"])
    model.load_state_dict({k: torch.from_numpy(f[f"state/{k}"]) for k in f["keys"]}, strict=True)
    return model.to(dev).eval()


def _f1_bound(counts, n):
    """|f1(counts') - f1(counts)| for |counts' - counts| <= n per entry: f = 2 TP / D, D = 2 TP + FP + FN, so
    |df| <= 2 n / D' + 2 TP * 4 n / (D D') <= 6 n / (D - 4 n)"""
    tp, fp, fn, _ = (float(v) for v in counts)
    d = 2 * tp + fp + fn
    return 0.0 if n == 0 else (1.0 if d <= 4 * n else 6 * n / (d - 4 * n))


def test_office_eval_all_matches_reference():
    """eval_adv_v2(eval_mode='all') on the fixture's model against the reference's own scores (fp64), val and test, f1 and acc;
    each product's counts against the reference's within the recorded near-band numbers.  Bars: pair scores move by at most what
    near-band pairs can move them (_f1_bound; accuracy: TP + TN moves by at most 2 n of m pairs) plus 1e-12 of rounding in the
    score itself.  Classifier scores: fp32 logits may turn the argmax of a row whose two best classes tie within rounding; one
    such row moves the accuracy by 1 / rows and a 31-class macro f1 by less than 1e-2 (the bar tests/test_gpu_simlearner.py
    derives for the same split), so those are the bars."""
    from bridged_gnn_amd import simlearner as SL
    dev = _dev()
    f = load_golden(FIX_ALL)
    ds, dt = office(dev)
    model = _fixture_model(f, ds, dt, dev)
    sim = model.source_learner.sim_net
    with torch.no_grad():
        z = {"src": SL._encode(model, ds, "source"), "tar": SL._encode(model, dt, "target")}
    y = {"src": ds.y, "tar": dt.y}
    for split in ("val", "test"):
        near, ref_counts = {}, {}
        for name, (d1, d2) in (("src", ("src", "src")), ("tar", ("tar", "tar")), ("cross1", ("src", "tar")), ("cross2", ("src", "tar"))):
            pre = f"prod/{split}/{name}/"
            r1, r2 = torch.from_numpy(f[pre + "rows1"]).to(dev), torch.from_numpy(f[pre + "rows2"]).to(dev)
            got = sim.pair_counts(z[d1], z[d2], r1, r2, y[d1], y[d2]).cpu().numpy()
            near[name], ref_counts[name] = int(f[pre + "near"]), f[pre + "counts"]
            print(f"{split} {name}: got {got.tolist()} reference {ref_counts[name].tolist()} near band {near[name]}")
            assert int(got.sum()) == r1.numel() * r2.numel()
            assert np.abs(got - ref_counts[name]).max() <= near[name], f"{split} {name}"
        near["cross"] = near["cross1"] + near["cross2"]
        ref_counts["cross"] = ref_counts["cross1"] + ref_counts["cross2"]
        n_rows = {"src": int(f[f"mask/src_{split}"].sum()), "tar": int(f[f"mask/tar_{split}"].sum())}
        for metric in ("f1", "acc"):
            got = np.array(SL.eval_adv_v2(ds, dt, model, split=split, metric=metric, enu_list=None, eval_mode="all"))
            ref = f[f"eval/{split}_{metric}"]
            print(f"{split} {metric}: got {got} reference {ref}")
            for pos, name in ((0, "src"), (2, "tar"), (4, "cross")):
                if metric == "f1":
                    bar = _f1_bound(ref_counts[name], near[name])
                else:
                    bar = 2.0 * near[name] / float(ref_counts[name].sum())
                assert abs(got[pos] - ref[pos]) <= bar + 1e-12, f"{split} {metric} pair {name}: {got[pos]} vs {ref[pos]} (bar {bar})"
            for pos, name in ((1, "src"), (3, "tar")):
                bar = 1e-2 if metric == "f1" else 1.0 / n_rows[name]
                assert abs(got[pos] - ref[pos]) <= bar + 1e-12, f"{split} {metric} clf {name}: {got[pos]} vs {ref[pos]}"
        # the three single evaluations agree with eval_adv_v2's shared encodings
        got = SL.eval_adv_v2(ds, dt, model, split=split, metric="f1", eval_mode="all")
        one = (SL.eval_within_domain_v2(ds, model, split=split, domain="source", eval_mode="all")
               + SL.eval_within_domain_v2(dt, model, split=split, domain="target", eval_mode="all")
               + (SL.eval_cross_domain_v2(ds, dt, model, split=split, eval_mode="all"),))
        assert tuple(got) == tuple(one)


def test_main_adv_v2_eval_all_end_to_end(tmp_path):
    import types
    from bridged_gnn_amd import simlearner as SL
    from bridged_gnn_amd.bridge import BridgeScorer
    dev = _dev()
    ds, dt = office(dev)
    args = types.SimpleNamespace(dataset_name="office_amazon2dslr")
    state, best = SL.main_adv_v2(args, ds, dt, save=True, repeat=1, num_epoch=3, seed=0, hidden=128, norm_mode="None",
                                 start_eval_epoch=1, max_class_num=10, sample_size=40000, device=dev, ckpt_dir=str(tmp_path),
                                 eval_mode="all", verbose=False)
    assert state is not None and 1 <= best["epoch"] <= 3 and np.isfinite(best["loss"])
    assert all(0.0 <= v <= 1.0 for k in ("val", "test") for v in best[k])
    ck = torch.load(tmp_path / "model_AdvLearner_office_amazon2dslr_best.ckpt", map_location="cpu")
    assert list(ck.keys()) == list(load_golden(FIX)["keys"]) == list(state.keys())
    assert all(torch.isfinite(v.float()).all() for v in ck.values())
    assert os.path.exists(tmp_path / "model_AdvLearner_office_amazon2dslr_final.ckpt")
    scorer = BridgeScorer(ck, dev)
    assert scorer.version == "v2" and scorer.sim_mode == "mlp"


def test_eval_sampling_unchanged_against_fixture():
    """eval_mode='sampling' through the refactored pair_scores: three training steps as the reference's fixture ran them, then the
    recorded s3/eval within the bar tests/test_gpu_simlearner.py holds the same numbers to (1e-2, derived there).  metric='acc'
    on the same lists (TN = P - TP - FP - FN) is checked for its range and the classifier accuracy for being a multiple of
    1 / rows."""
    from bridged_gnn_amd import simlearner as SL
    f = load_golden(FIX)
    dev = _dev()
    ds, dt = office(dev)
    model = seeded_model(ds, dt, dropout=False).to(dev)
    opt, opt_d = SL.make_optimizers(model)
    enu = (SL.Pair_Enumerator(ds, "train"), SL.Pair_Enumerator(dt, "train"), SL.Pair_Enumerator_cross(ds, dt, "train"))
    np.random.seed(0)
    for step in range(1, 4):
        SL.train_adv_few_shot(step, ds, dt, model, opt, opt_d, pair_enumerator_src_train=enu[0], pair_enumerator_tar_train=enu[1],
                              pair_enumerator_cross_train=enu[2], max_class_num=10, sample_size=40000, use_clf=True)
    enu_val = (SL.Pair_Enumerator(ds, "val"), SL.Pair_Enumerator(dt, "val"), SL.Pair_Enumerator_cross(ds, dt, "val"))
    enu_test = (SL.Pair_Enumerator(ds, "test"), SL.Pair_Enumerator(dt, "test"), SL.Pair_Enumerator_cross(ds, dt, "test"))
    ev = SL.eval_adv_v2(ds, dt, model, split="val", enu_list=enu_val) + SL.eval_adv_v2(ds, dt, model, split="test", enu_list=enu_test)
    print("eval after step 3:", np.array(ev), "reference:", f["s3/eval"])
    assert np.abs(np.array(ev) - f["s3/eval"]).max() <= 1e-2
    acc = SL.eval_adv_v2(ds, dt, model, split="test", metric="acc", enu_list=enu_test)
    assert all(0.0 <= v <= 1.0 for v in acc)
    n_test = int(dt.test_mask.sum())
    assert abs(acc[3] * n_test - round(acc[3] * n_test)) < 1e-6


if __name__ == "__main__" and "--big-child" in sys.argv:
    _big_child()
