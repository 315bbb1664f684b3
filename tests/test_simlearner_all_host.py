"""CPU: the Cartesian evaluation (eval_mode='all') of bridged_gnn_amd.simlearner where no GPU is needed -- the row sets of its
products against the ones the reference enumerated (tools/gen_golden_simlearner_all.py), the refusals that stay, and the shared
helpers of tests/test_gpu_simlearner_all.py (seeded random cases of the product count and their fp64 restatement)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_simlearner_host import office

FIX_ALL = "simlearner_all_office_a2d.npz"
NEAR = 1e-4          # |fp64 logit| below which an fp32 evaluation may count a pair on the other side (the fixture's band)
NEAR_CAP = 1e-3      # every case keeps its band within 0.1 % of the product
W = 128


def count_case(seed, nA, nB, m1, m2, rows="subset", ld=W, dev="cpu"):
    """A seeded case of ops.pair_mlp_count: tables [nA, 128] / [nB, 128] (row stride ld), row lists of m1 / m2 ids ('subset':
    distinct ids in random order, 'repeat': drawn with replacement), 5 label values, BN2 affine with every 7th scale 0 and w2 of
    both signs.  Magnitudes are chosen so that the fp32 error of a logit stays far below NEAR: sum_c |w2 h| is about 5, so even
    the worst-case bound (128 + a few) * 2^-24 * 5 ~ 4e-5 is under 1e-4, while the logits spread over ~0.7 -- a band of 2e-4 then
    holds ~1e-4 of the pairs, a tenth of NEAR_CAP (checked on every case)."""
    g = torch.Generator().manual_seed(seed)
    A = (0.5 * torch.randn(nA, ld, generator=g))[:, :W]
    B = (0.5 * torch.randn(nB, ld, generator=g))[:, :W]
    scale2 = 0.5 + torch.rand(W, generator=g)
    scale2[::7] = 0.0
    shift2 = 0.3 * torch.randn(W, generator=g)
    w2 = torch.randn(W, generator=g) / 8
    b2 = 0.1 * torch.randn(1, generator=g)
    lab1 = torch.randint(0, 5, (nA,), generator=g)
    lab2 = torch.randint(0, 5, (nB,), generator=g)
    if rows == "subset":
        rows1, rows2 = torch.randperm(nA, generator=g)[:m1], torch.randperm(nB, generator=g)[:m2]
    else:
        rows1, rows2 = torch.randint(0, nA, (m1,), generator=g), torch.randint(0, nB, (m2,), generator=g)
    assert rows1.shape[0] == m1 and rows2.shape[0] == m2
    to = lambda t: t.to(dev)                                                              # noqa: E731
    return dict(A=to(A), B=to(B), rows1=to(rows1), rows2=to(rows2), lab1=to(lab1), lab2=to(lab2), scale2=to(scale2), shift2=to(shift2),
                w2=to(w2), b2=to(b2))


def restate_logits(c, chunk=64):
    """fp64 logits [m1, m2] of the enumerated product, the scorer as the reference states it (BN2 affine, ReLU, w2 dot, b2)"""
    Ad, Bd = c["A"].double()[c["rows1"]], c["B"].double()[c["rows2"]]
    s, t, w, b = c["scale2"].double(), c["shift2"].double(), c["w2"].double(), c["b2"].double()
    out = torch.empty(Ad.shape[0], Bd.shape[0], dtype=torch.float64, device=Ad.device)
    for i0 in range(0, Ad.shape[0], chunk):
        u = Ad[i0:i0 + chunk, None, :] + Bd[None, :, :]
        out[i0:i0 + chunk] = torch.relu(u * s + t) @ w + b
    return out


def restate_counts(c):
    """-> (int64 [TP, FP, FN, TN] at sigmoid(logit) > 0.5 in fp64, number of pairs inside the near band)"""
    logit = restate_logits(c)
    pos = torch.sigmoid(logit) > 0.5
    same = c["lab1"][c["rows1"]][:, None] == c["lab2"][c["rows2"]][None, :]
    counts = torch.stack(((pos & same).sum(), (pos & ~same).sum(), (~pos & same).sum(), (~pos & ~same).sum())).cpu().long()
    return counts, int((logit.abs() < NEAR).sum().item())


#            seed  nA    nB    m1   m2   rows      ld
COUNT_CASES = [(1, 300, 200, 300, 200, "subset", W),        # whole tables, neither side a multiple of the 128-row tile
               (2, 1000, 700, 129, 257, "subset", W),       # row subsets of larger tables, one row past a tile on each side
               (3, 97, 61, 333, 150, "repeat", W),          # repeated rows
               (4, 256, 128, 256, 128, "subset", W),        # exact tiles
               (5, 400, 300, 1, 1, "subset", W),            # m = 1
               (6, 400, 300, 1, 130, "subset", W),
               (7, 400, 300, 131, 1, "repeat", 136),        # padded rows (ld > 128)
               (8, 50, 40, 0, 40, "subset", W),             # m = 0
               (9, 50, 40, 50, 0, "subset", W),
               (10, 50, 40, 0, 0, "subset", W)]


@pytest.mark.parametrize("case", COUNT_CASES, ids=lambda c: f"m{c[3]}x{c[4]}_{c[5]}")
def test_random_cases_keep_their_near_band_within_the_cap(case):
    c = count_case(*case)
    counts, near = restate_counts(c)
    m = case[3] * case[4]
    assert int(counts.sum()) == m
    assert near <= NEAR_CAP * m, f"near band {near} of {m} pairs"
    if m >= 10000:
        assert min(counts.tolist()) > 0, "a case should exercise all four counts"


def _ids(mask):
    return torch.nonzero(mask).reshape(-1).numpy()


@pytest.mark.parametrize("split", ["val", "test"])
def test_all_row_sets_match_reference(split):
    from bridged_gnn_amd import simlearner as SL
    f = load_golden(FIX_ALL)
    ds, dt = office()
    for dn, d in (("src", ds), ("tar", dt)):
        for m in ("train", "val", "test"):
            assert np.array_equal(getattr(d, m + "_mask").numpy(), f[f"mask/{dn}_{m}"])
        m1, m2 = SL._all_masks_within(d, split)
        assert np.array_equal(_ids(m1), f[f"prod/{split}/{dn}/rows1"]), dn
        assert np.array_equal(_ids(m2), f[f"prod/{split}/{dn}/rows2"]), dn
    for name, (ms, mt) in zip(("cross1", "cross2"), SL._all_masks_cross(ds, dt, split)):
        assert np.array_equal(_ids(ms), f[f"prod/{split}/{name}/rows1"]), name
        assert np.array_equal(_ids(mt), f[f"prod/{split}/{name}/rows2"]), name


def test_fixture_near_band_within_cap():
    f = load_golden(FIX_ALL)
    for split in ("val", "test"):
        for name in ("src", "tar", "cross1", "cross2"):
            pre = f"prod/{split}/{name}/"
            m = f[pre + "rows1"].size * f[pre + "rows2"].size
            assert int(f[pre + "counts"].sum()) == m
            assert int(f[pre + "near"]) <= NEAR_CAP * m, pre


def test_unknown_eval_mode_and_auc_raise():
    from bridged_gnn_amd import simlearner as SL
    ds, dt = office()
    with pytest.raises(NotImplementedError, match="Not Implemented Eval Mode:everything"):
        SL.eval_within_domain_v2(ds, None, eval_mode="everything")
    with pytest.raises(NotImplementedError, match="Not Implemented Eval Mode:everything"):
        SL.eval_cross_domain_v2(ds, dt, None, eval_mode="everything")
    with pytest.raises(NotImplementedError, match="Not Implemented Eval Mode:everything"):
        SL.eval_adv_v2(ds, dt, None, enu_list=(None, None, None), eval_mode="everything")
    for mode in ("sampling", "all"):
        with pytest.raises(NotImplementedError):
            SL.eval_within_domain_v2(ds, None, metric="auc", eval_mode=mode)
        with pytest.raises(NotImplementedError):
            SL.eval_cross_domain_v2(ds, dt, None, metric="auc", eval_mode=mode)
        with pytest.raises(NotImplementedError):
            SL.eval_adv_v2(ds, dt, None, metric="auc", enu_list=(None, None, None), eval_mode=mode)
        with pytest.raises(NotImplementedError):
            SL.eval_within_domain_v2(ds, None, conf_lower_bound=0.9, eval_mode=mode)
    with pytest.raises(NotImplementedError):
        SL.train_adv_few_shot(1, ds, dt, None, None, None, metric="acc")


def test_pair_score_from_counts():
    from bridged_gnn_amd import simlearner as SL
    assert SL._pair_score(3, 1, 2, 4, "f1") == SL.f1_from_counts(3, 1, 2) == 6 / 9
    assert SL._pair_score(3, 1, 2, 4, "acc") == 0.7
    assert SL._list_score(torch.tensor([3., 1., 2.], dtype=torch.float64), 10, "acc") == 0.7
    assert SL._list_score(torch.tensor([3., 1., 2.], dtype=torch.float64), 10, "f1") == 6 / 9
