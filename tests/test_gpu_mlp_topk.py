"""GPU: the mlp pair top-k (`bgnn_mlp_pair_topk_f32`, `ops.mlp_pair_topk`) against the declared rule -- canonical fp64 score
descending, ties to the lower candidate index -- as the C oracle (`oracle_c.mlp_topk`) states it, on the same fp32 arrays.
Indices must be BIT-EXACT; raw scores within (rtol 1e-6, atol 1e-7 max|ref|), probabilities within (1e-5, 1e-6), the bars of
the cosine tests.  Covers both shortlist geometries (k <= 24: 64-entry buffers, k > 24: 128-entry buffers, two entries per
lane), partial blocks and tiles, k == Nc, exact ties, dead hidden units, and inputs whose large terms cancel, where the fp32
pass's error follows S = |b2| + sum_h |w2_h t_h| and not |score| (the case the error bound of the proof has to cover)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_close, sub
from oracle import oracle_c as OC
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 128
E_SHAPE, E_WORKSPACE, E_RANGE = -2, -3, -5          # include/bgnn.h


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu(A, B, scale, shift, w2, b2, k, apply_sigmoid):
    from bridged_gnn_amd import ops
    idx, val, nfb = ops.mlp_pair_topk(_t(A), _t(B), _t(scale), _t(shift), _t(w2), float(b2), k, apply_sigmoid=apply_sigmoid)
    return idx.cpu().numpy(), val.cpu().numpy(), int(nfb[0].item())


def _check(case, args, k, ref, apply_sigmoid, values=True):
    """one GPU call against the oracle's (values, indices) of the same arrays -> n_fallback[0]"""
    rv, ri = ref
    idx, val, nfb = _gpu(*args, k, apply_sigmoid)
    wrong = int((idx != ri).any(axis=1).sum())
    assert np.array_equal(idx, ri), f"{case} k={k} n_fallback={nfb}: {wrong} of {ri.shape[0]} rows differ from the declared rule"
    if values:
        if apply_sigmoid:
            assert_close(val, O.sigmoid_f32(rv), rtol=1e-5, atol_scale=1e-6, what=f"probs {case}")
        else:
            assert_close(val, rv, rtol=1e-6, atol_scale=1e-7, what=f"scores {case}")
    return nfb


# ---- (a) shape sweep on O(1) terms ----------------------------------------------------------------
def _office_like(seed, nq, nc):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nc, H)).astype(np.float32)
    B = rng.standard_normal((nq, H)).astype(np.float32)
    scale = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    shift = (0.1 * rng.standard_normal(H)).astype(np.float32)
    w2 = (rng.standard_normal(H) / np.sqrt(H)).astype(np.float32)
    return A, B, scale, shift, w2, np.float32(0.1)


SHAPES = [(1, 1, 1),                                    # the smallest call
          (127, 33, 3), (128, 32, 8), (129, 31, 24),    # around the 128-query block and the 32-candidate tile; partial tile, k just under Nc
          (300, 5000, 24), (300, 5000, 25),             # both sides of the geometry switch
          (200, 3000, 40), (130, 1500, 56),             # the wide geometry up to the largest k
          (64, 56, 56)]                                 # k == Nc: every candidate is returned, only the order is tested
_shape_cache = {}


def _shape_case(nq, nc, k):
    if (nq, nc, k) not in _shape_cache:
        args = _office_like(1000 + nq + nc + k, nq, nc)
        _shape_cache[(nq, nc, k)] = (args, OC.mlp_topk(*args, k))
    return _shape_cache[(nq, nc, k)]


@pytest.mark.parametrize("apply_sigmoid", [False, True])
@pytest.mark.parametrize("nq,nc,k", SHAPES)
def test_mlp_topk_shapes_bit_exact(nq, nc, k, apply_sigmoid):
    args, ref = _shape_case(nq, nc, k)
    nfb = _check(f"seed={1000 + nq + nc + k} Nq={nq} Nc={nc}", args, k, ref, apply_sigmoid)
    if k < nc:              # continuous data, no ties: the proof must carry (almost) every row
        assert nfb <= max(2, nq // 100), nfb


# ---- (b) fuzz --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
def test_mlp_topk_fuzz_bit_exact(seed):
    """seeded random (Nq, Nc, k); clustered terms, exact and near duplicates among the candidates, w2 of mixed signs, negative
    scales and strongly negative shifts (whole hidden units dead for every pair: the ReLU clamp of the fp32 pass and of the
    canonical re-score)."""
    rng = np.random.default_rng(7000 + seed)
    k = int(rng.choice([1, 3, 8, 20, 24, 25, 30, 56]))
    nq, nc = int(rng.integers(1, 400)), int(rng.integers(max(k, 33), 6000))
    centers = rng.standard_normal((8, H))
    spread = rng.choice([0.05, 0.3, 1.0])
    A = (centers[rng.integers(0, 8, nc)] + rng.standard_normal((nc, H)) * spread).astype(np.float32)
    B = (centers[rng.integers(0, 8, nq)] + rng.standard_normal((nq, H)) * spread).astype(np.float32)
    A[rng.integers(0, nc, 5)] = A[rng.integers(0, nc, 5)]                  # exact duplicates
    A[rng.integers(0, nc, 5)] *= np.float32(1.0 + 1e-6)                    # near duplicates
    scale = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    shift = (0.1 * rng.standard_normal(H)).astype(np.float32)
    scale[rng.integers(0, H, 12)] *= np.float32(-1.0)                      # units that fire on the negative side
    shift[rng.integers(0, H, 12)] = np.float32(-40.0)                      # units dead for every pair (|scale (a + b)| < 40)
    w2 = rng.standard_normal(H).astype(np.float32)                         # mixed signs
    b2 = np.float32(rng.standard_normal())
    args = (A, B, scale, shift, w2, b2)
    _check(f"seed={seed} Nq={nq} Nc={nc}", args, k, OC.mlp_topk(*args, k), apply_sigmoid=bool(seed & 1))


# ---- (c) ties --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 30])
def test_mlp_topk_exact_ties_and_duplicates(k):
    """duplicated candidate rows give exactly equal scores: the lower index must win, everywhere."""
    nq = 200
    base, B, scale, shift, w2, b2 = _office_like(31 + k, nq, 700)
    A = np.concatenate([base, base[:300], base[100:200], base])         # up to 4 copies
    args = (A, B, scale, shift, w2, b2)
    _check(f"seed={31 + k} Nq={nq} Nc={A.shape[0]} copies", args, k, OC.mlp_topk(*args, k), apply_sigmoid=True)
    # all-identical candidates: every score ties -> indices 0..k-1; no margin proof can hold -> every row is re-done exhaustively
    A2 = np.repeat(base[:1], 500, axis=0)
    idx, _, nfb = _gpu(A2, B, scale, shift, w2, b2, k, True)
    assert np.array_equal(idx, np.tile(np.arange(k), (nq, 1))), f"seed={31 + k} Nq={nq} Nc=500 identical k={k} n_fallback={nfb}"
    assert nfb == nq, nfb


# ---- (d) cancellation ------------------------------------------------------------------------------
def _cancelling(seed, nq, nc, amp, pert=1e-6):
    """Every pair shares one large common level that b2 cancels: |score| << S = |b2| + sum_h |w2_h t_h|, and the candidates of a
    row differ by a few fp32 rounding errors of S only."""
    rng = np.random.default_rng(seed)
    base, bbase = rng.standard_normal(H), rng.standard_normal(H)
    A = ((base + pert * rng.standard_normal((nc, H))) * amp).astype(np.float32)
    B = ((bbase + pert * rng.standard_normal((nq, H))) * amp).astype(np.float32)
    scale = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    shift = (0.1 * rng.standard_normal(H)).astype(np.float32)
    w2 = rng.standard_normal(H).astype(np.float32)
    b2 = np.float32(-np.median(O.mlp_scores_canonical(A, B, scale, shift, w2, 0.0)))
    return A, B, scale, shift, w2, b2


def _term_magnitudes(A, B, scale, shift, w2, b2):
    """S = |b2| + sum_h |w2_h relu(scale_h (a_h + b_h) + shift_h)| in fp64, [Nq, Nc]"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    s = np.zeros((B.shape[0], A.shape[0]))
    for h in range(H):
        s += abs(float(w2[h])) * np.maximum(float(scale[h]) * (B64[:, h:h + 1] + A64[:, h][None, :]) + float(shift[h]), 0.0)
    return s + abs(float(b2))


@pytest.mark.parametrize("amp", [64.0, 256.0])
@pytest.mark.parametrize("seed,k,nq,nc", [(1, 8, 128, 4000), (4, 30, 128, 4000), (5, 56, 130, 1500)])
def test_mlp_topk_cancelling_terms_bit_exact(seed, k, nq, nc, amp):
    """The fp32 pass errs by a few 2^-24 S here, far above any bound tied to |score|, and the k-th / (k+1)-th canonical scores of
    almost every row lie closer than that: a proof whose bound is too small reports wrong indices as proven.
    With the bound this test was written against (1e-4 (1 + |score|), hard-coded) an MI355X returned wrong indices in
    (amp 64) 13 / 65 / 128 and (amp 256) 9 / 0 / 2 rows of Nq for (seed 1, k 8) / (seed 4, k 30) / (seed 5, k 56), with
    2 / 23 / 2 and 115 / 128 / 128 rows counted as re-done exhaustively (at amp 256 the shortlists overflow and most rows reach
    the exhaustive stage anyway).  With the bound per query every row of these cases goes to the exhaustive stage."""
    args = _cancelling(seed, nq, nc, amp)
    rv1, ri1 = OC.mlp_topk(*args, k + 1)
    # the case is not vacuous (host side, from the oracle's fp64 scores alone)
    s_min = float(_term_magnitudes(*args).min())
    gap = rv1[:, k - 1] - rv1[:, k]
    assert (gap > 0).all(), "exact tie at the k boundary"
    assert (gap < 8 * 2.0 ** -24 * s_min).mean() >= 0.9, (float(np.median(gap)), s_min)
    assert float(np.median(np.abs(O.mlp_scores_canonical(*args)))) < 1e-3 * s_min
    _check(f"seed={seed} Nq={nq} Nc={nc} amp={amp}", args, k, (rv1[:, :k], ri1[:, :k]), apply_sigmoid=False, values=False)


# ---- the shipped office checkpoints: the bound must not push rows to the exhaustive stage ------------
@pytest.mark.parametrize("tag,k", [("a2d", 20), ("a2w", 8)])
def test_mlp_topk_office_fallback_cap(golden, tag, k):
    f = golden(f"knn_office_{tag}.npz")
    args = O.mlp_pair_terms(f["z_src"], f["z_tar"], sub(f, "sim."))
    nq = args[1].shape[0]
    nfb = _check(f"office {tag} Nq={nq} Nc={args[0].shape[0]}", args, k, OC.mlp_topk(*args, k), apply_sigmoid=True)
    print(f"office {tag}: rows re-done exhaustively {nfb} of {nq}")
    assert nfb <= max(2, nq // 100), nfb


# ---- (e) refusals ----------------------------------------------------------------------------------
def test_mlp_topk_refusals():
    from bridged_gnn_amd import _lib as L
    lib = L.lib()
    nq, nc, k = 5, 40, 3
    A, B, scale, shift, w2, b2 = (_t(a) if isinstance(a, np.ndarray) and a.ndim else a for a in _office_like(3, nq, nc))
    idx = torch.full((nq, 56), -7, dtype=torch.int64, device=DEV)
    val = torch.full((nq, 56), -7.0, dtype=torch.float32, device=DEV)
    nfb = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    wsb = max(lib.bgnn_topk_workspace_bytes(nq, nc, kk) for kk in (3, 56))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)

    def call(Nq=nq, Nc=nc, Hh=H, kk=k, ws_bytes=wsb):
        rc = lib.bgnn_mlp_pair_topk_f32(L.ptr(A), L.ptr(B), L.ptr(scale), L.ptr(shift), L.ptr(w2), float(b2), Nq, Nc, Hh, kk, 1,
                                        L.ptr(idx), L.ptr(val), L.ptr(nfb), L.ptr(ws), ws_bytes, L.stream())
        torch.cuda.synchronize()
        return rc

    assert call(kk=0) == E_RANGE and call(kk=57) == E_RANGE and call(kk=nc + 1) == E_RANGE
    assert call(Hh=64) == E_SHAPE and call(Hh=129) == E_SHAPE and call(Nc=0) == E_SHAPE
    assert call(ws_bytes=lib.bgnn_topk_workspace_bytes(nq, nc, k) - 1) == E_WORKSPACE
    assert call(Nq=0) == 0
    # nothing above was allowed to write
    assert bool((idx == -7).all()) and bool((val == -7.0).all()) and bool((nfb == -7).all()) and bool((ws == 0).all())
    assert call(ws_bytes=lib.bgnn_topk_workspace_bytes(nq, nc, k)) == 0          # the exact size is enough
    rv, ri = OC.mlp_topk(A.cpu().numpy(), B.cpu().numpy(), scale.cpu().numpy(), shift.cpu().numpy(), w2.cpu().numpy(), b2, k)
    assert np.array_equal(idx.view(-1)[: nq * k].view(nq, k).cpu().numpy(), ri)
