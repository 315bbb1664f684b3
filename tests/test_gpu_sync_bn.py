"""GPU: the split-phase BatchNorm1d -> ReLU -> dropout entries (bgnn_bn_colstats_f32 and the three *_rows entries; KTGNN.py:420-430
on a node partition) against the fused single-GPU pair on the whole activation and against fp64 torch.

x has 777 rows, dealt to three parts by `r % 3` (so `row_ids` is not contiguous) plus a fourth part without rows.  Each part
reduces its rows, the parts' sums are added (the all-reduce), each part applies with its global row numbers; the reassembled
result must be the whole-graph call's: same dropout pattern, same values.

Bars.  Split and whole differ only in the order of the fp64 column sums, so an element can move by an ulp of the fp32 mean or
1/std at the most: |split - whole| <= 1e-6 * (|whole| + 1) per element -- 1e-6 relative, with the floor of a unit-variance
normalised activation for the elements next to zero.  Running buffers: 1e-6 absolute.  Against fp64 torch: the project's activation
bar (1e-5 of the tensor's max) forward and its gradient bar (2e-5 of each tensor's max) backward."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, P, SEED, EPS, MOM = 777, 0.5, 0x1234_5678_9ABC, 1e-5, 0.1
DS = [4, 12, 64, 128, 1024]
COMBOS = [(True, True), (False, True), (True, False), (False, False)]          # (relu, gamma / beta present)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(D):
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((N, D)) * rng.uniform(0.5, 3.0, D) + rng.uniform(-2, 2, D)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, D).astype(np.float32)
    beta = (10 + rng.random(D)).astype(np.float32)                               # every output positive: a zero means "dropped"
    gy = rng.standard_normal((N, D)).astype(np.float32)
    return _t(x), _t(gamma), _t(beta), _t(gy)


def _parts():
    r = torch.arange(N, device=DEV)
    return [r[r % 3 == k].contiguous() for k in range(3)] + [r[:0].contiguous()]


@functools.lru_cache(maxsize=None)
def _whole(D, relu, affine, p=P, seed=SEED):
    """the fused single-GPU pair on the whole x, computed once per case -> (y, stats, running_mean, running_var, gx, gsum)"""
    from bridged_gnn_amd import ops
    x, gamma, beta, gy = _inputs(D)
    g, b = (gamma, beta) if affine else (None, None)
    rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
    y, stats = ops.bn_relu_dropout(x, g, b, EPS, relu, p, seed, MOM, rm, rv)
    gx, gsum = ops.bn_relu_dropout_bwd(x, gy, stats, g, b, EPS, relu, p, seed)
    return y, stats, rm, rv, gx, gsum


def _close(a, b):
    """|a - b| <= 1e-6 * (|b| + 1) everywhere -> (ok, worst ratio)"""
    r = ((a - b).abs() / (1e-6 * (b.abs() + 1))).max() if a.numel() else torch.zeros(())
    return bool(r <= 1), float(r)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def _split_forward(D, relu, affine, p=P, seed=SEED, seed_dev=None, contiguous=False):
    from bridged_gnn_amd import ops
    x, gamma, beta, _ = _inputs(D)
    g, b = (gamma, beta) if affine else (None, None)
    if contiguous:                                                               # row_base + local row, a part without rows in the middle
        spans = [(0, 300), (300, 300), (300, N)]
        rows = [torch.arange(lo, hi, device=DEV) for lo, hi in spans]
        kws = [dict(row_base=lo) for lo, _ in spans]
    else:
        rows = _parts()
        kws = [dict(row_ids=ids) for ids in rows]
    xs = [x[ids].contiguous() for ids in rows]
    shares = [ops.bn_colstats(xk) for xk in xs]
    for xk, s in zip(xs, shares):
        if xk.shape[0] == 0:
            assert s.shape == (2 * D,) and not bool(s.any()), "a part without rows contributes zero sums"
    totals = torch.stack(shares).sum(0)                                          # stands in for the all-reduce
    y = torch.full((N, D), float("nan"), device=DEV)
    bufs = []
    for ids, xk, kw in zip(rows, xs, kws):
        rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
        yk = ops.bn_apply_rows(xk, totals, N, g, b, EPS, relu, p, seed, momentum=MOM, running_mean=rm, running_var=rv, seed_dev=seed_dev, **kw)
        assert yk.shape == xk.shape
        y[ids] = yk
        bufs.append((rm, rv))
    return y, totals, bufs, (rows, xs, kws)


@pytest.mark.parametrize("D", DS)
def test_split_forward_is_the_whole_graph_forward(D):
    """colstats per part -> summed -> apply per part with `row_ids`, for ReLU on / off and gamma / beta present / absent: the dropout
    pattern, the values and EVERY part's running buffers (the empty part's too) are those of `ops.bn_relu_dropout` on the whole x;
    the values also follow the fp64 formula with the kept pattern of the whole-graph call."""
    x, gamma, beta, _ = _inputs(D)
    for relu, affine in COMBOS:
        y_ref, stats, rm_ref, rv_ref = _whole(D, relu, affine)[:4]
        y, totals, bufs, _ = _split_forward(D, relu, affine)
        assert not bool(torch.isnan(y).any())
        if affine:
            assert torch.equal(y == 0, y_ref == 0), (D, relu, "dropout pattern")
            frac = float((y == 0).float().mean())
            assert abs(frac - P) < 0.5 / np.sqrt(N * D) * 6 + 1e-3, frac           # six sigma of a Bernoulli(0.5) mean
        ok, worst = _close(y, y_ref)
        print(f"D={D} relu={relu} affine={affine}: forward worst / bar {worst:.3f}")
        assert ok, (D, relu, affine, worst)
        assert _rel(totals, stats.view(-1, 2 * D).sum(0)) < 1e-12
        for rm, rv in bufs:
            assert float((rm - rm_ref).abs().max()) <= 1e-6 and float((rv - rv_ref).abs().max()) <= 1e-6
        # fp64 restatement with the whole-graph call's kept pattern
        xd = x.double()
        z = (xd - xd.mean(0)) / torch.sqrt(xd.var(0, unbiased=False) + EPS)
        z = z * gamma.double() + beta.double() if affine else z
        z = torch.relu(z) if relu else z
        keep = (y_ref != 0) | (z.abs() <= 1e-6)
        z = torch.where(keep, z * 2.0, torch.zeros_like(z))                      # thr = 32768: keep scale exactly 2
        assert _rel(y, z) < 1e-5, (D, relu, affine, _rel(y, z))
        assert _rel(rm_ref, MOM * xd.mean(0)) < 1e-6 and _rel(rv_ref, 1 - MOM + MOM * xd.var(0, unbiased=True)) < 1e-6


@pytest.mark.parametrize("D", [12, 128])
def test_row_base_and_device_seed_word(D):
    """`row_base` on a contiguous split equals `row_ids`; `seed = a, seed_dev = b` draws the mask of `seed = a + b`; p = 0 keeps
    everything"""
    y_ref = _whole(D, True, True)[0]
    y, _, _, _ = _split_forward(D, True, True, contiguous=True)
    assert torch.equal(y == 0, y_ref == 0) and _close(y, y_ref)[0]
    a, b = 0x0123_4567, SEED - 0x0123_4567
    word = torch.tensor([b], dtype=torch.int64, device=DEV)
    y, _, _, _ = _split_forward(D, True, True, seed=a, seed_dev=word)
    assert torch.equal(y == 0, y_ref == 0) and _close(y, y_ref)[0]
    y_other, _, _, _ = _split_forward(D, True, True, seed=a)
    assert not torch.equal(y_other == 0, y_ref == 0), "another seed, another mask"
    y0, _, _, _ = _split_forward(D, True, True, p=0.0)
    y0_ref = _whole(D, True, True, p=0.0)[0]
    assert not bool((y0 == 0).any()) and _close(y0, y0_ref)[0]


@pytest.mark.parametrize("D", DS)
def test_split_backward_is_the_whole_graph_backward(D):
    """reduce per part -> summed -> apply per part: grad_x, sum g' and sum g'.xhat against `ops.bn_relu_dropout_bwd` on the whole x and
    against fp64 autograd with the GPU's keep / ReLU pattern, at 2e-5 of each tensor's max; a part without rows contributes zeros."""
    from bridged_gnn_amd import ops
    x, gamma, beta, gy = _inputs(D)
    for relu, affine in COMBOS:
        g, b = (gamma, beta) if affine else (None, None)
        y_ref, _, _, _, gx_ref, gsum_ref = _whole(D, relu, affine)
        _, totals, _, (rows, xs, kws) = _split_forward(D, relu, affine)
        gys = [gy[ids].contiguous() for ids in rows]
        shares = [ops.bn_bwd_reduce_rows(xk, gk, totals, N, g, b, EPS, relu, P, SEED, **kw) for xk, gk, kw in zip(xs, gys, kws)]
        assert shares[3].shape == (2 * D,) and not bool(shares[3].any())
        gtot = torch.stack(shares).sum(0)
        gx = torch.full((N, D), float("nan"), device=DEV)
        for ids, xk, gk, kw in zip(rows, xs, gys, kws):
            out = ops.bn_bwd_apply_rows(xk, gk, totals, gtot, N, g, b, EPS, relu, P, SEED, **kw)
            assert out.shape == xk.shape
            gx[ids] = out
        assert not bool(torch.isnan(gx).any())
        # fp64 autograd with the kernel's pattern
        xo = x.double().clone().requires_grad_(True)
        go = (gamma.double() if affine else torch.ones(D, dtype=torch.float64, device=DEV)).clone().requires_grad_(True)
        bo = (beta.double() if affine else torch.zeros(D, dtype=torch.float64, device=DEV)).clone().requires_grad_(True)
        z = (xo - xo.mean(0)) / torch.sqrt(xo.var(0, unbiased=False) + EPS) * go + bo
        z = torch.relu(z) if relu else z
        keep = (y_ref != 0) | (z.detach().abs() <= 1e-6)
        (torch.where(keep, z * 2.0, torch.zeros_like(z)) * gy.double()).sum().backward()
        errs = {"gx|whole": _rel(gx, gx_ref), "gsum|whole": _rel(gtot, gsum_ref), "gx|fp64": _rel(gx, xo.grad),
                "sum g'|fp64": _rel(gtot[:D], bo.grad), "sum g'.xhat|fp64": _rel(gtot[D:], go.grad)}
        print(f"D={D} relu={relu} affine={affine}: {errs}")
        assert all(v < 2e-5 for v in errs.values()), (D, relu, affine, errs)


def test_bad_calls_return_the_documented_codes():
    from bridged_gnn_amd import ops
    x = torch.randn(8, 6, device=DEV)                                            # D % 4 != 0
    with pytest.raises(RuntimeError, match="BGNN_E_SHAPE|shape"):
        ops.bn_colstats(x)
    x = torch.randn(8, 8, device=DEV)
    tot = ops.bn_colstats(x)
    with pytest.raises(RuntimeError, match="BGNN_E_SHAPE|shape"):                # n_total below the rank's own rows
        ops.bn_apply_rows(x, tot, 4, None, None, EPS, True, 0.0, 0)
