"""GPU: the split-phase BatchNorm1d -> ReLU -> dropout entries (bgnn_bn_colstats_f32 and the three *_rows entries; KTGNN.py:420-430
on a node partition) against the fused single-GPU pair on the whole activation and against fp64 torch.

x has 777 rows, dealt to three parts by `r % 3` (so `row_ids` is not contiguous) plus a fourth part without rows.  Each part
reduces its rows, the parts' sums are added (the all-reduce), each part applies with its global row numbers; the reassembled
result must be the whole-graph call's: same dropout pattern, same values.

Bars.  Split and whole differ only in the order of the fp64 column sums, so an element can move by an ulp of the fp32 mean or
1/std at the most: |split - whole| <= 1e-6 * (|whole| + 1) per element -- 1e-6 relative, with the floor of a unit-variance
normalised activation for the elements next to zero.  Running buffers: 1e-6 absolute.  Against fp64 torch: the project's activation
bar (1e-5 of the tensor's max) forward and its gradient bar (2e-5 of each tensor's max) backward.

Past the grid cap: the fused pair and the split phase at (D, rows) = (1024, 4101), (128, 32771), (12, 348167),
more rows than 2048 blocks hold, under the same bars; the split phase dealt in thirds and as one part with every row.
Row stride: `[:, :D]` views of [777, D + 4] buffers with NaN pad columns, bit for bit the contiguous call.
Numeric edges (4101 rows, 8 columns): columns of mean / std = 1e3 and 2e3 and two constant columns, forward under a derived
per-element bound, backward at the gradient bar."""
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
def _inputs(D, n=N):
    rng = np.random.default_rng(D if n == N else [D, n])
    x = (rng.standard_normal((n, D)) * rng.uniform(0.5, 3.0, D) + rng.uniform(-2, 2, D)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, D).astype(np.float32)
    beta = (10 + rng.random(D)).astype(np.float32)                               # every output positive: a zero means "dropped"
    gy = rng.standard_normal((n, D)).astype(np.float32)
    return _t(x), _t(gamma), _t(beta), _t(gy)


def _parts(n=N, layout="thirds"):
    """the rows of each part: dealt by `r % 3` plus a part without rows, or ("all") one part with every row plus one without"""
    r = torch.arange(n, device=DEV)
    if layout == "all":
        return [r, r[:0].contiguous()]
    return [r[r % 3 == k].contiguous() for k in range(3)] + [r[:0].contiguous()]


@functools.lru_cache(maxsize=None)
def _whole(D, relu, affine, p=P, seed=SEED, n=N):
    """the fused single-GPU pair on the whole x, computed once per case -> (y, stats, running_mean, running_var, gx, gsum)"""
    from bridged_gnn_amd import ops
    x, gamma, beta, gy = _inputs(D, n)
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


def _split_forward(D, relu, affine, p=P, seed=SEED, seed_dev=None, contiguous=False, n=N, layout="thirds"):
    from bridged_gnn_amd import ops
    x, gamma, beta, _ = _inputs(D, n)
    g, b = (gamma, beta) if affine else (None, None)
    if contiguous:                                                               # row_base + local row, a part without rows in the middle
        spans = [(0, 300), (300, 300), (300, n)]
        rows = [torch.arange(lo, hi, device=DEV) for lo, hi in spans]
        kws = [dict(row_base=lo) for lo, _ in spans]
    else:
        rows = _parts(n, layout)
        kws = [dict(row_ids=ids) for ids in rows]
    xs = [x[ids].contiguous() for ids in rows]
    shares = [ops.bn_colstats(xk) for xk in xs]
    for xk, s in zip(xs, shares):
        if xk.shape[0] == 0:
            assert s.shape == (2 * D,) and not bool(s.any()), "a part without rows contributes zero sums"
    totals = torch.stack(shares).sum(0)                                          # stands in for the all-reduce
    y = torch.full((n, D), float("nan"), device=DEV)
    bufs = []
    for ids, xk, kw in zip(rows, xs, kws):
        rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
        yk = ops.bn_apply_rows(xk, totals, n, g, b, EPS, relu, p, seed, momentum=MOM, running_mean=rm, running_var=rv, seed_dev=seed_dev, **kw)
        assert yk.shape == xk.shape
        y[ids] = yk
        bufs.append((rm, rv))
    return y, totals, bufs, (rows, xs, kws)


def _split_backward(D, relu, affine, totals, parts, n=N):
    """reduce per part -> summed -> apply per part over the parts `_split_forward` returned -> (grad_x [n, D], the summed pair [2 * D]);
    a part without rows contributes zeros"""
    from bridged_gnn_amd import ops
    _, gamma, beta, gy = _inputs(D, n)
    g, b = (gamma, beta) if affine else (None, None)
    rows, xs, kws = parts
    gys = [gy[ids].contiguous() for ids in rows]
    shares = [ops.bn_bwd_reduce_rows(xk, gk, totals, n, g, b, EPS, relu, P, SEED, **kw) for xk, gk, kw in zip(xs, gys, kws)]
    for xk, s in zip(xs, shares):
        if xk.shape[0] == 0:
            assert s.shape == (2 * D,) and not bool(s.any())
    gtot = torch.stack(shares).sum(0)
    gx = torch.full((n, D), float("nan"), device=DEV)
    for ids, xk, gk, kw in zip(rows, xs, gys, kws):
        out = ops.bn_bwd_apply_rows(xk, gk, totals, gtot, n, g, b, EPS, relu, P, SEED, **kw)
        assert out.shape == xk.shape
        gx[ids] = out
    assert not bool(torch.isnan(gx).any())
    return gx, gtot


def _fp64_pair(x, gy, gamma, beta, relu, y_kernel):
    """BatchNorm1d(train) -> ReLU -> dropout(0.5) and its gradients in fp64 torch on the kernel's own kept pattern (an output of 0 is
    a dropped element: the callers' beta >= 10 keeps every activation away from 0) -> (y, mean, biased var, grad_x, dbeta, dgamma)"""
    D = x.shape[1]
    xo = x.double().clone().requires_grad_(True)
    go = (gamma.double() if gamma is not None else torch.ones(D, dtype=torch.float64, device=DEV)).clone().requires_grad_(True)
    bo = (beta.double() if beta is not None else torch.zeros(D, dtype=torch.float64, device=DEV)).clone().requires_grad_(True)
    mean, var = xo.mean(0), xo.var(0, unbiased=False)
    z = (xo - mean) / torch.sqrt(var + EPS) * go + bo
    z = torch.relu(z) if relu else z
    keep = (y_kernel != 0) | (z.detach().abs() <= 1e-6)
    y = torch.where(keep, z * 2.0, torch.zeros_like(z))                          # thr = 32768: keep scale exactly 2
    (y * gy.double()).sum().backward()
    return y.detach(), mean.detach(), var.detach(), xo.grad, bo.grad, go.grad


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
    x, gamma, beta, gy = _inputs(D)
    for relu, affine in COMBOS:
        y_ref, _, _, _, gx_ref, gsum_ref = _whole(D, relu, affine)
        _, totals, _, parts = _split_forward(D, relu, affine)
        assert parts[1][3].shape[0] == 0                                         # the fourth part has no rows
        gx, gtot = _split_backward(D, relu, affine, totals, parts)
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


# ---- past the grid cap: every block takes a second trip of its grid-stride loop ----------------------------------------------------
GRID_CAP = 2048                                                                  # bgnn_norm.hip grid_for: `if (g > 2048) g = 2048`
BIG = [(1024, 4101), (128, 32771), (12, 348167)]                                 # (D, rows): 1 / 8 / 85 rows per block pass (D = 12: thread 255 idles)


def _blocks(n, D):
    return -(-n // (256 // (D // 4)))                                            # bgnn_norm.hip grid_for: rpp = NT / (D / 4) rows per block, NT = 256


@pytest.mark.parametrize("D,n", BIG)
def test_fused_pair_past_the_grid_cap(D, n):
    """`ops.bn_relu_dropout` and `_bwd` (ReLU, gamma / beta, p = 0.5) on more rows than 2048 blocks hold, against the fp64 torch formula
    on the kernel's own kept pattern: activation 1e-5, grad_x / dbeta / dgamma 2e-5 of each tensor's max, running buffers 1e-6."""
    assert _blocks(n, D) > GRID_CAP
    x, gamma, beta, gy = _inputs(D, n)
    y, _, rm, rv, gx, gsum = _whole(D, True, True, n=n)
    assert y.shape == (n, D) and gx.shape == (n, D) and gsum.shape == (2 * D,)
    frac = float((y == 0).float().mean())
    assert abs(frac - P) < 0.5 / np.sqrt(n * D) * 6, frac                        # six sigma of a Bernoulli(0.5) mean
    y64, mean, var, gx64, dbeta, dgamma = _fp64_pair(x, gy, gamma, beta, True, y)
    errs = {"y": _rel(y, y64), "gx": _rel(gx, gx64), "dbeta": _rel(gsum[:D], dbeta), "dgamma": _rel(gsum[D:], dgamma)}
    bufs = {"running_mean": float((rm.double() - MOM * mean).abs().max()),
            "running_var": float((rv.double() - (1 - MOM + MOM * var * n / (n - 1))).abs().max())}
    print(f"D={D} n={n}: {errs} {bufs}")
    assert errs["y"] < 1e-5 and all(errs[k] < 2e-5 for k in ("gx", "dbeta", "dgamma")), errs
    assert all(v <= 1e-6 for v in bufs.values()), bufs


@pytest.mark.parametrize("layout", ["thirds", "all"])
@pytest.mark.parametrize("D,n", BIG)
def test_split_phase_past_the_grid_cap(D, n, layout):
    """colstats -> sum -> apply_rows, then bwd_reduce_rows -> sum -> bwd_apply_rows, against the fused pair on the same rows under the
    module's split-against-whole rule, dropout patterns identical.  "thirds": three parts dealt by `r % 3` plus one without rows
    (the parts' sums and global row numbers at scale; a third of the rows is 1367 blocks, so a part's own launch stays below the
    cap).  "all": every row in one part plus one without rows, so that the *_rows kernels themselves run past the cap."""
    assert _blocks(n, D) > GRID_CAP
    y_ref, stats, rm_ref, rv_ref, gx_ref, gsum_ref = _whole(D, True, True, n=n)
    y, totals, bufs, parts = _split_forward(D, True, True, n=n, layout=layout)
    sizes = [ids.shape[0] for ids in parts[0]]
    assert sum(sizes) == n and sizes[-1] == 0
    if layout == "all":
        assert _blocks(sizes[0], D) > GRID_CAP
    assert not bool(torch.isnan(y).any()) and torch.equal(y == 0, y_ref == 0), (D, n, layout, "dropout pattern")
    gx, gtot = _split_backward(D, True, True, totals, parts, n=n)
    worst = {"y": _close(y, y_ref), "gx": _close(gx, gx_ref), "gsum": _close(gtot, gsum_ref)}
    print(f"D={D} n={n} {layout}: worst / bar {({k: round(v[1], 4) for k, v in worst.items()})}")
    assert all(v[0] for v in worst.values()), worst
    assert _rel(totals, stats.view(-1, 2 * D).sum(0)) < 1e-12
    for rm, rv in bufs:
        assert float((rm - rm_ref).abs().max()) <= 1e-6 and float((rv - rv_ref).abs().max()) <= 1e-6


# ---- row stride -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [12, 128])
def test_rows_with_a_stride_beyond_the_width(D):
    """x and grad_y as `[:, :D]` views of [N, D + 4] buffers whose pad columns hold NaN: every entry, fused and split, returns what it
    returns on contiguous rows -- y, stats, grad_x, the gradient sums and the running buffers, bit for bit.
    The blocks' fp64 column sums reach their replica of the accumulator as atomics, in arrival order (98 blocks at D = 128: 12 or
    13 per replica), so equality of two calls needs sums that no order can round.  x and grad_y are therefore multiples of 2^-8
    below 32: sum x, sum x^2 (multiples of 2^-16 below 2^20) and sum g' are exact in fp64 whatever the order.  sum g'.xhat is
    not (xhat is any fp32 value): at D = 12 it is still order-free (10 blocks, at most two per replica, and a + b = b + a); at
    D = 128 two calls on the SAME buffer may differ in its last bits, so there it is held to what 13 additions in another order can
    move it, 2 * 13 * 2^-53 * sum |g'.xhat| per column, and grad_x, which reads it through an fp32 rounding, to equality."""
    from bridged_gnn_amd import ops
    x, gamma, beta, gy = _inputs(D)
    x, gy = torch.round(x * 256) / 256, torch.round(gy * 256) / 256
    assert float(x.abs().max()) < 32 and float(gy.abs().max()) < 32

    def strided(t):
        buf = torch.full((N, D + 4), float("nan"), device=DEV)
        buf[:, :D] = t
        return buf[:, :D]
    xs, gs = strided(x), strided(gy)
    assert xs.stride() == (D + 4, 1) and gs.stride() == (D + 4, 1) and bool(torch.isnan(xs._base[:, D:]).all())
    per_replica = -(-_blocks(N, D) // 8)                                         # bgnn_norm.hip: NREP = 8, block b adds into replica b % NREP
    assert per_replica == (2 if D == 12 else 13)
    xd = x.double()
    xh_abs = ((xd - xd.mean(0)) / torch.sqrt(xd.var(0, unbiased=False) + EPS)).abs()
    room = 2 * per_replica * 2.0 ** -53 * 1.01 * (2 * gy.double().abs() * xh_abs).sum(0)      # |g'| <= 2 |grad_y|; 1.01: xhat in fp32

    for relu, affine in COMBOS:
        g, b = (gamma, beta) if affine else (None, None)
        outs = []
        for xv, gv in ((x, gy), (xs, gs)):
            rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
            y, stats = ops.bn_relu_dropout(xv, g, b, EPS, relu, P, SEED, MOM, rm, rv)
            gx, gsum = ops.bn_relu_dropout_bwd(xv, gv, stats, g, b, EPS, relu, P, SEED)
            tot = ops.bn_colstats(xv)
            rm2, rv2 = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
            y2 = ops.bn_apply_rows(xv, tot, N, g, b, EPS, relu, P, SEED, row_base=0, momentum=MOM, running_mean=rm2, running_var=rv2)
            gtot = ops.bn_bwd_reduce_rows(xv, gv, tot, N, g, b, EPS, relu, P, SEED, row_base=0)
            gx2 = ops.bn_bwd_apply_rows(xv, gv, tot, gtot, N, g, b, EPS, relu, P, SEED, row_base=0)
            outs.append(dict(y=y, stats=stats, rm=rm, rv=rv, gx=gx, gsum=gsum, colstats=tot, y_rows=y2, rm_rows=rm2, rv_rows=rv2,
                             gsum_rows=gtot, gx_rows=gx2))
        want, got = outs
        assert not any(bool(torch.isnan(v).any()) for v in got.values()), "a pad column was read"
        for k in want:
            if k in ("gsum", "gsum_rows") and per_replica > 2:
                assert torch.equal(got[k][:D], want[k][:D]), (D, relu, affine, k, "sum g'")
                assert bool(((got[k][D:] - want[k][D:]).abs() <= room).all()), (D, relu, affine, k, "sum g'.xhat")
            else:
                assert torch.equal(got[k], want[k]), (D, relu, affine, k)
        assert torch.equal(got["y"] == 0, got["y_rows"] == 0)


# ---- numeric edges ----------------------------------------------------------------------------------------------------------------
EDGE_N, EDGE_D = 4101, 8


@functools.lru_cache(maxsize=None)
def _edge_case():
    """columns 0 / 1: mean / std = 1e3 / 2e3; 2 / 3: constants (one a dyadic fraction, one not); 4-7: plain normal deviates
    -> (x, grad_y) as fp32 numpy arrays"""
    rng = np.random.default_rng(8)
    x = rng.standard_normal((EDGE_N, EDGE_D))
    x[:, 0] = 100 + 0.1 * x[:, 0]
    x[:, 1] = 1000 + 0.5 * x[:, 1]
    x[:, 2] = 0.75
    x[:, 3] = np.float32(0.1)
    return x.astype(np.float32), rng.standard_normal((EDGE_N, EDGE_D)).astype(np.float32)


def _edge_ref64(x):
    """two-pass fp64 -> (mean, biased var, 1/std, xhat)"""
    xd = x.astype(np.float64)
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + EPS)
    return mean, var, rstd, (xd - mean) * rstd


def _edge_bound(x):
    """|y - xhat64| <= rstd64 * ulp32(|mean64|) / 2 + 8 * 2^-24 * |xhat64| per element: the first term is a mean rounded to fp32, the
    second three fp32 roundings (x - mean, 1/std, their product) with slack"""
    mean, _, rstd, ref = _edge_ref64(x)
    half_ulp = 0.5 * np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
    return rstd * half_ulp + 8 * 2.0 ** -24 * np.abs(ref)


def _edge_restatement(x):
    """the kernel's forward formula in numpy: fp64 sums of exact products, the mean as an fp32 pair (high and low word), 1/std in fp32,
    fp32 arithmetic on the elements"""
    xd = x.astype(np.float64)
    n = x.shape[0]
    m = xd.sum(0) / n
    var = np.maximum((xd * xd).sum(0) / n - m * m, 0.0)
    hi = m.astype(np.float32)
    lo = (m - hi.astype(np.float64)).astype(np.float32)
    rstd = (1.0 / np.sqrt(var + np.float64(np.float32(EPS)))).astype(np.float32)
    return ((x - hi) - lo) * rstd


def test_forward_numeric_edges():
    """no affine, no ReLU, p = 0: the output is xhat itself.  Constant columns are exactly 0 (the fp64 sum of N copies of an fp32 value
    and its quotient by N are exact, so x - mean is 0) and leave running_var at 0.9; every other element obeys the derived bound of
    `_edge_bound`, which the numpy restatement of the kernel's formula meets on the host.  A kernel that summed in fp32, or took
    the variance from fp32 moments, misses the bound by orders of magnitude on columns 0 and 1."""
    from bridged_gnn_amd import ops
    x, _ = _edge_case()
    mean, var, rstd, ref = _edge_ref64(x)
    assert 900 < mean[0] * rstd[0] < 1100 and 1800 < mean[1] * rstd[1] < 2200 and var[2] == 0 and var[3] == 0
    bound = _edge_bound(x)
    host = np.abs(_edge_restatement(x).astype(np.float64) - ref)
    assert (host <= bound).all(), "the bound must hold for the formula itself"
    rm, rv = torch.zeros(EDGE_D, device=DEV), torch.ones(EDGE_D, device=DEV)
    y, _ = ops.bn_relu_dropout(_t(x), None, None, EPS, False, 0.0, 0, MOM, rm, rv)
    y = y.cpu().numpy()
    assert np.count_nonzero(y[:, 2:4]) == 0, "a constant column normalises to exactly 0"
    assert float((rv[2:4].cpu().double() - (1 - MOM)).abs().max()) <= 1e-6
    err = np.abs(y.astype(np.float64) - ref)
    for c in range(EDGE_D):
        print(f"column {c}: max err {err[:, c].max():.3e} (host restatement {host[:, c].max():.3e}), bound {bound[:, c].max():.3e}, "
              f"worst err / bound {(err[:, c] / np.maximum(bound[:, c], 1e-300)).max():.3f}")
    assert (err <= bound).all()
    unb = var * EDGE_N / (EDGE_N - 1)
    assert np.abs(rm.cpu().numpy() - MOM * mean).max() <= 1e-6 * np.abs(MOM * mean).max()
    assert np.abs(rv.cpu().numpy() - (1 - MOM + MOM * unb)).max() <= 1e-6


def test_backward_numeric_edges():
    """grad_x, sum g' and sum g'.xhat on the same input against the fp64 formula at the gradient bar (2e-5 of each tensor's max),
    the constant columns included (xhat = 0, 1/std = 1/sqrt(eps) = 316).  The ill-conditioned columns get no tighter bound here
    than that bar; sum g'.xhat of column 1 is the entry that feels the mean: a mean rounded once to fp32 moves it by
    (ulp32(1000) / 2) / std * |sum g'| = 6e-5 * |sum g'|, which passes or misses the bar with the draw (on this draw it misses by
    5x), so the kernels carry the mean's low word."""
    from bridged_gnn_amd import ops
    x, gy = _edge_case()
    _, _, rstd, xh = _edge_ref64(x)
    gd = gy.astype(np.float64)
    want = {"gx": rstd * (gd - gd.mean(0) - xh * (gd * xh).mean(0)), "sum g'": gd.sum(0), "sum g'.xhat": (gd * xh).sum(0)}
    xt, gt = _t(x), _t(gy)
    _, stats = ops.bn_relu_dropout(xt, None, None, EPS, False, 0.0, 0)
    gx, gsum = ops.bn_relu_dropout_bwd(xt, gt, stats, None, None, EPS, False, 0.0, 0)
    tot = ops.bn_colstats(xt)
    gtot = ops.bn_bwd_reduce_rows(xt, gt, tot, EDGE_N, None, None, EPS, False, 0.0, 0)
    gx_rows = ops.bn_bwd_apply_rows(xt, gt, tot, gtot, EDGE_N, None, None, EPS, False, 0.0, 0)
    for name, a, s in (("fused", gx, gsum), ("split", gx_rows, gtot)):
        got = {"gx": a.cpu().numpy(), "sum g'": s[:EDGE_D].cpu().numpy(), "sum g'.xhat": s[EDGE_D:].cpu().numpy()}
        errs = {k: float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()) for k in want}
        k = "sum g'.xhat"
        print(f"{name}: {errs}; column 1 of {k}: {got[k][1]:.6f} against {want[k][1]:.6f}")
        assert all(v < 2e-5 for v in errs.values()), (name, errs)


def test_bad_calls_return_the_documented_codes():
    from bridged_gnn_amd import ops
    x = torch.randn(8, 6, device=DEV)                                            # D % 4 != 0
    with pytest.raises(RuntimeError, match="BGNN_E_SHAPE|shape"):
        ops.bn_colstats(x)
    x = torch.randn(8, 8, device=DEV)
    tot = ops.bn_colstats(x)
    with pytest.raises(RuntimeError, match="BGNN_E_SHAPE|shape"):                # n_total below the rank's own rows
        ops.bn_apply_rows(x, tot, 4, None, None, EPS, True, 0.0, 0)
