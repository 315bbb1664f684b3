"""GPU: the GIN baseline (bridged_gnn_amd.gin, models/backbones.py:26-57) on the fused HIP sum aggregation -- the forward entry
against an fp64 torch restatement (index_add_) of PyG's aggregate-first formula ((1 + eps) x_i + sum_{j -> i} x_j) W^T + b on the
generator of test_gpu_gcn.py with the shapes of test_gpu_appnp.py, the edges EXACTLY as generated (no self loop added or dropped;
A: 3000 nodes, no hub; B: 2000 nodes, node 3 with >= 700 in-edges and node 5 with >= 700 out-edges; both with duplicates, self
loops, rows without in-edges, asymmetric; C: 70 000 nodes, past the persistent grid's cap, a row of 30 000 edges, forward only;
A1: 3001 rows, a ragged last tile; A2: 20 000 nodes, past the backward's grids at D = 128), its epilogues and dropout law,
malformed input, the backward entry against fp64 autograd, GINConv.run under autograd, GINNet on the office fixture
(tools/gen_golden_gin.py) and `train_gin_noDTC`.
The table the entry takes is T = x W^T formed in fp64 and rounded once to fp32 (the GEMM is not under test here): the rounding
moves a sum of k rows by at most 2^-24 * sum |T_j|, far inside the bars.
Bars: those of test_gpu_gcn.py (activations 1e-5, gradients 2e-5 of each tensor's max); grad_eps: |deps - deps64| <= 2e-5 *
sum_i |g_i * T_i|.  Layer-level references take every ReLU / dropout state from the GPU forward's own output (mask = y > 0, scale
1 / (1 - p): the backward's contract), as test_gpu_gcn2.py explains and does.
The 30 000-edge row of graph C, restated on the CPU in fp32 in the kernel's own order (test_forward_past_the_persistent_cap
does it before the GPU run): with plain running sums it took 0.19 of the bar at D = 5 and 0.51 at D = 128 (on a randn table), so
the kernel adds each batch of U gathered rows to its running sum by a compensated add, as bgnn_gen.hip does; the restatement of
that order takes 0.006 at both widths.
Measured on an MI355X, worst error as a share of its bar (each test prints its own): forward 0.017 on graph A and 0.103 on graph
B; log_softmax 0.018 and 0.011; graph C 0.006 at D = 5 and at D = 128 (its 30 000-edge row: 0.006); backward 0.023 (grad_tbl) /
0.019 (grad_bias) / 0.000 (grad_eps) on graph A, 0.020 / 0.032 / 0.000 on graph B, 0.022 / 0.006 / 0.000 at 3001 rows, 0.030 / 0.015 /
0.000 on graph A2; layers 0.101 on graph A and 0.060 on graph B; the model 0.013 (logp) and 0.097 (gradients) on the graph as
shipped, 0.013 and 0.094 undirected, no ReLU kink flip."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub
from test_gin_host import OFFICE_MODELS, mult_adj, restate
from test_gpu_appnp import GRAPHS
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _dev, _graph

pytestmark = pytest.mark.gpu

KINK_CAP = 2e-4          # test_gpu_gcn.py's: the most a ReLU kink flip of the fp32 model moves a gradient tensor
DS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 100, 128, 129, 200)
EPSS = (0.0, 0.3, -1.0, -2.5)
DIN = 8
SEED = 1234
_CACHE = {}
_EXTRA = {"A1": dict(n=3001, e=30000, seed=24, hub=0), "A2": dict(n=20000, e=120000, seed=25, hub=0)}


def _case(name):
    """(n, SageGraph, src, dst) of graph A, B, C (test_gpu_appnp.GRAPHS), A1 or A2, edges as generated; built once"""
    if name not in _CACHE:
        from bridged_gnn_amd.sage import SageGraph
        cfg = GRAPHS.get(name) or _EXTRA[name]
        n, hub = cfg["n"], cfg["hub"]
        ei = _graph(n, cfg["e"], seed=cfg["seed"], hub=hub)
        indeg, outdeg = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
        assert (indeg == 0).any() and not np.array_equal(indeg, outdeg)                 # rows without in-edges; asymmetric
        assert (ei[0] == ei[1]).any()                                                    # self loops, ordinary edges here
        pairs = ei[0] * n + ei[1]
        assert np.unique(pairs).shape[0] < pairs.shape[0]                                # duplicates
        if hub:
            assert indeg[3] >= hub and outdeg[5] >= hub
        eid = torch.from_numpy(ei).to(_dev())
        g = SageGraph(eid, n)
        assert g.csr.num_edges == ei.shape[1]                                            # nothing added, nothing dropped
        _CACHE[name] = (n, g, eid[0], eid[1])
    return _CACHE[name]


def _agg64(x, src, dst, eps):
    """(1 + eps) x_i + sum_{j -> i} x_j in fp64"""
    return (1.0 + eps) * x + torch.zeros_like(x).index_add_(0, dst, x[src])


def _share(got, ref, bar):
    return (got.double() - ref).abs().max().item() / (bar * ref.abs().max().item() + 1e-6)


def _ok(got, ref, bar, what):
    _bar_ok(got.double().cpu(), ref.detach().cpu().numpy(), bar, what)
    return _share(got, ref.detach(), bar)


def _inputs(rng, n, D, dev):
    """x [n, DIN], W [D, DIN], b [D] in fp64 and T = x W^T rounded once to fp32, [n, pad4(D)] with zero pad columns"""
    from bridged_gnn_amd import ops
    x = torch.from_numpy(rng.standard_normal((n, DIN))).to(dev)
    W = torch.from_numpy(rng.standard_normal((D, DIN)) / np.sqrt(DIN)).to(dev)
    b = torch.from_numpy(rng.standard_normal(D)).to(dev)
    T = torch.zeros(n, ops.pad4(D), dtype=torch.float32, device=dev)
    T[:, :D] = (x @ W.t()).float()
    return x, W, b, T


def _et(eps, dev):
    return torch.tensor([eps], dtype=torch.float32, device=dev)


def _bias(b, D, dev):
    from bridged_gnn_amd import ops
    bp = torch.zeros(ops.pad4(D), dtype=torch.float32, device=dev)
    bp[:D] = b.float()
    return bp


def _fwd(T, g, eps, n, D, **kw):
    from bridged_gnn_amd import ops
    return ops.gin_aggregate(T, g.by_dst[0], g.by_dst[1], eps, n, D, **kw)


# ---- forward entry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_every_width_and_eps(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(71)
    worst = 0.0
    for D in DS:
        Dp = ops.pad4(D)
        x, W, b, T = _inputs(rng, n, D, dev)
        bp = _bias(b, D, dev)
        b32 = bp[:D].double()
        # T as a view of a wider buffer, once per width: what surrounds the view and its pad columns hold NaN
        wide = torch.full((n, Dp + 8), float("nan"), device=dev)
        wide[:, 4:4 + D] = T[:, :D]
        Tv = wide[:, 4:4 + Dp]
        for k, eps in enumerate(EPSS):
            what = f"graph {name} D={D} eps={eps}"
            bias = None if k == 1 else bp                                # without bias once per width
            ref = _agg64(x, src, dst, float(np.float32(eps))) @ W.t()
            if bias is not None:
                ref = ref + b32
            out = _fwd(Tv if k == 0 else T, g, _et(eps, dev), n, D, bias=bias)
            worst = max(worst, _ok(out[:, :D], ref, ACT_BAR, what))
            assert bool(torch.isfinite(out).all()), what
            if Dp > D:
                assert torch.count_nonzero(out[:, D:]).item() == 0, what + ": pad columns must be 0"
            if k == 0:                                                   # eps = 0: no eps tensor gives the same bits
                assert torch.equal(_fwd(T, g, None, n, D, bias=bias), out), what + ": eps=None is not eps=0"
            if eps == -1.0:                                              # the self term vanishes: the plain sum of the SAGE entry
                plain = ops.sage_mean_aggregate(T, g.by_dst[0], g.by_dst[1], n, D, mean=False)
                worst = max(worst, _ok(out[:, :D] - (bp[:D] if bias is not None else 0), plain[:, :D].double(), ACT_BAR, what + " vs plain sum"))
        # the eps tensor is read by the kernel at every call: no host value is cached
        e = _et(0.3, dev)
        o1 = _fwd(T, g, e, n, D, bias=bp)
        e.fill_(-2.5)
        o2 = _fwd(T, g, e, n, D, bias=bp)
        assert torch.equal(o2, _fwd(T, g, _et(-2.5, dev), n, D, bias=bp)) and not torch.equal(o1, o2), f"graph {name} D={D}: a cached eps"
    print(f"graph {name}: worst forward error {worst:.3f} of the bar")


@pytest.mark.parametrize("name", ["A", "B"])
def test_log_softmax_epilogue_and_its_width_limit(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(72)
    worst = 0.0
    for D in (2, 31, 128):
        x, W, b, T = _inputs(rng, n, D, dev)
        bp = _bias(b, D, dev)
        ref = torch.log_softmax(_agg64(x, src, dst, float(np.float32(0.3))) @ W.t() + bp[:D].double(), 1)
        out = _fwd(T, g, _et(0.3, dev), n, D, bias=bp, epilogue="log_softmax")
        worst = max(worst, _ok(out[:, :D], ref, ACT_BAR, f"graph {name} D={D} log_softmax"))
        if ops.pad4(D) > D:
            assert torch.count_nonzero(out[:, D:]).item() == 0
    x, W, b, T = _inputs(rng, n, 129, dev)
    with pytest.raises(ValueError, match="D <= 128"):
        _fwd(T, g, _et(0.3, dev), n, 129, epilogue="log_softmax")
    # the C entry refuses it as well (a shape error), for a caller that goes round ops.py
    from bridged_gnn_amd import _lib as L
    out = torch.empty(n, ops.pad4(129), device=dev)
    rc = L.lib().bgnn_gin_aggregate_f32(L.ptr_rows(T), T.stride(0), n, None, None, L.ptr(g.by_dst[0]), L.ptr(g.by_dst[1]),
                                        int(g.by_dst[1].shape[0]), n, 129, 2, 0.0, 0, None, None, L.ptr_rows(out), out.stride(0), L.stream())
    assert rc == -2
    print(f"graph {name}: worst log_softmax error {worst:.3f} of the bar")


def _permuted(g, n, idx, T, dev):
    """the rows idx of the graph as a call of their own: (table with those rows first, rowptr, col) with col renumbered"""
    rowptr = g.by_dst[0].cpu().numpy().astype(np.int64)
    col = g.by_dst[1].cpu().numpy()
    rest = np.setdiff1d(np.arange(n), idx)
    perm = np.concatenate([idx, rest])
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    cols = [inv[col[rowptr[r]:rowptr[r + 1]]] for r in idx]
    rp = np.concatenate([[0], np.cumsum([c.shape[0] for c in cols])]).astype(np.int32)
    return (T[torch.from_numpy(perm).to(dev)].contiguous(), torch.from_numpy(rp).to(dev),
            torch.from_numpy(np.concatenate(cols).astype(np.int32)).to(dev))


@pytest.mark.parametrize("name", ["A", "B"])
def test_relu_dropout_mask_law_seeds_and_row_ids(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(73)
    for D in (5, 64, 200):
        x, W, b, T = _inputs(rng, n, D, dev)
        bp = _bias(b, D, dev)
        e = _et(0.3, dev)
        what = f"graph {name} D={D}"
        z = _fwd(T, g, e, n, D, bias=bp)
        y0 = _fwd(T, g, e, n, D, bias=bp, epilogue="relu")
        assert torch.equal(y0, torch.relu(z)), what + ": relu epilogue"
        y = _fwd(T, g, e, n, D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED)
        # the mask `ops.feature_dropout` draws for an [n, D] tensor of ones with the same seed, scaled by the same keep scale
        m = ops.feature_dropout(torch.ones(n, D, device=dev), 0.5, SEED)
        keep = m > 0
        assert 0.45 < keep.float().mean().item() < 0.55 and bool((m[keep] == 2.0).all())
        assert torch.equal(y[:, :D], y0[:, :D] * m), what + ": kept elements are the no-dropout output times the keep scale, the rest 0"
        if ops.pad4(D) > D:
            assert torch.count_nonzero(y[:, D:]).item() == 0
        assert not torch.equal(_fwd(T, g, e, n, D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED + 1), y), what + ": two seeds, one mask"
        word = torch.tensor([1000], dtype=torch.int64, device=dev)
        assert torch.equal(_fwd(T, g, e, n, D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED - 1000, seed_dev=word), y), \
            what + ": seed + device word is the seed"
        # a row subset with its global ids draws the whole-graph masks of those rows (and sums the same rows in the same order)
        idx = np.sort(np.random.default_rng(74).choice(n, 517, replace=False))
        Tp, rp, cp = _permuted(g, n, idx, T, dev)
        ids = torch.from_numpy(idx).to(dev)
        ys = ops.gin_aggregate(Tp, rp, cp, e, idx.shape[0], D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED, row_ids=ids)
        assert torch.equal(ys, y[ids]), what + ": row_ids"
        if idx[0] != 0 or idx[-1] != idx.shape[0] - 1:
            assert not torch.equal(ops.gin_aggregate(Tp, rp, cp, e, idx.shape[0], D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED), y[ids])


def _walk32(rows, U):
    """the kernel's running sum of one sub-group in fp32: batches of U rows, each entering by a compensated add"""
    acc = np.zeros(rows.shape[1], np.float32)
    cmp = np.zeros_like(acc)
    for k in range(0, rows.shape[0], U):
        b = rows[k].copy()
        for r in rows[k + 1:k + U]:
            b = b + r
        y = b - cmp
        t = acc + y
        cmp = (t - acc) - y
        acc = t
    return acc


@pytest.mark.parametrize("D", [5, 128])
def test_forward_past_the_persistent_cap(D):
    """graph C.  The row of 30 000 in-edges (node 3), restated in fp32 on the CPU in the kernel's summation order before the GPU
    run, takes 0.007 of the bar at D = 5 and 0.006 at D = 128 (plain running sums: 0.19 and 0.51, which is why the batches enter
    by compensated adds)."""
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case("C")
    # bgnn_gin.hip gin_agg_kernel: RPB = 4 * (64 / (LF * EP)) rows per tile; lf_ladder: (LF, EP, U) = (2, 4, 4) at D = 5 -> 32 rows,
    # (32, 1, 8) at D = 128 -> 8 rows; bgnn_conv_common.h persistent_grid: at most 8 blocks per CU
    rpb, EP, U = {5: (32, 4, 4), 128: (8, 1, 8)}[D]
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-n // rpb) > cap, f"graph C must have more tiles of {rpb} rows than the {cap} blocks of a persistent grid"
    rng = np.random.default_rng([75, D])
    x, W, b, T = _inputs(rng, n, D, dev)
    bp = _bias(b, D, dev)
    eps = 0.3
    ref = _agg64(x, src, dst, float(np.float32(eps))) @ W.t() + bp[:D].double()
    # the hub row in the kernel's order: sub-group s of EP walks the row's edges s, s + EP, ... in batches of U; fixed butterfly
    rowptr = g.by_dst[0].cpu().numpy()
    cols = g.by_dst[1].cpu().numpy()[rowptr[3]:rowptr[4]]
    assert cols.shape[0] >= 30000
    Tc = T[:, :D].cpu().numpy()
    subs = [_walk32(Tc[cols[s::EP]], U) for s in range(EP)]
    while len(subs) > 1:
        subs = [subs[k] + subs[k + 1] for k in range(0, len(subs), 2)]
    self_w = np.float32(1.0) + np.float32(eps)
    cpu = (self_w.astype(np.float64) * Tc[3] + subs[0]).astype(np.float32) + bp[:D].cpu().numpy()     # fma: one rounding
    tol = ACT_BAR * ref.abs().max().item() + 1e-6
    cpu_share = np.abs(cpu.astype(np.float64) - ref[3].cpu().numpy()).max() / tol
    print(f"graph C D={D}: the 30 000-edge row restated in fp32 takes {cpu_share:.3f} of the bar")
    assert cpu_share <= 0.5
    out = _fwd(T, g, _et(eps, dev), n, D, bias=bp)
    worst = _ok(out[:, :D], ref, ACT_BAR, f"graph C D={D}")
    hub = (out[3, :D].double() - ref[3]).abs().max().item() / tol
    if ops.pad4(D) > D:
        assert torch.count_nonzero(out[:, D:]).item() == 0
    print(f"graph C D={D}: worst forward error {worst:.3f} of the bar (the 30 000-edge row: {hub:.3f})")


def test_malformed_csr_gives_finite_wrong_sums_and_no_error_state():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case("A")
    rng = np.random.default_rng(76)
    rowptr, col = g.by_dst[0], g.by_dst[1]
    E = int(col.shape[0])
    for D in (5, 64, 200):
        x, W, b, T = _inputs(rng, n, D, dev)
        good = _fwd(T, g, _et(0.3, dev), n, D)
        # ids at and past the table, and negative ones: those edges add nothing
        bad = col.clone()
        bad[::97] = n
        bad[5::101] = n + 12345
        bad[7::103] = -3
        ok = ((bad >= 0) & (bad < n))
        csr_dst = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:n + 1] - rowptr[:n]).long())
        ref = (1.0 + float(np.float32(0.3))) * T[:, :D].double() + \
            torch.zeros(n, D, dtype=torch.float64, device=dev).index_add_(0, csr_dst[ok], T[:, :D].double()[bad[ok].long()])
        out = ops.gin_aggregate(T, rowptr, bad, _et(0.3, dev), n, D)
        _ok(out[:, :D], ref, ACT_BAR, f"D={D}: ids outside the table add nothing")
        # a table shorter than the ids: rows past n_tbl are never read
        half = n // 2
        out = ops.gin_aggregate(T[:half + 8], rowptr, col, _et(0.3, dev), half, D)
        assert bool(torch.isfinite(out).all())
        # a rowptr that is not monotone: wrong sums, finite, nothing read past the edge arrays
        rp = rowptr.clone()
        rp[10:2000:7] = rp[10:2000:7].flip(0)
        out = ops.gin_aggregate(T, rp, col, _et(0.3, dev), n, D)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and tuple(out.shape) == (n, ops.pad4(D))
        assert not torch.equal(out, good)
        assert int(rp.max()) <= E and int(rp.min()) >= 0
        assert torch.equal(_fwd(T, g, _et(0.3, dev), n, D), good)                   # and the next well-formed call is unharmed


# ---- backward entry ----------------------------------------------------------------------------------------------
def _backward_case(name, D, epi, eps, rng, worst):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case(name)
    Dp = ops.pad4(D)
    x, W, b, T = _inputs(rng, n, D, dev)
    bp = _bias(b, D, dev)
    e = _et(eps, dev)
    p = 0.5 if epi == "relu" else 0.0
    y = _fwd(T, g, e, n, D, bias=bp, epilogue=epi, p_drop=p, seed=SEED)
    t_rowptr, t_dst = g.by_dst[2], g.by_dst[3]
    dy = torch.zeros(n, Dp, device=dev)
    dy[:, :D] = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
    what = f"graph {name} D={D} epi={epi} eps={eps}"
    gt, gb, ge = ops.gin_aggregate_bwd(T, y, dy, t_rowptr, t_dst, e, n, D, epilogue=epi, p_drop=p)
    gt2, gb2, ge2 = ops.gin_aggregate_bwd(T, y, dy, t_rowptr, t_dst, e, n, D, epilogue=epi, p_drop=p)
    assert torch.equal(gt, gt2) and torch.equal(gb, gb2) and torch.equal(ge, ge2), what + ": two runs differ"
    assert tuple(ge.shape) == (1,) and ge.dtype == torch.float32 and tuple(gb.shape) == (D,) and tuple(gt.shape) == (n, Dp)
    # without grad_eps: no eps pass, no table needed, the same grad_tbl and grad_bias
    gt3, gb3, ge3 = ops.gin_aggregate_bwd(None, y, dy, t_rowptr, t_dst, e, n, D, epilogue=epi, p_drop=p, want_eps=False)
    assert ge3 is None and torch.equal(gt3, gt) and torch.equal(gb3, gb), what + ": want_eps=False"
    assert ops.gin_aggregate_bwd(T, y, dy, t_rowptr, t_dst, e, n, D, epilogue=epi, p_drop=p, want_bias=False)[1] is None
    # fp64 autograd; the ReLU / dropout state is the forward output's (y > 0, scale 1 / (1 - p))
    t64 = T[:, :D].double().requires_grad_(True)
    b64 = bp[:D].double().requires_grad_(True)
    e64 = e.double().requires_grad_(True)
    pre = _agg64(t64, src, dst, e64) + b64
    if epi == "relu":
        out = pre * (y[:, :D] > 0).double() / (1.0 - p)
    elif epi == "log_softmax":
        out = torch.log_softmax(pre, 1)
    else:
        out = pre
    rt, rb, re_, rg = torch.autograd.grad((out * dy[:, :D].double()).sum(), [t64, b64, e64, pre])
    worst[0] = max(worst[0], _ok(gt[:, :D], rt, GRAD_BAR, what + " grad_tbl"))
    worst[1] = max(worst[1], _ok(gb, rb, GRAD_BAR, what + " grad_bias"))
    err, tol = abs(ge.item() - re_.item()), GRAD_BAR * (rg * t64.detach()).abs().sum().item()
    print(f"{what} grad_eps: err {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what} grad_eps: {ge.item()} vs {re_.item()}, err {err:.3e} > {tol:.3e}"
    worst[2] = max(worst[2], err / tol if tol > 0 else 0.0)     # log_softmax over one column: g = 0, both sides exactly 0
    if Dp > D:
        assert torch.count_nonzero(gt[:, D:]).item() == 0, what + ": pad columns must be 0"


def _backward_cases(name, widths, seed):
    rng = np.random.default_rng(seed)
    worst = [0.0, 0.0, 0.0]
    for D in widths:
        for epi, eps in ((None, 0.3), ("relu", -2.5), ("log_softmax", 0.0)):
            if epi == "log_softmax" and D > 128:
                continue
            _backward_case(name, D, epi, eps, rng, worst)
    print(f"graph {name}: worst backward error {worst[0]:.3f} (grad_tbl), {worst[1]:.3f} (grad_bias), {worst[2]:.3f} (grad_eps) of the bar")


@pytest.mark.parametrize("name", ["A", "B"])
def test_backward_matches_fp64_autograd_and_is_deterministic(name):
    _backward_cases(name, (1, 5, 31, 64, 128, 129, 200), 77)


def test_backward_at_3001_rows():
    _backward_cases("A1", (5, 64, 200), 78)


def test_backward_past_the_grid_caps():
    """graph A2 (20 000 nodes, no hub) at D = 128: more tiles of 8 rows than the persistent grid of pass B has blocks, and more
    blocks' worth of rows than the 2048 blocks of the row passes, so blocks walk several tiles and the fp64 partials of grad_eps
    are made of more than one tile"""
    n = _EXTRA["A2"]["n"]
    # bgnn_gin.hip: pass B is gin_agg_kernel (8 rows per tile at D = 128, persistent_grid: at most 8 blocks per CU); the row passes
    # (conv_bwd_rows_kernel, gin_eps_dot_kernel: 256 / LF = 8 rows per block at D = 128) launch at most 2048 blocks
    cap = max(8 * torch.cuda.get_device_properties(0).multi_processor_count, 2048)
    assert -(-n // 8) > cap, f"graph A2 must have more tiles of 8 rows than the {cap} blocks of the backward's grids"
    _backward_cases("A2", (128,), 79)


# ---- the layer under autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_ginconv_run_gradients(name):
    from bridged_gnn_amd.gin import GINConv
    from bridged_gnn_amd.ktgnn import Linear
    dev = _dev()
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(80)
    worst = 0.0
    for din, D, epi, p, train_eps in ((12, 5, "relu", 0.5, True), (64, 64, "relu", 0.5, True), (40, 200, "relu", 0.0, True),
                                      (64, 128, "log_softmax", 0.0, True), (33, 31, None, 0.0, True), (64, 64, "relu", 0.5, False),
                                      (16, 130, "log_softmax", 0.0, True)):
        torch.manual_seed(din + D)
        conv = GINConv(Linear(din, D), eps=0.3, train_eps=train_eps).to(dev)
        x = torch.from_numpy(rng.standard_normal((n, din)).astype(np.float32)).to(dev)
        dy = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
        what = f"graph {name} {din}->{D} epi={epi} p={p} train_eps={train_eps}"
        xd = x.clone().requires_grad_(True)
        y = conv.run(xd, g, epilogue=epi, p_drop=p)
        names = [k for k, _ in conv.named_parameters()]
        assert ("eps" in names) == train_eps
        got = torch.autograd.grad((y * dy).sum(), [xd] + [prm for _, prm in conv.named_parameters()])
        P = {k: v.detach().double().requires_grad_(True) for k, v in conv.state_dict().items()}
        x64 = x.double().requires_grad_(True)
        pre = _agg64(x64, src, dst, P["eps"]) @ P["nn.weight"].t() + P["nn.bias"]
        if epi == "relu":                                               # the GPU forward's own ReLU / dropout state
            out = pre * (y.detach() > 0).double() / (1.0 - p)
            if p > 0:
                assert 0.15 < (y.detach() > 0).float().mean().item() < 0.35
        elif epi == "log_softmax":
            out = torch.log_softmax(pre, 1)
        else:
            out = pre
        worst = max(worst, _ok(y.detach(), out, ACT_BAR, what + " forward"))
        ref = torch.autograd.grad((out * dy.double()).sum(), [x64] + [P[k] for k in names])
        for gg, rr, k in zip(got, ref, ["x"] + names):
            worst = max(worst, _ok(gg.reshape(rr.shape), rr, GRAD_BAR, f"{what} grad {k}"))
        if p == 0:
            with torch.no_grad():
                _ok(conv.run(x, g, epilogue=epi), out, ACT_BAR, what + " under no_grad")
    print(f"graph {name}: worst layer error {worst:.3f} of the bar")


# ---- model level -------------------------------------------------------------------------------------------------
def _fixture_case(variant):
    from bridged_gnn_amd.data import Data
    dev = _dev()
    g, fx = load_golden("office_a2d_graph.npz"), load_golden("gin_office_a2d.npz")
    data = Data(x=torch.from_numpy(g["x"]).to(dev), edge_index=torch.from_numpy(g["edge_index"]).long().to(dev),
                y=torch.from_numpy(g["y"]).long().to(dev))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(fx["train_mask"]).to(dev)          # the driver's mask (y == -1 cleared, :404)
    ds = types.SimpleNamespace(num_features=g["x"].shape[1], num_classes=int(g["y"].max()) + 1)
    return data, tm, ds, fx


def _model(ds, fx, name, L, hidden, dropout=0.5):
    """the fixture's model: torch.manual_seed(0), checked against the stored parameter sums"""
    from bridged_gnn_amd.gin import GINNet
    torch.manual_seed(0)
    m = GINNet(ds, layer_num=L, hidden=hidden, dropout=dropout)
    sums = sub(fx, f"{name}/param_sum/")
    assert sorted(sums) == sorted(m.state_dict())
    for k, v in m.state_dict().items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, atol=1e-300, err_msg=k)
    return m.to(_dev())


def _params64(m):
    leaves = {k for k, _ in m.named_parameters()}
    return {k: v.detach().double().cpu().requires_grad_(k in leaves) for k, v in m.state_dict().items()}


def _ref_grads(fx, pre, P, names, x64, A, y, tm, relu_masks=None):
    """the fixture's gradients where it holds them, else those of the fp64 restatement test_gin_host.py pins to the fixture"""
    if relu_masks is None and sub(fx, pre + "grad/"):
        return {k: fx[pre + "grad/" + k] for k in names}
    loss = F.nll_loss(restate(P, x64, A, relu_masks=relu_masks)[tm], y[tm])
    return {k: gr.numpy() for k, gr in zip(names, torch.autograd.grad(loss, [P[k] for k in names]))}


@pytest.mark.parametrize("variant", ["raw", "und"])
def test_model_matches_the_reference_fixture(variant):
    data, tm, ds, fx = _fixture_case(variant)
    rows = torch.from_numpy(fx["rows"])
    x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
    A = mult_adj(data.edge_index.cpu(), x64.shape[0])
    worst = [0.0, 0.0]
    for name, L, hidden in OFFICE_MODELS:
        m = _model(ds, fx, name, L, hidden).eval()
        P = _params64(m)
        names = [k for k, _ in m.named_parameters()]
        assert ("convs.0.eps" in names) == (L > 1)
        pre = f"{variant}/{name}/"
        with torch.no_grad():
            lp = m(data).cpu()
        _bar_ok(lp[rows], fx[pre + "logp"], ACT_BAR, pre + "logp")                              # the reference, at the fixture's rows
        ref_lp = restate(P, x64, A).detach()
        _bar_ok(lp, ref_lp.numpy(), ACT_BAR, pre + "logp (every row, fp64 restatement)")
        worst[0] = max(worst[0], _share(lp, ref_lp, ACT_BAR))
        ref = _ref_grads(fx, pre, P, names, x64, A, y, tmc)
        out = m(data)                                                                             # the autograd path, eval mode
        _bar_ok(out.detach().cpu()[rows], fx[pre + "logp"], ACT_BAR, pre + "logp (autograd path)")
        loss = F.nll_loss(out[tm], data.y[tm])
        assert abs(loss.item() - float(fx[pre + "loss"])) <= 1e-5 * abs(float(fx[pre + "loss"]))
        loss.backward()
        bad = []
        for k, prm in m.named_parameters():
            got = prm.grad.double().cpu().numpy()
            err = np.abs(got - ref[k]).max()
            print(f"{pre}{k}: grad err {err / np.abs(ref[k]).max():.3e} of max")
            if err > GRAD_BAR * np.abs(ref[k]).max():
                assert err <= KINK_CAP * np.abs(ref[k]).max(), f"{pre}{k}: {err:.3e} beyond any ReLU kink flip"
                bad.append(k)
            else:
                worst[1] = max(worst[1], err / (GRAD_BAR * np.abs(ref[k]).max()))
        if bad:
            # ReLU kink flips: an fp32 pre-activation within rounding of zero may take the other side.  The fp64 restatement
            # with the GPU's ReLU pattern must then meet the ordinary bar on every tensor.
            with torch.no_grad():
                g = m.graph(data.edge_index, data.x.shape[0])
                h, masks = data.x, []
                for conv in m.convs[:-1]:
                    h = conv.run(h, g, epilogue="relu")
                    masks.append(torch.from_numpy((h.cpu().numpy() > 0).astype(np.float64)))
            ref = _ref_grads(fx, pre, P, names, x64, A, y, tmc, relu_masks=masks)
            for k, prm in m.named_parameters():
                _bar_ok(prm.grad.cpu(), ref[k], GRAD_BAR, f"{pre}{k} (GPU ReLU pattern)")
            print(f"{pre}: ReLU kink flips explained for {bad}")
    print(f"GINNet {variant}: worst error {worst[0]:.3f} (logp), {worst[1]:.3f} (gradients) of the bar")


def test_adam_trajectory_matches_the_reference_fixture():
    for variant in ("raw", "und"):
        data, tm, ds, fx = _fixture_case(variant)
        x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
        A = mult_adj(data.edge_index.cpu(), x64.shape[0])
        for name, L, hidden in OFFICE_MODELS:
            m = _model(ds, fx, name, L, hidden, dropout=0.0).train()
            pre = f"{variant}/{name}/"
            names = [k for k, _ in m.named_parameters()]
            if sub(fx, pre + "adam/"):
                ref = {k: fx[pre + "adam/" + k] for k in names}
            else:                                            # the fp64 restatement's five steps
                P = _params64(m)
                ropt = torch.optim.Adam([P[k] for k in names], lr=1e-3, weight_decay=5e-3)
                for _ in range(5):
                    ropt.zero_grad()
                    F.nll_loss(restate(P, x64, A)[tmc], y[tmc]).backward()
                    ropt.step()
                ref = {k: P[k].detach().numpy() for k in names}
            opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(m(data)[tm], data.y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            np.testing.assert_allclose(losses, fx[pre + "adam_loss"], rtol=1e-5, err_msg=pre)
            for k, prm in m.named_parameters():
                _bar_ok(prm.detach().cpu(), ref[k], 1e-4, pre + "adam/" + k)


# ---- driver ------------------------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(dataset_name="office")


def _run(data, hist, **kw):
    from bridged_gnn_amd import gin, transfer
    cfg = dict(repeat=1, num_epoch=8, use_scheduler=False, seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)
    cfg.update(kw)
    return gin.train_gin_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, **cfg)


def test_driver_loss_falls_runs_are_seeded_and_the_checkpoint_loads_back(tmp_path):
    from bridged_gnn_amd import gin, transfer
    from test_gpu_appnp import _office_data
    data = _office_data()
    h0, h1, h2 = {}, {}, {}
    assert _run(data, h0, dropout=0.0, num_layer=3) is None
    assert len(h0["loss_train"]) == 8 and len(h0["eval_res"]) == 8 and all(len(r) == 3 for r in h0["eval_res"])
    assert 0 <= h0["best_epoch"] < 8
    print("GIN driver losses", h0["loss_train"])
    assert all(np.isfinite(h0["loss_train"])) and all(np.isfinite(np.asarray(h0["eval_res"], dtype=np.float64)).ravel())
    assert h0["loss_train"][-1] < h0["loss_train"][0]
    assert _run(data, h1, save=True, ckpt_dir=str(tmp_path)) is None and _run(data, h2) is None
    assert all(np.isfinite(h1["loss_train"])) and all(np.isfinite(np.asarray(h1["eval_res"], dtype=np.float64)).ravel())
    assert h1["loss_train"] == h2["loss_train"] and h1["eval_res"] == h2["eval_res"]        # the host generator's seeds, no atomics
    path = os.path.join(str(tmp_path), "model_GIN_office_share_best.ckpt")
    assert os.path.exists(path)
    m = gin.GINNet(transfer.pyg_dataset(data), 2, hidden=64).to(_dev())
    m.load_state_dict(torch.load(path, map_location=_dev()), strict=True)
    assert transfer.test_noDTC(data, m) == h1["eval_res"][h1["best_epoch"]]
    with pytest.raises(NotImplementedError, match="graphed"):
        _run(data, {}, graphed=True)


def test_main_runs_from_a_saved_bridged_graph(tmp_path, capsys):
    from bridged_gnn_amd import gin
    from bridged_gnn_amd.data import Data, save_bridged_graph
    og = load_golden("office_a2d_graph.npz")
    d = Data(x=torch.from_numpy(og["x"]), edge_index=torch.from_numpy(og["edge_index"]).long(), y=torch.from_numpy(og["y"]).long(),
             **{k: torch.from_numpy(og[k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    path = str(tmp_path / "office_amazon2dslr_bridged_graph.dat")
    save_bridged_graph(d, path)
    res = gin.main(["--num_layer", "3", "--hidden_dim", "32", "--num_epoch", "3", "--dataset_name", "office_amazon2dslr", "--path_data", path,
                    "--to_undirected", "--dropout", "0.2"])
    out = capsys.readouterr().out
    assert res is None
    assert out.count("Epoch: 00") == 3 and "[Run-1 score]" in out and "GINNet" in out and "nan" not in out.lower()
