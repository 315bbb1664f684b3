"""GPU: the JKNet baseline (bridged_gnn_amd.jknet, models/backbones.py:60-107) on the fused HIP convs and jumping-knowledge head.

The conv entry against an fp64 torch restatement (index_add_) of out_i = w_i T_i + s_i sum_{j -> i} s_j T_j + b on the generator of
test_gpu_gcn.py with the shapes of test_gpu_appnp.py and the extra cases of test_gpu_gin.py, self loops dropped and none appended
(A: 3000 nodes, no hub; B: 2000 nodes, node 3 with >= 700 in-edges and node 5 with >= 700 out-edges; A1: 3001 rows, a ragged last
tile; C: 70 000 nodes, past the persistent grid's cap, a row of 30 000 edges, forward only; A2: 20 000 nodes, past the backward's
grids at D = 128): every width with and without bias, as views inside NaN-filled wider buffers, against `ops.gcn_aggregate` with
w = s^2, the dropout law; its backward against fp64 autograd with equal bits on two runs; the head against fp64 in both modes with
the winners of max mode pinned to torch's rule (lowest layer on exact ties) and its backward against fp64 autograd with the
winners taken from the GPU forward's own uint8 state (the backward's contract, as test_gpu_gcn2.py does for ReLU states); JKNet on
the office and small fixtures (tools/gen_golden_jknet.py) and `train_jknet_noDTC`.
The table the conv entry takes is T = x W^T formed in fp64 and rounded once to fp32, and the references take the entry's own fp32
s and w (the graph's fp64 scales rounded once; the rounding itself is checked against an fp64 restatement to one ulp).
Bars: those of test_gpu_gcn.py (activations 1e-5, gradients 2e-5 of each tensor's max).  The fixture tool reported no gradient
tensor of the fp32 reference beyond GRAD_BAR, so no model gradient may lean on KINK_CAP.
Restated on the CPU in fp32 in the kernels' own order before the GPU runs (test_cpu_restatements_of_the_kernels_orders): the head's
widest product (L * H = 512, C = 32: four split-K partial chains of 128 fmas per class) takes 0.020 of the activation bar (as one
chain of 512: 0.061), the conv's 30 000-edge row with its compensated batch adds 0.001 at D = 5 and at D = 128 (a plain running
sum: 0.010; the row's scales s are about 1 / 170, so its sum is small against the tensor's maximum).
Measured on an MI355X, worst error as a share of its bar (each test prints its own): conv forward 0.008 on graph A, 0.007 on B,
0.008 at 3001 rows; against gcn_aggregate 0.011; graph C 0.006 at D = 5 and 0.007 at D = 128 (its 30 000-edge row: 0.001); conv
backward 0.005 (grad_tbl) / 0.003 (grad_bias) on graph A, 0.004 / 0.002 on B, at 3001 rows and on A2; head forward 0.025 at 3001
rows (cat and max), 0.027 (cat) and 0.020 (max) at 70 000; head backward 0.014 (grad_x) / 0.065 (grad_weight) / 0.016 (grad_bias)
in cat mode and 0.022 / 0.011 / 0.008 in max mode; the model 0.018 (logp) and 0.110 (gradients) on the graph as shipped, 0.021 and
0.065 undirected, no gradient tensor beyond the bar."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, sub
from test_gpu_appnp import GRAPHS
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _dev, _graph
from test_gpu_gin import _EXTRA
from test_jknet_host import OFFICE_MODELS, SMALL_MODELS, mult_adj, operator, restate

pytestmark = pytest.mark.gpu

DS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 100, 128, 129, 200)
DIN = 8
SEED = 4321
_CACHE = {}


def _scales64(src, dst, n, renormalize=True):
    """(s, w) in fp64 from the loop-free edges, by index_add_ (not the prefix sums JKGraph uses)"""
    one = torch.ones(src.shape[0], dtype=torch.float64, device=src.device)
    dinv = (1.0 + torch.zeros(n, dtype=torch.float64, device=src.device).index_add_(0, dst, one)).pow(-0.5)
    if not renormalize:
        return dinv, dinv * dinv
    d2 = 1.0 + dinv * torch.zeros(n, dtype=torch.float64, device=src.device).index_add_(0, dst, dinv[src])
    return dinv * d2.pow(-0.5), 1.0 / d2


def _case(name):
    """(n, JKGraph, src, dst, edge_index) of graph A, B, C (test_gpu_appnp.GRAPHS), A1 or A2 (test_gpu_gin._EXTRA); src / dst without
    the self loops; built once"""
    if name not in _CACHE:
        from bridged_gnn_amd.jknet import JKGraph
        cfg = GRAPHS.get(name) or _EXTRA[name]
        n, hub = cfg["n"], cfg["hub"]
        ei = _graph(n, cfg["e"], seed=cfg["seed"], hub=hub)
        keep = ei[0] != ei[1]
        assert not keep.all()                                                            # self loops to drop
        indeg, outdeg = np.bincount(ei[1][keep], minlength=n), np.bincount(ei[0][keep], minlength=n)
        assert (indeg == 0).any() and not np.array_equal(indeg, outdeg)                 # rows without in-edges; asymmetric
        pairs = ei[0] * n + ei[1]
        assert np.unique(pairs).shape[0] < pairs.shape[0]                                # duplicates
        if hub:
            assert indeg[3] >= hub and outdeg[5] >= hub
        eid = torch.from_numpy(ei).to(_dev())
        g = JKGraph(eid, n)
        assert g.csr.num_edges == int(keep.sum()) and int(g.col.shape[0]) == int(keep.sum())   # loops dropped, none appended
        src, dst = eid[0][eid[0] != eid[1]], eid[1][eid[0] != eid[1]]
        s64, w64 = _scales64(src, dst, n)
        torch.testing.assert_close(g.s.double(), s64, rtol=1.2e-7, atol=0)               # fp64, rounded once
        torch.testing.assert_close(g.w.double(), w64, rtol=1.2e-7, atol=0)
        _CACHE[name] = (n, g, src, dst, eid)
    return _CACHE[name]


def _conv64(T, src, dst, s, w):
    return w[:, None] * T + s[:, None] * torch.zeros_like(T).index_add_(0, dst, s[src][:, None] * T[src])


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
    bp = torch.zeros(ops.pad4(D), dtype=torch.float32, device=dev)
    bp[:D] = b.float()
    return T, bp


def _fwd(T, g, n, D, **kw):
    from bridged_gnn_amd import ops
    return ops.jk_gcn_aggregate(T, g.rowptr, g.col, g.s, g.w, n, D, **kw)


# ---- the kernels' summation orders, restated on the CPU ---------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _head32(J, W, b):
    """bgnn_jk.hip jk_head_kernel's product in fp32: per (row, class) four accumulators e = 0..3; step j adds, as one fma chain over
    kq = 0..3, the products at k = 16 j + 4 kq + e; z = ((a0 + a1) + (a2 + a3)) + bias"""
    n, K = J.shape
    acc = [np.zeros((n, W.shape[0]), np.float32) for _ in range(4)]
    for j in range(K // 16):
        for e in range(4):
            for kq in range(4):
                k = 16 * j + 4 * kq + e
                acc[e] = _fma32(J[:, k:k + 1], W[None, :, k], acc[e])
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + b[None, :]


def _walk32(rows, sc, U):
    """jk_agg_kernel's running sum of one sub-group in fp32: batches of U scaled rows (a product, then an fma chain), each batch
    entering by a compensated add"""
    acc = np.zeros(rows.shape[1], np.float32)
    cmp = np.zeros_like(acc)
    for k in range(0, rows.shape[0], U):
        b = sc[k] * rows[k]
        for u in range(k + 1, min(k + U, rows.shape[0])):
            b = _fma32(sc[u], rows[u], b)
        y = b - cmp
        t = acc + y
        cmp = (t - acc) - y
        acc = t
    return acc


def _hub_row32(T, cols, s, w, i, bias, EP, U):
    subs = [_walk32(T[cols[q::EP]], s[cols[q::EP]], U) for q in range(EP)]
    while len(subs) > 1:
        subs = [subs[k] + subs[k + 1] for k in range(0, len(subs), 2)]
    return _fma32(s[i], subs[0], w[i] * T[i]) + bias


def test_cpu_restatements_of_the_kernels_orders():
    """no GPU work: the shares of the activation bar the two longest sums take in fp32 in the kernels' own order"""
    rng = np.random.default_rng(90)
    K, C = 512, 32
    J = np.maximum(rng.standard_normal((64, K)), 0).astype(np.float32)                  # four layers of ReLU outputs
    bound = 1.0 / np.sqrt(K)
    W = rng.uniform(-bound, bound, (C, K)).astype(np.float32)                           # the Linear's own initialiser
    b = rng.uniform(-bound, bound, C).astype(np.float32)
    ref = J.astype(np.float64) @ W.astype(np.float64).T + b
    z = _head32(J, W, b)
    share = np.abs(z - ref).max() / (ACT_BAR * np.abs(ref).max() + 1e-6)
    print(f"head 512 x 32 restated in fp32 (split-K by 4): {share:.3f} of the bar")
    assert share <= 0.25
    # and ten times the scale of a trained layer's activations and weights
    z = _head32(10 * J, 3 * W, b)
    ref = (10 * J).astype(np.float64) @ (3 * W).astype(np.float64).T + b
    share = np.abs(z - ref).max() / (ACT_BAR * np.abs(ref).max() + 1e-6)
    print(f"head 512 x 32, larger operands: {share:.3f} of the bar")
    assert share <= 0.25


# ---- conv forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "A1"])
def test_conv_forward_every_width(name):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst, _ = _case(name)
    s, w = g.s.double(), g.w.double()
    rng = np.random.default_rng(91)
    worst = 0.0
    for D in DS:
        Dp = ops.pad4(D)
        T, bp = _inputs(rng, n, D, dev)
        what = f"graph {name} D={D}"
        agg = _conv64(T[:, :D].double(), src, dst, s, w)
        out = _fwd(T, g, n, D, bias=bp)
        worst = max(worst, _ok(out[:, :D], agg + bp[:D].double(), ACT_BAR, what))
        worst = max(worst, _ok(_fwd(T, g, n, D)[:, :D], agg, ACT_BAR, what + " no bias"))
        assert tuple(out.shape) == (n, Dp) and (Dp == D or torch.count_nonzero(out[:, D:]).item() == 0), what + ": pad columns"
        assert torch.equal(_fwd(T, g, n, D, bias=bp, epilogue="relu"), torch.relu(out)), what + ": relu epilogue"
        # tbl and out as views inside NaN-filled wider buffers: the same bits, nothing outside the view written, pad columns 0
        wide = torch.full((n, Dp + 8), float("nan"), device=dev)
        wide[:, 4:4 + D] = T[:, :D]
        obuf = torch.full((n, Dp + 12), float("nan"), device=dev)
        ov = obuf[:, 8:8 + Dp]
        ret = _fwd(wide[:, 4:4 + Dp], g, n, D, bias=bp, out=ov)
        assert ret.data_ptr() == ov.data_ptr() and torch.equal(ov, out), what + ": views"
        assert bool(torch.isnan(obuf[:, :8]).all()) and bool(torch.isnan(obuf[:, 8 + Dp:]).all()), what + ": written outside the view"
    print(f"graph {name}: worst conv forward error {worst:.3f} of the bar")


@pytest.mark.parametrize("name", ["A", "B"])
def test_conv_with_w_equal_s_squared_is_the_gcn_operator(name):
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gcn import GcnGraph
    from bridged_gnn_amd.jknet import JKGraph
    dev = _dev()
    n, _, src, dst, eid = _case(name)
    g1 = JKGraph(eid, n, renormalize=False)
    gg = GcnGraph(eid, n)
    torch.testing.assert_close(g1.w.double(), gg.dinv.double() ** 2, rtol=2.4e-7, atol=0)   # fp64 dinv^2 rounded once | fp32 dinv squared
    assert torch.equal(g1.s, gg.dinv), "renormalize=False must rebuild GcnGraph's dinv bit for bit"
    rng = np.random.default_rng(92)
    worst = 0.0
    for D in DS:
        T, bp = _inputs(rng, n, D, dev)
        bp = bp * 0.05                              # a small bias: about half of the pre-activations stay positive at every width
        what = f"graph {name} D={D}"
        a = ops.jk_gcn_aggregate(T, g1.rowptr, g1.col, g1.s, g1.w, n, D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED)
        b = ops.gcn_aggregate(T, gg.csr.rowptr, gg.col, gg.dinv, n, D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED, hubs=gg.hubs)
        worst = max(worst, _ok(a[:, :D], b[:, :D].double(), ACT_BAR, what + " against gcn_aggregate"))
        # the zero pattern: dropout's (the same hash, element index and seed) and the ReLU's; a pre-activation within rounding of 0
        # may take either side of the ReLU in the two summation orders, so those elements are left out
        z = _conv64(T[:, :D].double(), src, dst, g1.s.double(), g1.w.double()) + bp[:D].double()
        clear = z.abs() > 1e-4
        assert clear.float().mean().item() > 0.99
        assert torch.equal((a[:, :D] == 0)[clear], (b[:, :D] == 0)[clear]), what + ": zero patterns differ"
        assert 0.6 < (a[:, :D] == 0).float().mean().item() < 0.9
    print(f"graph {name}: worst difference to gcn_aggregate {worst:.3f} of the bar")


def test_conv_dropout_law_and_seeds():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst, _ = _case("A")
    rng = np.random.default_rng(93)
    for D, p in ((5, 0.5), (64, 0.3), (200, 0.5), (128, 0.8)):
        T, bp = _inputs(rng, n, D, dev)
        what = f"D={D} p={p}"
        y0 = _fwd(T, g, n, D, bias=bp, epilogue="relu")
        y = _fwd(T, g, n, D, bias=bp, epilogue="relu", p_drop=p, seed=SEED)
        pos = y0[:, :D] > 0
        kept = (y[:, :D] > 0) & pos
        npos, nkept = int(pos.sum()), int(kept.sum())
        # kept ~ Binomial(npos, 1 - p'), p' = p quantised to 16 bits: five standard deviations plus the quantisation
        assert abs(nkept - npos * (1 - p)) <= 5 * np.sqrt(npos * p * (1 - p)) + npos / 65536, what + f": kept {nkept} of {npos}"
        assert torch.count_nonzero(y[:, :D][~pos]).item() == 0
        ratio = (y[:, :D][kept].double() / y0[:, :D][kept].double())
        assert (ratio - 1 / (1 - p)).abs().max().item() <= (0.5 / 65536) / (1 - p) ** 2 * 1.01 + 1e-6, what + ": scale is not 1 / (1 - p)"
        # the mask `ops.feature_dropout` draws for an [n, D] tensor with the same seed: element index row * D + column
        m = ops.feature_dropout(torch.ones(n, D, device=dev), p, SEED)
        assert torch.equal(y[:, :D], y0[:, :D] * m), what + ": not the shared hash at row * D + column"
        assert torch.equal(_fwd(T, g, n, D, bias=bp, epilogue="relu", p_drop=p, seed=SEED), y), what + ": not reproducible"
        assert not torch.equal(_fwd(T, g, n, D, bias=bp, epilogue="relu", p_drop=p, seed=SEED + 1), y), what + ": two seeds, one mask"
        word = torch.tensor([1000], dtype=torch.int64, device=dev)
        assert torch.equal(_fwd(T, g, n, D, bias=bp, epilogue="relu", p_drop=p, seed=SEED - 1000, seed_dev=word), y), \
            what + ": seed + device word is the seed"
        if ops.pad4(D) > D:
            assert torch.count_nonzero(y[:, D:]).item() == 0


@pytest.mark.parametrize("D", [5, 128])
def test_conv_forward_past_the_persistent_cap(D):
    """graph C.  The row of 30 000 in-edges (node 3) is restated in fp32 on the CPU in the kernel's order before the GPU run."""
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst, _ = _case("C")
    # jk_agg_kernel: RPB = 4 * (64 / (LF * EP)) rows per tile; lf_ladder: (LF, EP, U) = (2, 4, 4) at D = 5 -> 32 rows, (32, 1, 8) at
    # D = 128 -> 8 rows; persistent_grid: at most 8 blocks per CU
    rpb, EP, U = {5: (32, 4, 4), 128: (8, 1, 8)}[D]
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-n // rpb) > cap, f"graph C must have more tiles of {rpb} rows than the {cap} blocks of a persistent grid"
    rng = np.random.default_rng([94, D])
    T, bp = _inputs(rng, n, D, dev)
    ref = _conv64(T[:, :D].double(), src, dst, g.s.double(), g.w.double()) + bp[:D].double()
    rowptr = g.rowptr.cpu().numpy()
    cols = g.col.cpu().numpy()[rowptr[3]:rowptr[4]]
    assert cols.shape[0] >= 30000
    cpu = _hub_row32(T[:, :D].cpu().numpy(), cols, g.s.cpu().numpy(), g.w.cpu().numpy(), 3, bp[:D].cpu().numpy(), EP, U)
    tol = ACT_BAR * ref.abs().max().item() + 1e-6
    cpu_share = np.abs(cpu.astype(np.float64) - ref[3].cpu().numpy()).max() / tol
    print(f"graph C D={D}: the 30 000-edge row restated in fp32 takes {cpu_share:.3f} of the bar")
    assert cpu_share <= 0.5
    out = _fwd(T, g, n, D, bias=bp)
    worst = _ok(out[:, :D], ref, ACT_BAR, f"graph C D={D}")
    hub = (out[3, :D].double() - ref[3]).abs().max().item() / tol
    if ops.pad4(D) > D:
        assert torch.count_nonzero(out[:, D:]).item() == 0
    print(f"graph C D={D}: worst conv forward error {worst:.3f} of the bar (the 30 000-edge row: {hub:.3f})")


def test_conv_ids_outside_the_table_add_nothing():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst, _ = _case("A")
    rng = np.random.default_rng(95)
    for D in (5, 64, 200):
        T, bp = _inputs(rng, n, D, dev)
        bad = g.col.clone()
        bad[::97] = n
        bad[5::101] = n + 12345
        bad[7::103] = -3
        ok = (bad >= 0) & (bad < n)
        csr_dst = torch.repeat_interleave(torch.arange(n, device=dev), (g.rowptr[1:n + 1] - g.rowptr[:n]).long())
        ref = _conv64(T[:, :D].double(), bad[ok].long(), csr_dst[ok], g.s.double(), g.w.double())
        out = ops.jk_gcn_aggregate(T, g.rowptr, bad, g.s, g.w, n, D)
        _ok(out[:, :D], ref, ACT_BAR, f"D={D}: ids outside the table add nothing")
    with pytest.raises(ValueError, match="epilogue"):
        _fwd(T, g, n, 200, epilogue="log_softmax")
    with pytest.raises(ValueError, match="distinct"):
        _fwd(T, g, n, 200, out=T)
    with pytest.raises(ValueError, match="s must be"):
        ops.jk_gcn_aggregate(T, g.rowptr, g.col, g.s[:n - 1], g.w, n, 200)


# ---- conv backward -----------------------------------------------------------------------------------------------
def _backward_cases(name, widths, seed):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst, _ = _case(name)
    s, w = g.s.double(), g.w.double()
    rng = np.random.default_rng(seed)
    worst = [0.0, 0.0]
    for D in widths:
        Dp = ops.pad4(D)
        for epi, p in ((None, 0.0), ("relu", 0.5)):
            T, bp = _inputs(rng, n, D, dev)
            what = f"graph {name} D={D} epi={epi}"
            # the forward's output as a slice of a wider buffer, as the model hands it over
            buf = torch.full((n, Dp + 8), float("nan"), device=dev)
            y = _fwd(T, g, n, D, bias=bp, epilogue=epi, p_drop=p, seed=SEED, out=buf[:, 4:4 + Dp])
            dy = torch.zeros(n, Dp, device=dev)
            dy[:, :D] = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
            gt, gb = ops.jk_gcn_aggregate_bwd(y, dy, g.t_rowptr, g.t_dst, g.s, g.w, n, D, epilogue=epi, p_drop=p)
            gt2, gb2 = ops.jk_gcn_aggregate_bwd(y, dy, g.t_rowptr, g.t_dst, g.s, g.w, n, D, epilogue=epi, p_drop=p)
            assert torch.equal(gt, gt2) and torch.equal(gb, gb2), what + ": two runs differ"
            assert tuple(gb.shape) == (D,) and tuple(gt.shape) == (n, Dp)
            assert ops.jk_gcn_aggregate_bwd(y, dy, g.t_rowptr, g.t_dst, g.s, g.w, n, D, epilogue=epi, p_drop=p, want_bias=False)[1] is None
            t64 = T[:, :D].double().requires_grad_(True)
            b64 = bp[:D].double().requires_grad_(True)
            pre = _conv64(t64, src, dst, s, w) + b64
            out = pre * (y[:, :D] > 0).double() / (1.0 - p) if epi == "relu" else pre       # the forward's own ReLU / dropout state
            rt, rb = torch.autograd.grad((out * dy[:, :D].double()).sum(), [t64, b64])
            worst[0] = max(worst[0], _ok(gt[:, :D], rt, GRAD_BAR, what + " grad_tbl"))
            worst[1] = max(worst[1], _ok(gb, rb, GRAD_BAR, what + " grad_bias"))
            if Dp > D:
                assert torch.count_nonzero(gt[:, D:]).item() == 0, what + ": pad columns must be 0"
    print(f"graph {name}: worst conv backward error {worst[0]:.3f} (grad_tbl), {worst[1]:.3f} (grad_bias) of the bar")


@pytest.mark.parametrize("name", ["A", "B"])
def test_conv_backward_matches_fp64_autograd_and_is_deterministic(name):
    _backward_cases(name, (1, 5, 31, 64, 128, 129, 200), 96)


def test_conv_backward_at_3001_rows():
    _backward_cases("A1", (5, 64, 200), 97)


def test_conv_backward_past_the_grid_caps():
    """graph A2 (20 000 nodes) at D = 128: more tiles of 8 rows than the persistent grid of pass B has blocks and more blocks' worth of
    rows than the 2048 blocks of the row pass"""
    n = _EXTRA["A2"]["n"]
    cap = max(8 * torch.cuda.get_device_properties(0).multi_processor_count, 2048)
    assert -(-n // 8) > cap
    _backward_cases("A2", (128,), 98)


# ---- the head ----------------------------------------------------------------------------------------------------
LS, HS, CS = (1, 2, 3, 4), (1, 3, 4, 5, 31, 32, 33, 64, 100, 128), (1, 2, 3, 5, 31, 32)


def _layers(rng, n, L, H, dev):
    """the layer buffer [n, L * pad4(H)] (pad columns 0) and the layers [n, L, H]: ReLU outputs (exact zeros in every layer: ties),
    rows whose last layer repeats the first (exact positive ties), rows that are 0 in every layer"""
    from bridged_gnn_amd import ops
    Hp = ops.pad4(H)
    x = torch.from_numpy(np.maximum(rng.standard_normal((n, L, H)), 0).astype(np.float32)).to(dev)
    x[::7, L - 1] = x[::7, 0]
    x[5::11] = 0
    buf = torch.zeros(n, L * Hp, device=dev)
    buf.view(n, L, Hp)[:, :, :H] = x
    return buf, x


def _head_params(rng, L, H, C, mode, dev):
    K = L * H if mode == "cat" else H
    W = torch.from_numpy((rng.standard_normal((C, K)) / np.sqrt(K)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(dev)
    return W, b


def _jump64(x, mode, win=None):
    """[n, L, H] fp64 -> the jumped rows; max mode with `win` [n, H]: the given winners' elements"""
    n, L, H = x.shape
    if mode == "cat":
        return x.reshape(n, L * H)
    if win is None:
        return x.max(1)[0]
    return torch.gather(x, 1, win.long().unsqueeze(1)).squeeze(1)


def _head_forward_cases(n, mode, combos, seed):
    from bridged_gnn_amd import ops
    dev = _dev()
    rng = np.random.default_rng(seed)
    worst = 0.0
    for L, H, C in combos:
        Hp, Cp = ops.pad4(H), ops.pad4(C)
        assert ops.jk_head_supported(L, H, C, mode)
        buf, x = _layers(rng, n, L, H, dev)
        W, b = _head_params(rng, L, H, C, mode, dev)
        wp = ops.jk_pack_weight(W, L, H, mode)
        what = f"n={n} {mode} L={L} H={H} C={C}"
        z = _jump64(x.double(), mode) @ W.double().t() + b.double()
        out, win, jump = ops.jk_head(buf, L, H, mode, wp, b, C, log_softmax=True, want_state=True)
        worst = max(worst, _ok(out[:, :C], torch.log_softmax(z, 1), ACT_BAR, what + " log_softmax"))
        raw = ops.jk_head(buf, L, H, mode, wp, b, C, log_softmax=False)
        worst = max(worst, _ok(raw[:, :C], z, ACT_BAR, what + " logits"))
        worst = max(worst, _ok(ops.jk_head(buf, L, H, mode, wp, None, C, log_softmax=False)[:, :C], z - b.double(), ACT_BAR,
                               what + " no bias"))
        assert tuple(out.shape) == (n, Cp) and (Cp == C or torch.count_nonzero(out[:, C:]).item() == 0), what + ": pad columns"
        assert Cp == C or torch.count_nonzero(raw[:, C:]).item() == 0
        assert torch.equal(ops.jk_head(buf, L, H, mode, wp, b, C), out), what + ": the evaluation call differs"
        if mode == "cat":
            assert win is None and jump is None
        else:
            # torch's winners: the maximum's first (lowest) layer -- unique maxima and exact ties alike (fp32 inputs: exact)
            mx = x.max(1)[0]
            first = (x == mx.unsqueeze(1)).to(torch.uint8).argmax(1)
            assert win.dtype == torch.uint8 and tuple(win.shape) == (n, Hp)
            assert torch.equal(win[:, :H].long(), first), what + ": winners"
            assert torch.equal(jump[:, :H], mx) and torch.count_nonzero(jump[:, H:]).item() == 0, what + ": jumped rows"
            assert torch.count_nonzero(win[:, H:]).item() == 0
            if L > 1:
                ties = (x == mx.unsqueeze(1)).sum(1) > 1
                assert bool(ties.any()) and bool((mx[ties] > 0).any())                  # zero ties and positive ties were there
    print(f"head forward n={n} {mode}: worst error {worst:.3f} of the bar")


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("mode", ["cat", "max"])
def test_head_forward_every_shape(mode, L):
    _head_forward_cases(3001, mode, [(L, H, C) for H in HS for C in CS], 100 + L)


@pytest.mark.parametrize("mode", ["cat", "max"])
def test_head_forward_past_the_persistent_cap(mode):
    n = 70000
    # bgnn_jk.hip launch_head: a tile is 64 rows; W of the widest shape takes 64 KB of a CU's 160 KB of LDS, so two blocks stay
    # resident on a CU and the grid is capped there
    from bridged_gnn_amd import ops
    cap = (160 * 1024 // ops.JK_HEAD_LDS_BYTES) * torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-n // 64) > cap, f"(4, 128, 32): more tiles of 64 rows than the {cap} blocks of its persistent grid"
    _head_forward_cases(n, mode, [(2, 64, 2), (3, 33, 31), (4, 128, 32)], 110)


def test_head_outside_its_envelope_is_composed_by_the_module():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.jknet import JKNet
    dev = _dev()
    assert not ops.jk_head_supported(2, 16, 33, "cat") and not ops.jk_head_supported(2, 16, 33, "max")
    with pytest.raises(ValueError, match="envelope"):
        ops.jk_head(torch.zeros(8, 32, device=dev), 2, 16, "cat", torch.zeros(33, 32, device=dev), None, 33)
    d = load_golden("jknet_small.npz")
    n = d["x"].shape[0]
    ei = torch.from_numpy(d["edge_index"]).long()
    A = operator(mult_adj(ei, n))[0]
    data = Data(x=torch.from_numpy(d["x"]).to(dev), edge_index=ei.to(dev))
    for mode in ("cat", "max"):
        torch.manual_seed(5)
        m = JKNet(d["x"].shape[1], 16, 33, 2, 0.5, mode=mode).to(dev).eval()
        P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}
        ref = restate(P, torch.from_numpy(d["x"]).double(), A, mode)
        with torch.no_grad():
            _bar_ok(m(data).cpu(), ref.detach().numpy(), ACT_BAR, f"C=33 {mode} composed head")
        out = m(data)
        dy = torch.from_numpy(np.random.default_rng(6).standard_normal((n, 33)).astype(np.float32))
        (out * dy.to(dev)).sum().backward()
        rg = torch.autograd.grad((ref * dy.double()).sum(), list(P.values()))
        for (k, prm), r in zip(m.named_parameters(), [rg[list(P).index(k)] for k, _ in m.named_parameters()]):
            _bar_ok(prm.grad.cpu(), r.numpy(), GRAD_BAR, f"C=33 {mode} grad {k}")


@pytest.mark.parametrize("mode", ["cat", "max"])
def test_head_backward_matches_fp64_autograd(mode):
    from bridged_gnn_amd import ops
    dev = _dev()
    n = 3001
    rng = np.random.default_rng(120)
    worst = [0.0, 0.0, 0.0]
    for L, H, C in ((1, 5, 3), (2, 64, 2), (3, 33, 31), (4, 128, 32), (2, 100, 5), (3, 32, 16), (4, 3, 1)):
        Hp, Cp = ops.pad4(H), ops.pad4(C)
        for lsm in (True, False):
            buf, x = _layers(rng, n, L, H, dev)
            W, b = _head_params(rng, L, H, C, mode, dev)
            wp = ops.jk_pack_weight(W, L, H, mode)
            what = f"{mode} L={L} H={H} C={C} log_softmax={lsm}"
            out, win, jump = ops.jk_head(buf, L, H, mode, wp, b, C, log_softmax=lsm, want_state=True)
            dy = torch.zeros(n, Cp, device=dev)
            dy[:, :C] = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).to(dev)
            gx, gwp, gb = ops.jk_head_bwd(buf, L, H, mode, wp, C, out, dy, log_softmax=lsm, win=win, jump=jump)
            gx2, gwp2, gb2 = ops.jk_head_bwd(buf, L, H, mode, wp, C, out, dy, log_softmax=lsm, win=win, jump=jump)
            assert torch.equal(gx, gx2) and torch.equal(gb, gb2), what + ": two runs differ"
            x64 = x.double().requires_grad_(True)
            W64, b64 = W.double().requires_grad_(True), b.double().requires_grad_(True)
            # the winners are the GPU forward's own uint8 state: the backward's contract
            z = _jump64(x64, mode, None if mode == "cat" else win[:, :H]) @ W64.t() + b64
            o = torch.log_softmax(z, 1) if lsm else z
            rx, rw, rb = torch.autograd.grad((o * dy[:, :C].double()).sum(), [x64, W64, b64])
            nl = L if mode == "cat" else 1
            gw = gwp.reshape(C, nl, Hp)[:, :, :H].reshape(C, nl * H)
            g3 = gx.view(n, L, Hp)
            worst[0] = max(worst[0], _ok(g3[:, :, :H], rx, GRAD_BAR, what + " grad_x"))
            worst[1] = max(worst[1], _ok(gw, rw, GRAD_BAR, what + " grad_weight"))
            worst[2] = max(worst[2], _ok(gb, rb, GRAD_BAR, what + " grad_bias"))
            assert Hp == H or torch.count_nonzero(g3[:, :, H:]).item() == 0, what + ": pad columns of grad_x"
            assert Hp == H or torch.count_nonzero(gwp.reshape(C, nl, Hp)[:, :, H:]).item() == 0
            if mode == "max":                       # a slice gets dJ where it won and 0 elsewhere
                lost = win[:, :H].long().unsqueeze(1) != torch.arange(L, device=dev).view(1, L, 1)
                assert torch.count_nonzero(g3[:, :, :H][lost]).item() == 0, what + ": a losing slice got a gradient"
    print(f"head backward {mode}: worst error {worst[0]:.3f} (grad_x), {worst[1]:.3f} (grad_weight), {worst[2]:.3f} (grad_bias) of the bar")


# ---- model level -------------------------------------------------------------------------------------------------
def _fixture_case(variant):
    from bridged_gnn_amd.data import Data
    dev = _dev()
    g, fx = load_golden("office_a2d_graph.npz"), load_golden("jknet_office_a2d.npz")
    data = Data(x=torch.from_numpy(g["x"]).to(dev), edge_index=torch.from_numpy(g["edge_index"]).long().to(dev),
                y=torch.from_numpy(g["y"]).long().to(dev))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(fx["train_mask"]).to(dev)          # the driver's mask (y == -1 cleared, :404)
    return data, tm, g["x"].shape[1], int(g["y"].max()) + 1, fx


def _model(F_in, C, fx, name, mode, L, hidden, dropout=0.5):
    """the fixture's model: torch.manual_seed(0), checked against the stored parameter sums"""
    from bridged_gnn_amd.jknet import JKNet
    torch.manual_seed(0)
    m = JKNet(F_in, hidden, C, L, dropout, mode=mode)
    sums = sub(fx, f"{name}/param_sum/")
    assert sorted(sums) == sorted(m.state_dict())
    for k, v in m.state_dict().items():
        vd = v.double()
        np.testing.assert_allclose([vd.sum().item(), (vd * vd).sum().item()], sums[k], rtol=1e-12, atol=1e-300, err_msg=k)
    return m.to(_dev())


@pytest.mark.parametrize("variant", ["raw", "und"])
def test_model_matches_the_reference_fixture(variant):
    data, tm, F_in, C, fx = _fixture_case(variant)
    rows = torch.from_numpy(fx["rows"])
    x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
    A = operator(mult_adj(data.edge_index.cpu(), x64.shape[0]))[0]
    worst = [0.0, 0.0]
    for name, mode, L, hidden, _ in OFFICE_MODELS:
        m = _model(F_in, C, fx, name, mode, L, hidden).eval()
        P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}
        names = [k for k, _ in m.named_parameters()]
        pre = f"{variant}/{name}/"
        assert fx[pre + "flipped"].size == 0                       # the fp32 reference met GRAD_BAR on every tensor: so must the model
        with torch.no_grad():
            lp = m(data).cpu()
        _bar_ok(lp[rows], fx[pre + "logp"], ACT_BAR, pre + "logp")                              # the reference, at the fixture's rows
        ref_lp = restate(P, x64, A, mode)
        _bar_ok(lp, ref_lp.detach().numpy(), ACT_BAR, pre + "logp (every row, fp64 restatement)")
        worst[0] = max(worst[0], _share(lp, ref_lp.detach(), ACT_BAR))
        if sub(fx, pre + "grad/"):
            ref = {k: fx[pre + "grad/" + k] for k in names}
        else:                                                      # the fp64 restatement test_jknet_host.py pins to the fixture
            rl = F.nll_loss(ref_lp[tmc], y[tmc])
            ref = {k: gr.numpy() for k, gr in zip(names, torch.autograd.grad(rl, [P[k] for k in names]))}
        out = m(data)                                                                             # the autograd path, eval mode
        _bar_ok(out.detach().cpu()[rows], fx[pre + "logp"], ACT_BAR, pre + "logp (autograd path)")
        loss = F.nll_loss(out[tm], data.y[tm])
        assert abs(loss.item() - float(fx[pre + "loss"])) <= 1e-5 * abs(float(fx[pre + "loss"]))
        loss.backward()
        for k, prm in m.named_parameters():
            _bar_ok(prm.grad.double().cpu().numpy(), ref[k], GRAD_BAR, f"{pre}grad {k}")
            worst[1] = max(worst[1], np.abs(prm.grad.double().cpu().numpy() - ref[k]).max() / (GRAD_BAR * np.abs(ref[k]).max() + 1e-6))
    print(f"JKNet {variant}: worst error {worst[0]:.3f} (logp), {worst[1]:.3f} (gradients) of the bar")


def test_adam_losses_match_the_reference_fixture():
    for variant in ("raw", "und"):
        data, tm, F_in, C, fx = _fixture_case(variant)
        for name, mode, L, hidden, _ in OFFICE_MODELS:
            m = _model(F_in, C, fx, name, mode, L, hidden, dropout=0.0).train()
            pre = f"{variant}/{name}/"
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
                if pre + "adam/" + k in fx:
                    _bar_ok(prm.detach().cpu(), fx[pre + "adam/" + k], 1e-4, pre + "adam/" + k)


def test_small_fixture_models_and_the_single_normalisation():
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.jknet import JKNet
    dev = _dev()
    d = load_golden("jknet_small.npz")
    data = Data(x=torch.from_numpy(d["x"]).to(dev), edge_index=torch.from_numpy(d["edge_index"]).long().to(dev),
                y=torch.from_numpy(d["y"]).long().to(dev))
    tm = torch.from_numpy(d["train_mask"]).to(dev)
    assert any(not r for *_, r in SMALL_MODELS)
    for name, mode, L, hidden, renorm in SMALL_MODELS:
        m = JKNet(d["x"].shape[1], hidden, int(d["y"].max()) + 1, L, 0.5, mode=mode, renormalize=renorm)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sub(d, f"{name}/param/").items()})
        m = m.to(dev).eval()
        pre = f"raw/{name}/"
        out = m(data)
        _bar_ok(out.detach().cpu(), d[pre + "logp"], ACT_BAR, pre + "logp")
        F.nll_loss(out[tm], data.y[tm]).backward()
        for k, prm in m.named_parameters():
            _bar_ok(prm.grad.cpu(), d[pre + "grad/" + k], GRAD_BAR, f"{pre}grad {k}")
        # training mode: num_layers dropout sites, zeros in every slice, finite log-probabilities
        m.train()
        torch.manual_seed(1)
        a = m(data)
        torch.manual_seed(1)
        b = m(data)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and not torch.equal(a, out)


# ---- driver ------------------------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(dataset_name="office")


def _run(data, hist, **kw):
    from bridged_gnn_amd import jknet, transfer
    cfg = dict(repeat=1, num_epoch=8, use_scheduler=False, seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)
    cfg.update(kw)
    return jknet.train_jknet_noDTC(ARGS, transfer.pyg_dataset(data), data, history=hist, **cfg)


def test_driver_loss_falls_runs_are_seeded_and_the_checkpoint_loads_back(tmp_path):
    from bridged_gnn_amd import jknet, transfer
    from test_gpu_appnp import _office_data
    data = _office_data()
    h0, h1, h2 = {}, {}, {}
    assert _run(data, h0, dropout=0.0, num_layer=3, mode="max") is None
    assert len(h0["loss_train"]) == 8 and len(h0["eval_res"]) == 8 and all(len(r) == 3 for r in h0["eval_res"])
    print("JKNet driver losses", h0["loss_train"])
    assert all(np.isfinite(h0["loss_train"])) and h0["loss_train"][-1] < h0["loss_train"][0]
    assert _run(data, h1, save=True, ckpt_dir=str(tmp_path)) is None and _run(data, h2) is None
    assert all(np.isfinite(h1["loss_train"])) and all(np.isfinite(np.asarray(h1["eval_res"], dtype=np.float64)).ravel())
    assert h1["loss_train"][-1] < h1["loss_train"][0]
    assert h1["loss_train"] == h2["loss_train"] and h1["eval_res"] == h2["eval_res"]        # the host generator's seeds, no atomics
    path = os.path.join(str(tmp_path), "model_JKNet_office_share_best.ckpt")
    assert os.path.exists(path)
    ds = transfer.pyg_dataset(data)
    m = jknet.JKNet(ds.num_features, 64, ds.num_classes, 2, 0.5).to(_dev())
    m.load_state_dict(torch.load(path, map_location=_dev()), strict=True)
    assert transfer.test_noDTC(data, m) == h1["eval_res"][h1["best_epoch"]]
    with pytest.raises(NotImplementedError, match="graphed"):
        _run(data, {}, graphed=True)


def test_main_runs_from_a_saved_bridged_graph(tmp_path, capsys):
    from bridged_gnn_amd import jknet
    from bridged_gnn_amd.data import Data, save_bridged_graph
    og = load_golden("office_a2d_graph.npz")
    d = Data(x=torch.from_numpy(og["x"]), edge_index=torch.from_numpy(og["edge_index"]).long(), y=torch.from_numpy(og["y"]).long(),
             **{k: torch.from_numpy(og[k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    path = str(tmp_path / "office_amazon2dslr_bridged_graph.dat")
    save_bridged_graph(d, path)
    res = jknet.main(["--num_layer", "3", "--hidden_dim", "32", "--num_epoch", "3", "--dataset_name", "office_amazon2dslr", "--path_data",
                      path, "--to_undirected", "--dropout", "0.2", "--mode", "max"])
    out = capsys.readouterr().out
    assert res is None
    assert out.count("Epoch: 00") == 3 and "[Run-1 score]" in out and "JKNet" in out and "nan" not in out.lower()
