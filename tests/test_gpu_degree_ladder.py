"""GPU: every row-walking kernel on the exact degree edges of its edge loop.

One deterministic bipartite multigraph (tests/degree_ladder.py) whose by-destination AND by-source views hold every degree at
which a loop over batches of EP * U slots can go wrong -- 0, fewer edges than sub-groups, k * batch - 1, k * batch, k * batch + 1
for the batches of 4, 8, 16 and 32 slots and k = 1, 2, 3 -- at every lane-group position of a wave, with a ragged last tile.
Every kernel runs over it forward (by destination) and backward (by source) at one width per rung of lf_ladder, 3, 7, 12, 31, 64,
100, and at 132 (a second column slice) where the op takes it.  Each test first asserts, on the CPU, that the view its kernel
walks holds every ladder degree at every position of that width's mapping, and prints the degrees it saw.

Exact layer: integer-valued fp32 features in [-8, 8] under unit coefficients -- every partial sum is an integer below 2^24 in any
order -- against the int64 sums of the same CSR with torch.equal: GIN at eps = 0, JKNet's conv at s = w = 1, GCN and one APPNP
step at dinv = 1, the plain-sum SAGE entry, rows_segment_add, and the gather pass of each of their backwards.  For the attention
kernels: under zero attention vectors every logit is 0, so the softmax denominator a row's state holds is its degree exactly,
the rows whose degree is a power of two (1 / deg and every product exact) carry exact sums, and the GAT backward's by-source
gather under coefficients of all ones is an integer sum again.
fp64 layer: random fp32 inputs against the fp64 restatements of tests/degree_ladder.py (pinned to dense formulations by
tests/test_degree_ladder_host.py) from the same inputs and the same CSR.  The bars are the families' own, 1e-5 for activations and
2e-5 for gradients (ACT_BAR / GRAD_BAR of tests/test_gpu_gcn.py, which every step-2 family's GPU file imports or restates;
conftest.assert_close's 1e-5 and tests/test_gpu_pull_wide.py's 2e-5 for AdaptedConv), applied ROW BY ROW: a row's scale is the
largest column of its fp64 sum of |coefficient * value|, never the tensor's maximum, so a dropped or doubled edge of a short row
is not hidden behind a long one.
AdaptedConv runs twice: the whole-graph call (agg_wide_fast_kernel at D > 32) and a first-part call that parks no row, which the
fast plan refuses (agg_wide_kernel).  DeeperGCN's grad_t is held to GRAD_BAR on the fp64 sum of its edges' absolute terms, its lse
to ACT_BAR on max_j |t v_j| + log(deg) of the row itself.
Every output buffer that the op lets the caller hand in starts as NaN inside a wider NaN buffer: the rows end finite, the pad
columns 0, everything around them NaN; two calls give equal bits.  Each test prints its worst row: degree and share of the bar."""
import numpy as np
import pytest
import torch

import degree_ladder as dl
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _dev

pytestmark = pytest.mark.gpu

WIDTHS = dl.WIDTHS + (dl.WIDE,)
NARROW = dl.WIDTHS                       # the ops that stop at 128 columns
SLOPE = 0.2
_CACHE = {}


# ---- the graph on the device, as each family's own graph class hands it to the kernel ------------------------------------------------
def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t if dtype is None else t.to(dtype)


def _case(family):
    """family -> dict: the Ladder, the graph object, the walked views on the device and, for the restatements, on the CPU"""
    if family in _CACHE:
        return _CACHE[family]
    from bridged_gnn_amd import ops
    variant = {"sage": "plain", "jk": "loops_dropped", "gcn": "loops_rewritten", "gat": "loops_rewritten", "adapted": "loops_rewritten"}[family]
    lad = dl.Ladder(variant)
    ei = _t(lad.ei)
    c = dict(lad=lad, N=lad.N, n=lad.n)
    if family == "sage":
        from bridged_gnn_amd.sage import SageGraph
        g = SageGraph(ei, lad.N)
        c["rowptr"], c["col"], c["t_rowptr"], c["t_dst"] = g.by_dst
    elif family == "jk":
        from bridged_gnn_amd.jknet import JKGraph
        g = JKGraph(ei, lad.N)
        c["rowptr"], c["col"], c["t_rowptr"], c["t_dst"] = g.rowptr, g.col, g.t_rowptr, g.t_dst
    elif family == "gcn":
        from bridged_gnn_amd.gcn import GcnGraph
        g = GcnGraph(ei, lad.N)
        c["rowptr"], c["col"], c["t_rowptr"], c["t_dst"] = g.csr.rowptr, g.col, g.t_rowptr, g.t_dst
    elif family == "gat":
        from bridged_gnn_amd.gat import GatGraph
        g = GatGraph(ei, lad.N)
        c["rowptr"], c["col"], c["t_rowptr"], c["t_dst"], c["t_eid"] = g.rowptr, g.col, g.t_rowptr, g.t_dst, g.t_eid
    else:
        g = ops.build_dst_csr(ei, lad.N)                                      # KTGNN._prepare: the loops rewritten
        c["rowptr"], c["col"] = g.rowptr, g.col[: g.num_edges]
        c["t_rowptr"], _, c["t_dst"] = g.transposed()
    c["g"] = g
    for k in ("rowptr", "col", "t_rowptr", "t_dst"):
        c[k + "_h"] = c[k].cpu().long().numpy()
    # the graph class kept exactly the edges the CPU restatement of its rule keeps, in its order
    src, dst = lad.walked()
    rp, col = dl.csr_by(dst, src, lad.N)
    assert np.array_equal(c["rowptr_h"], rp) and np.array_equal(c["col_h"], col), f"{family}: the graph class's CSR is not the restated one"
    t_rp, t_col = dl.csr_by(src, dst, lad.N)
    assert np.array_equal(c["t_rowptr_h"], t_rp) and np.array_equal(c["t_dst_h"], t_col), f"{family}: by-source view"
    assert lad.duplicates() > 0
    c["deg"] = rp[1:] - rp[:-1]
    c["t_deg"] = t_rp[1:] - t_rp[:-1]
    _CACHE[family] = c
    return c


def _cover(c, D, what, table=dl.LF_LADDER, views=("rowptr_h", "t_rowptr_h"), heads=1, u_caps=()):
    """the condition on the inputs, before any launch: the restated table is the one the ladder was built for, and the walked
    views hold every ladder degree at every lane-group position of this width's mapping.  A width past 128 runs as column
    slices, each at its own rung: the slice of 128 columns and the tail slice are both checked.  heads: the attention kernels
    give a lane group the virtual row i * heads + h.  u_caps: the depths at which a kernel of the family runs the rung's EP
    instead of the table's U (GAT_EDGE_U, GEN_BWD_U_CAP): those batch sizes are asserted and printed too."""
    dl.assert_batches_bracketed(c["lad"].degrees + [0], what)
    for W in ([D] if D <= 128 else [128, D - 128]):
        LF, EP, U = dl.rung(W, table)
        batches = [EP * U] + [EP * min(U, cap) for cap in u_caps]
        assert all(b in dl.BATCHES for b in batches) and (EP == 1 or EP in dl.SUBGROUPS), (W, LF, EP, U, batches)
        rpw = 64 // (LF * EP)
        assert rpw <= dl.POSITIONS
        seen = [dl.assert_coverage(c[v], c["lad"].degrees, rpw, f"{what} D={D} slice of {W} columns {v}", heads=heads) for v in views]
        print(f"{what} D={D}, slice of {W} columns: (LF, EP, U) = ({LF}, {EP}, {U}), {rpw} rows per wave, batches {batches}, {heads} "
              f"head(s); degrees walked by destination {seen[0]}" + (f", by source {seen[1]}" if len(seen) > 1 else ""))


# ---- inputs and buffers ---------------------------------------------------------------------------------------------------------------
def _ints(rng, rows, D):
    """integer-valued fp32 in [-8, 8], [rows, pad4(D)] with zero pad columns (CPU)"""
    Dp = (D + 3) // 4 * 4
    x = torch.zeros(rows, Dp)
    x[:, :D] = torch.from_numpy(rng.integers(-8, 9, size=(rows, D)).astype(np.float32))
    return x


def _randn(rng, rows, D, scale=1.0):
    Dp = (D + 3) // 4 * 4
    x = torch.zeros(rows, Dp)
    x[:, :D] = torch.from_numpy((rng.standard_normal((rows, D)) * scale).astype(np.float32))
    return x


def _nan_view(rows, D, extra_rows=3):
    """-> (big, view): a [rows, pad4(D)] view (16-byte aligned, row stride a multiple of 4) inside a wider and longer NaN buffer"""
    Dp = (D + 3) // 4 * 4
    big = torch.full((rows + extra_rows, Dp + 8), float("nan"), device=_dev())
    return big, big[:rows, 4:4 + Dp]


def _untouched(big, rows, D, what):
    """the view's rows finite, its pad columns 0, everything around it still NaN"""
    Dp = (D + 3) // 4 * 4
    v = big[:rows, 4:4 + Dp]
    assert bool(torch.isfinite(v).all()), f"{what}: a row of the range was left unwritten or non-finite"
    if Dp > D:
        assert torch.count_nonzero(v[:, D:]).item() == 0, f"{what}: pad columns must be 0"
    assert bool(torch.isnan(big[rows:]).all()) and bool(torch.isnan(big[:, :4]).all()) and bool(torch.isnan(big[:, 4 + Dp:]).all()), \
        f"{what}: memory outside the output rows was written"


def _int_walk(rowptr, col, X):
    """int64 sums of the CSR's rows over an integer-valued table"""
    dst, src = dl._edges(rowptr, col)
    Xi = X.long()
    return torch.zeros(len(rowptr) - 1, X.shape[1], dtype=torch.int64).index_add(0, dst, Xi[src])


def _exact(got, want_i64, D, what):
    assert torch.equal(got[:, :D].cpu().double(), want_i64[:, :D].double()), \
        f"{what}: rows {torch.nonzero((got[:, :D].cpu().double() != want_i64[:, :D].double()).any(1)).reshape(-1).tolist()[:12]} are not the integer sums"


def _twice(fn, what):
    """fn() -> (big, view); two calls, equal bits -> the first call's pair"""
    b1, v1 = fn()
    b2, v2 = fn()
    assert torch.equal(v1, v2), f"{what}: two calls differ"
    return b1, v1


def _report(what, shares):
    w = max(shares, key=lambda s: s[0])
    print(f"{what}: worst row has degree {w[1]} at {w[0]:.3f} of the bar")


# ---- SAGE --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_sage(D):
    from bridged_gnn_amd import ops
    c = _case("sage")
    _cover(c, D, "sage")
    N, dev = c["N"], _dev()
    rng = np.random.default_rng(100 + D)
    shares = []
    # exact: the plain sum with an integer root
    Ti, Ri = _ints(rng, N, D), _ints(rng, N, D)

    def run_sum():
        big, out = _nan_view(N, D)
        ops.sage_mean_aggregate(Ti.to(dev), c["rowptr"], c["col"], N, D, root=Ri.to(dev), mean=False, out=out)
        return big, out
    big, out = _twice(run_sum, f"sage D={D} sum")
    _untouched(big, N, D, f"sage D={D} sum")
    _exact(out, _int_walk(c["rowptr_h"], c["col_h"], Ti) + Ri.long(), D, f"sage D={D} plain sum")
    # fp64: the mean with a root, forward and backward
    T, R, gy = _randn(rng, N, D), _randn(rng, N, D), _randn(rng, N, D)

    def run_mean():
        big, out = _nan_view(N, D)
        ops.sage_mean_aggregate(T.to(dev), c["rowptr"], c["col"], N, D, root=R.to(dev), out=out)
        return big, out
    big, out = _twice(run_mean, f"sage D={D} mean")
    _untouched(big, N, D, f"sage D={D} mean")
    ref, sc = dl.sage_ref(c["rowptr_h"], c["col_h"], T[:, :D], R[:, :D])
    shares.append(dl.judge(out[:, :D], ref, sc, ACT_BAR, c["deg"], f"sage D={D} forward"))

    def run_bwd():
        bt, gt = _nan_view(N, D)
        br, gr = _nan_view(N, D)
        ops.sage_mean_aggregate_bwd(None, gy.to(dev), c["rowptr"], c["t_rowptr"], c["t_dst"], N, D, grad_tbl=gt, grad_root=gr)
        assert torch.equal(gr[:, :D].cpu(), gy[:, :D]), "grad_root is grad_y"
        _untouched(br, N, D, f"sage D={D} grad_root")
        return bt, gt
    bt, gt = _twice(run_bwd, f"sage D={D} backward")
    _untouched(bt, N, D, f"sage D={D} grad_tbl")
    deg = torch.from_numpy(c["deg"]).double()
    ref, sc = dl.walk(c["t_rowptr_h"], c["t_dst_h"], gy[:, :D].double() / deg.clamp(min=1)[:, None])     # (no edge leaves a row of degree 0)
    shares.append(dl.judge(gt[:, :D], ref, sc, GRAD_BAR, c["t_deg"], f"sage D={D} grad_tbl"))
    _report(f"sage D={D}", shares)


# ---- rows_segment_add ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_rows_segment_add(D):
    """segment lengths = the by-destination view's ladder rows; the written rows are a permutation's image, the rest untouched"""
    from bridged_gnn_amd import ops
    c = _case("sage")
    _cover(c, D, "rows_segment_add", views=("rowptr_h",))
    N, dev = c["N"], _dev()
    rng = np.random.default_rng(200 + D)
    n_dst = N + 37
    row = rng.permutation(n_dst)[:N].astype(np.int32)
    seg_ptr, idx, rowt = c["rowptr"], c["col"], _t(row)
    rest = torch.from_numpy(np.setdiff1d(np.arange(n_dst), row))
    ri = torch.from_numpy(row.astype(np.int64))
    shares = []
    for acc in (True, False):
        for exact in (True, False):
            src = (_ints if exact else _randn)(rng, N, D)
            d0 = (_ints if exact else _randn)(rng, n_dst, D)
            d0[rest] = float("nan")                                            # rows no segment names stay as they are
            outs = []
            for _ in range(2):
                big = torch.full((n_dst, d0.shape[1] + 8), float("nan"), device=dev)
                dst = big[:, 4:4 + d0.shape[1]]
                dst.copy_(d0)
                ops.rows_segment_add(src.to(dev), seg_ptr, idx, rowt, dst, D=D, accumulate=acc)
                outs.append(dst)
            what = f"rows_segment_add D={D} accumulate={acc} exact={exact}"
            assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), what + ": two calls differ"   # (bits: NaN rows)
            got = outs[0].cpu()
            assert bool(torch.isnan(got[rest]).all()) and bool(torch.isnan(big[:, :4]).all()) and bool(torch.isnan(big[:, 4 + d0.shape[1]:]).all()), what
            assert bool(torch.isfinite(got[ri]).all()), what
            assert torch.count_nonzero(got[row.astype(np.int64), D:]).item() == 0, what + ": pad columns"
            base = d0[ri] if acc else torch.zeros(N, d0.shape[1])
            if exact:
                _exact(got[ri], _int_walk(c["rowptr_h"], c["col_h"], src) + base.long(), D, what)
            else:
                S, A = dl.walk(c["rowptr_h"], c["col_h"], src[:, :D])
                shares.append(dl.judge(got[row.astype(np.int64), :D], S + base[:, :D].double(), A + base[:, :D].double().abs(), ACT_BAR, c["deg"], what))
    _report(f"rows_segment_add D={D}", shares)


# ---- GCN ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_gcn(D):
    from bridged_gnn_amd import ops
    c = _case("gcn")
    _cover(c, D, "gcn")
    g, N, dev = c["g"], c["N"], _dev()
    # no ladder row reaches the hub threshold: with the graph's own hub tables or without any, the plain walk runs
    assert c["deg"].max() < ops.GCN_HUB_THRESHOLD and c["t_deg"].max() < ops.GCN_HUB_THRESHOLD
    assert g.hubs is None and g.t_hubs is None and g.csr.hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT) is None
    rng = np.random.default_rng(300 + D)
    ones = torch.ones(N, device=dev)
    shares = []
    for exact in (True, False):
        T, gy = (_ints if exact else _randn)(rng, N, D), (_ints if exact else _randn)(rng, N, D)
        dinv = ones if exact else g.dinv
        what = f"gcn D={D} exact={exact}"

        def fwd(hubs="graph"):
            big, out = _nan_view(N, D)
            ops.gcn_aggregate(T.to(dev), c["rowptr"], c["col"], dinv, N, D, out=out, **({"hubs": g.hubs} if hubs == "graph" else {}))
            return big, out
        big, out = _twice(fwd, what)
        _untouched(big, N, D, what)
        assert torch.equal(out, fwd(hubs=None)[1]), what + ": with and without the hub tables"

        def bwd():
            big, gt = _nan_view(N, D)
            ops.gcn_aggregate_bwd(None, gy.to(dev), c["t_rowptr"], c["t_dst"], dinv, N, D, want_bias=False, grad_tbl=gt, hubs=g.t_hubs)
            return big, gt
        bb, gt = _twice(bwd, what + " backward")
        _untouched(bb, N, D, what + " backward")
        if exact:
            _exact(out, _int_walk(c["rowptr_h"], c["col_h"], T), D, what + " forward")
            _exact(gt, _int_walk(c["t_rowptr_h"], c["t_dst_h"], gy), D, what + " backward")
        else:
            dv = g.dinv.cpu()
            ref, sc = dl.scaled_ref(c["rowptr_h"], c["col_h"], T[:, :D], dv, dv)
            shares.append(dl.judge(out[:, :D], ref, sc, ACT_BAR, c["deg"], what + " forward"))
            ref, sc = dl.scaled_ref(c["t_rowptr_h"], c["t_dst_h"], gy[:, :D], dv, dv)
            shares.append(dl.judge(gt[:, :D], ref, sc, GRAD_BAR, c["t_deg"], what + " grad_tbl"))
    _report(f"gcn D={D}", shares)


# ---- APPNP -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", NARROW)
def test_appnp(D):
    from bridged_gnn_amd import ops
    c = _case("gcn")
    _cover(c, D, "appnp")
    g, N, dev = c["g"], c["N"], _dev()
    rng = np.random.default_rng(400 + D)
    ones = torch.ones(N, device=dev)
    shares = []
    # one step, exact: 0.5 * (sum + h) of integers is exact in fp32; forward view and by-source view
    Ti, hi = _ints(rng, N, D), _ints(rng, N, D)
    for view, (rp, cl) in (("by destination", ("rowptr", "col")), ("by source", ("t_rowptr", "t_dst"))):
        def step():
            big, out = _nan_view(N, D)
            ops.appnp_step(Ti.to(dev), hi.to(dev), c[rp], c[cl], ones, N, D, 0.5, True, "out", out=out)
            return big, out
        big, out = _twice(step, f"appnp_step D={D} {view}")
        _untouched(big, N, D, f"appnp_step D={D} {view}")
        want = (_int_walk(c[rp + "_h"], c[cl + "_h"], Ti) + hi.long()).double() * 0.5
        assert torch.equal(out[:, :D].cpu().double(), want[:, :D]), f"appnp_step D={D} {view}: not the exact half sums"
    # one step and the propagation against fp64, both views (the by-source view is the gradient with respect to h)
    dv = g.dinv.cpu()
    T, h = _randn(rng, N, D), _randn(rng, N, D)
    for view, (rp, cl), bar, degs in (("by destination", ("rowptr", "col"), ACT_BAR, c["deg"]), ("by source", ("t_rowptr", "t_dst"), GRAD_BAR, c["t_deg"])):
        out = ops.appnp_step(T.to(dev), h.to(dev), c[rp], c[cl], g.dinv, N, D, 0.1, True, "out")
        s, a = dl.scaled_ref(c[rp + "_h"], c[cl + "_h"], T[:, :D], dv, dv)
        shares.append(dl.judge(out[:, :D], 0.9 * s + 0.1 * h[:, :D].double(), 0.9 * a + 0.1 * h[:, :D].double().abs(), bar, degs,
                               f"appnp_step D={D} {view}"))
        for K in (1, 3):
            def prop():
                big, out = _nan_view(N, D)
                ops.appnp_propagate(h.to(dev), c[rp], c[cl], g.dinv, N, D, K, 0.1, out=out, hubs=g.hubs)
                return big, out
            big, out = _twice(prop, f"appnp_propagate D={D} K={K} {view}")
            _untouched(big, N, D, f"appnp_propagate D={D} K={K} {view}")
            ref, sc = dl.appnp_ref(c[rp + "_h"], c[cl + "_h"], h[:, :D], dv, K, 0.1)
            shares.append(dl.judge(out[:, :D], ref, sc, bar, degs, f"appnp_propagate D={D} K={K} {view}"))
    _report(f"appnp D={D}", shares)


# ---- GCNII -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", NARROW)
def test_gcn2(H):
    from bridged_gnn_amd import ops
    c = _case("gcn")
    _cover(c, H, "gcn2")
    g, N, dev = c["g"], c["N"], _dev()
    rng = np.random.default_rng(500 + H)
    Hp = ops.pad4(H)
    x, x0, gy = _randn(rng, N, H), _randn(rng, N, H), _randn(rng, N, H)
    M = torch.zeros(Hp, Hp)
    M[:H, :H] = 0.7 * torch.eye(H) + 0.3 * torch.from_numpy((rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32))
    dv = g.dinv.cpu()
    shares = []

    def fwd():
        big, out = _nan_view(N, H)
        bm, m = _nan_view(N, H)
        ops.gcn2_conv(x.to(dev), x0.to(dev), M.to(dev), c["rowptr"], c["col"], g.dinv, N, H, 0.1, hubs=g.hubs, m_out=m, out=out)
        _untouched(bm, N, H, f"gcn2 H={H} m_out")
        fwd.m = m
        return big, out
    big, out = _twice(fwd, f"gcn2 H={H}")
    _untouched(big, N, H, f"gcn2 H={H}")
    ref, m64, sc, msc = dl.gcn2_ref(c["rowptr_h"], c["col_h"], x[:, :H], x0[:, :H], M[:H, :H], dv, 0.1)
    shares.append(dl.judge(fwd.m[:, :H], m64, msc, ACT_BAR, c["deg"], f"gcn2 H={H} mix"))
    y = out[:, :H].cpu()
    shares.append(dl.judge(y, ref, sc, ACT_BAR, c["deg"], f"gcn2 H={H} out"))           # (ReLU is 1-Lipschitz: no kink in the value)
    # backward: the dense half, then the walk over the by-source view
    gz, t, gx0 = ops.gcn2_conv_bwd(out, gy.to(dev), M.to(dev), H, 0.1, 0.0)

    def bwd():
        big, gx = _nan_view(N, H)
        ops.gcn_aggregate(t, c["t_rowptr"], c["t_dst"], g.dinv, N, H, out=gx, hubs=g.t_hubs)
        return big, gx
    bb, gx = _twice(bwd, f"gcn2 H={H} backward")
    _untouched(bb, N, H, f"gcn2 H={H} backward")
    gz64 = gy[:, :H].double() * (y > 0)                                                  # the ReLU state is the kernel's own, as in test_gpu_gcn2.py
    gm, gma = gz64 @ M[:H, :H].double().t(), gz64.abs() @ M[:H, :H].double().abs().t()
    shares.append(dl.judge(t[:, :H], 0.9 * gm, 0.9 * gma, GRAD_BAR, c["deg"], f"gcn2 H={H} t"))
    shares.append(dl.judge(gx0[:, :H], 0.1 * gm, 0.1 * gma, GRAD_BAR, c["deg"], f"gcn2 H={H} grad_x0"))
    # grad_x from the kernel's own t (fp32): the walk alone is under test here
    ref, sc = dl.scaled_ref(c["t_rowptr_h"], c["t_dst_h"], t[:, :H].cpu(), dv, dv)
    shares.append(dl.judge(gx[:, :H], ref, sc, GRAD_BAR, c["t_deg"], f"gcn2 H={H} grad_x"))
    _report(f"gcn2 H={H}", shares)


# ---- DeeperGCN's softmax aggregation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1.0, -0.7, 40.0])
@pytest.mark.parametrize("H", WIDTHS)
def test_gen_softmax(H, t):
    from bridged_gnn_amd import ops
    c = _case("sage")
    _cover(c, H, "gen", u_caps=(dl.GEN_BWD_U_CAP,))                       # gen_bwd_kernel runs at min(U, 4) slots a sub-group
    N, dev = c["N"], _dev()
    rng = np.random.default_rng(600 + H)
    x, gz = _randn(rng, N, H), _randn(rng, N, H)
    tt = torch.tensor([t], dtype=torch.float32, device=dev)
    t32 = float(np.float32(t))
    shares = []

    def fwd():
        big, out = _nan_view(N, H)
        bl, lse = _nan_view(N, H)
        bo, o = _nan_view(N, H)
        if lse.stride(0) != o.stride(0):
            raise AssertionError
        ops.gen_softmax_aggregate(x.to(dev), c["rowptr"], c["col"], tt, N, H, save=(lse, o), out=out)
        _untouched(bl, N, H, f"gen H={H} t={t} lse")
        _untouched(bo, N, H, f"gen H={H} t={t} o")
        fwd.save = (lse, o)
        return big, out
    big, z = _twice(fwd, f"gen H={H} t={t}")
    _untouched(big, N, H, f"gen H={H} t={t}")
    lse, o = fwd.save
    z64, lse64, o64, zsc = dl.gen_ref(c["rowptr_h"], c["col_h"], x[:, :H], t32)
    shares.append(dl.judge(z[:, :H], z64, zsc, ACT_BAR, c["deg"], f"gen H={H} t={t} z"))
    shares.append(dl.judge(o[:, :H], o64, o64.abs(), ACT_BAR, c["deg"], f"gen H={H} t={t} o"))
    # lse = max + log(sum), judged element by element on the row's own scale: max_j |t v_j| over its neighbours + log(deg_i)
    lsc = dl.gen_lse_scale(c["rowptr_h"], c["col_h"], x[:, :H], t32)
    shares.append(dl.judge(lse[:, :H].reshape(-1, 1), lse64.reshape(-1, 1), lsc.reshape(-1, 1), ACT_BAR, np.repeat(c["deg"], H),
                           f"gen H={H} t={t} lse"))
    zero = torch.from_numpy(c["deg"] == 0)
    assert torch.equal(z[:, :H].cpu()[zero], x[:, :H][zero]), "a row without in-edges is x bit for bit"

    def bwd():
        big, gx = _nan_view(N, H)
        _, gt = ops.gen_softmax_aggregate_bwd(x.to(dev), gz.to(dev), (lse, o), c["t_rowptr"], c["t_dst"], tt, H, grad_x=gx)
        bwd.gt = getattr(bwd, "gt", gt)
        assert torch.equal(bwd.gt, gt), "grad_t: two calls differ"
        return big, gx
    bb, gx = _twice(bwd, f"gen H={H} t={t} backward")
    _untouched(bb, N, H, f"gen H={H} t={t} backward")
    gx64, gt64, gsc, gtsc = dl.gen_bwd_ref(c["rowptr_h"], c["col_h"], x[:, :H], gz[:, :H], t32)
    shares.append(dl.judge(gx[:, :H], gx64, gsc, GRAD_BAR, c["t_deg"], f"gen H={H} t={t} grad_x"))
    # grad_t sums every edge and channel: its scale is the fp64 sum of |a g (v_j - o_i) v_j| over them
    gt_err = abs(bwd.gt.item() - gt64.item())
    print(f"gen H={H} t={t}: grad_t {bwd.gt.item():.6e} (fp64 {gt64.item():.6e}), error {gt_err / (GRAD_BAR * gtsc.item()):.3f} of the bar")
    assert np.isfinite(bwd.gt.item()) and gt_err <= GRAD_BAR * gtsc.item(), \
        f"gen H={H} t={t} grad_t: {bwd.gt.item():.9e} against {gt64.item():.9e}, scale {gtsc.item():.3e}"
    _report(f"gen H={H} t={t}", shares)


# ---- GIN ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_gin(D):
    from bridged_gnn_amd import ops
    c = _case("sage")
    _cover(c, D, "gin")
    N, dev = c["N"], _dev()
    rng = np.random.default_rng(700 + D)
    shares = []
    for exact in (True, False):
        T, gy = (_ints if exact else _randn)(rng, N, D), (_ints if exact else _randn)(rng, N, D)
        eps = 0.0 if exact else 0.3
        et = torch.tensor([eps], dtype=torch.float32, device=dev)
        e32 = float(np.float32(eps))
        what = f"gin D={D} eps={eps}"

        def fwd():
            big, out = _nan_view(N, D)
            ops.gin_aggregate(T.to(dev), c["rowptr"], c["col"], et, N, D, out=out)
            return big, out
        big, out = _twice(fwd, what)
        _untouched(big, N, D, what)

        def bwd():
            big, gt = _nan_view(N, D)
            ops.gin_aggregate_bwd(None, None, gy.to(dev), c["t_rowptr"], c["t_dst"], et, N, D, want_bias=False, want_eps=False, grad_tbl=gt)
            return big, gt
        bb, gt = _twice(bwd, what + " backward")
        _untouched(bb, N, D, what + " backward")
        if exact:
            _exact(out, _int_walk(c["rowptr_h"], c["col_h"], T) + T.long(), D, what + " forward")
            _exact(gt, _int_walk(c["t_rowptr_h"], c["t_dst_h"], gy) + gy.long(), D, what + " backward")
            assert torch.equal(ops.gin_aggregate(T.to(dev), c["rowptr"], c["col"], None, N, D), out), what + ": eps=None"
        else:
            one = torch.ones(N)
            ref, sc = dl.scaled_ref(c["rowptr_h"], c["col_h"], T[:, :D], one, one, own=T[:, :D], w_own=1 + e32)
            shares.append(dl.judge(out[:, :D], ref, sc, ACT_BAR, c["deg"], what + " forward"))
            ref, sc = dl.scaled_ref(c["t_rowptr_h"], c["t_dst_h"], gy[:, :D], one, one, own=gy[:, :D], w_own=1 + e32)
            shares.append(dl.judge(gt[:, :D], ref, sc, GRAD_BAR, c["t_deg"], what + " grad_tbl"))
    _report(f"gin D={D}", shares)


# ---- JKNet's conv ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_jk_gcn(D):
    from bridged_gnn_amd import ops
    c = _case("jk")
    _cover(c, D, "jk")
    g, N, dev = c["g"], c["N"], _dev()
    rng = np.random.default_rng(800 + D)
    ones = torch.ones(N, device=dev)
    shares = []
    for exact in (True, False):
        T, gy = (_ints if exact else _randn)(rng, N, D), (_ints if exact else _randn)(rng, N, D)
        s, w = (ones, ones) if exact else (g.s, g.w)
        what = f"jk D={D} exact={exact}"

        def fwd():
            big, out = _nan_view(N, D)
            ops.jk_gcn_aggregate(T.to(dev), c["rowptr"], c["col"], s, w, N, D, out=out)
            return big, out
        big, out = _twice(fwd, what)
        _untouched(big, N, D, what)

        def bwd():
            big, gt = _nan_view(N, D)
            ops.jk_gcn_aggregate_bwd(None, gy.to(dev), c["t_rowptr"], c["t_dst"], s, w, N, D, want_bias=False, grad_tbl=gt)
            return big, gt
        bb, gt = _twice(bwd, what + " backward")
        _untouched(bb, N, D, what + " backward")
        if exact:
            _exact(out, _int_walk(c["rowptr_h"], c["col_h"], T) + T.long(), D, what + " forward")
            _exact(gt, _int_walk(c["t_rowptr_h"], c["t_dst_h"], gy) + gy.long(), D, what + " backward")
        else:
            sh, wh = g.s.cpu(), g.w.cpu()
            ref, sc = dl.scaled_ref(c["rowptr_h"], c["col_h"], T[:, :D], sh, sh, own=T[:, :D], w_own=wh)
            shares.append(dl.judge(out[:, :D], ref, sc, ACT_BAR, c["deg"], what + " forward"))
            ref, sc = dl.scaled_ref(c["t_rowptr_h"], c["t_dst_h"], gy[:, :D], sh, sh, own=gy[:, :D], w_own=wh)
            shares.append(dl.judge(gt[:, :D], ref, sc, GRAD_BAR, c["t_deg"], what + " grad_tbl"))
    _report(f"jk D={D}", shares)


# ---- GAT ---------------------------------------------------------------------------------------------------------------------------------
def _pow2_rows(deg):
    return torch.from_numpy((deg & (deg - 1)) == 0) & torch.from_numpy(deg > 0)


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("C", NARROW)
def test_gat(H, C):
    from bridged_gnn_amd import ops
    c = _case("gat")
    _cover(c, C, f"gat H={H}", heads=H, u_caps=(dl.GAT_EDGE_U,))          # gat_bwd_edge_kernel: U = 4 at every rung
    for v in ("rowptr_h", "t_rowptr_h"):                                  # gat_alpha_kernel<8, 4>: 8 virtual rows per wave at every C
        dl.assert_coverage(c[v], c["lad"].degrees, 64 // 8, f"gat H={H} alpha sweep {v}", heads=H)
    assert {k * dl.GAT_ALPHA_SWEEP + o for k in dl.ROUNDS for o in (-1, 0, 1)} <= set(c["lad"].degrees), "the alpha sweep's stride"
    N, dev = c["N"], _dev()
    HC = H * C
    rng = np.random.default_rng(900 + 10 * C + H)
    shares = []
    # exact: zero attention vectors -> every logit 0, state = (0, degree), coefficients 1 / degree
    Ti, gi = _ints(rng, N, HC), _ints(rng, N, HC)
    zero = torch.zeros(H, C, device=dev)
    s_src, s_dst = ops.gat_scores(Ti.to(dev), zero, zero, H, C)
    assert torch.count_nonzero(s_src).item() == 0 and torch.count_nonzero(s_dst).item() == 0
    out, state, pre, alpha = ops.gat_aggregate(Ti.to(dev), s_src, s_dst, c["rowptr"], c["col"], N, H, C, want_pre=True, return_alpha=True)
    degf = torch.from_numpy(c["deg"]).float()
    assert torch.equal(state[:, :, 0].cpu(), torch.zeros(N, H)), f"gat H={H} C={C}: a row maximum of zero logits is not 0"
    assert torch.equal(state[:, :, 1].cpu(), degf[:, None].expand(N, H)), \
        f"gat H={H} C={C}: softmax denominators of zero logits are not the degrees at rows " \
        f"{torch.nonzero((state[:, :, 1].cpu() != degf[:, None]).any(1)).reshape(-1).tolist()[:12]}"
    p2 = _pow2_rows(c["deg"])
    S = _int_walk(c["rowptr_h"], c["col_h"], Ti)[:, :HC].double() / degf.double()[:, None]
    assert torch.equal(out[:, :HC].cpu().double()[p2], S[p2]), f"gat H={H} C={C}: rows of power-of-two degree are not the exact means"
    ones_alpha = torch.ones_like(alpha)
    gt = ops.gat_aggregate_bwd(Ti.to(dev), s_src, s_dst, state, ones_alpha, pre, gi.to(dev), c["rowptr"], c["col"], c["t_rowptr"],
                               c["t_eid"], c["t_dst"], H, C, want_bias=False)[0]
    _exact(gt, _int_walk(c["t_rowptr_h"], c["t_dst_h"], gi), HC, f"gat H={H} C={C} backward gather under unit coefficients")
    # fp64
    T, gy = _randn(rng, N, HC), _randn(rng, N, HC)
    a_s = torch.from_numpy((rng.standard_normal((H, C)) / np.sqrt(C)).astype(np.float32))
    a_d = torch.from_numpy((rng.standard_normal((H, C)) / np.sqrt(C)).astype(np.float32))
    what = f"gat H={H} C={C}"

    def run():
        s_src, s_dst = ops.gat_scores(T.to(dev), a_s.to(dev), a_d.to(dev), H, C)
        out, state, pre, alpha = ops.gat_aggregate(T.to(dev), s_src, s_dst, c["rowptr"], c["col"], N, H, C, negative_slope=SLOPE,
                                                   want_pre=True, return_alpha=True)
        back = ops.gat_aggregate_bwd(T.to(dev), s_src, s_dst, state, alpha, pre, gy.to(dev), c["rowptr"], c["col"], c["t_rowptr"],
                                     c["t_eid"], c["t_dst"], H, C, negative_slope=SLOPE, want_bias=False)
        return (s_src, s_dst, out, state, alpha) + tuple(back[:3])
    r1, r2 = run(), run()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b), what + ": two calls differ"
    s_src, s_dst, out, state, alpha, gt, ds_src, ds_dst = r1
    assert bool(torch.isfinite(out).all()) and torch.count_nonzero(out[:, HC:]).item() == 0, what + ": pad columns"
    assert torch.count_nonzero(gt[:, HC:]).item() == 0, what + ": pad columns of grad_tbl"
    ref = dl.gat_ref(c["rowptr_h"], c["col_h"], T, a_s, a_d, H, C, SLOPE, gy=gy)
    Tv = T[:, :HC].double().reshape(N, H, C)
    shares.append(dl.judge(s_src, ref["s_src"], (Tv * a_s.double()).abs().sum(-1), ACT_BAR, c["deg"], what + " s_src"))
    shares.append(dl.judge(s_dst, ref["s_dst"], (Tv * a_d.double()).abs().sum(-1), ACT_BAR, c["deg"], what + " s_dst"))
    # every (row, head) pair is a row of its own: one head's scale never covers for another's
    ph, deg_h, t_deg_h = (lambda x: x.reshape(-1, C)), np.repeat(c["deg"], H), np.repeat(c["t_deg"], H)
    col1 = lambda x: x.reshape(-1, 1)
    shares.append(dl.judge(ph(out[:, :HC]), ph(ref["out"]), ph(ref["out_abs"]), ACT_BAR, deg_h, what + " out"))
    # a coefficient on the scale of its row's largest coefficient
    dst, _ = dl._edges(c["rowptr_h"], c["col_h"])
    amax = torch.zeros(N, H, dtype=torch.float64).index_reduce(0, dst, ref["alpha"], "amax")
    edeg = np.repeat(c["deg"][dst.numpy()], H)
    shares.append(dl.judge(col1(alpha), col1(ref["alpha"]), col1(amax[dst]), ACT_BAR, edeg, what + " alpha"))
    shares.append(dl.judge(ph(gt[:, :HC]), ph(ref["grad_tbl"]), ph(ref["grad_tbl_abs"]), GRAD_BAR, t_deg_h, what + " grad_tbl"))
    shares.append(dl.judge(col1(ds_src), col1(ref["ds_src"]), col1(ref["ds_src_abs"]), GRAD_BAR, t_deg_h, what + " ds_src"))
    shares.append(dl.judge(col1(ds_dst), col1(ref["ds_dst"]), col1(ref["ds_dst_abs"]), GRAD_BAR, deg_h, what + " ds_dst"))
    _report(what, shares)


# ---- GATv2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("C", NARROW)
def test_gatv2(H, C):
    from bridged_gnn_amd import ops
    c = _case("gat")
    _cover(c, C, f"gatv2 H={H}", heads=H, u_caps=(dl.GAT_EDGE_U,))        # every bgnn_gatv2.hip walk: U = 4 at every rung
    N, dev = c["N"], _dev()
    HC = H * C
    P = ops.pad4(HC)
    rng = np.random.default_rng(1000 + 10 * C + H)
    shares = []

    def table(XL, XR):
        t = torch.zeros(N, 2 * P)
        t[:, :HC], t[:, P:P + HC] = XL[:, :HC], XR[:, :HC]
        return t.to(dev)
    # exact: a zero attention vector -> every logit 0
    Xi, Ri = _ints(rng, N, HC), _ints(rng, N, HC)
    out, state, _, _ = ops.gatv2_aggregate(table(Xi, Ri), torch.zeros(HC, device=dev), c["rowptr"], c["col"], N, H, C)
    degf = torch.from_numpy(c["deg"]).float()
    assert torch.equal(state[:, :, 0].cpu(), torch.zeros(N, H)), f"gatv2 H={H} C={C}: a row maximum of zero logits is not 0"
    assert torch.equal(state[:, :, 1].cpu(), degf[:, None].expand(N, H)), \
        f"gatv2 H={H} C={C}: softmax denominators of zero logits are not the degrees at rows " \
        f"{torch.nonzero((state[:, :, 1].cpu() != degf[:, None]).any(1)).reshape(-1).tolist()[:12]}"
    p2 = _pow2_rows(c["deg"])
    S = _int_walk(c["rowptr_h"], c["col_h"], Xi)[:, :HC].double() / degf.double()[:, None]
    assert torch.equal(out[:, :HC].cpu().double()[p2], S[p2]), f"gatv2 H={H} C={C}: rows of power-of-two degree are not the exact means"
    # fp64
    XL, XR, gy = _randn(rng, N, HC), _randn(rng, N, HC), _randn(rng, N, HC)
    att = torch.from_numpy((rng.standard_normal((H, C)) / np.sqrt(C)).astype(np.float32))
    tbl = table(XL, XR)
    what = f"gatv2 H={H} C={C}"

    def run():
        out, state, pre, alpha = ops.gatv2_aggregate(tbl, att.to(dev), c["rowptr"], c["col"], N, H, C, negative_slope=SLOPE, want_pre=True,
                                                     return_alpha=True)
        back = ops.gatv2_aggregate_bwd(tbl, att.to(dev), state, pre, gy.to(dev), c["rowptr"], c["col"], c["t_rowptr"], c["t_eid"],
                                       c["t_dst"], H, C, negative_slope=SLOPE, want_bias=False)
        return (out, state, alpha) + tuple(back[:2])
    r1, r2 = run(), run()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b), what + ": two calls differ"
    out, state, alpha, gtbl, gatt = r1
    assert bool(torch.isfinite(out).all()) and torch.count_nonzero(out[:, HC:]).item() == 0, what + ": pad columns"
    assert torch.count_nonzero(gtbl[:, HC:P]).item() == 0 and torch.count_nonzero(gtbl[:, P + HC:]).item() == 0, what + ": pad columns of grad_tbl"
    ref = dl.gatv2_ref(c["rowptr_h"], c["col_h"], XL, XR, att, H, C, SLOPE, gy=gy)
    ph, deg_h, t_deg_h = (lambda x: x.reshape(-1, C)), np.repeat(c["deg"], H), np.repeat(c["t_deg"], H)   # (row, head) pairs, as in test_gat
    col1 = lambda x: x.reshape(-1, 1)
    shares.append(dl.judge(ph(out[:, :HC]), ph(ref["out"]), ph(ref["out_abs"]), ACT_BAR, deg_h, what + " out"))
    dst, _ = dl._edges(c["rowptr_h"], c["col_h"])
    amax = torch.zeros(N, H, dtype=torch.float64).index_reduce(0, dst, ref["alpha"], "amax")
    shares.append(dl.judge(col1(alpha), col1(ref["alpha"]), col1(amax[dst]), ACT_BAR, np.repeat(c["deg"][dst.numpy()], H), what + " alpha"))
    shares.append(dl.judge(ph(gtbl[:, :HC]), ph(ref["dxl"]), ph(ref["dxl_abs"]), GRAD_BAR, t_deg_h, what + " dx_l"))
    shares.append(dl.judge(ph(gtbl[:, P:P + HC]), ph(ref["dxr"]), ph(ref["dxr_abs"]), GRAD_BAR, deg_h, what + " dx_r"))
    shares.append(dl.judge(gatt.reshape(1, -1), ref["datt"].reshape(1, -1), ref["datt_abs"].reshape(1, -1), GRAD_BAR, [0], what + " grad_att"))
    _report(what, shares)


# ---- the single-head AdaptedConv aggregation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", dl.ADAPTED_WIDTHS)
def test_adaptedconv(D):
    from bridged_gnn_amd import ops
    c = _case("adapted")
    _cover(c, D, "adaptedconv", table=dl.ADAPTED_LADDER)
    assert c["deg"].max() < ops.HUB_THRESHOLD and c["t_deg"].max() < ops.HUB_THRESHOLD and c["g"].hub_tables() is None
    N, dev = c["N"], _dev()
    rng = np.random.default_rng(1100 + D)
    # a domain mask that mixes both domains inside every row: the sources alternate, and a destination takes the domain its first
    # neighbour is not in -- its own node is one of its row's neighbours (the self loop), so every row of two edges or more is mixed
    mask = np.arange(N) % 2 == 0
    rp, cl = c["rowptr_h"], c["col_h"]
    many = np.nonzero(c["deg"] >= 2)[0]
    assert (cl[rp[many]] != many).all(), "the self loop is a row's last edge"
    mask[many] = ~mask[cl[rp[many]]]
    dst, src = dl._edges(rp, cl)
    both = torch.zeros(N, 2).index_put_((dst, torch.from_numpy(mask)[src].long()), torch.ones(dst.shape[0]), accumulate=True)
    assert bool(((both > 0).sum(1) == 2)[torch.from_numpy(c["deg"] >= 2)].all()), "every row of two edges or more holds both domains"
    assert 0.3 < mask.mean() < 0.7
    m8 = _t(mask).to(torch.uint8)
    hS, hT, gout = _randn(rng, N, D), _randn(rng, N, D), _randn(rng, N, D)
    a1 = torch.from_numpy((rng.standard_normal(D) * 0.3).astype(np.float32))
    a2 = torch.from_numpy((rng.standard_normal(D) * 0.3).astype(np.float32))
    what = f"adaptedconv D={D}"
    shares = []

    def fwd():
        big2 = torch.full((N + 3, ops.pad4(D)), float("nan"), device=dev)          # the op takes a contiguous out: rows beyond stay NaN
        o, al = ops.adaptedconv_aggregate(hS.to(dev), hT.to(dev), a1.to(dev), a2.to(dev), c["g"], m8, D, SLOPE, want_alpha=True,
                                          out=big2[:N])
        fwd.alpha = al
        return big2, o
    big, out = _twice(fwd, what)
    assert bool(torch.isfinite(out).all()) and bool(torch.isnan(big[N:]).all()), what + ": rows outside the range"
    if out.shape[1] > D:
        assert torch.count_nonzero(out[:, D:]).item() == 0, what + ": pad columns"
    alpha = fwd.alpha
    ref = dl.adapted_ref(c["rowptr_h"], c["col_h"], hS, hT, a1, a2, mask, D, SLOPE, gout=gout)
    shares.append(dl.judge(out[:, :D], ref["out"], ref["out_abs"], ACT_BAR, c["deg"], what + " out"))

    # The whole-graph call above runs agg_wide_fast_kernel at D > 32 (fast_plan admits it).  A first-part call (part = 1) is
    # refused by fast_plan and walks the general kernels, agg_wide_kernel at D > 32: with park_begin = row_end no row is parked,
    # every row is finished in this launch, and the state buffer is never written.
    def part1():
        big2 = torch.full((N + 3, ops.pad4(D)), float("nan"), device=dev)
        part1.ms = torch.full((N, 2), float("nan"), device=dev)
        o = ops.adaptedconv_aggregate(hS.to(dev), hT.to(dev), a1.to(dev), a2.to(dev), c["g"], m8, D, SLOPE, out=big2[:N],
                                      row_begin=0, row_end=N, state_ms=part1.ms, part=1, park_begin=N)
        return big2, o
    bigp, outp = _twice(part1, what + " part 1")
    assert bool(torch.isfinite(outp).all()) and bool(torch.isnan(bigp[N:]).all()), what + " part 1: rows outside the range"
    assert bool(torch.isnan(part1.ms).all()), what + " part 1: no row is parked, the state buffer stays as it was"
    if outp.shape[1] > D:
        assert torch.count_nonzero(outp[:, D:]).item() == 0, what + " part 1: pad columns"
    shares.append(dl.judge(outp[:, :D], ref["out"], ref["out_abs"], ACT_BAR, c["deg"], what + " part 1 (general kernel) out"))
    amax = torch.zeros(N, dtype=torch.float64).index_reduce(0, dst, ref["alpha"], "amax")
    shares.append(dl.judge(alpha.reshape(-1, 1), ref["alpha"].reshape(-1, 1), amax[dst].reshape(-1, 1), ACT_BAR,
                           torch.from_numpy(c["deg"])[dst], what + " alpha"))
    g1 = ops.adaptedconv_aggregate_bwd(hS.to(dev), hT.to(dev), a1.to(dev), a2.to(dev), c["g"], m8, D, out, alpha, gout.to(dev), SLOPE)
    g2 = ops.adaptedconv_aggregate_bwd(hS.to(dev), hT.to(dev), a1.to(dev), a2.to(dev), c["g"], m8, D, out, alpha, gout.to(dev), SLOPE)
    # the table gradients are pulled without atomics; at D <= 128 the two attention-vector gradients are accumulated by float
    # atomics (ops.adaptedconv_aggregate_bwd, as tests/test_gpu_training.py takes it): no bit contract there
    for a, b, name in zip(g1[:2], g2[:2], ("dh_t2s", "dh_s2t")):
        assert torch.equal(a, b), f"{what} {name}: two calls differ"
    # a table row is read as a neighbour (by source) and as the row's own node (by destination): judged on the scale of both
    both_deg = c["deg"] + c["t_deg"]
    for k, name in ((0, "dh_t2s"), (1, "dh_s2t")):
        shares.append(dl.judge(g1[k][:, :D], ref["grads"][k], ref["grads_abs"], GRAD_BAR, both_deg, f"{what} {name}"))
    for k, name in ((2, "da_t2s"), (3, "da_s2t")):
        r = ref["grads"][k].reshape(1, -1)
        # (the attention vectors' gradients are sums over every edge: the bar of tests/test_gpu_pull_wide.py, of the vector's maximum)
        shares.append(dl.judge(g1[k][:D].reshape(1, -1), r, r.abs().max().expand_as(r), GRAD_BAR, [0], f"{what} {name}"))
    _report(what, shares)
