"""GPU: segmented hub rows of the GIN walk (bgnn_gin_aggregate_hub_f32 / bgnn_gin_aggregate_bwd_hub_f32, `ops.gin_aggregate_hubs` /
`ops.gin_aggregate_bwd_hubs`, `GINNet(segment_hubs=True)`; models/backbones.py:26-57) on the graphs of test_gpu_gin.py (A, A1, A2: no
hub; B: node 3 with >= 700 in-edges, node 5 with >= 700 out-edges; C: 70 000 rows, a row of 30 000 edges) with that file's bars
(ACT_BAR / GRAD_BAR) and fp64 restatements.  What is pinned bit for bit: hubs=None is the old call; with tables every non-hub row is
the unsegmented call's row; a hub of ONE segment is the unsegmented row as well (one partial added to 0, then the same own row, bias
and epilogue) at every width class, eps, with and without bias, under ReLU + dropout and log_softmax, out of NaN-filled buffers; two
runs agree; the dropout zero pattern is the unsegmented call's.  Several segments per hub (sizes 128, 100, 37 at threshold 256, and
(8, 5) where most rows are hubs) are held to the fp64 restatement; graph C's 30 000-edge row is first restated on the CPU in fp32 in
the segmented order.  The backward runs over the by-source tables (node 5 a hub source), square and rectangular (a hub source past
n_rows has no own term); the rectangular forward with row ids carries the square call's bits and masks.  Malformed hub arguments
are refused with error codes or give finite wrong sums.
Each test prints its worst share of the bar.  Measured on an MI355X: forward 0.015 on graph B at (256, 128) and 0.019 over the
segment sizes; graph C 0.007 at D = 5 and 0.015 at D = 128 (its 30 000-edge row: the same, and the CPU restatement of the segmented
order takes 0.007 and 0.015); backward 0.023 (grad_tbl) / 0.016 (grad_bias) / 0.000 (grad_eps) on graph B, 0.022 / 0.014 / 0.000 at
3001 rows, 0.029 / 0.013 / 0.000 on graph A2; the rectangular backward 0.004; the model 0.013 (logp) and 0.094 (gradients) undirected
at the shipped sizes, 0.014 and 0.093 at (8, 5)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gin_host import OFFICE_MODELS, mult_adj, restate
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _dev
from test_gpu_gin import (SEED, _agg64, _bias, _case, _et, _fixture_case, _inputs, _model, _ok, _params64, _walk32)

pytestmark = pytest.mark.gpu

WIDTHS = (1, 4, 5, 33, 64, 128, 129, 200)


def _tabs(g, thr, seg, by_source=False, need=True):
    t = g.csr.transposed_hub_tables(thr, seg) if by_source else g.csr.hub_tables(thr, seg)
    if t is None:
        assert not need
        return None
    return (thr, t[0], t[1], t[2])


def _fwd(T, g, eps, n, D, hubs, **kw):
    from bridged_gnn_amd import ops
    return ops.gin_aggregate_hubs(T, g.by_dst[0], g.by_dst[1], eps, n, D, hubs=hubs, **kw)


def _plain(T, g, eps, n, D, **kw):
    from bridged_gnn_amd import ops
    return ops.gin_aggregate(T, g.by_dst[0], g.by_dst[1], eps, n, D, **kw)


def _maxdeg(g, n):
    rp = g.by_dst[0].long()
    return int((rp[1:n + 1] - rp[:n]).max().item())


# ---- bits ----------------------------------------------------------------------------------------------------------
def test_none_is_the_old_call_and_non_hub_rows_keep_their_bits():
    dev = _dev()
    n, g, src, dst = _case("B")
    rng = np.random.default_rng(171)
    hubs = _tabs(g, 256, 128)
    hub_rows = hubs[1].long()
    assert 3 in hub_rows.tolist()
    rest = torch.ones(n, dtype=torch.bool, device=dev)
    rest[hub_rows] = False
    worst = 0.0
    for D in (5, 64, 200):
        x, W, b, T = _inputs(rng, n, D, dev)
        bp = _bias(b, D, dev)
        e = _et(0.3, dev)
        for kw in (dict(), dict(epilogue="relu", p_drop=0.5, seed=SEED)):
            old = _plain(T, g, e, n, D, bias=bp, **kw)
            assert torch.equal(_fwd(T, g, e, n, D, None, bias=bp, **kw), old), f"D={D}: hubs=None is not the old call"
            new = _fwd(T, g, e, n, D, hubs, bias=bp, **kw)
            assert torch.equal(new[rest], old[rest]), f"D={D} {kw}: a non-hub row moved"
        ref = _agg64(x, src, dst, float(np.float32(0.3))) @ W.t() + bp[:D].double()
        worst = max(worst, _ok(_fwd(T, g, e, n, D, hubs, bias=bp)[:, :D], ref, ACT_BAR, f"graph B D={D} (256, 128)"))
    print(f"graph B (256, 128): worst forward error {worst:.3f} of the bar")


def test_one_segment_per_hub_is_bitwise_the_unsegmented_row():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case("B")
    seg = _maxdeg(g, n)
    hubs = _tabs(g, 256, seg)
    assert 3 in hubs[1].tolist() and hubs[3].shape[0] // 2 == hubs[1].shape[0]           # one segment per hub
    rng = np.random.default_rng(172)
    for D in WIDTHS:
        Dp = ops.pad4(D)
        x, W, b, T = _inputs(rng, n, D, dev)
        bp = _bias(b, D, dev)
        # the table as a view of a wider NaN buffer (pad columns NaN as well), the output a view of another
        wide = torch.full((n, Dp + 8), float("nan"), device=dev)
        wide[:, 4:4 + D] = T[:, :D]
        Tv = wide[:, 4:4 + Dp]
        for k, eps in enumerate((0.0, 0.3, -1.0)):
            bias = None if k == 1 else bp
            for kw in (dict(epilogue="relu", p_drop=0.5, seed=SEED), dict(epilogue="log_softmax")):
                if kw["epilogue"] == "log_softmax" and D > 128:
                    continue
                what = f"D={D} eps={eps} bias={bias is not None} {kw['epilogue']}"
                old = _plain(Tv, g, _et(eps, dev), n, D, bias=bias, **kw)
                box = torch.full((n + 2, Dp + 8), float("nan"), device=dev)
                new = _fwd(Tv, g, _et(eps, dev), n, D, hubs, bias=bias, out=box[1:n + 1, 4:4 + Dp], **kw)
                assert torch.equal(new, old), what + ": a hub of one segment is not the unsegmented row"
                assert bool(torch.isfinite(new).all()), what
                if Dp > D:
                    assert torch.count_nonzero(new[:, D:]).item() == 0, what + ": pad columns must be 0"
                assert bool(torch.isnan(box[0]).all()) and bool(torch.isnan(box[n + 1]).all()) and bool(torch.isnan(box[:, :4]).all()) \
                    and bool(torch.isnan(box[:, 4 + Dp:]).all()), what + ": written outside the output rows"


def test_several_segments_per_hub():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case("B")
    rng = np.random.default_rng(173)
    worst, ragged = 0.0, False
    for thr, seg in ((256, 128), (256, 100), (256, 37), (8, 5)):
        hubs = _tabs(g, thr, seg)
        rows, sp, bounds = hubs[1].tolist(), hubs[2].tolist(), hubs[3].view(-1, 2).tolist()
        assert 3 in rows
        if thr == 8:
            assert len(rows) > n // 2                                                    # most rows are hubs
        h3 = rows.index(3)
        assert sp[h3 + 1] - sp[h3] >= 2
        last = bounds[sp[h3 + 1] - 1]
        ragged = ragged or (last[1] - last[0]) < seg
        for D in (5, 64, 200):
            x, W, b, T = _inputs(rng, n, D, dev)
            bp = _bias(b, D, dev)
            e = _et(0.3, dev)
            what = f"graph B D={D} ({thr}, {seg})"
            ref = _agg64(x, src, dst, float(np.float32(0.3))) @ W.t() + bp[:D].double()
            out = _fwd(T, g, e, n, D, hubs, bias=bp)
            worst = max(worst, _ok(out[:, :D], ref, ACT_BAR, what))
            assert torch.equal(_fwd(T, g, e, n, D, hubs, bias=bp), out), what + ": two runs differ"
            if D <= 128:
                lref = torch.log_softmax(ref, 1)
                worst = max(worst, _ok(_fwd(T, g, e, n, D, hubs, bias=bp, epilogue="log_softmax")[:, :D], lref, ACT_BAR, what + " lsm"))
            # dropout: the zero pattern of the unsegmented call at the same seed; kept elements are the no-dropout output scaled
            y0 = _fwd(T, g, e, n, D, hubs, bias=bp, epilogue="relu")
            assert torch.equal(y0, torch.relu(out)), what + ": relu epilogue"
            y = _fwd(T, g, e, n, D, hubs, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED)
            old = _plain(T, g, e, n, D, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED)
            m = ops.feature_dropout(torch.ones(n, D, device=dev), 0.5, SEED)
            assert torch.equal(y[:, :D], y0[:, :D] * m), what + ": the mask law"
            live = (y0[:, :D] > 0) & (_plain(T, g, e, n, D, bias=bp, epilogue="relu")[:, :D] > 0)
            assert torch.equal((y[:, :D] == 0)[live], (old[:, :D] == 0)[live]), what + ": the zero pattern moved"
            word = torch.tensor([1000], dtype=torch.int64, device=dev)
            assert torch.equal(_fwd(T, g, e, n, D, hubs, bias=bp, epilogue="relu", p_drop=0.5, seed=SEED - 1000, seed_dev=word), y), \
                what + ": seed + device word is the seed"
            if ops.pad4(D) > D:
                assert torch.count_nonzero(y[:, D:]).item() == 0
    assert ragged, "no segment size left node 3 a ragged last segment"
    print(f"graph B, several segments: worst forward error {worst:.3f} of the bar")


def _group32(rows, EP, U):
    """one lane group's fp32 sum of `rows` in the kernel's order: sub-group s walks rows s, s + EP, ... (`_walk32`), fixed butterfly"""
    subs = [_walk32(rows[s::EP], U) if rows[s::EP].shape[0] else np.zeros(rows.shape[1], np.float32) for s in range(EP)]
    while len(subs) > 1:
        subs = [subs[k] + subs[k + 1] for k in range(0, len(subs), 2)]
    return subs[0]


@pytest.mark.parametrize("D", [5, 128])
def test_graph_c_segmented(D):
    """graph C forward.  The 30 000-edge row restated on the CPU in fp32 in the segmented order (a compensated sum per segment of
    128 edges, then the compensated sum of the 235 partial rows) before the GPU run."""
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case("C")
    EP, U = {5: (4, 4), 128: (1, 8)}[D]                                # lf_ladder: (LF, EP, U) = (2, 4, 4) at D = 5, (32, 1, 8) at D = 128
    rng = np.random.default_rng([175, D])
    x, W, b, T = _inputs(rng, n, D, dev)
    bp = _bias(b, D, dev)
    eps = 0.3
    ref = _agg64(x, src, dst, float(np.float32(eps))) @ W.t() + bp[:D].double()
    rowptr = g.by_dst[0].cpu().numpy()
    cols = g.by_dst[1].cpu().numpy()[rowptr[3]:rowptr[4]]
    assert cols.shape[0] >= 30000
    Tc = T[:, :D].cpu().numpy()
    parts = np.stack([_group32(Tc[cols[k:k + 128]], EP, U) for k in range(0, cols.shape[0], 128)])
    total = _group32(parts, EP, U)
    self_w = np.float32(1.0) + np.float32(eps)
    cpu = (self_w.astype(np.float64) * Tc[3] + total).astype(np.float32) + bp[:D].cpu().numpy()        # fma: one rounding
    tol = ACT_BAR * ref.abs().max().item() + 1e-6
    cpu_share = np.abs(cpu.astype(np.float64) - ref[3].cpu().numpy()).max() / tol
    print(f"graph C D={D}: the 30 000-edge row restated in fp32 in the segmented order takes {cpu_share:.3f} of the bar")
    assert cpu_share <= 0.5
    hubs = _tabs(g, 256, 128)
    assert 3 in hubs[1].tolist()
    out = _fwd(T, g, _et(eps, dev), n, D, hubs, bias=bp)
    worst = _ok(out[:, :D], ref, ACT_BAR, f"graph C D={D} segmented")
    hub = (out[3, :D].double() - ref[3]).abs().max().item() / tol
    if ops.pad4(D) > D:
        assert torch.count_nonzero(out[:, D:]).item() == 0
    print(f"graph C D={D} segmented: worst forward error {worst:.3f} of the bar (the 30 000-edge row: {hub:.3f})")


# ---- backward ------------------------------------------------------------------------------------------------------
def _backward_case(name, D, epi, eps, t_hubs, rng, worst):
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case(name)
    Dp = ops.pad4(D)
    x, W, b, T = _inputs(rng, n, D, dev)
    bp = _bias(b, D, dev)
    e = _et(eps, dev)
    p = 0.5 if epi == "relu" else 0.0
    y = _plain(T, g, e, n, D, bias=bp, epilogue=epi, p_drop=p, seed=SEED)
    t_rowptr, t_dst = g.by_dst[2], g.by_dst[3]
    dy = torch.zeros(n, Dp, device=dev)
    dy[:, :D] = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
    what = f"graph {name} D={D} epi={epi} eps={eps} hubs=({t_hubs[0]}, .)"
    run = lambda **kw: ops.gin_aggregate_bwd_hubs(kw.pop("tbl", T), y, dy, t_rowptr, t_dst, e, n, D, epilogue=epi, p_drop=p, hubs=t_hubs, **kw)
    gt, gb, ge = run()
    gt2, gb2, ge2 = run()
    assert torch.equal(gt, gt2) and torch.equal(gb, gb2) and torch.equal(ge, ge2), what + ": two runs differ"
    gt3, gb3, ge3 = run(tbl=None, want_eps=False)
    assert ge3 is None and torch.equal(gt3, gt) and torch.equal(gb3, gb), what + ": want_eps=False"
    # g, grad_bias and grad_eps are the launches of the call without hubs; so is every non-hub source's row
    ot, ob, oe = ops.gin_aggregate_bwd(T, y, dy, t_rowptr, t_dst, e, n, D, epilogue=epi, p_drop=p)
    rest = torch.ones(n, dtype=torch.bool, device=dev)
    rest[t_hubs[1].long()] = False
    assert torch.equal(ob, gb) and torch.equal(oe, ge) and torch.equal(ot[rest], gt[rest]), what + ": a non-hub result moved"
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
    assert err <= tol, f"{what} grad_eps: {ge.item()} vs {re_.item()}, err {err:.3e} > {tol:.3e}"
    worst[2] = max(worst[2], err / tol if tol > 0 else 0.0)
    if Dp > D:
        assert torch.count_nonzero(gt[:, D:]).item() == 0, what + ": pad columns must be 0"


@pytest.mark.parametrize("name,widths,cfgs", [("B", (5, 64, 129), ((256, 128), (256, 37), (8, 5))), ("A1", (5, 64), ((8, 5),)),
                                              ("A2", (128,), ((8, 5),))])
def test_backward_with_by_source_tables(name, widths, cfgs):
    n, g, src, dst = _case(name)
    rng = np.random.default_rng(177)
    worst = [0.0, 0.0, 0.0]
    for thr, seg in cfgs:
        t_hubs = _tabs(g, thr, seg, by_source=True)
        if name == "B":
            assert 5 in t_hubs[1].tolist()                                               # node 5 is a hub source
        for D in widths:
            for epi, eps in ((None, 0.3), ("relu", -2.5), ("log_softmax", 0.0)):
                if epi == "log_softmax" and D > 128:
                    continue
                _backward_case(name, D, epi, eps, t_hubs, rng, worst)
    print(f"graph {name}: worst segmented backward error {worst[0]:.3f} (grad_tbl), {worst[1]:.3f} (grad_bias), {worst[2]:.3f} (grad_eps) "
          "of the bar")


# ---- rectangular calls ---------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _renumbered(seed=178, frac=0.6):
    """graph B with its nodes renumbered, new row i = old node perm[i]: a random 60 % of the nodes are the owned rows (node 3 among
    them), the rest trailing table slots (node 5 among them); every owned row keeps its edge order, so its sums -- and the segments
    of its hubs -- are the square call's.  -> (n, g, n_own, perm (device), rowptr_o, col_o)"""
    n, g, _, _ = _case("B")
    rp, colc = g.by_dst[0].long().cpu().numpy(), g.by_dst[1].long().cpu().numpy()
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    order = order[~np.isin(order, [3, 5])]
    n_own = int(frac * n)
    own = rng.permutation(np.concatenate([[3], order[:n_own - 1]]))
    perm = np.concatenate([own, [5], order[n_own - 1:]]).astype(np.int64)
    assert perm.shape[0] == n and np.array_equal(np.sort(perm), np.arange(n))
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    assert inv[3] < n_own <= inv[5]
    deg = (rp[1:] - rp[:-1])[own]
    rowptr_o = np.concatenate([[0], np.cumsum(deg)])
    eidx = np.repeat(rp[own] - rowptr_o[:-1], deg) + np.arange(rowptr_o[-1])     # the owned rows' edges, row by row, in their order
    col_o = inv[colc[eidx]]
    assert int((col_o >= n_own).sum()) > 1000                                     # plenty of edges read table slots
    return n, g, n_own, _t(perm), inv, _t(rowptr_o.astype(np.int32)), _t(col_o.astype(np.int32))


def test_rectangular_call_with_row_ids_carries_the_square_bits():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, n_own, perm, inv, rowptr_o, col_o = _renumbered()
    rng = np.random.default_rng(179)
    for thr, seg in ((256, 128), (8, 5)):
        hubs = _tabs(g, thr, seg)
        tabs = ops.DstCSR(rowptr_o, col_o, None, int(col_o.shape[0]), n_own).hub_tables(thr, seg)
        hubs_o = (thr, tabs[0], tabs[1], tabs[2])
        assert int(inv[3]) in hubs_o[1].tolist()
        ids = perm[:n_own].contiguous()
        for D in (5, 64, 200):
            Dp = ops.pad4(D)
            x, W, b, T = _inputs(rng, n, D, dev)
            bp = _bias(b, D, dev)
            e = _et(0.3, dev)
            what = f"D={D} ({thr}, {seg})"
            kw = dict(bias=bp, epilogue="relu", p_drop=0.5, seed=SEED)
            sq = _fwd(T, g, e, n, D, hubs, **kw)
            Tp = T[perm].contiguous()
            box = torch.full((n, Dp), float("nan"), device=dev)
            got = ops.gin_aggregate_hubs(Tp, rowptr_o, col_o, e, n_own, D, hubs=hubs_o, row_ids=ids, out=box[:n_own], **kw)
            assert torch.equal(got, sq[ids]), what + ": the owned rows do not carry the square call's bits and masks"
            assert bool(torch.isnan(box[n_own:]).all()), what + ": the tail was written"
            noid = ops.gin_aggregate_hubs(Tp, rowptr_o, col_o, e, n_own, D, hubs=hubs_o, **kw)
            assert not torch.equal(noid, got), what + ": without ids the masks must differ"
            if D >= 64:
                assert not torch.equal(noid[int(inv[3])], got[int(inv[3])]), what + ": the hub's finish group ignored its row id"


def test_rectangular_backward_hub_source_past_n_rows_has_no_own_term():
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, n_own, perm, inv, rowptr_o, col_o = _renumbered()
    E = int(col_o.shape[0])
    rowptr_e = torch.cat([rowptr_o, torch.full((n - n_own,), E, dtype=torch.int32, device=dev)])
    csr = ops.DstCSR(rowptr_e, col_o, None, E, n)
    t_rowptr, _, t_dst = csr.transposed()
    dst_o = torch.repeat_interleave(torch.arange(n_own, device=dev), (rowptr_o[1:] - rowptr_o[:-1]).long())
    rng = np.random.default_rng(180)
    worst = 0.0
    for thr, seg in ((256, 128), (8, 5)):
        t = csr.transposed_hub_tables(thr, seg)
        t_hubs = (thr, t[0], t[1], t[2])
        assert int(inv[5]) in t_hubs[1].tolist() and int(inv[5]) >= n_own                 # a hub source past n_rows
        for D in (5, 64, 129):
            Dp = ops.pad4(D)
            dy = torch.zeros(n_own, Dp, device=dev)
            dy[:, :D] = torch.from_numpy(rng.standard_normal((n_own, D)).astype(np.float32)).to(dev)
            Tt = torch.zeros(n_own, Dp, device=dev)
            Tt[:, :D] = torch.from_numpy(rng.standard_normal((n_own, D)).astype(np.float32)).to(dev)
            e = _et(0.3, dev)
            what = f"rectangular D={D} ({thr}, {seg})"
            gt, gb, ge = ops.gin_aggregate_bwd_hubs(Tt, None, dy, t_rowptr, t_dst, e, n, D, hubs=t_hubs)
            gt2, _, _ = ops.gin_aggregate_bwd_hubs(Tt, None, dy, t_rowptr, t_dst, e, n, D, hubs=t_hubs)
            assert torch.equal(gt, gt2), what + ": two runs differ"
            g64 = dy[:, :D].double()
            ref = torch.zeros(n, D, dtype=torch.float64, device=dev).index_add_(0, col_o.long(), g64[dst_o])
            ref[:n_own] += (1.0 + float(np.float32(0.3))) * g64                           # rows past n_own have no own term
            worst = max(worst, _ok(gt[:, :D], ref, GRAD_BAR, what + " grad_tbl"))
            old, ob, oe = ops.gin_aggregate_bwd(Tt, None, dy, t_rowptr, t_dst, e, n, D)
            rest = torch.ones(n, dtype=torch.bool, device=dev)
            rest[t_hubs[1].long()] = False
            assert torch.equal(old[rest], gt[rest]) and torch.equal(ob, gb) and torch.equal(oe, ge), what
            _ok(gb, g64.sum(0), GRAD_BAR, what + " grad_bias")
            ee, tol = abs(ge.item() - (g64 * Tt[:, :D].double()).sum().item()), GRAD_BAR * (g64 * Tt[:, :D].double()).abs().sum().item()
            assert ee <= tol, what + " grad_eps"
    print(f"rectangular backward: worst grad_tbl error {worst:.3f} of the bar")


# ---- malformed input -----------------------------------------------------------------------------------------------
def test_malformed_hub_arguments_are_refused_or_give_finite_wrong_sums():
    from bridged_gnn_amd import _lib as L
    from bridged_gnn_amd import ops
    dev = _dev()
    n, g, src, dst = _case("B")
    rng = np.random.default_rng(181)
    D = 64
    x, W, b, T = _inputs(rng, n, D, dev)
    rowptr, col = g.by_dst[0], g.by_dst[1]
    thr, rows, sp, bounds = _tabs(g, 256, 100)
    nh, ns = int(rows.shape[0]), int(bounds.shape[0]) // 2
    good = _fwd(T, g, _et(0.3, dev), n, D, (thr, rows, sp, bounds))
    # ids outside the table inside a hub's segments: those edges add nothing
    rp = rowptr.long()
    bad = col.clone()
    lo, hi = int(rp[3]), int(rp[4])
    bad[lo:hi:3] = n + 7
    bad[lo + 1:hi:5] = -2
    ok = (bad >= 0) & (bad < n)
    csr_dst = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:n + 1] - rp[:n]))
    ref = (1.0 + float(np.float32(0.3))) * T[:, :D].double() + \
        torch.zeros(n, D, dtype=torch.float64, device=dev).index_add_(0, csr_dst[ok], T[:, :D].double()[bad[ok].long()])
    out = ops.gin_aggregate_hubs(T, rowptr, bad, _et(0.3, dev), n, D, hubs=(thr, rows, sp, bounds))
    _ok(out[:, :D], ref, ACT_BAR, "ids outside the table in a hub's segments add nothing")
    # segment bounds and segment ranges past their arrays, a hub row outside the output: wrong sums, finite, nothing stray
    b2 = bounds.clone()
    b2[1] = int(col.shape[0]) + 1000
    b2[2] = -5
    s2 = sp.clone()
    s2[-1] = ns + 50
    r2 = rows.clone()
    r2[0] = n + 3
    for tabs in ((thr, rows, sp, b2), (thr, rows, s2, bounds), (thr, r2, sp, bounds)):
        box = torch.zeros(n, ops.pad4(D), device=dev)
        out = ops.gin_aggregate_hubs(T, rowptr, col, _et(0.3, dev), n, D, hubs=tabs, out=box)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
    assert torch.equal(_fwd(T, g, _et(0.3, dev), n, D, (thr, rows, sp, bounds)), good)       # the next well-formed call is unharmed
    # the C entry's argument checks
    lib = L.lib()
    out = torch.empty(n, ops.pad4(D), device=dev)
    wsb = int(lib.bgnn_gin_aggregate_hub_workspace_bytes(ns, D))
    assert wsb >= ns * ops.pad4(D) * 4
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def call(hub_rows, n_hubs, seg_ptr, seg_bounds, n_seg, wsp, ws_bytes, thr_=thr):
        return lib.bgnn_gin_aggregate_hub_f32(L.ptr_rows(T), T.stride(0), n, None, None, L.ptr(rowptr), L.ptr(col), int(col.shape[0]), n, D,
                                              0, 0.0, 0, None, thr_, hub_rows, n_hubs, seg_ptr, seg_bounds, n_seg, wsp, ws_bytes, None,
                                              L.ptr_rows(out), out.stride(0), L.stream())
    assert call(L.ptr(rows), nh, L.ptr(sp), L.ptr(bounds), ns, L.ptr(ws), wsb) == 0
    assert call(L.ptr(rows), nh, L.ptr(sp), L.ptr(bounds), nh - 1, L.ptr(ws), wsb) == -2       # n_seg < n_hubs
    assert call(L.ptr(rows), nh, L.ptr(sp), L.ptr(bounds), ns, L.ptr(ws), wsb, thr_=0) == -2   # no threshold
    assert call(L.ptr(rows), -1, L.ptr(sp), L.ptr(bounds), ns, L.ptr(ws), wsb) == -2
    for k in range(3):                                                                       # a NULL table with n_hubs > 0
        a = [L.ptr(rows), L.ptr(sp), L.ptr(bounds)]
        a[k] = None
        assert call(a[0], nh, a[1], a[2], ns, L.ptr(ws), wsb) == -1
    assert call(L.ptr(rows), nh, L.ptr(sp), L.ptr(bounds), ns, None, wsb) == -1
    assert call(L.ptr(rows), nh, L.ptr(sp), L.ptr(bounds), ns, L.ptr(ws), wsb - 32) == -3      # a short workspace
    assert call(None, 0, None, None, 0, None, 0) == 0                                        # no hubs: no table is looked at
    torch.cuda.synchronize()
    assert torch.equal(out, ops.gin_aggregate(T, rowptr, col, None, n, D))
    # the backward entry: the hub workspace follows the grad_eps partials
    dy = torch.zeros(n, ops.pad4(D), device=dev)
    gbuf, gt, ge = torch.empty_like(dy), torch.empty_like(dy), torch.empty(1, device=dev)
    t_rowptr, t_dst = g.by_dst[2], g.by_dst[3]
    tt = g.csr.transposed_hub_tables(256, 100)
    tnh, tns = int(tt[0].shape[0]), int(tt[2].shape[0]) // 2
    head = int(lib.bgnn_gin_aggregate_bwd_workspace_bytes(n, D))
    need = head + int(lib.bgnn_gin_aggregate_hub_workspace_bytes(tns, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def bcall(n_seg, ws_bytes, want_eps=True):
        return lib.bgnn_gin_aggregate_bwd_hub_f32(L.ptr_rows(T), T.stride(0), None, 0, L.ptr_rows(dy), dy.stride(0), n, L.ptr(t_rowptr),
                                                  L.ptr(t_dst), int(t_dst.shape[0]), n, D, None, 0, 0.0, 256, L.ptr(tt[0]), tnh,
                                                  L.ptr(tt[1]), L.ptr(tt[2]), n_seg, L.ptr_rows(gbuf), gbuf.stride(0), L.ptr_rows(gt),
                                                  gt.stride(0), L.ptr(ge) if want_eps else None, L.ptr(ws), ws_bytes, L.stream())
    assert bcall(tns, need) == 0
    assert bcall(tns, need - head, want_eps=False) == 0
    assert bcall(tns, need - 32) == -3 and bcall(tns, head - 16) == -3 and bcall(tnh - 1, need) == -2
    torch.cuda.synchronize()


# ---- model level ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,cfg", [("und", None), ("raw", (8, 5))])
def test_model_with_segmented_hubs_stays_within_the_model_bars(variant, cfg, monkeypatch):
    """GINNet(segment_hubs=True) on the office fixture: log-probabilities against the fixture and the fp64 restatement, gradients
    against the restatement on the model's own ReLU pattern.  cfg None: the shipped (threshold, segment) on the undirected graph;
    (8, 5): most rows are hubs."""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gin import GINNet, graph_hubs
    if cfg is not None:
        monkeypatch.setattr(ops, "GIN_HUB_THRESHOLD", cfg[0])
        monkeypatch.setattr(ops, "GIN_HUB_SEGMENT", cfg[1])
    data, tm, ds, fx = _fixture_case(variant)
    rows = torch.from_numpy(fx["rows"])
    x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
    A = mult_adj(data.edge_index.cpu(), x64.shape[0])
    worst = [0.0, 0.0]
    for name, L_, hidden in OFFICE_MODELS:
        base = _model(ds, fx, name, L_, hidden).eval()
        m = GINNet(ds, layer_num=L_, hidden=hidden, segment_hubs=True).to(_dev()).eval()
        m.load_state_dict(base.state_dict())
        g = m.graph(data.edge_index, data.x.shape[0])
        hubs = graph_hubs(g)
        if cfg is not None:
            assert hubs[0] is not None and hubs[1] is not None and hubs[0][1].shape[0] > 100
        P = _params64(m)
        names = [k for k, _ in m.named_parameters()]
        pre = f"{variant}/{name}/"
        out = m(data)
        lp = out.detach().cpu()
        _bar_ok(lp[rows], fx[pre + "logp"], ACT_BAR, pre + "logp")
        ref_lp = restate(P, x64, A).detach()
        _bar_ok(lp, ref_lp.numpy(), ACT_BAR, pre + "logp (every row)")
        worst[0] = max(worst[0], (lp.double() - ref_lp).abs().max().item() / (ACT_BAR * ref_lp.abs().max().item()))
        if hubs[0] is None and hubs[1] is None:
            with torch.no_grad():
                assert torch.equal(base(data), out.detach())                               # no hub: the unsegmented launches
        F.nll_loss(out[tm], data.y[tm]).backward()
        with torch.no_grad():
            h, masks = data.x, []
            for conv in m.convs[:-1]:
                h = conv.run(h, g, epilogue="relu", hubs=hubs)
                masks.append(torch.from_numpy((h.cpu().numpy() > 0).astype(np.float64)))
        loss = F.nll_loss(restate(P, x64, A, relu_masks=masks if masks else None)[tmc], y[tmc])
        for k, gr in zip(names, torch.autograd.grad(loss, [P[k] for k in names])):
            got = dict(m.named_parameters())[k].grad.cpu()
            _bar_ok(got, gr.numpy(), GRAD_BAR, f"{pre}{k} (GPU ReLU pattern)")
            worst[1] = max(worst[1], (got.double() - gr).abs().max().item() / (GRAD_BAR * gr.abs().max().item()))
    print(f"GINNet segment_hubs {variant} {cfg}: worst error {worst[0]:.3f} (logp), {worst[1]:.3f} (gradients) of the bar")
