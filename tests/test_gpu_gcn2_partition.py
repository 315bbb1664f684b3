"""GPU: GCNII on a destination-node partition (bridged_gnn_amd.dist_gcn2) -- `ops.gcn2_conv` with row ids and over a rectangular
graph (bgnn_gcn2_conv_rows_f32) against the square entry it shares its launch sequence with: identity ids bitwise, a renumbered
graph B whose owned rows carry the square call's bits and masks (hub row and hub source included, NaN wherever the kernel must not
read or write), graph C with 42 000 owned rows; world 1 against `GCN2` (fused and composed routes); simulated worlds 2/4/8 in one
process (ranks as threads), forward and the backward's edge walk with its return exchange and fold; REAL ranks in a gloo group
sharing the GPU: all-reduced gradients on the office graph against the fp64 restatement on the ranks' own ReLU patterns, three Adam
steps at dropout 0.5 against the single-GPU steps, twice, the second run bitwise the first; and the refusals.
Bars: test_gpu_gcn.py's (activations 1e-5, gradients 2e-5 of each tensor's max) and test_gpu_gcn_partition.py's (Adam parameters
1e-4, losses 1e-5 relative), imported; world 1 uses the bars of test_world1_matches_gcnnet (loss 2e-6 relative, parameters after one
Adam step 2e-6)."""
import copy
import math
import threading
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_appnp import _case, _office_data, _params64
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _sparse_parts
from test_gpu_gcn2 import _agg64, _conv64, _mix_matrix, _model64
from test_gpu_gcn_partition import ADAM_BAR, LOSS_BAR, _Box, _graph, _steps, _t, _ThreadComm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 4321
ALPHA, BETA = 0.1, math.log(1.5)
assert _agg64 and _conv64                                  # the restatement `_model64` is built from


def _inputs(n, H, gen):
    from bridged_gnn_amd import ops
    Hp = ops.pad4(H)
    x, x0 = torch.randn(n, Hp, generator=gen), torch.randn(n, Hp, generator=gen)
    w = torch.randn(H, H, generator=gen) / math.sqrt(H)
    return x, x0, w


# ---- ops.gcn2_conv with row ids ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_identity_ids_are_the_plain_kernel_bitwise(name):
    from bridged_gnn_amd import ops
    n, g, _ = _case(name)
    assert (g.hubs is not None) == (name == "B")
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    gen = torch.Generator().manual_seed(71)
    for H in (1, 3, 4, 5, 31, 32, 33, 64, 100, 128):
        Hp = ops.pad4(H)
        x, x0, w = _inputs(n, H, gen)
        x, x0, M = x.to(DEV), x0.to(DEV), _mix_matrix(w, BETA).to(DEV)
        for p in (0.0, 0.5):
            for hubs in ((g.hubs, None) if g.hubs is not None else (None,)):
                for with_m in (False, True):
                    what = f"graph {name} H={H} p={p} hubs={hubs is not None} m_out={with_m}"
                    kw = dict(p_drop=p, seed=SEED, hubs=hubs)
                    m_ref = torch.full((n, Hp), float("nan"), device=DEV) if with_m else None
                    m_got = torch.full((n, Hp), float("nan"), device=DEV) if with_m else None
                    ref = ops.gcn2_conv(x, x0, M, g.csr.rowptr, g.col, g.dinv, n, H, ALPHA, m_out=m_ref, **kw)
                    got = ops.gcn2_conv(x, x0, M, g.csr.rowptr, g.col, g.dinv, n, H, ALPHA, m_out=m_got, row_ids=ids,
                                        out=torch.full((n, Hp), float("nan"), device=DEV), **kw)
                    assert torch.equal(got, ref), what
                    if with_m:
                        assert torch.equal(m_got, m_ref), what + " (m)"


def _renumbered(name, frac, owned, slots, seed):
    """graph `name` with its nodes renumbered, new row i = old node perm[i]: a random `frac` of the nodes are the owned rows (the
    nodes `owned` among them), the rest trailing table slots (the nodes `slots` among them); every owned row keeps its edge order,
    so its sums are the square call's bit for bit.  -> (n, g, n_own, perm, rowptr_o, col_o, hubs_o | None, dinv_p), on the device"""
    from bridged_gnn_amd import ops
    n, g, _ = _case(name)
    rp, colc = g.csr.rowptr.long().cpu().numpy(), g.col.long().cpu().numpy()
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    order = order[~np.isin(order, list(owned) + list(slots))]
    n_own = int(frac * n)
    k = n_own - len(owned)
    own = rng.permutation(np.concatenate([np.asarray(owned, dtype=np.int64), order[:k]]))
    perm = np.concatenate([own, np.asarray(slots, dtype=np.int64), order[k:]]).astype(np.int64)
    assert perm.shape[0] == n and np.array_equal(np.sort(perm), np.arange(n))
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    assert all(inv[v] < n_own for v in owned) and all(inv[v] >= n_own for v in slots)
    deg = (rp[1:] - rp[:-1])[own]
    rowptr_o = np.concatenate([[0], np.cumsum(deg)])
    eidx = np.repeat(rp[own] - rowptr_o[:-1], deg) + np.arange(rowptr_o[-1])   # the owned rows' edges, row by row, in their order
    col_o = inv[colc[eidx]]
    assert int((col_o >= n_own).sum()) > 1000                                   # plenty of edges read table slots
    rowptr_o, col_o = _t(rowptr_o.astype(np.int32)), _t(col_o.astype(np.int32))
    tabs = ops.DstCSR(rowptr_o, col_o, None, int(col_o.shape[0]), n_own).hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT)
    hubs_o = None if tabs is None else (ops.GCN_HUB_THRESHOLD, tabs[0], tabs[1], tabs[2])
    perm_d = _t(perm)
    return n, g, n_own, perm_d, inv, rowptr_o, col_o, hubs_o, g.dinv[perm_d].contiguous()


def _nan_rows(n, n_own, Hp):
    """an [n, Hp] buffer of NaN and its first n_own rows"""
    buf = torch.full((n, Hp), float("nan"), device=DEV)
    return buf, buf[:n_own]


def _rect_call(H, p, x, x0, w, n, n_own, perm, rowptr_o, col_o, hubs, dinv_p, ids="own", **kw):
    """the rectangular call on the renumbered graph with NaN wherever the kernel must not read: the pad columns of x and x0, the
    rows of x0's buffer past n_own, M's padding; out and m_out are the fronts of [n, pad4(H)] buffers of NaN.
    -> (out buffer, m buffer)"""
    from bridged_gnn_amd import ops
    Hp = ops.pad4(H)
    xp = x.to(DEV)[perm].contiguous()
    x0buf, x0v = _nan_rows(n, n_own, Hp)
    x0v.copy_(x0.to(DEV)[perm[:n_own]])
    if Hp > H:
        xp[:, H:] = float("nan")
        x0v[:, H:] = float("nan")
    obuf, ov = _nan_rows(n, n_own, Hp)
    mbuf, mv = _nan_rows(n, n_own, Hp)
    M = _mix_matrix(w, BETA, pad=float("nan")).to(DEV)
    got = ops.gcn2_conv(xp, x0v, M, rowptr_o, col_o, dinv_p, n_own, H, ALPHA, p_drop=p, seed=SEED, hubs=hubs, m_out=mv, out=ov,
                        row_ids=perm[:n_own].contiguous() if ids == "own" else ids, **kw)
    assert got.data_ptr() == obuf.data_ptr()
    return obuf, mbuf


def test_rectangular_call_gives_the_owned_rows_and_masks_of_the_square_call():
    """graph B renumbered: a random 60 % of the nodes are owned (the hub row, node 3, among them), the rest trailing table slots (the
    hub source, node 5, among them).  With row_ids = the owned rows' old ids the call equals the square call's rows, out and m,
    bitwise, at p = 0 and at p = 0.5; the pad columns are 0; the buffers' tails stay NaN; without the ids the masks differ."""
    from bridged_gnn_amd import ops
    n, g, n_own, perm, inv, rowptr_o, col_o, hubs_o, dinv_p = _renumbered("B", 0.6, owned=(3,), slots=(5,), seed=72)
    assert hubs_o is not None and int(inv[3]) in hubs_o[1].cpu().tolist()
    fed = int((col_o.cpu() == int(inv[5])).sum())
    assert fed >= 256, f"the slot of node 5 feeds {fed} edges of owned rows"
    own = perm[:n_own]
    gen = torch.Generator().manual_seed(73)
    for H in (2, 5, 31, 64, 100, 128):
        Hp = ops.pad4(H)
        x, x0, w = _inputs(n, H, gen)
        M = _mix_matrix(w, BETA).to(DEV)
        for p in (0.0, 0.5):
            for hubs in (hubs_o, None):
                what = f"H={H} p={p} hubs={hubs is not None}"
                m_ref = torch.empty(n, Hp, device=DEV)
                ref = ops.gcn2_conv(x.to(DEV), x0.to(DEV), M, g.csr.rowptr, g.col, g.dinv, n, H, ALPHA, p_drop=p, seed=SEED,
                                    hubs=g.hubs if hubs is not None else None, m_out=m_ref)
                obuf, mbuf = _rect_call(H, p, x, x0, w, n, n_own, perm, rowptr_o, col_o, hubs, dinv_p)
                assert torch.equal(obuf[:n_own], ref[own]), what + " out"
                assert torch.equal(mbuf[:n_own], m_ref[own]), what + " m_out"
                assert bool(torch.isnan(obuf[n_own:]).all()) and bool(torch.isnan(mbuf[n_own:]).all()), what + ": the tail was written"
                if Hp > H:
                    assert torch.count_nonzero(obuf[:n_own, H:]).item() == 0 and torch.count_nonzero(mbuf[:n_own, H:]).item() == 0, what
                if p > 0 and hubs is not None and H >= 5:
                    plain, _ = _rect_call(H, p, x, x0, w, n, n_own, perm, rowptr_o, col_o, hubs, dinv_p, ids=None)
                    assert not torch.equal(plain[:n_own], ref[own]), what + ": local rows draw other masks"
    # refusals
    H, Hp = 5, 8
    x, x0, w = _inputs(n, H, gen)
    xp, x0p, M = x.to(DEV)[perm].contiguous(), x0.to(DEV)[own].contiguous(), _mix_matrix(w, BETA).to(DEV)
    rect = (M, rowptr_o, col_o)
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|dinv"):          # the gather reads dinv over the whole table
        ops.gcn2_conv(xp, x0p, *rect, dinv_p[:n_own].contiguous(), n_own, H, ALPHA, row_ids=own)
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|rows"):
        ops.gcn2_conv(xp[:n_own - 1], x0p, *rect, dinv_p, n_own, H, ALPHA, row_ids=own)
    with pytest.raises(ValueError, match="rows"):                                      # x0 stays at exactly n_own rows
        ops.gcn2_conv(xp, xp, *rect, dinv_p, n_own, H, ALPHA, row_ids=own)
    with pytest.raises(ValueError, match="row_ids"):
        ops.gcn2_conv(xp, x0p, *rect, dinv_p, n_own, H, ALPHA, row_ids=own.int())
    with pytest.raises(ValueError, match="row_ids"):
        ops.gcn2_conv(xp, x0p, *rect, dinv_p, n_own, H, ALPHA, row_ids=own[:-1].contiguous())
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|overlap"):        # the front of x's own buffer as the output
        ops.gcn2_conv(xp, x0p, *rect, dinv_p, n_own, H, ALPHA, row_ids=own, out=xp[:n_own])
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|overlap"):
        ops.gcn2_conv(xp, x0p, *rect, dinv_p, n_own, H, ALPHA, row_ids=own, m_out=xp[:n_own])
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|overlap"):        # ... without ids as well
        ops.gcn2_conv(xp, x0p, *rect, dinv_p, n_own, H, ALPHA, out=xp[:n_own])
    # the C entry makes the same check on the byte extents
    from bridged_gnn_amd import _lib as L
    rc = L.lib().bgnn_gcn2_conv_rows_f32(
        L.ptr_rows(xp), xp.stride(0), n, L.ptr_rows(x0p), x0p.stride(0), L.ptr(M), L.ptr(rowptr_o), L.ptr(col_o), L.ptr(dinv_p), n,
        n_own, L.ptr(own), H, ALPHA, 0.0, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, L.ptr_rows(xp[8:]), xp.stride(0),
        L.stream())
    assert rc == -2, f"out inside x: expected BGNN_E_SHAPE, got {rc}"


@pytest.mark.parametrize("H", [2, 128])
def test_rectangular_call_on_graph_c(H):
    """graph C (70 000 nodes), a random 60 % owned, the two 30 000-edge hubs (nodes 3 and 5) among the owned rows, p = 0.5: the
    square call's owned rows, bitwise.  At H = 128 a tile has 16 rows (bgnn_gcn2.hip Tile: TR = RPB * NB, lf_ladder (32, 1)) and the
    42 000 owned rows make more tiles than a persistent grid has blocks (bgnn_conv_common.h persistent_grid: at most 8 per CU); at
    H = 2 a tile has 32 rows and only the square reference passes the cap -- that case carries a hub of some 235 segments through the
    finish launch's id lookup at the narrowest width."""
    from bridged_gnn_amd import ops
    n, g, n_own, perm, inv, rowptr_o, col_o, hubs_o, dinv_p = _renumbered("C", 0.6, owned=(3, 5), slots=(), seed=74)
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-n_own // {2: 32, 128: 16}[H])
    print(f"H={H}: {tiles} tiles of owned rows, at most {cap} blocks")
    if H == 128:
        assert tiles > cap
    assert hubs_o is not None and int(inv[3]) in hubs_o[1].cpu().tolist()
    assert int(np.diff(hubs_o[2].cpu().numpy()).max()) > 64                           # a hub of more than 64 segments
    own = perm[:n_own]
    Hp = ops.pad4(H)
    x, x0, w = _inputs(n, H, torch.Generator().manual_seed(75 + H))
    m_ref = torch.empty(n, Hp, device=DEV)
    ref = ops.gcn2_conv(x.to(DEV), x0.to(DEV), _mix_matrix(w, BETA).to(DEV), g.csr.rowptr, g.col, g.dinv, n, H, ALPHA, p_drop=0.5,
                        seed=SEED, hubs=g.hubs, m_out=m_ref)
    obuf, mbuf = _rect_call(H, 0.5, x, x0, w, n, n_own, perm, rowptr_o, col_o, hubs_o, dinv_p)
    assert torch.equal(obuf[:n_own], ref[own]) and torch.equal(mbuf[:n_own], m_ref[own])
    assert bool(torch.isnan(obuf[n_own:]).all())
    if Hp > H:
        assert torch.count_nonzero(obuf[:n_own, H:]).item() == 0


# ---- the driver --------------------------------------------------------------------------------------------------
def _gcn2(F_in, C, L, hidden, dropout, seed=0):
    from bridged_gnn_amd.gcn2 import GCN2
    torch.manual_seed(seed)
    return GCN2(types.SimpleNamespace(num_features=F_in, num_classes=C), hidden, L, 0.1, 0.5, dropout=dropout).to(DEV)


@pytest.mark.parametrize("L,hidden", [(1, 64), (4, 64), (2, 132)])
def test_world1_matches_gcn2(L, hidden):
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_gcn2 import PartitionedGCN2
    n = 5000
    ei = _graph(n, 40000, seed=8)
    x = torch.randn(n, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    y = torch.randint(0, 5, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tm = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) < 0.5
    data = Data(x=x, edge_index=_t(ei))
    m = _gcn2(48, 5, L, hidden, 0.5).eval()
    pg = PartitionedGCN2(m, ei, n, 0, 1, DEV)
    own = pg.owned_global
    assert pg.n_halo == 0 and pg.n_local == n
    with torch.no_grad():
        _bar_ok(pg.forward(x[own]).cpu(), m(data)[own].cpu(), ACT_BAR, f"L={L} hidden={hidden} eval forward")
    # one training step with dropout 0.5 (the same host seeds and global-row masks)
    m2 = copy.deepcopy(m).train()
    m.train()
    pg = PartitionedGCN2(m2, ei, n, 0, 1, DEV)
    o1 = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, weight_decay=5e-3)
    torch.manual_seed(11)
    l1 = F.nll_loss(m(data)[tm], y[tm])
    l1.backward()
    torch.manual_seed(11)
    l2 = pg.nll_loss(pg.forward(x[own]), y[own], tm[own])
    l2.backward()
    pg.sync_grads()
    print(f"L={L} hidden={hidden} loss {l1.item():.8f} partitioned {l2.item():.8f}")
    assert abs(l1.item() - l2.item()) <= 2e-6 * abs(l1.item())
    for (k, a), b in zip(m.named_parameters(), m2.parameters()):
        err, top = (a.grad - b.grad).abs().max().item(), a.grad.abs().max().item()
        print(f"L={L} hidden={hidden} {k}: grad err {err / top:.3e} of max")
        assert err <= GRAD_BAR * top, k
    o1.step(); o2.step()
    for (k, a), b in zip(m.named_parameters(), m2.parameters()):
        assert (a - b).abs().max().item() <= 2e-6, k


@pytest.mark.parametrize("world", [2, 4, 8])
def test_simulated_ranks_eval_rows_and_backward_walk_match_single_gpu(world):
    """eval forward of every rank against `GCN2` (L = 4, hidden 64), and the backward's edge walk -- each rank's `ops.gcn_aggregate`
    over the by-source view of t's owned rows, the returned halo rows and the fold, called directly: a barrier inside `backward`
    would block autograd's one device thread -- against the single-GPU A^ t"""
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_gcn2 import PartitionedGCN2, _walk_back
    n_src, n_tar = 4000, 3000
    ei, mask = synth.bridged_graph(n_src, n_tar, 4, 8, 9000, cluster=128, p_local=0.8, seed=world)
    n = n_src + n_tar
    rng = np.random.default_rng(world)
    # node 2: a hub DESTINATION fed from every rank; node 1: a hub SOURCE feeding >= 256 rows of every rank (a halo slot that is a hub
    # of the by-source view on the ranks that do not own it)
    ei = np.concatenate([ei, np.stack([rng.choice(n, 1000, replace=False), np.full(1000, 2)]),
                         np.stack([np.full(3500, 1), rng.choice(n, 3500, replace=False)])], axis=1).astype(np.int64)
    x = torch.randn(n, 40, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world))
    H = 64
    T = torch.randn(n, H, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world + 100))
    m = _gcn2(40, 7, 4, H, 0.5).eval()
    data = Data(x=x, edge_index=_t(ei))
    g = m.graph(data.edge_index, n)
    with torch.no_grad():
        ref = m(data)
        ref_t = ops.gcn_aggregate(T, g.t_rowptr, g.t_dst, g.dinv, n, H, hubs=g.t_hubs)
    for owner in (None, partition_nodes(mask, world)):
        box = _Box(world)
        res, errs = [None] * world, []

        def run(r):
            try:
                pg = PartitionedGCN2(m, ei, n, r, world, DEV, owner=owner)
                pg.comm = _ThreadComm(box, r)
                th = pg.tables.t_hubs
                with torch.no_grad():
                    out = pg.forward(x[pg.owned_global])
                    gx = _walk_back(pg, T[pg.owned_global].contiguous(), H)
                res[r] = (pg.owned_global, out, gx, pg.n_halo, pg.tables.hubs is not None,
                          th is not None and int(th[1].max()) >= pg.n_local)
            except BaseException as e:                     # noqa: BLE001 -- reported below
                errs.append(e)
                box.bar.abort()

        ths = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        if errs:
            raise errs[0]
        torch.cuda.synchronize()
        assert max(r[3] for r in res) > 0, "no halo at all"
        assert sum(r[4] for r in res) >= 1, "the hub destination is a hub on its owner's rank"
        assert sum(r[5] for r in res) >= 1, "no rank holds a halo slot that is a hub source"
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        for r, (own, out, gx, _, _, _) in enumerate(res):
            _bar_ok(out.cpu(), ref[own].cpu(), ACT_BAR, f"world {world} rank {r} forward")
            _bar_ok(gx.cpu(), ref_t[own].cpu(), GRAD_BAR, f"world {world} rank {r} A^ t")
            seen[own] += 1
        assert bool((seen == 1).all()), "every node is covered once"


def test_out_of_scope_raises():
    from bridged_gnn_amd.dist_gcn2 import PartitionedGCN2
    from bridged_gnn_amd.gcn2 import GCN2
    ei = _graph(200, 1000, seed=9)
    with pytest.raises(NotImplementedError, match="graphed"):
        PartitionedGCN2(_gcn2(8, 3, 2, 8, 0.0), ei, 200, 0, 1, DEV, graphed=True)
    with pytest.raises(NotImplementedError):
        PartitionedGCN2(GCN2(types.SimpleNamespace(num_features=8, num_classes=3), 8, 2, 0.1, 0.5, shared_weights=False), ei, 200, 0, 1, DEV)
    with pytest.raises(RuntimeError, match="no CPU"):
        PartitionedGCN2(_gcn2(8, 3, 2, 8, 0.0), ei, 200, 0, 1, "cpu")
    pg = PartitionedGCN2(_gcn2(8, 3, 2, 8, 0.0).eval(), ei, 200, 0, 1, DEV)
    with pytest.raises(RuntimeError, match="no CPU"):
        pg.forward(torch.zeros(200, 8))
    with pytest.raises(ValueError):
        pg(torch.zeros(199, 8, device=DEV))
    # log_softmax is fused into no kernel of this model: more than 128 classes run
    wide = PartitionedGCN2(_gcn2(8, 130, 1, 8, 0.0).eval(), ei, 200, 0, 1, DEV)
    with torch.no_grad():
        assert wide.forward(torch.zeros(200, 8, device=DEV)).shape == (200, 130)


# ---- real ranks (gloo group, one GPU) ---------------------------------------------------------------------------------
OFFICE_L, OFFICE_H = 2, 64


def _layer_outputs(out):
    """the conv outputs y kept by the autograd nodes of `_PartGcn2LayerFn` (ctx.y) / `_Gcn2LayerFn` (saved tensors m, y, M), first
    conv first"""
    ys, seen, stack = [], set(), [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        if "Gcn2LayerFn" in type(fn).__name__:
            ys.append(fn.y if hasattr(fn, "y") else fn.saved_tensors[1])
        stack.extend(f for f, _ in fn.next_functions)
    return ys[::-1]


def _rank_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth, transfer
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_gcn2 import PartitionedGCN2
        from bridged_gnn_amd.gcn2 import GCN2
        res = {}
        # (a) office graph, dropout 0: all-reduced loss and gradients, and this rank's ReLU patterns (x0 and every conv's y; compared
        #     in the parent with the fp64 restatement on those patterns)
        data = _office_data()
        n = data.x.shape[0]
        torch.manual_seed(0)
        m = GCN2(transfer.pyg_dataset(data), OFFICE_H, OFFICE_L, 0.1, 0.5, dropout=0.0).to(DEV).train()
        pg = PartitionedGCN2(m, data.edge_index.cpu().numpy(), n, rank, world, DEV)
        own = pg.owned_global
        seen = []
        hook = m.lins[0].register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))
        out = pg.forward(data.x[own])
        hook.remove()
        ys = _layer_outputs(out)
        assert len(ys) == OFFICE_L
        loss = pg.nll_loss(out, data.y[own], data.train_mask[own])
        loss.backward()
        pg.sync_grads()
        tot = loss.detach().double().cpu().reshape(1)
        dist.all_reduce(tot)
        res["office"] = (float(tot), {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()}, own.cpu().numpy(),
                         (seen[0] > 0).cpu().numpy(), [(y[:, :OFFICE_H] > 0).cpu().numpy() for y in ys], pg.n_halo)
        # (b) synth graph, dropout 0.5: three Adam steps against the single-GPU steps, then the same steps again
        n = 6000
        ei, _ = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        ei = np.concatenate([ei, ei[:, :500], np.stack([np.arange(0, n, 11)] * 2)], axis=1)   # duplicates + self loops
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, 5, (n,), device=DEV, generator=g)
        tm = torch.rand(n, device=DEV, generator=g) < 0.5
        data = Data(x=x, edge_index=_t(ei))
        torch.manual_seed(0)
        m0 = GCN2(types.SimpleNamespace(num_features=64, num_classes=5), 64, 4, 0.1, 0.5, dropout=0.5).to(DEV).train()
        ref_m, runs = copy.deepcopy(m0), []

        def single():
            lp = ref_m(data)
            loss = F.nll_loss(lp[tm], y[tm])
            loss.backward()
            return float(loss.detach())
        ref_rec, ref_par = _steps(ref_m, single)
        for _ in range(2):
            m = copy.deepcopy(m0)
            pg = PartitionedGCN2(m, ei, n, rank, world, DEV)
            own = pg.owned_global
            xl = x[own].contiguous()

            def part():
                loss = pg.nll_loss(pg.forward(xl), y[own], tm[own])
                loss.backward()
                pg.sync_grads()
                tot = loss.detach().double().cpu().reshape(1)
                dist.all_reduce(tot)
                return float(tot)
            runs.append(_steps(m, part))
        # the kept patterns of the first step's forward, this rank's rows against the single-GPU run's (printed by the parent)
        torch.manual_seed(100)
        ya = _layer_outputs(copy.deepcopy(m0)(data))
        torch.manual_seed(100)
        pf = PartitionedGCN2(copy.deepcopy(m0), ei, n, rank, world, DEV)
        yb = _layer_outputs(pf.forward(xl))
        flips = [int(((a[own][:, :64] > 0) != (b[:, :64] > 0)).sum()) for a, b in zip(ya, yb)]
        w = {"loss": 0.0, "param": 0.0, "param_of": "", "grad": 0.0, "grad_of": "", "repeat": True, "flips": flips}
        for (lr_, gr), (lp, gp) in zip(ref_rec, runs[0][0]):
            w["loss"] = max(w["loss"], abs(lp - lr_) / abs(lr_))
            for k in gr:
                e = float((gp[k] - gr[k]).abs().max()) / float(gr[k].abs().max())
                if e > w["grad"]:
                    w["grad"], w["grad_of"] = e, k
        for k in ref_par:                                   # in units of the bar: ADAM_BAR * max|ref| + 1e-6 (test_gpu_gcn._bar_ok)
            e = float((runs[0][1][k] - ref_par[k]).abs().max()) / (ADAM_BAR * float(ref_par[k].abs().max()) + 1e-6)
            if e > w["param"]:
                w["param"], w["param_of"] = e, k
        (r1, p1), (r2, p2) = runs
        w["repeat"] = (all(a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1]) for a, b in zip(r1, r2))
                       and all(torch.equal(p1[k], p2[k]) for k in p1))
        res["synth"], res["summary"] = w, {"n_halo": pg.n_halo, "n_local": pg.n_local}
        q.put((rank, res))
    except Exception:                                            # report instead of leaving the parent waiting for the queue
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_real_ranks_train_gcn2(world):
    import queue
    import socket
    import torch.multiprocessing as mp
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.gcn2 import GCN2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            rank, r = q.get(timeout=300)                    # the one wait: a rank that does not report ends the test
            res[rank] = r
    except queue.Empty:
        pass
    for p in procs:
        p.join(timeout=30 if len(res) == world else 0)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    for r in sorted(res):
        assert "error" not in res[r], res[r]["error"]
    assert len(res) == world and codes == [0] * world, f"ranks reported: {sorted(res)}, exit codes: {codes}"
    for r in range(world):
        print(r, res[r]["synth"], res[r]["summary"])
        assert res[r]["summary"]["n_halo"] > 0
    # (a) office: the all-reduced loss and gradients against the fp64 restatement on the ranks' own ReLU patterns
    data = _office_data()
    n = data.x.shape[0]
    parts = _sparse_parts(data.edge_index.cpu(), n)
    torch.manual_seed(0)
    ref_m = GCN2(transfer.pyg_dataset(data), OFFICE_H, OFFICE_L, 0.1, 0.5)
    P = _params64(ref_m)
    betas = [c.beta for c in ref_m.convs]
    x64, y, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    relu0 = torch.zeros(n, OFFICE_H, dtype=torch.float64)
    relus = [torch.zeros(n, OFFICE_H, dtype=torch.float64) for _ in range(OFFICE_L)]
    cover = np.zeros(n, dtype=np.int64)
    for r in range(world):
        _, _, own, pat0, pats, _ = res[r]["office"]
        relu0[torch.from_numpy(own)] = torch.from_numpy(pat0.astype(np.float64))
        for l in range(OFFICE_L):
            relus[l][torch.from_numpy(own)] = torch.from_numpy(pats[l].astype(np.float64))
        cover[own] += 1
    assert (cover == 1).all() and sum(res[r]["office"][5] for r in range(world)) > 0
    loss, grads = res[0]["office"][:2]
    for r in range(1, world):                               # every rank holds the same all-reduced gradients
        assert all(np.array_equal(grads[k], res[r]["office"][1][k]) for k in grads)
    one = torch.ones((), dtype=torch.float64)
    ref_loss = F.nll_loss(_model64(P, OFFICE_L, 0.1, betas, x64, parts, masks=(one, relu0, one, relus))[tm], y[tm])
    ref = dict(zip(P, torch.autograd.grad(ref_loss, list(P.values()))))
    print(f"office: loss {loss:.8f} fp64 {ref_loss.item():.8f}")
    assert abs(loss - ref_loss.item()) <= LOSS_BAR * abs(ref_loss.item())
    for k in ref:
        _bar_ok(grads[k], ref[k].numpy(), GRAD_BAR, f"office grad {k}")
    # (b) synth, dropout 0.5: three Adam steps against the single-GPU steps; a repeated run is bitwise equal
    for r in range(world):
        w = res[r]["synth"]
        print(f"rank {r}: elements whose (y > 0) differs from the single-GPU forward, per conv: {w['flips']}")
        assert w["loss"] <= LOSS_BAR and w["grad"] <= GRAD_BAR and w["param"] <= 1.0, (r, w)
        assert w["repeat"], (r, "two identical runs differ")
