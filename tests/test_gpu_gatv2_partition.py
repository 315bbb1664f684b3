"""GPU: GATv2 on a destination-node partition (bridged_gnn_amd.dist_gatv2) -- the global-position dropout hashes of the one-pass
attention conv (`row_ids` for the feature mask, `edge_base` for the attention mask) in the forward and in the backward that
redraws them, and the backward over more sources than rows (n_src = n_ext > n_rows = n_local): identity ids against the plain
entries, renumbered rows, and every rank's extended graph of a 3-way partition against the whole-graph call; the entries'
argument checks; world 1 against the single-GPU model; simulated worlds 2/4/8 in one process (ranks as threads, the exchange by
row copies); and REAL ranks in a gloo group sharing the GPU (payload staged through the host, kernels the production ones):
gradients against the reference's fp64 gradients on the office graph, and three Adam steps with dropout 0.6 / 0.5 against the
single-GPU steps, twice, the second run bitwise the first.
Bars: those of test_gpu_gatv2.py (activations 1e-5 of the tensor's max + 1e-6, gradients 2e-5 of the max, LeakyReLU-kink cap 2e-4,
Adam losses and parameters 1e-4).  A partitioned step differs from the single-GPU one only in the order of some fp32 sums (the
by-source pass, the blocks' partial rows of grad_att, the gradient return, dW and db).
The kernel tests run on a graph of 300 nodes: a hub row (node 3, > 200 in-edges: several passes of a lane group, which takes at
most 32 edges per pass), a hub source (node 5), duplicate edges, input self loops and a node whose only edge is its self loop."""
import copy
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_gatv2 as G1
from test_gatv2_host import OFFICE_MODELS, edge_list, params64
from test_gpu_gcn_partition import _Box, _ThreadComm, _steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_BAR, GRAD_BAR, KINK_CAP = G1.ACT_BAR, G1.GRAD_BAR, G1.KINK_CAP      # 1e-5, 2e-5, 2e-4
ADAM_BAR, LOSS_BAR = 1e-4, 1e-4                                         # test_gpu_gatv2.py's Adam bars (parameters, losses)
OFFICE_LOSS_BAR = 1e-5                                                  # its bar on the fixture's loss
SHAPES = ((1, 2), (1, 31), (3, 8), (3, 64), (8, 16))
N, HUB = 300, 200
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -3                                # include/bgnn.h


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _edges():
    rng = np.random.default_rng(5)
    m = N - 1                                                            # node N-1 takes part in no edge but its own loop
    ei = np.stack([rng.integers(0, m, 2400), rng.integers(0, m, 2400)])
    loops = np.concatenate([np.arange(0, m, 7), [N - 1]])
    return np.concatenate([ei, ei[:, :120],                               # duplicates
                           np.stack([rng.integers(0, m, HUB), np.full(HUB, 3)]),        # node 3: a hub row
                           np.stack([np.full(HUB, 5), rng.integers(0, m, HUB)]),        # node 5: a hub source
                           np.stack([loops, loops])], axis=1).astype(np.int64)


_CACHE = {}


def _graph():
    """the kernel tests' graph, built once: (edge list, test_gpu_gatv2._G of it)"""
    if "g" not in _CACHE:
        ei = _edges()
        G = G1._G(ei, N)
        assert G.indeg[3] >= HUB > 32 and G.outdeg[5] >= HUB and G.indeg[N - 1] == 0 and G.outdeg[N - 1] == 0
        pairs = ei[0] * N + ei[1]
        assert np.unique(pairs).shape[0] < pairs.shape[0], "duplicate edges"
        _CACHE["g"] = (ei, G)
    return _CACHE["g"]


def _settings(H):
    """(p_att, epilogue, p_drop): attention dropout off / on crossed with the ELU epilogue without / with feature dropout, and the
    log_softmax epilogue where it exists (one head)"""
    out = [(pa, "elu", pd) for pa in (0.0, 0.6) for pd in (0.0, 0.6)]
    if H == 1:
        out += [(0.0, "log_softmax", 0.0), (0.6, "log_softmax", 0.0)]
    return out


def _fwd(T, att, b, rowptr, col, n_rows, H, C, p_att, epi, p_drop, **ids):
    """-> (out, state, pre, alpha)"""
    from bridged_gnn_amd import ops
    return ops.gatv2_aggregate(T, att, rowptr, col, n_rows, H, C, bias=b, p_att=p_att, seed_att=1234, epilogue=epi, p_drop=p_drop,
                               seed=99, want_pre=True, return_alpha=True, **ids)


def _bwd(T, att, kept, dy, rowptr, col, tr, H, C, b, p_att, epi, p_drop, **kw):
    """-> (grad_tbl, grad_att, grad_bias)"""
    from bridged_gnn_amd import ops
    _, state, pre, _ = kept
    return ops.gatv2_aggregate_bwd(T, att, state, pre, dy, rowptr, col, tr[0], tr[1], tr[2], H, C, bias=b, p_att=p_att,
                                   seed_att=1234, epilogue=epi, p_drop=p_drop, seed=99, **kw)


def _bwd_raw(T, att, kept, dy, rowptr, col, tr, n_src, n_rows, H, C, b, p_att, epi, p_drop, row_ids=None, edge_base=None,
             ws_bytes=None):
    """bgnn_gatv2_aggregate_bwd_f32 itself, on outputs pre-filled with NaN -> (return code, g, grad_tbl, grad_att)"""
    from bridged_gnn_amd import _lib as L
    from bridged_gnn_amd import ops
    _, state, pre, _ = kept
    P, E = ops.pad4(H * C), int(col.shape[0])
    nan = float("nan")
    g = torch.full((max(n_rows, 1), P), nan, device=DEV)
    gt = torch.full((max(n_src, 1), 2 * P), nan, device=DEV)
    ga = torch.full((H * C,), nan, device=DEV)
    need = int(L.lib().bgnn_gatv2_aggregate_workspace_bytes(E, n_rows, H, C))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    rc = L.lib().bgnn_gatv2_aggregate_bwd_f32(
        L.ptr_rows(T), T.stride(0), n_src, L.ptr(att.reshape(-1)), L.ptr(b), L.ptr(state), L.ptr_rows(pre), pre.stride(0),
        L.ptr_rows(dy), dy.stride(0), L.ptr(rowptr), L.ptr(col), L.ptr(tr[0]), L.ptr(tr[1]), L.ptr(tr[2]), E, n_rows, H, C, 0.2,
        float(p_att), 1234, None, ops.GAT_EPILOGUES[epi], float(p_drop), 99, None, L.ptr(ws), need if ws_bytes is None else ws_bytes,
        L.ptr(row_ids), L.ptr(edge_base), L.ptr_rows(g), g.stride(0), L.ptr_rows(gt), gt.stride(0), L.ptr(ga), L.stream())
    return rc, g, gt, ga


def _pads_zero(t, HC, P):
    """the pad columns H*C .. P of every P-wide half of t are exactly 0"""
    return all(torch.count_nonzero(t[:, o + HC:o + P]).item() == 0 for o in range(0, t.shape[1], P))


# ---- kernel: identity ids ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", SHAPES)
def test_identity_ids_are_the_plain_kernels(H, C):
    """row_ids = arange(n) and edge_base = rowptr[:-1] name the positions the plain entries hash: bitwise the plain call, forward
    (out, state, pre, alpha) and backward (grad_tbl, grad_att, grad_bias); pad columns 0"""
    from bridged_gnn_amd import ops
    _, G = _graph()
    g, n, HC, P = G.g, G.n, H * C, ops.pad4(H * C)
    T, att, b, dy = (t.to(DEV) for t in G1._inputs(n, H, C, seed=40 + H * 131 + C))
    ids = dict(row_ids=torch.arange(n, dtype=torch.int64, device=DEV), edge_base=g.rowptr[:-1].long().contiguous())
    tr = (g.t_rowptr, g.t_eid, g.t_dst)
    for p_att, epi, p_drop in _settings(H):
        tag = f"H={H} C={C} p_att={p_att} epi={epi} p_drop={p_drop}"
        plain = _fwd(T, att, b, g.rowptr, g.col, n, H, C, p_att, epi, p_drop)
        got = _fwd(T, att, b, g.rowptr, g.col, n, H, C, p_att, epi, p_drop, **ids)
        assert all(torch.equal(x, y) for x, y in zip(plain, got)), tag + ": forward"
        assert _pads_zero(got[0], HC, P) and _pads_zero(got[2], HC, P), tag + ": pad columns"
        if p_att > 0:
            assert bool((got[3] == 0).any()), tag + ": the attention mask drops something"
        bp = _bwd(T, att, plain, dy, g.rowptr, g.col, tr, H, C, b, p_att, epi, p_drop)
        bg = _bwd(T, att, plain, dy, g.rowptr, g.col, tr, H, C, b, p_att, epi, p_drop, n_rows=n, **ids)
        assert all(torch.equal(x, y) for x, y in zip(bp, bg)), tag + ": backward"
        assert _pads_zero(bg[0], HC, P), tag + ": pad columns of grad_tbl"


# ---- kernel: renumbered rows -------------------------------------------------------------------------------------------
def _permuted():
    """the graph with its nodes renumbered (new node i = old node perm[i]; every row keeps its edge order)"""
    if "perm" not in _CACHE:
        from bridged_gnn_amd import ops
        _, G = _graph()
        n = G.n
        rp, colc = G.g.rowptr.long().cpu(), G.g.col.long().cpu()
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(4))
        inv = torch.empty(n, dtype=torch.int64)
        inv[perm] = torch.arange(n)
        deg = (rp[1:] - rp[:-1])[perm]
        rowptr_p = torch.zeros(n + 1, dtype=torch.int64)
        rowptr_p[1:] = torch.cumsum(deg, 0)
        pos = torch.repeat_interleave(rp[perm] - rowptr_p[:-1], deg) + torch.arange(int(rowptr_p[-1]))   # position in the original CSR
        col_p = inv[colc[pos]]
        rowptr_d, col_d = rowptr_p.to(torch.int32).to(DEV), col_p.to(torch.int32).to(DEV)
        csr = ops.DstCSR(rowptr_d, col_d, None, int(col_d.shape[0]), n)
        _CACHE["perm"] = dict(perm=perm.to(DEV), pos=pos.to(DEV), rowptr=rowptr_d, col=col_d, tr=csr.transposed(),
                              edge_base=rp[perm].contiguous().to(DEV))
    return _CACHE["perm"]


@pytest.mark.parametrize("H,C", SHAPES)
def test_ids_carry_both_masks_to_renumbered_rows(H, C):
    """renumbered nodes with row_ids = perm and edge_base = rowptr_original[perm] give bitwise the rows of the original call (out,
    state, pre, every row's coefficients: both masks are recovered equal) and, in the backward, bitwise the x_r half of grad_tbl
    (a row's own sum over its edges in their order); the by-source sums, the blocks' partial rows of grad_att and the column sums
    change their order: gradient bar.  Without the ids the renumbered call draws other masks."""
    from bridged_gnn_amd import ops
    _, G = _graph()
    g, n, HC, P = G.g, G.n, H * C, ops.pad4(H * C)
    Q = _permuted()
    perm, pos = Q["perm"], Q["pos"]
    T, att, b, dy = (t.to(DEV) for t in G1._inputs(n, H, C, seed=70 + H * 131 + C))
    Tp, dyp = T[perm].contiguous(), dy[perm].contiguous()
    ids = dict(row_ids=perm, edge_base=Q["edge_base"])
    for p_att, epi, p_drop in _settings(H):
        tag = f"permuted H={H} C={C} p_att={p_att} epi={epi} p_drop={p_drop}"
        ref = _fwd(T, att, b, g.rowptr, g.col, n, H, C, p_att, epi, p_drop)
        got = _fwd(Tp, att, b, Q["rowptr"], Q["col"], n, H, C, p_att, epi, p_drop, **ids)
        for x, y, what in zip(got[:3], ref[:3], ("out", "state", "pre")):
            assert torch.equal(x, y[perm]), f"{tag}: {what}"
        assert torch.equal(got[3], ref[3][pos]), tag + ": coefficients"
        assert torch.equal(got[3] == 0, ref[3][pos] == 0) and torch.equal(got[0] == 0, ref[0][perm] == 0), tag + ": masks"
        assert _pads_zero(got[0], HC, P)
        plain = _fwd(Tp, att, b, Q["rowptr"], Q["col"], n, H, C, p_att, epi, p_drop)
        if p_att > 0:
            assert bool((got[3] == 0).any()) and not torch.equal(plain[3], ref[3][pos]), tag + ": local positions draw another mask"
        if p_drop > 0:
            assert bool((got[0][:, :HC] == 0).any()) and not torch.equal(plain[0], ref[0][perm]), tag
        rb = _bwd(T, att, ref, dy, g.rowptr, g.col, (g.t_rowptr, g.t_eid, g.t_dst), H, C, b, p_att, epi, p_drop)
        gb = _bwd(Tp, att, got, dyp, Q["rowptr"], Q["col"], Q["tr"], H, C, b, p_att, epi, p_drop, n_rows=n, **ids)
        assert torch.equal(gb[0][:, P:], rb[0][perm][:, P:]), tag + ": the x_r half of grad_tbl"
        assert _pads_zero(gb[0], HC, P)
        G1._grad_ok(gb[0][:, :P].cpu(), rb[0][perm][:, :P].cpu(), tag + " grad_tbl, x_l half")
        G1._grad_ok(gb[1].cpu(), rb[1].cpu(), tag + " grad_att")
        G1._grad_ok(gb[2].cpu(), rb[2].cpu(), tag + " grad_bias")


# ---- kernel: the extended graphs of a partition ----------------------------------------------------------------------
@pytest.mark.parametrize("H,C", SHAPES)
def test_extended_graphs_of_a_partition_match_the_whole_graph(H, C):
    """every rank of a 3-way partition runs forward and backward over its extended graph (n_src = n_ext > n_rows = n_local in the
    backward) on rows of T and grad_y picked by global id -- no communication; the x_r half of the halo rows of T is NaN (never
    read).  Forward rows bitwise the whole-graph call's; g and the x_r half of grad_tbl of the owned rows bitwise; the x_l half
    and grad_att, summed over the ranks by global id, within the gradient bar; rows n_rows .. n_src of the x_r half and every pad
    column exactly 0 in outputs that were NaN before the call; two identical calls bitwise equal."""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.dist_gat import GatPartition, _GatTables
    ei, G = _graph()
    g, n, HC, P = G.g, G.n, H * C, ops.pad4(H * C)
    T, att, b, dy = (t.to(DEV) for t in G1._inputs(n, H, C, seed=90 + H * 131 + C))
    tr = (g.t_rowptr, g.t_eid, g.t_dst)
    if "parts" not in _CACHE:
        parts = [GatPartition(ei, n, r, 3) for r in range(3)]
        _CACHE["parts"] = [(p, _GatTables(p, DEV)) for p in parts]
    assert sum(p.n_halo for p, _ in _CACHE["parts"]) > 0
    for p_att, epi, p_drop in _settings(H):
        tag = f"extended H={H} C={C} p_att={p_att} epi={epi} p_drop={p_drop}"
        ref = _fwd(T, att, b, g.rowptr, g.col, n, H, C, p_att, epi, p_drop)
        rc, g_ref, gt_ref, ga_ref = _bwd_raw(T, att, ref, dy, g.rowptr, g.col, tr, n, n, H, C, b, p_att, epi, p_drop)
        assert rc == 0
        rb = _bwd(T, att, ref, dy, g.rowptr, g.col, tr, H, C, b, p_att, epi, p_drop)
        assert torch.equal(gt_ref, rb[0]) and torch.equal(ga_ref, rb[1]), tag + ": without ids and halo the raw call is the wrapper's"
        dxl = torch.zeros(n, P, dtype=torch.float64, device=DEV)
        datt = torch.zeros(HC, dtype=torch.float64, device=DEV)
        for part, tb in _CACHE["parts"]:
            r, nl, ne = part.rank, part.n_local, part.n_ext
            ext, own = _t(part.ext_global()), tb.owned_global
            ids = dict(row_ids=own, edge_base=tb.edge_base)
            Te, dyo = T[ext].contiguous(), dy[own].contiguous()
            Te[nl:, P:] = float("nan")
            got = _fwd(Te, att, b, tb.rowptr_local, tb.col, nl, H, C, p_att, epi, p_drop, **ids)
            for x, y, what in zip(got[:3], ref[:3], ("out", "state", "pre")):
                assert torch.equal(x, y[own]), f"{tag} rank {r}: {what}"
            rpl = tb.rowptr_local.long()
            deg = rpl[1:] - rpl[:-1]
            pos = torch.repeat_interleave(tb.edge_base - rpl[:-1], deg) + torch.arange(part.num_edges, device=DEV)
            assert torch.equal(got[3], ref[3][pos]), f"{tag} rank {r}: coefficients"
            trl = (tb.t_rowptr, tb.t_eid, tb.t_dst)
            rc, g_r, gt, ga = _bwd_raw(Te, att, got, dyo, tb.rowptr_local, tb.col, trl, ne, nl, H, C, b, p_att, epi, p_drop, **ids)
            assert rc == 0
            assert torch.equal(g_r, g_ref[own]), f"{tag} rank {r}: g"
            assert torch.equal(gt[:nl, P:], gt_ref[own][:, P:]), f"{tag} rank {r}: the x_r half of the owned rows"
            assert torch.count_nonzero(gt[nl:, P:]).item() == 0, f"{tag} rank {r}: the x_r half of the halo rows"
            assert _pads_zero(gt, HC, P) and _pads_zero(g_r, HC, P), f"{tag} rank {r}: pad columns"
            assert bool(torch.isfinite(gt).all()) and bool(torch.isfinite(ga).all())
            again = _bwd_raw(Te, att, got, dyo, tb.rowptr_local, tb.col, trl, ne, nl, H, C, b, p_att, epi, p_drop, **ids)
            assert torch.equal(again[1], g_r) and torch.equal(again[2], gt) and torch.equal(again[3], ga), f"{tag} rank {r}: repeat"
            w = _bwd(Te, att, got, dyo, tb.rowptr_local, tb.col, trl, H, C, b, p_att, epi, p_drop, n_rows=nl, **ids)
            assert w[0].shape == (ne, 2 * P) and torch.equal(w[0], gt) and torch.equal(w[1], ga), f"{tag} rank {r}: the wrapper"
            dxl.index_add_(0, ext, gt[:, :P].double())
            datt += ga.double()
        G1._grad_ok(dxl.cpu(), gt_ref[:, :P].cpu(), tag + " grad_tbl, x_l half over the ranks")
        G1._grad_ok(datt.cpu(), ga_ref.cpu(), tag + " grad_att over the ranks")


# ---- kernel: argument checks -------------------------------------------------------------------------------------------
def test_rows_entries_refuse_inconsistent_arguments():
    """n_src < n_rows, an id array of the wrong length or alone, and a short workspace are refused before any launch"""
    from bridged_gnn_amd import _lib as L
    from bridged_gnn_amd import ops
    _, G = _graph()
    g, n, H, C = G.g, G.n, 3, 8
    T, att, b, dy = (t.to(DEV) for t in G1._inputs(n, H, C, seed=5))
    tr = (g.t_rowptr, g.t_eid, g.t_dst)
    ids = dict(row_ids=torch.arange(n, dtype=torch.int64, device=DEV), edge_base=g.rowptr[:-1].long().contiguous())
    kept = _fwd(T, att, b, g.rowptr, g.col, n, H, C, 0.6, "elu", 0.6, **ids)
    need = int(L.lib().bgnn_gatv2_aggregate_workspace_bytes(int(g.col.shape[0]), n, H, C))
    args = (T, att, kept, dy, g.rowptr, g.col, tr)
    assert _bwd_raw(*args, n - 1, n, H, C, b, 0.6, "elu", 0.6, **ids)[0] == E_SHAPE, "n_src < n_rows"
    assert _bwd_raw(*args, n, n, H, C, b, 0.6, "elu", 0.6, ws_bytes=need - 1, **ids)[0] == E_WORKSPACE
    assert _bwd_raw(*args, n, n, H, C, b, 0.6, "elu", 0.6, row_ids=ids["row_ids"])[0] == E_NULL, "one id array alone"
    assert _bwd_raw(*args, n, n, H, C, b, 0.6, "elu", 0.6, **ids)[0] == 0
    torch.cuda.synchronize()
    short = dict(row_ids=ids["row_ids"][:n - 1].contiguous(), edge_base=ids["edge_base"])
    with pytest.raises(ValueError, match="row_ids must be"):
        _fwd(T, att, b, g.rowptr, g.col, n, H, C, 0.6, "elu", 0.6, **short)
    with pytest.raises(ValueError, match="row_ids must be"):
        _bwd(*args, H, C, b, 0.6, "elu", 0.6, **short)
    with pytest.raises(ValueError, match="edge_base must be"):
        _bwd(*args, H, C, b, 0.6, "elu", 0.6, row_ids=ids["row_ids"], edge_base=ids["edge_base"].int())
    with pytest.raises(ValueError, match="together"):
        _fwd(T, att, b, g.rowptr, g.col, n, H, C, 0.6, "elu", 0.6, edge_base=ids["edge_base"])
    with pytest.raises(ValueError, match="on the table's device"):
        _fwd(T, att, b, g.rowptr, g.col, n, H, C, 0.6, "elu", 0.6, row_ids=ids["row_ids"].cpu(), edge_base=ids["edge_base"].cpu())
    with pytest.raises(ValueError, match="n_rows = "):
        _bwd(*args, H, C, b, 0.6, "elu", 0.6, n_rows=n + 1)
    with pytest.raises(ValueError, match="state must be"):          # n_rows < N: state, pre and grad_y are over n_rows
        _bwd(*args, H, C, b, 0.6, "elu", 0.6, n_rows=n - 1)


# ---- the driver ------------------------------------------------------------------------------------------------------
def _gatv2(F_in, C, hidden, layers, heads, dropout=0.6, att_dropout=0.5, seed=0):
    from bridged_gnn_amd.gatv2 import GATv2
    torch.manual_seed(seed)
    return GATv2(F_in, hidden, C, layers, heads, dropout, att_dropout).to(DEV)


def _model_graph(n, e, seed):
    from bridged_gnn_amd import synth
    ei, _ = synth.random_multigraph(n, e, n_isolated=max(n // 50, 1), seed=seed)
    loops = np.arange(0, n, 7)
    return np.concatenate([ei, ei[:, : e // 20], np.stack([loops, loops])], axis=1).astype(np.int64)


@pytest.mark.parametrize("layers,heads", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_world1_matches_gatv2(layers, heads):
    """one rank owning every row: the eval forward, the training forward at dropout 0.6 / 0.5 from the same host seeds, and the
    gradients of one step, against `gatv2.GATv2`"""
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_gatv2 import PartitionedGATv2
    n = 2000
    ei = _model_graph(n, 16000, seed=8)
    x = torch.randn(n, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    y = torch.randint(0, 5, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tm = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) < 0.5
    data = Data(x=x, edge_index=_t(ei))
    m = _gatv2(48, 5, 16, layers, heads).eval()
    pg = PartitionedGATv2(m, ei, n, 0, 1, DEV)
    own = pg.owned_global
    assert pg.n_halo == 0 and pg.n_local == n and len(m.convs) == layers
    with torch.no_grad():
        G1._act_ok(pg.forward(x[own]).cpu(), m(data)[own].cpu(), "world 1 eval forward")
    m2 = copy.deepcopy(m).train()
    m.train()
    pg = PartitionedGATv2(m2, ei, n, 0, 1, DEV)
    torch.manual_seed(11)
    o1 = m(data)
    l1 = F.nll_loss(o1[tm], y[tm])
    l1.backward()
    torch.manual_seed(11)
    o2 = pg.forward(x[own])
    l2 = pg.nll_loss(o2, y[own], tm[own])
    l2.backward()
    pg.sync_grads()
    G1._act_ok(o2.detach().cpu(), o1.detach()[own].cpu(), "world 1 training forward")
    print(f"loss {l1.item():.8f} partitioned {l2.item():.8f}")
    assert abs(l1.item() - l2.item()) <= LOSS_BAR * abs(l1.item())
    named = {k: p for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(named) == sorted(k for k, p in m2.named_parameters() if p.grad is not None)
    assert sorted(named) == sorted(k for k, _ in m.named_parameters() if not k.startswith("bns.")), "every conv tensor, no BatchNorm"
    other = dict(m2.named_parameters())
    for k, a in named.items():
        G1._grad_ok(other[k].grad.cpu(), a.grad.cpu(), f"world 1 grad {k}")


def _bridged(world):
    """`synth.bridged_graph` at the size tests/test_gpu_gat_partition.py uses, with a hub destination fed from every rank (node 2)
    and a hub source feeding rows of every rank (node 1: a halo slot elsewhere)"""
    from bridged_gnn_amd import synth
    n_src, n_tar = 4000, 3000
    ei, mask = synth.bridged_graph(n_src, n_tar, 4, 8, 9000, cluster=128, p_local=0.8, seed=world)
    n = n_src + n_tar
    rng = np.random.default_rng(world)
    ei = np.concatenate([ei, np.stack([rng.choice(n, 1000, replace=False), np.full(1000, 2)]),
                         np.stack([np.full(3500, 1), rng.choice(n, 3500, replace=False)])], axis=1).astype(np.int64)
    return ei, mask, n


@pytest.mark.parametrize("world", [2, 4, 8])
def test_simulated_ranks_eval_rows_match_single_gpu(world):
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_gatv2 import PartitionedGATv2
    ei, mask, n = _bridged(world)
    x = torch.randn(n, 40, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world))
    m = _gatv2(40, 7, 16, 3, 3).eval()
    data = Data(x=x, edge_index=_t(ei))
    with torch.no_grad():
        ref = m(data)
    for owner in (None, partition_nodes(mask, world)):
        box = _Box(world)
        res, errs = [None] * world, []

        def run(r):
            try:
                pg = PartitionedGATv2(m, ei, n, r, world, DEV, owner=owner)
                pg.comm = _ThreadComm(box, r)
                with torch.no_grad():
                    res[r] = (pg.owned_global, pg.forward(x[pg.owned_global]), pg.n_halo)
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
        assert sum(r[2] for r in res) > 0, "no halo at all"
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        for r, (own, out, _) in enumerate(res):
            G1._act_ok(out.cpu(), ref[own].cpu(), f"world {world} rank {r} forward")
            seen[own] += 1
        assert bool((seen == 1).all()), "every node is covered once"


def test_out_of_scope_raises():
    from bridged_gnn_amd.dist_gatv2 import PartitionedGATv2
    ei = _model_graph(200, 1000, seed=9)
    pg = PartitionedGATv2(_gatv2(8, 3, 8, 2, 2, 0.0, 0.0).eval(), ei, 200, 0, 1, DEV)
    with pytest.raises(RuntimeError, match="no CPU"):
        pg.forward(torch.zeros(200, 8))
    with pytest.raises(ValueError):
        pg.forward(torch.zeros(199, 8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU"):
        PartitionedGATv2(_gatv2(8, 3, 8, 2, 2, 0.0, 0.0), ei, 200, 0, 1, "cpu")
    with pytest.raises(RuntimeError, match="GATv2Conv: unsupported shape"):
        PartitionedGATv2(_gatv2(8, 3, 8, 2, 9, 0.0, 0.0), ei, 200, 0, 1, DEV)
    assert not hasattr(pg, "get_emb")


# ---- real ranks (gloo group, one GPU) ---------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_gatv2 import PartitionedGATv2
        res = {"office": {}, "summary": None}
        # (1) office graph, no dropout (eval mode, gradients enabled: as test_gpu_gatv2.test_gradients_match_reference): all-reduced
        # gradients, compared in the parent with the reference's fp64 gradients
        for variant in ("raw", "und"):
            data, tm, dims, fx, _ = G1._case("office", variant)
            ei = data.edge_index.cpu().numpy()
            n = data.x.shape[0]
            for name, hidden, heads, layers, seed in OFFICE_MODELS:
                m = G1._model(dims, fx, name, hidden, heads, layers, seed)
                pg = PartitionedGATv2(m, ei, n, rank, world, DEV)
                own = pg.owned_global
                loss = pg.nll_loss(pg.forward(data.x[own]), data.y[own], tm[own])
                loss.backward()
                pg.sync_grads()
                tot = loss.detach().double().cpu().reshape(1)
                dist.all_reduce(tot)
                res["office"][f"{variant}/{name}"] = (float(tot), {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()
                                                                   if p.grad is not None})
        # (2) synth graph, dropout 0.6 / 0.5: three Adam steps against the single-GPU steps, then the same steps again
        n = 6000
        ei, mask = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        ei = np.concatenate([ei, ei[:, :500], np.stack([np.arange(0, n, 11)] * 2)], axis=1)   # duplicates + self loops
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, 5, (n,), device=DEV, generator=g)
        tm = torch.rand(n, device=DEV, generator=g) < 0.5
        data = Data(x=x, edge_index=_t(ei))
        m0 = _gatv2(64, 5, 32, 3, 3, 0.6, 0.5).train()
        ref_m, runs = copy.deepcopy(m0), []

        def single():
            loss = F.nll_loss(ref_m(data)[tm], y[tm])
            loss.backward()
            return float(loss.detach())
        ref_rec, ref_par = _steps(ref_m.convs, single)       # the convs hold every trained tensor: bns.* never gets a gradient
        for _ in range(2):
            m = copy.deepcopy(m0)
            pg = PartitionedGATv2(m, ei, n, rank, world, DEV)
            own = pg.owned_global
            xl = x[own].contiguous()                        # one tensor: its halo rows are fetched once

            def part():
                loss = pg.nll_loss(pg.forward(xl), y[own], tm[own])
                loss.backward()
                pg.sync_grads()
                assert all(p.grad is None for p in m.bns.parameters())
                tot = loss.detach().double().cpu().reshape(1)
                dist.all_reduce(tot)
                return float(tot)
            runs.append(_steps(m.convs, part))
        w = {"loss": 0.0, "param": 0.0, "param_of": "", "grad": 0.0, "grad_of": "", "repeat": True}
        for (lr_, gr), (lp, gp) in zip(ref_rec, runs[0][0]):
            w["loss"] = max(w["loss"], abs(lp - lr_) / abs(lr_))
            for k in gr:
                e = float((gp[k] - gr[k]).abs().max()) / float(gr[k].abs().max())
                if e > w["grad"]:
                    w["grad"], w["grad_of"] = e, k
        for k in ref_par:                                   # in units of the bar: ADAM_BAR * max|ref|
            e = float((runs[0][1][k] - ref_par[k]).abs().max()) / (ADAM_BAR * float(ref_par[k].abs().max()))
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
def test_real_ranks_train_gatv2(world):
    import queue
    import socket
    import torch.multiprocessing as mp
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
    # (1) office: the all-reduced loss and gradients against the reference's fp64 fixture, with test_gpu_gatv2.py's LeakyReLU-kink rule
    for variant in ("raw", "und"):
        data, tm, dims, fx, _ = G1._case("office", variant)
        x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
        edges = edge_list(data.edge_index.cpu(), x64.shape[0])
        for name, hidden, heads, layers, seed in OFFICE_MODELS:
            key = f"{variant}/{name}"
            pre = key + "/"
            loss, grads = res[0]["office"][key]
            for r in range(1, world):                       # every rank holds the same all-reduced gradients
                assert sorted(res[r]["office"][key][1]) == sorted(grads)
                assert all(np.array_equal(grads[k], res[r]["office"][key][1][k]) for k in grads)
            m = G1._model(dims, fx, name, hidden, heads, layers, seed)
            P = params64(m.state_dict())
            assert sorted(grads) == sorted(P)               # every conv tensor, and no BatchNorm, receives a gradient
            ref_loss = float(fx[pre + "loss"])
            print(f"{key}: loss {loss:.8f} fixture {ref_loss:.8f}")
            assert abs(loss - ref_loss) <= OFFICE_LOSS_BAR * abs(ref_loss), key
            ref = G1._ref_grads(fx, pre, name, P, x64, edges, y, tmc)
            bad = []
            for k in grads:
                got, want = ref(k, grads[k])
                err = np.abs(got - want).max()
                print(f"{pre}{k}: grad err {err / np.abs(want).max():.3e} of max")
                if err > GRAD_BAR * np.abs(want).max():
                    assert err <= KINK_CAP * np.abs(want).max(), f"{pre}{k}: {err:.3e} beyond any LeakyReLU kink flip"
                    bad.append(k)
            if bad:                                          # the fp64 restatement with the GPU's LeakyReLU side pattern
                ref = G1._ref_grads(fx, pre, name, P, x64, edges, y, tmc, sides=G1._gpu_sides(m, data, edges))
                for k in grads:
                    G1._grad_ok(*ref(k, grads[k]), f"{pre}{k} (GPU LeakyReLU pattern)")
                print(f"{pre}: LeakyReLU kink flips explained for {bad}")
    # (2) synth, dropout 0.6 / 0.5: three Adam steps against the single-GPU steps; a repeated run is bitwise equal
    for r in range(world):
        w = res[r]["synth"]
        assert w["loss"] <= LOSS_BAR and w["grad"] <= GRAD_BAR and w["param"] <= 1.0, (r, w)
        assert w["repeat"], (r, "two identical runs differ")
