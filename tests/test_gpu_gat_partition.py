"""GPU: GAT on a destination-node partition (bridged_gnn_amd.dist_gat) -- the global-position dropout hashes of the GAT aggregation
(`row_ids` for the feature mask, `edge_base` for the attention mask) in the forward and in the backward that redraws them:
identity ids against the plain entries, renumbered rows, and every rank's extended graph of a 3-way partition against the
whole-graph call (n_src > n_rows in the backward); world 1 against the single-GPU model; simulated worlds 2/4/8 in one process
(ranks as threads, the exchange by row copies); and REAL ranks in a gloo group sharing the GPU (payload staged through the host,
kernels the production ones): gradients against the reference's fp64 gradients on the office graph, and three Adam steps with
dropout 0.6 against the single-GPU steps, twice, the second run bitwise the first.
Bars: those of test_gpu_gat.py (activations 1e-5 of the tensor's max + 1e-6, gradients 2e-5 of the max, LeakyReLU-kink cap 2e-4,
Adam losses and parameters 1e-4) and, for world 1, those of test_gpu_gcn_partition.test_world1_matches_gcnnet.  A partitioned step
differs from the single-GPU one only in the order of some fp32 sums (the by-source pass, the gradient return, dW)."""
import copy
import threading
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_gat as G1
from test_gat_host import OFFICE_MODELS, edge_list, params64
from test_gpu_gcn_partition import _Box, _ThreadComm, _steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_BAR, GRAD_BAR, KINK_CAP = G1.ACT_BAR, G1.GRAD_BAR, G1.KINK_CAP      # 1e-5, 2e-5, 2e-4
ADAM_BAR, LOSS_BAR = 1e-4, 1e-4                                         # test_gpu_gat.py's Adam bars (parameters, losses)
OFFICE_LOSS_BAR = 1e-5                                                  # its bar on the fixture's loss
SHAPES = ((1, 2), (1, 31), (3, 8), (3, 64), (8, 16))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _settings(H):
    """(p_att, epilogue, p_drop): attention dropout off / on, the ELU epilogue without and with feature dropout, and the
    log_softmax epilogue where it exists (one head)"""
    out = [(pa, "elu", pd) for pa in (0.0, 0.6) for pd in (0.0, 0.6)]
    if H == 1:
        out += [(0.0, "log_softmax", 0.0), (0.6, "log_softmax", 0.0)]
    return out


def _fwd(T, a_s, a_d, b, rowptr, col, n_rows, H, C, p_att, epi, p_drop, **ids):
    from bridged_gnn_amd import ops
    s_src, s_dst = ops.gat_scores(T, a_s, a_d, H, C)
    s_dst = s_dst[:n_rows]
    out, state, pre, alpha = ops.gat_aggregate(T, s_src, s_dst, rowptr, col, n_rows, H, C, bias=b, p_att=p_att, seed_att=1234,
                                               epilogue=epi, p_drop=p_drop, seed=99, want_pre=True, return_alpha=True, **ids)
    return (s_src, s_dst), (out, state, alpha, pre)


def _bwd(T, scores, kept, dy, rowptr, col, tr, H, C, b, p_att, epi, p_drop, **kw):
    from bridged_gnn_amd import ops
    out, state, alpha, pre = kept
    return ops.gat_aggregate_bwd(T, scores[0], scores[1], state, alpha, pre, dy, rowptr, col, tr[0], tr[1], tr[2], H, C, bias=b,
                                 p_att=p_att, seed_att=1234, epilogue=epi, p_drop=p_drop, seed=99, **kw)


# ---- kernel: identity ids ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,C", SHAPES)
def test_identity_ids_are_the_plain_kernels(H, C):
    """row_ids = arange(n) and edge_base = rowptr[:-1] name the positions the plain entries hash: bitwise the plain call, forward
    (out, state, alpha, pre) and backward (all four outputs); pad columns 0"""
    G = G1._shared_graph(G1.SMALLG)
    g, n, HC = G.g, G.n, H * C
    T, a_s, a_d, b, dy = (t.to(DEV) for t in G1._inputs(n, H, C, seed=40 + H * 131 + C))
    ids = dict(row_ids=torch.arange(n, dtype=torch.int64, device=DEV), edge_base=g.rowptr[:-1].long().contiguous())
    tr = (g.t_rowptr, g.t_eid, g.t_dst)
    for p_att, epi, p_drop in _settings(H):
        tag = f"H={H} C={C} p_att={p_att} epi={epi} p_drop={p_drop}"
        sc, plain = _fwd(T, a_s, a_d, b, g.rowptr, g.col, n, H, C, p_att, epi, p_drop)
        _, got = _fwd(T, a_s, a_d, b, g.rowptr, g.col, n, H, C, p_att, epi, p_drop, **ids)
        assert all(torch.equal(x, y) for x, y in zip(plain, got)), tag + ": forward"
        if got[0].shape[1] > HC:
            assert torch.count_nonzero(got[0][:, HC:]).item() == 0 and torch.count_nonzero(got[3][:, HC:]).item() == 0, "pad columns"
        bp = _bwd(T, sc, plain, dy, g.rowptr, g.col, tr, H, C, b, p_att, epi, p_drop)
        bg = _bwd(T, sc, plain, dy, g.rowptr, g.col, tr, H, C, b, p_att, epi, p_drop, n_rows=n, **ids)
        assert all(torch.equal(x, y) for x, y in zip(bp, bg)), tag + ": backward"
        if bg[0].shape[1] > HC:
            assert torch.count_nonzero(bg[0][:, HC:]).item() == 0, "pad columns"


# ---- kernel: permuted rows ---------------------------------------------------------------------------------------------
_PERM = {}


def _permuted():
    """the SMALLG graph with its nodes renumbered (new node i = old node perm[i]; every row keeps its edge order)"""
    if not _PERM:
        from bridged_gnn_amd import ops
        G = G1._shared_graph(G1.SMALLG)
        n = G.n
        rp, colc = G.g.rowptr.long().cpu(), G.g.col.long().cpu()
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(4))
        inv = torch.empty(n, dtype=torch.int64)
        inv[perm] = torch.arange(n)
        deg = (rp[1:] - rp[:-1])[perm]
        rowptr_p = torch.zeros(n + 1, dtype=torch.int64)
        rowptr_p[1:] = torch.cumsum(deg, 0)
        # position in the original CSR of every edge of the renumbered one
        pos = torch.repeat_interleave(rp[perm] - rowptr_p[:-1], deg) + torch.arange(int(rowptr_p[-1]))
        col_p = inv[colc[pos]]
        rowptr_d, col_d = rowptr_p.to(torch.int32).to(DEV), col_p.to(torch.int32).to(DEV)
        csr = ops.DstCSR(rowptr_d, col_d, None, int(col_d.shape[0]), n)
        _PERM.update(perm=perm.to(DEV), pos=pos.to(DEV), rowptr=rowptr_d, col=col_d, tr=csr.transposed(),
                     edge_base=rp[perm].contiguous().to(DEV))
    return _PERM


@pytest.mark.parametrize("H,C", [(1, 31), (3, 8), (3, 64)])
def test_ids_carry_both_masks_to_permuted_rows(H, C):
    """renumbered nodes with row_ids = perm and edge_base = rowptr_original[perm] give bitwise the rows of the original call at
    dropout 0.5 / 0.5 (out, pre, state, every row's coefficients, ds_dst); without the ids the renumbered call draws other masks
    (what a rank would get from its local numbering); the by-source sums change their order: gradient bar"""
    G = G1._shared_graph(G1.SMALLG)
    g, n, HC = G.g, G.n, H * C
    P = _permuted()
    perm = P["perm"]
    T, a_s, a_d, b, dy = (t.to(DEV) for t in G1._inputs(n, H, C, seed=70 + H * 131 + C))
    sc, ref = _fwd(T, a_s, a_d, b, g.rowptr, g.col, n, H, C, 0.5, "elu", 0.5)
    Tp, dyp = T[perm].contiguous(), dy[perm].contiguous()
    ids = dict(row_ids=perm, edge_base=P["edge_base"])
    scp, got = _fwd(Tp, a_s, a_d, b, P["rowptr"], P["col"], n, H, C, 0.5, "elu", 0.5, **ids)
    assert torch.equal(scp[0], sc[0][perm]) and torch.equal(scp[1], sc[1][perm])
    out, state, alpha, pre = got
    assert torch.equal(out, ref[0][perm]) and torch.equal(pre, ref[3][perm]) and torch.equal(state, ref[1][perm]), f"H={H} C={C}"
    assert torch.equal(alpha, ref[2][P["pos"]]), f"H={H} C={C}: coefficients"
    assert bool((alpha == 0).any()) and bool((out[:, :HC] == 0).any()), "both masks drop something"
    _, plain = _fwd(Tp, a_s, a_d, b, P["rowptr"], P["col"], n, H, C, 0.5, "elu", 0.5)
    assert not torch.equal(plain[0], ref[0][perm]) and not torch.equal(plain[2], ref[2][P["pos"]])
    if out.shape[1] > HC:
        assert torch.count_nonzero(out[:, HC:]).item() == 0
    rb = _bwd(T, sc, ref, dy, g.rowptr, g.col, (g.t_rowptr, g.t_eid, g.t_dst), H, C, b, 0.5, "elu", 0.5)
    gb = _bwd(Tp, scp, got, dyp, P["rowptr"], P["col"], P["tr"], H, C, b, 0.5, "elu", 0.5, n_rows=n, **ids)
    assert torch.equal(gb[2], rb[2][perm]), "ds_dst is the row's own sum: bitwise"
    what = f"permuted H={H} C={C}"
    G1._grad_ok(gb[0].cpu(), rb[0][perm].cpu(), what + " grad_tbl")
    G1._grad_ok(gb[1].cpu(), rb[1][perm].cpu(), what + " ds_src")
    G1._grad_ok(gb[3].cpu(), rb[3].cpu(), what + " grad_bias")


# ---- kernel: the extended graphs of a partition ----------------------------------------------------------------------
HUBS = (3000, 30000, 1, 1000)      # SMALLG's graph plus a 1000-edge hub destination (node 3) and hub source (node 5)


@pytest.mark.parametrize("H,C", [(1, 31), (3, 8), (3, 64)])
def test_extended_graphs_of_a_partition_match_the_whole_graph(H, C):
    """every rank of a 3-way partition runs forward and backward over its extended graph (n_src = n_ext > n_rows = n_local in the
    backward) on rows of T and grad_y picked by global id -- no communication: forward rows and ds_dst bitwise the whole-graph
    call's at dropout 0.5 / 0.5; grad_tbl and ds_src, scatter-added by global id over the ranks, within the gradient bar"""
    from bridged_gnn_amd.dist_gat import GatPartition, _GatTables
    G = G1._shared_graph(HUBS)
    g, n, HC = G.g, G.n, H * C
    assert G.indeg[3] >= 1000 and G.outdeg[5] >= 1000
    ei = G1._graph(*HUBS)
    T, a_s, a_d, b, dy = (t.to(DEV) for t in G1._inputs(n, H, C, seed=90 + H * 131 + C))
    sc, ref = _fwd(T, a_s, a_d, b, g.rowptr, g.col, n, H, C, 0.5, "elu", 0.5)
    rb = _bwd(T, sc, ref, dy, g.rowptr, g.col, (g.t_rowptr, g.t_eid, g.t_dst), H, C, b, 0.5, "elu", 0.5)
    dT = torch.zeros(n, rb[0].shape[1], dtype=torch.float64, device=DEV)
    dss = torch.zeros(n, H, dtype=torch.float64, device=DEV)
    halo = 0
    for r in range(3):
        part = GatPartition(ei, n, r, 3)
        tb = _GatTables(part, DEV)
        nl, ext, own = part.n_local, _t(part.ext_global()), tb.owned_global
        halo += part.n_halo
        ids = dict(row_ids=own, edge_base=tb.edge_base)
        Te, dyo = T[ext].contiguous(), dy[own].contiguous()
        sce, got = _fwd(Te, a_s, a_d, b, tb.rowptr_local, tb.col, nl, H, C, 0.5, "elu", 0.5, **ids)
        for x, y, what in zip(got, ref, ("out", "state", "alpha", "pre")):
            if what != "alpha":
                assert torch.equal(x, y[own]), f"rank {r} H={H} C={C}: {what}"
        gb = _bwd(Te, sce, got, dyo, tb.rowptr_local, tb.col, (tb.t_rowptr, tb.t_eid, tb.t_dst), H, C, b, 0.5, "elu", 0.5,
                  n_rows=nl, **ids)
        assert gb[0].shape[0] == part.n_ext and gb[1].shape == (part.n_ext, H) and gb[2].shape == (nl, H)
        assert torch.equal(gb[2], rb[2][own]), f"rank {r}: ds_dst"
        dT.index_add_(0, ext, gb[0].double())
        dss.index_add_(0, ext, gb[1].double())
    assert halo > 0
    G1._grad_ok(dT.cpu(), rb[0].cpu(), f"extended H={H} C={C} grad_tbl")
    G1._grad_ok(dss.cpu(), rb[1].cpu(), f"extended H={H} C={C} ds_src")


# ---- the driver ------------------------------------------------------------------------------------------------------
def _gat(F_in, C, hidden, head, dropout, seed=0):
    from bridged_gnn_amd.gat import GAT
    torch.manual_seed(seed)
    return GAT(types.SimpleNamespace(num_features=F_in, num_classes=C), hidden=hidden, head=head, dropout=dropout).to(DEV)


def _graph(n, e, seed):
    from bridged_gnn_amd import synth
    ei, _ = synth.random_multigraph(n, e, n_isolated=max(n // 50, 1), seed=seed)
    loops = np.arange(0, n, 7)
    return np.concatenate([ei, ei[:, : e // 20], np.stack([loops, loops])], axis=1).astype(np.int64)


def test_world1_matches_gat():
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_gat import PartitionedGAT
    n = 5000
    ei = _graph(n, 40000, seed=8)
    x = torch.randn(n, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    y = torch.randint(0, 5, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tm = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) < 0.5
    data = Data(x=x, edge_index=_t(ei))
    m = _gat(48, 5, 64, 3, 0.6).eval()
    pg = PartitionedGAT(m, ei, n, 0, 1, DEV)
    own = pg.owned_global
    assert pg.n_halo == 0 and pg.n_local == n
    with torch.no_grad():
        G1._act_ok(pg.forward(x[own]).cpu(), m(data)[own].cpu(), "world 1 forward")
        G1._act_ok(pg.get_emb(x[own]).cpu(), m.get_emb(data)[own].cpu(), "world 1 get_emb")
    # one training step with dropout 0.6 (the same host seeds, the global positions of both masks)
    m2 = copy.deepcopy(m).train()
    m.train()
    pg = PartitionedGAT(m2, ei, n, 0, 1, DEV)
    o1 = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, weight_decay=5e-3)
    torch.manual_seed(11)
    l1 = F.nll_loss(m(data)[tm], y[tm])
    l1.backward()
    torch.manual_seed(11)
    l2 = pg.nll_loss(pg.forward(x[own]), y[own], tm[own])
    l2.backward()
    pg.sync_grads()
    print(f"loss {l1.item():.8f} partitioned {l2.item():.8f}")
    assert abs(l1.item() - l2.item()) <= 2e-6 * abs(l1.item())
    for (k, a), b in zip(m.named_parameters(), m2.parameters()):
        err, top = (a.grad - b.grad).abs().max().item(), a.grad.abs().max().item()
        print(f"{k}: grad err {err / top:.3e} of max")
        assert err <= GRAD_BAR * top, k
    o1.step(); o2.step()
    for (k, a), b in zip(m.named_parameters(), m2.parameters()):
        err = (a - b).abs().max().item()
        print(f"{k}: parameter err after the step {err:.3e}")
        assert err <= 2e-6, k


@pytest.mark.parametrize("world", [2, 4, 8])
def test_simulated_ranks_eval_rows_match_single_gpu(world):
    from bridged_gnn_amd import synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_gat import PartitionedGAT
    n_src, n_tar = 4000, 3000
    ei, mask = synth.bridged_graph(n_src, n_tar, 4, 8, 9000, cluster=128, p_local=0.8, seed=world)
    n = n_src + n_tar
    rng = np.random.default_rng(world)
    # node 2: a hub DESTINATION fed from every rank; node 1: a hub SOURCE feeding rows of every rank (a halo slot elsewhere)
    ei = np.concatenate([ei, np.stack([rng.choice(n, 1000, replace=False), np.full(1000, 2)]),
                         np.stack([np.full(3500, 1), rng.choice(n, 3500, replace=False)])], axis=1).astype(np.int64)
    x = torch.randn(n, 40, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world))
    m = _gat(40, 7, 16, 3, 0.6).eval()
    data = Data(x=x, edge_index=_t(ei))
    with torch.no_grad():
        ref, ref_emb = m(data), m.get_emb(data)
    for owner in (None, partition_nodes(mask, world)):
        box = _Box(world)
        res, errs = [None] * world, []

        def run(r):
            try:
                pg = PartitionedGAT(m, ei, n, r, world, DEV, owner=owner)
                pg.comm = _ThreadComm(box, r)
                with torch.no_grad():
                    xl = x[pg.owned_global]
                    res[r] = (pg.owned_global, pg.forward(xl), pg.get_emb(xl), pg.n_halo)
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
        assert sum(r[3] for r in res) > 0, "no halo at all"
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        for r, (own, out, emb, _) in enumerate(res):
            G1._act_ok(out.cpu(), ref[own].cpu(), f"world {world} rank {r} forward")
            G1._act_ok(emb.cpu(), ref_emb[own].cpu(), f"world {world} rank {r} get_emb")
            seen[own] += 1
        assert bool((seen == 1).all()), "every node is covered once"


def test_out_of_scope_raises():
    from bridged_gnn_amd.dist_gat import PartitionedGAT
    ei = _graph(200, 1000, seed=9)
    pg = PartitionedGAT(_gat(8, 3, 8, 2, 0.0).eval(), ei, 200, 0, 1, DEV)
    for call in (pg.forward, pg.get_emb):
        with pytest.raises(RuntimeError, match="no CPU"):
            call(torch.zeros(200, 8))
        with pytest.raises(ValueError):
            call(torch.zeros(199, 8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU"):
        PartitionedGAT(_gat(8, 3, 8, 2, 0.0), ei, 200, 0, 1, "cpu")
    with pytest.raises(RuntimeError, match="shape"):
        PartitionedGAT(_gat(8, 3, 8, 9, 0.0), ei, 200, 0, 1, DEV)


# ---- real ranks (gloo group, one GPU) ---------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_gat import PartitionedGAT
        res = {"office": {}, "summary": None}
        # (1) office graph, dropout 0: all-reduced gradients (compared in the parent with the reference's fp64 gradients)
        for variant in ("raw", "und"):
            data, tm, ds, fx, _ = G1._case("office", variant)
            ei = data.edge_index.cpu().numpy()
            n = data.x.shape[0]
            for name, hidden, head in OFFICE_MODELS:
                m = G1._model(ds, fx, name, hidden, head, dropout=0.0).train()
                pg = PartitionedGAT(m, ei, n, rank, world, DEV)
                own = pg.owned_global
                loss = pg.nll_loss(pg.forward(data.x[own]), data.y[own], tm[own])
                loss.backward()
                pg.sync_grads()
                tot = loss.detach().double().cpu().reshape(1)
                dist.all_reduce(tot)
                res["office"][f"{variant}/{name}"] = (float(tot), {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()})
        # (2) synth graph, dropout 0.6: three Adam steps against the single-GPU steps, then the same steps again
        n = 6000
        ei, mask = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        ei = np.concatenate([ei, ei[:, :500], np.stack([np.arange(0, n, 11)] * 2)], axis=1)   # duplicates + self loops
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, 5, (n,), device=DEV, generator=g)
        tm = torch.rand(n, device=DEV, generator=g) < 0.5
        data = Data(x=x, edge_index=_t(ei))
        m0 = _gat(64, 5, 32, 3, 0.6).train()
        ref_m, runs = copy.deepcopy(m0), []

        def single():
            loss = F.nll_loss(ref_m(data)[tm], y[tm])
            loss.backward()
            return float(loss.detach())
        ref_rec, ref_par = _steps(ref_m, single)
        for _ in range(2):
            m = copy.deepcopy(m0)
            pg = PartitionedGAT(m, ei, n, rank, world, DEV)
            own = pg.owned_global
            xl = x[own].contiguous()                        # one tensor: its halo rows are fetched once

            def part():
                loss = pg.nll_loss(pg.forward(xl), y[own], tm[own])
                loss.backward()
                pg.sync_grads()
                tot = loss.detach().double().cpu().reshape(1)
                dist.all_reduce(tot)
                return float(tot)
            runs.append(_steps(m, part))
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
def test_real_ranks_train_gat(world):
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
    # (1) office: the all-reduced loss and gradients against the reference's fp64 fixture, with test_gpu_gat.py's LeakyReLU-kink rule
    for variant in ("raw", "und"):
        data, tm, ds, fx, _ = G1._case("office", variant)
        x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
        edges = edge_list(data.edge_index.cpu(), x64.shape[0])
        for name, hidden, head in OFFICE_MODELS:
            key = f"{variant}/{name}"
            pre = key + "/"
            loss, grads = res[0]["office"][key]
            for r in range(1, world):                       # every rank holds the same all-reduced gradients
                assert all(np.array_equal(grads[k], res[r]["office"][key][1][k]) for k in grads)
            m = G1._model(ds, fx, name, hidden, head).eval()
            P = params64(m.state_dict())
            assert sorted(grads) == sorted(P)
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
    # (2) synth, dropout 0.6: three Adam steps against the single-GPU steps; a repeated run is bitwise equal
    for r in range(world):
        w = res[r]["synth"]
        assert w["loss"] <= LOSS_BAR and w["grad"] <= GRAD_BAR and w["param"] <= 1.0, (r, w)
        assert w["repeat"], (r, "two identical runs differ")
