"""GPU: GCN on a destination-node partition (bridged_gnn_amd.dist_gcn) -- the row-id dropout hash of the GCN aggregation in the
row kernel, the hub finish pass and the column-slice path; world 1 against the single-GPU model; simulated worlds 2/4/8 in one
process (ranks as threads, the exchange by row copies); and REAL ranks in a gloo group sharing the GPU (payload staged through the
host, kernels the production ones): gradients against the reference's fp64 gradients on the office graph, and three Adam steps
with dropout 0.5 against the single-GPU steps, twice, the second run bitwise the first.
Bars: those of test_gpu_gcn.py (activations 1e-5, gradients 2e-5 of each tensor's max, ReLU-kink cap 2e-4, Adam parameters 1e-4,
losses 1e-5 relative) and, for world 1, those of test_gpu_sage_partition.test_world1_matches_graphsage."""
import copy
import threading
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_gcn_host import OFFICE_MODELS, norm_adj, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DS = (1, 3, 4, 5, 31, 64, 128, 200)
ACT_BAR, GRAD_BAR, KINK_CAP = 1e-5, 2e-5, 2e-4                   # test_gpu_gcn.py's bars
ADAM_BAR, LOSS_BAR = 1e-4, 1e-5                                  # its header's Adam-parameter bar and its loss bar


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bar_ok(got, ref, rel, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref).max()
    tol = rel * np.abs(ref).max() + 1e-6
    print(f"{what}: max err {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


# ---- kernel ----------------------------------------------------------------------------------------------------------
N_K, ROW_256, ROW_255 = 3000, 2990, 2991          # the two rows sit among the nodes random_multigraph leaves without in-edges


def _kernel_graph(seed):
    """test_gpu_gcn._graph (duplicates, self loops, isolated nodes) with a destination hub (node 3) and a source hub (node 5) of
    1000 edges each -- several 128-edge segments above the 256 threshold -- and rows of exactly 256 and 255 edges (self loop
    included): one on each side of the threshold"""
    from bridged_gnn_amd import synth
    n, e = N_K, 30000
    ei, _ = synth.random_multigraph(n, e, n_isolated=n // 50, seed=seed)
    loops = np.arange(0, n, 7)
    rng = np.random.default_rng(seed)
    extra = [ei, ei[:, : e // 20], np.stack([loops, loops]), np.stack([loops[:5], loops[:5]]),
             np.stack([rng.integers(0, n, 1000), np.full(1000, 3)]),
             np.stack([np.full(1000, 5), rng.integers(0, n - n // 50, 1000)]),
             np.stack([np.arange(100, 355), np.full(255, ROW_256)]),
             np.stack([np.arange(400, 654), np.full(254, ROW_255)])]
    return np.concatenate(extra, axis=1).astype(np.int64)


def _kernel_case(seed):
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.gcn import GcnGraph
    g = GcnGraph(_t(_kernel_graph(seed)), N_K)
    deg = (g.csr.rowptr[1:] - g.csr.rowptr[:-1]).cpu().numpy()
    assert deg[ROW_256] == 256 == ops.GCN_HUB_THRESHOLD and deg[ROW_255] == 255 and deg[3] >= 1000
    hub_rows = g.hubs[1].cpu().numpy()
    assert ROW_256 in hub_rows and 3 in hub_rows and ROW_255 not in hub_rows
    assert g.hubs[3].shape[0] // 2 >= 8 + 2                      # node 3: >= 8 segments, row 256: 2
    return g


def test_row_ids_identity_is_the_plain_kernel():
    from bridged_gnn_amd import ops
    g = _kernel_case(seed=1)
    n = N_K
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    gen = torch.Generator().manual_seed(2)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.randn(n, Dp, generator=gen).to(DEV)
        b = torch.randn(Dp, generator=gen).to(DEV)
        for epi, p in ((None, 0.0), ("relu", 0.0), ("relu", 0.5), ("log_softmax", 0.0)):
            if epi == "log_softmax" and D > 128:
                continue
            kw = dict(bias=b, epilogue=epi, p_drop=p, seed=77, hubs=g.hubs)
            a = ops.gcn_aggregate(T, g.csr.rowptr, g.col, g.dinv, n, D, **kw)
            c = ops.gcn_aggregate(T, g.csr.rowptr, g.col, g.dinv, n, D, row_ids=ids, **kw)
            assert torch.equal(a, c), f"D={D} epi={epi} p={p}"
            if Dp > D:
                assert torch.count_nonzero(c[:, D:]).item() == 0, "pad columns must be 0"


def test_row_ids_carry_the_masks_to_permuted_rows():
    """the graph with its nodes renumbered (new node i = old node perm[i]; every row keeps its edge order) and row_ids = perm
    gives bitwise the rows of the original call at dropout 0.5 -- hub rows, finished by the hub pass, included; without the ids
    the renumbered call draws other masks (what a rank would get from its local row numbers)"""
    from bridged_gnn_amd import ops
    g = _kernel_case(seed=3)
    n = N_K
    rp = g.csr.rowptr.long().cpu()
    colc = g.col.long().cpu()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(4))
    inv = torch.empty(n, dtype=torch.int64)
    inv[perm] = torch.arange(n)
    assert int(inv[3]) != 3 and int(inv[ROW_256]) != ROW_256   # the hub rows move
    deg = (rp[1:] - rp[:-1])[perm]
    rowptr_p = torch.zeros(n + 1, dtype=torch.int64)
    rowptr_p[1:] = torch.cumsum(deg, 0)
    col_p = torch.cat([inv[colc[rp[i]:rp[i + 1]]] for i in perm.tolist()])
    rowptr_p, col_p, perm_d = rowptr_p.to(torch.int32).to(DEV), col_p.to(torch.int32).to(DEV), perm.to(DEV)
    csr_p = ops.DstCSR(rowptr_p, col_p, None, int(col_p.shape[0]), n)
    tabs = csr_p.hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT)
    hubs_p = (ops.GCN_HUB_THRESHOLD, tabs[0], tabs[1], tabs[2])
    assert sorted(perm[tabs[0].long().cpu()].tolist()) == sorted(g.hubs[1].cpu().tolist())
    dinv_p = g.dinv[perm_d].contiguous()
    gen = torch.Generator().manual_seed(5)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.randn(n, Dp, generator=gen).to(DEV)
        b = torch.randn(Dp, generator=gen).to(DEV)
        kw = dict(bias=b, epilogue="relu", p_drop=0.5, seed=99)
        ref = ops.gcn_aggregate(T, g.csr.rowptr, g.col, g.dinv, n, D, hubs=g.hubs, **kw)
        Tp = T[perm_d].contiguous()
        got = ops.gcn_aggregate(Tp, rowptr_p, col_p, dinv_p, n, D, hubs=hubs_p, row_ids=perm_d, **kw)
        assert torch.equal(got, ref[perm_d]), f"D={D}"
        plain = ops.gcn_aggregate(Tp, rowptr_p, col_p, dinv_p, n, D, hubs=hubs_p, **kw)
        assert not torch.equal(plain, ref[perm_d]), f"D={D}"
        if Dp > D:
            assert torch.count_nonzero(got[:, D:]).item() == 0, "pad columns must be 0"


# ---- the driver ------------------------------------------------------------------------------------------------------
def _gcn(F_in, C, L, hidden, dropout, seed=0):
    from bridged_gnn_amd.gcn import GCNNet
    torch.manual_seed(seed)
    return GCNNet(types.SimpleNamespace(num_features=F_in, num_classes=C), layer_num=L, hidden=hidden, dropout=dropout).to(DEV)


def _graph(n, e, seed):
    from bridged_gnn_amd import synth
    ei, _ = synth.random_multigraph(n, e, n_isolated=max(n // 50, 1), seed=seed)
    loops = np.arange(0, n, 7)
    return np.concatenate([ei, ei[:, : e // 20], np.stack([loops, loops])], axis=1).astype(np.int64)


def _hidden_outputs(out):
    """the layer outputs kept by the autograd nodes of the GCN layer functions (ctx.y), first conv first, the last conv left out"""
    ys, seen, stack = [], set(), [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        if hasattr(fn, "y") and hasattr(fn, "cfg"):
            ys.append(fn.y)
        stack.extend(f for f, _ in fn.next_functions)
    return ys[::-1][:-1]


@pytest.mark.parametrize("L", [1, 2, 3])
def test_world1_matches_gcnnet(L):
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_gcn import PartitionedGCN
    n = 5000
    ei = _graph(n, 40000, seed=8)
    x = torch.randn(n, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    y = torch.randint(0, 5, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tm = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) < 0.5
    data = Data(x=x, edge_index=_t(ei))
    m = _gcn(48, 5, L, 64, 0.5).eval()
    pg = PartitionedGCN(m, ei, n, 0, 1, DEV)
    own = pg.owned_global
    assert pg.n_halo == 0 and pg.n_local == n
    with torch.no_grad():
        for what in ("forward", "get_emb", "get_logits"):
            ref = getattr(m, what)(data)
            got = getattr(pg, what)(x[own])
            _bar_ok(got.cpu(), ref[own].cpu(), ACT_BAR, f"L={L} {what}")
    # one training step with dropout 0.5 (the same host seeds and global-row masks)
    m2 = copy.deepcopy(m).train()
    m.train()
    pg = PartitionedGCN(m2, ei, n, 0, 1, DEV)
    o1 = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, weight_decay=5e-3)
    torch.manual_seed(11)
    l1 = F.nll_loss(m(data)[tm], y[tm])
    l1.backward()
    torch.manual_seed(11)
    l2 = pg.nll_loss(pg.forward(x[own]), y[own], tm[own])
    l2.backward()
    pg.sync_grads()
    print(f"L={L} loss {l1.item():.8f} partitioned {l2.item():.8f}")
    assert abs(l1.item() - l2.item()) <= 2e-6 * abs(l1.item())
    for (k, a), b in zip(m.named_parameters(), m2.parameters()):
        err, top = (a.grad - b.grad).abs().max().item(), a.grad.abs().max().item()
        print(f"L={L} {k}: grad err {err / top:.3e} of max")
        assert err <= GRAD_BAR * top, k
    o1.step(); o2.step()
    for (k, a), b in zip(m.named_parameters(), m2.parameters()):
        assert (a - b).abs().max().item() <= 2e-6, k


class _Box:
    def __init__(self, world):
        self.world, self.slots = world, [None] * world
        self.bar = threading.Barrier(world, timeout=120)


class _ThreadComm:
    """the collectives of `dist_train._Comm` between ranks that are threads of one process (row copies on the device)"""

    def __init__(self, box, rank):
        self.box, self.rank, self.world, self.live, self.host = box, rank, box.world, True, False

    def _swap(self, v):
        self.box.slots[self.rank] = v
        self.box.bar.wait()
        got = list(self.box.slots)
        self.box.bar.wait()
        return got

    def all_to_all(self, send, send_splits, recv_splits):
        got = self._swap((send, list(send_splits)))
        chunks = []
        for s, sp in got:
            o = sum(sp[:self.rank])
            chunks.append(s[o:o + sp[self.rank]])
        out = torch.cat(chunks).contiguous()
        assert out.shape[0] == sum(recv_splits)
        return out

    def all_reduce(self, t):
        got = self._swap(t.clone())
        return torch.stack(got).sum(0)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_simulated_ranks_eval_rows_match_single_gpu(world):
    from bridged_gnn_amd import synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_gcn import PartitionedGCN
    n_src, n_tar = 4000, 3000
    ei, mask = synth.bridged_graph(n_src, n_tar, 4, 8, 9000, cluster=128, p_local=0.8, seed=world)
    n = n_src + n_tar
    rng = np.random.default_rng(world)
    # node 2: a hub DESTINATION fed from every rank; node 1: a hub SOURCE feeding >= 256 rows of every rank (a halo slot that is
    # a hub of the by-source view on the ranks that do not own it)
    ei = np.concatenate([ei, np.stack([rng.choice(n, 1000, replace=False), np.full(1000, 2)]),
                         np.stack([np.full(3500, 1), rng.choice(n, 3500, replace=False)])], axis=1).astype(np.int64)
    x = torch.randn(n, 40, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world))
    for L, owner in ((2, None), (3, partition_nodes(mask, world))):
        m = _gcn(40, 7, L, 64, 0.5).eval()
        data = Data(x=x, edge_index=_t(ei))
        with torch.no_grad():
            ref, ref_emb = m(data), m.get_emb(data)
        box = _Box(world)
        res, errs = [None] * world, []

        def run(r):
            try:
                pg = PartitionedGCN(m, ei, n, r, world, DEV, owner=owner)
                pg.comm = _ThreadComm(box, r)
                th = pg.tables.t_hubs
                with torch.no_grad():
                    xl = x[pg.owned_global]
                    res[r] = (pg.owned_global, pg.forward(xl), pg.get_emb(xl), pg.n_halo, pg.tables.hubs is not None,
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
        assert sum(r[3] for r in res) > 0, "no halo at all"
        assert sum(r[4] for r in res) >= 1, "the hub destination is a hub on its owner's rank"
        assert sum(r[5] for r in res) >= 1, "no rank holds a halo slot that is a hub source"
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        for r, (own, out, emb, _, _, _) in enumerate(res):
            _bar_ok(out.cpu(), ref[own].cpu(), ACT_BAR, f"world {world} L={L} rank {r} forward")
            _bar_ok(emb.cpu(), ref_emb[own].cpu(), ACT_BAR, f"world {world} L={L} rank {r} get_emb")
            seen[own] += 1
        assert bool((seen == 1).all()), "every node is covered once"


def test_out_of_scope_raises():
    from bridged_gnn_amd.dist_gcn import PartitionedGCN
    ei = _graph(200, 1000, seed=9)
    with pytest.raises(NotImplementedError):
        PartitionedGCN(_gcn(8, 130, 2, 8, 0.0), ei, 200, 0, 1, DEV)
    pg = PartitionedGCN(_gcn(8, 3, 2, 8, 0.0).eval(), ei, 200, 0, 1, DEV)
    for call in (pg.forward, pg.get_emb, pg.get_logits):
        with pytest.raises(RuntimeError, match="no CPU"):
            call(torch.zeros(200, 8))
        with pytest.raises(ValueError):
            call(torch.zeros(199, 8, device=DEV))


# ---- real ranks (gloo group, one GPU) ---------------------------------------------------------------------------------
def _office(variant):
    from bridged_gnn_amd.data import Data
    g, fx = load_golden("office_a2d_graph.npz"), load_golden("gcn_office_a2d.npz")
    data = Data(x=torch.from_numpy(g["x"]).to(DEV), edge_index=torch.from_numpy(g["edge_index"]).long().to(DEV),
                y=torch.from_numpy(g["y"]).long().to(DEV))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(fx["train_mask"]).to(DEV)          # the driver's mask (y == -1 cleared, :404)
    return data, tm, types.SimpleNamespace(num_features=g["x"].shape[1], num_classes=int(g["y"].max()) + 1), fx


def _steps(m, run, steps=3):
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
    rec = []
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        torch.manual_seed(100 + step)                      # the host generator behind the dropout seeds
        loss = run()
        rec.append((loss, {k: p.grad.clone() for k, p in m.named_parameters()}))
        opt.step()
    return rec, {k: p.detach().clone() for k, p in m.named_parameters()}


def _rank_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_gcn import PartitionedGCN
        from bridged_gnn_amd.gcn import GCNNet
        res = {"office": {}, "summary": None}
        # (1) office graph, dropout 0: all-reduced gradients (compared in the parent with the reference's fp64 gradients)
        for variant in ("raw", "und"):
            data, tm, ds, _ = _office(variant)
            ei = data.edge_index.cpu().numpy()
            n = data.x.shape[0]
            for name, L, hidden in OFFICE_MODELS:
                torch.manual_seed(0)
                m = GCNNet(ds, layer_num=L, hidden=hidden, dropout=0.0).to(DEV).train()
                pg = PartitionedGCN(m, ei, n, rank, world, DEV)
                own = pg.owned_global
                out = pg.forward(data.x[own])
                loss = pg.nll_loss(out, data.y[own], tm[own])
                loss.backward()
                pg.sync_grads()
                tot = loss.detach().double().cpu().reshape(1)
                dist.all_reduce(tot)
                res["office"][f"{variant}/{name}"] = (
                    float(tot), {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()}, own.cpu().numpy(),
                    [(y[:, :hidden].cpu().numpy() > 0) for y in _hidden_outputs(out)])
        # (2) synth graph, dropout 0.5: three Adam steps against the single-GPU steps, then the same steps again
        n = 6000
        ei, mask = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        ei = np.concatenate([ei, ei[:, :500], np.stack([np.arange(0, n, 11)] * 2)], axis=1)   # duplicates + self loops
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, 5, (n,), device=DEV, generator=g)
        tm = torch.rand(n, device=DEV, generator=g) < 0.5
        data = Data(x=x, edge_index=_t(ei))
        torch.manual_seed(0)
        m0 = GCNNet(types.SimpleNamespace(num_features=64, num_classes=5), layer_num=3, hidden=64, dropout=0.5).to(DEV).train()
        ref_m, runs = copy.deepcopy(m0), []

        def single():
            loss = F.nll_loss(ref_m(data)[tm], y[tm])
            loss.backward()
            return float(loss.detach())
        ref_rec, ref_par = _steps(ref_m, single)
        for _ in range(2):
            m = copy.deepcopy(m0)
            pg = PartitionedGCN(m, ei, n, rank, world, DEV)
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
def test_real_ranks_train_gcn(world):
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
    # (1) office: the all-reduced loss and gradients against the reference's fp64 fixture (where it stores gradients; else the
    #     fp64 restatement tests/test_gcn_host.py pins to it), with test_gpu_gcn.py's ReLU-kink handling
    from bridged_gnn_amd.gcn import GCNNet
    for variant in ("raw", "und"):
        data, tm, ds, fx = _office(variant)
        x64, y, tmc = data.x.double().cpu(), data.y.cpu(), tm.cpu()
        A = norm_adj(data.edge_index.cpu(), x64.shape[0])
        for name, L, hidden in OFFICE_MODELS:
            key = f"{variant}/{name}"
            pre = key + "/"
            loss, grads, _, _ = res[0]["office"][key]
            for r in range(1, world):                       # every rank holds the same all-reduced gradients
                assert all(np.array_equal(grads[k], res[r]["office"][key][1][k]) for k in grads)
            torch.manual_seed(0)                            # the fixture's initial parameters (test_gpu_gcn.py checks them)
            m = GCNNet(ds, layer_num=L, hidden=hidden)
            P = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}

            def ref_grads(masks=None):
                if masks is None and pre + "grad/convs.0.lin.weight" in fx:
                    return {k: fx[pre + "grad/" + k] for k in P}
                lo = F.nll_loss(restate(P, x64, A, relu_masks=masks)[tmc], y[tmc])
                return {k: g.numpy() for k, g in zip(P, torch.autograd.grad(lo, list(P.values())))}
            ref_loss = float(fx[pre + "loss"])
            print(f"{key}: loss {loss:.8f} fixture {ref_loss:.8f}")
            assert abs(loss - ref_loss) <= LOSS_BAR * abs(ref_loss), key
            ref = ref_grads()
            bad = []
            for k in ref:
                err = np.abs(grads[k] - ref[k]).max()
                print(f"{pre}{k}: grad err {err / np.abs(ref[k]).max():.3e} of max")
                if err > GRAD_BAR * np.abs(ref[k]).max():
                    assert err <= KINK_CAP * np.abs(ref[k]).max(), f"{pre}{k}: {err:.3e} beyond any ReLU kink flip"
                    bad.append(k)
            if bad:                                          # the fp64 restatement with the ranks' ReLU pattern
                masks = [torch.zeros(x64.shape[0], hidden, dtype=torch.float64) for _ in range(L - 1)]
                for r in range(world):
                    _, _, own, pats = res[r]["office"][key]
                    for i, pat in enumerate(pats):
                        masks[i][torch.from_numpy(own)] = torch.from_numpy(pat.astype(np.float64))
                with torch.no_grad():                        # rows whose pattern differs from the fp64 pattern: kink rows only
                    h, flipped = x64, 0
                    for i in range(L - 1):
                        h = A @ (h @ P[f"convs.{i}.lin.weight"].t()) + P[f"convs.{i}.bias"]
                        flipped += int(((h > 0).double() != masks[i]).any(1).sum())
                        h = h * masks[i]
                print(f"{key}: {flipped} rows with a flipped ReLU")
                assert flipped <= max(1, KINK_CAP * x64.shape[0] * (L - 1)), f"{key}: {flipped} rows disagree with the fp64 pattern"
                ref = ref_grads(masks)
                for k in ref:
                    _bar_ok(grads[k], ref[k], GRAD_BAR, f"{pre}{k} (ranks' ReLU pattern)")
                print(f"{key}: ReLU kink flips explained for {bad}")
    # (2) synth, dropout 0.5: three Adam steps against the single-GPU steps; a repeated run is bitwise equal
    for r in range(world):
        w = res[r]["synth"]
        assert w["loss"] <= LOSS_BAR and w["grad"] <= GRAD_BAR and w["param"] <= 1.0, (r, w)
        assert w["repeat"], (r, "two identical runs differ")
