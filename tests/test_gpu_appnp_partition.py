"""GPU: APPNP on a destination-node partition (bridged_gnn_amd.dist_appnp) -- `ops.appnp_step` against the K-step entry it shares its
launch sequence with (bitwise, square and rectangular graphs, hub rows included); the row-id feature dropout against the plain
pass (bitwise: identity ids, permuted rows, every D % 4, the aligned fast path, past the grid cap, ragged last quads); world 1
against `APPNP_Net`; simulated worlds 2/4/8 in one process (ranks as threads), forward and the transposed partition's P^T g;
REAL ranks in a gloo group sharing the GPU: all-reduced gradients on the office graph against the fp64 restatement, three Adam
steps at dropout 0.5 against the single-GPU steps, twice, the second run bitwise the first; and the out-of-scope refusals.
Bars: test_gpu_gcn.py's (activations 1e-5, gradients 2e-5 of each tensor's max) and test_gpu_gcn_partition.py's (Adam parameters
1e-4, losses 1e-5 relative), imported."""
import copy
import threading
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_appnp import _case, _office_data, _params64, _restate
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok, _sparse_parts
from test_gpu_gcn_partition import ADAM_BAR, LOSS_BAR, _Box, _graph, _steps, _t, _ThreadComm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- ops.appnp_step ----------------------------------------------------------------------------------------------
def _by_steps(h, rowptr, col, dinv, n, D, K, alpha, epi, hubs):
    """the K-step call as K `ops.appnp_step` calls over two alternating state buffers"""
    from bridged_gnn_amd import ops
    bufs = [torch.full((n, ops.pad4(D)), float("nan"), device=h.device) for _ in range(2)]
    src = h
    for k in range(K):
        last = k == K - 1
        store = ("log_softmax" if epi else "out") if last else "state"
        src = ops.appnp_step(src, h, rowptr, col, dinv, n, D, alpha, first=k == 0, store=store, hubs=hubs,
                             out=None if last else bufs[k & 1])
    return src


@pytest.mark.parametrize("name", ["A", "B"])
def test_k_steps_are_the_k_step_entry_bitwise(name):
    from bridged_gnn_amd import ops
    n, g, _ = _case(name)
    assert (g.hubs is not None) == (name == "B")
    gen = torch.Generator().manual_seed(51)
    for D in (1, 2, 3, 5, 31, 128):
        h = torch.randn(n, ops.pad4(D), generator=gen).to(DEV)
        for K in (1, 2, 10):
            for epi in (None, "log_softmax"):
                for hubs in ((g.hubs, None) if g.hubs is not None else (None,)):
                    ref = ops.appnp_propagate(h, g.csr.rowptr, g.col, g.dinv, n, D, K, 0.1, epilogue=epi, hubs=hubs)
                    got = _by_steps(h, g.csr.rowptr, g.col, g.dinv, n, D, K, 0.1, epi, hubs)
                    assert torch.equal(got, ref), f"graph {name} D={D} K={K} epi={epi} hubs={hubs is not None}"
        # the by-source view (the single-GPU backward's walk)
        ref = ops.appnp_propagate(h, g.t_rowptr, g.t_dst, g.dinv, n, D, 10, 0.1, hubs=g.t_hubs)
        assert torch.equal(_by_steps(h, g.t_rowptr, g.t_dst, g.dinv, n, D, 10, 0.1, None, g.t_hubs), ref), f"graph {name} D={D} by source"


def test_rectangular_step_gives_the_owned_rows_of_the_square_call():
    """graph B renumbered: a random 60 % of the nodes are the owned rows (the hub row, node 3, among them), the rest trailing table
    slots (the hub source, node 5, among them); every row keeps its edge order, so the sums are the square call's bit for bit"""
    from bridged_gnn_amd import ops
    n, g, _ = _case("B")
    rp, colc = g.csr.rowptr.long().cpu(), g.col.long().cpu()
    gen = torch.Generator().manual_seed(52)
    order = torch.randperm(n, generator=gen)
    order = order[(order != 3) & (order != 5)]
    n_own = int(0.6 * n)
    perm = torch.cat([torch.tensor([3]), order[:n_own - 1], torch.tensor([5]), order[n_own - 1:]])      # new row i = old node perm[i]
    perm[:n_own] = perm[:n_own][torch.randperm(n_own, generator=gen)]
    assert perm.shape[0] == n and sorted(perm.tolist()) == list(range(n))
    inv = torch.empty(n, dtype=torch.int64)
    inv[perm] = torch.arange(n)
    assert int(inv[3]) < n_own <= int(inv[5])
    own = perm[:n_own]
    deg = (rp[1:] - rp[:-1])[own]
    rowptr_o = torch.zeros(n_own + 1, dtype=torch.int64)
    rowptr_o[1:] = torch.cumsum(deg, 0)
    col_o = torch.cat([inv[colc[rp[i]:rp[i + 1]]] for i in own.tolist()])
    fed = sum(int((col_o[rowptr_o[i]:rowptr_o[i + 1]] == inv[5]).any()) for i in range(n_own))
    assert fed >= 256, f"the slot of node 5 feeds {fed} owned rows"
    assert int((col_o >= n_own).sum()) > 1000                                    # plenty of edges read table slots
    rowptr_o, col_o = rowptr_o.to(torch.int32).to(DEV), col_o.to(torch.int32).to(DEV)
    tabs = ops.DstCSR(rowptr_o, col_o, None, int(col_o.shape[0]), n_own).hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT)
    assert tabs is not None and int(inv[3]) in tabs[0].cpu().tolist()
    hubs_o = (ops.GCN_HUB_THRESHOLD, tabs[0], tabs[1], tabs[2])
    perm_d, own_d = perm.to(DEV), own.to(DEV)
    dinv_p = g.dinv[perm_d].contiguous()
    for D in (2, 5, 31, 128):
        Dp = ops.pad4(D)
        h = torch.randn(n, Dp, generator=gen).to(DEV)
        sq = (g.csr.rowptr, g.col, g.dinv, n, D, 0.1)
        s1 = ops.appnp_step(h, h, *sq, first=True, store="state", hubs=g.hubs)
        hp, s1p = h[perm_d].contiguous(), s1[perm_d].contiguous()
        rect = (rowptr_o, col_o, dinv_p, n_own, D, 0.1)
        for hubs in (hubs_o, None):
            got1 = ops.appnp_step(hp, hp[:n_own], *rect, first=True, store="state", hubs=hubs)
            ref1 = s1 if hubs is not None else ops.appnp_step(h, h, *sq, first=True, store="state")
            assert got1.shape == (n_own, Dp) and torch.equal(got1, ref1[own_d]), f"D={D} first step hubs={hubs is not None}"
            for store in ("state", "out", "log_softmax"):
                ref2 = ops.appnp_step(s1, h, *sq, first=False, store=store, hubs=g.hubs if hubs is not None else None)
                got2 = ops.appnp_step(s1p, hp[:n_own], *rect, first=False, store=store, hubs=hubs)
                assert torch.equal(got2, ref2[own_d]), f"D={D} state step store={store} hubs={hubs is not None}"
                if Dp > D:
                    assert torch.count_nonzero(got2[:, D:]).item() == 0 and torch.count_nonzero(got1[:, D:]).item() == 0
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|dinv"):          # the first step gathers dinv over the whole table
        ops.appnp_step(hp, hp[:n_own], rowptr_o, col_o, dinv_p[:n_own].contiguous(), n_own, D, 0.1, first=True, store="state")
    with pytest.raises((RuntimeError, ValueError), match="(?i)shape|rows"):
        ops.appnp_step(hp[:n_own - 1], hp[:n_own], *rect, first=True, store="state")
    with pytest.raises(ValueError, match="store"):
        ops.appnp_step(hp, hp[:n_own], *rect, first=True, store="relu")


# ---- feature dropout with row ids --------------------------------------------------------------------------------
def _fdrop_pair(n, D, p=0.5, seed=1234, cases=((False, False), (True, True), (True, False))):
    """on an [n, D] activation: identity ids are the plain pass bit for bit, permuted rows with row_ids = perm are the plain
    result's permuted rows (forward, backward), and without the ids they are not.  Outputs start as NaN: an element that no lane
    reaches is seen."""
    from bridged_gnn_amd import ops
    gen = torch.Generator().manual_seed(61 + n + D)
    x = torch.randn(n, D, generator=gen).to(DEV)
    b = torch.randn(D, generator=gen).to(DEV)
    dy = torch.randn(n, D, generator=gen).to(DEV)
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    perm = torch.randperm(n, generator=gen).to(DEV)

    def nan():
        return torch.full((n, D), float("nan"), device=DEV)
    xp, dyp = x[perm].contiguous(), dy[perm].contiguous()
    for relu, with_bias in cases:
        bias = b if with_bias else None
        what = f"[{n}, {D}] p={p} relu={relu} bias={with_bias}"
        y = ops.feature_dropout(x, p, seed, bias=bias, relu=relu)
        assert torch.equal(ops.feature_dropout(x, p, seed, bias=bias, relu=relu, row_ids=ids, out=nan()), y), what + " identity"
        yp = ops.feature_dropout(xp, p, seed, bias=bias, relu=relu, row_ids=perm, out=nan())
        assert torch.equal(yp, y[perm]), what + " permuted"
        gx = ops.feature_dropout_bwd(dy, p, seed, y=y if relu else None, relu=relu)
        assert torch.equal(ops.feature_dropout_bwd(dy, p, seed, y=y if relu else None, relu=relu, row_ids=ids, out=nan()), gx), what
        gxp = ops.feature_dropout_bwd(dyp, p, seed, y=yp if relu else None, relu=relu, row_ids=perm, out=nan())
        assert torch.equal(gxp, gx[perm]), what + " backward permuted"
        if p > 0 and n * D >= 64:
            assert not torch.equal(ops.feature_dropout(xp, p, seed, bias=bias, relu=relu), y[perm]), what + ": local rows draw other masks"
            if not relu:
                assert not torch.equal(ops.feature_dropout_bwd(dyp, p, seed), gx[perm]), what
    return x, perm


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 7, 64])
def test_feature_dropout_row_ids(D):
    from bridged_gnn_amd import ops
    n = 2049                                              # several blocks at every width; n * D % 4 != 0 for every odd D and D = 2
    assert (n * D % 4 != 0) == (D % 4 != 0)               # a ragged last quad wherever the width allows one
    x, perm = _fdrop_pair(n, D)
    _fdrop_pair(n, D, p=0.0, cases=((True, True),))       # p = 0: act(x + b), no mask drawn
    # the (seed, seed_dev) pair composes as in the plain pass
    word = torch.tensor([1000], dtype=torch.int64, device=DEV)
    xp = x[perm].contiguous()
    assert torch.equal(ops.feature_dropout(xp, 0.5, 234, seed_dev=word, row_ids=perm), ops.feature_dropout(xp, 0.5, 1234, row_ids=perm))
    assert torch.equal(ops.feature_dropout_bwd(xp, 0.5, 234, seed_dev=word, row_ids=perm), ops.feature_dropout_bwd(xp, 0.5, 1234, row_ids=perm))
    # rows of a larger graph: a rank's block in the middle of the whole activation
    big = torch.randn(3 * n, D, generator=torch.Generator().manual_seed(D)).to(DEV)
    ids = torch.arange(n, 2 * n, dtype=torch.int64, device=DEV)
    assert torch.equal(ops.feature_dropout(big[n:2 * n].clone(), 0.5, 99, row_ids=ids), ops.feature_dropout(big, 0.5, 99)[n:2 * n])
    with pytest.raises(ValueError, match="row_ids"):
        ops.feature_dropout(x, 0.5, 1, row_ids=perm[:-1])
    with pytest.raises(ValueError, match="row_ids"):
        ops.feature_dropout_bwd(x, 0.5, 1, row_ids=perm.int())


@pytest.mark.parametrize("n,D", [(8193, 513), (8200, 512)])
def test_feature_dropout_row_ids_past_the_grid_cap(n, D):
    """more quads than the capped grid holds in one trip, on the per-element path (D % 4 = 1, a ragged last quad) and on the aligned
    one"""
    tot = n * D
    # bgnn_appnp.hip launch_fdrop_rows: FDROP_ROWS_MAX_GRID = 4096 blocks of 256 lanes, one quad per lane and trip
    assert (tot + 3) // 4 > 4096 * 256
    assert (tot % 4 != 0) == (D % 4 != 0)
    _fdrop_pair(n, D, cases=((True, True), (False, False)))


# ---- the driver --------------------------------------------------------------------------------------------------
def _appnp(F_in, C, hidden, dropout, K=10, seed=0):
    from bridged_gnn_amd.appnp import APPNP_Net
    torch.manual_seed(seed)
    return APPNP_Net(types.SimpleNamespace(num_features=F_in, num_classes=C), hidden=hidden, dropout=dropout, K=K).to(DEV)


def test_world1_matches_appnp_net():
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_appnp import PartitionedAPPNP
    n = 5000
    ei = _graph(n, 40000, seed=8)
    x = torch.randn(n, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    y = torch.randint(0, 5, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tm = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) < 0.5
    data = Data(x=x, edge_index=_t(ei))
    m = _appnp(48, 5, 64, 0.5).eval()
    pa = PartitionedAPPNP(m, ei, n, 0, 1, DEV)
    own = pa.owned_global
    assert pa.n_halo == 0 and pa.n_local == n and pa.part.t.n_halo == 0
    with torch.no_grad():
        _bar_ok(pa.forward(x[own]).cpu(), m(data)[own].cpu(), ACT_BAR, "world 1 eval forward")
        for K in (0, 1, 2):                                # no state exchange at K <= 1, none at all at K = 0
            mk = _appnp(48, 5, 64, 0.5, K=K).eval()
            _bar_ok(PartitionedAPPNP(mk, ei, n, 0, 1, DEV).forward(x[own]).cpu(), mk(data)[own].cpu(), ACT_BAR, f"world 1 K={K}")
    # one training step with dropout 0.5 (the same host seeds and global-row masks)
    m2 = copy.deepcopy(m).train()
    m.train()
    pa = PartitionedAPPNP(m2, ei, n, 0, 1, DEV)
    torch.manual_seed(11)
    l1 = F.nll_loss(m(data)[tm], y[tm])
    l1.backward()
    torch.manual_seed(11)
    l2 = pa.nll_loss(pa.forward(x[own]), y[own], tm[own])
    l2.backward()
    pa.sync_grads()
    print(f"loss {l1.item():.8f} partitioned {l2.item():.8f}")
    assert abs(l1.item() - l2.item()) <= 2e-6 * abs(l1.item())
    for (k, a), b in zip(m.named_parameters(), m2.parameters()):
        err, top = (a.grad - b.grad).abs().max().item(), a.grad.abs().max().item()
        print(f"{k}: grad err {err / top:.3e} of max")
        assert err <= GRAD_BAR * top, k


@pytest.mark.parametrize("world", [2, 4, 8])
def test_simulated_ranks_eval_rows_match_single_gpu(world):
    """eval forward of every rank against `APPNP_Net`, and the backward's propagation -- P^T g through the transposed partition's
    tables, called directly: a barrier inside `backward` would block autograd's one device thread -- against the single-GPU
    walk of the by-source view"""
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_appnp import PartitionedAPPNP, _ext_rows, _propagate
    n_src, n_tar = 4000, 3000
    ei, mask = synth.bridged_graph(n_src, n_tar, 4, 8, 9000, cluster=128, p_local=0.8, seed=world)
    n = n_src + n_tar
    rng = np.random.default_rng(world)
    # node 2: a hub DESTINATION fed from every rank; node 1: a hub SOURCE feeding every rank -- a hub row of the transposed partition
    ei = np.concatenate([ei, np.stack([rng.choice(n, 1000, replace=False), np.full(1000, 2)]),
                         np.stack([np.full(3500, 1), rng.choice(n, 3500, replace=False)])], axis=1).astype(np.int64)
    x = torch.randn(n, 40, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world))
    C = 7
    G = torch.zeros(n, ops.pad4(C), device=DEV)
    G[:, :C] = torch.randn(n, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world + 100))
    m = _appnp(40, C, 64, 0.5).eval()
    data = Data(x=x, edge_index=_t(ei))
    g = m.graph(data.edge_index, n)
    with torch.no_grad():
        ref = m(data)
        ref_t = ops.appnp_propagate(G, g.t_rowptr, g.t_dst, g.dinv, n, C, 10, 0.1, hubs=g.t_hubs)[:, :C]
    for owner in (None, partition_nodes(mask, world)):
        box = _Box(world)
        res, errs = [None] * world, []

        def run(r):
            try:
                pa = PartitionedAPPNP(m, ei, n, r, world, DEV, owner=owner)
                pa.comm = _ThreadComm(box, r)
                with torch.no_grad():
                    out = pa.forward(x[pa.owned_global])
                    gx = _ext_rows(pa.t_tables, C, DEV)
                    ops.gather_rows(G[pa.owned_global].contiguous(), pa.t_from_f, out=gx[:pa.n_local])
                    dh = ops.gather_rows(_propagate(pa.comm, pa.t_tables, gx, C, 10, 0.1, None), pa.f_from_t)[:, :C]
                res[r] = (pa.owned_global, out, dh, pa.n_halo + pa.part.t.n_halo, pa.tables.hubs is not None, pa.t_tables.hubs is not None)
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
        assert sum(r[5] for r in res) >= 1, "the hub source is a hub row of its owner's transposed partition"
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        for r, (own, out, dh, _, _, _) in enumerate(res):
            _bar_ok(out.cpu(), ref[own].cpu(), ACT_BAR, f"world {world} rank {r} forward")
            _bar_ok(dh.cpu(), ref_t[own].cpu(), GRAD_BAR, f"world {world} rank {r} P^T g")
            seen[own] += 1
        assert bool((seen == 1).all()), "every node is covered once"


def test_out_of_scope_raises():
    from bridged_gnn_amd.dist_appnp import PartitionedAPPNP
    ei = _graph(200, 1000, seed=9)
    with pytest.raises(NotImplementedError, match="128 classes"):
        PartitionedAPPNP(_appnp(8, 130, 8, 0.0), ei, 200, 0, 1, DEV)
    with pytest.raises(NotImplementedError, match="graphed"):
        PartitionedAPPNP(_appnp(8, 3, 8, 0.0), ei, 200, 0, 1, DEV, graphed=True)
    pa = PartitionedAPPNP(_appnp(8, 3, 8, 0.0).eval(), ei, 200, 0, 1, DEV)
    with pytest.raises(RuntimeError, match="no CPU"):
        pa.forward(torch.zeros(200, 8))
    with pytest.raises(ValueError):
        pa.forward(torch.zeros(199, 8, device=DEV))


# ---- real ranks (gloo group, one GPU) ---------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth, transfer
        from bridged_gnn_amd.appnp import APPNP_Net
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_appnp import PartitionedAPPNP
        res = {}
        # (1) office graph, dropout 0: all-reduced loss and gradients, and this rank's ReLU pattern (compared in the parent with
        #     the fp64 restatement on that pattern)
        data = _office_data()
        n = data.x.shape[0]
        torch.manual_seed(0)
        m = APPNP_Net(transfer.pyg_dataset(data), hidden=64, dropout=0).to(DEV).train()
        pa = PartitionedAPPNP(m, data.edge_index.cpu().numpy(), n, rank, world, DEV)
        own = pa.owned_global
        seen = []
        hook = m.lin1.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))
        loss = pa.nll_loss(pa.forward(data.x[own]), data.y[own], data.train_mask[own])
        hook.remove()
        loss.backward()
        pa.sync_grads()
        tot = loss.detach().double().cpu().reshape(1)
        dist.all_reduce(tot)
        res["office"] = (float(tot), {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()}, own.cpu().numpy(),
                         (seen[0] > 0).cpu().numpy(), pa.n_halo)
        # (2) synth graph, dropout 0.5: three Adam steps against the single-GPU steps, then the same steps again
        n = 6000
        ei, _ = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        ei = np.concatenate([ei, ei[:, :500], np.stack([np.arange(0, n, 11)] * 2)], axis=1)   # duplicates + self loops
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, 5, (n,), device=DEV, generator=g)
        tm = torch.rand(n, device=DEV, generator=g) < 0.5
        data = Data(x=x, edge_index=_t(ei))
        torch.manual_seed(0)
        m0 = APPNP_Net(types.SimpleNamespace(num_features=64, num_classes=5), hidden=64, dropout=0.5).to(DEV).train()
        ref_m, runs = copy.deepcopy(m0), []

        def single():
            loss = F.nll_loss(ref_m(data)[tm], y[tm])
            loss.backward()
            return float(loss.detach())
        ref_rec, ref_par = _steps(ref_m, single)
        for _ in range(2):
            m = copy.deepcopy(m0)
            pa = PartitionedAPPNP(m, ei, n, rank, world, DEV)
            own = pa.owned_global
            xl = x[own].contiguous()

            def part():
                loss = pa.nll_loss(pa.forward(xl), y[own], tm[own])
                loss.backward()
                pa.sync_grads()
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
        res["synth"], res["summary"] = w, {"n_halo": pa.n_halo, "t_halo": pa.part.t.n_halo, "n_local": pa.n_local}
        q.put((rank, res))
    except Exception:                                            # report instead of leaving the parent waiting for the queue
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_real_ranks_train_appnp(world):
    import queue
    import socket
    import torch.multiprocessing as mp
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.appnp import APPNP_Net
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
        assert res[r]["summary"]["n_halo"] > 0 and res[r]["summary"]["t_halo"] > 0
    # (1) office: the all-reduced loss and gradients against the fp64 restatement on the ranks' ReLU pattern
    data = _office_data()
    n = data.x.shape[0]
    parts = _sparse_parts(data.edge_index.cpu(), n)
    torch.manual_seed(0)
    P = _params64(APPNP_Net(transfer.pyg_dataset(data), hidden=64))
    x64, y, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    mask = torch.zeros(n, 64, dtype=torch.float64)
    cover = np.zeros(n, dtype=np.int64)
    for r in range(world):
        _, _, own, pat, _ = res[r]["office"]
        mask[torch.from_numpy(own)] = torch.from_numpy(pat.astype(np.float64))
        cover[own] += 1
    assert (cover == 1).all() and sum(res[r]["office"][4] for r in range(world)) > 0
    loss, grads = res[0]["office"][:2]
    for r in range(1, world):                               # every rank holds the same all-reduced gradients
        assert all(np.array_equal(grads[k], res[r]["office"][1][k]) for k in grads)
    ref_loss = F.nll_loss(_restate(P, x64, parts, relu_mask=mask)[tm], y[tm])
    ref = dict(zip(P, torch.autograd.grad(ref_loss, list(P.values()))))
    print(f"office: loss {loss:.8f} fp64 {ref_loss.item():.8f}")
    assert abs(loss - ref_loss.item()) <= LOSS_BAR * abs(ref_loss.item())
    for k in ref:
        _bar_ok(grads[k], ref[k].numpy(), GRAD_BAR, f"office grad {k}")
    # (2) synth, dropout 0.5: three Adam steps against the single-GPU steps; a repeated run is bitwise equal
    for r in range(world):
        w = res[r]["synth"]
        assert w["loss"] <= LOSS_BAR and w["grad"] <= GRAD_BAR and w["param"] <= 1.0, (r, w)
        assert w["repeat"], (r, "two identical runs differ")
