"""GPU: GIN on a destination-node partition (bridged_gnn_amd.dist_gin) -- world 1 against `GINNet` at 1, 2 and 3 layers, dropout 0
and 0.5, unsegmented (outputs bitwise) and at hub_cfg (8, 5), with the bars of test_world1_matches_gcnnet (loss 2e-6 relative,
parameters after one Adam step 2e-6); simulated worlds 2/4/8 in one process (ranks as threads) on a bridged graph with a planted hub
row and a planted hub source at hub_cfg (32, 16): the eval rows and the backward's dT after return and fold against the single-GPU
run; REAL ranks in a gloo group sharing the GPU: all-reduced gradients (every eps included) on the office graph against the fp64
restatement of test_gin_host.py on the ranks' own ReLU patterns, three Adam steps at dropout 0.5 against the single-GPU steps,
twice, the second run bitwise the first; and the refusals.
Bars: test_gpu_gcn.py's (activations 1e-5, gradients 2e-5 of each tensor's max) and test_gpu_gcn_partition.py's (Adam parameters
1e-4, losses 1e-5 relative), imported."""
import copy
import threading
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gin_host import mult_adj, restate
from test_gpu_appnp import _office_data
from test_gpu_gcn import ACT_BAR, GRAD_BAR, _bar_ok
from test_gpu_gcn_partition import ADAM_BAR, LOSS_BAR, _Box, _graph, _steps, _t, _ThreadComm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OFFICE_L, OFFICE_H = 3, 32


def _gin(F_in, C, L, hidden, dropout, seed=0, eps=None):
    from bridged_gnn_amd.gin import GINNet
    torch.manual_seed(seed)
    m = GINNet(types.SimpleNamespace(num_features=F_in, num_classes=C), layer_num=L, hidden=hidden, dropout=dropout).to(DEV)
    if eps is not None:                                     # away from the initial 0, so that a dropped eps shows
        with torch.no_grad():
            for k, conv in enumerate(m.convs):
                conv.eps.fill_(eps * (k + 1))
    return m


# ---- world 1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub_cfg", [None, (8, 5)])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_world1_matches_ginnet(L, hub_cfg):
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_gin import PartitionedGIN
    n = 5000
    ei = _graph(n, 40000, seed=8)
    x = torch.randn(n, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    y = torch.randint(0, 5, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tm = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) < 0.5
    data = Data(x=x, edge_index=_t(ei))
    for dropout in (0.0, 0.5):
        what = f"L={L} hubs={hub_cfg} dropout={dropout}"
        m = _gin(48, 5, L, 64, dropout, eps=0.2).eval()
        pg = PartitionedGIN(m, ei, n, 0, 1, DEV, hub_cfg=hub_cfg)
        own = pg.owned_global
        assert pg.n_halo == 0 and pg.n_local == n
        assert (pg.tables.hubs is not None and pg.tables.t_hubs is not None) == (hub_cfg is not None)
        with torch.no_grad():
            ref, got = m(data)[own], pg.forward(x[own])
        _bar_ok(got.cpu(), ref.cpu(), ACT_BAR, what + " eval forward")
        if hub_cfg is None:
            assert torch.equal(got, ref), what + ": unsegmented, the eval outputs are the single-GPU bits"
        # one training step (the same host seeds and global-row masks)
        m2 = copy.deepcopy(m).train()
        m.train()
        pg = PartitionedGIN(m2, ei, n, 0, 1, DEV, hub_cfg=hub_cfg)
        o1 = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
        o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, weight_decay=5e-3)
        torch.manual_seed(11)
        out1 = m(data)
        l1 = F.nll_loss(out1[tm], y[tm])
        l1.backward()
        torch.manual_seed(11)
        out2 = pg.forward(x[own])
        l2 = pg.nll_loss(out2, y[own], tm[own])
        l2.backward()
        pg.sync_grads()
        if hub_cfg is None:
            assert torch.equal(out2.detach(), out1.detach()[own]), what + ": unsegmented, the training outputs are the single-GPU bits"
        print(f"{what} loss {l1.item():.8f} partitioned {l2.item():.8f}")
        assert abs(l1.item() - l2.item()) <= 2e-6 * abs(l1.item())
        names = [k for k, _ in m.named_parameters()]
        assert (f"convs.{L - 1}.eps" in names) == (L > 1)
        for (k, a), b in zip(m.named_parameters(), m2.parameters()):
            assert b.grad is not None, k
            _bar_ok(b.grad.cpu(), a.grad.cpu().numpy(), GRAD_BAR, f"{what} grad {k}")
        o1.step(); o2.step()
        for (k, a), b in zip(m.named_parameters(), m2.parameters()):
            assert (a - b).abs().max().item() <= 2e-6, k


def test_more_than_128_classes_run_through_torchs_log_softmax():
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_gin import PartitionedGIN
    ei = _graph(200, 1000, seed=9)
    x = torch.randn(200, 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    m = _gin(8, 130, 2, 8, 0.0).eval()
    pg = PartitionedGIN(m, ei, 200, 0, 1, DEV)
    with torch.no_grad():
        got, ref = pg.forward(x[pg.owned_global]), m(Data(x=x, edge_index=_t(ei)))[pg.owned_global]
    assert got.shape == (200, 130)
    _bar_ok(got.cpu(), ref.cpu(), ACT_BAR, "130 classes")


# ---- simulated ranks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4, 8])
def test_simulated_ranks_eval_rows_and_backward_match_single_gpu(world):
    """eval forward of every rank against `GINNet` (L = 3, hidden 64), and a conv's backward -- `dist_gin._conv_backward`: the walk
    over the by-source view with its hub tables, the returned halo rows and the fold, called directly (a barrier inside `backward`
    would block autograd's one device thread) -- against the single-GPU `ops.gin_aggregate_bwd`"""
    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist import partition_nodes
    from bridged_gnn_amd.dist_gin import PartitionedGIN, _conv_backward
    n_src, n_tar = 4000, 3000
    ei, mask = synth.bridged_graph(n_src, n_tar, 4, 8, 9000, cluster=128, p_local=0.8, seed=world)
    n = n_src + n_tar
    rng = np.random.default_rng(world)
    # node 2: a hub ROW fed from every rank; node 1: a hub SOURCE feeding rows of every rank (a halo slot that is a hub of the
    # by-source view on the ranks that do not own it)
    ei = np.concatenate([ei, np.stack([rng.choice(n, 1000, replace=False), np.full(1000, 2)]),
                         np.stack([np.full(3500, 1), rng.choice(n, 3500, replace=False)])], axis=1).astype(np.int64)
    x = torch.randn(n, 40, device=DEV, generator=torch.Generator(device=DEV).manual_seed(world))
    H = 64
    gen = torch.Generator(device=DEV).manual_seed(world + 100)
    T = torch.randn(n, H, device=DEV, generator=gen)
    gy = torch.randn(n, H, device=DEV, generator=gen)
    m = _gin(40, 7, 3, H, 0.5, eps=0.2).eval()
    data = Data(x=x, edge_index=_t(ei))
    g = m.graph(data.edge_index, n)
    eps = m.convs[0].eps.detach()
    with torch.no_grad():
        ref = m(data)
        ref_t, ref_b, ref_e = ops.gin_aggregate_bwd(T, None, gy, g.by_dst[2], g.by_dst[3], eps, n, H)
    for owner in (None, partition_nodes(mask, world)):
        box = _Box(world)
        res, errs = [None] * world, []

        def run(r):
            try:
                pg = PartitionedGIN(m, ei, n, r, world, DEV, owner=owner, hub_cfg=(32, 16))
                pg.comm = _ThreadComm(box, r)
                th, own = pg.tables.t_hubs, pg.owned_global
                with torch.no_grad():
                    out = pg.forward(x[own])
                    dT, gb, ge = _conv_backward(pg, T[own].contiguous(), None, gy[own].contiguous(), eps, H, None, 0.0, True, True)
                res[r] = (own, out, dT, gb, ge, pg.n_halo, pg.tables.hubs is not None,
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
        assert max(r[5] for r in res) > 0, "no halo at all"
        assert sum(r[6] for r in res) >= 1, "no rank owns a hub row"
        assert sum(r[7] for r in res) >= 1, "no rank holds a halo slot that is a hub source"
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        for r, (own, out, dT, _, _, _, _, _) in enumerate(res):
            _bar_ok(out.cpu(), ref[own].cpu(), ACT_BAR, f"world {world} rank {r} forward")
            _bar_ok(dT.cpu(), ref_t[own].cpu(), GRAD_BAR, f"world {world} rank {r} dT after return and fold")
            seen[own] += 1
        assert bool((seen == 1).all()), "every node is covered once"
        _bar_ok(sum(r[3].double() for r in res).cpu(), ref_b.double().cpu(), GRAD_BAR, f"world {world} grad_bias, summed over the ranks")
        ge = sum(r[4].double() for r in res).item()
        assert abs(ge - ref_e.item()) <= GRAD_BAR * (gy.double() * T.double()).abs().sum().item(), f"world {world} grad_eps"


def test_out_of_scope_raises():
    from bridged_gnn_amd.dist_gin import PartitionedGIN
    ei = _graph(200, 1000, seed=9)
    with pytest.raises(NotImplementedError, match="graphed"):
        PartitionedGIN(_gin(8, 3, 2, 8, 0.0), ei, 200, 0, 1, DEV, graphed=True)
    with pytest.raises(RuntimeError, match="no CPU"):
        PartitionedGIN(_gin(8, 3, 2, 8, 0.0), ei, 200, 0, 1, "cpu")
    with pytest.raises(ValueError, match="hub_cfg"):
        PartitionedGIN(_gin(8, 3, 2, 8, 0.0), ei, 200, 0, 1, DEV, hub_cfg=(0, 5))
    pg = PartitionedGIN(_gin(8, 3, 2, 8, 0.0).eval(), ei, 200, 0, 1, DEV)
    with pytest.raises(RuntimeError, match="no CPU"):
        pg.forward(torch.zeros(200, 8))
    with pytest.raises(ValueError):
        pg(torch.zeros(199, 8, device=DEV))


# ---- real ranks (gloo group, one GPU) ---------------------------------------------------------------------------------
def _layer_outputs(out):
    """the conv outputs y kept by the autograd nodes of `_PartGinLayerFn` / `_GinLayerFn` (ctx.y), first conv first"""
    ys, seen, stack = [], set(), [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        if "GinLayerFn" in type(fn).__name__:
            ys.append(fn.y)
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
        from bridged_gnn_amd.dist_gin import PartitionedGIN
        from bridged_gnn_amd.gin import GINNet
        res = {}
        # (a) office graph, dropout 0: all-reduced loss and gradients, and this rank's ReLU patterns (compared in the parent with
        #     the fp64 restatement on those patterns)
        data = _office_data()
        n = data.x.shape[0]
        torch.manual_seed(0)
        m = GINNet(transfer.pyg_dataset(data), OFFICE_L, OFFICE_H, dropout=0.0).to(DEV).train()
        with torch.no_grad():
            for k, conv in enumerate(m.convs):
                conv.eps.fill_(0.1 * (k + 1))
        pg = PartitionedGIN(m, data.edge_index.cpu().numpy(), n, rank, world, DEV, hub_cfg=(32, 16))
        own = pg.owned_global
        out = pg.forward(data.x[own])
        ys = _layer_outputs(out)
        assert len(ys) == OFFICE_L
        loss = pg.nll_loss(out, data.y[own], data.train_mask[own])
        loss.backward()
        pg.sync_grads()
        tot = loss.detach().double().cpu().reshape(1)
        dist.all_reduce(tot)
        res["office"] = (float(tot), {k: p.grad.double().cpu().numpy() for k, p in m.named_parameters()}, own.cpu().numpy(),
                         [(y[:, :OFFICE_H] > 0).cpu().numpy() for y in ys[:-1]], pg.n_halo)
        # (b) synth graph, dropout 0.5: three Adam steps against the single-GPU steps, then the same steps again
        n = 6000
        ei, _ = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        rng = np.random.default_rng(5)
        # duplicates + self loops, a hub row (node 2) and a hub source (node 1) at hub_cfg (32, 16)
        ei = np.concatenate([ei, ei[:, :500], np.stack([np.arange(0, n, 11)] * 2), np.stack([rng.choice(n, 400, replace=False), np.full(400, 2)]),
                             np.stack([np.full(1200, 1), rng.choice(n, 1200, replace=False)])], axis=1).astype(np.int64)
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, 5, (n,), device=DEV, generator=g)
        tm = torch.rand(n, device=DEV, generator=g) < 0.5
        data = Data(x=x, edge_index=_t(ei))
        torch.manual_seed(0)
        m0 = GINNet(types.SimpleNamespace(num_features=64, num_classes=5), 3, 64, dropout=0.5).to(DEV).train()
        ref_m, runs = copy.deepcopy(m0), []

        def single():
            lp = ref_m(data)
            loss = F.nll_loss(lp[tm], y[tm])
            loss.backward()
            return float(loss.detach())
        ref_rec, ref_par = _steps(ref_m, single)
        for _ in range(2):
            m = copy.deepcopy(m0)
            pg = PartitionedGIN(m, ei, n, rank, world, DEV, hub_cfg=(32, 16))
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
        res["synth"] = w
        res["summary"] = {"n_halo": pg.n_halo, "n_local": pg.n_local, "hubs": pg.tables.hubs is not None,
                          "t_hubs": pg.tables.t_hubs is not None}
        q.put((rank, res))
    except Exception:                                            # report instead of leaving the parent waiting for the queue
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_real_ranks_train_gin(world):
    import queue
    import socket
    import torch.multiprocessing as mp
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.gin import GINNet
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
    assert any(res[r]["summary"]["hubs"] for r in range(world)) and any(res[r]["summary"]["t_hubs"] for r in range(world))
    # (a) office: the all-reduced loss and gradients against the fp64 restatement on the ranks' own ReLU patterns
    data = _office_data()
    n = data.x.shape[0]
    torch.manual_seed(0)
    ref_m = GINNet(transfer.pyg_dataset(data), OFFICE_L, OFFICE_H, dropout=0.0)
    with torch.no_grad():
        for k, conv in enumerate(ref_m.convs):
            conv.eps.fill_(0.1 * (k + 1))
    P = {k: v.detach().double().requires_grad_(True) for k, v in ref_m.state_dict().items()}
    x64, y, tm = data.x.double().cpu(), data.y.cpu(), data.train_mask.cpu()
    A = mult_adj(data.edge_index.cpu(), n)
    relus = [torch.zeros(n, OFFICE_H, dtype=torch.float64) for _ in range(OFFICE_L - 1)]
    cover = np.zeros(n, dtype=np.int64)
    for r in range(world):
        _, _, own, pats, _ = res[r]["office"]
        for l in range(OFFICE_L - 1):
            relus[l][torch.from_numpy(own)] = torch.from_numpy(pats[l].astype(np.float64))
        cover[own] += 1
    assert (cover == 1).all() and sum(res[r]["office"][4] for r in range(world)) > 0
    loss, grads = res[0]["office"][:2]
    assert sorted(grads) == sorted(P) and sum(k.endswith(".eps") for k in grads) == OFFICE_L
    for r in range(1, world):                               # every rank holds the same all-reduced gradients
        assert all(np.array_equal(grads[k], res[r]["office"][1][k]) for k in grads)
    ref_loss = F.nll_loss(restate(P, x64, A, relu_masks=relus)[tm], y[tm])
    ref = dict(zip(P, torch.autograd.grad(ref_loss, list(P.values()))))
    print(f"office: loss {loss:.8f} fp64 {ref_loss.item():.8f}")
    assert abs(loss - ref_loss.item()) <= LOSS_BAR * abs(ref_loss.item())
    for k in ref:
        _bar_ok(grads[k], ref[k].numpy(), GRAD_BAR, f"office grad {k}")
    # (b) synth, dropout 0.5: three Adam steps against the single-GPU steps; a repeated run is bitwise equal
    for r in range(world):
        w = res[r]["synth"]
        assert w["loss"] <= LOSS_BAR and w["grad"] <= GRAD_BAR and w["param"] <= 1.0, (r, w)
        assert w["repeat"], f"rank {r}: the second run is not bitwise the first"
