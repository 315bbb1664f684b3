"""GPU: GraphSAGE on a destination-node partition (bridged_gnn_amd.dist_sage) -- the two kernels it adds (row-id dropout hashing,
the deterministic segment add of returned gradient rows), world 1 against the single-GPU model, simulated worlds 2/4/8 in one
process (ranks as threads, the exchange by row copies), and REAL ranks in a gloo group sharing the GPU (payload staged through
the host, kernels the production ones): gradients against the reference's fp64 gradients on the office graph, and three Adam
steps with dropout 0.5 against the single-GPU steps."""
import threading
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DS = (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 64, 100, 128, 200)     # the widths of test_gpu_graphsage.py
GRAD_BAR, KINK_CAP = 2e-5, 2e-4                                  # test_gpu_graphsage.py's bars


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _graph(n, e, seed, hubs=False):
    from bridged_gnn_amd import synth
    ei, _ = synth.random_multigraph(n, e, n_isolated=max(n // 50, 1), seed=seed)
    extra = [ei, ei[:, : e // 20], np.stack([np.arange(0, n, 7), np.arange(0, n, 7)])]   # duplicates + self loops
    if hubs:
        rng = np.random.default_rng(seed)
        extra.append(np.stack([rng.integers(0, n, 6000), np.full(6000, 3)]))             # node 3: >= 5000 in-edges
    return np.concatenate(extra, axis=1).astype(np.int64)


# ---- kernels ---------------------------------------------------------------------------------------------------------
def test_row_ids_identity_is_the_plain_kernel():
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.sage import SageGraph
    n = 3000
    g = SageGraph(_t(_graph(n, 30000, seed=1, hubs=True)), n)
    rowptr, col = g.view(False)[:2]
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    gen = torch.Generator().manual_seed(2)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.randn(n, 2 * Dp, generator=gen).to(DEV)
        for epi, p in ((None, 0.0), ("relu", 0.0), ("relu", 0.5), ("log_softmax", 0.0)):
            if epi == "log_softmax" and D > 128:
                continue
            a = ops.sage_mean_aggregate(T[:, :Dp], rowptr, col, n, D, root=T[:, Dp:], epilogue=epi, p_drop=p, seed=77)
            b = ops.sage_mean_aggregate(T[:, :Dp], rowptr, col, n, D, root=T[:, Dp:], epilogue=epi, p_drop=p, seed=77, row_ids=ids)
            assert torch.equal(a, b), f"D={D} epi={epi} p={p}"


def test_row_ids_carry_the_masks_to_permuted_rows():
    """a row-permuted CSR with row_ids = the permutation gives bitwise the rows of the unpermuted call, dropout 0.5 included"""
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.sage import SageGraph
    n = 3000
    g = SageGraph(_t(_graph(n, 30000, seed=3, hubs=True)), n)
    rowptr, col = g.view(False)[:2]
    rp = rowptr.long().cpu()
    colc = col[: int(rp[-1])].cpu()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(4))
    deg = (rp[1:] - rp[:-1])[perm]
    rowptr_p = torch.zeros(n + 1, dtype=torch.int64)
    rowptr_p[1:] = torch.cumsum(deg, 0)
    col_p = torch.cat([colc[rp[i]:rp[i + 1]] for i in perm.tolist()])
    rowptr_p, col_p, perm_d = rowptr_p.to(torch.int32).to(DEV), col_p.to(DEV), perm.to(DEV)
    gen = torch.Generator().manual_seed(5)
    for D in DS:
        Dp = ops.pad4(D)
        T = torch.randn(n, 2 * Dp, generator=gen).to(DEV)
        ref = ops.sage_mean_aggregate(T[:, :Dp], rowptr, col, n, D, root=T[:, Dp:], epilogue="relu", p_drop=0.5, seed=99)
        got = ops.sage_mean_aggregate(T[:, :Dp], rowptr_p, col_p, n, D, root=T[perm_d, Dp:], epilogue="relu", p_drop=0.5, seed=99,
                                      row_ids=perm_d)
        assert torch.equal(got, ref[perm_d]), f"D={D}"
        # without the ids the permuted call draws other masks (what a rank would get from local row numbers)
        plain = ops.sage_mean_aggregate(T[:, :Dp], rowptr_p, col_p, n, D, root=T[perm_d, Dp:], epilogue="relu", p_drop=0.5, seed=99)
        assert not torch.equal(plain, ref[perm_d]), f"D={D}"


def test_rows_segment_add_matches_fp64_and_is_deterministic():
    from bridged_gnn_amd import ops
    rng = np.random.default_rng(6)
    n_src, n_dst, n_seg = 20000, 5000, 3000
    sizes = rng.integers(0, 6, n_seg)
    sizes[::97] = 0                                                    # empty segments
    sizes[5], sizes[1000] = 6000, 5200                                 # hub-sized segments
    seg_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    idx = rng.integers(0, n_src, int(seg_ptr[-1])).astype(np.int32)
    row = rng.choice(n_dst, n_seg, replace=False).astype(np.int32)
    seg_row = np.repeat(row, sizes)
    for D in (1, 3, 4, 8, 31, 64, 200):
        Dp = ops.pad4(D)
        src = torch.from_numpy(rng.standard_normal((n_src, Dp)).astype(np.float32))
        dst0 = torch.from_numpy(rng.standard_normal((n_dst, Dp)).astype(np.float32))
        for acc in (True, False):
            ref = dst0.double().clone()
            if not acc:
                ref[torch.from_numpy(row).long()] = 0
            ref.index_add_(0, torch.from_numpy(seg_row).long(), src.double()[torch.from_numpy(idx).long()])
            outs = []
            for _ in range(2):
                dst = dst0.to(DEV)
                ops.rows_segment_add(src.to(DEV), _t(seg_ptr), _t(idx), _t(row), dst, D=D, accumulate=acc)
                outs.append(dst)
            assert torch.equal(outs[0], outs[1]), f"D={D}: two runs differ"
            got = outs[0].cpu().double()
            err = (got[:, :D] - ref[:, :D]).abs().max().item()
            assert err <= 1e-5 * ref[:, :D].abs().max().item() + 1e-5, f"D={D} accumulate={acc}: {err:.3e}"
            if Dp > D:     # pad columns of the written rows are 0, every other row is untouched
                assert torch.count_nonzero(got[torch.from_numpy(row).long(), D:]).item() == 0
            rest = np.setdiff1d(np.arange(n_dst), row)
            assert torch.equal(got[rest], dst0[rest].double())
    # a strided column slice as the destination (dT_l half of an interleaved [n, 2 Dp] table): bitwise the contiguous call (the
    # summation order does not depend on the stride), and within the bar above of the fp64 sums; the other columns untouched
    gen = torch.Generator().manual_seed(7)
    big0 = torch.randn(n_dst, 16, generator=gen)
    src = torch.randn(n_src, 8, generator=gen)
    big = big0.to(DEV)
    ops.rows_segment_add(src.to(DEV), _t(seg_ptr), _t(idx), _t(row), big[:, :8], accumulate=True)
    flat = big0[:, :8].contiguous().to(DEV)
    ops.rows_segment_add(src.to(DEV), _t(seg_ptr), _t(idx), _t(row), flat, accumulate=True)
    got = big.cpu()
    assert torch.equal(got[:, :8], flat.cpu()) and torch.equal(got[:, 8:], big0[:, 8:])
    ref = big0[:, :8].double().index_add_(0, torch.from_numpy(seg_row).long(), src.double()[torch.from_numpy(idx).long()])
    err = (got[:, :8].double() - ref).abs().max().item()
    assert err <= 1e-5 * ref.abs().max().item() + 1e-5, f"strided destination: {err:.3e}"


# ---- the driver ------------------------------------------------------------------------------------------------------
def _sage(F_in, C, L, hidden, dropout, seed=0):
    from bridged_gnn_amd.sage import GraphSAGE
    torch.manual_seed(seed)
    return GraphSAGE(types.SimpleNamespace(num_features=F_in, num_classes=C), layer_num=L, hidden=hidden, dropout=dropout).to(DEV)


def _hidden_outputs(out):
    """the layer outputs kept by the autograd nodes of the SAGE layer functions (ctx.y), first conv first"""
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


def test_world1_matches_graphsage():
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_sage import PartitionedGraphSAGE
    n = 5000
    ei = _graph(n, 40000, seed=8)
    x = torch.randn(n, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    y = torch.randint(0, 5, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tm = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) < 0.5
    data = Data(x=x, edge_index=_t(ei))
    for L in (1, 2, 3):
        m = _sage(48, 5, L, 64, 0.5).eval()
        ps = PartitionedGraphSAGE(m, ei, n, 0, 1, DEV)
        own = ps.owned_global
        with torch.no_grad():
            ref = m(data)
            got = ps.forward(x[own])
        assert torch.allclose(got, ref[own], rtol=1e-6, atol=1e-6)
        assert torch.equal(got, ref[own]), f"L={L}: both CSRs keep the input edge order, so the bits agree"
        # one training step with dropout 0.5 (the same host seeds and global-row masks)
        import copy
        m2 = copy.deepcopy(m).train()
        m.train()
        ps = PartitionedGraphSAGE(m2, ei, n, 0, 1, DEV)
        o1, o2 = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3), torch.optim.Adam(m2.parameters(), lr=1e-3, weight_decay=5e-3)
        torch.manual_seed(11)
        l1 = F.nll_loss(m(data)[tm], y[tm])
        l1.backward()
        torch.manual_seed(11)
        l2 = ps.nll_loss(ps.forward(x[own]), y[own], tm[own])
        l2.backward()
        ps.sync_grads()
        assert abs(l1.item() - l2.item()) <= 2e-6 * abs(l1.item())
        for (k, a), b in zip(m.named_parameters(), m2.parameters()):
            assert (a.grad - b.grad).abs().max().item() <= 1e-5 * a.grad.abs().max().item() + 1e-12, k
        o1.step(); o2.step()
        for a, b in zip(m.parameters(), m2.parameters()):
            assert (a - b).abs().max().item() <= 2e-6


class _Box:
    def __init__(self, world):
        self.world, self.slots = world, [None] * world
        self.bar = threading.Barrier(world, timeout=300)


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
    from bridged_gnn_amd.dist_sage import PartitionedGraphSAGE
    n_src, n_tar = 4000, 3000
    ei, mask = synth.bridged_graph(n_src, n_tar, 4, 8, 9000, cluster=128, p_local=0.8, seed=world)
    n = n_src + n_tar
    x = torch.randn(n, 40, device=DEV)
    for L, owner in ((2, None), (3, partition_nodes(mask, world))):
        m = _sage(40, 7, L, 64, 0.5).eval()
        with torch.no_grad():
            ref = m(Data(x=x, edge_index=_t(ei)))
        box = _Box(world)
        res, errs = [None] * world, []

        def run(r):
            try:
                ps = PartitionedGraphSAGE(m, ei, n, r, world, DEV, owner=owner)
                ps.comm = _ThreadComm(box, r)
                with torch.no_grad():
                    res[r] = (ps.owned_global, ps.forward(x[ps.owned_global]), ps.n_halo)
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
        assert sum(h for _, _, h in res) > 0
        seen = torch.zeros(n, dtype=torch.bool, device=DEV)
        for own, out, _ in res:
            assert torch.allclose(out, ref[own], rtol=1e-6, atol=1e-6), f"world {world} L={L}"
            seen[own] = True
        assert bool(seen.all())


def test_out_of_scope_raises():
    from bridged_gnn_amd.dist_sage import PartitionedGraphSAGE
    ei = _graph(200, 1000, seed=9)
    m = _sage(8, 3, 2, 8, 0.0)
    ps = PartitionedGraphSAGE(m, ei, 200, 0, 1, DEV)
    with pytest.raises(NotImplementedError):
        ps.get_emb(None)
    with pytest.raises(NotImplementedError):
        ps.get_logits(None)
    m.convs[0].normalize = True
    with pytest.raises(NotImplementedError):
        PartitionedGraphSAGE(m, ei, 200, 0, 1, DEV)
    with pytest.raises(NotImplementedError):
        PartitionedGraphSAGE(_sage(8, 130, 2, 8, 0.0), ei, 200, 0, 1, DEV)


# ---- real ranks (gloo group, one GPU) ---------------------------------------------------------------------------------
OFFICE_MODELS = (("l2h64", 2, 64), ("l1", 1, 16), ("l3h32", 3, 32))


def _office(variant):
    from bridged_gnn_amd.data import Data
    g = load_golden("office_a2d_graph.npz")
    data = Data(x=torch.from_numpy(g["x"]).to(DEV), edge_index=torch.from_numpy(g["edge_index"]).long().to(DEV),
                y=torch.from_numpy(g["y"]).long().to(DEV))
    if variant == "und":
        data.to_undirected_()                               # ToUndirected(merge=True), main_graph_knowledge_transfer.py:411
    tm = torch.from_numpy(g["train_mask"]).to(DEV)
    tm[data.y == -1] = False
    return data, tm, types.SimpleNamespace(num_features=g["x"].shape[1], num_classes=int(g["y"].max()) + 1)


def _restate(P, x, ei, L, relu_masks=None):
    """fp64 GraphSAGE (eval form) on the CPU; relu_masks: force the ReLU pattern of the hidden layers"""
    src, dst = ei[0], ei[1]
    n = x.shape[0]
    cnt = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64)).clamp(min=1)
    h = x
    for i in range(L):
        c = f"convs.{i}."
        agg = torch.zeros(n, h.shape[1], dtype=torch.float64).index_add_(0, dst, h[src]) / cnt[:, None]
        h = agg @ P[c + "lin_l.weight"].t() + P[c + "lin_l.bias"] + h @ P[c + "lin_r.weight"].t()
        if i < L - 1:
            h = h * relu_masks[i] if relu_masks is not None else torch.relu(h)
    return torch.log_softmax(h, 1)


def _steps(m, run, steps=3):
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)
    rec = []
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        torch.manual_seed(100 + step)                      # the host generator behind the dropout seeds
        loss, hidden = run()
        rec.append((loss, {k: p.grad.clone() for k, p in m.named_parameters()}, hidden))
        opt.step()
    return rec, {k: p.detach().clone() for k, p in m.named_parameters()}


def _rank_worker(rank, world, port, q):
    import copy
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_sage import PartitionedGraphSAGE
        from bridged_gnn_amd.sage import GraphSAGE
        res = {"office": {}, "summary": None}
        # (1) office graph, dropout 0: all-reduced gradients (compared in the parent with the reference's fp64 gradients)
        for variant in ("raw", "und"):
            data, tm, ds = _office(variant)
            ei = data.edge_index.cpu().numpy()
            n = data.x.shape[0]
            for name, L, hidden in OFFICE_MODELS:
                torch.manual_seed(0)
                m = GraphSAGE(ds, layer_num=L, hidden=hidden, root_weight=True, dropout=0.0).to(DEV).train()
                ps = PartitionedGraphSAGE(m, ei, n, rank, world, DEV)
                own = ps.owned_global
                out = ps.forward(data.x[own])
                loss = ps.nll_loss(out, data.y[own], tm[own])
                loss.backward()
                ps.sync_grads()
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
        m0 = GraphSAGE(types.SimpleNamespace(num_features=64, num_classes=5), layer_num=3, hidden=64, dropout=0.5).to(DEV).train()
        ref_m, runs = copy.deepcopy(m0), []

        def single():
            out = ref_m(data)
            loss = F.nll_loss(out[tm], y[tm])
            loss.backward()
            return float(loss.detach()), [h[:, :64] for h in _hidden_outputs(out)]
        ref_rec, ref_par = _steps(ref_m, single)
        for _ in range(2):
            m = copy.deepcopy(m0)
            ps = PartitionedGraphSAGE(m, ei, n, rank, world, DEV)
            own = ps.owned_global
            xl = x[own].contiguous()                        # one tensor: its halo rows are fetched once

            def part():
                out = ps.forward(xl)
                loss = ps.nll_loss(out, y[own], tm[own])
                loss.backward()
                ps.sync_grads()
                tot = loss.detach().double().cpu().reshape(1)
                dist.all_reduce(tot)
                return float(tot), [h[:, :64] for h in _hidden_outputs(out)]
            runs.append(_steps(m, part))
        w = {"loss": 0.0, "param": 0.0, "grad": 0.0, "grad_of": "", "pattern": True, "repeat": True}
        for (lr_, gr, hr), (lp, gp, hp) in zip(ref_rec, runs[0][0]):
            w["loss"] = max(w["loss"], abs(lp - lr_) / abs(lr_))
            for k in gr:
                e = float((gp[k] - gr[k]).abs().max()) / float(gr[k].abs().max())
                if e > w["grad"]:
                    w["grad"], w["grad_of"] = e, k
            assert len(hr) == len(hp) == 2
            w["pattern"] = w["pattern"] and all(torch.equal(a[own] == 0, b == 0) for a, b in zip(hr, hp))
        for k in ref_par:
            w["param"] = max(w["param"], float((runs[0][1][k] - ref_par[k]).abs().max()))
        (r1, p1), (r2, p2) = runs
        w["repeat"] = (all(a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1]) for a, b in zip(r1, r2))
                       and all(torch.equal(p1[k], p2[k]) for k in p1))
        res["synth"], res["summary"] = w, {"n_halo": ps.n_halo, "n_local": ps.n_local}
        q.put((rank, res))
    except Exception:                                            # report instead of leaving the parent waiting for the queue
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_real_ranks_train_graphsage(world):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        assert "error" not in res[r], res[r]["error"]
        print(r, res[r]["synth"], res[r]["summary"])
        assert res[r]["summary"]["n_halo"] > 0
    # (1) office: the all-reduced gradients against the reference's fp64 gradients (raw: the fixture; und: the fp64 restatement,
    #     which tests/test_graphsage_host.py pins to the fixture), with test_gpu_graphsage.py's ReLU-kink handling
    fx = load_golden("graphsage_office_a2d.npz")
    for variant in ("raw", "und"):
        data, tm, _ = _office(variant)
        x64, ei, y, tmc = data.x.double().cpu(), data.edge_index.cpu(), data.y.cpu(), tm.cpu()
        for name, L, hidden in OFFICE_MODELS:
            key = f"{variant}/{name}"
            loss, grads, _, _ = res[0]["office"][key]
            for r in range(1, world):                       # every rank holds the same all-reduced gradients
                assert all(np.array_equal(grads[k], res[r]["office"][key][1][k]) for k in grads)
            torch.manual_seed(0)                            # the fixture's initial parameters (test_gpu_graphsage.py checks their sums)
            from bridged_gnn_amd.sage import GraphSAGE
            m = GraphSAGE(types.SimpleNamespace(num_features=x64.shape[1], num_classes=int(y.max()) + 1), layer_num=L, hidden=hidden)
            P = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}

            def ref_grads(masks=None):
                if masks is None and f"{key}/grad/convs.0.lin_l.weight" in fx:
                    return float(fx[f"{key}/loss"]), {k: fx[f"{key}/grad/{k}"] for k in P}
                lo = F.nll_loss(_restate(P, x64, ei, L, masks)[tmc], y[tmc])
                return lo.item(), {k: g.numpy() for k, g in zip(P, torch.autograd.grad(lo, list(P.values())))}
            ref_loss, ref = ref_grads()
            assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), key
            bad = []
            for k in ref:
                err = np.abs(grads[k] - ref[k]).max()
                if err > GRAD_BAR * np.abs(ref[k]).max():
                    assert err <= KINK_CAP * np.abs(ref[k]).max(), f"{key} {k}: {err:.3e} beyond any ReLU kink flip"
                    bad.append(k)
            if bad:                                          # the fp64 restatement with the ranks' ReLU pattern
                masks = [torch.zeros(x64.shape[0], hidden, dtype=torch.float64) for _ in range(L - 1)]
                for r in range(world):
                    _, _, own, pats = res[r]["office"][key]
                    for i, pat in enumerate(pats):
                        masks[i][torch.from_numpy(own)] = torch.from_numpy(pat.astype(np.float64))
                _, ref = ref_grads(masks)
                for k in ref:
                    err = np.abs(grads[k] - ref[k]).max()
                    assert err <= GRAD_BAR * np.abs(ref[k]).max() + 1e-6, f"{key} {k} (ranks' ReLU pattern): {err:.3e}"
                print(f"{key}: ReLU kink flips explained for {bad}")
    # (2) synth, dropout 0.5: three Adam steps against the single-GPU steps; a repeated run is bitwise equal
    for r in range(world):
        w = res[r]["synth"]
        assert w["loss"] <= 2e-6 and w["param"] <= 2e-6 and w["grad"] <= 1e-5, (r, w)
        assert w["pattern"], (r, "the hidden convs' zero pattern on the owned rows differs from the single-GPU pattern")
        assert w["repeat"], (r, "two identical runs differ")
