"""GPU: the partitioned KT-GNN training step (dist_train.PartitionedTrainer) beyond 4 classes -- the wide three-head walk for
4 < C <= 32 and three per-conv walks above -- with REAL gloo ranks sharing the GPU (payload staged through the host), against the
single-GPU training step on the whole graph and, for office, against the reference's own fp64 gradients."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(target, world, *args, timeout=300):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q, *args)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in res:
        assert "error" not in r[1], r[1]["error"]
    return sorted(res, key=lambda r: r[0])


def _train_worker(rank, world, port, q, classes):
    """three SGD steps, partitioned vs the single-GPU default training step (tests/test_gpu_dist.py::_train_worker with C classes)"""
    import copy
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.pop("BGNN_WIDE_TRAIN_HEADS", None)             # the single-GPU side takes its default (per-conv) route
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_train import PartitionedTrainer
        from bridged_gnn_amd.ktgnn import KTGNN_no_complement
        from test_gpu_dist import _ref_loss
        n = 6000
        ei, mask = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        torch.manual_seed(0)
        model = KTGNN_no_complement(64, classes, 2, 64, use_bn=True, dim_share=64, dropout=0.0).to(DEV).train()
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, classes, (n,), device=DEV, generator=g)
        tm = torch.rand(n, device=DEV, generator=g) < 0.5
        cm = _t(mask)
        data = Data(x=x, edge_index=_t(ei), central_mask=cm)
        ref = copy.deepcopy(model)
        tr = PartitionedTrainer(model, ei, mask, rank, world, DEV)
        own = tr.owned_global
        o_ref, o_par = torch.optim.SGD(ref.parameters(), lr=0.05), torch.optim.SGD(model.parameters(), lr=0.05)
        worst = {"loss": 0.0, "out": 0.0, "grad": 0.0, "param": 0.0, "bn": 0.0, "grad_of": ""}
        for step in range(3):
            o_ref.zero_grad(set_to_none=True)
            out_r = ref(data)
            loss_r = _ref_loss(out_r, y, tm, cm, n)
            loss_r.backward()
            o_par.zero_grad(set_to_none=True)
            out_p = tr.forward(x[own].contiguous())
            loss_p = tr.reference_loss(out_p, y[own], tm[own])
            loss_p.backward()
            tr.sync_grads()
            tot = loss_p.detach().double().cpu().reshape(1)
            dist.all_reduce(tot)
            worst["loss"] = max(worst["loss"], abs(float(tot) - float(loss_r)) / abs(float(loss_r)))
            for a, b in zip(out_p, out_r[:3]):
                worst["out"] = max(worst["out"], float((a - b[own]).abs().max()))
            gmax = max(float(r.grad.abs().max()) for r in ref.parameters())
            for (nm, p), r in zip(model.named_parameters(), ref.parameters()):
                assert p.grad is not None and r.grad is not None, nm
                e = float((p.grad - r.grad).abs().max()) / (float(r.grad.abs().max()) + 1e-3 * gmax)
                if e > worst["grad"]:
                    worst["grad"], worst["grad_of"] = e, nm
            o_ref.step(); o_par.step()
            for p, r in zip(model.parameters(), ref.parameters()):
                worst["param"] = max(worst["param"], float((p - r).abs().max()))
            for b1, b2 in zip(model.buffers(), ref.buffers()):
                if b1.dtype.is_floating_point:
                    worst["bn"] = max(worst["bn"], float((b1 - b2).abs().max()))
        q.put((rank, worst, tr.plan.summary()))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}, {"n_halo": -1}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("classes,world", [(31, 2), (31, 3), (40, 2)])
def test_partitioned_training_beyond_four_classes_matches_the_single_gpu_step(classes, world):
    """C = 31: the wide three-head walk; C = 40: three per-conv walks over the same exchanged tables.  Bars of
    tests/test_gpu_dist.py::test_partitioned_training_step_matches_the_single_gpu_step."""
    for rank, w, summ in _run(_train_worker, world, classes):
        print(rank, w, summ)
        assert summ["n_halo"] > 0
        assert w["loss"] < 2e-6 and w["out"] < 2e-5 and w["grad"] < 3e-3 and w["param"] < 2e-6 and w["bn"] < 1e-6, (rank, w)


def _office_worker(rank, world, port, q, case):
    """one partitioned step of a reference fixture case: the all-reduced gradients and the summed loss (rank 0 reports them)"""
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd.dist_train import PartitionedTrainer
        from test_gpu_grads_reference import _setup
        c, model, data = _setup(case)
        tr = PartitionedTrainer(model, c["edge_index"], c["central_mask"], rank, world, DEV)
        own = tr.owned_global
        model.zero_grad(set_to_none=True)
        out = tr.forward(data.x[own].contiguous())
        loss = tr.reference_loss(out, data.y[own], data.train_mask[own])
        loss.backward()
        tr.sync_grads()
        tot = loss.detach().double().cpu().reshape(1)
        dist.all_reduce(tot)
        grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()} if rank == 0 else None
        q.put((rank, {"loss": float(tot), "grads": grads}, tr.plan.summary()))
    except Exception:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}, {"n_halo": -1}))
    finally:
        dist.destroy_process_group()


def test_partitioned_office_step_matches_reference_fp64_gradients():
    """office64 (31 classes) on two real ranks: the summed loss and the all-reduced gradients against the reference's own fp64
    training step (tests/golden/grads_office_a2d.npz) at the GRAD_BAR / kink-flip rules of test_gpu_grads_reference.py"""
    from oracle import grad_cases as GC
    from test_gpu_grads_reference import _check_grads, _oracle
    res = _run(_office_worker, 2, "office64")
    c = GC.load("office64")
    w = res[0][1]
    assert all(r[2]["n_halo"] > 0 for r in res)
    assert abs(w["loss"] - c["loss"][0]) <= 1e-6 * abs(c["loss"][0]), (w["loss"], c["loss"][0])
    _check_grads(c, _oracle("office64"), {k: torch.from_numpy(v) for k, v in w["grads"].items()}, "office64 partitioned (2 ranks)")
