"""GPU: the partitioned KT-GNN training step WITH dropout (the reference's 0.5) is the single-GPU step: `dist_train._SyncBnReluDrop`
runs the single-GPU BatchNorm -> ReLU -> dropout kernels in four phases and draws the single-GPU seeds, so a rank's masks are its
rows of the whole-graph masks.  Real ranks (gloo group, payload staged through the host because RCCL refuses two ranks per device),
production kernels.  The step, the data and the bars are those of
tests/test_gpu_dist.py::test_partitioned_training_step_matches_the_single_gpu_step, which runs at dropout 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ref_loss(out, y, tm, cm, n):
    """main_graph_knowledge_transfer.py:44-54 on the whole graph"""
    import torch.nn.functional as F
    lb, lt, lth = out[:3]
    tmt = tm & ~cm
    yi = y[:, None]
    nll = lambda logp, w: -(logp.gather(1, yi).squeeze(1) * w).sum()
    return (2 * nll(lb, tm.float() / tm.sum()) + nll(lt, tmt.float() / tmt.sum()) + nll(lth, tmt.float() / tmt.sum())) / 4 \
        + F.kl_div(lth, lt, log_target=True, reduction="batchmean")


def _train_worker(rank, world, port, q, layers):
    import copy
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import synth
        from bridged_gnn_amd.data import Data
        from bridged_gnn_amd.dist_train import PartitionedTrainer
        from bridged_gnn_amd.ktgnn import KTGNN_no_complement
        n = 6000
        ei, mask = synth.bridged_graph(3500, 2500, 4, 8, 7000, cluster=128, p_local=0.8, seed=4)
        torch.manual_seed(0)
        model = KTGNN_no_complement(64, 3, layers, 64, use_bn=True, dim_share=64, dropout=0.5).to(DEV).train()
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, 64, device=DEV, generator=g)
        y = torch.randint(0, 3, (n,), device=DEV, generator=g)
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
            torch.manual_seed(100 + step)                        # the host generator both forwards draw their dropout seeds from
            out_r = ref(data)
            loss_r = _ref_loss(out_r, y, tm, cm, n)
            loss_r.backward()
            o_par.zero_grad(set_to_none=True)
            torch.manual_seed(100 + step)
            out_p = tr.forward(x[own].contiguous())
            loss_p = tr.reference_loss(out_p, y[own], tm[own])
            loss_p.backward()
            tr.sync_grads()
            tot = loss_p.detach().double().cpu().reshape(1)
            dist.all_reduce(tot)
            worst["loss"] = max(worst["loss"], abs(float(tot) - float(loss_r)) / abs(float(loss_r)))
            for a, b in zip(out_p, out_r[:3]):
                worst["out"] = max(worst["out"], float((a - b[own]).abs().max()))
            # (error of a tensor relative to its own largest gradient plus 1e-3 of the largest gradient of the model: see test_gpu_dist.py)
            gmax = max(float(r.grad.abs().max()) for r in ref.parameters())
            for (nm, p), r in zip(model.named_parameters(), ref.parameters()):
                assert p.grad is not None and r.grad is not None, nm
                e = float((p.grad - r.grad).abs().max()) / (float(r.grad.abs().max()) + 1e-3 * gmax)
                if e > worst["grad"]:
                    worst["grad"], worst["grad_of"] = e, f"{nm} (|ref| max {float(r.grad.abs().max()):.2e}, model max {gmax:.2e})"
            o_ref.step(); o_par.step()
            for p, r in zip(model.parameters(), ref.parameters()):
                worst["param"] = max(worst["param"], float((p - r).abs().max()))
            for b1, b2 in zip(model.buffers(), ref.buffers()):
                if b1.dtype.is_floating_point:
                    worst["bn"] = max(worst["bn"], float((b1 - b2).abs().max()))
        q.put((rank, worst, tr.plan.summary()))
    except Exception:                                            # report instead of leaving the parent waiting for the queue
        import traceback
        q.put((rank, {"error": traceback.format_exc()}, {"n_halo": -1}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,layers", [(2, 2), (3, 2), (2, 3)])
def test_partitioned_training_step_with_dropout_matches_the_single_gpu_step(world, layers):
    """three SGD steps at dropout 0.5 against the same steps of the single-GPU training path on the whole graph, the host generator
    re-seeded alike before the two forwards: loss 2e-6, owned outputs 2e-5, all-reduced gradients 3e-3 (by the existing test's rule),
    parameters 2e-6, BatchNorm buffers 1e-6.  With masks drawn by `torch.rand_like` per rank the loss alone misses by orders of
    magnitude."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_train_worker, args=(r, world, port, q, layers)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, w, summ in res:
        print(rank, w, summ)
        assert "error" not in w, w["error"]
        assert summ["n_halo"] > 0
        assert w["loss"] < 2e-6 and w["out"] < 2e-5 and w["grad"] < 3e-3 and w["param"] < 2e-6 and w["bn"] < 1e-6, (rank, w)
