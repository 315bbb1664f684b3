"""GPU: `dist_transfer.train_gnn_partitioned` -- step 2's KT-GNN training on a node partition -- IS the single-GPU eager run
(`transfer.train_gnn(graphed=False)`): office A->D graph, 6 epochs, hidden 64, dropout 0.5, StepLR(3), seed 0, at world 2 and 3 with
real ranks (gloo group, the ranks sharing the GPU; at most 3 ranks + this process hold it).

Bars: the four loss series within TRAJ_RTOL (2e-4, the project's bar for loss trajectories of equal-seed loops); the best epoch
equal; per epoch and combination |counts_partitioned - counts_single|.sum() <= 4, i.e. at most two rows whose argmax moved on a
near-tie (each moves one count out of a cell and one into another).  The single-GPU run's own eager-vs-graphed counts do not differ
on this input (tests/test_gpu_transfer_graphed.py::test_graphed_dropout_run_equals_the_eager_run asserts equal scores over 8 epochs of
this configuration), so the cap is not used up by the yardstick itself."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ_RTOL = 2e-4
COUNT_CAP = 4
ARGS = types.SimpleNamespace(dataset_name="office")
CFG = dict(repeat=1, num_epoch=6, step_size=3, gamma=0.1, gnn="KTGNN", seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)
_SINGLE = {}


def _office_data():
    """tests/golden/office_a2d_graph.npz preprocessed as the driver's `main` does (:404, :411)"""
    from bridged_gnn_amd.data import Data
    og = load_golden("office_a2d_graph.npz")
    d = Data(x=torch.from_numpy(og["x"]).to(DEV), edge_index=torch.from_numpy(og["edge_index"]).long().to(DEV),
             y=torch.from_numpy(og["y"]).long().to(DEV),
             **{k: torch.from_numpy(og[k]).to(DEV) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    d.train_mask[d.y == -1] = False
    d.to_undirected_()
    return d


def _series(lb):
    return np.array([lb["source&target"], lb["target_hat"], lb["target"], lb["kl"]]).T


def _single():
    """the single-GPU eager run, once for all tests of this file -> (loss_bucket, res_bucket_each, history, per-epoch counts)"""
    if not _SINGLE:
        from bridged_gnn_amd import transfer
        data = _office_data()
        counts, drain0 = [], transfer._History.drain

        def drain(self):                                         # the driver keeps scores only: look at the counts it drains
            rows = drain0(self)
            counts.extend(np.array(c) for _, c, _ in rows)
            return rows
        transfer._History.drain = drain
        try:
            hist = {}
            lb, each = transfer.train_gnn(ARGS, transfer.pyg_dataset(data), data, history=hist, graphed=False, **CFG)
        finally:
            transfer._History.drain = drain0
        _SINGLE.update(lb=lb, each=each, hist=hist, counts=counts)
    return _SINGLE


def _worker(rank, world, port, q, ckpt_root):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bridged_gnn_amd import dist_transfer, transfer
        data = _office_data()
        hist = {}
        lb, each = dist_transfer.train_gnn_partitioned(ARGS, transfer.pyg_dataset(data), data, rank, world, DEV, history=hist, save=True,
                                                       ckpt_dir=os.path.join(ckpt_root, f"rank{rank}"), **CFG)
        q.put((rank, {"lb": lb, "each": each, "hist": hist}))
    except Exception:                                            # report instead of leaving the parent waiting for the queue
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_run_is_the_single_gpu_eager_run(world, tmp_path):
    import socket
    import torch.multiprocessing as mp
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.ktgnn import KTGNN_no_complement
    single = _single()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(world):
        assert "error" not in res[r], res[r]["error"]
    r0 = res[0]
    for r in range(1, world):                                    # every rank returns the same buckets
        assert res[r]["lb"] == r0["lb"] and res[r]["each"] == r0["each"]
        assert res[r]["hist"]["eval_res"] == r0["hist"]["eval_res"] and res[r]["hist"]["best_epoch"] == r0["hist"]["best_epoch"]
    got, want = _series(r0["lb"]), _series(single["lb"])
    print("max rel dev per loss series", (np.abs(got - want) / np.abs(want)).max(0))
    assert got.shape == (6, 4) and np.allclose(got, want, rtol=TRAJ_RTOL), (got, want)
    assert r0["hist"]["best_epoch"] == single["hist"]["best_epoch"]
    c_got, c_want = np.array(r0["hist"]["counts"]), np.array(single["counts"])
    assert c_got.shape == c_want.shape and c_got.shape[:2] == (6, 5)
    moved = np.abs(c_got - c_want).reshape(6, 5, -1).sum(-1)
    print("counts that moved, per epoch and combination:\n", moved)
    assert (c_got.reshape(6, 5, -1).sum(-1) == c_want.reshape(6, 5, -1).sum(-1)).all(), "every scored row is counted once"
    assert moved.max() <= COUNT_CAP, moved
    # rank 0 alone saved; the file is the best epoch's model
    assert sorted(os.listdir(tmp_path)) == ["rank0"] and os.listdir(tmp_path / "rank0") == ["model_KTGNN_office_best.ckpt"]
    data = _office_data()
    C = int(data.y.max()) + 1
    model = KTGNN_no_complement(data.x.shape[1], C, 2, 64, root_weight=False, use_dist_loss=False, dropout=0.5, use_bn=True, step=1,
                                dim_share=data.x.shape[1], need_complement=False).to(DEV)
    model.load_state_dict(torch.load(tmp_path / "rank0" / "model_KTGNN_office_best.ckpt", map_location=DEV))
    best = r0["hist"]["best_epoch"]
    counts, _ = transfer._eval_dtc(data, model, transfer._plan(data, True))      # the eval forward + count launch `transfer.test` scores from
    moved = np.abs(counts.cpu().numpy() - c_got[best]).reshape(5, -1).sum(-1)
    print("saved model against the best epoch's counts:", moved)
    assert moved.max() <= COUNT_CAP, moved


def test_unsupported_modes_raise():
    from bridged_gnn_amd import dist_transfer
    with pytest.raises(NotImplementedError, match="auc"):
        dist_transfer.train_gnn_partitioned(ARGS, None, None, 0, 1, DEV, gnn="KTGNN", metric="auc")
    with pytest.raises(NotImplementedError, match="graphed"):    # refused before any rank or device is looked at
        dist_transfer.main(["--graphed"])
