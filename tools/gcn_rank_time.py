"""Compute side of ONE rank of an 8-way partition of the C4-shaped graph for GCN (bridged_gnn_amd.dist_gcn), on one GPU: the real
partition of rank r (GcnPartition: owned rows, extended CSR of A' + I, global-degree dinv, hub tables of both views, send lists,
segment CSR of the gradient return) with the collectives replaced by local stand-ins of the same size (all_to_all = a device
copy into a buffer of the received size, all-reduce = identity), as tools/sage_rank_time.py does for GraphSAGE.  The numbers are
the per-rank GPU work an 8-GPU run cannot go below; outputs are NOT the model's (the halo holds stand-in rows).  The single-GPU
`GCNNet` on the whole graph is timed in the same process, so the rank's share stands next to 1 / world of it.
Prints one JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/gcn_rank_time.py`."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import synth  # noqa: E402
from bridged_gnn_amd.data import Data  # noqa: E402
from bridged_gnn_amd.dist_gcn import PartitionedGCN  # noqa: E402
from bridged_gnn_amd.gcn import GCNNet  # noqa: E402


class StandInComm:
    """`dist_train._Comm` with the payload moved by a device copy of the received size instead of a collective"""
    live, host = True, False

    def all_to_all(self, send, send_splits, recv_splits):
        n = int(sum(recv_splits))
        recv = torch.zeros((n,) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
        k = min(n, send.shape[0])
        recv[:k].copy_(send[:k])
        return recv

    def all_reduce(self, t):
        return t


def timed(fn, reps):
    """median over `reps` single calls of device-event time (ms)"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def measure(forward, loss, model, reps, sync_grads=None):
    """(eval forward ms, training step ms) of one model: forward() -> log-probs, loss(out) -> scalar, sync_grads() after backward"""
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-3)

    def fwd_eval():
        with torch.no_grad():
            forward()

    def step():
        opt.zero_grad(set_to_none=True)
        loss(forward()).backward()
        if sync_grads is not None:
            sync_grads()
        opt.step()

    model.eval()
    fwd_eval()
    torch.cuda.synchronize()
    fwd_ms = timed(fwd_eval, reps * 2)
    model.train()
    for _ in range(3):
        step()
    return fwd_ms, timed(step, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gcn_rank_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)                  # tools/gcn_time.py's graph
    ds = types.SimpleNamespace(num_features=128, num_classes=2)
    x = torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=1)).to(dev)
    y = torch.randint(0, 2, (n,), device=dev)

    # the single-GPU model on the whole graph
    torch.manual_seed(0)
    m1 = GCNNet(ds, layer_num=2, hidden=64).to(dev)
    data = Data(x=x, edge_index=torch.from_numpy(ei).to(dev))
    single_fwd, single_step = measure(lambda: m1(data), lambda out: F.nll_loss(out, y), m1, a.reps)
    g1 = m1.graph(data.edge_index, n)
    single = {"eval_forward": round(single_fwd, 4), "train_step": round(single_step, 4),
              "hub_rows": 0 if g1.hubs is None else int(g1.hubs[1].shape[0]),
              "hub_sources": 0 if g1.t_hubs is None else int(g1.t_hubs[1].shape[0])}
    del m1, data, g1

    # one rank of the partition
    torch.manual_seed(0)
    m = GCNNet(ds, layer_num=2, hidden=64).to(dev)
    t0 = time.perf_counter()
    pg = PartitionedGCN(m, ei, n, a.rank, a.world, dev)
    plan_s = time.perf_counter() - t0
    pg.comm = StandInComm()
    xl = x[pg.owned_global].contiguous()
    yl = y[pg.owned_global]
    ones = torch.ones(pg.n_local, dtype=torch.bool, device=dev)

    fwd_ms, step_ms = measure(lambda: pg.forward(xl), lambda out: pg.nll_loss(out, yl, ones), m, a.reps, pg.sync_grads)
    p, t = pg.part, pg.tables
    line = {"tool": "gcn_rank_time", "measured": "one rank's GPU work, collectives replaced by device copies of the same size; "
            "no multi-GPU run", "nodes": n, "edges": int(ei.shape[1]), "world": a.world, "rank": a.rank,
            "n_local": p.n_local, "n_halo": p.n_halo, "send_rows": int(p.send_rows.shape[0]), "local_edges": p.num_edges,
            "hub_rows": 0 if t.hubs is None else int(t.hubs[1].shape[0]),
            "hub_sources": 0 if t.t_hubs is None else int(t.t_hubs[1].shape[0]),
            "halo_hub_sources": 0 if t.t_hubs is None else int((t.t_hubs[1] >= p.n_local).sum()),
            "plan_s": round(plan_s, 2), "eval_forward_ms": round(fwd_ms, 4), "train_step_ms": round(step_ms, 4),
            "single_gpu_ms": single,
            "rank_share_of_single_gpu": {"eval_forward": round(fwd_ms / single_fwd, 4), "train_step": round(step_ms / single_step, 4),
                                         "ideal": round(1.0 / a.world, 4)},
            "device": torch.cuda.get_device_name(0)}
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
