"""Compute side of ONE rank of an 8-way partition of the C4-shaped graph for GraphSAGE (bridged_gnn_amd.dist_sage), on one GPU:
the real partition of rank r (SagePartition: owned rows, extended CSR, send lists, segment CSR of the gradient return) with the
collectives replaced by local stand-ins of the same size (all_to_all = a device copy into a buffer of the received size,
all-reduce = identity), as tools/rank_of_8_time.py does for KT-GNN.  The numbers are the per-rank GPU work an 8-GPU run cannot
go below, next to the single-GPU 0.98 / 3.96 ms of profiles/sage/; outputs are NOT the model's (the halo holds stand-in rows).
Prints one JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/sage_rank_time.py`."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import synth  # noqa: E402
from bridged_gnn_amd.dist_sage import PartitionedGraphSAGE  # noqa: E402
from bridged_gnn_amd.sage import GraphSAGE  # noqa: E402

SINGLE_GPU_MS = {"eval_forward": 0.98, "train_step": 3.96}      # profiles/sage/sage_time.json


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sage_rank_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)                  # tools/sage_time.py's graph
    torch.manual_seed(0)
    m = GraphSAGE(types.SimpleNamespace(num_features=128, num_classes=2), layer_num=2, hidden=64).to(dev)
    t0 = time.perf_counter()
    ps = PartitionedGraphSAGE(m, ei, n, a.rank, a.world, dev)
    plan_s = time.perf_counter() - t0
    ps.comm = StandInComm()
    x = torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=1)).to(dev)
    xl = x[ps.owned_global].contiguous()
    y = torch.randint(0, 2, (ps.n_local,), device=dev)
    ones = torch.ones(ps.n_local, dtype=torch.bool, device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)

    def fwd_eval():
        with torch.no_grad():
            ps.forward(xl)

    def step():
        opt.zero_grad(set_to_none=True)
        ps.nll_loss(ps.forward(xl), y, ones).backward()
        ps.sync_grads()
        opt.step()

    m.eval()
    fwd_eval()
    torch.cuda.synchronize()
    fwd_ms = timed(fwd_eval, a.reps * 2)
    m.train()
    for _ in range(3):
        step()
    step_ms = timed(step, a.reps)
    p = ps.part
    line = {"tool": "sage_rank_time", "measured": "one rank's GPU work, collectives replaced by device copies of the same size; "
            "no multi-GPU run", "nodes": n, "edges": int(ei.shape[1]), "world": a.world, "rank": a.rank,
            "n_local": p.n_local, "n_halo": p.n_halo, "send_rows": int(p.send_rows.shape[0]), "local_edges": p.num_edges,
            "plan_s": round(plan_s, 2), "eval_forward_ms": round(fwd_ms, 4), "train_step_ms": round(step_ms, 4),
            "single_gpu_ms": SINGLE_GPU_MS,
            "speedup_vs_single_gpu": {"eval_forward": round(SINGLE_GPU_MS["eval_forward"] / fwd_ms, 2),
                                      "train_step": round(SINGLE_GPU_MS["train_step"] / step_ms, 2)},
            "device": torch.cuda.get_device_name(0)}
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
