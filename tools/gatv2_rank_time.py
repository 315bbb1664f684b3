"""Compute side of ONE rank of an 8-way partition of the C4-shaped graph for GATv2 (bridged_gnn_amd.dist_gatv2), on one GPU: the
real partition of rank r (GatPartition: owned rows, extended CSR of A' + I, edge_base, both views, send lists, segment CSR of the
gradient return) with the collectives replaced by local stand-ins of the same size (all_to_all = a device copy into a buffer of
the received size, all-reduce = identity), as tools/gat_rank_time.py does for GAT.  The numbers are the per-rank GPU work an 8-GPU
run cannot go below; outputs are NOT the model's (the halo holds stand-in rows).  The single-GPU `GATv2` (hidden 64, 2 convs, one
head, dropout 0.6, attention dropout 0.5: the reference's) on the whole graph is timed in the same process, so the rank's share
stands next to 1 / world of it.
Prints one JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/gatv2_rank_time.py`."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gcn_rank_time import StandInComm, measure  # noqa: E402  (next to this file: the stand-in collectives and the timing loop)

from bridged_gnn_amd import synth  # noqa: E402
from bridged_gnn_amd.data import Data  # noqa: E402
from bridged_gnn_amd.dist_gatv2 import PartitionedGATv2  # noqa: E402
from bridged_gnn_amd.gatv2 import GATv2  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gatv2_rank_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)                  # tools/gatv2_time.py's graph
    x = torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=1)).to(dev)
    y = torch.randint(0, 2, (n,), device=dev)

    def model():
        torch.manual_seed(0)
        return GATv2(128, a.hidden, 2, a.layers, a.heads, 0.6, 0.5).to(dev)

    # the single-GPU model on the whole graph
    m1 = model()
    data = Data(x=x, edge_index=torch.from_numpy(ei).to(dev))
    single_fwd, single_step = measure(lambda: m1(data), lambda out: F.nll_loss(out, y), m1, a.reps)
    single = {"eval_forward": round(single_fwd, 4), "train_step": round(single_step, 4)}
    del m1, data

    # one rank of the partition
    m = model()
    t0 = time.perf_counter()
    pg = PartitionedGATv2(m, ei, n, a.rank, a.world, dev)
    plan_s = time.perf_counter() - t0
    pg.comm = StandInComm()
    xl = x[pg.owned_global].contiguous()
    yl = y[pg.owned_global]
    ones = torch.ones(pg.n_local, dtype=torch.bool, device=dev)

    fwd_ms, step_ms = measure(lambda: pg.forward(xl), lambda out: pg.nll_loss(out, yl, ones), m, a.reps, pg.sync_grads)
    p = pg.part
    line = {"tool": "gatv2_rank_time", "measured": "one rank's GPU work, collectives replaced by device copies of the same size; "
            "no multi-GPU run", "nodes": n, "edges": int(ei.shape[1]), "world": a.world, "rank": a.rank, "hidden": a.hidden,
            "heads": a.heads, "layers": a.layers, "dropout": m.dropout, "att_dropout": m.convs[0].dropout, "n_local": p.n_local,
            "n_halo": p.n_halo, "send_rows": int(p.send_rows.shape[0]), "local_edges": p.num_edges, "plan_s": round(plan_s, 2),
            "eval_forward_ms": round(fwd_ms, 4), "train_step_ms": round(step_ms, 4), "single_gpu_ms": single,
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
