"""Compute side of ONE rank of an 8-way partition of the C4-shaped graph for GCNII (bridged_gnn_amd.dist_gcn2), on one GPU: the real
partition of rank r (`dist_gcn.GcnPartition`: owned rows, extended CSR of A' + I, global-degree dinv, hub tables of both views,
send lists, segment CSR of the gradient return) with the collectives replaced by local stand-ins of the same size (all_to_all = a
device copy into a buffer of the received size, all-reduce = identity), as tools/gcn_rank_time.py does for GCN.  The numbers are
the per-rank GPU work an 8-GPU run cannot go below; outputs are NOT the model's (the halo holds stand-in rows).  Per hidden width
(64 and 128, `--num_layer` 4) it reports, next to the single-GPU `GCN2` on the whole graph timed in the same process:
  eval_forward_ms / train_step_ms : the rank's evaluation forward and its training step (forward, backward, sync_grads, Adam);
  conv_ms                         : one `ops.gcn2_conv` over the rank's rectangular graph (three launches with hub tables), evaluation
                                    form and training form (m written, dropout 0.5, row ids);
  pack_land_ms                    : one exchange's device passes, `ops.gather_rows` of the send list and the copy into the tail;
  model_bytes                     : the byte model per rank and layer, E_r (4H + 8) + n_local (8H + 4) + 4H^2 for the kernel plus
                                    4 pad4(H) bytes per send row and per halo row, and conv_model_GBps over the evaluation conv.
Every width runs in a child process of its own under a time limit (`--limit` seconds); the first child that fails ends the run.
Prints one JSON line per width.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gcn2_rank_time.py --child 64`."""
import argparse
import json
import math
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(a, H):
    import torch
    import torch.nn.functional as F

    from bridged_gnn_amd import ops, synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.dist_gcn2 import PartitionedGCN2, _exchange, _ext_rows
    from bridged_gnn_amd.gcn2 import GCN2, _mix_matrix
    from gcn_rank_time import StandInComm, measure, timed          # the stand-in collectives and the timing of tools/gcn_rank_time.py

    assert torch.cuda.is_available(), "gcn2_rank_time needs an MI355X"
    dev = torch.device("cuda:0")
    n, L = a.nodes, a.num_layer
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)                  # tools/gcn_time.py's graph
    ds = types.SimpleNamespace(num_features=128, num_classes=2)
    x = torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=1)).to(dev)
    y = torch.randint(0, 2, (n,), device=dev)

    # the single-GPU model on the whole graph
    torch.manual_seed(0)
    m1 = GCN2(ds, H, L, 0.1, 0.5, dropout=0.5).to(dev)
    data = Data(x=x, edge_index=torch.from_numpy(ei).to(dev))
    single_fwd, single_step = measure(lambda: m1(data), lambda out: F.nll_loss(out, y), m1, a.reps)
    del m1, data

    # one rank of the partition
    torch.manual_seed(0)
    m = GCN2(ds, H, L, 0.1, 0.5, dropout=0.5).to(dev)
    t0 = time.perf_counter()
    pg = PartitionedGCN2(m, ei, n, a.rank, a.world, dev)
    plan_s = time.perf_counter() - t0
    pg.comm = StandInComm()
    xl = x[pg.owned_global].contiguous()
    yl = y[pg.owned_global]
    ones = torch.ones(pg.n_local, dtype=torch.bool, device=dev)
    fwd_ms, step_ms = measure(lambda: pg.forward(xl), lambda out: pg.nll_loss(out, yl, ones), m, a.reps, pg.sync_grads)

    # one conv and one exchange's device passes, apart
    p, t = pg.part, pg.tables
    Hp = ops.pad4(H)
    cur, nxt = _ext_rows(pg, H, dev).normal_(), _ext_rows(pg, H, dev)
    x0 = torch.randn(p.n_local, Hp, device=dev)
    M = _mix_matrix(torch.randn(H, H, device=dev) / math.sqrt(H), math.log(1.5))
    mo = torch.empty(p.n_local, Hp, device=dev)
    rect = (M, t.rowptr_local, t.col, t.dinv, p.n_local, H, 0.1)

    def conv_eval():
        ops.gcn2_conv(cur, x0, *rect, hubs=t.hubs, out=nxt[:p.n_local])

    def conv_train():
        ops.gcn2_conv(cur, x0, *rect, p_drop=0.5, seed=1234, hubs=t.hubs, m_out=mo, out=nxt[:p.n_local], row_ids=t.owned_global)

    for f in (conv_eval, conv_train, lambda: _exchange(pg, cur)):
        f()
    torch.cuda.synchronize()
    conv_eval_ms, conv_train_ms = timed(conv_eval, a.reps * 2), timed(conv_train, a.reps * 2)
    pack_land_ms = timed(lambda: _exchange(pg, cur), a.reps * 2)
    n_send = int(p.send_rows.shape[0])
    kernel_bytes = p.num_edges * (4 * H + 8) + p.n_local * (8 * H + 4) + 4 * H * H
    line = {"tool": "gcn2_rank_time", "measured": "one rank's GPU work, collectives replaced by device copies of the same size; "
            "no multi-GPU run", "hidden": H, "num_layer": L, "nodes": n, "edges": int(ei.shape[1]), "world": a.world, "rank": a.rank,
            "n_local": p.n_local, "n_halo": p.n_halo, "send_rows": n_send, "local_edges": p.num_edges,
            "hub_rows": 0 if t.hubs is None else int(t.hubs[1].shape[0]),
            "hub_sources": 0 if t.t_hubs is None else int(t.t_hubs[1].shape[0]),
            "halo_hub_sources": 0 if t.t_hubs is None else int((t.t_hubs[1] >= p.n_local).sum()),
            "plan_s": round(plan_s, 2), "eval_forward_ms": round(fwd_ms, 4), "train_step_ms": round(step_ms, 4),
            "conv_ms": {"eval": round(conv_eval_ms, 4), "train": round(conv_train_ms, 4)}, "pack_land_ms": round(pack_land_ms, 4),
            "model_bytes": {"kernel": kernel_bytes, "exchange": 4 * Hp * (n_send + p.n_halo)},
            "conv_model_GBps": round(kernel_bytes / (conv_eval_ms * 1e-3) / 1e9, 1),
            "single_gpu_ms": {"eval_forward": round(single_fwd, 4), "train_step": round(single_step, 4)},
            "rank_share_of_single_gpu": {"eval_forward": round(fwd_ms / single_fwd, 4), "train_step": round(step_ms / single_step, 4),
                                         "ideal": round(1.0 / a.world, 4)},
            "device": torch.cuda.get_device_name(0)}
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--num_layer", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each width's child process, seconds")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", type=int, default=None, help="run one hidden width in this process")
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    for H in (64, 128):                                     # a fresh process per GPU step, each under its own time limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(H)] + sys.argv[1:]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"[gcn2_rank_time] H={H} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
