"""Compute side of ONE rank of an 8-way partition of the C4-shaped graph for GIN (bridged_gnn_amd.dist_gin), on one GPU: the real
partition of rank r (`dist_sage.SagePartition`, the edges as given: owned rows, extended CSR, hub tables of both views, send lists,
segment CSR of the gradient return) with the collectives replaced by local stand-ins of the same size (all_to_all = a device copy
into a buffer of the received size, all-reduce = identity), as tools/gcn2_rank_time.py does for GCNII.  The numbers are the per-rank
GPU work an 8-GPU run cannot go below; outputs are NOT the model's (the halo holds stand-in rows).  Per hidden width (64 and 128,
`--num_layer` 2, two classes) it reports, next to the single-GPU `GINNet` on the whole graph timed in the same process:
  eval_forward_ms / train_step_ms : the rank's evaluation forward and its training step (forward, backward, sync_grads, Adam);
  agg_ms                          : one `ops.gin_aggregate_hubs` over the rank's rectangular graph at the hidden width (ReLU,
                                    dropout 0.5, row ids) and one `ops.gin_aggregate_bwd_hubs` over its by-source view;
  pack_land_ms                    : one exchange's device passes, `ops.gather_rows` of the send list and the copy into the tail;
  exchange_bytes_per_layer        : 4 pad4(D) bytes per send row and per halo row at every layer's output width D, from the shapes.
`--hub_cfg 0 0` runs the rank unsegmented.  Every width runs in a child process of its own under a time limit (`--limit` seconds);
the first child that fails ends the run.  Prints one JSON line per width."""
import argparse
import json
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
    from bridged_gnn_amd.dist_gin import PartitionedGIN
    from bridged_gnn_amd.gin import GINNet
    from gcn_rank_time import StandInComm, measure, timed          # the stand-in collectives and the timing of tools/gcn_rank_time.py

    assert torch.cuda.is_available(), "gin_rank_time needs an MI355X"
    dev = torch.device("cuda:0")
    n, L, C = a.nodes, a.num_layer, 2
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)                  # tools/gin_time.py's graph
    ds = types.SimpleNamespace(num_features=128, num_classes=C)
    x = torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=1)).to(dev)
    y = torch.randint(0, C, (n,), device=dev)
    hub_cfg = tuple(a.hub_cfg) if a.hub_cfg[0] > 0 else None

    # the single-GPU model on the whole graph
    torch.manual_seed(0)
    m1 = GINNet(ds, L, H, dropout=0.5, segment_hubs=hub_cfg is not None).to(dev)
    data = Data(x=x, edge_index=torch.from_numpy(ei).to(dev))
    single_fwd, single_step = measure(lambda: m1(data), lambda out: F.nll_loss(out, y), m1, a.reps)
    del m1, data

    # one rank of the partition
    torch.manual_seed(0)
    m = GINNet(ds, L, H, dropout=0.5).to(dev)
    t0 = time.perf_counter()
    pg = PartitionedGIN(m, ei, n, a.rank, a.world, dev, hub_cfg=hub_cfg)
    plan_s = time.perf_counter() - t0
    pg.comm = StandInComm()
    xl = x[pg.owned_global].contiguous()
    yl = y[pg.owned_global]
    ones = torch.ones(pg.n_local, dtype=torch.bool, device=dev)
    fwd_ms, step_ms = measure(lambda: pg.forward(xl), lambda out: pg.nll_loss(out, yl, ones), m, a.reps, pg.sync_grads)

    # one aggregation each way and one exchange's device passes, apart
    p, t = pg.part, pg.tables
    Hp = ops.pad4(H)
    buf = torch.randn(p.n_ext, Hp, device=dev)
    gy = torch.randn(p.n_local, Hp, device=dev)
    eps = torch.tensor([0.3], device=dev)
    out = torch.empty(p.n_local, Hp, device=dev)
    dT = torch.empty(p.n_ext, Hp, device=dev)

    def agg_fwd():
        return ops.gin_aggregate_hubs(buf, t.rowptr_local, t.col, eps, p.n_local, H, epilogue="relu", p_drop=0.5, seed=1234,
                                      row_ids=t.owned_global, hubs=t.hubs, out=out)

    def agg_bwd():
        return ops.gin_aggregate_bwd_hubs(buf[:p.n_local], out, gy, t.t_rowptr, t.t_dst, eps, p.n_ext, H, epilogue="relu", p_drop=0.5,
                                          grad_tbl=dT, hubs=t.t_hubs)

    def exchange():
        send = ops.gather_rows(buf, t.send_rows)
        recv = pg.comm.all_to_all(send, p.send_splits, p.recv_splits)
        if p.n_halo:
            buf[p.n_local:].copy_(recv)

    for f in (agg_fwd, agg_bwd, exchange):
        f()
    torch.cuda.synchronize()
    agg_fwd_ms, agg_bwd_ms = timed(agg_fwd, a.reps * 2), timed(agg_bwd, a.reps * 2)
    pack_land_ms = timed(exchange, a.reps * 2)
    n_send = int(p.send_rows.shape[0])
    widths = [H] * (L - 1) + [C] if L > 1 else [C]
    line = {"tool": "gin_rank_time", "measured": "one rank's GPU work, collectives replaced by device copies of the same size; "
            "no multi-GPU run", "hidden": H, "num_layer": L, "nodes": n, "edges": int(ei.shape[1]), "world": a.world, "rank": a.rank,
            "hub_cfg": hub_cfg, "n_local": p.n_local, "n_halo": p.n_halo, "send_rows": n_send, "local_edges": p.num_edges,
            "hub_rows": 0 if t.hubs is None else int(t.hubs[1].shape[0]),
            "hub_sources": 0 if t.t_hubs is None else int(t.t_hubs[1].shape[0]),
            "halo_hub_sources": 0 if t.t_hubs is None else int((t.t_hubs[1] >= p.n_local).sum()),
            "plan_s": round(plan_s, 2), "eval_forward_ms": round(fwd_ms, 4), "train_step_ms": round(step_ms, 4),
            "agg_ms": {"forward": round(agg_fwd_ms, 4), "backward": round(agg_bwd_ms, 4)}, "pack_land_ms": round(pack_land_ms, 4),
            "exchange_bytes_per_layer": [4 * ops.pad4(D) * (n_send + p.n_halo) for D in widths],
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
    ap.add_argument("--num_layer", type=int, default=2)
    ap.add_argument("--hub_cfg", type=int, nargs=2, default=[256, 128], help="(threshold, segment); 0 0 = unsegmented")
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each width's child process, seconds")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", type=int, default=None, help="run one hidden width in this process")
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    for H in a.widths:                                      # a fresh process per GPU step, each under its own time limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(H)] + sys.argv[1:]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"[gin_rank_time] H={H} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
