"""Forward + backward of the partitioned BatchNorm1d -> ReLU -> dropout layer (`dist_train._SyncBnReluDrop`) at world size 1, where
its two collectives are identities: the torch path (`_SyncBnReluDropTorch`, the layer before the split-phase kernels) and the HIP
path, alternately in one process.  Shape: a rank's share of the benchmark graph, 125 000 rows x 128 columns, p = 0.5.
Also one eager partitioned epoch (`dist_transfer.train_gnn_partitioned`, rank 0 of world 1) next to the single-GPU eager epoch
(`transfer.train_gnn`) on the office A->D graph, as the slope between a short and a long run of each, alternating.
Prints one JSON line; `--readme PATH` writes it with a kernel table (`--kernel-stats`: the `*kernel_stats.csv` of a separate
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/sync_bn_time.py --skip-epoch --reps 3` run)."""
import argparse
import csv
import glob
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

from bridged_gnn_amd import dist_transfer, transfer  # noqa: E402
from bridged_gnn_amd.data import Data  # noqa: E402
from bridged_gnn_amd.dist_train import _Comm, _SyncBnReluDrop, _SyncBnReluDropTorch  # noqa: E402

DEV = "cuda:0"


def batch_ms(fn, iters):
    """device-event time of `iters` back-to-back calls, per call (ms)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def layer_times(rows, D, p, reps, iters):
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm1d(D).to(DEV).train()
    x = torch.randn(rows, D, device=DEV, requires_grad=True)
    gy = torch.randn(rows, D, device=DEV)
    ids = torch.arange(rows, device=DEV)
    comm = _Comm(None, DEV, 1)

    def torch_path():
        x.grad = None
        _SyncBnReluDropTorch.apply(x, bn.weight, bn.bias, bn, True, p, comm, rows).backward(gy)

    def hip_path():
        x.grad = None
        _SyncBnReluDrop.apply(x, bn.weight, bn.bias, bn, True, p, comm, rows, ids).backward(gy)

    for fn in (torch_path, hip_path):                   # warm-up of every shape the timed window uses
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t, h = [], []
    for _ in range(reps):                               # alternating: other work shares the host
        t.append(batch_ms(torch_path, iters))
        h.append(batch_ms(hip_path, iters))
    stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return {"rows": rows, "D": D, "p": p, "reps": reps, "iters_per_rep": iters, "torch_path": stat(t), "hip_path": stat(h),
            "torch_over_hip": round(float(np.median(t) / np.median(h)), 3)}


def office():
    og = dict(np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz")))
    d = Data(x=torch.from_numpy(og["x"]).to(DEV), edge_index=torch.from_numpy(og["edge_index"]).long().to(DEV),
             y=torch.from_numpy(og["y"]).long().to(DEV),
             **{k: torch.from_numpy(og[k]).to(DEV) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    d.train_mask[d.y == -1] = False
    d.to_undirected_()
    return d


def epoch_times(short, long, reps):
    data = office()
    args = types.SimpleNamespace(dataset_name="office")
    cfg = dict(repeat=1, step_size=100, gnn="KTGNN", seed=0, num_layer=2, hidden=64, dropout=0.5, verbose=False)

    def wall(run, epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(epochs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    single = lambda e: transfer.train_gnn(args, transfer.pyg_dataset(data), data, num_epoch=e, graphed=False, **cfg)
    part = lambda e: dist_transfer.train_gnn_partitioned(args, transfer.pyg_dataset(data), data, 0, 1, DEV, num_epoch=e, **cfg)
    single(2), part(2)
    s, q = [], []
    for _ in range(reps):
        s.append((wall(single, long) - wall(single, short)) / (long - short) * 1e3)
        q.append((wall(part, long) - wall(part, short)) / (long - short) * 1e3)
    return {"graph": "office A->D", "nodes": int(data.x.shape[0]), "epochs": [short, long], "reps": reps,
            "single_gpu_eager_epoch_ms": [round(v, 3) for v in s], "partitioned_world1_epoch_ms": [round(v, 3) for v in q]}


def kernel_table(path):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return "No kernel statistics were found.\n"
    rows = list(csv.DictReader(open(files[0])))
    out = ["| kernel | calls | average us | total ms | share % |", "|---|---|---|---|---|"]
    for r in rows[:16]:
        name = r.get("Name", "?").replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:80]
        out.append("| `{}` | {} | {:.1f} | {:.2f} | {} |".format(name, r.get("Calls", "?"), float(r.get("AverageNs", 0)) / 1e3,
                                                           float(r.get("TotalDurationNs", 0)) / 1e6, r.get("Percentage", "?")))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *kernel_stats.csv, or a directory holding one")
    ap.add_argument("--readme", default=None, help="write the line and the kernel table here (profiles/sync_bn/README.md)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sync_bn_time needs an MI355X"
    line = {"tool": "sync_bn_time", "device": torch.cuda.get_device_name(0), "world": 1,
            "layer_fwd_bwd": layer_times(a.rows, a.dim, a.p, a.reps, a.iters)}
    if not a.skip_epoch:
        line["epoch"] = epoch_times(5, 45, 3)
    s = json.dumps(line)
    print(s, flush=True)
    if a.readme:
        os.makedirs(os.path.dirname(os.path.abspath(a.readme)), exist_ok=True)
        with open(a.readme, "w") as f:
            f.write("# The partitioned BatchNorm -> ReLU -> dropout layer at world size 1 (`tools/sync_bn_time.py`) on one MI355X\n\n"
                    "Forward + backward of `dist_train._SyncBnReluDrop`, torch path and HIP path alternating in one process, the two\n"
                    "collectives being identities at world size 1; and one eager epoch of `dist_transfer.train_gnn_partitioned` (rank 0 of\n"
                    "world 1) next to `transfer.train_gnn(graphed=False)`.  No multi-GPU run.\n\n```\n" + s + "\n```\n\n"
                    "## Kernels (a `rocprofv3 --kernel-trace --stats` run of its own, `--skip-epoch --reps 3`)\n\n"
                    + (kernel_table(a.kernel_stats) if a.kernel_stats else "Not collected.\n"))


if __name__ == "__main__":
    main()
