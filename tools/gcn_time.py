"""Times the GCN normalised aggregation (ops.gcn_aggregate / gcn_aggregate_bwd) on a C4-shaped graph (synth.bridged_graph, 1M
nodes / 20M edges + one self loop per node) at D = 64 (ReLU + dropout epilogue) and D = 4 (log_softmax epilogue), and an office
epoch of `train_gnn_noDTC(gnn='GCN')` eager and graphed.  One JSON line.  Per width, in this process, alternating blocks:
  fused_fwd / fused_bwd : the one-launch forward and the backward (row pass + by-source walk + column sums);
  composed_fwd          : the same layer from the ops that existed before -- `ops.sage_mean_aggregate(mean=False)` over a
                          dinv-scaled table, then torch for the row scale, the bias and ReLU + dropout / log_softmax;
  torch_fwd             : torch eager (index_add_ of dinv-weighted rows, same epilogue);
  sage_sibling_fwd      : `bgnn_sage_mean_aggregate_f32` at the same width (its edge loop moves the same rows, without the
                          4 B dinv gather).
Byte model of the fused forward: E'(4D + 4 + 4) + N(4D + 4D + 4); `fwd_frac_of_8TBps` is that over the time as a share of
8 TB/s (a fabric-side figure: most gathers are L2 hits).  Timing: a warm-up, a rehearsal burst, then one event pair round K
launches per sample; the median of the samples.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gcn_time.py --skip-office` (profiles/gcn/README.md)."""
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

from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.gcn import GcnGraph  # noqa: E402

FABRIC_BPS = 8e12


def burst(fn, k):
    """ms per call over one event pair round k launches"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def alternate(fns, rounds, k):
    """the candidates in alternating blocks -> median ms per call of each"""
    for f in fns.values():
        f()
        burst(f, k)                               # rehearsal burst
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            ts[name].append(burst(f, k))
    return {name: float(np.median(v)) for name, v in ts.items()}


def office_epochs(graphed, epochs):
    from bridged_gnn_amd import transfer
    from bridged_gnn_amd.data import Data
    og = dict(np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz")))
    dev = torch.device("cuda:0")
    d = Data(x=torch.from_numpy(og["x"]).to(dev), edge_index=torch.from_numpy(og["edge_index"]).long().to(dev),
             y=torch.from_numpy(og["y"]).long().to(dev),
             **{k: torch.from_numpy(og[k]).to(dev) for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    d.train_mask[d.y == -1] = False
    d.to_undirected_()
    args = types.SimpleNamespace(dataset_name="office")
    out = []
    for n in (4, epochs, 2 * epochs):              # a warm-up run, then the difference of two run lengths leaves the per-run set-up out
        torch.cuda.synchronize()
        t = time.perf_counter()
        transfer.train_gnn_noDTC(args, transfer.pyg_dataset(d), d, repeat=1, num_epoch=n, gnn="GCN", seed=0, num_layer=2, hidden=64,
                                 use_scheduler=False, verbose=False, graphed=graphed)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return (out[2] - out[1]) / epochs * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, default=10, help="launches per event pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--office-epochs", type=int, default=200)
    ap.add_argument("--skip-office", action="store_true")
    ap.add_argument("--office-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gcn_time needs an MI355X"
    dev = torch.device("cuda:0")
    if a.office_only:
        print(json.dumps({"tool": "gcn_time", "office_epoch_ms": {"eager": round(office_epochs(False, a.office_epochs), 4),
                                                                  "graphed": round(office_epochs(True, a.office_epochs), 4)}}))
        return
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)
    g = GcnGraph(torch.from_numpy(ei).to(dev), n)
    E = int(g.csr.num_edges)
    rowptr, col, dinv = g.csr.rowptr, g.col, g.dinv
    src, dst = col.long(), torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).long())
    w_edge = (dinv[src] * dinv[dst]).unsqueeze(1)
    res = {"tool": "gcn_time", "nodes": n, "edges_with_self_loops": E, "hub_rows": 0 if g.hubs is None else int(g.hubs[1].shape[0]),
           "hub_sources": 0 if g.t_hubs is None else int(g.t_hubs[1].shape[0]), "widths": {}}
    for D, epi in ((64, "relu"), (4, "log_softmax")):
        p = 0.5 if epi == "relu" else 0.0
        T = torch.randn(n, D, device=dev)
        b = torch.randn(D, device=dev)
        dy = torch.randn(n, D, device=dev)
        zero_root = None

        def epilogue(z):
            return F.dropout(F.relu(z), p=p, training=True) if epi == "relu" else F.log_softmax(z, dim=1)

        def fused():
            return ops.gcn_aggregate(T, rowptr, col, dinv, n, D, bias=b, epilogue=epi, p_drop=p, seed=7, hubs=g.hubs)

        def composed():
            s = ops.sage_mean_aggregate(T * dinv.unsqueeze(1), rowptr, col, n, D, root=zero_root, mean=False)
            return epilogue(s * dinv.unsqueeze(1) + b)

        def torch_eager():
            return epilogue(torch.zeros(n, D, device=dev).index_add_(0, dst, T[src] * w_edge) + b)

        def sibling():
            return ops.sage_mean_aggregate(T, rowptr, col, n, D, root=None, mean=True, epilogue=epi, p_drop=p, seed=7)

        yv = fused()

        def fused_bwd():
            return ops.gcn_aggregate_bwd(yv, dy, g.t_rowptr, g.t_dst, dinv, n, D, epilogue=epi, p_drop=p, hubs=g.t_hubs)

        err = float((ops.gcn_aggregate(T, rowptr, col, dinv, n, D, bias=b, hubs=g.hubs)
                     - (ops.sage_mean_aggregate(T * dinv.unsqueeze(1), rowptr, col, n, D, mean=False) * dinv.unsqueeze(1) + b)).abs().max().item())
        t = alternate({"fused_fwd": fused, "composed_fwd": composed, "torch_fwd": torch_eager, "sage_sibling_fwd": sibling,
                       "fused_bwd": fused_bwd}, a.rounds, a.k)
        byts = E * (4 * D + 8) + n * (8 * D + 4)
        res["widths"][f"D{D}"] = {**{k + "_ms": round(v, 4) for k, v in t.items()}, "epilogue": epi, "model_bytes": byts,
                                  "fwd_frac_of_8TBps": round(byts / (t["fused_fwd"] * 1e-3) / FABRIC_BPS, 4),
                                  "fused_over_composed": round(t["composed_fwd"] / t["fused_fwd"], 3),
                                  "fused_over_torch": round(t["torch_fwd"] / t["fused_fwd"], 3),
                                  "fused_over_sibling": round(t["sage_sibling_fwd"] / t["fused_fwd"], 3),
                                  "max_abs_diff_vs_composed": err}
    if not a.skip_office:
        res["office_epoch_ms"] = {"eager": round(office_epochs(False, a.office_epochs), 4),
                                  "graphed": round(office_epochs(True, a.office_epochs), 4)}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
