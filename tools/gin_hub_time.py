"""Times the GIN aggregation with and without segmented hub rows (ops.gin_aggregate_hubs / ops.gin_aggregate_bwd_hubs, hubs=None
against the hub tables of `--hub_cfg`) on a hub graph: the C4-shaped graph of tools/gin_time.py (synth.bridged_graph) plus ONE row
of N / 10 in-edges (node 3) and ONE source of N / 10 out-edges (node 5), the edges as generated.  D = 64 (ReLU epilogue) and D = 2
(log_softmax epilogue), eps = 0.3 on the device.  The candidates run in alternating blocks in this process (tools/gin_time.py's
`alternate`: the median of the samples and their spread, max - min, per candidate).  The unsegmented side is the call without
tables: the kernels of `ops.gin_aggregate`.  One JSON line with N, E, the largest in- and out-degree, the hub counts and the times."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.gin import graph_hubs  # noqa: E402
from bridged_gnn_amd.sage import SageGraph  # noqa: E402
from gin_time import alternate, note  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--hub_cfg", type=int, nargs=2, default=[ops.GIN_HUB_THRESHOLD, ops.GIN_HUB_SEGMENT])
    ap.add_argument("--k", type=int, default=5, help="calls per event pair")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gin_hub_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0), cluster=1024, seed=0)
    rng = np.random.default_rng(0)
    h = n // 10
    ei = np.concatenate([ei, np.stack([rng.choice(n, h, replace=False), np.full(h, 3)]),
                         np.stack([np.full(h, 5), rng.choice(n, h, replace=False)])], axis=1).astype(np.int64)
    g = SageGraph(torch.from_numpy(ei).to(dev), n)
    rowptr, col, t_rowptr, t_dst = g.by_dst
    E = int(g.csr.num_edges)
    hubs, t_hubs = graph_hubs(g, *a.hub_cfg)
    eps = torch.tensor([0.3], dtype=torch.float32, device=dev)
    deg = lambda rp: int((rp[1:].long() - rp[:-1].long()).max().item())
    res = {"tool": "gin_hub_time", "nodes": n, "edges": E, "max_in_degree": deg(rowptr), "max_out_degree": deg(t_rowptr),
           "hub_cfg": list(a.hub_cfg), "hub_rows": 0 if hubs is None else int(hubs[1].shape[0]),
           "hub_sources": 0 if t_hubs is None else int(t_hubs[1].shape[0]), "widths": {}}
    for D, epi in ((64, "relu"), (2, "log_softmax")):
        torch.manual_seed(D)
        Dp = ops.pad4(D)
        T, gy = torch.zeros(n, Dp, device=dev), torch.zeros(n, Dp, device=dev)
        T[:, :D] = torch.randn(n, D, device=dev)
        gy[:, :D] = torch.randn(n, D, device=dev)
        b = torch.zeros(Dp, device=dev)
        b[:D] = torch.randn(D, device=dev)
        y_buf, ys_buf, dT_buf, dTs_buf = (torch.empty(n, Dp, device=dev) for _ in range(4))
        fwd = lambda hb, out: ops.gin_aggregate_hubs(T, rowptr, col, eps, n, D, bias=b, epilogue=epi, out=out, hubs=hb)
        y = fwd(None, y_buf)
        bwd = lambda hb, out: ops.gin_aggregate_bwd_hubs(T, y, gy, t_rowptr, t_dst, eps, n, D, epilogue=epi, grad_tbl=out, hubs=hb)
        ys = fwd(hubs, ys_buf)
        d0, d1 = bwd(None, dT_buf)[0], bwd(t_hubs, dTs_buf)[0]
        err_f = float((y - ys).abs().max().item() / y.abs().max().item())
        err_b = float((d0 - d1).abs().max().item() / d0.abs().max().item())
        tm = alternate({"plain_fwd": lambda: fwd(None, y_buf), "segmented_fwd": lambda: fwd(hubs, ys_buf),
                        "plain_bwd": lambda: bwd(None, dT_buf), "segmented_bwd": lambda: bwd(t_hubs, dTs_buf)}, a.rounds, a.k)
        note(f"D={D}: {tm}")
        res["widths"][f"D{D}"] = {"epilogue": epi, **{k + "_ms": round(v[0], 4) for k, v in tm.items()},
                                  **{k + "_spread_ms": round(v[1], 4) for k, v in tm.items()},
                                  "fwd_plain_over_segmented": round(tm["plain_fwd"][0] / tm["segmented_fwd"][0], 3),
                                  "bwd_plain_over_segmented": round(tm["plain_bwd"][0] / tm["segmented_bwd"][0], 3),
                                  "max_rel_diff_fwd": err_f, "max_rel_diff_bwd_dT": err_b}
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
