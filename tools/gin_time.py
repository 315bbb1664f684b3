"""Times one GIN aggregation (ops.gin_aggregate / ops.gin_aggregate_bwd) against its composition from the GraphSAGE entry on the
C4-shaped graph of tools/gcn_time.py (synth.bridged_graph, 1M nodes / 20M edges, the edges as generated) at D = 64 (a hidden layer:
ReLU epilogue) and D = 2 (a two-class head: log_softmax epilogue), eps = 0.3 on the device.  One JSON line.
Per width, in this process, alternating blocks:
  fused_fwd     : ops.gin_aggregate -- the row's own table row is its root, eps is read by the kernel;
  composed_fwd  : root = (1 + eps) * T + b in torch (one pass that reads T and writes a second [N, D] buffer), then
                  ops.sage_mean_aggregate(mean=False, root=root) with the same epilogue;
  fused_bwd     : ops.gin_aggregate_bwd -- g, <g, T> in fp64 partials and their fixed-order sum, the walk over the by-source view,
                  and the column sums of g for grad_bias;
  composed_bwd  : g from the epilogue's own backward op (ops.feature_dropout_bwd(relu=True) / ops.appnp_log_softmax_bwd), the plain
                  sum ops.sage_mean_aggregate(g, by-source view, mean=False, root=(1 + eps) * g) with the root formed in torch,
                  grad_eps = (g * T).sum() in torch and the same column sums.
Byte model of one walk (Dp = pad4(D)): E(4 Dp + 4) + N(12 Dp + 4) -- a gathered row and a column id per edge; the own row, the
output row and rowptr per node; the backward adds its row pass N * 12 Dp (y, dy, g) and N * 8 Dp for grad_eps.  `*_model_GBps` is
that count over the measured time.
Timing: a warm-up, a rehearsal burst, then one event pair round `--k` calls per sample; the median of the samples and their
spread (max - min) per candidate.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gin_time.py`
(profiles/gin/README.md)."""
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
from bridged_gnn_amd.sage import SageGraph  # noqa: E402


def burst(fn, k):
    """ms per call over one event pair round k calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def alternate(fns, rounds, k):
    """the candidates in alternating blocks -> (median, max - min) ms per call of each"""
    for f in fns.values():
        f()
        burst(f, k)                               # rehearsal burst
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            ts[name].append(burst(f, k))
    return {name: (float(np.median(v)), float(np.max(v) - np.min(v))) for name, v in ts.items()}


def note(*a):
    """progress on stderr (stdout carries the one JSON line)"""
    print("[gin_time]", *a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--eps", type=float, default=0.3)
    ap.add_argument("--k", type=int, default=5, help="calls per event pair")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gin_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0), cluster=1024, seed=0)
    g = SageGraph(torch.from_numpy(ei).to(dev), n)
    rowptr, col, t_rowptr, t_dst = g.by_dst
    E = int(g.csr.num_edges)
    eps = torch.tensor([a.eps], dtype=torch.float32, device=dev)
    res = {"tool": "gin_time", "eps": a.eps, "nodes": n, "edges": E, "widths": {}}

    for D, epi in ((64, "relu"), (2, "log_softmax")):
        torch.manual_seed(D)
        Dp = ops.pad4(D)
        T, gy = torch.zeros(n, Dp, device=dev), torch.zeros(n, Dp, device=dev)
        T[:, :D] = torch.randn(n, D, device=dev)
        gy[:, :D] = torch.randn(n, D, device=dev)
        b = torch.zeros(Dp, device=dev)
        b[:D] = torch.randn(D, device=dev)
        y_buf, yc_buf, dT_buf, dTc_buf = (torch.empty(n, Dp, device=dev) for _ in range(4))

        def fused_fwd():
            return ops.gin_aggregate(T, rowptr, col, eps, n, D, bias=b, epilogue=epi, out=y_buf)

        def composed_fwd():
            root = (1.0 + eps) * T + b
            return ops.sage_mean_aggregate(T, rowptr, col, n, D, root=root, mean=False, epilogue=epi, out=yc_buf)

        y = fused_fwd()
        yc = composed_fwd()

        def fused_bwd():
            return ops.gin_aggregate_bwd(T, y, gy, t_rowptr, t_dst, eps, n, D, epilogue=epi, grad_tbl=dT_buf)

        def composed_bwd():
            gg = ops.feature_dropout_bwd(gy, 0.0, 0, y=y, relu=True) if epi == "relu" else ops.appnp_log_softmax_bwd(y, gy, D)
            dT = ops.sage_mean_aggregate(gg, t_rowptr, t_dst, n, D, root=(1.0 + eps) * gg, mean=False, out=dTc_buf)
            return dT, ops.column_sums(gg)[:D], (gg * T).sum().reshape(1)

        scale = float(y[:, :D].abs().max().item())
        err_f = float((y - yc).abs().max().item())
        fb, cb = fused_bwd(), composed_bwd()
        err_b = [float((u - v).abs().max().item() / max(v.abs().max().item(), 1e-30)) for u, v in zip(fb, cb)]
        tm = alternate({"fused_fwd": fused_fwd, "composed_fwd": composed_fwd, "fused_bwd": fused_bwd, "composed_bwd": composed_bwd},
                       a.rounds, a.k)
        walk = E * (4 * Dp + 4) + n * (12 * Dp + 4)
        model = {"fused_fwd": walk, "fused_bwd": walk + n * 20 * Dp}
        note(f"D={D}: {tm}")
        res["widths"][f"D{D}"] = {"epilogue": epi,
                                  **{k + "_ms": round(v[0], 4) for k, v in tm.items()},
                                  **{k + "_spread_ms": round(v[1], 4) for k, v in tm.items()},
                                  **{k + "_model_bytes": v for k, v in model.items()},
                                  **{k + "_model_GBps": round(v / (tm[k][0] * 1e-3) / 1e9, 1) for k, v in model.items()},
                                  "fwd_composed_over_fused": round(tm["composed_fwd"][0] / tm["fused_fwd"][0], 3),
                                  "bwd_composed_over_fused": round(tm["composed_bwd"][0] / tm["fused_bwd"][0], 3),
                                  "max_abs_diff_fwd": err_f, "max_abs_fwd": scale, "max_rel_diff_bwd_dT_db_deps": err_b}
        del fb, cb
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
