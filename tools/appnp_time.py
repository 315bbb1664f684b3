"""Times the fused APPNP propagation (ops.appnp_propagate) on the C4-shaped graph of tools/gcn_time.py (synth.bridged_graph, 1M
nodes / 20M edges + one self loop per node) at C = 2 and C = 31, K = 10, alpha = 0.1, with the closing log_softmax, and an office
epoch of `train_appnp_noDTC` (eager: the driver refuses `graphed=True`).  One JSON line.  Per width, in this process, alternating blocks:
  fused_fwd    : K launches (3K with hub tables), teleport term, state scaling and log_softmax inside;
  composed_fwd : what the package offered before -- ten `ops.gcn_aggregate(bias=None)` calls, each followed by torch
                 `mul_` / `add_` for the teleport term, then `F.log_softmax`;
  fused_bwd    : the row pass (g = dy - exp(y) rowsum(dy)) and the same propagation over the by-source view;
  composed_bwd : torch autograd over that composition (each aggregation an autograd node whose backward is
                 `ops.gcn_aggregate_bwd`; out-of-place `mul` / `add`; `F.log_softmax`): 20 ops and ten saved intermediates;
                 the graph is built once and walked with retain_graph, so only the backward is timed.
Byte model of one fused step at Dp = pad4(C): E'(4 Dp + 4) + N(8 Dp + 8); of one composed step: E'(4 Dp + 8) + N(4 Dp + 8) for
the aggregation plus 20 Dp N for `mul_` (read + write) and `add_` (two reads + write).
Timing: a warm-up, a rehearsal burst, then one event pair round `--k` calls per sample; the median of the samples.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/appnp_time.py --skip-office` (profiles/appnp/README.md)."""
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
    """the candidates in alternating blocks -> median ms per call of each"""
    for f in fns.values():
        f()
        burst(f, k)                               # rehearsal burst
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            ts[name].append(burst(f, k))
    return {name: float(np.median(v)) for name, v in ts.items()}


class _Agg(torch.autograd.Function):
    """ops.gcn_aggregate(bias=None) as an autograd node: the composition's sparse step"""

    @staticmethod
    def forward(ctx, t, g, n, C):
        ctx.cfg = (g, n, C)
        return ops.gcn_aggregate(t, g.csr.rowptr, g.col, g.dinv, n, C, hubs=g.hubs)

    @staticmethod
    def backward(ctx, gy):
        g, n, C = ctx.cfg
        return ops.gcn_aggregate_bwd(None, gy.contiguous(), g.t_rowptr, g.t_dst, g.dinv, n, C, want_bias=False, hubs=g.t_hubs)[0], None, None, None


def note(*a):
    """progress on stderr (stdout carries the one JSON line)"""
    print("[appnp_time]", *a, file=sys.stderr, flush=True)


def office_epochs(epochs):
    from bridged_gnn_amd import appnp, transfer
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
        appnp.train_appnp_noDTC(args, transfer.pyg_dataset(d), d, repeat=1, num_epoch=n, seed=0, hidden=64, use_scheduler=False,
                                verbose=False)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
        note(f"office epochs={n}: {out[-1]:.3f} s")
    return (out[2] - out[1]) / epochs * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--k", type=int, default=3, help="calls per event pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--office-epochs", type=int, default=100)
    ap.add_argument("--skip-office", action="store_true")
    ap.add_argument("--office-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "appnp_time needs an MI355X"
    dev = torch.device("cuda:0")
    res = {"tool": "appnp_time", "K": a.K, "alpha": a.alpha}
    if not a.office_only:
        n, K, alpha = a.nodes, a.K, a.alpha
        n_tar = n - n // 2
        ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                    cluster=1024, seed=0)
        g = GcnGraph(torch.from_numpy(ei).to(dev), n)
        E = int(g.csr.num_edges)
        res.update(nodes=n, edges_with_self_loops=E, hub_rows=0 if g.hubs is None else int(g.hubs[1].shape[0]),
                   hub_sources=0 if g.t_hubs is None else int(g.t_hubs[1].shape[0]), widths={})
        views = {"dst": (g.csr.rowptr, g.col, g.hubs), "src": (g.t_rowptr, g.t_dst, g.t_hubs)}

        for C in (2, 31):
            Dp = ops.pad4(C)
            h = torch.randn(n, Dp, device=dev)
            dy = torch.randn(n, Dp, device=dev)
            dy[:, C:] = 0

            def composed(t, view):
                rowptr, col, hubs = views[view]
                z = t
                for _ in range(K):
                    z = ops.gcn_aggregate(z, rowptr, col, g.dinv, n, C, hubs=hubs).mul_(1.0 - alpha).add_(t, alpha=alpha)
                return z

            def fused_fwd():
                return ops.appnp_propagate(h, *views["dst"][:2], g.dinv, n, C, K, alpha, epilogue="log_softmax", hubs=g.hubs)

            def composed_fwd():
                return F.log_softmax(composed(h, "dst")[:, :C], dim=1)

            y = fused_fwd()

            def fused_bwd():
                gz = ops.appnp_log_softmax_bwd(y, dy, C)
                return ops.appnp_propagate(gz, *views["src"][:2], g.dinv, n, C, K, alpha, hubs=g.t_hubs)

            hr = h.clone().requires_grad_(True)
            z = hr
            for _ in range(K):
                z = _Agg.apply(z, g, n, C) * (1.0 - alpha) + alpha * hr
            yc = F.log_softmax(z[:, :C], dim=1)

            def composed_bwd():
                return torch.autograd.grad(yc, hr, dy[:, :C], retain_graph=True)[0]

            err_f = float((fused_fwd()[:, :C] - composed_fwd()).abs().max().item())
            err_b = float((fused_bwd()[:, :C] - composed_bwd()[:, :C]).abs().max().item())
            t = alternate({"fused_fwd": fused_fwd, "composed_fwd": composed_fwd, "fused_bwd": fused_bwd, "composed_bwd": composed_bwd},
                          a.rounds, a.k)
            fused_bytes = E * (4 * Dp + 4) + n * (8 * Dp + 8)
            comp_bytes = E * (4 * Dp + 8) + n * (4 * Dp + 8) + 20 * Dp * n
            note(f"C={C}: {t}")
            res["widths"][f"C{C}"] = {**{k + "_ms": round(v, 4) for k, v in t.items()},
                                      "fused_step_model_bytes": fused_bytes, "composed_step_model_bytes": comp_bytes,
                                      "fwd_composed_over_fused": round(t["composed_fwd"] / t["fused_fwd"], 3),
                                      "bwd_composed_over_fused": round(t["composed_bwd"] / t["fused_bwd"], 3),
                                      "max_abs_diff_fwd": err_f, "max_abs_diff_bwd": err_b}
    if not a.skip_office:
        res["office_epoch_ms"] = {"eager": round(office_epochs(a.office_epochs), 4)}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
