"""Times one GCNII layer (ops.gcn2_conv / ops.gcn2_conv_bwd) on the C4-shaped graph of tools/gcn_time.py (synth.bridged_graph, 1M
nodes / 20M edges + one self loop per node) at H = 64 and H = 128, alpha = 0.1, beta = log(1.5).  One JSON line.  Per width, in
this process, alternating blocks:
  fused_eval     : one pass (three launches with hub tables), m never written, p = 0;
  composed_eval  : what the package offered before -- `ops.gcn_aggregate`, torch `mul_` / `add_` for the mix, `torch.addmm` for
                   (1 - beta) m + beta m W, `relu_`;
  fused_train    : the same pass with m written and dropout at p = 0.5;
  composed_train : the composition with `ops.feature_dropout(relu=True)` as its last pass;
  fused_bwd      : `ops.gcn2_conv_bwd`, `ops.gram` (grad_weight1) and `ops.gcn_aggregate` over the by-source view (grad_x);
  composed_bwd   : torch autograd over the composition (the aggregation an autograd node whose backward is
                   `ops.gcn_aggregate_bwd`, out-of-place mix, `addmm`, the feature-dropout node); the graph is built once and
                   walked with retain_graph, so only the backward is timed.
Byte model of the fused evaluation forward: E'(4H + 8) + N(8H + 4) + 4H^2 (a gathered row, a column id and dinv[col] per edge; x0,
y, rowptr per node; M once); `fused_eval_model_GBps` is that count over the measured time.
Timing: a warm-up, a rehearsal burst, then one event pair round `--k` calls per sample; the median of the samples.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gcn2_time.py` (profiles/gcn2/README.md)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.appnp import _FeatureDropFn  # noqa: E402
from bridged_gnn_amd.gcn import GcnGraph  # noqa: E402

SEED = 1234


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
    def forward(ctx, t, g, n, H):
        ctx.cfg = (g, n, H)
        return ops.gcn_aggregate(t, g.csr.rowptr, g.col, g.dinv, n, H, hubs=g.hubs)

    @staticmethod
    def backward(ctx, gy):
        g, n, H = ctx.cfg
        return ops.gcn_aggregate_bwd(None, gy.contiguous(), g.t_rowptr, g.t_dst, g.dinv, n, H, want_bias=False, hubs=g.t_hubs)[0], None, None, None


def note(*a):
    """progress on stderr (stdout carries the one JSON line)"""
    print("[gcn2_time]", *a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--p", type=float, default=0.5, help="dropout of the training forward")
    ap.add_argument("--k", type=int, default=3, help="calls per event pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gcn2_time needs an MI355X"
    dev = torch.device("cuda:0")
    n, alpha, p, beta = a.nodes, a.alpha, a.p, math.log(1.5)
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0), cluster=1024, seed=0)
    g = GcnGraph(torch.from_numpy(ei).to(dev), n)
    E = int(g.csr.num_edges)
    res = {"tool": "gcn2_time", "alpha": alpha, "beta": round(beta, 6), "p_train": p, "nodes": n, "edges_with_self_loops": E,
           "hub_rows": 0 if g.hubs is None else int(g.hubs[1].shape[0]),
           "hub_sources": 0 if g.t_hubs is None else int(g.t_hubs[1].shape[0]), "widths": {}}
    graph = (g.csr.rowptr, g.col, g.dinv, n)

    for H in (64, 128):
        torch.manual_seed(H)
        x, x0, dy = (torch.randn(n, H, device=dev) for _ in range(3))
        W = torch.randn(H, H, device=dev) / math.sqrt(H)
        M = ((1.0 - beta) * torch.eye(H, device=dev) + beta * W).contiguous()
        m_buf = torch.empty(n, H, device=dev)

        def composed_z():
            m = ops.gcn_aggregate(x, *graph, H, hubs=g.hubs).mul_(1.0 - alpha).add_(x0, alpha=alpha)
            return torch.addmm(m, m, W, beta=1.0 - beta, alpha=beta)

        def fused_eval():
            return ops.gcn2_conv(x, x0, M, *graph, H, alpha, hubs=g.hubs)

        def composed_eval():
            return composed_z().relu_()

        def fused_train():
            return ops.gcn2_conv(x, x0, M, *graph, H, alpha, p_drop=p, seed=SEED, hubs=g.hubs, m_out=m_buf)

        def composed_train():
            z = composed_z()
            return ops.feature_dropout(z, p, SEED, relu=True, out=z)

        y = fused_train().clone()

        def fused_bwd(y=y, m=m_buf):
            gz, t, gx0 = ops.gcn2_conv_bwd(y, dy, M, H, alpha, p)
            gw = ops.gram(m, gz).mul_(beta)
            return ops.gcn_aggregate(t, g.t_rowptr, g.t_dst, g.dinv, n, H, hubs=g.t_hubs), gx0, gw

        xr, x0r, Wr = (v.clone().requires_grad_(True) for v in (x, x0, W))
        mr = _Agg.apply(xr, g, n, H) * (1.0 - alpha) + alpha * x0r
        yc = _FeatureDropFn.apply(torch.addmm(mr, mr, Wr, beta=1.0 - beta, alpha=beta), p, SEED, None, True, None)

        def composed_bwd():
            return torch.autograd.grad(yc, [xr, x0r, Wr], dy, retain_graph=True)

        scale = float(composed_eval().abs().max().item())
        err_e = float((fused_eval() - composed_eval()).abs().max().item())
        err_t = float((fused_train() - composed_train()).abs().max().item())
        # the backward's contract: the ReLU and dropout state is read off the y it is handed -- the composition's here, whose few
        # pre-activations next to 0 may have the other sign than the fused forward's
        fb, cb = fused_bwd(yc.detach(), mr.detach().contiguous()), composed_bwd()
        err_b = [float((u - v).abs().max().item() / v.abs().max().item()) for u, v in zip(fb, cb)]
        t = alternate({"fused_eval": fused_eval, "composed_eval": composed_eval, "fused_train": fused_train,
                       "composed_train": composed_train, "fused_bwd": fused_bwd, "composed_bwd": composed_bwd}, a.rounds, a.k)
        model = E * (4 * H + 8) + n * (8 * H + 4) + 4 * H * H
        note(f"H={H}: {t}")
        res["widths"][f"H{H}"] = {**{k + "_ms": round(v, 4) for k, v in t.items()},
                                  "fused_eval_model_bytes": model,
                                  "fused_eval_model_GBps": round(model / (t["fused_eval"] * 1e-3) / 1e9, 1),
                                  "eval_composed_over_fused": round(t["composed_eval"] / t["fused_eval"], 3),
                                  "train_composed_over_fused": round(t["composed_train"] / t["fused_train"], 3),
                                  "bwd_composed_over_fused": round(t["composed_bwd"] / t["fused_bwd"], 3),
                                  "max_abs_diff_eval": err_e, "max_abs_diff_train": err_t, "max_abs_eval": scale,
                                  "max_rel_diff_bwd_gx_gx0_gw": err_b}
        del xr, x0r, Wr, mr, yc
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
