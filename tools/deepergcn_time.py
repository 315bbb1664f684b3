"""Times one DeeperGCN softmax aggregation (ops.gen_softmax_aggregate / ops.gen_softmax_aggregate_bwd) on the C4-shaped graph of
tools/gcn_time.py (synth.bridged_graph, 1M nodes / 20M edges, the edges as generated) at H = 64 and H = 128, t = 1.  One JSON line.
Per width, in this process, alternating blocks:
  fused_eval     : one walk, no tables written;
  fused_train    : the same walk with the (lse, o) tables written;
  composed_fwd   : the same formula in torch eager, as PyG composes it -- relu + eps, a gather of the source rows, a `scatter_reduce_`
                   amax for the per-destination maximum, exp, two `index_add_` and a division, then + x;
  fused_bwd      : one walk over the by-source view plus the one-block sum of the grad_t partials;
  composed_bwd   : torch autograd over the composition (the graph is built once and walked with retain_graph, so only the backward
                   is timed).
Byte model (Hp = pad4(H)): evaluation forward E(4 Hp + 4) + N(8 Hp + 4) -- a gathered row and a column id per edge; x_i, z_i and
rowptr per node -- training forward + 8 N Hp (the tables), backward E(12 Hp + 4) + N(12 Hp + 4) (g, lse, o per edge; x_j, g_j,
grad_x_j per node); `*_model_GBps` is that count over the measured time.
Timing: a warm-up, a rehearsal burst, then one event pair round `--k` calls per sample; the median of the samples.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/deepergcn_time.py` (profiles/deepergcn/README.md)."""
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
    """the candidates in alternating blocks -> median ms per call of each"""
    for f in fns.values():
        f()
        burst(f, k)                               # rehearsal burst
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            ts[name].append(burst(f, k))
    return {name: float(np.median(v)) for name, v in ts.items()}


def composed(x, t, src, dst):
    """PyG's softmax aggregation in torch eager: the maximum is taken without a gradient, as PyG's `softmax` does"""
    v = torch.relu(x) + 1e-7
    vs = v[src]
    a = t * vs
    with torch.no_grad():
        m = torch.full_like(x, float("-inf")).scatter_reduce_(0, dst.unsqueeze(1).expand_as(a), a, "amax", include_self=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(a - m[dst])
    s = torch.zeros_like(x).index_add_(0, dst, e)
    w = torch.zeros_like(x).index_add_(0, dst, e * vs)
    return w / s.clamp_min(1e-30) + x


def note(*a):
    """progress on stderr (stdout carries the one JSON line)"""
    print("[deepergcn_time]", *a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--t", type=float, default=1.0)
    ap.add_argument("--k", type=int, default=3, help="calls per event pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "deepergcn_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0), cluster=1024, seed=0)
    eid = torch.from_numpy(ei).to(dev)
    g = SageGraph(eid, n)
    rowptr, col, t_rowptr, t_dst = g.by_dst
    E = int(g.csr.num_edges)
    src, dst = eid[0].contiguous(), eid[1].contiguous()
    t = torch.tensor([a.t], dtype=torch.float32, device=dev)
    res = {"tool": "deepergcn_time", "t": a.t, "nodes": n, "edges": E, "widths": {}}

    for H in (64, 128):
        torch.manual_seed(H)
        x, gz = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev)
        tabs = (torch.empty(n, H, device=dev), torch.empty(n, H, device=dev))
        z_buf, gx_buf = torch.empty(n, H, device=dev), torch.empty(n, H, device=dev)

        def fused_eval():
            return ops.gen_softmax_aggregate(x, rowptr, col, t, n, H, out=z_buf)

        def fused_train():
            return ops.gen_softmax_aggregate(x, rowptr, col, t, n, H, save=tabs, out=z_buf)

        def composed_fwd():
            with torch.no_grad():
                return composed(x, t, src, dst)

        def fused_bwd():
            return ops.gen_softmax_aggregate_bwd(x, gz, tabs, t_rowptr, t_dst, t, H, grad_x=gx_buf)

        xr, tr = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
        zc = composed(xr, tr, src, dst)

        def composed_bwd():
            return torch.autograd.grad(zc, [xr, tr], gz, retain_graph=True)

        zf = fused_train().clone()
        scale = float(zc.detach().abs().max().item())
        err_f = float((zf - zc.detach()).abs().max().item())
        fb, cb = fused_bwd(), composed_bwd()
        err_b = [float((u.reshape(v.shape) - v).abs().max().item() / v.abs().max().item()) for u, v in zip(fb, cb)]
        tm = alternate({"fused_eval": fused_eval, "fused_train": fused_train, "composed_fwd": composed_fwd, "fused_bwd": fused_bwd,
                        "composed_bwd": composed_bwd}, a.rounds, a.k)
        Hp = ops.pad4(H)
        model = {"fused_eval": E * (4 * Hp + 4) + n * (8 * Hp + 4), "fused_train": E * (4 * Hp + 4) + n * (16 * Hp + 4),
                 "fused_bwd": E * (12 * Hp + 4) + n * (12 * Hp + 4)}
        note(f"H={H}: {tm}")
        res["widths"][f"H{H}"] = {**{k + "_ms": round(v, 4) for k, v in tm.items()},
                                  **{k + "_model_bytes": v for k, v in model.items()},
                                  **{k + "_model_GBps": round(v / (tm[k] * 1e-3) / 1e9, 1) for k, v in model.items()},
                                  "eval_composed_over_fused": round(tm["composed_fwd"] / tm["fused_eval"], 3),
                                  "train_composed_over_fused": round(tm["composed_fwd"] / tm["fused_train"], 3),
                                  "bwd_composed_over_fused": round(tm["composed_bwd"] / tm["fused_bwd"], 3),
                                  "max_abs_diff_fwd": err_f, "max_abs_fwd": scale, "max_rel_diff_bwd_gx_gt": err_b}
        del xr, tr, zc, cb
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
