"""Times GraphSAGE (bridged_gnn_amd.sage) on a C4-shaped graph (synth.bridged_graph, 1M nodes / 20M edges; Din 128, hidden 64,
C = 2) and prints one JSON line:
  eval forward ms, training step ms (forward + backward + Adam, dropout 0.5), the mean aggregations alone (event-timed) with the
  SURVEY 8(d) byte model at width D, E'(4D + 4) + N(8D + 4), as a fraction of 8 TB/s (a fabric-side figure: the gathers are
  mostly L2 hits, so this is not an HBM share), and two comparisons timed in this process, alternating:
    agg_vs_zero_attention: the forward aggregation at width 64 against the zero-attention `ops.adaptedconv_aggregate` route
                           (uniform attention == mean) that bridge.py's SAGE encoder takes -- the kernels alone
                           ("kernel_only": the SAGE kernel also adds the root half) and for the same output
                           ("same_output": the zero-attention mean plus a torch add of the root half);
    step_vs_torch:         the training step against a torch-only formulation (index_add_ mean, autograd, same Adam).
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/sage_time.py` (see profiles/sage/README.md)."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.sage import GraphSAGE  # noqa: E402

FABRIC_BPS = 8e12


def timed(fn, reps):
    """median over `reps` single calls of device-event time (ms)"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def alternate(fa, fb, rounds, reps):
    """A and B in alternating blocks; -> (median A, median B) over the blocks' medians"""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    return float(np.median(ta)), float(np.median(tb))


class TorchSAGE(torch.nn.Module):
    """torch-only GraphSAGE of the same shape: mean by index_add_, autograd, F.dropout."""

    def __init__(self, m):
        super().__init__()
        self.lins = torch.nn.ModuleList()
        for conv in m.convs:
            lin_l = torch.nn.Linear(conv.in_channels, conv.out_channels)
            lin_r = torch.nn.Linear(conv.in_channels, conv.out_channels, bias=False)
            with torch.no_grad():
                lin_l.weight.copy_(conv.lin_l.weight); lin_l.bias.copy_(conv.lin_l.bias); lin_r.weight.copy_(conv.lin_r.weight)
            self.lins.append(torch.nn.ModuleList([lin_l, lin_r]))

    def forward(self, x, src, dst, inv_deg):
        for i, (lin_l, lin_r) in enumerate(self.lins):
            agg = torch.zeros_like(x).index_add_(0, dst, x[src]) * inv_deg
            x = lin_l(agg) + lin_r(x)
            if i < len(self.lins) - 1:
                x = F.dropout(F.relu(x), p=0.5, training=self.training)
        return F.log_softmax(x, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sage_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)
    x = torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=1)).to(dev)
    y = torch.randint(0, 2, (n,), device=dev)
    data = types.SimpleNamespace(x=x, edge_index=torch.from_numpy(ei).to(dev))
    E = int(ei.shape[1])
    torch.manual_seed(0)
    m = GraphSAGE(types.SimpleNamespace(num_features=128, num_classes=2), layer_num=2, hidden=64).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)

    def fwd_eval():
        with torch.no_grad():
            m(data)

    def step():
        opt.zero_grad(set_to_none=True)
        F.nll_loss(m(data), y).backward()
        opt.step()

    m.eval()
    fwd_eval()
    torch.cuda.synchronize()
    fwd_ms = timed(fwd_eval, a.reps * 2)
    m.train()
    for _ in range(3):
        step()
    step_ms = timed(step, a.reps)

    # the aggregations alone
    g = m.graph(data.edge_index, n)
    rowptr, col, t_rowptr, t_col = g.view(False)
    aggs = {}
    for D in (64, 2):
        Dp = ops.pad4(D)
        T = torch.randn(n, 2 * Dp, device=dev)
        dy = torch.randn(n, Dp, device=dev)
        yv = ops.sage_mean_aggregate(T[:, :Dp], rowptr, col, n, D, root=T[:, Dp:], epilogue="relu")
        f = lambda: ops.sage_mean_aggregate(T[:, :Dp], rowptr, col, n, D, root=T[:, Dp:], epilogue="relu")
        b = lambda: ops.sage_mean_aggregate_bwd(yv, dy, rowptr, t_rowptr, t_col, n, D, epilogue="relu")
        f(); b()
        tf, tb = timed(f, a.reps * 2), timed(b, a.reps * 2)
        byts = E * (4 * D + 4) + n * (8 * D + 4)
        aggs[f"D{D}"] = {"fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4), "model_bytes": byts,
                         "fwd_frac_of_8TBps": round(byts / (tf * 1e-3) / FABRIC_BPS, 4),
                         "bwd_frac_of_8TBps": round(2 * byts / (tb * 1e-3) / FABRIC_BPS, 4)}

    # comparison 1: forward aggregation at width 64 vs the zero-attention route (same graph, no self-loop rewrite)
    D = 64
    tab = torch.randn(n, 2 * D, device=dev)
    zero_a = torch.zeros(D, device=dev)
    ones = torch.ones(n, dtype=torch.uint8, device=dev)
    new = lambda: ops.sage_mean_aggregate(tab[:, :D], rowptr, col, n, D, root=tab[:, D:])
    old = lambda: ops.adaptedconv_aggregate(tab[:, :D], tab[:, :D], zero_a, zero_a, g.csr, ones, D)
    old_route = lambda: old()[:, :D] + tab[:, D:]          # the same result: the zero-attention mean plus the root half
    agg_err = float((new()[:, :D] - old_route()).abs().max().item())
    t_new, t_old = alternate(new, old, a.rounds, a.reps)
    t_new2, t_route = alternate(new, old_route, a.rounds, a.reps)

    # comparison 2: training step vs the torch-only formulation
    tm = TorchSAGE(m).to(dev).train()
    topt = torch.optim.Adam(tm.parameters(), lr=1e-3, weight_decay=5e-3)
    src, dst = data.edge_index[0], data.edge_index[1]
    inv_deg = (1.0 / torch.bincount(dst, minlength=n).clamp(min=1).float()).unsqueeze(1)

    def tstep():
        topt.zero_grad(set_to_none=True)
        F.nll_loss(tm(x, src, dst, inv_deg), y).backward()
        topt.step()

    tstep()
    s_new, s_torch = alternate(step, tstep, a.rounds, max(a.reps // 2, 2))
    torch.cuda.synchronize()
    res = {"tool": "sage_time", "nodes": n, "edges": E, "din": 128, "hidden": 64, "classes": 2,
           "eval_forward_ms": round(fwd_ms, 4), "train_step_ms": round(step_ms, 4), "aggregations": aggs,
           "agg_vs_zero_attention": {"kernel_only": {"sage_ms": round(t_new, 4), "zero_attention_ms": round(t_old, 4),
                                                     "speedup": round(t_old / t_new, 3)},
                                     "same_output": {"sage_ms": round(t_new2, 4), "zero_attention_plus_root_ms": round(t_route, 4),
                                                     "speedup": round(t_route / t_new2, 3)},
                                     "max_abs_diff": agg_err},
           "step_vs_torch": {"sage_ms": round(s_new, 4), "torch_ms": round(s_torch, 4), "speedup": round(s_torch / s_new, 3)},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
