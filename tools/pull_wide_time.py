"""Timing of the aggregation backward at 128 < D <= 256 on the C4-shaped graph (bench.py's generator: 1M nodes / ~21M edges):
the atomic-free pair (bgnn_adaptedconv_aggregate_bwd_pull_f32 at these widths: pass A + merge + da sum + pass B + merge) against the
atomic scatter form (zero-fill of both dH tables + bgnn_adaptedconv_aggregate_bwd_f32, what `ops.adaptedconv_aggregate_bwd` did at
these widths before), one device-event interval per call, the two forms alternating in one process.  Prints ONE JSON line:
  widths[D] -- median / min / p10 / p90 ms of both forms, `spread_ms` = the larger p10..p90 range of the two, `gain_ms` = scatter
               median - pull median, `keep_route` = gain_ms > spread_ms, `ratio` = scatter median / pull median, and the worst
               difference of the two forms' outputs (of each tensor's max);
  step      -- the single-GPU training step (forward + reference loss + backward) at --hidden, the op's route against the same
               step with the scatter form put back for D > 128, alternating.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/pull_wide_time.py --skip step --reps 3`."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import _lib as L  # noqa: E402
from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.data import Data  # noqa: E402
from bridged_gnn_amd.ktgnn import KTGNN_no_complement  # noqa: E402

_pull_route = ops.adaptedconv_aggregate_bwd


def scatter_bwd(h_t2s, h_s2t, a_t2s, a_s2t, csr, mask_u8, D, out, alpha, grad_out, negative_slope=0.1):
    """the atomic form as the op ran it for D > 128 (narrower widths keep the op's own route)"""
    if D <= 128:
        return _pull_route(h_t2s, h_s2t, a_t2s, a_s2t, csr, mask_u8, D, out, alpha, grad_out, negative_slope)
    lib = L.lib()
    dev = h_t2s.device
    da_t2s = torch.zeros(D, dtype=torch.float32, device=dev)
    da_s2t = torch.zeros(D, dtype=torch.float32, device=dev)
    grad_out = grad_out.contiguous()
    dh_t2s, dh_s2t = torch.zeros_like(h_t2s), torch.zeros_like(h_s2t)
    rc = lib.bgnn_adaptedconv_aggregate_bwd_f32(
        L.ptr(h_t2s), L.ptr(h_s2t), h_t2s.stride(0), L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col),
        L.ptr(mask_u8), 0, csr.num_nodes, D, float(negative_slope), L.ptr(out), out.stride(0), L.ptr(alpha),
        L.ptr(grad_out), grad_out.stride(0), L.ptr(dh_t2s), L.ptr(dh_s2t), L.ptr(da_t2s), L.ptr(da_s2t), L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_bwd_f32")
    return dh_t2s, dh_s2t, da_t2s, da_s2t


def ev_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warmup=3):
    """{name: [ms, ...]}, the variants run alternately"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(ev_time(f))
    return ts


def stats(v):
    v = np.asarray(v)
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4),
                p10_ms=round(float(np.percentile(v, 10)), 4), p90_ms=round(float(np.percentile(v, 90)), 4))


def compare(ts, a, b):
    """a = the new form, b = the old one"""
    sa, sb = stats(ts[a]), stats(ts[b])
    spread = max(sa["p90_ms"] - sa["p10_ms"], sb["p90_ms"] - sb["p10_ms"])
    gain = sb["median_ms"] - sa["median_ms"]
    return {a: sa, b: sb, "spread_ms": round(spread, 4), "gain_ms": round(gain, 4), "keep_route": bool(gain > spread),
            "ratio": round(sb["median_ms"] / sa["median_ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--widths", default="192,256")
    ap.add_argument("--hidden", type=int, default=256, help="hidden size of the training step")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma list of parts to skip: widths,step")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) - {""}
    assert torch.cuda.is_available(), "pull_wide_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, mask = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                   cluster=1024, p_local=0.9, seed=0)            # bench.py's C4 (graph "local")
    g = torch.Generator(device=dev).manual_seed(1)
    cm = torch.from_numpy(mask).to(dev)
    m_u8 = cm.to(torch.uint8).contiguous()
    edge_index = torch.from_numpy(ei).to(dev)
    csr = ops.build_dst_csr(edge_index, n)
    rec = dict(nodes=n, edges=int(csr.num_edges), reps=a.reps,
               hub_rows=[0 if t is None else int(t[0].numel()) for t in (csr.hub_tables(), csr.transposed_hub_tables())])

    if "widths" not in skip:
        rec["widths"] = {}
        for D in [int(w) for w in a.widths.split(",")]:
            ld = ops.pad4(D)
            hS, hT = torch.zeros(n, ld, device=dev), torch.zeros(n, ld, device=dev)
            hS[:, :D] = torch.randn(n, D, device=dev, generator=g)
            hT[:, :D] = torch.randn(n, D, device=dev, generator=g)
            a1, a2 = torch.randn(D, device=dev, generator=g) * 0.3, torch.randn(D, device=dev, generator=g) * 0.3
            out, alpha = ops.adaptedconv_aggregate(hS, hT, a1, a2, csr, m_u8, D, 0.1, want_alpha=True)
            go = torch.zeros(n, ld, device=dev)
            go[:, :D] = torch.randn(n, D, device=dev, generator=g)
            args = (hS, hT, a1, a2, csr, m_u8, D, out, alpha, go, 0.1)
            p, s = _pull_route(*args), scatter_bwd(*args)
            diff = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(p, s))
            same = all(torch.equal(x, y) for x, y in zip(p, _pull_route(*args)))
            del p, s
            ts = alternate({"pull_ms": lambda: _pull_route(*args), "scatter_ms": lambda: scatter_bwd(*args)}, a.reps)
            rec["widths"][str(D)] = dict(compare(ts, "pull_ms", "scatter_ms"), max_rel_diff=diff, pull_bitwise_repeatable=same)
            del hS, hT, out, alpha, go, args
            torch.cuda.empty_cache()

    if "step" not in skip:
        torch.manual_seed(0)
        model = KTGNN_no_complement(128, 2, 2, a.hidden, use_bn=True, dim_share=128, dropout=0.0).to(dev).train()
        x = torch.randn(n, 128, device=dev, generator=g)
        y = torch.randint(0, 2, (n,), device=dev, generator=g)
        tm = torch.rand(n, device=dev, generator=g) < 0.5
        data = Data(x=x, edge_index=edge_index, central_mask=cm)
        tmt = tm & ~cm
        yi = y[:, None]

        def loss(o):
            lb, lt, lth = o[:3]
            nll = lambda logp, w: -(logp.gather(1, yi).squeeze(1) * w).sum()
            return (2 * nll(lb, tm.float() / tm.sum()) + nll(lt, tmt.float() / tmt.sum()) + nll(lth, tmt.float() / tmt.sum())) / 4 \
                + F.kl_div(lth, lt, log_target=True, reduction="batchmean")

        def step(fn):
            def f():
                ops.adaptedconv_aggregate_bwd = fn            # ktgnn's backward looks the op up at call time
                model.zero_grad(set_to_none=True)
                loss(model(data)).backward()
            return f
        ts = alternate({"pull_step_ms": step(_pull_route), "scatter_step_ms": step(scatter_bwd)}, max(a.reps // 2, 3))
        ops.adaptedconv_aggregate_bwd = _pull_route
        rec["step"] = dict(compare(ts, "pull_step_ms", "scatter_step_ms"), hidden=a.hidden)

    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
