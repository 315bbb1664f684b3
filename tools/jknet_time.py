"""Times JKNet's two fused passes against their compositions on the C4-shaped graph of tools/gcn_time.py and tools/gin_time.py
(synth.bridged_graph, 1M nodes / about 20M edges).  One JSON line.  Per shape, in this process, alternating blocks:

conv at D = 64 and D = 128 (ReLU + dropout 0.5 epilogue, the twice-normalised operator's s and w):
  fused_fwd     : ops.jk_gcn_aggregate over the loop-free CSR -- the row's own table row is its root, w_i on it;
  composed_fwd  : ops.gcn_aggregate(dinv=s) over the CSR WITH one self loop per row (`GcnGraph`: the loop is an edge of weight s_i^2),
                  the diagonal correction (w - s^2) * T added in torch, then ops.feature_dropout(relu=True, bias=);
  fused_bwd     : ops.jk_gcn_aggregate_bwd (g from (y, dy), the walk over the by-source view, the column sums of g);
  composed_bwd  : ops.feature_dropout_bwd(relu=True), ops.gcn_aggregate_bwd(epilogue=None, dinv=s) over the with-loop by-source
                  view, the diagonal correction on g in torch, and the same column sums.
  Byte model of one walk (Dp = pad4(D)): E(4 Dp + 8) + N(12 Dp + 12) -- a gathered row, its scale and a column id per edge; the own
  row, the output row, rowptr, s and w per node; the backward adds its row pass N * 12 Dp (y, dy, g).

head at (L, H, C) = (2, 64, 2), (3, 64, 31), (4, 128, 31), modes cat and max (log_softmax on):
  fused_fwd     : ops.jk_head on the layer buffer (evaluation: nothing but the log-probabilities is written);
  composed_fwd  : torch.cat / torch.stack().max of the L layer slices, torch.addmm, F.log_softmax;
  fused_fb      : ops.jk_head(want_state=True) + ops.jk_head_bwd (training forward and backward);
  composed_fb   : the composition under autograd, forward and torch.autograd.grad to the layers, the weight and the bias.
  Byte model of the forward: N * 4 * (L * Hp + pad4(C)); FLOP: 2 N K C with K = L * H (cat) or H (max), against the fp32-input
  MFMA peak of 157.3 TFLOP/s.

`*_model_GBps` is the byte count over the measured time.  Timing: a warm-up, a rehearsal burst, then one event pair round `--k`
calls per sample; the median of the samples and their spread (max - min) per candidate."""
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

from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.gcn import GcnGraph  # noqa: E402
from bridged_gnn_amd.jknet import JKGraph  # noqa: E402

MFMA_F32_PEAK = 157.3e12


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
    print("[jknet_time]", *a, file=sys.stderr, flush=True)


def report(tm, model):
    out = {k + "_ms": round(v[0], 4) for k, v in tm.items()}
    out.update({k + "_spread_ms": round(v[1], 4) for k, v in tm.items()})
    out.update({k + "_model_bytes": v for k, v in model.items()})
    out.update({k + "_model_GBps": round(v / (tm[k][0] * 1e-3) / 1e9, 1) for k, v in model.items()})
    return out


def conv_case(g, gg, n, E, D, dev, a):
    torch.manual_seed(D)
    Dp = ops.pad4(D)
    p, seed = 0.5, 77
    T, gy = torch.randn(n, Dp, device=dev), torch.randn(n, Dp, device=dev)
    b = torch.randn(Dp, device=dev)
    diag = (g.w.double() - g.s.double() ** 2).float().unsqueeze(1)       # what the with-loop walk gets wrong on the diagonal
    y_buf, dT_buf, z_buf, dTc_buf = (torch.empty(n, Dp, device=dev) for _ in range(4))

    def fused_fwd():
        return ops.jk_gcn_aggregate(T, g.rowptr, g.col, g.s, g.w, n, D, bias=b, epilogue="relu", p_drop=p, seed=seed, out=y_buf)

    def composed_fwd():
        z = ops.gcn_aggregate(T, gg.csr.rowptr, gg.col, g.s, n, D, out=z_buf, hubs=gg.hubs)
        z = torch.addcmul(z, diag, T)
        return ops.feature_dropout(z, p, seed, bias=b, relu=True)

    y = fused_fwd()
    yc = composed_fwd()

    def fused_bwd():
        return ops.jk_gcn_aggregate_bwd(y, gy, g.t_rowptr, g.t_dst, g.s, g.w, n, D, epilogue="relu", p_drop=p, grad_tbl=dT_buf)

    def composed_bwd():
        gz = ops.feature_dropout_bwd(gy, p, seed, y=y, relu=True)
        dT, _ = ops.gcn_aggregate_bwd(None, gz, gg.t_rowptr, gg.t_dst, g.s, n, D, want_bias=False, grad_tbl=dTc_buf, hubs=gg.t_hubs)
        return torch.addcmul(dT, diag, gz), ops.column_sums(gz)[:D]

    err_f = float((y - yc).abs().max().item() / y.abs().max().item())
    fb, cb = fused_bwd(), composed_bwd()
    err_b = [float((u - v).abs().max().item() / max(v.abs().max().item(), 1e-30)) for u, v in zip(fb, cb)]
    tm = alternate({"fused_fwd": fused_fwd, "composed_fwd": composed_fwd, "fused_bwd": fused_bwd, "composed_bwd": composed_bwd},
                   a.rounds, a.k)
    walk = E * (4 * Dp + 8) + n * (12 * Dp + 12)
    note(f"conv D={D}: {tm}")
    return {**report(tm, {"fused_fwd": walk, "fused_bwd": walk + n * 12 * Dp}),
            "fwd_composed_over_fused": round(tm["composed_fwd"][0] / tm["fused_fwd"][0], 3),
            "bwd_composed_over_fused": round(tm["composed_bwd"][0] / tm["fused_bwd"][0], 3),
            "max_rel_diff_fwd": err_f, "max_rel_diff_bwd_dT_db": err_b}


def head_case(n, L, H, C, mode, dev, a):
    torch.manual_seed(L * 1000 + H + C)
    Hp, Cp = ops.pad4(H), ops.pad4(C)
    K = (L if mode == "cat" else 1) * H
    buf = torch.relu(torch.randn(n, L * Hp, device=dev))
    ys = [buf[:, l * Hp:l * Hp + H] for l in range(L)]
    W = torch.randn(C, K, device=dev) / np.sqrt(K)
    b = torch.randn(C, device=dev)
    wp = ops.jk_pack_weight(W, L, H, mode)
    gy = torch.zeros(n, Cp, device=dev)
    gy[:, :C] = torch.randn(n, C, device=dev)

    def jump(xs):
        return torch.cat(xs, 1) if mode == "cat" else torch.stack(xs, -1).max(-1)[0]

    def fused_fwd():
        return ops.jk_head(buf, L, H, mode, wp, b, C)

    def composed_fwd():
        with torch.no_grad():
            return F.log_softmax(torch.addmm(b, jump(ys), W.t()), 1)

    def fused_fb():
        out, win, jmp = ops.jk_head(buf, L, H, mode, wp, b, C, want_state=True)
        return ops.jk_head_bwd(buf, L, H, mode, wp, C, out, gy, win=win, jump=jmp)

    leaves = [y.detach().clone().requires_grad_(True) for y in ys]
    Wl, bl = W.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def composed_fb():
        out = F.log_softmax(torch.addmm(bl, jump(leaves), Wl.t()), 1)
        return torch.autograd.grad(out, leaves + [Wl, bl], grad_outputs=gy[:, :C])

    err_f = float((fused_fwd()[:, :C] - composed_fwd()).abs().max().item())
    gx, gwp, gb = fused_fb()
    cg = composed_fb()
    err_b = [float((gx[:, l * Hp:l * Hp + H] - cg[l]).abs().max().item() / max(cg[l].abs().max().item(), 1e-30)) for l in range(L)]
    err_b.append(float((gb - cg[-1]).abs().max().item() / cg[-1].abs().max().item()))
    tm = alternate({"fused_fwd": fused_fwd, "composed_fwd": composed_fwd, "fused_fb": fused_fb, "composed_fb": composed_fb},
                   a.rounds, a.k)
    note(f"head L={L} H={H} C={C} {mode}: {tm}")
    flop = 2.0 * n * K * C
    return {**report(tm, {"fused_fwd": n * 4 * (L * Hp + Cp)}),
            "fused_fwd_TFLOPs": round(flop / (tm["fused_fwd"][0] * 1e-3) / 1e12, 3),
            "fused_fwd_share_of_mfma_f32_peak": round(flop / (tm["fused_fwd"][0] * 1e-3) / MFMA_F32_PEAK, 4),
            "fwd_composed_over_fused": round(tm["composed_fwd"][0] / tm["fused_fwd"][0], 3),
            "fb_composed_over_fused": round(tm["composed_fb"][0] / tm["fused_fb"][0], 3),
            "max_abs_diff_fwd": err_f, "max_rel_diff_bwd_layers_db": err_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, default=5, help="calls per event pair")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "jknet_time needs an MI355X"
    dev = torch.device("cuda:0")
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0), cluster=1024, seed=0)
    eid = torch.from_numpy(ei).to(dev)
    g, gg = JKGraph(eid, n), GcnGraph(eid, n)
    E = int(g.csr.num_edges)
    res = {"tool": "jknet_time", "nodes": n, "edges_without_loops": E, "conv": {}, "head": {}}
    for D in (64, 128):
        res["conv"][f"D{D}"] = conv_case(g, gg, n, E, D, dev, a)
        torch.cuda.empty_cache()
    del g, gg
    for L, H, C in ((2, 64, 2), (3, 64, 31), (4, 128, 31)):
        for mode in ("cat", "max"):
            res["head"][f"L{L}_H{H}_C{C}_{mode}"] = head_case(n, L, H, C, mode, dev, a)
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
