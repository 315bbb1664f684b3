"""Times the GATv2 attention conv (ops.gatv2_aggregate / gatv2_aggregate_bwd) on the C4-shaped graph tools/gcn_time.py and
tools/gat_time.py use (synth.bridged_graph, 1M nodes / 20M edges + one self loop per node) at (heads, channels) = (1, 64) with the
ELU + dropout epilogue and attention dropout 0.5 (the reference's first conv) and (1, 2) with the log_softmax epilogue (its last),
and an office epoch of `train_gatv2_noDTC` eager and graphed.  One JSON line.  Per shape, in this process, alternating blocks:
  fused_fwd     : the one-pass forward (one launch);
  fused_fwd_bwd : the same (keeping the pre-activation) followed by the backward (row pass, by-destination pass, datt sum,
                  by-source pass, column sums of g);
  torch_fwd     : the composition from torch index ops -- gathers of x_l[src] and x_r[dst], leaky_relu, the att product and row
                  sum, scatter_reduce(amax), exp, index_add_ for the denominator, dropout, index_add_ of the weighted rows, the
                  same epilogue;
  gat_fwd       : GAT's conv at the same (H, C) on the same graph (scores + coefficient pass + gather pass, three launches).
Byte model of the fused forward: E'(4HC + 4) + N(12HC): one neighbour row and one column index per edge and head group, the row's
own x_r, and the output written once; `fwd_frac_of_8TBps` is that over the time as a share of 8 TB/s (a fabric-side figure: most
gathers are L2 hits).
Timing: a warm-up, a rehearsal burst, then one event pair round K launches per sample; the median of the samples.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gatv2_time.py --skip-office --skip-torch` (profiles/gatv2/README.md)."""
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
from bridged_gnn_amd.gat import GatGraph  # noqa: E402

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
    from bridged_gnn_amd import gatv2, transfer
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
        gatv2.train_gatv2_noDTC(args, transfer.pyg_dataset(d), d, repeat=1, num_epoch=n, seed=0, hidden=64, heads=1,
                                use_scheduler=False, verbose=False, graphed=graphed)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return (out[2] - out[1]) / epochs * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, default=5, help="launches per event pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--office-epochs", type=int, default=200)
    ap.add_argument("--skip-office", action="store_true")
    ap.add_argument("--office-only", action="store_true")
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch composition out (a profile of the kernels alone)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gatv2_time needs an MI355X"
    dev = torch.device("cuda:0")
    if a.office_only:
        print(json.dumps({"tool": "gatv2_time", "office_epoch_ms": {"eager": round(office_epochs(False, a.office_epochs), 4),
                                                                    "graphed": round(office_epochs(True, a.office_epochs), 4)}}))
        return
    n = a.nodes
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)
    g = GatGraph(torch.from_numpy(ei).to(dev), n)
    E = int(g.csr.num_edges)
    rowptr, col = g.rowptr, g.col
    deg = (rowptr[1:] - rowptr[:-1]).long()
    src, dst = col.long(), torch.repeat_interleave(torch.arange(n, device=dev), deg)
    res = {"tool": "gatv2_time", "nodes": n, "edges_with_self_loops": E, "max_in_degree": int(deg.max().item()), "shapes": {}}
    for H, C, epi in ((1, 64, "elu"), (1, 2, "log_softmax")):
        HC, P = H * C, ops.pad4(H * C)
        p = 0.6 if epi == "elu" else 0.0
        p_att = 0.5
        T = torch.zeros(n, 2 * P, device=dev)
        T[:, :HC] = torch.randn(n, HC, device=dev)
        T[:, P:P + HC] = torch.randn(n, HC, device=dev)
        att = torch.randn(1, H, C, device=dev) / C ** 0.5
        b = torch.zeros(P, device=dev)
        b[:HC] = torch.randn(HC, device=dev)
        dy = torch.zeros(n, P, device=dev)
        dy[:, :HC] = torch.randn(n, HC, device=dev)
        idx = dst.unsqueeze(1).expand(-1, H)
        Tl = T[:, :P]                                    # GAT's table: the x_l half

        def fused(p_att=p_att, p=p, keep=False):
            return ops.gatv2_aggregate(T, att, rowptr, col, n, H, C, bias=b, p_att=p_att, seed_att=5, epilogue=epi, p_drop=p, seed=7,
                                       want_pre=keep)

        def fused_fwd_bwd():
            _, state, pre, _ = fused(keep=True)
            return ops.gatv2_aggregate_bwd(T, att, state, pre, dy, rowptr, col, g.t_rowptr, g.t_eid, g.t_dst, H, C, bias=b, p_att=p_att,
                                           seed_att=5, epilogue=epi, p_drop=p, seed=7)

        def gat_fwd():
            s_src, s_dst = ops.gat_scores(Tl, att, att, H, C)
            return ops.gat_aggregate(Tl, s_src, s_dst, rowptr, col, n, H, C, bias=b, p_att=p_att, seed_att=5, epilogue=epi, p_drop=p,
                                     seed=7)

        def torch_eager(p_att=p_att, p=p):
            XL, XR = T[:, :HC].reshape(n, H, C), T[:, P:P + HC].reshape(n, H, C)
            e = (F.leaky_relu(XL[src] + XR[dst], 0.2) * att).sum(-1)
            m = torch.full((n, H), -float("inf"), device=dev).scatter_reduce(0, idx, e, "amax")
            ex = (e - m[dst]).exp()
            den = torch.zeros(n, H, device=dev).index_add_(0, dst, ex)
            al = F.dropout(ex / den[dst], p=p_att, training=True)
            z = torch.zeros(n, H, C, device=dev).index_add_(0, dst, XL[src] * al.unsqueeze(-1)).view(n, HC) + b[:HC]
            return F.dropout(F.elu(z), p=p, training=True) if epi == "elu" else F.log_softmax(z, dim=1)

        fns = {"fused_fwd": fused, "fused_fwd_bwd": fused_fwd_bwd, "gat_fwd": gat_fwd}
        err = None
        if not a.skip_torch:
            err = float((fused(0.0, 0.0)[0][:, :HC] - torch_eager(0.0, 0.0)).abs().max().item())
            fns["torch_fwd"] = torch_eager
        t = alternate(fns, a.rounds, a.k)
        byts = E * (4 * HC + 4) + n * (12 * HC)
        res["shapes"][f"H{H}C{C}"] = {**{k + "_ms": round(v, 4) for k, v in t.items()}, "epilogue": epi, "model_bytes": byts,
                                      "fwd_model_bytes_per_s": round(byts / (t["fused_fwd"] * 1e-3), 1),
                                      "fwd_frac_of_8TBps": round(byts / (t["fused_fwd"] * 1e-3) / FABRIC_BPS, 4),
                                      "max_abs_diff_vs_torch": err}
        if "torch_fwd" in t:
            res["shapes"][f"H{H}C{C}"]["fused_over_torch"] = round(t["torch_fwd"] / t["fused_fwd"], 3)
        del T, Tl, dy
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
