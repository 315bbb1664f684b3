"""Times the GAT attention aggregation (ops.gat_scores / gat_aggregate / gat_aggregate_bwd) on a C4-shaped graph
(synth.bridged_graph, 1M nodes / 20M edges + one self loop per node) at (heads, channels) = (3, 64) with the ELU + dropout
epilogue and attention dropout 0.6 (the reference's first conv) and (1, 2) with the log_softmax epilogue (its second), and an
office epoch of `train_gat_noDTC` eager and graphed.  One JSON line.  Per shape, in this process, alternating blocks:
  fused_fwd     : scores + softmax-state/coefficient pass + gather pass (three launches);
  fused_fwd_bwd : the same followed by the backward (row pass, by-destination edge pass, by-source gather, column sums);
  torch_fwd     : the composition from torch index ops -- gather of the scores, leaky_relu, scatter_reduce(amax), exp,
                  index_add_ for the denominator, dropout, index_add_ of the weighted rows, the same epilogue.
Byte model of the fused forward: E'(4HC + 8H) + N(8HC); `fwd_frac_of_8TBps` is that over the time as a share of 8 TB/s (a
fabric-side figure: most gathers are L2 hits).  What the kernels actually move per edge and head is 20 B next to the 4C B row
(two 4 B score gathers, one 4 B coefficient written and read back, 4 B of column index per head group).  `hub_row_ms`: the
forward at (3, 64) on a graph whose only long row has 30 000 in-edges, minus the same graph without that row.
Timing: a warm-up, a rehearsal burst, then one event pair round K launches per sample; the median of the samples.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/gat_time.py --skip-office` (profiles/gat/README.md)."""
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
    from bridged_gnn_amd import gat, transfer
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
        gat.train_gat_noDTC(args, transfer.pyg_dataset(d), d, repeat=1, num_epoch=n, seed=0, hidden=64, head=3, use_scheduler=False,
                            verbose=False, graphed=graphed)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return (out[2] - out[1]) / epochs * 1e3


def hub_row_ms(dev, k):
    """what one 30 000-edge row costs the (3, 64) forward: a 200k-node graph with and without it"""
    n, H, C = 200_000, 3, 64
    base, _ = synth.random_multigraph(n, 2_000_000, n_isolated=0, seed=5)
    rng = np.random.default_rng(6)
    hub = np.stack([rng.integers(0, n, 30000), np.full(30000, 3)])
    T = torch.randn(n, H * C, device=dev)
    att = torch.randn(H * C, device=dev) / 8
    ms = []
    for ei in (base, np.concatenate([base, hub], axis=1)):
        g = GatGraph(torch.from_numpy(ei.astype(np.int64)).to(dev), n)

        def fwd():
            s = ops.gat_scores(T, att, att, H, C)
            return ops.gat_aggregate(T, s[0], s[1], g.rowptr, g.col, n, H, C)
        fwd()
        burst(fwd, k)
        ms.append(float(np.median([burst(fwd, k) for _ in range(5)])))
    return {"without_ms": round(ms[0], 4), "with_ms": round(ms[1], 4), "hub_row_ms": round(ms[1] - ms[0], 4)}


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
    assert torch.cuda.is_available(), "gat_time needs an MI355X"
    dev = torch.device("cuda:0")
    if a.office_only:
        print(json.dumps({"tool": "gat_time", "office_epoch_ms": {"eager": round(office_epochs(False, a.office_epochs), 4),
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
    res = {"tool": "gat_time", "nodes": n, "edges_with_self_loops": E, "max_in_degree": int(deg.max().item()), "shapes": {}}
    for H, C, epi in ((3, 64, "elu"), (1, 2, "log_softmax")):
        HC, W = H * C, ops.pad4(H * C)
        p = 0.6 if epi == "elu" else 0.0
        p_att = 0.6
        T = torch.zeros(n, W, device=dev)
        T[:, :HC] = torch.randn(n, HC, device=dev)
        a_s, a_d = torch.randn(1, H, C, device=dev) / C ** 0.5, torch.randn(1, H, C, device=dev) / C ** 0.5
        b = torch.zeros(W, device=dev)
        b[:HC] = torch.randn(HC, device=dev)
        dy = torch.zeros(n, W, device=dev)
        dy[:, :HC] = torch.randn(n, HC, device=dev)
        idx = dst.unsqueeze(1).expand(-1, H)

        def fused(p_att=p_att, p=p, keep=False):
            s_src, s_dst = ops.gat_scores(T, a_s, a_d, H, C)
            return (s_src, s_dst) + ops.gat_aggregate(T, s_src, s_dst, rowptr, col, n, H, C, bias=b, p_att=p_att, seed_att=5,
                                                      epilogue=epi, p_drop=p, seed=7, want_pre=keep, return_alpha=keep)

        def fused_fwd_bwd():
            s_src, s_dst, _, state, pre, alpha = fused(keep=True)
            return ops.gat_aggregate_bwd(T, s_src, s_dst, state, alpha, pre, dy, rowptr, col, g.t_rowptr, g.t_eid, g.t_dst, H, C, bias=b,
                                         p_att=p_att, seed_att=5, epilogue=epi, p_drop=p, seed=7)

        def torch_eager(p_att=p_att, p=p):
            Tv = T[:, :HC].view(n, H, C) if W == HC else T[:, :HC].reshape(n, H, C)
            e = F.leaky_relu((Tv * a_s).sum(-1)[src] + (Tv * a_d).sum(-1)[dst], 0.2)
            m = torch.full((n, H), -float("inf"), device=dev).scatter_reduce(0, idx, e, "amax")
            ex = (e - m[dst]).exp()
            den = torch.zeros(n, H, device=dev).index_add_(0, dst, ex)
            al = F.dropout(ex / den[dst], p=p_att, training=True)
            z = torch.zeros(n, H, C, device=dev).index_add_(0, dst, Tv[src] * al.unsqueeze(-1)).view(n, HC) + b[:HC]
            return F.dropout(F.elu(z), p=p, training=True) if epi == "elu" else F.log_softmax(z, dim=1)

        err = float((fused(0.0, 0.0)[2][:, :HC] - torch_eager(0.0, 0.0)).abs().max().item())
        fns = {"fused_fwd": fused, "fused_fwd_bwd": fused_fwd_bwd}
        if not a.skip_torch:
            fns["torch_fwd"] = torch_eager
        t = alternate(fns, a.rounds, a.k)
        byts = E * (4 * HC + 8 * H) + n * (8 * HC)
        res["shapes"][f"H{H}C{C}"] = {**{k + "_ms": round(v, 4) for k, v in t.items()}, "epilogue": epi, "model_bytes": byts,
                                      "fwd_model_bytes_per_s": round(byts / (t["fused_fwd"] * 1e-3), 1),
                                      "fwd_frac_of_8TBps": round(byts / (t["fused_fwd"] * 1e-3) / FABRIC_BPS, 4),
                                      "max_abs_diff_vs_torch": err}
        if "torch_fwd" in t:
            res["shapes"][f"H{H}C{C}"]["fused_over_torch"] = round(t["torch_fwd"] / t["fused_fwd"], 3)
        del T, dy
    res["hub_row"] = hub_row_ms(dev, a.k)
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
