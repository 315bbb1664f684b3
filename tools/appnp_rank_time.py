"""GPU side of ONE rank of a partition of the C4-shaped graph for APPNP's propagation (bridged_gnn_amd.dist_appnp), on one GPU: the
real partitions of rank r (AppnpPartition: owned rows, rectangular CSR of A' + I and of its transpose, global-degree dinv, hub
tables, send lists) with the collective replaced by a local stand-in of the same size (all_to_all = a device copy into a buffer of
the received size), as tools/gcn_rank_time.py does for GCN.  Per width C in {2, 31} and world in {1, 2, 4, 8}, K = 10, alpha = 0.1:
  forward  : `_propagate` over the forward tables with the closing log_softmax (K steps, K exchanges);
  backward : the row pass g = dy - exp(y) rowsum(dy), the gather into the transposed partition's row order, `_propagate` over the
             transposed tables, the gather back;
each split into  steps_ms  (the K `ops.appnp_step` calls alone -- kernel time)  and  exchange_ms  (the K exchanges alone: pack with
`ops.gather_rows`, the stand-in copy, the landing copy -- the GPU work of an exchange, NOT its time on a fabric), next to the
whole call (total_ms) and to the single-GPU `ops.appnp_propagate` on the whole graph, timed in the same process as
tools/appnp_time.py times it.  The numbers are the per-rank GPU work a multi-GPU run cannot go below; the outputs are NOT the
model's (the halo holds stand-in rows).  No multi-GPU run is made: the latency of 2K all_to_alls per epoch is not in these numbers.
Timing: a warm-up, a rehearsal burst, then one event pair round `--k` calls per sample; the median of `--rounds` samples.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.dist_appnp import AppnpPartition, _exchange, _ext_rows, _propagate, _StepTables  # noqa: E402
from bridged_gnn_amd.gcn import GcnGraph  # noqa: E402


class StandInComm:
    """`dist_train._Comm` with the payload moved by a device copy of the received size instead of a collective"""
    live, host = True, False

    def all_to_all(self, send, send_splits, recv_splits):
        n = int(sum(recv_splits))
        recv = torch.zeros((n,) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
        k = min(n, send.shape[0])
        recv[:k].copy_(send[:k])
        return recv


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
    return {name: round(float(np.median(v)), 4) for name, v in ts.items()}


def note(*a):
    print("[appnp_rank_time]", *a, file=sys.stderr, flush=True)


def steps_only(tabs, hx, C, K, alpha, last):
    """the K step launches of `_propagate` with no exchange between them"""
    nl = tabs.n_local
    state = [torch.empty(tabs.n_ext, hx.shape[1], dtype=torch.float32, device=hx.device) for _ in range(2)]
    out = torch.empty(nl, hx.shape[1], dtype=torch.float32, device=hx.device)

    def run():
        src = hx
        for k in range(K):
            fin = k == K - 1
            dst = out if fin else state[k & 1][:nl]
            ops.appnp_step(src, hx[:nl], tabs.rowptr, tabs.col, tabs.dinv, nl, C, alpha, first=k == 0, store=last if fin else "state",
                           hubs=tabs.hubs, out=dst)
            src = out if fin else state[k & 1]
    return run


def rank_case(part_tabs, t_tabs, perm, C, K, alpha, comm, rounds, k, dev):
    Dp = ops.pad4(C)
    nl = part_tabs.n_local
    hx = _ext_rows(part_tabs, C, dev).normal_()
    hx[:, C:] = 0
    dy = torch.randn(nl, Dp, device=dev)
    dy[:, C:] = 0
    gx = _ext_rows(t_tabs, C, dev).zero_()
    y = _propagate(comm, part_tabs, hx, C, K, alpha, "log_softmax")

    def backward():
        g = ops.appnp_log_softmax_bwd(y, dy, C)
        ops.gather_rows(g, perm[0], out=gx[:nl])
        return ops.gather_rows(_propagate(comm, t_tabs, gx, C, K, alpha, None), perm[1])

    def exchanges(tabs, buf):
        def run():
            for _ in range(K):
                _exchange(comm, tabs, buf)
        return run

    t = alternate({"fwd_total": lambda: _propagate(comm, part_tabs, hx, C, K, alpha, "log_softmax"),
                   "fwd_steps": steps_only(part_tabs, hx, C, K, alpha, "log_softmax"),
                   "fwd_exchange": exchanges(part_tabs, hx),
                   "bwd_total": backward,
                   "bwd_steps": steps_only(t_tabs, gx, C, K, alpha, "out"),
                   "bwd_exchange": exchanges(t_tabs, gx)}, rounds, k)
    return {k_ + "_ms": v for k_, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--worlds", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--k", type=int, default=3, help="calls per event pair")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "appnp_rank_time needs an MI355X"
    dev = torch.device("cuda:0")
    n, K, alpha = a.nodes, a.K, a.alpha
    n_tar = n - n // 2
    ei, _ = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                cluster=1024, seed=0)                  # tools/appnp_time.py's graph
    res = {"tool": "appnp_rank_time", "measured": "one rank's GPU work, the all_to_all replaced by a device copy of the same size; "
           "no multi-GPU run", "nodes": n, "edges": int(ei.shape[1]), "K": K, "alpha": alpha, "rank": a.rank, "single_gpu_ms": {},
           "worlds": {}}

    # the single-GPU propagation on the whole graph (tools/appnp_time.py's fused_fwd / fused_bwd)
    g = GcnGraph(torch.from_numpy(ei).to(dev), n)
    for C in (2, 31):
        Dp = ops.pad4(C)
        h = torch.randn(n, Dp, device=dev)
        dy = torch.randn(n, Dp, device=dev)
        dy[:, C:] = 0
        y = ops.appnp_propagate(h, g.csr.rowptr, g.col, g.dinv, n, C, K, alpha, epilogue="log_softmax", hubs=g.hubs)
        t = alternate({"fwd": lambda: ops.appnp_propagate(h, g.csr.rowptr, g.col, g.dinv, n, C, K, alpha, epilogue="log_softmax",
                                                          hubs=g.hubs),
                       "bwd": lambda: ops.appnp_propagate(ops.appnp_log_softmax_bwd(y, dy, C), g.t_rowptr, g.t_dst, g.dinv, n, C, K,
                                                          alpha, hubs=g.t_hubs)}, a.rounds, a.k)
        res["single_gpu_ms"][f"C{C}"] = t
        note(f"single GPU C={C}: {t}")
        del h, dy, y
    del g
    torch.cuda.empty_cache()

    comm = StandInComm()
    for world in a.worlds:
        t0 = time.perf_counter()
        part = AppnpPartition(ei, n, min(a.rank, world - 1), world)
        plan_s = time.perf_counter() - t0
        tabs, t_tabs = _StepTables(part, dev), _StepTables(part.t, dev)
        perm = (torch.from_numpy(part.t_from_f).to(dev), torch.from_numpy(part.f_from_t).to(dev))
        w = {"n_local": part.n_local, "n_halo": part.n_halo, "send_rows": int(part.send_rows.shape[0]), "local_edges": part.num_edges,
             "t_n_halo": part.t.n_halo, "t_send_rows": int(part.t.send_rows.shape[0]), "t_local_edges": part.t.num_edges,
             "hub_rows": 0 if tabs.hubs is None else int(tabs.hubs[1].shape[0]),
             "t_hub_rows": 0 if t_tabs.hubs is None else int(t_tabs.hubs[1].shape[0]), "plan_s": round(plan_s, 2)}
        for C in (2, 31):
            Dp = ops.pad4(C)
            r = rank_case(tabs, t_tabs, perm, C, K, alpha, comm, a.rounds, a.k, dev)
            r["exchange_bytes_per_step"] = {"fwd_send": int(part.send_rows.shape[0]) * Dp * 4, "fwd_recv": part.n_halo * Dp * 4,
                                            "bwd_send": int(part.t.send_rows.shape[0]) * Dp * 4, "bwd_recv": part.t.n_halo * Dp * 4}
            single = res["single_gpu_ms"][f"C{C}"]
            r["share_of_single_gpu"] = {"fwd": round(r["fwd_total_ms"] / single["fwd"], 4), "bwd": round(r["bwd_total_ms"] / single["bwd"], 4),
                                        "ideal": round(1.0 / world, 4)}
            w[f"C{C}"] = r
            note(f"world {world} C={C}: {r}")
        res["worlds"][str(world)] = w
        del tabs, t_tabs, part
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
