"""Times one epoch of step 2's driver eager against `graphed=True` (one replay of the captured epoch, `transfer._GraphedEpoch`), and
the fused Adam against torch's, with the method of tools/sage_time.py (device events, medians, alternating blocks).  One JSON line
per case:
  epoch:  office A->D (tests/golden/office_a2d_graph.npz, C = 31, hidden 64), the Twitter stand-in (`synth.twitter_standin`, C = 2,
          hidden 128) and the C4-shaped graph (synth.bridged_graph, 1M nodes / 20M edges, C = 2, hidden 64): `eager_ms` is the epoch
          of `train_gnn(graphed=False)` (torch Adam, train step, eval forward, counts into the history), `graphed_ms` one replay;
          `eager_launches` counts the device kernels of one eager epoch (torch profiler; null where it is not available);
          `spread` is (max - min) / median over the blocks' medians, per column;
  adam:   `FusedAdam.step()` against `torch.optim.Adam` (foreach) and `Adam(capturable=True)` on the office model's parameters.
`--replay-only N`: N graphed office epochs and nothing else (for `rocprofv3 --kernel-trace --stats -- python
tools/transfer_graphed_time.py --replay-only 50`, see profiles/transfer_graphed/README.md)."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import ops, synth, transfer  # noqa: E402
from bridged_gnn_amd.data import Data  # noqa: E402
from bridged_gnn_amd.ktgnn import KTGNN_no_complement  # noqa: E402
from bridged_gnn_amd.optim import FusedAdam  # noqa: E402
from tools.sage_time import timed  # noqa: E402
from tools.transfer_time import c4_data, office_data  # noqa: E402


def twitter_data(dev):
    x, ei, y, cm = synth.twitter_standin()
    g = torch.Generator().manual_seed(1)
    u = torch.rand(x.shape[0], generator=g)
    cm = torch.from_numpy(cm)
    d = Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei).long(), y=torch.from_numpy(y), train_mask=u < 0.5,
             val_mask=(u >= 0.5) & (u < 0.7) & ~cm, test_mask=(u >= 0.7) & ~cm, central_mask=cm).to(dev)
    return d.to_undirected_()


def blocks(fa, fb, rounds, reps):
    """A and B in alternating blocks -> per column (median of the blocks' medians, (max - min) / median of them)"""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    col = lambda t: (float(np.median(t)), float((max(t) - min(t)) / np.median(t)))
    return col(ta), col(tb)


def kernel_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as e:                                  # the figure is reported as missing, with the reason
        print(f"# kernel count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def build(data, C, hidden):
    dev = data.x.device
    plan = transfer._plan(data, True)
    torch.manual_seed(0)
    m = KTGNN_no_complement(data.x.shape[1], C, 2, hidden, use_bn=True, dim_share=data.x.shape[1], dropout=0.5).to(dev)
    transfer._prime(m, data, lambda o: ops.step2_loss(o[0], o[1], o[2], plan.y, plan.train_u8, plan.central_u8, 1.0))
    return m, plan


def epoch_case(name, data, C, hidden, a):
    dev = data.x.device
    E = 1 << 12
    # eager: the loop body of train_gnn(graphed=False)
    m_e, plan = build(data, C, hidden)
    opt = torch.optim.Adam(m_e.parameters(), lr=1e-3, weight_decay=5e-3)
    h_e = transfer._History(dev, 1, 8, len(transfer._DTC_COMBOS), C, False, 1)

    def eager():
        h_e.n = 0
        t, c, _ = h_e.slot()
        t.copy_(transfer._train_step(data, m_e, opt, plan, 1.0))
        transfer._eval_dtc(data, m_e, plan, counts_out=c)
    # graphed: the same body as one replay
    m_g, _ = build(data, C, hidden)
    h_g = transfer._History(dev, E, 8, len(transfer._DTC_COMBOS), C, False, 0)
    fopt = transfer._graphed_optimizer(m_g, 1e-3, 5e-3, E, 100, 0.1)
    ge = transfer._GraphedEpoch(data, m_g, fopt, h_g, E, 1,
                                lambda o: ops.step2_loss(o[0], o[1], o[2], plan.y, plan.train_u8, plan.central_u8, 1.0, return_terms=True),
                                lambda counts, auc: transfer._eval_dtc(data, m_g, plan, counts_out=counts, auc_out=auc))
    for _ in range(3):
        eager(); ge.replay()
    torch.cuda.synchronize()
    (t_e, s_e), (t_g, s_g) = blocks(eager, ge.replay, a.rounds, a.reps)
    n_launch = kernel_launches(eager)
    return {"tool": "transfer_graphed_time", "case": name, "nodes": int(data.x.shape[0]), "edges": int(data.edge_index.shape[1]), "classes": C,
            "hidden": hidden, "epoch": {"eager_ms": round(t_e, 4), "graphed_ms": round(t_g, 4), "speedup": round(t_e / t_g, 3),
                                        "eager_spread": round(s_e, 4), "graphed_spread": round(s_g, 4), "eager_launches": n_launch,
                                        "graphed_submissions": 1},
            "device": torch.cuda.get_device_name(0)}


def adam_case(data, a):
    dev = data.x.device
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in KTGNN_no_complement(data.x.shape[1], 31, 2, 64, use_bn=True, dim_share=data.x.shape[1]).parameters()]

    def params():
        ps = [torch.randn(s, device=dev).requires_grad_() for s in shapes]
        for p in ps:
            p.grad = torch.randn_like(p) * 0.1
        return ps
    fused = FusedAdam(params(), lr=1e-3, weight_decay=5e-3)
    foreach = torch.optim.Adam(params(), lr=1e-3, weight_decay=5e-3, foreach=True)
    capt = torch.optim.Adam(params(), lr=1e-3, weight_decay=5e-3, capturable=True)
    for o in (fused, foreach, capt):
        for _ in range(3):
            o.step()
    torch.cuda.synchronize()
    cols = {"fused": [], "foreach": [], "capturable": []}
    for _ in range(a.rounds):
        cols["fused"].append(timed(fused.step, a.reps))
        cols["foreach"].append(timed(foreach.step, a.reps))
        cols["capturable"].append(timed(capt.step, a.reps))
    med = {k: float(np.median(v)) for k, v in cols.items()}
    return {"tool": "transfer_graphed_time", "case": "adam_office_params", "tensors": len(shapes), "elements": int(sum(int(np.prod(s)) for s in shapes)),
            "step": {"fused_ms": round(med["fused"], 4), "torch_foreach_ms": round(med["foreach"], 4),
                     "torch_capturable_ms": round(med["capturable"], 4), "fused_launches": kernel_launches(fused.step),
                     "torch_foreach_launches": kernel_launches(foreach.step), "torch_capturable_launches": kernel_launches(capt.step)},
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="office,adam,twitter,c4", help="comma-separated subset of office, adam, twitter, c4")
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--replay-only", type=int, default=0, help="this many graphed office epochs through train_gnn and nothing else")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transfer_graphed_time needs an MI355X"
    dev = torch.device("cuda:0")
    if a.replay_only:
        data = office_data(dev)
        transfer.train_gnn(types.SimpleNamespace(dataset_name="office"), transfer.pyg_dataset(data), data, repeat=1, num_epoch=a.replay_only,
                           gnn="KTGNN", seed=0, hidden=64, verbose=False, graphed=True)
        torch.cuda.synchronize()
        return
    lines = []
    for name in a.cases.split(","):
        if name == "office":
            res = epoch_case("office_a2d", office_data(dev), 31, 64, a)
        elif name == "adam":
            res = adam_case(office_data(dev), a)
        elif name == "twitter":
            res = epoch_case("twitter_standin", twitter_data(dev), 2, 128, a)
        elif name == "c4":
            res = epoch_case("c4_C2", c4_data(a.nodes, a.edges, 2, dev), 2, 64, a)
        else:
            raise SystemExit(f"unknown case {name!r}")
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
