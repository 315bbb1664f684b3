"""Timing of the wide three-head classifier walk (bgnn_adaptedconv_aggregate_heads_wide_f32 + backward) on the C4-shaped graph
(bench.py's generator: 1M nodes / ~21M edges, hidden 128) with C = 31 classes.  Prints JSON lines:
  stage  -- the classifier stage's aggregation forward + backward over the same six tables: three per-conv walks (_AggregateFn +
            torch log_softmax, the default route at C > 4) against the wide heads (_AggregateWideHeadsFn), alternating;
  step   -- the full single-GPU training step (forward, reference loss, backward) with BGNN_WIDE_TRAIN_HEADS unset and =1, alternating;
  rank   -- one rank's GPU work of an 8-way partitioned training step (dist_train.PartitionedTrainer, wide route at C = 31), the
            collectives replaced by same-sized device copies as in tools/sage_rank_time.py (outputs are NOT the model's).
Times are medians of device-event times.  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/wide_heads_time.py`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bridged_gnn_amd import ops, synth  # noqa: E402
from bridged_gnn_amd.data import Data  # noqa: E402
from bridged_gnn_amd.ktgnn import KTGNN_no_complement, _AggregateFn, _AggregateWideHeadsFn  # noqa: E402


class StandInComm:
    """`dist_train._Comm` with the payload moved by a device copy of the received size instead of a collective"""
    live, host = True, False

    def all_to_all(self, send, send_splits, recv_splits):
        n = int(sum(recv_splits))
        recv = torch.zeros((n,) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)
        k = min(n, send.shape[0])
        recv[:k].copy_(send[:k])
        return recv

    def all_reduce(self, t):
        return t


def ev_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warmup=3):
    """{name: median ms}, the variants run alternately"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(ev_time(f))
    return {k: float(np.median(v)) for k, v in ts.items()}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def ref_loss(out, y, tm, cm, n):
    lb, lt, lth = out[:3]
    tmt = tm & ~cm
    yi = y[:, None]
    nll = lambda logp, w: -(logp.gather(1, yi).squeeze(1) * w).sum()
    return (2 * nll(lb, tm.float() / tm.sum()) + nll(lt, tmt.float() / tmt.sum()) + nll(lth, tmt.float() / tmt.sum())) / 4 \
        + F.kl_div(lth, lt, log_target=True, reduction="batchmean")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--classes", type=int, default=31)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=7)
    ap.add_argument("--skip", default="", help="comma list of parts to skip: stage,step,rank")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) - {""}
    assert torch.cuda.is_available(), "wide_heads_time needs an MI355X"
    dev = torch.device("cuda:0")
    n, C = a.nodes, a.classes
    n_tar = n - n // 2
    ei, mask = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(a.edges - 6 * n - 20 * n_tar, 0),
                                   cluster=1024, p_local=0.9, seed=0)            # bench.py's C4 (graph "local")
    torch.manual_seed(0)
    model = KTGNN_no_complement(128, C, 2, a.hidden, use_bn=True, dim_share=128, dropout=0.0).to(dev).train()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, 128, device=dev, generator=g)
    y = torch.randint(0, C, (n,), device=dev, generator=g)
    tm = torch.rand(n, device=dev, generator=g) < 0.5
    cm = torch.from_numpy(mask).to(dev)
    data = Data(x=x, edge_index=torch.from_numpy(ei).to(dev), central_mask=cm)
    os.environ.pop("BGNN_WIDE_TRAIN_HEADS", None)
    model(data)                                                                    # builds and caches the CSR
    csr = model._csr
    base = dict(nodes=n, edges=int(csr.num_edges), classes=C, hidden=a.hidden)

    if "stage" not in skip:
        m_u8 = cm.to(torch.uint8).contiguous()
        h = torch.randn(n, a.hidden, device=dev, generator=g)
        with torch.no_grad():
            tabs = [t.contiguous() for t in (*model.clf_base._transform_autograd(h, m_u8), *model.clf_target._transform_autograd(h, m_u8),
                                             *model.clf_target._transform_autograd(h, m_u8))]
        tabs = [t.requires_grad_(True) for t in tabs]
        cs = (model.clf_base, model.clf_target, model.clf_target)
        a_t = torch.stack([c.a_f_t2s.weight.detach().reshape(-1) for c in cs]).requires_grad_(True)
        a_s = torch.stack([c.a_f_s2t.weight.detach().reshape(-1) for c in cs]).requires_grad_(True)
        gl = torch.randn(n, 3, C, device=dev, generator=g)
        slope = model.clf_base.negative_slope

        def per_conv():
            outs = [F.log_softmax(_AggregateFn.apply(tabs[2 * j], tabs[2 * j + 1], a_t[j], a_s[j], csr, m_u8, C, slope)[:, :C], dim=1)
                    for j in range(3)]
            torch.autograd.backward(outs, [gl[:, j] for j in range(3)])

        def wide():
            logp = _AggregateWideHeadsFn.apply(csr, m_u8, C, slope, a_t, a_s, *tabs)[:, :, :C]
            logp.backward(gl)

        def per_conv_fwd():
            with torch.no_grad():
                for j in range(3):
                    F.log_softmax(_AggregateFn.apply(tabs[2 * j], tabs[2 * j + 1], a_t[j], a_s[j], csr, m_u8, C, slope)[:, :C], dim=1)

        def wide_fwd():
            with torch.no_grad():
                _AggregateWideHeadsFn.apply(csr, m_u8, C, slope, a_t, a_s, *tabs)
        r = alternate({"per_conv_ms": per_conv, "wide_ms": wide}, a.reps)
        rf = alternate({"per_conv_fwd_ms": per_conv_fwd, "wide_fwd_ms": wide_fwd}, a.reps)
        emit(dict(base, what="classifier stage aggregation, forward + backward", **r, **rf), a.out)

    if "step" not in skip:
        def step(flag):
            def f():
                if flag:
                    os.environ["BGNN_WIDE_TRAIN_HEADS"] = "1"
                else:
                    os.environ.pop("BGNN_WIDE_TRAIN_HEADS", None)
                model.zero_grad(set_to_none=True)
                ref_loss(model(data), y, tm, cm, n).backward()
            return f
        r = alternate({"default_ms": step(False), "wide_opt_in_ms": step(True)}, a.reps)
        os.environ.pop("BGNN_WIDE_TRAIN_HEADS", None)
        emit(dict(base, what="single-GPU training step (forward + loss + backward)", **r), a.out)

    if "rank" not in skip:
        from bridged_gnn_amd.dist_train import PartitionedTrainer
        t0 = time.perf_counter()
        tr = PartitionedTrainer(model, ei, mask, a.rank, a.world, dev)
        plan_s = time.perf_counter() - t0
        tr.comm = StandInComm()
        own = tr.owned_global
        xl, yl, tml = x[own].contiguous(), y[own], tm[own]

        def rank_step():
            model.zero_grad(set_to_none=True)
            tr.reference_loss(tr.forward(xl), yl, tml).backward()
        r = alternate({"rank_step_ms": rank_step}, a.reps)
        emit(dict(base, what=f"rank {a.rank} of {a.world}: partitioned training step, collectives as device copies",
                  plan=tr.plan.summary(), plan_build_s=round(plan_s, 1), **r), a.out)


if __name__ == "__main__":
    main()
