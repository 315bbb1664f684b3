"""Times step 2's fused loss and one epoch of `transfer.train_gnn`'s loop, with the method of tools/sage_time.py (device events,
alternating blocks, medians).  Prints one JSON line per case:
  loss:   `ops.step2_loss` forward + backward against the torch-op form of bench.py:706-715 (gather / weights / F.kl_div + autograd)
          on the same three [N, C] tables;
  epoch:  one epoch of the driver (train step with the fused loss, ONE eval forward, one count launch, nothing read back) against
          the composed loop (train step with the torch-op loss, TWO eval forwards, predictions copied to the host and scored there
          from np.bincount confusion counts, as the reference's sklearn calls would be fed); `parts` splits the difference: one eval
          forward, the host-side scoring (mask compaction, copies, counting) against the device count launch, the loss.
Cases: the C4-shaped graph (synth.bridged_graph, 1M nodes / 20M edges, Din 128, hidden 64) with C = 2 and C = 31, and the office
graph (tests/golden/office_a2d_graph.npz, 3408 nodes, C = 31).  `--epoch-only` runs a few driver epochs and nothing else (for
`rocprofv3 --kernel-trace --stats -- python tools/transfer_time.py --epoch-only`, see profiles/transfer/README.md)."""
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

from bridged_gnn_amd import ops, synth, transfer  # noqa: E402
from bridged_gnn_amd.data import Data  # noqa: E402
from bridged_gnn_amd.ktgnn import KTGNN_no_complement  # noqa: E402
from tools.sage_time import alternate  # noqa: E402


def c4_data(n, edges, C, dev):
    n_tar = n - n // 2
    ei, cm = synth.bridged_graph(n // 2, n_tar, k_within=6, k_cross=20, n_extra=max(edges - 6 * n - 20 * n_tar, 0), cluster=1024, seed=0)
    g = torch.Generator().manual_seed(1)
    u = torch.rand(n, generator=g)
    cm = torch.from_numpy(cm)
    return Data(x=torch.from_numpy(synth.gaussian_embeddings(n, 128, seed=1)), edge_index=torch.from_numpy(ei).long(),
                y=torch.randint(0, C, (n,), generator=g), train_mask=u < 0.5, val_mask=(u >= 0.5) & (u < 0.7) & ~cm,
                test_mask=(u >= 0.7) & ~cm, central_mask=cm).to(dev)


def office_data(dev):
    og = np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz"))
    d = Data(x=torch.from_numpy(og["x"]), edge_index=torch.from_numpy(og["edge_index"]).long(), y=torch.from_numpy(og["y"]).long(),
             **{k: torch.from_numpy(og[k]) for k in ("train_mask", "val_mask", "test_mask", "central_mask")}).to(dev)
    d.train_mask[d.y == -1] = False
    return d.to_undirected_()


def case(name, data, C, hidden, a):
    dev = data.x.device
    plan = transfer._plan(data, True)
    y, tm, cm = plan.y, data.train_mask, data.central_mask
    tmt = tm & ~cm
    w_b, w_t = tm.float() / tm.sum(), tmt.float() / tmt.sum()
    yi = y[:, None]
    nll = lambda logp, w: -(logp.gather(1, yi).squeeze(1) * w).sum()
    torch_loss = lambda lb, lt, lth: (2 * nll(lb, w_b) + nll(lt, w_t) + nll(lth, w_t)) / 4 + F.kl_div(lth, lt, log_target=True, reduction="batchmean")
    fused_loss = lambda lb, lt, lth: ops.step2_loss(lb, lt, lth, y, plan.train_u8, plan.central_u8, 1.0)
    N = y.shape[0]
    tabs = [F.log_softmax(torch.randn(N, C, device=dev), dim=1).requires_grad_(True) for _ in range(3)]

    def fb(fn):
        def run():
            for t in tabs:
                t.grad = None
            fn(*tabs).backward()
        return run
    fb(fused_loss)(); fb(torch_loss)()
    diff = abs(float(fused_loss(*tabs).detach()) - float(torch_loss(*tabs).detach()))
    t_f, t_t = alternate(fb(fused_loss), fb(torch_loss), a.rounds, a.reps)

    def make(loss_fn):
        torch.manual_seed(0)
        m = KTGNN_no_complement(data.x.shape[1], C, 2, hidden, use_bn=True, dim_share=data.x.shape[1], dropout=0.5).to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-3)

        def train():
            m.train()
            opt.zero_grad()
            lb, lt, lth, _ = m(data)
            loss_fn(lb, lt, lth).backward()
            opt.step()
        return m, train
    m_new, train_new = make(fused_loss)
    m_old, train_old = make(torch_loss)
    counts = torch.empty(5, C, C, dtype=torch.int64, device=dev)

    def epoch_new():
        train_new()
        transfer._eval_dtc(data, m_new, plan, counts_out=counts)

    def host_f1(pred, mask):
        yy, pp = y[mask].cpu().numpy(), pred.cpu().numpy()
        return transfer.f1_from_counts(np.bincount(yy * C + pp, minlength=C * C).reshape(C, C))

    def score_on_host(lb, lt, lth):
        """what the two scoring functions hand to the host: six masked prediction arrays and their labels"""
        [host_f1(lp[mk].max(1)[1], mk) for lp, mk in ((lb, plan.bits[0]), (lth, plan.bits[1]), (lth, plan.bits[2]))]
        [host_f1(lp[plan.bits[2]].max(1)[1], plan.bits[2]) for lp in (lb, lt, lth)]

    def eval_old():
        m_old.eval()
        with torch.no_grad():
            return m_old(data)

    def epoch_old():
        train_old()
        lb, lt, lth, _ = eval_old()                              # test()
        eval_old()                                               # get_each_clf_res(): the same forward again
        score_on_host(lb, lt, lth)
    for _ in range(3):
        epoch_new(); epoch_old()
    torch.cuda.synchronize()
    e_new, e_old = alternate(epoch_new, epoch_old, a.rounds, max(a.reps // 2, 2))
    # where the composed loop's extra time goes: the second eval forward, host-side scoring (mask compaction + copies + counting), the loss
    from tools.sage_time import timed
    outs = eval_old()[:3]
    t_eval = timed(eval_old, a.reps)
    t_score = timed(lambda: score_on_host(*outs), a.reps)
    t_counts = timed(lambda: ops.step2_counts(outs, y, plan.sel, transfer._DTC_COMBOS, out=counts), a.reps)
    return {"tool": "transfer_time", "case": name, "nodes": N, "edges": int(data.edge_index.shape[1]), "classes": C, "hidden": hidden,
            "loss_fwd_bwd": {"fused_ms": round(t_f, 4), "torch_ops_ms": round(t_t, 4), "speedup": round(t_t / t_f, 3), "abs_diff": diff},
            "epoch": {"driver_ms": round(e_new, 4), "composed_ms": round(e_old, 4), "speedup": round(e_old / e_new, 3),
                      "parts": {"one_eval_forward_ms": round(t_eval, 4), "host_scoring_ms": round(t_score, 4),
                                "device_counts_ms": round(t_counts, 4), "loss_saving_ms": round(t_t - t_f, 4)}},
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--epoch-only", action="store_true", help="ten driver epochs on the C4-shaped graph (C = 2) and nothing else")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transfer_time needs an MI355X"
    dev = torch.device("cuda:0")
    if a.epoch_only:
        import types
        data = c4_data(a.nodes, a.edges, 2, dev)
        transfer.train_gnn(types.SimpleNamespace(dataset_name="c4"), transfer.pyg_dataset(data), data, repeat=1, num_epoch=10, gnn="KTGNN", seed=0,
                           hidden=64, verbose=False)
        torch.cuda.synchronize()
        return
    lines = []
    for C in (2, 31):
        lines.append(json.dumps(case(f"c4_C{C}", c4_data(a.nodes, a.edges, C, dev), C, 64, a)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(case("office_a2d", office_data(dev), 31, 64, a)))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
