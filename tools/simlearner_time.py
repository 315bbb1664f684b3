"""Times the pair part of the v2 similarity learner's training (Similar_v2(mode='mlp') + BCE, forward and backward) and its
evaluation, HIP pair passes (bridged_gnn_amd.simlearner) against a torch-eager restatement of the reference's pair path
(models/models.py:949-951: cat(z1[idx1], z2[idx2]) -> BN -> Linear -> BN -> ReLU -> Linear -> sigmoid, scripts.py:39-50 BCE) on
the same GPU and the same tensors.  One JSON line per case on stdout:
  office_step   one training step's three 40 000-pair lists (src-src, tar-tar, src-tar), 2817 / 591 nodes, hidden 128
  office_eval   one evaluated epoch's six 99 262-pair balanced lists (no grad, running statistics)
  scaled_step   200 000 source x 50 000 target nodes, hidden 128, three lists of 4 000 000 pairs (sample_size 4e6)
Usage: python tools/simlearner_time.py [--case office_step,office_eval,scaled_step] [--reps 20]"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def _lists(n_src, n_tar, P, n_lists, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    shapes = [(n_src, n_src), (n_tar, n_tar), (n_src, n_tar), (n_src, n_src), (n_tar, n_tar), (n_src, n_tar)][:n_lists]
    out = []
    for a, b in shapes:
        i1 = torch.randint(0, a, (P,), device=dev, generator=g)
        i2 = torch.randint(0, b, (P,), device=dev, generator=g)
        out.append((a, b, i1, i2, (i1 % 31 == i2 % 31).to(torch.uint8)))
    return out


def run(case, reps):
    from bridged_gnn_amd.simlearner import Similar_v2
    dev = torch.device("cuda:0")
    H = 128
    n_src, n_tar, P, n_lists = {"office_step": (2817, 591, 40000, 3), "office_eval": (2817, 591, 99262, 6),
                                "scaled_step": (200000, 50000, 4000000, 3)}[case]
    train = case.endswith("step")
    torch.manual_seed(0)
    zs = torch.randn(n_src, H, device=dev, requires_grad=train)
    zt = torch.randn(n_tar, H, device=dev, requires_grad=train)
    tab = {n_src: zs, n_tar: zt}
    lists = _lists(n_src, n_tar, P, n_lists, dev)
    sim = Similar_v2(H, 31, train_dropout=False).to(dev)
    ref = nn.Sequential(nn.BatchNorm1d(2 * H), nn.Linear(2 * H, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Linear(128, 1)).to(dev)
    ref.load_state_dict(sim.lin_self.state_dict())
    sim.train(train)
    ref.train(train)

    def hip():
        if train:
            loss = 0
            for a, b, i1, i2, y in lists:
                loss = loss + sim.pair_bce(tab[a], tab[b], i1, i2, y)[1]
            loss.backward()
        else:
            for a, b, i1, i2, y in lists:
                sim.pair_scores(tab[a], tab[b], i1, i2, y)

    def eager():
        if train:
            loss = 0
            for a, b, i1, i2, y in lists:
                p = torch.sigmoid(ref(torch.cat((tab[a][i1], tab[b][i2]), 1)).squeeze(-1))
                loss = loss + F.binary_cross_entropy(p, y.float())
                (p > 0.5).long()
            loss.backward()
        else:
            with torch.no_grad():
                for a, b, i1, i2, y in lists:
                    p = torch.sigmoid(ref(torch.cat((tab[a][i1], tab[b][i2]), 1)).squeeze(-1))
                    (p > 0.5).long()
    t_hip = _time(hip, reps)
    t_eager = _time(eager, reps)
    return {"case": case, "pairs_per_list": P, "lists": n_lists, "nodes": [n_src, n_tar], "hidden": H,
            "hip_ms": round(t_hip, 4), "torch_eager_ms": round(t_eager, 4), "speedup": round(t_eager / t_hip, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="office_step,office_eval,scaled_step")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    for c in args.case.split(","):
        print(json.dumps(run(c, args.reps)), flush=True)


if __name__ == "__main__":
    main()
