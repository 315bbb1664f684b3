"""Times the pair part of the v2 similarity learner's training (Similar_v2(mode='mlp') + BCE, forward and backward) and its
evaluation, HIP pair passes (bridged_gnn_amd.simlearner) against a torch-eager restatement of the reference's pair path
(models/models.py:949-951: cat(z1[idx1], z2[idx2]) -> BN -> Linear -> BN -> ReLU -> Linear -> sigmoid, scripts.py:39-50 BCE) on
the same GPU and the same tensors.  One JSON line per case on stdout:
  office_step   one training step's three 40 000-pair lists (src-src, tar-tar, src-tar), 2817 / 591 nodes, hidden 128
  office_eval   one evaluated epoch's six 99 262-pair balanced lists (no grad, running statistics)
  scaled_step   200 000 source x 50 000 target nodes, hidden 128, three lists of 4 000 000 pairs (sample_size 4e6)
  all_office    eval_mode='all': the four products of one office `test` evaluation (1.59 M + 71 k + 333 k + 270 k pairs)
  all_scaled    one product of 100 000 x 20 000 rows (2e9 pairs) drawn from 200 000 / 50 000-node tables
The `all` cases time three routes to the same confusion counts: the product count pass (ops.pair_mlp_count, no pair list), the
materialised lists through the list pass (ops.pair_mlp_eval on chunks of 2^22 pairs, index construction included) and torch
eager in the reference's gathered form (cat(z1[idx1], z2[idx2]) -> lin_self on chunks of 2^20 pairs).  On all_scaled the two
list routes run on the first 10 000 x 20 000 rows and their times are scaled by 10 (`extrapolated`: the routes are linear in m1).
Usage: python tools/simlearner_time.py [--case office_step,office_eval,scaled_step,all_office,all_scaled] [--reps 20]"""
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


def run_all(case, reps):
    from bridged_gnn_amd import ops
    from bridged_gnn_amd.simlearner import Similar_v2
    dev = torch.device("cuda:0")
    H = 128
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    if case == "all_office":
        n_src, n_tar = 2817, 591
        # (table 1, table 2, m1, m2) of the office A->D `test` evaluation: source, target, and the two cross products
        prods = [(n_src, n_src, 2817, 563), (n_tar, n_tar, 591, 120), (n_src, n_tar, 563, 591), (n_src, n_tar, 2254, 120)]
        frac = 1
    else:
        n_src, n_tar = 200000, 50000
        prods = [(n_src, n_tar, 100000, 20000)]
        frac = 10
    zs, zt = torch.randn(n_src, H, device=dev), torch.randn(n_tar, H, device=dev)
    tab = {n_src: zs, n_tar: zt}
    lab = {n: torch.randint(0, 31, (n,), device=dev, generator=g) for n in (n_src, n_tar)}
    sim = Similar_v2(H, 31, train_dropout=False).to(dev).eval()
    ref = nn.Sequential(nn.BatchNorm1d(2 * H), nn.Linear(2 * H, 128), nn.BatchNorm1d(128), nn.ReLU(), nn.Linear(128, 1)).to(dev)
    ref.load_state_dict(sim.lin_self.state_dict())
    ref.eval()
    rows = [(a, b, torch.randperm(a, device=dev, generator=g)[:m1].contiguous(), torch.randperm(b, device=dev, generator=g)[:m2].contiguous())
            for a, b, m1, m2 in prods]

    def product():
        for a, b, r1, r2 in rows:
            sim.pair_counts(tab[a], tab[b], r1, r2, lab[a], lab[b])

    def chunks(r1, r2, size):
        per = max(1, size // r2.shape[0])
        for i0 in range(0, r1.shape[0] // frac, per):
            part = r1[i0:min(i0 + per, r1.shape[0] // frac)]
            yield part.repeat_interleave(r2.shape[0]), r2.repeat(part.shape[0])

    def lists():
        with torch.no_grad():
            for a, b, r1, r2 in rows:
                A, B, s2, t2, w2, b2 = sim._eval_tables(tab[a], tab[b])
                for i1, i2 in chunks(r1, r2, 1 << 22):
                    ops.pair_mlp_eval(A, B, i1, i2, s2, t2, w2, b2, (lab[a][i1] == lab[b][i2]).to(torch.uint8))

    def eager():
        with torch.no_grad():
            for a, b, r1, r2 in rows:
                for i1, i2 in chunks(r1, r2, 1 << 20):
                    p = torch.sigmoid(ref(torch.cat((tab[a][i1], tab[b][i2]), 1)).squeeze(-1))
                    pred, y = p > 0.5, lab[a][i1] == lab[b][i2]
                    (pred & y).sum(), (pred & ~y).sum(), (~pred & y).sum(), (~pred & ~y).sum()
    t_prod = _time(product, reps)
    t_list = _time(lists, max(2, reps // 4), warm=1) * frac
    t_eager = _time(eager, max(2, reps // 4), warm=1) * frac
    pairs = sum(m1 * m2 for _, _, m1, m2 in prods)
    return {"case": case, "pairs": pairs, "products": [[m1, m2] for _, _, m1, m2 in prods], "hidden": H,
            "product_count_ms": round(t_prod, 4), "list_pass_ms": round(t_list, 4), "torch_eager_ms": round(t_eager, 4),
            "extrapolated": frac != 1, "pair_columns_per_s": round(pairs * 128 / (t_prod * 1e-3), 1),
            "speedup_vs_list": round(t_list / t_prod, 2), "speedup_vs_eager": round(t_eager / t_prod, 2)}


def run(case, reps):
    if case.startswith("all_"):
        return run_all(case, reps)
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
