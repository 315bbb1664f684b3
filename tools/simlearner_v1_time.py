"""Times the pair part of the v1 similarity learner (the cosine scorer Similar + BCE, forward and backward) and its Cartesian
evaluation, HIP pair passes (bridged_gnn_amd.simlearner_v1) against a torch-eager restatement of the reference's pair path
(models/models.py:124-130, :143-148: lin_self per call, biasatt on the gathered rows, CosineSimilarity, sigmoid; scripts.py:36-48
BCE; scripts.py:98-190 evaluation, chunked so that it fits) on the same GPU and the same tensors.  One JSON line per case:
  office_step    one training step's three 40 000-pair lists (src-src, tar-tar, src-tar), 2817 / 591 nodes, hidden 64
  twitter_step   the same on the Twitter stand-in's shape (581 / 20 230 nodes)
  twitter_eval   one evaluated epoch (eval_adv val + test) on the Twitter stand-in (synth.twitter_standin, hidden 64)
  twitter_main   a seeded main_adv run on the Twitter stand-in: 400 epochs, evaluation from 300, hidden 64 (wall time)
Usage: python tools/simlearner_v1_time.py [--case office_step,twitter_step,twitter_eval,twitter_main] [--reps 20] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time(fn, reps, warm=2):
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
    return ts


def _stats(ts):
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4), "reps": len(ts)}


def twitter_data(dev):
    from bridged_gnn_amd import bridge, synth
    from bridged_gnn_amd.data import Data
    from bridged_gnn_amd.simlearner_v1 import twitter_self_loops
    x, ei, y, mask = synth.twitter_standin()
    d = Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei), y=torch.from_numpy(y), central_mask=torch.from_numpy(mask))
    ds, dt, _, _ = bridge.dataset_conversion(d, seed=0)
    twitter_self_loops(ds)
    for d in (ds, dt):
        for k, v in list(vars(d).items()):
            if torch.is_tensor(v):
                setattr(d, k, v.to(dev))
    return ds, dt


def _eager_step(sim, hs, ht, lists):
    cs = torch.nn.CosineSimilarity(dim=1)
    (i1s, i2s, ys), (i1t, i2t, yt), (i1c, i2c, yc) = lists
    z = sim.lin_self(hs)
    l_s = F.binary_cross_entropy(torch.sigmoid(cs(z[i1s] + sim.biasatt(z[i1s]), z[i2s] + sim.biasatt(z[i2s]))), ys.float())
    z = sim.lin_self(ht)
    l_t = F.binary_cross_entropy(torch.sigmoid(cs(z[i1t] + sim.biasatt(z[i1t]), z[i2t] + sim.biasatt(z[i2t]))), yt.float())
    zs, zt = sim.lin_self(hs), sim.lin_self(ht)
    l_c = F.binary_cross_entropy(torch.sigmoid(cs(zs[i1c] + sim.biasatt(zs[i1c]), zt[i2c] + sim.biasatt(zt[i2c]))), yc.float())
    (l_s + l_t + l_c).backward()


def _hip_step(sim, hs, ht, lists):
    from bridged_gnn_amd.simlearner_v1 import cos_pair_losses
    qs, qt = sim.node_qhat(hs), sim.node_qhat(ht)
    sim.advance_bn(hs, ht)
    losses, _ = cos_pair_losses((qs, qt), ((0, 0), (1, 1), (0, 1)), lists)
    sum(losses).backward()


def run_step(case, reps):
    from bridged_gnn_amd.simlearner_v1 import Similar
    dev = torch.device("cuda:0")
    H, P = 64, 40000
    n_src, n_tar = {"office_step": (2817, 591), "twitter_step": (581, 20230)}[case]
    torch.manual_seed(0)
    hs = torch.randn(n_src, H, device=dev, requires_grad=True)
    ht = torch.randn(n_tar, H, device=dev, requires_grad=True)
    g = torch.Generator(device=dev).manual_seed(0)
    lists = []
    for a, b in ((n_src, n_src), (n_tar, n_tar), (n_src, n_tar)):
        i1 = torch.randint(0, a, (P,), device=dev, generator=g)
        i2 = torch.randint(0, b, (P,), device=dev, generator=g)
        lists.append((i1, i2, (i1 % 2 == i2 % 2)))
    sim = Similar(H, 2, train_dropout=False).to(dev).train()
    t_hip = _time(lambda: _hip_step(sim, hs, ht, lists), reps)
    t_eager = _time(lambda: _eager_step(sim, hs, ht, lists), reps)
    return {"case": case, "pairs": 3 * P, "hip": _stats(t_hip), "eager": _stats(t_eager),
            "speedup": round(t_eager[len(t_eager) // 2] / t_hip[len(t_hip) // 2], 2)}


def _eager_counts(sim, za, zb, r1, r2, ya, yb, chunk=1 << 21):
    """the reference's pair path on the Cartesian list r1 x r2, chunked: lin_self per node, biasatt on gathered rows, cosine, sigmoid"""
    ua, ub = sim.lin_self(za), sim.lin_self(zb)
    cs = torch.nn.CosineSimilarity(dim=1)
    tp = fp = fn = 0
    m1 = r1.shape[0]
    P = m1 * r2.shape[0]
    for s in range(0, P, chunk):
        p = torch.arange(s, min(P, s + chunk), device=za.device)
        i1, i2 = r1[p % m1], r2[p // m1]
        prob = torch.sigmoid(cs(ua[i1] + sim.biasatt(ua[i1]), ub[i2] + sim.biasatt(ub[i2])))
        pos, same = prob > 0.5, ya[i1] == yb[i2]
        tp += (pos & same).sum()
        fp += (pos & ~same).sum()
        fn += (~pos & same).sum()
    return tp, fp, fn


def _eager_epoch(model, ds, dt):
    sim = model.source_learner.sim_net
    with torch.no_grad():
        model.eval()
        zs = model.source_learner.backbone(ds.x, ds.edge_index)
        zt, _ = model.target_learner.encode(dt)
        for mode in ("val", "test"):
            for d, z in ((ds, zs), (dt, zt)):
                m2 = d.val_mask if mode == "val" else d.test_mask
                _eager_counts(sim, z, z, torch.nonzero(d.train_mask | d.val_mask | d.test_mask).reshape(-1),
                              torch.nonzero(m2).reshape(-1), d.y, d.y)
            if mode == "val":
                prods = ((ds.val_mask, dt.train_mask | dt.val_mask), (ds.train_mask, dt.val_mask))
            else:
                prods = ((ds.test_mask, dt.train_mask | dt.test_mask | dt.val_mask), (ds.train_mask | ds.val_mask, dt.test_mask))
            for ms, mt in prods:
                _eager_counts(sim, zs, zt, torch.nonzero(ms).reshape(-1), torch.nonzero(mt).reshape(-1), ds.y, dt.y)


def _epoch_pairs(ds, dt):
    n = 0
    for mode in ("val", "test"):
        for d in (ds, dt):
            m2 = d.val_mask if mode == "val" else d.test_mask
            n += int((d.train_mask | d.val_mask | d.test_mask).sum()) * int(m2.sum())
        if mode == "val":
            n += int(ds.val_mask.sum()) * int((dt.train_mask | dt.val_mask).sum()) + int(ds.train_mask.sum()) * int(dt.val_mask.sum())
        else:
            n += int(ds.test_mask.sum()) * int((dt.train_mask | dt.test_mask | dt.val_mask).sum()) \
                + int((ds.train_mask | ds.val_mask).sum()) * int(dt.test_mask.sum())
    return n


def run_eval(reps):
    from bridged_gnn_amd import simlearner_v1 as V1
    from bridged_gnn_amd.utils import set_random_seed
    dev = torch.device("cuda:0")
    ds, dt = twitter_data(dev)
    set_random_seed(0)
    model = V1.Adversarial_Learner(ds, dt, dim_hidden=64, norm_mode="None").to(dev)
    hip = lambda: (V1.eval_adv(ds, dt, model, mode="val"), V1.eval_adv(ds, dt, model, mode="test"))  # noqa: E731
    t_hip = _time(hip, reps)
    t_eager = _time(lambda: _eager_epoch(model, ds, dt), max(3, reps // 5), warm=1)
    pairs = _epoch_pairs(ds, dt)
    med = t_hip[len(t_hip) // 2]
    return {"case": "twitter_eval", "pairs": pairs, "hip": _stats(t_hip), "eager": _stats(t_eager),
            "speedup": round(t_eager[len(t_eager) // 2] / med, 2), "pair_tflops_hip_incl_encoders": round(256 * pairs / med / 1e9, 2)}


def run_main(out_dir):
    import types
    from bridged_gnn_amd import simlearner_v1 as V1
    dev = torch.device("cuda:0")
    ds, dt = twitter_data(dev)
    args = types.SimpleNamespace(dataset_name="twitter_standin")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    state, best = V1.main_adv(args, ds, dt, save=True, repeat=1, num_epoch=400, seed=0, hidden=64, norm_mode="None",
                              start_eval_epoch=300, eval_per_epoch=1, device=dev, ckpt_dir=out_dir, verbose=False)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ok = os.path.exists(os.path.join(out_dir, "model_AdvLearner_twitter_standin_best.ckpt"))
    return {"case": "twitter_main", "epochs": 400, "start_eval_epoch": 300, "wall_s": round(wall, 2), "best_epoch": best["epoch"],
            "best_val_cross_f1": round(float(best["val"][2]), 4), "checkpoint_written": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="office_step,twitter_step,twitter_eval")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="checkpoint directory of twitter_main (default: a temporary directory)")
    a = ap.parse_args()
    for case in a.case.split(","):
        if case == "twitter_eval":
            r = run_eval(a.reps)
        elif case == "twitter_main":
            import tempfile
            out = a.out or tempfile.mkdtemp()
            os.makedirs(out, exist_ok=True)
            r = run_main(out)
        else:
            r = run_step(case, a.reps)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
