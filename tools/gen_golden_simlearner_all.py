"""Generates tests/golden/simlearner_all_office_a2d.npz from the REFERENCE's own Cartesian evaluation of the v2 similarity
learner: eval_adv_v2(..., eval_mode='all') (scripts.py:315-426) on a seeded Adversarial_Learner_v2 (backbone='mlp',
sim_mode='mlp', models/models.py:852-1142) after warm-up steps of its own training (train_adv_few_shot, scripts.py:28-94), run in
fp64 on one CPU thread under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_simlearner_all.py [--out DIR] [--steps N]     (deterministic: fixed seeds, one CPU thread)

Inputs: tests/golden/office_a2d_graph.npz -> the reference's dataset_conversion(seed=0) (2817 source / 591 target nodes, 31
classes, 256 features); norm_mode 'None', max_class_num 10, sample_size 40000 (run.sh #2).  dim_hidden is 64 (the reference's
default) and not run.sh's 128, so that the whole state_dict fits a fixture of a few hundred KB; at that width the reference's
materialised lists ([m1 * m2, 2H] gathered rows, the largest product has 1.6 M pairs) fit in memory in fp64, so the evaluation
is the reference's own, unchunked.  The process-local patches of gen_golden_simlearner.py apply (F.dropout is the identity,
F.binary_cross_entropy casts its target), and the model's get_probs_within_domain / get_probs_cross_domain are wrapped to
record the lists and probabilities they are called with.

One warm-up step is the default: it moves the running statistics of both BatchNorms off their initial values while the scorer
still predicts both classes on the source product (TP, FP, FN and TN all in the ten thousands).  From the second step on this
schedule's scorer predicts "different" for every evaluated pair (2, 3 and 5 steps were tried), which would leave TP = FP = 0 in
every product and the near band empty.

After the warm-up every floating-point tensor of the model is rounded to fp32 (model.float().double()) BEFORE the
evaluation, so the stored fp32 state_dict is exactly the model that was evaluated.

Contents:
  hidden, steps                        dim_hidden and the number of warm-up training steps
  mask/{src,tar}_{train,val,test}      the split masks
  keys (str), state/{key}              the evaluated model's state_dict (fp32 / int64), keys in the model's order
  eval/{val,test}_{f1,acc} [5]         eval_adv_v2(eval_mode='all'): pair_src, clf_src, pair_tar, clf_tar, pair_cross
  prod/{val,test}/{src,tar,cross1,cross2}/rows1, rows2   sorted distinct node ids of each side of the product, as they appear
                                       in the reference's list (cross1 / cross2: the two concatenated products of
                                       eval_cross_domain_v2, in its order)
  prod/.../counts [4]                  TP, FP, FN, TN of the product at p > 0.5 (fp64 probabilities)
  prod/.../near                        pairs of the product with |logit| < 1e-4 (logit = log p - log(1 - p) in fp64): the pairs
                                       an fp32 evaluation may count on the other side
The generator asserts that every product's near band holds at most 0.1 % of its pairs.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HIDDEN = 64
NEAR = 1e-4
NEAR_CAP = 1e-3


def product_stats(p, y, i1, i2):
    p, y = p.reshape(-1).double(), y.reshape(-1).bool()
    pos = p > 0.5
    counts = np.array([(pos & y).sum().item(), (pos & ~y).sum().item(), (~pos & y).sum().item(), (~pos & ~y).sum().item()], np.int64)
    logit = torch.log(p) - torch.log1p(-p)
    near = int((logit.abs() < NEAR).sum().item())
    r1, r2 = torch.unique(i1).numpy().astype(np.int64), torch.unique(i2).numpy().astype(np.int64)
    assert r1.size * r2.size == p.numel(), "the reference's list is not a full product"
    assert near <= NEAR_CAP * p.numel(), f"near band {near} of {p.numel()} pairs exceeds the cap: change --steps"
    return {"rows1": r1, "rows2": r2, "counts": counts, "near": np.array(near, np.int64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--steps", type=int, default=1)
    args = ap.parse_args()
    torch.set_num_threads(1)
    from oracle.ref_import import import_reference, REF_CODE
    import_reference()
    cwd = os.getcwd()
    os.chdir(REF_CODE)
    try:
        import models as M
        import scripts as S
        import utils as RU
        from torch_geometric.data import Data
    finally:
        os.chdir(cwd)

    g = np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz"))
    data = Data(x=torch.from_numpy(g["x"]), edge_index=torch.from_numpy(g["edge_index"]).long(), y=torch.from_numpy(g["y"]),
                train_mask=torch.from_numpy(g["train_mask"]), val_mask=torch.from_numpy(g["val_mask"]),
                test_mask=torch.from_numpy(g["test_mask"]), central_mask=torch.from_numpy(g["central_mask"]))
    data_src, data_tar, _, _ = RU.dataset_conversion(data, seed=0)
    out = {"hidden": np.array(HIDDEN, np.int64), "steps": np.array(args.steps, np.int64)}
    for dn, d in (("src", data_src), ("tar", data_tar)):
        for m in ("train", "val", "test"):
            out[f"mask/{dn}_{m}"] = getattr(d, m + "_mask").numpy().astype(bool)

    RU.set_random_seed(0)
    model = M.Adversarial_Learner_v2(data_src, data_tar, dim_hidden=HIDDEN, num_layer=2, use_norm=True, source_clf=True,
                                     norm_mode="None", norm_scale=1., sim_mode="mlp", backbone="mlp").double()
    for d in (data_src, data_tar):
        d.x = d.x.double()
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x
    bce0 = F.binary_cross_entropy
    F.binary_cross_entropy = lambda inp, target, *a, **k: bce0(inp, target.to(inp.dtype), *a, **k)

    lr, b1, b2 = 1e-3, 0.5, 0.999
    opt = torch.optim.Adam([{"params": model.source_learner.parameters(), "lr": 1e-2, "weight_decay": 5e-3},
                            {"params": model.target_learner.parameters(), "lr": lr, "betas": (b1, b2)}])
    opt_d = torch.optim.Adam(model.discriminator.parameters(), lr=lr, betas=(b1, b2))
    enu = (M.Pair_Enumerator(data_src, mode="train"), M.Pair_Enumerator(data_tar, mode="train"),
           M.Pair_Enumerator_cross(data_src, data_tar, mode="train"))
    np.random.seed(0)
    for step in range(1, 1 + args.steps):
        r = S.train_adv_few_shot(step, data_src, data_tar, model, opt, opt_d, metric="f1", pair_enumerator_src_train=enu[0],
                                 pair_enumerator_tar_train=enu[1], pair_enumerator_cross_train=enu[2], max_class_num=10,
                                 sample_size=40000, use_clf=True)
        print("step", step, "loss_sim", r[0], "f1", r[1])

    model = model.float().double()                 # the evaluated model is exactly its fp32 state_dict
    sd = model.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        out[f"state/{k}"] = v.numpy().astype(np.float32) if v.is_floating_point() else v.numpy().astype(np.int64)
        if v.is_floating_point():
            assert np.array_equal(out[f"state/{k}"].astype(np.float64), v.numpy()), k

    calls = []
    within0, cross0 = model.get_probs_within_domain, model.get_probs_cross_domain

    def within(data_, idx1, idx2, domain="target"):
        r = within0(data_, idx1, idx2, domain=domain)
        calls.append(("src" if domain == "source" else "tar", r[0].detach(), data_.y[idx1] == data_.y[idx2], idx1, idx2))
        return r

    def cross(data_s, data_t, idx1, idx2, return_representation=False):
        r = cross0(data_s, data_t, idx1, idx2, return_representation=return_representation)
        calls.append(("cross", r[0].detach(), data_s.y[idx1] == data_t.y[idx2], idx1, idx2))
        return r
    model.get_probs_within_domain, model.get_probs_cross_domain = within, cross

    for split in ("val", "test"):
        for metric in ("f1", "acc"):
            calls.clear()
            ev = S.eval_adv_v2(data_src, data_tar, model, split=split, metric=metric, enu_list=(None, None, None), eval_mode="all")
            out[f"eval/{split}_{metric}"] = np.array(ev, np.float64)
            print(split, metric, ev)
            if metric != "f1":
                continue
            for name, p, y, i1, i2 in calls:
                if name != "cross":
                    parts = [(name, slice(None))]
                else:
                    # eval_cross_domain_v2 concatenates two products; the first one's size from its own masks (scripts.py:317-318)
                    m_s = data_src.val_mask if split == "val" else data_src.test_mask
                    m_t = (data_tar.train_mask + data_tar.val_mask if split == "val"
                           else data_tar.train_mask + data_tar.test_mask + data_tar.val_mask)
                    n1 = int(m_s.sum()) * int(m_t.sum())
                    parts = [("cross1", slice(0, n1)), ("cross2", slice(n1, None))]
                for pn, sl in parts:
                    st = product_stats(p.reshape(-1)[sl], y[sl], i1[sl], i2[sl])
                    print(" ", split, pn, "pairs", st["rows1"].size * st["rows2"].size, "counts", st["counts"], "near", st["near"])
                    for k, v in st.items():
                        out[f"prod/{split}/{pn}/{k}"] = v
    path = os.path.join(args.out, "simlearner_all_office_a2d.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
