"""Generates tests/golden/simlearner_v1_office_a2d.npz from the REFERENCE's own v1 similarity learner (Adversarial_Learner with
GraphSAGE encoders and the cosine scorer Similar, models/models.py:67-169, :220-263, :576-622, :704-750, :815-844), its training
step (train_adv_few_shot, scripts.py:28-94) and its evaluation (eval_adv, scripts.py:98-196), run in fp64 on one CPU thread
under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_simlearner_v1.py [--out DIR]     (deterministic: fixed seeds, one CPU thread)

Inputs: tests/golden/office_a2d_graph.npz -> the reference's dataset_conversion(seed=0) (2817 source / 591 target nodes, 31
classes, 256 features); hidden 64, norm_mode 'None', max_class_num 2, sample_size 40000 (main_adv's v1 settings).  Two variants:
  a/   the graphs as given
  b/   twitter-style: the source edges replaced by self loops (main_bridged_graph.py:335-340) and y % 2 in both domains (the
       binary classifier f1 of scripts.py:177)
Process-local patches: F.dropout is the identity (tests switch dropout off the same way), F.binary_cross_entropy casts its target
to the input's dtype, the enumerators / optimizers / f1_score are wrapped to record what they draw, step with and count.

Contents (per variant prefix a/ or b/):
  keys (str), shapes                  state_dict key and shape list of Adversarial_Learner(...) in its own order  (a/ only)
  init_sum/{key}                      (sum, sum of squares) in fp64 of the seeded model's fp32 parameters (torch.manual_seed(0))
  s1/idx/{src,tar,cross}              step 1's (idx1, idx2) lists [2, 40000] after np.random.seed(0) (a/; b/: s1/digest/..., the
                                      sha256 of the two int64 lists)
  s1/loss                             step 1's [bce_src, bce_tar, bce_cross, loss_recons, loss_g, nll_src, nll_tar, loss_sim]
  s1/grad/{key}, s1/dgrad/{key}       gradients after loss_sim.backward() / loss_d.backward(): fp32 roundings of the fp64 values,
                                      full for a/'s sim_net gradients and tensors of <= 4096 entries, else `sub` (fp32) at the flat indices
                                      `s1/grad_idx/{key}` (2048 seeded) and `max` = max |g| of the whole tensor
  step/tuple [3, 8]                   per step: loss_sim, f1 src / tar / cross, loss_d, loss_ae, loss_g, loss_recons
  s3/param/{key}                      parameters after step 3: full (<= 4096 entries) or sub (same indices as the gradients), plus max
  s3/bn/{key}                         BatchNorm running stats and num_batches_tracked after step 3
  {init,s3}/eval [10]                 eval_adv val then test (pair_src, clf_src, pair_tar, clf_tar, pair_cross)
  {init,s3}/counts [2, 3, 3]          TP, FP, FN of the three pair f1s (src, tar, cross) for val and test
  {init,s3}/border [2, 3]             per f1 the number of pairs with fp64 |cos| < 1e-5 (where fp32 may decide otherwise)
Plus ckpt/{twitter,hamilton,howard}/{keys,shapes,nbt} of the shipped v1 checkpoints (key / shape lists, num_batches_tracked).
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FULL_MAX = 4096
N_SUB = 2048
BORDER = 1e-5
REC = {"bce": [], "nll": [], "f1": []}      # what the patched losses and f1_score record
CKPTS = (("twitter", "twitter_unrelational"), ("hamilton", "fb_hamilton2caltech"), ("howard", "fb_howard2simmons"))


def digest(a, b):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(np.asarray(a, np.int64)).tobytes())
    h.update(np.ascontiguousarray(np.asarray(b, np.int64)).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def sub_index(key, numel):
    seed = int.from_bytes(hashlib.sha256(key.encode()).digest()[:4], "little")
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(numel, N_SUB, replace=False)).astype(np.int64)


def put_tensor(out, prefix, key, t, vp):
    """full for tensors of <= FULL_MAX entries and for variant a's step-1 sim_net gradients, else sub-sampled (size limit)"""
    v = t.detach().double().reshape(-1).numpy()
    if v.size <= FULL_MAX or (".sim_net." in key and vp == "a/" and prefix == "s1/grad"):
        out[f"{vp}{prefix}/{key}"] = v.reshape(tuple(t.shape)).astype(np.float32)
        return
    idx = sub_index(key, v.size)
    out[f"{vp}s1/grad_idx/{key}"] = idx
    out[f"{vp}{prefix}/{key}/sub"] = v[idx].astype(np.float32)
    out[f"{vp}{prefix}/{key}/max"] = np.array(np.abs(v).max())


def qhat(model, z):
    sim = model.source_learner.sim_net
    u = sim.lin_self(z)
    q = u + sim.biasatt(u)
    return q / q.norm(dim=1, keepdim=True).clamp_min(1e-8)


def border_counts(model, ds, dt, mode):
    """fp64 |cos| < BORDER pairs of the three Cartesian evaluations (scripts.py:98-190) in eval mode"""
    with torch.no_grad():
        model.eval()
        zs = model.source_learner.backbone(ds.x, ds.edge_index)
        zt, _ = model.target_learner.encode(dt)
        qs, qt = qhat(model, zs), qhat(model, zt)

        def n(qa, qb, ma, mb):
            c = qa[torch.where(ma)[0]] @ qb[torch.where(mb)[0]].t()
            return int((c.abs() < BORDER).sum().item())
        res = []
        for d, q in ((ds, qs), (dt, qt)):
            res.append(n(q, q, d.train_mask | d.val_mask | d.test_mask, d.val_mask if mode == "val" else d.test_mask))
        if mode == "val":
            res.append(n(qs, qt, ds.val_mask, dt.train_mask | dt.val_mask) + n(qs, qt, ds.train_mask, dt.val_mask))
        else:
            res.append(n(qs, qt, ds.test_mask, dt.train_mask | dt.test_mask | dt.val_mask)
                       + n(qs, qt, ds.train_mask | ds.val_mask, dt.test_mask))
    return res


def run_variant(M, S, RU, data_src, data_tar, vp, out, with_keys):
    RU.set_random_seed(0)
    model = M.Adversarial_Learner(data_src, data_tar, dim_hidden=64, num_layer=2, source_clf=True, norm_mode="None", norm_scale=1.)
    sd = model.state_dict()
    if with_keys:
        out["keys"] = np.array(list(sd.keys()))
        out["shapes"] = np.array([list(v.shape) + [-1] * (2 - v.dim()) for v in sd.values()], np.int64)
    for k, v in model.named_parameters():
        vd = v.detach().double()
        out[f"{vp}init_sum/{k}"] = np.array([vd.sum().item(), vd.square().sum().item()])
    model = model.double()
    for d in (data_src, data_tar):
        d.x = d.x.double()

    rec = REC
    f1_0 = S.f1_score

    def f1(y_true, y_pred, *a, **k):
        yt, yp = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
        rec["f1"].append([int(((yp == 1) & (yt == 1)).sum()), int(((yp == 1) & (yt == 0)).sum()), int(((yp == 0) & (yt == 1)).sum())])
        return f1_0(y_true, y_pred, *a, **k)
    S.f1_score = f1

    def eval_both(tag):
        res, counts = [], []
        for mode in ("val", "test"):
            rec["f1"].clear()
            res += list(S.eval_adv(data_src, data_tar, model, mode=mode))
            counts.append([rec["f1"][0], rec["f1"][2], rec["f1"][4]])      # pair f1s: src, tar, cross (clf at 1, 3)
        out[f"{vp}{tag}/eval"] = np.array(res, np.float64)
        out[f"{vp}{tag}/counts"] = np.array(counts, np.int64)
        out[f"{vp}{tag}/border"] = np.array([border_counts(model, data_src, data_tar, m) for m in ("val", "test")], np.int64)
    eval_both("init")

    lr, b1, b2 = 1e-3, 0.5, 0.999
    opt = torch.optim.Adam([{"params": model.source_learner.parameters(), "lr": 1e-2, "weight_decay": 5e-3},
                            {"params": model.target_learner.parameters(), "lr": lr, "betas": (b1, b2)}])
    opt_d = torch.optim.Adam(model.discriminator.parameters(), lr=lr, betas=(b1, b2))
    names = {id(p): k for k, p in model.named_parameters()}
    state = {"step": 0}

    def wrap_step(o, prefix):
        real = o.step

        def step(*a, **k):
            if state["step"] == 1:
                for grp in o.param_groups:
                    for p in grp["params"]:
                        put_tensor(out, prefix, names[id(p)], p.grad, vp=vp)
            return real(*a, **k)
        o.step = step
    wrap_step(opt, "s1/grad")
    wrap_step(opt_d, "s1/dgrad")

    enu = (M.Pair_Enumerator(data_src, mode="train"), M.Pair_Enumerator(data_tar, mode="train"),
           M.Pair_Enumerator_cross(data_src, data_tar, mode="train"))
    for name, e in zip(("src", "tar", "cross"), enu):
        real = e.sampling

        def samp(*a, _real=real, _name=name, **k):
            i1, i2 = _real(*a, **k)
            if state["step"] == 1 and vp == "a/":
                out[f"{vp}s1/idx/{_name}"] = np.stack((i1.numpy(), i2.numpy())).astype(np.int16)
            elif state["step"] == 1:
                out[f"{vp}s1/digest/{_name}"] = digest(i1.numpy(), i2.numpy())
            return i1, i2
        e.sampling = samp

    np.random.seed(0)
    tuples = []
    for step in range(1, 4):
        state["step"] = step
        rec["bce"].clear()
        rec["nll"].clear()
        r = S.train_adv_few_shot(step, data_src, data_tar, model, opt, opt_d, metric="f1", pair_enumerator_src_train=enu[0],
                                 pair_enumerator_tar_train=enu[1], pair_enumerator_cross_train=enu[2], max_class_num=2,
                                 sample_size=40000, use_clf=True)
        loss_sim, (fs, ft, fc), loss_d, loss_ae, loss_g, loss_recons = r
        tuples.append([loss_sim, fs, ft, fc, loss_d, loss_ae, loss_g, loss_recons])
        if step == 1:
            out[f"{vp}s1/loss"] = np.array(rec["bce"][:3] + [rec["mse"], rec["bce"][3]] + rec["nll"][:2] + [loss_sim])
    out[f"{vp}step/tuple"] = np.array(tuples)
    for k, p in model.named_parameters():
        put_tensor(out, "s3/param", k, p, vp=vp)
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"{vp}s3/bn/{k}"] = v.double().numpy() if v.is_floating_point() else v.numpy()
    eval_both("s3")
    S.f1_score = f1_0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    from oracle.ref_import import import_reference, REF_CODE, REF_ROOT
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

    F.dropout = lambda x, p=0.5, training=True, inplace=False: x
    bce0, nll0, mse0 = F.binary_cross_entropy, F.nll_loss, F.mse_loss

    def bce(inp, target, *a, **k):
        r = bce0(inp, target.to(inp.dtype), *a, **k)
        REC["bce"].append(r.item())
        return r

    def nll(*a, **k):
        r = nll0(*a, **k)
        REC["nll"].append(r.item())
        return r

    def mse(*a, **k):
        r = mse0(*a, **k)
        REC["mse"] = r.item()
        return r
    F.binary_cross_entropy, F.nll_loss, F.mse_loss = bce, nll, mse

    out = {}
    g = np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz"))
    for vp in ("a/", "b/"):
        data = Data(x=torch.from_numpy(g["x"]), edge_index=torch.from_numpy(g["edge_index"]).long(), y=torch.from_numpy(g["y"]),
                    train_mask=torch.from_numpy(g["train_mask"]), val_mask=torch.from_numpy(g["val_mask"]),
                    test_mask=torch.from_numpy(g["test_mask"]), central_mask=torch.from_numpy(g["central_mask"]))
        data_src, data_tar, _, _ = RU.dataset_conversion(data, seed=0)
        if vp == "b/":
            n = data_src.num_nodes
            data_src.edge_index = torch.stack([torch.arange(n) for _ in range(2)], dim=0)
            data_src.y = data_src.y % 2
            data_tar.y = data_tar.y % 2
        run_variant(M, S, RU, data_src, data_tar, vp, out, vp == "a/")

    for tag, name in CKPTS:
        sd = torch.load(os.path.join(REF_ROOT, "ckpt", f"model_AdvLearner_{name}_best.ckpt"), map_location="cpu")
        out[f"ckpt/{tag}/keys"] = np.array(list(sd.keys()))
        out[f"ckpt/{tag}/shapes"] = np.array([list(v.shape) + [-1] * (2 - v.dim()) for v in sd.values()], np.int64)
        out[f"ckpt/{tag}/nbt"] = np.array([int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")], np.int64)
    path = os.path.join(args.out, "simlearner_v1_office_a2d.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for vp in ("a/", "b/"):
        print(vp, "tuples", out[f"{vp}step/tuple"], "init eval", out[f"{vp}init/eval"], "s3 eval", out[f"{vp}s3/eval"],
              "border", out[f"{vp}init/border"].tolist(), out[f"{vp}s3/border"].tolist())


if __name__ == "__main__":
    main()
