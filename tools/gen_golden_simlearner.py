"""Generates tests/golden/simlearner_office_a2d.npz from the REFERENCE's own v2 similarity learner (Adversarial_Learner_v2 with
backbone='mlp', sim_mode='mlp', models/models.py:852-1142) and its training step (train_adv_few_shot, scripts.py:28-94) and
evaluation (eval_adv_v2, scripts.py:313-429), run in fp64 on one CPU thread under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_simlearner.py [--out DIR]     (deterministic: fixed seeds, one CPU thread)

Inputs: tests/golden/office_a2d_graph.npz -> the reference's dataset_conversion(seed=0) (2817 source / 591 target nodes, 31
classes, 256 features); hidden 128, norm_mode 'None', max_class_num 10, sample_size 40000 (run.sh #2).  Three process-local
patches: F.dropout is the identity (tests switch dropout off the same way), F.binary_cross_entropy casts its target to the
input's dtype (the reference's `.float()` labels meet fp64 probabilities), and the enumerators / optimizers are wrapped to
record what they draw and the gradients they step with.

Contents:
  mask/{src,tar}_{train,val,test}   the split masks
  keys (str), shapes                  state_dict key and shape list of Adversarial_Learner_v2(...) in its own order
  init_sum/{key}                      (sum, sum of squares) in fp64 of the seeded model's fp32 parameters (torch.manual_seed(0))
  s1/idx/{src,tar,cross}              step 1's (idx1, idx2) lists [2, 40000] after np.random.seed(0)
  eval/digest                         sha256 of the six eval lists of the epoch after step 3 (val src/tar/cross, test ...)
  s1/loss                             step 1's [bce_src, bce_tar, bce_cross, loss_recons, loss_g, nll_src, nll_tar, loss_sim]
  s1/grad/{key}, s1/dgrad/{key}       gradients after loss_sim.backward() / loss_d.backward(): fp32 roundings of the fp64 values, full for sim_net
                                      and tensors of <= 4096 entries, else `sub` = values at the flat indices `s1/grad_idx/{key}` (2048 seeded) and
                                      `max` = max |g| of the whole tensor
  step/tuple [3, 8]                   per step: loss_sim, f1 src / tar / cross, loss_d, loss_ae, loss_g, loss_recons
  s3/param/{key}                      parameters after step 3: full or sub (same indices as the gradients), plus max
  s3/bn/{key}                         BatchNorm running stats and num_batches_tracked after step 3
  s3/eval [10]                        eval_adv_v2 val then test after step 3 (pair_src, clf_src, pair_tar, clf_tar, pair_cross)
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


def digest(a, b):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(np.asarray(a, np.int64)).tobytes())
    h.update(np.ascontiguousarray(np.asarray(b, np.int64)).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def sub_index(key, numel):
    seed = int.from_bytes(hashlib.sha256(key.encode()).digest()[:4], "little")
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(numel, N_SUB, replace=False)).astype(np.int64)


def put_tensor(out, prefix, key, t, with_idx):
    v = t.detach().double().reshape(-1).numpy()
    if v.size <= FULL_MAX or ".sim_net." in key:
        out[f"{prefix}/{key}"] = v.reshape(tuple(t.shape)).astype(np.float32)
        return
    idx = sub_index(key, v.size)
    if with_idx:
        out[f"s1/grad_idx/{key}"] = idx
    out[f"{prefix}/{key}/sub"] = v[idx]
    out[f"{prefix}/{key}/max"] = np.array(np.abs(v).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
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
    out = {}
    for dn, d in (("src", data_src), ("tar", data_tar)):
        for m in ("train", "val", "test"):
            out[f"mask/{dn}_{m}"] = getattr(d, m + "_mask").numpy().astype(bool)

    RU.set_random_seed(0)
    model = M.Adversarial_Learner_v2(data_src, data_tar, dim_hidden=128, num_layer=2, use_norm=True, source_clf=True, norm_mode="None",
                                     norm_scale=1., sim_mode="mlp", backbone="mlp")
    sd = model.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([list(v.shape) + [-1] * (2 - v.dim()) for v in sd.values()], np.int64)
    for k, v in model.named_parameters():
        vd = v.detach().double()
        out[f"init_sum/{k}"] = np.array([vd.sum().item(), vd.square().sum().item()])

    model = model.double()
    for d in (data_src, data_tar):
        d.x = d.x.double()
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x
    bce0 = F.binary_cross_entropy
    rec = {"bce": [], "nll": []}

    def bce(inp, target, *a, **k):
        r = bce0(inp, target.to(inp.dtype), *a, **k)
        rec["bce"].append(r.item())
        return r
    nll0 = F.nll_loss

    def nll(*a, **k):
        r = nll0(*a, **k)
        rec["nll"].append(r.item())
        return r
    F.binary_cross_entropy, F.nll_loss = bce, nll
    mse0 = F.mse_loss

    def mse(*a, **k):
        r = mse0(*a, **k)
        rec["mse"] = r.item()
        return r
    F.mse_loss = mse

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
                        put_tensor(out, prefix, names[id(p)], p.grad, with_idx=True)
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
            if state["step"] == 1:
                out[f"s1/idx/{_name}"] = np.stack((i1.numpy(), i2.numpy())).astype(np.int16)
            return i1, i2
        e.sampling = samp

    np.random.seed(0)
    tuples = []
    for step in range(1, 4):
        state["step"] = step
        rec["bce"].clear()
        rec["nll"].clear()
        r = S.train_adv_few_shot(step, data_src, data_tar, model, opt, opt_d, metric="f1", pair_enumerator_src_train=enu[0],
                                 pair_enumerator_tar_train=enu[1], pair_enumerator_cross_train=enu[2], max_class_num=10,
                                 sample_size=40000, use_clf=True)
        loss_sim, (fs, ft, fc), loss_d, loss_ae, loss_g, loss_recons = r
        tuples.append([loss_sim, fs, ft, fc, loss_d, loss_ae, loss_g, loss_recons])
        if step == 1:
            out["s1/loss"] = np.array(rec["bce"][:3] + [rec["mse"], rec["bce"][3]] + rec["nll"][:2] + [loss_sim])
    out["step/tuple"] = np.array(tuples)
    for k, p in model.named_parameters():
        put_tensor(out, "s3/param", k, p, with_idx=False)
    for k, v in model.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"s3/bn/{k}"] = v.double().numpy() if v.is_floating_point() else v.numpy()

    enu_val = (M.Pair_Enumerator(data_src, mode="val"), M.Pair_Enumerator(data_tar, mode="val"),
               M.Pair_Enumerator_cross(data_src, data_tar, mode="val"))
    enu_test = (M.Pair_Enumerator(data_src, mode="test"), M.Pair_Enumerator(data_tar, mode="test"),
                M.Pair_Enumerator_cross(data_src, data_tar, mode="test"))
    digests = []
    for e in enu_val + enu_test:
        real = e.balanced_sampling

        def bal(*a, _real=real, **k):
            i1, i2 = _real(*a, **k)
            digests.append(digest(i1.numpy(), i2.numpy()))
            return i1, i2
        e.balanced_sampling = bal
    ev = S.eval_adv_v2(data_src, data_tar, model, split="val", metric="f1", enu_list=enu_val, eval_mode="sampling")
    et = S.eval_adv_v2(data_src, data_tar, model, split="test", metric="f1", enu_list=enu_test, eval_mode="sampling")
    out["s3/eval"] = np.array(list(ev) + list(et), np.float64)
    out["eval/digest"] = np.stack(digests)
    path = os.path.join(args.out, "simlearner_office_a2d.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", "tuples", np.array(tuples))


if __name__ == "__main__":
    main()
