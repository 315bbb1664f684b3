"""Generates tests/golden/transfer_office_a2d.npz from the REFERENCE's own step-2 driver (main_graph_knowledge_transfer.py: train
:39-68, test :73-118, get_each_clf_res :119-142, train_gnn :143-262), run on one CPU thread under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_transfer.py [--out DIR]     (deterministic: fixed seeds, one CPU thread)

Process-local patches: F.dropout is the identity, StepLR drops `verbose=` (torch no longer accepts it), the driver's `test` is
wrapped to record what it returns, its prints are swallowed.

Contents
  office/...   tests/golden/office_a2d_graph.npz made undirected (ToUndirected(merge=True), :411), train_mask[y == -1] = False (:404).
    office/param/{key}           a KTGNN_no_complement (built as at :179, seed 0) after WARM_EPOCHS of the driver's own `train`
                                 at lr 1e-2 in fp32: trained far enough that every scored row's argmax is decided (office/margin)
    office/rows [512]            seeded row subset; office/lp_{s,t,h} [512, 31] the eval forward's fp32 log-probs at those rows
    office/sub_{y,train,central} labels and masks of those rows
    office/loss [5]              fp64: total, nll_s, nll_t, nll_t^, kl of `train`'s loss (:44-54, Lambda 1) on the 512-row tables, taken
                                 from `train` itself run on a stand-in model that returns the tables in fp64
    office/grad_{s,t,h}          its autograd gradients w.r.t. the tables (fp32 roundings of the fp64 values)
    office/test_f1 [3], office/test_acc [3], office/test_f1_micro [3], office/each_f1 [3]
                                 `test` (f1 macro / acc / f1 micro) and `get_each_clf_res` (f1) of the fp32 model on the whole graph
    office/pred_{s,t,h} [N]      int8: the three heads' argmax (`max(1)[1]`) on the whole graph
    office/margin [2]            min over the scored rows of (top-1 - top-2 log-prob) and the bar it was checked against:
                                 2 (1e-5 |lp| + 1e-6 max |lp|), twice the forward parity bar (conftest.assert_close)
  bin/...      a seeded 200-node multigraph (oracle.grad_cases.multigraph), 16 features, binary labels, KTGNN at seed 0, eval mode
    bin/{x,edge_index,y,train_mask,val_mask,test_mask,central_mask}
    bin/lp_{s,t,h} [200, 2]      fp32 log-probs;  bin/score_{s,t,h} = exp(lp[:, 1]) as the driver forms it (CPU fp32)
    bin/test_auc [3], bin/each_auc [3]           `test(metric='auc')`, `get_each_clf_res(metric='auc')`
    bin/test_f1, bin/test_f1_micro, bin/test_acc, bin/each_f1 [3]    the other metrics on the same tables
    bin/tie/...                  the same with the log-probs rounded to multiples of 0.02 (tied positive / negative pairs occur: bin/tie/n_tied)
  run64/..., run32/...   `train_gnn` as `main` calls it (:419-421: seed 0, lr 1e-3, wd 5e-3, StepLR(100, 0.1), Lambda 1) for 20 epochs,
                         hidden 64, 2 layers, in fp64 and in fp32 (both from the fp32 seeded initial values):
    loss [20, 4]                 per epoch loss_train, loss_target, loss_target_only, loss_kl
    eval_res [20, 3], eval_res_each [20, 3], best_epoch (0-based, the rule of :238)
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARM_EPOCHS, WARM_LR = 60, 1e-2
N_SUB = 512
EPOCHS = 20


def _driver():
    from oracle.ref_import import REF_CODE, import_reference
    import_reference()
    cwd = os.getcwd()
    os.chdir(REF_CODE)
    try:
        import main_graph_knowledge_transfer as M
    finally:
        os.chdir(cwd)
    from torch.optim.lr_scheduler import StepLR
    M.StepLR = lambda opt, step_size, gamma, verbose=None: StepLR(opt, step_size=step_size, gamma=gamma)
    F.dropout = lambda x, p=0.5, training=True, inplace=False: x
    return M


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def office_data(dtype):
    from torch_geometric.data import Data
    from torch_geometric.transforms import ToUndirected
    g = np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz"))
    d = Data(x=torch.from_numpy(g["x"]).to(dtype), edge_index=torch.from_numpy(g["edge_index"]).long(), y=torch.from_numpy(g["y"]).long(),
             **{k: torch.from_numpy(g[k]).clone() for k in ("train_mask", "val_mask", "test_mask", "central_mask")})
    d.train_mask[d.y == -1] = False
    ToUndirected(merge=True)(d)
    return d


class Tables(torch.nn.Module):
    """stand-in model: returns three given tables (what `train` / `test` see of a model)"""

    def __init__(self, s, t, h):
        super().__init__()
        self.s, self.t, self.h = s, t, h

    def forward(self, data):
        return self.s, self.t, self.h, None


class NoOpt:
    def zero_grad(self):
        pass

    def step(self):
        pass


def build(M, data, C, hidden):
    return M.KTGNN_no_complement(data.x.shape[1], C, 2, hidden, root_weight=False, use_dist_loss=False, dropout=0.5, use_bn=True, step=1,
                                 dim_share=data.x.shape[1], need_complement=False)


def office(M, out):
    data = office_data(torch.float32)
    C = int(data.y.max()) + 1
    torch.manual_seed(0)
    model = build(M, data, C, 64)
    opt = torch.optim.Adam(model.parameters(), lr=WARM_LR, weight_decay=5e-3)
    for _ in range(WARM_EPOCHS):
        quiet(M.train, data, model, opt, gnn="KTGNN", Lambda=1.)
    for k, v in model.state_dict().items():
        out[f"office/param/{k}"] = v.detach().numpy().copy()
    model.eval()
    with torch.no_grad():
        lps = [t.clone() for t in model(data)[:3]]
    # every scored row's argmax must survive the forward parity bar (zero rows excluded)
    tgt = ~data.central_mask
    scored = ((lps[0], data.train_mask | (data.test_mask & tgt)), (lps[1], data.test_mask & tgt), (lps[2], (data.val_mask | data.test_mask) & tgt))
    margin, bar = np.inf, 0.0
    for lp, rows in scored:
        top = lp[rows].double().topk(2, dim=1).values
        b = 2 * (1e-5 * top.abs().max(1).values + 1e-6 * lp.abs().max().double())
        m = top[:, 0] - top[:, 1]
        assert bool((m > b).all()), f"{int((m <= b).sum())} scored rows are undecided at the forward bar: train longer or change the seed"
        margin, bar = min(margin, float(m.min())), max(bar, float(b.max()))
    out["office/margin"] = np.array([margin, bar])
    for name, lp in zip("sth", lps):
        out[f"office/pred_{name}"] = lp.max(1)[1].numpy().astype(np.int8)
    out["office/test_f1"] = np.array(quiet(M.test, data, model, "office", gnn="KTGNN", metric="f1", f1_average="macro"))
    out["office/test_f1_micro"] = np.array(quiet(M.test, data, model, "office", gnn="KTGNN", metric="f1", f1_average="micro"))
    out["office/test_acc"] = np.array(quiet(M.test, data, model, "office", gnn="KTGNN", metric="acc"))
    out["office/each_f1"] = np.array(quiet(M.get_each_clf_res, data, model, metric="f1"))
    # loss and gradients on a row subset, by the driver's own train()
    rows = np.sort(np.random.Generator(np.random.PCG64(0)).choice(data.x.shape[0], N_SUB, replace=False)).astype(np.int64)
    r = torch.from_numpy(rows)
    out["office/rows"] = rows
    from torch_geometric.data import Data
    sub = Data(y=data.y[r], train_mask=data.train_mask[r], central_mask=data.central_mask[r])
    out["office/sub_y"], out["office/sub_train"], out["office/sub_central"] = sub.y.numpy(), sub.train_mask.numpy(), sub.central_mask.numpy()
    tabs = [lp[r].double().requires_grad_(True) for lp in lps]
    for name, lp in zip("sth", lps):
        out[f"office/lp_{name}"] = lp[r].numpy()
    loss, t2, t1, kl = quiet(M.train, sub, Tables(*tabs), NoOpt(), gnn="KTGNN", Lambda=1.)
    nll_s = F.nll_loss(tabs[0].detach()[sub.train_mask], sub.y[sub.train_mask]).item()
    out["office/loss"] = np.array([loss, nll_s, t1, t2, kl])
    for name, t in zip("sth", tabs):
        out[f"office/grad_{name}"] = t.grad.float().numpy()


def binary(M, out):
    from oracle import grad_cases
    from torch_geometric.data import Data
    n = 200
    ei, cm = grad_cases.multigraph(n, 1500, 5)
    rng = np.random.Generator(np.random.PCG64(17))
    x = rng.standard_normal((n, 16), dtype=np.float32)
    y = rng.integers(0, 2, n)
    u = rng.random(n)
    train, val, test = u < 0.5, (u >= 0.5) & (u < 0.7) & ~cm, (u >= 0.7) & ~cm
    data = Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei), y=torch.from_numpy(y).long(), train_mask=torch.from_numpy(train),
                val_mask=torch.from_numpy(val), test_mask=torch.from_numpy(test), central_mask=torch.from_numpy(cm))
    for k in ("x", "edge_index", "y", "train_mask", "val_mask", "test_mask", "central_mask"):
        out[f"bin/{k}"] = getattr(data, k).numpy()
    torch.manual_seed(0)
    model = build(M, data, 2, 16).eval()
    with torch.no_grad():
        lps = [t.clone() for t in model(data)[:3]]
    for pre, tabs in (("bin/", lps), ("bin/tie/", [torch.round(t * 50) / 50 for t in lps])):
        m = Tables(*tabs)
        for name, lp in zip("sth", tabs):
            out[f"{pre}lp_{name}"] = lp.numpy()
            out[f"{pre}score_{name}"] = lp[:, 1].exp().numpy()
        out[pre + "test_auc"] = np.array(quiet(M.test, data, m, "bin", gnn="KTGNN", metric="auc"))
        out[pre + "each_auc"] = np.array(quiet(M.get_each_clf_res, data, m, metric="auc"))
        out[pre + "test_f1"] = np.array(quiet(M.test, data, m, "bin", gnn="KTGNN", metric="f1", f1_average="macro"))
        out[pre + "test_f1_micro"] = np.array(quiet(M.test, data, m, "bin", gnn="KTGNN", metric="f1", f1_average="micro"))
        out[pre + "test_acc"] = np.array(quiet(M.test, data, m, "bin", gnn="KTGNN", metric="acc"))
        out[pre + "each_f1"] = np.array(quiet(M.get_each_clf_res, data, m, metric="f1"))
    sc, rows = out["bin/tie/score_h"], test
    pos, neg = sc[rows & (y == 1)], sc[rows & (y == 0)]
    out["bin/tie/n_tied"] = np.array(int((pos[:, None] == neg[None, :]).sum()))
    assert 0 < out["bin/tie/n_tied"] < pos.size * neg.size


def run(M, out, dtype, pre):
    import types
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        data = office_data(dtype)
        rec = []
        test0, ctor0 = M.test, M.KTGNN_no_complement
        M.test = lambda *a, **k: (rec.append(test0(*a, **k)), rec[-1])[1]

        def ctor(*a, **k):
            # the seeded initial values are the fp32 ones in both runs (an fp64 default dtype would draw other numbers)
            torch.set_default_dtype(torch.float32)
            try:
                return ctor0(*a, **k).to(dtype)
            finally:
                torch.set_default_dtype(dtype)
        M.KTGNN_no_complement = ctor
        try:
            lb, each = quiet(M.train_gnn, types.SimpleNamespace(dataset_name="office_amazon2dslr"), M.pyg_dataset(data), data, save=False,
                             repeat=1, num_epoch=EPOCHS, step_size=100, gamma=0.1, gnn="KTGNN", seed=0, num_layer=2, hidden=64, lr=1e-3,
                             wd=5e-3, use_shceduler=True, step=1, Lambda=1., metric="f1", f1_average="macro")
        finally:
            M.test, M.KTGNN_no_complement = test0, ctor0
    finally:
        torch.set_default_dtype(old)
    out[pre + "loss"] = np.array([lb["source&target"], lb["target_hat"], lb["target"], lb["kl"]], dtype=np.float64).T
    out[pre + "eval_res"] = np.array(rec, dtype=np.float64)
    out[pre + "eval_res_each"] = np.array([each["source&target"], each["target"], each["target_hat"]], dtype=np.float64).T
    best, best_epoch = 666, -1
    for i, v in enumerate(lb["target_hat"]):
        if v < best:
            best, best_epoch = v, i
    out[pre + "best_epoch"] = np.array(best_epoch)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args(argv)
    torch.set_num_threads(1)
    M = _driver()
    out = {}
    office(M, out)
    binary(M, out)
    run(M, out, torch.float64, "run64/")
    run(M, out, torch.float32, "run32/")
    os.makedirs(a.out, exist_ok=True)
    np.savez_compressed(os.path.join(a.out, "transfer_office_a2d.npz"), **out)


if __name__ == "__main__":
    main()
