"""Generates the GIN fixtures tests/golden/gin_office_a2d.npz and tests/golden/gin_small.npz from the REFERENCE's own
`GINNet` class (models/backbones.py:26-57), run in fp64 on the CPU under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_gin.py [--out DIR]     (deterministic: fixed seeds, one CPU thread)

PyG is absent and the shim's GINConv is a placeholder, so this file defines a small restatement of PyG's GINConv
(out_i = nn((1 + eps) * x_i + sum_{j -> i} x_j) over the edges exactly as given; eps a Parameter [1] under train_eps=True and a
buffer [1] otherwise; reset_parameters resets `nn`, then fills eps with its initial value, and runs in the constructor, so `nn`
is drawn twice as in PyG) and assigns it to `backbones.GINConv`.  What the fixtures pin to the reference's program is therefore
GINNet -- layer wiring, the single-layer variant, key names, initial draws -- and the driver's loss; GINConv's own arithmetic is
pinned by this restatement only.

Contents, per fixture and variant v in {raw, und} (und = the driver's ToUndirected(merge=True), main_graph_knowledge_transfer.py:411)
and per model c (torch.manual_seed(MODEL_SEED) GINNet(dataset, layer_num, hidden)); every array is fp64 unless noted:
  {c}/param/{key}          initial state_dict (fp32, the model's own values; eps included, buffer or not)
  {v}/{c}/logp             eval forward log-probabilities at the rows `rows`
  {v}/{c}/loss             F.nll_loss over the driver's train mask (:268, mask with y == -1 cleared :404), eval mode
  {v}/{c}/grad/{key}       its parameter gradients (a buffer eps has none)
  {v}/{c}/adam_loss [5]    five steps of Adam(lr=1e-3, weight_decay=5e-3) in eval mode: loss before each step
  {v}/{c}/adam/{key}       the parameters after the five steps
plus train_mask (the driver's) and rows.  gin_small.npz holds every key, every row and its inputs x, y, edge_index (raw): a graph
of 40 nodes with duplicate edges, self loops (one of them twice) and nodes without in-edges.  gin_office_a2d.npz is kept small:
its inputs are tests/golden/office_a2d_graph.npz; instead of {c}/param/{key} it holds {c}/param_sum/{key} = (sum, sum of squares);
outputs at 160 rows (128 seeded draws + up to 16 rows without in-edges + up to 16 without out-edges); gradients and Adam
parameters for the graph as shipped only ("und" keeps loss and adam_loss).

While it runs, the tool also takes the reference's gradients in fp32 and prints, per case, how many parameter tensors differ from
the fp64 ones by more than the GPU tests' GRAD_BAR (2e-5 of the tensor's max: ReLU kink flips) and asserts that none exceeds
KINK_CAP (2e-4).  MODEL_SEED is 0, as in the GCN fixtures: no case needed another."""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OFFICE_MODELS = (("l2h64", 2, 64), ("l1", 1, 16), ("l3h32", 3, 32))
SMALL_MODELS = (("l2h8", 2, 8), ("l1", 1, 16), ("l3h6", 3, 6))
GRAD_BAR, KINK_CAP = 2e-5, 2e-4
MODEL_SEED = 0


def _backbones():
    from oracle.ref_import import import_reference
    import_reference()
    import backbones

    class GINConv(torch.nn.Module):
        def __init__(self, nn, eps=0., train_eps=False):
            super().__init__()
            self.nn = nn
            self.initial_eps = eps
            if train_eps:
                self.eps = torch.nn.Parameter(torch.Tensor([eps]))
            else:
                self.register_buffer('eps', torch.Tensor([eps]))
            self.reset_parameters()

        def reset_parameters(self):
            self.nn.reset_parameters()
            self.eps.data.fill_(self.initial_eps)

        def forward(self, x, edge_index):
            out = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]])
            return self.nn(out + (1 + self.eps) * x)

    backbones.GINConv = GINConv
    return backbones


def _to_undirected(edge_index, n):
    from torch_geometric.transforms import ToUndirected
    d = types.SimpleNamespace(edge_index=edge_index, num_nodes=n)
    ToUndirected(merge=True)(d)
    return d.edge_index


def _sample_rows(edge_index, n, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    ei = edge_index.numpy()
    no_in = np.flatnonzero(np.bincount(ei[1], minlength=n) == 0)[:16]
    no_out = np.flatnonzero(np.bincount(ei[0], minlength=n) == 0)[:16]
    return np.unique(np.concatenate([rng.choice(n, 128, replace=False), no_in, no_out])).astype(np.int64)


def _cases(bb, x, y, train_mask, edge_index, models, out, full):
    n, F_in = x.shape
    C = int(y.max()) + 1
    ds = types.SimpleNamespace(num_features=F_in, num_classes=C)
    tm = train_mask.clone()
    tm[y == -1] = False
    und = _to_undirected(edge_index.clone(), n)
    rows = np.arange(n, dtype=np.int64) if full else _sample_rows(edge_index, n)
    out["train_mask"], out["rows"] = tm.numpy(), rows
    if full:
        out["x"], out["y"], out["edge_index"] = x.numpy(), y.numpy(), edge_index.numpy()
    xd = x.double()
    for name, L, hidden in models:
        torch.manual_seed(MODEL_SEED)
        model = bb.GINNet(ds, layer_num=L, hidden=hidden)
        sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k, v in sd0.items():
            if full:
                out[f"{name}/param/{k}"] = v.numpy()
            else:
                vd = v.double()
                out[f"{name}/param_sum/{k}"] = np.array([vd.sum().item(), (vd * vd).sum().item()])
        for var, ei in (("raw", edge_index), ("und", und)):
            pre = f"{var}/{name}/"
            model.load_state_dict(sd0)
            model = model.float().eval()
            model.zero_grad()
            F.nll_loss(model(types.SimpleNamespace(x=x, edge_index=ei))[tm], y[tm]).backward()
            g32 = {k: p.grad.double().clone() for k, p in model.named_parameters()}
            data = types.SimpleNamespace(x=xd, edge_index=ei)
            model = model.double().eval()
            with torch.no_grad():
                out[pre + "logp"] = model(data)[rows].numpy()
            keep_params = full or var == "raw"
            model.zero_grad()
            loss = F.nll_loss(model(data)[tm], y[tm])
            loss.backward()
            out[pre + "loss"] = np.float64(loss.item())
            flips = 0
            for k, p in model.named_parameters():
                err = (g32[k] - p.grad).abs().max().item() / p.grad.abs().max().item()
                assert err <= KINK_CAP, f"{pre}{k}: fp32 reference {err:.3e} of max away from its fp64 self"
                flips += err > GRAD_BAR
                if keep_params:
                    out[pre + "grad/" + k] = p.grad.numpy().copy()
            print(f"{pre}: {flips} gradient tensors of the fp32 reference beyond {GRAD_BAR} (all within {KINK_CAP})")
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(model(data)[tm], y[tm])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            out[pre + "adam_loss"] = np.array(losses, dtype=np.float64)
            if keep_params:
                for k, p in model.named_parameters():
                    out[pre + "adam/" + k] = p.detach().numpy().copy()
            model = model.float()
    return out


def office(bb):
    g = np.load(os.path.join(ROOT, "tests", "golden", "office_a2d_graph.npz"))
    x = torch.from_numpy(g["x"])
    y = torch.from_numpy(g["y"]).long()
    ei = torch.from_numpy(g["edge_index"]).long()
    return _cases(bb, x, y, torch.from_numpy(g["train_mask"]), ei, OFFICE_MODELS, {}, full=False)


def small(bb):
    n, e, F_in, C = 40, 160, 12, 5
    rng = np.random.Generator(np.random.PCG64(11))
    ei = np.stack([rng.integers(0, n, e), rng.integers(4, n, e)])            # nodes 0..3 receive no edge
    loops = np.array([5, 6, 7, 7, 0])                                         # self loops: 7 twice, 0 (a node without other in-edges)
    ei = np.concatenate([ei, ei[:, :25], np.stack([loops, loops])], axis=1)  # 25 duplicate edges
    x = torch.from_numpy(rng.standard_normal((n, F_in), dtype=np.float32))
    y = torch.from_numpy(rng.integers(-1, C, size=n)).long()
    y[0] = C - 1
    train_mask = torch.from_numpy(rng.random(n) < 0.6)
    return _cases(bb, x, y, train_mask, torch.from_numpy(ei).long(), SMALL_MODELS, {}, full=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args(argv)
    torch.set_num_threads(1)
    bb = _backbones()
    os.makedirs(a.out, exist_ok=True)
    np.savez_compressed(os.path.join(a.out, "gin_office_a2d.npz"), **office(bb))
    np.savez_compressed(os.path.join(a.out, "gin_small.npz"), **small(bb))


if __name__ == "__main__":
    main()
