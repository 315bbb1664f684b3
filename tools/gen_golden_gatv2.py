"""Generates the GATv2 fixtures tests/golden/gatv2_office_a2d.npz and tests/golden/gatv2_small.npz from the REFERENCE's own `GATv2`
class (models/backbones.py:302-358), run in fp64 on the CPU under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_gatv2.py [--out DIR]     (deterministic: fixed seeds, one CPU thread)

PyG is absent and the shim's GATv2Conv is a placeholder, so this file defines a small restatement of PyG 2.0-2.2's GATv2Conv with
share_weights=False (`lin_l`, `lin_r`: two glorot Linears with bias; att [1, H, C] glorot; bias zeros; remove_self_loops +
add_self_loops; per edge j -> i the logit <att, leaky_relu(x_l[j] + x_r[i], 0.2)>, softmax per destination with PyG's 1e-16 in the
denominator; F.dropout on the coefficients; propagate(aggr='add') of x_l[j]; concat or mean over heads; + bias; parameters drawn by
Linear.__init__ (lin_l, lin_r) and again by reset_parameters in the order lin_l, lin_r, att) and assigns it to
`backbones.GATv2Conv`.  The shim's torch_sparse.SparseTensor, remove_self_loops and add_self_loops, which GATv2.forward calls, are
used as they are.  What the fixtures pin to the reference's program is therefore GATv2 -- layer wiring (num_layers -> convs, the
registered and unused BatchNorms), ELU, key names, initial draws -- and the driver's loss; GATv2Conv's own arithmetic and draw
order are pinned by this restatement only.

Contents, per fixture and variant v in {raw, und} (und = the driver's ToUndirected(merge=True), main_graph_knowledge_transfer.py:411)
and per model c (torch.manual_seed(seed of c) GATv2(F, hidden, C, layers, heads, 0.6, 0.5)); every array is fp64 unless noted:
  {c}/param/{key}          initial state_dict (the model's own values and dtypes)
  {v}/{c}/logp             eval forward log-probabilities at the rows `rows`
  {v}/{c}/loss             F.nll_loss over the driver's train mask (:268, mask with y == -1 cleared :404), eval mode
  {v}/{c}/grad/{key}       its parameter gradients (the parameters that receive one: the BatchNorms' do not)
  {v}/{c}/adam_loss [5]    five steps of Adam(lr=1e-3, weight_decay=5e-3) in eval mode: loss before each step
  {v}/{c}/adam/{key}       those parameters after the five steps
plus train_mask (the driver's) and rows.  gatv2_small.npz holds every key, every row and its inputs x, y, edge_index (raw): the
40-node graph of gat_small.npz (duplicate edges, self loops, one of them twice, nodes without in-edges).  gatv2_office_a2d.npz
stays under the 1 MiB a committed file may have: its inputs are tests/golden/office_a2d_graph.npz; instead of {c}/param/{key} it
holds {c}/param_sum/{key} = (sum, sum of squares); logp at 160 rows (128 seeded draws + up to 16 rows without in-edges + up to 16
without out-edges); gradients and Adam parameters for the graph as shipped only ("und" keeps loss and adam_loss), and of the first
conv's two [H*C, 256] weights only the rows `wrows/{c}` together with {..}/grad_sum/{key} and {..}/adam_sum/{key} = (sum, sum of
squares) of the whole tensor.

While it runs, the tool also takes the reference's gradients in fp32 and prints, per case, how many parameter tensors differ from
the fp64 ones by more than the GPU tests' GRAD_BAR (2e-5 of the tensor's max: LeakyReLU kink flips and fp32 rounding) and checks
that none exceeds their KINK_CAP (2e-4).  It takes the five Adam steps in fp32 as well and checks that every parameter ends within
a tenth of the GPU tests' Adam bar (1e-4 of the tensor's max) of the fp64 run.  That check chose the seeds: the gradient of lin_r
is what the LeakyReLU sides leave of a sum of terms that cancel (the de of a row sum to zero), Adam divides every element by its
own magnitude, so an element whose gradient is rounding noise moves by the full step in either direction, and on the office graph
the reference ALONE, fp32 against fp64 on the CPU, ends up to 1e-2 of the max apart (seeds 0..11: h64x1l2 1.1e-4, 9.1e-3, 2.2e-5,
2.1e-4, 3.7e-6, ...; h16x3l3 1.0e-3, 2.7e-4, 1.2e-3, 1.5e-4, 9.4e-5, 1.8e-4, 2.8e-4, 1.4e-2, 6.6e-6, ...; seeds 1, 4, 6 and 7 of one
or the other also break the kink cap on the gradients).  Per office model the seed is the first of 0, 1, 2, ... at which the fp32
reference passes both checks on both variants (the tenth: another fp32 machine is another draw of the same noise); the small
models pass at seed 0.  Said plainly: the GPU tests' five Adam steps therefore run on seeds screened to be benign.  At most
other seeds of the office models ANY fp32 implementation, the reference's own included, misses the 1e-4 Adam bar for reasons
that are not a kernel's; the kernels' own arithmetic is pinned by the kernel-level tests and by the gradient tests' two-tier
rule, which hold at every seed."""
import argparse
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OFFICE_MODELS = (("h64x1l2", 64, 1, 2, 4), ("h16x3l3", 16, 3, 3, 8))    # (name, hidden, heads, num_layers, seed)
SMALL_MODELS = (("h8x3l2", 8, 3, 2, 0), ("h6x1l3", 6, 1, 3, 0), ("h5x2l2", 5, 2, 2, 0))
GRAD_BAR, KINK_CAP, ADAM_BAR = 2e-5, 2e-4, 1e-4
W_ROWS = 16
BIG = ("convs.0.lin_l.weight", "convs.0.lin_r.weight")
DROPOUT, ATT_DROPOUT = 0.6, 0.5


def _backbones():
    from oracle.ref_import import import_reference
    import_reference()
    import backbones
    from torch_geometric.nn.dense.linear import Linear

    class GATv2Conv(torch.nn.Module):
        def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0):
            super().__init__()
            self.heads, self.out_channels, self.concat = heads, out_channels, concat
            self.negative_slope, self.dropout = negative_slope, dropout
            self.lin_l = Linear(in_channels, heads * out_channels, bias=True, weight_initializer="glorot")
            self.lin_r = Linear(in_channels, heads * out_channels, bias=True, weight_initializer="glorot")
            self.att = torch.nn.Parameter(torch.empty(1, heads, out_channels))
            self.bias = torch.nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
            self.reset_parameters()

        def reset_parameters(self):
            self.lin_l.reset_parameters()
            self.lin_r.reset_parameters()
            a = math.sqrt(6.0 / (self.att.size(-2) + self.att.size(-1)))
            torch.nn.init.uniform_(self.att, -a, a)
            torch.nn.init.zeros_(self.bias)

        def forward(self, x, edge_index):
            n, H, C = x.shape[0], self.heads, self.out_channels
            x_l = self.lin_l(x).view(-1, H, C)
            x_r = self.lin_r(x).view(-1, H, C)
            keep = edge_index[0] != edge_index[1]                       # remove_self_loops, add_self_loops
            loops = torch.arange(n, dtype=edge_index.dtype)
            src = torch.cat([edge_index[0][keep], loops])
            dst = torch.cat([edge_index[1][keep], loops])
            e = (F.leaky_relu(x_l[src] + x_r[dst], self.negative_slope) * self.att).sum(-1)
            idx = dst.unsqueeze(1).expand(-1, H)
            m = torch.full((n, H), -math.inf, dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax")
            ex = (e - m[dst]).exp()
            den = torch.zeros(n, H, dtype=e.dtype).index_add_(0, dst, ex)
            alpha = ex / (den[dst] + 1e-16)
            alpha = F.dropout(alpha, p=self.dropout, training=self.training)
            out = torch.zeros(n, H, C, dtype=x_l.dtype).index_add_(0, dst, x_l[src] * alpha.unsqueeze(-1))
            out = out.view(-1, H * C) if self.concat else out.mean(dim=1)
            return out + self.bias

    backbones.GATv2Conv = GATv2Conv
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


def _sums(v):
    vd = torch.as_tensor(v).double()
    return np.array([vd.sum().item(), (vd * vd).sum().item()])


def _cases(bb, x, y, train_mask, edge_index, models, out, full):
    n, F_in = x.shape
    C = int(y.max()) + 1
    tm = train_mask.clone()
    tm[y == -1] = False
    und = _to_undirected(edge_index.clone(), n)
    rows = np.arange(n, dtype=np.int64) if full else _sample_rows(edge_index, n)
    out["train_mask"], out["rows"] = tm.numpy(), rows
    if full:
        out["x"], out["y"], out["edge_index"] = x.numpy(), y.numpy(), edge_index.numpy()
    xd = x.double()

    def keep_tensor(prefix, name, k, v):
        v = v.detach().numpy().copy()
        if not full and k in BIG:
            out[f"{prefix}_sum/{k}"] = _sums(v)
            v = v[out[f"wrows/{name}"]]
        out[f"{prefix}/{k}"] = v

    def fresh(model, dtype):
        """the reference caches the adjacency of its first call (adj_t_cache) and never reads it: cleared between variants"""
        model.adj_t_cache = None
        return model.to(dtype).eval()

    for name, hidden, heads, layers, seed in models:
        torch.manual_seed(seed)
        model = bb.GATv2(F_in, hidden, C, layers, heads, DROPOUT, ATT_DROPOUT)
        sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k, v in sd0.items():
            if full:
                out[f"{name}/param/{k}"] = v.numpy()
            else:
                out[f"{name}/param_sum/{k}"] = _sums(v)
        if not full:
            rng = np.random.Generator(np.random.PCG64(1))
            out[f"wrows/{name}"] = np.sort(rng.choice(hidden * heads, W_ROWS, replace=False)).astype(np.int64)
        for var, ei in (("raw", edge_index), ("und", und)):
            pre = f"{var}/{name}/"
            model.load_state_dict(sd0)
            model = fresh(model, torch.float32)
            model.zero_grad()
            F.nll_loss(model(types.SimpleNamespace(x=x, edge_index=ei))[tm], y[tm]).backward()
            g32 = {k: p.grad.double().clone() for k, p in model.named_parameters() if p.grad is not None}
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-3)
            for _ in range(5):
                opt.zero_grad()
                F.nll_loss(model(types.SimpleNamespace(x=x, edge_index=ei))[tm], y[tm]).backward()
                opt.step()
            a32 = {k: p.detach().double().clone() for k, p in model.named_parameters() if k in g32}
            model.load_state_dict(sd0)
            data = types.SimpleNamespace(x=xd, edge_index=ei)
            model = fresh(model, torch.float64)
            with torch.no_grad():
                out[pre + "logp"] = model(data)[rows].numpy()
            keep_params = full or var == "raw"
            model.zero_grad()
            loss = F.nll_loss(model(data)[tm], y[tm])
            loss.backward()
            out[pre + "loss"] = np.float64(loss.item())
            trained = [(k, p) for k, p in model.named_parameters() if p.grad is not None]
            assert sorted(k for k, _ in trained) == sorted(k for k, _ in model.named_parameters() if not k.startswith("bns."))
            flips = 0
            for k, p in trained:
                err = (g32[k] - p.grad).abs().max().item() / p.grad.abs().max().item()
                assert err <= KINK_CAP, f"{pre}{k}: fp32 reference {err:.3e} of max away from its fp64 self"
                flips += err > GRAD_BAR
                if keep_params:
                    keep_tensor(pre + "grad", name, k, p.grad)
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
            for k, p in trained:
                err = (a32[k] - p.detach()).abs().max().item() / p.detach().abs().max().item()
                assert err <= ADAM_BAR / 10, f"{pre}{k}: fp32 reference after five Adam steps {err:.3e} of max away from its fp64 self"
                if keep_params:
                    keep_tensor(pre + "adam", name, k, p)
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
    np.savez_compressed(os.path.join(a.out, "gatv2_office_a2d.npz"), **office(bb))
    np.savez_compressed(os.path.join(a.out, "gatv2_small.npz"), **small(bb))


if __name__ == "__main__":
    main()
