"""Generates the JKNet fixtures tests/golden/jknet_office_a2d.npz and tests/golden/jknet_small.npz from the REFERENCE's own
`JKNet` class (models/backbones.py:60-107), run in fp64 on the CPU under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_jknet.py [--out DIR]     (deterministic: fixed seeds, one CPU thread)

PyG and torch_sparse are absent; the shim's GCNConv, JumpingKnowledge and gcn_norm are placeholders and its SparseTensor is minimal.
This file therefore defines small restatements and assigns them into the imported `backbones` module and into `torch_sparse`
before the class is used:
  SparseTensor     COO that keeps duplicate entries (torch_sparse.SparseTensor(row, col, value) does), with the handful of methods
                   the restated gcn_norm needs
  gcn_norm         PyG's SparseTensor branch, step by step: fill_value(1.) when there are no values; fill_diag(adj_t, 1.) -- spelled
                   out as torch_sparse does it: every diagonal entry removed, then one entry of 1 per node; deg = sum(dim=1);
                   deg^-1/2 with inf -> 0; mul by the column vector, mul by the row vector
  GCNConv          lin (glorot, no bias; drawn in Linear's constructor and again in reset_parameters, as PyG does) and a zero
                   bias; forward normalises AGAIN when handed a SparseTensor (normalize=True, cached=False), then lin, matmul, bias
  JumpingKnowledge cat and max
What the fixtures pin to the reference's PROGRAM is therefore JKNet itself: layer wiring (ReLU and dropout after every conv, the
last included; the jump; the Linear; log_softmax), key names, the order and number of initial draws, and the call sequence
gcn_norm(SparseTensor(row=dst, col=src, value=1)) once in JKNet.forward and once more inside every conv.  What gcn_norm, fill_diag,
GCNConv and JumpingKnowledge compute is pinned by the restatements above only (they follow PyG's and torch_sparse's published
sources).  The adjacency values are created by the reference with torch's default dtype, so the fp64 runs set the default dtype to
float64 for the forward (parameters are drawn under float32 first), and `adj_t_cache` -- which the reference never invalidates -- is
cleared by this tool whenever the edges or the precision change.

Contents, per fixture and variant v in {raw, und} (und = the driver's ToUndirected(merge=True), main_graph_knowledge_transfer.py:411)
and per model c (torch.manual_seed(MODEL_SEED) JKNet(F, hidden, C, L, 0.5, mode)); every array is fp64 unless noted:
  {c}/param/{key}          initial state_dict (fp32, the model's own values)
  {v}/{c}/logp             eval forward log-probabilities at the rows `rows`
  {v}/{c}/loss             F.nll_loss over the driver's train mask (:268, mask with y == -1 cleared :404), eval mode
  {v}/{c}/grad/{key}       its parameter gradients
  {v}/{c}/adam_loss [5]    five steps of Adam(lr=1e-3, weight_decay=5e-3) in eval mode: loss before each step
  {v}/{c}/adam/{key}       the parameters after the five steps
  {v}/{c}/flipped          int64 [n_flipped]: indices (into the model's named_parameters order) of the gradient tensors whose fp32
                           reference run differs from the fp64 one by more than GRAD_BAR
plus train_mask (the driver's) and rows.  Models: cat and max at L = 2 and L = 3.  jknet_small.npz holds every key, every row and
its inputs x, y, edge_index (raw): the 40-node graph of gen_golden_gin.small (duplicate edges, self loops, one of them twice, nodes
without in-edges), and one more model, `single_cat_l2h8`: the same class with every conv's second normalisation switched off
(conv.normalize = False) -- the textbook single normalisation, THIS TOOL'S OWN restatement and not the reference's behaviour; it
pins `renormalize=False`.  jknet_office_a2d.npz is kept small: its inputs are tests/golden/office_a2d_graph.npz; instead of
{c}/param/{key} it holds {c}/param_sum/{key} = (sum, sum of squares); outputs at 160 rows; gradients and Adam parameters for the
graph as shipped only ("und" keeps loss and adam_loss).

While it runs, the tool also takes the reference's gradients in fp32 and prints, per case, how many parameter tensors differ from
the fp64 ones by more than the GPU tests' GRAD_BAR (2e-5 of the tensor's max: ReLU kink flips and, in max mode, winner flips
between layers) and asserts that none exceeds KINK_CAP (2e-4).  MODEL_SEED is 0, as in the GCN and GIN fixtures: no case needed
another."""
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

# (name, mode, layers, hidden)
OFFICE_MODELS = (("cat_l2h32", "cat", 2, 32), ("max_l2h20", "max", 2, 20), ("cat_l3h16", "cat", 3, 16), ("max_l3h10", "max", 3, 10))
SMALL_MODELS = (("cat_l2h8", "cat", 2, 8), ("max_l2h8", "max", 2, 8), ("cat_l3h6", "cat", 3, 6), ("max_l3h6", "max", 3, 6))
SINGLE_MODEL = ("single_cat_l2h8", "cat", 2, 8)
GRAD_BAR, KINK_CAP = 2e-5, 2e-4
MODEL_SEED = 0


class SparseTensor:
    """COO [rows, cols] that keeps duplicates; value None = no values yet"""

    def __init__(self, row=None, col=None, value=None, sparse_sizes=None, **kw):
        self.row, self.col = row.reshape(-1).long(), col.reshape(-1).long()
        self.value = value
        self.sizes = tuple(int(s) for s in sparse_sizes)

    def has_value(self):
        return self.value is not None

    def fill_value(self, v):
        return SparseTensor(self.row, self.col, torch.full((self.row.shape[0],), float(v)), self.sizes)

    def sparse_sizes(self):
        return self.sizes


def fill_diag(a, v):
    """torch_sparse.fill_diag: every diagonal entry is removed, then one entry of `v` per node is set"""
    keep = a.row != a.col
    n = min(a.sizes)
    loops = torch.arange(n)
    return SparseTensor(torch.cat([a.row[keep], loops]), torch.cat([a.col[keep], loops]),
                        torch.cat([a.value[keep], torch.full((n,), float(v), dtype=a.value.dtype)]), a.sizes)


def gcn_norm(adj_t, edge_weight=None, num_nodes=None, improved=False, add_self_loops=True, dtype=None):
    """PyG gcn_norm, SparseTensor branch"""
    assert isinstance(adj_t, SparseTensor) and edge_weight is None and not improved
    if not adj_t.has_value():
        adj_t = adj_t.fill_value(1.)
    if add_self_loops:
        adj_t = fill_diag(adj_t, 1.)
    deg = torch.zeros(adj_t.sizes[0], dtype=adj_t.value.dtype).index_add_(0, adj_t.row, adj_t.value)     # sum(adj_t, dim=1)
    dis = deg.pow(-0.5)
    dis = dis.masked_fill(dis == float('inf'), 0.)
    value = adj_t.value * dis[adj_t.row]            # mul(adj_t, deg_inv_sqrt.view(-1, 1))
    value = value * dis[adj_t.col]                  # mul(adj_t, deg_inv_sqrt.view(1, -1))
    return SparseTensor(adj_t.row, adj_t.col, value, adj_t.sizes)


def _backbones():
    from oracle.ref_import import import_reference
    import_reference()
    import backbones
    import torch_sparse
    from torch_geometric.nn.dense.linear import Linear

    class GCNConv(torch.nn.Module):
        def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True):
            super().__init__()
            assert not improved and not cached and add_self_loops
            self.normalize, self.add_self_loops = normalize, add_self_loops
            self.lin = Linear(in_channels, out_channels, bias=False, weight_initializer='glorot')
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
            self.reset_parameters()

        def reset_parameters(self):
            self.lin.reset_parameters()
            torch.nn.init.zeros_(self.bias)

        def forward(self, x, edge_index):
            assert isinstance(edge_index, SparseTensor)
            if self.normalize:                      # cached=False: nothing is remembered, the matrix handed in is normalised again
                edge_index = gcn_norm(edge_index, None, x.size(0), False, self.add_self_loops)
            x = self.lin(x)
            out = torch.zeros_like(x).index_add_(0, edge_index.row, x[edge_index.col] * edge_index.value.unsqueeze(1))
            return out + self.bias

    class JumpingKnowledge(torch.nn.Module):
        def __init__(self, mode, channels=None, num_layers=None):
            super().__init__()
            self.mode = mode.lower()
            assert self.mode in ('cat', 'max')

        def reset_parameters(self):
            pass

        def forward(self, xs):
            if self.mode == 'cat':
                return torch.cat(xs, dim=-1)
            return torch.stack(xs, dim=-1).max(dim=-1)[0]

    backbones.GCNConv, backbones.JumpingKnowledge, backbones.gcn_norm = GCNConv, JumpingKnowledge, gcn_norm
    torch_sparse.SparseTensor, torch_sparse.fill_diag = SparseTensor, fill_diag
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


def _run(model, data, dtype):
    """the reference's forward under `dtype` as torch's default (its adjacency values take the default), cache cleared first"""
    model.adj_t_cache = None
    torch.set_default_dtype(dtype)
    try:
        return model(data)
    finally:
        torch.set_default_dtype(torch.float32)


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
    for name, mode, L, hidden in models:
        torch.manual_seed(MODEL_SEED)
        model = bb.JKNet(F_in, hidden, C, L, 0.5, mode=mode)
        if name.startswith("single_"):
            for conv in model.convs:
                conv.normalize = False               # this tool's single-normalisation restatement, not the reference's behaviour
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
            F.nll_loss(_run(model, types.SimpleNamespace(x=x, edge_index=ei), torch.float32)[tm], y[tm]).backward()
            g32 = {k: p.grad.double().clone() for k, p in model.named_parameters()}
            data = types.SimpleNamespace(x=xd, edge_index=ei)
            model = model.double().eval()
            with torch.no_grad():
                out[pre + "logp"] = _run(model, data, torch.float64)[rows].numpy()
            keep_params = full or var == "raw"
            model.zero_grad()
            loss = F.nll_loss(_run(model, data, torch.float64)[tm], y[tm])
            loss.backward()
            out[pre + "loss"] = np.float64(loss.item())
            flipped = []
            for idx, (k, p) in enumerate(model.named_parameters()):
                err = (g32[k] - p.grad).abs().max().item() / p.grad.abs().max().item()
                assert err <= KINK_CAP, f"{pre}{k}: fp32 reference {err:.3e} of max away from its fp64 self"
                if err > GRAD_BAR:
                    flipped.append(idx)
                if keep_params:
                    out[pre + "grad/" + k] = p.grad.numpy().copy()
            out[pre + "flipped"] = np.array(flipped, dtype=np.int64)
            print(f"{pre}: {len(flipped)} gradient tensors of the fp32 reference beyond {GRAD_BAR} (all within {KINK_CAP})")
            opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-3)
            losses = []
            for _ in range(5):
                opt.zero_grad()
                loss = F.nll_loss(_run(model, data, torch.float64)[tm], y[tm])
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
    """the graph of gen_golden_gin.small: same generator, same seed"""
    n, e, F_in, C = 40, 160, 12, 5
    rng = np.random.Generator(np.random.PCG64(11))
    ei = np.stack([rng.integers(0, n, e), rng.integers(4, n, e)])            # nodes 0..3 receive no edge
    loops = np.array([5, 6, 7, 7, 0])                                         # self loops: 7 twice, 0 (a node without other in-edges)
    ei = np.concatenate([ei, ei[:, :25], np.stack([loops, loops])], axis=1)  # 25 duplicate edges
    x = torch.from_numpy(rng.standard_normal((n, F_in), dtype=np.float32))
    y = torch.from_numpy(rng.integers(-1, C, size=n)).long()
    y[0] = C - 1
    train_mask = torch.from_numpy(rng.random(n) < 0.6)
    return _cases(bb, x, y, train_mask, torch.from_numpy(ei).long(), SMALL_MODELS + (SINGLE_MODEL,), {}, full=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args(argv)
    torch.set_num_threads(1)
    bb = _backbones()
    os.makedirs(a.out, exist_ok=True)
    np.savez_compressed(os.path.join(a.out, "jknet_office_a2d.npz"), **office(bb))
    np.savez_compressed(os.path.join(a.out, "jknet_small.npz"), **small(bb))


if __name__ == "__main__":
    main()
