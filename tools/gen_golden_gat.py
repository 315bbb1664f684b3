"""Generates the GAT fixtures tests/golden/gat_office_a2d.npz and tests/golden/gat_small.npz from the REFERENCE's own `GAT`
class (models/backbones.py:404-438), run in fp64 on the CPU under oracle/shim.

Build-container only: it needs the reference tree (oracle.ref_import).  Only numeric arrays are written.
Re-run:  python tools/gen_golden_gat.py [--out DIR]     (deterministic: fixed seeds, one CPU thread)

PyG is absent and the shim's GATConv is a placeholder, so this file defines a small restatement of PyG 2.0-2.2's GATConv
(`lin_src` = `lin_dst`, one glorot Linear without bias; att_src / att_dst [1, H, C] glorot; bias zeros; remove_self_loops +
add_self_loops; softmax per destination of leaky_relu(alpha_src[j] + alpha_dst[i], 0.2) with PyG's 1e-16 in the denominator;
F.dropout on the coefficients; propagate(aggr='add'); concat or mean over heads; + bias; parameters drawn by Linear.__init__ and
again by reset_parameters in the order lin_src, lin_dst, att_src, att_dst) and assigns it to `backbones.GATConv`.  What the
fixtures pin to the reference's program is therefore GAT -- layer wiring, ELU, key names, initial draws -- and the driver's loss;
GATConv's own arithmetic and draw order are pinned by this restatement only.

Contents, per fixture and variant v in {raw, und} (und = the driver's ToUndirected(merge=True), main_graph_knowledge_transfer.py:411)
and per model c (torch.manual_seed(0) GAT(dataset, hidden, head)); every array is fp64 unless noted:
  {c}/param/{key}          initial state_dict (fp32, the model's own values)
  {v}/{c}/logp             eval forward log-probabilities at the rows `rows`
  {v}/{c}/emb              get_emb at the rows `emb_rows`
  {v}/{c}/loss             F.nll_loss over the driver's train mask (:268, mask with y == -1 cleared :404), eval mode
  {v}/{c}/grad/{key}       its parameter gradients (named_parameters: the shared Linear appears once, as conv?.lin_src.weight)
  {v}/{c}/adam_loss [5]    five steps of Adam(lr=1e-3, weight_decay=5e-3) in eval mode: loss before each step
  {v}/{c}/adam/{key}       the parameters after the five steps
plus train_mask (the driver's), rows and emb_rows.  gat_small.npz holds every key, every row and its inputs x, y, edge_index (raw):
a graph of 40 nodes with duplicate edges, self loops (one of them twice) and nodes without in-edges.  gat_office_a2d.npz has to
stay under the 1 MiB (1 048 576 B) a committed file may have (gcn_office_a2d.npz: 1 035 818 B; with emb at all 160 rows and
conv1's whole weight gradient and Adam result this file would be about 2.4 MB of incompressible fp64): its inputs are
tests/golden/office_a2d_graph.npz; instead of {c}/param/{key} it holds {c}/param_sum/{key} = (sum, sum of squares); logp at 160 rows (128 seeded draws + up to 16 rows without in-edges + up to 16
without out-edges), emb at the first 48 of them; gradients and Adam parameters for the graph as shipped only ("und" keeps loss and
adam_loss), and of conv1's [H*C, 256] weight only the rows `wrows/{c}` together with {..}/grad_sum/{key} and {..}/adam_sum/{key} =
(sum, sum of squares) of the whole tensor.

While it runs, the tool also takes the reference's gradients in fp32 and prints, per case, how many parameter tensors differ from
the fp64 ones by more than the GPU tests' GRAD_BAR (2e-5 of the tensor's max: LeakyReLU kink flips) and checks that none exceeds
their KINK_CAP (2e-4)."""
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

OFFICE_MODELS = (("h64x3", 64, 3), ("h16x8", 16, 8))
SMALL_MODELS = (("h8x3", 8, 3), ("h6x1", 6, 1), ("h5x2", 5, 2))
GRAD_BAR, KINK_CAP = 2e-5, 2e-4
EMB_ROWS, W_ROWS = 48, 32
BIG = "conv1.lin_src.weight"


def _backbones():
    from oracle.ref_import import import_reference
    import_reference()
    import backbones
    from torch_geometric.nn.dense.linear import Linear

    def glorot(t):
        a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
        torch.nn.init.uniform_(t, -a, a)

    class GATConv(torch.nn.Module):
        def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0):
            super().__init__()
            self.heads, self.out_channels, self.concat = heads, out_channels, concat
            self.negative_slope, self.dropout = negative_slope, dropout
            self.lin_src = Linear(in_channels, heads * out_channels, bias=False, weight_initializer="glorot")
            self.lin_dst = self.lin_src
            self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels))
            self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels))
            self.bias = torch.nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
            self.reset_parameters()

        def reset_parameters(self):
            self.lin_src.reset_parameters()
            self.lin_dst.reset_parameters()
            glorot(self.att_src)
            glorot(self.att_dst)
            torch.nn.init.zeros_(self.bias)

        def forward(self, x, edge_index):
            n, H, C = x.shape[0], self.heads, self.out_channels
            xs = self.lin_src(x).view(-1, H, C)
            a_src = (xs * self.att_src).sum(-1)
            a_dst = (xs * self.att_dst).sum(-1)
            keep = edge_index[0] != edge_index[1]                       # remove_self_loops, add_self_loops
            loops = torch.arange(n, dtype=edge_index.dtype)
            src = torch.cat([edge_index[0][keep], loops])
            dst = torch.cat([edge_index[1][keep], loops])
            e = F.leaky_relu(a_src[src] + a_dst[dst], self.negative_slope)
            idx = dst.unsqueeze(1).expand(-1, H)
            m = torch.full((n, H), -math.inf, dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax")
            ex = (e - m[dst]).exp()
            den = torch.zeros(n, H, dtype=e.dtype).index_add_(0, dst, ex)
            alpha = ex / (den[dst] + 1e-16)
            alpha = F.dropout(alpha, p=self.dropout, training=self.training)
            out = torch.zeros(n, H, C, dtype=xs.dtype).index_add_(0, dst, xs[src] * alpha.unsqueeze(-1))
            out = out.view(-1, H * C) if self.concat else out.mean(dim=1)
            return out + self.bias

    backbones.GATConv = GATConv
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
    ds = types.SimpleNamespace(num_features=F_in, num_classes=C)
    tm = train_mask.clone()
    tm[y == -1] = False
    und = _to_undirected(edge_index.clone(), n)
    rows = np.arange(n, dtype=np.int64) if full else _sample_rows(edge_index, n)
    emb_rows = rows if full else rows[:EMB_ROWS]
    out["train_mask"], out["rows"], out["emb_rows"] = tm.numpy(), rows, emb_rows
    if full:
        out["x"], out["y"], out["edge_index"] = x.numpy(), y.numpy(), edge_index.numpy()
    xd = x.double()

    def keep_tensor(prefix, name, k, v):
        v = v.detach().numpy().copy()
        if not full and k == BIG:
            out[f"{prefix}_sum/{k}"] = _sums(v)
            v = v[out[f"wrows/{name}"]]
        out[f"{prefix}/{k}"] = v

    for name, hidden, head in models:
        torch.manual_seed(0)
        model = bb.GAT(ds, hidden=hidden, head=head)
        sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k, v in sd0.items():
            if full:
                out[f"{name}/param/{k}"] = v.numpy()
            else:
                out[f"{name}/param_sum/{k}"] = _sums(v)
        if not full:
            rng = np.random.Generator(np.random.PCG64(1))
            out[f"wrows/{name}"] = np.sort(rng.choice(hidden * head, W_ROWS, replace=False)).astype(np.int64)
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
                out[pre + "emb"] = model.get_emb(data)[emb_rows].numpy()
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
            if keep_params:
                for k, p in model.named_parameters():
                    keep_tensor(pre + "adam", name, k, p)
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
    np.savez_compressed(os.path.join(a.out, "gat_office_a2d.npz"), **office(bb))
    np.savez_compressed(os.path.join(a.out, "gat_small.npz"), **small(bb))


if __name__ == "__main__":
    main()
