"""GraphSAGE on the HIP mean aggregation: the model the reference trains in step 2 when `--no_dtc` is passed
(main_graph_knowledge_transfer.py:326, :414-417 -> models/backbones.py:440-498).

Each conv is evaluated transform-first: lin_l is linear, so W_l mean_j(x_j) = mean_j(W_l x_j).  One GEMM per layer makes the
interleaved table T = x [W_l ; W_r]^T + [0 ; b_l] ([N, 2*pad4(D)]: T_l | T_r), and `ops.sage_mean_aggregate` averages rows of
the OUTPUT width and adds the root half, with the ReLU + dropout between convs or the closing log_softmax fused into the same
pass.  The backward (`ops.sage_mean_aggregate_bwd`) recovers the epilogue's gradient from the forward's output, so nothing but
x, the weights and the layer output is kept.

`get_emb` / `get_logits` keep the reference's quirk: they build the adjacency with row = edge_index[0] and so average over
OUT-neighbours.  That is exactly a forward over the by-source view (`DstCSR.transposed()`) of the same edges."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ktgnn import Linear, dropout_seed

__all__ = ["SAGEConv", "GraphSAGE", "SageGraph"]


class SageGraph:
    """The two CSR views of an edge_index that GraphSAGE walks: by destination (in-neighbours; reference forward :464) and by
    source (out-neighbours; get_emb / get_logits :475, :489).  Edges are kept exactly as given: no self loop is added or
    removed and duplicates keep their multiplicity (torch_sparse SparseTensor semantics)."""

    def __init__(self, edge_index, num_nodes):
        self.num_nodes = int(num_nodes)
        self.csr = ops.build_dst_csr(edge_index.long().contiguous(), self.num_nodes, rewrite_self_loops=False)
        t_rowptr, _, t_dst = self.csr.transposed()
        col = self.csr.col[: self.csr.num_edges]
        self.by_dst = (self.csr.rowptr, col, t_rowptr, t_dst)      # (rows, cols) of the pass, then the swapped view
        self.by_src = (t_rowptr, t_dst, self.csr.rowptr, col)

    def view(self, out_neighbours=False):
        return self.by_src if out_neighbours else self.by_dst


def _transform(x, wcat, bcat):
    """T = x wcat^T + bcat: the W-stationary kernel inside its envelope, the library GEMM outside it."""
    if (ops.linear_supported(x.shape[1], wcat.shape[0]) and x.dtype == torch.float32 and x.stride(1) == 1
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0):
        return ops.linear(x, wcat, bcat)
    return torch.addmm(bcat, x, wcat.t())


def _pack(w_l, b_l, w_r):
    """[W_l ; W_r] as [2*Dp, Din] with zero pad rows, and [0 ; b_l] (the bias rides in the root half)."""
    D, din = w_l.shape
    Dp = ops.pad4(D)
    wcat = torch.zeros(2 * Dp, din, dtype=torch.float32, device=w_l.device)
    bcat = torch.zeros(2 * Dp, dtype=torch.float32, device=w_l.device)
    wcat[:D] = w_l
    if w_r is not None:
        wcat[Dp:Dp + D] = w_r
    if b_l is not None:
        bcat[Dp:Dp + D] = b_l
    return wcat, bcat


def _layer_forward(x, wcat, bcat, D, view, epilogue, p_drop, seed, seed_dev=None):
    N = x.shape[0]
    Dp = ops.pad4(D)
    T = _transform(x, wcat, bcat)
    rowptr, col = view[0], view[1]
    return ops.sage_mean_aggregate(T[:, :Dp], rowptr, col, N, D, root=T[:, Dp:], mean=True, epilogue=epilogue,
                                   p_drop=p_drop, seed=seed, seed_dev=seed_dev)


class _SageLayerFn(torch.autograd.Function):
    """out = epi(mean_{j -> i} x_j W_l^T + b_l + x_i W_r^T) with hand-written backward (dT from the aggregation backward, then
    dW = dT^T x, db_l = column sums of dT_r, dx = dT [W_l ; W_r])."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, view, epilogue, p_drop, seed, seed_dev=None):
        D = w_l.shape[0]
        wcat, bcat = _pack(w_l.detach(), b_l.detach() if b_l is not None else None, w_r.detach() if w_r is not None else None)
        y = _layer_forward(x.detach(), wcat, bcat, D, view, epilogue, p_drop, seed, seed_dev)
        ctx.save_for_backward(x, wcat)
        ctx.y, ctx.view, ctx.cfg = y, view, (D, epilogue, p_drop, b_l is not None, w_r is not None)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wcat = ctx.saved_tensors
        D, epilogue, p_drop, has_b, has_r = ctx.cfg
        y, (rowptr, _, t_rowptr, t_col) = ctx.y, ctx.view
        N, Dp = x.shape[0], ops.pad4(D)
        if Dp != D or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            g = torch.zeros(N, Dp, dtype=torch.float32, device=gy.device)
            g[:, :D] = gy
            gy = g
        dT = torch.empty(N, 2 * Dp, dtype=torch.float32, device=x.device)
        ops.sage_mean_aggregate_bwd(y, gy, rowptr, t_rowptr, t_col, N, D, epilogue=epilogue, p_drop=p_drop,
                                    grad_tbl=dT[:, :Dp], grad_root=dT[:, Dp:])
        xd = x.detach()
        if (ops.gram_supported(2 * Dp, xd.shape[1]) and xd.stride(1) == 1 and xd.stride(0) % 4 == 0 and xd.data_ptr() % 16 == 0):
            dW = ops.gram(dT, xd)
        else:
            dW = dT.t().mm(xd)
        gw_l = dW[:D]
        gw_r = dW[Dp:Dp + D] if has_r else None
        gb_l = ops.column_sums(dT)[Dp:Dp + D] if has_b else None
        gx = None
        if ctx.needs_input_grad[0]:
            din = x.shape[1]
            if ops.linear_supported(2 * Dp, din):
                gx = ops.linear(dT, wcat.t().contiguous(), torch.zeros(din, dtype=torch.float32, device=x.device))
            else:
                gx = dT.mm(wcat)
        return gx, gw_l, gb_l, gw_r, None, None, None, None, None


class SAGEConv(nn.Module):
    """Stand-in for `torch_geometric.nn.SAGEConv` (mean aggregation) as the reference builds it (backbones.py:445-456):
    out_i = W_l mean_{j -> i} x_j + b_l (+ W_r x_i with root_weight); lin_l / lin_r carry the reference's state_dict keys.
    `normalize=True` (PyG's L2 row normalisation of the output; the reference never sets it) runs in torch."""

    def __init__(self, in_channels, out_channels, normalize=False, root_weight=True, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.root_weight = normalize, root_weight
        self.lin_l = Linear(in_channels, out_channels, bias=bias)
        if root_weight:
            self.lin_r = Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        if self.root_weight:
            self.lin_r.reset_parameters()

    def _params(self):
        return self.lin_l.weight, self.lin_l.bias, (self.lin_r.weight if self.root_weight else None)

    def run(self, x, graph, epilogue=None, p_drop=0.0, out_neighbours=False):
        """conv output with an optional fused epilogue ("relu" then dropout at p_drop, or "log_softmax"); graph: SageGraph."""
        if not x.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x.device} tensor)")
        w_l, b_l, w_r = self._params()
        D = self.out_channels
        torch_epi = self.normalize or (epilogue == "log_softmax" and D > 128)
        kern_epi = None if torch_epi else epilogue
        kern_p = p_drop if kern_epi == "relu" else 0.0
        seed, seed_dev = dropout_seed(kern_p, step_word=False)       # a captured epoch: 0 and this layer's device word
        view = graph.view(out_neighbours)
        x = x.float()
        if torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in (w_l, b_l, w_r))):
            out = _SageLayerFn.apply(x, w_l, b_l, w_r, view, kern_epi, float(kern_p), seed, seed_dev)
        else:
            wcat, bcat = _pack(w_l.detach(), b_l.detach() if b_l is not None else None, w_r.detach() if w_r is not None else None)
            out = _layer_forward(x, wcat, bcat, D, view, kern_epi, float(kern_p), seed, seed_dev)[:, :D]
        if torch_epi:
            if self.normalize:
                out = F.normalize(out, p=2.0, dim=-1)
            if epilogue == "relu":
                out = F.dropout(F.relu(out), p=p_drop, training=p_drop > 0)
            elif epilogue == "log_softmax":
                out = F.log_softmax(out, dim=1)
        return out

    def forward(self, x, edge_index):
        graph = edge_index if isinstance(edge_index, SageGraph) else SageGraph(edge_index, x.shape[0])
        return self.run(x, graph)


class GraphSAGE(nn.Module):
    """models/backbones.py:440-498 on the HIP aggregation.  Same constructor and state_dict keys (convs.{i}.lin_l.weight,
    convs.{i}.lin_l.bias, convs.{i}.lin_r.weight); `dropout` (default the reference's hard-coded 0.5) lets tests switch it off.
    forward -> log-probabilities; get_emb (all convs but the last) and get_logits (raw logits) average over OUT-neighbours, as the
    reference does.  The autograd path runs whenever grad is enabled and a parameter requires it; dropout only in training mode."""

    def __init__(self, dataset, layer_num=2, hidden=16, root_weight=True, dropout=0.5):
        super().__init__()
        self.dropout = float(dropout)
        F_in, C = dataset.num_features, dataset.num_classes
        self.convs = nn.ModuleList()
        if layer_num == 1:
            self.convs.append(SAGEConv(F_in, C, root_weight=root_weight))
        else:
            for num in range(layer_num):
                if num == 0:
                    self.convs.append(SAGEConv(F_in, hidden, root_weight=root_weight))
                elif num == layer_num - 1:
                    self.convs.append(SAGEConv(hidden, C, root_weight=root_weight))
                else:
                    self.convs.append(SAGEConv(hidden, hidden, root_weight=root_weight))
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """SageGraph of edge_index, cached against the tensor (identity, in-place version, shape): the reference rebuilds its
        SparseTensor per call, the cache changes no result.  `Data.to_undirected_()` replaces the tensor and so the cache."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = SageGraph(edge_index, num_nodes)
            self._graph_key = (edge_index, key)
        return self._graph

    def _run(self, data, out_neighbours, n_convs, last_epilogue):
        x = data.x
        g = self.graph(data.edge_index, x.shape[0])
        p = self.dropout if self.training else 0.0
        for ind in range(n_convs):
            last = ind == len(self.convs) - 1
            x = self.convs[ind].run(x, g, epilogue=last_epilogue if last else "relu", p_drop=0.0 if last else p,
                                    out_neighbours=out_neighbours)
        return x

    def forward(self, data):
        return self._run(data, False, len(self.convs), "log_softmax")

    def get_emb(self, data, layer_num=1):
        return self._run(data, True, len(self.convs) - 1, None)

    def get_logits(self, data, layer_num=1):
        return self._run(data, True, len(self.convs), None)
