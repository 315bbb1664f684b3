"""GCN on the HIP normalised aggregation: the baseline `train_gnn_noDTC` trains by default (`gnn='GCN'`,
main_graph_knowledge_transfer.py:302 -> models/backbones.py:246-300).

Each conv is PyG's `GCNConv(in, out)` with its defaults (add_self_loops, normalize, bias; no edge weights): the transform comes
first (T = x W^T, one GEMM per layer, as GCNConv itself does), then `ops.gcn_aggregate` forms
dinv_i * sum_{j -> i} dinv_j T_j + b over the graph with exactly one self loop per node, with the ReLU + dropout between convs or
the closing log_softmax fused into the same pass.  The backward (`ops.gcn_aggregate_bwd`) recovers the epilogue's gradient from
the forward's output, so nothing but x, the weight and the layer output is kept.

Unlike GraphSAGE's, the reference's `get_emb` / `get_logits` pass the same edge_index to the same convs as `forward`: all three
walk in-neighbours."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ktgnn import Linear, dropout_seed

__all__ = ["GCNConv", "GCNNet", "GcnGraph"]


class GcnGraph:
    """What GCN walks, built once per graph: the by-destination CSR of edge_index with every self loop dropped and one appended
    per node (PyG `add_remaining_self_loops` with unit weights; duplicate non-loop edges keep their multiplicity), its by-source
    view for the backward, dinv = deg^-1/2 over the in-degree of that CSR (>= 1), and the hub tables of both views."""

    def __init__(self, edge_index, num_nodes):
        self.num_nodes = N = int(num_nodes)
        self.csr = ops.build_dst_csr(edge_index.long().contiguous(), N, rewrite_self_loops=True)
        rowptr = self.csr.rowptr
        self.col = self.csr.col[: self.csr.num_edges]
        self.t_rowptr, _, self.t_dst = self.csr.transposed()
        deg = (rowptr[1:N + 1] - rowptr[:N]).double()
        self.dinv = deg.rsqrt().float().contiguous()              # correctly rounded 1/sqrt(deg)
        self.hubs = self._hubs(self.csr.hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT))
        self.t_hubs = self._hubs(self.csr.transposed_hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT))

    @staticmethod
    def _hubs(tables):
        return None if tables is None else (ops.GCN_HUB_THRESHOLD, tables[0], tables[1], tables[2])


def _transform(x, w):
    """T = x w^T: the W-stationary kernel inside its envelope, the library GEMM outside it.  w: [pad4(D), Din], zero pad rows."""
    if (ops.linear_supported(x.shape[1], w.shape[0]) and x.dtype == torch.float32 and x.stride(1) == 1
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0):
        return ops.linear(x, w, torch.zeros(w.shape[0], dtype=torch.float32, device=x.device))
    return x.mm(w.t())


def _pad_rows(w):
    D, din = w.shape
    Dp = ops.pad4(D)
    if Dp == D:
        return w.contiguous()
    wp = torch.zeros(Dp, din, dtype=torch.float32, device=w.device)
    wp[:D] = w
    return wp


def _pad_bias(b, D):
    """the bias as an aligned row of pad4(D) floats (a parameter's storage is not promised to be 16-byte aligned)"""
    if b is None:
        return None
    bp = torch.zeros(ops.pad4(D), dtype=torch.float32, device=b.device)
    bp[:D] = b
    return bp


def _layer_forward(x, wp, bp, D, graph, epilogue, p_drop, seed, seed_dev=None):
    T = _transform(x, wp)
    return ops.gcn_aggregate(T, graph.csr.rowptr, graph.col, graph.dinv, graph.num_nodes, D, bias=bp, epilogue=epilogue,
                             p_drop=p_drop, seed=seed, seed_dev=seed_dev, hubs=graph.hubs)


class _GcnLayerFn(torch.autograd.Function):
    """out = epi(A^ x W^T + b) with hand-written backward: dT and db from the aggregation backward, dW = dT^T x, dx = dT W."""

    @staticmethod
    def forward(ctx, x, w, b, graph, epilogue, p_drop, seed, seed_dev=None):
        D = w.shape[0]
        wp = _pad_rows(w.detach())
        y = _layer_forward(x.detach(), wp, _pad_bias(b.detach(), D) if b is not None else None, D, graph, epilogue, p_drop,
                           seed, seed_dev)
        ctx.save_for_backward(x, wp)
        ctx.y, ctx.graph, ctx.cfg = y, graph, (D, epilogue, p_drop, b is not None)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wp = ctx.saved_tensors
        D, epilogue, p_drop, has_b = ctx.cfg
        y, graph = ctx.y, ctx.graph
        N, Dp = x.shape[0], ops.pad4(D)
        if Dp != D or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            g = torch.zeros(N, Dp, dtype=torch.float32, device=gy.device)
            g[:, :D] = gy
            gy = g
        dT, gb = ops.gcn_aggregate_bwd(y, gy, graph.t_rowptr, graph.t_dst, graph.dinv, N, D, epilogue=epilogue, p_drop=p_drop,
                                       want_bias=has_b, hubs=graph.t_hubs)
        xd = x.detach()
        if ops.gram_supported(Dp, xd.shape[1]) and xd.stride(1) == 1 and xd.stride(0) % 4 == 0 and xd.data_ptr() % 16 == 0:
            dW = ops.gram(dT, xd)
        else:
            dW = dT.t().mm(xd)
        gx = None
        if ctx.needs_input_grad[0]:
            din = x.shape[1]
            if ops.linear_supported(Dp, din):
                gx = ops.linear(dT, wp.t().contiguous(), torch.zeros(din, dtype=torch.float32, device=x.device))
            else:
                gx = dT.mm(wp)
        return gx, dW[:D], gb, None, None, None, None, None


class GCNConv(nn.Module):
    """Stand-in for `torch_geometric.nn.GCNConv` as the reference builds it (backbones.py:252-261: defaults only):
    out = D^-1/2 (A' + I) D^-1/2 x W^T + b, A' = the edges without self loops, duplicates counted.  `lin` (glorot, no bias) and
    `bias` (zeros) carry PyG's state_dict keys and initialisers."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True):
        super().__init__()
        if improved or cached or not add_self_loops or not normalize:
            raise NotImplementedError("GCNConv: only PyG's defaults (improved=False, cached=False, add_self_loops=True, "
                                      "normalize=True) are implemented")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = Linear(in_channels, out_channels, bias=False, weight_initializer="glorot")
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()          # PyG draws `lin` twice (Linear.__init__, then here): a seeded model keeps its draws

    def reset_parameters(self):
        self.lin.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def run(self, x, graph, epilogue=None, p_drop=0.0):
        """conv output with an optional fused epilogue ("relu" then dropout at p_drop, or "log_softmax"); graph: GcnGraph."""
        if not x.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x.device} tensor)")
        w, b = self.lin.weight, self.bias
        D = self.out_channels
        torch_epi = epilogue == "log_softmax" and D > 128
        kern_epi = None if torch_epi else epilogue
        kern_p = p_drop if kern_epi == "relu" else 0.0
        seed, seed_dev = dropout_seed(kern_p, step_word=False)       # a captured epoch: 0 and this layer's device word
        x = x.float()
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)):
            out = _GcnLayerFn.apply(x, w, b, graph, kern_epi, float(kern_p), seed, seed_dev)
        else:
            out = _layer_forward(x, _pad_rows(w.detach()), _pad_bias(b.detach(), D) if b is not None else None, D, graph,
                                 kern_epi, float(kern_p), seed, seed_dev)[:, :D]
        if torch_epi:
            out = F.log_softmax(out, dim=1)
        return out

    def forward(self, x, edge_index):
        graph = edge_index if isinstance(edge_index, GcnGraph) else GcnGraph(edge_index, x.shape[0])
        return self.run(x, graph)


class GCNNet(nn.Module):
    """models/backbones.py:246-300 on the HIP aggregation.  Same constructor and state_dict keys (convs.{i}.bias,
    convs.{i}.lin.weight); `dropout` (default the reference's hard-coded 0.5) lets tests switch it off.  forward ->
    log-probabilities; get_emb (all convs but the last) and get_logits (raw logits) walk the same graph as forward.  The autograd
    path runs whenever grad is enabled and a parameter requires it; dropout only in training mode."""

    def __init__(self, dataset, layer_num=2, hidden=16, dropout=0.5):
        super().__init__()
        self.dropout = float(dropout)
        F_in, C = dataset.num_features, dataset.num_classes
        self.convs = nn.ModuleList()
        if layer_num == 1:
            self.convs.append(GCNConv(F_in, C))
        else:
            for num in range(layer_num):
                if num == 0:
                    self.convs.append(GCNConv(F_in, hidden))
                elif num == layer_num - 1:
                    self.convs.append(GCNConv(hidden, C))
                else:
                    self.convs.append(GCNConv(hidden, hidden))
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """GcnGraph of edge_index, cached against the tensor (identity, in-place version, shape) as `GraphSAGE.graph` does."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = GcnGraph(edge_index, num_nodes)
            self._graph_key = (edge_index, key)
        return self._graph

    def _run(self, data, n_convs, last_epilogue):
        x = data.x
        g = self.graph(data.edge_index, x.shape[0])
        p = self.dropout if self.training else 0.0
        for ind in range(n_convs):
            last = ind == len(self.convs) - 1
            x = self.convs[ind].run(x, g, epilogue=last_epilogue if last else "relu", p_drop=0.0 if last else p)
        return x

    def forward(self, data):
        return self._run(data, len(self.convs), "log_softmax")

    def get_emb(self, data):
        return self._run(data, len(self.convs) - 1, None)

    def get_logits(self, data):
        return self._run(data, len(self.convs), None)
