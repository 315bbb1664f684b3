"""GIN on the fused HIP sum aggregation: the `GINNet` baseline of the reference's zoo (models/backbones.py:26-57).

The model is `layer_num` PyG `GINConv(Linear(in, out), train_eps=True)` layers with ReLU + dropout(0.5) between them and a closing
log_softmax; the single-layer model is `GINConv(Linear(F, C))`, whose eps is a buffer at 0.  PyG's layer is
    out_i = nn((1 + eps) * x_i + sum_{j -> i} x_j)
over the edges exactly as given (`sage.SageGraph`: no self loop added or removed, duplicates are separate messages).  `nn` is one
affine map, so the transform comes first (T = x W^T, one GEMM per layer at the output width, `gcn._transform`) and
`ops.gin_aggregate` forms (1 + eps) * T_i + sum_j T_j + b with the ReLU + dropout or the log_softmax fused into the same pass.  eps
stays on the device.  The backward (`ops.gin_aggregate_bwd`) recovers the epilogue's gradient from the forward's output and sums
grad_eps = sum_i <g_i, T_i> in a fixed order; x, the padded weight, T (only where eps trains) and the layer output are kept."""
import argparse

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .appnp import _no_cpu
from .gcn import _pad_bias, _pad_rows, _transform
from .ktgnn import Linear, dropout_seed
from .sage import SageGraph

__all__ = ["GINConv", "GINNet", "train_gin_noDTC"]


def graph_hubs(graph, threshold=None, segment=None):
    """the `hubs` argument of `GINConv.run` for a SageGraph: (hub tables of the by-destination view | None, of the by-source view |
    None), each (threshold, hub_rows, hub_seg_ptr, seg_bounds); built once per graph and (threshold, segment)"""
    thr = ops.GIN_HUB_THRESHOLD if threshold is None else int(threshold)
    seg = ops.GIN_HUB_SEGMENT if segment is None else int(segment)
    pick = lambda t: None if t is None else (thr, t[0], t[1], t[2])
    return pick(graph.csr.hub_tables(thr, seg)), pick(graph.csr.transposed_hub_tables(thr, seg))


def _layer_forward(x, wp, bp, eps, D, graph, epilogue, p_drop, seed, seed_dev=None, hubs=None):
    T = _transform(x, wp)
    rowptr, col = graph.by_dst[0], graph.by_dst[1]
    return T, ops.gin_aggregate_hubs(T, rowptr, col, eps, graph.num_nodes, D, bias=bp, epilogue=epilogue, p_drop=p_drop, seed=seed,
                                     seed_dev=seed_dev, hubs=hubs[0] if hubs is not None else None)


class _GinLayerFn(torch.autograd.Function):
    """out = epi((1 + eps) T + A T + b), T = x W^T, with hand-written backward: dT, db and deps from the aggregation backward,
    dW = dT^T x, dx = dT W.  A buffer eps (no gradient wanted) keeps no T and runs no eps pass."""

    @staticmethod
    def forward(ctx, x, w, b, eps, graph, epilogue, p_drop, seed, seed_dev=None, hubs=None):
        D = w.shape[0]
        wp = _pad_rows(w.detach())
        T, y = _layer_forward(x.detach(), wp, _pad_bias(b.detach(), D) if b is not None else None, eps.detach(), D, graph, epilogue,
                              p_drop, seed, seed_dev, hubs)
        want_eps = eps.requires_grad
        ctx.save_for_backward(x, wp, eps)
        ctx.T = T if want_eps else None
        ctx.t_hubs = hubs[1] if hubs is not None else None
        ctx.y, ctx.graph, ctx.cfg = y, graph, (D, epilogue, p_drop, b is not None, want_eps)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wp, eps = ctx.saved_tensors
        D, epilogue, p_drop, has_b, want_eps = ctx.cfg
        y, graph = ctx.y, ctx.graph
        N, Dp = x.shape[0], ops.pad4(D)
        if Dp != D or gy.dtype != torch.float32 or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            g = torch.zeros(N, Dp, dtype=torch.float32, device=gy.device)
            g[:, :D] = gy
            gy = g
        t_rowptr, t_dst = graph.by_dst[2], graph.by_dst[3]
        dT, gb, ge = ops.gin_aggregate_bwd_hubs(ctx.T, y, gy, t_rowptr, t_dst, eps.detach(), N, D, epilogue=epilogue, p_drop=p_drop,
                                                want_bias=has_b and ctx.needs_input_grad[2],
                                                want_eps=want_eps and ctx.needs_input_grad[3], hubs=ctx.t_hubs)
        xd = x.detach()
        dW = None
        if ctx.needs_input_grad[1]:
            if ops.gram_supported(Dp, xd.shape[1]) and xd.stride(1) == 1 and xd.stride(0) % 4 == 0 and xd.data_ptr() % 16 == 0:
                dW = ops.gram(dT, xd)[:D]
            else:
                dW = dT.t().mm(xd)[:D]
        gx = None
        if ctx.needs_input_grad[0]:
            din = x.shape[1]
            if ops.linear_supported(Dp, din):
                gx = ops.linear(dT, wp.t().contiguous(), torch.zeros(din, dtype=torch.float32, device=x.device))
            else:
                gx = dT.mm(wp)
        return gx, dW, gb, (ge.reshape(eps.shape) if ge is not None else None), None, None, None, None, None, None


class GINConv(nn.Module):
    """Stand-in for `torch_geometric.nn.GINConv` as the reference builds it (backbones.py:26-57): out_i = nn((1 + eps) * x_i +
    sum_{j -> i} x_j).  `nn` must be ONE `Linear` (this package's or torch's): the layer is computed transform first, which a
    deeper MLP does not allow -- anything else raises NotImplementedError.  `eps` ([1]) is a Parameter under train_eps=True and a
    buffer otherwise, exactly as PyG makes it; state_dict keys eps, nn.weight, nn.bias.  reset_parameters resets `nn`, then fills
    eps with its initial value (PyG draws `nn` in its own constructor and again here: a seeded model keeps its draws)."""

    def __init__(self, nn, eps=0., train_eps=False, **kwargs):
        super().__init__()
        if not isinstance(nn, (Linear, torch.nn.Linear)):
            raise NotImplementedError("GINConv: `nn` must be a single Linear (the layer runs transform first); "
                                      f"got {type(nn).__name__}")
        if kwargs:
            raise NotImplementedError(f"GINConv: MessagePassing options are not implemented: {sorted(kwargs)}")
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer('eps', torch.empty(1))
        self.nn = nn
        self.in_channels = nn.in_channels if hasattr(nn, "in_channels") else nn.in_features
        self.out_channels = nn.out_channels if hasattr(nn, "out_channels") else nn.out_features
        self.reset_parameters()

    def reset_parameters(self):
        self.nn.reset_parameters()
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)

    def run(self, x, graph, epilogue=None, p_drop=0.0, hubs=None):
        """conv output with an optional fused epilogue ("relu" then dropout at p_drop, or "log_softmax"); graph: SageGraph.  hubs:
        None (every row is walked by one lane group, the default) or `graph_hubs(graph)`: hub rows of the forward and hub sources of
        the backward are summed in segments across the grid."""
        _no_cpu(x)
        if x.shape[1] != self.in_channels:
            raise ValueError(f"GINConv: x must have {self.in_channels} columns, got {x.shape[1]}")
        w, b, eps = self.nn.weight, self.nn.bias, self.eps
        D = self.out_channels
        torch_epi = epilogue == "log_softmax" and D > 128
        kern_epi = None if torch_epi else epilogue
        kern_p = p_drop if kern_epi == "relu" else 0.0
        seed, seed_dev = dropout_seed(kern_p, step_word=False)       # a captured epoch: 0 and this layer's device word
        x = x.float()
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad) or eps.requires_grad):
            out = _GinLayerFn.apply(x, w, b, eps, graph, kern_epi, float(kern_p), seed, seed_dev, hubs)
        else:
            out = _layer_forward(x, _pad_rows(w.detach()), _pad_bias(b.detach(), D) if b is not None else None, eps.detach(), D, graph,
                                 kern_epi, float(kern_p), seed, seed_dev, hubs)[1][:, :D]
        if torch_epi:
            out = F.log_softmax(out, dim=1)
        return out

    def forward(self, x, edge_index, edge_attr=None, size=None):
        if edge_attr is not None or size is not None:
            raise NotImplementedError("GINConv: edge attributes and bipartite sizes are not implemented (the reference passes none)")
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("GINConv: bipartite (x_src, x_dst) inputs are not implemented (the reference passes none)")
        _no_cpu(x)
        graph = edge_index if isinstance(edge_index, SageGraph) else SageGraph(edge_index, x.shape[0])
        return self.run(x, graph)

    def extra_repr(self):
        return f"nn={self.nn}"


class GINNet(nn.Module):
    """models/backbones.py:26-57 on the HIP aggregation.  Same constructor and state_dict keys (convs.{i}.eps, convs.{i}.nn.weight,
    convs.{i}.nn.bias), parameters drawn in the reference's order; layer_num == 1 builds `GINConv(Linear(F, C))` with a buffer eps,
    as the reference does.  `dropout` (default the reference's hard-coded 0.5) lets tests switch it off.  forward ->
    log-probabilities.  Dropout sites in forward order: one per conv but the last.  `segment_hubs=True` sums rows (and, in the
    backward, sources) of at least `ops.GIN_HUB_THRESHOLD` edges in segments of `ops.GIN_HUB_SEGMENT` across the grid; off by default:
    a hub's sum is then added in another order, within the same bound but not the same bits."""

    def __init__(self, dataset, layer_num=2, hidden=16, dropout=0.5, segment_hubs=False):
        super().__init__()
        self.dropout = float(dropout)
        self.segment_hubs = bool(segment_hubs)
        F_in, C = dataset.num_features, dataset.num_classes
        self.convs = nn.ModuleList()
        if layer_num == 1:
            self.convs.append(GINConv(Linear(F_in, C)))
        else:
            for num in range(layer_num):
                if num == 0:
                    self.convs.append(GINConv(Linear(F_in, hidden), train_eps=True))
                elif num == layer_num - 1:
                    self.convs.append(GINConv(Linear(hidden, C), train_eps=True))
                else:
                    self.convs.append(GINConv(Linear(hidden, hidden), train_eps=True))
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """SageGraph of edge_index, cached against the tensor (identity, in-place version, shape) as `DeeperGCN.graph` does."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = SageGraph(edge_index, num_nodes)
            self._graph_key = (edge_index, key)
        return self._graph

    def forward(self, data):
        x = data.x
        _no_cpu(x)
        g = self.graph(data.edge_index, x.shape[0])
        p = self.dropout if self.training else 0.0
        hubs = graph_hubs(g) if self.segment_hubs else None
        for ind, conv in enumerate(self.convs):
            last = ind == len(self.convs) - 1
            x = conv.run(x, g, epilogue="log_softmax" if last else "relu", p_drop=0.0 if last else p, hubs=hubs)
        return x


def train_gin_noDTC(args, dataset, data, save=False, repeat=3, num_epoch=200, seed=None, num_layer=2, hidden=64, lr=1e-3, wd=5e-3,
                    use_scheduler=True, step=1, step_size=100, gamma=0.1, metric='f1', f1_average='macro', dropout=0.5, verbose=True,
                    ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:302-396 on `GINNet(dataset, num_layer, hidden)` (`step` is accepted and unused): the run of
    `transfer.train_gnn_noDTC` -- Adam(lr, wd), optional StepLR, best epoch by the lowest `loss_train` -- on this module's model.
    `save=True` writes {ckpt_dir}/model_GIN_{args.dataset_name}_share_best.ckpt.  Returns None like the reference; `history`,
    `dropout`, `verbose`, `ckpt_dir` as in `train_gnn_noDTC`; `graphed=True` raises NotImplementedError."""
    from .transfer import _train_plain_backbone
    if graphed:
        raise NotImplementedError("train_gin_noDTC(graphed=True): the GIN epoch is not offered as a HIP-graph replay; run it eagerly")
    return _train_plain_backbone(args, dataset, data, lambda: GINNet(dataset, num_layer, hidden, dropout=dropout), 'GIN',
                                 lambda model: len(model.convs) - 1 if dropout > 0 else 0, save, repeat, num_epoch, seed, lr, wd,
                                 use_scheduler, step_size, gamma, metric, f1_average, verbose, ckpt_dir, history, graphed)


def build_parser():
    """step 2's flags and defaults (`transfer.build_parser`) with --num_layer 2 and --hidden_dim 64, plus `--dropout`; --model_name,
    --no_dtc and --baseline are accepted and ignored: this entry always trains GIN (--graphed is refused by the driver)"""
    from .transfer import _FLAGS
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.gin", description="Step 2 of Bridged-GNN with the GIN baseline")
    own = {"num_layer": 2, "hidden_dim": 64}
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=own.get(name, default), choices=choices, help=text)
    ap.add_argument("--dropout", type=float, default=0.5, help="dropout probability between the convs")
    return ap


def main(args=None, verbose=True):
    """main_graph_knowledge_transfer.py:399-421 routed to `train_gin_noDTC`.  `args`: the parsed namespace, or a list of
    command-line words (None: sys.argv)."""
    from .bridge import eval_bridged_Graph
    from .data import load_bridged_graph
    from .transfer import _device_of, _say, pyg_dataset
    from .utils import set_random_seed
    if args is None or isinstance(args, (list, tuple)):
        args = build_parser().parse_args(args)
    set_random_seed(0)
    dev = _device_of(args)
    with torch.cuda.device(dev):
        data = load_bridged_graph(args.path_data).to(dev)
        _say(verbose, data)
        eval_bridged_Graph(data)
        data.train_mask[data.y == -1] = False
        dataset = pyg_dataset(data)
        if args.to_undirected:
            data.to_undirected_()
        return train_gin_noDTC(args, dataset, data, save=args.save, repeat=1, num_epoch=args.num_epoch, seed=0,
                               num_layer=args.num_layer, hidden=args.hidden_dim, lr=1e-3, wd=5e-3, use_scheduler=False, step=1,
                               step_size=100, gamma=0.1, metric=args.eval_metric, f1_average='macro', dropout=args.dropout,
                               verbose=verbose, graphed=args.graphed)


if __name__ == '__main__':
    _args = build_parser().parse_args()
    print(_args)
    main(_args)
