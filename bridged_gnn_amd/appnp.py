"""APPNP on the HIP K-step propagation: the `APPNP_Net` baseline of the reference's zoo (models/backbones.py:110-128).

The model is an MLP -- dropout(x) -> lin1 -> ReLU -> dropout -> lin2 -- followed by PyG's `APPNP(K=10, alpha=0.1)` with its
defaults: K personalised-PageRank steps z_{k+1} = (1 - alpha) A^ z_k + alpha h over the GCN-normalised graph (`gcn.GcnGraph`:
one self loop per node, duplicates counted, dinv = deg^-1/2), at class width, then log_softmax.  `ops.appnp_propagate` runs
the K steps as K launches with the teleport term, the state scaling and the closing log_softmax fused in.  The operator is
linear with symmetric dinv products, so its backward is the same call over the graph's by-source view applied to the output
gradient: nothing but the output is kept.  The two dropout sites are `ops.feature_dropout` passes whose masks come from a
(seed, element index) hash with a (seed, seed_dev) pair like every other dropout site of the package."""
import argparse

import torch
import torch.nn as nn

from . import ops
from .gcn import GcnGraph, _pad_bias, _pad_rows
from .ktgnn import Linear, dropout_seed

__all__ = ["APPNP", "APPNP_Net", "train_appnp_noDTC"]


def _no_cpu(t):
    if not t.is_cuda:
        raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                           f"(got a {t.device} tensor)")


def _rows4(t, D):
    """t[:, :D] as rows the kernels take (unit column stride, a row stride that is a multiple of 4 floats, 16-byte aligned base):
    t itself where it already is, else a zero-padded [N, pad4(D)] copy"""
    if t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= ops.pad4(D) and t.data_ptr() % 16 == 0:
        return t
    p = torch.zeros(t.shape[0], ops.pad4(D), dtype=torch.float32, device=t.device)
    p[:, :D] = t[:, :D]
    return p


def _flat4(t):
    """t as a contiguous, 16-byte aligned float32 tensor (the streaming passes' operand)"""
    t = t.float()
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


class _AppnpFn(torch.autograd.Function):
    """out = epi(P h), P = ((1-a)A^)^K + a sum_{m<K} ((1-a)A^)^m; grad_h = P^T g is the same recurrence over the by-source view with
    g (the gradient at z_K: dy, or dy - exp(y) rowsum(dy) under log_softmax) in h's place."""

    @staticmethod
    def forward(ctx, h, graph, K, alpha, epilogue):
        D = h.shape[1]
        y = ops.appnp_propagate(_rows4(h.detach(), D), graph.csr.rowptr, graph.col, graph.dinv, graph.num_nodes, D, K, alpha,
                                epilogue=epilogue, hubs=graph.hubs)
        ctx.y = y if epilogue == "log_softmax" else None
        ctx.graph, ctx.cfg = graph, (D, K, alpha)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        D, K, alpha = ctx.cfg
        graph = ctx.graph
        g = _rows4(gy, D)
        if ctx.y is not None:
            g = ops.appnp_log_softmax_bwd(ctx.y, g, D)
        gh = ops.appnp_propagate(g, graph.t_rowptr, graph.t_dst, graph.dinv, graph.num_nodes, D, K, alpha, epilogue=None,
                                 hubs=graph.t_hubs)
        return gh[:, :D], None, None, None, None


def _streamable(t):
    return t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def _logits(x, wp, bp):
    """h = x wp^T + bp as [N, pad4(D)] rows (zero pad columns): the W-stationary kernel inside its envelope, the library GEMM outside"""
    if ops.linear_supported(x.shape[1], wp.shape[0]) and _streamable(x):
        return ops.linear(x, wp, bp)
    return torch.addmm(bp, x, wp.t())


def _head_forward(x, wp, bp, D, graph, K, alpha, epilogue):
    return ops.appnp_propagate(_logits(x, wp, bp), graph.csr.rowptr, graph.col, graph.dinv, graph.num_nodes, D, K, alpha,
                               epilogue=epilogue, hubs=graph.hubs)


class _HeadFn(torch.autograd.Function):
    """out = epi(P (x W^T + b)): the class-width Linear and the propagation as one node, so that the logits are formed as padded
    rows (no copy in front of the kernel) and the bias gradient is the fixed-order column-sum kernel over the padded gradient --
    torch's `sum(0)` over a width that is no multiple of 4 is a multi-block reduction, which a captured epoch must not hold (the
    memset-node rule of `transfer._GraphedEpoch`).  dh = P^T g over the by-source view, dW = dh^T x, db = colsum(dh), dx = dh W."""

    @staticmethod
    def forward(ctx, x, w, b, graph, K, alpha, epilogue):
        D = w.shape[0]
        wp = _pad_rows(w.detach())
        y = _head_forward(x.detach(), wp, _pad_bias(b.detach(), D), D, graph, K, alpha, epilogue)
        ctx.save_for_backward(x, wp)
        ctx.y = y if epilogue == "log_softmax" else None
        ctx.graph, ctx.cfg = graph, (D, K, alpha)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wp = ctx.saved_tensors
        D, K, alpha = ctx.cfg
        graph = ctx.graph
        Dp = ops.pad4(D)
        g = _rows4(gy, D)
        if ctx.y is not None:
            g = ops.appnp_log_softmax_bwd(ctx.y, g, D)
        dh = ops.appnp_propagate(g, graph.t_rowptr, graph.t_dst, graph.dinv, graph.num_nodes, D, K, alpha, epilogue=None,
                                 hubs=graph.t_hubs)                         # [N, pad4(D)], pad columns 0
        xd = x.detach()
        if ops.gram_supported(Dp, xd.shape[1]) and _streamable(xd):
            dW = ops.gram(dh, xd)
        else:
            dW = dh.t().mm(xd)
        gb = ops.column_sums(dh)[:D]
        gx = None
        if ctx.needs_input_grad[0]:
            din = x.shape[1]
            if ops.linear_supported(Dp, din):
                gx = ops.linear(dh, wp.t().contiguous(), torch.zeros(din, dtype=torch.float32, device=x.device))
            else:
                gx = dh.mm(wp)
        return gx, dW[:D], gb, None, None, None, None


class APPNP(nn.Module):
    """Stand-in for `torch_geometric.nn.APPNP` as the reference builds it (backbones.py:115: `APPNP(10, 0.1)`, defaults otherwise):
    K steps of z <- (1 - alpha) D^-1/2 (A' + I) D^-1/2 z + alpha h.  No parameters, no buffers."""

    def __init__(self, K, alpha, dropout=0., cached=False, add_self_loops=True, normalize=True):
        super().__init__()
        if dropout != 0 or cached or not add_self_loops or not normalize:
            raise NotImplementedError("APPNP: only PyG's defaults (dropout=0, cached=False, add_self_loops=True, normalize=True) "
                                      "are implemented")
        self.K, self.alpha = int(K), float(alpha)

    def reset_parameters(self):
        pass

    def run(self, h, graph, epilogue=None):
        """the propagated logits with an optional fused epilogue ("log_softmax"); graph: GcnGraph."""
        _no_cpu(h)
        h = h.float()
        if torch.is_grad_enabled() and h.requires_grad:
            return _AppnpFn.apply(h, graph, self.K, self.alpha, epilogue)
        D = h.shape[1]
        return ops.appnp_propagate(_rows4(h.detach(), D), graph.csr.rowptr, graph.col, graph.dinv, graph.num_nodes, D, self.K,
                                   self.alpha, epilogue=epilogue, hubs=graph.hubs)[:, :D]

    def forward(self, x, edge_index, edge_weight=None):
        if edge_weight is not None:
            raise NotImplementedError("APPNP: edge weights are not implemented (the reference passes none)")
        _no_cpu(x)
        graph = edge_index if isinstance(edge_index, GcnGraph) else GcnGraph(edge_index, x.shape[0])
        return self.run(x, graph)

    def extra_repr(self):
        return f"K={self.K}, alpha={self.alpha}"


class _FeatureDropFn(torch.autograd.Function):
    """y = drop(relu?(x)) on the streaming HIP pass; the backward reads the mask off y (ReLU) or redraws it from the seed.
    row_ids: the global row of every row (a rank's rows of a partition draw the whole-graph masks), or None."""

    @staticmethod
    def forward(ctx, x, p, seed, seed_dev, relu, row_ids=None):
        y = ops.feature_dropout(_flat4(x.detach()), p, seed, seed_dev, relu=relu, row_ids=row_ids)
        if relu:
            ctx.save_for_backward(y)           # the node's own output: kept as a saved tensor, never as an attribute (a cycle
        ctx.cfg, ctx.seed_dev = (p, seed, relu, row_ids), seed_dev     # output -> node -> output would keep the graph above it alive)
        return y

    @staticmethod
    def backward(ctx, gy):
        p, seed, relu, row_ids = ctx.cfg
        y = ctx.saved_tensors[0] if relu else None
        return ops.feature_dropout_bwd(_flat4(gy), p, seed, ctx.seed_dev, y=y, relu=relu, row_ids=row_ids), None, None, None, None, None


def _feature_drop(x, p, relu, row_ids=None):
    """one dropout site: takes its seed (in forward order) only where a mask is drawn"""
    if p <= 0 and not relu:
        return x
    seed, seed_dev = dropout_seed(p, step_word=False)        # a captured epoch: 0 and this site's device word
    if torch.is_grad_enabled() and x.requires_grad:
        return _FeatureDropFn.apply(x, float(p), seed, seed_dev, relu, row_ids)
    return ops.feature_dropout(_flat4(x.detach()), float(p), seed, seed_dev, relu=relu, row_ids=row_ids)


class APPNP_Net(nn.Module):
    """models/backbones.py:110-128 on the HIP propagation.  Same members and state_dict keys (lin1.weight, lin1.bias, lin2.weight,
    lin2.bias; prop1 has no state), parameters drawn in the reference's order; `dropout` (default the reference's hard-coded 0.5),
    `K` and `alpha` (the reference's 10 and 0.1) let tests and the driver set them.  forward -> log-probabilities.  The two
    dropout sites take their seeds in forward order: the input, then the hidden activation."""

    def __init__(self, dataset, hidden=16, dropout=0.5, K=10, alpha=0.1):
        super().__init__()
        self.dropout = float(dropout)
        self.lin1 = Linear(dataset.num_features, hidden)
        self.lin2 = Linear(hidden, dataset.num_classes)
        self.prop1 = APPNP(K, alpha)
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """GcnGraph of edge_index, cached against the tensor (identity, in-place version, shape) as `GCNNet.graph` does."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = GcnGraph(edge_index, num_nodes)
            self._graph_key = (edge_index, key)
        return self._graph

    def forward(self, data):
        x = data.x
        _no_cpu(x)
        g = self.graph(data.edge_index, x.shape[0])
        p = self.dropout if self.training else 0.0
        x = _feature_drop(x, p, relu=False)
        x = _feature_drop(self.lin1(x), p, relu=True).float()
        w, b = self.lin2.weight, self.lin2.bias          # lin2 and prop1 as one autograd node (_HeadFn)
        K, alpha = self.prop1.K, self.prop1.alpha
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad):
            return _HeadFn.apply(x, w, b, g, K, alpha, "log_softmax")
        D = w.shape[0]
        return _head_forward(x, _pad_rows(w.detach()), _pad_bias(b.detach(), D), D, g, K, alpha, "log_softmax")[:, :D]


def train_appnp_noDTC(args, dataset, data, save=False, repeat=3, num_epoch=200, seed=None, num_layer=2, hidden=64, K=10, alpha=0.1,
                      lr=1e-3, wd=5e-3, use_scheduler=True, step=1, step_size=100, gamma=0.1, metric='f1', f1_average='macro',
                      dropout=0.5, verbose=True, ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:302-396 on `APPNP_Net(dataset, hidden)` (`num_layer` and `step` are accepted and unused): the
    run of `transfer.train_gnn_noDTC` -- Adam(lr, wd), optional StepLR, best epoch by the lowest `loss_train` -- on this module's
    model.  `save=True` writes {ckpt_dir}/model_APPNP_{args.dataset_name}_share_best.ckpt.  Returns None like the reference;
    `history`, `dropout`, `verbose`, `ckpt_dir` as in `train_gnn_noDTC`; `graphed=True` raises NotImplementedError."""
    from .transfer import _train_plain_backbone
    if graphed:
        raise NotImplementedError("train_appnp_noDTC(graphed=True): the APPNP epoch is not offered as a HIP-graph replay yet (its "
                                  "capture has not been made to work; see DESIGN section 19); run it eagerly")
    return _train_plain_backbone(args, dataset, data, lambda: APPNP_Net(dataset, hidden, dropout=dropout, K=K, alpha=alpha), 'APPNP',
                                 lambda model: 2 if dropout > 0 else 0, save, repeat, num_epoch, seed, lr, wd, use_scheduler, step_size,
                                 gamma, metric, f1_average, verbose, ckpt_dir, history, graphed)


def build_parser():
    """step 2's flags and defaults (`transfer.build_parser`) plus `--K` and `--alpha`; --model_name, --no_dtc and --baseline are
    accepted and ignored: this entry always trains APPNP_Net (--graphed is refused by the driver)"""
    from .transfer import _FLAGS
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.appnp", description="Step 2 of Bridged-GNN with the APPNP baseline")
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=default, choices=choices, help=text)
    ap.add_argument("--K", type=int, default=10, help="propagation steps (the reference builds APPNP(10, 0.1))")
    ap.add_argument("--alpha", type=float, default=0.1, help="teleport probability")
    return ap


def main(args=None, verbose=True):
    """main_graph_knowledge_transfer.py:399-421 routed to `train_appnp_noDTC`.  `args`: the parsed namespace, or a list of
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
        return train_appnp_noDTC(args, dataset, data, save=args.save, repeat=1, num_epoch=args.num_epoch, seed=0,
                                 num_layer=args.num_layer, hidden=args.hidden_dim, K=args.K, alpha=args.alpha, lr=1e-3, wd=5e-3,
                                 use_scheduler=False, step=1, step_size=100, gamma=0.1, metric=args.eval_metric, f1_average='macro',
                                 verbose=verbose, graphed=args.graphed)


if __name__ == '__main__':
    _args = build_parser().parse_args()
    print(_args)
    main(_args)
