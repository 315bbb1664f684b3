"""GCNII on the fused HIP propagate-and-mix conv: the `GCN2` baseline of the reference's zoo (models/backbones.py:163-197).

The model is lins[0] -> ReLU (x0), L layers of PyG's `GCN2Conv(H, alpha, theta, layer, shared_weights=True, normalize=False)` each
followed by ReLU, then lins[1] and log_softmax, with a dropout in front of lins[0], of every conv and of lins[1].  A layer is
    a = A^ x,  m = (1 - alpha) a + alpha x0,  out = (1 - beta) m + beta m weight1,  beta = log(theta / layer + 1),
over the GCN-normalised graph (`gcn.GcnGraph`: one self loop per node, duplicates counted, dinv = deg^-1/2 -- what `gcn_norm`
leaves in the reference's cached adjacency).  `ops.gcn2_conv` runs the aggregation, the mix, the product with
M = (1 - beta) I + beta weight1, the ReLU and the dropout that FOLLOWS the layer as one pass; in evaluation m never reaches
memory, in training it is written once because grad_weight1 = beta m^T gz needs it.  The backward is one dense pass
(`ops.gcn2_conv_bwd`: gz, t = (1 - alpha) gz M^T, gx0 = alpha gz M^T), the Gram kernel for grad_weight1, and the GCN walk over
the by-source view for grad_x.  Dropout sites take their seeds in forward order through `ktgnn.dropout_seed`: the input, x0 on
its way into the first conv (both `ops.feature_dropout` passes), then one per conv (fused)."""
import argparse
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .appnp import _feature_drop, _no_cpu, _rows4
from .gcn import GcnGraph
from .ktgnn import Linear, dropout_seed

__all__ = ["GCN2Conv", "GCN2", "train_gcn2_noDTC"]


def _mix_matrix(weight1, beta):
    """M = (1 - beta) I + beta weight1 as [pad4(H), pad4(H)] with zero padding: m @ M = (1 - beta) m + beta m weight1"""
    H = weight1.shape[0]
    Hp = ops.pad4(H)
    M = torch.zeros(Hp, Hp, dtype=torch.float32, device=weight1.device)
    M[:H, :H] = beta * weight1
    M.diagonal()[:H].add_(1.0 - beta)
    return M


class _Gcn2LayerFn(torch.autograd.Function):
    """y = drop(relu(((1 - alpha) A^ x + alpha x0) M)) with hand-written backward.  Kept: m, y and M."""

    @staticmethod
    def forward(ctx, x, x0, weight1, graph, alpha, beta, p_drop, seed, seed_dev):
        H = weight1.shape[0]
        N = graph.num_nodes
        M = _mix_matrix(weight1.detach().float(), beta)
        m = torch.empty(N, ops.pad4(H), dtype=torch.float32, device=x.device)
        y = ops.gcn2_conv(_rows4(x.detach(), H), _rows4(x0.detach(), H), M, graph.csr.rowptr, graph.col, graph.dinv, N, H, alpha,
                          p_drop=p_drop, seed=seed, seed_dev=seed_dev, hubs=graph.hubs, m_out=m)
        ctx.save_for_backward(m, y, M)
        ctx.graph, ctx.cfg = graph, (H, alpha, beta, p_drop)
        return y[:, :H]

    @staticmethod
    def backward(ctx, gy):
        m, y, M = ctx.saved_tensors
        H, alpha, beta, p_drop = ctx.cfg
        graph = ctx.graph
        Hp = ops.pad4(H)
        gz, t, gx0 = ops.gcn2_conv_bwd(y, _rows4(gy, H), M, H, alpha, p_drop)
        gw = gx = None
        if ctx.needs_input_grad[2]:
            gw = (ops.gram(m, gz) if ops.gram_supported(Hp, Hp) else m.t().mm(gz))[:H, :H] * beta
        if ctx.needs_input_grad[0]:
            # A^ is symmetric in its dinv products: the forward walk over the by-source view, no bias, no epilogue
            gx = ops.gcn_aggregate(t, graph.t_rowptr, graph.t_dst, graph.dinv, graph.num_nodes, H, hubs=graph.t_hubs)[:, :H]
        return gx, (gx0[:, :H] if ctx.needs_input_grad[1] else None), gw, None, None, None, None, None, None


def _prop(x, rowptr, col, hubs, graph):
    """A^ x over one view of the graph on `ops.gcn_aggregate` (any width)"""
    D = x.shape[1]
    return ops.gcn_aggregate(_rows4(x, D), rowptr, col, graph.dinv, graph.num_nodes, D, hubs=hubs)[:, :D]


class _PropFn(torch.autograd.Function):
    """a = A^ x; grad_x = A^ grad_a over the by-source view (the operator is symmetric in its dinv products)."""

    @staticmethod
    def forward(ctx, x, graph):
        ctx.graph = graph
        return _prop(x.detach(), graph.csr.rowptr, graph.col, graph.hubs, graph)

    @staticmethod
    def backward(ctx, ga):
        graph = ctx.graph
        return _prop(ga, graph.t_rowptr, graph.t_dst, graph.t_hubs, graph), None


def _glorot_(t):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    return nn.init.uniform_(t, -a, a)


class GCN2Conv(nn.Module):
    """Stand-in for `torch_geometric.nn.GCN2Conv` as the reference builds it (backbones.py:173-176: shared weights, layer = l + 1,
    normalize=False over an adjacency that `gcn_norm` has normalised already): out = (1 - beta) m + beta m weight1 with
    m = (1 - alpha) A^ x + alpha x_0, beta = log(theta / layer + 1) (1 when theta or layer is None).  `weight1` ([H, H], glorot,
    applied untransposed) carries PyG's state_dict key.  `normalize` is accepted either way: the layer always walks a `GcnGraph`,
    the normalised operator the reference hands it."""

    def __init__(self, channels, alpha, theta=None, layer=None, shared_weights=True, cached=False, add_self_loops=True,
                 normalize=True):
        super().__init__()
        if not shared_weights or cached or not add_self_loops:
            raise NotImplementedError("GCN2Conv: only shared_weights=True, cached=False and add_self_loops=True are implemented")
        self.channels, self.alpha = int(channels), float(alpha)
        self.beta = 1.0
        if theta is not None or layer is not None:
            assert theta is not None and layer is not None
            self.beta = math.log(theta / layer + 1)
        self.weight1 = nn.Parameter(torch.empty(self.channels, self.channels))
        self.register_parameter("weight2", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot_(self.weight1)

    def _mix(self, x, x0, graph):
        if torch.is_grad_enabled() and x.requires_grad:
            a = _PropFn.apply(x, graph)
        else:
            a = _prop(x.detach(), graph.csr.rowptr, graph.col, graph.hubs, graph)
        return (1.0 - self.alpha) * a + self.alpha * x0

    def run(self, x, x0, graph, p_drop=0.0):
        """drop(relu(conv(x, x0))): the layer as the model uses it, with the dropout that follows it; graph: GcnGraph."""
        _no_cpu(x)
        x, x0, w = x.float(), x0.float(), self.weight1
        H, p_drop = self.channels, float(p_drop)
        if not ops.gcn2_supported(H):                # outside the kernel's envelope: the aggregation kernel and the library GEMM
            m = self._mix(x, x0, graph)
            return _feature_drop(torch.addmm(m, m, w, beta=1.0 - self.beta, alpha=self.beta), p_drop, relu=True)
        seed, seed_dev = dropout_seed(p_drop, step_word=False)
        if torch.is_grad_enabled() and (x.requires_grad or x0.requires_grad or w.requires_grad):
            return _Gcn2LayerFn.apply(x, x0, w, graph, self.alpha, self.beta, p_drop, seed, seed_dev)
        return ops.gcn2_conv(_rows4(x.detach(), H), _rows4(x0.detach(), H), _mix_matrix(w.detach().float(), self.beta),
                             graph.csr.rowptr, graph.col, graph.dinv, graph.num_nodes, H, self.alpha, p_drop=p_drop, seed=seed,
                             seed_dev=seed_dev, hubs=graph.hubs)[:, :H]

    def forward(self, x, x_0, edge_index, edge_weight=None):
        """the bare conv output (no ReLU), as PyG returns it; composed from the aggregation kernel and one GEMM"""
        if edge_weight is not None:
            raise NotImplementedError("GCN2Conv: edge weights are not implemented (the reference passes none)")
        _no_cpu(x)
        graph = edge_index if isinstance(edge_index, GcnGraph) else GcnGraph(edge_index, x.shape[0])
        m = self._mix(x.float(), x_0.float()[:, :self.channels], graph)
        return torch.addmm(m, m, self.weight1, beta=1.0 - self.beta, alpha=self.beta)

    def extra_repr(self):
        return f"{self.channels}, alpha={self.alpha}, beta={self.beta}"


class GCN2(nn.Module):
    """models/backbones.py:163-197 on the HIP conv.  Same constructor and state_dict keys (lins.0.weight, lins.0.bias, lins.1.weight,
    lins.1.bias, convs.{l}.weight1), parameters drawn in the reference's order (lins, then convs).  forward -> log-probabilities.
    Dropout sites in forward order: 0 the input, 1 x0 on its way into the first conv (x0 itself stays undropped), 2 .. L+1 after
    each conv's ReLU (fused into the conv; the last one feeds lins[1])."""

    def __init__(self, dataset, hidden_channels, num_layers, alpha, theta, shared_weights=True, dropout=0.0):
        super().__init__()
        self.lins = nn.ModuleList([Linear(dataset.num_features, hidden_channels), Linear(hidden_channels, dataset.num_classes)])
        self.convs = nn.ModuleList([GCN2Conv(hidden_channels, alpha, theta, layer + 1, shared_weights, normalize=False)
                                    for layer in range(num_layers)])
        self.dropout = float(dropout)
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()

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
        x = _feature_drop(x, p, relu=False)                              # site 0
        x0 = _feature_drop(self.lins[0](x), 0.0, relu=True).float()      # x0 = relu(lins[0](x)): no mask, no seed
        x = _feature_drop(x0, p, relu=False)                             # site 1
        for conv in self.convs:
            x = conv.run(x, x0, g, p_drop=p)                             # sites 2 .. L+1, behind each conv's ReLU
        return F.log_softmax(self.lins[1](x), dim=1)


def train_gcn2_noDTC(args, dataset, data, save=False, repeat=3, num_epoch=200, seed=None, num_layer=2, hidden=64, alpha=0.1,
                     theta=0.5, lr=1e-3, wd=5e-3, use_scheduler=True, step=1, step_size=100, gamma=0.1, metric='f1',
                     f1_average='macro', dropout=0.5, verbose=True, ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:302-396 on `GCN2(dataset, hidden, num_layer, alpha, theta)` (`step` is accepted and unused):
    the run of `transfer.train_gnn_noDTC` -- Adam(lr, wd), optional StepLR, best epoch by the lowest `loss_train` -- on this
    module's model.  `save=True` writes {ckpt_dir}/model_GCN2_{args.dataset_name}_share_best.ckpt.  Returns None like the reference;
    `history`, `dropout`, `verbose`, `ckpt_dir` as in `train_gnn_noDTC`; `graphed=True` raises NotImplementedError."""
    from .transfer import _train_plain_backbone
    if graphed:
        raise NotImplementedError("train_gcn2_noDTC(graphed=True): the GCN2 epoch is not offered as a HIP-graph replay; run it eagerly")
    return _train_plain_backbone(args, dataset, data, lambda: GCN2(dataset, hidden, num_layer, alpha, theta, dropout=dropout), 'GCN2',
                                 lambda model: len(model.convs) + 2 if dropout > 0 else 0, save, repeat, num_epoch, seed, lr, wd,
                                 use_scheduler, step_size, gamma, metric, f1_average, verbose, ckpt_dir, history, graphed)


def build_parser():
    """step 2's flags and defaults (`transfer.build_parser`) plus `--alpha`, `--theta` and `--dropout`; --model_name, --no_dtc and
    --baseline are accepted and ignored: this entry always trains GCN2 (--graphed is refused by the driver)"""
    from .transfer import _FLAGS
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.gcn2", description="Step 2 of Bridged-GNN with the GCNII baseline")
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=default, choices=choices, help=text)
    ap.add_argument("--alpha", type=float, default=0.1, help="initial-residual weight")
    ap.add_argument("--theta", type=float, default=0.5, help="identity-mapping strength: beta_l = log(theta / l + 1)")
    ap.add_argument("--dropout", type=float, default=0.5, help="dropout probability of every site")
    return ap


def main(args=None, verbose=True):
    """main_graph_knowledge_transfer.py:399-421 routed to `train_gcn2_noDTC`.  `args`: the parsed namespace, or a list of
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
        return train_gcn2_noDTC(args, dataset, data, save=args.save, repeat=1, num_epoch=args.num_epoch, seed=0,
                                num_layer=args.num_layer, hidden=args.hidden_dim, alpha=args.alpha, theta=args.theta, lr=1e-3,
                                wd=5e-3, use_scheduler=False, step=1, step_size=100, gamma=0.1, metric=args.eval_metric,
                                f1_average='macro', dropout=args.dropout, verbose=verbose, graphed=args.graphed)


if __name__ == '__main__':
    _args = build_parser().parse_args()
    print(_args)
    main(_args)
