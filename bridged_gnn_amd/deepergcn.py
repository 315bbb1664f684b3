"""DeeperGCN on the fused HIP softmax aggregation: the `DeeperGCN` baseline of the reference's zoo (models/backbones.py:130-161).

The model is node_encoder, then layers[0].conv alone, then `DeepGCNLayer(conv, norm, act, block='res+', dropout=0.1)` for every
further layer -- x + conv(dropout(relu(norm(x)))) -- and relu(layers[0].norm(x)) -> dropout(0.1) -> lin -> log_softmax.  Each conv
is PyG's `GENConv(H, H, aggr='softmax', t=1.0, learn_t=True, num_layers=2, norm='layer')` (PyG 2.0.x semantics):
    v_j = relu(x_j) + 1e-7,  alpha_ij = softmax_j(t * v_j) per destination i AND per channel,  z_i = sum_j alpha_ij v_j + x_i,
    out = mlp(z),  mlp = Linear(H, 2H) -> LayerNorm(2H) -> ReLU -> Dropout(0) -> Linear(2H, H)
over the edges exactly as given (`sage.SageGraph`: no self loop added or removed, duplicates are separate messages).
`ops.gen_softmax_aggregate` runs message, softmax, weighted sum and root add as one edge walk; in training it also stores
lse_i and o_i per row and channel, from which `ops.gen_softmax_aggregate_bwd` forms grad_x and grad_t in one walk over the
by-source view.  The temperature stays on the device.  The dense parts run on the library GEMM and `F.layer_norm`; every
ReLU -> dropout site is one `ops.feature_dropout(relu=True)` pass whose mask comes from a (seed, element index) hash, the seeds
taken in forward order through `ktgnn.dropout_seed`: one per res+ layer, then the closing one."""
import argparse

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .appnp import _feature_drop, _no_cpu, _rows4
from .ktgnn import Linear
from .sage import SageGraph

__all__ = ["GENConv", "DeepGCNLayer", "DeeperGCN", "train_deepergcn_noDTC"]


class _GenAggFn(torch.autograd.Function):
    """z = softmax-aggregate(x; t) + x with hand-written backward.  Kept: x, t and the forward's (lse, o) tables."""

    @staticmethod
    def forward(ctx, x, t, graph):
        H = x.shape[1]
        N = graph.num_nodes
        xr = _rows4(x.detach(), H)
        rowptr, col = graph.by_dst[0], graph.by_dst[1]
        lse, o = (torch.empty(N, ops.pad4(H), dtype=torch.float32, device=x.device) for _ in range(2))
        z = ops.gen_softmax_aggregate(xr, rowptr, col, t.detach(), N, H, save=(lse, o))
        ctx.save_for_backward(xr, t, lse, o)
        ctx.graph, ctx.H = graph, H
        return z[:, :H]

    @staticmethod
    def backward(ctx, gz):
        xr, t, lse, o = ctx.saved_tensors
        H = ctx.H
        t_rowptr, t_dst = ctx.graph.by_dst[2], ctx.graph.by_dst[3]
        gx, gt = ops.gen_softmax_aggregate_bwd(xr, _rows4(gz, H), (lse, o), t_rowptr, t_dst, t.detach(), H)
        return (gx[:, :H] if ctx.needs_input_grad[0] else None), (gt.reshape(t.shape) if ctx.needs_input_grad[1] else None), None


class GENConv(nn.Module):
    """Stand-in for `torch_geometric.nn.GENConv` as the reference builds it (backbones.py:138-139): softmax aggregation with a
    learnable temperature `t` ([1]), then `mlp` = Linear(in, 2 in) -> LayerNorm(2 in) -> ReLU -> Dropout(0) -> Linear(2 in, out);
    state_dict keys t, mlp.0.*, mlp.1.*, mlp.4.*.  Everything else of PyG's layer -- another `aggr`, `msg_norm`, `learn_p`,
    `learn_t=False`, another `norm`, depth or eps, edge attributes -- raises NotImplementedError."""

    def __init__(self, in_channels, out_channels, aggr='softmax', t=1.0, learn_t=False, p=1.0, learn_p=False, msg_norm=False,
                 learn_msg_scale=False, norm='batch', num_layers=2, eps=1e-7):
        super().__init__()
        if aggr != 'softmax':
            raise NotImplementedError(f"GENConv: only aggr='softmax' is implemented, got {aggr!r}")
        if msg_norm or learn_msg_scale or learn_p:
            raise NotImplementedError("GENConv: msg_norm, learn_msg_scale and learn_p are not implemented (the reference sets none)")
        if not learn_t or norm != 'layer' or num_layers != 2 or eps != 1e-7:
            raise NotImplementedError("GENConv: only learn_t=True, norm='layer', num_layers=2 and eps=1e-7 are implemented")
        self.in_channels, self.out_channels, self.aggr, self.eps = int(in_channels), int(out_channels), aggr, eps
        self.initial_t = float(t)
        hid = 2 * self.in_channels
        self.mlp = nn.Sequential(nn.Linear(self.in_channels, hid), nn.LayerNorm(hid, elementwise_affine=True), nn.ReLU(),
                                 nn.Dropout(0.0), nn.Linear(hid, self.out_channels))
        self.t = nn.Parameter(torch.empty(1))
        self.reset_parameters()

    def reset_parameters(self):
        for m in self.mlp:
            if hasattr(m, "reset_parameters"):
                m.reset_parameters()
        with torch.no_grad():
            self.t.fill_(self.initial_t)

    def aggregate(self, x, graph):
        """z = sum_j alpha_ij v_j + x_i over a `SageGraph`: [N, in_channels]"""
        H = self.in_channels
        if torch.is_grad_enabled() and (x.requires_grad or self.t.requires_grad):
            return _GenAggFn.apply(x, self.t, graph)
        return ops.gen_softmax_aggregate(_rows4(x.detach(), H), graph.by_dst[0], graph.by_dst[1], self.t.detach(), graph.num_nodes, H)[:, :H]

    def forward(self, x, edge_index, edge_attr=None, size=None):
        if edge_attr is not None or size is not None:
            raise NotImplementedError("GENConv: edge attributes and bipartite sizes are not implemented (the reference passes none)")
        _no_cpu(x)
        if x.shape[1] != self.in_channels:
            raise ValueError(f"GENConv: x must have {self.in_channels} columns, got {x.shape[1]}")
        graph = edge_index if isinstance(edge_index, SageGraph) else SageGraph(edge_index, x.shape[0])
        z = self.aggregate(x.float(), graph)
        h = F.layer_norm(self.mlp[0](z), self.mlp[1].normalized_shape, self.mlp[1].weight, self.mlp[1].bias, self.mlp[1].eps)
        return self.mlp[4](_feature_drop(h, 0.0, relu=True))       # mlp.2 / mlp.3: ReLU, Dropout(0)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, aggr={self.aggr}"


class DeepGCNLayer(nn.Module):
    """Stand-in for `torch_geometric.nn.DeepGCNLayer` with block='res+': x + conv(dropout(act(norm(x)))).  `act` is None or
    nn.ReLU (it runs fused with the dropout); `ckpt_grad` only trades memory for recomputation and is accepted and ignored."""

    def __init__(self, conv=None, norm=None, act=None, block='res+', dropout=0.0, ckpt_grad=False):
        super().__init__()
        if block != 'res+':
            raise NotImplementedError(f"DeepGCNLayer: only block='res+' is implemented, got {block!r}")
        if act is not None and not isinstance(act, nn.ReLU):
            raise NotImplementedError("DeepGCNLayer: only act=None or nn.ReLU is implemented")
        self.conv, self.norm, self.act = conv, norm, act
        self.block, self.dropout, self.ckpt_grad = block, float(dropout), ckpt_grad

    def reset_parameters(self):
        self.conv.reset_parameters()
        if self.norm is not None:
            self.norm.reset_parameters()

    def forward(self, x, edge_index, *args, **kwargs):
        _no_cpu(x)
        h = x if self.norm is None else self.norm(x)
        h = _feature_drop(h, self.dropout if self.training else 0.0, relu=self.act is not None)
        return x + self.conv(h, edge_index, *args, **kwargs)

    def extra_repr(self):
        return f"block={self.block}, dropout={self.dropout}"


class DeeperGCN(nn.Module):
    """models/backbones.py:130-161 on the HIP softmax aggregation.  Same members and state_dict keys (node_encoder.*,
    layers.{i}.conv.{t, mlp.0.*, mlp.1.*, mlp.4.*}, layers.{i}.norm.*, lin.*), parameters drawn in the reference's order;
    `dropout` (default the reference's hard-coded 0.1) sets every site.  forward -> log-probabilities.  Layer 0 contributes its
    conv at the front and its norm at the end, as in the reference.  Dropout sites in forward order: one per layer of
    layers[1:], then the one in front of `lin`."""

    def __init__(self, dataset, hidden_channels, num_layers, dropout=0.1):
        super().__init__()
        self.dropout = float(dropout)
        self.node_encoder = Linear(dataset.num_features, hidden_channels)
        self.layers = nn.ModuleList()
        for i in range(1, num_layers + 1):
            conv = GENConv(hidden_channels, hidden_channels, aggr='softmax', t=1.0, learn_t=True, num_layers=2, norm='layer')
            norm = nn.LayerNorm(hidden_channels, elementwise_affine=True)
            act = nn.ReLU(inplace=True)
            self.layers.append(DeepGCNLayer(conv, norm, act, block='res+', dropout=self.dropout, ckpt_grad=i % 3))
        self.lin = Linear(hidden_channels, dataset.num_classes)
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        self.node_encoder.reset_parameters()
        for layer in self.layers:
            layer.reset_parameters()
        self.lin.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """SageGraph of edge_index, cached against the tensor (identity, in-place version, shape) as `GCNNet.graph` does."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = SageGraph(edge_index, num_nodes)
            self._graph_key = (edge_index, key)
        return self._graph

    def forward(self, data):
        x = data.x
        _no_cpu(x)
        g = self.graph(data.edge_index, x.shape[0])
        x = self.node_encoder(x)
        x = self.layers[0].conv(x, g)
        for layer in self.layers[1:]:
            x = layer(x, g)
        x = _feature_drop(self.layers[0].norm(x), self.dropout if self.training else 0.0, relu=True)
        return F.log_softmax(self.lin(x), dim=1)


def train_deepergcn_noDTC(args, dataset, data, save=False, repeat=3, num_epoch=200, seed=None, num_layer=3, hidden=64, lr=1e-3,
                          wd=5e-3, use_scheduler=True, step=1, step_size=100, gamma=0.1, metric='f1', f1_average='macro', dropout=0.1,
                          verbose=True, ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:302-396 on `DeeperGCN(dataset, hidden, num_layer)` (`step` is accepted and unused): the run of
    `transfer.train_gnn_noDTC` -- Adam(lr, wd), optional StepLR, best epoch by the lowest `loss_train` -- on this module's model.
    `save=True` writes {ckpt_dir}/model_DeeperGCN_{args.dataset_name}_share_best.ckpt.  Returns None like the reference; `history`,
    `dropout`, `verbose`, `ckpt_dir` as in `train_gnn_noDTC`; `graphed=True` raises NotImplementedError."""
    from .transfer import _train_plain_backbone
    if graphed:
        raise NotImplementedError("train_deepergcn_noDTC(graphed=True): the DeeperGCN epoch is not offered as a HIP-graph replay; run it eagerly")
    return _train_plain_backbone(args, dataset, data, lambda: DeeperGCN(dataset, hidden, num_layer, dropout=dropout), 'DeeperGCN',
                                 lambda model: len(model.layers) if dropout > 0 else 0, save, repeat, num_epoch, seed, lr, wd,
                                 use_scheduler, step_size, gamma, metric, f1_average, verbose, ckpt_dir, history, graphed)


def build_parser():
    """step 2's flags and defaults (`transfer.build_parser`) with --num_layer 3 and --hidden_dim 64, plus `--dropout`; --model_name,
    --no_dtc and --baseline are accepted and ignored: this entry always trains DeeperGCN (--graphed is refused by the driver)"""
    from .transfer import _FLAGS
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.deepergcn", description="Step 2 of Bridged-GNN with the DeeperGCN baseline")
    own = {"num_layer": 3, "hidden_dim": 64}
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=own.get(name, default), choices=choices, help=text)
    ap.add_argument("--dropout", type=float, default=0.1, help="dropout probability of every site")
    return ap


def main(args=None, verbose=True):
    """main_graph_knowledge_transfer.py:399-421 routed to `train_deepergcn_noDTC`.  `args`: the parsed namespace, or a list of
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
        return train_deepergcn_noDTC(args, dataset, data, save=args.save, repeat=1, num_epoch=args.num_epoch, seed=0,
                                     num_layer=args.num_layer, hidden=args.hidden_dim, lr=1e-3, wd=5e-3, use_scheduler=False, step=1,
                                     step_size=100, gamma=0.1, metric=args.eval_metric, f1_average='macro', dropout=args.dropout,
                                     verbose=verbose, graphed=args.graphed)


if __name__ == '__main__':
    _args = build_parser().parse_args()
    print(_args)
    main(_args)
