"""JKNet on the fused HIP convs and jumping-knowledge head: the `JKNet` baseline of the reference's zoo (models/backbones.py:60-107).

The model is `num_layers` PyG `GCNConv(…, cached=False)` layers, EVERY one followed by ReLU + dropout, whose outputs meet in
`JumpingKnowledge(cat | max)`, a Linear and log_softmax.  The reference does not hand its convs the edges: it builds
`adj_t_cache = gcn_norm(SparseTensor(row=dst, col=src, value=1))` once and passes that, and GCNConv (normalize=True, no cache,
SparseTensor branch) runs `gcn_norm` AGAIN on the already normalised, now weighted matrix; `fill_diag` replaces the diagonal with 1 a
second time.  With m_ij the multiplicity of edge j -> i (self loops dropped), d_i = 1 + sum_{j != i} m_ij and dinv = d^-1/2 (the
operator of `gcn.GcnGraph`), the second pass gives d2_i = 1 + dinv_i * sum_{j != i} m_ij dinv_j and the convs apply
    A2_ij = s_i s_j m_ij  (j != i),  s_i = dinv_i * d2_i^-1/2;        A2_ii = 1 / d2_i   (not s_i^2).
The off-diagonal part is a product form, the diagonal is not, so `ops.gcn_aggregate` (self loop = an ordinary edge of weight
dinv_i^2) cannot express it: `ops.jk_gcn_aggregate` walks the loop-free CSR with two [N] arrays, s and w = 1 / d2.

Layer l is `gcn._transform` and then `ops.jk_gcn_aggregate(..., out=slice l)` of ONE layer buffer [N, L * pad4(H)]: no cat or
stack exists in the eval or the training forward.  The head (`ops.jk_head`) forms the jumped row in registers, multiplies it by the
Linear's weight held in LDS and applies the log_softmax; outside its envelope (`ops.jk_head_supported`) the module composes it
from torch.  Backwards are hand-written autograd Functions; layer l's output feeds layer l + 1 and the head, autograd sums the
two gradients; ReLU and dropout states come from the forward's own output."""
import argparse

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .appnp import _no_cpu
from .gcn import GCNConv, _pad_bias, _pad_rows, _transform
from .ktgnn import Linear, dropout_seed

__all__ = ["JKGraph", "JumpingKnowledge", "JKNet", "train_jknet_noDTC"]


class JKGraph:
    """What JKNet walks, built once per graph: the by-destination CSR of edge_index with every self loop dropped and NONE appended
    (duplicate edges keep their multiplicity), its by-source view, and the two scale arrays of `ops.jk_gcn_aggregate`, formed in
    fp64 on the device and rounded once to fp32 (as `GcnGraph.dinv`).  renormalize=True: the reference's twice-normalised operator
    (module docstring); renormalize=False: the textbook single normalisation, s = dinv, w = dinv^2.
    `ops.build_dst_csr` either keeps the loops as edges or rewrites them to one per node, so the loops are removed with torch ops
    first and the CSR is built with rewrite_self_loops=False."""

    def __init__(self, edge_index, num_nodes, renormalize=True):
        self.num_nodes = N = int(num_nodes)
        self.renormalize = bool(renormalize)
        ei = edge_index.long()
        ei = ei[:, ei[0] != ei[1]].contiguous()
        self.csr = ops.build_dst_csr(ei, N, rewrite_self_loops=False)
        self.rowptr = self.csr.rowptr
        self.col = self.csr.col[: self.csr.num_edges]
        self.t_rowptr, _, self.t_dst = self.csr.transposed()
        s, w = JKGraph.scales(self.rowptr[:N + 1].long(), self.col.long(), self.renormalize)
        self.s, self.w = s.float().contiguous(), w.float().contiguous()

    @staticmethod
    def scales(rowptr, col, renormalize=True):
        """(s, w) in fp64 from the loop-free by-destination CSR (int64 rowptr [N + 1], col [E]).  The row sums of dinv[col] are
        differences of one fp64 prefix sum: a fixed order, the same bits on every run."""
        deg = (rowptr[1:] - rowptr[:-1]).double()
        dinv = (1.0 + deg).rsqrt()
        if not renormalize:
            return dinv, dinv * dinv
        pre = torch.zeros(col.shape[0] + 1, dtype=torch.float64, device=col.device)
        pre[1:] = torch.cumsum(dinv[col], 0)
        d2 = 1.0 + dinv * (pre[rowptr[1:]] - pre[rowptr[:-1]])
        return dinv * d2.rsqrt(), 1.0 / d2


class JumpingKnowledge(nn.Module):
    """Stand-in for `torch_geometric.nn.JumpingKnowledge` as the reference builds it (backbones.py:71): 'cat' concatenates the layer
    outputs, 'max' takes their elementwise maximum; neither has parameters, as in PyG.  mode='lstm' raises NotImplementedError.
    `forward(xs)` on a list of tensors gives torch's result through torch; inside `JKNet` the jump is part of the fused head."""

    def __init__(self, mode, channels=None, num_layers=None):
        super().__init__()
        self.mode = str(mode).lower()
        if self.mode == "lstm":
            raise NotImplementedError("JumpingKnowledge(mode='lstm'): the lstm jump is a per-node bidirectional LSTM over the layer "
                                      "outputs with no sparse path; it is not part of this package (modes: 'cat', 'max')")
        if self.mode not in ("cat", "max"):
            raise ValueError(f"JumpingKnowledge: mode must be 'cat' or 'max', got {mode!r}")
        self.channels, self.num_layers = channels, num_layers

    def reset_parameters(self):
        pass

    def forward(self, xs):
        xs = list(xs)
        if self.mode == "cat":
            return torch.cat(xs, dim=-1)
        return torch.stack(xs, dim=-1).max(dim=-1)[0]

    def extra_repr(self):
        return self.mode


def _layer_forward(x, wp, bp, D, graph, out, p_drop, seed, seed_dev=None):
    T = _transform(x, wp)
    return ops.jk_gcn_aggregate(T, graph.rowptr, graph.col, graph.s, graph.w, graph.num_nodes, D, bias=bp, epilogue="relu",
                                p_drop=p_drop, seed=seed, seed_dev=seed_dev, out=out)


class _JkLayerFn(torch.autograd.Function):
    """slice of the layer buffer = dropout(relu(A2 x W^T + b)) with hand-written backward: dT and db from the aggregation backward,
    dW = dT^T x, dx = dT W.  Only x, the padded weight and the output slice are kept."""

    @staticmethod
    def forward(ctx, x, w, b, graph, buf, lo, p_drop, seed, seed_dev=None):
        D = w.shape[0]
        wp = _pad_rows(w.detach())
        y = buf.detach()[:, lo:lo + ops.pad4(D)]
        _layer_forward(x.detach(), wp, _pad_bias(b.detach(), D) if b is not None else None, D, graph, y, p_drop, seed, seed_dev)
        ctx.save_for_backward(x, wp)
        ctx.y, ctx.graph, ctx.cfg = y, graph, (D, p_drop, b is not None)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wp = ctx.saved_tensors
        D, p_drop, has_b = ctx.cfg
        y, graph = ctx.y, ctx.graph
        N, Dp = x.shape[0], ops.pad4(D)
        if Dp != D or gy.dtype != torch.float32 or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            g = torch.zeros(N, Dp, dtype=torch.float32, device=gy.device)
            g[:, :D] = gy
            gy = g
        dT, gb = ops.jk_gcn_aggregate_bwd(y, gy, graph.t_rowptr, graph.t_dst, graph.s, graph.w, N, D, epilogue="relu", p_drop=p_drop,
                                          want_bias=has_b and ctx.needs_input_grad[2])
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
        return gx, dW, gb, None, None, None, None, None, None


class _JkHeadFn(torch.autograd.Function):
    """log_softmax(jump(layers) W^T + b) over the layer buffer.  The layer outputs `ys` are the autograd inputs (views of the
    buffer the kernel reads); their gradients are the column blocks of dJ (cat) or the routing pass's slices (max)."""

    @staticmethod
    def forward(ctx, buf, L, H, mode, w, b, *ys):
        C = w.shape[0]
        wp = ops.jk_pack_weight(w, L, H, mode)
        out, win, jump = ops.jk_head(buf.detach(), L, H, mode, wp, b.detach().contiguous() if b is not None else None, C,
                                     log_softmax=True, want_state=True)
        ctx.state = (buf.detach(), wp, out, win, jump)
        ctx.cfg = (L, H, mode, C, b is not None)
        return out[:, :C]

    @staticmethod
    def backward(ctx, gy):
        buf, wp, out, win, jump = ctx.state
        L, H, mode, C, has_b = ctx.cfg
        N, Cp, Hp = buf.shape[0], ops.pad4(C), ops.pad4(H)
        if Cp != C or gy.dtype != torch.float32 or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            g = torch.zeros(N, Cp, dtype=torch.float32, device=gy.device)
            g[:, :C] = gy
            gy = g
        want_x = any(ctx.needs_input_grad[6:])
        gx, gwp, gb = ops.jk_head_bwd(buf, L, H, mode, wp, C, out, gy, log_softmax=True, win=win, jump=jump, want_x=want_x)
        nl = L if mode == "cat" else 1
        gw = gwp.reshape(C, nl, Hp)[:, :, :H].reshape(C, nl * H) if ctx.needs_input_grad[4] else None
        gys = tuple(gx[:, l * Hp:l * Hp + H] if want_x and ctx.needs_input_grad[6 + l] else None for l in range(L))
        return (None, None, None, None, gw, gb if has_b and ctx.needs_input_grad[5] else None) + gys


class JKNet(nn.Module):
    """models/backbones.py:60-107 on the HIP convs and head.  The reference's constructor arguments, parameters drawn in its order
    (each GCNConv draws `lin` twice, as PyG does; the jump has none; then `lin`), state_dict keys convs.{i}.lin.weight,
    convs.{i}.bias, lin.weight, lin.bias.  `renormalize=True` is the reference's twice-normalised operator, False the textbook GCN
    operator (module docstring).  forward -> log-probabilities.  Every conv is followed by ReLU and dropout, the last one included:
    `num_layers` dropout sites in forward order.
    The graph is cached against the `edge_index` tensor (identity, in-place version, shape), as `GCNNet.graph`; the reference never
    invalidates its `adj_t_cache`, so a second graph handed to the same reference model is silently walked as the first."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout, mode='cat', renormalize=True):
        super().__init__()
        if num_layers < 1:
            raise ValueError(f"JKNet: num_layers must be >= 1, got {num_layers}")
        self.convs = nn.ModuleList()
        self.convs.append(GCNConv(in_channels, hidden_channels, cached=False))
        for _ in range(num_layers - 1):
            self.convs.append(GCNConv(hidden_channels, hidden_channels, cached=False))
        self.jump = JumpingKnowledge(mode=mode, channels=hidden_channels, num_layers=num_layers)
        self.mode = self.jump.mode
        if self.mode == 'cat':
            self.lin = Linear(num_layers * hidden_channels, out_channels)
        else:
            self.lin = Linear(hidden_channels, out_channels)
        self.dropout = float(dropout)
        self.hidden_channels, self.out_channels, self.num_layers = int(hidden_channels), int(out_channels), int(num_layers)
        self.renormalize = bool(renormalize)
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        self.jump.reset_parameters()
        self.lin.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """JKGraph of edge_index, cached against the tensor (identity, in-place version, shape) as `GCNNet.graph` does."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = JKGraph(edge_index, num_nodes, self.renormalize)
            self._graph_key = (edge_index, key)
        return self._graph

    def forward(self, data):
        x = data.x
        _no_cpu(x)
        x = x.float()
        g = self.graph(data.edge_index, x.shape[0])
        N, L, H, C = x.shape[0], self.num_layers, self.hidden_channels, self.out_channels
        Hp = ops.pad4(H)
        p = self.dropout if self.training else 0.0
        buf = torch.empty(N, L * Hp, dtype=torch.float32, device=x.device)    # every slice is written whole, pad columns as 0
        grad = torch.is_grad_enabled()
        ys = []
        for l, conv in enumerate(self.convs):
            w, b = conv.lin.weight, conv.bias
            seed, seed_dev = dropout_seed(p, step_word=False)
            if grad and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)):
                x = _JkLayerFn.apply(x, w, b, g, buf, l * Hp, float(p), seed, seed_dev)
            else:
                out = buf[:, l * Hp:(l + 1) * Hp]
                _layer_forward(x, _pad_rows(w.detach()), _pad_bias(b.detach(), H) if b is not None else None, H, g, out, float(p),
                               seed, seed_dev)
                x = out[:, :H]
            ys.append(x)
        w, b = self.lin.weight, self.lin.bias
        if not ops.jk_head_supported(L, H, C, self.mode):
            # outside the head's envelope: the composition from torch (autograd follows it)
            return F.log_softmax(torch.addmm(b, self.jump(ys), w.t()), dim=-1)
        if grad and (w.requires_grad or b.requires_grad or any(y.requires_grad for y in ys)):
            return _JkHeadFn.apply(buf, L, H, self.mode, w, b, *ys)
        return ops.jk_head(buf, L, H, self.mode, ops.jk_pack_weight(w, L, H, self.mode), b.detach().contiguous(), C)[:, :C]


def train_jknet_noDTC(args, dataset, data, save=False, repeat=3, num_epoch=200, seed=None, num_layer=2, hidden=64, lr=1e-3, wd=5e-3,
                      use_scheduler=True, step=1, step_size=100, gamma=0.1, metric='f1', f1_average='macro', dropout=0.5, mode='cat',
                      renormalize=True, verbose=True, ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:302-396 on `JKNet(F, hidden, C, num_layer, dropout, mode)` (`step` is accepted and unused):
    the run of `transfer.train_gnn_noDTC` -- Adam(lr, wd), optional StepLR, best epoch by the lowest `loss_train` -- on this module's
    model.  `save=True` writes {ckpt_dir}/model_JKNet_{args.dataset_name}_share_best.ckpt.  Returns None like the reference;
    `history`, `verbose`, `ckpt_dir` as in `train_gnn_noDTC`; `graphed=True` raises NotImplementedError."""
    from .transfer import _train_plain_backbone
    if graphed:
        raise NotImplementedError("train_jknet_noDTC(graphed=True): the JKNet epoch is not offered as a HIP-graph replay; run it "
                                  "eagerly")
    return _train_plain_backbone(args, dataset, data,
                                 lambda: JKNet(dataset.num_features, hidden, dataset.num_classes, num_layer, dropout, mode=mode,
                                               renormalize=renormalize),
                                 'JKNet', lambda model: len(model.convs) if dropout > 0 else 0, save, repeat, num_epoch, seed, lr, wd,
                                 use_scheduler, step_size, gamma, metric, f1_average, verbose, ckpt_dir, history, graphed)


def build_parser():
    """step 2's flags and defaults (`transfer.build_parser`) with --num_layer 2 and --hidden_dim 64, plus `--dropout`, `--mode` and
    `--no_renormalize`; --model_name, --no_dtc and --baseline are accepted and ignored: this entry always trains JKNet (--graphed is
    refused by the driver)"""
    from .transfer import _FLAGS
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.jknet", description="Step 2 of Bridged-GNN with the JKNet baseline")
    own = {"num_layer": 2, "hidden_dim": 64}
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=own.get(name, default), choices=choices, help=text)
    ap.add_argument("--dropout", type=float, default=0.5, help="dropout probability after every conv")
    ap.add_argument("--mode", type=str, default="cat", choices=("cat", "max"), help="jumping-knowledge mode")
    ap.add_argument("--no_renormalize", action="store_true", default=False,
                    help="the textbook GCN operator instead of the reference's twice-normalised one")
    return ap


def main(args=None, verbose=True):
    """main_graph_knowledge_transfer.py:399-421 routed to `train_jknet_noDTC`.  `args`: the parsed namespace, or a list of
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
        return train_jknet_noDTC(args, dataset, data, save=args.save, repeat=1, num_epoch=args.num_epoch, seed=0,
                                 num_layer=args.num_layer, hidden=args.hidden_dim, lr=1e-3, wd=5e-3, use_scheduler=False, step=1,
                                 step_size=100, gamma=0.1, metric=args.eval_metric, f1_average='macro', dropout=args.dropout,
                                 mode=args.mode, renormalize=not args.no_renormalize, verbose=verbose, graphed=args.graphed)


if __name__ == '__main__':
    _args = build_parser().parse_args()
    print(_args)
    main(_args)
