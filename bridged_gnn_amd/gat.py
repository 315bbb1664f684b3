"""GAT on the HIP attention aggregation: the `gnn='GAT'` baseline of step 2 (main_graph_knowledge_transfer.py:327-328 ->
models/backbones.py:404-438).

Each conv is PyG's `GATConv(in, out, heads, concat, dropout=0.6)` of PyG 2.0-2.2 (one shared `lin_src` / `lin_dst`, additive
per-node scores): the transform comes first (T = x W^T, [N, H*C]), `ops.gat_scores` forms the per-node scores, and
`ops.gat_aggregate` runs the per-destination softmax, the attention dropout on the edge coefficients and the weighted sum over the
graph with exactly one self loop per node, with the ELU + dropout between the convs or the closing log_softmax fused into the same
pass.  The backward (`ops.gat_aggregate_bwd`) is atomic-free; it keeps x, T, the scores, the softmax state, the coefficients and
the conv output before the epilogue, and redraws both dropout masks from their seeds.

`train_gat_noDTC` is the reference's `train_gnn_noDTC(gnn='GAT')`; `python -m bridged_gnn_amd.gat` runs it with step 2's flags."""
import argparse
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .gcn import _pad_bias, _pad_rows, _transform
from .ktgnn import Linear, dropout_seed

__all__ = ["GATConv", "GAT", "GatGraph", "train_gat_noDTC", "build_parser", "main"]


class GatGraph:
    """What GAT walks, built once per graph: the by-destination CSR of edge_index with every self loop dropped and one appended per
    node (PyG `remove_self_loops` + `add_self_loops`; duplicate edges stay separate edges) and its by-source view for the
    backward.  No hub tables: a row of any degree is walked by one lane group."""

    def __init__(self, edge_index, num_nodes):
        self.num_nodes = N = int(num_nodes)
        self.csr = ops.build_dst_csr(edge_index.long().contiguous(), N, rewrite_self_loops=True)
        self.rowptr = self.csr.rowptr
        self.col = self.csr.col[: self.csr.num_edges]
        self.t_rowptr, self.t_eid, self.t_dst = self.csr.transposed()


def _aligned_rows(t, width):
    """t [N, >= width] as a float32 table the kernels take (unit column stride, rows and base 16-byte aligned, pad4(width) columns)"""
    W = ops.pad4(width)
    if t.dtype == torch.float32 and t.shape[1] >= W and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    out = torch.zeros(t.shape[0], W, dtype=torch.float32, device=t.device)
    out[:, :width] = t[:, :width]
    return out


def _conv_forward(x, wp, att_src, att_dst, bp, graph, cfg, seeds, keep):
    """-> (out, kept): kept = (T, s_src, s_dst, state, alpha, pre) when `keep` (what the backward reads), else None"""
    H, C, slope, p_att, epilogue, p_drop = cfg
    seed_att, seed_att_dev, seed, seed_dev = seeds
    T = _aligned_rows(_transform(x, wp), H * C)
    s_src, s_dst = ops.gat_scores(T, att_src, att_dst, H, C)
    out, state, pre, alpha = ops.gat_aggregate(T, s_src, s_dst, graph.rowptr, graph.col, graph.num_nodes, H, C, bias=bp,
                                               negative_slope=slope, p_att=p_att, seed_att=seed_att, seed_att_dev=seed_att_dev,
                                               epilogue=epilogue, p_drop=p_drop, seed=seed, seed_dev=seed_dev, want_pre=keep,
                                               return_alpha=keep)
    return out, ((T, s_src, s_dst, state, alpha, pre) if keep else None)


def _head_column_sums(Tv, ds, width):
    """sum_n ds[n,h] * Tv[n,h,:] -> [H, C] through the fixed-order fp64 column sums (no torch multi-block reduction)"""
    N, H, C = Tv.shape
    buf = torch.empty(N, width, dtype=torch.float32, device=Tv.device)
    if width != H * C:
        buf[:, H * C:] = 0
    torch.mul(Tv, ds.unsqueeze(-1), out=buf[:, :H * C].unflatten(1, (H, C)))
    return ops.column_sums(buf)[:H * C].view(H, C)


class _GatLayerFn(torch.autograd.Function):
    """out = epi(sum_t a~ T_j + b), T = x W^T, with hand-written backward: dT, ds_src, ds_dst and db from the aggregation backward,
    then dT += ds_src (x) att_src + ds_dst (x) att_dst, datt = sum_n ds * T, dW = dT^T x, dx = dT W."""

    @staticmethod
    def forward(ctx, x, w, att_src, att_dst, b, graph, cfg, seeds):
        H, C = cfg[0], cfg[1]
        wp = _pad_rows(w.detach())
        bp = _pad_bias(b.detach(), H * C) if b is not None else None
        out, kept = _conv_forward(x.detach(), wp, att_src.detach(), att_dst.detach(), bp, graph, cfg, seeds, True)
        ctx.save_for_backward(x, wp, att_src, att_dst)
        ctx.kept, ctx.bp, ctx.graph, ctx.cfg, ctx.seeds = kept, bp, graph, cfg, seeds
        return out[:, :H * C]

    @staticmethod
    def backward(ctx, gy):
        x, wp, att_src, att_dst = ctx.saved_tensors
        H, C, slope, p_att, epilogue, p_drop = ctx.cfg
        seed_att, seed_att_dev, seed, seed_dev = ctx.seeds
        T, s_src, s_dst, state, alpha, pre = ctx.kept
        graph = ctx.graph
        HC, W = H * C, ops.pad4(H * C)
        gy = _aligned_rows(gy, HC)
        dT, ds_src, ds_dst, gb = ops.gat_aggregate_bwd(T, s_src, s_dst, state, alpha, pre, gy, graph.rowptr, graph.col, graph.t_rowptr,
                                                       graph.t_eid, graph.t_dst, H, C, bias=ctx.bp, negative_slope=slope, p_att=p_att,
                                                       seed_att=seed_att, seed_att_dev=seed_att_dev, epilogue=epilogue, p_drop=p_drop,
                                                       seed=seed, seed_dev=seed_dev, want_bias=ctx.bp is not None)
        a_s, a_d = att_src.detach().reshape(1, H, C), att_dst.detach().reshape(1, H, C)
        Tv = T[:, :HC].unflatten(1, (H, C))
        g_as = _head_column_sums(Tv, ds_src, W).view(1, H, C)
        g_ad = _head_column_sums(Tv, ds_dst, W).view(1, H, C)
        dTv = dT[:, :HC].unflatten(1, (H, C))
        dTv.addcmul_(ds_src.unsqueeze(-1), a_s).addcmul_(ds_dst.unsqueeze(-1), a_d)
        xd = x.detach()
        if ops.gram_supported(W, xd.shape[1]) and xd.stride(1) == 1 and xd.stride(0) % 4 == 0 and xd.data_ptr() % 16 == 0:
            dW = ops.gram(dT, xd)
        else:
            dW = dT.t().mm(xd)
        gx = None
        if ctx.needs_input_grad[0]:
            din = x.shape[1]
            if ops.linear_supported(W, din):
                gx = ops.linear(dT, wp.t().contiguous(), torch.zeros(din, dtype=torch.float32, device=x.device))
            else:
                gx = dT.mm(wp)
        return gx, dW[:HC], g_as, g_ad, gb, None, None, None


class GATConv(nn.Module):
    """Stand-in for `torch_geometric.nn.GATConv` of PyG 2.0-2.2 as the reference builds it (backbones.py:407-418):
    out[i] = sum_j softmax_j(leaky_relu(<T_j, att_src> + <T_i, att_dst>)) T_j + b over the edges without self loops plus one self
    loop per node, T = lin_src(x) viewed [N, heads, out_channels]; attention dropout on the coefficients in training mode.
    State_dict keys and initial draws are PyG's: `lin_src` and `lin_dst` are ONE glorot Linear without bias under two names, drawn
    by Linear.__init__ and again twice by reset_parameters, then `att_src`, `att_dst` ([1, heads, out_channels], glorot), `bias`
    zeros ([heads * out_channels], or [out_channels] with concat=False)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 edge_dim=None, fill_value="mean", bias=True):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("GATConv: bipartite inputs (a pair of in_channels) are not implemented")
        if edge_dim is not None:
            raise NotImplementedError("GATConv: edge features (edge_dim) are not implemented")
        if not add_self_loops:
            raise NotImplementedError("GATConv: add_self_loops=False is not implemented")
        if not concat and heads != 1:
            raise NotImplementedError("GATConv: concat=False (the mean over heads) is implemented for heads == 1 only")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, int(heads), bool(concat)
        self.negative_slope, self.dropout, self.add_self_loops = float(negative_slope), float(dropout), True
        self.lin_src = Linear(in_channels, heads * out_channels, bias=False, weight_initializer="glorot")
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_src.reset_parameters()
        self.lin_dst.reset_parameters()          # the same module: PyG draws it again, and a seeded model keeps its draws
        for att in (self.att_src, self.att_dst):
            a = math.sqrt(6.0 / (att.size(-2) + att.size(-1)))
            nn.init.uniform_(att, -a, a)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def run(self, x, graph, epilogue=None, p_drop=0.0):
        """conv output with an optional fused epilogue ("elu" then dropout at p_drop, or "log_softmax"); graph: GatGraph."""
        if not x.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x.device} tensor)")
        H, C = self.heads, self.out_channels
        if not (1 <= H <= ops.GAT_MAX_HEADS and 1 <= C <= ops.GAT_MAX_C):
            raise RuntimeError(f"GATConv: unsupported shape: heads = {H}, out_channels = {C} (the HIP aggregation takes "
                               f"1 <= heads <= {ops.GAT_MAX_HEADS}, 1 <= out_channels <= {ops.GAT_MAX_C})")
        w, b = self.lin_src.weight, self.bias
        torch_epi = epilogue == "log_softmax" and H != 1
        kern_epi = None if torch_epi else epilogue
        p_att = self.dropout if self.training else 0.0
        kern_p = float(p_drop) if kern_epi == "elu" else 0.0
        seed_att, seed_att_dev = dropout_seed(p_att, step_word=False)      # a captured epoch: 0 and this site's device word
        seed, seed_dev = dropout_seed(kern_p, step_word=False)
        cfg = (H, C, self.negative_slope, float(p_att), kern_epi, kern_p)
        seeds = (seed_att, seed_att_dev, seed, seed_dev)
        x = x.float()
        params = (w, self.att_src, self.att_dst) + ((b,) if b is not None else ())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            out = _GatLayerFn.apply(x, w, self.att_src, self.att_dst, b, graph, cfg, seeds)
        else:
            out = _conv_forward(x, _pad_rows(w.detach()), self.att_src.detach(), self.att_dst.detach(),
                                _pad_bias(b.detach(), H * C) if b is not None else None, graph, cfg, seeds, False)[0][:, :H * C]
        if torch_epi:
            out = F.log_softmax(out, dim=1)
        return out

    def forward(self, x, edge_index):
        graph = edge_index if isinstance(edge_index, GatGraph) else GatGraph(edge_index, x.shape[0])
        return self.run(x, graph)


class GAT(nn.Module):
    """models/backbones.py:404-438 on the HIP attention aggregation.  Same constructor and state_dict keys (conv{1,2}.att_src,
    .att_dst, .bias, .lin_src.weight, .lin_dst.weight); `dropout` (default the reference's hard-coded 0.6) sets both the attention
    dropout of the two convs and the feature dropout between them, so tests can switch them off.  forward -> log-probabilities;
    get_emb -> elu(conv1) without the feature dropout, as in the reference.  The three dropout sites take their seeds in forward
    order: conv1's attention, the feature dropout, conv2's attention."""

    def __init__(self, dataset, hidden=16, head=8, dropout=0.6):
        super().__init__()
        self.dropout = float(dropout)
        self.conv1 = GATConv(dataset.num_features, hidden, heads=head, concat=True, dropout=self.dropout)
        self.conv2 = GATConv(hidden * head, dataset.num_classes, heads=1, concat=False, dropout=self.dropout)
        self._graph_key = None
        self._graph = None

    def reset_parameters(self):
        self.conv1.reset_parameters()
        self.conv2.reset_parameters()

    def graph(self, edge_index, num_nodes):
        """GatGraph of edge_index, cached against the tensor (identity, in-place version, shape) as `GCNNet.graph` does."""
        key = (edge_index._version, tuple(edge_index.shape), edge_index.data_ptr(), int(num_nodes))
        if self._graph is None or self._graph_key is None or self._graph_key[0] is not edge_index or self._graph_key[1] != key:
            self._graph = GatGraph(edge_index, num_nodes)
            self._graph_key = (edge_index, key)
        return self._graph

    def forward(self, data):
        g = self.graph(data.edge_index, data.x.shape[0])
        x = self.conv1.run(data.x, g, epilogue="elu", p_drop=self.dropout if self.training else 0.0)
        return self.conv2.run(x, g, epilogue="log_softmax")

    def get_emb(self, data):
        g = self.graph(data.edge_index, data.x.shape[0])
        return self.conv1.run(data.x, g, epilogue="elu", p_drop=0.0)


def train_gat_noDTC(args, dataset, data, save=False, repeat=3, num_epoch=200, seed=None, num_layer=2, hidden=64, head=3, lr=1e-3,
                    wd=5e-3, use_scheduler=True, step=1, step_size=100, gamma=0.1, metric='f1', f1_average='macro', dropout=0.6,
                    verbose=True, ckpt_dir='../ckpt', history=None, graphed=False):
    """main_graph_knowledge_transfer.py:302-396 with `gnn='GAT'` (:327-328: `GAT(dataset, hidden, head=3)`; `num_layer` and `step`
    are accepted and unused, as there): the run of `transfer.train_gnn_noDTC` -- Adam(lr, wd), optional StepLR, best epoch by the
    lowest `loss_train` -- on this module's `GAT`.  `save=True` writes {ckpt_dir}/model_GAT_{args.dataset_name}_share_best.ckpt.
    Returns None like the reference; `history`, `graphed`, `dropout`, `verbose`, `ckpt_dir` as in `train_gnn_noDTC`."""
    from .transfer import _train_plain_backbone
    return _train_plain_backbone(args, dataset, data, lambda: GAT(dataset, hidden, head=head, dropout=dropout), 'GAT',
                                 lambda model: 3 if dropout > 0 else 0, save, repeat, num_epoch, seed, lr, wd, use_scheduler, step_size,
                                 gamma, metric, f1_average, verbose, ckpt_dir, history, graphed)


def build_parser():
    """step 2's flags and defaults (`transfer.build_parser`) plus `--head`; --model_name, --no_dtc and --baseline are accepted and
    ignored: this entry always trains GAT"""
    from .transfer import _FLAGS
    ap = argparse.ArgumentParser(prog="python -m bridged_gnn_amd.gat", description="Step 2 of Bridged-GNN with the GAT baseline")
    for name, (typ, default, choices, text) in _FLAGS.items():
        if typ is None:
            ap.add_argument("--" + name, action="store_true", default=default, help=text)
        else:
            ap.add_argument("--" + name, type=typ, default=default, choices=choices, help=text)
    ap.add_argument("--head", type=int, default=3, help="attention heads of the first conv (the reference builds 3)")
    return ap


def main(args=None, verbose=True):
    """main_graph_knowledge_transfer.py:399-421 routed to `train_gat_noDTC`.  `args`: the parsed namespace, or a list of
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
        return train_gat_noDTC(args, dataset, data, save=args.save, repeat=1, num_epoch=args.num_epoch, seed=0,
                               num_layer=args.num_layer, hidden=args.hidden_dim, head=args.head, lr=1e-3, wd=5e-3, use_scheduler=False,
                               step=1, step_size=100, gamma=0.1, metric=args.eval_metric, f1_average='macro', verbose=verbose,
                               graphed=args.graphed)


if __name__ == '__main__':
    _args = build_parser().parse_args()
    print(_args)
    main(_args)
