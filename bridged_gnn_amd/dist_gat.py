"""GAT (the `gnn='GAT'` baseline, `gat.GAT`, reference models/backbones.py:404-438) on a destination-node partition: evaluation
and the training step, one process per GPU; new -- the reference is single-device.

Rank r owns a block of rows and all their in-edges of A' + I (`dist.PartitionPlan` with ONE table and rewrite_self_loops: every
input self loop dropped, one added per node as the LAST edge of its row, duplicate edges kept in input order -- the `GatGraph`
contract, and the order of the whole graph's CSR inside every row).  Its graph is "extended": the owned rows followed by one slot
per halo node (a remote source of an owned row), made square by giving the halo slots no in-edges.  Every conv runs
transform-first as on one GPU (T = x W^T, [., H*C]), so what crosses ranks is OUTPUT-width: pad4(H*C) floats per row.
  * scores: `ops.gat_scores` runs over the extended table -- the fixed-order kernel the owner of a halo row runs on the same row,
    so s_src of a halo slot needs no exchange; s_dst is its first n_local rows;
  * conv 0 reads the graph's input features: their halo rows stay resident (fetched once per version of x), the rank transforms
    its own and its halo rows and aggregates with no exchange; the halo rows' share of the weight gradient is this rank's;
  * conv 1 transforms the own rows, packs the send rows (`ops.gather_rows`) and does ONE all_to_all; backward walks the by-source
    view over all n_ext sources (`ops.gat_aggregate_bwd` with n_rows = n_local), adds ds_src (x) att_src into every extended row
    of dT, sends the halo part of dT back (the reverse exchange) and the owner folds it into its own dT rows with
    `ops.rows_segment_add` (no atomics, deterministic); att_src's gradient is summed over the extended rows (a halo slot holds
    this rank's share of ds_src of that node), att_dst's over the owned rows: the ranks' sums add up under `sync_grads`;
  * dropout: the seeds are drawn exactly as `GATConv.run` draws them (`ktgnn.dropout_seed`: per conv the attention seed, then
    the epilogue's) and the kernels hash the whole graph's positions: the feature mask at (GLOBAL row id) * (H*C) + column
    (`row_ids`), the attention mask at (GLOBAL edge position) * H + head (`edge_base`: where the row's first edge sits in the
    whole graph's by-destination CSR), in the forward and where the backward redraws them; every rank draws the single-GPU masks
    (`row_id_opt` / `edge_base_opt` of the one entry each, bgnn_gat_aggregate_f32 and bgnn_gat_aggregate_bwd_f32, ABI 116);
  * the loss is a sum over the owned rows with the GLOBAL normaliser (`nll_loss`); parameter gradients are summed in ONE
    bucketed all-reduce (`sync_grads`).
`get_emb` is supported (conv 0 alone: no exchange).  The host pieces (`GatPartition`, `_GatTables`) carry nothing of GAT's
scoring: an attention conv with another score over the same graph contract can take them as they are."""
import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .dist_sage import SagePartition, _dx, _gram_dw, _Layer, _RankModel
from .dist_train import _Comm
from .gat import _aligned_rows, _head_column_sums
from .gcn import _pad_bias, _pad_rows, _transform
from .ktgnn import dropout_seed

__all__ = ["GatPartition", "PartitionedGAT"]


class GatPartition(SagePartition):
    """Host side (numpy, device agnostic) of one rank's partition for an attention conv -- built identically on every rank, no
    communication.  `SagePartition`'s fields over the edges of A' + I (exactly one self loop per owned row, the last edge of its
    row; the other edges of a row in input order), and
        edge_base [n_local] int64     position of the first edge of every owned row in the WHOLE graph's by-destination CSR
    The device CSR (stable sort by destination, the self loop appended last) and `PartitionPlan` keep the same order inside a row,
    so edge k of owned row i is edge edge_base[i] + k of the whole graph: the element the attention dropout is hashed at."""

    def __init__(self, edge_index, num_nodes, rank, world, owner=None):
        ei = np.asarray(edge_index, dtype=np.int64)
        super().__init__(ei, num_nodes, rank, world, owner=owner, rewrite_self_loops=True)
        deg = np.bincount(ei[1][ei[0] != ei[1]], minlength=self.N).astype(np.int64) + 1      # non-loop in-edges + the self loop
        first = np.concatenate([[0], np.cumsum(deg)[:-1]]) if self.N else np.zeros(0, dtype=np.int64)
        self.edge_base = np.ascontiguousarray(first[self.owned_global], dtype=np.int64)


class _GatTables(_Layer):
    """device tables of one rank shared by every conv: `dist_sage._Layer`'s, the by-source view's edge positions (t_eid, which
    `_Layer` drops) and edge_base"""

    def __init__(self, part, device):
        super().__init__(part, device)
        E = part.num_edges                                 # the attention wrappers take the edge arrays at their exact length
        self.col, self.t_dst = self.col[:E], self.t_dst[:E]
        self.t_eid = self.csr.transposed()[1]
        self.edge_base = torch.from_numpy(part.edge_base).to(device)


def _conv_forward(ps, x, wp, att_src, att_dst, bp, resident, cfg, seeds, keep):
    """one conv on this rank's rows -> (out [n_local, pad4(H*C)], kept).  resident: x already holds the halo rows ([n_ext, Din],
    conv 0); else x is [n_local, Din] and the T rows of the halo come through one all_to_all.  kept = (T over the extended rows,
    s_src, s_dst, state, alpha, pre) when `keep` (what the backward reads), else None."""
    H, C, slope, p_att, epilogue, p_drop = cfg
    seed_att, seed_att_dev, seed, seed_dev = seeds
    part, g = ps.part, ps.tables
    T = _aligned_rows(_transform(x, wp), H * C)
    if not resident:
        halo = ps.halo_rows(T)
        if part.n_halo:
            T = torch.cat((T, halo))
    s_src, s_dst = ops.gat_scores(T, att_src, att_dst, H, C)
    s_dst = s_dst[:part.n_local]
    masked = p_att > 0 or p_drop > 0
    out, state, pre, alpha = ops.gat_aggregate(T, s_src, s_dst, g.rowptr_local, g.col, part.n_local, H, C, bias=bp,
                                               negative_slope=slope, p_att=p_att, seed_att=seed_att, seed_att_dev=seed_att_dev,
                                               epilogue=epilogue, p_drop=p_drop, seed=seed, seed_dev=seed_dev, want_pre=keep,
                                               return_alpha=keep, row_ids=g.owned_global if masked else None,
                                               edge_base=g.edge_base if masked else None)
    return out, ((T, s_src, s_dst, state, alpha, pre) if keep else None)


class _PartGatLayerFn(torch.autograd.Function):
    """one conv of the partitioned model with its hand-written backward (the partitioned form of `gat._GatLayerFn`): dT, ds_src
    (both over the extended rows), ds_dst and db from `gat_aggregate_bwd`, dT += ds_src (x) att_src + ds_dst (x) att_dst, the att
    gradients from the rank's rows, the halo part of dT returned to the owners and folded in (conv 1), then dW = dT^T x and
    dx = dT W."""

    @staticmethod
    def forward(ctx, x, w, att_src, att_dst, b, ps, resident, cfg, seeds):
        H, C = cfg[0], cfg[1]
        wp = _pad_rows(w.detach())
        bp = _pad_bias(b.detach(), H * C) if b is not None else None
        xd = x.detach()
        out, kept = _conv_forward(ps, xd, wp, att_src.detach(), att_dst.detach(), bp, resident, cfg, seeds, True)
        ctx.save_for_backward(xd, wp, att_src, att_dst)
        ctx.kept, ctx.bp, ctx.ps, ctx.resident, ctx.cfg, ctx.seeds = kept, bp, ps, resident, cfg, seeds
        return out[:, :H * C]

    @staticmethod
    def backward(ctx, gy):
        x, wp, att_src, att_dst = ctx.saved_tensors
        H, C, slope, p_att, epilogue, p_drop = ctx.cfg
        seed_att, seed_att_dev, seed, seed_dev = ctx.seeds
        T, s_src, s_dst, state, alpha, pre = ctx.kept
        ps, resident = ctx.ps, ctx.resident
        part, g = ps.part, ps.tables
        nl, HC, W = part.n_local, H * C, ops.pad4(H * C)
        masked = p_att > 0 or p_drop > 0
        gy = _aligned_rows(gy, HC)
        dT, ds_src, ds_dst, gb = ops.gat_aggregate_bwd(T, s_src, s_dst, state, alpha, pre, gy, g.rowptr_local, g.col, g.t_rowptr,
                                                       g.t_eid, g.t_dst, H, C, bias=ctx.bp, negative_slope=slope, p_att=p_att,
                                                       seed_att=seed_att, seed_att_dev=seed_att_dev, epilogue=epilogue,
                                                       p_drop=p_drop, seed=seed, seed_dev=seed_dev, want_bias=ctx.bp is not None,
                                                       n_rows=nl, row_ids=g.owned_global if masked else None,
                                                       edge_base=g.edge_base if masked else None)
        a_s, a_d = att_src.detach().reshape(1, H, C), att_dst.detach().reshape(1, H, C)
        Tv = T[:, :HC].unflatten(1, (H, C))
        g_as = _head_column_sums(Tv, ds_src, W).view(1, H, C)                  # every extended row: a halo slot holds this rank's share
        g_ad = _head_column_sums(Tv[:nl], ds_dst, W).view(1, H, C)
        dTv = dT[:, :HC].unflatten(1, (H, C))
        dTv.addcmul_(ds_src.unsqueeze(-1), a_s)
        dTv[:nl].addcmul_(ds_dst.unsqueeze(-1), a_d)
        if not resident:
            # reverse exchange: the halo rows' dT go back to their owners, who add them into their own rows
            ps.return_halo(dT[nl:], dT[:nl], W)
            dT = dT[:nl]
        dW = _gram_dw(dT, x)
        gx = _dx(dT, wp) if (ctx.needs_input_grad[0] and not resident) else None
        return gx, dW[:HC], g_as, g_ad, gb, None, None, None, None


class PartitionedGAT(_RankModel):
    """`gat.GAT` on rank `rank`'s rows of a destination-node partition (see the module docstring).

        pg = PartitionedGAT(model, edge_index, num_nodes, rank, world, device)
        out = pg.forward(x[pg.owned_global])                 # log-probs of the owned rows; differentiable when model.training
        loss = pg.nll_loss(out, y[pg.owned_global], train_mask[pg.owned_global])
        opt.zero_grad(); loss.backward(); pg.sync_grads(); opt.step()

    owner: int32 [num_nodes] owner rank of every node (default: contiguous blocks; `dist.partition_nodes(central_mask, world)`
    is accepted).  group: the torch.distributed group (a gloo group with CUDA tensors stages the payload through the host)."""

    def __init__(self, model, edge_index, num_nodes, rank, world, device, owner=None, group=None):
        if isinstance(edge_index, torch.Tensor):
            edge_index = edge_index.detach().cpu().numpy()
        self.model, self.rank, self.world, self.device, self.group = model, rank, world, torch.device(device), group
        if self.device.type != "cuda":
            raise RuntimeError(f"bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path (got device {self.device})")
        for conv in (model.conv1, model.conv2):
            H, C = conv.heads, conv.out_channels
            if not (1 <= H <= ops.GAT_MAX_HEADS and 1 <= C <= ops.GAT_MAX_C):
                raise RuntimeError(f"GATConv: unsupported shape: heads = {H}, out_channels = {C} (the HIP aggregation takes "
                                   f"1 <= heads <= {ops.GAT_MAX_HEADS}, 1 <= out_channels <= {ops.GAT_MAX_C})")
        self.part = GatPartition(edge_index, num_nodes, rank, world, owner=owner)
        self.tables = _GatTables(self.part, self.device)
        self.comm = _Comm(group, device, world)
        self.owned_global = self.tables.owned_global
        self.n_local, self.n_halo, self.num_nodes = self.part.n_local, self.part.n_halo, int(num_nodes)
        self._x_ext = None

    def _conv(self, conv, h, resident, epilogue, p_drop):
        """`GATConv.run` on this rank's rows: the same seeds in the same order, the same routing of the epilogue"""
        H, C = conv.heads, conv.out_channels
        w, b = conv.lin_src.weight, conv.bias
        torch_epi = epilogue == "log_softmax" and H != 1
        kern_epi = None if torch_epi else epilogue
        p_att = conv.dropout if conv.training else 0.0
        kern_p = float(p_drop) if kern_epi == "elu" else 0.0
        seed_att, seed_att_dev = dropout_seed(p_att, step_word=False)          # as GATConv.run draws them: attention, then epilogue
        seed, seed_dev = dropout_seed(kern_p, step_word=False)
        cfg = (H, C, conv.negative_slope, float(p_att), kern_epi, kern_p)
        seeds = (seed_att, seed_att_dev, seed, seed_dev)
        params = (w, conv.att_src, conv.att_dst) + ((b,) if b is not None else ())
        if torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for p in params)):
            out = _PartGatLayerFn.apply(h, w, conv.att_src, conv.att_dst, b, self, resident, cfg, seeds)
        else:
            out = _conv_forward(self, h.detach(), _pad_rows(w.detach()), conv.att_src.detach(), conv.att_dst.detach(),
                                _pad_bias(b.detach(), H * C) if b is not None else None, resident, cfg, seeds, False)[0][:, :H * C]
        if torch_epi:
            out = F.log_softmax(out, dim=1)
        return out

    def _check(self, x_local):
        if not x_local.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x_local.device} tensor)")
        if x_local.shape[0] != self.n_local:
            raise ValueError(f"x_local has {x_local.shape[0]} rows, this rank owns {self.n_local}")

    def forward(self, x_local):
        """x_local [n_local, F] (the rows of owned_global) -> log-probabilities [n_local, C] of the owned rows.  Training mode:
        attention and feature dropout at model.dropout with the single-GPU masks, differentiable in the parameters; eval mode: the
        plain forward."""
        self._check(x_local)
        m = self.model
        h = self._conv(m.conv1, self._input_ext(x_local), True, "elu", m.dropout if m.training else 0.0)
        return self._conv(m.conv2, h, False, "log_softmax", 0.0)

    __call__ = forward

    def get_emb(self, x_local):
        """`GAT.get_emb` on the owned rows: elu(conv1) without the feature dropout.  No exchange: conv 0 reads the resident halo."""
        self._check(x_local)
        return self._conv(self.model.conv1, self._input_ext(x_local), True, "elu", 0.0)
