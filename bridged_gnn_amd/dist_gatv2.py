"""GATv2 (the `gnn='GATv2'` baseline, `gatv2.GATv2`, reference models/backbones.py:302-358) on a destination-node partition:
evaluation and the training step, one process per GPU; new -- the reference is single-device.

The partition, the extended graph and the device tables are `dist_gat`'s (`GatPartition`, `_GatTables`: the owned rows and all
their in-edges of A' + I in the whole graph's order inside a row, followed by one halo slot per remote source, the halo slots
without in-edges).  Every conv runs transform-first as on one GPU, into ONE table T = x [W_l ; W_r]^T + [b_l ; b_r] with x_l at
columns [0, P) and x_r at [P, 2P), P = pad4(H*C).  A halo slot is only ever a SOURCE, so only its x_l half exists on this rank:
  * conv 0 reads the graph's input features: their halo rows stay resident (fetched once per version of x), the rank transforms
    its own and its halo rows and aggregates with no exchange; the halo rows' share of dW_l and db_l is this rank's, their x_r
    columns get zero gradient (`ops.gatv2_aggregate_bwd` leaves that half of the rows n_local .. n_ext as 0);
  * every later conv transforms the own rows, packs the x_l half of the send rows (`ops.gather_rows`) and does ONE all_to_all of
    P floats per row; the x_r half of a halo slot is filled with 0 and never read.  The backward walks the by-source view over all
    n_ext sources (`ops.gatv2_aggregate_bwd` with n_rows = n_local), sends the x_l half of the halo rows of dT back (the reverse
    exchange) and the owner folds it into its own rows with `ops.rows_segment_add` (no atomics, deterministic);
  * grad_att is the sum over this rank's edges, dW_cat = dT^T x and db_cat = column sums of dT over this rank's rows: per-rank
    sums that add up under `sync_grads` (the `bns.*` parameters, registered and never applied, have no gradient on any rank and
    are left out of the bucket on every rank alike);
  * dropout: the seeds are drawn exactly as `GATv2Conv.run` draws them (`ktgnn.dropout_seed`: per conv the attention seed, then
    the epilogue's) and the kernels hash the whole graph's positions (`row_ids`, `edge_base`: `row_id_opt` / `edge_base_opt` of
    the one entry each, bgnn_gatv2_aggregate_f32 and bgnn_gatv2_aggregate_bwd_f32, ABI 116), in the forward and where the
    backward redraws them; every rank draws the single-GPU masks;
  * the loss is a sum over the owned rows with the GLOBAL normaliser (`nll_loss`).
There is no `get_emb` (the model has none) and no graphed run."""
import torch
import torch.nn.functional as F

from . import ops
from .dist_gat import GatPartition, _GatTables
from .dist_sage import _dx, _gram_dw, _RankModel
from .dist_train import _Comm
from .gat import _aligned_rows
from .gatv2 import _cat_params, _transform_cat
from .gcn import _pad_bias
from .ktgnn import dropout_seed

__all__ = ["PartitionedGATv2"]


def _conv_forward(ps, x, wcat, bcat, att, bp, resident, cfg, seeds, keep):
    """one conv on this rank's rows -> (out [n_local, pad4(H*C)], kept).  resident: x already holds the halo rows ([n_ext, Din],
    conv 0); else x is [n_local, Din] and the x_l half of the halo rows of T comes through one all_to_all.  kept = (T over the
    extended rows, state, pre) when `keep` (what the backward reads), else None."""
    H, C, slope, p_att, epilogue, p_drop = cfg
    seed_att, seed_att_dev, seed, seed_dev = seeds
    part, g = ps.part, ps.tables
    P = ops.pad4(H * C)
    T = _aligned_rows(_transform_cat(x, wcat, bcat), 2 * P)
    if not resident:
        halo = ps.halo_rows(T[:, :P])
        if part.n_halo:
            ext = T.new_zeros(part.n_ext, T.shape[1])          # a halo slot's x_r half is never read: 0
            ext[:part.n_local] = T
            ext[part.n_local:, :P] = halo
            T = ext
    masked = p_att > 0 or p_drop > 0
    out, state, pre, _ = ops.gatv2_aggregate(T, att, g.rowptr_local, g.col, part.n_local, H, C, bias=bp, negative_slope=slope,
                                             p_att=p_att, seed_att=seed_att, seed_att_dev=seed_att_dev, epilogue=epilogue,
                                             p_drop=p_drop, seed=seed, seed_dev=seed_dev, want_pre=keep,
                                             row_ids=g.owned_global if masked else None,
                                             edge_base=g.edge_base if masked else None)
    return out, ((T, state, pre) if keep else None)


class _PartGatv2LayerFn(torch.autograd.Function):
    """one conv of the partitioned model with its hand-written backward (the partitioned form of `gatv2._Gatv2LayerFn`): dT over
    the extended rows (both halves), datt and db from `gatv2_aggregate_bwd`, the x_l half of the halo rows of dT returned to the
    owners and folded in (every conv but the first), then dW_cat = dT^T x, db_cat = column sums of dT and dx = dT W_cat."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, b_r, att, b, ps, resident, cfg, seeds):
        H, C = cfg[0], cfg[1]
        wcat, bcat = _cat_params(w_l.detach(), b_l.detach(), w_r.detach(), b_r.detach(), H * C)
        bp = _pad_bias(b.detach(), H * C) if b is not None else None
        xd = x.detach()
        out, kept = _conv_forward(ps, xd, wcat, bcat, att.detach(), bp, resident, cfg, seeds, True)
        ctx.save_for_backward(xd, wcat, att)
        ctx.kept, ctx.bp, ctx.ps, ctx.resident, ctx.cfg, ctx.seeds = kept, bp, ps, resident, cfg, seeds
        return out[:, :H * C]

    @staticmethod
    def backward(ctx, gy):
        x, wcat, att = ctx.saved_tensors
        H, C, slope, p_att, epilogue, p_drop = ctx.cfg
        seed_att, seed_att_dev, seed, seed_dev = ctx.seeds
        T, state, pre = ctx.kept
        ps, resident = ctx.ps, ctx.resident
        part, g = ps.part, ps.tables
        nl, HC, P = part.n_local, H * C, ops.pad4(H * C)
        masked = p_att > 0 or p_drop > 0
        gy = _aligned_rows(gy, HC)
        dT, datt, gb = ops.gatv2_aggregate_bwd(T, att.detach(), state, pre, gy, g.rowptr_local, g.col, g.t_rowptr, g.t_eid, g.t_dst,
                                               H, C, bias=ctx.bp, negative_slope=slope, p_att=p_att, seed_att=seed_att,
                                               seed_att_dev=seed_att_dev, epilogue=epilogue, p_drop=p_drop, seed=seed,
                                               seed_dev=seed_dev, want_bias=ctx.bp is not None, n_rows=nl,
                                               row_ids=g.owned_global if masked else None,
                                               edge_base=g.edge_base if masked else None)
        if not resident:
            # reverse exchange: the x_l half of the halo rows' dT goes back to the owners, who add it into their own rows
            ps.return_halo(dT[nl:, :P], dT[:nl, :P], P)
            dT = dT[:nl]
        dW = _gram_dw(dT, x)
        db = ops.column_sums(dT)
        gx = _dx(dT, wcat) if (ctx.needs_input_grad[0] and not resident) else None
        return gx, dW[:HC], db[:HC], dW[P:P + HC], db[P:P + HC], datt.view(1, H, C), gb, None, None, None, None


class PartitionedGATv2(_RankModel):
    """`gatv2.GATv2` (any number of convs) on rank `rank`'s rows of a destination-node partition (see the module docstring).

        pg = PartitionedGATv2(model, edge_index, num_nodes, rank, world, device)
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
        for conv in model.convs:
            H, C = conv.heads, conv.out_channels
            if not (1 <= H <= ops.GAT_MAX_HEADS and 1 <= C <= ops.GAT_MAX_C):
                raise RuntimeError(f"GATv2Conv: unsupported shape: heads = {H}, out_channels = {C} (the HIP conv takes "
                                   f"1 <= heads <= {ops.GAT_MAX_HEADS}, 1 <= out_channels <= {ops.GAT_MAX_C})")
        self.part = GatPartition(edge_index, num_nodes, rank, world, owner=owner)
        self.tables = _GatTables(self.part, self.device)
        self.comm = _Comm(group, device, world)
        self.owned_global = self.tables.owned_global
        self.n_local, self.n_halo, self.num_nodes = self.part.n_local, self.part.n_halo, int(num_nodes)
        self._x_ext = None

    def _conv(self, conv, h, resident, epilogue, p_drop):
        """`GATv2Conv.run` on this rank's rows: the same seeds in the same order, the same routing of the epilogue"""
        H, C = conv.heads, conv.out_channels
        zeros = None
        if conv.lin_l.bias is None:                                     # bias=False: the Linears have none either
            zeros = torch.zeros(H * C, dtype=torch.float32, device=h.device)
        w_l, w_r, b = conv.lin_l.weight, conv.lin_r.weight, conv.bias
        b_l = conv.lin_l.bias if zeros is None else zeros
        b_r = conv.lin_r.bias if zeros is None else zeros
        torch_epi = epilogue == "log_softmax" and H != 1
        kern_epi = None if torch_epi else epilogue
        p_att = conv.dropout if conv.training else 0.0
        kern_p = float(p_drop) if kern_epi == "elu" else 0.0
        seed_att, seed_att_dev = dropout_seed(p_att, step_word=False)          # as GATv2Conv.run draws them: attention, then epilogue
        seed, seed_dev = dropout_seed(kern_p, step_word=False)
        cfg = (H, C, conv.negative_slope, float(p_att), kern_epi, kern_p)
        seeds = (seed_att, seed_att_dev, seed, seed_dev)
        h = h.float()
        params = [p for p in (w_l, w_r, conv.att, conv.lin_l.bias, conv.lin_r.bias, b) if p is not None]
        if torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for p in params)):
            out = _PartGatv2LayerFn.apply(h, w_l, b_l, w_r, b_r, conv.att, b, self, resident, cfg, seeds)
        else:
            wcat, bcat = _cat_params(w_l.detach(), b_l.detach(), w_r.detach(), b_r.detach(), H * C)
            out = _conv_forward(self, h.detach(), wcat, bcat, conv.att.detach(), _pad_bias(b.detach(), H * C) if b is not None else None,
                                resident, cfg, seeds, False)[0][:, :H * C]
        if torch_epi:
            out = F.log_softmax(out, dim=1)
        return out

    def forward(self, x_local):
        """x_local [n_local, F] (the rows of owned_global) -> log-probabilities [n_local, C] of the owned rows.  Training mode:
        attention and feature dropout at the model's rates with the single-GPU masks, differentiable in the parameters; eval mode:
        the plain forward."""
        if not x_local.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x_local.device} tensor)")
        if x_local.shape[0] != self.n_local:
            raise ValueError(f"x_local has {x_local.shape[0]} rows, this rank owns {self.n_local}")
        m = self.model
        h = self._input_ext(x_local)
        for k, conv in enumerate(m.convs[:-1]):
            h = self._conv(conv, h, k == 0, "elu", m.dropout if m.training else 0.0)
        return self._conv(m.convs[-1], h, len(m.convs) == 1, "log_softmax", 0.0)

    __call__ = forward
