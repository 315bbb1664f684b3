"""GCN (the default backbone of `train_gnn_noDTC`, `gcn.GCNNet`, reference models/backbones.py:246-300) on a destination-node
partition: evaluation and the training step, one process per GPU; new -- the reference is single-device.

Rank r owns a block of rows and all their in-edges of A' + I (`dist.PartitionPlan` with ONE table and rewrite_self_loops: every
input self loop dropped, one added per node, duplicate non-loop edges kept -- the `GcnGraph` contract).  Its graph is "extended":
the owned rows followed by one slot per halo node (a remote source of an owned row), made square by giving the halo slots no
in-edges.  Every conv runs transform-first as on one GPU (T = x W^T, then dinv_i * sum dinv_j T_j + b), so what crosses ranks is
OUTPUT-width: pad4(D) floats per row.
  * dinv: `dinv_ext` holds deg^-1/2 of the GLOBAL in-degree (self loop included) for the owned rows and for the halo slots, taken
    from the whole edge list (a halo slot has no in-edges here) and rounded as `GcnGraph` rounds it (fp64 rsqrt, then fp32): every
    rank multiplies by exactly the single-GPU factors;
  * conv 0 reads the graph's input features: their halo rows stay resident (fetched once per version of x), the rank transforms
    its own and its halo rows and aggregates with no exchange; the halo rows' share of the weight gradient is this rank's;
  * conv l >= 1 transforms the own rows, packs the send rows (`ops.gather_rows`) and does ONE all_to_all; backward walks the
    by-source view over all n_ext sources (`ops.gcn_aggregate_bwd` with n_src = n_ext), sends the halo part of dT back (the
    reverse exchange) and the owner folds it into its own dT rows with `ops.rows_segment_add` (no atomics, deterministic);
  * hub rows: a destination of >= `ops.GCN_HUB_THRESHOLD` in-edges is a hub on its owner's rank; a hub SOURCE may be a halo slot
    (a node feeding many rows of another rank), so the by-source hub tables cover the extended numbering;
  * dropout: the seeds are drawn exactly as `GCNConv.run` draws them (`ktgnn.dropout_seed`: host generator, one draw per dropout
    conv per forward) and the kernel hashes (seed, GLOBAL row id * D + column) (`row_ids`: `row_id_opt` of the one entry
    bgnn_gcn_aggregate_f32, ABI 116), in the row kernel and in a hub's finish pass alike, so every rank draws the masks of the
    single-GPU step;
  * the loss is a sum over the owned rows with the GLOBAL normaliser (`nll_loss`); parameter gradients are summed in ONE
    bucketed all-reduce (`sync_grads`).
`get_emb` / `get_logits` walk the same in-neighbours as `forward` (see gcn.py) and are supported.  Out of scope (raise):
log_softmax at D > 128."""
import numpy as np
import torch

from . import ops
from .dist_sage import SagePartition, _dx, _gram_dw, _Layer, _RankModel
from .dist_train import _Comm
from .gcn import _pad_bias, _pad_rows, _transform
from .ktgnn import dropout_seed

__all__ = ["GcnPartition", "PartitionedGCN"]


class GcnPartition(SagePartition):
    """Host side (numpy, device agnostic) of one rank's GCN partition -- built identically on every rank, no communication.
    `SagePartition`'s fields over the edges of A' + I (exactly one self loop per owned row, the last edge of its row), and
        dinv_ext [n_ext] float32      1/sqrt(global in-degree incl. the self loop) of the owned rows, then of the halo slots"""

    def __init__(self, edge_index, num_nodes, rank, world, owner=None):
        ei = np.asarray(edge_index, dtype=np.int64)
        super().__init__(ei, num_nodes, rank, world, owner=owner, rewrite_self_loops=True)
        deg = np.bincount(ei[1][ei[0] != ei[1]], minlength=self.N).astype(np.float64) + 1.0
        self.dinv_ext = (1.0 / np.sqrt(deg[self.ext_global()])).astype(np.float32)      # fp64, then rounded: GcnGraph's dinv


class _GcnTables(_Layer):
    """device tables of one rank shared by every conv: `dist_sage._Layer`'s, dinv and the hub tables of both views"""

    def __init__(self, part, device):
        super().__init__(part, device)
        self.dinv = torch.from_numpy(part.dinv_ext).to(device)
        hubs = lambda t: None if t is None else (ops.GCN_HUB_THRESHOLD, t[0], t[1], t[2])
        self.hubs = hubs(self.csr.hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT))               # owned rows only
        self.t_hubs = hubs(self.csr.transposed_hub_tables(ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT))  # owned and halo sources


def _conv_forward(ps, x, wp, bp, D, resident, epilogue, p_drop, seed, seed_dev=None):
    """one conv on this rank's rows -> y [n_local, pad4(D)].  resident: x already holds the halo rows ([n_ext, Din], conv 0); else
    x is [n_local, Din] and the T rows of the halo come through one all_to_all."""
    part, g = ps.part, ps.tables
    T = _transform(x, wp)
    if not resident:
        halo = ps.halo_rows(T)
        if part.n_halo:
            T = torch.cat((T, halo))
    return ops.gcn_aggregate(T, g.rowptr_local, g.col, g.dinv, part.n_local, D, bias=bp, epilogue=epilogue, p_drop=p_drop,
                             seed=seed, seed_dev=seed_dev, hubs=g.hubs, row_ids=g.owned_global if p_drop > 0 else None)


class _PartGcnLayerFn(torch.autograd.Function):
    """one conv of the partitioned model with its hand-written backward (the partitioned form of `gcn._GcnLayerFn`): dT over the
    extended graph and db from `gcn_aggregate_bwd`, the halo part of dT returned to the owners and folded in (conv l >= 1), then
    dW = dT^T x and dx = dT W."""

    @staticmethod
    def forward(ctx, x, w, b, ps, resident, epilogue, p_drop, seed, seed_dev):
        D = w.shape[0]
        wp = _pad_rows(w.detach())
        xd = x.detach()
        y = _conv_forward(ps, xd, wp, _pad_bias(b.detach(), D) if b is not None else None, D, resident, epilogue, p_drop, seed,
                          seed_dev)
        ctx.save_for_backward(xd, wp)
        ctx.y, ctx.ps, ctx.cfg = y, ps, (D, resident, epilogue, p_drop, b is not None)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wp = ctx.saved_tensors
        D, resident, epilogue, p_drop, has_b = ctx.cfg
        ps, y = ctx.ps, ctx.y
        part, g = ps.part, ps.tables
        nl, ne, Dp = part.n_local, part.n_ext, ops.pad4(D)
        if Dp != D or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            gp = torch.zeros(nl, Dp, dtype=torch.float32, device=gy.device)
            gp[:, :D] = gy
            gy = gp
        dT, gb = ops.gcn_aggregate_bwd(y, gy, g.t_rowptr, g.t_dst, g.dinv, ne, D, epilogue=epilogue, p_drop=p_drop,
                                       want_bias=has_b, hubs=g.t_hubs)
        if not resident:
            # reverse exchange: the halo rows' dT go back to their owners, who add them into their own rows
            ps.return_halo(dT[nl:], dT[:nl], Dp)
            dT = dT[:nl]
        dW = _gram_dw(dT, x)
        gx = _dx(dT, wp) if (ctx.needs_input_grad[0] and not resident) else None
        return gx, dW[:D], gb, None, None, None, None, None, None


class PartitionedGCN(_RankModel):
    """`gcn.GCNNet` on rank `rank`'s rows of a destination-node partition (see the module docstring).

        pg = PartitionedGCN(model, edge_index, num_nodes, rank, world, device)
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
        if model.convs[-1].out_channels > 128:
            raise NotImplementedError("PartitionedGCN: the fused log_softmax needs <= 128 classes")
        self.part = GcnPartition(edge_index, num_nodes, rank, world, owner=owner)
        self.tables = _GcnTables(self.part, self.device)
        self.comm = _Comm(group, device, world)
        self.owned_global = self.tables.owned_global
        self.n_local, self.n_halo, self.num_nodes = self.part.n_local, self.part.n_halo, int(num_nodes)
        self._x_ext = None

    def _run(self, x_local, n_convs, last_epilogue):
        m = self.model
        if not x_local.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x_local.device} tensor)")
        if x_local.shape[0] != self.n_local:
            raise ValueError(f"x_local has {x_local.shape[0]} rows, this rank owns {self.n_local}")
        p = m.dropout if m.training else 0.0
        L = len(m.convs)
        if n_convs == 0:
            return x_local
        h = self._input_ext(x_local)
        for ind in range(n_convs):
            conv = m.convs[ind]
            last = ind == L - 1
            epi = last_epilogue if last else "relu"
            kp = 0.0 if last else p
            seed, seed_dev = dropout_seed(kp, step_word=False)                  # as GCNConv.run draws it
            w, b = conv.lin.weight, conv.bias
            D = conv.out_channels
            if torch.is_grad_enabled() and (w.requires_grad or (b is not None and b.requires_grad)):
                h = _PartGcnLayerFn.apply(h, w, b, self, ind == 0, epi, float(kp), seed, seed_dev)
            else:
                h = _conv_forward(self, h.detach(), _pad_rows(w.detach()), _pad_bias(b.detach(), D) if b is not None else None, D,
                                  ind == 0, epi, float(kp), seed, seed_dev)[:, :D]
        return h

    def forward(self, x_local):
        """x_local [n_local, F] (the rows of owned_global) -> log-probabilities [n_local, C] of the owned rows.  Training mode:
        dropout at model.dropout with the single-GPU masks, differentiable in the parameters; eval mode: the plain forward."""
        return self._run(x_local, len(self.model.convs), "log_softmax")

    __call__ = forward

    def get_emb(self, x_local):
        """`GCNNet.get_emb` on the owned rows: every conv but the last (ReLU, and dropout in training mode, after each)"""
        return self._run(x_local, len(self.model.convs) - 1, None)

    def get_logits(self, x_local):
        """`GCNNet.get_logits` on the owned rows: the raw class scores"""
        return self._run(x_local, len(self.model.convs), None)
