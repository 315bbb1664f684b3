"""GraphSAGE (the --no_dtc model, `sage.GraphSAGE`, reference models/backbones.py:440-498) on a destination-node partition:
evaluation and the training step, one process per GPU; new -- the reference is single-device.

Rank r owns a block of rows and all their in-edges (`dist.PartitionPlan` with ONE table and the edges exactly as given: no self
loop added or removed, duplicates kept, the `SageGraph` contract).  Its graph is "extended": the owned rows followed by one slot
per halo node (a remote source of an owned row), made square by giving the halo slots no in-edges.  Every conv runs
transform-first as on one GPU (T = x [W_l ; W_r]^T + [0 ; b_l], then the mean of T_l rows plus the T_r row), so what crosses
ranks is OUTPUT-width: pad4(D) floats per row.
  * conv 0 reads the graph's input features: their halo rows stay resident (fetched once per version of x), the rank transforms
    its own and its halo rows and aggregates with no exchange; the halo rows' share of the weight gradient is this rank's;
  * conv l >= 1 transforms the own rows, packs the T_l half of the send rows (`ops.gather_rows`) and does ONE all_to_all;
    backward sends the halo part of dT_l back (the reverse exchange) and the owner folds it into its own dT_l rows with
    `ops.rows_segment_add` (a row sent to k ranks gets k rows back; no atomics, deterministic);
  * dropout: the seeds are drawn exactly as `SAGEConv.run` draws them (host generator, one draw per dropout conv per forward) and
    the kernel hashes (seed, GLOBAL row id * D + column) (`row_ids`: `row_id_opt` of the one entry bgnn_sage_mean_aggregate_f32,
    ABI 116), so every rank draws the masks of the single-GPU step;
  * the loss is a sum over the owned rows with the GLOBAL normaliser (`nll_loss`): the ranks' shares add up to the reference's
    F.nll_loss; parameter gradients are summed in ONE bucketed all-reduce (`sync_grads`).
Out of scope (raise): get_emb / get_logits (out-neighbour averaging needs a source partition), normalize=True, log_softmax at
D > 128."""
import numpy as np
import torch

from . import ops
from .dist import PartitionPlan
from .dist_train import _Comm
from .sage import _pack, _transform

__all__ = ["SagePartition", "PartitionedGraphSAGE"]


class SagePartition:
    """Host side (numpy, device agnostic) of one rank's GraphSAGE partition -- built identically on every rank, no communication:
        owned_global [n_local]        global id of every owned row (`PartitionPlan` order: interior rows first)
        rowptr [n_ext + 1], col [E]   extended by-destination CSR; col < n_local: an owned row, n_local + p: halo slot p
        halo_global [n_halo]          global id of halo slot p (one slot per node; slots sorted by (owner, id))
        send_rows [n_send]            local row of every send entry, in send order (peer-major), send_splits / recv_splits
        seg_ptr, seg_idx, seg_row     segment CSR of the send list for the gradient return: segment s collects the send
                                      entries seg_idx[seg_ptr[s]:seg_ptr[s+1]] (ascending) of the owned row seg_row[s]"""

    def __init__(self, edge_index, num_nodes, rank, world, owner=None, rewrite_self_loops=False):
        N = int(num_nodes)
        plan = PartitionPlan(edge_index, np.ones(N, dtype=bool), rank, world, owner=owner, rewrite_self_loops=rewrite_self_loops)
        assert plan.n_halo_by_table[1] == 0 and (plan.halo_ext_perm == np.arange(plan.n_halo)).all()
        self.plan, self.rank, self.world, self.N = plan, rank, world, N
        self.owned_global = plan.owned_global.astype(np.int64)
        self.n_local, self.n_halo = plan.n_local, plan.n_halo
        self.n_ext = self.n_local + self.n_halo
        self.num_edges = plan.local_num_edges
        self.rowptr = np.concatenate([plan.rowptr, np.full(self.n_halo, plan.rowptr[-1], dtype=np.int32)]).astype(np.int32)
        self.col = plan.col_ext.astype(np.int32)
        self.halo_global = plan.halo_global.astype(np.int64)
        self.send_rows = plan.send_rows_local.astype(np.int64)
        self.send_splits, self.recv_splits = list(plan.send_splits), list(plan.recv_splits)
        order = np.argsort(self.send_rows, kind="stable")
        rows, counts = np.unique(self.send_rows[order], return_counts=True)
        self.seg_idx = order.astype(np.int32)
        self.seg_row = rows.astype(np.int32)
        self.seg_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

    def ext_global(self):
        """global id of every extended row: owned rows, then halo slots"""
        return np.concatenate([self.owned_global, self.halo_global])


class _Layer:
    """device tables of one rank shared by every conv"""

    def __init__(self, part, device):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.rowptr = t(part.rowptr)
        self.rowptr_local = self.rowptr[:part.n_local + 1]
        self.col = t(part.col) if part.num_edges else torch.zeros(1, dtype=torch.int32, device=device)
        self.csr = csr = ops.DstCSR(self.rowptr, self.col, None, part.num_edges, part.n_ext)
        self.t_rowptr, _, self.t_dst = csr.transposed()
        if self.t_dst.numel() == 0:
            self.t_dst = torch.zeros(1, dtype=torch.int32, device=device)
        self.owned_global = t(part.owned_global)
        self.send_rows = t(part.send_rows)
        self.seg_ptr, self.seg_idx, self.seg_row = t(part.seg_ptr), t(part.seg_idx), t(part.seg_row)


def _gram_dw(dT, x):
    if ops.gram_supported(dT.shape[1], x.shape[1]) and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0:
        return ops.gram(dT, x)
    return dT.t().mm(x)


def _dx(dT, wcat):
    din = wcat.shape[1]
    if ops.linear_supported(dT.shape[1], din):
        return ops.linear(dT, wcat.t().contiguous(), torch.zeros(din, dtype=torch.float32, device=dT.device))
    return dT.mm(wcat)


def _conv_forward(ps, x, wcat, bcat, D, resident, epilogue, p_drop, seed):
    """one conv on this rank's rows -> y [n_local, pad4(D)].  resident: x already holds the halo rows ([n_ext, Din], conv 0); else
    x is [n_local, Din] and the T_l rows of the halo come through one all_to_all."""
    part, g = ps.part, ps.tables
    nl, Dp = part.n_local, ops.pad4(D)
    T = _transform(x, wcat, bcat)
    if resident:
        tl = T[:, :Dp]
    else:
        halo = ps.halo_rows(T[:, :Dp])
        tl = torch.cat((T[:, :Dp], halo)) if part.n_halo else T[:, :Dp]
    y = ops.sage_mean_aggregate(tl, g.rowptr_local, g.col, nl, D, root=T[:nl, Dp:], mean=True, epilogue=epilogue,
                                p_drop=p_drop, seed=seed, row_ids=g.owned_global if p_drop > 0 else None)
    return y


class _PartSageLayerFn(torch.autograd.Function):
    """one conv of the partitioned model with its hand-written backward (the partitioned form of `sage._SageLayerFn`):
    dT over the extended graph from `sage_mean_aggregate_bwd`, the halo part of dT_l returned to the owners and folded in
    (conv l >= 1), then dW = dT^T x, db_l = column sums of dT_r, dx = dT [W_l ; W_r]."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, ps, resident, epilogue, p_drop, seed):
        D = w_l.shape[0]
        wcat, bcat = _pack(w_l.detach(), b_l.detach() if b_l is not None else None, w_r.detach() if w_r is not None else None)
        xd = x.detach()
        y = _conv_forward(ps, xd, wcat, bcat, D, resident, epilogue, p_drop, seed)
        ctx.save_for_backward(xd, wcat)
        ctx.y, ctx.ps, ctx.cfg = y, ps, (D, resident, epilogue, p_drop, b_l is not None, w_r is not None)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wcat = ctx.saved_tensors
        D, resident, epilogue, p_drop, has_b, has_r = ctx.cfg
        ps, y = ctx.ps, ctx.y
        part, g = ps.part, ps.tables
        nl, ne, Dp = part.n_local, part.n_ext, ops.pad4(D)
        if Dp != D or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            gp = torch.zeros(nl, Dp, dtype=torch.float32, device=gy.device)
            gp[:, :D] = gy
            gy = gp
        dT = torch.empty(ne, 2 * Dp, dtype=torch.float32, device=gy.device)
        if ne > nl:
            dT[nl:, Dp:] = 0                                  # halo rows have no root half
        ops.sage_mean_aggregate_bwd(y, gy, g.rowptr_local, g.t_rowptr, g.t_dst, ne, D, epilogue=epilogue, p_drop=p_drop,
                                    grad_tbl=dT[:, :Dp], grad_root=dT[:nl, Dp:])
        if not resident:
            # reverse exchange: the halo rows' dT_l go back to their owners, who add them into their own rows
            ps.return_halo(dT[nl:, :Dp], dT[:nl, :Dp], Dp)
            dT = dT[:nl]
        dW = _gram_dw(dT, x)
        gw_l = dW[:D]
        gw_r = dW[Dp:Dp + D] if has_r else None
        gb_l = ops.column_sums(dT)[Dp:Dp + D] if has_b else None
        gx = _dx(dT, wcat) if (ctx.needs_input_grad[0] and not resident) else None
        return gx, gw_l, gb_l, gw_r, None, None, None, None, None


class _RankModel:
    """what the partitioned baselines share: the resident input halo, a conv's halo exchange and its return, the loss share and
    the gradient all-reduce.  A subclass sets model, part, tables (send_rows, seg_ptr, seg_idx, seg_row), comm and `_x_ext = None`."""

    def _input_ext(self, x_local):
        """[x own rows ; x halo rows] for the current version of the input features: the halo is fetched on first use and again
        whenever x_local is another tensor object or was written in place"""
        key = (x_local._version, tuple(x_local.shape), x_local.data_ptr())
        if self._x_ext is None or self._x_ext[0] is not x_local or self._x_ext[1] != key:
            xf = x_local.detach().float().contiguous()
            if self.part.n_halo or self.comm.live:
                send = xf.index_select(0, self.tables.send_rows)
                halo = self.comm.all_to_all(send, self.part.send_splits, self.part.recv_splits)
                ext = torch.cat((xf, halo)).contiguous()
            else:
                ext = xf
            self._x_ext = (x_local, key, ext)
        return self._x_ext[2]

    def invalidate_input_cache(self):
        """forget the resident input halo (after a write to x that does not advance its version)"""
        self._x_ext = None

    def halo_rows(self, X):
        """the rows of X [n_local, W] (a row-strided view) that this rank's halo slots stand for, [n_halo, W]: ONE all_to_all"""
        part = self.part
        send = ops.gather_rows(X, self.tables.send_rows) if part.send_rows.shape[0] else X.new_zeros(0, X.shape[1])
        return self.comm.all_to_all(send, part.send_splits, part.recv_splits)

    def return_halo(self, dT_halo, dT_own, W):
        """the reverse exchange: the halo slots' gradient rows go back to their owners (ONE all_to_all), who add what they get
        into dT_own over W columns (a row sent to k ranks gets k rows back; no atomics, deterministic)"""
        part, g = self.part, self.tables
        back = self.comm.all_to_all(dT_halo, part.recv_splits, part.send_splits)
        if back.shape[0]:
            ops.rows_segment_add(back, g.seg_ptr, g.seg_idx, g.seg_row, dT_own, D=W, accumulate=True)

    def nll_loss(self, out, y_local, train_mask_local):
        """this rank's share of F.nll_loss(logp[train_mask], y[train_mask]): the owned training rows' terms over the GLOBAL count"""
        tm = train_mask_local.bool()
        cnt = self.comm.all_reduce(tm.sum().reshape(1).double()).float().clamp_min(1)
        yi = y_local.clamp_min(0)[:, None]
        return -(out.gather(1, yi).squeeze(1) * tm.float()).sum() / cnt[0]

    def sync_grads(self):
        """sum the parameter gradients over the ranks: ONE all-reduce of one flat bucket"""
        ps = [p for p in self.model.parameters() if p.grad is not None]
        if not ps or not self.comm.live:
            return
        flat = self.comm.all_reduce(torch.cat([p.grad.reshape(-1) for p in ps]))
        o = 0
        for p in ps:
            n = p.grad.numel()
            p.grad.copy_(flat[o:o + n].view_as(p.grad))
            o += n


class PartitionedGraphSAGE(_RankModel):
    """`sage.GraphSAGE` on rank `rank`'s rows of a destination-node partition (see the module docstring).

        ps = PartitionedGraphSAGE(model, edge_index, num_nodes, rank, world, device)
        out = ps.forward(x[ps.owned_global])                 # log-probs of the owned rows; differentiable when model.training
        loss = ps.nll_loss(out, y[ps.owned_global], train_mask[ps.owned_global])
        opt.zero_grad(); loss.backward(); ps.sync_grads(); opt.step()

    owner: int32 [num_nodes] owner rank of every node (default: contiguous blocks; `dist.partition_nodes(central_mask, world)`
    is accepted).  group: the torch.distributed group (a gloo group with CUDA tensors stages the payload through the host)."""

    def __init__(self, model, edge_index, num_nodes, rank, world, device, owner=None, group=None):
        if isinstance(edge_index, torch.Tensor):
            edge_index = edge_index.detach().cpu().numpy()
        self.model, self.rank, self.world, self.device, self.group = model, rank, world, torch.device(device), group
        self.part = SagePartition(edge_index, num_nodes, rank, world, owner=owner)
        self.tables = _Layer(self.part, self.device)
        self.comm = _Comm(group, device, world)
        self.owned_global = self.tables.owned_global
        self.n_local, self.n_halo, self.num_nodes = self.part.n_local, self.part.n_halo, int(num_nodes)
        self._x_ext = None
        for conv in model.convs:
            if conv.normalize:
                raise NotImplementedError("PartitionedGraphSAGE: normalize=True is not supported")
        if model.convs[-1].out_channels > 128:
            raise NotImplementedError("PartitionedGraphSAGE: the fused log_softmax needs <= 128 classes")

    def forward(self, x_local):
        """x_local [n_local, F] (the rows of owned_global) -> log-probabilities [n_local, C] of the owned rows.  Training mode:
        dropout at model.dropout with the single-GPU masks, differentiable in the parameters; eval mode: the plain forward."""
        m = self.model
        if x_local.shape[0] != self.n_local:
            raise ValueError(f"x_local has {x_local.shape[0]} rows, this rank owns {self.n_local}")
        p = m.dropout if m.training else 0.0
        L = len(m.convs)
        h = self._input_ext(x_local)
        for ind, conv in enumerate(m.convs):
            last = ind == L - 1
            epi = "log_softmax" if last else "relu"
            kp = 0.0 if last else p
            seed = int(torch.empty((), dtype=torch.int64).random_().item()) if kp > 0 else 0   # as SAGEConv.run draws it
            w_l, b_l, w_r = conv._params()
            D = conv.out_channels
            if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (w_l, b_l, w_r)):
                h = _PartSageLayerFn.apply(h, w_l, b_l, w_r, self, ind == 0, epi, float(kp), seed)
            else:
                wcat, bcat = _pack(w_l.detach(), b_l.detach() if b_l is not None else None,
                                   w_r.detach() if w_r is not None else None)
                h = _conv_forward(self, h.detach(), wcat, bcat, D, ind == 0, epi, float(kp), seed)[:, :D]
        return h

    __call__ = forward

    def get_emb(self, *args, **kwargs):
        raise NotImplementedError("PartitionedGraphSAGE.get_emb: out-neighbour averaging needs a source partition")

    def get_logits(self, *args, **kwargs):
        raise NotImplementedError("PartitionedGraphSAGE.get_logits: out-neighbour averaging needs a source partition")
