"""APPNP (`appnp.APPNP_Net`, reference models/backbones.py:110-128) on a destination-node partition: evaluation and the training
step, one process per GPU; new -- the reference is single-device.

Rank r owns a block of rows and all their in-edges of A' + I (`dist_gcn.GcnPartition`: one self loop per owned row, duplicates
kept, `dinv_ext` the GLOBAL deg^-1/2 of the owned rows and of the halo slots).  The MLP (dropout, lin1, ReLU, dropout, lin2) runs
on the owned rows alone; what crosses ranks is class width, pad4(C) floats per row.
  * dropout: the two sites take their seeds in `APPNP_Net`'s order (`ktgnn.dropout_seed`) and hash (seed, GLOBAL row * D + column)
    (`ops.feature_dropout(row_ids=owned_global)`), so every rank draws the masks of the single-GPU step in its rows;
  * propagation: the K-step entry walks a square graph inside one call; here every step is one `ops.appnp_step` over the
    rectangular graph (owned rows gather from [owned rows ; halo slots]) with ONE all_to_all in front of it: h's send rows before
    step 0, the scaled state's (s_k = dinv (.) z_k, scaled by its owner) before steps 1 .. K-1 -- K exchanges of pad4(C) floats per
    send row.  The state lives in two alternating [n_ext, pad4(C)] buffers: the step stores the owned rows, `ops.gather_rows` packs
    the send list, the received rows land in the tail.  K = 0 exchanges nothing; log_softmax is fused into the last step;
  * backward: grad_h = P^T g is the same recurrence over A^T.  The out-edges of an owned row belong to other ranks, so the
    by-source view of this rank's rows would need a return exchange and a fold per step (three passes instead of the fused one).
    Instead each rank holds a SECOND partition, of the flipped edge list under the same owners (`AppnpPartition.t`), whose
    `dinv_ext` is overridden with the original graph's in-degree factors (A^'s products are symmetric in them; the flipped graph's
    own degrees would be the out-degrees): the backward is the forward's step-and-exchange loop on those tables with
    g = dy - exp(y) rowsum(dy) in h's place -- no fold, no atomics, no saved z_k, at the price of a second set of CSR and send
    tables.  The two partitions order their owned rows differently (interior rows first, and interior depends on the direction),
    so g enters and grad_h leaves through one `ops.gather_rows` each;
  * lin2 and the propagation are one autograd node, as `appnp._HeadFn`: dW = dh^T x, db = `ops.column_sums(dh)`, dx = dh W;
  * the loss is `nll_loss` (the GLOBAL normaliser), parameter gradients are summed in ONE `sync_grads`.
Out of scope (raise NotImplementedError): more than 128 classes, `graphed=True`."""
import numpy as np
import torch

from . import ops
from .appnp import _feature_drop, _rows4, _streamable
from .dist_gcn import GcnPartition
from .dist_sage import _dx, _gram_dw, _RankModel
from .dist_train import _Comm
from .gcn import _pad_bias, _pad_rows

__all__ = ["AppnpPartition", "PartitionedAPPNP"]


class AppnpPartition(GcnPartition):
    """Host side (numpy) of one rank's APPNP partition: `GcnPartition` of the graph, and in `t` the `GcnPartition` of the flipped
    edge list under the same owners -- the graph of A^T, whose rows the backward walks -- with `t.dinv_ext` replaced by the
    ORIGINAL graph's factors at `t.ext_global()`.
        t_from_f [n_local] int64   forward-order local row of the k-th owned row in t's order;  f_from_t: the inverse"""

    def __init__(self, edge_index, num_nodes, rank, world, owner=None):
        ei = np.asarray(edge_index, dtype=np.int64)
        super().__init__(ei, num_nodes, rank, world, owner=owner)
        self.t = GcnPartition(ei[::-1], num_nodes, rank, world, owner=self.plan.owner)
        deg = np.bincount(ei[1][ei[0] != ei[1]], minlength=self.N).astype(np.float64) + 1.0      # in-degrees of A' + I
        self.t.dinv_ext = (1.0 / np.sqrt(deg[self.t.ext_global()])).astype(np.float32)
        g2l = np.full(self.N, -1, dtype=np.int64)
        g2l[self.owned_global] = np.arange(self.n_local)
        self.t_from_f = g2l[self.t.owned_global]
        assert (self.t_from_f >= 0).all() and self.t.n_local == self.n_local
        self.f_from_t = np.empty_like(self.t_from_f)
        self.f_from_t[self.t_from_f] = np.arange(self.n_local)


class _StepTables:
    """device tables of one rank's propagation over one `GcnPartition`: the owned rows' CSR, dinv, the owned rows' hub tables and
    the send list (no by-source view: nothing here walks one)"""

    def __init__(self, part, device):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.n_local, self.n_ext = part.n_local, part.n_ext
        self.rowptr = t(part.rowptr[:part.n_local + 1])
        self.col = t(part.col) if part.num_edges else torch.zeros(1, dtype=torch.int32, device=device)
        self.dinv = t(part.dinv_ext)
        tabs = ops.DstCSR._hub_tables_of(self.rowptr, part.n_local, ops.GCN_HUB_THRESHOLD, ops.GCN_HUB_SEGMENT)
        self.hubs = None if tabs is None else (ops.GCN_HUB_THRESHOLD, tabs[0], tabs[1], tabs[2])
        self.send_rows = t(part.send_rows)
        self.send_splits, self.recv_splits = part.send_splits, part.recv_splits


def _exchange(comm, tabs, buf):
    """the halo slots of buf [n_ext, W] <- the rows their owners hold in their own buf[:n_local]: pack, ONE all_to_all, land"""
    send = ops.gather_rows(buf, tabs.send_rows) if tabs.send_rows.shape[0] else buf.new_zeros(0, buf.shape[1])
    recv = comm.all_to_all(send, tabs.send_splits, tabs.recv_splits)
    if tabs.n_ext > tabs.n_local:
        buf[tabs.n_local:].copy_(recv)


def _propagate(comm, tabs, hx, D, K, alpha, epilogue):
    """epi(P h) on this rank's rows -> [n_local, pad4(D)].  hx [n_ext, pad4(D)]: h's owned rows in front (pad columns 0), the tail
    is filled here.  K steps, one exchange in front of each."""
    nl, Dp = tabs.n_local, hx.shape[1]
    h = hx[:nl]
    if K == 0:                                        # epi(h): no edge is walked, nothing is exchanged
        return ops.appnp_propagate(h, tabs.rowptr, tabs.col, tabs.dinv, nl, D, 0, alpha, epilogue=epilogue)
    out = torch.empty(nl, Dp, dtype=torch.float32, device=hx.device)
    state = [torch.empty(tabs.n_ext, Dp, dtype=torch.float32, device=hx.device) for _ in range(min(K - 1, 2))]
    src = hx
    for k in range(K):
        _exchange(comm, tabs, src)
        last = k == K - 1
        dst = out if last else state[k & 1]
        ops.appnp_step(src, h, tabs.rowptr, tabs.col, tabs.dinv, nl, D, alpha, first=k == 0,
                       store=("log_softmax" if epilogue == "log_softmax" else "out") if last else "state", hubs=tabs.hubs,
                       out=dst if last else dst[:nl])
        src = dst
    return out


def _ext_rows(tabs, D, device):
    return torch.empty(tabs.n_ext, ops.pad4(D), dtype=torch.float32, device=device)


def _head_forward(pa, x, wp, bp, D, K, alpha, epilogue):
    """epi(P (x wp^T + bp)) on the owned rows: the logits are formed straight into the front of the extended buffer"""
    hx = _ext_rows(pa.tables, D, x.device)
    if ops.linear_supported(x.shape[1], wp.shape[0]) and _streamable(x):
        hx[:pa.n_local].copy_(ops.linear(x, wp, bp))
    else:
        torch.addmm(bp, x, wp.t(), out=hx[:pa.n_local])
    return _propagate(pa.comm, pa.tables, hx, D, K, alpha, epilogue)


class _PartHeadFn(torch.autograd.Function):
    """the partitioned form of `appnp._HeadFn`: out = log_softmax(P (x W^T + b)) on the owned rows; dh = P^T g through the same
    loop over the transposed partition's tables, then dW = dh^T x, db = colsum(dh), dx = dh W (this rank's shares)."""

    @staticmethod
    def forward(ctx, x, w, b, pa, K, alpha, epilogue):
        D = w.shape[0]
        wp = _pad_rows(w.detach())
        xd = x.detach()
        y = _head_forward(pa, xd, wp, _pad_bias(b.detach(), D), D, K, alpha, epilogue)
        ctx.save_for_backward(xd, wp)
        ctx.y = y if epilogue == "log_softmax" else None
        ctx.pa, ctx.cfg = pa, (D, K, alpha)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wp = ctx.saved_tensors
        D, K, alpha = ctx.cfg
        pa = ctx.pa
        nl = pa.n_local
        g = _rows4(gy, D)
        if ctx.y is not None:
            g = ops.appnp_log_softmax_bwd(ctx.y, g, D)                   # [n_local, pad4(D)], pad columns 0
        gx = _ext_rows(pa.t_tables, D, g.device)
        ops.gather_rows(g, pa.t_from_f, out=gx[:nl])                     # into the transposed partition's row order
        dh_t = _propagate(pa.comm, pa.t_tables, gx, D, K, alpha, None)
        dh = ops.gather_rows(dh_t, pa.f_from_t)                          # and back
        dW = _gram_dw(dh, x)
        gb = ops.column_sums(dh)[:D]
        gxin = _dx(dh, wp) if ctx.needs_input_grad[0] else None
        return gxin, dW[:D], gb, None, None, None, None


class PartitionedAPPNP(_RankModel):
    """`appnp.APPNP_Net` on rank `rank`'s rows of a destination-node partition (see the module docstring).

        pa = PartitionedAPPNP(model, edge_index, num_nodes, rank, world, device)
        out = pa.forward(x[pa.owned_global])                 # log-probs of the owned rows; differentiable when model.training
        loss = pa.nll_loss(out, y[pa.owned_global], train_mask[pa.owned_global])
        opt.zero_grad(); loss.backward(); pa.sync_grads(); opt.step()

    owner: int32 [num_nodes] owner rank of every node (default: contiguous blocks; `dist.partition_nodes(central_mask, world)`
    is accepted).  group: the torch.distributed group (a gloo group with CUDA tensors stages the payload through the host)."""

    def __init__(self, model, edge_index, num_nodes, rank, world, device, owner=None, group=None, graphed=False):
        if isinstance(edge_index, torch.Tensor):
            edge_index = edge_index.detach().cpu().numpy()
        self.model, self.rank, self.world, self.device, self.group = model, rank, world, torch.device(device), group
        if self.device.type != "cuda":
            raise RuntimeError(f"bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path (got device {self.device})")
        if graphed:
            raise NotImplementedError("PartitionedAPPNP(graphed=True): a partitioned epoch is not captured into a HIP graph")
        if model.lin2.out_channels > 128:
            raise NotImplementedError("PartitionedAPPNP: the class-width propagation needs <= 128 classes")
        self.part = AppnpPartition(edge_index, num_nodes, rank, world, owner=owner)
        self.tables = _StepTables(self.part, self.device)
        self.t_tables = _StepTables(self.part.t, self.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.owned_global = t(self.part.owned_global)
        self.t_from_f, self.f_from_t = t(self.part.t_from_f), t(self.part.f_from_t)
        self.comm = _Comm(group, device, world)
        self.n_local, self.n_halo, self.num_nodes = self.part.n_local, self.part.n_halo, int(num_nodes)
        self._x_ext = None

    def forward(self, x_local):
        """x_local [n_local, F] (the rows of owned_global) -> log-probabilities [n_local, C] of the owned rows.  Training mode:
        dropout at model.dropout with the single-GPU masks, differentiable in the parameters; eval mode: the plain forward."""
        m = self.model
        if not x_local.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x_local.device} tensor)")
        if x_local.shape[0] != self.n_local:
            raise ValueError(f"x_local has {x_local.shape[0]} rows, this rank owns {self.n_local}")
        p = m.dropout if m.training else 0.0
        x = _feature_drop(x_local, p, relu=False, row_ids=self.owned_global)
        x = _feature_drop(m.lin1(x), p, relu=True, row_ids=self.owned_global).float()
        w, b = m.lin2.weight, m.lin2.bias
        K, alpha = m.prop1.K, m.prop1.alpha
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad):
            return _PartHeadFn.apply(x, w, b, self, K, alpha, "log_softmax")
        D = w.shape[0]
        return _head_forward(self, x, _pad_rows(w.detach()), _pad_bias(b.detach(), D), D, K, alpha, "log_softmax")[:, :D]

    __call__ = forward
