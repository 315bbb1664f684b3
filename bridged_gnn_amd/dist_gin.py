"""GIN (`gin.GINNet`, reference models/backbones.py:26-57) on a destination-node partition: evaluation and the training step, one
process per GPU; new -- the reference is single-device.

Rank r owns a block of rows and all their in-edges, exactly as given (`dist_sage.SagePartition(rewrite_self_loops=False)`: no self
loop added or removed, duplicates kept, the `SageGraph` contract).  Its device tables are `dist_sage._Layer`'s plus the hub tables
of both views (`hub_cfg = (threshold, segment)`): `csr.hub_tables` for the owned rows, `csr.transposed_hub_tables` for the owned AND
the halo sources -- a node feeding many rows of another rank is a hub source among this rank's halo slots.  A rank that walks a hub
as one lane group keeps every other rank waiting at the next exchange; `hub_cfg=None` runs unsegmented.

Every conv runs transform first, as on one GPU, and at EVERY layer (the APPNP / GCNII choice): no input halo stays resident, what
crosses ranks is pad4(D) floats a row, never F.
  * forward of a conv: T = x W^T of the owned rows goes into the front of an extended buffer [n_ext, pad4(D)]; `ops.gather_rows`
    packs the send list, ONE all_to_all, the received rows land in the buffer's tail; then `ops.gin_aggregate_hubs` over the
    rectangular graph (n_local rows gathering from n_ext; a row's own table row is its root) with `row_ids = owned_global`;
  * dropout: the seeds are drawn exactly as `GINNet.forward` draws them (`ktgnn.dropout_seed(p, step_word=False)` per conv, in forward
    order) and the kernels hash (seed, GLOBAL row * D + column), in the row kernel and in a hub's finish group alike: every rank
    draws the masks of the single-GPU step;
  * the last conv fuses the log_softmax up to 128 classes and leaves it to torch beyond; the single-layer model (eps a buffer) runs
    the same route without an eps pass;
  * backward of a conv (the partitioned `gin._GinLayerFn`): `ops.gin_aggregate_bwd_hubs` takes grad_y of the owned rows, n_src =
    n_ext, the by-source view and its hub tables; the halo rows of dT go back to their owners (ONE all_to_all, `return_halo`) and
    `ops.rows_segment_add` folds them in in a fixed order -- no atomics, a second run gives the same bits; dW, dx and db come from
    the owned rows; grad_eps is the rank's sum_i <g_i, T_i> over its owned rows;
  * the loss is `nll_loss` (the GLOBAL normaliser); `sync_grads` sums every parameter gradient, eps included, in ONE all-reduce.
A rank with no halo or no send rows still takes part in every collective.  Out of scope (raise NotImplementedError): `graphed=True`.
No epoch driver: none of the partitioned baselines has one."""
import torch
import torch.nn.functional as F

from . import ops
from .dist_sage import SagePartition, _dx, _gram_dw, _Layer, _RankModel
from .dist_train import _Comm
from .gcn import _pad_bias, _pad_rows
from .ktgnn import dropout_seed

__all__ = ["PartitionedGIN"]

_DEFAULT_HUB_CFG = (ops.GIN_HUB_THRESHOLD, ops.GIN_HUB_SEGMENT)


class _GinTables(_Layer):
    """device tables of one rank shared by every conv: `dist_sage._Layer`'s and the hub tables of both views"""

    def __init__(self, part, device, hub_cfg):
        super().__init__(part, device)
        self.hubs = self.t_hubs = None
        if hub_cfg is not None:
            thr, seg = int(hub_cfg[0]), int(hub_cfg[1])
            pick = lambda t: None if t is None else (thr, t[0], t[1], t[2])
            self.hubs = pick(self.csr.hub_tables(thr, seg))                # owned rows only: a halo slot has no in-edges
            self.t_hubs = pick(self.csr.transposed_hub_tables(thr, seg))   # owned and halo sources


def _transform_into(x, wp, buf, nl):
    """T = x wp^T of the owned rows into the front of buf [n_ext, pad4(D)] (`gcn._transform`'s two routes)"""
    if (ops.linear_supported(x.shape[1], wp.shape[0]) and x.dtype == torch.float32 and x.stride(1) == 1
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0):
        buf[:nl].copy_(ops.linear(x, wp, torch.zeros(wp.shape[0], dtype=torch.float32, device=x.device)))
    elif nl:
        torch.mm(x, wp.t(), out=buf[:nl])


def _conv_forward(ps, x, wp, bp, eps, D, epilogue, p_drop, seed, seed_dev):
    """one conv on this rank's rows: x [n_local, Din] -> (T_ext [n_ext, pad4(D)], y [n_local, pad4(D)])"""
    part, g = ps.part, ps.tables
    nl = part.n_local
    buf = torch.empty(part.n_ext, ops.pad4(D), dtype=torch.float32, device=x.device)
    _transform_into(x, wp, buf, nl)
    send = ops.gather_rows(buf, g.send_rows) if part.send_rows.shape[0] else buf.new_zeros(0, buf.shape[1])
    recv = ps.comm.all_to_all(send, part.send_splits, part.recv_splits)
    if part.n_halo:
        buf[nl:].copy_(recv)
    y = ops.gin_aggregate_hubs(buf, g.rowptr_local, g.col, eps, nl, D, bias=bp, epilogue=epilogue, p_drop=p_drop, seed=seed,
                               seed_dev=seed_dev, row_ids=g.owned_global if p_drop > 0 else None, hubs=g.hubs)
    return buf, y


def _conv_backward(ps, T, y, gy, eps, D, epilogue, p_drop, want_bias, want_eps):
    """grad_y [n_local, >= pad4(D)] of the owned rows -> (dT [n_local, pad4(D)] with the halo rows' share returned and folded in,
    this rank's grad_bias | None, this rank's grad_eps | None)"""
    part, g = ps.part, ps.tables
    nl = part.n_local
    dT, gb, ge = ops.gin_aggregate_bwd_hubs(T, y, gy, g.t_rowptr, g.t_dst, eps, part.n_ext, D, epilogue=epilogue, p_drop=p_drop,
                                            want_bias=want_bias, want_eps=want_eps, hubs=g.t_hubs)
    # reverse exchange: the halo slots' dT rows go back to their owners, who add them into their own rows
    ps.return_halo(dT[nl:], dT[:nl], ops.pad4(D))
    return dT[:nl], gb, ge


class _PartGinLayerFn(torch.autograd.Function):
    """the partitioned form of `gin._GinLayerFn`: y = epi((1 + eps) T + A T + b) on the owned rows, T = x W^T.  Kept: x, the padded
    weight, y, and (where eps trains) the extended table, whose front is T of the owned rows."""

    @staticmethod
    def forward(ctx, x, w, b, eps, ps, epilogue, p_drop, seed, seed_dev):
        D = w.shape[0]
        wp = _pad_rows(w.detach())
        xd = x.detach()
        T, y = _conv_forward(ps, xd, wp, _pad_bias(b.detach(), D) if b is not None else None, eps.detach(), D, epilogue, p_drop, seed,
                             seed_dev)
        want_eps = eps.requires_grad
        ctx.save_for_backward(xd, wp, eps)
        ctx.T = T[:ps.part.n_local] if want_eps else None
        ctx.y, ctx.ps, ctx.cfg = y, ps, (D, epilogue, p_drop, b is not None, want_eps)
        return y[:, :D]

    @staticmethod
    def backward(ctx, gy):
        x, wp, eps = ctx.saved_tensors
        D, epilogue, p_drop, has_b, want_eps = ctx.cfg
        ps, y = ctx.ps, ctx.y
        nl, Dp = ps.part.n_local, ops.pad4(D)
        if Dp != D or gy.dtype != torch.float32 or gy.stride(1) != 1 or gy.stride(0) % 4 != 0 or gy.data_ptr() % 16 != 0:
            gp = torch.zeros(nl, Dp, dtype=torch.float32, device=gy.device)
            gp[:, :D] = gy
            gy = gp
        dT, gb, ge = _conv_backward(ps, ctx.T, y, gy, eps.detach(), D, epilogue, p_drop, has_b and ctx.needs_input_grad[2],
                                    want_eps and ctx.needs_input_grad[3])
        dW = _gram_dw(dT, x)[:D] if ctx.needs_input_grad[1] else None
        gx = _dx(dT, wp) if ctx.needs_input_grad[0] else None
        return gx, dW, gb, (ge.reshape(eps.shape) if ge is not None else None), None, None, None, None, None


class PartitionedGIN(_RankModel):
    """`gin.GINNet` on rank `rank`'s rows of a destination-node partition (see the module docstring).

        pg = PartitionedGIN(model, edge_index, num_nodes, rank, world, device)
        out = pg.forward(x[pg.owned_global])                 # log-probs of the owned rows; differentiable when model.training
        loss = pg.nll_loss(out, y[pg.owned_global], train_mask[pg.owned_global])
        opt.zero_grad(); loss.backward(); pg.sync_grads(); opt.step()

    owner: int32 [num_nodes] owner rank of every node (default: contiguous blocks; `dist.partition_nodes(central_mask, world)`
    is accepted).  group: the torch.distributed group (a gloo group with CUDA tensors stages the payload through the host).
    hub_cfg: (threshold, segment) of the segmented hub rows and hub sources, or None to walk every row as one lane group."""

    def __init__(self, model, edge_index, num_nodes, rank, world, device, owner=None, group=None, hub_cfg=_DEFAULT_HUB_CFG,
                 graphed=False):
        if isinstance(edge_index, torch.Tensor):
            edge_index = edge_index.detach().cpu().numpy()
        self.model, self.rank, self.world, self.device, self.group = model, rank, world, torch.device(device), group
        if self.device.type != "cuda":
            raise RuntimeError(f"bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path (got device {self.device})")
        if graphed:
            raise NotImplementedError("PartitionedGIN(graphed=True): a partitioned epoch is not captured into a HIP graph")
        if hub_cfg is not None and (len(hub_cfg) != 2 or int(hub_cfg[0]) < 1 or int(hub_cfg[1]) < 1):
            raise ValueError(f"hub_cfg must be None or (threshold >= 1, segment >= 1), got {hub_cfg!r}")
        self.hub_cfg = None if hub_cfg is None else (int(hub_cfg[0]), int(hub_cfg[1]))
        self.part = SagePartition(edge_index, num_nodes, rank, world, owner=owner, rewrite_self_loops=False)
        self.tables = _GinTables(self.part, self.device, self.hub_cfg)
        self.comm = _Comm(group, device, world)
        self.owned_global = self.tables.owned_global
        self.n_local, self.n_halo, self.num_nodes = self.part.n_local, self.part.n_halo, int(num_nodes)
        self._x_ext = None                                   # `_RankModel`'s resident input halo: never filled here

    def forward(self, x_local):
        """x_local [n_local, F] (the rows of owned_global) -> log-probabilities [n_local, C] of the owned rows.  Training mode:
        dropout at model.dropout with the single-GPU masks, differentiable in the parameters; eval mode: the plain forward."""
        m = self.model
        if x_local.shape[0] != self.n_local:
            raise ValueError(f"x_local has {x_local.shape[0]} rows, this rank owns {self.n_local}")
        if not x_local.is_cuda:
            raise RuntimeError("bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path "
                               f"(got a {x_local.device} tensor)")
        p = m.dropout if m.training else 0.0
        x = x_local.float()
        L = len(m.convs)
        for ind, conv in enumerate(m.convs):
            last = ind == L - 1
            w, b, eps = conv.nn.weight, conv.nn.bias, conv.eps
            D = conv.out_channels
            torch_epi = last and D > 128
            epi = None if torch_epi else ("log_softmax" if last else "relu")
            kp = p if epi == "relu" else 0.0
            seed, seed_dev = dropout_seed(kp, step_word=False)             # as GINConv.run draws it
            if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)
                                            or eps.requires_grad):
                x = _PartGinLayerFn.apply(x, w, b, eps, self, epi, float(kp), seed, seed_dev)
            else:
                x = _conv_forward(self, x.detach(), _pad_rows(w.detach()), _pad_bias(b.detach(), D) if b is not None else None,
                                  eps.detach(), D, epi, float(kp), seed, seed_dev)[1][:, :D]
            if torch_epi:
                x = F.log_softmax(x, dim=1)
        return x

    __call__ = forward
