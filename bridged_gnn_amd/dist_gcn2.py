"""GCNII (`gcn2.GCN2`, reference models/backbones.py:163-197) on a destination-node partition: evaluation and the training step, one
process per GPU; new -- the reference is single-device.

Rank r owns a block of rows and all their in-edges of A' + I: `PartitionedGCN`'s partition, unchanged (`dist_gcn.GcnPartition` and
`_GcnTables`: one self loop per owned row, duplicates kept, `dinv_ext` the GLOBAL deg^-1/2 of the owned rows and of the halo slots,
hub tables of both views, send lists, fold segments).  The two Linear layers run on the owned rows alone, and so does x0 =
relu(lins[0](x)): the first thing that crosses ranks is the first conv's input, at hidden width, so NO input halo stays resident
(APPNP's saving; GCN and GraphSAGE keep the input features of their halo).
  * dropout: sites 0 (the input) and 1 (x0 on its way into the first conv) are `ops.feature_dropout(row_ids=owned_global)`, the conv
    sites are fused into `ops.gcn2_conv(row_ids=owned_global)` (bgnn_gcn2_conv_rows_f32); every site takes its seed in `GCN2.forward`'s
    order (`ktgnn.dropout_seed`) and hashes (seed, GLOBAL row * H + column): every rank draws the masks of the single-GPU step;
  * a conv: the layer's input lives in an extended buffer [n_ext, pad4(H)] whose front holds the owned rows.  `ops.gather_rows`
    packs the send list, ONE all_to_all of pad4(H) floats per send row, the received rows land in the buffer's tail; then one
    `ops.gcn2_conv` over the rectangular graph (n_local rows gathering from n_ext), which stores straight into the front of the NEXT
    layer's extended buffer.  No concatenation of own and halo rows: per layer the rank moves the kernel's bytes plus 4 pad4(H)
    bytes per send row (pack) and per halo row (land);
  * buffers: evaluation alternates TWO extended buffers (layer l reads one and writes the other's front).  Training gives every
    layer an extended buffer of its own, because its front is y, which the backward reads (y > 0 is the kept pattern), plus the
    layer's m [n_local, pad4(H)] and M;
  * backward of a conv (the partitioned `gcn2._Gcn2LayerFn`): gz, t, gx0 = `ops.gcn2_conv_bwd` on the owned rows; grad_weight1 =
    beta * gram(m, gz) is this rank's share; grad_x = A^ t is `ops.gcn_aggregate` over the by-source view with all n_ext sources
    (hub SOURCES among the halo slots included: `t_hubs`), the halo rows of the result go back to their owners (ONE all_to_all) and
    `ops.rows_segment_add` folds them in in a fixed order -- no atomics, a second run gives the same bits.  APPNP's alternative, a
    second partition of the flipped edges, would spare the fold pass but needs a second set of CSR, hub and send tables and a
    reorder of the rows on the way in and out of every layer's backward, for the same one exchange per layer: not taken;
  * hidden > 128 (`ops.gcn2_supported` false) composes on the rank as `GCN2Conv.run` does: `ops.gcn_aggregate` over the rectangular
    graph (backward through the by-source view and the fold), the mix, `addmm`, `ops.feature_dropout(relu=True, row_ids=...)`; this
    route copies the layer's input into the extended buffer (it pays four [n, H] passes on one GPU as well);
  * the loss is `nll_loss` (the GLOBAL normaliser), parameter gradients are summed in ONE `sync_grads`.
log_softmax is not fused into any kernel here, so the class count is not limited.  Out of scope (raise NotImplementedError):
`graphed=True`; `shared_weights=False` is refused by the model itself."""
import torch
import torch.nn.functional as F

from . import ops
from .appnp import _feature_drop, _rows4
from .dist_gcn import GcnPartition, _GcnTables
from .dist_sage import _RankModel
from .dist_train import _Comm
from .gcn2 import _mix_matrix
from .ktgnn import dropout_seed

__all__ = ["PartitionedGCN2"]


def _ext_rows(ps, H, device):
    return torch.empty(ps.part.n_ext, ops.pad4(H), dtype=torch.float32, device=device)


def _exchange(ps, buf):
    """the halo slots of buf [n_ext, W] <- the rows their owners hold in their own buf[:n_local]: pack, ONE all_to_all, land"""
    part, g = ps.part, ps.tables
    send = ops.gather_rows(buf, g.send_rows) if part.send_rows.shape[0] else buf.new_zeros(0, buf.shape[1])
    recv = ps.comm.all_to_all(send, part.send_splits, part.recv_splits)
    if part.n_halo:
        buf[part.n_local:].copy_(recv)


def _fill_front(ps, buf, x, H):
    """x [n_local, H] -> the front of buf, pad columns 0"""
    nl = ps.part.n_local
    buf[:nl, :H].copy_(x)
    if buf.shape[1] > H:
        buf[:nl, H:].zero_()


def _conv_forward(ps, cur, x0p, M, nxt, H, alpha, p_drop, seed, seed_dev, m_out=None):
    """one fused conv: cur [n_ext, pad4(H)] holds the owned rows in front, its tail is filled here; the owned rows of the layer's
    output go to the front of nxt"""
    part, g = ps.part, ps.tables
    _exchange(ps, cur)
    ops.gcn2_conv(cur, x0p, M, g.rowptr_local, g.col, g.dinv, part.n_local, H, alpha, p_drop=p_drop, seed=seed, seed_dev=seed_dev,
                  hubs=g.hubs, m_out=m_out, out=nxt[:part.n_local], row_ids=g.owned_global if p_drop > 0 else None)


def _walk_back(ps, t, H):
    """A^ t on the owned rows from t [n_local, pad4(H)] of the owned rows: the walk over the by-source view with all n_ext sources,
    the halo rows returned to their owners and folded in -> [n_local, pad4(H)]"""
    part, g = ps.part, ps.tables
    nl = part.n_local
    gx = ops.gcn_aggregate(t, g.t_rowptr, g.t_dst, g.dinv, part.n_ext, H, hubs=g.t_hubs)
    ps.return_halo(gx[nl:], gx[:nl], ops.pad4(H))
    return gx[:nl]


class _PartGcn2LayerFn(torch.autograd.Function):
    """the partitioned form of `gcn2._Gcn2LayerFn`: y = drop(relu(((1 - alpha) A^ x + alpha x0) M)) on the owned rows.  `cur`: the
    extended buffer whose front holds x's values (x itself only carries the gradient).  Kept: m, M and y, the front of the layer's own
    output buffer, which is left in `ps._ext_out` for the next layer.  y is kept as an attribute, not a saved tensor: the next layer's
    exchange lands its halo rows in the TAIL of that buffer in place, which moves the version counter the front shares with it."""

    @staticmethod
    def forward(ctx, x, x0, weight1, ps, cur, alpha, beta, p_drop, seed, seed_dev):
        H = weight1.shape[0]
        nl = ps.part.n_local
        M = _mix_matrix(weight1.detach().float(), beta)
        m = torch.empty(nl, ops.pad4(H), dtype=torch.float32, device=cur.device)
        nxt = _ext_rows(ps, H, cur.device)
        _conv_forward(ps, cur, _rows4(x0.detach(), H), M, nxt, H, alpha, p_drop, seed, seed_dev, m_out=m)
        y = nxt[:nl]
        ctx.save_for_backward(m, M)
        ctx.y, ctx.ps, ctx.cfg = y, ps, (H, alpha, beta, p_drop)
        ps._ext_out = nxt
        return y[:, :H]

    @staticmethod
    def backward(ctx, gy):
        m, M = ctx.saved_tensors
        H, alpha, beta, p_drop = ctx.cfg
        ps, y = ctx.ps, ctx.y
        Hp = ops.pad4(H)
        gz, t, gx0 = ops.gcn2_conv_bwd(y, _rows4(gy, H), M, H, alpha, p_drop)
        gw = gx = None
        if ctx.needs_input_grad[2]:
            gw = (ops.gram(m, gz) if ops.gram_supported(Hp, Hp) else m.t().mm(gz))[:H, :H] * beta
        if ctx.needs_input_grad[0]:
            gx = _walk_back(ps, t, H)[:, :H]
        return gx, (gx0[:, :H] if ctx.needs_input_grad[1] else None), gw, None, None, None, None, None, None, None


def _prop(ps, x, H):
    """A^ x on the owned rows (any width): x into the front of an extended buffer, the exchange, `ops.gcn_aggregate` over the
    rectangular graph"""
    part, g = ps.part, ps.tables
    buf = _ext_rows(ps, H, x.device)
    _fill_front(ps, buf, x, H)
    _exchange(ps, buf)
    return ops.gcn_aggregate(buf, g.rowptr_local, g.col, g.dinv, part.n_local, H, hubs=g.hubs)[:, :H]


class _PartPropFn(torch.autograd.Function):
    """a = A^ x on the owned rows; grad_x = A^ grad_a through the by-source view, the return exchange and the fold"""

    @staticmethod
    def forward(ctx, x, ps):
        ctx.ps = ps
        return _prop(ps, x.detach(), x.shape[1])

    @staticmethod
    def backward(ctx, ga):
        H = ga.shape[1]
        return _walk_back(ctx.ps, _rows4(ga, H), H)[:, :H], None


class PartitionedGCN2(_RankModel):
    """`gcn2.GCN2` on rank `rank`'s rows of a destination-node partition (see the module docstring).

        pg = PartitionedGCN2(model, edge_index, num_nodes, rank, world, device)
        out = pg.forward(x[pg.owned_global])                 # log-probs of the owned rows; differentiable when model.training
        loss = pg.nll_loss(out, y[pg.owned_global], train_mask[pg.owned_global])
        opt.zero_grad(); loss.backward(); pg.sync_grads(); opt.step()

    owner: int32 [num_nodes] owner rank of every node (default: contiguous blocks; `dist.partition_nodes(central_mask, world)`
    is accepted).  group: the torch.distributed group (a gloo group with CUDA tensors stages the payload through the host)."""

    def __init__(self, model, edge_index, num_nodes, rank, world, device, owner=None, group=None, graphed=False):
        if isinstance(edge_index, torch.Tensor):
            edge_index = edge_index.detach().cpu().numpy()
        self.model, self.rank, self.world, self.device, self.group = model, rank, world, torch.device(device), group
        if self.device.type != "cuda":
            raise RuntimeError(f"bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path (got device {self.device})")
        if graphed:
            raise NotImplementedError("PartitionedGCN2(graphed=True): a partitioned epoch is not captured into a HIP graph")
        self.part = GcnPartition(edge_index, num_nodes, rank, world, owner=owner)
        self.tables = _GcnTables(self.part, self.device)
        self.comm = _Comm(group, device, world)
        self.owned_global = self.tables.owned_global
        self.n_local, self.n_halo, self.num_nodes = self.part.n_local, self.part.n_halo, int(num_nodes)
        self._x_ext = None                                   # `_RankModel`'s resident input halo: never filled here
        self._ext_out = self._spare = None

    def _conv(self, conv, x, x0, cur, p):
        """drop(relu(conv(x, x0))) on the owned rows, as `GCN2Conv.run`.  cur: the extended buffer whose front holds x, or None (the
        composed route, which builds its own).  Returns (y [n_local, H], the extended buffer whose front is y | None)."""
        H, w = conv.channels, conv.weight1
        if not ops.gcn2_supported(H):
            if torch.is_grad_enabled() and x.requires_grad:
                a = _PartPropFn.apply(x, self)
            else:
                a = _prop(self, x.detach(), H)
            m = (1.0 - conv.alpha) * a + conv.alpha * x0
            z = torch.addmm(m, m, w, beta=1.0 - conv.beta, alpha=conv.beta)
            return _feature_drop(z, p, relu=True, row_ids=self.owned_global), None
        seed, seed_dev = dropout_seed(p, step_word=False)                  # as GCN2Conv.run draws it
        if cur is None:
            cur = _ext_rows(self, H, x.device)
            _fill_front(self, cur, x.detach(), H)
        if torch.is_grad_enabled() and (x.requires_grad or x0.requires_grad or w.requires_grad):
            y = _PartGcn2LayerFn.apply(x, x0, w, self, cur, conv.alpha, conv.beta, float(p), seed, seed_dev)
            nxt, self._ext_out = self._ext_out, None
            return y, nxt
        nxt = self._spare if self._spare is not None and self._spare.shape == cur.shape else _ext_rows(self, H, x.device)
        self._spare = cur                                                  # evaluation: two buffers alternate
        _conv_forward(self, cur, _rows4(x0.detach(), H), _mix_matrix(w.detach().float(), conv.beta), nxt, H, conv.alpha, float(p),
                      seed, seed_dev)
        return nxt[:self.n_local, :H], nxt

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
        ids = self.owned_global
        x = _feature_drop(x_local, p, relu=False, row_ids=ids)                            # site 0
        x0 = _feature_drop(m.lins[0](x), 0.0, relu=True).float()                          # x0: no mask, no seed
        x = _feature_drop(x0, p, relu=False, row_ids=ids)                                 # site 1
        cur, self._spare = None, None
        for conv in m.convs:
            x, cur = self._conv(conv, x, x0, cur, p)                                      # sites 2 .. L+1
        self._spare = None
        return F.log_softmax(m.lins[1](x), dim=1)

    __call__ = forward
