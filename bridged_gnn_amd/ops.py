"""Tensor-level wrappers over the C ABI (one Python function per entry point of include/bgnn.h).
Every function takes/returns CUDA(HIP) tensors on the current device and launches on torch's
current stream.  No CPU path exists: host tensors raise."""
import ctypes
import os

import torch

from . import _lib as L

__all__ = ["DstCSR", "build_dst_csr", "domain_delta", "pack_transform_heads", "adaptedconv_transform", "adaptedconv_aggregate", "linear", "linear_supported", "linear_narrow_supported", "linear_narrow_transform", "narrow_transform_finish", "gram", "gram_supported", "rowdot", "transform_bwd_prep", "topk_edges_coalesced",
           "l2_normalize_rows", "cosine_topk", "mlp_pair_topk", "topk_edges", "coalesce", "gather_rows", "pad4",
           "sage_mean_aggregate", "sage_mean_aggregate_bwd", "rows_segment_add", "gcn_aggregate", "gcn_aggregate_bwd", "gat_scores", "gat_aggregate", "gat_aggregate_bwd", "gatv2_aggregate", "gatv2_aggregate_bwd", "wide_heads_supported",
           "adaptedconv_aggregate_heads_wide", "adaptedconv_aggregate_heads_wide_bwd", "pair_csr", "pair_mlp_stats", "pair_mlp_loss",
           "pair_mlp_segsum", "pair_mlp_eval", "pair_mlp_count", "PAIR_MLP_WIDTH", "pair_cos_loss", "pair_cos_segsum", "pair_cos_count",
           "PAIR_COS_WIDTH"]


def pad4(n):
    return (int(n) + 3) // 4 * 4


# rows with at least this many in-edges are cut into segments of HUB_SEGMENT edges (AggParams::hub_threshold); tools/hub_sweep.py:
# config 3 (128, 64) 0.313 = (192, 64) 0.313, (192, 32) 0.330, (64, 32) 0.366 ms; config 2 (128, 64) 0.144, (192, 64) 0.155, off 0.162 ms
HUB_THRESHOLD = 128
HUB_SEGMENT = 64


class DstCSR:
    """By-destination CSR of the rewritten edge set: the build's replacement for the cached
    (edge_index1, edge_index2) pair of `KTGNN_no_complement.graph_partition`
    (reference models/KTGNN.py:385-398, :409-412).  Domain of a row = central_mask[row]."""

    def __init__(self, rowptr, col, eperm, num_edges, num_nodes):
        self.rowptr, self.col, self.eperm = rowptr, col, eperm
        self.num_edges, self.num_nodes = int(num_edges), int(num_nodes)
        self._transposed = None
        self._hubs = {}

    @staticmethod
    def _hub_tables_of(rowptr, N, threshold, segment):
        rp = rowptr[:N + 1].long()
        deg = rp[1:] - rp[:-1]
        hubs = torch.nonzero(deg >= threshold).reshape(-1)               # one-time sync, like the CSR build itself
        if hubs.numel() == 0:
            return None
        nseg = (deg[hubs] + segment - 1) // segment                       # segments per hub row
        seg_ptr = torch.zeros(hubs.numel() + 1, dtype=torch.int64, device=hubs.device)
        seg_ptr[1:] = torch.cumsum(nseg, 0)
        total = int(seg_ptr[-1].item())
        seg_hub = torch.repeat_interleave(torch.arange(hubs.numel(), device=hubs.device), nseg)   # hub index of a segment
        seg_in_hub = torch.arange(total, device=hubs.device) - seg_ptr[seg_hub]
        start = rp[hubs][seg_hub] + seg_in_hub * segment
        end = torch.minimum(start + segment, rp[hubs + 1][seg_hub])
        # hub rows are not adjacent in the edge arrays, so a segment carries its own (begin, end) pair: v -> bounds[2v], bounds[2v+1]
        bounds = torch.stack((start, end), dim=1).reshape(-1)
        return (hubs.to(torch.int32).contiguous(), seg_ptr.to(torch.int32).contiguous(),
                bounds.to(torch.int32).contiguous(), hubs[seg_hub].to(torch.int32).contiguous())

    def hub_tables(self, threshold=HUB_THRESHOLD, segment=HUB_SEGMENT):
        """Rows with >= `threshold` in-edges, cut into segments of <= `segment` edges, built once per graph:
        None when the graph has no such row, else (hub_rows [nh], hub_seg_ptr [nh+1], seg_bounds [2 nseg] = (begin, end) edge
        offsets into `col` per segment, seg_node [nseg]), int32 device tensors (see bgnn_adaptedconv_aggregate_hub_f32)."""
        key = (int(threshold), int(segment))
        if key not in self._hubs:
            self._hubs[key] = DstCSR._hub_tables_of(self.rowptr, self.num_nodes, threshold, segment)
        return self._hubs[key]

    def transposed_hub_tables(self, threshold=HUB_THRESHOLD, segment=HUB_SEGMENT):
        """the same over the by-SOURCE view (`transposed()`): sources with >= `threshold` out-edges; offsets into t_eid / t_dst"""
        key = ("t", int(threshold), int(segment))
        if key not in self._hubs:
            self._hubs[key] = DstCSR._hub_tables_of(self.transposed()[0], self.num_nodes, threshold, segment)
        return self._hubs[key]

    def tile_need(self, mask_u8, rows_per_tile=32, table_mask_u8=None):
        """Per 32-row tile: which of a node's two transformed rows does the aggregation over THIS graph ever read?  bit 0 = h_s2t
        (gathered by target-domain destinations, KTGNN.py:293,:295), bit 1 = h_t2s (source-domain destinations, :292,:294); a
        row's own table counts (the logit reads h_i).  -> int32 [ceil(rows / 32)] for `adaptedconv_transform(tile_need=...)`, or
        None when every tile needs both tables.  Built once per (graph, mask); with s -> t bridge edges only, no target node
        feeds a source destination and the target half of h_t2s is never read.
        `table_mask_u8` (a rank's graph: destinations = its own rows, tables = own rows followed by halo rows): the domain flags of
        ALL table rows; the tiles then cover the extended tables and a halo row counts only where an edge reads it."""
        key = (mask_u8.data_ptr(), mask_u8._version, int(rows_per_tile), None if table_mask_u8 is None else table_mask_u8.data_ptr())
        c = getattr(self, "_tile_need", None)
        if c is None or c[0] != key:
            E, N = self.num_edges, self.num_nodes
            R = N if table_mask_u8 is None else int(table_mask_u8.shape[0])      # rows of the tables
            m = mask_u8[:N].bool()
            deg = (self.rowptr[1:N + 1] - self.rowptr[:N]).long()
            dst_s = torch.repeat_interleave(m, deg)                       # domain of every edge's destination (by-destination order)
            col = self.col[:E].long()
            need_t2s = torch.zeros(R, dtype=torch.bool, device=m.device)
            need_s2t = torch.zeros(R, dtype=torch.bool, device=m.device)
            need_t2s[:N], need_s2t[:N] = m, ~m
            need_t2s[col[dst_s]] = True
            need_s2t[col[~dst_s]] = True
            T = (R + rows_per_tile - 1) // rows_per_tile
            pad = T * rows_per_tile - R

            def tiles(v):
                v = torch.cat((v, v.new_zeros(pad))) if pad else v
                return v.view(T, rows_per_tile).any(1)
            need = (tiles(need_s2t).to(torch.int32) | (tiles(need_t2s).to(torch.int32) << 1)).contiguous()
            full = bool((need == 3).all().item())                         # one-time sync, like the CSR build
            self._tile_need = c = (key, None if full else need, mask_u8, table_mask_u8)  # (masks kept alive: the key holds their addresses)
        return c[1]

    def gather_hint(self, window=1024, samples=64):
        """1: neighbouring destination rows share neighbours (the aggregation's gathers live off the L2s), 2: they do not (HBM-bound
        gathers) -- `bgnn_adaptedconv_aggregate_bounded_f32(gather_hint=...)`.  Measured once per graph: over `samples` evenly spaced
        windows of `window` consecutive destination rows (about what one XCD has in flight), reuse = 1 - distinct neighbour ids / edges."""
        if getattr(self, "_gather_hint", None) is None:
            N, E = self.num_nodes, self.num_edges
            hint = 1
            if N > 4 * window and E > 0:
                starts = torch.linspace(0, N - window, samples, device=self.rowptr.device).long()
                rp = self.rowptr.long()
                tot = dist = 0
                b, e = rp[starts].tolist(), rp[starts + window].tolist()            # one-time sync, like tile_need / the CSR build
                for lo, hi in zip(b, e):
                    if hi > lo:
                        tot += hi - lo
                        dist += int(torch.unique(self.col[lo:hi]).numel())
                if tot > 0 and 1.0 - dist / tot < 0.3:
                    hint = 2
            self._gather_hint = hint
        return self._gather_hint

    def transposed(self):
        """By-SOURCE view of the same edges, built once per graph (training only): (t_rowptr [N+1], t_eid [E'] = position
        of the edge in the by-destination order, t_dst [E'] = its destination), int32.  The atomic-free aggregation
        backward gathers over it instead of scattering with float atomics."""
        if self._transposed is None:
            E, N = self.num_edges, self.num_nodes
            col = self.col[:E].long()
            deg_in = (self.rowptr[1:] - self.rowptr[:-1]).long()
            dst = torch.repeat_interleave(torch.arange(N, device=col.device), deg_in)
            order = torch.sort(col, stable=True).indices
            t_rowptr = torch.zeros(N + 1, dtype=torch.int64, device=col.device)
            t_rowptr[1:] = torch.cumsum(torch.bincount(col, minlength=N), 0)
            self._transposed = (t_rowptr.to(torch.int32).contiguous(), order.to(torch.int32).contiguous(),
                                dst[order].to(torch.int32).contiguous())
        return self._transposed


def build_dst_csr(edge_index, num_nodes, rewrite_self_loops=True, want_eperm=False):
    """edge_index int64 [2,E] (CUDA) -> DstCSR.  One D2H read of E' (the CSR is built once per graph
    and cached, like the reference caches graph_partition)."""
    lib = L.lib()
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must be int64 [2, E]")
    ei = edge_index.contiguous()
    E, N = int(ei.shape[1]), int(num_nodes)
    dev = ei.device
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E + N, dtype=torch.int32, device=dev)
    eperm = torch.empty(E + N, dtype=torch.int32, device=dev) if want_eperm else None
    e_out = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = lib.bgnn_csr_workspace_bytes(N, E)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.bgnn_build_dst_csr(L.ptr(ei) if E > 0 else None, E, N, 1 if rewrite_self_loops else 0, L.ptr(rowptr),
                                L.ptr(col), L.ptr(eperm), L.ptr(e_out), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_build_dst_csr")
    ne = int(e_out.item())
    return DstCSR(rowptr, col[:ne], eperm[:ne] if want_eperm else None, ne, N)


class ZeroArena:
    """One zero-filled float64 allocation per forward that hands out the [2*Din+2] accumulators of `domain_sums` and of
    the `colsum` epilogues (one fill launch instead of one per accumulator)."""

    def __init__(self, device, doubles):
        self.buf = torch.zeros(int(doubles), dtype=torch.float64, device=device)
        self.used = 0

    def take(self, n):
        n = int(n)
        if self.used + n > self.buf.numel():            # undersized arena: still correct, one more fill
            return torch.zeros(n, dtype=torch.float64, device=self.buf.device)
        t = self.buf[self.used: self.used + n]
        self.used += (n + 1) // 2 * 2                   # keep slices 16-byte aligned
        return t


def domain_sums(x, mask_u8, out=None, deterministic=False):
    """Per-domain column sums + counts as a float64 [2*Din+2] tensor (all-reducible).  `out`: zero-filled accumulator.
    `deterministic`: the two-stage form (per-block partial rows + a second small launch, no atomics: run-to-run
    bit-identical); measured the same speed at C4 size and no faster on a rank's share, so the one-launch form stays
    the default."""
    lib = L.lib()
    N, Din = x.shape
    sums = torch.zeros(2 * Din + 2, dtype=torch.float64, device=x.device) if out is None else out
    assert sums.numel() == 2 * Din + 2 and sums.dtype == torch.float64
    if not deterministic:
        rc = lib.bgnn_domain_sums_f64(L.ptr(x), N, Din, x.stride(0), L.ptr(mask_u8), L.ptr(sums), L.stream())
        L.check(rc, "bgnn_domain_sums_f64")
        return sums
    ws = torch.empty(lib.bgnn_domain_sums_workspace_bytes(Din), dtype=torch.uint8, device=x.device)   # per call (see _tile_queue)
    rc = lib.bgnn_domain_sums_ws_f64(L.ptr(x), N, Din, x.stride(0), L.ptr(mask_u8), L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_domain_sums_ws_f64")
    return sums


def column_sums(x):
    """sum over the rows of x [N, D] (fp64 accumulation, D % 4 == 0 and a 16-byte aligned, row-contiguous x) -> float32 [D]: the bias
    gradient of a Linear.  One streaming launch of the domain-sums kernel with every row in one domain; torch's `x.sum(0)` is a
    multi-block reduction whose semaphore buffer is cleared by a memset node when captured into a HIP graph (see bgnn_zero_async)."""
    N, D = x.shape
    mask = torch.zeros(N, dtype=torch.uint8, device=x.device)
    return domain_sums(x, mask)[D:2 * D].float()


def total_sum(x):
    """sum of all elements of a float32 tensor as a 0-dim float32 tensor, through `column_sums` (no torch multi-block reduction: safe
    inside a captured training step, see `KTGNN_no_complement.graphed_train_step`).  Differentiable (d/dx = 1)."""
    return _TotalSumFn.apply(x)


class _TotalSumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = x.shape
        flat = x.contiguous().view(-1)
        pad = (-flat.numel()) % 64
        if pad:
            flat = torch.cat((flat, flat.new_zeros(pad)))
        return column_sums(flat.view(-1, 64)).sum()          # 64 values: a single-block reduction

    @staticmethod
    def backward(ctx, g):
        return g.expand(ctx.shape)


def domain_delta(sums, Din):
    delta = torch.empty(Din, dtype=torch.float32, device=sums.device)
    rc = L.lib().bgnn_domain_delta_f32(L.ptr(sums), Din, L.ptr(delta), L.stream())
    L.check(rc, "bgnn_domain_delta_f32")
    return delta


def linear_supported(din, dout):
    """envelope of `linear` (the W-stationary MFMA kernel): Din <= 128, Din % 4 == 0, Dout % 64 == 0."""
    return din <= 128 and din % 4 == 0 and dout % 64 == 0


def linear(x, weight, bias, relu=False, mask_u8=None, colsum=None):
    """relu?(x @ weight.T + bias) (KTGNN.py:407-411/:433, clf_transformer's first Linear with eval BatchNorm folded in);
    `colsum` (zeroed float64 [2*Dout+2], needs mask_u8) also receives the per-domain column sums of the result."""
    N, din = x.shape
    dout = weight.shape[0]
    out = torch.empty(N, dout, dtype=torch.float32, device=x.device)
    rc = L.lib().bgnn_linear_f32(L.ptr_rows(x), N, din, x.stride(0), L.ptr(weight), L.ptr(bias), dout, 1 if relu else 0,
                                 L.ptr(mask_u8), L.ptr(colsum), L.ptr(out), dout, L.stream())
    L.check(rc, "bgnn_linear_f32")
    return out


def linear_narrow_supported(din, dout, packed):
    """envelope of `linear_narrow_transform`: W-stationary kernel with the whole activation row in one column group, and a
    consumer conv of one head with D <= 4."""
    Wp, bp, gates, D, ldh, gconst = packed
    return (din <= 128 and din % 4 == 0 and dout in (64, 128, 256) and gates.shape[0] == 1 and ldh == 4
            and Wp.shape == (8, dout))


def linear_narrow_transform(x, weight, bias, mask_u8, colsum, packed, relu=True):
    """Stage A of the fused clf_transformer -> clf_target path (KTGNN.py:433): raw [N,12] per-row products of
    a = relu?(x W^T + b) with the consumer conv's packed rows and gate vectors, `colsum` (zeroed float64 [2*Dout+2])
    += the per-domain column sums of a.  The activation itself is never written."""
    N, din = x.shape
    dout = weight.shape[0]
    Wp, bp, gates, D, ldh, gconst = packed
    raw = torch.empty(N, 12, dtype=torch.float32, device=x.device)
    rc = L.lib().bgnn_linear_narrow_transform_f32(L.ptr_rows(x), N, din, x.stride(0), L.ptr(weight), L.ptr(bias), dout,
                                                  1 if relu else 0, L.ptr(mask_u8), L.ptr(colsum), L.ptr(Wp), L.ptr(gates),
                                                  L.ptr(raw), L.stream())
    L.check(rc, "bgnn_linear_narrow_transform_f32")
    return raw


def classifier_stage_supported(x, packed_pair, weight, packed_t):
    """envelope of `classifier_stage` (bgnn.h: bgnn_classifier_stage_f32)"""
    Wp, bp, gates, D, ldh, gconst = packed_pair
    din = x.shape[1]
    return (x.is_cuda and x.dtype == torch.float32 and x.stride(1) == 1 and 64 < din <= 128 and din % 4 == 0
            and weight.shape == (128, din) and Wp.shape[0] <= 24 and Wp.shape[1] == din and packed_t[0].shape == (8, 128)
            and os.environ.get("BGNN_FUSED_CLS", "1") != "0")


def classifier_stage(x, mask_u8, sums_x, packed_pair, outs, weight, bias, colsum, packed_t, relu=True, rows32=None):
    """ONE pass over the hidden activation x for the whole classifier stage's dense work (KTGNN.py:432-434): the narrow
    (h_t2s, h_s2t) tables of the convs in `packed_pair` (clf_base, clf_target on x; `outs` = list of (h_t2s, h_s2t) views) and
    stage A of the fused clf_transformer -> clf_target path (`linear_narrow_transform`: -> raw [N, 12], `colsum` += the
    per-domain column sums of the activation).
    `rows32` = (t2s, s2t), two [>= N, 8] tables of 32-byte rows, instead of `outs`: both heads' two columns go to the rows' first
    16 bytes (bgnn.h: bgnn_classifier_stage_rows32_f32)."""
    N, din = x.shape
    Wp, bp, gates, D, ldh, gconst = packed_pair
    H = gates.shape[0]
    Wp2, _, gates2, _, _, _ = packed_t
    raw = torch.empty(N, 12, dtype=torch.float32, device=x.device)
    small = torch.empty(H * (2 * ldh + 2) + 8, dtype=torch.float32, device=x.device)
    if rows32 is not None:
        t2s, s2t = rows32
        assert H == 2 and ldh == 4 and D <= 2 and t2s.shape[0] >= N and s2t.shape[0] >= N and t2s.stride(0) == s2t.stride(0)
        rc = L.lib().bgnn_classifier_stage_rows32_f32(L.ptr_rows(x), N, din, x.stride(0), L.ptr(mask_u8), L.ptr(sums_x), D, L.ptr(Wp),
                                                      L.ptr(bp), L.ptr(gates), L.ptr(gconst), L.ptr_rows(s2t), L.ptr_rows(t2s),
                                                      t2s.stride(0), L.ptr(weight), L.ptr(bias), weight.shape[0], 1 if relu else 0,
                                                      L.ptr(colsum), L.ptr(Wp2), L.ptr(gates2), L.ptr(raw), L.ptr(small), L.stream())
        L.check(rc, "bgnn_classifier_stage_rows32_f32")
        return raw
    row_stride = outs[0][0].stride(0)
    for a, b in outs:
        assert a.shape[0] >= N and b.shape[0] >= N and a.stride(0) == row_stride and b.stride(0) == row_stride
    o1 = outs[1] if H > 1 else (None, None)
    rc = L.lib().bgnn_classifier_stage_f32(L.ptr_rows(x), N, din, x.stride(0), L.ptr(mask_u8), L.ptr(sums_x), H, D, L.ptr(Wp), L.ptr(bp),
                                           L.ptr(gates), L.ptr(gconst), L.ptr_rows(outs[0][1]), L.ptr_rows(outs[0][0]),
                                           L.ptr_rows(o1[1]), L.ptr_rows(o1[0]), ldh, row_stride, L.ptr(weight), L.ptr(bias),
                                           weight.shape[0], 1 if relu else 0, L.ptr(colsum), L.ptr(Wp2), L.ptr(gates2), L.ptr(raw),
                                           L.ptr(small), L.stream())
    L.check(rc, "bgnn_classifier_stage_f32")
    return raw


def narrow_transform_finish(raw, mask_u8, sums, packed, out, rows32=False):
    """Stage B: raw [N,12] + the (all-reduced) domain sums of the activation -> the conv's (h_t2s, h_s2t) rows in `out`
    (two [>=N, 4] views with a common row stride).  `rows32`: `out` is the second half of 32-byte rows, columns D.. are +0."""
    Wp, bp, gates, D, ldh, gconst = packed
    h_t2s, h_s2t = out
    N = raw.shape[0]
    assert h_t2s.stride(0) == h_s2t.stride(0) and sums.dtype == torch.float64 and sums.numel() == 2 * Wp.shape[1] + 2
    assert not rows32 or D <= 2
    small = torch.empty(16, dtype=torch.float32, device=raw.device)
    name = "bgnn_narrow_transform_finish_rows32_f32" if rows32 else "bgnn_narrow_transform_finish_f32"
    rc = getattr(L.lib(), name)(L.ptr(raw), N, L.ptr(mask_u8), L.ptr(sums), Wp.shape[1], L.ptr(Wp), L.ptr(bp),
                                L.ptr(gates), L.ptr(gconst), L.ptr_rows(h_s2t), L.ptr_rows(h_t2s),
                                h_t2s.stride(0), L.ptr(small), L.stream())
    L.check(rc, name)
    return out


def transform_bwd_prep(x, G_s2t, G_t2s, D, mask_u8, gx, gconst, wd, counts, out=None, want_ex=False):
    """-> (Gall [N, pad4(2D+3)], side [N, 4]): the row-local part of the transform backward in one pass (see bgnn.h);
    `counts` = float64 [2] (n_S, n_T), e.g. the tail of the domain sums.  `out` = (Gall view, side view or None): column
    slices of wider buffers when several convs on the same x share the launches that follow.
    want_ex (D <= 128): -> (Gall, ex [p, 4]) instead -- the used entries of Gall^T side from the same pass, no side buffer."""
    N, din = x.shape
    p = pad4(2 * D + 3)
    assert counts.dtype == torch.float64 and counts.numel() == 2
    if out is None:
        Gall = torch.empty(N, p, dtype=torch.float32, device=x.device)
        side = None if want_ex else torch.empty(N, 4, dtype=torch.float32, device=x.device)
    else:
        Gall, side = out
        assert Gall.shape == (N, p) and (side is None or side.shape == (N, 4))
    assert G_s2t.stride(0) == G_t2s.stride(0) and G_s2t.stride(1) == 1 and G_t2s.stride(1) == 1
    lib = L.lib()
    ex = ws = None
    wsb = 0
    if want_ex:
        ex = torch.empty(p, 4, dtype=torch.float32, device=x.device)
        wsb = lib.bgnn_transform_bwd_prep_workspace_bytes(N, p)
        ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    rc = lib.bgnn_transform_bwd_prep_f32(L.ptr_rows(x), x.stride(0), N, din, L.ptr_rows(G_s2t), L.ptr_rows(G_t2s),
                                         G_s2t.stride(0), D, L.ptr(mask_u8), L.ptr(gx), L.ptr(gconst), L.ptr(wd),
                                         L.ptr(counts), L.ptr_rows(Gall), p, Gall.stride(0),
                                         L.ptr_rows(side) if side is not None else None, side.stride(0) if side is not None else 4,
                                         L.ptr(ex), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_transform_bwd_prep_f32")
    return (Gall, ex) if want_ex else (Gall, side)


def transform_bwd_consts(W_s, W_t, g1, g2, delta, din):
    """-> (gx [2, din], gconst [2], wd [2, 2D]): the small operands of `transform_bwd_prep` in one launch (see bgnn.h)."""
    D = W_s.shape[0]
    dev = W_s.device
    gx = torch.empty(2, din, dtype=torch.float32, device=dev)
    gconst = torch.empty(2, dtype=torch.float32, device=dev)
    wd = torch.empty(2, 2 * D, dtype=torch.float32, device=dev)
    rc = L.lib().bgnn_transform_bwd_consts_f32(L.ptr(W_s), L.ptr(W_t), L.ptr(g1), L.ptr(g2), L.ptr(delta), D, din,
                                               L.ptr(gx), L.ptr(gconst), L.ptr(wd), L.stream())
    L.check(rc, "bgnn_transform_bwd_consts_f32")
    return gx, gconst, wd


def transform_bwd_finish(dWall, ex, W_s, W_t, g1, g2, delta, din, wcat_t):
    """-> (dW_s, dW_t, dg1 [2 din], dg2 [2 din], db_s, db_t); fills wcat_t ([din, p] view, unit column stride): see bgnn.h."""
    D = W_s.shape[0]
    p = dWall.shape[0]
    dev = W_s.device
    dW_s, dW_t = torch.empty(D, din, dtype=torch.float32, device=dev), torch.empty(D, din, dtype=torch.float32, device=dev)
    dg1, dg2 = torch.empty(2 * din, dtype=torch.float32, device=dev), torch.empty(2 * din, dtype=torch.float32, device=dev)
    db_s, db_t = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
    assert dWall.is_contiguous() and ex.is_contiguous() and wcat_t.shape == (din, p) and wcat_t.stride(1) == 1
    rc = L.lib().bgnn_transform_bwd_finish_f32(L.ptr(dWall), L.ptr(ex), L.ptr(W_s), L.ptr(W_t), L.ptr(g1), L.ptr(g2), L.ptr(delta),
                                               D, din, p, L.ptr(dW_s), L.ptr(dW_t), L.ptr(dg1), L.ptr(dg2), L.ptr(db_s), L.ptr(db_t),
                                               L.ptr_rows(wcat_t), wcat_t.stride(0), L.stream())
    L.check(rc, "bgnn_transform_bwd_finish_f32")
    return dW_s, dW_t, dg1, dg2, db_s, db_t


def gram_supported(p, q):
    return 0 < p <= 288 and 0 < q <= 128 and p % 4 == 0 and q % 4 == 0


def gram(A, B):
    """A^T B for tall-skinny row-major A [N,p], B [N,q] (the node count is the reduction dimension): the weight-gradient
    products of the training path (KTGNN.py:275-284 under autograd)."""
    N, p = A.shape
    q = B.shape[1]
    lib = L.lib()
    wsb = lib.bgnn_gram_workspace_bytes(p, q)
    ws = torch.empty(wsb, dtype=torch.uint8, device=A.device)
    out = torch.empty(p, q, dtype=torch.float32, device=A.device)
    rc = lib.bgnn_gram_f32(L.ptr_rows(A), A.stride(0), p, L.ptr_rows(B), B.stride(0), q, N, L.ptr(out), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_gram_f32")
    return out


def bn_relu_dropout_supported(x):
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] % 4 == 0
            and 4 <= x.shape[1] <= 1024 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)


def bn_relu_dropout(x, gamma, beta, eps, relu, p_drop, seed, momentum=0.0, running_mean=None, running_var=None, seed_dev=None):
    """Training-mode BatchNorm1d -> ReLU -> dropout (KTGNN.py:420-430) -> (y, stats); `stats` (fp64 column sums of x | x^2)
    is what the backward needs besides x.  `seed_dev`: optional int64 device tensor [1] added to `seed` inside the kernels (the step
    counter of a captured training step)."""
    N, D = x.shape
    y = torch.empty(N, D, dtype=torch.float32, device=x.device)
    stats = torch.empty(L.lib().bgnn_bn_acc_doubles(D), dtype=torch.float64, device=x.device)   # R x [2D] partial accumulators
    rc = L.lib().bgnn_bn_relu_dropout_f32(L.ptr_rows(x), N, D, x.stride(0), L.ptr(gamma) if gamma is not None else None,
                                          L.ptr(beta) if beta is not None else None, float(eps), int(bool(relu)), float(p_drop),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(seed_dev) if seed_dev is not None else None, float(momentum),
                                          L.ptr(running_mean) if running_mean is not None else None,
                                          L.ptr(running_var) if running_var is not None else None,
                                          L.ptr(y), D, L.ptr(stats), L.stream())
    L.check(rc, "bgnn_bn_relu_dropout_f32")
    return y, stats


def bn_relu_dropout_bwd(x, grad_y, stats, gamma, beta, eps, relu, p_drop, seed, seed_dev=None):
    """-> (dL/dx [N,D], gsum fp64 [2*D] = dL/dbeta | dL/dgamma)."""
    N, D = x.shape
    gx = torch.empty(N, D, dtype=torch.float32, device=x.device)
    gsum = torch.empty(L.lib().bgnn_bn_acc_doubles(D), dtype=torch.float64, device=x.device)
    rc = L.lib().bgnn_bn_relu_dropout_bwd_f32(L.ptr_rows(x), L.ptr_rows(grad_y), N, D, x.stride(0), grad_y.stride(0), L.ptr(stats),
                                              L.ptr(gamma) if gamma is not None else None, L.ptr(beta) if beta is not None else None,
                                              float(eps), int(bool(relu)), float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              L.ptr(seed_dev) if seed_dev is not None else None,
                                              L.ptr(gx), D, L.ptr(gsum), L.stream())
    L.check(rc, "bgnn_bn_relu_dropout_bwd_f32")
    return gx, gsum.view(-1, 2 * D).sum(0)


# ---- the same layer in four phases for a node partition (include/bgnn.h: the *_rows entries): a rank reduces its rows, the caller
#      all-reduces the [2 * D] doubles, the apply passes take the totals over all ranks, the global row count and the global row
#      numbers (`row_ids` int64 [n_rows], or `row_base` + local row) that fix the dropout counter
def _bn_rows_args(x, totals, n_total, gamma, beta, eps, relu, p_drop, seed, seed_dev, row_ids, row_base):
    D = x.shape[1]
    if totals.dtype != torch.float64 or totals.numel() != 2 * D:
        raise RuntimeError(f"totals must be {2 * D} doubles (sum x | sum x^2 over all ranks' rows)")
    if row_ids is not None and (row_ids.dtype != torch.int64 or row_ids.numel() != x.shape[0]):
        raise RuntimeError("row_ids must hold one int64 global row number per local row")
    return (L.ptr(totals), int(n_total), L.ptr(gamma) if gamma is not None else None, L.ptr(beta) if beta is not None else None,
            float(eps), int(bool(relu)), float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(seed_dev) if seed_dev is not None else None,
            L.ptr(row_ids) if row_ids is not None else None, int(row_base))


def bn_colstats(x):
    """-> fp64 [2 * D]: the column sums of x | x^2 over this rank's rows (zeros for no rows)"""
    N, D = x.shape
    acc = torch.empty(L.lib().bgnn_bn_acc_doubles(D), dtype=torch.float64, device=x.device)
    L.check(L.lib().bgnn_bn_colstats_f32(L.ptr_rows(x), N, D, x.stride(0), L.ptr(acc), L.stream()), "bgnn_bn_colstats_f32")
    return acc.view(-1, 2 * D).sum(0)


def bn_apply_rows(x, totals, n_total, gamma, beta, eps, relu, p_drop, seed, row_ids=None, row_base=0, momentum=0.0, running_mean=None,
                  running_var=None, seed_dev=None):
    """-> y [n_rows, D]: BatchNorm1d(train) -> ReLU -> dropout of this rank's rows from the totals over `n_total` rows of all ranks"""
    N, D = x.shape
    y = torch.empty(N, D, dtype=torch.float32, device=x.device)
    a = _bn_rows_args(x, totals, n_total, gamma, beta, eps, relu, p_drop, seed, seed_dev, row_ids, row_base)
    rc = L.lib().bgnn_bn_apply_rows_f32(L.ptr_rows(x), N, D, x.stride(0), *a, float(momentum),
                                        L.ptr(running_mean) if running_mean is not None else None,
                                        L.ptr(running_var) if running_var is not None else None, L.ptr(y), D, L.stream())
    L.check(rc, "bgnn_bn_apply_rows_f32")
    return y


def bn_bwd_reduce_rows(x, grad_y, totals, n_total, gamma, beta, eps, relu, p_drop, seed, row_ids=None, row_base=0, seed_dev=None):
    """-> fp64 [2 * D]: this rank's share of sum g' (= dL/dbeta) | sum g'.xhat (= dL/dgamma)"""
    N, D = x.shape
    gacc = torch.empty(L.lib().bgnn_bn_acc_doubles(D), dtype=torch.float64, device=x.device)
    a = _bn_rows_args(x, totals, n_total, gamma, beta, eps, relu, p_drop, seed, seed_dev, row_ids, row_base)
    rc = L.lib().bgnn_bn_bwd_reduce_rows_f32(L.ptr_rows(x), L.ptr_rows(grad_y), N, D, x.stride(0), grad_y.stride(0), *a, L.ptr(gacc), L.stream())
    L.check(rc, "bgnn_bn_bwd_reduce_rows_f32")
    return gacc.view(-1, 2 * D).sum(0)


def bn_bwd_apply_rows(x, grad_y, totals, gtotals, n_total, gamma, beta, eps, relu, p_drop, seed, row_ids=None, row_base=0, seed_dev=None):
    """-> dL/dx [n_rows, D] from the all-reduced pair of `bn_bwd_reduce_rows`"""
    N, D = x.shape
    if gtotals.dtype != torch.float64 or gtotals.numel() != 2 * D:
        raise RuntimeError(f"gtotals must be {2 * D} doubles (sum g' | sum g'.xhat over all ranks' rows)")
    gx = torch.empty(N, D, dtype=torch.float32, device=x.device)
    a = _bn_rows_args(x, totals, n_total, gamma, beta, eps, relu, p_drop, seed, seed_dev, row_ids, row_base)
    rc = L.lib().bgnn_bn_bwd_apply_rows_f32(L.ptr_rows(x), L.ptr_rows(grad_y), N, D, x.stride(0), grad_y.stride(0), a[0], L.ptr(gtotals), *a[1:],
                                            L.ptr(gx), D, L.stream())
    L.check(rc, "bgnn_bn_bwd_apply_rows_f32")
    return gx


def rowdot(X, V):
    """X [N,d] (unit column stride, 16-B aligned rows) times up to four vectors V [nv,d] -> [N,nv] in one pass over X."""
    N, d = X.shape
    nv = V.shape[0]
    out = torch.empty(N, nv, dtype=torch.float32, device=X.device)
    rc = L.lib().bgnn_rowdot_f32(L.ptr_rows(X), X.stride(0), N, d, L.ptr(V), V.stride(0), nv, L.ptr(out), L.stream())
    L.check(rc, "bgnn_rowdot_f32")
    return out


def pack_transform_heads(heads, din_pad):
    """Pack 1-2 convs that share an input for `adaptedconv_transform`.  `heads` = list of dicts with
    W_s, b_s, W_t, b_t ([D, Din] / [D] or None) and g_s2t, g_t2s ([2*Din], [x || delta] order).
    Optional per head: "gate_const" = (c_s2t, c_t2s) added to the gate pre-activations.
    -> (Wp [H*2*ldh, din_pad], bias_p [H*2*ldh], gates [H, 2, 2*din_pad], D, ldh, gate_const [H, 2])."""
    D = heads[0]["W_s"].shape[0]
    din = heads[0]["W_s"].shape[1]
    ldh = pad4(D)
    dev = heads[0]["W_s"].device
    H = len(heads)
    Wp = torch.zeros(H * 2 * ldh, din_pad, dtype=torch.float32, device=dev)
    bp = torch.zeros(H * 2 * ldh, dtype=torch.float32, device=dev)
    gates = torch.zeros(H, 2, 2 * din_pad, dtype=torch.float32, device=dev)
    gconst = torch.zeros(H, 2, dtype=torch.float32, device=dev)
    for h, hd in enumerate(heads):
        if hd.get("gate_const") is not None:
            gconst[h, 0], gconst[h, 1] = hd["gate_const"]
        base = h * 2 * ldh
        Wp[base: base + D, :din] = hd["W_t"]
        Wp[base + ldh: base + ldh + D, :din] = hd["W_s"]
        if hd.get("b_t") is not None:
            bp[base: base + D] = hd["b_t"]
        if hd.get("b_s") is not None:
            bp[base + ldh: base + ldh + D] = hd["b_s"]
        for t, key in enumerate(("g_s2t", "g_t2s")):
            g = hd[key].reshape(-1)
            gates[h, t, :din] = g[:din]
            gates[h, t, din_pad: din_pad + din] = g[din:]
    return Wp, bp, gates, D, ldh, gconst


_N_CU = {}              # device -> compute units (the stream kernel launches one block per CU)
TEAM_MIN_TILES = 4      # a team run must give every block of the launch this many tiles (a re-arm costs about one tile's time)


def single_table_runs(tile_need):
    """The longest run of consecutive tiles that need ONLY h_s2t (`tile_need` == 1) and the longest that need ONLY h_t2s (== 2):
    -> [(first tile, one past the last, table), ...], at most two, by first tile.  Decided once per need mask (one host copy, like
    DstCSR.tile_need itself) and kept on the tensor."""
    key = (tile_need.data_ptr(), tile_need._version)
    c = getattr(tile_need, "_single_table_runs", None)
    if c is None or c[0] != key:
        v = tile_need.detach().cpu()
        runs = []
        if v.numel():
            cut = torch.nonzero(v[1:] != v[:-1]).reshape(-1) + 1
            begin = torch.cat((cut.new_zeros(1), cut))
            end = torch.cat((cut, cut.new_full((1,), v.numel())))
            val = v[begin]
            for table in (0, 1):
                sel = torch.nonzero(val == (1 << table)).reshape(-1)
                if sel.numel():
                    k = sel[torch.argmax((end - begin)[sel])]
                    runs.append((int(begin[k]), int(end[k]), table))
        tile_need._single_table_runs = c = (key, sorted(runs))
    return list(c[1])


def transform_team_runs(N, device, tile_need=None, tail_single=(0, 0)):
    """The plan of the hidden transform's team mode (bgnn.h: bgnn_adaptedconv_transform_f32, team_runs_host_opt): the runs of
    single-table tiles -- out of the need mask, or the two tail groups -- that give every block of the stream kernel's launch (one per CU) at least
    TEAM_MIN_TILES tiles.  [] = team mode stays off for this graph."""
    if tile_need is None and not (tail_single[0] or tail_single[1]):
        return []
    if tile_need is not None:                  # per need mask the plan is decided once (this runs in front of every launch)
        c = getattr(tile_need, "_team_plan", None)
        if c is not None and c[0] == (int(N), device, tile_need._version):
            return c[1]
    ntiles = (int(N) + 31) // 32
    if ntiles == 0:
        return []
    n_cu = _N_CU.get(device)
    if n_cu is None:
        n_cu = _N_CU[device] = torch.cuda.get_device_properties(device).multi_processor_count
    n_blocks = min(ntiles, n_cu)
    if tile_need is not None:
        cand = single_table_runs(tile_need)
    else:
        n_t2s, n_s2t = int(tail_single[0]), int(tail_single[1])
        t2s_begin, s2t_begin = N - n_t2s - n_s2t, N - n_s2t             # rows: [t2s_begin, s2t_begin) h_t2s only, [s2t_begin, N) h_s2t only
        cand = [((t2s_begin + 31) // 32, s2t_begin // 32, 1), ((s2t_begin + 31) // 32, ntiles, 0)] if (n_t2s or n_s2t) else []
    plan = [(b, e, t) for b, e, t in cand if (e - b) // n_blocks >= TEAM_MIN_TILES]
    if tile_need is not None:
        tile_need._team_plan = ((int(N), device, tile_need._version), plan)
    return plan


def adaptedconv_transform(x, mask_u8, delta, packed, out=None, sums=None, tail_single=(0, 0), tile_need=None):
    """One pass over x -> per head (h_t2s, h_s2t) as [N, ldh] tensors (ldh = pad4(D); columns >= D are
    zero; `tile_need`: see DstCSR.tile_need).  `packed` = pack_transform_heads(...).  `out` = list of (h_t2s, h_s2t) preallocated tables
    (>= N rows, row stride ldh; multi-GPU: halo rows follow the N local rows).  With `delta=None` the domain
    `sums` ([2*Din+2] float64) are consumed directly (same delta, one launch less).  `tail_single=(n_t2s, n_s2t)`
    (sums form only): the last n_t2s + n_s2t rows need only h_t2s / only h_s2t; their other table may stay unwritten."""
    lib = L.lib()
    Wp, bp, gates, D, ldh, gconst = packed
    H = gates.shape[0]
    N, Din = x.shape
    dev = x.device
    if out is None:
        out = [(torch.empty(N, ldh, dtype=torch.float32, device=dev), torch.empty(N, ldh, dtype=torch.float32, device=dev))
               for _ in range(H)]
    row_stride = out[0][0].stride(0)
    for a, b in out:
        assert a.shape[0] >= N and b.shape[0] >= N and a.stride(0) == row_stride and b.stride(0) == row_stride
    small = torch.empty(H * (2 * ldh + 2) + 8, dtype=torch.float32, device=dev)
    o1 = out[1] if H > 1 else (None, None)
    if delta is None:
        if sums is None or sums.dtype != torch.float64 or sums.numel() != 2 * Din + 2:
            raise ValueError("adaptedconv_transform needs delta [Din] or the float64 domain sums [2*Din+2]")
    elif tuple(tail_single) != (0, 0):
        raise ValueError("tail_single needs the sums form of the transform")
    if tile_need is not None:
        # `tile_need` (DstCSR.tile_need): rows of a table that the aggregation never reads may stay unwritten (sums form only)
        if delta is not None or tuple(tail_single) != (0, 0):
            raise ValueError("tile_need needs the sums form of the transform and no tail_single")
        if tile_need.dtype != torch.int32 or tile_need.numel() != (N + 31) // 32:
            raise ValueError("tile_need: one int32 per 32-row tile")
    runs = []
    if delta is None and H == 1 and (tile_need is not None or tail_single[0] or tail_single[1]):
        c = getattr(tile_need, "_team_plan", None)                    # (the plan of this need mask, decided at its first launch)
        runs = c[1] if (c is not None and c[0] == (N, dev, tile_need._version)) else transform_team_runs(N, dev, tile_need, tail_single)
    flat = (ctypes.c_int64 * (3 * len(runs)))(*[v for r in runs for v in r]) if runs else None     # host memory, read during the call
    rc = lib.bgnn_adaptedconv_transform_f32(
        L.ptr(x), N, Din, x.stride(0), L.ptr(mask_u8), L.ptr(delta), None if delta is not None else L.ptr(sums), H, D, L.ptr(Wp), L.ptr(bp),
        L.ptr(gates), L.ptr(gconst), L.ptr_rows(out[0][1]), L.ptr_rows(out[0][0]), L.ptr_rows(o1[1]), L.ptr_rows(o1[0]), ldh, row_stride,
        int(tail_single[0]), int(tail_single[1]), L.ptr(tile_need), flat, len(runs), L.ptr(small), L.stream())
    L.check(rc, "bgnn_adaptedconv_transform_f32")
    return out


# second-part launches (a boundary row's two or three remote-source edges) run without the tile queue: nothing to keep
# L2-resident there, and the claims' latency is most of such a short row's time (0.67 -> 0.64 ms per rank-sized forward)
_P2_STATIC = os.environ.get("BGNN_P2_STATIC", "1") != "0"


_TILE_QUEUE_WORDS = None


def _tile_queue(dev):
    """uint32 scratch for the aggregation kernels' per-XCD dynamic tile counters: `bgnn_aggregate_tile_queue_words()` words, 8 for
    chunk claims or 8 * NQ counters a cache line apart for the fast wide kernel's single-tile claims (the C entry zeroes what the
    launch uses on the stream per launch, with one kernel of its own -- see bgnn_zero_async in csrc/bgnn_common.h).  A fresh
    allocation per call: the scratch has no life outside its launch, so nothing created inside a HIP-graph capture has to stay
    valid between replays."""
    global _TILE_QUEUE_WORDS
    if _TILE_QUEUE_WORDS is None:
        _TILE_QUEUE_WORDS = max(8, int(L.lib().bgnn_aggregate_tile_queue_words()))
    return torch.empty(_TILE_QUEUE_WORDS, dtype=torch.int32, device=dev)


def heads_log_softmax_supported(heads, D):
    """Envelope of the fused log_softmax epilogue (bgnn.h: ep_relu == 2)."""
    return heads in (2, 3) and D <= 4


def _hub_shape_ok(D, ldh, ldo, heads, slope):
    """the shapes whose kernels understand hub segments (bgnn.h: bgnn_adaptedconv_aggregate_hub_f32)"""
    if heads in (2, 3) and D <= 4 and ldh == 4 and ldo == 4:
        return True
    return heads == 1 and D > 32 and 0.0 <= slope <= 1.0


def adaptedconv_aggregate(h_t2s, h_s2t, a_t2s, a_s2t, csr, mask_u8, D, negative_slope=0.1, n_dst=None,
                          want_alpha=False, ep_scale=None, ep_shift=None, ep_relu=False, out=None,
                          row_begin=0, row_end=None, state_ms=None, part=0, heads=1, colsum=None, log_softmax=False,
                          park_begin=None):
    """-> out [n_dst, pad4(D)] (use out[:, :D]); optionally alpha [E'] in CSR order.
    part=1: rows [row_begin, park_begin) are finished in this launch, rows [park_begin, row_end) parked for part=2
    (default: all parked).
    `log_softmax` (interleaved narrow heads only, see `heads_log_softmax_supported`): the finished rows leave the kernel
    as log_softmax over each head's D classes (KTGNN.py:435).
    Only rows [row_begin, row_end) are computed (default: all n_dst rows).
    heads > 1: tables are [rows, heads*pad4(D)] (heads interleaved per node), a_* are [heads, D], out is
    [n_dst, heads*pad4(D)]: one pass over the CSR serves all heads."""
    lib = L.lib()
    n_dst = csr.num_nodes if n_dst is None else int(n_dst)
    row_end = n_dst if row_end is None else int(row_end)
    ldh = h_t2s.stride(0) // heads
    ldo = pad4(D)
    dev = h_t2s.device
    if out is None:
        out = torch.empty(n_dst, heads * ldo, dtype=torch.float32, device=dev)
    assert h_t2s.stride(0) == h_s2t.stride(0) and h_t2s.stride(0) % heads == 0 and out.stride(0) % heads == 0
    alpha = torch.empty(csr.num_edges, dtype=torch.float32, device=dev) if want_alpha else None
    tq = _tile_queue(dev) if heads == 1 else None            # (alive until the launch below has been issued)
    if row_end <= int(row_begin):                    # empty row range (e.g. no boundary rows at world size 1)
        return (out, alpha) if want_alpha else out
    # graphs with hub rows: segments + merge (bgnn.h).  Whole-graph, single-launch calls of the two hub-aware kernels only.
    if ((not want_alpha or heads == 1) and part in (0, 3) and int(row_begin) == 0 and row_end == csr.num_nodes == n_dst and h_t2s.shape[0] == n_dst
            and (ep_scale is None or heads == 1) and _hub_shape_ok(D, ldh, out.stride(0) // heads, heads, negative_slope)
            and os.environ.get("BGNN_HUB_ROWS", "1") != "0"):
        hubs = csr.hub_tables()
        if hubs is not None:
            hub_rows, seg_ptr, seg_bounds, seg_node = hubs
            nseg = int(seg_node.numel())
            wsb = lib.bgnn_aggregate_hub_workspace_bytes(nseg, heads, out.stride(0) // heads)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            rc = lib.bgnn_adaptedconv_aggregate_hub_f32(
                L.ptr_rows(h_t2s), L.ptr_rows(h_s2t), ldh, L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col),
                L.ptr(mask_u8), n_dst, D, float(negative_slope), L.ptr_rows(out), out.stride(0) // heads,
                L.ptr(ep_scale), L.ptr(ep_shift), 2 if log_softmax else (1 if ep_relu else 0),
                L.ptr(state_ms) if part == 3 else None, int(heads), L.ptr(colsum),
                L.ptr(tq), HUB_THRESHOLD, L.ptr(hub_rows), int(hub_rows.numel()),
                L.ptr(seg_ptr), L.ptr(seg_bounds), L.ptr(seg_node), nseg, L.ptr(alpha), L.ptr(ws), wsb, L.stream())
            L.check(rc, "bgnn_adaptedconv_aggregate_hub_f32")
            return (out, alpha) if want_alpha else out
    # the tables' row count bounds every id in csr.col (a CSR over these tables): lets the plain wide launch use 32-bit addressing
    queue = tq if not (part == 2 and _P2_STATIC) else None
    rc = lib.bgnn_adaptedconv_aggregate_queued_f32(
        L.ptr_rows(h_t2s), L.ptr_rows(h_s2t), ldh, L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col),
        L.ptr(mask_u8), int(row_begin), row_end, D, float(negative_slope), L.ptr_rows(out), out.stride(0) // heads, L.ptr(alpha),
        L.ptr(ep_scale), L.ptr(ep_shift), 2 if log_softmax else (1 if ep_relu else 0), L.ptr(state_ms), int(part),
        int(row_begin) if park_begin is None else int(park_begin), int(heads), L.ptr(colsum),
        L.ptr(queue), 0 if queue is None else int(queue.numel()), min(int(h_t2s.shape[0]), int(h_s2t.shape[0])),
        csr.gather_hint() if (heads == 1 and D > 32 and part == 0) else 0, L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_queued_f32")
    return (out, alpha) if want_alpha else out


def heads_rows32_plan(t2s, s2t, csr, D, negative_slope, row_end=None):
    """would `adaptedconv_aggregate_heads_rows32` walk these two [rows, 8] tables (bgnn.h: ..._heads_rows32_plan)?  Asked BEFORE
    the tables are filled: no other kernel reads 32-byte rows.  A graph with hub rows is walked in segments, on padded rows."""
    if not (t2s.is_cuda and t2s.dtype == s2t.dtype == torch.float32 and t2s.dim() == s2t.dim() == 2 and t2s.shape[1] == s2t.shape[1] == 8
            and t2s.stride() == s2t.stride() == (8, 1)):
        return False
    if os.environ.get("BGNN_HUB_ROWS", "1") != "0" and csr.hub_tables() is not None:
        return False
    rows = min(int(t2s.shape[0]), int(s2t.shape[0]))
    row_end = csr.num_nodes if row_end is None else int(row_end)
    return bool(L.lib().bgnn_adaptedconv_aggregate_heads_rows32_plan(L.ptr(t2s), L.ptr(s2t), rows, row_end, int(D), float(negative_slope)))


def adaptedconv_aggregate_heads_rows32(t2s, s2t, a_t2s, a_s2t, csr, mask_u8, D, negative_slope=0.1, log_softmax=False,
                                       row_begin=0, row_end=None, out=None):
    """`adaptedconv_aggregate(..., heads=3)` for D <= 2 over tables of 32-byte rows [h0c0 h0c1 h1c0 h1c1 | h2c0 h2c1 0 0]
    -> out [n_dst, 3 * 4], the same bits as the walk over padded rows.  Raises outside `heads_rows32_plan`."""
    row_end = csr.num_nodes if row_end is None else int(row_end)
    if out is None:
        out = torch.empty(csr.num_nodes, 12, dtype=torch.float32, device=t2s.device)
    assert t2s.stride() == s2t.stride() == (8, 1) and out.stride() == (12, 1) and out.shape[0] >= row_end
    rc = L.lib().bgnn_adaptedconv_aggregate_heads_rows32_f32(
        L.ptr(t2s), L.ptr(s2t), L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col), L.ptr(mask_u8), int(row_begin), row_end,
        int(D), float(negative_slope), L.ptr(out), 2 if log_softmax else 0, min(int(t2s.shape[0]), int(s2t.shape[0])), L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_heads_rows32_f32")
    return out


def _bwd_hub_args(csr, use=True):
    """-> (args, nd, ns): the hub-table argument group of the two pull-form backward entries (bgnn.h) for `csr` -- threshold, then
    per side (d_*: destinations, s_*: sources) rows, count, seg_ptr, seg_bounds, seg_node, segment count -- and the two segment
    counts for the workspace query.  A side without hub rows, `use=False` or BGNN_HUB_ROWS=0: its zero-hubs group."""
    use = use and os.environ.get("BGNN_HUB_ROWS", "1") != "0"
    args, nseg = [HUB_THRESHOLD], []
    for tables in ((csr.hub_tables(), csr.transposed_hub_tables()) if use else (None, None)):
        rows, seg_ptr, bounds, node = tables if tables is not None else (None, None, None, None)
        nseg.append(0 if tables is None else int(node.numel()))
        args += [L.ptr(rows), 0 if tables is None else int(rows.numel()), L.ptr(seg_ptr), L.ptr(bounds), L.ptr(node), nseg[-1]]
    return args, nseg[0], nseg[1]


def adaptedconv_aggregate_bwd(h_t2s, h_s2t, a_t2s, a_s2t, csr, mask_u8, D, out, alpha, grad_out, negative_slope=0.1):
    """-> (dh_t2s, dh_s2t, da_t2s, da_s2t): gradients of the fused aggregation w.r.t. both tables and
    both attention vectors (reference: autograd through models/KTGNN.py:292-305)."""
    lib = L.lib()
    dev = h_t2s.device
    da_t2s = torch.zeros(D, dtype=torch.float32, device=dev)
    da_s2t = torch.zeros(D, dtype=torch.float32, device=dev)
    grad_out = grad_out.contiguous()
    ldh, ldo, ldg = h_t2s.stride(0), out.stride(0), grad_out.stride(0)
    # atomic-free pull over the by-source CSR (float atomics retire at ~1.3 TB/s on MI355X; for D > 128 da is summed in a fixed
    # order too, so all four gradients are bitwise reproducible): whole-graph calls with an aligned grad_out.  Row ranges keep the
    # atomic form below, and so do misaligned tables / out at D > 128 (at D <= 128 the entry refuses them).
    pull = D <= 256 and ldg % 4 == 0 and grad_out.data_ptr() % 16 == 0 and h_t2s.shape[0] == csr.num_nodes
    if pull and D > 128:
        pull = (ldh % 4 == 0 and ldo % 4 == 0 and h_t2s.data_ptr() % 16 == 0 and h_s2t.data_ptr() % 16 == 0
                and out.data_ptr() % 16 == 0)
    if pull:
        t_rowptr, t_eid, t_dst = csr.transposed()
        dh_t2s, dh_s2t = torch.empty_like(h_t2s), torch.empty_like(h_s2t)
        narrow = D <= 4 and ldh == 4 and ldo == 4 and ldg == 4              # (the narrow kernels know no hub segments)
        hub_args, nd, ns = _bwd_hub_args(csr, use=not narrow)
        wsb = lib.bgnn_aggregate_bwd_pull_workspace_bytes(csr.num_nodes, csr.num_edges, ldh, D, nd, ns)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = lib.bgnn_adaptedconv_aggregate_bwd_pull_f32(
            L.ptr(h_t2s), L.ptr(h_s2t), ldh, L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col),
            L.ptr(mask_u8), L.ptr(t_rowptr), L.ptr(t_eid), L.ptr(t_dst), csr.num_nodes, csr.num_edges, D, float(negative_slope),
            L.ptr(out), ldo, L.ptr(alpha), L.ptr(grad_out), ldg,
            L.ptr(dh_t2s), L.ptr(dh_s2t), L.ptr(da_t2s), L.ptr(da_s2t), *hub_args, L.ptr(ws), wsb, L.stream())
        L.check(rc, "bgnn_adaptedconv_aggregate_bwd_pull_f32")
        return dh_t2s, dh_s2t, da_t2s, da_s2t
    dh_t2s, dh_s2t = torch.zeros_like(h_t2s), torch.zeros_like(h_s2t)
    rc = lib.bgnn_adaptedconv_aggregate_bwd_f32(
        L.ptr(h_t2s), L.ptr(h_s2t), ldh, L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col),
        L.ptr(mask_u8), 0, csr.num_nodes, D, float(negative_slope), L.ptr(out), ldo, L.ptr(alpha),
        L.ptr(grad_out), ldg, L.ptr(dh_t2s), L.ptr(dh_s2t), L.ptr(da_t2s), L.ptr(da_s2t), L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_bwd_f32")
    return dh_t2s, dh_s2t, da_t2s, da_s2t


def adaptedconv_aggregate_heads_bwd(t2s, s2t, a_t2s, a_s2t, csr, mask_u8, D, heads, out, state_ms, grad_out, log_softmax,
                                    negative_slope=0.1):
    """backward of `adaptedconv_aggregate(..., heads=2|3, part=3)` for interleaved narrow heads ([N, heads*4] tables):
    -> (dh_t2s, dh_s2t [N, heads*4], da_t2s, da_s2t [heads, D]); one CSR walk per pass for all heads."""
    lib = L.lib()
    dev = t2s.device
    N = csr.num_nodes
    assert t2s.shape == (N, heads * 4) and t2s.is_contiguous() and s2t.is_contiguous() and out.is_contiguous() and grad_out.is_contiguous()
    da_t2s = torch.zeros(heads, D, dtype=torch.float32, device=dev)
    da_s2t = torch.zeros(heads, D, dtype=torch.float32, device=dev)
    dh_t2s, dh_s2t = torch.empty_like(t2s), torch.empty_like(s2t)
    t_rowptr, _, t_dst = csr.transposed()
    hub_args, nd, ns = _bwd_hub_args(csr)               # graphs with hub rows: segments + merges (bgnn.h)
    wsb = lib.bgnn_aggregate_heads_bwd_workspace_bytes(N, csr.num_edges, heads, nd, ns)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.bgnn_adaptedconv_aggregate_heads_bwd_f32(
        L.ptr(t2s), L.ptr(s2t), L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col), L.ptr(mask_u8),
        L.ptr(t_rowptr), L.ptr(t_dst), N, csr.num_edges, D, heads, float(negative_slope),
        L.ptr(out), L.ptr(state_ms), L.ptr(grad_out), int(bool(log_softmax)), L.ptr(dh_t2s), L.ptr(dh_s2t),
        L.ptr(da_t2s), L.ptr(da_s2t), *hub_args, L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_heads_bwd_f32")
    return dh_t2s, dh_s2t, da_t2s, da_s2t


def wide_heads_supported(heads, D):
    """Envelope of the wide three-head classifier walk (bgnn.h: bgnn_adaptedconv_aggregate_heads_wide_f32): 4 < D <= 32."""
    return heads in (2, 3) and 4 < int(D) <= 32


def adaptedconv_aggregate_heads_wide(t2s, s2t, a_t2s, a_s2t, csr, mask_u8, D, heads, negative_slope=0.1):
    """`heads` interleaved wide convs ([N, heads*pad4(D)] tables, a_* [heads, D]) in one CSR walk, log_softmax per head:
    -> (log-probs [N, heads*pad4(D)] (pad columns 0), state_ms [N, heads, 2] for the backward)."""
    lib = L.lib()
    N, ld = csr.num_nodes, pad4(D)
    assert t2s.shape == (N, heads * ld) and s2t.shape == t2s.shape and t2s.is_contiguous() and s2t.is_contiguous()
    out = torch.empty(N, heads * ld, dtype=torch.float32, device=t2s.device)
    ms = torch.empty(N, heads, 2, dtype=torch.float32, device=t2s.device)
    rc = lib.bgnn_adaptedconv_aggregate_heads_wide_f32(
        L.ptr(t2s), L.ptr(s2t), ld, L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col), L.ptr(mask_u8),
        N, int(D), int(heads), float(negative_slope), L.ptr(out), L.ptr(ms), L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_heads_wide_f32")
    return out, ms


def adaptedconv_aggregate_heads_wide_bwd(t2s, s2t, a_t2s, a_s2t, csr, mask_u8, D, heads, out, state_ms, grad_out,
                                         negative_slope=0.1):
    """backward of `adaptedconv_aggregate_heads_wide` (grad_out = dL/dlog-probs, [N, heads*pad4(D)]):
    -> (dh_t2s, dh_s2t [N, heads*pad4(D)], da_t2s, da_s2t [heads, D]); deterministic (no float atomics)."""
    lib = L.lib()
    dev = t2s.device
    N, ld = csr.num_nodes, pad4(D)
    assert t2s.shape == (N, heads * ld) and t2s.is_contiguous() and s2t.is_contiguous() and out.is_contiguous() and grad_out.is_contiguous()
    da_t2s = torch.empty(heads, D, dtype=torch.float32, device=dev)
    da_s2t = torch.empty(heads, D, dtype=torch.float32, device=dev)
    dh_t2s, dh_s2t = torch.empty_like(t2s), torch.empty_like(s2t)
    t_rowptr, _, t_dst = csr.transposed()
    wsb = lib.bgnn_aggregate_heads_wide_bwd_workspace_bytes(N, heads, ld)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.bgnn_adaptedconv_aggregate_heads_wide_bwd_f32(
        L.ptr(t2s), L.ptr(s2t), ld, L.ptr(a_t2s), L.ptr(a_s2t), L.ptr(csr.rowptr), L.ptr(csr.col), L.ptr(mask_u8),
        L.ptr(t_rowptr), L.ptr(t_dst), N, int(D), int(heads), float(negative_slope), L.ptr(out), L.ptr(state_ms), L.ptr(grad_out),
        L.ptr(dh_t2s), L.ptr(dh_s2t), L.ptr(da_t2s), L.ptr(da_s2t), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_adaptedconv_aggregate_heads_wide_bwd_f32")
    return dh_t2s, dh_s2t, da_t2s, da_s2t


def l2_normalize_rows(q, eps=1e-8):
    out = torch.empty_like(q)
    rc = L.lib().bgnn_l2_normalize_rows_f32(L.ptr(q), q.shape[0], q.shape[1], float(eps), L.ptr(out), L.stream())
    L.check(rc, "bgnn_l2_normalize_rows_f32")
    return out


_COS_D = (32, 64, 128, 256)


def _pad_cols(t, d):
    if t.shape[1] == d:
        return t.contiguous()
    out = torch.zeros(t.shape[0], d, dtype=t.dtype, device=t.device)
    out[:, : t.shape[1]] = t
    return out


def cosine_topk(qn_query, qn_cand, k, apply_sigmoid=True):
    """Top-k cosine neighbours of every query among the candidates (both already L2-normalised).
    -> (idx int64 [Nq,k], val fp32 [Nq,k], n_fallback int32[2] = (rows re-done exhaustively, rows sent to the precise pass))."""
    lib = L.lib()
    d = qn_query.shape[1]
    dk = next((c for c in _COS_D if c >= d), None)
    if dk is None:
        raise ValueError("embedding width > 256 unsupported")
    qq, qc = _pad_cols(qn_query, dk), _pad_cols(qn_cand, dk)   # zero columns do not change a dot product
    Nq, Nc = qq.shape[0], qc.shape[0]
    dev = qq.device
    idx = torch.empty(Nq, k, dtype=torch.int64, device=dev)
    val = torch.empty(Nq, k, dtype=torch.float32, device=dev)
    nfb = torch.zeros(2, dtype=torch.int32, device=dev)
    wsb = lib.bgnn_topk_workspace_bytes(Nq, Nc, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.bgnn_cosine_topk_f32(L.ptr(qq), L.ptr(qc), Nq, Nc, dk, k, 1 if apply_sigmoid else 0, L.ptr(idx),
                                  L.ptr(val), L.ptr(nfb), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_cosine_topk_f32")
    return idx, val, nfb


def mlp_pair_topk(A_cand, B_query, bn_scale, bn_shift, w2, b2, k, apply_sigmoid=True):
    lib = L.lib()
    Nq, Nc, H = B_query.shape[0], A_cand.shape[0], A_cand.shape[1]
    dev = A_cand.device
    idx = torch.empty(Nq, k, dtype=torch.int64, device=dev)
    val = torch.empty(Nq, k, dtype=torch.float32, device=dev)
    nfb = torch.zeros(2, dtype=torch.int32, device=dev)
    wsb = lib.bgnn_topk_workspace_bytes(Nq, Nc, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.bgnn_mlp_pair_topk_f32(L.ptr(A_cand), L.ptr(B_query), L.ptr(bn_scale), L.ptr(bn_shift), L.ptr(w2),
                                    float(b2), Nq, Nc, H, k, 1 if apply_sigmoid else 0, L.ptr(idx), L.ptr(val),
                                    L.ptr(nfb), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_mlp_pair_topk_f32")
    return idx, val, nfb


def topk_edges(idx, cand_base=0, query_base=0):
    """[Nq,k] top-k table -> edge_index [2, Nq*k] with (from = candidate, to = query)."""
    Nq, k = idx.shape
    out = torch.empty(2, Nq * k, dtype=torch.int64, device=idx.device)
    rc = L.lib().bgnn_topk_edges_i64(L.ptr(idx), Nq, k, int(cand_base), int(query_base), L.ptr(out), L.stream())
    L.check(rc, "bgnn_topk_edges_i64")
    return out


def topk_edges_coalesced(idx, n_cand, cand_base=0, query_base=0):
    """coalesce(topk_edges(idx)) in one call for a table of DISTINCT valid candidates per query (0 <= idx < n_cand,
    k <= n_cand: what the top-k kernels return): a stable 32-bit pair sort by candidate id, no device-to-host read."""
    Nq, k = idx.shape
    lib = L.lib()
    out = torch.empty(2, Nq * k, dtype=torch.int64, device=idx.device)
    wsb = lib.bgnn_topk_edges_coalesced_workspace_bytes(Nq, k)
    ws = torch.empty(wsb, dtype=torch.uint8, device=idx.device)
    rc = lib.bgnn_topk_edges_coalesced_i64(L.ptr(idx), Nq, k, int(n_cand), int(cand_base), int(query_base), L.ptr(out), L.ptr(ws), wsb,
                                           L.stream())
    L.check(rc, "bgnn_topk_edges_coalesced_i64")
    return out


def gather_rows(src, idx, out=None):
    """out[r] = src[idx[r]] for a 2-D float32 table with unit column stride and a row length that is a multiple of 4
    (the halo send lists; `index_select` needs 44 us for 2e5 rows of 48 bytes, this kernel the time of the bytes)."""
    n, w = int(idx.shape[0]), int(src.shape[1])
    if out is None:
        out = torch.empty(n, w, dtype=torch.float32, device=src.device)
    assert src.dtype == torch.float32 and idx.dtype == torch.int64 and w % 4 == 0 and out.shape == (n, w)
    rc = L.lib().bgnn_gather_rows_f32(L.ptr_rows(src), src.shape[0], src.stride(0), L.ptr(idx), n, w, L.ptr_rows(out),
                                      out.stride(0), L.stream())
    L.check(rc, "bgnn_gather_rows_f32")
    return out


def coalesce(edge_index, num_nodes=None):
    """torch_geometric.utils.coalesce on the GPU (sorted by row*n+col, duplicates dropped)."""
    lib = L.lib()
    ei = edge_index.contiguous().clone()
    E = int(ei.shape[1])
    if E == 0:
        return ei
    n = int(num_nodes) if num_nodes is not None else int(ei.max().item()) + 1
    dev = ei.device
    e_out = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = lib.bgnn_coalesce_workspace_bytes(E)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.bgnn_coalesce_i64(L.ptr(ei), E, n, L.ptr(e_out), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_coalesce_i64")
    ne = int(e_out.item())
    return ei[:, :ne].contiguous()


SAGE_EPILOGUES = {None: 0, "none": 0, "relu": 1, "log_softmax": 2}


def _seed_args(seed, seed_dev):
    return int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(seed_dev)


def sage_mean_aggregate(tbl, rowptr, col, n_rows, D, root=None, mean=True, epilogue=None, p_drop=0.0, seed=0, seed_dev=None,
                        out=None, row_ids=None):
    """GraphSAGE aggregation (models/backbones.py:440-498, bgnn.h: bgnn_sage_mean_aggregate_f32) ->
    out [n_rows, pad4(D)] (use out[:, :D]): out[i] = epi(s_i * sum_{t in row i} tbl[col[t]] + root[i]), s_i = 1/deg_i when `mean`.
    tbl / root / out: 2-D row-strided views (unit column stride, e.g. the two halves of one interleaved table).  (rowptr, col) is
    a DstCSR (in-neighbours) or its `transposed()` (t_rowptr, t_dst: out-neighbours).  epilogue: None, "relu" (then dropout at
    p_drop with the (seed, element index) hash of `bn_relu_dropout`) or "log_softmax" (D <= 128).
    row_ids: int64 [n_rows], the GLOBAL row id of every output row (a rank's rows of a partition): the dropout element index is
    then row_ids[i] * D + column, the masks of the whole-graph call; None = row i itself."""
    n_rows, D = int(n_rows), int(D)
    if out is None:
        out = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=tbl.device)
    ldr = 0 if root is None else (root.stride(0) if root.shape[0] > 1 else 0)
    if row_ids is not None:
        assert row_ids.dtype == torch.int64 and row_ids.dim() == 1 and row_ids.shape[0] == n_rows and row_ids.is_contiguous()
    rc = L.lib().bgnn_sage_mean_aggregate_f32(
        L.ptr_rows(tbl), tbl.stride(0), int(tbl.shape[0]), L.ptr_rows(root), ldr, L.ptr(rowptr), L.ptr(col), n_rows, D,
        1 if mean else 0, SAGE_EPILOGUES[epilogue], float(p_drop), *_seed_args(seed, seed_dev), L.ptr(row_ids), L.ptr_rows(out),
        out.stride(0), L.stream())
    L.check(rc, "bgnn_sage_mean_aggregate_f32")
    return out


def sage_mean_aggregate_bwd(y, grad_y, rowptr, t_rowptr, t_col, n_src, D, epilogue=None, p_drop=0.0, grad_tbl=None, grad_root=None):
    """Backward of `sage_mean_aggregate(tbl, rowptr, col, n_rows, D, root, mean=True, epilogue, p_drop)` -> (grad_tbl [n_src, pad4(D)],
    grad_root [n_rows, pad4(D)]).  y: the forward's output (unused without an epilogue, may be None); (t_rowptr, t_col): the view of
    the same edges with the roles swapped (grad_tbl[j] sums grad_root[i] / deg_i over the edges j -> i).  Two launches, no atomics."""
    n_rows, n_src, D = int(rowptr.shape[0]) - 1, int(n_src), int(D)
    dev = grad_y.device
    lib = L.lib()
    if grad_tbl is None:
        grad_tbl = torch.empty(n_src, pad4(D), dtype=torch.float32, device=dev)
    if grad_root is None:
        grad_root = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=dev)
    wsb = lib.bgnn_sage_mean_aggregate_bwd_workspace_bytes(n_rows, D)
    ws = torch.empty(max(int(wsb), 16), dtype=torch.uint8, device=dev)
    rc = lib.bgnn_sage_mean_aggregate_bwd_f32(
        L.ptr_rows(y), y.stride(0) if y is not None else 0, L.ptr_rows(grad_y), grad_y.stride(0), L.ptr(rowptr), n_rows,
        L.ptr(t_rowptr), L.ptr(t_col), n_src, D, SAGE_EPILOGUES[epilogue], float(p_drop), L.ptr_rows(grad_tbl), grad_tbl.stride(0),
        L.ptr_rows(grad_root), grad_root.stride(0), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_sage_mean_aggregate_bwd_f32")
    return grad_tbl, grad_root


# rows with at least GCN_HUB_THRESHOLD edges are cut into segments of GCN_HUB_SEGMENT edges (bgnn_gcn_aggregate_f32): a row below
# the threshold is at most 32 rounds of 8 gathers for its lane group
GCN_HUB_THRESHOLD = 256
GCN_HUB_SEGMENT = 128


def _gcn_hub_args(hubs, D, dev):
    """hubs: None or (threshold, hub_rows, hub_seg_ptr, seg_bounds) -> the hub arguments of the GCN entry points + the workspace"""
    if hubs is None:
        return (0, None, 0, None, None, 0, None, 0), None
    thr, rows, seg_ptr, bounds = hubs
    n_seg = int(bounds.shape[0]) // 2
    wsb = int(L.lib().bgnn_gcn_aggregate_workspace_bytes(n_seg, int(D)))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    return (int(thr), L.ptr(rows), int(rows.shape[0]), L.ptr(seg_ptr), L.ptr(bounds), n_seg, L.ptr(ws), ws.numel()), ws


def gcn_aggregate(tbl, rowptr, col, dinv, n_rows, D, bias=None, epilogue=None, p_drop=0.0, seed=0, seed_dev=None, out=None,
                  hubs=None, row_ids=None):
    """GCN normalised aggregation (models/backbones.py:246-300, bgnn.h: bgnn_gcn_aggregate_f32) -> out [n_rows, pad4(D)] (use
    out[:, :D]): out[i] = epi(dinv[i] * sum_{t in row i} dinv[col[t]] * tbl[col[t]] + bias) over a CSR that holds one self loop per
    row (`build_dst_csr(rewrite_self_loops=True)`) or its `transposed()` view; dinv float32 [>= max(n_rows, tbl rows)].
    tbl / out: 2-D row-strided views with unit column stride; bias: float32 [>= D], 16-byte aligned, or None.  epilogue: None,
    "relu" (then dropout at p_drop, the (seed, element index) hash of `sage_mean_aggregate`) or "log_softmax" (D <= 128).
    hubs: None (every row is walked by one lane group) or (threshold, hub_rows, hub_seg_ptr, seg_bounds) from
    `DstCSR.hub_tables(threshold, segment)` of the SAME view: those rows are summed segment by segment across the grid.
    row_ids: int64 [n_rows], the GLOBAL row id of every output row (a rank's rows of a partition): the dropout element index is
    then row_ids[i] * D + column, the masks of the whole-graph call; None = row i itself."""
    n_rows, D = int(n_rows), int(D)
    if out is None:
        out = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=tbl.device)
    if bias is not None and (bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] < D):
        raise ValueError("bias must be float32 [>= D]")
    if dinv.dtype != torch.float32 or dinv.dim() != 1:
        raise ValueError("dinv must be float32 [N]")
    hub_args, ws = _gcn_hub_args(hubs, D, tbl.device)
    if row_ids is not None:
        assert row_ids.dtype == torch.int64 and row_ids.dim() == 1 and row_ids.shape[0] == n_rows and row_ids.is_contiguous()
    rc = L.lib().bgnn_gcn_aggregate_f32(
        L.ptr_rows(tbl), tbl.stride(0), int(tbl.shape[0]), L.ptr(bias), L.ptr(rowptr), L.ptr(col), L.ptr(dinv), int(dinv.shape[0]),
        n_rows, D, SAGE_EPILOGUES[epilogue], float(p_drop), *_seed_args(seed, seed_dev), *hub_args, L.ptr(row_ids), L.ptr_rows(out),
        out.stride(0), L.stream())
    L.check(rc, "bgnn_gcn_aggregate_f32")
    return out


def gcn_aggregate_bwd(y, grad_y, t_rowptr, t_col, dinv, n_src, D, epilogue=None, p_drop=0.0, want_bias=True, grad_tbl=None,
                      hubs=None):
    """Backward of `gcn_aggregate(tbl, rowptr, col, dinv, n_rows, D, bias, epilogue, p_drop)` -> (grad_tbl [n_src, pad4(D)],
    grad_bias [D] | None).  y: the forward's output (unused without an epilogue, may be None); (t_rowptr, t_col): the view of the
    same edges with the roles swapped, `hubs` that view's hub tables.  g (the gradient at the epilogue's input) comes from one row
    pass, grad_bias = its fixed-order column sums (`column_sums`), grad_tbl[j] = dinv[j] * sum_{i : j -> i} dinv[i] * g[i] from the
    forward walk over the swapped view.  No atomics: bit-identical from run to run."""
    n_rows, n_src, D = int(grad_y.shape[0]), int(n_src), int(D)
    dev = grad_y.device
    if grad_tbl is None:
        grad_tbl = torch.empty(n_src, pad4(D), dtype=torch.float32, device=dev)
    g = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=dev)
    hub_args, ws = _gcn_hub_args(hubs, D, dev)
    rc = L.lib().bgnn_gcn_aggregate_bwd_f32(
        L.ptr_rows(y), y.stride(0) if y is not None else 0, L.ptr_rows(grad_y), grad_y.stride(0), n_rows, L.ptr(t_rowptr),
        L.ptr(t_col), L.ptr(dinv), int(dinv.shape[0]), n_src, D, SAGE_EPILOGUES[epilogue], float(p_drop), *hub_args,
        L.ptr_rows(g), g.stride(0), L.ptr_rows(grad_tbl), grad_tbl.stride(0), L.stream())
    L.check(rc, "bgnn_gcn_aggregate_bwd_f32")
    return grad_tbl, (column_sums(g)[:D] if want_bias else None)


APPNP_EPILOGUES = {None: 0, "none": 0, "log_softmax": 2}


def _need_rows_f32(t, what, D):
    L._check_device(t)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < D:
        raise ValueError(f"{what} must be float32 [rows, >= D]")
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < pad4(D) or t.data_ptr() % 16 != 0:
        raise ValueError(f"{what}: rows must have unit column stride, a stride that is a multiple of 4 floats and >= pad4(D), and a "
                         "16-byte aligned base")


def appnp_propagate(h, rowptr, col, dinv, n_rows, D, K, alpha, epilogue=None, hubs=None, out=None):
    """APPNP propagation (models/backbones.py:110-128, bgnn.h: bgnn_appnp_propagate_f32) -> out [n_rows, pad4(D)] (use out[:, :D]):
    z_0 = h, z_{k+1} = (1 - alpha) * A^ z_k + alpha * h for k < K, out = epi(z_K), A^ = D^-1/2 (A' + I) D^-1/2 over the CSR of
    `gcn_aggregate` (one self loop per row; `GcnGraph`: csr.rowptr, col, dinv, hubs) or, for the gradient with respect to h, its
    by-source view (t_rowptr, t_dst, t_hubs) applied to the output gradient.  h / out: 2-D row-strided views with unit column
    stride, n_rows rows, distinct.  1 <= D <= 128, K >= 0 (0: epi(h)), 0 <= alpha <= 1 (1: h bit for bit); epilogue None or
    "log_softmax".  One launch per step (three with `hubs`), no atomics, no host synchronisation."""
    n_rows, D, K, alpha = int(n_rows), int(D), int(K), float(alpha)
    if epilogue not in APPNP_EPILOGUES:
        raise ValueError(f"epilogue must be None or 'log_softmax', got {epilogue!r}")
    if D < 1:
        raise ValueError("D must be at least 1")
    _need_rows_f32(h, "h", D)
    if h.shape[0] != n_rows:
        raise ValueError(f"h must have n_rows = {n_rows} rows (the graph is square), got {h.shape[0]}")
    if dinv.dtype != torch.float32 or dinv.dim() != 1 or dinv.shape[0] < n_rows:
        raise ValueError("dinv must be float32 [>= n_rows]")
    if rowptr.dtype != torch.int32 or rowptr.dim() != 1 or rowptr.shape[0] < n_rows + 1 or col.dtype != torch.int32 or col.dim() != 1:
        raise ValueError("rowptr must be int32 [n_rows + 1] and col int32 [E]")
    if K < 0:
        raise ValueError("K must be >= 0")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    if out is None:
        out = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=h.device)
    else:
        _need_rows_f32(out, "out", D)
        if out.shape[0] != n_rows:
            raise ValueError(f"out must have n_rows = {n_rows} rows")
    lib = L.lib()
    if hubs is None:
        hub_args, n_seg = (0, None, 0, None, None, 0), 0
    else:
        thr, rows, seg_ptr, bounds = hubs
        n_seg = int(bounds.shape[0]) // 2
        hub_args = (int(thr), L.ptr(rows), int(rows.shape[0]), L.ptr(seg_ptr), L.ptr(bounds), n_seg)
    wsb = int(lib.bgnn_appnp_propagate_workspace_bytes(n_rows, D, n_seg))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=h.device)
    rc = lib.bgnn_appnp_propagate_f32(
        L.ptr_rows(h), h.stride(0), L.ptr(rowptr), L.ptr(col), L.ptr(dinv), int(dinv.shape[0]), n_rows, D, K, alpha,
        APPNP_EPILOGUES[epilogue], *hub_args, L.ptr(ws), ws.numel(), L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_appnp_propagate_f32")
    return out


GCN2_MAX_WIDTH = 128


def gcn2_supported(H):
    """the hidden widths `gcn2_conv` / `gcn2_conv_bwd` take (any H of the range, a multiple of 4 or not)"""
    return 1 <= int(H) <= GCN2_MAX_WIDTH


def _gcn2_need_m(M, H):
    L._check_device(M)
    if M.dtype != torch.float32 or tuple(M.shape) != (pad4(H), pad4(H)) or not M.is_contiguous():
        raise ValueError(f"M must be a contiguous float32 [pad4(H), pad4(H)] = [{pad4(H)}, {pad4(H)}] (zero padding)")


def _rows_extent(t, H):
    """[first byte, one past the last byte) that a row-strided [rows, >= pad4(H)] view spans over pad4(H) columns"""
    lo = t.data_ptr()
    return lo, lo + ((int(t.shape[0]) - 1) * t.stride(0) + pad4(H)) * 4 if t.shape[0] else lo


def gcn2_conv(x, x0, M, rowptr, col, dinv, n_rows, H, alpha, p_drop=0.0, seed=0, seed_dev=None, hubs=None, m_out=None, out=None,
              row_ids=None):
    """One GCNII layer with its ReLU and dropout (models/backbones.py:163-197: GCN2Conv(H, alpha, theta, layer) + relu + the next
    F.dropout; bgnn.h: bgnn_gcn2_conv_f32 / bgnn_gcn2_conv_rows_f32) -> out [n_rows, pad4(H)] (use out[:, :H]):
    m_i = (1 - alpha) * dinv[i] * sum_{t in row i} dinv[col[t]] * x[col[t]] + alpha * x0[i],  out_i = drop(relu(m_i @ M)),
    M = (1 - beta) * I + beta * weight1 as float32 [pad4(H), pad4(H)] with zero padding (applied untransposed), over the CSR of
    `gcn_aggregate` (`GcnGraph`: csr.rowptr, col, dinv, hubs).  x / x0 / out / m_out: 2-D row-strided views with unit column
    stride (x may be a view of a wider table); 1 <= H <= 128, 0 <= alpha <= 1.
    The graph may be RECTANGULAR (a rank's rows of a partition): rowptr [n_rows + 1] and x0 / out / m_out have exactly n_rows rows,
    x has x.shape[0] >= n_rows rows (the owned rows, then the halo slots), ids in col < x.shape[0], and dinv covers the table:
    dinv.shape[0] >= x.shape[0] (the gather reads dinv[col]).
    Dropout at p_drop keeps element i * H + column by the (seed + seed_dev, element index) hash of `gcn_aggregate`; p_drop = 0
    draws no mask.  row_ids: int64 [n_rows], contiguous, the GLOBAL row id of every output row: the element is then
    row_ids[i] * H + column, in the row launch and in a hub row's finish launch -- the masks of the whole-graph call in this
    rank's rows; None = row i itself.
    m_out: None (evaluation: the mix never leaves the chip) or a [n_rows, >= pad4(H)] buffer that receives m (training: the
    backward's operand); out has the same bits either way.  hubs: as in `gcn_aggregate`, the tables of the n_rows rows.
    A square call without row_ids takes bgnn_gcn2_conv_f32 as before; every other call takes bgnn_gcn2_conv_rows_f32, the same
    launch sequence (identity ids on a square graph give the same bits).  Still refused: H > 128, x with fewer than n_rows rows,
    x0 / out / m_out of another row count, dinv shorter than x, and out or m_out overlapping x -- the same tensor always; on the
    rectangular / row-id route any overlap of the byte extents of the views, so the front rows of x's own buffer cannot be the
    output.  No atomics, no host synchronisation."""
    n_rows, H, alpha = int(n_rows), int(H), float(alpha)
    if not gcn2_supported(H):
        raise ValueError(f"gcn2_conv takes 1 <= H <= {GCN2_MAX_WIDTH}, got {H}")
    _need_rows_f32(x, "x", H)
    _need_rows_f32(x0, "x0", H)
    _gcn2_need_m(M, H)
    n_tbl = int(x.shape[0])
    if n_tbl < n_rows or x0.shape[0] != n_rows:
        raise ValueError(f"x must have at least n_rows = {n_rows} rows and x0 exactly n_rows rows, got {n_tbl} and {x0.shape[0]}")
    if dinv.dtype != torch.float32 or dinv.dim() != 1 or dinv.shape[0] < n_tbl:
        raise ValueError("dinv must be float32 [>= rows of x]")
    if rowptr.dtype != torch.int32 or rowptr.dim() != 1 or rowptr.shape[0] < n_rows + 1 or col.dtype != torch.int32 or col.dim() != 1:
        raise ValueError("rowptr must be int32 [n_rows + 1] and col int32 [E]")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    if not 0.0 <= float(p_drop) < 1.0:
        raise ValueError("p_drop must lie in [0, 1)")
    if row_ids is not None:
        L._check_device(row_ids)
        if row_ids.dtype != torch.int64 or row_ids.dim() != 1 or row_ids.shape[0] != n_rows or not row_ids.is_contiguous():
            raise ValueError(f"row_ids must be a contiguous int64 [n_rows] = [{n_rows}]")
    if out is None:
        out = torch.empty(n_rows, pad4(H), dtype=torch.float32, device=x.device)
    else:
        _need_rows_f32(out, "out", H)
    if m_out is not None:
        _need_rows_f32(m_out, "m_out", H)
    if out.shape[0] != n_rows or (m_out is not None and m_out.shape[0] != n_rows):
        raise ValueError(f"out and m_out must have n_rows = {n_rows} rows")
    rows_entry = row_ids is not None or n_tbl != n_rows
    if rows_entry:
        xlo, xhi = _rows_extent(x, H)
        for name, t in (("out", out), ("m_out", m_out)):
            if t is not None and n_rows:
                lo, hi = _rows_extent(t, H)
                if lo < xhi and xlo < hi:
                    raise ValueError(f"{name} overlaps x: the rows of x are gathered while {name} is written")
    lib = L.lib()
    if hubs is None:
        hub_args, ws = (0, None, 0, None, None, 0, None, 0), None
    else:
        thr, rows, seg_ptr, bounds = hubs
        n_seg = int(bounds.shape[0]) // 2
        ws = torch.empty(max(int(lib.bgnn_gcn2_conv_workspace_bytes(n_seg, H)), 16), dtype=torch.uint8, device=x.device)
        hub_args = (int(thr), L.ptr(rows), int(rows.shape[0]), L.ptr(seg_ptr), L.ptr(bounds), n_seg, L.ptr(ws), ws.numel())
    tail = (*_seed_args(seed, seed_dev), *hub_args, L.ptr_rows(m_out), m_out.stride(0) if m_out is not None else 0, L.ptr_rows(out),
            out.stride(0), L.stream())
    if rows_entry:
        rc = lib.bgnn_gcn2_conv_rows_f32(
            L.ptr_rows(x), x.stride(0), n_tbl, L.ptr_rows(x0), x0.stride(0), L.ptr(M), L.ptr(rowptr), L.ptr(col), L.ptr(dinv),
            int(dinv.shape[0]), n_rows, L.ptr(row_ids), H, alpha, float(p_drop), *tail)
        L.check(rc, "bgnn_gcn2_conv_rows_f32")
    else:
        rc = lib.bgnn_gcn2_conv_f32(
            L.ptr_rows(x), x.stride(0), L.ptr_rows(x0), x0.stride(0), L.ptr(M), L.ptr(rowptr), L.ptr(col), L.ptr(dinv),
            int(dinv.shape[0]), n_rows, H, alpha, float(p_drop), *tail)
        L.check(rc, "bgnn_gcn2_conv_f32")
    return out


def gcn2_conv_bwd(y, grad_y, M, H, alpha, p_drop):
    """Dense half of `gcn2_conv`'s backward (models/backbones.py:163-197; bgnn.h: bgnn_gcn2_conv_bwd_f32) -> (gz, t, gx0), each
    [rows, pad4(H)] with zero pad columns: gz = grad_y * [y > 0] / (1 - p_drop) (y: the forward's output; y > 0 <=> kept and
    positive, no mask is redrawn), gm = gz @ M^T, t = (1 - alpha) * gm, gx0 = alpha * gm.  The caller finishes with
    grad_weight1 = beta * m^T gz (`gram`) and grad_x = `gcn_aggregate(t, t_rowptr, t_dst, dinv, ..., hubs=t_hubs)`."""
    H, alpha = int(H), float(alpha)
    if not gcn2_supported(H):
        raise ValueError(f"gcn2_conv_bwd takes 1 <= H <= {GCN2_MAX_WIDTH}, got {H}")
    _need_rows_f32(y, "y", H)
    _need_rows_f32(grad_y, "grad_y", H)
    _gcn2_need_m(M, H)
    if grad_y.shape[0] != y.shape[0]:
        raise ValueError("y and grad_y must have the same number of rows")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    if not 0.0 <= float(p_drop) < 1.0:
        raise ValueError("p_drop must lie in [0, 1)")
    N = int(y.shape[0])
    gz, t, gx0 = (torch.empty(N, pad4(H), dtype=torch.float32, device=y.device) for _ in range(3))
    rc = L.lib().bgnn_gcn2_conv_bwd_f32(L.ptr_rows(y), y.stride(0), L.ptr_rows(grad_y), grad_y.stride(0), L.ptr(M), N, H, alpha,
                                        float(p_drop), L.ptr_rows(gz), gz.stride(0), L.ptr_rows(t), t.stride(0), L.ptr_rows(gx0),
                                        gx0.stride(0), L.stream())
    L.check(rc, "bgnn_gcn2_conv_bwd_f32")
    return gz, t, gx0


def _gen_need_t(t):
    L._check_device(t)
    if t.dtype != torch.float32 or t.numel() != 1 or not t.is_contiguous():
        raise ValueError("t must be a float32 tensor of one element (the temperature stays on the device)")


def _gen_need_csr(rowptr, col, n_rows, what="rowptr"):
    if rowptr.dtype != torch.int32 or rowptr.dim() != 1 or rowptr.shape[0] < n_rows + 1 or col.dtype != torch.int32 or col.dim() != 1:
        raise ValueError(f"{what} must be int32 [rows + 1] and its ids int32 [E]")


def gen_softmax_aggregate(x, rowptr, col, t, n_rows, H, save=None, out=None):
    """DeeperGCN's softmax aggregation with the root add (models/backbones.py:130-161: GENConv(aggr='softmax', learn_t=True) in
    front of its MLP; bgnn.h: bgnn_gen_softmax_aggregate_f32) -> z [n_rows, pad4(H)] (use z[:, :H]):
    v_j = relu(x_j) + 1e-7, alpha_ij = softmax over the in-edges of row i of t * v_j PER CHANNEL, z_i = sum_j alpha_ij v_j + x_i
    (a row without in-edges: x_i bit for bit).  (rowptr, col) is the by-destination CSR exactly as given (`SageGraph`: duplicates
    are separate messages, self loops ordinary edges).  x: a 2-D row-strided view with unit column stride and at least n_rows
    rows (it may be a view of a wider table; ids in col outside it add nothing); t: a float32 tensor of ONE element on the device
    (the learnable temperature, any sign or 0; never read by the host); any H >= 1.
    save: None (evaluation) or a pair (lse, o) of [n_rows, >= pad4(H)] buffers with one row stride that receive
    lse_i = log sum_j exp(t * v_j) and o_i = z_i - x_i per row and channel (training: `gen_softmax_aggregate_bwd`'s operands); z has
    the same bits either way.  Pad columns of z, lse and o are written as 0.  No atomics, no host synchronisation."""
    n_rows, H = int(n_rows), int(H)
    if H < 1:
        raise ValueError(f"gen_softmax_aggregate takes H >= 1, got {H}")
    _need_rows_f32(x, "x", H)
    _gen_need_t(t)
    if x.shape[0] < n_rows:
        raise ValueError(f"x must have at least n_rows = {n_rows} rows, got {x.shape[0]}")
    _gen_need_csr(rowptr, col, n_rows)
    lse = o = None
    if save is not None:
        lse, o = save
        for name, s in (("lse", lse), ("o", o)):
            _need_rows_f32(s, name, H)
            if s.shape[0] != n_rows:
                raise ValueError(f"{name} must have n_rows = {n_rows} rows")
        if lse.stride(0) != o.stride(0) or lse.data_ptr() == o.data_ptr():
            raise ValueError("lse and o must be two distinct buffers with one row stride")
    if out is None:
        out = torch.empty(n_rows, pad4(H), dtype=torch.float32, device=x.device)
    else:
        _need_rows_f32(out, "out", H)
        if out.shape[0] != n_rows or out.data_ptr() == x.data_ptr():
            raise ValueError(f"out must have n_rows = {n_rows} rows and be distinct from x")
    rc = L.lib().bgnn_gen_softmax_aggregate_f32(
        L.ptr_rows(x), x.stride(0), int(x.shape[0]), L.ptr(rowptr), L.ptr(col), int(col.shape[0]), n_rows, H, L.ptr(t),
        L.ptr_rows(lse), L.ptr_rows(o), lse.stride(0) if lse is not None else 0, L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_gen_softmax_aggregate_f32")
    return out


def gen_softmax_aggregate_bwd(x, grad_z, save, t_rowptr, t_dst, t, H, grad_x=None):
    """Backward of `gen_softmax_aggregate(x, rowptr, col, t, n_rows, H, save)` (models/backbones.py:130-161; bgnn.h:
    bgnn_gen_softmax_aggregate_bwd_f32) -> (grad_x [rows of x, pad4(H)] with zero pad columns, grad_t float32 [1]).
    grad_z: the gradient at z, [n_rows, >= pad4(H)]; save = (lse, o): the forward's tables; (t_rowptr, t_dst): the by-source view of
    the same edges (`DstCSR.transposed()`), t_rowptr over the rows of x.  One walk: the group of source row j forms
    a = exp(t * v_j - lse_i) per out-edge and accumulates dv_j = sum a g_i (1 + t (v_j - o_i)) and the centred
    grad_t = sum a g_i (v_j - o_i)^2; grad_x[j] = [x_j > 0] dv_j + g_j is written once.  grad_t is summed from per-block fp64
    partials in a fixed order: no atomics, the same bits on every run, nothing carried over between calls, no host
    synchronisation."""
    H = int(H)
    if H < 1:
        raise ValueError(f"gen_softmax_aggregate_bwd takes H >= 1, got {H}")
    lse, o = save
    _need_rows_f32(x, "x", H)
    _need_rows_f32(grad_z, "grad_z", H)
    _need_rows_f32(lse, "lse", H)
    _need_rows_f32(o, "o", H)
    _gen_need_t(t)
    n_src, n_rows = int(x.shape[0]), int(grad_z.shape[0])
    if lse.shape[0] != n_rows or o.shape[0] != n_rows or lse.stride(0) != o.stride(0):
        raise ValueError("lse and o must have grad_z's rows and one row stride")
    _gen_need_csr(t_rowptr, t_dst, n_src, "t_rowptr")
    if grad_x is None:
        grad_x = torch.empty(n_src, pad4(H), dtype=torch.float32, device=x.device)
    else:
        _need_rows_f32(grad_x, "grad_x", H)
        if grad_x.shape[0] != n_src:
            raise ValueError(f"grad_x must have the {n_src} rows of x")
    lib = L.lib()
    grad_t = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(int(lib.bgnn_gen_softmax_aggregate_workspace_bytes(n_src, H)), 16), dtype=torch.uint8, device=x.device)
    rc = lib.bgnn_gen_softmax_aggregate_bwd_f32(
        L.ptr_rows(x), x.stride(0), n_src, L.ptr_rows(grad_z), grad_z.stride(0), L.ptr_rows(lse), L.ptr_rows(o), lse.stride(0), n_rows,
        L.ptr(t_rowptr), L.ptr(t_dst), int(t_dst.shape[0]), H, L.ptr(t), L.ptr_rows(grad_x), grad_x.stride(0), L.ptr(grad_t),
        L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_gen_softmax_aggregate_bwd_f32")
    return grad_x, grad_t


def _gin_need_eps(eps):
    if eps is None:
        return
    if not isinstance(eps, torch.Tensor):
        raise ValueError("eps must be a float32 tensor of one element on the device, or None (it stays on the device: a Python "
                         f"number is not taken, got {type(eps).__name__})")
    L._check_device(eps)
    if eps.dtype != torch.float32 or eps.numel() != 1 or not eps.is_contiguous():
        raise ValueError("eps must be a float32 tensor of one element (it stays on the device)")


def _gin_need_cfg(what, D, epilogue, p_drop):
    if D < 1:
        raise ValueError(f"{what} takes D >= 1, got {D}")
    if epilogue not in SAGE_EPILOGUES:
        raise ValueError(f"{what}: epilogue must be None, 'relu' or 'log_softmax', got {epilogue!r}")
    if not 0.0 <= float(p_drop) < 1.0 or (p_drop > 0 and epilogue != "relu"):
        raise ValueError(f"{what}: 0 <= p_drop < 1, and dropout only after the 'relu' epilogue")
    if epilogue == "log_softmax" and D > 128:
        raise ValueError(f"{what}: the fused log_softmax serves D <= 128, got {D}")


# rows with at least GIN_HUB_THRESHOLD edges are cut into segments of GIN_HUB_SEGMENT edges (bgnn_gin_aggregate_hub_f32): GCN's
# values -- the lane group and its depth of 8 gathers a round are the same
GIN_HUB_THRESHOLD = 256
GIN_HUB_SEGMENT = 128


def _gin_hub_args(hubs, D, dev, head_bytes=0):
    """hubs: (threshold, hub_rows, hub_seg_ptr, seg_bounds) -> the hub arguments of the GIN hub entries (without the workspace) and
    the workspace: `head_bytes` for the caller, then the partial rows"""
    if len(hubs) != 4:
        raise ValueError("hubs must be (threshold, hub_rows, hub_seg_ptr, seg_bounds)")
    thr, rows, seg_ptr, bounds = hubs
    for t, what in ((rows, "hub_rows"), (seg_ptr, "hub_seg_ptr"), (bounds, "seg_bounds")):
        L._check_device(t)
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"hubs: {what} must be a contiguous int32 vector")
    if int(thr) < 1 or seg_ptr.shape[0] != rows.shape[0] + 1 or bounds.shape[0] % 2:
        raise ValueError("hubs: threshold >= 1, hub_seg_ptr [n_hubs + 1], seg_bounds [2 n_seg]")
    n_seg = int(bounds.shape[0]) // 2
    wsb = int(head_bytes) + int(L.lib().bgnn_gin_aggregate_hub_workspace_bytes(n_seg, int(D)))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    return (int(thr), L.ptr(rows), int(rows.shape[0]), L.ptr(seg_ptr), L.ptr(bounds), n_seg), ws


def gin_aggregate(tbl, rowptr, col, eps, n_rows, D, bias=None, epilogue=None, p_drop=0.0, seed=0, seed_dev=None, out=None,
                  row_ids=None):
    """GIN sum aggregation (models/backbones.py:26-57: PyG GINConv(Linear, train_eps=True) after its transform; bgnn.h:
    bgnn_gin_aggregate_f32) -> out [n_rows, pad4(D)] (use out[:, :D]):
    out[i] = epi((1 + eps) * tbl[i] + sum_{t in row i} tbl[col[t]] + bias) over the by-destination CSR exactly as given (`SageGraph`:
    no self loop added or removed, duplicates are separate messages) or its `transposed()` view.  Row i of tbl is row i's root: no
    root buffer.  tbl: a 2-D row-strided view with unit column stride and at least n_rows rows (it may be a view of a wider
    table; ids in col outside it add nothing); eps: a float32 tensor of ONE element on the device (GINConv's eps, never read by the
    host: changing it in place changes the next call), or None for weight 1 (the bits of a device 0); bias: float32 [>= D] or None.
    epilogue: None, "relu" (then dropout at p_drop, the (seed, element index) hash of `sage_mean_aggregate`) or "log_softmax"
    (D <= 128).  row_ids: int64 [n_rows], the GLOBAL row id of every output row (a rank's rows of a partition): the dropout element
    index is then row_ids[i] * D + column; None = row i itself.  Pad columns of out are written as 0.  No atomics, no host
    synchronisation.  Hub rows walk as one lane group each: `gin_aggregate_hubs` segments them."""
    return _gin_aggregate(tbl, rowptr, col, eps, n_rows, D, bias, epilogue, p_drop, seed, seed_dev, out, row_ids, None)


def gin_aggregate_hubs(tbl, rowptr, col, eps, n_rows, D, bias=None, epilogue=None, p_drop=0.0, seed=0, seed_dev=None, out=None,
                       row_ids=None, hubs=None):
    """`gin_aggregate` (models/backbones.py:26-57; bgnn.h: bgnn_gin_aggregate_hub_f32) with segmented hub rows.  hubs: None -- the
    call of `gin_aggregate`, the same launches and the same bits -- or (threshold, hub_rows, hub_seg_ptr, seg_bounds) from
    `DstCSR.hub_tables(threshold, segment)` of the SAME view (`transposed_hub_tables` for the by-source view): those rows are summed
    segment by segment across the grid, then finished (own row, bias, epilogue, the mask of row_ids[hub row]) by one lane group a hub.
    Every other row carries the bits of `gin_aggregate`, and so does a hub of one segment."""
    return _gin_aggregate(tbl, rowptr, col, eps, n_rows, D, bias, epilogue, p_drop, seed, seed_dev, out, row_ids, hubs)


def _gin_aggregate(tbl, rowptr, col, eps, n_rows, D, bias, epilogue, p_drop, seed, seed_dev, out, row_ids, hubs):
    n_rows, D = int(n_rows), int(D)
    _gin_need_cfg("gin_aggregate", D, epilogue, p_drop)
    _gin_need_eps(eps)
    _need_rows_f32(tbl, "tbl", D)
    if tbl.shape[0] < n_rows:
        raise ValueError(f"tbl must have at least n_rows = {n_rows} rows, got {tbl.shape[0]}")
    _gen_need_csr(rowptr, col, n_rows)
    if bias is not None:
        if bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] < D:
            raise ValueError("bias must be float32 [>= D]")
        if bias.shape[0] < pad4(D) or bias.data_ptr() % 16 != 0:      # the kernel reads whole float4 slots of an aligned row
            bp = torch.zeros(pad4(D), dtype=torch.float32, device=bias.device)
            bp[:D] = bias[:D]
            bias = bp
    if row_ids is not None and (row_ids.dtype != torch.int64 or row_ids.dim() != 1 or row_ids.shape[0] != n_rows
                                or not row_ids.is_contiguous()):
        raise ValueError("row_ids must be a contiguous int64 [n_rows]")
    if out is None:
        out = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=tbl.device)
    else:
        _need_rows_f32(out, "out", D)
        if out.shape[0] != n_rows or out.data_ptr() == tbl.data_ptr():
            raise ValueError(f"out must have n_rows = {n_rows} rows and be distinct from tbl")
    if hubs is not None:
        hub_args, ws = _gin_hub_args(hubs, D, tbl.device)
        rc = L.lib().bgnn_gin_aggregate_hub_f32(
            L.ptr_rows(tbl), tbl.stride(0), int(tbl.shape[0]), L.ptr(eps), L.ptr(bias), L.ptr(rowptr), L.ptr(col), int(col.shape[0]),
            n_rows, D, SAGE_EPILOGUES[epilogue], float(p_drop), *_seed_args(seed, seed_dev), *hub_args, L.ptr(ws), ws.numel(),
            L.ptr(row_ids), L.ptr_rows(out), out.stride(0), L.stream())
        L.check(rc, "bgnn_gin_aggregate_hub_f32")
        return out
    rc = L.lib().bgnn_gin_aggregate_f32(
        L.ptr_rows(tbl), tbl.stride(0), int(tbl.shape[0]), L.ptr(eps), L.ptr(bias), L.ptr(rowptr), L.ptr(col), int(col.shape[0]),
        n_rows, D, SAGE_EPILOGUES[epilogue], float(p_drop), *_seed_args(seed, seed_dev), L.ptr(row_ids), L.ptr_rows(out),
        out.stride(0), L.stream())
    L.check(rc, "bgnn_gin_aggregate_f32")
    return out


def gin_aggregate_bwd(tbl, y, grad_y, t_rowptr, t_col, eps, n_src, D, epilogue=None, p_drop=0.0, want_bias=True, want_eps=True,
                      grad_tbl=None):
    """Backward of `gin_aggregate(tbl, rowptr, col, eps, n_rows, D, bias, epilogue, p_drop)` (models/backbones.py:26-57; bgnn.h:
    bgnn_gin_aggregate_bwd_f32) -> (grad_tbl [n_src, pad4(D)], grad_bias [D] | None, grad_eps float32 [1] | None).
    tbl: the forward's table (read only for grad_eps; may be None with want_eps=False); y: the forward's output (unused without an
    epilogue, may be None); grad_y: [n_rows, >= pad4(D)]; (t_rowptr, t_col): the by-source view of the same edges
    (`DstCSR.transposed()`).  g (the gradient at the epilogue's input) comes from one row pass, grad_bias = its fixed-order column
    sums (`column_sums`), grad_eps = sum_i <g_i, tbl_i> from per-block fp64 partials summed in a fixed order, and
    grad_tbl[j] = (1 + eps) * g[j] + sum_{i : j -> i} g[i] from the forward walk over the swapped view with the same eps tensor.
    want_eps=False launches no eps pass.  No atomics: bit-identical from run to run; no host synchronisation."""
    return _gin_aggregate_bwd(tbl, y, grad_y, t_rowptr, t_col, eps, n_src, D, epilogue, p_drop, want_bias, want_eps, grad_tbl, None)


def gin_aggregate_bwd_hubs(tbl, y, grad_y, t_rowptr, t_col, eps, n_src, D, epilogue=None, p_drop=0.0, want_bias=True, want_eps=True,
                           grad_tbl=None, hubs=None):
    """`gin_aggregate_bwd` (models/backbones.py:26-57; bgnn.h: bgnn_gin_aggregate_bwd_hub_f32) with the walk over the by-source view
    segmented.  hubs: None -- the call of `gin_aggregate_bwd`, the same launches and bits -- or the hub tables of the BY-SOURCE view
    (`DstCSR.transposed_hub_tables`): (threshold, hub_rows, hub_seg_ptr, seg_bounds).  A hub source j >= grad_y's rows (a rank's
    halo slot) has no own term.  g, grad_bias and grad_eps are formed as without hubs."""
    return _gin_aggregate_bwd(tbl, y, grad_y, t_rowptr, t_col, eps, n_src, D, epilogue, p_drop, want_bias, want_eps, grad_tbl, hubs)


def _gin_aggregate_bwd(tbl, y, grad_y, t_rowptr, t_col, eps, n_src, D, epilogue, p_drop, want_bias, want_eps, grad_tbl, hubs):
    n_src, D = int(n_src), int(D)
    _gin_need_cfg("gin_aggregate_bwd", D, epilogue, p_drop)
    _gin_need_eps(eps)
    _need_rows_f32(grad_y, "grad_y", D)
    n_rows = int(grad_y.shape[0])
    if epilogue is not None and epilogue != "none":
        if y is None:
            raise ValueError("y (the forward's output) is needed under an epilogue")
    if y is not None:
        _need_rows_f32(y, "y", D)
        if y.shape[0] != n_rows:
            raise ValueError(f"y must have grad_y's {n_rows} rows")
    if want_eps:
        if tbl is None:
            raise ValueError("tbl (the forward's table) is needed for grad_eps")
        _need_rows_f32(tbl, "tbl", D)
        if tbl.shape[0] < n_rows:
            raise ValueError(f"tbl must have at least grad_y's {n_rows} rows, got {tbl.shape[0]}")
    _gen_need_csr(t_rowptr, t_col, n_src, "t_rowptr")
    dev = grad_y.device
    if grad_tbl is None:
        grad_tbl = torch.empty(n_src, pad4(D), dtype=torch.float32, device=dev)
    else:
        _need_rows_f32(grad_tbl, "grad_tbl", D)
        if grad_tbl.shape[0] != n_src:
            raise ValueError(f"grad_tbl must have n_src = {n_src} rows")
    lib = L.lib()
    g = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=dev)
    grad_eps = ws = None
    if want_eps:
        grad_eps = torch.empty(1, dtype=torch.float32, device=dev)
    if hubs is not None:
        hub_args, ws = _gin_hub_args(hubs, D, dev, lib.bgnn_gin_aggregate_bwd_workspace_bytes(n_rows, D) if want_eps else 0)
        rc = lib.bgnn_gin_aggregate_bwd_hub_f32(
            L.ptr_rows(tbl) if want_eps else None, tbl.stride(0) if want_eps else 0, L.ptr_rows(y), y.stride(0) if y is not None else 0,
            L.ptr_rows(grad_y), grad_y.stride(0), n_rows, L.ptr(t_rowptr), L.ptr(t_col), int(t_col.shape[0]), n_src, D, L.ptr(eps),
            SAGE_EPILOGUES[epilogue], float(p_drop), *hub_args, L.ptr_rows(g), g.stride(0), L.ptr_rows(grad_tbl), grad_tbl.stride(0),
            L.ptr(grad_eps), L.ptr(ws), ws.numel(), L.stream())
        L.check(rc, "bgnn_gin_aggregate_bwd_hub_f32")
        return grad_tbl, (column_sums(g)[:D] if want_bias else None), grad_eps
    if want_eps:
        ws = torch.empty(max(int(lib.bgnn_gin_aggregate_bwd_workspace_bytes(n_rows, D)), 16), dtype=torch.uint8, device=dev)
    rc = lib.bgnn_gin_aggregate_bwd_f32(
        L.ptr_rows(tbl) if want_eps else None, tbl.stride(0) if want_eps else 0, L.ptr_rows(y), y.stride(0) if y is not None else 0,
        L.ptr_rows(grad_y), grad_y.stride(0), n_rows, L.ptr(t_rowptr), L.ptr(t_col), int(t_col.shape[0]), n_src, D, L.ptr(eps),
        SAGE_EPILOGUES[epilogue], float(p_drop), L.ptr_rows(g), g.stride(0), L.ptr_rows(grad_tbl), grad_tbl.stride(0),
        L.ptr(grad_eps), L.ptr(ws), ws.numel() if ws is not None else 0, L.stream())
    L.check(rc, "bgnn_gin_aggregate_bwd_f32")
    return grad_tbl, (column_sums(g)[:D] if want_bias else None), grad_eps


JK_MODES = {"cat": 0, "max": 1}


def _jk_need_cfg(what, D, epilogue, p_drop):
    if D < 1:
        raise ValueError(f"{what} takes D >= 1, got {D}")
    if epilogue not in (None, "none", "relu"):
        raise ValueError(f"{what}: epilogue must be None or 'relu', got {epilogue!r}")
    if not 0.0 <= float(p_drop) < 1.0 or (p_drop > 0 and epilogue != "relu"):
        raise ValueError(f"{what}: 0 <= p_drop < 1, and dropout only after the 'relu' epilogue")


def _jk_need_scales(s, w, n, what):
    for t, name in ((s, "s"), (w, "w")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] < n or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous float32 [>= {n}]")
        L._check_device(t)


def jk_gcn_aggregate(tbl, rowptr, col, s, w, n_rows, D, bias=None, epilogue=None, p_drop=0.0, seed=0, seed_dev=None, out=None):
    """JKNet's scaled-sum conv (models/backbones.py:60-107: PyG GCNConv handed the already normalised adj_t_cache, after its
    transform; bgnn.h: bgnn_jk_gcn_aggregate_f32) -> out [n_rows, pad4(D)] (use out[:, :D]):
    out[i] = epi(w[i] * tbl[i] + s[i] * sum_{t in row i} s[col[t]] * tbl[col[t]] + bias) over a by-destination CSR WITHOUT self
    loops (`JKGraph`; duplicates are separate messages) or its by-source view.  Row i of tbl is row i's root.  tbl: a 2-D row-strided
    view with unit column stride and at least n_rows rows; s, w: float32 [>= tbl rows]; bias: float32 [>= D] or None.  epilogue: None
    or "relu" (then dropout at p_drop, element index row * D + column under the hash of `gcn_aggregate`).  out: None, or a
    row-strided view that MAY BE A COLUMN SLICE OF A WIDER BUFFER (a layer's slice of the layer buffer): only its pad4(D) columns
    are written, the pad columns as 0.  No atomics, no host synchronisation."""
    n_rows, D = int(n_rows), int(D)
    _jk_need_cfg("jk_gcn_aggregate", D, epilogue, p_drop)
    _need_rows_f32(tbl, "tbl", D)
    if tbl.shape[0] < n_rows:
        raise ValueError(f"tbl must have at least n_rows = {n_rows} rows, got {tbl.shape[0]}")
    _jk_need_scales(s, w, int(tbl.shape[0]), "jk_gcn_aggregate")
    _gen_need_csr(rowptr, col, n_rows)
    if bias is not None:
        if bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] < D:
            raise ValueError("bias must be float32 [>= D]")
        if bias.shape[0] < pad4(D) or bias.data_ptr() % 16 != 0:      # the kernel reads whole float4 slots of an aligned row
            bp = torch.zeros(pad4(D), dtype=torch.float32, device=bias.device)
            bp[:D] = bias[:D]
            bias = bp
    if out is None:
        out = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=tbl.device)
    else:
        _need_rows_f32(out, "out", D)
        if out.shape[0] != n_rows or out.data_ptr() == tbl.data_ptr():
            raise ValueError(f"out must have n_rows = {n_rows} rows and be distinct from tbl")
    rc = L.lib().bgnn_jk_gcn_aggregate_f32(
        L.ptr_rows(tbl), tbl.stride(0), int(tbl.shape[0]), L.ptr(s), L.ptr(w), L.ptr(bias), L.ptr(rowptr), L.ptr(col),
        int(col.shape[0]), n_rows, D, SAGE_EPILOGUES[epilogue], float(p_drop), *_seed_args(seed, seed_dev), L.ptr_rows(out),
        out.stride(0), L.stream())
    L.check(rc, "bgnn_jk_gcn_aggregate_f32")
    return out


def jk_gcn_aggregate_bwd(y, grad_y, t_rowptr, t_col, s, w, n_src, D, epilogue=None, p_drop=0.0, want_bias=True, grad_tbl=None):
    """Backward of `jk_gcn_aggregate` (models/backbones.py:60-107; bgnn.h: bgnn_jk_gcn_aggregate_bwd_f32) ->
    (grad_tbl [n_src, pad4(D)], grad_bias [D] | None).  y: the forward's output (a slice of the layer buffer is fine; unused
    without an epilogue, may be None); grad_y: [n_rows, >= pad4(D)], n_rows == n_src; (t_rowptr, t_col): the by-source view of the
    same edges.  g comes from one row pass, grad_bias = its fixed-order column sums (`column_sums`), and
    grad_tbl[j] = w[j] * g[j] + s[j] * sum_{i : j -> i} s[i] * g[i] from the forward walk over the swapped view.  No atomics:
    bit-identical from run to run; no host synchronisation."""
    n_src, D = int(n_src), int(D)
    _jk_need_cfg("jk_gcn_aggregate_bwd", D, epilogue, p_drop)
    _need_rows_f32(grad_y, "grad_y", D)
    n_rows = int(grad_y.shape[0])
    if n_rows != n_src:
        raise ValueError(f"grad_y must have n_src = {n_src} rows (one node set), got {n_rows}")
    if epilogue is not None and epilogue != "none" and y is None:
        raise ValueError("y (the forward's output) is needed under an epilogue")
    if y is not None:
        _need_rows_f32(y, "y", D)
        if y.shape[0] != n_rows:
            raise ValueError(f"y must have grad_y's {n_rows} rows")
    _jk_need_scales(s, w, n_src, "jk_gcn_aggregate_bwd")
    _gen_need_csr(t_rowptr, t_col, n_src, "t_rowptr")
    dev = grad_y.device
    if grad_tbl is None:
        grad_tbl = torch.empty(n_src, pad4(D), dtype=torch.float32, device=dev)
    else:
        _need_rows_f32(grad_tbl, "grad_tbl", D)
        if grad_tbl.shape[0] != n_src:
            raise ValueError(f"grad_tbl must have n_src = {n_src} rows")
    g = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=dev)
    rc = L.lib().bgnn_jk_gcn_aggregate_bwd_f32(
        L.ptr_rows(y), y.stride(0) if y is not None else 0, L.ptr_rows(grad_y), grad_y.stride(0), n_rows, L.ptr(t_rowptr),
        L.ptr(t_col), int(t_col.shape[0]), n_src, L.ptr(s), L.ptr(w), D, SAGE_EPILOGUES[epilogue], float(p_drop), L.ptr_rows(g),
        g.stride(0), L.ptr_rows(grad_tbl), grad_tbl.stride(0), L.stream())
    L.check(rc, "bgnn_jk_gcn_aggregate_bwd_f32")
    return grad_tbl, (column_sums(g)[:D] if want_bias else None)


JK_HEAD_LDS_BYTES = 65536
JK_MAX_LAYERS = 8


def jk_head_supported(L_, H, C, mode):
    """envelope of `jk_head` (bgnn.h: bgnn_jk_head_supported, restated on the host so that no library is needed to ask): mode 'cat' or
    'max', 1 <= L <= 8, 1 <= C <= 32, and W -- 16 (C <= 16) or 32 rows of K floats, K = L * pad4(H) (cat) or pad4(H) (max) rounded
    up to 16 -- fits 64 KB of LDS."""
    L_, H, C = int(L_), int(H), int(C)
    if mode not in JK_MODES or not 1 <= L_ <= JK_MAX_LAYERS or H < 1 or not 1 <= C <= 32:
        return False
    K = L_ * pad4(H) if mode == "cat" else pad4(H)
    return (16 if C <= 16 else 32) * ((K + 15) // 16 * 16) * 4 <= JK_HEAD_LDS_BYTES


def jk_pack_weight(weight, L_, H, mode):
    """the head's weight [C, L*H] (cat) or [C, H] (max) in the layer buffer's padded column layout: [C, L*pad4(H)] | [C, pad4(H)],
    pad columns 0"""
    C, Hp = weight.shape[0], pad4(H)
    nl = L_ if mode == "cat" else 1
    if weight.shape[1] != nl * H:
        raise ValueError(f"weight must be [C, {nl * H}] in mode {mode!r}, got {tuple(weight.shape)}")
    if Hp == H:
        return weight.detach().float().contiguous()
    wp = torch.zeros(C, nl, Hp, dtype=torch.float32, device=weight.device)
    wp[:, :, :H] = weight.detach().float().reshape(C, nl, H)
    return wp.reshape(C, nl * Hp)


def _jk_need_x(x, L_, H):
    Hp = pad4(H)
    if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < L_ * Hp or x.stride(1) != 1
            or x.stride(0) % 4 != 0):
        raise ValueError(f"x must be a float32 [N, >= L * pad4(H) = {L_ * Hp}] row-strided view (row stride % 4 == 0)")
    L._check_device(x)
    if x.data_ptr() % 16 != 0:
        raise ValueError("x must be 16-byte aligned")


def jk_head(x, L_, H, mode, weight_packed, bias, C, log_softmax=True, want_state=False, out=None):
    """JKNet's head in one pass (models/backbones.py:60-107: JumpingKnowledge(cat | max), Linear, log_softmax; bgnn.h:
    bgnn_jk_head_f32) -> out [N, pad4(C)] (use out[:, :C]), or (out, winners uint8 [N, pad4(H)], jumped [N, pad4(H)]) with
    want_state (max mode: what `jk_head_bwd` needs; cat mode returns (out, None, None)).  x: the layer buffer [N, L * pad4(H)], layer l
    in columns [l * pad4(H), l * pad4(H) + H), pad columns 0; weight_packed: `jk_pack_weight(weight, L, H, mode)`; bias: float32 [C]
    or None.  Raises ValueError outside `jk_head_supported(L, H, C, mode)`."""
    L_, H, C = int(L_), int(H), int(C)
    if mode not in JK_MODES:
        raise ValueError(f"jk_head: mode must be 'cat' or 'max', got {mode!r}")
    if H < 1 or C < 1 or L_ < 1:
        raise ValueError(f"jk_head takes L, H, C >= 1, got {(L_, H, C)}")
    if not jk_head_supported(L_, H, C, mode):
        raise ValueError(f"jk_head: (L, H, C, mode) = {(L_, H, C, mode)} is outside the kernel's envelope (jk_head_supported)")
    _jk_need_x(x, L_, H)
    Hp, Cp = pad4(H), pad4(C)
    K = L_ * Hp if mode == "cat" else Hp
    wp = weight_packed
    if (not isinstance(wp, torch.Tensor) or wp.dtype != torch.float32 or wp.dim() != 2 or tuple(wp.shape) != (C, K)
            or not wp.is_contiguous()):
        raise ValueError(f"weight_packed must be a contiguous float32 [{C}, {K}] (jk_pack_weight)")
    if wp.data_ptr() % 16 != 0:
        wp = wp.clone()
    if bias is not None and (bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] != C or not bias.is_contiguous()):
        raise ValueError(f"bias must be a contiguous float32 [{C}]")
    N = int(x.shape[0])
    if out is None:
        out = torch.empty(N, Cp, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != N or out.shape[1] < Cp or out.stride(1) != 1:
        raise ValueError(f"out must be float32 [N, >= {Cp}] with unit column stride")
    win = jump = None
    if want_state and mode == "max":
        win = torch.empty(N, Hp, dtype=torch.uint8, device=x.device)
        jump = torch.empty(N, Hp, dtype=torch.float32, device=x.device)
    rc = L.lib().bgnn_jk_head_f32(L.ptr_rows(x), x.stride(0), N, L_, H, JK_MODES[mode], L.ptr(wp), K, L.ptr(bias), C,
                                  1 if log_softmax else 0, L.ptr_rows(out), out.stride(0), L.ptr(win), L.ptr(jump), Hp, L.stream())
    L.check(rc, "bgnn_jk_head_f32")
    return (out, win, jump) if want_state else out


def jk_head_bwd(x, L_, H, mode, weight_packed, C, logp, grad_out, log_softmax=True, win=None, jump=None, want_x=True):
    """Backward of `jk_head` (models/backbones.py:60-107) -> (grad_x [N, L * pad4(H)] | None, grad_weight_packed [C, K], grad_bias
    [C]).  dlogits from (logp, grad_out) in a row pass (`appnp_log_softmax_bwd`; grad_out itself without the log_softmax), grad_bias
    = `column_sums`, grad_weight = dlogits^T J by `gram` where supported (J: x itself in cat mode, the forward's jumped rows in max
    mode), dJ = dlogits W by `linear` or mm; cat: dJ's column blocks are the layer gradients; max: one streaming pass
    (bgnn.h: bgnn_jk_max_route_f32) writes every layer's slice from dJ and the forward's uint8 winners.  grad_weight is in the
    padded layout of `jk_pack_weight`."""
    L_, H, C = int(L_), int(H), int(C)
    if mode not in JK_MODES:
        raise ValueError(f"jk_head_bwd: mode must be 'cat' or 'max', got {mode!r}")
    _jk_need_x(x, L_, H)
    Hp, Cp = pad4(H), pad4(C)
    N = int(x.shape[0])
    K = L_ * Hp if mode == "cat" else Hp
    if mode == "max":
        if (win is None or jump is None or win.dtype != torch.uint8 or tuple(win.shape) != (N, Hp) or not win.is_contiguous()
                or jump.dtype != torch.float32 or tuple(jump.shape) != (N, Hp) or not jump.is_contiguous()):
            raise ValueError(f"max mode needs the forward's state: win uint8 [{N}, {Hp}] and jump float32 [{N}, {Hp}]")
    _need_rows_f32(grad_out, "grad_out", C)
    if grad_out.shape[0] != N:
        raise ValueError(f"grad_out must have {N} rows")
    if log_softmax:
        _need_rows_f32(logp, "logp", C)
        dz = appnp_log_softmax_bwd(logp, grad_out, C)
    else:
        dz = torch.zeros(N, Cp, dtype=torch.float32, device=x.device)
        dz[:, :C] = grad_out[:, :C]
    gb = column_sums(dz)[:C]
    J = x[:, :K] if mode == "cat" else jump
    if gram_supported(K, Cp) and J.stride(0) % 4 == 0 and J.data_ptr() % 16 == 0:
        gw = gram(J, dz).t()[:C].contiguous()                   # the kernel's wide operand comes first: (J^T dz)^T
    else:
        gw = dz.t().mm(J)[:C]
    gx = None
    if want_x:
        wpad = torch.zeros(Cp, K, dtype=torch.float32, device=x.device)
        wpad[:C] = weight_packed
        if linear_supported(Cp, K):
            dj = linear(dz, wpad.t().contiguous(), torch.zeros(K, dtype=torch.float32, device=x.device))
        else:
            dj = dz.mm(wpad)
        if mode == "cat":
            gx = dj
        else:
            gx = torch.empty(N, L_ * Hp, dtype=torch.float32, device=x.device)
            rc = L.lib().bgnn_jk_max_route_f32(L.ptr_rows(dj), dj.stride(0), L.ptr(win), N, L_, H, L.ptr_rows(gx), gx.stride(0),
                                               L.stream())
            L.check(rc, "bgnn_jk_max_route_f32")
    return gx, gw, gb


APPNP_STORES = {"state": 0, "out": 1, "log_softmax": 2}


def appnp_step(tbl, h, rowptr, col, dinv, n_rows, D, alpha, first, store, hubs=None, out=None):
    """One step of `appnp_propagate`'s recurrence over a RECTANGULAR graph (models/backbones.py:110-128 on a node partition; bgnn.h:
    bgnn_appnp_step_f32) -> out [n_rows, pad4(D)]: row i = store((1 - alpha) * dinv[i] * sum_t w_t * tbl[col[t]] + alpha * h[i]).
    tbl [n_tbl >= n_rows, >= pad4(D)]: the owned rows followed by the halo slots -- h's rows with `first` (w_t = dinv[col[t]], dinv
    float32 [>= n_tbl]), else the scaled state dinv * z_k (w_t = 1, dinv [>= n_rows]); h: the n_rows teleport rows; (rowptr, col): the
    CSR of the n_rows owned rows, `hubs` its hub tables.  store: "state" (dinv[i] * z, the next step's table rows), "out" (z) or
    "log_softmax".  K calls on a square graph are `appnp_propagate` bit for bit (the same launches).  No allocation beyond `out` and
    the hub partial rows, no host synchronisation."""
    n_rows, D, alpha = int(n_rows), int(D), float(alpha)
    if store not in APPNP_STORES:
        raise ValueError(f"store must be 'state', 'out' or 'log_softmax', got {store!r}")
    if D < 1:
        raise ValueError("D must be at least 1")
    _need_rows_f32(tbl, "tbl", D)
    _need_rows_f32(h, "h", D)
    n_tbl = int(tbl.shape[0])
    if h.shape[0] != n_rows:
        raise ValueError(f"h must have n_rows = {n_rows} rows, got {h.shape[0]}")
    if n_tbl < n_rows:
        raise ValueError(f"tbl must have at least n_rows = {n_rows} rows (the owned rows, then the halo slots), got {n_tbl}")
    if dinv.dtype != torch.float32 or dinv.dim() != 1 or dinv.shape[0] < (n_tbl if first else n_rows):
        raise ValueError("dinv must be float32 [>= rows of tbl] on the first step, [>= n_rows] otherwise")
    if rowptr.dtype != torch.int32 or rowptr.dim() != 1 or rowptr.shape[0] < n_rows + 1 or col.dtype != torch.int32 or col.dim() != 1:
        raise ValueError("rowptr must be int32 [n_rows + 1] and col int32 [E]")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    if out is None:
        out = torch.empty(n_rows, pad4(D), dtype=torch.float32, device=h.device)
    else:
        _need_rows_f32(out, "out", D)
        if out.shape[0] != n_rows:
            raise ValueError(f"out must have n_rows = {n_rows} rows")
    if hubs is None:
        hub_args, ws = (0, None, 0, None, None, 0), None
    else:
        thr, rows, seg_ptr, bounds = hubs
        n_seg = int(bounds.shape[0]) // 2
        hub_args = (int(thr), L.ptr(rows), int(rows.shape[0]), L.ptr(seg_ptr), L.ptr(bounds), n_seg)
        ws = torch.empty(n_seg * pad4(D) * 4 + 16, dtype=torch.uint8, device=h.device)
    rc = L.lib().bgnn_appnp_step_f32(
        L.ptr_rows(tbl), tbl.stride(0), n_tbl, L.ptr_rows(h), h.stride(0), L.ptr(rowptr), L.ptr(col), L.ptr(dinv), int(dinv.shape[0]),
        n_rows, D, alpha, 1 if first else 0, APPNP_STORES[store], *hub_args, L.ptr(ws), ws.numel() if ws is not None else 0,
        L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_appnp_step_f32")
    return out


def appnp_log_softmax_bwd(y, grad_y, D, out=None):
    """g = grad_y - exp(y) * rowsum(grad_y) over D <= 128 columns (bgnn.h: bgnn_appnp_log_softmax_bwd_f32): the gradient at z_K of
    `appnp_propagate(..., epilogue="log_softmax")` from its output y -> g [rows, pad4(D)], pad columns 0; `appnp_propagate` over
    the by-source view then turns g into the gradient with respect to h."""
    D = int(D)
    _need_rows_f32(y, "y", D)
    _need_rows_f32(grad_y, "grad_y", D)
    if grad_y.shape[0] != y.shape[0]:
        raise ValueError("y and grad_y must have the same number of rows")
    if out is None:
        out = torch.empty(y.shape[0], pad4(D), dtype=torch.float32, device=y.device)
    else:
        _need_rows_f32(out, "out", D)
    rc = L.lib().bgnn_appnp_log_softmax_bwd_f32(L.ptr_rows(y), y.stride(0), L.ptr_rows(grad_y), grad_y.stride(0), int(y.shape[0]), D,
                                                L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_appnp_log_softmax_bwd_f32")
    return out


def _fdrop_check(t, what, shape=None):
    if t.dtype != torch.float32 or t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{what} must be float32 [N, D]" + (f" = {tuple(shape)}" if shape is not None else ""))
    L._check_device(t)
    if not t.is_contiguous() or t.data_ptr() % 16 != 0:
        raise ValueError(f"{what} must be contiguous and 16-byte aligned")


def _fdrop_row_ids(row_ids, N):
    if row_ids.dtype != torch.int64 or row_ids.dim() != 1 or row_ids.shape[0] != N or not row_ids.is_contiguous():
        raise ValueError(f"row_ids must be a contiguous int64 [{N}]")
    L._check_device(row_ids)


def feature_dropout(x, p, seed, seed_dev=None, bias=None, relu=False, out=None, row_ids=None):
    """y = drop(act(x + bias)) over a contiguous [N, D] activation of any width (models/backbones.py:110-128: APPNP_Net's
    F.dropout(x) and F.dropout(F.relu(lin1(x))); bgnn.h: bgnn_feature_dropout_f32).  act = ReLU when `relu`; bias float32 [D] or
    None; element row * D + column is kept by the (seed + seed_dev, element index) hash of `bn_relu_dropout` and scaled by
    1 / (1 - p).  0 <= p < 1; `out` may be x.  row_ids: int64 [N], the GLOBAL row of every row (a rank's rows of a partition): the
    element index is then row_ids[r] * D + column, the masks of the whole-graph call (bgnn_feature_dropout_rows_f32); None = row r."""
    _fdrop_check(x, "x")
    if not 0.0 <= float(p) < 1.0:
        raise ValueError("p must lie in [0, 1)")
    N, D = x.shape
    if D < 1:
        raise ValueError("x needs at least one column")
    if bias is not None and (bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] != D):
        raise ValueError("bias must be float32 [D]")
    if out is None:
        out = torch.empty_like(x)
    else:
        _fdrop_check(out, "out", x.shape)
    if row_ids is not None:
        _fdrop_row_ids(row_ids, N)
        rc = L.lib().bgnn_feature_dropout_rows_f32(L.ptr(x), L.ptr(bias), L.ptr(row_ids), N, D, 1 if relu else 0, float(p),
                                                   *_seed_args(seed, seed_dev), L.ptr(out), L.stream())
        L.check(rc, "bgnn_feature_dropout_rows_f32")
        return out
    rc = L.lib().bgnn_feature_dropout_f32(L.ptr(x), L.ptr(bias), N, D, 1 if relu else 0, float(p), *_seed_args(seed, seed_dev),
                                          L.ptr(out), L.stream())
    L.check(rc, "bgnn_feature_dropout_f32")
    return out


def feature_dropout_bwd(grad_y, p, seed, seed_dev=None, y=None, relu=False, out=None, row_ids=None):
    """Backward of `feature_dropout(x, p, seed, seed_dev, bias, relu)` -> grad_x = grad_y * keep / (1 - p) * [act'] (the bias
    gradient is its column sums).  With `relu` the mask and the ReLU state are read off the forward's output `y` (y > 0 <=> kept
    and positive); without it the mask is redrawn from the seed and `y` is not needed.  row_ids: as in the forward."""
    _fdrop_check(grad_y, "grad_y")
    if not 0.0 <= float(p) < 1.0:
        raise ValueError("p must lie in [0, 1)")
    if relu:
        if y is None:
            raise ValueError("feature_dropout_bwd(relu=True) needs the forward's output y")
        _fdrop_check(y, "y", grad_y.shape)
    N, D = grad_y.shape
    if out is None:
        out = torch.empty_like(grad_y)
    else:
        _fdrop_check(out, "out", grad_y.shape)
    if row_ids is not None:
        _fdrop_row_ids(row_ids, N)
        rc = L.lib().bgnn_feature_dropout_rows_bwd_f32(L.ptr(y) if relu else None, L.ptr(grad_y), L.ptr(row_ids), N, D,
                                                       1 if relu else 0, float(p), *_seed_args(seed, seed_dev), L.ptr(out), L.stream())
        L.check(rc, "bgnn_feature_dropout_rows_bwd_f32")
        return out
    rc = L.lib().bgnn_feature_dropout_bwd_f32(L.ptr(y) if relu else None, L.ptr(grad_y), N, D, 1 if relu else 0, float(p),
                                              *_seed_args(seed, seed_dev), L.ptr(out), L.stream())
    L.check(rc, "bgnn_feature_dropout_bwd_f32")
    return out


GAT_EPILOGUES = {None: 0, "none": 0, "elu": 1, "log_softmax": 2}
GAT_MAX_HEADS, GAT_MAX_C = 8, 128


def _gat_check(tbl, H, C, what):
    H, C = int(H), int(C)
    if not tbl.is_cuda:
        raise RuntimeError(f"bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path (got a {tbl.device} tensor)")
    if not (1 <= H <= GAT_MAX_HEADS and 1 <= C <= GAT_MAX_C):
        raise RuntimeError(f"{what}: unsupported shape: heads = {H}, channels per head = {C} (1 <= heads <= {GAT_MAX_HEADS}, "
                           f"1 <= channels <= {GAT_MAX_C})")
    if tbl.dtype != torch.float32 or tbl.dim() != 2 or tbl.shape[1] < pad4(H * C):
        raise ValueError(f"{what}: the table must be float32 [N, >= pad4(H*C)]")
    return H, C


def _gat_need(t, what, shape, dtype=torch.float32):
    """an operand of the GAT entry points: dtype, exact shape and contiguity, before its raw pointer goes to a kernel"""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} (got {t.dtype} {tuple(t.shape)})")


def _gat_need_rows(t, what, rows, width):
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or t.shape[1] < width or t.stride(1) != 1:
        raise ValueError(f"{what} must be float32 [{rows}, >= {width}] with unit column stride (got {t.dtype} {tuple(t.shape)})")


def _gat_need_bias(bias, HC):
    if bias is not None and (bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] < HC):
        raise ValueError("bias must be float32 [>= H*C]")


def _gat_need_seed_words(seed_att_dev, seed_dev):
    for w, what in ((seed_att_dev, "seed_att_dev"), (seed_dev, "seed_dev")):
        if w is not None and (w.dtype != torch.int64 or w.numel() != 1):
            raise ValueError(f"{what} must be an int64 device tensor of one element")


def _gat_need_probs(p_att, p_drop):
    if not (0.0 <= float(p_att) < 1.0 and 0.0 <= float(p_drop) < 1.0):
        raise ValueError("p_att and p_drop must lie in [0, 1)")


def _gat_need_csrs(rowptr, col, t_rowptr, t_eid, t_dst, R, N, E):
    """the backwards' two views of the edges: by destination over R rows, by source over N"""
    for t, what, n in ((rowptr, "rowptr", R + 1), (col, "col", E), (t_rowptr, "t_rowptr", N + 1), (t_eid, "t_eid", E), (t_dst, "t_dst", E)):
        _gat_need(t, what, (n,), torch.int32)


def _gat_fwd_outputs(n_rows, H, W, epilogue, want_pre, dev):
    """-> (out, state, pre | None, pre_arg): without an epilogue `pre` IS out, and the entry is handed no second buffer"""
    out = torch.empty(n_rows, W, dtype=torch.float32, device=dev)
    state = torch.empty(n_rows, H, 2, dtype=torch.float32, device=dev)
    pre = None
    if want_pre:
        pre = out if GAT_EPILOGUES[epilogue] == 0 else torch.empty(n_rows, W, dtype=torch.float32, device=dev)
    return out, state, pre, (pre if (pre is not None and pre is not out) else None)


def _gat_ids_paired(row_ids, edge_base, what):
    """both ids or neither: checked before anything else, a half-given pair is a caller's mistake on any device"""
    if (row_ids is None) != (edge_base is None):
        raise ValueError(f"{what}: row_ids and edge_base are given together (a rank's rows need the global positions of both masks)")


def _gat_ids(row_ids, edge_base, n_rows, dev, what):
    """the id pair, when given: int64, contiguous, [n_rows], on the table's device"""
    if row_ids is None:
        return
    for t, name in ((row_ids, "row_ids"), (edge_base, "edge_base")):
        _gat_need(t, name, (n_rows,), torch.int64)
        if t.device != dev:
            raise ValueError(f"{what}: {name} must be on the table's device {dev} (got {t.device})")


def gat_scores(tbl, att_src, att_dst, H, C):
    """s_src[n,h] = <tbl[n,h,:], att_src[h,:]>, s_dst likewise (models/backbones.py:404-438 -> GATConv's alpha_src / alpha_dst;
    bgnn.h: bgnn_gat_scores_f32) -> two float32 [N, H] in one read of tbl [N, >= pad4(H*C)].  att_*: float32 with H*C elements."""
    H, C = _gat_check(tbl, H, C, "gat_scores")
    a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
    if a_s.dtype != torch.float32 or a_d.dtype != torch.float32 or a_s.numel() != H * C or a_d.numel() != H * C:
        raise ValueError("att_src / att_dst must be float32 with H*C elements")
    if a_s.data_ptr() % 16:
        a_s = a_s.clone()
    if a_d.data_ptr() % 16:
        a_d = a_d.clone()
    N = int(tbl.shape[0])
    s_src = torch.empty(N, H, dtype=torch.float32, device=tbl.device)
    s_dst = torch.empty(N, H, dtype=torch.float32, device=tbl.device)
    rc = L.lib().bgnn_gat_scores_f32(L.ptr_rows(tbl), tbl.stride(0), N, H, C, L.ptr(a_s), L.ptr(a_d), L.ptr(s_src), L.ptr(s_dst),
                                     L.stream())
    L.check(rc, "bgnn_gat_scores_f32")
    return s_src, s_dst


def gat_aggregate(tbl, s_src, s_dst, rowptr, col, n_rows, H, C, bias=None, negative_slope=0.2, p_att=0.0, seed_att=0,
                  seed_att_dev=None, epilogue=None, p_drop=0.0, seed=0, seed_dev=None, want_pre=False, return_alpha=False, row_ids=None,
                  edge_base=None):
    """GAT attention aggregation (models/backbones.py:404-438, bgnn.h: bgnn_gat_aggregate_f32) over a CSR that holds one self loop per
    row (`build_dst_csr(rewrite_self_loops=True)`): out[i,h,:] = epi(sum_t a~[t,h] * tbl[col[t],h,:] + bias[h,:]) with
    a~ = softmax_t(leaky_relu(s_src[col[t],h] + s_dst[i,h])) * m[t,h], m the attention-dropout mask at p_att (element t*H + h of the
    counter hash, seed_att + seed_att_dev).  epilogue: None, "elu" (then dropout at p_drop, seed + seed_dev, element
    i*(H*C) + column) or "log_softmax" (H == 1).  bias: float32 [>= H*C], 16-byte aligned, or None.
    -> (out [n_rows, pad4(H*C)], state [n_rows, H, 2] = (max, denominator), pre | None, alpha | None): pre (want_pre) is the conv
    output before the epilogue, alpha (return_alpha) the post-dropout coefficients [E', H] in CSR order.
    row_ids, edge_base: int64 [n_rows] each, given together (a rank's rows of a partition): the GLOBAL
    id of every output row and the position of its first edge in the whole graph's CSR; the masks are then hashed at
    row_ids[i]*(H*C) + column and (edge_base[i] + (t - rowptr[i]))*H + h, those of the whole-graph call.  None: row i, edge t."""
    _gat_ids_paired(row_ids, edge_base, "gat_aggregate")
    H, C = _gat_check(tbl, H, C, "gat_aggregate")
    n_rows, E = int(n_rows), int(col.shape[0])
    dev = tbl.device
    if epilogue == "log_softmax" and H != 1:
        raise RuntimeError("gat_aggregate: unsupported shape: the log_softmax epilogue needs heads == 1")
    _gat_need_bias(bias, H * C)
    _gat_need(s_src, "s_src", (int(tbl.shape[0]), H))
    _gat_need(s_dst, "s_dst", (n_rows, H))
    _gat_need(rowptr, "rowptr", (n_rows + 1,), torch.int32)
    _gat_need(col, "col", (E,), torch.int32)
    _gat_ids(row_ids, edge_base, n_rows, dev, "gat_aggregate")
    _gat_need_seed_words(seed_att_dev, seed_dev)
    _gat_need_probs(p_att, p_drop)
    out, state, pre, pre_arg = _gat_fwd_outputs(n_rows, H, pad4(H * C), epilogue, want_pre, dev)
    alpha = torch.empty(E, H, dtype=torch.float32, device=dev)       # always formed: the gather pass streams it
    rc = L.lib().bgnn_gat_aggregate_f32(
        L.ptr_rows(tbl), tbl.stride(0), int(tbl.shape[0]), L.ptr(s_src), L.ptr(s_dst), L.ptr(bias), L.ptr(rowptr), L.ptr(col), E,
        n_rows, H, C, float(negative_slope), float(p_att), *_seed_args(seed_att, seed_att_dev), GAT_EPILOGUES[epilogue],
        float(p_drop), *_seed_args(seed, seed_dev), L.ptr(row_ids), L.ptr(edge_base), L.ptr(state), L.ptr(alpha), None, 0,
        L.ptr_rows(pre_arg), pre_arg.stride(0) if pre_arg is not None else 0, L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_gat_aggregate_f32")
    return out, state, pre, (alpha if return_alpha else None)


def gat_aggregate_bwd(tbl, s_src, s_dst, state, alpha, pre, grad_y, rowptr, col, t_rowptr, t_eid, t_dst, H, C, bias=None,
                      negative_slope=0.2, p_att=0.0, seed_att=0, seed_att_dev=None, epilogue=None, p_drop=0.0, seed=0, seed_dev=None,
                      want_bias=True, n_rows=None, row_ids=None, edge_base=None):
    """Backward of `gat_aggregate` (bgnn.h: bgnn_gat_aggregate_bwd_f32) from what the forward returned (state, alpha with
    return_alpha, pre with want_pre) and grad_y [N, >= pad4(H*C)] -> (grad_tbl [N, pad4(H*C)] = the gather part of dL/dtbl,
    ds_src [N, H], ds_dst [N, H], grad_bias [H*C] | None).  The caller adds ds_src (x) att_src + ds_dst (x) att_dst to grad_tbl and
    forms the att gradients.  (t_rowptr, t_eid, t_dst) = `DstCSR.transposed()`.  Three launches, no atomics: bit-identical runs.
    n_rows: the destination rows when the table holds more sources than that (a rank's extended graph: N = tbl rows = n_ext
    sources, the first n_rows of them the owned rows).  Then s_dst, state, pre, grad_y and rowptr ([n_rows + 1]) are over n_rows,
    s_src and t_rowptr ([N + 1]) over N, and the results are grad_tbl [N, .], ds_src [N, H], ds_dst [n_rows, H].  None: N.
    row_ids, edge_base: as in `gat_aggregate`: both masks are redrawn at the global positions."""
    _gat_ids_paired(row_ids, edge_base, "gat_aggregate_bwd")
    H, C = _gat_check(tbl, H, C, "gat_aggregate_bwd")
    N, E = int(tbl.shape[0]), int(col.shape[0])
    R = N if n_rows is None else int(n_rows)
    if not 0 <= R <= N:
        raise ValueError(f"gat_aggregate_bwd: n_rows = {R} must lie in [0, {N}] (the table's rows are the sources)")
    dev = tbl.device
    W = pad4(H * C)
    _gat_need(s_src, "s_src", (N, H))
    _gat_need(s_dst, "s_dst", (R, H))
    _gat_need(state, "state", (R, H, 2))
    _gat_need(alpha, "alpha", (E, H))
    _gat_need_rows(pre, "pre", R, W)
    _gat_need_rows(grad_y, "grad_y", R, W)
    _gat_need_csrs(rowptr, col, t_rowptr, t_eid, t_dst, R, N, E)
    _gat_ids(row_ids, edge_base, R, dev, "gat_aggregate_bwd")
    _gat_need_bias(bias, H * C)
    _gat_need_seed_words(seed_att_dev, seed_dev)
    lib = L.lib()
    g = torch.empty(R, W, dtype=torch.float32, device=dev)
    grad_tbl = torch.empty(N, W, dtype=torch.float32, device=dev)
    ds_src = torch.empty(N, H, dtype=torch.float32, device=dev)
    ds_dst = torch.empty(R, H, dtype=torch.float32, device=dev)
    wsb = int(lib.bgnn_gat_aggregate_workspace_bytes(E, R, H))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    rc = lib.bgnn_gat_aggregate_bwd_f32(
        L.ptr_rows(tbl), tbl.stride(0), N, L.ptr(s_src), L.ptr(s_dst), L.ptr(bias), L.ptr(state), L.ptr(alpha), L.ptr_rows(pre),
        pre.stride(0), L.ptr_rows(grad_y), grad_y.stride(0), L.ptr(rowptr), L.ptr(col), L.ptr(t_rowptr), L.ptr(t_eid), L.ptr(t_dst),
        E, R, H, C, float(negative_slope), float(p_att), *_seed_args(seed_att, seed_att_dev), GAT_EPILOGUES[epilogue], float(p_drop),
        *_seed_args(seed, seed_dev), L.ptr(ws), ws.numel(), L.ptr(row_ids), L.ptr(edge_base), L.ptr_rows(g), g.stride(0),
        L.ptr_rows(grad_tbl), grad_tbl.stride(0), L.ptr(ds_src), L.ptr(ds_dst), L.stream())
    L.check(rc, "bgnn_gat_aggregate_bwd_f32")
    return grad_tbl, ds_src, ds_dst, (column_sums(g)[:H * C] if want_bias else None)


def _gatv2_check(tbl, att, H, C, what):
    """the one table [N, >= 2 * pad4(H*C)] (XL at column 0, XR at column pad4(H*C)) and att [H*C] -> (H, C, att flat and aligned)"""
    H, C = int(H), int(C)
    if not tbl.is_cuda:
        raise RuntimeError(f"bridged_gnn_amd ops need CUDA(HIP) tensors; there is no CPU path (got a {tbl.device} tensor)")
    if not (1 <= H <= GAT_MAX_HEADS and 1 <= C <= GAT_MAX_C):
        raise RuntimeError(f"{what}: unsupported shape: heads = {H}, channels per head = {C} (1 <= heads <= {GAT_MAX_HEADS}, "
                           f"1 <= channels <= {GAT_MAX_C})")
    if tbl.dtype != torch.float32 or tbl.dim() != 2 or tbl.shape[1] < 2 * pad4(H * C) or tbl.stride(1) != 1:
        raise ValueError(f"{what}: the table must be float32 [N, >= 2 * pad4(H*C)] with unit column stride")
    a = att.reshape(-1).contiguous()
    if a.dtype != torch.float32 or a.numel() != H * C or a.device != tbl.device:
        raise ValueError("att must be float32 with H*C elements on the table's device")
    if a.data_ptr() % 16:
        a = a.clone()
    return H, C, a


def gatv2_aggregate(tbl, att, rowptr, col, n_rows, H, C, bias=None, negative_slope=0.2, p_att=0.0, seed_att=0, seed_att_dev=None,
                    epilogue=None, p_drop=0.0, seed=0, seed_dev=None, want_pre=False, return_alpha=False, row_ids=None, edge_base=None):
    """GATv2 attention conv in one pass (models/backbones.py:302-358, bgnn.h: bgnn_gatv2_aggregate_f32) over a CSR that holds one self
    loop per row (`build_dst_csr(rewrite_self_loops=True)`).  tbl [N, >= 2P], P = pad4(H*C): x_l at columns [0, H*C), x_r at
    [P, P + H*C).  out[i,h,:] = epi(sum_t a~[t,h] * x_l[col[t],h,:] + bias[h,:]), a~ = softmax_t(<att[h], leaky_relu(x_l[col[t],h] +
    x_r[i,h])>) * m[t,h], m the attention-dropout mask at p_att (element t*H + h of the counter hash, seed_att + seed_att_dev).
    epilogue: None, "elu" (then dropout at p_drop, seed + seed_dev, element i*(H*C) + column) or "log_softmax" (H == 1).  bias:
    float32 [>= H*C], 16-byte aligned, or None.
    -> (out [n_rows, P], state [n_rows, H, 2] = (max, denominator), pre | None, alpha | None): pre (want_pre) is the conv output
    before the epilogue, alpha (return_alpha) the post-dropout coefficients [E', H] in CSR order.
    row_ids, edge_base: int64 [n_rows] each, given together (a rank's rows of a partition): the GLOBAL
    id of every output row and the position of its first edge in the whole graph's CSR; the masks are then hashed at
    row_ids[i]*(H*C) + column and (edge_base[i] + (t - rowptr[i]))*H + h, those of the whole-graph call.  None: row i, edge t."""
    _gat_ids_paired(row_ids, edge_base, "gatv2_aggregate")
    n_rows, E = int(n_rows), int(col.shape[0])
    if row_ids is not None:                                # dtype and length: a caller's mistake on any device, as the pairing
        _gat_need(row_ids, "row_ids", (n_rows,), torch.int64)
        _gat_need(edge_base, "edge_base", (n_rows,), torch.int64)
    H, C, a = _gatv2_check(tbl, att, H, C, "gatv2_aggregate")
    dev = tbl.device
    if epilogue == "log_softmax" and H != 1:
        raise RuntimeError("gatv2_aggregate: unsupported shape: the log_softmax epilogue needs heads == 1")
    _gat_need_bias(bias, H * C)
    if int(tbl.shape[0]) < n_rows:
        raise ValueError("the table must hold a row for every destination row")
    _gat_need(rowptr, "rowptr", (n_rows + 1,), torch.int32)
    _gat_need(col, "col", (E,), torch.int32)
    _gat_ids(row_ids, edge_base, n_rows, dev, "gatv2_aggregate")
    _gat_need_seed_words(seed_att_dev, seed_dev)
    _gat_need_probs(p_att, p_drop)
    out, state, pre, pre_arg = _gat_fwd_outputs(n_rows, H, pad4(H * C), epilogue, want_pre, dev)
    alpha = torch.empty(E, H, dtype=torch.float32, device=dev) if return_alpha else None
    rc = L.lib().bgnn_gatv2_aggregate_f32(
        L.ptr_rows(tbl), tbl.stride(0), int(tbl.shape[0]), L.ptr(a), L.ptr(bias), L.ptr(rowptr), L.ptr(col), E, n_rows, H, C,
        float(negative_slope), float(p_att), *_seed_args(seed_att, seed_att_dev), GAT_EPILOGUES[epilogue], float(p_drop),
        *_seed_args(seed, seed_dev), L.ptr(row_ids), L.ptr(edge_base), L.ptr(state), L.ptr(alpha), L.ptr_rows(pre_arg),
        pre_arg.stride(0) if pre_arg is not None else 0, L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_gatv2_aggregate_f32")
    return out, state, pre, alpha


def gatv2_aggregate_bwd(tbl, att, state, pre, grad_y, rowptr, col, t_rowptr, t_eid, t_dst, H, C, bias=None, negative_slope=0.2,
                        p_att=0.0, seed_att=0, seed_att_dev=None, epilogue=None, p_drop=0.0, seed=0, seed_dev=None, want_bias=True,
                        n_rows=None, row_ids=None, edge_base=None):
    """Backward of `gatv2_aggregate` (bgnn.h: bgnn_gatv2_aggregate_bwd_f32) from the forward's table, (state, pre with want_pre) and
    grad_y [N, >= pad4(H*C)] -> (grad_tbl [N, 2P] = the whole dL/dtbl: dx_l at columns [0, H*C), dx_r at [P, P + H*C), pad columns 0;
    grad_att [H*C]; grad_bias [H*C] | None).  (t_rowptr, t_eid, t_dst) = `DstCSR.transposed()`.  The coefficients are rebuilt from
    the state and both dropout masks redrawn from their seeds.  Four launches, no atomics: bit-identical runs.
    n_rows: the destination rows when the table holds more sources than that (a rank's extended graph: N = tbl rows = n_ext
    sources, the first n_rows of them the owned rows).  Then state, pre, grad_y and rowptr
    ([n_rows + 1]) are over n_rows, t_rowptr ([N + 1]) over N, and grad_tbl is [N, 2P] with the dx_r half of the rows n_rows .. N
    exactly 0; grad_att sums this call's edges.  None: N.
    row_ids, edge_base: as in `gatv2_aggregate`: both masks are redrawn at the global positions."""
    _gat_ids_paired(row_ids, edge_base, "gatv2_aggregate_bwd")
    N, E = int(tbl.shape[0]), int(col.shape[0])
    R = N if n_rows is None else int(n_rows)
    if not 0 <= R <= N:
        raise ValueError(f"gatv2_aggregate_bwd: n_rows = {R} must lie in [0, {N}] (the table's rows are the sources)")
    if row_ids is not None:                                # as in `gatv2_aggregate`
        _gat_need(row_ids, "row_ids", (R,), torch.int64)
        _gat_need(edge_base, "edge_base", (R,), torch.int64)
    H, C, a = _gatv2_check(tbl, att, H, C, "gatv2_aggregate_bwd")
    dev = tbl.device
    W = pad4(H * C)
    _gat_need(state, "state", (R, H, 2))
    _gat_need_rows(pre, "pre", R, W)
    _gat_need_rows(grad_y, "grad_y", R, W)
    _gat_need_csrs(rowptr, col, t_rowptr, t_eid, t_dst, R, N, E)
    _gat_ids(row_ids, edge_base, R, dev, "gatv2_aggregate_bwd")
    _gat_need_bias(bias, H * C)
    _gat_need_seed_words(seed_att_dev, seed_dev)
    lib = L.lib()
    g = torch.empty(R, W, dtype=torch.float32, device=dev)
    grad_tbl = torch.empty(N, 2 * W, dtype=torch.float32, device=dev)
    grad_att = torch.empty(H * C, dtype=torch.float32, device=dev)
    wsb = int(lib.bgnn_gatv2_aggregate_workspace_bytes(E, R, H, C))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    rc = lib.bgnn_gatv2_aggregate_bwd_f32(
        L.ptr_rows(tbl), tbl.stride(0), N, L.ptr(a), L.ptr(bias), L.ptr(state), L.ptr_rows(pre), pre.stride(0), L.ptr_rows(grad_y),
        grad_y.stride(0), L.ptr(rowptr), L.ptr(col), L.ptr(t_rowptr), L.ptr(t_eid), L.ptr(t_dst), E, R, H, C, float(negative_slope),
        float(p_att), *_seed_args(seed_att, seed_att_dev), GAT_EPILOGUES[epilogue], float(p_drop), *_seed_args(seed, seed_dev),
        L.ptr(ws), ws.numel(), L.ptr(row_ids), L.ptr(edge_base), L.ptr_rows(g), g.stride(0), L.ptr_rows(grad_tbl), grad_tbl.stride(0),
        L.ptr(grad_att), L.stream())
    L.check(rc, "bgnn_gatv2_aggregate_bwd_f32")
    return grad_tbl, grad_att, (column_sums(g)[:H * C] if want_bias else None)


def rows_segment_add(src, seg_ptr, idx, row, dst, D=None, accumulate=True):
    """dst[row[s]] (+)= sum_{k in [seg_ptr[s], seg_ptr[s+1])} src[idx[k]] (bgnn.h: bgnn_rows_segment_add_f32) -> dst.
    src / dst: 2-D float32 row-strided views with unit column stride; seg_ptr [n_seg+1], idx, row [n_seg]: int32 (distinct rows).
    D columns (default: all of dst's; pad columns up to pad4(D) are written as 0).  No atomics: bit-identical from run to run.
    The owner's fold of the gradient rows returned by the reverse halo exchange (`dist_sage.PartitionedGraphSAGE`)."""
    D = int(dst.shape[1]) if D is None else int(D)
    n_seg = int(row.shape[0])
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.dim() == 2 and dst.dim() == 2
    assert all(t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() for t in (seg_ptr, idx, row))
    assert seg_ptr.shape[0] == n_seg + 1 and pad4(D) <= min(src.shape[1], dst.shape[1])
    rc = L.lib().bgnn_rows_segment_add_f32(L.ptr_rows(src), src.stride(0), int(src.shape[0]), L.ptr(seg_ptr), L.ptr(idx), L.ptr(row),
                                           n_seg, D, 1 if accumulate else 0, L.ptr_rows(dst), dst.stride(0), int(dst.shape[0]),
                                           L.stream())
    L.check(rc, "bgnn_rows_segment_add_f32")
    return dst


# ---- similarity-learner pair passes (bgnn.h: bgnn_pair_mlp_*, csrc/bgnn_pair_mlp.hip) -------------------------------------------
PAIR_MLP_WIDTH = 128          # u = Linear(2H, 128) output width of Similar_v2(mode='mlp'), models/models.py:918


def _pair_ws(P, dev):
    return torch.empty(int(L.lib().bgnn_pair_mlp_workspace_bytes(int(P))), dtype=torch.uint8, device=dev)


def pair_csr(idx_by, idx_other, n_by, n_other):
    """Pairs grouped by `idx_by` (the by-destination CSR build of bgnn_build_dst_csr over the edges idx_other -> idx_by, self
    loops kept, stable): -> (rowptr int32 [n_by+1], perm int32 [P] = pair ids, input order inside a node).  No host read."""
    lib = L.lib()
    P = int(idx_by.shape[0])
    N = max(int(n_by), int(n_other))
    if P + N >= 1 << 31:
        # rowptr / perm are int32 and the build takes P + N slots; the pair passes would otherwise clamp wrapped ids silently
        raise ValueError(f"pair list too large for int32 CSR offsets: P + N = {P + N} >= 2^31")
    dev = idx_by.device
    ei = torch.stack((idx_other, idx_by)).contiguous()
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    col = torch.empty(P + N, dtype=torch.int32, device=dev)
    perm = torch.empty(P + N, dtype=torch.int32, device=dev)
    e_out = torch.empty(1, dtype=torch.int64, device=dev)
    wsb = lib.bgnn_csr_workspace_bytes(N, P)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = lib.bgnn_build_dst_csr(L.ptr(ei), P, N, 0, L.ptr(rowptr), L.ptr(col), L.ptr(perm), L.ptr(e_out), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_build_dst_csr")
    return rowptr[:int(n_by) + 1], perm[:P]


def _pm_tables(A, B, idx1, idx2):
    assert A.dtype == torch.float32 and B.dtype == torch.float32 and A.shape[1] == PAIR_MLP_WIDTH == B.shape[1]
    assert idx1.dtype == torch.int64 and idx2.dtype == torch.int64 and idx1.shape == idx2.shape and idx1.dim() == 1
    assert idx1.is_contiguous() and idx2.is_contiguous()
    return (L.ptr_rows(A), A.stride(0), int(A.shape[0]), L.ptr_rows(B), B.stride(0), int(B.shape[0]), L.ptr(idx1), L.ptr(idx2),
            int(idx1.shape[0]))


def pair_mlp_stats(A, B, idx1, idx2, momentum=0.1, running_mean=None, running_var=None):
    """BN2's batch statistics of u_p = A[idx1[p]] + B[idx2[p]] -> fp64 [256] (mean, biased variance); updates the running
    buffers (fp32 [128]) in place like nn.BatchNorm1d in train mode."""
    P = int(idx1.shape[0])
    if P <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size [{P}, {PAIR_MLP_WIDTH}]")
    stats = torch.empty(2 * PAIR_MLP_WIDTH, dtype=torch.float64, device=A.device)
    ws = _pair_ws(P, A.device)
    rc = L.lib().bgnn_pair_mlp_stats_f32(*_pm_tables(A, B, idx1, idx2), float(momentum), L.ptr(running_mean), L.ptr(running_var),
                                         L.ptr(stats), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_pair_mlp_stats_f32")
    return stats


def pair_mlp_loss(A, B, idx1, idx2, y_u8, stats, gamma2, beta2, w2, b2, eps=1e-5):
    """-> (p [P], dl [P] = d mean-BCE / d logit, sums fp64 [392]) (bgnn.h: bgnn_pair_mlp_loss_f32 for the layout of sums)."""
    P = int(idx1.shape[0])
    assert y_u8.dtype == torch.uint8 and y_u8.shape == (P,)
    dev = A.device
    p = torch.empty(P, dtype=torch.float32, device=dev)
    dl = torch.empty(P, dtype=torch.float32, device=dev)
    sums = torch.empty(3 * PAIR_MLP_WIDTH + 8, dtype=torch.float64, device=dev)
    ws = _pair_ws(P, dev)
    t = _pm_tables(A, B, idx1, idx2)
    rc = L.lib().bgnn_pair_mlp_loss_f32(*t[:8], L.ptr(y_u8), t[8], L.ptr(stats), L.ptr(gamma2), L.ptr(beta2),
                                        L.ptr(w2), L.ptr(b2), float(eps), L.ptr(p), L.ptr(dl), L.ptr(sums), L.ptr(ws), ws.numel(),
                                        L.stream())
    L.check(rc, "bgnn_pair_mlp_loss_f32")
    return p, dl, sums


def pair_mlp_segsum(own, other, rowptr, perm, idx_other, dl, stats, sums, gamma2, beta2, w2, eps=1e-5, out=None):
    """S [n_own, 128]: per node of `own`, the sum of du_p over its pairs (rowptr / perm from `pair_csr`)."""
    n_own = int(rowptr.shape[0]) - 1
    assert n_own == own.shape[0] and own.shape[1] == PAIR_MLP_WIDTH == other.shape[1]
    assert rowptr.dtype == torch.int32 and perm.dtype == torch.int32 and idx_other.dtype == torch.int64
    if out is None:
        out = torch.empty(n_own, PAIR_MLP_WIDTH, dtype=torch.float32, device=own.device)
    rc = L.lib().bgnn_pair_mlp_segsum_f32(L.ptr_rows(own), own.stride(0), n_own, L.ptr_rows(other), other.stride(0), int(other.shape[0]),
                                          L.ptr(rowptr), L.ptr(perm), L.ptr(idx_other), int(idx_other.shape[0]), L.ptr(dl),
                                          L.ptr(stats), L.ptr(sums), L.ptr(gamma2), L.ptr(beta2), L.ptr(w2), float(eps),
                                          L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_pair_mlp_segsum_f32")
    return out


def pair_mlp_eval(A, B, idx1, idx2, scale2, shift2, w2, b2, y_u8=None):
    """Eval-mode scores p [P] (running statistics: BN2 as scale2 / shift2) and, with labels, fp64 counts [TP, FP, FN]."""
    P = int(idx1.shape[0])
    dev = A.device
    p = torch.empty(P, dtype=torch.float32, device=dev)
    counts = torch.empty(4, dtype=torch.float64, device=dev) if y_u8 is not None else None
    if P == 0:
        if counts is not None:
            counts.zero_()
        return p, counts
    ws = _pair_ws(P, dev)
    t = _pm_tables(A, B, idx1, idx2)
    rc = L.lib().bgnn_pair_mlp_eval_f32(*t[:8], L.ptr(y_u8), t[8], L.ptr(scale2), L.ptr(shift2), L.ptr(w2), L.ptr(b2),
                                        L.ptr(p), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_pair_mlp_eval_f32")
    return p, None if counts is None else counts[:3]


def pair_mlp_count(A, B, rows1, rows2, lab1, lab2, scale2, shift2, w2, b2):
    """int64 [4] = TP, FP, FN, TN of the eval-mode scorer (`pair_mlp_eval`'s sigmoid(logit) > 0.5 on u = A[rows1[i]] + B[rows2[j]])
    against lab1[rows1[i]] == lab2[rows2[j]] over the whole product rows1 x rows2 (eval_within_domain_v2 / eval_cross_domain_v2's
    eval_mode='all' lists, never materialised)."""
    assert A.dtype == torch.float32 and B.dtype == torch.float32 and A.dim() == 2 and B.dim() == 2
    assert A.shape[1] == PAIR_MLP_WIDTH == B.shape[1] and A.stride(1) == 1 and B.stride(1) == 1
    assert rows1.dtype == torch.int64 and rows2.dtype == torch.int64 and rows1.dim() == 1 and rows2.dim() == 1
    assert lab1.dtype == torch.int64 and lab2.dtype == torch.int64
    assert lab1.shape[0] == A.shape[0] and lab2.shape[0] == B.shape[0] and lab1.is_contiguous() and lab2.is_contiguous()
    for v in (scale2, shift2, w2):
        assert v.dtype == torch.float32 and v.shape == (PAIR_MLP_WIDTH,) and v.is_contiguous()
    assert b2.dtype == torch.float32 and b2.numel() == 1
    rows1, rows2 = rows1.contiguous(), rows2.contiguous()
    m1, m2 = int(rows1.shape[0]), int(rows2.shape[0])
    counts = torch.empty(4, dtype=torch.int64, device=A.device)
    ws = torch.empty(max(1, int(L.lib().bgnn_pair_mlp_count_workspace_bytes(m1, m2))), dtype=torch.uint8, device=A.device)
    rc = L.lib().bgnn_pair_mlp_count_f32(L.ptr_rows(A), A.stride(0), int(A.shape[0]), L.ptr_rows(B), B.stride(0), int(B.shape[0]),
                                         L.ptr(rows1), m1, L.ptr(rows2), m2, L.ptr(lab1), L.ptr(lab2), L.ptr(scale2), L.ptr(shift2),
                                         L.ptr(w2), L.ptr(b2), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_pair_mlp_count_f32")
    return counts


# ---- cosine similarity-learner pair passes (bgnn.h: bgnn_pair_cos_*, csrc/bgnn_pair_cos.hip) ------------------------------------
PAIR_COS_WIDTH = 128          # q = u + biasatt(u): biasatt is Linear(128, 64) -> Linear(64, 128), models/models.py:70-74


def _pc_table(T):
    assert T.dtype == torch.float32 and T.dim() == 2 and T.shape[1] == PAIR_COS_WIDTH and T.stride(1) == 1
    return L.ptr_rows(T), T.stride(0), int(T.shape[0])


def pair_cos_loss(A, B, idx1, idx2, y_u8):
    """Train-mode pair pass over normalised tables: -> (p [P], dl [P] = d mean-BCE / d cos, sums fp64 [4] = BCE sum, TP, FP, FN)."""
    P = int(idx1.shape[0])
    assert idx1.dtype == torch.int64 and idx2.dtype == torch.int64 and idx1.shape == idx2.shape and idx1.dim() == 1
    assert idx1.is_contiguous() and idx2.is_contiguous() and y_u8.dtype == torch.uint8 and y_u8.shape == (P,)
    if P < 1:
        raise ValueError("pair_cos_loss: empty pair list")
    dev = A.device
    p = torch.empty(P, dtype=torch.float32, device=dev)
    dl = torch.empty(P, dtype=torch.float32, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.lib().bgnn_pair_cos_loss_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    rc = L.lib().bgnn_pair_cos_loss_f32(*_pc_table(A), *_pc_table(B), L.ptr(idx1), L.ptr(idx2), L.ptr(y_u8), P, L.ptr(p), L.ptr(dl),
                                        L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_pair_cos_loss_f32")
    return p, dl, sums


def pair_cos_segsum(other, rowptr, perm, idx_other, dl, out=None):
    """G [n_own, 128]: per node, sum of dl[p] * other[idx_other[p]] over its pairs (rowptr / perm from `pair_csr`); atomic-free."""
    n_own = int(rowptr.shape[0]) - 1
    P = int(idx_other.shape[0])
    assert rowptr.dtype == torch.int32 and perm.dtype == torch.int32 and idx_other.dtype == torch.int64 and dl.dtype == torch.float32
    assert perm.shape[0] == P and dl.shape[0] == P and idx_other.is_contiguous() and dl.is_contiguous()
    if out is None:
        out = torch.empty(n_own, PAIR_COS_WIDTH, dtype=torch.float32, device=other.device)
    if n_own == 0:
        return out
    if P == 0:
        return out.zero_()
    rc = L.lib().bgnn_pair_cos_segsum_f32(*_pc_table(other), L.ptr(rowptr), L.ptr(perm), L.ptr(idx_other), P, L.ptr(dl), n_own,
                                          L.ptr_rows(out), out.stride(0), L.stream())
    L.check(rc, "bgnn_pair_cos_segsum_f32")
    return out


def pair_cos_count(A, B, rows1, rows2, lab1, lab2):
    """int64 [4] = TP, FP, FN, TN of (sigmoid(A[rows1[i]] . B[rows2[j]]) > 0.5) against lab1[rows1[i]] == lab2[rows2[j]] over the
    whole product rows1 x rows2 (eval_within_domain / eval_cross_domain's Cartesian lists, never materialised)."""
    assert rows1.dtype == torch.int64 and rows2.dtype == torch.int64 and rows1.dim() == 1 and rows2.dim() == 1
    assert lab1.dtype == torch.int64 and lab2.dtype == torch.int64
    assert lab1.shape[0] == A.shape[0] and lab2.shape[0] == B.shape[0] and lab1.is_contiguous() and lab2.is_contiguous()
    rows1, rows2 = rows1.contiguous(), rows2.contiguous()
    m1, m2 = int(rows1.shape[0]), int(rows2.shape[0])
    counts = torch.empty(4, dtype=torch.int64, device=A.device)
    ws = torch.empty(max(1, int(L.lib().bgnn_pair_cos_count_workspace_bytes(m1, m2))), dtype=torch.uint8, device=A.device)
    rc = L.lib().bgnn_pair_cos_count_f32(*_pc_table(A), *_pc_table(B), L.ptr(rows1), m1, L.ptr(rows2), m2, L.ptr(lab1), L.ptr(lab2),
                                         L.ptr(counts), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "bgnn_pair_cos_count_f32")
    return counts


# ---- step 2's loss and metric passes (bgnn.h: bgnn_step2_*, csrc/bgnn_step2.hip) -------------------------------------------------
STEP2_TERMS = ("total", "nll_s", "nll_t", "nll_t_hat", "kl", "n_train", "n_target")     # layout of the loss pass's fp64 [8] output


def _s2_table(T, N=None, C=None):
    assert T.dtype == torch.float32 and T.dim() == 2 and T.stride(1) == 1 and T.stride(0) >= T.shape[1], \
        "step-2 tables are fp32 [N, C] with unit column stride"
    assert (N is None or T.shape[0] == N) and (C is None or T.shape[1] == C), "step-2 tables must have one shape"
    return L.ptr_rows(T), T.stride(0)


def _s2_rows(y, *masks):
    N = int(y.shape[0])
    assert y.dtype == torch.int64 and y.dim() == 1 and y.is_contiguous()
    for m in masks:
        assert m.dtype == torch.uint8 and m.shape == (N,) and m.is_contiguous(), "step-2 masks are contiguous uint8 [N]"
    return N


def _s2_ws(N, C, dev):
    return torch.empty(int(L.lib().bgnn_step2_loss_workspace_bytes(N, C)), dtype=torch.uint8, device=dev)


def as_u8(mask):
    """bool / uint8 mask -> contiguous uint8 (a reinterpreting view for bool: no copy, no launch)"""
    return (mask.view(torch.uint8) if mask.dtype == torch.bool else mask).contiguous()


class _Step2LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp_s, lp_t, lp_h, y, train_u8, central_u8, Lambda):
        N = _s2_rows(y, train_u8, central_u8)
        C = int(lp_s.shape[1])
        if N < 1 or C < 1:
            raise ValueError("step2_loss: empty table")
        dev = lp_s.device
        terms = torch.empty(8, dtype=torch.float64, device=dev)
        ws = _s2_ws(N, C, dev)
        rc = L.lib().bgnn_step2_loss_f32(*_s2_table(lp_s, N, C), *_s2_table(lp_t, N, C), *_s2_table(lp_h, N, C), N, C, L.ptr(y),
                                         L.ptr(train_u8), L.ptr(central_u8), float(Lambda), L.ptr(terms), L.ptr(ws), ws.numel(),
                                         L.stream())
        L.check(rc, "bgnn_step2_loss_f32")
        ctx.save_for_backward(lp_t, lp_h, y, train_u8, central_u8, terms)
        ctx.Lambda = float(Lambda)
        ctx.mark_non_differentiable(terms)
        return terms[0].float(), terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        lp_t, lp_h, y, train_u8, central_u8, terms = ctx.saved_tensors
        N, C = lp_t.shape
        gs, gt, gh = (torch.empty(N, C, dtype=torch.float32, device=lp_t.device) for _ in range(3))
        g = g.reshape(1).float().contiguous()
        rc = L.lib().bgnn_step2_loss_bwd_f32(*_s2_table(lp_t), *_s2_table(lp_h), N, C, L.ptr(y), L.ptr(train_u8), L.ptr(central_u8),
                                             ctx.Lambda, L.ptr(terms), L.ptr(g), L.ptr(gs), L.ptr(gt), L.ptr(gh), C, L.stream())
        L.check(rc, "bgnn_step2_loss_bwd_f32")
        return gs, gt, gh, None, None, None, None


def step2_loss(lp_s, lp_t, lp_t_hat, y, train_mask, central_mask, Lambda=1.0, return_terms=False):
    """Step 2's training loss (main_graph_knowledge_transfer.py:44-54) in one HIP pass forward and one backward:
        (2 nll(lp_s | train) + nll(lp_t | train & ~central) + nll(lp_t_hat | train & ~central)) / 4 + Lambda KL_batchmean(lp_t_hat || lp_t)
    -> 0-dim fp32 loss (differentiable w.r.t. the three tables).  With `return_terms` also the pass's fp64 [8] vector, laid out as
    STEP2_TERMS (total, the three NLL means, the KL term without Lambda, the two row counts).  Masks: bool or uint8 [N].  No host
    synchronisation, no boolean indexing, fixed-order fp64 sums (two calls are bitwise equal), no memset node: usable as the
    `loss_fn` of `graphed_train_step`.  An empty selection gives NaN for its mean, like F.nll_loss."""
    loss, terms = _Step2LossFn.apply(lp_s, lp_t, lp_t_hat, y.contiguous(), as_u8(train_mask), as_u8(central_mask), Lambda)
    return (loss, terms) if return_terms else loss


class _Step2NllFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, y, mask_u8):
        N = _s2_rows(y, mask_u8)
        C = int(lp.shape[1])
        if N < 1 or C < 1:
            raise ValueError("step2_nll: empty table")
        terms = torch.empty(2, dtype=torch.float64, device=lp.device)
        ws = _s2_ws(N, C, lp.device)
        rc = L.lib().bgnn_step2_nll_f32(*_s2_table(lp, N, C), N, C, L.ptr(y), L.ptr(mask_u8), L.ptr(terms), L.ptr(ws), ws.numel(), L.stream())
        L.check(rc, "bgnn_step2_nll_f32")
        ctx.save_for_backward(y, mask_u8, terms)
        ctx.shape = (N, C)
        ctx.mark_non_differentiable(terms)
        return terms[0].float(), terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        y, mask_u8, terms = ctx.saved_tensors
        N, C = ctx.shape
        out = torch.empty(N, C, dtype=torch.float32, device=y.device)
        g = g.reshape(1).float().contiguous()
        rc = L.lib().bgnn_step2_nll_bwd_f32(N, C, L.ptr(y), L.ptr(mask_u8), L.ptr(terms), L.ptr(g), L.ptr(out), C, L.stream())
        L.check(rc, "bgnn_step2_nll_bwd_f32")
        return out, None, None


def step2_nll(lp, y, mask, return_terms=False):
    """F.nll_loss(lp[mask], y[mask]) (train_noDTC, main_graph_knowledge_transfer.py:269) without compacting rows -> 0-dim fp32 loss;
    `return_terms`: also fp64 [2] = (mean, row count)."""
    loss, terms = _Step2NllFn.apply(lp, y.contiguous(), as_u8(mask))
    return (loss, terms) if return_terms else loss


def step2_counts(tables, y, sel_u8, combos, out=None):
    """Confusion counts of per-row argmax predictions: tables = up to three [N, C] log-prob tables (None for unused slots), sel_u8
    uint8 [N] with bit b = row is in selection b, combos = [(table index, selection bit), ...] (at most 8)
    -> int64 [len(combos), C, C], counts[k, true, predicted].  Ties go to the lowest index."""
    tables = list(tables) + [None] * (3 - len(tables))
    first = next(t for t in tables if t is not None)
    N, C = int(first.shape[0]), int(first.shape[1])
    assert _s2_rows(y, sel_u8) == N and 1 <= len(combos) <= 8
    code = 0
    for k, (tb, bit) in enumerate(combos):
        assert 0 <= tb <= 2 and tables[tb] is not None and 0 <= bit <= 7
        code |= (tb | (bit << 2)) << (8 * k)
    if out is None:
        out = torch.empty(len(combos), C, C, dtype=torch.int64, device=first.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == len(combos) * C * C
    args = []
    for t in tables:
        args += list(_s2_table(t, N, C)) if t is not None else [None, 0]
    rc = L.lib().bgnn_step2_counts_f32(*args, N, C, L.ptr(y), L.ptr(sel_u8), code, len(combos), L.ptr(out), L.stream())
    L.check(rc, "bgnn_step2_counts_f32")
    return out


def step2_auc(score, y, sel):
    """roc_auc_score(y[sel], score[sel]) for binary labels as a 0-dim fp64 DEVICE tensor (NaN when one class is absent): the
    tie-aware rank statistic, a tied positive / negative pair counting 1/2.  The per-node arrays stay on the device: torch sorts the
    negatives' scores, one HIP pass counts, for every positive row, the negatives below it and level with it (integers)."""
    N = int(score.shape[0])
    assert score.dtype == torch.float32 and score.dim() == 1 and y.shape == (N,) and sel.shape == (N,)
    score = score.contiguous()
    sel = sel.bool()
    neg, pos = sel & (y == 0), sel & (y == 1)
    keys = torch.where(neg, score, torch.full_like(score, float("inf"))).sort().values
    n_neg = neg.sum().reshape(1)
    out = torch.empty(2, dtype=torch.int64, device=score.device)
    rc = L.lib().bgnn_step2_auc_count_f32(L.ptr(score), L.ptr(as_u8(pos)), N, L.ptr(keys), L.ptr(n_neg), L.ptr(out), L.stream())
    L.check(rc, "bgnn_step2_auc_count_f32")
    return out[0].double() / (2.0 * out[1].double() * n_neg[0].double())


# ---- step 1's edge-validity filters (csrc/bgnn_edge_filter.hip) --------------------------------------------------------------------
def quantile_f32(values, q):
    """`torch.quantile(values, q)` (linear interpolation) of a 1-D fp32 tensor as a 0-dim fp32 tensor, by radix selection instead of
    a sort: no 2^24 element limit (1 <= n <= 2^31 - 1), no host synchronisation, bitwise reproducible.  -0 and +0 are one value
    (returned as +0).  NaN input is out of contract (torch returns NaN; this returns the order statistic of the bit patterns)."""
    v = values.reshape(-1)
    if v.dtype != torch.float32:
        raise TypeError(f"quantile_f32 needs fp32 values (got {v.dtype})")
    v = v.contiguous()
    lib = L.lib()
    out = torch.empty((), dtype=torch.float32, device=v.device)
    wsb = lib.bgnn_quantile_workspace_bytes(v.shape[0])
    ws = torch.empty(wsb // 8, dtype=torch.int64, device=v.device)
    rc = lib.bgnn_quantile_f32(L.ptr(v), v.shape[0], float(q), L.ptr(out), L.ptr(ws), wsb, L.stream())
    L.check(rc, "bgnn_quantile_f32")
    return out


def row_inv_norms(x, eps=1e-8):
    """1 / max(||x_i||_2, eps) per row of a contiguous [N, F] fp32 table (the divisor of F.cosine_similarity), any F."""
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    rc = L.lib().bgnn_row_inv_norms_f32(L.ptr(x), x.shape[0], x.shape[1], float(eps), L.ptr(out), L.stream())
    L.check(rc, "bgnn_row_inv_norms_f32")
    return out


def edge_validity(edge_index, nodes_from, nodes_to, within, thres_conf_quantile, thres_feat_sim, e_sim=None, idx_mat=None,
                  e_sim_mat=None):
    """The five removal rules of main_bridged_graph.py:123-161 (within=True) / :225-264 (within=False) over an edge list [2, E]
    (int64; row 0 indexes `nodes_from`, row 1 `nodes_to`) without [E, F] or [E, k] temporaries.
      nodes_from = (x [N, F] fp32, inv_norm [N] fp32, pred [N] int32, y [N] int32), nodes_to = the same plus train_mask [N] uint8;
      similarity of an edge: `e_sim` [E] fp32 as given (the reference's top-k-ordered vector), or looked up in the top-k tables
      `idx_mat` / `e_sim_mat` [n_to, k] the list was made from (a miss raises).
    -> (flags [E] uint8: bit r-1 = removed by rule r (1 = similarity below its `thres_conf_quantile` quantile, 2 / 3 = a wrong
    prediction at `from` / `to`, 4 = predictions differ, 5 = raw-feature cosine < thres_feat_sim), counts: the five cumulative
    removal counts as Python ints (ONE device read), sim [E] fp32).  The list may be in any order; one sorted by row 0 (a coalesced
    list) is gathered faster because neighbouring edges share a feature row."""
    lib = L.lib()
    ei = edge_index.contiguous()
    if ei.dtype != torch.int64 or ei.dim() != 2 or ei.shape[0] != 2:
        raise TypeError("edge_index must be int64 [2, E]")
    E, dev = int(ei.shape[1]), ei.device
    xa, inva, preda, ya = nodes_from
    xb, invb, predb, yb, trainb = nodes_to
    F = int(xa.shape[1])
    if int(xb.shape[1]) != F:
        raise ValueError(f"feature widths differ ({F} vs {int(xb.shape[1])})")
    flags = torch.empty(E, dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    aligned = idx_mat is not None
    if aligned:
        idx_mat, e_sim_mat = idx_mat.contiguous(), e_sim_mat.contiguous()
        if idx_mat.dtype != torch.int64 or e_sim_mat.dtype != torch.float32 or idx_mat.shape != e_sim_mat.shape or idx_mat.shape[0] != xb.shape[0]:
            raise ValueError("idx_mat (int64) / e_sim_mat (fp32) must both be [n_to, k]")
        sim = torch.empty(E, dtype=torch.float32, device=dev)
    else:
        sim = e_sim.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        if sim.shape[0] != E:
            raise ValueError(f"e_sim has {sim.shape[0]} entries for {E} edges")
    rc = lib.bgnn_edge_validity_f32(L.ptr(ei), E, L.ptr(xa), xa.shape[0], L.ptr(inva), L.ptr(preda), L.ptr(ya), L.ptr(xb), xb.shape[0],
                                    L.ptr(invb), L.ptr(predb), L.ptr(yb), L.ptr(trainb), F, 1 if within else 0, float(thres_feat_sim),
                                    L.ptr(idx_mat) if aligned else None, L.ptr(e_sim_mat) if aligned else None,
                                    int(idx_mat.shape[1]) if aligned else 0, L.ptr(sim) if aligned else None, L.ptr(flags),
                                    L.ptr(counts), L.stream())
    L.check(rc, "bgnn_edge_validity_f32")
    if E > 0:
        thres = quantile_f32(sim, thres_conf_quantile)
        rc = lib.bgnn_edge_rule1_counts_f32(L.ptr(sim), L.ptr(thres), E, L.ptr(flags), L.ptr(counts), L.stream())
        L.check(rc, "bgnn_edge_rule1_counts_f32")
    c = counts.tolist()
    if c[6]:
        raise RuntimeError(f"edge_validity: {c[6]} edges name a node outside the tables")
    if c[5]:
        raise RuntimeError(f"edge_validity: {c[5]} edges do not come from these top-k tables")
    return flags, c[:5], sim
