// GCN normalised aggregation for gfx950 (wave64): forward and atomic-free backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:246-300): PyG GCNConv's gcn_norm(add_self_loops=True, improved=False) with
// unit edge weights + propagate(aggr='add') + bias, and the F.relu / F.dropout between convs and the closing F.log_softmax.
// The host transforms first (tbl = x W^T, as GCNConv itself does) and this file walks a by-destination CSR that already holds
// exactly one self loop per row (bgnn_build_dst_csr with rewrite_self_loops):
//   forward : out_i = epi( dinv_i * sum_{t in row i} dinv[col[t]] * tbl[col[t]] + bias ),  dinv_i = 1/sqrt(deg_i)
//   backward: a row pass forms g_i from (y_i, dy_i) (the three rules of bgnn_sage.hip); grad_bias = column sums of g (host:
//             the fixed-order fp64 column-sum kernel); grad_tbl[j] = dinv_j * sum_{i : j -> i} dinv_i * g_i, which is the
//             forward walk (no epilogue, no bias) over the by-source view of the same edges.  No float atomics anywhere.
// dinv[col[t]] is gathered in the edge loop (4 B per edge next to the 4*D B row).  Bytes at width D: E'(4D + 8) + N(8D + 4).
//
// Mapping, dropout hash, epilogue pieces, backward row kernel and launch helpers: bgnn_conv_common.h.  At most 128 columns per
// launch, wider rows run as slices.
//
// Hub rows (a source node of a bridged graph after ToUndirected has thousands of in-edges): with hub tables the row kernel
// skips every row of at least `hub_threshold` edges; the same kernel then runs twice more -- SEGMENT mode sums each segment
// (an explicit (begin, end) pair of edge offsets) into a partial row of the workspace, FINISH mode adds a hub's partial rows
// in segment order, scales by dinv_i, adds the bias and applies the epilogue.  One group per segment: a hub is spread over
// the whole grid, its bits do not depend on which block took which segment.
//
// Rows of a larger graph (row_id_opt of bgnn_gcn_aggregate_f32, a rank's rows of a node partition): ROW_ID kernels draw the
// dropout mask of output row io for row_id[io], its GLOBAL row, in the row kernel and in a hub's FINISH group alike; the id is
// loaded once per row after the gather loop.  Without ids (or without dropout) the kernels launched are the ones without the
// template flag.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;
constexpr int EPI_RELU = EPI_ACT;   // code 1 here: ReLU, then dropout
enum { MODE_ROWS = 0, MODE_SEGMENT = 1, MODE_FINISH = 2 };

struct GcnParams {
  const float* tbl; int64_t ldt; int64_t n_tbl;    // neighbour table (column-offset to the slice); FINISH: the partial rows
  const float* bias;                               // one row (column-offset to the slice) or NULL
  const int32_t* rowptr; const int32_t* col;       // ROWS: the CSR; SEGMENT: rowptr = (begin, end) pairs; FINISH: rowptr = hub_seg_ptr
  const float* dinv; int64_t n_dinv;
  int64_t n_rows;                                  // rows / segments / hubs of this launch
  int32_t D;                                       // columns of this slice (<= SLICE)
  int32_t hub_threshold;                           // ROWS: rows of at least this many edges are left to the hub launches (0: none)
  const int32_t* hub_rows; int64_t n_out;          // FINISH: output row of hub h, rows of out
  float* out; int64_t ldo;
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  int32_t d_full; int32_t c0;
  const int64_t* row_id;                           // ROW_ID: dropout row of output row io (element index row_id[io] * d_full + col)
};

template <int LF, int EP, int U, int EPI, int MODE, bool ROW_ID = false>
__global__ __launch_bounds__(256) void gcn_agg_kernel(GcnParams p) {
  constexpr int GL = LF * EP;            // lanes per output row
  constexpr int GPW = 64 / GL;           // rows per wave
  constexpr int RPB = 4 * GPW;           // rows per block iteration (4 waves)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int f0 = (lg % LF) * 4;
  const bool fvalid = f0 < p.D;
  uint64_t seed = p.seed;
  if (EPI == EPI_RELU && p.seed_dev != nullptr) seed += *p.seed_dev;

  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                                       // block-uniform
    const int64_t i = gt * RPB + wave * GPW + g;
    bool rvalid = i < p.n_rows;
    int32_t beg = 0, end = 0;
    if (rvalid) {
      if (MODE == MODE_SEGMENT) { beg = p.rowptr[2 * i]; end = p.rowptr[2 * i + 1]; }
      else { beg = p.rowptr[i]; end = p.rowptr[i + 1]; }
    }
    if (MODE == MODE_ROWS && p.hub_threshold > 0 && end - beg >= p.hub_threshold) {   // the hub launches own this row
      rvalid = false; beg = end = 0;
    }
    const int32_t deg = end - beg;
    const int32_t niter = (deg + EP * U - 1) / (EP * U);       // uniform inside the group

    float4 acc = f4_zero();
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? (MODE == MODE_FINISH ? e : p.col[e]) : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float4 v[U];
      float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // ids outside the table are never dereferenced (a malformed CSR gives a wrong sum, not a stray read)
        const bool ok = nid[u] >= 0 && (int64_t)nid[u] < p.n_tbl && fvalid;
        v[u] = ok ? *reinterpret_cast<const float4*>(p.tbl + (int64_t)nid[u] * p.ldt + f0) : f4_zero();
        if (MODE == MODE_FINISH) w[u] = 1.f;
        else w[u] = (ok && (int64_t)nid[u] < p.n_dinv) ? p.dinv[nid[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? (MODE == MODE_FINISH ? e : p.col[e]) : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc.x += w[u] * v[u].x; acc.y += w[u] * v[u].y; acc.z += w[u] * v[u].z; acc.w += w[u] * v[u].w;
      }
    }
    acc = ep_sum<LF, GL>(acc);
    // the row written: the segment's partial row, the hub's own row, or row i
    int64_t io = i;
    if (MODE == MODE_FINISH) io = rvalid ? (int64_t)p.hub_rows[i] : 0;
    const bool ovalid = MODE == MODE_FINISH ? (rvalid && io >= 0 && io < p.n_out) : rvalid;
    float o[4] = {acc.x, acc.y, acc.z, acc.w};
    if (MODE != MODE_SEGMENT) {
      const float s = (ovalid && io < p.n_dinv) ? p.dinv[io] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] *= s;
      if (p.bias != nullptr && fvalid) {
        const float4 b = *reinterpret_cast<const float4*>(p.bias + f0);
        o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w;
      }
    }
    if (EPI == EPI_RELU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
      if (p.thr != 0u) {
        // the row the mask is drawn for: one 8-byte load per group after the gather loop (a hub's finish group reads its hub's)
        const int64_t ih = ovalid ? (ROW_ID ? p.row_id[io] : io) : 0;
        const uint64_t e = (uint64_t)ih * (uint64_t)p.d_full + (uint64_t)(p.c0 + f0);
        drop4(o, e, (p.d_full & 3) == 0, seed, p.thr, p.keep_scale);
      }
    } else if (EPI == EPI_LOGSOFTMAX) {
      log_softmax4<LF>(o, f0, p.D);
    }
    if (ovalid && sub == 0 && fvalid) {
#pragma unroll
      for (int c = 0; c < 4; ++c) if (f0 + c >= p.D) o[c] = 0.f;   // pad columns of the row leave as 0
      *reinterpret_cast<float4*>(p.out + io * p.ldo + f0) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int LF, int EP, int U, int EPI, int MODE, bool ROW_ID>
int launch_agg(const GcnParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const int grid = persistent_grid(gcn_agg_kernel<LF, EP, U, EPI, MODE, ROW_ID>, ntiles, &cap);
  hipLaunchKernelGGL((gcn_agg_kernel<LF, EP, U, EPI, MODE, ROW_ID>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int EPI, int MODE, bool ROW_ID = false>
int dispatch_agg(const GcnParams& p, hipStream_t st) {
  return lf_ladder((p.D + 3) / 4,   // float4 slots of the slice
                   [&](auto LF, auto EP, auto U) { return launch_agg<LF, EP, U, EPI, MODE, ROW_ID>(p, st); });
}

template <int MODE>
int dispatch_epi(int epilogue, const GcnParams& p, hipStream_t st) {
  // the row-id variant exists only where a mask is drawn; every other call runs the kernels it always ran
  if (epilogue == EPI_RELU && p.row_id != nullptr && p.thr != 0u) return dispatch_agg<EPI_RELU, MODE, true>(p, st);
  return epi_switch(epilogue, [&](auto EPI) { return dispatch_agg<EPI, MODE>(p, st); });
}

int64_t part_ld(int32_t D) { return D < SLICE ? ((int64_t)D + 3) / 4 * 4 : SLICE; }

}  // namespace

extern "C" size_t bgnn_gcn_aggregate_workspace_bytes(int64_t n_seg, int32_t D) {
  if (n_seg <= 0 || D <= 0) return 0;
  return (size_t)n_seg * (size_t)part_ld(D) * sizeof(float) + 16;
}

extern "C" int bgnn_gcn_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* bias_opt, const int32_t* rowptr,
                                      const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows, int32_t D,
                                      int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                      int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                                      const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                      void* ws_opt, size_t ws_bytes, const int64_t* row_id_opt, float* out, int64_t ldo,
                                      void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tbl || !rowptr || !col || !dinv || !out) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < 0 || D <= 0 || n_dinv < n_rows || n_dinv < n_tbl) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if (!ld_ok(ldt, D) || !ld_ok(ldo, D)) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(tbl) || !bgnn_aligned16(out) || (bias_opt && !bgnn_aligned16(bias_opt))) return BGNN_E_ALIGN;
  const bool hubs = n_hubs > 0;
  if (n_hubs < 0 || n_seg < 0) return BGNN_E_SHAPE;
  float* part = nullptr;
  if (hubs) {
    if (hub_threshold < 1 || n_seg < n_hubs) return BGNN_E_SHAPE;
    if (!hub_rows_opt || !hub_seg_ptr_opt || !seg_bounds_opt || !ws_opt) return BGNN_E_NULL;
    if (ws_bytes < (size_t)n_seg * (size_t)part_ld(D) * sizeof(float) + 16) return BGNN_E_WORKSPACE;
    part = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws_opt), 16));
  }
  if (n_rows == 0) return 0;
  for (int32_t c0 = 0; c0 < D; c0 += SLICE) {
    GcnParams p{};
    p.tbl = tbl + c0; p.ldt = ldt; p.n_tbl = n_tbl;
    p.bias = bias_opt ? bias_opt + c0 : nullptr;
    p.rowptr = rowptr; p.col = col; p.dinv = dinv; p.n_dinv = n_dinv; p.n_rows = n_rows;
    p.D = D - c0 < SLICE ? D - c0 : SLICE;
    p.hub_threshold = hubs ? hub_threshold : 0;
    p.n_out = n_rows;
    p.out = out + c0; p.ldo = ldo;
    drop_consts(p_drop, p.thr, p.keep_scale);
    p.seed = seed; p.seed_dev = seed_dev_opt; p.d_full = D; p.c0 = c0;
    p.row_id = row_id_opt;                   // [n_rows]: the row kernel reads row_id[i], a hub's finish group row_id[hub_rows[h]]
    int rc = dispatch_epi<MODE_ROWS>(epilogue, p, st);
    if (rc != 0) return rc;
    if (hubs) {
      GcnParams s = p;                       // partial rows of the segments (the slice's columns, densely packed)
      s.bias = nullptr; s.rowptr = seg_bounds_opt; s.n_rows = n_seg; s.hub_threshold = 0;
      s.out = part; s.ldo = part_ld(D); s.thr = 0u;
      rc = dispatch_agg<EPI_NONE, MODE_SEGMENT>(s, st);
      if (rc != 0) return rc;
      GcnParams f = p;                       // a hub's partial rows in segment order, then the row's scale, bias and epilogue
      f.tbl = part; f.ldt = part_ld(D); f.n_tbl = n_seg;
      f.rowptr = hub_seg_ptr_opt; f.col = nullptr; f.n_rows = n_hubs; f.hub_threshold = 0; f.hub_rows = hub_rows_opt;
      rc = dispatch_epi<MODE_FINISH>(epilogue, f, st);
      if (rc != 0) return rc;
    }
  }
  return 0;
}

extern "C" int bgnn_gcn_aggregate_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, int64_t n_rows,
                                          const int32_t* t_rowptr, const int32_t* t_col, const float* dinv, int64_t n_dinv,
                                          int64_t n_src, int32_t D, int epilogue, float p_drop,
                                          int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                                          const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                          void* ws_opt, size_t ws_bytes, float* g, int64_t ldg, float* grad_tbl, int64_t ldgt,
                                          void* stream) {
  if (!grad_y || !t_rowptr || !t_col || !dinv || !g || !grad_tbl) return BGNN_E_NULL;
  if (epilogue == EPI_RELU && !y) return BGNN_E_NULL;
  if (epilogue == EPI_LOGSOFTMAX && !y) return BGNN_E_NULL;
  if (n_rows < 0 || n_src < 0 || D <= 0) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if ((y && !ld_ok(ldy, D)) || !ld_ok(ldgy, D) || !ld_ok(ldg, D) || !ld_ok(ldgt, D)) return BGNN_E_ALIGN;
  if ((y && !bgnn_aligned16(y)) || !bgnn_aligned16(grad_y) || !bgnn_aligned16(g) || !bgnn_aligned16(grad_tbl)) return BGNN_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (n_rows > 0) {
    BwdRowsParams p{};
    p.y = y; p.ldy = ldy; p.gy = grad_y; p.ldgy = ldgy; p.n_rows = n_rows; p.D = D;
    uint32_t thr;
    drop_consts(p_drop, thr, p.keep_scale);
    p.g = g; p.ldg = ldg;
    const int rc = dispatch_bwd_rows<false>(epilogue, p, st);
    if (rc != 0) return rc;
  }
  // the forward walk over the by-source view (every id in t_col is a destination row < n_rows)
  return bgnn_gcn_aggregate_f32(g, ldg, n_rows, nullptr, t_rowptr, t_col, dinv, n_dinv, n_src, D, EPI_NONE, 0.f, 0, nullptr,
                                hub_threshold, hub_rows_opt, n_hubs, hub_seg_ptr_opt, seg_bounds_opt, n_seg, ws_opt, ws_bytes,
                                nullptr, grad_tbl, ldgt, stream);
}
