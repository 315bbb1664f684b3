// GraphSAGE mean aggregation for gfx950 (wave64): forward and atomic-free backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:440-498): torch_sparse `matmul(adj_t, x, reduce='mean')` inside each
// SAGEConv plus the F.relu / F.dropout between convs and the closing F.log_softmax.  The host transforms first
// (T = x [W_l ; W_r]^T + [0 ; b_l], one GEMM per layer: W_l is linear, so mean_j(W_l x_j) = W_l mean_j(x_j)) and this file
// averages rows of the OUTPUT width:
//   forward : out_i = epi( s_i * sum_{t in row i} T_l[col[t]] + T_r[i] ),   s_i = 1/deg_i (mean) or 1 (plain sum)
//   backward: pass A (per destination) g_i from (y_i, dy_i), dT_r[i] = g_i, scratch S[i] = g_i / deg_i;
//             pass B (per source)      dT_l[j] = sum over the out-edges of j of S[dst]  (the forward kernel, plain sum, over the
//             by-source view) -- two launches, no float atomics, bit-identical from run to run.
// There is no attention math: the forward is gather-bound.  Algorithmic bytes at width D: E'(4D + 4) + N(8D + 4).
//
// Mapping, dropout hash, epilogue pieces, backward row kernel and launch helpers: bgnn_conv_common.h.  A launch
// covers at most 128 columns; wider rows run as column slices (one launch per slice).
//
// Two compile-time variants of the same kernel serve a destination-node partition (dist_sage.py): ROW_ID keys the dropout hash
// on a caller-given GLOBAL row id per output row (a rank's rows then draw the masks of the whole-graph call), and OUT_ROW
// writes output row s to dst[row[s]] (optionally adding what is there): bgnn_rows_segment_add_f32, which folds the gradient
// rows returned by the reverse halo exchange into their owners' rows.  The plain entry point instantiates neither.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;
constexpr int EPI_RELU = EPI_ACT;   // code 1 here: ReLU, then dropout

struct SageParams {
  const float* tbl; int64_t ldt; int64_t n_tbl;    // neighbour table (column-offset to the slice), its stride and row count
  const float* root; int64_t ldr;                  // optional per-row addend (column-offset to the slice)
  const int32_t* rowptr; const int32_t* col;
  int64_t n_rows;
  int32_t D;                                       // columns of this slice (<= SLICE)
  int mean;
  float* out; int64_t ldo;                         // column-offset to the slice
  // dropout after the ReLU: element index = row * d_full + c0 + column (the hash of bgnn_norm.hip)
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  int32_t d_full; int32_t c0;
  const int64_t* row_id;                           // ROW_ID: dropout row of output row i (element index row_id[i] * d_full + col)
  const int32_t* out_row; int64_t n_out;          // OUT_ROW: output row i lands in (and its root is read from) row out_row[i]
};

template <int LF, int EP, int U, int EPI, bool ROW_ID = false, bool OUT_ROW = false>
__global__ __launch_bounds__(256) void sage_agg_kernel(SageParams p) {
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
    const bool rvalid = i < p.n_rows;
    const int32_t beg = rvalid ? p.rowptr[i] : 0;
    const int32_t end = rvalid ? p.rowptr[i + 1] : 0;
    const int32_t deg = end - beg;
    const int32_t niter = (deg + EP * U - 1) / (EP * U);       // uniform inside the group

    float4 acc = f4_zero();
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.col[e] : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // ids outside the table are never dereferenced (a malformed CSR gives a wrong sum, not a stray read)
        const bool ok = nid[u] >= 0 && (int64_t)nid[u] < p.n_tbl && fvalid;
        v[u] = ok ? *reinterpret_cast<const float4*>(p.tbl + (int64_t)nid[u] * p.ldt + f0) : f4_zero();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.col[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
      }
    }
    acc = ep_sum<LF, GL>(acc);
    const float s = (p.mean && deg > 0) ? 1.f / (float)deg : 1.f;
    float o[4] = {acc.x * s, acc.y * s, acc.z * s, acc.w * s};
    const int64_t io = OUT_ROW ? (rvalid ? (int64_t)p.out_row[i] : 0) : i;   // the row written (and whose root is added)
    const bool ovalid = OUT_ROW ? (rvalid && io >= 0 && io < p.n_out) : rvalid;  // a row id out of range is never touched
    if (p.root != nullptr && ovalid && fvalid) {
      const float4 r = *reinterpret_cast<const float4*>(p.root + io * p.ldr + f0);
      o[0] += r.x; o[1] += r.y; o[2] += r.z; o[3] += r.w;
    }
    if (EPI == EPI_RELU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
      if (p.thr != 0u) {
        const int64_t ih = ROW_ID ? (rvalid ? p.row_id[i] : 0) : (rvalid ? i : 0);
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

template <int LF, int EP, int U, int EPI, bool ROW_ID, bool OUT_ROW>
int launch_agg(const SageParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const int grid = persistent_grid(sage_agg_kernel<LF, EP, U, EPI, ROW_ID, OUT_ROW>, ntiles, &cap);
  hipLaunchKernelGGL((sage_agg_kernel<LF, EP, U, EPI, ROW_ID, OUT_ROW>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int EPI, bool ROW_ID = false, bool OUT_ROW = false>
int dispatch_agg(const SageParams& p, hipStream_t st) {
  return lf_ladder((p.D + 3) / 4,   // float4 slots of the slice
                   [&](auto LF, auto EP, auto U) { return launch_agg<LF, EP, U, EPI, ROW_ID, OUT_ROW>(p, st); });
}

}  // namespace

extern "C" int bgnn_sage_mean_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* root_opt, int64_t ldr,
                                            const int32_t* rowptr, const int32_t* col, int64_t n_rows, int32_t D, int mean,
                                            int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                            const int64_t* row_id_opt, float* out, int64_t ldo, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tbl || !rowptr || !col || !out) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < 0 || D <= 0) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if (!ld_ok(ldt, D) || !ld_ok(ldo, D) || (root_opt && !(ldr == 0 || ld_ok(ldr, D)))) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(tbl) || !bgnn_aligned16(out) || (root_opt && !bgnn_aligned16(root_opt))) return BGNN_E_ALIGN;
  if (n_rows == 0) return 0;
  for (int32_t c0 = 0; c0 < D; c0 += SLICE) {
    SageParams p{};
    p.tbl = tbl + c0; p.ldt = ldt; p.n_tbl = n_tbl;
    p.root = root_opt ? root_opt + c0 : nullptr; p.ldr = ldr;
    p.rowptr = rowptr; p.col = col; p.n_rows = n_rows;
    p.D = D - c0 < SLICE ? D - c0 : SLICE;
    p.mean = mean;
    p.out = out + c0; p.ldo = ldo;
    drop_consts(p_drop, p.thr, p.keep_scale);
    p.seed = seed; p.seed_dev = seed_dev_opt; p.d_full = D; p.c0 = c0;
    p.row_id = row_id_opt;
    // the row id only feeds the dropout hash: without dropout (or without ids) the plain kernel runs
    int rc = epilogue == EPI_RELU ? (row_id_opt != nullptr && p.thr != 0u ? dispatch_agg<EPI_RELU, true>(p, st) : dispatch_agg<EPI_RELU>(p, st))
           : epilogue == EPI_LOGSOFTMAX ? dispatch_agg<EPI_LOGSOFTMAX>(p, st) : dispatch_agg<EPI_NONE>(p, st);
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" int bgnn_rows_segment_add_f32(const float* src, int64_t lds, int64_t n_src, const int32_t* seg_ptr,
                                         const int32_t* idx, const int32_t* row, int64_t n_seg, int32_t D, int accumulate,
                                         float* dst, int64_t ldd, int64_t n_dst, void* stream) {
  if (!src || !seg_ptr || !idx || !row || !dst) return BGNN_E_NULL;
  if (n_seg < 0 || n_src < 0 || n_dst < 0 || D <= 0) return BGNN_E_SHAPE;
  if (!ld_ok(lds, D) || !ld_ok(ldd, D)) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(src) || !bgnn_aligned16(dst)) return BGNN_E_ALIGN;
  if (n_seg == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  for (int32_t c0 = 0; c0 < D; c0 += SLICE) {
    SageParams p{};
    p.tbl = src + c0; p.ldt = lds; p.n_tbl = n_src;
    p.root = accumulate ? dst + c0 : nullptr; p.ldr = ldd;      // dst[row[s]] + sum: the root half is the destination row itself
    p.rowptr = seg_ptr; p.col = idx; p.n_rows = n_seg;
    p.D = D - c0 < SLICE ? D - c0 : SLICE;
    p.mean = 0;
    p.out = dst + c0; p.ldo = ldd;
    p.keep_scale = 1.f; p.d_full = D; p.c0 = c0;
    p.out_row = row; p.n_out = n_dst;
    const int rc = dispatch_agg<EPI_NONE, false, true>(p, st);
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" size_t bgnn_sage_mean_aggregate_bwd_workspace_bytes(int64_t n_rows, int32_t D) {
  if (n_rows < 0 || D <= 0) return 0;
  return (size_t)n_rows * (size_t)(((int64_t)D + 3) / 4 * 4) * sizeof(float) + 16;
}

extern "C" int bgnn_sage_mean_aggregate_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy,
                                                const int32_t* rowptr, int64_t n_rows, const int32_t* t_rowptr, const int32_t* t_col,
                                                int64_t n_src, int32_t D, int epilogue, float p_drop,
                                                float* grad_tbl, int64_t ldgt, float* grad_root, int64_t ldgr,
                                                void* ws, size_t ws_bytes, void* stream) {
  if (!grad_y || !rowptr || !t_rowptr || !t_col || !grad_tbl || !grad_root || !ws) return BGNN_E_NULL;
  if (epilogue != EPI_NONE && !y) return BGNN_E_NULL;
  if (n_rows < 0 || n_src < 0 || D <= 0) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if (ws_bytes < bgnn_sage_mean_aggregate_bwd_workspace_bytes(n_rows, D)) return BGNN_E_WORKSPACE;
  if ((y && !ld_ok(ldy, D)) || !ld_ok(ldgy, D) || !ld_ok(ldgt, D) || !ld_ok(ldgr, D)) return BGNN_E_ALIGN;
  if ((y && !bgnn_aligned16(y)) || !bgnn_aligned16(grad_y) || !bgnn_aligned16(grad_tbl) || !bgnn_aligned16(grad_root))
    return BGNN_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int64_t lds = ((int64_t)D + 3) / 4 * 4;
  float* s = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws), 16));
  if (n_rows > 0) {
    BwdRowsParams p{};
    p.y = y; p.ldy = ldy; p.gy = grad_y; p.ldgy = ldgy; p.rowptr = rowptr; p.n_rows = n_rows; p.D = D;
    uint32_t thr;
    drop_consts(p_drop, thr, p.keep_scale);
    p.g = grad_root; p.ldg = ldgr; p.s = s; p.lds = lds;
    const int rc = dispatch_bwd_rows<true>(epilogue, p, st);   // pass A: dT_r = g, S = g / deg
    if (rc != 0) return rc;
  }
  // pass B: plain sum of the scratch rows over the by-source view (every id in t_col is a destination row < n_rows)
  return bgnn_sage_mean_aggregate_f32(s, lds, n_rows, nullptr, 0, t_rowptr, t_col, n_src, D, 0, EPI_NONE, 0.f, 0, nullptr, nullptr,
                                      grad_tbl, ldgt, stream);
}
