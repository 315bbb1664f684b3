// GIN sum aggregation for gfx950 (wave64): forward and atomic-free backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:26-57): the propagate(aggr='add') and the (1 + eps) * x_i self term of PyG's
// GINConv(Linear(in, out), train_eps=True), the bias of its Linear, and the F.relu / F.dropout between convs and the closing
// F.log_softmax.  `nn` is one affine map, so the host transforms first (T = x W^T, one GEMM per layer at the output width) and
// this file walks the by-destination CSR exactly as given (duplicates are separate messages, self loops ordinary edges, none
// added):
//   forward : out_i = epi( (1 + eps) * T_i + sum_{t in row i} T[col[t]] + b )
//   backward: pass A (per destination) g_i from (y_i, dy_i) by conv_bwd_rows_kernel; with grad_eps wanted a second row pass
//             forms <g_i, T_i> in fp64, one partial per block, and a one-block launch sums the partials in a fixed order;
//             pass B (per source) dT_j = (1 + eps) * g_j + sum_{i : j -> i} g_i -- the forward kernel over the by-source view
//             with the same eps pointer, no bias, no epilogue.  No float atomics, bit-identical from run to run.
// eps is read from device memory by every kernel that needs it: the host never waits for it.  The row's own table row is its
// root: no [N, D] root buffer exists.  The walk is gather-bound; algorithmic bytes at width D: E(4D + 4) + N(12D + 4) a pass
// (forward: gather, own row, out; pass B likewise), pass A N * 12D (+ N * 8D for grad_eps).
//
// Mapping, dropout hash, epilogue pieces, backward row kernel and launch helpers: bgnn_conv_common.h (the mapping and the
// in-flight depth of sage_agg_kernel).  A launch covers at most 128 columns; wider rows run as column slices.
//
// Hub rows (a source node of a bridged graph after ToUndirected has thousands of in-edges): without hub tables a hub row walks
// as one lane group.  With them (bgnn_gin_aggregate_hub_f32, the scheme of bgnn_gcn.hip) the row kernel leaves every row of at
// least `hub_threshold` edges alone and the same kernel runs twice more: SEGMENT mode sums each segment (an explicit (begin,
// end) pair of edge offsets) into a partial row of the workspace with the row walk's batches and compensated add -- no own row,
// no bias, no epilogue; FINISH mode adds a hub's partial rows in segment order through the same compensated add, joins the
// hub's own row of the REAL table by the same fma, then bias and epilogue, the dropout mask drawn for the hub's (global) row.
// One group per segment: a hub is spread over the whole grid and its bits do not depend on which block took which segment.
// A hub of ONE segment carries the bits of the unsegmented walk (one partial, added to 0).  The launches without hub tables
// are the instantiations with HUBS = false, MODE_ROWS: the kernels of the entry without hubs.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;
constexpr int EPI_RELU = EPI_ACT;      // code 1 here: ReLU, then dropout
constexpr int GIN_MAX_BLOCKS = 2048;   // partial slots of the grad_eps row pass (the grid cap of launch_bwd_rows)
enum { MODE_ROWS = 0, MODE_SEGMENT = 1, MODE_FINISH = 2 };

struct GinParams {
  const float* tbl; int64_t ldt; int64_t n_tbl;    // table (column-offset to the slice), its stride and row count
  const float* eps;                                // device scalar or NULL (weight 1 on the own row)
  const float* bias;                               // one row (column-offset to the slice) or NULL
  const int32_t* rowptr; const int32_t* col; int64_t n_edges;
  int64_t n_rows;
  int32_t D;                                       // columns of this slice (<= SLICE)
  float* out; int64_t ldo;                         // column-offset to the slice
  // dropout after the ReLU: element index = row * d_full + c0 + column (the hash of bgnn_norm.hip)
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  int32_t d_full; int32_t c0;
  const int64_t* row_id;                           // ROW_ID: dropout row of output row i
  // hub launches.  ROWS (HUBS): rows of at least hub_threshold edges are left to them.  SEGMENT: rowptr = (begin, end) pairs,
  // n_rows segments, out = the partial rows.  FINISH: tbl = the partial rows (n_tbl = n_seg of them, n_edges = n_seg), rowptr =
  // hub_seg_ptr, n_rows hubs, hub_rows[h] the output row of hub h among n_out, own = the real table (n_own rows)
  int32_t hub_threshold;
  const int32_t* hub_rows; int64_t n_out;
  const float* own; int64_t ldown; int64_t n_own;
};

template <int LF, int EP, int U, int EPI, bool ROW_ID = false, int MODE = MODE_ROWS, bool HUBS = false>
__global__ __launch_bounds__(256) void gin_agg_kernel(GinParams p) {
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
  const float self_w = (MODE != MODE_SEGMENT && p.eps != nullptr) ? 1.f + *p.eps : 1.f;

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
    if (MODE == MODE_ROWS && HUBS && end - beg >= p.hub_threshold) {   // the hub launches own this row: no gather, no store
      rvalid = false; beg = end = 0;
    }
    clamp_row(beg, end, p.n_edges);
    // the row written: row i, the segment's partial row, or the hub's row (one outside the output is dropped)
    int64_t io = i;
    if (MODE == MODE_FINISH) {
      io = rvalid ? (int64_t)p.hub_rows[i] : 0;
      if (io < 0 || io >= p.n_out) { rvalid = false; io = 0; beg = end = 0; }
    }
    const int32_t niter = (end - beg + EP * U - 1) / (EP * U);  // uniform inside the group

    // the row's own table row: requested in front of the gathers (a row past the table, pass B of a rectangular graph, has none)
    float4 own = f4_zero();
    if (MODE == MODE_ROWS) {
      if (rvalid && fvalid && i < p.n_tbl) own = *reinterpret_cast<const float4*>(p.tbl + i * p.ldt + f0);
    } else if (MODE == MODE_FINISH) {               // the hub's own row of the real table
      if (rvalid && fvalid && io < p.n_own) own = *reinterpret_cast<const float4*>(p.own + io * p.ldown + f0);
    }

    // a batch of U rows enters the running sum by a compensated add (cmp: what the adds so far rounded away): a hub row of
    // 30 000 edges, whose running sum dwarfs every late batch, keeps fp32's last digits; the walk is gather-bound, the adds free
    float4 acc = f4_zero(), cmp = f4_zero();
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? (MODE == MODE_FINISH ? e : p.col[e]) : -1;
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
        nid[u] = e < end ? (MODE == MODE_FINISH ? e : p.col[e]) : -1;
      }
      float4 b = v[0];
#pragma unroll
      for (int u = 1; u < U; ++u) {
        b.x += v[u].x; b.y += v[u].y; b.z += v[u].z; b.w += v[u].w;
      }
      const float4 y = make_float4(b.x - cmp.x, b.y - cmp.y, b.z - cmp.z, b.w - cmp.w);
      const float4 t = make_float4(acc.x + y.x, acc.y + y.y, acc.z + y.z, acc.w + y.w);
      cmp = make_float4((t.x - acc.x) - y.x, (t.y - acc.y) - y.y, (t.z - acc.z) - y.z, (t.w - acc.w) - y.w);
      acc = t;
    }
    acc = ep_sum<LF, GL>(acc);
    if (MODE == MODE_SEGMENT) {                     // the partial row: the sum alone (pad columns are never read as values)
      if (rvalid && sub == 0 && fvalid) *reinterpret_cast<float4*>(p.out + i * p.ldo + f0) = acc;
      continue;
    }
    float o[4] = {fmaf(self_w, own.x, acc.x), fmaf(self_w, own.y, acc.y), fmaf(self_w, own.z, acc.z), fmaf(self_w, own.w, acc.w)};
    if (p.bias != nullptr && fvalid) {
      const float4 b = *reinterpret_cast<const float4*>(p.bias + f0);
      o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w;
    }
    if (EPI == EPI_RELU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
      if (p.thr != 0u) {
        const int64_t ih = rvalid ? (ROW_ID ? p.row_id[io] : io) : 0;
        const uint64_t e = (uint64_t)ih * (uint64_t)p.d_full + (uint64_t)(p.c0 + f0);
        drop4(o, e, (p.d_full & 3) == 0, seed, p.thr, p.keep_scale);
      }
    } else if (EPI == EPI_LOGSOFTMAX) {
      log_softmax4<LF>(o, f0, p.D);
    }
    if (rvalid && sub == 0 && fvalid) {
#pragma unroll
      for (int c = 0; c < 4; ++c) if (f0 + c >= p.D) o[c] = 0.f;   // pad columns of the row leave as 0
      *reinterpret_cast<float4*>(p.out + io * p.ldo + f0) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// <g_i, T_i> over rows i < n_rows and columns < D, in fp64: the rows of conv_bwd_rows_kernel, one partial per block
template <int LF>
__global__ __launch_bounds__(256) void gin_eps_dot_kernel(const float* g, int64_t ldg, const float* tbl, int64_t ldt, int64_t n_rows,
                                                           int32_t D, double* partial) {
  constexpr int RPB = 256 / LF;
  __shared__ double wsum[4];
  const int r = threadIdx.x / LF;
  const int f0 = (threadIdx.x % LF) * 4;
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < n_rows; base += (int64_t)gridDim.x * RPB) {
    const int64_t i = base + r;
    if (i >= n_rows) continue;
    for (int f = f0; f < D; f += 4 * LF) {
      const float4 a = *reinterpret_cast<const float4*>(g + i * ldg + f);     // pad columns of g are 0
      const float4 b = *reinterpret_cast<const float4*>(tbl + i * ldt + f);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) if (f + c < D) acc = fma((double)av[c], (double)bv[c], acc);
    }
  }
  // the block's partial: fixed butterfly inside a wave, then the four waves in order
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// grad_eps = sum of `count` partials in a fixed order
__global__ __launch_bounds__(256) void gin_eps_finish_kernel(const double* partial, int count, float* grad_eps) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int k = threadIdx.x; k < count; k += 256) a += partial[k];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *grad_eps = (float)sh[0];
}

template <int LF, int EP, int U, int EPI, bool ROW_ID, int MODE, bool HUBS>
int launch_agg(const GinParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const int grid = persistent_grid(gin_agg_kernel<LF, EP, U, EPI, ROW_ID, MODE, HUBS>, ntiles, &cap);
  hipLaunchKernelGGL((gin_agg_kernel<LF, EP, U, EPI, ROW_ID, MODE, HUBS>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int EPI, bool ROW_ID = false, int MODE = MODE_ROWS, bool HUBS = false>
int dispatch_agg(const GinParams& p, hipStream_t st) {
  return lf_ladder((p.D + 3) / 4,   // float4 slots of the slice
                   [&](auto LF, auto EP, auto U) { return launch_agg<LF, EP, U, EPI, ROW_ID, MODE, HUBS>(p, st); });
}

// the epilogue's instantiation of one mode.  The row id only feeds the dropout hash: without dropout (or without ids) the plain
// kernel runs
template <int MODE, bool HUBS>
int dispatch_epi(int epilogue, const GinParams& p, hipStream_t st) {
  if (epilogue == EPI_RELU && p.row_id != nullptr && p.thr != 0u) return dispatch_agg<EPI_RELU, true, MODE, HUBS>(p, st);
  return epi_switch(epilogue, [&](auto EPI) { return dispatch_agg<EPI, false, MODE, HUBS>(p, st); });
}

// the segment tables of a hub call, checked by the entries
struct GinHubs {
  int32_t threshold; const int32_t* rows; int64_t n_hubs; const int32_t* seg_ptr; const int32_t* bounds; int64_t n_seg;
  float* part;                                     // [n_seg, part_ld(D)] partial rows
};

int64_t part_ld(int32_t D) { return D < SLICE ? ((int64_t)D + 3) / 4 * 4 : SLICE; }

template <int LF>
int launch_eps_dot(const float* g, int64_t ldg, const float* tbl, int64_t ldt, int64_t n_rows, int32_t D, double* partial,
                   int* grid_out, hipStream_t st) {
  constexpr int RPB = 256 / LF;
  int64_t grid = (n_rows + RPB - 1) / RPB;
  if (grid > GIN_MAX_BLOCKS) grid = GIN_MAX_BLOCKS;
  if (grid < 1) grid = 1;
  *grid_out = (int)grid;
  hipLaunchKernelGGL((gin_eps_dot_kernel<LF>), dim3((unsigned)grid), dim3(256), 0, st, g, ldg, tbl, ldt, n_rows, D, partial);
  BGNN_LAUNCH_CHECK();
  return 0;
}

bool edges_ok(int64_t n_edges) { return n_edges >= 0 && n_edges <= (int64_t)INT32_MAX; }

// the column slices of one walk; the callers have checked shapes and alignment
int run_agg(const float* tbl, int64_t ldt, int64_t n_tbl, const float* eps, const float* bias, const int32_t* rowptr,
            const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t D, int epilogue, float p_drop, uint64_t seed,
            const uint64_t* seed_dev, const int64_t* row_id, float* out, int64_t ldo, hipStream_t st,
            const GinHubs* hubs = nullptr) {
  for (int32_t c0 = 0; c0 < D; c0 += SLICE) {
    GinParams p{};
    p.tbl = tbl + c0; p.ldt = ldt; p.n_tbl = n_tbl;
    p.eps = eps;
    p.bias = bias ? bias + c0 : nullptr;
    p.rowptr = rowptr; p.col = col; p.n_edges = n_edges; p.n_rows = n_rows;
    p.D = D - c0 < SLICE ? D - c0 : SLICE;
    p.out = out + c0; p.ldo = ldo;
    drop_consts(p_drop, p.thr, p.keep_scale);
    p.seed = seed; p.seed_dev = seed_dev; p.d_full = D; p.c0 = c0;
    p.row_id = row_id;
    if (hubs == nullptr) {
      const int rc = dispatch_epi<MODE_ROWS, false>(epilogue, p, st);
      if (rc != 0) return rc;
      continue;
    }
    p.hub_threshold = hubs->threshold;
    int rc = dispatch_epi<MODE_ROWS, true>(epilogue, p, st);
    if (rc != 0) return rc;
    GinParams s = p;                         // partial rows of the segments (the slice's columns, densely packed)
    s.eps = nullptr; s.bias = nullptr; s.rowptr = hubs->bounds; s.n_rows = hubs->n_seg;
    s.out = hubs->part; s.ldo = part_ld(D); s.thr = 0u; s.row_id = nullptr;
    rc = dispatch_agg<EPI_NONE, false, MODE_SEGMENT, false>(s, st);
    if (rc != 0) return rc;
    GinParams f = p;                         // a hub's partial rows in segment order, its own row, then bias and epilogue
    f.tbl = hubs->part; f.ldt = part_ld(D); f.n_tbl = hubs->n_seg;
    f.rowptr = hubs->seg_ptr; f.col = nullptr; f.n_edges = hubs->n_seg; f.n_rows = hubs->n_hubs;
    f.hub_rows = hubs->rows; f.n_out = n_rows;
    f.own = p.tbl; f.ldown = ldt; f.n_own = n_tbl;
    rc = dispatch_epi<MODE_FINISH, false>(epilogue, f, st);
    if (rc != 0) return rc;
  }
  return 0;
}

// the hub arguments of an entry -> GinHubs (n_hubs == 0: no hub launches, *use = false); ws: where the partial rows go
int check_hubs(int32_t hub_threshold, const int32_t* hub_rows, int64_t n_hubs, const int32_t* hub_seg_ptr, const int32_t* seg_bounds,
               int64_t n_seg, void* ws, size_t ws_bytes, int32_t D, GinHubs* h, bool* use) {
  *use = false;
  if (n_hubs < 0 || n_seg < 0) return BGNN_E_SHAPE;
  if (n_hubs == 0) return 0;
  if (hub_threshold < 1 || n_seg < n_hubs || n_seg > (int64_t)INT32_MAX) return BGNN_E_SHAPE;
  if (!hub_rows || !hub_seg_ptr || !seg_bounds || !ws) return BGNN_E_NULL;
  if (ws_bytes < bgnn_gin_aggregate_hub_workspace_bytes(n_seg, D)) return BGNN_E_WORKSPACE;
  h->threshold = hub_threshold; h->rows = hub_rows; h->n_hubs = n_hubs; h->seg_ptr = hub_seg_ptr; h->bounds = seg_bounds;
  h->n_seg = n_seg;
  h->part = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws), 16));
  *use = true;
  return 0;
}

}  // namespace

extern "C" int bgnn_gin_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* eps, const float* bias_opt,
                                      const int32_t* rowptr, const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t D,
                                      int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                      const int64_t* row_id_opt, float* out, int64_t ldo, void* stream) {
  if (!tbl || !rowptr || !col || !out) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < n_rows || D <= 0 || !edges_ok(n_edges)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if (!tbl_ok(tbl, ldt, D) || !tbl_ok(out, ldo, D) || (bias_opt && !bgnn_aligned16(bias_opt))) return BGNN_E_ALIGN;
  if (out == tbl) return BGNN_E_SHAPE;
  if (n_rows == 0) return 0;
  return run_agg(tbl, ldt, n_tbl, eps, bias_opt, rowptr, col, n_edges, n_rows, D, epilogue, p_drop, seed, seed_dev_opt, row_id_opt,
                 out, ldo, (hipStream_t)stream);
}

extern "C" size_t bgnn_gin_aggregate_hub_workspace_bytes(int64_t n_seg, int32_t D) {
  if (n_seg <= 0 || D <= 0) return 0;
  return (size_t)n_seg * (size_t)part_ld(D) * sizeof(float) + 16;
}

extern "C" int bgnn_gin_aggregate_hub_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* eps, const float* bias_opt,
                                          const int32_t* rowptr, const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t D,
                                          int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                          int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                                          const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                          void* ws_opt, size_t ws_bytes, const int64_t* row_id_opt, float* out, int64_t ldo,
                                          void* stream) {
  if (!tbl || !rowptr || !col || !out) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < n_rows || D <= 0 || !edges_ok(n_edges)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if (!tbl_ok(tbl, ldt, D) || !tbl_ok(out, ldo, D) || (bias_opt && !bgnn_aligned16(bias_opt))) return BGNN_E_ALIGN;
  if (out == tbl) return BGNN_E_SHAPE;
  GinHubs h{};
  bool use = false;
  if (const int rc = check_hubs(hub_threshold, hub_rows_opt, n_hubs, hub_seg_ptr_opt, seg_bounds_opt, n_seg, ws_opt, ws_bytes, D, &h,
                                &use)) return rc;
  if (n_rows == 0) return 0;
  return run_agg(tbl, ldt, n_tbl, eps, bias_opt, rowptr, col, n_edges, n_rows, D, epilogue, p_drop, seed, seed_dev_opt, row_id_opt,
                 out, ldo, (hipStream_t)stream, use ? &h : nullptr);
}

extern "C" size_t bgnn_gin_aggregate_bwd_workspace_bytes(int64_t n_rows, int32_t D) {
  if (n_rows < 0 || D <= 0) return 0;
  return (size_t)GIN_MAX_BLOCKS * sizeof(double) + 16;          // one row pass's partials
}

// both backward entries: the checks, pass A, the grad_eps passes, then pass B -- with `hubs` through the hub walk
static int gin_bwd(const float* tbl_opt, int64_t ldt, const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, int64_t n_rows,
                   const int32_t* t_rowptr, const int32_t* t_col, int64_t n_edges, int64_t n_src, int32_t D, const float* eps,
                   int epilogue, float p_drop, float* g, int64_t ldg, float* grad_tbl, int64_t ldgt, float* grad_eps_opt,
                   void* ws_opt, size_t ws_bytes, void* stream, const GinHubs* hubs) {
  if (!grad_y || !t_rowptr || !t_col || !g || !grad_tbl) return BGNN_E_NULL;
  if (epilogue != EPI_NONE && !y) return BGNN_E_NULL;
  if (grad_eps_opt && (!tbl_opt || !ws_opt)) return BGNN_E_NULL;
  if (n_rows < 0 || n_src < 0 || D <= 0 || !edges_ok(n_edges)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if (grad_eps_opt && ws_bytes < bgnn_gin_aggregate_bwd_workspace_bytes(n_rows, D)) return BGNN_E_WORKSPACE;
  if ((y && !tbl_ok(y, ldy, D)) || !tbl_ok(grad_y, ldgy, D) || !tbl_ok(g, ldg, D) || !tbl_ok(grad_tbl, ldgt, D)) return BGNN_E_ALIGN;
  if (grad_eps_opt && !tbl_ok(tbl_opt, ldt, D)) return BGNN_E_ALIGN;
  if (grad_tbl == g || grad_tbl == grad_y || (y && grad_tbl == y)) return BGNN_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (n_rows > 0) {
    BwdRowsParams p{};
    p.y = y; p.ldy = ldy; p.gy = grad_y; p.ldgy = ldgy; p.n_rows = n_rows; p.D = D;
    uint32_t thr;
    drop_consts(p_drop, thr, p.keep_scale);
    p.g = g; p.ldg = ldg;
    const int rc = dispatch_bwd_rows<false>(epilogue, p, st);   // pass A: g
    if (rc != 0) return rc;
  }
  if (grad_eps_opt) {                                           // <g, T>: per-block fp64 partials, then their fixed-order sum
    double* partial = reinterpret_cast<double*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws_opt), 16));
    int grid = 0;
    if (n_rows > 0) {
      const int rc = lf_ladder((D + 3) / 4, [&](auto LF, auto, auto) {
        return launch_eps_dot<LF>(g, ldg, tbl_opt, ldt, n_rows, D, partial, &grid, st);
      });
      if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(gin_eps_finish_kernel, dim3(1), dim3(256), 0, st, partial, grid, grad_eps_opt);
    BGNN_LAUNCH_CHECK();
  }
  if (n_src == 0) return 0;
  // pass B: the forward walk over the by-source view; source row j adds (1 + eps) * g_j where j is a destination row too
  return run_agg(g, ldg, n_rows, eps, nullptr, t_rowptr, t_col, n_edges, n_src, D, EPI_NONE, 0.f, 0, nullptr, nullptr, grad_tbl,
                 ldgt, st, hubs);
}

extern "C" int bgnn_gin_aggregate_bwd_f32(const float* tbl_opt, int64_t ldt, const float* y, int64_t ldy, const float* grad_y,
                                          int64_t ldgy, int64_t n_rows, const int32_t* t_rowptr, const int32_t* t_col,
                                          int64_t n_edges, int64_t n_src, int32_t D, const float* eps, int epilogue, float p_drop,
                                          float* g, int64_t ldg, float* grad_tbl, int64_t ldgt, float* grad_eps_opt, void* ws_opt,
                                          size_t ws_bytes, void* stream) {
  return gin_bwd(tbl_opt, ldt, y, ldy, grad_y, ldgy, n_rows, t_rowptr, t_col, n_edges, n_src, D, eps, epilogue, p_drop, g, ldg,
                 grad_tbl, ldgt, grad_eps_opt, ws_opt, ws_bytes, stream, nullptr);
}

// ws_opt: the grad_eps partials first (bgnn_gin_aggregate_bwd_workspace_bytes, only with grad_eps_opt), then the partial rows
extern "C" int bgnn_gin_aggregate_bwd_hub_f32(const float* tbl_opt, int64_t ldt, const float* y, int64_t ldy, const float* grad_y,
                                              int64_t ldgy, int64_t n_rows, const int32_t* t_rowptr, const int32_t* t_col,
                                              int64_t n_edges, int64_t n_src, int32_t D, const float* eps, int epilogue,
                                              float p_drop, int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                                              const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                              float* g, int64_t ldg, float* grad_tbl, int64_t ldgt, float* grad_eps_opt,
                                              void* ws_opt, size_t ws_bytes, void* stream) {
  if (D <= 0 || n_rows < 0) return BGNN_E_SHAPE;
  const size_t eps_bytes = grad_eps_opt ? bgnn_gin_aggregate_bwd_workspace_bytes(n_rows, D) : 0;
  if (n_hubs > 0 && (!ws_opt || ws_bytes < eps_bytes)) return ws_opt ? BGNN_E_WORKSPACE : BGNN_E_NULL;
  GinHubs h{};
  bool use = false;
  if (const int rc = check_hubs(hub_threshold, hub_rows_opt, n_hubs, hub_seg_ptr_opt, seg_bounds_opt, n_seg,
                                ws_opt ? static_cast<char*>(ws_opt) + eps_bytes : nullptr, n_hubs > 0 ? ws_bytes - eps_bytes : 0, D,
                                &h, &use)) return rc;
  return gin_bwd(tbl_opt, ldt, y, ldy, grad_y, ldgy, n_rows, t_rowptr, t_col, n_edges, n_src, D, eps, epilogue, p_drop, g, ldg,
                 grad_tbl, ldgt, grad_eps_opt, ws_opt, use ? eps_bytes : ws_bytes, stream, use ? &h : nullptr);
}
