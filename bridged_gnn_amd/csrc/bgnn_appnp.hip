// APPNP propagation and feature dropout for gfx950 (wave64).
//
// Replaces (reference, Bridged-GNN/models/backbones.py:110-128): PyG `APPNP(K=10, alpha=0.1)` behind APPNP_Net's MLP -- K
// personalised-PageRank steps over gcn_norm(add_self_loops=True) with unit edge weights -- with the closing F.log_softmax, and
// the two F.dropout(p=0.5) sites of that MLP.  The graph is the by-destination CSR of bgnn_gcn.hip (exactly one self loop per row):
//   z_0 = h,  z_{k+1} = (1 - alpha) * A^ z_k + alpha * h,  out = epi(z_K),  A^_ij = dinv_i * dinv_j over the edges j -> i.
// The operator is linear and A^'s products are symmetric, so the gradient with respect to h is the same recurrence over the
// by-source view with the output gradient in h's place: this file has no backward kernel, the caller walks the other view.
//
// Scaled state: between steps the state is kept as s_k = dinv (.) z_k in two alternating [N, pad4(D)] buffers of the workspace, so
// the edge loop of a step gathers rows only:
//   z_{k+1,i} = (1 - alpha) * dinv_i * sum_{t in row i} s_k[col[t]] + alpha * h_i,   stored as s_{k+1,i} = dinv_i * z_{k+1,i};
// the last step stores z_K itself, or its row log_softmax, with the pad columns as 0.  The FIRST step has no scaled state yet:
// a template flag makes it read h and gather dinv[col[t]] next to the row, as gcn_agg_kernel does (no pre-pass that writes s_0).
// K == 0 is the last-step kernel with the edge walk switched off and alpha = 1: out = epi(h).
// Bytes per step at width D (Dp = pad4(D)): E'(4 Dp + 4) + N(8 Dp + 8) -- a gathered row and a column id per edge; the
// teleport row, the stored row, rowptr and dinv_i per node -- against the composition's E'(4 Dp + 8) + N(4 Dp + 8) for the
// aggregation plus at least 12 Dp N for the torch pass that scales it and adds the teleport term.
//
// Mapping, log_softmax and launch helpers: bgnn_conv_common.h; the kernel follows gcn_agg_kernel, hub rows included (the row
// kernel skips rows of at least hub_threshold edges, SEGMENT mode sums a (begin, end) segment into a partial row, FINISH mode
// adds a hub's partial rows in segment order and applies the step's scaling, teleport term, store and epilogue).  One launch
// per step (three with hubs) on the caller's stream; steps are ordered by launch order alone.  No float atomics.
// bgnn_appnp_step_f32 is that per-step launch sequence (run_step) as an entry of its own, over a rectangular graph: n_rows owned
// rows gather from a table of n_tbl >= n_rows rows (owned rows, then halo slots), so that a rank of a node partition can exchange
// the halo rows of the state between steps.
//
// Feature dropout: streaming passes over a contiguous [N, D] activation of any width, four consecutive elements per lane
// (16-byte accesses; element index = row * D + column = the flat index, so a quad shares one word pair of the dropout hash).
// The _rows_ passes take the GLOBAL row of every local row and hash row_ids[r] * D + column: a rank's rows draw the whole-graph masks.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;
enum { MODE_ROWS = 0, MODE_SEGMENT = 1, MODE_FINISH = 2 };
enum { STORE_STATE = 0, STORE_OUT = 1, STORE_LOGSOFTMAX = 2 };   // dinv_i * z into the next state buffer | z_K | log_softmax(z_K)

struct AppnpParams {
  const float* tbl; int64_t ldt; int64_t n_tbl;    // gathered rows: h (FIRST), the scaled state, or (FINISH) the partial rows
  const float* h; int64_t ldh;                     // teleport rows
  const int32_t* rowptr; const int32_t* col;       // ROWS: the CSR; SEGMENT: rowptr = (begin, end) pairs; FINISH: rowptr = hub_seg_ptr
  const float* dinv; int64_t n_dinv;
  int64_t n_rows;                                  // rows / segments / hubs of this launch
  int32_t D;
  int32_t hub_threshold;                           // ROWS: rows of at least this many edges are left to the hub launches (0: none)
  int32_t no_edges;                                // ROWS: every row is walked as empty (K == 0)
  const int32_t* hub_rows; int64_t n_out;          // FINISH: output row of hub h, rows of out
  float alpha, beta;                               // teleport weight and 1 - alpha
  float* out; int64_t ldo;
};

template <int LF, int EP, int U, int MODE, bool FIRST, int STORE>
__global__ __launch_bounds__(256) void appnp_step_kernel(AppnpParams p) {
  constexpr int GL = LF * EP;            // lanes per output row
  constexpr int GPW = 64 / GL;           // rows per wave
  constexpr int RPB = 4 * GPW;           // rows per block iteration (4 waves)
  constexpr bool WEIGHTED = FIRST && MODE != MODE_FINISH;   // the gathered rows are h's: scale each by dinv[col]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int f0 = (lg % LF) * 4;
  const bool fvalid = f0 < p.D;

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
    if (MODE == MODE_ROWS && p.no_edges) beg = end = 0;
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
        if (WEIGHTED) w[u] = (ok && (int64_t)nid[u] < p.n_dinv) ? p.dinv[nid[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? (MODE == MODE_FINISH ? e : p.col[e]) : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (WEIGHTED) { acc.x += w[u] * v[u].x; acc.y += w[u] * v[u].y; acc.z += w[u] * v[u].z; acc.w += w[u] * v[u].w; }
        else { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
      }
    }
    acc = ep_sum<LF, GL>(acc);
    // the row written: the segment's partial row, the hub's own row, or row i
    int64_t io = i;
    if (MODE == MODE_FINISH) io = rvalid ? (int64_t)p.hub_rows[i] : 0;
    const bool ovalid = MODE == MODE_FINISH ? (rvalid && io >= 0 && io < p.n_out) : rvalid;
    float o[4] = {acc.x, acc.y, acc.z, acc.w};
    if (MODE != MODE_SEGMENT) {
      const float di = (ovalid && io < p.n_dinv) ? p.dinv[io] : 0.f;
      float4 hv = f4_zero();
      if (ovalid && fvalid) hv = *reinterpret_cast<const float4*>(p.h + io * p.ldh + f0);
      const float t[4] = {hv.x, hv.y, hv.z, hv.w};
      const float s = p.beta * di;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        o[c] = s * o[c] + p.alpha * t[c];                       // z_{k+1}: alpha == 1 leaves h's bits
        if (STORE == STORE_STATE) o[c] *= di;
      }
      if (STORE == STORE_LOGSOFTMAX) log_softmax4<LF>(o, f0, p.D);
    }
    if (ovalid && sub == 0 && fvalid) {
#pragma unroll
      for (int c = 0; c < 4; ++c) if (f0 + c >= p.D) o[c] = 0.f;   // pad columns of the row leave as 0
      *reinterpret_cast<float4*>(p.out + io * p.ldo + f0) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int LF, int EP, int U, int MODE, bool FIRST, int STORE>
int launch_step(const AppnpParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const int grid = persistent_grid(appnp_step_kernel<LF, EP, U, MODE, FIRST, STORE>, ntiles, &cap);
  hipLaunchKernelGGL((appnp_step_kernel<LF, EP, U, MODE, FIRST, STORE>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int MODE, bool FIRST, int STORE>
int dispatch_lf(const AppnpParams& p, hipStream_t st) {
  return lf_ladder((p.D + 3) / 4, [&](auto LF, auto EP, auto U) { return launch_step<LF, EP, U, MODE, FIRST, STORE>(p, st); });
}

// a ROWS or FINISH launch of one step (SEGMENT stores raw partial sums: dispatch_lf<MODE_SEGMENT, FIRST, STORE_STATE> directly)
template <int MODE>
int dispatch_step(bool first, int store, const AppnpParams& p, hipStream_t st) {
  constexpr bool F = MODE != MODE_FINISH;    // a finish group adds partial rows that are weighted already: one instantiation
  if (store == STORE_STATE) return first && F ? dispatch_lf<MODE, F, STORE_STATE>(p, st) : dispatch_lf<MODE, false, STORE_STATE>(p, st);
  if (store == STORE_OUT) return first && F ? dispatch_lf<MODE, F, STORE_OUT>(p, st) : dispatch_lf<MODE, false, STORE_OUT>(p, st);
  return first && F ? dispatch_lf<MODE, F, STORE_LOGSOFTMAX>(p, st) : dispatch_lf<MODE, false, STORE_LOGSOFTMAX>(p, st);
}

int64_t pad4_ld(int32_t D) { return ((int64_t)D + 3) / 4 * 4; }
size_t state_floats(int64_t n_rows, int32_t D) { return (size_t)n_rows * (size_t)pad4_ld(D); }

// the hub argument group of one step; n_hubs == 0: every row is walked by the row kernel
struct HubTables {
  int32_t threshold; const int32_t* rows; int64_t n_hubs; const int32_t* seg_ptr; const int32_t* seg_bounds; int64_t n_seg;
  float* part;                                     // [n_seg, pad4(D)] partial rows
};

// one step of the recurrence over p's graph (p: the ROWS launch with tbl, h, out and the CSR set; hub_threshold is set here): the
// row launch and, with hub tables, the segment and finish launches.  The K-step entry and bgnn_appnp_step_f32 both run this.
int run_step(AppnpParams p, bool first, int store, const HubTables& ht, hipStream_t st) {
  const bool hubs = ht.n_hubs > 0;
  p.hub_threshold = hubs ? ht.threshold : 0;
  int rc = dispatch_step<MODE_ROWS>(first, store, p, st);
  if (rc != 0 || !hubs) return rc;
  const int64_t ldw = pad4_ld(p.D);
  AppnpParams s = p;                         // partial rows of the segments
  s.rowptr = ht.seg_bounds; s.n_rows = ht.n_seg; s.hub_threshold = 0;
  s.out = ht.part; s.ldo = ldw;
  rc = first ? dispatch_lf<MODE_SEGMENT, true, STORE_STATE>(s, st) : dispatch_lf<MODE_SEGMENT, false, STORE_STATE>(s, st);
  if (rc != 0) return rc;
  AppnpParams f = p;                         // a hub's partial rows in segment order, then the step's scaling, teleport and store
  f.tbl = ht.part; f.ldt = ldw; f.n_tbl = ht.n_seg;
  f.rowptr = ht.seg_ptr; f.col = nullptr; f.n_rows = ht.n_hubs; f.hub_threshold = 0; f.hub_rows = ht.rows;
  return dispatch_step<MODE_FINISH>(first, store, f, st);
}

// ---- feature dropout ---------------------------------------------------------------------------------------------------------
struct FdropParams {
  const float* x;            // forward: the input; backward: y (read only under ReLU)
  const float* gy;           // backward
  const float* bias;
  int64_t total; int32_t D;
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  float* y;                  // forward: the output; backward: grad_x
};

// one quad (elements e .. e+3 of the flat activation) of a pass: load, bias and activation (forward) or the gradient (backward),
// the mask through drop(o), store.  col_of(): the column of element e, asked for only where a bias is added.
template <bool RELU, bool BWD, class ColOf, class Drop>
__device__ __forceinline__ void fdrop_quad(const FdropParams& p, int64_t e, ColOf col_of, Drop drop) {
  const bool full = e + 3 < p.total;                            // the last quad of a tensor of total % 4 != 0 goes element by element
  float v[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
  const bool need_v = !BWD || RELU;
  if (full) {
    if (need_v) { const float4 t = *reinterpret_cast<const float4*>(p.x + e); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    if (BWD) { const float4 t = *reinterpret_cast<const float4*>(p.gy + e); d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w; }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) if (e + c < p.total) { if (need_v) v[c] = p.x[e + c]; if (BWD) d[c] = p.gy[e + c]; }
  }
  float o[4];
  if (BWD && RELU) {
    // ReLU then dropout: y > 0 <=> kept and positive
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = v[c] > 0.f ? d[c] * p.keep_scale : 0.f;
  } else {
    if (!BWD) {
      if (p.bias != nullptr) {
        int32_t col = col_of();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (e + c < p.total) v[c] += p.bias[col];
          if (++col == p.D) col = 0;
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = RELU ? fmaxf(v[c], 0.f) : v[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = d[c];
    }
    if (p.thr != 0u) drop(o);
  }
  if (full) {
    *reinterpret_cast<float4*>(p.y + e) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) if (e + c < p.total) p.y[e + c] = o[c];
  }
}

template <bool RELU, bool BWD>
__global__ __launch_bounds__(256) void feature_dropout_kernel(FdropParams p) {
  uint64_t seed = p.seed;
  if (p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;
  const int64_t nquad = (p.total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
    const int64_t e = q << 2;
    fdrop_quad<RELU, BWD>(p, e, [&] { return (int32_t)(e % p.D); },
                          [&](float (&o)[4]) { drop4(o, (uint64_t)e, true, seed, p.thr, p.keep_scale); });
  }
}

template <bool RELU, bool BWD>
int launch_fdrop(const FdropParams& p, hipStream_t st) {
  int64_t grid = ((p.total + 3) / 4 + 255) / 256;
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((feature_dropout_kernel<RELU, BWD>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

// The same pass over a rank's rows of a partitioned activation: element (r, c) draws the bits of flat element
// row_ids[r] * D + c, the whole-graph call's.  The data are still walked as quads of the local flat index (16-byte accesses);
// one division per quad splits it into (row, column), the other three elements follow by increment and wrap.
// ALIGNED (D % 4 == 0): a quad lies inside one row and its global index is a multiple of 4, so it shares one word pair.
// Otherwise a quad may straddle rows and word pairs: each element is hashed at its own index, the word pair kept while
// the index's quad does not change.
template <bool RELU, bool BWD, bool ALIGNED>
__global__ __launch_bounds__(256) void feature_dropout_rows_kernel(FdropParams p, const int64_t* __restrict__ row_ids) {
  uint64_t seed = p.seed;
  if (p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;
  const int64_t nquad = (p.total + 3) >> 2;
  const bool narrow = p.total < ((int64_t)1 << 32);             // block-uniform: a 32-bit division where the index fits
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
    const int64_t e = q << 2;
    const int64_t row0 = narrow ? (int64_t)((uint32_t)e / (uint32_t)p.D) : e / p.D;
    const int32_t col0 = (int32_t)(e - row0 * p.D);
    fdrop_quad<RELU, BWD>(p, e, [&] { return col0; }, [&](float (&o)[4]) {
      if (ALIGNED) {                                            // D % 4 == 0: total % 4 == 0 too, every quad is full
        drop4(o, (uint64_t)row_ids[row0] * (uint64_t)p.D + (uint64_t)col0, true, seed, p.thr, p.keep_scale);
        return;
      }
      int64_t row = row0;
      int32_t col = col0;
      uint64_t base = (uint64_t)row_ids[row] * (uint64_t)p.D, pair = ~(uint64_t)0;
      uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (e + c < p.total) {
          const uint64_t g = base + (uint64_t)col;
          if ((g >> 2) != pair) { pair = g >> 2; drop_words(pair, seed, w0, w1); }
          const uint32_t w = (g & 2) ? w1 : w0;
          const uint32_t bits = (g & 1) ? (w >> 16) : (w & 0xFFFFu);
          o[c] = bits >= p.thr ? o[c] * p.keep_scale : 0.f;
          if (++col == p.D) {                                   // the next element opens the next row
            col = 0; ++row;
            if (c < 3 && e + c + 1 < p.total) base = (uint64_t)row_ids[row] * (uint64_t)p.D;
          }
        }
      }
    });
  }
}

constexpr int FDROP_ROWS_MAX_GRID = 4096;    // blocks of 256 lanes, one quad per lane and trip; the rest is walked by stride

template <bool RELU, bool BWD>
int launch_fdrop_rows(const FdropParams& p, const int64_t* row_ids, hipStream_t st) {
  int64_t grid = ((p.total + 3) / 4 + 255) / 256;
  if (grid > FDROP_ROWS_MAX_GRID) grid = FDROP_ROWS_MAX_GRID;
  if (grid < 1) grid = 1;
  if (p.D % 4 == 0)
    hipLaunchKernelGGL((feature_dropout_rows_kernel<RELU, BWD, true>), dim3((unsigned)grid), dim3(256), 0, st, p, row_ids);
  else
    hipLaunchKernelGGL((feature_dropout_rows_kernel<RELU, BWD, false>), dim3((unsigned)grid), dim3(256), 0, st, p, row_ids);
  BGNN_LAUNCH_CHECK();
  return 0;
}

int fdrop_check(const float* a, const float* b, int64_t n_rows, int32_t D, float p_drop) {
  if (!a || !b) return BGNN_E_NULL;
  if (n_rows < 0 || D <= 0 || !(p_drop >= 0.f && p_drop < 1.f)) return BGNN_E_SHAPE;
  if (!bgnn_aligned16(a) || !bgnn_aligned16(b)) return BGNN_E_ALIGN;
  return 0;
}

}  // namespace

extern "C" size_t bgnn_appnp_propagate_workspace_bytes(int64_t n_rows, int32_t D, int64_t n_seg) {
  if (n_rows <= 0 || D <= 0) return 0;
  if (n_seg < 0) n_seg = 0;
  return (2 * state_floats(n_rows, D) + state_floats(n_seg, D)) * sizeof(float) + 16;
}

extern "C" int bgnn_appnp_propagate_f32(const float* h, int64_t ld_h, const int32_t* rowptr, const int32_t* col, const float* dinv,
                                        int64_t n_dinv, int64_t n_rows, int32_t D, int32_t K, float alpha, int epilogue,
                                        int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                                        const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                        void* ws_opt, size_t ws_bytes, float* out, int64_t ld_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!h || !rowptr || !col || !dinv || !out) return BGNN_E_NULL;
  if (n_rows < 0 || D < 1 || D > SLICE || K < 0 || n_dinv < n_rows) return BGNN_E_SHAPE;
  if (!(alpha >= 0.f && alpha <= 1.f)) return BGNN_E_SHAPE;
  if (epilogue != EPI_NONE && epilogue != EPI_LOGSOFTMAX) return BGNN_E_SHAPE;
  if (!ld_ok(ld_h, D) || !ld_ok(ld_out, D)) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(h) || !bgnn_aligned16(out)) return BGNN_E_ALIGN;
  if (h == out) return BGNN_E_SHAPE;
  if (n_hubs < 0 || n_seg < 0) return BGNN_E_SHAPE;
  const bool hubs = n_hubs > 0 && K > 0;
  if (n_hubs > 0) {
    if (hub_threshold < 1 || n_seg < n_hubs) return BGNN_E_SHAPE;
    if (!hub_rows_opt || !hub_seg_ptr_opt || !seg_bounds_opt) return BGNN_E_NULL;
  }
  const int64_t ldw = pad4_ld(D);
  const size_t nstate = K >= 2 ? state_floats(n_rows, D) : 0;
  const size_t npart = hubs ? state_floats(n_seg, D) : 0;
  float *s0 = nullptr, *s1 = nullptr, *part = nullptr;
  if (n_rows > 0 && (nstate > 0 || npart > 0)) {
    if (!ws_opt) return BGNN_E_NULL;
    if (ws_bytes < (2 * nstate + npart) * sizeof(float) + 16) return BGNN_E_WORKSPACE;
    s0 = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws_opt), 16));
    s1 = s0 + nstate;
    part = s1 + nstate;
  }
  if (n_rows == 0) return 0;
  const int last_store = epilogue == EPI_LOGSOFTMAX ? STORE_LOGSOFTMAX : STORE_OUT;

  AppnpParams p{};
  p.h = h; p.ldh = ld_h;
  p.rowptr = rowptr; p.col = col; p.dinv = dinv; p.n_dinv = n_dinv; p.n_rows = n_rows; p.D = D;
  p.n_out = n_rows;
  p.alpha = alpha; p.beta = 1.f - alpha;
  if (K == 0) {                              // out = epi(h): the last-step kernel with no edge walked and the teleport term alone
    p.tbl = h; p.ldt = ld_h; p.n_tbl = n_rows;
    p.no_edges = 1; p.alpha = 1.f; p.beta = 0.f;
    p.out = out; p.ldo = ld_out;
    return dispatch_step<MODE_ROWS>(true, last_store, p, st);
  }
  HubTables ht{};
  if (hubs) ht = HubTables{hub_threshold, hub_rows_opt, n_hubs, hub_seg_ptr_opt, seg_bounds_opt, n_seg, part};
  for (int32_t k = 0; k < K; ++k) {
    const bool first = k == 0, last = k == K - 1;
    float* src = (k & 1) ? s0 : s1;          // step k reads what step k-1 wrote: s0 after steps 0, 2, .., s1 after 1, 3, ..
    float* dst = (k & 1) ? s1 : s0;
    if (first) { p.tbl = h; p.ldt = ld_h; } else { p.tbl = src; p.ldt = ldw; }
    p.n_tbl = n_rows;
    if (last) { p.out = out; p.ldo = ld_out; } else { p.out = dst; p.ldo = ldw; }
    if (const int rc = run_step(p, first, last ? last_store : STORE_STATE, ht, st)) return rc;
  }
  return 0;
}

extern "C" int bgnn_appnp_step_f32(const float* tbl, int64_t ld_tbl, int64_t n_tbl, const float* h, int64_t ld_h,
                                   const int32_t* rowptr, const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows,
                                   int32_t D, float alpha, int first, int store,
                                   int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                                   const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                   void* ws_opt, size_t ws_bytes, float* out, int64_t ld_out, void* stream) {
  if (!tbl || !h || !rowptr || !col || !dinv || !out) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < n_rows || D < 1 || D > SLICE) return BGNN_E_SHAPE;
  if (n_dinv < (first ? n_tbl : n_rows)) return BGNN_E_SHAPE;           // the first step gathers dinv[col] over the whole table
  if (!(alpha >= 0.f && alpha <= 1.f)) return BGNN_E_SHAPE;
  if (store != STORE_STATE && store != STORE_OUT && store != STORE_LOGSOFTMAX) return BGNN_E_SHAPE;
  if (!ld_ok(ld_tbl, D) || !ld_ok(ld_h, D) || !ld_ok(ld_out, D)) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(tbl) || !bgnn_aligned16(h) || !bgnn_aligned16(out)) return BGNN_E_ALIGN;
  if (out == tbl || out == h) return BGNN_E_SHAPE;
  if (n_hubs < 0 || n_seg < 0) return BGNN_E_SHAPE;
  HubTables ht{};
  if (n_hubs > 0) {
    if (hub_threshold < 1 || n_seg < n_hubs) return BGNN_E_SHAPE;
    if (!hub_rows_opt || !hub_seg_ptr_opt || !seg_bounds_opt || !ws_opt) return BGNN_E_NULL;
    if (ws_bytes < state_floats(n_seg, D) * sizeof(float) + 16) return BGNN_E_WORKSPACE;
    float* part = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws_opt), 16));
    ht = HubTables{hub_threshold, hub_rows_opt, n_hubs, hub_seg_ptr_opt, seg_bounds_opt, n_seg, part};
  }
  if (n_rows == 0) return 0;
  AppnpParams p{};
  p.tbl = tbl; p.ldt = ld_tbl; p.n_tbl = n_tbl;
  p.h = h; p.ldh = ld_h;
  p.rowptr = rowptr; p.col = col; p.dinv = dinv; p.n_dinv = n_dinv; p.n_rows = n_rows; p.D = D;
  p.n_out = n_rows;
  p.alpha = alpha; p.beta = 1.f - alpha;
  p.out = out; p.ldo = ld_out;
  return run_step(p, first != 0, store, ht, (hipStream_t)stream);
}

extern "C" int bgnn_appnp_log_softmax_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, int64_t n_rows,
                                             int32_t D, float* g, int64_t ldg, void* stream) {
  if (!y || !grad_y || !g) return BGNN_E_NULL;
  if (n_rows < 0 || D < 1 || D > SLICE) return BGNN_E_SHAPE;
  if (!ld_ok(ldy, D) || !ld_ok(ldgy, D) || !ld_ok(ldg, D)) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(y) || !bgnn_aligned16(grad_y) || !bgnn_aligned16(g)) return BGNN_E_ALIGN;
  if (n_rows == 0) return 0;
  BwdRowsParams p{};                         // the log_softmax rule of the convs' backward row pass
  p.y = y; p.ldy = ldy; p.gy = grad_y; p.ldgy = ldgy; p.n_rows = n_rows; p.D = D; p.keep_scale = 1.f;
  p.g = g; p.ldg = ldg;
  return dispatch_bwd_rows<false>(EPI_LOGSOFTMAX, p, (hipStream_t)stream);
}

extern "C" int bgnn_feature_dropout_f32(const float* x, const float* bias_opt, int64_t n_rows, int32_t D, int relu, float p_drop,
                                        uint64_t seed, const uint64_t* seed_dev_opt, float* y, void* stream) {
  if (const int rc = fdrop_check(x, y, n_rows, D, p_drop)) return rc;
  if (n_rows == 0) return 0;
  FdropParams p{};
  p.x = x; p.bias = bias_opt; p.total = n_rows * (int64_t)D; p.D = D;
  drop_consts(p_drop, p.thr, p.keep_scale);
  p.seed = seed; p.seed_dev = seed_dev_opt; p.y = y;
  return relu ? launch_fdrop<true, false>(p, (hipStream_t)stream) : launch_fdrop<false, false>(p, (hipStream_t)stream);
}

extern "C" int bgnn_feature_dropout_bwd_f32(const float* y_opt, const float* grad_y, int64_t n_rows, int32_t D, int relu,
                                            float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, float* grad_x, void* stream) {
  if (const int rc = fdrop_check(grad_y, grad_x, n_rows, D, p_drop)) return rc;
  if (relu && !y_opt) return BGNN_E_NULL;
  if (relu && !bgnn_aligned16(y_opt)) return BGNN_E_ALIGN;
  if (n_rows == 0) return 0;
  FdropParams p{};
  p.x = y_opt; p.gy = grad_y; p.total = n_rows * (int64_t)D; p.D = D;
  drop_consts(p_drop, p.thr, p.keep_scale);
  p.seed = seed; p.seed_dev = seed_dev_opt; p.y = grad_x;
  return relu ? launch_fdrop<true, true>(p, (hipStream_t)stream) : launch_fdrop<false, true>(p, (hipStream_t)stream);
}

extern "C" int bgnn_feature_dropout_rows_f32(const float* x, const float* bias_opt, const int64_t* row_ids, int64_t n_rows, int32_t D,
                                             int relu, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, float* y,
                                             void* stream) {
  if (const int rc = fdrop_check(x, y, n_rows, D, p_drop)) return rc;
  if (!row_ids) return BGNN_E_NULL;
  if (n_rows == 0) return 0;
  FdropParams p{};
  p.x = x; p.bias = bias_opt; p.total = n_rows * (int64_t)D; p.D = D;
  drop_consts(p_drop, p.thr, p.keep_scale);
  p.seed = seed; p.seed_dev = seed_dev_opt; p.y = y;
  return relu ? launch_fdrop_rows<true, false>(p, row_ids, (hipStream_t)stream)
              : launch_fdrop_rows<false, false>(p, row_ids, (hipStream_t)stream);
}

extern "C" int bgnn_feature_dropout_rows_bwd_f32(const float* y_opt, const float* grad_y, const int64_t* row_ids, int64_t n_rows,
                                                 int32_t D, int relu, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                                 float* grad_x, void* stream) {
  if (const int rc = fdrop_check(grad_y, grad_x, n_rows, D, p_drop)) return rc;
  if (!row_ids) return BGNN_E_NULL;
  if (relu && !y_opt) return BGNN_E_NULL;
  if (relu && !bgnn_aligned16(y_opt)) return BGNN_E_ALIGN;
  if (n_rows == 0) return 0;
  FdropParams p{};
  p.x = y_opt; p.gy = grad_y; p.total = n_rows * (int64_t)D; p.D = D;
  drop_consts(p_drop, p.thr, p.keep_scale);
  p.seed = seed; p.seed_dev = seed_dev_opt; p.y = grad_x;
  return relu ? launch_fdrop_rows<true, true>(p, row_ids, (hipStream_t)stream)
              : launch_fdrop_rows<false, true>(p, row_ids, (hipStream_t)stream);
}
