// Building blocks shared by the step-2 conv files (bgnn_sage.hip, bgnn_gcn.hip, bgnn_gat.hip, bgnn_gatv2.hip).  Nothing here is exported.
//
// Mapping of their edge-walking kernels (as agg_kernel in bgnn_aggregate.hip): a group of GL = LF*EP consecutive lanes owns one
// output row; LF lanes span the columns (float4 per lane), EP sub-groups walk different edges of the row (narrow rows), each
// sub-group keeps U neighbour rows in flight.  Blocks are persistent over the XCD-balanced segment order of bgnn_common.h.
//
// Dropout contract (with bgnn_norm.hip): element e = row * width + column of an activation takes the 16 bits drop_bits(e, seed)
// and is kept when they reach the threshold.  A rank's rows of a partitioned graph draw the whole-graph masks by passing their
// global row, and a backward recovers the forward's mask (ReLU: y > 0) or redraws it from the same (seed, e).
#pragma once
#include <type_traits>
#include "bgnn_common.h"

namespace bgnn_conv {

constexpr int SLICE = 128;   // columns per launch of a row-owning group (LF <= 32); wider rows run as column slices

// epilogue codes of the C ABI; 1 is the owning file's activation followed by dropout (ReLU: sage, gcn; ELU: gat)
enum { EPI_NONE = 0, EPI_ACT = 1, EPI_LOGSOFTMAX = 2 };

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// 16 dropout bits of element e
__device__ __forceinline__ uint32_t drop_bits(uint64_t e, uint64_t seed) {
  uint32_t w0, w1;
  drop_words(e >> 2, seed, w0, w1);
  const uint32_t w = (e & 2) ? w1 : w0;
  return (e & 1) ? (w >> 16) : (w & 0xFFFFu);
}

// dropout of the four consecutive elements e..e+3; shared_pair: e % 4 == 0, the four share one word pair (as bgnn_norm.hip)
__device__ __forceinline__ void drop4(float (&o)[4], uint64_t e, bool shared_pair, uint64_t seed, uint32_t thr, float keep_scale) {
  if (shared_pair) {
    uint32_t w0, w1;
    drop_words(e >> 2, seed, w0, w1);
    const uint32_t bits[4] = {w0 & 0xFFFFu, w0 >> 16, w1 & 0xFFFFu, w1 >> 16};
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = bits[c] >= thr ? o[c] * keep_scale : 0.f;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = drop_bits(e + c, seed) >= thr ? o[c] * keep_scale : 0.f;
  }
}

// log_softmax of a row of D <= 4*LF columns that sits in the LF lanes of a group (columns f0..f0+3 in this lane); every lane
// of the wave takes part in the cross-lane steps
template <int LF>
__device__ __forceinline__ void log_softmax4(float (&o)[4], int f0, int D) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < 4; ++c) if (f0 + c < D) m = fmaxf(m, o[c]);
  m = bgnn::group_max<LF>(m);
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) if (f0 + c < D) se += expf(o[c] - m);
  se = bgnn::group_sum<LF>(se);
  const float lse = m + logf(se);
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] -= lse;
}

// sum of the EP = GL/LF sub-groups' partial rows (fixed butterfly: deterministic)
template <int LF, int GL>
__device__ __forceinline__ float4 ep_sum(float4 acc) {
#pragma unroll
  for (int off = LF; off < GL; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off); acc.y += __shfl_xor(acc.y, off);
    acc.z += __shfl_xor(acc.z, off); acc.w += __shfl_xor(acc.w, off);
  }
  return acc;
}

// ---- the attention convs (bgnn_gat.hip, bgnn_gatv2.hip) -----------------------------------------------------------------------
constexpr int EPI_ELU = EPI_ACT;   // their code 1: ELU, then dropout
constexpr int MAX_HEADS = 8;
constexpr int MAX_C = SLICE;

// leaky_relu with a ROUNDED product: never contracted into the subtraction of the row maximum that follows, so the three kernels
// that form e (state sweep, coefficient sweep, backward edge pass) agree bit for bit
__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.f ? z : __fmul_rn(slope, z); }

// a row's edge range cut to the edge arrays: a malformed rowptr gives a wrong sum, never a read or write past them
__device__ __forceinline__ void clamp_row(int32_t& beg, int32_t& end, int64_t n_edges) {
  if (beg < 0) beg = 0;
  if ((int64_t)end > n_edges) end = (int32_t)n_edges;
  if (end < beg) end = beg;
}

// four columns k0..k0+3 of a head slice of C floats at `base` (vec: the slice is 16-byte aligned and C % 4 == 0)
__device__ __forceinline__ void load4(const float* base, int k0, int C, bool vec, bool ok, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (!ok || k0 >= C) return;
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(base + k0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) if (k0 + c < C) v[c] = base[k0 + c];
  }
}

__device__ __forceinline__ void store4(float* base, int k0, int C, bool vec, const float (&v)[4]) {
  if (k0 >= C) return;
  if (vec) {
    *reinterpret_cast<float4*>(base + k0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) if (k0 + c < C) base[k0 + c] = v[c];
  }
}

__device__ __forceinline__ void softmax_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  const float a = m == -INFINITY ? 0.f : s * expf(m - M);
  const float b = m2 == -INFINITY ? 0.f : s2 * expf(m2 - M);
  m = M; s = a + b;
}

// ---- backward row pass of the ReLU convs (sage, gcn): g from (y, dy) per destination row; SCALED also writes s = g / deg ------
struct BwdRowsParams {
  const float* y; int64_t ldy;    // read only where the epilogue needs it (NULL allowed under EPI_NONE)
  const float* gy; int64_t ldgy;
  const int32_t* rowptr;          // SCALED
  int64_t n_rows;
  int32_t D;
  float keep_scale;
  float* g; int64_t ldg;
  float* s; int64_t lds;          // SCALED
};

template <int LF, int EPI, bool SCALED>
static __global__ __launch_bounds__(256) void conv_bwd_rows_kernel(BwdRowsParams p) {
  constexpr int RPB = 256 / LF;
  const int r = threadIdx.x / LF;
  const int f0 = (threadIdx.x % LF) * 4;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < p.n_rows; base += (int64_t)gridDim.x * RPB) {
    const int64_t i = base + r;
    const bool rvalid = i < p.n_rows;
    const int64_t ic = rvalid ? i : 0;
    float inv = 0.f;
    if (SCALED) {
      const int32_t deg = rvalid ? p.rowptr[i + 1] - p.rowptr[i] : 0;
      inv = deg > 0 ? 1.f / (float)deg : 0.f;
    }
    if (EPI == EPI_LOGSOFTMAX) {
      // g = dY - exp(Y) * sum(dY): one column chunk (D <= 4*LF); all lanes reach the group reduction
      float4 y = f4_zero(), dy = f4_zero();
      const bool fvalid = f0 < p.D && rvalid;
      if (fvalid) {
        y = *reinterpret_cast<const float4*>(p.y + ic * p.ldy + f0);
        dy = *reinterpret_cast<const float4*>(p.gy + ic * p.ldgy + f0);
      }
      const float yv[4] = {y.x, y.y, y.z, y.w}, dv[4] = {dy.x, dy.y, dy.z, dy.w};
      float t = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) if (f0 + c < p.D) t += dv[c];
      t = bgnn::group_sum<LF>(t);
      float o[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = (f0 + c < p.D) ? dv[c] - expf(yv[c]) * t : 0.f;
      if (fvalid) {
        *reinterpret_cast<float4*>(p.g + i * p.ldg + f0) = make_float4(o[0], o[1], o[2], o[3]);
        if (SCALED) *reinterpret_cast<float4*>(p.s + i * p.lds + f0) = make_float4(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv);
      }
    } else {
      if (!rvalid) continue;
      for (int f = f0; f < p.D; f += 4 * LF) {
        float4 y = f4_zero();
        if (EPI == EPI_ACT) y = *reinterpret_cast<const float4*>(p.y + i * p.ldy + f);
        const float4 dy = *reinterpret_cast<const float4*>(p.gy + i * p.ldgy + f);
        const float yv[4] = {y.x, y.y, y.z, y.w}, dv[4] = {dy.x, dy.y, dy.z, dy.w};
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          // ReLU then dropout: y > 0 <=> kept and positive, so no pre-activation is needed
          o[c] = EPI == EPI_ACT ? (yv[c] > 0.f ? dv[c] * p.keep_scale : 0.f) : dv[c];
          if (f + c >= p.D) o[c] = 0.f;
        }
        *reinterpret_cast<float4*>(p.g + i * p.ldg + f) = make_float4(o[0], o[1], o[2], o[3]);
        if (SCALED) *reinterpret_cast<float4*>(p.s + i * p.lds + f) = make_float4(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv);
      }
    }
  }
}

// ---- backward row pass of the attention convs (gat, gatv2): g from (pre, dy), r = <g, pre - bias> per virtual row (i, h) ----
struct RowParams {
  const float* pre; int64_t ldp;
  const float* gy; int64_t ldgy;
  const float* bias;
  int64_t n_rows; int32_t H; int32_t C; int32_t npad;
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  float* g; int64_t ldg;
  float* r;                                        // [n_rows, H]
  const int64_t* row_id;                           // ROW_ID: dropout row of row i (a rank's rows of a partition); NULL: row i itself
};

template <int LF, int EPI, bool ROW_ID = false>
static __global__ __launch_bounds__(256) void attn_bwd_rows_kernel(RowParams p) {
  constexpr int RPB = 256 / LF;
  const int q = threadIdx.x / LF;
  const int k0 = (threadIdx.x % LF) * 4;
  const bool vec = (p.C & 3) == 0;
  uint64_t seed = p.seed;
  if (EPI == EPI_ELU && p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;
  const int64_t nv = p.n_rows * p.H;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < nv; base += (int64_t)gridDim.x * RPB) {   // block-uniform trip count
    const int64_t v = base + q;
    const bool valid = v < nv;
    const int64_t i = valid ? v / p.H : 0;
    const int h = valid ? (int)(v - i * p.H) : 0;
    const int64_t hoff = (int64_t)h * p.C;
    float pr[4], dy[4], b[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    load4(p.pre + i * p.ldp + hoff, k0, p.C, vec, valid, pr);
    load4(p.gy + i * p.ldgy + hoff, k0, p.C, vec, valid, dy);
    if (p.bias != nullptr) load4(p.bias + hoff, k0, p.C, vec, true, b);
    if (EPI == EPI_ELU) {
      const uint64_t e = (uint64_t)(ROW_ID ? (valid ? p.row_id[i] : 0) : i) * (uint64_t)(p.H * p.C) + (uint64_t)(hoff + k0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        // the mask is redrawn, never read off y: ELU is 0 at a pre-activation of exactly 0, kept or not
        const float mk = p.thr == 0u ? 1.f : (drop_bits(e + c, seed) >= p.thr ? p.keep_scale : 0.f);
        o[c] = dy[c] * mk * (pr[c] > 0.f ? 1.f : expf(pr[c]));
      }
    } else if (EPI == EPI_LOGSOFTMAX) {
      float m = -INFINITY;
#pragma unroll
      for (int c = 0; c < 4; ++c) if (k0 + c < p.C) m = fmaxf(m, pr[c]);
      m = bgnn::group_max<LF>(m);
      float se = 0.f, t = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) if (k0 + c < p.C) { se += expf(pr[c] - m); t += dy[c]; }
      se = bgnn::group_sum<LF>(se);
      t = bgnn::group_sum<LF>(t);
      const float lse = m + logf(se);
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = dy[c] - expf(pr[c] - lse) * t;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = dy[c];
    }
    float rr = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (k0 + c >= p.C) o[c] = 0.f;
      rr += o[c] * (pr[c] - b[c]);
    }
    rr = bgnn::group_sum<LF>(rr);
    if (valid) {
      store4(p.g + i * p.ldg + hoff, k0, p.C, vec, o);
      if (k0 == 0) {
        p.r[v] = rr;
        if (h == p.H - 1)
          for (int c = 0; c < p.npad; ++c) p.g[i * p.ldg + (int64_t)p.H * p.C + c] = 0.f;
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// Grid of a persistent kernel of 256-thread blocks: what stays resident (at most 8 blocks per CU), in multiples of the 8 XCDs,
// no more than the tiles need.  `cap_cache` is a zero-initialised static of the calling instantiation: one query per kernel.
template <typename K>
int persistent_grid(K kernel, int64_t ntiles, int* cap_cache) {
  if (*cap_cache == 0) {
    int per_cu = 0, dev = 0, cap = 2048;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) == hipSuccess && per_cu >= 1) {
      if (per_cu > 8) per_cu = 8;
      cap = per_cu * prop.multiProcessorCount / 8 * 8;
      if (cap < 8) cap = 8;
    }
    __atomic_store_n(cap_cache, cap, __ATOMIC_RELEASE);
  }
  const int cap = __atomic_load_n(cap_cache, __ATOMIC_ACQUIRE);
  int64_t grid = ntiles < cap ? (ntiles + 7) / 8 * 8 : cap;     // multiple of 8 (XCD split)
  if (grid < 8) grid = 8;
  return (int)grid;
}

// The (LF, EP, U) of a row of nv float4 slots, handed to f as integral constants: f(LF, EP, U) launches that instantiation.
template <int V> using int_c = std::integral_constant<int, V>;
template <class F>
int lf_ladder(int nv, F&& f) {
  if (nv <= 1) return f(int_c<1>{}, int_c<8>{}, int_c<4>{});
  if (nv <= 2) return f(int_c<2>{}, int_c<4>{}, int_c<4>{});
  if (nv <= 4) return f(int_c<4>{}, int_c<2>{}, int_c<4>{});
  if (nv <= 8) return f(int_c<8>{}, int_c<1>{}, int_c<8>{});
  if (nv <= 16) return f(int_c<16>{}, int_c<1>{}, int_c<8>{});
  return f(int_c<32>{}, int_c<1>{}, int_c<8>{});
}

// f(EPI) with the epilogue code as an integral constant
template <class F>
int epi_switch(int epilogue, F&& f) {
  return epilogue == EPI_ACT ? f(int_c<EPI_ACT>{}) : epilogue == EPI_LOGSOFTMAX ? f(int_c<EPI_LOGSOFTMAX>{}) : f(int_c<EPI_NONE>{});
}

template <int LF, int EPI, bool SCALED>
int launch_bwd_rows(const BwdRowsParams& p, hipStream_t st) {
  constexpr int RPB = 256 / LF;
  int64_t grid = (p.n_rows + RPB - 1) / RPB;
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((conv_bwd_rows_kernel<LF, EPI, SCALED>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <bool SCALED>
int dispatch_bwd_rows(int epilogue, const BwdRowsParams& p, hipStream_t st) {
  return epi_switch(epilogue, [&](auto EPI) {
    return lf_ladder((p.D + 3) / 4, [&](auto LF, auto, auto) { return launch_bwd_rows<LF, EPI, SCALED>(p, st); });
  });
}

template <int LF, int EPI, bool ROW_ID = false>
int launch_rows(const RowParams& p, hipStream_t st) {
  constexpr int RPB = 256 / LF;
  int64_t grid = (p.n_rows * p.H + RPB - 1) / RPB;
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((attn_bwd_rows_kernel<LF, EPI, ROW_ID>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

inline int dispatch_rows(int epilogue, const RowParams& p, hipStream_t st) {
  if (epilogue == EPI_ELU && p.row_id != nullptr && p.thr != 0u)   // the ids matter only where the mask is redrawn
    return lf_ladder((p.C + 3) / 4, [&](auto LF, auto, auto) { return launch_rows<LF, EPI_ELU, true>(p, st); });
  return epi_switch(epilogue, [&](auto EPI) {
    return lf_ladder((p.C + 3) / 4, [&](auto LF, auto, auto) { return launch_rows<LF, EPI>(p, st); });
  });
}

// a leading dimension that holds D columns padded to float4
inline bool ld_ok(int64_t ld, int32_t D) { return ld >= ((int64_t)D + 3) / 4 * 4 && (ld & 3) == 0; }

// the (epilogue, p_drop, D) part of an entry point's shape check: a known code, 0 <= p_drop < 1, dropout only after the
// activation, log_softmax only over a row of one slice
inline int epi_check(int epilogue, float p_drop, int32_t D) {
  if (epilogue < 0 || epilogue > 2 || !(p_drop >= 0.f && p_drop < 1.f)) return BGNN_E_SHAPE;
  if (epilogue == EPI_LOGSOFTMAX && D > SLICE) return BGNN_E_SHAPE;
  if (p_drop > 0.f && epilogue != EPI_ACT) return BGNN_E_SHAPE;
  return 0;
}

// a [rows, H*C] table whose head slices the kernels touch: leading dimension >= pad4(H*C), a multiple of 4, 16-byte aligned base
inline bool tbl_ok(const float* t, int64_t ld, int32_t HC) { return bgnn_aligned16(t) && ld_ok(ld, HC); }

inline bool shape_ok(int32_t H, int32_t C) { return H >= 1 && H <= MAX_HEADS && C >= 1 && C <= MAX_C; }

// attention dropout: the threshold of the shared hash, but the kept coefficients are scaled by exactly 1/(1 - p) as F.dropout does
// (drop_consts scales by the reciprocal of the quantised keep probability, 1.5e-5 away at p = 0.6)
inline void att_drop_consts(float p_att, uint32_t& thr, float& scale) {
  drop_consts(p_att, thr, scale);
  if (p_att > 0.f) scale = 1.f / (1.f - p_att);
}

inline size_t coef_bytes(int64_t n_edges, int32_t H) { return bgnn_align_up((size_t)n_edges * (size_t)H * sizeof(float), 16); }

}  // namespace bgnn_conv
