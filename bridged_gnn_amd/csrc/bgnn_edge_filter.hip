// Edge-validity filters of step 1 (main_bridged_graph.py:123-161, :225-264) without [E, F] / [E, k] temporaries:
//   quantile : exact `e_sim.quantile(q)` (:135, :238) by radix selection over the order-preserving uint32 image of the fp32
//              values -- four 8-bit histogram passes that follow BOTH order statistics around q (n - 1), then torch's lerp.
//              No sort, no size limit (torch.quantile stops at 2^24 elements), no host synchronisation; integer histograms,
//              so two calls are bitwise equal.
//   inv norms: 1 / max(|x_i|, eps) per node row, one pass (F.cosine_similarity divides each row by max(norm, eps), :149, :252).
//   validity : ONE launch over the coalesced edge list: a group of 16 lanes per edge gathers the two feature rows (16-byte loads
//              when F % 4 == 0), forms the fp32 dot, scales it by the two inverse norms and evaluates the label rules from per-node
//              vectors; it writes one flag byte (bit r-1 = removed by rule r, r = 2..5) and the edge's similarity (looked up among
//              the k entries of its query row).  Consecutive edges of a coalesced list share the `from` row, which the 4 groups
//              of a wave then read from the same cache lines.
//   rule 1   : after the quantile of the per-edge similarities is known (on the device), a streaming launch ORs bit 0 into the
//              flags and accumulates the five cumulative removal counts the reference prints (:138-152, :241-255).
// Gather-bound: 2 * 4 F bytes read per edge (1.2 KB rows at F = 300), 5 bytes written.
#include "bgnn_common.h"

namespace {

constexpr int NT = 256;
constexpr int G = 16;                  // lanes per edge / per row: one DPP row, so group_sum<16> never leaves the group
constexpr int MAX_BLOCKS = 4096;       // 16 resident 256-thread blocks' worth of gathers per CU

// ---- radix select ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t key_of(float v) {
  uint32_t b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;        // -0 and +0 compare equal: one key (returned as +0)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

constexpr int SEL_PASSES = 4;
constexpr size_t SEL_HIST_WORDS = (size_t)SEL_PASSES * 2 * 256;
// workspace: uint32 hist[4][2][256], then unsigned long long state[4][4] = {prefix of rank 0, prefix of rank 1, rank 0, rank 1}
// (the state ENTERING pass p: key bits above the pass's digit, and the rank among the keys that share them)
constexpr size_t SEL_WS_BYTES = SEL_HIST_WORDS * sizeof(uint32_t) + SEL_PASSES * 4 * sizeof(unsigned long long);

// state entering `pass` into LDS `s`, by every block alike: pass 0 from the arguments, later ones from the previous pass's entering
// state and its finished histogram
__device__ __forceinline__ void select_state(int pass, int64_t r0, int64_t r1, const uint32_t* hist, const unsigned long long* st,
                                             uint32_t (*h)[256], unsigned long long* s) {
  if (pass == 0) {
    if (threadIdx.x == 0) { s[0] = 0; s[1] = 0; s[2] = (unsigned long long)r0; s[3] = (unsigned long long)r1; }
  } else {
    const uint32_t* hp = hist + (size_t)(pass - 1) * 512;
    for (int t = threadIdx.x; t < 512; t += NT) h[t >> 8][t & 255] = hp[t];
    __syncthreads();
    if (threadIdx.x < 2) {
      const int r = threadIdx.x;
      const unsigned long long prefix = st[(pass - 1) * 4 + r];
      unsigned long long rank = st[(pass - 1) * 4 + 2 + r], cum = 0;
      int d = 0;
      for (; d < 255; ++d) {
        const unsigned long long c = h[r][d];
        if (rank < cum + c) break;
        cum += c;
      }
      s[r] = (prefix << 8) | (unsigned long long)d;
      s[2 + r] = rank - cum;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(NT) void select_pass_kernel(const float* __restrict__ v, int64_t n, int pass, int64_t r0, int64_t r1,
                                                         uint32_t* hist, unsigned long long* st) {
  __shared__ uint32_t h[2][256];
  __shared__ unsigned long long s[4];
  select_state(pass, r0, r1, hist, st, h, s);
  const uint32_t p0 = (uint32_t)s[0], p1 = (uint32_t)s[1];
  if (blockIdx.x == 0 && threadIdx.x < 4) st[pass * 4 + threadIdx.x] = s[threadIdx.x];
  __syncthreads();
  for (int t = threadIdx.x; t < 512; t += NT) h[t >> 8][t & 255] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const bool same = p0 == p1;          // the two ranks still share their prefix: one histogram serves both
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
    const uint32_t key = key_of(v[i]);
    const uint32_t hi = (uint32_t)((uint64_t)key >> (shift + 8)), d = (key >> shift) & 255u;
    if (hi == p0) atomicAdd(&h[0][d], 1u);
    if (!same && hi == p1) atomicAdd(&h[1][d], 1u);
  }
  __syncthreads();
  uint32_t* hp = hist + (size_t)pass * 512;
  for (int t = threadIdx.x; t < 512; t += NT) {
    const uint32_t c = h[same ? 0 : (t >> 8)][t & 255];
    if (c != 0u) atomicAdd(&hp[t], c);
  }
}

// the two order statistics from the last histogram, then torch's lerp (ATen/native/Lerp.h: two-sided form, contracted to fma)
__global__ __launch_bounds__(NT) void select_finish_kernel(int64_t r0, int64_t r1, float w, const uint32_t* hist,
                                                           const unsigned long long* st, float* out) {
  __shared__ uint32_t h[2][256];
  __shared__ unsigned long long s[4];
  select_state(SEL_PASSES, r0, r1, hist, st, h, s);
  if (threadIdx.x == 0) {
    const float a = value_of((uint32_t)s[0]), b = value_of((uint32_t)s[1]);
    const float diff = b - a;
    out[0] = w < 0.5f ? __builtin_fmaf(w, diff, a) : __builtin_fmaf(-diff, 1.f - w, b);
  }
}

// ---- per-row inverse norms ---------------------------------------------------------------------------------------------------------
template <bool VEC4>
__device__ __forceinline__ float group_dot(const float* __restrict__ ra, const float* __restrict__ rb, int F, int lane) {
  float acc = 0.f;
  if constexpr (VEC4) {
    const float4* va = reinterpret_cast<const float4*>(ra);
    const float4* vb = reinterpret_cast<const float4*>(rb);
    const int nv = F >> 2;
#pragma unroll 2
    for (int c = lane; c < nv; c += G) {
      const float4 u = va[c], w = vb[c];
      acc = fmaf(u.x, w.x, acc); acc = fmaf(u.y, w.y, acc); acc = fmaf(u.z, w.z, acc); acc = fmaf(u.w, w.w, acc);
    }
  } else {
#pragma unroll 2
    for (int c = lane; c < F; c += G) acc = fmaf(ra[c], rb[c], acc);
  }
  return bgnn::group_sum<G>(acc);
}

template <bool VEC4>
__global__ __launch_bounds__(NT) void row_inv_norms_kernel(const float* __restrict__ x, int64_t N, int F, float eps, float* __restrict__ out) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t step = (int64_t)gridDim.x * (NT / G);
  for (int64_t r = (int64_t)blockIdx.x * (NT / G) + threadIdx.x / G; r < N; r += step) {
    const float* row = x + r * (int64_t)F;
    const float ss = group_dot<VEC4>(row, row, F, lane);
    if (lane == 0) out[r] = 1.f / fmaxf(sqrtf(ss), eps);
  }
}

// ---- fused validity pass -----------------------------------------------------------------------------------------------------------
struct EdgeParams {
  const int64_t* e0; const int64_t* e1; int64_t E;
  const float* xa; int64_t na; const float* inva; const int32_t* preda; const int32_t* ya;
  const float* xb; int64_t nb; const float* invb; const int32_t* predb; const int32_t* yb; const uint8_t* trainb;
  int32_t F; int within; float thres;
  const int64_t* idx_mat; const float* sim_mat; int32_t k;
  float* sim_out; uint8_t* flags; unsigned long long* counts;
};

template <bool VEC4>
__global__ __launch_bounds__(NT) void edge_validity_kernel(EdgeParams p) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t step = (int64_t)gridDim.x * (NT / G);
  for (int64_t e = (int64_t)blockIdx.x * (NT / G) + threadIdx.x / G; e < p.E; e += step) {
    const int64_t a = p.e0[e], b = p.e1[e];
    if (a < 0 || a >= p.na || b < 0 || b >= p.nb) {            // never dereferenced: reported through counts[6]
      if (lane == 0) {
        atomicAdd(&p.counts[6], 1ull);
        p.flags[e] = 0x1Eu;
        if (p.sim_out != nullptr) p.sim_out[e] = 0.f;
      }
      continue;
    }
    const float dot = group_dot<VEC4>(p.xa + a * (int64_t)p.F, p.xb + b * (int64_t)p.F, p.F, lane);
    const float cosv = dot * p.inva[a] * p.invb[b];
    const int32_t pa = p.preda[a], pb = p.predb[b];
    const bool tm = p.trainb[b] != 0;
    const bool wrong_a = pa != p.ya[a], wrong_b = pb != p.yb[b];
    uint32_t f = 0u;
    if (p.within ? (wrong_a && tm) : wrong_a) f |= 2u;        // :140 (masked by train_mask[e1]) / :243 (unconditional)
    if (wrong_b && tm) f |= 4u;                                // :141 / :244
    if (pa != pb) f |= 8u;                                     // :145 / :248
    if (cosv < p.thres) f |= 16u;                              // :150 / :253
    if (p.idx_mat != nullptr) {                                // the edge's similarity: position of `from` in its query's top-k row
      const int64_t* cand = p.idx_mat + b * (int64_t)p.k;
      int pos = 0x7FFFFFFF;
      for (int j = lane; j < p.k; j += G)
        if (cand[j] == a && j < pos) pos = j;
#pragma unroll
      for (int m = G / 2; m >= 1; m >>= 1) {
        const int o = __shfl_xor(pos, m, G);
        pos = o < pos ? o : pos;
      }
      if (lane == 0) {
        float s = 0.f;
        if (pos == 0x7FFFFFFF) atomicAdd(&p.counts[5], 1ull);   // not an edge of these tables: the host raises
        else s = p.sim_mat[b * (int64_t)p.k + pos];
        p.sim_out[e] = s;
      }
    }
    if (lane == 0) p.flags[e] = (uint8_t)f;
  }
}

__global__ __launch_bounds__(NT) void edge_rule1_counts_kernel(const float* __restrict__ sim, const float* __restrict__ thres, int64_t E,
                                                               uint8_t* __restrict__ flags, unsigned long long* counts) {
  const float t = thres[0];
  uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < E; e += (int64_t)gridDim.x * NT) {
    uint32_t f = flags[e];
    if (sim[e] < t) {                                          // :136 / :239
      f |= 1u;
      flags[e] = (uint8_t)f;
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) c[r] += (f & ((2u << r) - 1u)) != 0u ? 1u : 0u;
  }
  __shared__ uint32_t red[NT / 64][5];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    uint32_t v = c[r];
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][r] = v;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    unsigned long long s = 0;
    for (int w = 0; w < NT / 64; ++w) s += red[w][threadIdx.x];
    if (s != 0) atomicAdd(&counts[threadIdx.x], s);
  }
}

int grid_for(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g > MAX_BLOCKS) g = MAX_BLOCKS;
  return g < 1 ? 1 : (int)g;
}

}  // namespace

extern "C" size_t bgnn_quantile_workspace_bytes(int64_t n) {
  (void)n;
  return SEL_WS_BYTES;
}

extern "C" int bgnn_quantile_f32(const float* values, int64_t n, double q, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!values || !out || !ws) return BGNN_E_NULL;
  if (n < 1 || n > 2147483647LL) return BGNN_E_SHAPE;
  if (!(q >= 0.0 && q <= 1.0)) return BGNN_E_RANGE;
  if (ws_bytes < SEL_WS_BYTES) return BGNN_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws) & 7u) != 0) return BGNN_E_ALIGN;
  // position q (n - 1): torch.quantile forms it in fp32 (q and the product both rounded), exact while n - 1 <= 2^24, which is
  // also where torch stops; beyond that fp32 cannot name every rank, so the position is formed in fp64
  int64_t r0, r1;
  float w;
  if (n - 1 <= (1 << 24)) {
    const float pos = (float)q * (float)(n - 1);
    const float lo = floorf(pos);
    r0 = (int64_t)lo; r1 = (int64_t)ceilf(pos); w = pos - lo;
  } else {
    const double pos = q * (double)(n - 1);
    const double lo = floor(pos);
    r0 = (int64_t)lo; r1 = (int64_t)ceil(pos); w = (float)(pos - lo);
  }
  if (r0 > n - 1) r0 = n - 1;
  if (r1 > n - 1) r1 = n - 1;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* hist = (uint32_t*)ws;
  unsigned long long* state = (unsigned long long*)(hist + SEL_HIST_WORDS);
  if (bgnn_zero_async(hist, SEL_HIST_WORDS * sizeof(uint32_t), st) != hipSuccess) return (int)hipErrorInvalidValue;
  const int grid = grid_for(n, NT * 8);
  for (int pass = 0; pass < SEL_PASSES; ++pass) {
    hipLaunchKernelGGL(select_pass_kernel, dim3(grid), dim3(NT), 0, st, values, n, pass, r0, r1, hist, state);
    BGNN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(NT), 0, st, r0, r1, w, hist, state, out);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_row_inv_norms_f32(const float* x, int64_t N, int32_t F, float eps, float* out, void* stream) {
  if (!x || !out) return BGNN_E_NULL;
  if (N < 0 || F <= 0) return BGNN_E_SHAPE;
  if (N == 0) return 0;
  const int grid = grid_for(N, NT / G);
  if ((F & 3) == 0 && bgnn_aligned16(x))
    hipLaunchKernelGGL(row_inv_norms_kernel<true>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, x, N, (int)F, eps, out);
  else
    hipLaunchKernelGGL(row_inv_norms_kernel<false>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, x, N, (int)F, eps, out);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_edge_validity_f32(const int64_t* edge_index, int64_t E, const float* x_from, int64_t n_from, const float* inv_from,
                                      const int32_t* pred_from, const int32_t* y_from, const float* x_to, int64_t n_to,
                                      const float* inv_to, const int32_t* pred_to, const int32_t* y_to, const uint8_t* train_to,
                                      int32_t F, int within, float thres_feat_sim, const int64_t* idx_mat_opt,
                                      const float* e_sim_mat_opt, int32_t k, float* sim_out_opt, uint8_t* flags, long long* counts,
                                      void* stream) {
  if (!edge_index || !x_from || !inv_from || !pred_from || !y_from || !x_to || !inv_to || !pred_to || !y_to || !train_to || !flags ||
      !counts)
    return BGNN_E_NULL;
  if ((idx_mat_opt != nullptr) && (!e_sim_mat_opt || !sim_out_opt)) return BGNN_E_NULL;
  if (E < 0 || E > 2147483647LL || n_from < 0 || n_to < 0 || F <= 0 || (idx_mat_opt != nullptr && k <= 0)) return BGNN_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (bgnn_zero_async(counts, 8 * sizeof(long long), st) != hipSuccess) return (int)hipErrorInvalidValue;
  if (E == 0) return 0;
  EdgeParams p{};
  p.e0 = edge_index; p.e1 = edge_index + E; p.E = E;
  p.xa = x_from; p.na = n_from; p.inva = inv_from; p.preda = pred_from; p.ya = y_from;
  p.xb = x_to; p.nb = n_to; p.invb = inv_to; p.predb = pred_to; p.yb = y_to; p.trainb = train_to;
  p.F = F; p.within = within; p.thres = thres_feat_sim;
  p.idx_mat = idx_mat_opt; p.sim_mat = e_sim_mat_opt; p.k = k;
  p.sim_out = sim_out_opt; p.flags = flags; p.counts = (unsigned long long*)counts;
  const int grid = grid_for(E, NT / G);
  if ((F & 3) == 0 && bgnn_aligned16(x_from) && bgnn_aligned16(x_to))
    hipLaunchKernelGGL(edge_validity_kernel<true>, dim3(grid), dim3(NT), 0, st, p);
  else
    hipLaunchKernelGGL(edge_validity_kernel<false>, dim3(grid), dim3(NT), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_edge_rule1_counts_f32(const float* sim, const float* thres, int64_t E, uint8_t* flags, long long* counts,
                                          void* stream) {
  if (!sim || !thres || !flags || !counts) return BGNN_E_NULL;
  if (E < 0 || E > 2147483647LL) return BGNN_E_SHAPE;
  if (E == 0) return 0;
  hipLaunchKernelGGL(edge_rule1_counts_kernel, dim3(grid_for(E, NT * 8)), dim3(NT), 0, (hipStream_t)stream, sim, thres, E, flags,
                     (unsigned long long*)counts);
  BGNN_LAUNCH_CHECK();
  return 0;
}
