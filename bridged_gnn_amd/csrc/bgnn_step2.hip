// Step 2's loss and metric counts (main_graph_knowledge_transfer.py:39-142, :265-300) as streaming passes over the three narrow
// log-probability tables lp_s, lp_t, lp_t^ [N, C] (fp32, row stride given, unit column stride, any C >= 1, no alignment needed).
//   loss:   L = (2 nll(lp_s | train) + nll(lp_t | train & ~central) + nll(lp_t^ | train & ~central)) / 4
//               + Lambda * sum_{r,c} exp(lp_t)(lp_t - lp_t^) / N                                   (:44-54), forward and backward;
//   nll:    nll(lp | mask), the loss of train_noDTC (:269), forward and backward;
//   counts: per-row argmax (ties -> lowest index) and int64 confusion counts [true, predicted] per (table, row selection);
//   auc:    the integer rank statistic of roc_auc_score over (positive row, sorted negative scores): ties count 1/2.
// Layout as in bgnn_norm.hip: GL = min(32, next power of two >= C) consecutive lanes own one row, lane l reads columns l, l + GL,
// ...: a wave reads 64 / GL consecutive rows, no tiling.  Loss sums are fp64 and reduced in a fixed order (lanes of a block by
// an LDS tree, blocks by one finishing block), the grid depends on N and C only: run-to-run identical, no atomics, and the
// partials are written, never accumulated, so nothing needs clearing.  The counts are integers (order-independent): LDS
// atomics per block, then one global atomic per non-zero cell; the output is cleared by bgnn_zero_async (a kernel, not a memset
// node: see bgnn_common.h), so every pass here is safe inside a captured training step.
#include "bgnn_common.h"

namespace {

constexpr int S2_MAX_BLOCKS = 1024;
constexpr int LOSS_W = 6;              // per block: -sum lp_s[y], -sum lp_t[y], -sum lp_t^[y], KL sum, #train, #train & ~central
constexpr int NLL_W = 2;               // per block: -sum lp[y], #mask
constexpr int CNT_LDS_MAX = 12288;     // int32 cells of a block's LDS histogram (48 KiB); larger K C^2 goes to global atomics
constexpr int CNT_ROWS_PER_BLOCK_MIN = 8;

inline int s2_group(int C) {
  int g = 1;
  while (g < C && g < 32) g <<= 1;
  return g;
}

inline int s2_blocks(int64_t N, int GL, int iters = 1) {
  const int64_t per = (int64_t)(256 / GL) * iters;
  const int64_t b = (N + per - 1) / per;
  return (int)(b < S2_MAX_BLOCKS ? (b < 1 ? 1 : b) : S2_MAX_BLOCKS);
}

// fixed-order sum of W per-thread doubles over the 256 threads of a block -> dst[0..W)
template <int W>
__device__ __forceinline__ void block_sum_store(const double (&v)[W], double* __restrict__ red, double* __restrict__ dst) {
  const int t = threadIdx.x;
#pragma unroll
  for (int w = 0; w < W; ++w) red[w * 256 + t] = v[w];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int w = 0; w < W; ++w) red[w * 256 + t] += red[w * 256 + t + o];
    }
    __syncthreads();
  }
  if (t < W) dst[t] = red[t * 256];
}

// fixed-order sum of the blocks' partials part[nblk][W] by one 256-thread block -> tot[0..W) in LDS (valid for every thread after return)
template <int W>
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int nblk, double* __restrict__ red, double* __restrict__ tot) {
  const int t = threadIdx.x;
  double v[W];
#pragma unroll
  for (int w = 0; w < W; ++w) v[w] = 0.0;
  for (int b = t; b < nblk; b += 256) {
#pragma unroll
    for (int w = 0; w < W; ++w) v[w] += part[(int64_t)b * W + w];
  }
  block_sum_store<W>(v, red, tot);
  __syncthreads();
}

// ---- 1. the three-table loss ----------------------------------------------------------------------------------------------
template <int GL>
__global__ __launch_bounds__(256) void s2_loss_fwd_kernel(const float* __restrict__ S, int64_t ld_s, const float* __restrict__ T, int64_t ld_t,
                                                          const float* __restrict__ H, int64_t ld_h, int64_t N, int C,
                                                          const int64_t* __restrict__ y, const uint8_t* __restrict__ train,
                                                          const uint8_t* __restrict__ central, double* __restrict__ part) {
  __shared__ double red[LOSS_W * 256];
  constexpr int RPB = 256 / GL;
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  double acc[LOSS_W];
#pragma unroll
  for (int w = 0; w < LOSS_W; ++w) acc[w] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * RPB + g; r < N; r += (int64_t)gridDim.x * RPB) {
    const float* t = T + r * ld_t;
    const float* h = H + r * ld_h;
    double kl = 0.0;
    for (int c = l; c < C; c += GL) {
      const double tv = (double)t[c], hv = (double)h[c];
      kl += exp(tv) * (tv - hv);
    }
    acc[3] += kl;
    if (l == 0 && train[r]) {
      const int64_t yy = y[r];
      if (yy >= 0 && yy < C) {                         // a label outside [0, C) selects nothing (the driver refuses it at set-up)
        acc[0] -= (double)S[r * ld_s + yy];
        acc[4] += 1.0;
        if (!central[r]) {
          acc[1] -= (double)t[yy];
          acc[2] -= (double)h[yy];
          acc[5] += 1.0;
        }
      }
    }
  }
  block_sum_store<LOSS_W>(acc, red, part + (int64_t)blockIdx.x * LOSS_W);
}

// terms[8]: total, nll_s, nll_t, nll_t^, KL (batchmean, without Lambda), #train, #train & ~central, 0.  An empty selection gives
// 0 / 0 = NaN for its mean, as F.nll_loss does.
__global__ __launch_bounds__(256) void s2_loss_finish_kernel(const double* __restrict__ part, int nblk, int64_t N, double lambda,
                                                             double* __restrict__ terms) {
  __shared__ double red[LOSS_W * 256];
  __shared__ double tot[LOSS_W];
  sum_partials<LOSS_W>(part, nblk, red, tot);
  if (threadIdx.x == 0) {
    const double nll_s = tot[0] / tot[4], nll_t = tot[1] / tot[5], nll_h = tot[2] / tot[5], kl = tot[3] / (double)N;
    terms[0] = (nll_s * 2.0 + nll_t + nll_h) / 4.0 + kl * lambda;
    terms[1] = nll_s; terms[2] = nll_t; terms[3] = nll_h; terms[4] = kl; terms[5] = tot[4]; terms[6] = tot[5]; terms[7] = 0.0;
  }
}

// dL/dlp_s = -g/2 [train, c = y] / #train;  dL/dlp_t = -g/4 [tt, c = y] / #tt + g Lambda exp(lp_t)(lp_t - lp_t^ + 1) / N;
// dL/dlp_t^ = -g/4 [tt, c = y] / #tt - g Lambda exp(lp_t) / N   (tt = train & ~central).  Every element of the
// three gradient tables is written.
template <int GL>
__global__ __launch_bounds__(256) void s2_loss_bwd_kernel(const float* __restrict__ T, int64_t ld_t, const float* __restrict__ H, int64_t ld_h,
                                                          int64_t N, int C, const int64_t* __restrict__ y, const uint8_t* __restrict__ train,
                                                          const uint8_t* __restrict__ central, const double* __restrict__ terms,
                                                          const float* __restrict__ gout, double lambda, float* __restrict__ GS,
                                                          float* __restrict__ GT, float* __restrict__ GH, int64_t ld_g) {
  constexpr int RPB = 256 / GL;
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  const double go = (double)gout[0];
  const double cs = -go * 0.5 / terms[5], ct = -go * 0.25 / terms[6], ck = go * lambda / (double)N;
  for (int64_t r = (int64_t)blockIdx.x * RPB + g; r < N; r += (int64_t)gridDim.x * RPB) {
    const float* t = T + r * ld_t;
    const float* h = H + r * ld_h;
    int64_t yy = train[r] ? y[r] : -1;
    if (yy >= C) yy = -1;
    const bool tt = yy >= 0 && !central[r];
    for (int c = l; c < C; c += GL) {
      const double tv = (double)t[c], hv = (double)h[c];
      const double e = ck * exp(tv);
      const bool hit = c == yy;
      const double nt = (hit && tt) ? ct : 0.0;
      GS[r * ld_g + c] = hit ? (float)cs : 0.f;
      GT[r * ld_g + c] = (float)(e * (tv - hv + 1.0) + nt);
      GH[r * ld_g + c] = (float)(nt - e);
    }
  }
}

// ---- 2. the single-table loss ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void s2_nll_fwd_kernel(const float* __restrict__ P, int64_t ld, int64_t N, int C, const int64_t* __restrict__ y,
                                                         const uint8_t* __restrict__ mask, double* __restrict__ part) {
  __shared__ double red[NLL_W * 256];
  double acc[NLL_W] = {0.0, 0.0};
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) {
    if (!mask[r]) continue;
    const int64_t yy = y[r];
    if (yy < 0 || yy >= C) continue;
    acc[0] -= (double)P[r * ld + yy];
    acc[1] += 1.0;
  }
  block_sum_store<NLL_W>(acc, red, part + (int64_t)blockIdx.x * NLL_W);
}

__global__ __launch_bounds__(256) void s2_nll_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ terms) {
  __shared__ double red[NLL_W * 256];
  __shared__ double tot[NLL_W];
  sum_partials<NLL_W>(part, nblk, red, tot);
  if (threadIdx.x == 0) {
    terms[0] = tot[0] / tot[1];
    terms[1] = tot[1];
  }
}

template <int GL>
__global__ __launch_bounds__(256) void s2_nll_bwd_kernel(int64_t N, int C, const int64_t* __restrict__ y, const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ terms, const float* __restrict__ gout,
                                                         float* __restrict__ G, int64_t ld_g) {
  constexpr int RPB = 256 / GL;
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  const float cs = (float)(-(double)gout[0] / terms[1]);
  for (int64_t r = (int64_t)blockIdx.x * RPB + g; r < N; r += (int64_t)gridDim.x * RPB) {
    const int64_t yy = mask[r] ? y[r] : -1;
    for (int c = l; c < C; c += GL) G[r * ld_g + c] = (c == yy) ? cs : 0.f;
  }
}

// ---- 3. confusion counts --------------------------------------------------------------------------------------------------
// combos: byte k = table (bits 0-1) | selection bit (bits 2-4) of combination k < K <= 8; sel[r]: bit b = row r is in selection b.
template <int GL>
__device__ __forceinline__ int row_argmax(const float* __restrict__ row, int C, int l, bool valid) {
  float v = -INFINITY;
  int i = 0x7fffffff;
  if (valid) {
    for (int c = l; c < C; c += GL) {
      const float x = row[c];
      if (x > v) { v = x; i = c; }                       // strict: the lowest index of a lane's columns wins a tie
    }
  }
#pragma unroll
  for (int o = GL / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  return i < C ? i : 0;                                  // a row of -inf / NaN only: index 0
}

template <int GL>
__global__ __launch_bounds__(256) void s2_counts_kernel(const float* __restrict__ T0, int64_t ld0, const float* __restrict__ T1, int64_t ld1,
                                                        const float* __restrict__ T2, int64_t ld2, int64_t N, int C,
                                                        const int64_t* __restrict__ y, const uint8_t* __restrict__ sel, uint64_t combos,
                                                        int K, unsigned long long* __restrict__ counts, int use_lds) {
  extern __shared__ int lc[];
  constexpr int RPB = 256 / GL;
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  const int cells = K * C * C;
  if (use_lds) {
    for (int i = threadIdx.x; i < cells; i += 256) lc[i] = 0;
    __syncthreads();
  }
  // every lane of the block walks the same number of iterations: the shuffles of row_argmax run under a uniform loop
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < N; base += (int64_t)gridDim.x * RPB) {
    const int64_t r = base + g;
    const bool in = r < N;
    const int s = in ? sel[r] : 0;
    int need = 0;                                        // tables some combination reads on this row
    for (int k = 0; k < K; ++k) {
      const int cb = (int)((combos >> (8 * k)) & 0xff);
      if ((s >> ((cb >> 2) & 7)) & 1) need |= 1 << (cb & 3);
    }
    int pred[3];
    pred[0] = row_argmax<GL>(T0 ? T0 + (in ? r : 0) * ld0 : nullptr, C, l, (need & 1) && T0);       // no arithmetic on an unused (NULL) slot
    pred[1] = row_argmax<GL>(T1 ? T1 + (in ? r : 0) * ld1 : nullptr, C, l, (need & 2) && T1);
    pred[2] = row_argmax<GL>(T2 ? T2 + (in ? r : 0) * ld2 : nullptr, C, l, (need & 4) && T2);
    if (l == 0 && need) {
      const int64_t yy = y[r];
      if (yy >= 0 && yy < C) {
        for (int k = 0; k < K; ++k) {
          const int cb = (int)((combos >> (8 * k)) & 0xff);
          const int tb = cb & 3;
          if (tb > 2 || !((s >> ((cb >> 2) & 7)) & 1)) continue;
          const int cell = (k * C + (int)yy) * C + pred[tb];
          if (use_lds) atomicAdd(&lc[cell], 1);
          else atomicAdd(&counts[cell], 1ull);
        }
      }
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += 256) {
      const int v = lc[i];
      if (v) atomicAdd(&counts[i], (unsigned long long)v);
    }
  }
}

// ---- 4. AUC rank statistic ------------------------------------------------------------------------------------------------
// out[0] += sum over positive rows of 2 #{negatives with a smaller score} + #{negatives with an equal score}, out[1] += #positives.
// neg_sorted[0 .. *n_neg) are the negatives' scores in ascending order.
__global__ __launch_bounds__(256) void s2_auc_kernel(const float* __restrict__ score, const uint8_t* __restrict__ pos, int64_t N,
                                                     const float* __restrict__ neg_sorted, const int64_t* __restrict__ n_neg,
                                                     unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[2];
  if (threadIdx.x < 2) red[threadIdx.x] = 0ull;
  __syncthreads();
  int64_t nn = n_neg[0];
  nn = nn < 0 ? 0 : (nn > N ? N : nn);
  unsigned long long u2 = 0ull, np = 0ull;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) {
    if (!pos[r]) continue;
    const float s = score[r];
    int64_t lo = 0, hi = nn;                             // lower bound: first key >= s
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (neg_sorted[mid] < s) lo = mid + 1; else hi = mid;
    }
    const int64_t lb = lo;
    hi = nn;                                             // upper bound: first key > s
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (neg_sorted[mid] <= s) lo = mid + 1; else hi = mid;
    }
    u2 += (unsigned long long)(2 * lb + (lo - lb));
    np += 1ull;
  }
  if (u2) atomicAdd(&red[0], u2);
  if (np) atomicAdd(&red[1], np);
  __syncthreads();
  if (threadIdx.x < 2 && red[threadIdx.x]) atomicAdd(&out[threadIdx.x], red[threadIdx.x]);
}

#define S2_DISPATCH_GL(GL, CALL)  \
  switch (GL) {                   \
    case 1: { constexpr int G_ = 1; CALL; } break;   \
    case 2: { constexpr int G_ = 2; CALL; } break;   \
    case 4: { constexpr int G_ = 4; CALL; } break;   \
    case 8: { constexpr int G_ = 8; CALL; } break;   \
    case 16: { constexpr int G_ = 16; CALL; } break; \
    default: { constexpr int G_ = 32; CALL; } break; \
  }

bool table_ok(const float* t, int64_t ld, int C) { return t && ld >= C; }

}  // namespace

extern "C" size_t bgnn_step2_loss_workspace_bytes(int64_t N, int32_t C) {
  (void)N; (void)C;
  return (size_t)S2_MAX_BLOCKS * LOSS_W * sizeof(double);
}

extern "C" int bgnn_step2_loss_f32(const float* lp_s, int64_t ld_s, const float* lp_t, int64_t ld_t, const float* lp_h, int64_t ld_h,
                                   int64_t N, int32_t C, const int64_t* y, const uint8_t* train_mask, const uint8_t* central_mask,
                                   double lambda, double* terms, void* ws, size_t ws_bytes, void* stream) {
  if (!lp_s || !lp_t || !lp_h || !y || !train_mask || !central_mask || !terms || !ws) return BGNN_E_NULL;
  if (N <= 0 || C < 1 || !table_ok(lp_s, ld_s, C) || !table_ok(lp_t, ld_t, C) || !table_ok(lp_h, ld_h, C)) return BGNN_E_SHAPE;
  if (ws_bytes < bgnn_step2_loss_workspace_bytes(N, C)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int GL = s2_group(C), nblk = s2_blocks(N, GL);
  double* part = (double*)ws;
  S2_DISPATCH_GL(GL, hipLaunchKernelGGL(s2_loss_fwd_kernel<G_>, dim3(nblk), dim3(256), 0, st, lp_s, ld_s, lp_t, ld_t, lp_h, ld_h, N, (int)C,
                                        y, train_mask, central_mask, part));
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(s2_loss_finish_kernel, dim3(1), dim3(256), 0, st, part, nblk, N, lambda, terms);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_step2_loss_bwd_f32(const float* lp_t, int64_t ld_t, const float* lp_h, int64_t ld_h, int64_t N, int32_t C,
                                       const int64_t* y, const uint8_t* train_mask, const uint8_t* central_mask, double lambda,
                                       const double* terms, const float* grad_out, float* g_s, float* g_t, float* g_h, int64_t ld_g,
                                       void* stream) {
  if (!lp_t || !lp_h || !y || !train_mask || !central_mask || !terms || !grad_out || !g_s || !g_t || !g_h) return BGNN_E_NULL;
  if (N <= 0 || C < 1 || !table_ok(lp_t, ld_t, C) || !table_ok(lp_h, ld_h, C) || ld_g < C) return BGNN_E_SHAPE;
  const int GL = s2_group(C), nblk = s2_blocks(N, GL);
  S2_DISPATCH_GL(GL, hipLaunchKernelGGL(s2_loss_bwd_kernel<G_>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, lp_t, ld_t, lp_h, ld_h, N,
                                        (int)C, y, train_mask, central_mask, terms, grad_out, lambda, g_s, g_t, g_h, ld_g));
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_step2_nll_f32(const float* lp, int64_t ld, int64_t N, int32_t C, const int64_t* y, const uint8_t* mask, double* terms,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (!lp || !y || !mask || !terms || !ws) return BGNN_E_NULL;
  if (N <= 0 || C < 1 || ld < C) return BGNN_E_SHAPE;
  if (ws_bytes < bgnn_step2_loss_workspace_bytes(N, C)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = s2_blocks(N, 1);
  double* part = (double*)ws;
  hipLaunchKernelGGL(s2_nll_fwd_kernel, dim3(nblk), dim3(256), 0, st, lp, ld, N, (int)C, y, mask, part);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(s2_nll_finish_kernel, dim3(1), dim3(256), 0, st, part, nblk, terms);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_step2_nll_bwd_f32(int64_t N, int32_t C, const int64_t* y, const uint8_t* mask, const double* terms,
                                      const float* grad_out, float* g, int64_t ld_g, void* stream) {
  if (!y || !mask || !terms || !grad_out || !g) return BGNN_E_NULL;
  if (N <= 0 || C < 1 || ld_g < C) return BGNN_E_SHAPE;
  const int GL = s2_group(C), nblk = s2_blocks(N, GL);
  S2_DISPATCH_GL(GL, hipLaunchKernelGGL(s2_nll_bwd_kernel<G_>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, N, (int)C, y, mask, terms,
                                        grad_out, g, ld_g));
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_step2_counts_f32(const float* t0, int64_t ld0, const float* t1, int64_t ld1, const float* t2, int64_t ld2, int64_t N,
                                     int32_t C, const int64_t* y, const uint8_t* sel, uint64_t combos, int32_t K, long long* counts,
                                     void* stream) {
  if (!y || !sel || !counts) return BGNN_E_NULL;
  if (N <= 0 || C < 1 || K < 1 || K > 8 || (int64_t)K * C * C >= (1ll << 31)) return BGNN_E_SHAPE;
  const float* tabs[3] = {t0, t1, t2};
  const int64_t lds[3] = {ld0, ld1, ld2};
  for (int k = 0; k < K; ++k) {
    const int tb = (int)((combos >> (8 * k)) & 3);
    if (tb > 2 || !tabs[tb]) return BGNN_E_NULL;
    if (lds[tb] < C) return BGNN_E_SHAPE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t cells = (int64_t)K * C * C;
  hipError_t e = bgnn_zero_async(counts, (size_t)cells * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  const int GL = s2_group(C), nblk = s2_blocks(N, GL, CNT_ROWS_PER_BLOCK_MIN);
  const int use_lds = cells <= CNT_LDS_MAX;
  const size_t lds_bytes = use_lds ? (size_t)cells * sizeof(int) : 0;
  S2_DISPATCH_GL(GL, hipLaunchKernelGGL(s2_counts_kernel<G_>, dim3(nblk), dim3(256), lds_bytes, st, t0, ld0, t1, ld1, t2, ld2, N, (int)C, y,
                                        sel, combos, (int)K, (unsigned long long*)counts, use_lds));
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_step2_auc_count_f32(const float* score, const uint8_t* pos, int64_t N, const float* neg_sorted, const int64_t* n_neg,
                                        long long* out, void* stream) {
  if (!score || !pos || !neg_sorted || !n_neg || !out) return BGNN_E_NULL;
  if (N <= 0) return BGNN_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = bgnn_zero_async(out, 2 * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(s2_auc_kernel, dim3(s2_blocks(N, 1)), dim3(256), 0, st, score, pos, N, neg_sorted, n_neg, (unsigned long long*)out);
  BGNN_LAUNCH_CHECK();
  return 0;
}
