// Pair passes of the train-mode mlp similarity scorer, Similar_v2(mode='mlp') (models/models.py:913-920, :949-951, :967-970)
// under the BCE of train_adv_few_shot (scripts.py:36-50):
//   x_pair = [z1[idx1] || z2[idx2]] -> BN1 -> Linear(2H, 128) -> BN2 -> ReLU -> Linear(128, 1) -> sigmoid -> BCE.
// BN1 and the first Linear are per-node work (u_p = A[idx1[p]] + B[idx2[p]], formed by the caller); what is left per pair is
// BN2 with batch statistics, ReLU, the w2 dot, the sigmoid and the BCE, forward and backward.
//
// Layout: a pair (or a node's segment) is owned by 16 consecutive lanes; lane l of the group holds columns 4l..4l+3 and
// 64+4l..64+4l+3 of a 128-float row (two float4 loads; 16 lanes cover one 512-byte row contiguously).  A block has 16 groups.
// Column sums are kept per lane in fp64 and reduced in a fixed order: groups of a block through LDS, then blocks by one thread
// per column block (column_sum).  The grid of the pair passes depends on P only, so every sum is run-to-run identical.
#include "bgnn_common.h"

namespace {

constexpr int U = 128;                 // width of u (Linear(2H, 128), models.py:918)
constexpr int GL = 16;                 // lanes per pair / node
constexpr int GPB = 16;                // groups per block (256 threads)
constexpr int PM_MAX_BLOCKS = 1024;
constexpr int STAT_W = 2 * U;          // per block: sum u, sum u^2
constexpr int LOSS_W = 3 * U + 8;      // per block: sum dy, sum dy*xh, sum dl*h, then dl, bce, tp, fp, fn (+3 pad)
constexpr int EVAL_W = 4;              // tp, fp, fn (+1 pad)

__host__ __device__ inline int pm_blocks(int64_t P) {
  const int64_t b = (P + GPB - 1) / GPB;
  return (int)(b < PM_MAX_BLOCKS ? (b < 1 ? 1 : b) : PM_MAX_BLOCKS);
}

__device__ __forceinline__ int64_t clampi(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the 8 columns of lane l: c(j) = 4l + j for j < 4, 64 + 4l + (j - 4) for j >= 4
__device__ __forceinline__ int col_of(int l, int j) { return j < 4 ? 4 * l + j : 64 + 4 * l + (j - 4); }

__device__ __forceinline__ void load_row8(const float* __restrict__ row, int l, float v[8]) {
  const float4 a = *reinterpret_cast<const float4*>(row + 4 * l);
  const float4 b = *reinterpret_cast<const float4*>(row + 64 + 4 * l);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load_vec8(const float* __restrict__ p, int l, float v[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = p[col_of(l, j)];
}

// BN2 constants of lane l's columns from the fp64 batch statistics (mean, biased variance): torch's invstd = 1 / sqrt(var + eps)
__device__ __forceinline__ void bn2_consts(const double* __restrict__ stats, float eps, int l, float mean[8], float rstd[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = col_of(l, j);
    mean[j] = (float)stats[c];
    rstd[j] = (float)(1.0 / sqrt(stats[U + c] + (double)eps));
  }
}

// block partial: red[g][w] over the 16 groups in order -> part[blockIdx.x][w]
__device__ __forceinline__ void block_partials(double* red, int W, double* __restrict__ part) {
  __syncthreads();
  for (int w = threadIdx.x; w < W; w += blockDim.x) {
    double s = 0.0;
    for (int g = 0; g < GPB; ++g) s += red[g * W + w];
    part[(int64_t)blockIdx.x * W + w] = s;
  }
}

// ---- 1. batch statistics of BN2: sum u, sum u^2 per column ------------------------------------------------------------
__global__ __launch_bounds__(256) void pm_stats_kernel(const float* __restrict__ A, int64_t lda, int64_t nA, const float* __restrict__ B,
                                                       int64_t ldb, int64_t nB, const int64_t* __restrict__ idx1,
                                                       const int64_t* __restrict__ idx2, int64_t P, double* __restrict__ part) {
  __shared__ double red[GPB * STAT_W];
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  double s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * GPB + g; p < P; p += (int64_t)gridDim.x * GPB) {
    float a[8], b[8];
    load_row8(A + clampi(idx1[p], nA) * lda, l, a);
    load_row8(B + clampi(idx2[p], nB) * ldb, l, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double u = (double)(a[j] + b[j]);
      s[j] += u;
      q[j] += u * u;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[g * STAT_W + col_of(l, j)] = s[j];
    red[g * STAT_W + U + col_of(l, j)] = q[j];
  }
  block_partials(red, STAT_W, part);
}

// column c of the blocks' partials, summed by one 256-thread block in a fixed order (strided per-thread sums, then an LDS tree);
// the result is valid in thread 0
__device__ __forceinline__ double column_sum(const double* __restrict__ part, int nblk, int W, int c, double* red) {
  const int t = threadIdx.x;
  double s = 0.0;
  for (int b = t; b < nblk; b += 256) s += part[(int64_t)b * W + c];
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// blocks' partials -> mean and biased variance (fp64) + nn.BatchNorm1d's running update (unbiased variance, fp32 buffers);
// one block per column
__global__ __launch_bounds__(256) void pm_stats_finish_kernel(const double* __restrict__ part, int nblk, int64_t P, float momentum,
                                                              float* __restrict__ run_mean, float* __restrict__ run_var,
                                                              double* __restrict__ stats) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const double s = column_sum(part, nblk, STAT_W, c, red);
  const double q = column_sum(part, nblk, STAT_W, U + c, red);
  if (threadIdx.x != 0) return;
  const double mean = s / (double)P;
  const double var = fmax(q / (double)P - mean * mean, 0.0);
  stats[c] = mean;
  stats[U + c] = var;
  if (run_mean) run_mean[c] = (float)((1.0 - momentum) * (double)run_mean[c] + momentum * mean);
  if (run_var) run_var[c] = (float)((1.0 - momentum) * (double)run_var[c] + momentum * var * (double)P / (double)(P - 1));
}

// fixed-order column sums of the blocks' partials, one block per column
__global__ __launch_bounds__(256) void pm_sum_partials_kernel(const double* __restrict__ part, int nblk, int W, double* __restrict__ out) {
  __shared__ double red[256];
  const double s = column_sum(part, nblk, W, blockIdx.x, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- 2. forward to the loss and the logit gradient ---------------------------------------------------------------------
// x2 = (u - mean) * rstd; h = relu(g2 x2 + be2); logit = w2.h + b2; p = sigmoid(logit);
// bce_p = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100))   (torch's clamp);
// dl_p = [(p - y) / max((1 - p) p, 1e-12) / P] * (1 - p) * p      (torch's binary_cross_entropy_backward, then sigmoid_backward:
//        exactly 0 where p rounds to 0 or 1, like the reference's).
__global__ __launch_bounds__(256) void pm_loss_kernel(const float* __restrict__ A, int64_t lda, int64_t nA, const float* __restrict__ B,
                                                      int64_t ldb, int64_t nB, const int64_t* __restrict__ idx1,
                                                      const int64_t* __restrict__ idx2, const uint8_t* __restrict__ y, int64_t P,
                                                      const double* __restrict__ stats, const float* __restrict__ g2,
                                                      const float* __restrict__ be2, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, float eps, float* __restrict__ p_out,
                                                      float* __restrict__ dl_out, double* __restrict__ part) {
  __shared__ double red[GPB * LOSS_W];
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  float mean[8], rstd[8], gam[8], bet[8], w[8];
  bn2_consts(stats, eps, l, mean, rstd);
  load_vec8(g2, l, gam);
  load_vec8(be2, l, bet);
  load_vec8(w2, l, w);
  const float bias2 = b2[0];
  const float Pf = (float)P;
  double sdy[8], sdyx[8], sdlh[8], sdl = 0.0, sbce = 0.0, tp = 0.0, fp = 0.0, fn = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) sdy[j] = sdyx[j] = sdlh[j] = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * GPB + g; p < P; p += (int64_t)gridDim.x * GPB) {
    float a[8], b[8], xh[8], h[8];
    load_row8(A + clampi(idx1[p], nA) * lda, l, a);
    load_row8(B + clampi(idx2[p], nB) * ldb, l, b);
    float part_logit = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xh[j] = (a[j] + b[j] - mean[j]) * rstd[j];
      h[j] = fmaxf(fmaf(gam[j], xh[j], bet[j]), 0.f);       // explicit fma: the same pre-activation as segsum's ReLU mask
      part_logit = fmaf(w[j], h[j], part_logit);
    }
    const float logit = bgnn::group_sum<GL>(part_logit) + bias2;
    const float pr = 1.f / (1.f + expf(-logit));
    const float yy = y[p] ? 1.f : 0.f;
    float gr = (pr - yy) / fmaxf((1.f - pr) * pr, 1e-12f);
    gr = gr / Pf;
    const float dl = gr * (1.f - pr) * pr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dy = h[j] > 0.f ? dl * w[j] : 0.f;
      sdy[j] += (double)dy;
      sdyx[j] += (double)dy * (double)xh[j];
      sdlh[j] += (double)dl * (double)h[j];
    }
    const double lp = fmax(log((double)pr), -100.0), l1p = fmax(log1p(-(double)pr), -100.0);
    sbce -= (double)yy * lp + (1.0 - (double)yy) * l1p;
    sdl += (double)dl;
    const bool pos = pr > 0.5f;
    tp += (pos && yy == 1.f) ? 1.0 : 0.0;
    fp += (pos && yy == 0.f) ? 1.0 : 0.0;
    fn += (!pos && yy == 1.f) ? 1.0 : 0.0;
    if (l == 0) {
      p_out[p] = pr;
      dl_out[p] = dl;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = col_of(l, j);
    red[g * LOSS_W + c] = sdy[j];
    red[g * LOSS_W + U + c] = sdyx[j];
    red[g * LOSS_W + 2 * U + c] = sdlh[j];
  }
  if (l == 0) {
    double* r = red + g * LOSS_W + 3 * U;
    r[0] = sdl; r[1] = sbce; r[2] = tp; r[3] = fp; r[4] = fn; r[5] = r[6] = r[7] = 0.0;
  }
  block_partials(red, LOSS_W, part);
}

// ---- 3. per-node segment sums of du -----------------------------------------------------------------------------------
// S[n] = sum over the pairs p of node n's segment (CSR rowptr / perm = pair ids) of
//   du_p = g2 rstd (dy_p - sum(dy)/P - x2_p sum(dy x2)/P),  dy_p = dl_p w2 [g2 x2_p + be2 > 0],
// with u_p = own[n] + other[idx_other[p]] recomputed from the two per-node tables.  One group per node, fp64 accumulation in
// registers, every row written once (zeros for nodes no pair references): no atomics.
__global__ __launch_bounds__(256) void pm_segsum_kernel(const float* __restrict__ own, int64_t ld_own, int64_t n_own,
                                                        const float* __restrict__ other, int64_t ld_other, int64_t n_other,
                                                        const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ idx_other, int64_t P,
                                                        const float* __restrict__ dl, const double* __restrict__ stats,
                                                        const double* __restrict__ sums, const float* __restrict__ g2,
                                                        const float* __restrict__ be2, const float* __restrict__ w2, float eps,
                                                        float* __restrict__ S, int64_t ld_s) {
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  float mean[8], rstd[8], gam[8], bet[8], w[8];
  double md[8], rd[8], k1[8], cb[8], cg[8];
  bn2_consts(stats, eps, l, mean, rstd);
  load_vec8(g2, l, gam);
  load_vec8(be2, l, bet);
  load_vec8(w2, l, w);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = col_of(l, j);
    md[j] = stats[c];
    rd[j] = 1.0 / sqrt(stats[U + c] + (double)eps);
    k1[j] = (double)gam[j] * rd[j];
    cb[j] = sums[c] / (double)P;
    cg[j] = sums[U + c] / (double)P;
  }
  for (int64_t n = (int64_t)blockIdx.x * GPB + g; n < n_own; n += (int64_t)gridDim.x * GPB) {
    float a[8];
    load_row8(own + n * ld_own, l, a);
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    const int32_t e0 = rowptr[n], e1 = rowptr[n + 1];
    for (int32_t e = e0; e < e1; ++e) {
      const int64_t p = clampi(perm[e], P);
      float b[8];
      load_row8(other + clampi(idx_other[p], n_other) * ld_other, l, b);
      const double d = (double)dl[p];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // the ReLU mask as the loss pass saw it (fp32, the same explicit fma); du itself in fp64: over a Cartesian list every node's segment meets the
        // same partners, so S[n] is a small difference of the per-pair terms
        const float xf = (a[j] + b[j] - mean[j]) * rstd[j];
        const double xh = ((double)a[j] + (double)b[j] - md[j]) * rd[j];
        const double dy = fmaf(gam[j], xf, bet[j]) > 0.f ? d * (double)w[j] : 0.0;
        acc[j] += k1[j] * (dy - cb[j] - xh * cg[j]);
      }
    }
    float* srow = S + n * ld_s;
    *reinterpret_cast<float4*>(srow + 4 * l) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    *reinterpret_cast<float4*>(srow + 64 + 4 * l) = make_float4((float)acc[4], (float)acc[5], (float)acc[6], (float)acc[7]);
  }
}

// ---- 4. eval: running statistics (BN2 as a per-column affine), p and the confusion counts ------------------------------
__global__ __launch_bounds__(256) void pm_eval_kernel(const float* __restrict__ A, int64_t lda, int64_t nA, const float* __restrict__ B,
                                                      int64_t ldb, int64_t nB, const int64_t* __restrict__ idx1,
                                                      const int64_t* __restrict__ idx2, const uint8_t* __restrict__ y, int64_t P,
                                                      const float* __restrict__ scale2, const float* __restrict__ shift2,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      float* __restrict__ p_out, double* __restrict__ part) {
  __shared__ double red[GPB * EVAL_W];
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  float sc[8], sh[8], w[8];
  load_vec8(scale2, l, sc);
  load_vec8(shift2, l, sh);
  load_vec8(w2, l, w);
  const float bias2 = b2[0];
  double tp = 0.0, fp = 0.0, fn = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * GPB + g; p < P; p += (int64_t)gridDim.x * GPB) {
    float a[8], b[8];
    load_row8(A + clampi(idx1[p], nA) * lda, l, a);
    load_row8(B + clampi(idx2[p], nB) * ldb, l, b);
    float part_logit = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) part_logit = fmaf(w[j], fmaxf(fmaf(a[j] + b[j], sc[j], sh[j]), 0.f), part_logit);
    const float pr = 1.f / (1.f + expf(-(bgnn::group_sum<GL>(part_logit) + bias2)));
    if (y) {
      const bool pos = pr > 0.5f, yy = y[p] != 0;
      tp += (pos && yy) ? 1.0 : 0.0;
      fp += (pos && !yy) ? 1.0 : 0.0;
      fn += (!pos && yy) ? 1.0 : 0.0;
    }
    if (l == 0) p_out[p] = pr;
  }
  if (l == 0) {
    red[g * EVAL_W + 0] = tp; red[g * EVAL_W + 1] = fp; red[g * EVAL_W + 2] = fn; red[g * EVAL_W + 3] = 0.0;
  }
  block_partials(red, EVAL_W, part);
}

bool rows_ok(const float* t, int64_t ld) { return bgnn_aligned16(t) && ld >= U && ld % 4 == 0; }

}  // namespace

extern "C" size_t bgnn_pair_mlp_workspace_bytes(int64_t P) { return (size_t)pm_blocks(P) * LOSS_W * sizeof(double); }

extern "C" int bgnn_pair_mlp_stats_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB,
                                       const int64_t* idx1, const int64_t* idx2, int64_t P, float momentum, float* run_mean_opt,
                                       float* run_var_opt, double* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !B || !idx1 || !idx2 || !stats || !ws) return BGNN_E_NULL;
  if (P <= 1 || nA <= 0 || nB <= 0) return BGNN_E_SHAPE;
  if (!rows_ok(A, lda) || !rows_ok(B, ldb)) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_pair_mlp_workspace_bytes(P)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = pm_blocks(P);
  double* part = (double*)ws;
  hipLaunchKernelGGL(pm_stats_kernel, dim3(nblk), dim3(256), 0, st, A, lda, nA, B, ldb, nB, idx1, idx2, P, part);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pm_stats_finish_kernel, dim3(U), dim3(256), 0, st, part, nblk, P, momentum, run_mean_opt, run_var_opt, stats);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_pair_mlp_loss_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB,
                                      const int64_t* idx1, const int64_t* idx2, const uint8_t* y, int64_t P, const double* stats,
                                      const float* g2, const float* be2, const float* w2, const float* b2, float eps, float* p_out,
                                      float* dl_out, double* sums, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !B || !idx1 || !idx2 || !y || !stats || !g2 || !be2 || !w2 || !b2 || !p_out || !dl_out || !sums || !ws)
    return BGNN_E_NULL;
  if (P <= 1 || nA <= 0 || nB <= 0) return BGNN_E_SHAPE;
  if (!rows_ok(A, lda) || !rows_ok(B, ldb)) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_pair_mlp_workspace_bytes(P)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = pm_blocks(P);
  double* part = (double*)ws;
  hipLaunchKernelGGL(pm_loss_kernel, dim3(nblk), dim3(256), 0, st, A, lda, nA, B, ldb, nB, idx1, idx2, y, P, stats, g2, be2, w2, b2,
                     eps, p_out, dl_out, part);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pm_sum_partials_kernel, dim3(LOSS_W), dim3(256), 0, st, part, nblk, LOSS_W, sums);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_pair_mlp_segsum_f32(const float* own, int64_t ld_own, int64_t n_own, const float* other, int64_t ld_other,
                                        int64_t n_other, const int32_t* rowptr, const int32_t* perm, const int64_t* idx_other,
                                        int64_t P, const float* dl, const double* stats, const double* sums, const float* g2,
                                        const float* be2, const float* w2, float eps, float* S, int64_t ld_s, void* stream) {
  if (!own || !other || !rowptr || !perm || !idx_other || !dl || !stats || !sums || !g2 || !be2 || !w2 || !S) return BGNN_E_NULL;
  if (P <= 1 || n_own <= 0 || n_other <= 0) return BGNN_E_SHAPE;
  if (!rows_ok(own, ld_own) || !rows_ok(other, ld_other) || !rows_ok(S, ld_s)) return BGNN_E_ALIGN;
  const int64_t nb = (n_own + GPB - 1) / GPB;
  const int nblk = (int)(nb < 4096 ? nb : 4096);
  hipLaunchKernelGGL(pm_segsum_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, own, ld_own, n_own, other, ld_other, n_other,
                     rowptr, perm, idx_other, P, dl, stats, sums, g2, be2, w2, eps, S, ld_s);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_pair_mlp_eval_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB,
                                      const int64_t* idx1, const int64_t* idx2, const uint8_t* y_opt, int64_t P, const float* scale2,
                                      const float* shift2, const float* w2, const float* b2, float* p_out, double* counts_opt,
                                      void* ws, size_t ws_bytes, void* stream) {
  if (!A || !B || !idx1 || !idx2 || !scale2 || !shift2 || !w2 || !b2 || !p_out || !ws) return BGNN_E_NULL;
  if ((y_opt == nullptr) != (counts_opt == nullptr)) return BGNN_E_NULL;
  if (P <= 0 || nA <= 0 || nB <= 0) return BGNN_E_SHAPE;
  if (!rows_ok(A, lda) || !rows_ok(B, ldb)) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_pair_mlp_workspace_bytes(P)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = pm_blocks(P);
  double* part = (double*)ws;
  hipLaunchKernelGGL(pm_eval_kernel, dim3(nblk), dim3(256), 0, st, A, lda, nA, B, ldb, nB, idx1, idx2, y_opt, P, scale2, shift2, w2, b2,
                     p_out, part);
  BGNN_LAUNCH_CHECK();
  if (counts_opt) {
    hipLaunchKernelGGL(pm_sum_partials_kernel, dim3(EVAL_W), dim3(256), 0, st, part, nblk, EVAL_W, counts_opt);
    BGNN_LAUNCH_CHECK();
  }
  return 0;
}
