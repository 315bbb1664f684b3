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
// The count pass (section 5) is the Cartesian evaluation: TP / FP / FN / TN of the eval-mode scorer over a whole product
// rows1 x rows2 as a register-tiled fp32 vector kernel, 128 x 128 pairs per 256-thread block, no pair materialised.
#include "bgnn_common.h"

namespace {

constexpr int U = 128;                 // width of u (Linear(2H, 128), models.py:918)
constexpr int GL = 16;                 // lanes per pair / node
constexpr int GPB = 16;                // groups per block (256 threads)
constexpr int PM_MAX_BLOCKS = 1024;
constexpr int STAT_W = 2 * U;          // per block: sum u, sum u^2
constexpr int LOSS_W = 3 * U + 8;      // per block: sum dy, sum dy*xh, sum dl*h, then dl, bce, tp, fp, fn (+3 pad)
constexpr int EVAL_W = 4;              // tp, fp, fn (+1 pad)

// count pass tiling (as the cosine count of bgnn_pair_cos.hip)
constexpr int CT = 128;                // rows1 and rows2 per tile
constexpr int KC = 32;                 // reduction chunk staged in LDS
constexpr int LDT = CT + 4;            // padded LDS row (k-major): breaks the bank pattern of the transposing stores
constexpr int CNT_MAX_BLOCKS = 2048;
constexpr int CNT_W = 4;               // per block: tp, fp, fn, tn (int64)

__host__ __device__ inline int64_t cnt_tiles(int64_t m1, int64_t m2) { return ((m1 + CT - 1) / CT) * ((m2 + CT - 1) / CT); }

__host__ __device__ inline int cnt_blocks(int64_t m1, int64_t m2) {
  const int64_t t = cnt_tiles(m1, m2);
  return (int)(t < CNT_MAX_BLOCKS ? (t < 1 ? 1 : t) : CNT_MAX_BLOCKS);
}

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

// ---- 5. eval over a whole product rows1 x rows2: confusion counts, no pair list ------------------------------------------
// logit(i, j) = b2 + sum_c w2[c] relu(scale2[c] (A[rows1[i]][c] + B[rows2[j]][c]) + shift2[c]).  BN2 is folded into the staged
// tables once per tile and chunk: a' = fma(scale2, A, shift2) on the rows1 side, b' = scale2 * B on the rows2 side, so a pair and
// column cost an add, a max and an fma with the block-uniform w2[c] (the adds and fmas on float2 lanes: packed fp32 issue).
// The columns are accumulated in ascending order into one fp32 sum per pair; the predicate is pm_eval_kernel's
// 1 / (1 + expf(-logit)) > 0.5f.  (pm_eval_kernel forms fma(a + b, scale2, shift2) and sums 16 lane partials of 8 columns
// each: a different rounding of the same real number, so the two passes may disagree on pairs whose logit is within fp32
// rounding of 0 -- DESIGN.md section 11.)
// Thread (tx, ty) of a 16 x 16 block owns tile rows {4ty + a, 64 + 4ty + a} and tile columns {4tx + b, 64 + 4tx + b}, a, b < 4;
// each 32-wide chunk of both sides is stored k-major in LDS, so a thread's 16 operands of a k-step are four float4 reads (the
// rows1 side a broadcast inside each 16-lane group, the rows2 side 64 consecutive dwords per group).  Rows past m1 / m2 are
// staged as zeros and masked out of the counts.
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int tile_off(int t4, int i) { return i < 4 ? 4 * t4 + i : 64 + 4 * t4 + (i - 4); }

template <bool SHIFTED>
__device__ __forceinline__ void stage_chunk(const float* __restrict__ T, int64_t ld, int64_t nT, const int64_t* __restrict__ rows,
                                            int64_t m, int64_t base, int k0, const float* __restrict__ scale2,
                                            const float* __restrict__ shift2, float* __restrict__ S) {
  // 128 rows x 32 floats = 1024 float4; 4 per thread.  Thread t: row t / 8 (+ 32 i), float4 (t % 8) of the chunk
  const int t = threadIdx.x;
  const int c4 = t % 8;
  const float4 sc = *reinterpret_cast<const float4*>(scale2 + k0 + 4 * c4);
  float4 sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (SHIFTED) sh = *reinterpret_cast<const float4*>(shift2 + k0 + 4 * c4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = t / 8 + 32 * i;
    const int64_t gi = base + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gi < m) {
      v = *reinterpret_cast<const float4*>(T + clampi(rows[gi], nT) * ld + k0 + 4 * c4);
      if (SHIFTED) {
        v.x = fmaf(sc.x, v.x, sh.x); v.y = fmaf(sc.y, v.y, sh.y); v.z = fmaf(sc.z, v.z, sh.z); v.w = fmaf(sc.w, v.w, sh.w);
      } else {
        v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
      }
    }
    S[(4 * c4 + 0) * LDT + r] = v.x;
    S[(4 * c4 + 1) * LDT + r] = v.y;
    S[(4 * c4 + 2) * LDT + r] = v.z;
    S[(4 * c4 + 3) * LDT + r] = v.w;
  }
}

__global__ __launch_bounds__(256) void pm_count_kernel(const float* __restrict__ A, int64_t lda, int64_t nA, const float* __restrict__ B,
                                                       int64_t ldb, int64_t nB, const int64_t* __restrict__ rows1, int64_t m1,
                                                       const int64_t* __restrict__ rows2, int64_t m2, const int64_t* __restrict__ lab1,
                                                       const int64_t* __restrict__ lab2, const float* __restrict__ scale2,
                                                       const float* __restrict__ shift2, const float* __restrict__ w2,
                                                       const float* __restrict__ b2, long long* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[KC * LDT];
  __shared__ __attribute__((aligned(16))) float Bs[KC * LDT];
  __shared__ float Ws[U];
  __shared__ long long red[256 * CNT_W];
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  if (threadIdx.x < U) Ws[threadIdx.x] = w2[threadIdx.x];   // visible after the first chunk's barrier
  const float bias2 = b2[0];
  const int64_t tiles_n = (m2 + CT - 1) / CT;
  const int64_t ntiles = cnt_tiles(m1, m2);
  long long tp = 0, fp = 0, fn = 0, tn = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base1 = (tile / tiles_n) * CT, base2 = (tile % tiles_n) * CT;
    f32x2 acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = f32x2{0.f, 0.f};
    for (int k0 = 0; k0 < U; k0 += KC) {
      __syncthreads();                                   // the previous chunk (or tile) is consumed
      stage_chunk<true>(A, lda, nA, rows1, m1, base1, k0, scale2, shift2, As);
      stage_chunk<false>(B, ldb, nB, rows2, m2, base2, k0, scale2, shift2, Bs);
      __syncthreads();
#pragma unroll 2
      for (int k = 0; k < KC; ++k) {
        const float4 a0 = *reinterpret_cast<const float4*>(As + k * LDT + 4 * ty);
        const float4 a1 = *reinterpret_cast<const float4*>(As + k * LDT + 64 + 4 * ty);
        const float4 b0 = *reinterpret_cast<const float4*>(Bs + k * LDT + 4 * tx);
        const float4 b1 = *reinterpret_cast<const float4*>(Bs + k * LDT + 64 + 4 * tx);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const f32x2 bv[4] = {f32x2{b0.x, b0.y}, f32x2{b0.z, b0.w}, f32x2{b1.x, b1.y}, f32x2{b1.z, b1.w}};
        const float w = Ws[k0 + k];
        const f32x2 wv = f32x2{w, w};
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          const f32x2 aa = f32x2{av[a], av[a]};
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const f32x2 x = aa + bv[b];
            const f32x2 h = f32x2{fmaxf(x.x, 0.f), fmaxf(x.y, 0.f)};
            acc[a][b] = __builtin_elementwise_fma(wv, h, acc[a][b]);
          }
        }
      }
    }
    int64_t la[8], lb[8];
    bool va[8], vb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t gi = base1 + tile_off(ty, i), gj = base2 + tile_off(tx, i);
      va[i] = gi < m1;
      vb[i] = gj < m2;
      la[i] = va[i] ? lab1[clampi(rows1[gi], nA)] : 0;
      lb[i] = vb[i] ? lab2[clampi(rows2[gj], nB)] : 0;
    }
    int ctp = 0, cfp = 0, cfn = 0, ctn = 0;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (!(va[a] && vb[b])) continue;
        const float logit = ((b & 1) ? acc[a][b / 2].y : acc[a][b / 2].x) + bias2;
        const bool pos = 1.f / (1.f + expf(-logit)) > 0.5f;
        const bool same = la[a] == lb[b];
        ctp += (pos && same);
        cfp += (pos && !same);
        cfn += (!pos && same);
        ctn += (!pos && !same);
      }
    tp += ctp; fp += cfp; fn += cfn; tn += ctn;
  }
  long long* r = red + threadIdx.x * CNT_W;
  r[0] = tp; r[1] = fp; r[2] = fn; r[3] = tn;
  __syncthreads();
  if (threadIdx.x < CNT_W) {
    long long s = 0;
    for (int t = 0; t < 256; ++t) s += red[t * CNT_W + threadIdx.x];
    part[(int64_t)blockIdx.x * CNT_W + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void pm_count_finish_kernel(const long long* __restrict__ part, int nblk, long long* __restrict__ counts) {
  if (threadIdx.x >= CNT_W) return;
  long long s = 0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * CNT_W + threadIdx.x];
  counts[threadIdx.x] = s;
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

extern "C" size_t bgnn_pair_mlp_count_workspace_bytes(int64_t m1, int64_t m2) {
  return (size_t)cnt_blocks(m1, m2) * CNT_W * sizeof(long long);
}

extern "C" int bgnn_pair_mlp_count_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB,
                                       const int64_t* rows1, int64_t m1, const int64_t* rows2, int64_t m2, const int64_t* lab1,
                                       const int64_t* lab2, const float* scale2, const float* shift2, const float* w2,
                                       const float* b2, long long* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !B || !lab1 || !lab2 || !scale2 || !shift2 || !w2 || !b2 || !counts || !ws) return BGNN_E_NULL;
  if (m1 < 0 || m2 < 0 || nA <= 0 || nB <= 0) return BGNN_E_SHAPE;
  if ((m1 > 0 && !rows1) || (m2 > 0 && !rows2)) return BGNN_E_NULL;
  if (!rows_ok(A, lda) || !rows_ok(B, ldb) || !bgnn_aligned16(scale2) || !bgnn_aligned16(shift2)) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_pair_mlp_count_workspace_bytes(m1, m2)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (m1 == 0 || m2 == 0) {
    const hipError_t e = hipMemsetAsync(counts, 0, CNT_W * sizeof(long long), st);
    return e == hipSuccess ? 0 : (int)e;
  }
  const int nblk = cnt_blocks(m1, m2);
  long long* part = (long long*)ws;
  hipLaunchKernelGGL(pm_count_kernel, dim3(nblk), dim3(256), 0, st, A, lda, nA, B, ldb, nB, rows1, m1, rows2, m2, lab1, lab2, scale2,
                     shift2, w2, b2, part);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pm_count_finish_kernel, dim3(1), dim3(64), 0, st, part, nblk, counts);
  BGNN_LAUNCH_CHECK();
  return 0;
}
