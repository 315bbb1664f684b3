// Pair passes of the cosine similarity scorer Similar (v1, models/models.py:67-169) under the BCE of train_adv_few_shot
// (scripts.py:36-50) and the Cartesian evaluation of eval_within_domain / eval_cross_domain (scripts.py:98-190).
// Everything in front of the cosine is per-node work done by the caller: q = u + biasatt(u), u = lin_self(z), and the row
// normalisation q^ = q / max(|q|, 1e-8).  What is left per pair is the dot of two normalised rows:
//   loss:   cos_p = q^1[idx1[p]] . q^2[idx2[p]], p = sigmoid(cos_p), BCE and its gradient dl_p = d mean-BCE / d cos_p;
//   segsum: G[n] = sum over node n's pairs of dl_p q^other[idx_other[p]]  (the only per-pair part of the backward);
//   count:  TP / FP / FN / TN of (sigmoid(cos) > 0.5) against label equality over a full product rows1 x rows2.
//
// Layout of the loss / segsum passes as in bgnn_pair_mlp.hip: 16 consecutive lanes own one pair (or node), lane l holds
// columns 4l..4l+3 and 64+4l..64+4l+3 of a 128-float row.  Sums are fp64 and reduced in a fixed order (groups of a block
// through LDS, then blocks by one thread per column block), the grid depends on P only: run-to-run identical, no atomics.
// The count pass is a register-tiled fp32 FMA product: 128 x 128 pairs per 256-thread block, 8 x 8 per thread, the 128-wide
// reduction staged through LDS in chunks of 32; no pair is materialised.
#include "bgnn_common.h"

namespace {

constexpr int Q = 128;                 // width of q (biasatt = Linear(128, 64) -> Linear(64, 128), models.py:70-74)
constexpr int GL = 16;                 // lanes per pair / node
constexpr int GPB = 16;                // groups per block (256 threads)
constexpr int PC_MAX_BLOCKS = 1024;
constexpr int LOSS_W = 4;              // per block: bce, tp, fp, fn

// count pass tiling
constexpr int TM = 128;                // rows1 per tile
constexpr int TN = 128;                // rows2 per tile
constexpr int KC = 32;                 // reduction chunk staged in LDS
constexpr int LDT = TM + 4;            // padded LDS row (k-major): breaks the bank pattern of the transposing stores
constexpr int CNT_MAX_BLOCKS = 2048;
constexpr int CNT_W = 4;               // per block: tp, fp, fn, tn (int64)

__host__ __device__ inline int pc_blocks(int64_t P) {
  const int64_t b = (P + GPB - 1) / GPB;
  return (int)(b < PC_MAX_BLOCKS ? (b < 1 ? 1 : b) : PC_MAX_BLOCKS);
}

__host__ __device__ inline int64_t cnt_tiles(int64_t m1, int64_t m2) { return ((m1 + TM - 1) / TM) * ((m2 + TN - 1) / TN); }

__host__ __device__ inline int cnt_blocks(int64_t m1, int64_t m2) {
  const int64_t t = cnt_tiles(m1, m2);
  return (int)(t < CNT_MAX_BLOCKS ? (t < 1 ? 1 : t) : CNT_MAX_BLOCKS);
}

__device__ __forceinline__ int64_t clampi(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ void load_row8(const float* __restrict__ row, int l, float v[8]) {
  const float4 a = *reinterpret_cast<const float4*>(row + 4 * l);
  const float4 b = *reinterpret_cast<const float4*>(row + 64 + 4 * l);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// the threshold of the reference: fp32 sigmoid, then > 0.5 (scripts.py:64, :126, :165)
__device__ __forceinline__ float sigmoidf_ref(float x) { return 1.f / (1.f + expf(-x)); }

// ---- 1. loss: p, dl and the fixed-order BCE sum / counts ----------------------------------------------------------------
// bce_p = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100))   (torch's clamp; never bites: p in [0.269, 0.731]);
// dl_p = [(p - y) / max((1 - p) p, 1e-12) / P] * (1 - p) * p      (torch's binary_cross_entropy_backward, then sigmoid_backward).
__global__ __launch_bounds__(256) void pc_loss_kernel(const float* __restrict__ A, int64_t lda, int64_t nA, const float* __restrict__ B,
                                                      int64_t ldb, int64_t nB, const int64_t* __restrict__ idx1,
                                                      const int64_t* __restrict__ idx2, const uint8_t* __restrict__ y, int64_t P,
                                                      float* __restrict__ p_out, float* __restrict__ dl_out, double* __restrict__ part) {
  __shared__ double red[GPB * LOSS_W];
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  const float Pf = (float)P;
  double sbce = 0.0, tp = 0.0, fp = 0.0, fn = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * GPB + g; p < P; p += (int64_t)gridDim.x * GPB) {
    float a[8], b[8];
    load_row8(A + clampi(idx1[p], nA) * lda, l, a);
    load_row8(B + clampi(idx2[p], nB) * ldb, l, b);
    float part_dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) part_dot = fmaf(a[j], b[j], part_dot);
    const float c = bgnn::group_sum<GL>(part_dot);
    const float pr = sigmoidf_ref(c);
    const float yy = y[p] ? 1.f : 0.f;
    float gr = (pr - yy) / fmaxf((1.f - pr) * pr, 1e-12f);
    gr = gr / Pf;
    const float dl = gr * (1.f - pr) * pr;
    const double lp = fmax(log((double)pr), -100.0), l1p = fmax(log1p(-(double)pr), -100.0);
    sbce -= (double)yy * lp + (1.0 - (double)yy) * l1p;
    const bool pos = pr > 0.5f;
    tp += (pos && yy == 1.f) ? 1.0 : 0.0;
    fp += (pos && yy == 0.f) ? 1.0 : 0.0;
    fn += (!pos && yy == 1.f) ? 1.0 : 0.0;
    if (l == 0) {
      p_out[p] = pr;
      dl_out[p] = dl;
    }
  }
  if (l == 0) {
    double* r = red + g * LOSS_W;
    r[0] = sbce; r[1] = tp; r[2] = fp; r[3] = fn;
  }
  __syncthreads();
  if (threadIdx.x < LOSS_W) {
    double s = 0.0;
    for (int gg = 0; gg < GPB; ++gg) s += red[gg * LOSS_W + threadIdx.x];
    part[(int64_t)blockIdx.x * LOSS_W + threadIdx.x] = s;
  }
}

// fixed-order sums of the blocks' partials: one 256-thread block per column (strided per-thread sums, then an LDS tree)
__global__ __launch_bounds__(256) void pc_sum_partials_kernel(const double* __restrict__ part, int nblk, int W, double* __restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x, c = blockIdx.x;
  double s = 0.0;
  for (int b = t; b < nblk; b += 256) s += part[(int64_t)b * W + c];
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) out[c] = red[0];
}

// ---- 2. per-node segment sums -----------------------------------------------------------------------------------------
// G[n] = sum over the pairs p of node n's segment (CSR rowptr / perm = pair ids) of dl[p] * other[idx_other[p]].  One group per
// node, fp64 accumulation in registers in the segment's order, every row written once (zeros for nodes no pair references).
__global__ __launch_bounds__(256) void pc_segsum_kernel(const float* __restrict__ other, int64_t ld_other, int64_t n_other,
                                                        const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ idx_other, int64_t P, const float* __restrict__ dl,
                                                        int64_t n_own, float* __restrict__ G, int64_t ld_g) {
  const int g = threadIdx.x / GL, l = threadIdx.x % GL;
  for (int64_t n = (int64_t)blockIdx.x * GPB + g; n < n_own; n += (int64_t)gridDim.x * GPB) {
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
      for (int j = 0; j < 8; ++j) acc[j] += d * (double)b[j];
    }
    float* grow = G + n * ld_g;
    *reinterpret_cast<float4*>(grow + 4 * l) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    *reinterpret_cast<float4*>(grow + 64 + 4 * l) = make_float4((float)acc[4], (float)acc[5], (float)acc[6], (float)acc[7]);
  }
}

// ---- 3. confusion counts over the product rows1 x rows2 -----------------------------------------------------------------
// Thread (tx, ty) of a 16 x 16 block owns tile rows {4ty + a, 64 + 4ty + a} and tile columns {4tx + b, 64 + 4tx + b}, a, b < 4.
// Each 32-wide chunk of both sides is stored k-major in LDS (As[k][row]), so the 8 operands of a thread are two float4 reads
// per side and k-step: 4 LDS reads per 64 FMAs.  Rows past m1 / m2 are staged as zeros and masked out of the counts.
__device__ __forceinline__ int tile_off(int t4, int i) { return i < 4 ? 4 * t4 + i : 64 + 4 * t4 + (i - 4); }

__device__ __forceinline__ void stage_chunk(const float* __restrict__ T, int64_t ld, int64_t nT, const int64_t* __restrict__ rows,
                                            int64_t m, int64_t base, int k0, float* __restrict__ S) {
  // 128 rows x 32 floats = 1024 float4; 4 per thread.  Thread t: row t / 8 (+ 32 i), float4 (t % 8) of the chunk
  const int t = threadIdx.x;
  const int c4 = t % 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = t / 8 + 32 * i;
    const int64_t gi = base + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gi < m) v = *reinterpret_cast<const float4*>(T + clampi(rows[gi], nT) * ld + k0 + 4 * c4);
    S[(4 * c4 + 0) * LDT + r] = v.x;
    S[(4 * c4 + 1) * LDT + r] = v.y;
    S[(4 * c4 + 2) * LDT + r] = v.z;
    S[(4 * c4 + 3) * LDT + r] = v.w;
  }
}

__global__ __launch_bounds__(256) void pc_count_kernel(const float* __restrict__ A, int64_t lda, int64_t nA, const float* __restrict__ B,
                                                       int64_t ldb, int64_t nB, const int64_t* __restrict__ rows1, int64_t m1,
                                                       const int64_t* __restrict__ rows2, int64_t m2, const int64_t* __restrict__ lab1,
                                                       const int64_t* __restrict__ lab2, long long* __restrict__ part) {
  __shared__ float As[KC * LDT];
  __shared__ float Bs[KC * LDT];
  __shared__ long long red[256 * CNT_W];
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  const int64_t tiles_n = (m2 + TN - 1) / TN;
  const int64_t ntiles = cnt_tiles(m1, m2);
  long long tp = 0, fp = 0, fn = 0, tn = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base1 = (tile / tiles_n) * TM, base2 = (tile % tiles_n) * TN;
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 8; ++b) acc[a][b] = 0.f;
    for (int k0 = 0; k0 < Q; k0 += KC) {
      __syncthreads();                                   // the previous chunk (or tile) is consumed
      stage_chunk(A, lda, nA, rows1, m1, base1, k0, As);
      stage_chunk(B, ldb, nB, rows2, m2, base2, k0, Bs);
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < KC; ++k) {
        const float4 a0 = *reinterpret_cast<const float4*>(As + k * LDT + 4 * ty);
        const float4 a1 = *reinterpret_cast<const float4*>(As + k * LDT + 64 + 4 * ty);
        const float4 b0 = *reinterpret_cast<const float4*>(Bs + k * LDT + 4 * tx);
        const float4 b1 = *reinterpret_cast<const float4*>(Bs + k * LDT + 64 + 4 * tx);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) acc[a][b] = fmaf(av[a], bv[b], acc[a][b]);
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
        const bool pos = sigmoidf_ref(acc[a][b]) > 0.5f;
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

__global__ __launch_bounds__(64) void pc_count_finish_kernel(const long long* __restrict__ part, int nblk, long long* __restrict__ counts) {
  if (threadIdx.x >= CNT_W) return;
  long long s = 0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * CNT_W + threadIdx.x];
  counts[threadIdx.x] = s;
}

bool rows_ok(const float* t, int64_t ld) { return bgnn_aligned16(t) && ld >= Q && ld % 4 == 0; }

}  // namespace

extern "C" size_t bgnn_pair_cos_loss_workspace_bytes(int64_t P) { return (size_t)pc_blocks(P) * LOSS_W * sizeof(double); }

extern "C" size_t bgnn_pair_cos_count_workspace_bytes(int64_t m1, int64_t m2) {
  return (size_t)cnt_blocks(m1, m2) * CNT_W * sizeof(long long);
}

extern "C" int bgnn_pair_cos_loss_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB,
                                      const int64_t* idx1, const int64_t* idx2, const uint8_t* y, int64_t P, float* p_out,
                                      float* dl_out, double* sums, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !B || !idx1 || !idx2 || !y || !p_out || !dl_out || !sums || !ws) return BGNN_E_NULL;
  if (P <= 0 || nA <= 0 || nB <= 0) return BGNN_E_SHAPE;
  if (!rows_ok(A, lda) || !rows_ok(B, ldb)) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_pair_cos_loss_workspace_bytes(P)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = pc_blocks(P);
  double* part = (double*)ws;
  hipLaunchKernelGGL(pc_loss_kernel, dim3(nblk), dim3(256), 0, st, A, lda, nA, B, ldb, nB, idx1, idx2, y, P, p_out, dl_out, part);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pc_sum_partials_kernel, dim3(LOSS_W), dim3(256), 0, st, part, nblk, LOSS_W, sums);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_pair_cos_segsum_f32(const float* other, int64_t ld_other, int64_t n_other, const int32_t* rowptr,
                                        const int32_t* perm, const int64_t* idx_other, int64_t P, const float* dl, int64_t n_own,
                                        float* G, int64_t ld_g, void* stream) {
  if (!other || !rowptr || !perm || !idx_other || !dl || !G) return BGNN_E_NULL;
  if (P <= 0 || n_own <= 0 || n_other <= 0) return BGNN_E_SHAPE;
  if (!rows_ok(other, ld_other) || !rows_ok(G, ld_g)) return BGNN_E_ALIGN;
  const int64_t nb = (n_own + GPB - 1) / GPB;
  const int nblk = (int)(nb < 4096 ? nb : 4096);
  hipLaunchKernelGGL(pc_segsum_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, other, ld_other, n_other, rowptr, perm, idx_other,
                     P, dl, n_own, G, ld_g);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" int bgnn_pair_cos_count_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB,
                                       const int64_t* rows1, int64_t m1, const int64_t* rows2, int64_t m2, const int64_t* lab1,
                                       const int64_t* lab2, long long* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !B || !lab1 || !lab2 || !counts || !ws) return BGNN_E_NULL;
  if (m1 < 0 || m2 < 0 || nA <= 0 || nB <= 0) return BGNN_E_SHAPE;
  if ((m1 > 0 && !rows1) || (m2 > 0 && !rows2)) return BGNN_E_NULL;
  if (!rows_ok(A, lda) || !rows_ok(B, ldb)) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_pair_cos_count_workspace_bytes(m1, m2)) return BGNN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (m1 == 0 || m2 == 0) {
    const hipError_t e = hipMemsetAsync(counts, 0, CNT_W * sizeof(long long), st);
    return e == hipSuccess ? 0 : (int)e;
  }
  const int nblk = cnt_blocks(m1, m2);
  long long* part = (long long*)ws;
  hipLaunchKernelGGL(pc_count_kernel, dim3(nblk), dim3(256), 0, st, A, lda, nA, B, ldb, nB, rows1, m1, rows2, m2, lab1, lab2, part);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(pc_count_finish_kernel, dim3(1), dim3(64), 0, st, part, nblk, counts);
  BGNN_LAUNCH_CHECK();
  return 0;
}
