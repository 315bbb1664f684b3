// GCNII (GCN2) conv for gfx950 (wave64): normalised aggregation, initial-residual mix, H x H identity-mapping product, ReLU and
// dropout in one pass; and the dense half of its backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:163-197): PyG GCN2Conv(H, alpha, theta, layer, shared_weights=True,
// normalize=False) over the cached gcn_norm adjacency, with the F.relu and the F.dropout that follow it in GCN2.forward.  The
// graph is the by-destination CSR of bgnn_gcn.hip (exactly one self loop per row, dinv = deg^-1/2):
//   m_i = (1 - alpha) * dinv_i * sum_{t in row i} dinv[col[t]] * x[col[t]] + alpha * x0_i
//   y_i = drop(relu(m_i @ M)),   M = (1 - beta) * I + beta * weight1   (formed by the host once per layer call)
// The edge walk is gcn_agg_kernel's (mapping ladder, persistent XCD-ordered grid, hub rows as SEGMENT / FINISH launches; helpers:
// bgnn_conv_common.h).  What is new is the dense step inside the tile: the finished m rows of a tile go to LDS (TR = 16 rows at
// H > 32, 32 below; at H > 64 a block iteration of the ladder has 8 rows, so two gather passes fill one tile), M sits in LDS once
// per persistent block, and the four waves form the TR x H product with the f32-input MFMA (v_mfma_f32_16x16x4_f32: an exact
// fp32 fmaf chain over k, so nothing is split or rounded to a narrower format).  The product goes back through LDS to the lanes
// that own the rows, which apply ReLU and the dropout hash and store float4 rows.  m is written to memory only when the
// caller passes m_out (training: the backward needs it); evaluation never stores it.
// Bytes in evaluation at width H: E'(4H + 8) + N(8H + 4) + 4H^2 -- the aggregation's own traffic plus x0 in place of nothing
// and M once per block from L2; the composition pays the aggregation and four more [N, H] passes.
//
// Two entries, one launch sequence (conv_run): bgnn_gcn2_conv_f32 over a square graph, and bgnn_gcn2_conv_rows_f32 over a
// rectangular one (a rank's owned rows gather from n_tbl >= n_rows table rows) with the GLOBAL id of every output row for the dropout
// hash -- element row_ids[io] * H + column in place of io * H + column, in the row launch and in a hub's finish launch (io =
// hub_rows[h]).  The lookup is a TEMPLATE FLAG (IDS), not a pointer test in the one kernel.  With the test, the pointer and its
// condition stay live across the gather loop and the product: the compiler's resource report gave the LF = 2 and LF = 4 row and
// finish instantiations (H in 5..16) four SGPRs more (104 / 103 and 102 / 101 where they had 100 / 99 and 98 / 97) and called
// that 7 waves per SIMD instead of 8, for callers that pass no ids.  (By the 16-register granules in which blocks are admitted
// both counts allow the same six blocks per CU, so the loss was probably on paper only; it was not measured.)  With the flag
// there is nothing to weigh: the id-free instantiations are the kernels they were -- same registers, LDS and bits -- the square
// entry and every p_drop = 0 call run them, and only a rank's training step runs the IDS ones.  Those hold one more 64-bit value
// per gathered row from the end of the gather
// to the epilogue (the load is issued before the product, not behind it): 2 SGPRs more each, 4 / 2 VGPRs more at LF = 32, no
// instantiation in another admission granule than its id-free twin except LF = 8 (96 -> 98 and 95 -> 97 SGPRs), which its 82 / 75
// VGPRs hold at 5 / 6 waves per SIMD already.
//
// LDS per block (floats): M as [4*LF rows][max(16, 4*LF) columns] (64 KB at H in 65..128, 16 KB at 33..64), plus the row tile
// [TR rows][4*LF + 4] for m and as much again for the product; at H > 64 the product overwrites the m rows instead (one more
// barrier), which keeps two blocks on a CU.  A wave reads back exactly the rows it wrote, so its next m rows never overwrite
// what another wave still reads.  Odd 16-column tiles of odd rows of M are swapped with their neighbours (XOR 16 on the
// column) where the row length is a multiple of 32 floats: the two k rows a 32-lane group of ds_read_b32 touches then fall on
// different banks.
//
// Backward dense entry: one streaming pass, gz = grad_y * [y > 0] * keep_scale (y > 0 <=> kept and positive: the rule of
// conv_bwd_rows_kernel, no mask is redrawn), gm = gz @ M^T through the same tile product with M^T in LDS, and three stores:
// gz, t = (1 - alpha) * gm, gx0 = alpha * gm.  grad_weight1 (beta * m^T gz) and grad_x (the forward walk of bgnn_gcn.hip over the
// by-source view applied to t) are the caller's, on entries that exist.  No float atomics anywhere.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;
enum { MODE_ROWS = 0, MODE_SEGMENT = 1, MODE_FINISH = 2 };
using f32x4 = __attribute__((ext_vector_type(4))) float;

// geometry of a tile (the rows of one product) under the (LF, EP) of lf_ladder
template <int LF, int EP>
struct Tile {
  static constexpr int GL = LF * EP;                       // lanes per output row
  static constexpr int GPW = 64 / GL;                      // rows per wave
  static constexpr int RPB = 4 * GPW;                      // rows per block iteration (4 waves)
  static constexpr int W = 4 * LF;                         // columns the lanes of a group span (>= pad4(H))
  static constexpr int NCT = W < 16 ? 1 : W / 16;          // 16-column tiles of the product
  static constexpr int LDM = NCT * 16;                     // row length of M in LDS
  static constexpr int NB = RPB < 16 ? 16 / RPB : 1;       // block iterations gathered per product (2 at H > 64: a full 16-row tile)
  static constexpr int TR = RPB * NB;                      // rows per tile: a multiple of 16
  static constexpr int RT = TR / 16;                       // 16-row tiles of the product
  static constexpr int LDA = W + 4;                        // row length of the m / product rows in LDS
  static constexpr bool ALIAS = NB > 1;                    // the product's rows overwrite the m rows (one more barrier) | follow them
  static constexpr int TILE_ROWS = ALIAS ? TR : 2 * TR;
  static constexpr int NT = RT * NCT;                      // 16 x 16 output tiles of the product
  static constexpr int TPW = (NT + 3) / 4;                 // per wave
  static_assert(TPW == 1 || RT == 1, "a wave with several tiles keeps one row tile");
  __device__ static float* os(float* tile) { return ALIAS ? tile : tile + TR * LDA; }
};

template <int LDM>
__device__ __forceinline__ int m_col(int j, int k) { return (LDM % 32 == 0) ? (j ^ ((k & 1) << 4)) : j; }

// M (TRANS: its transpose) into LDS, rows and columns from H on as 0: pad rows and columns of the caller's M never take part
template <int LF, int EP, bool TRANS>
__device__ __forceinline__ void load_m(const float* __restrict__ M, int64_t ldm, int H, float* Ms) {
  using T = Tile<LF, EP>;
  for (int idx = threadIdx.x; idx < T::W * T::LDM; idx += 256) {
    const int k = idx / T::LDM, j = idx % T::LDM;
    float v = 0.f;
    if (k < H && j < H) v = TRANS ? M[(int64_t)j * ldm + k] : M[(int64_t)k * ldm + j];
    Ms[k * T::LDM + m_col<T::LDM>(j, k)] = v;
  }
}

// rows [0, TR) of `tile` (KP columns each) times Ms -> T::os(tile): the rows that follow, or (ALIAS) the same rows once every wave
// has read its operands.  Every thread of the block calls it; it waits for the m rows first and for the product last.
template <int LF, int EP>
__device__ __forceinline__ void tile_product(float* tile, const float* Ms, int KP, int wave, int lane) {
  using T = Tile<LF, EP>;
  __syncthreads();
  const int r16 = lane & 15, kq = lane >> 4;
  f32x4 acc[T::TPW];
  int rt[T::TPW], ct[T::TPW];
#pragma unroll
  for (int s = 0; s < T::TPW; ++s) {
    const int t = wave + 4 * s;
    rt[s] = T::RT == 1 ? 0 : t / T::NCT;
    ct[s] = t % T::NCT;
    acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  if (wave < T::NT) {                                           // wave-uniform
    for (int k0 = 0; k0 < KP; k0 += 4) {
      const int k = k0 + kq;
#pragma unroll
      for (int s = 0; s < T::TPW; ++s) {
        const float a = tile[(rt[s] * 16 + r16) * T::LDA + k];
        const float b = Ms[k * T::LDM + m_col<T::LDM>(ct[s] * 16 + r16, k)];
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[s], 0, 0, 0);
      }
    }
  }
  if constexpr (T::ALIAS) __syncthreads();
  if (wave < T::NT) {
    float* os = T::os(tile);
#pragma unroll
    for (int s = 0; s < T::TPW; ++s) {
      const int c = ct[s] * 16 + r16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt[s] * 16 + kq * 4 + r;               // C/D layout: column = lane & 15, row = 4 * (lane >> 4) + register
        if (c < T::W) os[row * T::LDA + c] = acc[s][r];
      }
    }
  }
  __syncthreads();
}

struct Gcn2Params {
  const float* tbl; int64_t ldt; int64_t n_tbl;    // gathered rows: x; FINISH: the partial rows
  const float* x0; int64_t ldx0;                   // initial-residual rows
  const float* M; int64_t ldM;                     // [pad4(H), pad4(H)]
  const int32_t* rowptr; const int32_t* col;       // ROWS: the CSR; SEGMENT: rowptr = (begin, end) pairs; FINISH: rowptr = hub_seg_ptr
  const float* dinv; int64_t n_dinv;
  int64_t n_rows;                                  // rows / segments / hubs of this launch
  int32_t H;
  int32_t hub_threshold;                           // ROWS: rows of at least this many edges are left to the hub launches (0: none)
  const int32_t* hub_rows; int64_t n_out;          // FINISH: output row of hub h, rows of out
  const int64_t* row_ids;                          // NULL, or the global id of every output row: the row of the dropout hash
  float alpha, beta;                               // initial-residual weight and 1 - alpha
  float* m_out; int64_t ldmo;                      // the mix, or NULL
  float* out; int64_t ldo;                         // SEGMENT: the partial rows
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
};

// The weighted sum of the rows that row i of the launch gathers -- the edge walk of gcn_agg_kernel -- over the EP sub-groups of its lane
// group.  rvalid: the row exists and is this launch's (ROWS with hub tables leaves rows of at least hub_threshold edges out).
template <int LF, int EP, int U, int MODE>
__device__ __forceinline__ float4 gather_row(const Gcn2Params& p, int64_t i, int sub, int f0, bool fvalid, bool& rvalid) {
  rvalid = i < p.n_rows;
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
  return ep_sum<LF, LF * EP>(acc);
}

// IDS: the dropout hash takes its row from p.row_ids (a rank's rows of a partition); false: the row written, and no id is loaded
template <int LF, int EP, int U, int MODE, bool IDS>
__global__ __launch_bounds__(256) void gcn2_conv_kernel(Gcn2Params p) {
  using T = Tile<LF, EP>;
  constexpr int GL = T::GL, GPW = T::GPW, RPB = T::RPB, NB = T::NB, TR = T::TR;
  constexpr bool DENSE = MODE != MODE_SEGMENT;
  __shared__ __attribute__((aligned(16))) float Ms[DENSE ? T::W * T::LDM : 4];
  __shared__ __attribute__((aligned(16))) float tile[DENSE ? T::TILE_ROWS * T::LDA : 4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int f0 = (lg % LF) * 4;
  const bool fvalid = f0 < p.H;
  const int KP = (p.H + 3) & ~3;
  uint64_t seed = p.seed;
  if (DENSE && p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;
  if (DENSE) load_m<LF, EP, false>(p.M, p.ldM, p.H, Ms);       // read after tile_product's first barrier

  const int64_t ntiles = (p.n_rows + TR - 1) / TR;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                                       // block-uniform
    int64_t io_b[NB];                                           // per gather pass: the row written and whether it is written
    [[maybe_unused]] int64_t hr_b[IDS ? NB : 1];
    bool ov_b[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int lr = b * RPB + wave * GPW + g;                  // the row's place in the tile
      const int64_t i = gt * TR + lr;
      bool rvalid;
      const float4 acc = gather_row<LF, EP, U, MODE>(p, i, sub, f0, fvalid, rvalid);
      float o[4] = {acc.x, acc.y, acc.z, acc.w};
      if constexpr (MODE == MODE_SEGMENT) {
        if (rvalid && sub == 0 && fvalid) *reinterpret_cast<float4*>(p.out + i * p.ldo + f0) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
        // the row written: the hub's own row, or row i
        int64_t io = i;
        if (MODE == MODE_FINISH) io = rvalid ? (int64_t)p.hub_rows[i] : 0;
        const bool ovalid = MODE == MODE_FINISH ? (rvalid && io >= 0 && io < p.n_out) : rvalid;
        const float di = (ovalid && io < p.n_dinv) ? p.dinv[io] : 0.f;
        float4 rv = f4_zero();
        if (ovalid && fvalid) rv = *reinterpret_cast<const float4*>(p.x0 + io * p.ldx0 + f0);
        const float r0[4] = {rv.x, rv.y, rv.z, rv.w};
        const float s = p.beta * di;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          o[c] = s * o[c] + p.alpha * r0[c];                    // the mix; alpha == 1 leaves x0's bits
          if (f0 + c >= p.H) o[c] = 0.f;                        // pad columns of m are 0, in LDS and in memory
        }
        if (sub == 0) {
          *reinterpret_cast<float4*>(tile + lr * T::LDA + f0) = make_float4(o[0], o[1], o[2], o[3]);
          if (p.m_out != nullptr && ovalid && fvalid)
            *reinterpret_cast<float4*>(p.m_out + io * p.ldmo + f0) = make_float4(o[0], o[1], o[2], o[3]);
        }
        io_b[b] = io; ov_b[b] = ovalid;
        if constexpr (IDS) hr_b[b] = ovalid ? p.row_ids[io] : 0;   // the row the dropout hash sees: in flight across the product
      }
    }
    if constexpr (DENSE) {
      tile_product<LF, EP>(tile, Ms, KP, wave, lane);
      // a wave reads back the rows it wrote: its next m rows overwrite (ALIAS) nothing another wave still reads
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int lr = b * RPB + wave * GPW + g;
        const int64_t io = io_b[b];
        if (sub == 0 && ov_b[b] && fvalid) {
          const float4 z = *reinterpret_cast<const float4*>(T::os(tile) + lr * T::LDA + f0);
          float y[4] = {fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
          if (p.thr != 0u) drop4(y, (uint64_t)(IDS ? hr_b[b] : io) * (uint64_t)p.H + (uint64_t)f0, (p.H & 3) == 0, seed, p.thr, p.keep_scale);
#pragma unroll
          for (int c = 0; c < 4; ++c) if (f0 + c >= p.H) y[c] = 0.f;   // pad columns of the row leave as 0
          *reinterpret_cast<float4*>(p.out + io * p.ldo + f0) = make_float4(y[0], y[1], y[2], y[3]);
        }
      }
    }
  }
}

template <int LF, int EP, int U, int MODE, bool IDS>
int launch_conv(const Gcn2Params& p, hipStream_t st) {
  constexpr int TR = Tile<LF, EP>::TR;
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + TR - 1) / TR;
  const int grid = persistent_grid(gcn2_conv_kernel<LF, EP, U, MODE, IDS>, ntiles, &cap);
  hipLaunchKernelGGL((gcn2_conv_kernel<LF, EP, U, MODE, IDS>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

// the row-id instantiation only where an id is read: a dropout is drawn (thr != 0) by a launch that has an epilogue
template <int MODE>
int dispatch_conv(const Gcn2Params& p, hipStream_t st) {
  if (MODE != MODE_SEGMENT && p.row_ids != nullptr && p.thr != 0u)
    return lf_ladder((p.H + 3) / 4, [&](auto LF, auto EP, auto U) { return launch_conv<LF, EP, U, MODE, MODE != MODE_SEGMENT>(p, st); });
  return lf_ladder((p.H + 3) / 4, [&](auto LF, auto EP, auto U) { return launch_conv<LF, EP, U, MODE, false>(p, st); });
}

// ---- backward dense pass -----------------------------------------------------------------------------------------------------
struct Gcn2BwdParams {
  const float* y; int64_t ldy;
  const float* gy; int64_t ldgy;
  const float* M; int64_t ldM;
  int64_t n_rows; int32_t H;
  float alpha, beta, keep_scale;
  float* gz; int64_t ldgz;
  float* t; int64_t ldt;
  float* gx0; int64_t ldgx0;
};

template <int LF, int EP>
__global__ __launch_bounds__(256) void gcn2_bwd_kernel(Gcn2BwdParams p) {
  using T = Tile<LF, EP>;
  constexpr int GL = T::GL, GPW = T::GPW, RPB = T::RPB, NB = T::NB, TR = T::TR;
  __shared__ __attribute__((aligned(16))) float Ms[T::W * T::LDM];
  __shared__ __attribute__((aligned(16))) float tile[T::TILE_ROWS * T::LDA];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int f0 = (lg % LF) * 4;
  const bool fvalid = f0 < p.H;
  const int KP = (p.H + 3) & ~3;
  load_m<LF, EP, true>(p.M, p.ldM, p.H, Ms);

  const int64_t ntiles = (p.n_rows + TR - 1) / TR;
  for (int64_t gt = blockIdx.x; gt < ntiles; gt += gridDim.x) {   // block-uniform trip count
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int lr = b * RPB + wave * GPW + g;
      const int64_t i = gt * TR + lr;
      const bool live = i < p.n_rows && fvalid && sub == 0;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        const float4 y = *reinterpret_cast<const float4*>(p.y + i * p.ldy + f0);
        const float4 dy = *reinterpret_cast<const float4*>(p.gy + i * p.ldgy + f0);
        const float yv[4] = {y.x, y.y, y.z, y.w}, dv[4] = {dy.x, dy.y, dy.z, dy.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = (yv[c] > 0.f && f0 + c < p.H) ? dv[c] * p.keep_scale : 0.f;   // y > 0 <=> kept and positive
        *reinterpret_cast<float4*>(p.gz + i * p.ldgz + f0) = make_float4(o[0], o[1], o[2], o[3]);
      }
      if (sub == 0) *reinterpret_cast<float4*>(tile + lr * T::LDA + f0) = make_float4(o[0], o[1], o[2], o[3]);
    }
    tile_product<LF, EP>(tile, Ms, KP, wave, lane);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int lr = b * RPB + wave * GPW + g;
      const int64_t i = gt * TR + lr;
      if (i < p.n_rows && fvalid && sub == 0) {
        const float4 z = *reinterpret_cast<const float4*>(T::os(tile) + lr * T::LDA + f0);
        float gm[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) if (f0 + c >= p.H) gm[c] = 0.f;
        *reinterpret_cast<float4*>(p.t + i * p.ldt + f0) = make_float4(p.beta * gm[0], p.beta * gm[1], p.beta * gm[2], p.beta * gm[3]);
        *reinterpret_cast<float4*>(p.gx0 + i * p.ldgx0 + f0) =
            make_float4(p.alpha * gm[0], p.alpha * gm[1], p.alpha * gm[2], p.alpha * gm[3]);
      }
    }
  }
}

template <int LF, int EP>
int launch_bwd(const Gcn2BwdParams& p, hipStream_t st) {
  constexpr int TR = Tile<LF, EP>::TR;
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + TR - 1) / TR;
  const int grid = persistent_grid(gcn2_bwd_kernel<LF, EP>, ntiles, &cap);
  hipLaunchKernelGGL((gcn2_bwd_kernel<LF, EP>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

int64_t pad4_ld(int32_t H) { return ((int64_t)H + 3) / 4 * 4; }

}  // namespace

extern "C" size_t bgnn_gcn2_conv_workspace_bytes(int64_t n_seg, int32_t H) {
  if (n_seg <= 0 || H <= 0) return 0;
  return (size_t)n_seg * (size_t)pad4_ld(H) * sizeof(float) + 16;
}

// What both forward entries run: the argument checks, then the ROWS launch and, with hub tables, the SEGMENT and FINISH launches.
// n_tbl: rows of x (the gather's table); row_ids: NULL, or the global id of every output row for the dropout hash.
static int conv_run(const float* x, int64_t ldx, int64_t n_tbl, const float* x0, int64_t ldx0, const float* M, const int32_t* rowptr,
                    const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows, const int64_t* row_ids, int32_t H,
                    float alpha, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                    int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                    const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                    void* ws_opt, size_t ws_bytes, float* m_out_opt, int64_t ldm, float* out, int64_t ldo, hipStream_t st) {
  if (!x || !x0 || !M || !rowptr || !col || !dinv || !out) return BGNN_E_NULL;
  if (n_rows < 0 || H < 1 || H > SLICE || n_tbl < n_rows || n_dinv < n_tbl) return BGNN_E_SHAPE;
  if (!(alpha >= 0.f && alpha <= 1.f) || !(p_drop >= 0.f && p_drop < 1.f)) return BGNN_E_SHAPE;
  if (!ld_ok(ldx, H) || !ld_ok(ldx0, H) || !ld_ok(ldo, H) || (m_out_opt && !ld_ok(ldm, H))) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(x) || !bgnn_aligned16(x0) || !bgnn_aligned16(out) || (m_out_opt && !bgnn_aligned16(m_out_opt)))
    return BGNN_E_ALIGN;
  if (out == x || m_out_opt == x || (m_out_opt && m_out_opt == out)) return BGNN_E_SHAPE;   // other rows still gather x
  const bool hubs = n_hubs > 0;
  if (n_hubs < 0 || n_seg < 0) return BGNN_E_SHAPE;
  float* part = nullptr;
  const int64_t ldw = pad4_ld(H);
  if (hubs) {
    if (hub_threshold < 1 || n_seg < n_hubs) return BGNN_E_SHAPE;
    if (!hub_rows_opt || !hub_seg_ptr_opt || !seg_bounds_opt || !ws_opt) return BGNN_E_NULL;
    if (ws_bytes < (size_t)n_seg * (size_t)ldw * sizeof(float) + 16) return BGNN_E_WORKSPACE;
    part = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws_opt), 16));
  }
  if (n_rows == 0) return 0;
  Gcn2Params p{};
  p.tbl = x; p.ldt = ldx; p.n_tbl = n_tbl;
  p.x0 = x0; p.ldx0 = ldx0;
  p.M = M; p.ldM = ldw;
  p.rowptr = rowptr; p.col = col; p.dinv = dinv; p.n_dinv = n_dinv; p.n_rows = n_rows; p.H = H;
  p.hub_threshold = hubs ? hub_threshold : 0;
  p.n_out = n_rows;
  p.row_ids = row_ids;
  p.alpha = alpha; p.beta = 1.f - alpha;
  p.m_out = m_out_opt; p.ldmo = ldm;
  p.out = out; p.ldo = ldo;
  drop_consts(p_drop, p.thr, p.keep_scale);
  p.seed = seed; p.seed_dev = seed_dev_opt;
  int rc = dispatch_conv<MODE_ROWS>(p, st);
  if (rc != 0 || !hubs) return rc;
  Gcn2Params s = p;                          // partial rows of the segments
  s.rowptr = seg_bounds_opt; s.n_rows = n_seg; s.hub_threshold = 0;
  s.out = part; s.ldo = ldw; s.thr = 0u;
  rc = dispatch_conv<MODE_SEGMENT>(s, st);
  if (rc != 0) return rc;
  Gcn2Params f = p;                          // a hub's partial rows in segment order, then the row's mix, product and epilogue
  f.tbl = part; f.ldt = ldw; f.n_tbl = n_seg;
  f.rowptr = hub_seg_ptr_opt; f.col = nullptr; f.n_rows = n_hubs; f.hub_threshold = 0; f.hub_rows = hub_rows_opt;
  return dispatch_conv<MODE_FINISH>(f, st);
}

// [base, base + (rows - 1) * ld + pad4(H)) of two row-strided views share a float
static bool extents_overlap(const float* a, int64_t rows_a, int64_t lda, const float* b, int64_t rows_b, int64_t ldb, int32_t H) {
  if (rows_a <= 0 || rows_b <= 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a1 = a0 + (uintptr_t)((rows_a - 1) * lda + pad4_ld(H)) * sizeof(float);
  const uintptr_t b1 = b0 + (uintptr_t)((rows_b - 1) * ldb + pad4_ld(H)) * sizeof(float);
  return a0 < b1 && b0 < a1;
}

extern "C" int bgnn_gcn2_conv_f32(const float* x, int64_t ldx, const float* x0, int64_t ldx0, const float* M, const int32_t* rowptr,
                                  const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows, int32_t H, float alpha,
                                  float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                  int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                                  const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                  void* ws_opt, size_t ws_bytes, float* m_out_opt, int64_t ldm, float* out, int64_t ldo,
                                  void* stream) {
  return conv_run(x, ldx, n_rows, x0, ldx0, M, rowptr, col, dinv, n_dinv, n_rows, nullptr, H, alpha, p_drop, seed, seed_dev_opt,
                  hub_threshold, hub_rows_opt, n_hubs, hub_seg_ptr_opt, seg_bounds_opt, n_seg, ws_opt, ws_bytes, m_out_opt, ldm, out,
                  ldo, (hipStream_t)stream);
}

extern "C" int bgnn_gcn2_conv_rows_f32(const float* x, int64_t ldx, int64_t n_tbl, const float* x0, int64_t ldx0, const float* M,
                                       const int32_t* rowptr, const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows,
                                       const int64_t* row_ids_opt, int32_t H, float alpha, float p_drop, uint64_t seed,
                                       const uint64_t* seed_dev_opt, int32_t hub_threshold, const int32_t* hub_rows_opt,
                                       int64_t n_hubs, const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                                       void* ws_opt, size_t ws_bytes, float* m_out_opt, int64_t ldm, float* out, int64_t ldo,
                                       void* stream) {
  // x stays whole while rows are written: neither output may share a float with any of its n_tbl rows, as whole extents (two
  // column slices of one buffer are refused as well)
  if (x && out && H >= 1 && H <= SLICE && n_tbl >= n_rows && n_rows > 0 && ld_ok(ldx, H) && ld_ok(ldo, H)) {
    if (extents_overlap(x, n_tbl, ldx, out, n_rows, ldo, H)) return BGNN_E_SHAPE;
    if (m_out_opt && ld_ok(ldm, H) && extents_overlap(x, n_tbl, ldx, m_out_opt, n_rows, ldm, H)) return BGNN_E_SHAPE;
  }
  return conv_run(x, ldx, n_tbl, x0, ldx0, M, rowptr, col, dinv, n_dinv, n_rows, row_ids_opt, H, alpha, p_drop, seed, seed_dev_opt,
                  hub_threshold, hub_rows_opt, n_hubs, hub_seg_ptr_opt, seg_bounds_opt, n_seg, ws_opt, ws_bytes, m_out_opt, ldm, out,
                  ldo, (hipStream_t)stream);
}

extern "C" int bgnn_gcn2_conv_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, const float* M, int64_t n_rows,
                                      int32_t H, float alpha, float p_drop, float* gz, int64_t ldgz, float* t, int64_t ldt,
                                      float* gx0, int64_t ldgx0, void* stream) {
  if (!y || !grad_y || !M || !gz || !t || !gx0) return BGNN_E_NULL;
  if (n_rows < 0 || H < 1 || H > SLICE) return BGNN_E_SHAPE;
  if (!(alpha >= 0.f && alpha <= 1.f) || !(p_drop >= 0.f && p_drop < 1.f)) return BGNN_E_SHAPE;
  if (!ld_ok(ldy, H) || !ld_ok(ldgy, H) || !ld_ok(ldgz, H) || !ld_ok(ldt, H) || !ld_ok(ldgx0, H)) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(y) || !bgnn_aligned16(grad_y) || !bgnn_aligned16(gz) || !bgnn_aligned16(t) || !bgnn_aligned16(gx0))
    return BGNN_E_ALIGN;
  if (gz == t || gz == gx0 || t == gx0) return BGNN_E_SHAPE;
  if (n_rows == 0) return 0;
  Gcn2BwdParams p{};
  p.y = y; p.ldy = ldy; p.gy = grad_y; p.ldgy = ldgy; p.M = M; p.ldM = pad4_ld(H);
  p.n_rows = n_rows; p.H = H;
  p.alpha = alpha; p.beta = 1.f - alpha;
  uint32_t thr;
  drop_consts(p_drop, thr, p.keep_scale);
  p.gz = gz; p.ldgz = ldgz; p.t = t; p.ldt = ldt; p.gx0 = gx0; p.ldgx0 = ldgx0;
  return lf_ladder((H + 3) / 4, [&](auto LF, auto EP, auto) { return launch_bwd<LF, EP>(p, (hipStream_t)stream); });
}
