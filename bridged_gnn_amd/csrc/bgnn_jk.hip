// JKNet for gfx950 (wave64): the scaled-sum GCN conv with its atomic-free backward, the jumping-knowledge head and the routing pass
// of the head's max-mode backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:60-107): the propagate of PyG's GCNConv when it is handed the already
// normalised adj_t_cache (normalised a second time by GCNConv.forward: the diagonal 1 / d2_i is not a product form), its bias, the
// F.relu / F.dropout after every conv, and JumpingKnowledge(cat | max) + Linear + log_softmax.
//
// (a) conv.  The host transforms first (T = x W^T) and this file walks the by-destination CSR WITHOUT any self loop (loops dropped,
//     none appended, duplicates separate messages):
//       forward : out_i = epi( w_i * T_i + s_i * sum_{t in row i} s[col[t]] * T[col[t]] + b )
//       backward: pass A (per destination) g_i from (y_i, dy_i) by conv_bwd_rows_kernel; pass B (per source)
//                 dT_j = w_j * g_j + s_j * sum_{i : j -> i} s_i * g_i -- the forward kernel over the by-source view, no bias, no
//                 epilogue.  No float atomics, bit-identical from run to run.
//     The row's own table row is its root (as gin_agg_kernel): no [N, D] root buffer.  out may be a column slice of a wider buffer
//     (layer l of the model lands in its slice of the layer buffer).  Algorithmic bytes at width D: E(4D + 8) + N(12D + 12) a pass.
//     Mapping, dropout hash, epilogue pieces, backward row kernel and launch helpers: bgnn_conv_common.h.  A launch covers at most
//     128 columns; wider rows run as column slices.  A hub row walks as one lane group; batches of U gathered rows enter the
//     running sum by the compensated add of bgnn_gin.hip.
// (b) head.  X [N, L * Hp] holds layer l in columns [l * Hp, l * Hp + H), pad columns 0.  Per 16-row tile one wave forms the jumped
//     row in registers (cat: the L slices as they lie, K = L * Hp; max: the elementwise max over the slices, lowest l on ties,
//     K = Hp), multiplies it by W (LDS, once per persistent block) with v_mfma_f32_16x16x4_f32 (exact fp32 products, four
//     independent accumulators per 16-column tile: split-K partials summed at the end), adds the bias, applies log_softmax across the
//     16 lanes that hold a row and writes [N, pad4(C)], pad columns 0.  In training max mode also writes the winners (uint8
//     [N, Hp]) and the jumped row once (the backward's dW needs it).  Bytes: N * (4 L Hp + 4 pad4(C)) (+ N * 5 Hp in max training).
// (c) route.  dX[:, l * Hp + c] = winner[i, c] == l ? dJ[i, c] : 0, one streaming pass.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;
constexpr int EPI_RELU = EPI_ACT;      // code 1 here: ReLU, then dropout

struct JkParams {
  const float* tbl; int64_t ldt; int64_t n_tbl;    // table (column-offset to the slice), its stride and row count
  const float* s; const float* w;                  // [n_tbl] each: edge scale and self weight
  const float* bias;                               // one row (column-offset to the slice) or NULL
  const int32_t* rowptr; const int32_t* col; int64_t n_edges;
  int64_t n_rows;
  int32_t D;                                       // columns of this slice (<= SLICE)
  float* out; int64_t ldo;                         // column-offset to the slice
  // dropout after the ReLU: element index = row * d_full + c0 + column (the hash of bgnn_gcn.hip)
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  int32_t d_full; int32_t c0;
};

template <int LF, int EP, int U, int EPI>
__global__ __launch_bounds__(256) void jk_agg_kernel(JkParams p) {
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
    int32_t beg = rvalid ? p.rowptr[i] : 0;
    int32_t end = rvalid ? p.rowptr[i + 1] : 0;
    clamp_row(beg, end, p.n_edges);
    const int32_t niter = (end - beg + EP * U - 1) / (EP * U);  // uniform inside the group

    // the row's own table row and scales: requested in front of the gathers (a row past the table has none)
    const bool has_own = rvalid && i < p.n_tbl;
    float4 own = f4_zero();
    if (has_own && fvalid) own = *reinterpret_cast<const float4*>(p.tbl + i * p.ldt + f0);
    const float s_i = has_own ? p.s[i] : 0.f;
    const float w_i = has_own ? p.w[i] : 0.f;

    // a batch of U scaled rows enters the running sum by a compensated add (see bgnn_gin.hip: a 30 000-edge row keeps fp32's last
    // digits; the walk is gather-bound, the adds are free)
    float4 acc = f4_zero(), cmp = f4_zero();
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.col[e] : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float4 v[U];
      float sc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // ids outside the table are never dereferenced, in s or in tbl (a malformed CSR gives a wrong sum, not a stray read); the
        // scale is requested with the row (as dinv in gcn_agg_kernel): prefetched with the ids it cost 24 VGPRs and a wave per SIMD
        const bool ok = nid[u] >= 0 && (int64_t)nid[u] < p.n_tbl && fvalid;
        v[u] = ok ? *reinterpret_cast<const float4*>(p.tbl + (int64_t)nid[u] * p.ldt + f0) : f4_zero();
        sc[u] = ok ? p.s[nid[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.col[e] : -1;
      }
      float4 b = make_float4(sc[0] * v[0].x, sc[0] * v[0].y, sc[0] * v[0].z, sc[0] * v[0].w);
#pragma unroll
      for (int u = 1; u < U; ++u) {
        b.x = fmaf(sc[u], v[u].x, b.x); b.y = fmaf(sc[u], v[u].y, b.y);
        b.z = fmaf(sc[u], v[u].z, b.z); b.w = fmaf(sc[u], v[u].w, b.w);
      }
      const float4 y = make_float4(b.x - cmp.x, b.y - cmp.y, b.z - cmp.z, b.w - cmp.w);
      const float4 t = make_float4(acc.x + y.x, acc.y + y.y, acc.z + y.z, acc.w + y.w);
      cmp = make_float4((t.x - acc.x) - y.x, (t.y - acc.y) - y.y, (t.z - acc.z) - y.z, (t.w - acc.w) - y.w);
      acc = t;
    }
    acc = ep_sum<LF, GL>(acc);
    float o[4] = {fmaf(s_i, acc.x, w_i * own.x), fmaf(s_i, acc.y, w_i * own.y), fmaf(s_i, acc.z, w_i * own.z),
                  fmaf(s_i, acc.w, w_i * own.w)};
    if (p.bias != nullptr && fvalid) {
      const float4 b = *reinterpret_cast<const float4*>(p.bias + f0);
      o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w;
    }
    if (EPI == EPI_RELU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], 0.f);
      if (p.thr != 0u) {
        const uint64_t e = (uint64_t)(rvalid ? i : 0) * (uint64_t)p.d_full + (uint64_t)(p.c0 + f0);
        drop4(o, e, (p.d_full & 3) == 0, seed, p.thr, p.keep_scale);
      }
    }
    if (rvalid && sub == 0 && fvalid) {
#pragma unroll
      for (int c = 0; c < 4; ++c) if (f0 + c >= p.D) o[c] = 0.f;   // pad columns of the row leave as 0
      *reinterpret_cast<float4*>(p.out + i * p.ldo + f0) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int LF, int EP, int U, int EPI>
int launch_agg(const JkParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const int grid = persistent_grid(jk_agg_kernel<LF, EP, U, EPI>, ntiles, &cap);
  hipLaunchKernelGGL((jk_agg_kernel<LF, EP, U, EPI>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

bool edges_ok(int64_t n_edges) { return n_edges >= 0 && n_edges <= (int64_t)INT32_MAX; }

// the column slices of one walk; the callers have checked shapes and alignment
int run_agg(const float* tbl, int64_t ldt, int64_t n_tbl, const float* s, const float* w, const float* bias, const int32_t* rowptr,
            const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t D, int epilogue, float p_drop, uint64_t seed,
            const uint64_t* seed_dev, float* out, int64_t ldo, hipStream_t st) {
  for (int32_t c0 = 0; c0 < D; c0 += SLICE) {
    JkParams p{};
    p.tbl = tbl + c0; p.ldt = ldt; p.n_tbl = n_tbl;
    p.s = s; p.w = w;
    p.bias = bias ? bias + c0 : nullptr;
    p.rowptr = rowptr; p.col = col; p.n_edges = n_edges; p.n_rows = n_rows;
    p.D = D - c0 < SLICE ? D - c0 : SLICE;
    p.out = out + c0; p.ldo = ldo;
    drop_consts(p_drop, p.thr, p.keep_scale);
    p.seed = seed; p.seed_dev = seed_dev; p.d_full = D; p.c0 = c0;
    const int rc = lf_ladder((p.D + 3) / 4, [&](auto LF, auto EP, auto U) {
      return epilogue == EPI_RELU ? launch_agg<LF, EP, U, EPI_RELU>(p, st) : launch_agg<LF, EP, U, EPI_NONE>(p, st);
    });
    if (rc != 0) return rc;
  }
  return 0;
}

// ---- the head ----------------------------------------------------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;
enum { JK_CAT = 0, JK_MAX = 1 };
constexpr int JK_HEAD_LDS_BYTES = 65536;   // W in LDS: 16 * NCT * K16 floats
constexpr int JK_MAX_LAYERS = 8;

struct HeadParams {
  const float* x; int64_t ldx;            // [N, L * Hp]
  int64_t n_rows;
  int32_t L, Hp, K, K16;                  // K = L * Hp (cat) | Hp (max); K16 = K rounded up to 16
  const float* W; int64_t ldw;            // [C, ldw >= K], the padded layout (pad columns 0)
  const float* bias;                      // [C] or NULL
  int32_t C, Cp;
  int log_softmax;
  float* out; int64_t ldo;                // [N, >= Cp]
  uint8_t* win;                           // max training: [N, Hp] or NULL
  float* jump; int64_t ldj;               // max training: [N, >= Hp] or NULL
};

// LDS layout of W: float4 slot (ct, q, c) at ((ct * KQ + q) * 16 + c), q = k / 4, c = class % 16: the 16 lanes of a k-quarter read
// 256 contiguous bytes, the four quarters 1 KB -- no bank conflict and no padding
template <int NCT, int MODE>
__global__ __launch_bounds__(256) void jk_head_kernel(HeadParams p) {
  extern __shared__ __attribute__((aligned(16))) float Ws[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int KQ = p.K16 / 4;
  for (int idx = threadIdx.x; idx < NCT * KQ * 16; idx += 256) {
    const int c = idx & 15, q = (idx >> 4) % KQ, ct = (idx >> 4) / KQ;
    const int cls = ct * 16 + c;
    float4 v = f4_zero();
    if (cls < p.C && 4 * q < p.K) v = *reinterpret_cast<const float4*>(p.W + (int64_t)cls * p.ldw + 4 * q);
    reinterpret_cast<float4*>(Ws)[idx] = v;
  }
  __syncthreads();
  const float4* W4 = reinterpret_cast<const float4*>(Ws);
  float bv[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) bv[ct] = (p.bias != nullptr && ct * 16 + r16 < p.C) ? p.bias[ct * 16 + r16] : 0.f;

  const int64_t ntiles = (p.n_rows + 63) / 64;                  // a block iteration: 4 waves x 16 rows
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;
    const int64_t row0 = gt * 64 + wave * 16;
    if (row0 >= p.n_rows) continue;                             // wave-uniform: nothing below crosses waves
    const int64_t ir = row0 + r16;                              // the A row of this lane
    const bool avalid = ir < p.n_rows;
    const float* xr = p.x + (avalid ? ir : 0) * p.ldx;
    f32x4 acc[NCT][4];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ct][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    // 16 columns of the jumped row per step: this lane holds columns k..k+3 of row r16, k = 16 j + 4 kq, and feeds them to four
    // MFMAs (element e of every lane: the product does not care which four k meet in one instruction, W is read to match)
    for (int k0 = 0; k0 < p.K16; k0 += 16) {
      const int k = k0 + 4 * kq;
      float4 a = f4_zero();
      if (MODE == JK_CAT) {
        if (avalid && k < p.K) a = *reinterpret_cast<const float4*>(xr + k);
      } else {
        uint32_t wl = 0u;
        if (avalid && k < p.K) {
          a = *reinterpret_cast<const float4*>(xr + k);
          for (int l = 1; l < p.L; ++l) {                       // strict >: the lowest layer wins a tie (torch's rule)
            const float4 b = *reinterpret_cast<const float4*>(xr + (int64_t)l * p.Hp + k);
            if (b.x > a.x) { a.x = b.x; wl = (wl & 0xFFFFFF00u) | (uint32_t)l; }
            if (b.y > a.y) { a.y = b.y; wl = (wl & 0xFFFF00FFu) | ((uint32_t)l << 8); }
            if (b.z > a.z) { a.z = b.z; wl = (wl & 0xFF00FFFFu) | ((uint32_t)l << 16); }
            if (b.w > a.w) { a.w = b.w; wl = (wl & 0x00FFFFFFu) | ((uint32_t)l << 24); }
          }
          if (p.win != nullptr) *reinterpret_cast<uint32_t*>(p.win + ir * p.Hp + k) = wl;
          if (p.jump != nullptr) *reinterpret_cast<float4*>(p.jump + ir * p.ldj + k) = a;
        }
      }
      const int q = k >> 2;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const float4 b = W4[(ct * KQ + q) * 16 + r16];
        acc[ct][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[ct][0], 0, 0, 0);
        acc[ct][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[ct][1], 0, 0, 0);
        acc[ct][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[ct][2], 0, 0, 0);
        acc[ct][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[ct][3], 0, 0, 0);
      }
    }
    // C/D layout: column = lane & 15 (class ct * 16 + r16), row = 4 * (lane >> 4) + register
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float z[NCT];
      float m = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        z[ct] = ((acc[ct][0][r] + acc[ct][1][r]) + (acc[ct][2][r] + acc[ct][3][r])) + bv[ct];
        if (ct * 16 + r16 < p.C) m = fmaxf(m, z[ct]);
      }
      if (p.log_softmax) {
        m = bgnn::group_max<16>(m);
        float se = 0.f;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) if (ct * 16 + r16 < p.C) se += expf(z[ct] - m);
        se = bgnn::group_sum<16>(se);
        const float lse = m + logf(se);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) z[ct] -= lse;
      }
      const int64_t orow = row0 + 4 * kq + r;
      if (orow < p.n_rows) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const int cls = ct * 16 + r16;
          if (cls < p.Cp) p.out[orow * p.ldo + cls] = cls < p.C ? z[ct] : 0.f;   // pad columns leave as 0
        }
      }
    }
  }
}

template <int NCT, int MODE>
int launch_head(const HeadParams& p, hipStream_t st) {
  // residency: what the registers allow (queried once, without LDS), what this launch's W leaves room for, at most 8 blocks a CU
  static int cache[3] = {0, 0, 0};                             // blocks per CU by registers, LDS bytes per CU, CUs; [0] != 0: filled
  const int lds = NCT * 16 * p.K16 * (int)sizeof(float);
  if (__atomic_load_n(&cache[0], __ATOMIC_ACQUIRE) == 0) {
    int per_cu = 0, dev = 0, by_regs = 8, lds_cu = JK_HEAD_LDS_BYTES, ncu = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, jk_head_kernel<NCT, MODE>, 256, 0) == hipSuccess && per_cu >= 1) {
      by_regs = per_cu > 8 ? 8 : per_cu;
      ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : ncu;
      if ((int64_t)prop.maxSharedMemoryPerMultiProcessor > (int64_t)lds_cu) lds_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    }
    cache[1] = lds_cu; cache[2] = ncu;
    __atomic_store_n(&cache[0], by_regs, __ATOMIC_RELEASE);
  }
  int per_cu = __atomic_load_n(&cache[0], __ATOMIC_ACQUIRE);
  if (cache[1] / lds < per_cu) per_cu = cache[1] / lds;
  if (per_cu < 1) per_cu = 1;
  int cap = per_cu * cache[2] / 8 * 8;
  if (cap < 8) cap = 8;
  const int64_t ntiles = (p.n_rows + 63) / 64;
  int64_t grid = ntiles < cap ? (ntiles + 7) / 8 * 8 : cap;
  if (grid < 8) grid = 8;
  hipLaunchKernelGGL((jk_head_kernel<NCT, MODE>), dim3((unsigned)grid), dim3(256), (size_t)lds, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

// ---- the routing pass of max mode's backward ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jk_max_route_kernel(const float* dj, int64_t ldj, const uint8_t* win, int64_t n_rows, int32_t L,
                                                           int32_t Hp, float* dx, int64_t ldx) {
  const int64_t nq = Hp / 4, total = n_rows * nq;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t i = t / nq;
    const int k = (int)(t - i * nq) * 4;
    const float4 g = *reinterpret_cast<const float4*>(dj + i * ldj + k);
    const uint32_t wl = *reinterpret_cast<const uint32_t*>(win + i * Hp + k);
    for (int l = 0; l < L; ++l) {
      const uint32_t ul = (uint32_t)l;
      const float4 o = make_float4((wl & 0xFFu) == ul ? g.x : 0.f, ((wl >> 8) & 0xFFu) == ul ? g.y : 0.f,
                                   ((wl >> 16) & 0xFFu) == ul ? g.z : 0.f, (wl >> 24) == ul ? g.w : 0.f);
      *reinterpret_cast<float4*>(dx + i * ldx + (int64_t)l * Hp + k) = o;
    }
  }
}

}  // namespace

extern "C" int bgnn_jk_gcn_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* s, const float* w,
                                         const float* bias_opt, const int32_t* rowptr, const int32_t* col, int64_t n_edges,
                                         int64_t n_rows, int32_t D, int epilogue, float p_drop, uint64_t seed,
                                         const uint64_t* seed_dev_opt, float* out, int64_t ldo, void* stream) {
  if (!tbl || !s || !w || !rowptr || !col || !out) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < n_rows || D <= 0 || !edges_ok(n_edges)) return BGNN_E_SHAPE;
  if (epilogue != EPI_NONE && epilogue != EPI_RELU) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if (!tbl_ok(tbl, ldt, D) || !tbl_ok(out, ldo, D) || (bias_opt && !bgnn_aligned16(bias_opt))) return BGNN_E_ALIGN;
  if (out == tbl) return BGNN_E_SHAPE;
  if (n_rows == 0) return 0;
  return run_agg(tbl, ldt, n_tbl, s, w, bias_opt, rowptr, col, n_edges, n_rows, D, epilogue, p_drop, seed, seed_dev_opt, out, ldo,
                 (hipStream_t)stream);
}

extern "C" int bgnn_jk_gcn_aggregate_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, int64_t n_rows,
                                             const int32_t* t_rowptr, const int32_t* t_col, int64_t n_edges, int64_t n_src,
                                             const float* s, const float* w, int32_t D, int epilogue, float p_drop, float* g,
                                             int64_t ldg, float* grad_tbl, int64_t ldgt, void* stream) {
  if (!grad_y || !t_rowptr || !t_col || !s || !w || !g || !grad_tbl) return BGNN_E_NULL;
  if (epilogue != EPI_NONE && epilogue != EPI_RELU) return BGNN_E_SHAPE;
  if (epilogue != EPI_NONE && !y) return BGNN_E_NULL;
  // s and w are indexed by source and by destination row: one node set
  if (n_rows < 0 || n_src != n_rows || D <= 0 || !edges_ok(n_edges)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, D)) return rc;
  if ((y && !tbl_ok(y, ldy, D)) || !tbl_ok(grad_y, ldgy, D) || !tbl_ok(g, ldg, D) || !tbl_ok(grad_tbl, ldgt, D)) return BGNN_E_ALIGN;
  if (grad_tbl == g || grad_tbl == grad_y || (y && grad_tbl == y)) return BGNN_E_SHAPE;
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  BwdRowsParams p{};
  p.y = y; p.ldy = ldy; p.gy = grad_y; p.ldgy = ldgy; p.n_rows = n_rows; p.D = D;
  uint32_t thr;
  drop_consts(p_drop, thr, p.keep_scale);
  p.g = g; p.ldg = ldg;
  if (const int rc = dispatch_bwd_rows<false>(epilogue, p, st)) return rc;   // pass A: g
  // pass B: the forward walk over the by-source view
  return run_agg(g, ldg, n_rows, s, w, nullptr, t_rowptr, t_col, n_edges, n_src, D, EPI_NONE, 0.f, 0, nullptr, grad_tbl, ldgt, st);
}

extern "C" int bgnn_jk_head_supported(int32_t L, int32_t H, int32_t C, int mode) {
  if (L < 1 || L > JK_MAX_LAYERS || H < 1 || C < 1 || C > 32 || (mode != JK_CAT && mode != JK_MAX)) return 0;
  const int64_t Hp = ((int64_t)H + 3) / 4 * 4;
  const int64_t K = mode == JK_CAT ? (int64_t)L * Hp : Hp;
  const int64_t K16 = (K + 15) / 16 * 16;
  const int64_t nct = C <= 16 ? 1 : 2;
  return nct * 16 * K16 * (int64_t)sizeof(float) <= JK_HEAD_LDS_BYTES ? 1 : 0;
}

extern "C" int bgnn_jk_head_f32(const float* x, int64_t ldx, int64_t n_rows, int32_t L, int32_t H, int mode, const float* W,
                                int64_t ldw, const float* bias_opt, int32_t C, int log_softmax, float* out, int64_t ldo,
                                uint8_t* win_opt, float* jump_opt, int64_t ldj, void* stream) {
  if (!x || !W || !out) return BGNN_E_NULL;
  if (n_rows < 0 || !bgnn_jk_head_supported(L, H, C, mode)) return BGNN_E_SHAPE;
  if (mode != JK_MAX && (win_opt || jump_opt)) return BGNN_E_SHAPE;
  const int32_t Hp = (H + 3) / 4 * 4, Cp = (C + 3) / 4 * 4;
  const int32_t K = mode == JK_CAT ? L * Hp : Hp;
  if (!bgnn_aligned16(x) || (ldx & 3) != 0 || ldx < (int64_t)L * Hp) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(W) || (ldw & 3) != 0 || ldw < K) return BGNN_E_ALIGN;
  if (ldo < Cp) return BGNN_E_ALIGN;
  if (win_opt && (reinterpret_cast<uintptr_t>(win_opt) & 3u) != 0) return BGNN_E_ALIGN;
  if (jump_opt && (!bgnn_aligned16(jump_opt) || (ldj & 3) != 0 || ldj < Hp)) return BGNN_E_ALIGN;
  if (n_rows == 0) return 0;
  HeadParams p{};
  p.x = x; p.ldx = ldx; p.n_rows = n_rows; p.L = L; p.Hp = Hp; p.K = K; p.K16 = (K + 15) / 16 * 16;
  p.W = W; p.ldw = ldw; p.bias = bias_opt; p.C = C; p.Cp = Cp; p.log_softmax = log_softmax ? 1 : 0;
  p.out = out; p.ldo = ldo; p.win = win_opt; p.jump = jump_opt; p.ldj = ldj;
  hipStream_t st = (hipStream_t)stream;
  if (C <= 16) return mode == JK_CAT ? launch_head<1, JK_CAT>(p, st) : launch_head<1, JK_MAX>(p, st);
  return mode == JK_CAT ? launch_head<2, JK_CAT>(p, st) : launch_head<2, JK_MAX>(p, st);
}

extern "C" int bgnn_jk_max_route_f32(const float* grad_jump, int64_t ldj, const uint8_t* win, int64_t n_rows, int32_t L, int32_t H,
                                     float* grad_x, int64_t ldx, void* stream) {
  if (!grad_jump || !win || !grad_x) return BGNN_E_NULL;
  if (n_rows < 0 || L < 1 || L > JK_MAX_LAYERS || H < 1) return BGNN_E_SHAPE;
  const int32_t Hp = (H + 3) / 4 * 4;
  if (!bgnn_aligned16(grad_jump) || (ldj & 3) != 0 || ldj < Hp || !bgnn_aligned16(grad_x) || (ldx & 3) != 0 ||
      ldx < (int64_t)L * Hp || (reinterpret_cast<uintptr_t>(win) & 3u) != 0)
    return BGNN_E_ALIGN;
  if (n_rows == 0) return 0;
  int64_t blocks = (n_rows * (Hp / 4) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(jk_max_route_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad_jump, ldj, win, n_rows, L,
                     Hp, grad_x, ldx);
  BGNN_LAUNCH_CHECK();
  return 0;
}
