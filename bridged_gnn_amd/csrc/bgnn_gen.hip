// DeeperGCN softmax aggregation for gfx950 (wave64): forward and atomic-free backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:130-161): the message, the per-destination per-channel softmax and the root
// add of PyG's GENConv(H, H, aggr='softmax', t=1.0, learn_t=True) -- everything in front of its MLP:
//   v_j = relu(x_j) + 1e-7,   alpha_ij[c] = softmax_{j in row i}(t * v_j[c]),   o_i = sum_j alpha_ij * v_j,   z_i = o_i + x_i
// over the by-destination CSR exactly as given (duplicates are separate messages, self loops ordinary edges, none added).
//   forward : one walk.  Each lane keeps an online state (max of t*v, sum, weighted sum) per channel; the maximum over the U
//             gathered rows of a batch is taken first and the state rescaled once per batch: U + 1 exps per U edges and channel;
//             a batch's sums enter the running sums by a compensated add.
//             Training also stores lse_i = log sum_j exp(t * v_j) and o_i per row and channel.
//   backward: one walk over the by-source view.  The group of source row j holds x_j; per out-edge j -> i it gathers
//             (g_i, lse_i, o_i), forms a = exp(t * v_j - lse_i) (the forward's own rounded products, so a <= 1 up to rounding) and
//             accumulates dv_j += a g_i (1 + t (v_j - o_i)) and, CENTRED, dt += a g_i (v_j - o_i)^2.  dx_j = [x_j > 0] dv_j + g_j is
//             written once; dt leaves as one fp64 partial per block, summed in a fixed order by gen_dt_finish_kernel.
// No float atomics; forward and backward are bit-identical from run to run.  t is read from device memory: the host never waits.
// Algorithmic bytes at width D (Dp = pad4(D)): forward E(4 Dp + 4) + N(8 Dp + 4) (+ 8 N Dp for the tables),
// backward E(12 Dp + 4) + N(12 Dp + 4).
//
// Mapping and launch helpers: bgnn_conv_common.h (the mapping of sage_agg_kernel).  A launch covers at most 128 columns; the
// softmax is per channel, so wider rows run as independent column slices.  A hub row walks as one group.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;

constexpr float GEN_EPS = 1e-7f;       // GENConv's message offset
constexpr int GEN_MAX_BLOCKS = 4096;   // partial slots of one backward launch (a persistent grid has at most 8 blocks per CU)

struct GenParams {
  const float* x; int64_t ldx; int64_t n_tbl;      // node rows (column-offset to the slice), their stride and count
  const int32_t* rowptr; const int32_t* col;       // forward: by destination; backward: by source (t_rowptr, t_dst)
  int64_t n_edges;
  int64_t n_rows;                                  // rows walked (forward: destinations, backward: sources)
  int32_t D;                                       // columns of this slice (<= SLICE)
  const float* t;
  float* z; int64_t ldz;                           // forward output / backward grad_x (column-offset to the slice)
  float* lse; float* o; int64_t lds;               // forward: training tables (SAVE); backward: read
  const float* g; int64_t ldg; int64_t n_dst;      // backward: gradient at z and the row count of (g, lse, o)
  double* partial;                                 // backward: [gridDim.x] dt partials of this launch
};

// exp(x) for the softmax terms (x <= 0 up to rounding, -inf for an empty slot): the hardware exp2 on x * log2(e) formed in two
// pieces, so the argument keeps its low bits -- about 1 ulp over the whole range, where a single rounded product would lose
// |x| * 2^-24 relative; below -104 (and at -inf) the result is 0
__device__ __forceinline__ float gen_exp(float x) {
  const float y = __fmul_rn(x, 1.44269504f);
  const float r = fmaf(x, 1.44269504f, -y) + x * 1.925963033e-8f;
  const float e = __builtin_amdgcn_exp2f(y);
  const float v = fmaf(e, r * 0.693147181f, e);
  return x < -104.f ? 0.f : v;
}

__device__ __forceinline__ void msg4(const float4& r, float (&v)[4]) {
  v[0] = fmaxf(r.x, 0.f) + GEN_EPS; v[1] = fmaxf(r.y, 0.f) + GEN_EPS;
  v[2] = fmaxf(r.z, 0.f) + GEN_EPS; v[3] = fmaxf(r.w, 0.f) + GEN_EPS;
}

template <int LF, int EP, int U, bool SAVE>
__global__ __launch_bounds__(256) void gen_fwd_kernel(GenParams p) {
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
  const float t = *p.t;

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

    // online state per channel: m = running maximum of t*v (-inf: no edge yet), s = sum exp(t*v - m), w = sum exp(t*v - m) v; a
    // batch's sums enter s and w by a compensated add (cs, cw: what the adds so far rounded away), so a hub row of 30 000 edges,
    // whose late batches are tiny next to its running sums, keeps fp32's last digits
    float m[4], s[4], w[4], cs[4], cw[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { m[c] = -INFINITY; s[c] = 0.f; w[c] = 0.f; cs[c] = 0.f; cw[c] = 0.f; }
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.col[e] : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float4 r[U];
      bool ok[U];
      bool any = false;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // ids outside the table are never dereferenced (a malformed CSR gives a wrong sum, not a stray read)
        ok[u] = nid[u] >= 0 && (int64_t)nid[u] < p.n_tbl && fvalid;
        r[u] = ok[u] ? *reinterpret_cast<const float4*>(p.x + (int64_t)nid[u] * p.ldx + f0) : f4_zero();
        any = any || ok[u];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.col[e] : -1;
      }
      if (any) {
        float v[U][4], a[U][4], bm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int u = 0; u < U; ++u) {
          msg4(r[u], v[u]);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            // a ROUNDED product (the backward forms the same bits); the maximum is over t*v, so any sign of t is right
            a[u][c] = ok[u] ? __fmul_rn(t, v[u][c]) : -INFINITY;
            bm[c] = fmaxf(bm[c], a[u][c]);
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float nm = fmaxf(m[c], bm[c]);                  // finite: the batch holds an edge
          const float sc = gen_exp(m[c] - nm);                     // 0 while the state is empty
          float bs = 0.f, bw = 0.f;                             // the batch's own sums
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float e = gen_exp(a[u][c] - nm);                 // 0 for a slot without an edge
            bs += e;
            bw += e * v[u][c];
          }
          const float s0 = s[c] * sc, w0 = w[c] * sc;
          const float ys = bs - cs[c] * sc, yw = bw - cw[c] * sc;
          const float s1 = s0 + ys, w1 = w0 + yw;
          cs[c] = (s1 - s0) - ys; cw[c] = (w1 - w0) - yw;
          m[c] = nm; s[c] = s1; w[c] = w1;
        }
      }
    }
    // the EP sub-groups' states, fixed butterfly; a sub-group that saw no edge (m = -inf) contributes nothing
#pragma unroll
    for (int off = LF; off < GL; off <<= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float m2 = __shfl_xor(m[c], off), s2 = __shfl_xor(s[c], off), w2 = __shfl_xor(w[c], off);
        const float M = fmaxf(m[c], m2);
        const float fa = m[c] == -INFINITY ? 0.f : gen_exp(m[c] - M);
        const float fb = m2 == -INFINITY ? 0.f : gen_exp(m2 - M);
        m[c] = M;
        s[c] = __fmul_rn(s[c], fa) + __fmul_rn(s2, fb);
        w[c] = __fmul_rn(w[c], fa) + __fmul_rn(w2, fb);
      }
    }
    if (rvalid && sub == 0 && fvalid) {
      const float4 xr = *reinterpret_cast<const float4*>(p.x + i * p.ldx + f0);
      const float xi[4] = {xr.x, xr.y, xr.z, xr.w};
      float zz[4], oo[4], ll[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool none = m[c] == -INFINITY;                    // a row without edges: z = x exactly, o = 0, lse = 0
        oo[c] = none ? 0.f : w[c] / s[c];
        ll[c] = none ? 0.f : m[c] + logf(s[c]);
        zz[c] = none ? xi[c] : oo[c] + xi[c];
        if (f0 + c >= p.D) { zz[c] = 0.f; oo[c] = 0.f; ll[c] = 0.f; }   // pad columns leave as 0
      }
      *reinterpret_cast<float4*>(p.z + i * p.ldz + f0) = make_float4(zz[0], zz[1], zz[2], zz[3]);
      if (SAVE) {
        *reinterpret_cast<float4*>(p.lse + i * p.lds + f0) = make_float4(ll[0], ll[1], ll[2], ll[3]);
        *reinterpret_cast<float4*>(p.o + i * p.lds + f0) = make_float4(oo[0], oo[1], oo[2], oo[3]);
      }
    }
  }
}

template <int LF, int EP, int U>
__global__ __launch_bounds__(256) void gen_bwd_kernel(GenParams p) {
  constexpr int GL = LF * EP;
  constexpr int GPW = 64 / GL;
  constexpr int RPB = 4 * GPW;
  __shared__ double wsum[4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int f0 = (lg % LF) * 4;
  const bool fvalid = f0 < p.D;
  const float t = *p.t;
  double dta = 0.0;                                             // this lane's share of dt, over all its rows

  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                                       // block-uniform
    const int64_t j = gt * RPB + wave * GPW + g;
    const bool rvalid = j < p.n_rows;
    int32_t beg = rvalid ? p.rowptr[j] : 0;
    int32_t end = rvalid ? p.rowptr[j + 1] : 0;
    clamp_row(beg, end, p.n_edges);
    const int32_t niter = (end - beg + EP * U - 1) / (EP * U);

    float xj[4] = {0.f, 0.f, 0.f, 0.f}, v[4], a[4];
    if (rvalid && fvalid) {
      const float4 xr = *reinterpret_cast<const float4*>(p.x + j * p.ldx + f0);
      xj[0] = xr.x; xj[1] = xr.y; xj[2] = xr.z; xj[3] = xr.w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = fmaxf(xj[c], 0.f) + GEN_EPS;
      a[c] = __fmul_rn(t, v[c]);                                // the forward's bits
    }
    float dv[4] = {0.f, 0.f, 0.f, 0.f}, dtr[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.col[e] : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float4 gg[U], ll[U], oo[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[u] = nid[u] >= 0 && (int64_t)nid[u] < p.n_dst && fvalid;
        const int64_t d = ok[u] ? (int64_t)nid[u] : 0;
        gg[u] = ok[u] ? *reinterpret_cast<const float4*>(p.g + d * p.ldg + f0) : f4_zero();
        ll[u] = ok[u] ? *reinterpret_cast<const float4*>(p.lse + d * p.lds + f0) : f4_zero();
        oo[u] = ok[u] ? *reinterpret_cast<const float4*>(p.o + d * p.lds + f0) : f4_zero();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.col[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float gv[4] = {gg[u].x, gg[u].y, gg[u].z, gg[u].w}, lv[4] = {ll[u].x, ll[u].y, ll[u].z, ll[u].w},
                    ov[4] = {oo[u].x, oo[u].y, oo[u].z, oo[u].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float ag = ok[u] ? gen_exp(a[c] - lv[c]) * gv[c] : 0.f;   // alpha_ij * g_i; a slot without an edge adds nothing
          const float cd = v[c] - ov[c];
          dv[c] += ag * (1.f + t * cd);
          dtr[c] += ag * cd * cd;                                       // centred: sum alpha g (v - o)^2
        }
      }
    }
    const float4 dvs = ep_sum<LF, GL>(make_float4(dv[0], dv[1], dv[2], dv[3]));
    float rowdt = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) if (f0 + c < p.D) rowdt += dtr[c];     // pad columns take no part
    if (rvalid && fvalid) dta += (double)rowdt;
    if (rvalid && sub == 0 && fvalid) {
      float4 gj = f4_zero();
      if (j < p.n_dst) gj = *reinterpret_cast<const float4*>(p.g + j * p.ldg + f0);
      const float ds[4] = {dvs.x, dvs.y, dvs.z, dvs.w}, gs[4] = {gj.x, gj.y, gj.z, gj.w};
      float dx[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dx[c] = (xj[c] > 0.f ? ds[c] : 0.f) + gs[c];
        if (f0 + c >= p.D) dx[c] = 0.f;
      }
      *reinterpret_cast<float4*>(p.z + j * p.ldz + f0) = make_float4(dx[0], dx[1], dx[2], dx[3]);
    }
  }
  // the block's partial: fixed butterfly inside a wave, then the four waves in order
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) dta += __shfl_xor(dta, off);
  if (lane == 0) wsum[wave] = dta;
  __syncthreads();
  if (threadIdx.x == 0) p.partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// acc = (first ? 0 : acc) + sum of `count` partials in a fixed order; the last slice writes grad_t
__global__ __launch_bounds__(256) void gen_dt_finish_kernel(const double* partial, int count, double* acc, int first, float* grad_t) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int k = threadIdx.x; k < count; k += 256) a += partial[k];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double total = (first ? 0.0 : *acc) + sh[0];
    *acc = total;
    if (grad_t != nullptr) *grad_t = (float)total;
  }
}

template <int LF, int EP, int U, bool SAVE>
int launch_fwd(const GenParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const int grid = persistent_grid(gen_fwd_kernel<LF, EP, U, SAVE>, ntiles, &cap);
  hipLaunchKernelGGL((gen_fwd_kernel<LF, EP, U, SAVE>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

// the backward gathers three rows per edge: half the forward's rows in flight
template <int LF, int EP, int U>
int launch_bwd(const GenParams& p, hipStream_t st, int* grid_out) {
  constexpr int UB = U > 4 ? 4 : U;
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  int grid = persistent_grid(gen_bwd_kernel<LF, EP, UB>, ntiles, &cap);
  if (grid > GEN_MAX_BLOCKS) grid = GEN_MAX_BLOCKS;             // a multiple of 8 still
  *grid_out = grid;
  hipLaunchKernelGGL((gen_bwd_kernel<LF, EP, UB>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

bool edges_ok(int64_t n_edges) { return n_edges >= 0 && n_edges <= (int64_t)INT32_MAX; }

}  // namespace

extern "C" int bgnn_gen_softmax_aggregate_f32(const float* x, int64_t ldx, int64_t n_tbl, const int32_t* rowptr, const int32_t* col,
                                              int64_t n_edges, int64_t n_rows, int32_t H, const float* t, float* lse_opt,
                                              float* o_opt, int64_t lds, float* z, int64_t ldz, void* stream) {
  if (!x || !rowptr || !col || !t || !z) return BGNN_E_NULL;
  if ((lse_opt == nullptr) != (o_opt == nullptr)) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < n_rows || H <= 0 || !edges_ok(n_edges)) return BGNN_E_SHAPE;
  if (!tbl_ok(x, ldx, H) || !tbl_ok(z, ldz, H)) return BGNN_E_ALIGN;
  if (lse_opt && (!tbl_ok(lse_opt, lds, H) || !tbl_ok(o_opt, lds, H))) return BGNN_E_ALIGN;
  if (z == x || (lse_opt && (lse_opt == o_opt || lse_opt == z || o_opt == z || lse_opt == x || o_opt == x))) return BGNN_E_SHAPE;
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  for (int32_t c0 = 0; c0 < H; c0 += SLICE) {
    GenParams p{};
    p.x = x + c0; p.ldx = ldx; p.n_tbl = n_tbl;
    p.rowptr = rowptr; p.col = col; p.n_edges = n_edges; p.n_rows = n_rows;
    p.D = H - c0 < SLICE ? H - c0 : SLICE;
    p.t = t;
    p.z = z + c0; p.ldz = ldz;
    if (lse_opt) { p.lse = lse_opt + c0; p.o = o_opt + c0; p.lds = lds; }
    const int rc = lf_ladder((p.D + 3) / 4, [&](auto LF, auto EP, auto U) {
      return lse_opt ? launch_fwd<LF, EP, U, true>(p, st) : launch_fwd<LF, EP, U, false>(p, st);
    });
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" size_t bgnn_gen_softmax_aggregate_workspace_bytes(int64_t n_src, int32_t H) {
  if (n_src < 0 || H <= 0) return 0;
  return (size_t)(GEN_MAX_BLOCKS + 1) * sizeof(double) + 16;    // the running total, then one launch's partials
}

extern "C" int bgnn_gen_softmax_aggregate_bwd_f32(const float* x, int64_t ldx, int64_t n_src, const float* grad_z, int64_t ldg,
                                                  const float* lse, const float* o, int64_t lds, int64_t n_rows,
                                                  const int32_t* t_rowptr, const int32_t* t_dst, int64_t n_edges, int32_t H,
                                                  const float* t, float* grad_x, int64_t ldgx, float* grad_t, void* ws,
                                                  size_t ws_bytes, void* stream) {
  if (!x || !grad_z || !lse || !o || !t_rowptr || !t_dst || !t || !grad_x || !grad_t || !ws) return BGNN_E_NULL;
  if (n_rows < 0 || n_src < 0 || H <= 0 || !edges_ok(n_edges)) return BGNN_E_SHAPE;
  if (ws_bytes < bgnn_gen_softmax_aggregate_workspace_bytes(n_src, H)) return BGNN_E_WORKSPACE;
  if (!tbl_ok(x, ldx, H) || !tbl_ok(grad_z, ldg, H) || !tbl_ok(lse, lds, H) || !tbl_ok(o, lds, H) || !tbl_ok(grad_x, ldgx, H))
    return BGNN_E_ALIGN;
  if (grad_x == x || grad_x == grad_z || grad_x == lse || grad_x == o) return BGNN_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  double* acc = reinterpret_cast<double*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws), 16));
  double* partial = acc + 1;
  if (n_src == 0) {                                             // nothing walked: grad_t = 0
    hipLaunchKernelGGL(gen_dt_finish_kernel, dim3(1), dim3(256), 0, st, partial, 0, acc, 1, grad_t);
    BGNN_LAUNCH_CHECK();
    return 0;
  }
  for (int32_t c0 = 0; c0 < H; c0 += SLICE) {
    GenParams p{};
    p.x = x + c0; p.ldx = ldx; p.n_tbl = n_src;
    p.rowptr = t_rowptr; p.col = t_dst; p.n_edges = n_edges; p.n_rows = n_src;
    p.D = H - c0 < SLICE ? H - c0 : SLICE;
    p.t = t;
    p.z = grad_x + c0; p.ldz = ldgx;
    p.lse = const_cast<float*>(lse) + c0; p.o = const_cast<float*>(o) + c0; p.lds = lds;
    p.g = grad_z + c0; p.ldg = ldg; p.n_dst = n_rows;
    p.partial = partial;
    int grid = 0;
    const int rc = lf_ladder((p.D + 3) / 4, [&](auto LF, auto EP, auto U) { return launch_bwd<LF, EP, U>(p, st, &grid); });
    if (rc != 0) return rc;
    const bool last = c0 + SLICE >= H;
    hipLaunchKernelGGL(gen_dt_finish_kernel, dim3(1), dim3(256), 0, st, partial, grid, acc, c0 == 0 ? 1 : 0, last ? grad_t : nullptr);
    BGNN_LAUNCH_CHECK();
  }
  return 0;
}
