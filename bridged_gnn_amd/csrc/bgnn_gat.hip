// GAT attention aggregation for gfx950 (wave64): forward and atomic-free backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:404-438): PyG GATConv's per-destination softmax over
// leaky_relu(<T_j, att_src> + <T_i, att_dst>), the attention dropout on the edge coefficients, propagate(aggr='add') + bias, and
// the F.elu / F.dropout between the convs and the closing F.log_softmax.  The host transforms first (T = x W^T, [N, H*C]) and
// this file walks the by-destination CSR with exactly one self loop per row (bgnn_build_dst_csr with rewrite_self_loops).
//
// A VIRTUAL ROW is one (row i, head h) pair, v = i*H + h: its neighbour rows are the C floats at tbl[j*ldt + h*C], its edge
// coefficients the words at [t*H + h].  Every edge-walking kernel gives a virtual row to one lane group; blocks are persistent
// over the XCD-balanced segment order of bgnn_common.h.  Head slices that are not 16-byte aligned (C % 4 != 0) are read and
// written with scalar accesses, aligned ones with float4.
//
// Forward, three launches:
//   scores    s_src[n,h] = <T[n,h,:], att_src[h,:]>, s_dst likewise: one read of T.
//   alpha     per virtual row, 8 lanes stride the row's edges: an online (max, sum) over e = leaky_relu(s_src[j,h] + s_dst[i,h]),
//             merged over the lanes, kept as state[i,h] = (max, denominator >= 1); a second sweep writes the post-dropout
//             coefficient a~ = exp(e - max) / den * m to coef[t*H + h] (m from the counter hash at element t*H + h).
//   aggregate out[i,h,:] = sum_t coef[t,h] * T[col[t],h,:] (+ bias, epilogue): LF lanes span the head's columns, EP sub-groups walk
//             different edges, U rows in flight (the mapping of bgnn_conv_common.h).  The coefficients stream, only T rows are gathered.
// Backward, three launches (no float atomics):
//   rows      g = the gradient at the conv output (ELU derivative from the kept pre-activation, the feature mask REDRAWN from
//             (seed, row, col); log_softmax rule from the pre-activation), r[i,h] = <g[i,h,:], pre[i,h,:] - bias[h,:]>.
//   edges     by-destination: dot = <g[i,h,:], T[j,h,:]>, da = m * dot, de = alpha * (da - r), dz = de * (z > 0 ? 1 : slope);
//             dz goes to a [E', H] workspace; its row sum ds_dst[i,h] is formed from the row's own per-side sums (see there).
//   gather    by-source (t_rowptr, t_eid, t_dst): the aggregate kernel with coefficient index t_eid[u]:
//             dT[j,h,:] = sum_u coef[t_eid[u],h] * g[t_dst[u],h,:] and ds_src[j,h] = sum_u dz[t_eid[u],h].
// Rows of a larger graph (row_id_opt / edge_base_opt of the two entries, a rank's rows of a node partition): both
// masks are functions of a position, and a rank's local positions are not the whole graph's.  The ROW_ID / EDGE_ID kernels hash
// the feature mask at row_id[i] * (H*C) + column and the attention mask at (edge_base[i] + (t - rowptr[i])) * H + h: the row's
// GLOBAL id and the GLOBAL position of its first edge, both read once per virtual row.  The ids feed the hash only, never an address.
// Without ids (or without dropout) the entries launch the instantiations without the flags.  The backward takes n_rows destination rows and n_src >= n_rows
// source rows (a rank's extended graph: its halo slots are sources without in-edges); see bgnn.h for which operand is over which.
// Ids outside their table are never dereferenced and a row's edge range is cut to the edge arrays: a malformed CSR (ids or rowptr)
// gives a wrong sum, not a stray read or write.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;

// ---- scores ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gat_scores_kernel(const float* __restrict__ tbl, int64_t ldt, int64_t n, int H, int C,
                                                         const float* __restrict__ att_src, const float* __restrict__ att_dst,
                                                         float* __restrict__ s_src, float* __restrict__ s_dst) {
  const int64_t total = n * H;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = v / H;
    const int h = (int)(v - i * H);
    const float* t = tbl + i * ldt + (int64_t)h * C;
    const float* as = att_src + (int64_t)h * C;
    const float* ad = att_dst + (int64_t)h * C;
    float a = 0.f, b = 0.f;
    for (int c = 0; c < C; ++c) {                 // fixed order: deterministic
      const float x = t[c];
      a += x * as[c];
      b += x * ad[c];
    }
    s_src[v] = a;
    s_dst[v] = b;
  }
}

// ---- softmax state and post-dropout coefficients --------------------------------------------------------------------
struct AlphaParams {
  const float* s_src; int64_t n_src;               // [n_src, H]
  const float* s_dst;                              // [n_rows, H]
  const int32_t* rowptr; const int32_t* col;
  int64_t n_rows; int64_t n_edges; int32_t H;
  float slope;
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  float* state;                                    // [n_rows, H, 2] = (max, denominator)
  float* coef;                                     // [E', H]
  const int64_t* edge_base;                        // EDGE_ID: position of the row's first edge in the whole graph's CSR, [n_rows]
};

template <int GL, int U, bool EDGE_ID = false>
__global__ __launch_bounds__(256) void gat_alpha_kernel(AlphaParams p) {
  constexpr int RPB = 256 / GL;                    // virtual rows per block iteration
  const int g = threadIdx.x / GL;
  const int l = threadIdx.x % GL;
  uint64_t seed = p.seed;
  if (p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;
  const int64_t nv = p.n_rows * p.H;
  const int64_t ntiles = (nv + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                          // block-uniform
    const int64_t v = gt * RPB + g;
    const bool valid = v < nv;
    const int64_t i = valid ? v / p.H : 0;
    const int h = valid ? (int)(v - i * p.H) : 0;
    int32_t beg = 0, end = 0;
    float sd = 0.f;
    if (valid) { beg = p.rowptr[i]; end = p.rowptr[i + 1]; sd = p.s_dst[v]; }
    int64_t eshift = 0;                            // EDGE_ID: hashed position of edge e = e + eshift (from the raw rowptr[i])
    if (EDGE_ID && valid) eshift = p.edge_base[i] - (int64_t)beg;
    clamp_row(beg, end, p.n_edges);
    float m = -INFINITY, s = 0.f;
    for (int32_t e0 = beg + l; e0 < end; e0 += GL * U) {
      float z[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + u * GL;
        const int32_t j = e < end ? p.col[e] : -1;
        ok[u] = j >= 0 && (int64_t)j < p.n_src;
        z[u] = ok[u] ? p.s_src[(int64_t)j * p.H + h] + sd : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
        const float x = leaky(z[u], p.slope);
        if (x > m) { s = s * expf(m - x) + 1.f; m = x; }      // m = -inf: s = 0 stays 0 before the + 1
        else s += expf(x - m);
      }
    }
    // (max, sum) of the row from the lanes' partial pairs: fixed butterfly, every lane of the wave takes part
#pragma unroll
    for (int off = 1; off < GL; off <<= 1) {
      const float m2 = __shfl_xor(m, off), s2 = __shfl_xor(s, off);
      softmax_merge(m, s, m2, s2);
    }
    if (valid && l == 0) {
      p.state[2 * v] = m;
      p.state[2 * v + 1] = s;
    }
    for (int32_t e0 = beg + l; e0 < end; e0 += GL * U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + u * GL;
        if (e >= end || (int64_t)e >= p.n_edges) continue;      // an offset past the coefficient array is never written
        const int32_t j = p.col[e];
        float a = 0.f;
        if (j >= 0 && (int64_t)j < p.n_src) {
          const float zz = p.s_src[(int64_t)j * p.H + h] + sd;
          const float x = leaky(zz, p.slope);
          a = expf(x - m) / s;
          const uint64_t el = (EDGE_ID ? (uint64_t)((int64_t)e + eshift) : (uint64_t)e) * (uint64_t)p.H + (uint64_t)h;
          if (p.thr != 0u) a = drop_bits(el, seed) >= p.thr ? a * p.keep_scale : 0.f;
        }
        p.coef[(int64_t)e * p.H + h] = a;
      }
    }
  }
}

// ---- weighted gather: the forward aggregation and the backward's by-source pass ------------------------------------
struct AggParams {
  const float* tbl; int64_t ldt; int64_t n_tbl;    // gathered rows (T, or g in the backward)
  const float* bias;                               // [H*C] or NULL
  const int32_t* rowptr; const int32_t* col;       // the view walked; col = the gathered row of an edge
  const int32_t* eid; int64_t n_edges;             // BWD: position of the edge in the coefficient arrays (forward: its own offset)
  const float* coef;                               // [E', H]
  const float* dz; float* dsum;                    // BWD: [E', H] summed per virtual row into dsum [n_rows, H]
  int64_t n_rows; int32_t H; int32_t C; int32_t npad;
  float* out; int64_t ldo;
  float* pre; int64_t ldp;                         // the conv output before the epilogue, or NULL
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  const int64_t* row_id;                           // ROW_ID: dropout row of output row i (element index row_id[i] * (H*C) + column)
};

template <int LF, int EP, int U, int EPI, bool BWD, bool ROW_ID = false>
__global__ __launch_bounds__(256) void gat_agg_kernel(AggParams p) {
  constexpr int GL = LF * EP;
  constexpr int GPW = 64 / GL;
  constexpr int RPB = 4 * GPW;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int k0 = (lg % LF) * 4;
  const bool vec = (p.C & 3) == 0;
  uint64_t seed = p.seed;
  if (EPI == EPI_ELU && p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;

  const int64_t nv = p.n_rows * p.H;
  const int64_t ntiles = (nv + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                                       // block-uniform
    const int64_t v = gt * RPB + wave * GPW + g;
    const bool valid = v < nv;
    const int64_t i = valid ? v / p.H : 0;
    const int h = valid ? (int)(v - i * p.H) : 0;
    const int64_t hoff = (int64_t)h * p.C;
    int32_t beg = 0, end = 0;
    if (valid) { beg = p.rowptr[i]; end = p.rowptr[i + 1]; }
    clamp_row(beg, end, p.n_edges);
    const int32_t niter = (end - beg + EP * U - 1) / (EP * U);  // uniform inside the group

    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float dsum = 0.f;
    int32_t nid[U], wid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.col[e] : -1;
      wid[u] = BWD ? (e < end ? p.eid[e] : -1) : e;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float x[U][4];
      float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = nid[u] >= 0 && (int64_t)nid[u] < p.n_tbl && wid[u] >= 0 && (int64_t)wid[u] < p.n_edges;
        load4(p.tbl + (int64_t)(ok ? nid[u] : 0) * p.ldt + hoff, k0, p.C, vec, ok, x[u]);
        w[u] = ok ? p.coef[(int64_t)wid[u] * p.H + h] : 0.f;
        if (BWD) dsum += ok ? p.dz[(int64_t)wid[u] * p.H + h] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.col[e] : -1;
        wid[u] = BWD ? (e < end ? p.eid[e] : -1) : e;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += w[u] * x[u][c];
      }
    }
#pragma unroll
    for (int off = LF; off < GL; off <<= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += __shfl_xor(acc[c], off);
      if (BWD) dsum += __shfl_xor(dsum, off);
    }
    float o[4] = {acc[0], acc[1], acc[2], acc[3]};
    if (p.bias != nullptr) {
      float b[4];
      load4(p.bias + hoff, k0, p.C, vec, true, b);
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] += b[c];
    }
    const bool writer = valid && sub == 0;
    if (p.pre != nullptr && writer) {
      store4(p.pre + i * p.ldp + hoff, k0, p.C, vec, o);
      if (h == p.H - 1 && lg == 0)
        for (int q = 0; q < p.npad; ++q) p.pre[i * p.ldp + (int64_t)p.H * p.C + q] = 0.f;
    }
    if (EPI == EPI_ELU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = o[c] > 0.f ? o[c] : expm1f(o[c]);
      if (p.thr != 0u) {
        const uint64_t e = (uint64_t)(ROW_ID ? (valid ? p.row_id[i] : 0) : i) * (uint64_t)(p.H * p.C) + (uint64_t)(hoff + k0);
        // drop4's law, in place: through the shared function this kernel's forward at (3, 64) measured 0.9 % slower
        if (vec) {                                                // the four columns share one word pair (as bgnn_norm.hip)
          uint32_t w0, w1;
          drop_words(e >> 2, seed, w0, w1);
          const uint32_t bits[4] = {w0 & 0xFFFFu, w0 >> 16, w1 & 0xFFFFu, w1 >> 16};
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = bits[c] >= p.thr ? o[c] * p.keep_scale : 0.f;
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = drop_bits(e + c, seed) >= p.thr ? o[c] * p.keep_scale : 0.f;
        }
      }
    } else if (EPI == EPI_LOGSOFTMAX) {
      log_softmax4<LF>(o, k0, p.C);   // H == 1: the whole row (C <= 4*LF) sits in the LF lanes of the group
    }
    if (writer) {
      store4(p.out + i * p.ldo + hoff, k0, p.C, vec, o);
      if (h == p.H - 1 && lg == 0)                                // pad columns of the row leave as 0
        for (int q = 0; q < p.npad; ++q) p.out[i * p.ldo + (int64_t)p.H * p.C + q] = 0.f;
      if (BWD && lg == 0) p.dsum[v] = dsum;
    }
  }
}

// ---- backward edge pass over the by-destination CSR: dz per edge, ds_dst per virtual row ---------------------------
struct EdgeParams {
  const float* tbl; int64_t ldt; int64_t n_tbl;
  const float* g; int64_t ldg;
  const float* s_src; const float* s_dst; const float* state; const float* r;
  const int32_t* rowptr; const int32_t* col;
  int64_t n_rows; int64_t n_edges; int32_t H; int32_t C;
  float slope;
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;
  float* dz;                                       // [E', H]
  float* ds_dst;                                   // [n_rows, H]
  const int64_t* edge_base;                        // EDGE_ID: as AlphaParams
};

template <int LF, int EP, int U, bool EDGE_ID = false>
__global__ __launch_bounds__(256) void gat_bwd_edge_kernel(EdgeParams p) {
  constexpr int GL = LF * EP;
  constexpr int GPW = 64 / GL;
  constexpr int RPB = 4 * GPW;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int k0 = (lg % LF) * 4;
  const bool vec = (p.C & 3) == 0;
  uint64_t seed = p.seed;
  if (p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;

  const int64_t nv = p.n_rows * p.H;
  const int64_t ntiles = (nv + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                                       // block-uniform
    const int64_t v = gt * RPB + wave * GPW + g;
    const bool valid = v < nv;
    const int64_t i = valid ? v / p.H : 0;
    const int h = valid ? (int)(v - i * p.H) : 0;
    const int64_t hoff = (int64_t)h * p.C;
    int32_t beg = 0, end = 0;
    float sd = 0.f, mx = 0.f, den = 1.f, rr = 0.f;
    float gi[4];
    load4(p.g + i * p.ldg + hoff, k0, p.C, vec, valid, gi);
    if (valid) {
      beg = p.rowptr[i]; end = p.rowptr[i + 1];
      sd = p.s_dst[v]; mx = p.state[2 * v]; den = p.state[2 * v + 1]; rr = p.r[v];
    }
    int64_t eshift = 0;                                         // EDGE_ID: hashed position of edge e = e + eshift (raw rowptr[i])
    if (EDGE_ID && valid) eshift = p.edge_base[i] - (int64_t)beg;
    clamp_row(beg, end, p.n_edges);
    const int32_t niter = (end - beg + EP * U - 1) / (EP * U);  // uniform inside the group
    float sp = 0.f, sn = 0.f, zp = 0.f, zn = 0.f;               // sums of alpha * da and of alpha over the z > 0 / z <= 0 edges
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.col[e] : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float dot[U], ss[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[u] = nid[u] >= 0 && (int64_t)nid[u] < p.n_tbl;
        float x[4];
        load4(p.tbl + (int64_t)(ok[u] ? nid[u] : 0) * p.ldt + hoff, k0, p.C, vec, ok[u], x);
        ss[u] = ok[u] ? p.s_src[(int64_t)nid[u] * p.H + h] : 0.f;
        dot[u] = gi[0] * x[0] + gi[1] * x[1] + gi[2] * x[2] + gi[3] * x[3];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.col[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) dot[u] = bgnn::group_sum<LF>(dot[u]);   // the sub-group's LF lanes: one edge, one head
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float d = dot[u];
        if (!ok[u]) continue;
        const int32_t e = e0 + u * EP;
        const float z = ss[u] + sd;
        const float x = leaky(z, p.slope);
        const float alpha = expf(x - mx) / den;
        const uint64_t el = (EDGE_ID ? (uint64_t)((int64_t)e + eshift) : (uint64_t)e) * (uint64_t)p.H + (uint64_t)h;
        const float mk = p.thr == 0u ? 1.f : (drop_bits(el, seed) >= p.thr ? p.keep_scale : 0.f);
        const float de = alpha * (mk * d - rr);
        const float dzv = de * (z > 0.f ? 1.f : p.slope);
        if (k0 == 0 && (int64_t)e < p.n_edges) p.dz[(int64_t)e * p.H + h] = dzv;
        if (z > 0.f) { sp += alpha * (mk * d); zp += alpha; }
        else { sn += alpha * (mk * d); zn += alpha; }
      }
    }
#pragma unroll
    for (int off = LF; off < GL; off <<= 1) {
      sp += __shfl_xor(sp, off); sn += __shfl_xor(sn, off);
      zp += __shfl_xor(zp, off); zn += __shfl_xor(zn, off);
    }
    // ds_dst = sum_t dz_t.  The row's de sum to zero (softmax), so only the edges' different LeakyReLU slopes leave anything:
    // sum_t de_t f_t = (1 - slope) (S+ Z- - S- Z+) / Z with r taken as S / Z, the row's OWN sum -- exactly 0 for a row whose edges
    // all lie on one side, where summing the stored dz (r from the kept conv output, an fp32 rounding away from S) leaves noise
    // of the size of r itself.
    if (valid && lg == 0) {
      const double Z = (double)zp + (double)zn;
      p.ds_dst[v] = Z > 0.0 ? (float)((1.0 - (double)p.slope) * ((double)sp * (double)zn - (double)sn * (double)zp) / Z) : 0.f;
    }
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------
template <int LF, int EP, int U, int EPI, bool BWD, bool ROW_ID>
int launch_agg(const AggParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows * p.H + RPB - 1) / RPB;
  const int grid = persistent_grid(gat_agg_kernel<LF, EP, U, EPI, BWD, ROW_ID>, ntiles, &cap);
  hipLaunchKernelGGL((gat_agg_kernel<LF, EP, U, EPI, BWD, ROW_ID>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int EPI, bool BWD, bool ROW_ID = false>
int dispatch_agg(const AggParams& p, hipStream_t st) {
  return lf_ladder((p.C + 3) / 4,   // float4 slots of a head
                   [&](auto LF, auto EP, auto U) { return launch_agg<LF, EP, U, EPI, BWD, ROW_ID>(p, st); });
}

template <bool EDGE_ID>
int launch_alpha(const AlphaParams& a, hipStream_t st) {
  static int cap = 0;
  const int64_t ntiles = (a.n_rows * a.H + 31) / 32;
  const int grid = persistent_grid(gat_alpha_kernel<8, 4, EDGE_ID>, ntiles, &cap);
  hipLaunchKernelGGL((gat_alpha_kernel<8, 4, EDGE_ID>), dim3((unsigned)grid), dim3(256), 0, st, a);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int LF, int EP, int U, bool EDGE_ID>
int launch_edge(const EdgeParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows * p.H + RPB - 1) / RPB;
  const int grid = persistent_grid(gat_bwd_edge_kernel<LF, EP, U, EDGE_ID>, ntiles, &cap);
  hipLaunchKernelGGL((gat_bwd_edge_kernel<LF, EP, U, EDGE_ID>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <bool EDGE_ID>
int dispatch_edge(const EdgeParams& p, hipStream_t st) {
  // four rows in flight on every rung: the ladder's U is not taken
  return lf_ladder((p.C + 3) / 4, [&](auto LF, auto EP, auto) { return launch_edge<LF, EP, 4, EDGE_ID>(p, st); });
}

}  // namespace

extern "C" int bgnn_gat_scores_f32(const float* tbl, int64_t ldt, int64_t n, int32_t H, int32_t C, const float* att_src,
                                   const float* att_dst, float* s_src, float* s_dst, void* stream) {
  if (!tbl || !att_src || !att_dst || !s_src || !s_dst) return BGNN_E_NULL;
  if (n < 0 || !shape_ok(H, C) || ldt < (int64_t)H * C) return BGNN_E_SHAPE;
  if (n == 0) return 0;
  int64_t grid = (n * H + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(gat_scores_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, tbl, ldt, n, (int)H, (int)C, att_src,
                     att_dst, s_src, s_dst);
  BGNN_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t bgnn_gat_aggregate_workspace_bytes(int64_t n_edges, int64_t n_rows, int32_t H) {
  if (n_edges < 0 || n_rows < 0 || H <= 0) return 0;
  return coef_bytes(n_edges, H) + bgnn_align_up((size_t)n_rows * (size_t)H * sizeof(float), 16) + 16;
}

// the ids matter only where a mask is drawn: without dropout the plain instantiations run
extern "C" int bgnn_gat_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* s_src, const float* s_dst,
                                      const float* bias_opt, const int32_t* rowptr, const int32_t* col, int64_t n_edges,
                                      int64_t n_rows, int32_t H, int32_t C, float negative_slope, float p_att, uint64_t seed_att,
                                      const uint64_t* seed_att_dev_opt, int epilogue, float p_drop, uint64_t seed,
                                      const uint64_t* seed_dev_opt, const int64_t* row_id_opt, const int64_t* edge_base_opt,
                                      float* state, float* alpha_out_opt, void* ws_opt, size_t ws_bytes, float* pre_out_opt,
                                      int64_t ldp, float* out, int64_t ldo, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tbl || !s_src || !s_dst || !rowptr || !col || !state || !out) return BGNN_E_NULL;
  if (!alpha_out_opt && !ws_opt) return BGNN_E_NULL;
  if (n_rows < 0 || n_tbl < 0 || n_edges < 0 || !shape_ok(H, C) || !(p_att >= 0.f && p_att < 1.f)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, C)) return rc;
  if (epilogue == EPI_LOGSOFTMAX && H != 1) return BGNN_E_SHAPE;
  const int32_t HC = H * C;
  if (!tbl_ok(tbl, ldt, HC) || !tbl_ok(out, ldo, HC) || (pre_out_opt && !tbl_ok(pre_out_opt, ldp, HC))) return BGNN_E_ALIGN;
  if (bias_opt && !bgnn_aligned16(bias_opt)) return BGNN_E_ALIGN;
  float* coef = alpha_out_opt;
  if (!coef) {
    if (ws_bytes < coef_bytes(n_edges, H) + 16) return BGNN_E_WORKSPACE;
    coef = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws_opt), 16));
  }
  if (n_rows == 0) return 0;
  {
    AlphaParams a{};
    a.s_src = s_src; a.n_src = n_tbl; a.s_dst = s_dst; a.rowptr = rowptr; a.col = col; a.n_rows = n_rows; a.n_edges = n_edges; a.H = H;
    a.slope = negative_slope;
    att_drop_consts(p_att, a.thr, a.keep_scale);
    a.seed = seed_att; a.seed_dev = seed_att_dev_opt;
    a.state = state; a.coef = coef; a.edge_base = edge_base_opt;
    const int rc = (edge_base_opt != nullptr && a.thr != 0u) ? launch_alpha<true>(a, st) : launch_alpha<false>(a, st);
    if (rc != 0) return rc;
  }
  AggParams p{};
  p.tbl = tbl; p.ldt = ldt; p.n_tbl = n_tbl; p.bias = bias_opt; p.rowptr = rowptr; p.col = col; p.eid = nullptr; p.n_edges = n_edges;
  p.coef = coef; p.n_rows = n_rows; p.H = H; p.C = C; p.npad = (HC + 3) / 4 * 4 - HC;
  p.out = out; p.ldo = ldo; p.pre = pre_out_opt; p.ldp = ldp;
  drop_consts(p_drop, p.thr, p.keep_scale);
  p.seed = seed; p.seed_dev = seed_dev_opt; p.row_id = row_id_opt;
  if (epilogue == EPI_ELU && row_id_opt != nullptr && p.thr != 0u) return dispatch_agg<EPI_ELU, false, true>(p, st);
  return epi_switch(epilogue, [&](auto EPI) { return dispatch_agg<EPI, false>(p, st); });
}

extern "C" int bgnn_gat_aggregate_bwd_f32(const float* tbl, int64_t ldt, int64_t n_src, const float* s_src, const float* s_dst,
                                          const float* bias_opt, const float* state, const float* alpha, const float* pre, int64_t ldp,
                                          const float* grad_y, int64_t ldgy, const int32_t* rowptr, const int32_t* col,
                                          const int32_t* t_rowptr, const int32_t* t_eid, const int32_t* t_dst, int64_t n_edges,
                                          int64_t n_rows, int32_t H, int32_t C, float negative_slope, float p_att, uint64_t seed_att,
                                          const uint64_t* seed_att_dev_opt, int epilogue, float p_drop, uint64_t seed,
                                          const uint64_t* seed_dev_opt, void* ws, size_t ws_bytes, const int64_t* row_id_opt,
                                          const int64_t* edge_base_opt, float* g, int64_t ldg, float* grad_tbl, int64_t ldgt,
                                          float* ds_src, float* ds_dst, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tbl || !s_src || !s_dst || !state || !alpha || !pre || !grad_y || !rowptr || !col || !t_rowptr || !t_eid || !t_dst || !ws ||
      !g || !grad_tbl || !ds_src || !ds_dst)
    return BGNN_E_NULL;
  if (n_rows < 0 || n_src < 0 || n_edges < 0 || !shape_ok(H, C) || !(p_att >= 0.f && p_att < 1.f)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, C)) return rc;
  if (epilogue == EPI_LOGSOFTMAX && H != 1) return BGNN_E_SHAPE;
  const int32_t HC = H * C;
  if (!tbl_ok(tbl, ldt, HC) || !tbl_ok(pre, ldp, HC) || !tbl_ok(grad_y, ldgy, HC) || !tbl_ok(g, ldg, HC) || !tbl_ok(grad_tbl, ldgt, HC))
    return BGNN_E_ALIGN;
  if (bias_opt && !bgnn_aligned16(bias_opt)) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_gat_aggregate_workspace_bytes(n_edges, n_rows, H)) return BGNN_E_WORKSPACE;
  float* dz = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws), 16));
  float* r = dz + coef_bytes(n_edges, H) / sizeof(float);
  const int32_t npad = (HC + 3) / 4 * 4 - HC;
  if (n_rows > 0) {
    RowParams p{};
    p.pre = pre; p.ldp = ldp; p.gy = grad_y; p.ldgy = ldgy; p.bias = bias_opt; p.n_rows = n_rows; p.H = H; p.C = C; p.npad = npad;
    drop_consts(p_drop, p.thr, p.keep_scale);
    p.seed = seed; p.seed_dev = seed_dev_opt;
    p.g = g; p.ldg = ldg; p.r = r; p.row_id = row_id_opt;
    int rc = dispatch_rows(epilogue, p, st);
    if (rc != 0) return rc;
    EdgeParams e{};
    e.tbl = tbl; e.ldt = ldt; e.n_tbl = n_src; e.g = g; e.ldg = ldg; e.s_src = s_src; e.s_dst = s_dst; e.state = state; e.r = r;
    e.rowptr = rowptr; e.col = col; e.n_rows = n_rows; e.n_edges = n_edges; e.H = H; e.C = C; e.slope = negative_slope;
    att_drop_consts(p_att, e.thr, e.keep_scale);
    e.seed = seed_att; e.seed_dev = seed_att_dev_opt;
    e.dz = dz; e.ds_dst = ds_dst; e.edge_base = edge_base_opt;
    rc = (edge_base_opt != nullptr && e.thr != 0u) ? dispatch_edge<true>(e, st) : dispatch_edge<false>(e, st);
    if (rc != 0) return rc;
  }
  if (n_src == 0) return 0;
  // the forward walk over the by-source view: its n_src rows gather rows of g (n_rows of them: every id in t_dst is a row < n_rows)
  // with the forward's coefficients; a source without out-edges here (no halo slot is one) leaves as a zero row
  AggParams p{};
  p.tbl = g; p.ldt = ldg; p.n_tbl = n_rows; p.bias = nullptr; p.rowptr = t_rowptr; p.col = t_dst; p.eid = t_eid; p.n_edges = n_edges;
  p.coef = alpha; p.dz = dz; p.dsum = ds_src; p.n_rows = n_src; p.H = H; p.C = C; p.npad = npad;
  p.out = grad_tbl; p.ldo = ldgt; p.pre = nullptr;
  return dispatch_agg<EPI_NONE, true>(p, st);
}
