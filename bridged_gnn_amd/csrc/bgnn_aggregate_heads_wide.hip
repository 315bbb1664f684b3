// Three-head classifier walk for wide classes (4 < D <= 32), forward and backward, for gfx950 (wave64).
//
// KT-GNN's classifier stage (reference models/KTGNN.py:432-435: clf_base(x), clf_target(x), clf_target(T(x)), then a
// log_softmax per head) shares ONE graph between its HEADS convs.  The narrow kernels (agg_heads_lanes_kernel and the
// heads backward, bgnn_aggregate.hip / bgnn_aggregate_bwd.hip) cover D <= 4, one float4 per head; this file widens that
// walk to ldh = pad4(D) <= 32 (office: 31 classes).  Tables / out / grad / dH are [N][HEADS][ldh] (interleaved per node,
// the layout of the eval path), the attention vectors [HEADS][D].
//
// Mapping: a group of GL = HEADS * LF lanes owns one destination (forward, pass A) or one source (pass B): LF lanes per
// head, one float4 of columns each (LF * 4 >= ldh).  The lanes of an edge read the neighbour's HEADS * ldh floats (one
// contiguous 96..384-byte row); the id is a broadcast load shared by all heads.  The GATv2 logit and the dot products are
// reduced over the LF lanes of a head with xor shuffles (the lanes of a head are LF-aligned inside the wave).
//
// Nothing per EDGE is written: the forward leaves each finished row's softmax state (m, s) per head, and the backward
// rebuilds alpha from it.  The backward is the pull form: pass A walks destinations (log_softmax adjoint, dH_i side terms,
// da), pass B walks sources through the by-source view and writes every dH row once.  da is summed per block in a fixed
// order and then over blocks in a fixed order: two identical backwards are bitwise equal.
//
// Hub rows (many in- or out-edges) are walked by their one lane group, which is exact; they are not cut into segments.
#include "bgnn_common.h"

namespace {

struct WideHeadsParams {
  const float* h_t2s; const float* h_s2t; int64_t ldh;
  const float* a_t2s; const float* a_s2t;
  const int32_t* rowptr; const int32_t* col; const uint8_t* mask;
  int64_t N; int32_t D; float slope;
  float* out; float* state_ms;                        // forward outputs
  // backward
  const float* fout; const float* fms; const float* gout;
  const int32_t* t_rowptr; const int32_t* t_dst;
  float* gr;             // [N][HEADS][ldh]  log_softmax adjoint of the incoming gradient
  float4* rec;           // [N][HEADS]       (m, 1/(s + 1e-16), t_i = gr_i . o_i, domain of i)
  float* dstside;        // [N][HEADS][ldh]  dH_i terms of pass A (the logit's h_i side)
  float* dh_t2s; float* dh_s2t;
  float* da_part;        // [grid][2][HEADS][LF * 4] per-block da of pass A
  float* da_t2s; float* da_s2t;
};

__device__ __forceinline__ float4 load4(const float* p, bool ok) {
  return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// columns >= D of a lane's float4 -> 0 (the pad columns of a table are never read as data)
__device__ __forceinline__ float4 cols(float4 v, int f0, int D) {
  if (f0 + 0 >= D) v.x = 0.f;
  if (f0 + 1 >= D) v.y = 0.f;
  if (f0 + 2 >= D) v.z = 0.f;
  if (f0 + 3 >= D) v.w = 0.f;
  return v;
}
template <int LF>
__device__ __forceinline__ float head_sum(float x) {
#pragma unroll
  for (int off = 1; off < LF; off <<= 1) x += __shfl_xor(x, off);
  return x;
}
template <int LF>
__device__ __forceinline__ float head_max(float x) {
#pragma unroll
  for (int off = 1; off < LF; off <<= 1) x = fmaxf(x, __shfl_xor(x, off));
  return x;
}
__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }
// this lane's share of the GATv2 logit a . leaky(hj + hi) (the narrow kernels' operation order)
__device__ __forceinline__ float logit_part(const float4& hj, const float4& hi, const float4& a4, float slope) {
  float t = a4.x * leaky(hj.x + hi.x, slope);
  t = fmaf(a4.y, leaky(hj.y + hi.y, slope), t);
  t = fmaf(a4.z, leaky(hj.z + hi.z, slope), t);
  t = fmaf(a4.w, leaky(hj.w + hi.w, slope), t);
  return t;
}
__device__ __forceinline__ float4 attn4(const float* av, int h, int D, int f0) {
  float4 a;
  a.x = f0 + 0 < D ? av[h * D + f0 + 0] : 0.f;
  a.y = f0 + 1 < D ? av[h * D + f0 + 1] : 0.f;
  a.z = f0 + 2 < D ? av[h * D + f0 + 2] : 0.f;
  a.w = f0 + 3 < D ? av[h * D + f0 + 3] : 0.f;
  return a;
}

// ---- forward: one launch, log_softmax epilogue, (m, s) per (row, head) ------------------------------------------------------
template <int HEADS, int LF, int U>
__global__ __launch_bounds__(256) void agg_heads_wide_kernel(WideHeadsParams p) {
  constexpr int GL = HEADS * LF, GPW = 64 / GL, RPB = 4 * GPW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / GL, lg = lane % GL, h = lg / LF, f0 = (lg % LF) * 4;
  const bool lane_on = g < GPW;
  const bool fvalid = f0 < p.ldh;
  const int64_t rs = (int64_t)HEADS * p.ldh;
  const int64_t ntiles = (p.N + RPB - 1) / RPB;
  bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t tile = bgnn::xcd_tile_of(pos, ntiles);
    if (tile < 0) continue;
    const int64_t i = tile * RPB + wave * GPW + g;
    const bool rvalid = lane_on && i < p.N;               // uniform over a group
    const int64_t ic = rvalid ? i : 0;
    const bool dom_s = p.mask[ic] != 0;
    const float* __restrict__ H = dom_s ? p.h_t2s : p.h_s2t;
    const float4 a4 = attn4(dom_s ? p.a_t2s : p.a_s2t, h, p.D, f0);
    const float4 hi = cols(load4(H + ic * rs + h * p.ldh + f0, fvalid), f0, p.D);
    const int32_t beg = rvalid ? p.rowptr[ic] : 0, end = rvalid ? p.rowptr[ic + 1] : 0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float m = -INFINITY, s = 0.f;
    for (int32_t e0 = beg; e0 < end; e0 += U) {
      int32_t id[U];
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) id[u] = e0 + u < end ? p.col[e0 + u] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = cols(load4(H + (int64_t)max(id[u], 0) * rs + h * p.ldh + f0, fvalid && id[u] >= 0), f0, p.D);
      float lg_[U], cm = -INFINITY;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float t = head_sum<LF>(logit_part(v[u], hi, a4, p.slope));
        lg_[u] = id[u] >= 0 ? t : -INFINITY;
        cm = fmaxf(cm, lg_[u]);
      }
      const float mn = fmaxf(m, cm);
      const float sc = (m == mn) ? 1.f : __expf(m - mn);
      s *= sc;
      acc.x *= sc; acc.y *= sc; acc.z *= sc; acc.w *= sc;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float pe = (lg_[u] == -INFINITY) ? 0.f : __expf(lg_[u] - mn);
        s += pe;
        acc.x = fmaf(pe, v[u].x, acc.x); acc.y = fmaf(pe, v[u].y, acc.y);
        acc.z = fmaf(pe, v[u].z, acc.z); acc.w = fmaf(pe, v[u].w, acc.w);
      }
      m = mn;
    }
    if (rvalid) {
      const float inv = 1.f / (s + 1e-16f);
      float4 r = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
      // log_softmax over the head's D classes (KTGNN.py:435), reduced over the head's LF lanes
      float mx = -INFINITY;
      if (f0 + 0 < p.D) mx = fmaxf(mx, r.x);
      if (f0 + 1 < p.D) mx = fmaxf(mx, r.y);
      if (f0 + 2 < p.D) mx = fmaxf(mx, r.z);
      if (f0 + 3 < p.D) mx = fmaxf(mx, r.w);
      mx = head_max<LF>(mx);
      float se = 0.f;
      if (f0 + 0 < p.D) se += expf(r.x - mx);
      if (f0 + 1 < p.D) se += expf(r.y - mx);
      if (f0 + 2 < p.D) se += expf(r.z - mx);
      if (f0 + 3 < p.D) se += expf(r.w - mx);
      const float lse = logf(head_sum<LF>(se));
      r.x = f0 + 0 < p.D ? r.x - mx - lse : 0.f;
      r.y = f0 + 1 < p.D ? r.y - mx - lse : 0.f;
      r.z = f0 + 2 < p.D ? r.z - mx - lse : 0.f;
      r.w = f0 + 3 < p.D ? r.w - mx - lse : 0.f;
      if (fvalid) *reinterpret_cast<float4*>(p.out + i * rs + h * p.ldh + f0) = r;
      if (f0 == 0) {
        p.state_ms[2 * (i * HEADS + h)] = m;
        p.state_ms[2 * (i * HEADS + h) + 1] = s;
      }
    }
  }
}

// ---- backward pass A: destinations ---------------------------------------------------------------------------------------------
// Per (i, head): gr_i = g_i - exp(logp_i) sum(g_i) (log_softmax adjoint), t_i = gr_i . o_i (from logp_i: see below).
// Per edge j -> i: alpha = exp(logit - m) / (s + 1e-16), de = alpha (gr_i . h_j - t_i);
//   dstside_i += de a (.) leaky'(z),  da[dom i] += de leaky(z).
template <int HEADS, int LF, int U>
__global__ __launch_bounds__(256) void agg_heads_wide_bwd_dst_kernel(WideHeadsParams p) {
  constexpr int GL = HEADS * LF, GPW = 64 / GL, RPB = 4 * GPW, W = HEADS * LF * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / GL, lg = lane % GL, h = lg / LF, f0 = (lg % LF) * 4;
  const bool lane_on = g < GPW;
  const bool fvalid = f0 < p.ldh;
  const int64_t rs = (int64_t)HEADS * p.ldh;
  float4 accS = make_float4(0.f, 0.f, 0.f, 0.f), accT = accS;
  const int64_t ntiles = (p.N + RPB - 1) / RPB;
  bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t tile = bgnn::xcd_tile_of(pos, ntiles);
    if (tile < 0) continue;
    const int64_t i = tile * RPB + wave * GPW + g;
    const bool rvalid = lane_on && i < p.N;
    if (!rvalid) continue;                                 // uniform over a group: the shuffles below stay inside live groups
    const bool dom_s = p.mask[i] != 0;
    const float* __restrict__ H = dom_s ? p.h_t2s : p.h_s2t;
    const float4 a4 = attn4(dom_s ? p.a_t2s : p.a_s2t, h, p.D, f0);
    const int64_t o = i * rs + h * p.ldh + f0;
    const float4 hi = cols(load4(H + o, fvalid), f0, p.D);
    float4 gi = cols(load4(p.gout + o, fvalid), f0, p.D);
    const float4 oi = cols(load4(p.fout + o, fvalid), f0, p.D);
    const float sg = head_sum<LF>(gi.x + gi.y + gi.z + gi.w);
    if (f0 + 0 < p.D) gi.x -= expf(oi.x) * sg;
    if (f0 + 1 < p.D) gi.y -= expf(oi.y) * sg;
    if (f0 + 2 < p.D) gi.z -= expf(oi.z) * sg;
    if (f0 + 3 < p.D) gi.w -= expf(oi.w) * sg;
    // t_i = gr_i . o_i = gr_i . (logp_i - k) for any k (sum(gr_i) = 0); k = mean(logp_i) keeps the fp32 rounding of sum(gr_i) from
    // being amplified by |logp| ~ log D
    const float k = head_sum<LF>(oi.x + oi.y + oi.z + oi.w) / (float)p.D;
    float ti = 0.f;
    if (f0 + 0 < p.D) ti = fmaf(gi.x, oi.x - k, ti);
    if (f0 + 1 < p.D) ti = fmaf(gi.y, oi.y - k, ti);
    if (f0 + 2 < p.D) ti = fmaf(gi.z, oi.z - k, ti);
    if (f0 + 3 < p.D) ti = fmaf(gi.w, oi.w - k, ti);
    ti = head_sum<LF>(ti);
    const float mh = p.fms[2 * (i * HEADS + h)];
    const float inv = 1.f / (p.fms[2 * (i * HEADS + h) + 1] + 1e-16f);
    if (fvalid) *reinterpret_cast<float4*>(p.gr + o) = gi;
    if (f0 == 0) p.rec[i * HEADS + h] = make_float4(mh, inv, ti, dom_s ? 1.f : 0.f);
    const int32_t beg = p.rowptr[i], end = p.rowptr[i + 1];
    float4 accd = make_float4(0.f, 0.f, 0.f, 0.f), accz = accd;
    for (int32_t e0 = beg; e0 < end; e0 += U) {
      int32_t jj[U];
      float4 hj[U];
#pragma unroll
      for (int u = 0; u < U; ++u) jj[u] = e0 + u < end ? p.col[e0 + u] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) hj[u] = cols(load4(H + (int64_t)max(jj[u], 0) * rs + h * p.ldh + f0, fvalid && jj[u] >= 0), f0, p.D);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float zx = hj[u].x + hi.x, zy = hj[u].y + hi.y, zz = hj[u].z + hi.z, zw = hj[u].w + hi.w;
        const float4 lk = make_float4(zx > 0.f ? 1.f : p.slope, zy > 0.f ? 1.f : p.slope, zz > 0.f ? 1.f : p.slope, zw > 0.f ? 1.f : p.slope);
        const float4 lz = make_float4(zx * lk.x, zy * lk.y, zz * lk.z, zw * lk.w);
        const float t = head_sum<LF>(logit_part(hj[u], hi, a4, p.slope));
        const float gh = head_sum<LF>(gi.x * hj[u].x + gi.y * hj[u].y + gi.z * hj[u].z + gi.w * hj[u].w);
        if (jj[u] < 0) continue;
        const float al = __expf(t - mh) * inv;
        const float de = al * (gh - ti);
        accd.x += de * a4.x * lk.x; accd.y += de * a4.y * lk.y; accd.z += de * a4.z * lk.z; accd.w += de * a4.w * lk.w;
        accz.x += de * lz.x; accz.y += de * lz.y; accz.z += de * lz.z; accz.w += de * lz.w;
      }
    }
    if (fvalid) *reinterpret_cast<float4*>(p.dstside + o) = accd;
    if (dom_s) { accS.x += accz.x; accS.y += accz.y; accS.z += accz.z; accS.w += accz.w; }
    else       { accT.x += accz.x; accT.y += accz.y; accT.z += accz.z; accT.w += accz.w; }
  }
  // da: the block's groups in a fixed order (LDS slots, one sequential sum per column), no atomics
  __shared__ float red[4 * GPW][2][W];
  if (lane_on) {
    const int slot = wave * GPW + g, c = lg * 4;
    red[slot][0][c] = accS.x; red[slot][0][c + 1] = accS.y; red[slot][0][c + 2] = accS.z; red[slot][0][c + 3] = accS.w;
    red[slot][1][c] = accT.x; red[slot][1][c + 1] = accT.y; red[slot][1][c + 2] = accT.z; red[slot][1][c + 3] = accT.w;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * W; t += 256) {
    float a = 0.f;
    for (int sl = 0; sl < 4 * GPW; ++sl) a += red[sl][t / W][t % W];
    p.da_part[(int64_t)blockIdx.x * 2 * W + t] = a;
  }
}

// da = sum over the blocks of pass A.  One block per (domain, head, column): each thread adds a fixed strided slice of the
// partial rows in order, then a fixed LDS tree -- the same order on every call (the partial count depends only on N).
template <int HEADS, int LF>
__global__ __launch_bounds__(256) void heads_wide_da_kernel(WideHeadsParams p, int nblocks) {
  constexpr int W = HEADS * LF * 4;
  const int t = blockIdx.x;                          // column of da_part, < 2 W
  const int d = t / W, h = (t % W) / (LF * 4), c = t % (LF * 4);
  if (c >= p.D) return;                              // uniform over the block
  float a = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += 256) a += p.da_part[(int64_t)b * 2 * W + t];
  __shared__ float red[256];
  red[threadIdx.x] = a;
  __syncthreads();
#pragma unroll
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) (d == 0 ? p.da_t2s : p.da_s2t)[h * p.D + c] = red[0];
}

// ---- backward pass B: sources --------------------------------------------------------------------------------------------------
// Per edge j -> i (by-source view), the table of i's domain: dH_j += alpha gr_i + de a (.) leaky'(z); then dstside_j is added to
// the table of j's own domain and both dH rows of j are written (pad columns 0).
template <int HEADS, int LF, int U>
__global__ __launch_bounds__(256) void agg_heads_wide_bwd_src_kernel(WideHeadsParams p) {
  constexpr int GL = HEADS * LF, GPW = 64 / GL, RPB = 4 * GPW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / GL, lg = lane % GL, h = lg / LF, f0 = (lg % LF) * 4;
  const bool lane_on = g < GPW;
  const bool fvalid = f0 < p.ldh;
  const int64_t rs = (int64_t)HEADS * p.ldh;
  const float4 aS = attn4(p.a_t2s, h, p.D, f0), aT = attn4(p.a_s2t, h, p.D, f0);
  const int64_t ntiles = (p.N + RPB - 1) / RPB;
  bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t tile = bgnn::xcd_tile_of(pos, ntiles);
    if (tile < 0) continue;
    const int64_t j = tile * RPB + wave * GPW + g;
    if (!(lane_on && j < p.N)) continue;                  // uniform over a group
    const int64_t o = j * rs + h * p.ldh + f0;
    const float4 hS = cols(load4(p.h_t2s + o, fvalid), f0, p.D);
    const float4 hT = cols(load4(p.h_s2t + o, fvalid), f0, p.D);
    const int32_t beg = p.t_rowptr[j], end = p.t_rowptr[j + 1];
    float4 accS = make_float4(0.f, 0.f, 0.f, 0.f), accT = accS;
    for (int32_t k0 = beg; k0 < end; k0 += U) {
      int32_t ii[U];
      float4 rc[U], hi[U], gi[U];
#pragma unroll
      for (int u = 0; u < U; ++u) ii[u] = k0 + u < end ? p.t_dst[k0 + u] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t ic = max(ii[u], 0);
        rc[u] = p.rec[ic * HEADS + h];
        const int64_t oi = ic * rs + h * p.ldh + f0;
        gi[u] = load4(p.gr + oi, fvalid && ii[u] >= 0);
        hi[u] = cols(load4((rc[u].w != 0.f ? p.h_t2s : p.h_s2t) + oi, fvalid && ii[u] >= 0), f0, p.D);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ds = rc[u].w != 0.f;                     // (m, 1/s, t_i, domain of i)
        const float4 a4 = ds ? aS : aT, hj = ds ? hS : hT;
        const float zx = hj.x + hi[u].x, zy = hj.y + hi[u].y, zz = hj.z + hi[u].z, zw = hj.w + hi[u].w;
        const float4 lk = make_float4(zx > 0.f ? 1.f : p.slope, zy > 0.f ? 1.f : p.slope, zz > 0.f ? 1.f : p.slope, zw > 0.f ? 1.f : p.slope);
        const float t = head_sum<LF>(logit_part(hj, hi[u], a4, p.slope));
        const float gh = head_sum<LF>(gi[u].x * hj.x + gi[u].y * hj.y + gi[u].z * hj.z + gi[u].w * hj.w);
        if (ii[u] < 0) continue;
        const float al = __expf(t - rc[u].x) * rc[u].y;
        const float de = al * (gh - rc[u].z);
        float4 v;
        v.x = fmaf(al, gi[u].x, de * a4.x * lk.x); v.y = fmaf(al, gi[u].y, de * a4.y * lk.y);
        v.z = fmaf(al, gi[u].z, de * a4.z * lk.z); v.w = fmaf(al, gi[u].w, de * a4.w * lk.w);
        if (ds) { accS.x += v.x; accS.y += v.y; accS.z += v.z; accS.w += v.w; }
        else    { accT.x += v.x; accT.y += v.y; accT.z += v.z; accT.w += v.w; }
      }
    }
    if (fvalid) {
      const float4 ds4 = *reinterpret_cast<const float4*>(p.dstside + o);
      if (p.mask[j] != 0) { accS.x += ds4.x; accS.y += ds4.y; accS.z += ds4.z; accS.w += ds4.w; }
      else                { accT.x += ds4.x; accT.y += ds4.y; accT.z += ds4.z; accT.w += ds4.w; }
      *reinterpret_cast<float4*>(p.dh_t2s + o) = accS;
      *reinterpret_cast<float4*>(p.dh_s2t + o) = accT;
    }
  }
}

constexpr int WIDE_MAX_GRID = 2048;

template <int HEADS, int LF>
int64_t wide_grid(int64_t N) {
  constexpr int RPB = 4 * (64 / (HEADS * LF));
  const int64_t ntiles = (N + RPB - 1) / RPB;
  int64_t grid = ntiles < WIDE_MAX_GRID ? (ntiles + 7) / 8 * 8 : WIDE_MAX_GRID;
  return grid < 8 ? 8 : grid;
}

template <int HEADS, int LF>
int launch_wide_fwd(const WideHeadsParams& p, hipStream_t st) {
  hipLaunchKernelGGL((agg_heads_wide_kernel<HEADS, LF, 4>), dim3((unsigned)wide_grid<HEADS, LF>(p.N)), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int HEADS, int LF>
int launch_wide_bwd(const WideHeadsParams& p, hipStream_t st) {
  const int64_t grid = wide_grid<HEADS, LF>(p.N);     // pass A's grid is also the number of da partial rows
  hipLaunchKernelGGL((agg_heads_wide_bwd_dst_kernel<HEADS, LF, 4>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL((heads_wide_da_kernel<HEADS, LF>), dim3((unsigned)(2 * HEADS * LF * 4)), dim3(256), 0, st, p, (int)grid);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL((agg_heads_wide_bwd_src_kernel<HEADS, LF, 4>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int HEADS>
int dispatch_wide(const WideHeadsParams& p, hipStream_t st, bool bwd) {
  if (p.ldh <= 8) return bwd ? launch_wide_bwd<HEADS, 2>(p, st) : launch_wide_fwd<HEADS, 2>(p, st);
  if (p.ldh <= 16) return bwd ? launch_wide_bwd<HEADS, 4>(p, st) : launch_wide_fwd<HEADS, 4>(p, st);
  return bwd ? launch_wide_bwd<HEADS, 8>(p, st) : launch_wide_fwd<HEADS, 8>(p, st);
}

bool wide_envelope(int32_t D, int32_t heads, int64_t ldh) {
  return D > 4 && D <= 32 && (heads == 2 || heads == 3) && ldh == (int64_t)((D + 3) / 4 * 4);
}

}  // namespace

extern "C" int bgnn_adaptedconv_aggregate_heads_wide_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                                         const float* a_t2s, const float* a_s2t,
                                                         const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                                         int64_t N, int32_t D, int32_t heads, float negative_slope,
                                                         float* out, float* state_ms, void* stream) {
  if (!wide_envelope(D, heads, ldh) || N < 0) return BGNN_E_SHAPE;
  if (!h_t2s || !h_s2t || !a_t2s || !a_s2t || !rowptr || !col || !mask || !out || !state_ms) return BGNN_E_NULL;
  if (!bgnn_aligned16(h_t2s) || !bgnn_aligned16(h_s2t) || !bgnn_aligned16(out)) return BGNN_E_ALIGN;
  if (N == 0) return 0;
  WideHeadsParams p{};
  p.h_t2s = h_t2s; p.h_s2t = h_s2t; p.ldh = ldh; p.a_t2s = a_t2s; p.a_s2t = a_s2t;
  p.rowptr = rowptr; p.col = col; p.mask = mask; p.N = N; p.D = D; p.slope = negative_slope;
  p.out = out; p.state_ms = state_ms;
  hipStream_t st = (hipStream_t)stream;
  return heads == 3 ? dispatch_wide<3>(p, st, false) : dispatch_wide<2>(p, st, false);
}

extern "C" size_t bgnn_aggregate_heads_wide_bwd_workspace_bytes(int64_t N, int32_t heads, int64_t ldh) {
  const size_t n = (size_t)(N > 0 ? N : 0), h = (size_t)(heads > 0 ? heads : 0), l = (size_t)(ldh > 0 ? ldh : 0);
  return 2 * bgnn_align_up(sizeof(float) * n * h * l, 256) + bgnn_align_up(sizeof(float4) * n * h, 256) +
         bgnn_align_up(sizeof(float) * (size_t)WIDE_MAX_GRID * 2 * h * 32, 256) + 256;
}

extern "C" int bgnn_adaptedconv_aggregate_heads_wide_bwd_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                                             const float* a_t2s, const float* a_s2t,
                                                             const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                                             const int32_t* t_rowptr, const int32_t* t_dst,
                                                             int64_t N, int32_t D, int32_t heads, float negative_slope,
                                                             const float* out, const float* state_ms, const float* grad_out,
                                                             float* dh_t2s, float* dh_s2t, float* da_t2s, float* da_s2t,
                                                             void* ws, size_t ws_bytes, void* stream) {
  if (!wide_envelope(D, heads, ldh) || N < 0) return BGNN_E_SHAPE;
  if (!h_t2s || !h_s2t || !a_t2s || !a_s2t || !rowptr || !col || !mask || !t_rowptr || !t_dst || !out || !state_ms ||
      !grad_out || !dh_t2s || !dh_s2t || !da_t2s || !da_s2t || !ws)
    return BGNN_E_NULL;
  if (!bgnn_aligned16(h_t2s) || !bgnn_aligned16(h_s2t) || !bgnn_aligned16(out) || !bgnn_aligned16(grad_out) ||
      !bgnn_aligned16(dh_t2s) || !bgnn_aligned16(dh_s2t) || !bgnn_aligned16(ws))
    return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_aggregate_heads_wide_bwd_workspace_bytes(N, heads, ldh)) return BGNN_E_WORKSPACE;
  if (N == 0) {                                      // no rows: da is still written (zeros), as the header promises
    hipStream_t st0 = (hipStream_t)stream;
    hipError_t e = bgnn_zero_async(da_t2s, sizeof(float) * (size_t)heads * D, st0);
    if (e == hipSuccess) e = bgnn_zero_async(da_s2t, sizeof(float) * (size_t)heads * D, st0);
    return (int)e;
  }
  const size_t tab = bgnn_align_up(sizeof(float) * (size_t)N * heads * ldh, 256);
  WideHeadsParams p{};
  p.h_t2s = h_t2s; p.h_s2t = h_s2t; p.ldh = ldh; p.a_t2s = a_t2s; p.a_s2t = a_s2t;
  p.rowptr = rowptr; p.col = col; p.mask = mask; p.N = N; p.D = D; p.slope = negative_slope;
  p.fout = out; p.fms = state_ms; p.gout = grad_out; p.t_rowptr = t_rowptr; p.t_dst = t_dst;
  p.gr = (float*)ws;
  p.dstside = (float*)((char*)ws + tab);
  p.rec = (float4*)((char*)ws + 2 * tab);
  p.da_part = (float*)((char*)ws + 2 * tab + bgnn_align_up(sizeof(float4) * (size_t)N * heads, 256));
  p.dh_t2s = dh_t2s; p.dh_s2t = dh_s2t; p.da_t2s = da_t2s; p.da_s2t = da_s2t;
  hipStream_t st = (hipStream_t)stream;
  return heads == 3 ? dispatch_wide<3>(p, st, true) : dispatch_wide<2>(p, st, true);
}
