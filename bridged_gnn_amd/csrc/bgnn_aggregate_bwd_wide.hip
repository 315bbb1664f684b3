// The atomic-free ("pull") aggregation backward for 128 < D <= 256 (gfx950, wave64).  Same two passes and the same mathematics
// as agg_bwd_dst_kernel / agg_bwd_src_kernel (bgnn_aggregate_bwd.hip; reference: autograd through
// Bridged-GNN/models/KTGNN.py:292-305), one lane group widened to the whole wave:
//   pass A (by destination i):  c_ji = g_i . h_j,  t_i = g_i . out_i,  de_ji = alpha_ji (c_ji - t_i),
//                               dstside[i] = a * sum_j de_ji leaky'(z_ji),  da += sum_ji de_ji leaky(z_ji),  z_ji = h_j + h_i,
//                               and one record per edge (below), written in CSR order;
//   pass B (by source j):       dH_X[j] = sum_{i in X} (alpha_ji g_i + de_ji a_X * leaky'(z_ji)) + dstside[j]   (X = S, T),
//                               rebuilt from the record and dL/dout_i alone (neither h_i nor the logits are read again).
// Mapping: a wave owns a row, lane l the columns 4l..4l+3 (one float4), four rows per 256-thread block, U = 4 neighbour rows
// per step; per-XCD dynamic tile queues over xcd_pos_range / xcd_tile_of like the narrower lane groups.
//
// Record: 64 bytes per edge, 64-byte aligned (two per 128-byte line, none straddles a line), 48 of them written and read:
//   [0] {alpha, de, domain(i), 0}   [1] {bx.lo, bx.hi, by.lo, by.hi}   [2] {bz.lo, bz.hi, bw.lo, bw.hi}   [3] unused
// where bx .. bw are the 64-bit ballots of z.x .. z.w > 0 over the wave (bit l = lane l = column 4l + component).  Lanes 0..2
// store one 16-byte piece each (one 48-byte store instruction per edge).
//
// Hub rows: PullParams' scheme unchanged (rows with >= hub_threshold edges are skipped as rows and walked as <= 64-edge
// segments behind the real rows; pull_merge_* add the partial rows in a fixed order).
//
// da without atomics: the queue hands out CHUNKS of TQ_CHUNK consecutive positions of an XCD's sequence, and a chunk covers the
// same rows whichever block draws it.  So pass A leaves one partial [2][ldh] row per CHUNK (not per block: which block walks
// which rows changes from run to run): each wave sums its rows of the chunk in walk order, the four waves are added in wave
// order through LDS, and pull_wide_da_kernel sums the chunk rows in a fixed order.  All four outputs of a call are bitwise
// reproducible.
//
// Pad columns (D <= c < ldh) of the tables must hold finite values (zeros everywhere in this project); g, out and a are masked.
#include "bgnn_common.h"
#include "bgnn_aggregate_bwd_params.h"

namespace {

using bgnn_bwd::PullParams;

constexpr int RPB = 4;            // rows per block (one per wave)
constexpr int TQ_CHUNK = 4;       // tiles per queue fetch (bgnn_aggregate_bwd.hip)
constexpr int DA_SLICES = 128;    // first-stage slices of the da sum
constexpr int DA_DIRECT = 256;    // up to this many partial rows: one launch

// chunks of one XCD's position sequence (xcd_pos_range: XCD_NSEG * seg_len positions per XCD)
__host__ __device__ inline int64_t chunks_per_xcd(int64_t ntiles) {
  const int64_t per = (ntiles + 7) / 8, seg_len = (per + bgnn::XCD_NSEG - 1) / bgnn::XCD_NSEG;
  return (bgnn::XCD_NSEG * seg_len + TQ_CHUNK - 1) / TQ_CHUNK;
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
// columns >= D of a lane's float4 -> 0
__device__ __forceinline__ float4 cols(float4 v, int f0, int D) {
  if (f0 + 0 >= D) v.x = 0.f;
  if (f0 + 1 >= D) v.y = 0.f;
  if (f0 + 2 >= D) v.z = 0.f;
  if (f0 + 3 >= D) v.w = 0.f;
  return v;
}
__device__ __forceinline__ float4 attn4(const float* av, int f0, int D) {
  float4 a;
  a.x = f0 + 0 < D ? av[f0 + 0] : 0.f;
  a.y = f0 + 1 < D ? av[f0 + 1] : 0.f;
  a.z = f0 + 2 < D ? av[f0 + 2] : 0.f;
  a.w = f0 + 3 < D ? av[f0 + 3] : 0.f;
  return a;
}

__global__ __launch_bounds__(256) void agg_bwd_dst_wide_kernel(PullParams p, float* __restrict__ da_part) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = lane * 4;
  const bool fvalid = f0 < p.D;
  const int f0c = fvalid ? f0 : 0;
  float4 accS = zero4(), accT = zero4();                     // da of this wave's rows of the current chunk, per domain
  const int64_t ntiles = (p.N + p.d_nv + RPB - 1) / RPB;     // real rows, then the hub rows' segments
  const int64_t cpx = chunks_per_xcd(ntiles);
  bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);   // positions of this XCD's segment sequence (XCD balance)
  __shared__ unsigned int dyn_tile;
  __shared__ __attribute__((aligned(16))) float red[4][2][256];
  const int64_t xbase = tr.begin - (blockIdx.x / 8);
  int64_t tile = 0, chunk_left = 0, chunk = -1;
  for (;;) {
    // per-XCD dynamic tile queue (same reason as in the forward: the blocks of an XCD stay on neighbouring rows)
    if (chunk_left == 0) {
      const bool had = chunk >= 0;                           // block-uniform
      if (had) {
        *reinterpret_cast<float4*>(&red[wave][0][f0]) = accS;
        *reinterpret_cast<float4*>(&red[wave][1][f0]) = accT;
      }
      __syncthreads();
      if (threadIdx.x == 0) dyn_tile = atomicAdd(&p.queue[blockIdx.x % 8], 1u);
      if (had) {                                             // the finished chunk's partial row: waves added in wave order
        float* __restrict__ row = da_part + ((int64_t)(blockIdx.x % 8) * cpx + chunk) * 2 * p.ldh;
        for (int t = threadIdx.x; t < 512; t += 256) {
          const int d = t >> 8, c = t & 255;
          if (c < p.ldh) row[d * p.ldh + c] = ((red[0][d][c] + red[1][d][c]) + red[2][d][c]) + red[3][d][c];
        }
      }
      __syncthreads();
      chunk = dyn_tile;
      tile = xbase + chunk * TQ_CHUNK;
      chunk_left = TQ_CHUNK;
      accS = zero4(); accT = zero4();
      if (tile >= tr.end) break;                             // no position of this chunk exists (chunk >= cpx)
    } else {
      tile += 1;
    }
    --chunk_left;
    if (tile >= tr.end) continue;                            // the last chunk's tail: its partial row is still written above
    const int64_t gt = bgnn::xcd_tile_of(tile, ntiles);     // `tile` is a position in the XCD's sequence
    if (gt < 0) continue;
    const int64_t i0 = gt * RPB + wave;
    const bool in_range = i0 < p.N + p.d_nv;
    const bool virt = in_range && i0 >= p.N;                   // a segment of a hub destination
    const int64_t vix = virt ? i0 - p.N : 0;
    const int64_t i = virt ? (int64_t)p.d_vnode[vix] : i0;
    const int64_t ic = in_range ? i : 0;
    const bool dom_s = p.mask[ic] != 0;
    const float* __restrict__ H = dom_s ? p.h_t2s : p.h_s2t;
    int32_t beg = in_range ? (virt ? p.d_vbounds[2 * vix] : p.rowptr[ic]) : 0;
    int32_t end = in_range ? (virt ? p.d_vbounds[2 * vix + 1] : p.rowptr[ic + 1]) : 0;
    const bool hub = !virt && p.hub_threshold > 0 && end - beg >= p.hub_threshold;
    const bool rvalid = in_range && !hub;
    if (hub) { beg = 0; end = 0; }
    float4 gi = zero4(), oi = zero4();
    const float4 a4 = attn4(dom_s ? p.a_t2s : p.a_s2t, f0, p.D);
    const float4 hi = *reinterpret_cast<const float4*>(H + ic * p.ldh + f0c);
    if (fvalid) {
      if (rvalid) gi = cols(*reinterpret_cast<const float4*>(p.gout + ic * p.ldg + f0), f0, p.D);
      oi = cols(*reinterpret_cast<const float4*>(p.out + ic * p.ldo + f0), f0, p.D);
    }
    const float ti = bgnn::group_sum<64>(gi.x * oi.x + gi.y * oi.y + gi.z * oi.z + gi.w * oi.w);
    float4 accd = zero4(), accz = zero4();
    const int32_t niter = (end - beg + U - 1) / U;
    int32_t nid[U];
    float nal[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + u;
      nid[u] = e < end ? p.col[e] : -1;
      nal[u] = e < end ? p.alpha[e] : 0.f;
    }
    for (int32_t it = 0; it < niter; ++it) {
      int32_t id[U];
      float al[U];
      float4 hj[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        id[u] = nid[u]; al[u] = nal[u];
        hj[u] = *reinterpret_cast<const float4*>(H + (int64_t)max(id[u], 0) * p.ldh + f0c);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {                 // ids / alphas of the next step fly with this step's rows
        const int32_t e = beg + (it + 1) * U + u;
        nid[u] = e < end ? p.col[e] : -1;
        nal[u] = e < end ? p.alpha[e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float cdot = bgnn::group_sum<64>(gi.x * hj[u].x + gi.y * hj[u].y + gi.z * hj[u].z + gi.w * hj[u].w);
        const float de = id[u] >= 0 ? al[u] * (cdot - ti) : 0.f;
        const float zx = hj[u].x + hi.x, zy = hj[u].y + hi.y, zz = hj[u].z + hi.z, zw = hj[u].w + hi.w;
        const bool px = zx > 0.f, py = zy > 0.f, pz = zz > 0.f, pw = zw > 0.f;
        accd.x += de * a4.x * (px ? 1.f : p.slope); accd.y += de * a4.y * (py ? 1.f : p.slope);
        accd.z += de * a4.z * (pz ? 1.f : p.slope); accd.w += de * a4.w * (pw ? 1.f : p.slope);
        accz.x += de * (px ? zx : zx * p.slope); accz.y += de * (py ? zy : zy * p.slope);
        accz.z += de * (pz ? zz : zz * p.slope); accz.w += de * (pw ? zw : zw * p.slope);
        const unsigned long long bx = __ballot(px), by = __ballot(py), bz = __ballot(pz), bw = __ballot(pw);
        if (lane < 3 && id[u] >= 0) {               // lanes 0..2: one 16-byte piece of the record each
          uint4 w;
          if (lane == 0) {
            w.x = __float_as_uint(al[u]); w.y = __float_as_uint(de); w.z = dom_s ? 1u : 0u; w.w = 0u;
          } else {
            const unsigned long long b0 = lane == 1 ? bx : bz, b1 = lane == 1 ? by : bw;
            w.x = (uint32_t)b0; w.y = (uint32_t)(b0 >> 32); w.z = (uint32_t)b1; w.w = (uint32_t)(b1 >> 32);
          }
          p.rec[(int64_t)(beg + it * U + u) * 4 + lane] = w;
        }
      }
    }
    if (rvalid && f0 < p.ldh)
      *reinterpret_cast<float4*>((virt ? p.d_vpart + vix * p.ldh : p.dstside + i * p.ldh) + f0) = fvalid ? accd : zero4();
    if (rvalid && fvalid) {
      if (dom_s) { accS.x += accz.x; accS.y += accz.y; accS.z += accz.z; accS.w += accz.w; }
      else       { accT.x += accz.x; accT.y += accz.y; accT.z += accz.z; accT.w += accz.w; }
    }
  }
}

// Sum of `rows` rows of W = 2 * ldh floats in a fixed order.  Block (x, y): columns 64x..64x+63 of slice y (rows [y * per,
// (y + 1) * per)); wave w adds the slice's rows w, w + 4, .. in order, the four waves are added in wave order.  da_t2s == nullptr:
// the slice sums go to out[y][W] (first stage); else (one slice) the columns below D go to da_t2s / da_s2t.
__global__ __launch_bounds__(256) void pull_wide_da_kernel(const float* __restrict__ in, int64_t rows, int64_t per, int W, float* __restrict__ out,
                                                           float* __restrict__ da_t2s, float* __restrict__ da_s2t, int ldh, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int64_t lo = (int64_t)blockIdx.y * per, hi = lo + per < rows ? lo + per : rows;
  float a = 0.f;
  if (c < W)
    for (int64_t b = lo + wave; b < hi; b += 4) a += in[b * W + c];
  __shared__ float red[4][64];
  red[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && c < W) {
    const float v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    if (!da_t2s) out[(int64_t)blockIdx.y * W + c] = v;
    else if (c < ldh) { if (c < D) da_t2s[c] = v; }
    else if (c - ldh < D) da_s2t[c - ldh] = v;
  }
}

__global__ __launch_bounds__(256) void agg_bwd_src_wide_kernel(PullParams p) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = lane * 4;
  const bool fvalid = f0 < p.D;
  const int f0c = fvalid ? f0 : 0;
  const bool up = lane >= 32;                                 // this lane's bit: word lane / 32 of a ballot, bit lane % 32
  const int sh = lane & 31;
  const float4 aS = attn4(p.a_t2s, f0, p.D), aT = attn4(p.a_s2t, f0, p.D);
  const int64_t ntiles = (p.N + p.s_nv + RPB - 1) / RPB;     // real rows, then the hub sources' segments
  bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);   // positions of this XCD's segment sequence (XCD balance)
  __shared__ unsigned int dyn_tile;
  const int64_t xbase = tr.begin - (blockIdx.x / 8);
  int64_t tile = 0, chunk_left = 0;
  for (;;) {
    if (chunk_left == 0) {
      __syncthreads();
      if (threadIdx.x == 0) dyn_tile = atomicAdd(&p.queue[8 + blockIdx.x % 8], 1u);
      __syncthreads();
      tile = xbase + (int64_t)dyn_tile * TQ_CHUNK;
      chunk_left = TQ_CHUNK;
    } else {
      tile += 1;
    }
    --chunk_left;
    if (tile >= tr.end) break;
    const int64_t gt = bgnn::xcd_tile_of(tile, ntiles);     // `tile` is a position in the XCD's sequence
    if (gt < 0) continue;
    const int64_t j0 = gt * RPB + wave;
    const bool in_range = j0 < p.N + p.s_nv;
    const bool virt = in_range && j0 >= p.N;                   // a segment of a hub source
    const int64_t vix = virt ? j0 - p.N : 0;
    const int64_t j = virt ? (int64_t)p.s_vnode[vix] : j0;
    const int64_t jc = in_range ? j : 0;
    int32_t beg = in_range ? (virt ? p.s_vbounds[2 * vix] : p.t_rowptr[jc]) : 0;
    int32_t end = in_range ? (virt ? p.s_vbounds[2 * vix + 1] : p.t_rowptr[jc + 1]) : 0;
    const bool hub = !virt && p.hub_threshold > 0 && end - beg >= p.hub_threshold;
    const bool rvalid = in_range && !hub;
    if (hub) { beg = 0; end = 0; }
    float4 accS = zero4(), accT = zero4();
    const int32_t niter = (end - beg + U - 1) / U;
    int32_t ne[U], ni[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t k = beg + u;
      ne[u] = k < end ? p.t_eid[k] : -1;
      ni[u] = k < end ? p.t_dst[k] : 0;
    }
    for (int32_t it = 0; it < niter; ++it) {
      uint4 hd[U], m0[U], m1[U];
      float4 g4[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = ne[u] >= 0;
        const uint4* r = p.rec + (int64_t)max(ne[u], 0) * 4;
        hd[u] = r[0]; m0[u] = r[1]; m1[u] = r[2];
        if (!ok) { hd[u].x = 0u; hd[u].y = 0u; }                 // alpha = de = 0: no contribution
        g4[u] = cols(*reinterpret_cast<const float4*>(p.gout + (int64_t)ni[u] * p.ldg + f0c), f0, p.D);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {                 // edge ids / destinations of the next step fly with this step's gathers
        const int32_t k = beg + (it + 1) * U + u;
        ne[u] = k < end ? p.t_eid[k] : -1;
        ni[u] = k < end ? p.t_dst[k] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float al = __uint_as_float(hd[u].x), de = __uint_as_float(hd[u].y);
        const bool ds = hd[u].z != 0u;
        const float4 a4 = ds ? aS : aT;
        const uint32_t sx = up ? m0[u].y : m0[u].x, sy = up ? m0[u].w : m0[u].z;
        const uint32_t sz = up ? m1[u].y : m1[u].x, sw = up ? m1[u].w : m1[u].z;
        float4 v;
        v.x = fmaf(al, g4[u].x, de * a4.x * (((sx >> sh) & 1u) ? 1.f : p.slope));
        v.y = fmaf(al, g4[u].y, de * a4.y * (((sy >> sh) & 1u) ? 1.f : p.slope));
        v.z = fmaf(al, g4[u].z, de * a4.z * (((sz >> sh) & 1u) ? 1.f : p.slope));
        v.w = fmaf(al, g4[u].w, de * a4.w * (((sw >> sh) & 1u) ? 1.f : p.slope));
        if (ds) { accS.x += v.x; accS.y += v.y; accS.z += v.z; accS.w += v.w; }
        else    { accT.x += v.x; accT.y += v.y; accT.z += v.z; accT.w += v.w; }
      }
    }
    if (virt && f0 < p.ldh) {                                   // a segment: its partial sums, merged afterwards
      if (!fvalid) { accS = zero4(); accT = zero4(); }
      *reinterpret_cast<float4*>(p.s_vpartS + vix * p.ldh + f0) = accS;
      *reinterpret_cast<float4*>(p.s_vpartT + vix * p.ldh + f0) = accT;
    } else if (rvalid && f0 < p.ldh) {
      const bool dom_j = p.mask[j] != 0;
      const float4 ds4 = *reinterpret_cast<const float4*>(p.dstside + j * p.ldh + f0);
      if (!fvalid) { accS = zero4(); accT = zero4(); }
      if (dom_j) { accS.x += ds4.x; accS.y += ds4.y; accS.z += ds4.z; accS.w += ds4.w; }
      else       { accT.x += ds4.x; accT.y += ds4.y; accT.z += ds4.z; accT.w += ds4.w; }
      *reinterpret_cast<float4*>(p.dh_t2s + j * p.ldh + f0) = accS;
      *reinterpret_cast<float4*>(p.dh_s2t + j * p.ldh + f0) = accT;
    }
  }
}

}  // namespace

namespace bgnn_bwd {

// workspace: records (64 bytes per edge) | dstside | queue | da chunk rows | da slice rows | hub segment rows
PullLayout pull_wide_plan(int64_t N, int64_t E, int64_t ldh, int64_t d_nv, int64_t s_nv) {
  const size_t n = (size_t)(N > 0 ? N : 0), e = (size_t)(E > 0 ? E : 0), l = (size_t)(ldh > 0 ? ldh : 0);
  const size_t dv = (size_t)(d_nv > 0 ? d_nv : 0), sv = (size_t)(s_nv > 0 ? s_nv : 0);
  PullLayout w;
  w.nparts = 8 * chunks_per_xcd((int64_t)((n + dv + RPB - 1) / RPB));
  w.rec = 0;
  w.dstside = w.rec + bgnn_align_up((size_t)64 * e, 256);
  w.queue = w.dstside + bgnn_align_up(sizeof(float) * n * l, 256);
  w.da_part = w.queue + 256;
  w.da_stage = w.da_part + bgnn_align_up(sizeof(float) * (size_t)w.nparts * 2 * l, 256);
  w.seg = w.da_stage + bgnn_align_up(sizeof(float) * (size_t)DA_SLICES * 2 * l, 256);
  w.total = w.seg + bgnn_align_up(sizeof(float) * l * (dv + 2 * sv), 256) + 256;
  return w;
}

int pull_wide_launch(const PullParams& p, const PullHubs& hubs, const PullLayout& w, void* ws, hipStream_t st) {
  float* da_part = (float*)((char*)ws + w.da_part);
  float* da_stage = (float*)((char*)ws + w.da_stage);
  static const int cap = resident_cap(agg_bwd_dst_wide_kernel, agg_bwd_src_wide_kernel);
  const int64_t nmax = p.N + (p.d_nv > p.s_nv ? p.d_nv : p.s_nv);
  const unsigned grid = resident_grid((nmax + RPB - 1) / RPB, cap);
  hipLaunchKernelGGL(agg_bwd_dst_wide_kernel, dim3(grid), dim3(256), 0, st, p, da_part);
  BGNN_LAUNCH_CHECK();
  // the hub destinations' dstside rows, before pass B reads them
  if (const int rc = pull_merge_dst_launch(hubs, p.ldh, p.d_vpart, p.mask, p.dstside, st)) return rc;
  // da: the chunk rows in a fixed order (two stages above DA_DIRECT rows)
  const int W = (int)(2 * p.ldh);
  const unsigned cb = (unsigned)((W + 63) / 64);
  const float* src = da_part;
  int64_t rows = w.nparts;
  if (rows > DA_DIRECT) {
    const int64_t per = (rows + DA_SLICES - 1) / DA_SLICES, slices = (rows + per - 1) / per;
    hipLaunchKernelGGL(pull_wide_da_kernel, dim3(cb, (unsigned)slices), dim3(256), 0, st, src, rows, per, W, da_stage,
                       (float*)nullptr, (float*)nullptr, (int)p.ldh, (int)p.D);
    BGNN_LAUNCH_CHECK();
    src = da_stage; rows = slices;
  }
  hipLaunchKernelGGL(pull_wide_da_kernel, dim3(cb, 1), dim3(256), 0, st, src, rows, rows, W, (float*)nullptr, p.da_t2s, p.da_s2t,
                     (int)p.ldh, (int)p.D);
  BGNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(agg_bwd_src_wide_kernel, dim3(grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return pull_merge_src_launch(hubs, p.ldh, p.s_vpartS, p.s_vpartT, p.mask, p.dstside, p.dh_t2s, p.dh_s2t, st);
}

}  // namespace bgnn_bwd
