// GATv2 attention conv for gfx950 (wave64): a one-pass fused forward and an atomic-free backward.
//
// Replaces (reference, Bridged-GNN/models/backbones.py:302-358): PyG GATv2Conv's (share_weights=False) per-destination softmax
// over e = <att, leaky_relu(x_l[j] + x_r[i])>, the attention dropout on the edge coefficients, propagate(aggr='add') of x_l[j] + bias,
// and the F.elu / F.dropout between the convs and the closing log_softmax.  The host transforms first: ONE table
// T = x [W_l ; W_r]^T + [b_l ; b_r] with XL at columns [0, H*C) and XR at columns [P, P + H*C), P = pad4(H*C), leading dimension
// >= 2P; this file walks the by-destination CSR with exactly one self loop per row (bgnn_build_dst_csr with rewrite_self_loops).
//
// Unlike GAT's logit (additive in two per-node scalars: bgnn_gat.hip runs its softmax over scalars and gathers afterwards), this
// logit needs the C-wide neighbour row of every edge, and that gather is also the one the weighted sum needs: the forward is ONE
// pass over the edges with an online softmax (running max, denominator, rescaled accumulator), as agg_kernel of bgnn_aggregate.hip.
//
// The mapping is bgnn_gat.hip's: a VIRTUAL ROW is one (row i, head h) pair, v = i*H + h, given to one lane group (LF lanes x float4
// over C, EP sub-groups on different edges, U neighbour rows in flight); blocks are persistent over the XCD-balanced segment
// order; head slices with C % 4 != 0 use scalar accesses.  m = x_l[j] + x_r[i] is one rounded fp32 add and the logit one fixed
// chain of fused multiply-adds and lane steps (logit_part + group_sum) in EVERY kernel that forms them, so the forward's softmax
// state fits the backward's logits bit for bit and a host can reproduce every LeakyReLU side from the table.  Only m and e are
// pinned that way: the dot products and the accumulators (acc, dxr, datt) are plain expressions whose fma contraction is the
// compiler's, fixed per kernel, so identical calls agree bit for bit but those sums are not promised to match across kernels.
//
// Forward, one launch:  per edge gather xl_j, e = sum_c att_c * leaky(xl_j + xr_i), online softmax; the denominator sums every
//   edge, the accumulator adds mask * keep_scale * p * xl_j (mask from the counter hash at element t*H + h: GAT's contract); the EP
//   sub-groups merge with the fixed butterfly; out = acc / den + bias, epilogue (none | ELU then dropout | log_softmax, H == 1).
//   state[i,h] = (max, denominator).  With alpha_out the logits are parked there in the pass and turned into the post-dropout
//   coefficients by a sweep over the row's own words once (max, denominator) are known: no second gather.
// Backward, four launches (no float atomics; two identical calls are bitwise equal):
//   rows      g and r[i,h] = <g, pre - bias> (attn_bwd_rows_kernel of bgnn_conv_common.h, shared with GAT).
//   by-dst    regather xl_j, rebuild e, alpha = exp(e - max) / den, da = mask * <g_i, xl_j>, de = alpha * (da - r); de and the
//             post-dropout coefficient go to [E', H] workspaces; dXR[i,h,:] = sum_t de * att (.) leaky'(m) stays in the row's
//             registers; datt[h,:] += de * leaky(m) stays in the THREAD's registers over all its rows of one head (the kernel
//             walks head by head), is reduced over the block in a fixed order and written to the block's partial row.
//   datt      adds the blocks' partial rows in a fixed order (a block per column).
//   by-src    over (t_rowptr, t_eid, t_dst): gathers g_i and xr_i, dXL[j,h,:] = sum_u coef * g_i + de * att (.) leaky'(xl_j + xr_i).
// Rows of a larger graph (row_id_opt / edge_base_opt of the two entries, a rank's rows of a node partition): both
// masks are functions of a position, and a rank's local positions are not the whole graph's.  The IDS forward hashes the feature
// mask at row_id[i] * (H*C) + column and the attention mask at (edge_base[i] + (t - rowptr[i])) * H + h: the row's GLOBAL id and the
// GLOBAL position of its first edge, both read once per virtual row; the ids feed the hash only, never an address.  The backward
// takes n_rows destination rows and n_src >= n_rows source rows (a rank's extended graph: its halo slots are sources without
// in-edges): the ROWS by-destination pass checks neighbour ids against n_src and redraws the attention mask at the global
// position, the ROWS by-source pass walks n_src sources and leaves the x_r half of the rows n_rows .. n_src as 0; the shared row
// pass takes row_id.  The plain entries launch the instantiations without the flags.
// Ids outside their table are never dereferenced and a row's edge range is cut to the edge arrays: a malformed CSR (ids or rowptr)
// gives a wrong sum, not a stray read or write.
#include "bgnn_conv_common.h"

namespace {

using namespace bgnn_conv;

constexpr int DATT_BLOCKS = 2048;   // most blocks of the by-destination pass: the partial rows of datt are sized by it

// this lane's part of one edge's logit: m = xl + xr (ONE rounded add per column), then att . leaky(m) as a fixed chain of fmas
__device__ __forceinline__ float logit_part(const float (&x)[4], const float (&xr)[4], const float (&att)[4], float slope,
                                            float (&m)[4]) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    m[c] = __fadd_rn(x[c], xr[c]);
    s = __fmaf_rn(att[c], leaky(m[c], slope), s);
  }
  return s;
}

// ---- forward ------------------------------------------------------------------------------------------------------------
struct FwdParams {
  const float* tbl; int64_t ldt; int64_t n_tbl; int32_t xr_off;   // XL at column 0, XR at column xr_off = pad4(H*C)
  const float* att;                                              // [H*C]
  const float* bias;                                             // [H*C] or NULL
  const int32_t* rowptr; const int32_t* col; int64_t n_edges; int64_t n_rows;
  int32_t H; int32_t C; int32_t npad;
  float slope;
  uint32_t athr; float akeep; uint64_t aseed; const uint64_t* aseed_dev;      // attention dropout
  uint32_t thr; float keep_scale; uint64_t seed; const uint64_t* seed_dev;    // feature dropout of the ELU epilogue
  float* state;                                                  // [n_rows, H, 2] = (max, denominator)
  float* alpha;                                                  // [E', H] post-dropout coefficients, or NULL
  float* pre; int64_t ldp;                                       // the conv output before the epilogue, or NULL
  float* out; int64_t ldo;
  const int64_t* row_id;                                         // IDS: dropout row of row i (element index row_id[i] * (H*C) + column)
  const int64_t* edge_base;                                      // IDS: position of the row's first edge in the whole graph's CSR
};

template <int LF, int EP, int U, int EPI, bool IDS = false>
__global__ __launch_bounds__(256) void gatv2_fwd_kernel(FwdParams p) {
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
  uint64_t aseed = p.aseed, seed = p.seed;
  if (p.athr != 0u && p.aseed_dev != nullptr) aseed += *p.aseed_dev;
  if (EPI == EPI_ELU && p.thr != 0u && p.seed_dev != nullptr) seed += *p.seed_dev;

  const int64_t nv = p.n_rows * p.H;
  const int64_t ntiles = (nv + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                                       // block-uniform
    const int64_t v = gt * RPB + wave * GPW + g;
    const bool valid = v < nv;                                  // n_rows <= n_tbl: the row's own XR row lies in the table
    const int64_t i = valid ? v / p.H : 0;
    const int h = valid ? (int)(v - i * p.H) : 0;
    const int64_t hoff = (int64_t)h * p.C;
    int32_t beg = 0, end = 0;
    if (valid) { beg = p.rowptr[i]; end = p.rowptr[i + 1]; }
    int64_t eshift = 0, drow = 0;                               // IDS: hashed position of edge e = e + eshift (raw rowptr[i]); dropout row
    if (IDS && valid) { eshift = p.edge_base[i] - (int64_t)beg; drow = p.row_id[i]; }
    clamp_row(beg, end, p.n_edges);
    const int32_t niter = (end - beg + EP * U - 1) / (EP * U);  // uniform inside the group
    float xr[4], att[4];
    load4(p.tbl + i * p.ldt + p.xr_off + hoff, k0, p.C, vec, valid, xr);
    load4(p.att + hoff, k0, p.C, vec, true, att);

    float mx = -INFINITY, den = 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t nid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.col[e] : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float x[U][4], lg_e[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[u] = nid[u] >= 0 && (int64_t)nid[u] < p.n_tbl;
        load4(p.tbl + (int64_t)(ok[u] ? nid[u] : 0) * p.ldt + hoff, k0, p.C, vec, ok[u], x[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.col[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float m[4];
        lg_e[u] = logit_part(x[u], xr, att, p.slope, m);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) lg_e[u] = bgnn::group_sum<LF>(lg_e[u]);   // the sub-group's LF lanes: one edge, one head
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
        const int32_t e = e0 + u * EP;
        const float ev = lg_e[u];
        const uint64_t el = (IDS ? (uint64_t)((int64_t)e + eshift) : (uint64_t)e) * (uint64_t)p.H + (uint64_t)h;
        const float mk = p.athr == 0u ? 1.f : (drop_bits(el, aseed) >= p.athr ? p.akeep : 0.f);
        if (p.alpha != nullptr && k0 == 0) p.alpha[(int64_t)e * p.H + h] = ev;     // parked: the sweep below turns it into a~
        float w;
        if (ev > mx) {                                          // mx = -inf: the scale is 0 and den, acc are 0
          const float sc = expf(mx - ev);
          den = den * sc + 1.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] *= sc;
          mx = ev;
          w = mk;
        } else {
          const float pe = expf(ev - mx);
          den += pe;
          w = mk * pe;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += w * x[u][c];
      }
    }
    // the EP sub-groups' (max, denominator, accumulator): fixed butterfly, every lane of the wave takes part
#pragma unroll
    for (int off = LF; off < GL; off <<= 1) {
      const float m2 = __shfl_xor(mx, off), d2 = __shfl_xor(den, off);
      const float M = fmaxf(mx, m2);
      const float a = mx == -INFINITY ? 0.f : expf(mx - M);
      const float b = m2 == -INFINITY ? 0.f : expf(m2 - M);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float a2 = __shfl_xor(acc[c], off);
        acc[c] = __fmul_rn(acc[c], a) + __fmul_rn(a2, b);
      }
      den = __fmul_rn(den, a) + __fmul_rn(d2, b);
      mx = M;
    }
    if (valid && lg == 0) {
      p.state[2 * v] = mx;
      p.state[2 * v + 1] = den;
    }
    if (p.alpha != nullptr && k0 == 0) {
      for (int32_t e = beg + sub; e < end; e += EP) {           // the words this very lane parked
        const int32_t j = p.col[e];
        float a = 0.f;
        if (j >= 0 && (int64_t)j < p.n_tbl) {
          a = expf(p.alpha[(int64_t)e * p.H + h] - mx) / den;
          const uint64_t el = (IDS ? (uint64_t)((int64_t)e + eshift) : (uint64_t)e) * (uint64_t)p.H + (uint64_t)h;
          if (p.athr != 0u) a = drop_bits(el, aseed) >= p.athr ? a * p.akeep : 0.f;
        }
        p.alpha[(int64_t)e * p.H + h] = a;
      }
    }
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = den > 0.f ? acc[c] / den : 0.f;
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
      if (p.thr != 0u)
        drop4(o, (uint64_t)(IDS ? drow : i) * (uint64_t)(p.H * p.C) + (uint64_t)(hoff + k0), vec, seed, p.thr, p.keep_scale);
    } else if (EPI == EPI_LOGSOFTMAX) {
      log_softmax4<LF>(o, k0, p.C);   // H == 1: the whole row (C <= 4*LF) sits in the LF lanes of the group
    }
    if (writer) {
      store4(p.out + i * p.ldo + hoff, k0, p.C, vec, o);
      if (h == p.H - 1 && lg == 0)                                // pad columns of the row leave as 0
        for (int q = 0; q < p.npad; ++q) p.out[i * p.ldo + (int64_t)p.H * p.C + q] = 0.f;
    }
  }
}

// ---- backward, by destination: de and the coefficient per edge, dXR per virtual row, datt per block -------------------------
struct DstParams {
  const float* tbl; int64_t ldt; int32_t xr_off;
  const float* att;
  const float* g; int64_t ldg;
  const float* state; const float* r;
  const int32_t* rowptr; const int32_t* col; int64_t n_edges; int64_t n_rows;
  int32_t H; int32_t C; int32_t npad;
  float slope;
  uint32_t athr; float akeep; uint64_t aseed; const uint64_t* aseed_dev;
  float* de; float* coef;                          // [E', H] each
  float* grad_tbl; int64_t ldgt;                   // dXR goes to columns [xr_off, xr_off + H*C)
  float* part;                                     // [gridDim.x, H*C] partial rows of datt
  int64_t n_src;                                   // ROWS: rows of tbl (the sources), >= n_rows
  const int64_t* edge_base;                        // ROWS: as FwdParams, or NULL (edge t is hashed at t)
};

template <int LF, int EP, int U, bool ROWS = false>
__global__ __launch_bounds__(256) void gatv2_bwd_dst_kernel(DstParams p) {
  constexpr int GL = LF * EP;
  constexpr int GPW = 64 / GL;
  constexpr int RPB = 4 * GPW;
  constexpr int SLOTS = 256 / LF;                  // threads of the block that hold the same four columns
  __shared__ float red[4 * 256];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / GL;
  const int lg = lane % GL;
  const int sub = lg / LF;
  const int k0 = (lg % LF) * 4;
  const bool vec = (p.C & 3) == 0;
  uint64_t aseed = p.aseed;
  if (p.athr != 0u && p.aseed_dev != nullptr) aseed += *p.aseed_dev;

  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int h = 0; h < p.H; ++h) {                  // head by head: a thread's datt registers belong to one head at a time
    const int64_t hoff = (int64_t)h * p.C;
    float att[4];
    load4(p.att + hoff, k0, p.C, vec, true, att);
    float datt[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
      const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
      if (gt < 0) continue;                                     // block-uniform
      const int64_t row = gt * RPB + wave * GPW + g;
      const bool valid = row < p.n_rows;
      const int64_t i = valid ? row : 0;
      const int64_t v = i * p.H + h;
      int32_t beg = 0, end = 0;
      float mx = 0.f, den = 1.f, rr = 0.f;
      float gi[4], xr[4];
      load4(p.g + i * p.ldg + hoff, k0, p.C, vec, valid, gi);
      load4(p.tbl + i * p.ldt + p.xr_off + hoff, k0, p.C, vec, valid, xr);
      if (valid) {
        beg = p.rowptr[i]; end = p.rowptr[i + 1];
        mx = p.state[2 * v]; den = p.state[2 * v + 1]; rr = p.r[v];
      }
      int64_t eshift = 0;                                       // ROWS: hashed position of edge e = e + eshift (raw rowptr[i])
      if (ROWS && valid && p.edge_base != nullptr) eshift = p.edge_base[i] - (int64_t)beg;
      clamp_row(beg, end, p.n_edges);
      const int32_t niter = (end - beg + EP * U - 1) / (EP * U);  // uniform inside the group
      float dxr[4] = {0.f, 0.f, 0.f, 0.f};
      int32_t nid[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = beg + sub + u * EP;
        nid[u] = e < end ? p.col[e] : -1;
      }
      for (int32_t it = 0; it < niter; ++it) {
        const int32_t e0 = beg + it * (EP * U) + sub;
        float m[U][4], lg_e[U], dot[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          ok[u] = nid[u] >= 0 && (int64_t)nid[u] < (ROWS ? p.n_src : p.n_rows);
          float x[4];
          load4(p.tbl + (int64_t)(ok[u] ? nid[u] : 0) * p.ldt + hoff, k0, p.C, vec, ok[u], x);
          lg_e[u] = logit_part(x, xr, att, p.slope, m[u]);
          dot[u] = gi[0] * x[0] + gi[1] * x[1] + gi[2] * x[2] + gi[3] * x[3];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int32_t e = e0 + (U + u) * EP;
          nid[u] = e < end ? p.col[e] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          lg_e[u] = bgnn::group_sum<LF>(lg_e[u]);
          dot[u] = bgnn::group_sum<LF>(dot[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int32_t e = e0 + u * EP;
          if (!ok[u]) {                                         // an id outside the table: its words leave as 0 for the by-source pass
            if (k0 == 0 && e < end) {
              p.de[(int64_t)e * p.H + h] = 0.f;
              p.coef[(int64_t)e * p.H + h] = 0.f;
            }
            continue;
          }
          const float alpha = den > 0.f ? expf(lg_e[u] - mx) / den : 0.f;
          const uint64_t el = (ROWS ? (uint64_t)((int64_t)e + eshift) : (uint64_t)e) * (uint64_t)p.H + (uint64_t)h;
          const float mk = p.athr == 0u ? 1.f : (drop_bits(el, aseed) >= p.athr ? p.akeep : 0.f);
          const float dev = alpha * (mk * dot[u] - rr);
          if (k0 == 0) {
            p.de[(int64_t)e * p.H + h] = dev;
            p.coef[(int64_t)e * p.H + h] = mk * alpha;
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            dxr[c] += dev * (att[c] * (m[u][c] > 0.f ? 1.f : p.slope));
            datt[c] += dev * leaky(m[u][c], p.slope);
          }
        }
      }
#pragma unroll
      for (int off = LF; off < GL; off <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) dxr[c] += __shfl_xor(dxr[c], off);
      }
      if (valid && sub == 0) {
        store4(p.grad_tbl + i * p.ldgt + p.xr_off + hoff, k0, p.C, vec, dxr);
        if (h == p.H - 1 && lg == 0)
          for (int q = 0; q < p.npad; ++q) p.grad_tbl[i * p.ldgt + p.xr_off + (int64_t)p.H * p.C + q] = 0.f;
      }
    }
    // datt of this head over the block, in a fixed order: column k of the head is held by the SLOTS threads with tid % LF == k / 4
    __syncthreads();                                            // the previous head's sums have been read
    {
      const int lf = threadIdx.x % LF, slot = threadIdx.x / LF;
#pragma unroll
      for (int c = 0; c < 4; ++c) red[(lf * 4 + c) * SLOTS + slot] = datt[c];
    }
    __syncthreads();
    if ((int)threadIdx.x < 4 * LF && (int)threadIdx.x < p.C) {
      float s = 0.f;
      for (int q = 0; q < SLOTS; ++q) s += red[threadIdx.x * SLOTS + q];
      p.part[((int64_t)blockIdx.x * p.H + h) * p.C + threadIdx.x] = s;
    }
  }
}

// datt[k] = the blocks' partial rows added in a fixed order: one block per column, thread t adds the rows t, t + 256, ... in
// order, then the 256 partial sums fold in a fixed tree
__global__ __launch_bounds__(256) void gatv2_datt_sum_kernel(const float* __restrict__ part, int nblocks, int HC,
                                                             float* __restrict__ grad_att) {
  __shared__ float red[256];
  const int k = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += part[(int64_t)b * HC + k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) grad_att[k] = red[0];
}

// ---- backward, by source: dXL -----------------------------------------------------------------------------------------------
struct SrcParams {
  const float* tbl; int64_t ldt; int32_t xr_off;
  const float* att;
  const float* g; int64_t ldg;
  const int32_t* t_rowptr; const int32_t* t_eid; const int32_t* t_dst; int64_t n_edges; int64_t n_rows;
  int32_t H; int32_t C; int32_t npad;
  float slope;
  const float* de; const float* coef;              // [E', H] each, by-destination order
  float* grad_tbl; int64_t ldgt;                   // dXL goes to columns [0, H*C)
  int64_t n_src;                                   // ROWS: the sources walked, >= n_rows (g and x_r are read of rows < n_rows only)
};

template <int LF, int EP, int U, bool ROWS = false>
__global__ __launch_bounds__(256) void gatv2_bwd_src_kernel(SrcParams p) {
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

  const int64_t nv = (ROWS ? p.n_src : p.n_rows) * p.H;
  const int64_t ntiles = (nv + RPB - 1) / RPB;
  const bgnn::XcdRange tr = bgnn::xcd_pos_range(ntiles);
  for (int64_t pos = tr.begin; pos < tr.end; pos += tr.step) {
    const int64_t gt = bgnn::xcd_tile_of(pos, ntiles);
    if (gt < 0) continue;                                       // block-uniform
    const int64_t v = gt * RPB + wave * GPW + g;
    const bool valid = v < nv;
    const int64_t j = valid ? v / p.H : 0;
    const int h = valid ? (int)(v - j * p.H) : 0;
    const int64_t hoff = (int64_t)h * p.C;
    int32_t beg = 0, end = 0;
    if (valid) { beg = p.t_rowptr[j]; end = p.t_rowptr[j + 1]; }
    clamp_row(beg, end, p.n_edges);
    const int32_t niter = (end - beg + EP * U - 1) / (EP * U);  // uniform inside the group
    float xl[4], att[4];
    load4(p.tbl + j * p.ldt + hoff, k0, p.C, vec, valid, xl);
    load4(p.att + hoff, k0, p.C, vec, true, att);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t nid[U], wid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t e = beg + sub + u * EP;
      nid[u] = e < end ? p.t_dst[e] : -1;
      wid[u] = e < end ? p.t_eid[e] : -1;
    }
    for (int32_t it = 0; it < niter; ++it) {
      const int32_t e0 = beg + it * (EP * U) + sub;
      float gi[U][4], xr[U][4], w[U], dv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = nid[u] >= 0 && (int64_t)nid[u] < p.n_rows && wid[u] >= 0 && (int64_t)wid[u] < p.n_edges;
        const int64_t i = ok ? nid[u] : 0;
        load4(p.g + i * p.ldg + hoff, k0, p.C, vec, ok, gi[u]);
        load4(p.tbl + i * p.ldt + p.xr_off + hoff, k0, p.C, vec, ok, xr[u]);
        w[u] = ok ? p.coef[(int64_t)wid[u] * p.H + h] : 0.f;
        dv[u] = ok ? p.de[(int64_t)wid[u] * p.H + h] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t e = e0 + (U + u) * EP;
        nid[u] = e < end ? p.t_dst[e] : -1;
        wid[u] = e < end ? p.t_eid[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float m = __fadd_rn(xl[c], xr[u][c]);           // the forward's add: the same side of the kink
          acc[c] += w[u] * gi[u][c] + dv[u] * (att[c] * (m > 0.f ? 1.f : p.slope));
        }
      }
    }
#pragma unroll
    for (int off = LF; off < GL; off <<= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += __shfl_xor(acc[c], off);
    }
    if (valid && sub == 0) {
      store4(p.grad_tbl + j * p.ldgt + hoff, k0, p.C, vec, acc);
      if (h == p.H - 1 && lg == 0)
        for (int q = 0; q < p.npad; ++q) p.grad_tbl[j * p.ldgt + (int64_t)p.H * p.C + q] = 0.f;
      if (ROWS && j >= p.n_rows) {                                // a source that is no destination row: its dXR half leaves as 0
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        store4(p.grad_tbl + j * p.ldgt + p.xr_off + hoff, k0, p.C, vec, z);
        if (h == p.H - 1 && lg == 0)
          for (int q = 0; q < p.npad; ++q) p.grad_tbl[j * p.ldgt + p.xr_off + (int64_t)p.H * p.C + q] = 0.f;
      }
    }
  }
}


// ---- launchers ----------------------------------------------------------------------------------------------------------
template <int LF, int EP, int U, int EPI, bool IDS>
int launch_fwd(const FwdParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows * p.H + RPB - 1) / RPB;
  const int grid = persistent_grid(gatv2_fwd_kernel<LF, EP, U, EPI, IDS>, ntiles, &cap);
  hipLaunchKernelGGL((gatv2_fwd_kernel<LF, EP, U, EPI, IDS>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <bool IDS>
int dispatch_fwd(int epilogue, const FwdParams& p, hipStream_t st) {
  // four neighbour rows in flight on every rung (the ladder's U is not taken): each carries its logit beside its four columns
  return epi_switch(epilogue, [&](auto EPI) {
    return lf_ladder((p.C + 3) / 4, [&](auto LF, auto EP, auto) { return launch_fwd<LF, EP, 4, EPI, IDS>(p, st); });
  });
}

template <int LF, int EP, int U, bool ROWS>
int launch_dst(DstParams p, hipStream_t st, int* grid_out) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = (p.n_rows + RPB - 1) / RPB;
  int grid = persistent_grid(gatv2_bwd_dst_kernel<LF, EP, U, ROWS>, ntiles, &cap);
  if (grid > DATT_BLOCKS) grid = DATT_BLOCKS;                   // a multiple of 8 as well
  *grid_out = grid;
  hipLaunchKernelGGL((gatv2_bwd_dst_kernel<LF, EP, U, ROWS>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

template <int LF, int EP, int U, bool ROWS>
int launch_src(const SrcParams& p, hipStream_t st) {
  constexpr int RPB = 4 * (64 / (LF * EP));
  static int cap = 0;
  const int64_t ntiles = ((ROWS ? p.n_src : p.n_rows) * p.H + RPB - 1) / RPB;
  const int grid = persistent_grid(gatv2_bwd_src_kernel<LF, EP, U, ROWS>, ntiles, &cap);
  hipLaunchKernelGGL((gatv2_bwd_src_kernel<LF, EP, U, ROWS>), dim3((unsigned)grid), dim3(256), 0, st, p);
  BGNN_LAUNCH_CHECK();
  return 0;
}

size_t part_bytes(int32_t H, int32_t C) { return bgnn_align_up((size_t)DATT_BLOCKS * (size_t)H * (size_t)C * sizeof(float), 16); }
size_t rows_bytes(int64_t n_rows, int32_t H) { return bgnn_align_up((size_t)n_rows * (size_t)H * sizeof(float), 16); }

// the one table [rows, >= 2 * pad4(H*C)] with XL and XR: 16-byte aligned base, leading dimension a multiple of 4
bool cat_ok(const float* t, int64_t ld, int32_t HC) { return bgnn_aligned16(t) && (ld & 3) == 0 && ld >= 2 * (((int64_t)HC + 3) / 4 * 4); }

}  // namespace

extern "C" size_t bgnn_gatv2_aggregate_workspace_bytes(int64_t n_edges, int64_t n_rows, int32_t H, int32_t C) {
  if (n_edges < 0 || n_rows < 0 || !shape_ok(H, C)) return 0;
  return 2 * coef_bytes(n_edges, H) + rows_bytes(n_rows, H) + part_bytes(H, C) + 16;
}

// the ids matter only where a mask is drawn: without dropout the plain instantiations run
extern "C" int bgnn_gatv2_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* att, const float* bias_opt,
                                        const int32_t* rowptr, const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t H,
                                        int32_t C, float negative_slope, float p_att, uint64_t seed_att,
                                        const uint64_t* seed_att_dev_opt, int epilogue, float p_drop, uint64_t seed,
                                        const uint64_t* seed_dev_opt, const int64_t* row_id_opt, const int64_t* edge_base_opt,
                                        float* state, float* alpha_out_opt, float* pre_out_opt, int64_t ldp, float* out, int64_t ldo,
                                        void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tbl || !att || !rowptr || !col || !state || !out) return BGNN_E_NULL;
  if ((row_id_opt == nullptr) != (edge_base_opt == nullptr)) return BGNN_E_NULL;  // the forward hashes both: given together
  if (n_rows < 0 || n_tbl < n_rows || n_edges < 0 || !shape_ok(H, C) || !(p_att >= 0.f && p_att < 1.f)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, C)) return rc;
  if (epilogue == EPI_LOGSOFTMAX && H != 1) return BGNN_E_SHAPE;
  const int32_t HC = H * C;
  if (!cat_ok(tbl, ldt, HC) || !tbl_ok(out, ldo, HC) || (pre_out_opt && !tbl_ok(pre_out_opt, ldp, HC))) return BGNN_E_ALIGN;
  if (!bgnn_aligned16(att) || (bias_opt && !bgnn_aligned16(bias_opt))) return BGNN_E_ALIGN;
  if (n_rows == 0) return 0;
  FwdParams p{};
  p.tbl = tbl; p.ldt = ldt; p.n_tbl = n_tbl; p.xr_off = (HC + 3) / 4 * 4; p.att = att; p.bias = bias_opt;
  p.rowptr = rowptr; p.col = col; p.n_edges = n_edges; p.n_rows = n_rows; p.H = H; p.C = C; p.npad = p.xr_off - HC;
  p.slope = negative_slope;
  att_drop_consts(p_att, p.athr, p.akeep);
  p.aseed = seed_att; p.aseed_dev = seed_att_dev_opt;
  drop_consts(p_drop, p.thr, p.keep_scale);
  p.seed = seed; p.seed_dev = seed_dev_opt;
  p.state = state; p.alpha = alpha_out_opt; p.pre = pre_out_opt; p.ldp = ldp; p.out = out; p.ldo = ldo;
  p.row_id = row_id_opt; p.edge_base = edge_base_opt;
  if (row_id_opt != nullptr && (p.athr != 0u || (epilogue == EPI_ELU && p.thr != 0u))) return dispatch_fwd<true>(epilogue, p, st);
  return dispatch_fwd<false>(epilogue, p, st);
}

extern "C" int bgnn_gatv2_aggregate_bwd_f32(const float* tbl, int64_t ldt, int64_t n_src, const float* att, const float* bias_opt,
                                            const float* state, const float* pre, int64_t ldp, const float* grad_y, int64_t ldgy,
                                            const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_eid,
                                            const int32_t* t_dst, int64_t n_edges, int64_t n_rows, int32_t H, int32_t C,
                                            float negative_slope, float p_att, uint64_t seed_att, const uint64_t* seed_att_dev_opt,
                                            int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, void* ws,
                                            size_t ws_bytes, const int64_t* row_id_opt, const int64_t* edge_base_opt, float* g,
                                            int64_t ldg, float* grad_tbl, int64_t ldgt, float* grad_att, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tbl || !att || !state || !pre || !grad_y || !rowptr || !col || !t_rowptr || !t_eid || !t_dst || !ws || !g || !grad_tbl || !grad_att)
    return BGNN_E_NULL;
  if ((row_id_opt == nullptr) != (edge_base_opt == nullptr)) return BGNN_E_NULL;
  if (n_rows < 0 || n_src < n_rows || n_edges < 0 || !shape_ok(H, C) || !(p_att >= 0.f && p_att < 1.f)) return BGNN_E_SHAPE;
  if (const int rc = epi_check(epilogue, p_drop, C)) return rc;
  if (epilogue == EPI_LOGSOFTMAX && H != 1) return BGNN_E_SHAPE;
  const int32_t HC = H * C;
  if (!cat_ok(tbl, ldt, HC) || !cat_ok(grad_tbl, ldgt, HC) || !tbl_ok(pre, ldp, HC) || !tbl_ok(grad_y, ldgy, HC) || !tbl_ok(g, ldg, HC))
    return BGNN_E_ALIGN;
  if (!bgnn_aligned16(att) || (bias_opt && !bgnn_aligned16(bias_opt))) return BGNN_E_ALIGN;
  if (ws_bytes < bgnn_gatv2_aggregate_workspace_bytes(n_edges, n_rows, H, C)) return BGNN_E_WORKSPACE;
  float* de = reinterpret_cast<float*>(bgnn_align_up(reinterpret_cast<uintptr_t>(ws), 16));
  float* coef = de + coef_bytes(n_edges, H) / sizeof(float);
  float* r = coef + coef_bytes(n_edges, H) / sizeof(float);
  float* part = r + rows_bytes(n_rows, H) / sizeof(float);
  const int32_t P = (HC + 3) / 4 * 4, npad = P - HC;
  if (n_rows == 0) {                                              // no destination row, so no edge: every gradient is 0
    if (const hipError_t e = hipMemsetAsync(grad_att, 0, (size_t)HC * sizeof(float), st)) return (int)e;
    if (n_src == 0) return 0;
    return (int)hipMemset2DAsync(grad_tbl, (size_t)ldgt * sizeof(float), 0, (size_t)(2 * P) * sizeof(float), (size_t)n_src, st);
  }
  const bool ext = n_src != n_rows;
  {
    RowParams q{};
    q.pre = pre; q.ldp = ldp; q.gy = grad_y; q.ldgy = ldgy; q.bias = bias_opt; q.n_rows = n_rows; q.H = H; q.C = C; q.npad = npad;
    drop_consts(p_drop, q.thr, q.keep_scale);
    q.seed = seed; q.seed_dev = seed_dev_opt;
    q.g = g; q.ldg = ldg; q.r = r; q.row_id = row_id_opt;
    if (const int rc = dispatch_rows(epilogue, q, st)) return rc;
  }
  {
    DstParams d{};
    d.tbl = tbl; d.ldt = ldt; d.xr_off = P; d.att = att; d.g = g; d.ldg = ldg; d.state = state; d.r = r;
    d.rowptr = rowptr; d.col = col; d.n_edges = n_edges; d.n_rows = n_rows; d.H = H; d.C = C; d.npad = npad; d.slope = negative_slope;
    att_drop_consts(p_att, d.athr, d.akeep);
    d.aseed = seed_att; d.aseed_dev = seed_att_dev_opt;
    d.de = de; d.coef = coef; d.grad_tbl = grad_tbl; d.ldgt = ldgt; d.part = part;
    d.n_src = n_src; d.edge_base = d.athr != 0u ? edge_base_opt : nullptr;
    int grid = 0;
    const int rc = (ext || d.edge_base != nullptr)
                       ? lf_ladder((C + 3) / 4, [&](auto LF, auto EP, auto) { return launch_dst<LF, EP, 4, true>(d, st, &grid); })
                       : lf_ladder((C + 3) / 4, [&](auto LF, auto EP, auto) { return launch_dst<LF, EP, 4, false>(d, st, &grid); });
    if (rc != 0) return rc;
    hipLaunchKernelGGL(gatv2_datt_sum_kernel, dim3((unsigned)HC), dim3(256), 0, st, part, grid, (int)HC, grad_att);
    BGNN_LAUNCH_CHECK();
  }
  SrcParams s{};
  s.tbl = tbl; s.ldt = ldt; s.xr_off = P; s.att = att; s.g = g; s.ldg = ldg; s.t_rowptr = t_rowptr; s.t_eid = t_eid; s.t_dst = t_dst;
  s.n_edges = n_edges; s.n_rows = n_rows; s.H = H; s.C = C; s.npad = npad; s.slope = negative_slope; s.de = de; s.coef = coef;
  s.grad_tbl = grad_tbl; s.ldgt = ldgt; s.n_src = n_src;
  if (ext) return lf_ladder((C + 3) / 4, [&](auto LF, auto EP, auto) { return launch_src<LF, EP, 4, true>(s, st); });
  return lf_ladder((C + 3) / 4, [&](auto LF, auto EP, auto) { return launch_src<LF, EP, 4, false>(s, st); });
}
