// Parameters and host-side pieces of the atomic-free ("pull") aggregation backward, shared by its three files: the general and
// narrow kernels, the heads pair and the one dispatcher (bgnn_aggregate_bwd.hip), the 32-bit-addressed pair for the plain
// 64 < D <= 128 launch (bgnn_aggregate_bwd_fast.hip) and the wave-per-row pair for 128 < D <= 256 (bgnn_aggregate_bwd_wide.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/bgnn.h"

namespace bgnn_bwd {

struct PullParams {
  const float* h_t2s; const float* h_s2t; int64_t ldh;
  const float* a_t2s; const float* a_s2t;
  const int32_t* rowptr; const int32_t* col; const uint8_t* mask;
  int64_t N; int32_t D; float slope;
  const float* out; int64_t ldo; const float* alpha; const float* gout; int64_t ldg;
  const int32_t* t_rowptr; const int32_t* t_eid; const int32_t* t_dst;
  uint4* rec;            // [E'][2]
  unsigned int* queue;   // [16] per-XCD dynamic tile counters (pass A: 0..7, pass B: 8..15), zeroed per call
  float* dstside;        // [N][ldh]
  float* dh_t2s; float* dh_s2t; float* da_t2s; float* da_s2t;
  // Hub rows (wide kernels; the forward's scheme, bgnn_aggregate.hip AggParams): a row is walked by one lane group, so a row of
  // ~750 edges (the Twitter_Graph stand-in's source nodes) is a chain of ~190 dependent steps.  Rows with >= hub_threshold edges
  // are skipped as rows and walked as <= 64-edge segments that ride behind the real rows of the same launch; a segment leaves
  // its partial row sums in scratch and a merge launch adds them in a fixed order (deterministic like the rest).  Pass A
  // segments destinations by in-degree (d_*), pass B sources by out-degree (s_*, offsets into the by-source arrays).
  int32_t hub_threshold;
  const int32_t* d_vnode; const int32_t* d_vbounds; int64_t d_nv; float* d_vpart;                 // [d_nv][ldh]
  const int32_t* s_vnode; const int32_t* s_vbounds; int64_t s_nv; float* s_vpartS; float* s_vpartT;   // [s_nv][ldh] each
  // agg_bwd_*_fast_kernel only (filled by pull_fast_plan): both tables inside ONE window of < 4 GB (bgnn_aggregate.hip: fast_plan)
  int64_t E;
  const char* tbl_base;
  uint32_t tbl_bytes, off_t2s, off_s2t, dead_off;
};

// The hub argument group of the C entries (device pointers), in the entries' argument order.  Pass A segments destinations
// (d_*, over rowptr / col), pass B sources (s_*, over the by-source arrays); *_nv counts the segments of a side.
struct PullHubs {
  int32_t threshold;
  const int32_t* d_rows; int64_t d_nh; const int32_t* d_seg_ptr; const int32_t* d_bounds; const int32_t* d_node; int64_t d_nv;
  const int32_t* s_rows; int64_t s_nh; const int32_t* s_seg_ptr; const int32_t* s_bounds; const int32_t* s_node; int64_t s_nv;
  bool any() const { return d_nh > 0 || s_nh > 0; }
};

// Validates the group; no hubs on either side (tables may then be NULL, the threshold is not looked at) means no hub rows.
// A side without hubs has no segments afterwards.
inline int pull_hubs_check(PullHubs& h) {
  if (h.d_nh < 0 || h.s_nh < 0 || (h.d_nh > 0 && h.d_nv < h.d_nh) || (h.s_nh > 0 && h.s_nv < h.s_nh)) return BGNN_E_SHAPE;
  if (h.any() && h.threshold < 2) return BGNN_E_SHAPE;
  if ((h.d_nh > 0 && (!h.d_rows || !h.d_seg_ptr || !h.d_bounds || !h.d_node)) ||
      (h.s_nh > 0 && (!h.s_rows || !h.s_seg_ptr || !h.s_bounds || !h.s_node)))
    return BGNN_E_NULL;
  if (h.d_nh == 0) h.d_nv = 0;
  if (h.s_nh == 0) h.s_nv = 0;
  return 0;
}

// The hub fields of PullParams / HeadsBwdParams (same names): segment tables, and the segments' partial rows of `ld` floats
// carved from `seg` (d_nv rows of pass A, then s_nv rows per domain of pass B).  Without hubs the fields stay zero.
template <class P>
inline void pull_set_hubs(P& p, const PullHubs& h, float* seg, int64_t ld) {
  if (!h.any()) return;
  p.hub_threshold = h.threshold;
  p.d_vnode = h.d_node; p.d_vbounds = h.d_bounds; p.d_nv = h.d_nv; p.d_vpart = seg;
  p.s_vnode = h.s_node; p.s_vbounds = h.s_bounds; p.s_nv = h.s_nv;
  p.s_vpartS = seg + (size_t)h.d_nv * ld; p.s_vpartT = seg + (size_t)(h.d_nv + h.s_nv) * ld;
}

// Workspace of a route as byte offsets (256-byte aligned), from ONE function per route that both the workspace query and the
// entry use: records (per edge; per node for the heads pair) | dstside | queue | da chunk rows | da slice rows (D > 128 only) |
// hub segment rows.  `total` is what the query returns and the least the entry accepts.
struct PullLayout {
  size_t rec, dstside, queue, da_part, da_stage, seg, total;
  int64_t nparts;        // da chunk rows (D > 128)
};

// Grid cap of a persistent pass A / pass B pair: what stays resident (blocks per CU of the tighter kernel, at most 8), in
// multiples of the 8 XCDs.  Callers keep the result in a function-local static, so the query runs once per pair.
template <class KA, class KB>
inline int resident_cap(KA pass_a, KB pass_b) {
  int a = 0, b = 0, dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 2048;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, pass_a, 256, 0) != hipSuccess || a < 1) return 2048;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, pass_b, 256, 0) != hipSuccess || b < 1) return 2048;
  int per_cu = a < b ? a : b;
  if (per_cu > 8) per_cu = 8;
  return per_cu * prop.multiProcessorCount / 8 * 8;
}
inline unsigned resident_grid(int64_t ntiles, int64_t cap) {
  const int64_t grid = ntiles < cap ? (ntiles + 7) / 8 * 8 : cap;
  return (unsigned)(grid < 8 ? 8 : grid);
}

// Can the launch run the fast pair (no hub rows, 64 < D <= 128, windows below 4 GB, N <= 2^24)?  Fills the window fields.
bool pull_fast_plan(PullParams& p);
// pass A (by destination) + pass B (by source) on `st`; p.queue zeroed by the caller
int pull_fast_launch(const PullParams& p, hipStream_t st);
// The D > 128 pair: its workspace layout, and pass A + merge + da sums + pass B + merge on `st` with `ws` laid out by it;
// p.queue zeroed by the caller
PullLayout pull_wide_plan(int64_t N, int64_t E, int64_t ldh, int64_t d_nv, int64_t s_nv);
int pull_wide_launch(const PullParams& p, const PullHubs& hubs, const PullLayout& w, void* ws, hipStream_t st);
// Merges of the hub segments' partial rows of `ld` floats in a fixed order (pull_merge_dst_kernel / pull_merge_src_kernel,
// bgnn_aggregate_bwd.hip), after pass A / after pass B; nothing is launched for a side without hubs.
int pull_merge_dst_launch(const PullHubs& hubs, int64_t ld, const float* d_vpart, const uint8_t* mask, float* dstside, hipStream_t st);
int pull_merge_src_launch(const PullHubs& hubs, int64_t ld, const float* s_vpartS, const float* s_vpartT, const uint8_t* mask,
                          float* dstside, float* dh_t2s, float* dh_s2t, hipStream_t st);

}  // namespace bgnn_bwd
