// Multi-tensor Adam (main_graph_knowledge_transfer.py:205, :353 `torch.optim.Adam(lr, weight_decay)`, stepped at :67, :274) as ONE
// launch over every parameter tensor of a model, with its step number and its learning-rate schedule on the device, so that the
// update can sit inside a captured training step: nothing about it is baked into the graph but pointers.
//   records  [n_tensors][5] int64: parameter, gradient, exp_avg, exp_avg_sq (device addresses), element count.  A NULL gradient
//            skips the tensor, as torch skips a parameter whose .grad is None.
//   chunk map [n_chunks][2] int32: (tensor, chunk of that tensor); a chunk is ADAM_CHUNK consecutive elements, one block each, so one
//            grid covers a 31-element bias and an F x hidden weight alike.
//   step     device int64: the number of THIS step (1 for the first).  The kernel only reads it: whoever owns the loop advances it
//            (one word then also indexes the dropout seeds and the history row of a captured epoch).
//   lr_table device fp64 [lr_len]: the learning rate of step s is lr_table[min(s, lr_len) - 1]: the values a host scheduler
//            produced, not a re-derivation of them.
// Arithmetic: torch's `_single_tensor_adam` (amsgrad=False, maximize=False), L2 weight decay folded into the gradient, bias
// corrections and step size formed in fp64 from the step and rounded to fp32 where torch hands them to its fp32 kernels:
//   g += wd p;  m = lerp(m, g, 1 - b1);  v = v b2 + (1 - b2) g g;  p -= (lr / (1 - b1^s)) m / (sqrt(v) / sqrt(1 - b2^s) + eps).
// Every element is owned by one thread: no atomics, nothing to clear, vector stores only.
#include "bgnn_common.h"

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = 1024;           // elements per block: one float4 per thread on the aligned path

struct AdamRec {
  int64_t p, g, m, v, n;
};

struct AdamScalars {
  float wd, w1, b2, w2, bc2s, eps, neg_step;
  int lerp_low;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s) {
  if (s.wd != 0.f) g = g + s.wd * p;                                           // grad.add(param, alpha=weight_decay)
  const float d = g - m;
  m = s.lerp_low ? m + s.w1 * d : g - d * (1.f - s.w1);                        // exp_avg.lerp_(grad, 1 - beta1)
  v = __fmul_rn(v, s.b2);                                                      // exp_avg_sq.mul_(beta2): a kernel of its own in torch, so rounded
  v = v + s.w2 * g * g;                                                        //           .addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / s.bc2s + s.eps;                               // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p = p + s.neg_step * (m / denom);                                            // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const AdamRec* __restrict__ recs, int32_t n_tensors,
                                                                 const int32_t* __restrict__ chunk_map, const int64_t* __restrict__ step_p,
                                                                 const double* __restrict__ lr_table, int64_t lr_len, double beta1,
                                                                 double beta2, double eps, double wd) {
  const int32_t ti = chunk_map[2 * (int64_t)blockIdx.x], ci = chunk_map[2 * (int64_t)blockIdx.x + 1];
  if (ti < 0 || ti >= n_tensors || ci < 0) return;
  const AdamRec r = recs[ti];
  if (r.g == 0 || r.n <= 0) return;                                            // no gradient: the tensor is skipped
  const int64_t base = (int64_t)ci * ADAM_CHUNK;
  if (base >= r.n) return;
  int64_t step = *step_p;
  if (step < 1) step = 1;
  const double lr = lr_table[(step < lr_len ? step : lr_len) - 1];
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  AdamScalars s;
  s.wd = (float)wd;
  s.w1 = (float)(1.0 - beta1);
  s.lerp_low = (1.0 - beta1) < 0.5;
  s.b2 = (float)beta2;
  s.w2 = (float)(1.0 - beta2);
  s.bc2s = (float)sqrt(bc2);
  s.eps = (float)eps;
  s.neg_step = (float)(-(lr / bc1));
  float* __restrict__ p = reinterpret_cast<float*>(r.p);
  const float* __restrict__ g = reinterpret_cast<const float*>(r.g);
  float* __restrict__ m = reinterpret_cast<float*>(r.m);
  float* __restrict__ v = reinterpret_cast<float*>(r.v);
  const int64_t left = r.n - base;
  const int cnt = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
  const bool vec = ((r.p | r.g | r.m | r.v) & 15) == 0;                         // (base * 4 bytes keeps the alignment)
  const int t = threadIdx.x;
  if (vec && 4 * t + 4 <= cnt) {
    const int64_t e = base + 4 * t;
    float4 P = *reinterpret_cast<const float4*>(p + e), M = *reinterpret_cast<const float4*>(m + e);
    float4 V = *reinterpret_cast<const float4*>(v + e);
    const float4 G = *reinterpret_cast<const float4*>(g + e);
    adam_elem(P.x, G.x, M.x, V.x, s);
    adam_elem(P.y, G.y, M.y, V.y, s);
    adam_elem(P.z, G.z, M.z, V.z, s);
    adam_elem(P.w, G.w, M.w, V.w, s);
    *reinterpret_cast<float4*>(p + e) = P;
    *reinterpret_cast<float4*>(m + e) = M;
    *reinterpret_cast<float4*>(v + e) = V;
  }
  // unaligned tensors, and the last (partial) float4 of an aligned one (threads 0..2)
  const int first = vec ? (cnt & ~3) : 0;
  for (int i = first + t; i < cnt; i += ADAM_THREADS) {
    const int64_t e = base + i;
    float P = p[e], M = m[e], V = v[e];
    adam_elem(P, g[e], M, V, s);
    p[e] = P;
    m[e] = M;
    v[e] = V;
  }
}

}  // namespace

extern "C" int64_t bgnn_adam_chunk_elems(void) { return ADAM_CHUNK; }

extern "C" int bgnn_adam_step_f32(const void* records, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks, const int64_t* step,
                                  const double* lr_table, int64_t lr_len, double beta1, double beta2, double eps, double weight_decay,
                                  void* stream) {
  if (n_tensors == 0 || n_chunks == 0) return 0;
  if (!records || !chunk_map || !step || !lr_table) return BGNN_E_NULL;
  if (n_tensors < 0 || n_chunks < 0 || n_chunks > 0x7FFFFFFF || lr_len < 1) return BGNN_E_SHAPE;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return BGNN_E_RANGE;
  if ((reinterpret_cast<uintptr_t>(records) & 7u) || (reinterpret_cast<uintptr_t>(chunk_map) & 3u)) return BGNN_E_ALIGN;
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const AdamRec*>(records), n_tensors, chunk_map, step, lr_table, lr_len, beta1, beta2, eps,
                     weight_decay);
  BGNN_LAUNCH_CHECK();
  return 0;
}
