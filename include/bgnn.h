/* bgnn.h -- C ABI of libbgnn_hip.so: the MI355X (gfx950) drop-in for Bridged-GNN's hot path.
 *
 * The reference (wendongbi/Bridged-GNN) is pure Python and has NO FFI layer; its "operator
 * surface" is Python call signatures.  Each entry point below replaces the
 * third-party/ATen kernels launched by one reference call site; the reference interface it
 * stands in for is cited as file:line relative to Bridged-GNN/.  bridged_gnn_amd/_lib.py is the
 * ctypes binding a maintainer would add; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in `_host`;
 *   - nothing is allocated inside; scratch is passed as (ws, ws_bytes) sized by *_workspace_bytes;
 *   - calls are asynchronous on `stream` (a hipStream_t passed as void*), reentrant, no globals;
 *   - return value: 0 = success, <0 = argument error (BGNN_E_*), >0 = hipError_t of a failed launch;
 *   - row-major, fp32 features, int32 CSR, int64 edge_index ([2,E] contiguous, row 0 = source /
 *     "from", row 1 = destination / "to" as in torch_geometric).
 */
#ifndef BGNN_H_
#define BGNN_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision.  110 (round 3) is NOT call-compatible with 100: `bgnn_transform_bwd_prep_f32` takes 22 arguments (was 17)
 * and the `n_fallback_opt` of `bgnn_cosine_topk_f32` / `bgnn_mlp_pair_topk_f32` is int32[2] (was int32[1]) -- a caller built
 * against the old header must be recompiled; compare bgnn_version() with the BGNN_VERSION it was built with at load time.
 * 111 adds bgnn_adaptedconv_transform_need_f32, 112 bgnn_classifier_stage_f32, 113 bgnn_adaptedconv_aggregate_bounded_f32 (all
 * call-compatible with 110).  The GraphSAGE entry points (bgnn_sage_mean_aggregate_f32, bgnn_sage_mean_aggregate_bwd_f32 and its
 * workspace size) were added later as purely additive symbols: no existing signature changed, so the revision stays 113.  The
 * same holds for partitioned GraphSAGE's bgnn_rows_segment_add_f32, and for the similarity-learner pair passes
 * bgnn_pair_mlp_{stats,loss,segsum,eval}_f32 and their workspace size, and for the cosine scorer's
 * bgnn_pair_cos_{loss,segsum,count}_f32 and their workspace sizes, and for step 2's loss and metric passes
 * bgnn_step2_{loss,loss_bwd,nll,nll_bwd,counts,auc_count}_f32 and their workspace size, and for the GCN baseline's
 * bgnn_gcn_aggregate_f32, bgnn_gcn_aggregate_bwd_f32 and their workspace size, and for the GAT baseline's bgnn_gat_scores_f32,
 * bgnn_gat_aggregate_f32, bgnn_gat_aggregate_bwd_f32 and their workspace size (added after 114 without changing it), and for the
 * GATv2 baseline's bgnn_gatv2_aggregate_f32,
 * bgnn_gatv2_aggregate_bwd_f32 and their workspace size (likewise), and for bgnn_adaptedconv_aggregate_queued_f32 with
 * bgnn_aggregate_tile_queue_words (a tile queue of a stated size; the older entries keep their 8-word queue).
 * 114 is NOT call-compatible with 113: bgnn_adaptedconv_aggregate_bwd_pull_f32 and bgnn_adaptedconv_aggregate_heads_bwd_f32 take
 * the hub-table argument list for every width (heads: without t_eid), their workspace functions take the segment counts (the
 * single-head one also D), and the _pull_hub_, _pull_wide_ and _heads_bwd_hub_ entries and workspace functions are gone.
 * 115 is NOT call-compatible with 114: bgnn_adaptedconv_transform_f32 takes delta_opt AND sums_opt (exactly one non-NULL), the
 * tail counts, the need mask and the team runs for every caller, and the _transform_sums_, _transform_need_ and
 * _transform_need2_ entries that each took a prefix of that list are gone.
 * 116 is NOT call-compatible with 115: bgnn_sage_mean_aggregate_f32, bgnn_gcn_aggregate_f32, bgnn_gat_aggregate_f32,
 * bgnn_gat_aggregate_bwd_f32, bgnn_gatv2_aggregate_f32 and bgnn_gatv2_aggregate_bwd_f32 take the ids (and n_src) for every caller;
 * the _rows_ entries are gone.  The APPNP baseline's bgnn_appnp_propagate_f32 with its workspace size, bgnn_appnp_log_softmax_bwd_f32 and
 * bgnn_feature_dropout_f32 / bgnn_feature_dropout_bwd_f32 were added after 116 as purely additive symbols, and so were the
 * partitioned APPNP's bgnn_appnp_step_f32 and bgnn_feature_dropout_rows_f32 / bgnn_feature_dropout_rows_bwd_f32, and the GCNII
 * baseline's bgnn_gcn2_conv_f32 with its workspace size and bgnn_gcn2_conv_bwd_f32, and the partitioned GCNII's
 * bgnn_gcn2_conv_rows_f32, and the DeeperGCN baseline's bgnn_gen_softmax_aggregate_f32, bgnn_gen_softmax_aggregate_bwd_f32 and
 * its workspace size, and the GIN baseline's bgnn_gin_aggregate_f32, bgnn_gin_aggregate_bwd_f32 and its workspace size, and the
 * JKNet baseline's bgnn_jk_gcn_aggregate_f32, bgnn_jk_gcn_aggregate_bwd_f32, bgnn_jk_head_supported, bgnn_jk_head_f32 and
 * bgnn_jk_max_route_f32, and the segmented hub rows of the GIN walk: bgnn_gin_aggregate_hub_f32, bgnn_gin_aggregate_bwd_hub_f32 and
 * bgnn_gin_aggregate_hub_workspace_bytes. */
#define BGNN_VERSION 116
#define BGNN_E_NULL (-1)        /* required pointer is NULL                     */
#define BGNN_E_SHAPE (-2)       /* unsupported / inconsistent shape             */
#define BGNN_E_WORKSPACE (-3)   /* ws_bytes smaller than *_workspace_bytes()    */
#define BGNN_E_ALIGN (-4)       /* pointer or leading dimension not 16-B aligned */
#define BGNN_E_RANGE (-5)       /* k / index range not supported                */

int bgnn_version(void);
const char* bgnn_error_string(int code);
/* digest of the sources this library was built from (csrc/Makefile: HASHED); the loader compares it with the
 * tree next to the library so that a stale build cannot load silently.                         */
const char* bgnn_source_hash(void);

/* ------------------------------------------------------------------------------------------
 * (a10) graph_partition -> by-destination CSR.         models/KTGNN.py:385-398, cached :409-412
 * Drops self loops and appends one per node (rewrite_self_loops=1, the reference behaviour:
 * PyG remove_self_loops + add_self_loops), then groups edges by DESTINATION.  Inside a row the
 * order is input order with the self loop last (stable), so results are run-to-run identical.
 * The (edge_index1, edge_index2) split of the reference is the per-row domain flag mask[i].
 * col / eperm need capacity E+N.  *E_out_dev (device int64) receives E' = rowptr[N].
 * eperm_opt[t] = position of CSR slot t in the rewritten edge list (kept edges in input order,
 * then the N self loops) -- lets a caller map `alpha` back to the reference's edge order.      */
size_t bgnn_csr_workspace_bytes(int64_t N, int64_t E);
int bgnn_build_dst_csr(const int64_t* edge_index, int64_t E, int64_t N, int rewrite_self_loops,
                       int32_t* rowptr, int32_t* col, int32_t* eperm_opt, int64_t* E_out_dev,
                       void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a11) AdaptedConv dense part.                                       models/KTGNN.py:275-284
 * bgnn_domain_sums_f64: per-domain column sums of x ([2*Din] doubles: S then T) and node counts
 *   ([2] doubles) accumulated into sums_io (caller zeroes it; multi-GPU callers all-reduce it).
 * bgnn_domain_delta_f32: delta = sums_S/n_S - sums_T/n_T                        (:275)
 * bgnn_adaptedconv_transform_f32:                                               (:277-284)
 *   gate_s = tanh(x.g_s2t[:Din] + delta.g_s2t[Din:]),  gate_t likewise with g_t2s
 *   h_s2t = lin_t(x - gate_s*delta*[i in S]) ; h_t2s = lin_s(x + gate_t*delta*[i in T])
 *   evaluated by linearity as  W x + b -/+ gate * (W delta)  in ONE pass over x (the gate GEMVs ride in the staging
 *   loads, the rank-1 shift in the epilogue).  Products: for >= 128 packed columns and Din <= 128 every fp32 operand is
 *   split exactly into three bf16 pieces and a product is the six piece MFMAs >= 2^-24 relative
 *   (v_mfma_f32_32x32x16_bf16, fp32 accumulate; ~2e-7 relative to fp32 arithmetic); other shapes use
 *   v_mfma_f32_32x32x2_f32.  tanh of the gates: exp/rcp form, absolute error < 5e-7.  Up to n_heads = 2 convs that share the input x (clf_base / clf_target,
 *   KTGNN.py:432,:434) are evaluated together.
 *   Wp     [n_heads*2*ldh, Din] packed weights: per head ldh rows of lin_t.weight (rows >= D zero)
 *          followed by ldh rows of lin_s.weight (torch Linear.weight layout [out, in]);
 *   bias_p [n_heads*2*ldh]      matching packed biases (zeros where absent / padded);
 *   gates  [n_heads][2][2*Din]  a_g_s2t.weight then a_g_t2s.weight per head ([x || delta] order);
 *   gate_const_opt [n_heads][2] constants added to the gates' pre-activations (NULL = 0).  Together with composed
 *          weights this evaluates a conv on x' = x.M^T + c WITHOUT materialising x' (KTGNN.py:433: clf_target on
 *          clf_transformer's last Linear): W x' + b = (W M) x + (W c + b), [x'||delta'].g = x.(M^T g_x) + c.g_x + delta.(M^T g_d);
 *   each output row holds ldh >= D floats (ldh % 4 == 0; columns D..ldh-1 come out as 0) and rows are
 *   row_stride >= ldh floats apart (row_stride % 4 == 0), so several convs' tables can be interleaved in one
 *   allocation (multi-GPU: one halo exchange then carries the rows of all of them).
 * small_ws: n_heads*(2*ldh+2) floats of scratch (W.delta and the gates' delta halves).
 * The ONE transform entry takes delta or the domain sums, and optionally tail groups, a per-tile need mask and team
 * runs: see its declaration below.                                                           */
int bgnn_domain_sums_f64(const float* x, int64_t N, int32_t Din, int64_t ldx, const uint8_t* mask,
                         double* sums_io /*[2*Din+2]*/, void* stream);
/* Two-stage form of bgnn_domain_sums_f64 (same result up to fp64 summation order, and run-to-run identical): every CU
 * streams its share and leaves a partial row in ws (bgnn_domain_sums_workspace_bytes(Din) bytes, no initialisation
 * needed), a second small launch adds the rows into sums_io -- no atomics.  Same speed as the one-launch form on MI355X
 * (1M x 128: 0.11 ms either way); its point is determinism. */
size_t bgnn_domain_sums_workspace_bytes(int32_t Din);
int bgnn_domain_sums_ws_f64(const float* x, int64_t N, int32_t Din, int64_t ldx, const uint8_t* mask,
                            double* sums_io /*[2*Din+2]*/, void* ws, size_t ws_bytes, void* stream);
int bgnn_domain_delta_f32(const double* sums /*[2*Din+2]*/, int32_t Din, float* delta, void* stream);
/* bgnn_linear_f32: out = relu?(x W^T + bias) for the first Linear (+ folded eval BatchNorm + ReLU) of
 *   KTGNN_no_complement.clf_transformer (models/KTGNN.py:407-411, applied at :433), on the same W-stationary MFMA kernel
 *   as the transform; colsum_opt ([2*Dout+2], zeroed by the caller, needs mask_opt) additionally receives the per-domain
 *   column sums + node counts of the OUTPUT, i.e. the domain sums (:275) of the conv that consumes it -- no extra pass.
 *   W [Dout, Din] is torch Linear.weight layout.  Envelope: Din <= 128, Din % 4 == 0, Dout % 64 == 0 (else
 *   BGNN_E_SHAPE; callers use a library GEMM outside it). */
int bgnn_linear_f32(const float* x, int64_t N, int32_t Din, int64_t ldx, const float* W, const float* bias,
                    int32_t Dout, int relu, const uint8_t* mask_opt, double* colsum_opt,
                    float* out, int64_t ldo, void* stream);
/* Fused pair for KTGNN_no_complement.forward :433 (clf_target on clf_transformer(h), eval): the activation
 *   a = relu?(x W^T + bias) of the transformer's first Linear (+ folded BatchNorm) never reaches HBM.
 *   bgnn_linear_narrow_transform_f32 (stage A) leaves raw[N][12] = (W_t a [4] | W_s a [4] | a.g_s2t | a.g_t2s | 0 | 0)
 *   for the consumer conv's packed operands Wp2 [8][Dout] (4 rows of W_t, 4 of W_s, zero padded: D <= 4) and gates2
 *   [2][2*Dout], and accumulates the per-domain column sums + counts of a into colsum [2*Dout+2] (caller zero-fills;
 *   multi-GPU callers all-reduce it).  bgnn_narrow_transform_finish_f32 (stage B) turns raw into the conv's h_s2t /
 *   h_t2s rows (4 floats each, row_stride apart) with bias and the rank-1 domain shift of :277-284.
 *   Envelope of stage A: Din <= 128, Din % 4 == 0, Dout in {64, 128, 256} (else BGNN_E_SHAPE: use bgnn_linear_f32 +
 *   the transform).  small_ws: 16 floats. */
int bgnn_linear_narrow_transform_f32(const float* x, int64_t N, int32_t Din, int64_t ldx, const float* W,
                                     const float* bias, int32_t Dout, int relu, const uint8_t* mask,
                                     double* colsum, const float* Wp2, const float* gates2, float* raw, void* stream);
/* The classifier stage's dense work in ONE pass over the hidden activation x = h (KTGNN.py:432-434; ABI 112): the narrow tables of
 * the `sk_heads` (1 or 2) convs that read h itself -- the transform of bgnn_adaptedconv_transform_f32 in its sums form with `sums_x` for the packed
 * operands sk_Wp / sk_bias / sk_gates (sk_heads * 2 * sk_ldh <= 24 packed columns) -- AND stage A of the fused pair above (W, bias,
 * Dout = 128, colsum, Wp2, gates2, raw).  Same results as the two separate launches; Din in (64, 128], Din % 4 == 0, else
 * BGNN_E_SHAPE.  small_ws: sk_heads * (2 * sk_ldh + 2) + 8 floats. */
int bgnn_classifier_stage_f32(const float* x, int64_t N, int32_t Din, int64_t ldx, const uint8_t* mask,
                              const double* sums_x, int32_t sk_heads, int32_t sk_D, const float* sk_Wp,
                              const float* sk_bias, const float* sk_gates, const float* sk_gate_const_opt,
                              float* h_s2t_0, float* h_t2s_0, float* h_s2t_1, float* h_t2s_1, int64_t sk_ldh,
                              int64_t sk_row_stride, const float* W, const float* bias, int32_t Dout, int relu,
                              double* colsum, const float* Wp2, const float* gates2, float* raw, float* small_ws,
                              void* stream);
int bgnn_narrow_transform_finish_f32(const float* raw, int64_t N, const uint8_t* mask, const double* sums,
                                     int32_t Din, const float* Wp2, const float* bias2, const float* gates2,
                                     const float* gate_const_opt, float* h_s2t, float* h_t2s, int64_t row_stride,
                                     float* small_ws, void* stream);
/* The eval classifier stage on 32-BYTE node rows (additive symbols, the revision stays 116).  At D <= 2 classes half of a
 * [3 heads][4 floats] table row is padding; these entries keep per node and table 8 floats [h0c0 h0c1 h1c0 h1c1 | h2c0 h2c1 0 0]
 * (D = 1: the c1 columns are 0 too), the same values as the padded rows bit for bit.
 *   bgnn_classifier_stage_rows32_f32: bgnn_classifier_stage_f32 for its two heads (sk_heads = 2, sk_ldh = 4, sk_D <= 2), each
 *     row's first 16 bytes as ONE store at t_* + row * sk_row_stride; small_ws: 28 floats.
 *   bgnn_narrow_transform_finish_rows32_f32: bgnn_narrow_transform_finish_f32 with the padding written as +0 -- called with
 *     h_* = table + 4 and row_stride = 8 it defines the second 16 bytes of every row.
 *   bgnn_adaptedconv_aggregate_heads_rows32_f32: the three-head walk (heads = 3, mode 0, no hub rows, no alpha; ep_relu 0 or 2)
 *     over such tables; `out` keeps [rows][3][4].  Bit-identical to bgnn_adaptedconv_aggregate_queued_f32 on the padded tables.
 *     Only inside the plan that bgnn_adaptedconv_aggregate_heads_rows32_plan answers with 1 -- D <= 2, 0 <= slope <= 1, at most
 *     2^24 table rows, both tables inside one window below 4 GB, BGNN_HEADS_FAST and BGNN_HEADS_ROWS32 not 0 -- else BGNN_E_SHAPE:
 *     no other kernel reads this layout, so a caller asks the plan BEFORE it chooses the tables' layout. */
int bgnn_classifier_stage_rows32_f32(const float* x, int64_t N, int32_t Din, int64_t ldx, const uint8_t* mask,
                                     const double* sums_x, int32_t sk_D, const float* sk_Wp, const float* sk_bias,
                                     const float* sk_gates, const float* sk_gate_const_opt, float* t_s2t, float* t_t2s,
                                     int64_t sk_row_stride, const float* W, const float* bias, int32_t Dout, int relu,
                                     double* colsum, const float* Wp2, const float* gates2, float* raw, float* small_ws,
                                     void* stream);
int bgnn_narrow_transform_finish_rows32_f32(const float* raw, int64_t N, const uint8_t* mask, const double* sums,
                                            int32_t Din, const float* Wp2, const float* bias2, const float* gates2,
                                            const float* gate_const_opt, float* h_s2t, float* h_t2s, int64_t row_stride,
                                            float* small_ws, void* stream);
int bgnn_adaptedconv_aggregate_heads_rows32_plan(const float* t_t2s, const float* t_s2t, int64_t table_rows, int64_t row_end,
                                                 int32_t D, float negative_slope);
int bgnn_adaptedconv_aggregate_heads_rows32_f32(const float* t_t2s, const float* t_s2t, const float* a_t2s, const float* a_s2t,
                                                const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                                int64_t row_begin, int64_t row_end, int32_t D, float negative_slope,
                                                float* out, int ep_relu, int64_t table_rows, void* stream);
/* bgnn_gram_f32: out[a][b] = sum_i A[i][a] * B[i][b] for tall-skinny A [N,p], B [N,q] (p <= 288, q <= 128, both % 4 == 0).
 *   The training path's weight / gate gradients of the dense transform (KTGNN.py:275-284 under autograd) are
 *   [G_s2t | G_t2s | dgate]^T . x with the node count as the reduction dimension; one streaming pass, deterministic
 *   two-stage sum.  ws: bgnn_gram_workspace_bytes(p, q).  N = 0: out is all zeros, A and B are not read and may be NULL. */
size_t bgnn_gram_workspace_bytes(int32_t p, int32_t q);
int bgnn_gram_f32(const float* A, int64_t lda, int32_t p, const float* B, int64_t ldb, int32_t q, int64_t N,
                  float* out /*[p][q]*/, void* ws, size_t ws_bytes, void* stream);
/* Training-mode BatchNorm1d -> ReLU -> dropout over node rows (models/KTGNN.py:420-430: `self.bns[ind](x)`, `F.relu`,
 *   `F.dropout(x, p=self.dropout, training=self.training)`; :364-367 clf_transformer's BatchNorm1d + ReLU with p = 0) in two
 *   streaming launches.  x [N, D] (D % 4 == 0, D <= 1024), batch statistics over the N rows in fp64 (`stats`, bgnn_bn_acc_doubles(D) doubles = R x [2*D] partials: column sums
 *   of x | x^2, written here and kept for the backward); y = keep(seed, element) ? max(gamma*(x-mean)/sqrt(var+eps)+beta, 0) / (1-p) : 0.
 *   The dropout mask is a counter-based hash of (seed, element index) with 16 bits per element (p is rounded to 1/65536) -- the
 *   same Bernoulli(1-p) law as torch's Philox stream, not the same bits.  running_mean / running_var (both or neither) get torch's
 *   momentum update with the unbiased variance.  `seed_dev_opt` (device, may be NULL): a 64-bit word added to `seed` by the kernels --
 *   a captured HIP graph bakes the host value of `seed` in, the device word (advanced by the caller once per step) keeps the masks of
 *   successive replays different; forward and backward of one step must see the same word.
 * bgnn_bn_relu_dropout_bwd_f32: dL/dx from dL/dy; the ReLU state is re-derived from x and the mask from (seed, index); `gsum`
 *   (bgnn_bn_acc_doubles(D) doubles = R x [2*D] partials, written here; summed over R) returns sum g' = dL/dbeta and sum g'.xhat = dL/dgamma (g' = dL/d(BN output)). */
int64_t bgnn_bn_acc_doubles(int32_t D);   /* size in doubles of `stats` / `gsum` below: R partial accumulators of [2*D]; their sum over R is the total */
int bgnn_bn_relu_dropout_f32(const float* x, int64_t N, int32_t D, int64_t ldx, const float* gamma_opt,
                             const float* beta_opt, float eps, int relu, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                             float momentum, float* running_mean_opt, float* running_var_opt,
                             float* y, int64_t ldy, double* stats, void* stream);
int bgnn_bn_relu_dropout_bwd_f32(const float* x, const float* grad_y, int64_t N, int32_t D, int64_t ldx, int64_t ldg,
                                 const double* stats, const float* gamma_opt, const float* beta_opt, float eps,
                                 int relu, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, float* grad_x, int64_t ldgx,
                                 double* gsum, void* stream);
/* The same BatchNorm1d -> ReLU -> dropout (models/KTGNN.py:420-430, :364-367) in four separately callable phases, for a node
 *   partition whose ranks put a collective between a reduction and its apply pass.  Same envelope and error codes as above;
 *   n_rows == 0 is valid (row pointers may then be NULL); nothing uses a memset node.
 * bgnn_bn_colstats_f32: this rank's fp64 column sums of x | x^2 into `acc` (bgnn_bn_acc_doubles(D) doubles = R x [2*D] partials,
 *   cleared here by a kernel; their sum over R is the rank's share; n_rows == 0 leaves zeros).
 * The *_rows entries take `totals` (plain [2*D] doubles: sum x | sum x^2 over the rows of ALL ranks) and `n_total`, the row count
 *   those sums run over (>= n_rows, >= 1): mean, variance and the unbiased factor of the running buffers use n_total.  The dropout
 *   counter of local row r is global_row * (D/4) + column group with global_row = row_ids_opt[r] (device int64 [n_rows]) or, when
 *   row_ids_opt is NULL, row_base + r -- the counter of bgnn_bn_relu_dropout_f32 on the whole activation, same `seed` /
 *   `seed_dev_opt` convention, so a rank's mask is its rows of the whole-graph mask.
 * bgnn_bn_apply_rows_f32: y rows; running_mean / running_var (both or neither) are updated on every call, also with n_rows == 0.
 * bgnn_bn_bwd_reduce_rows_f32: this rank's partial sum g' | sum g'.xhat into `gacc` (bgnn_bn_acc_doubles(D) doubles, as `acc`).
 * bgnn_bn_bwd_apply_rows_f32: dL/dx rows from `gtotals` (plain [2*D] doubles: that pair summed over all ranks) and n_total. */
int bgnn_bn_colstats_f32(const float* x, int64_t n_rows, int32_t D, int64_t ldx, double* acc, void* stream);
int bgnn_bn_apply_rows_f32(const float* x, int64_t n_rows, int32_t D, int64_t ldx, const double* totals, int64_t n_total,
                           const float* gamma_opt, const float* beta_opt, float eps, int relu, float p_drop, uint64_t seed,
                           const uint64_t* seed_dev_opt, const int64_t* row_ids_opt, int64_t row_base,
                           float momentum, float* running_mean_opt, float* running_var_opt,
                           float* y, int64_t ldy, void* stream);
int bgnn_bn_bwd_reduce_rows_f32(const float* x, const float* grad_y, int64_t n_rows, int32_t D, int64_t ldx, int64_t ldg,
                                const double* totals, int64_t n_total, const float* gamma_opt, const float* beta_opt,
                                float eps, int relu, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                const int64_t* row_ids_opt, int64_t row_base, double* gacc, void* stream);
int bgnn_bn_bwd_apply_rows_f32(const float* x, const float* grad_y, int64_t n_rows, int32_t D, int64_t ldx, int64_t ldg,
                               const double* totals, const double* gtotals, int64_t n_total, const float* gamma_opt,
                               const float* beta_opt, float eps, int relu, float p_drop, uint64_t seed,
                               const uint64_t* seed_dev_opt, const int64_t* row_ids_opt, int64_t row_base,
                               float* grad_x, int64_t ldgx, void* stream);
/* bgnn_transform_bwd_prep_f32: row-local part of the transform's hand-derived backward (KTGNN.py:275-284 under autograd) in
 *   one stream over x and the two incoming gradient tables: gate values (tanh of x.gx[g] + gconst[g]), the gates'
 *   adjoints G.(W delta) (wd [2][2D]: row 0 = -(W_t delta) in columns 0..D-1, row 1 = W_s delta in columns D..2D-1), and
 *   Gall[N][p] = [G_s2t[:, :D] | G_t2s[:, :D] | dpre_0 dpre_1 | +1/n_S or -1/n_T | 0] (p = pad4(2D+3); counts = the
 *   two node counts at the end of the domain sums), side[N][4] = (c1, c2, 1, 0): the operands of the Gram / linear
 *   launches that follow (column 2D+2 carries the gradient through the domain means as one more rank).  din % 4 == 0.
 *   ld_gall >= p / ld_side >= 4 are the row strides: two convs on the same x write side by side into one pair of buffers.
 *   ex_opt (D <= 128; ws: bgnn_transform_bwd_prep_workspace_bytes(N, p)): the entries of ex = Gall^T side that the backward uses
 *   (ex[c][0] = sum_i c1_i G_s2t[i][c], ex[D+c][1] = sum_i c2_i G_t2s[i][c], ex[.][2] = column sums of G_s2t | G_t2s | dpre; all
 *   other entries 0) from the same pass -- per-block partials summed in a fixed order, deterministic; side_opt may then be NULL. */
size_t bgnn_transform_bwd_prep_workspace_bytes(int64_t N, int32_t p);
int bgnn_transform_bwd_prep_f32(const float* x, int64_t ldx, int64_t N, int32_t din, const float* G_s2t, const float* G_t2s,
                                int64_t ldg, int32_t D, const uint8_t* mask, const float* gx /*[2][din]*/,
                                const float* gconst /*[2]*/, const float* wd /*[2][2D]*/, const double* counts /*[2]*/,
                                float* Gall, int32_t p, int64_t ld_gall, float* side_opt, int64_t ld_side,
                                float* ex_opt /*[p][4]*/, void* ws_opt, size_t ws_bytes, void* stream);
/* The O(D x Din) algebra around the streaming launches of the transform backward (KTGNN.py:275-284 under autograd), one launch
 *   each.  consts: gx [2][din] = the x-halves of the gate vectors g1 = a_g_s2t, g2 = a_g_t2s ([x || delta] order, 2*din each),
 *   gconst [2] = delta . (their delta-halves), wd [2][2D] as bgnn_transform_bwd_prep_f32 takes it.  finish: from dWall = Gall^T x
 *   [p][din] and ex [p][4]: dW_t = dWall[:D] - u1 (x) delta, dW_s = dWall[D:2D] + u2 (x) delta, dg_g = [dWall[2D+g] | sp_g delta],
 *   db_t / db_s = ex[:D,2] / ex[D:2D,2], and wcat_t [din][ld_wcat] = the TRANSPOSED operand (W_t | W_s | g1_x | g2_x | ddl | 0) of
 *   the input-gradient launch dX = Gall . Wcat (ddl = sp_0 g1_d + sp_1 g2_d - W_t^T u1 + W_s^T u2: through the domain means).
 *   W_s, W_t are [D][din] contiguous. */
int bgnn_transform_bwd_consts_f32(const float* W_s, const float* W_t, const float* g1, const float* g2, const float* delta,
                                  int32_t D, int32_t din, float* gx, float* gconst, float* wd, void* stream);
int bgnn_transform_bwd_finish_f32(const float* dWall, const float* ex, const float* W_s, const float* W_t, const float* g1,
                                  const float* g2, const float* delta, int32_t D, int32_t din, int32_t p, float* dW_s,
                                  float* dW_t, float* dg1, float* dg2, float* db_s_opt, float* db_t_opt, float* wcat_t,
                                  int64_t ld_wcat, void* stream);
/* bgnn_rowdot_f32: out[i][j] = X[i,:d] . V[j,:d], j < nv <= 4, d <= 256 (gate pre-activations and gate adjoints of the
 *   training path): one stream over X for all vectors. */
int bgnn_rowdot_f32(const float* X, int64_t ldx, int64_t N, int32_t d, const float* V, int64_t ldv, int32_t nv,
                    float* out /*[N][nv]*/, void* stream);
/* The transform of (a11) above.  Exactly one of delta_opt / sums_opt is non-NULL (both or neither: BGNN_E_NULL):
 *   delta_opt  [Din] floats, 16-byte aligned: the domain-mean difference of bgnn_domain_delta_f32;
 *   sums_opt   [2*Din+2] doubles (after any all-reduce): the tiny W.delta kernel forms delta with the arithmetic of
 *              bgnn_domain_delta_f32 (bit-identical), one launch less per conv.
 * n_tail_t2s / n_tail_s2t: the LAST n_tail_t2s + n_tail_s2t of the N rows (in that order) are rows whose consumer reads
 *   only h_t2s / only h_s2t -- the resident input halo of a partitioned graph (dist.py): for them the other table MAY be
 *   left unwritten (single-table launches inside the W-stationary kernel's envelope, both tables outside it).
 * tile_need_opt: NULL, or one int32 per 32-row tile of x, bit 0 set = some row of the tile has its h_s2t row read by the
 *   aggregation, bit 1 = its h_t2s row (a node's h_t2s row is gathered only by source-domain destinations and as the node's own
 *   row if it is one, KTGNN.py:292-295; with s -> t bridge edges no target node feeds a source destination and half of the h_t2s
 *   table is dead).  Rows of a table that no tile needs MAY be left unwritten.  Only the stream kernel (one head, 128 / 256 packed
 *   columns, 64 < Din <= 128) honours the mask; other shapes write both tables.  Tail groups OR a need mask, not both
 *   (BGNN_E_SHAPE).
 * team_runs_host_opt: NULL, or n_team_runs <= 2 triples (first tile, one past the last tile, table) of int64 in HOST memory,
 *   read during the call: runs of 32-row tiles in which EVERY tile needs the one table `table` (0 = h_s2t, 1 = h_t2s) -- by
 *   tile_need_opt (value 1 << table) or by lying inside that table's tail group.  The caller vouches for that; it decides the runs
 *   once per graph.  Inside a run the stream kernel's two 4-wave teams both hold the needed table's columns and take a block's
 *   tiles in turn (csrc/bgnn_transform_stream.hip).  Outputs are bit for bit those of a call without runs.  A run that gives some
 *   block of the launch fewer than 4 tiles, or a shape the stream kernel does not take at 256 packed columns, is ignored; so are
 *   all runs with BGNN_TS_TEAMS=0 in the environment (read once). */
int bgnn_adaptedconv_transform_f32(const float* x, int64_t N, int32_t Din, int64_t ldx,
                                   const uint8_t* mask, const float* delta_opt, const double* sums_opt,
                                   int32_t n_heads, int32_t D, const float* Wp, const float* bias_p,
                                   const float* gates, const float* gate_const_opt,
                                   float* h_s2t_0, float* h_t2s_0, float* h_s2t_1, float* h_t2s_1,
                                   int64_t ldh, int64_t row_stride, int64_t n_tail_t2s, int64_t n_tail_s2t,
                                   const int32_t* tile_need_opt, const int64_t* team_runs_host_opt, int32_t n_team_runs,
                                   float* small_ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a11-a13) fused GATv2 logits + per-destination softmax + weighted neighbour sum.
 *                      models/KTGNN.py:292-305, message :317-319, PyG softmax (call site :299),
 *                      MessagePassing.propagate(aggr='add') (call sites :303-304)
 * For destination row i (row_begin <= i < row_end; rowptr/mask/out/H are indexed by the absolute
 * row so a caller can aggregate interior rows while a halo exchange for the boundary rows is in
 * flight): H = mask[i] ? h_t2s : h_s2t, a = mask[i] ? a_t2s : a_s2t,
 *   e_j = a . leaky_relu(H[col_j] + H[i], slope);  alpha = softmax_j(e_j) (+1e-16 in the
 *   denominator);  out[i] = sum_j alpha_j H[col_j].
 * One pass over the in-neighbours with an online softmax: every H row is read once per edge.
 * Feature tables may have more rows than row_end (multi-GPU: local rows then halo rows).
 * Optional fused node-wise epilogue of KTGNN_no_complement.forward (:425-430, eval mode):
 *   out = relu?(out * ep_scale[c] + ep_shift[c])  (BatchNorm1d eval affine; NULL = identity); ep_relu: 0 none, 1 ReLU,
 *   2 = log_softmax over the D classes of every head (:435; interleaved narrow heads only: heads in {2,3}, D <= 4,
 *   ldh == ldo == 4; like ReLU it applies when a row is finished, i.e. not in part = 1).
 * alpha_opt ([E'] in CSR order) is optional (tests / backward).
 * Two-part rows (multi-GPU overlap): part = 1 visits a row's first edge list and parks the online-softmax state
 * ((max, sum) in state_ms_opt [rows][2], the raw accumulator in out); part = 2 resumes from it over a second
 * edge list (another rowptr/col pair) and finishes the row.  part = 0 is the ordinary single launch; part = 3 (narrow
 * interleaved heads only) is a single launch that also leaves the finished rows' (max, sum) in state_ms_opt [rows][heads][2]
 * for bgnn_adaptedconv_aggregate_heads_bwd_f32.  In part = 1 the
 * rows [row_begin, park_begin) have no second part and are finished right away (epilogue, colsum), rows
 * [park_begin, row_end) are parked: one launch serves a rank's interior and boundary rows (park_begin = row_begin
 * parks every row).
 * heads > 1 evaluates several convs that share the graph in ONE pass (KTGNN.py:432-434: clf_base / clf_target /
 * clf_target-hat): their tables are interleaved row-wise ([rows, heads*ldh], head h of node r at (r*heads+h)*ldh),
 * a_t2s / a_s2t are [heads][D], out is [rows, heads*ldo] likewise; the in-neighbour ids are read once for all heads.
 * colsum_opt ([2*ldo+2] doubles, accumulated: caller zero-fills) receives the per-domain column sums and node
 * counts of the finished rows -- the `bgnn_domain_sums_f64` of the NEXT conv's input for free (heads == 1 only).
 * tile_queue_opt (8 x uint32 scratch, zeroed here on `stream`) switches the persistent blocks from static tile
 * striding to per-XCD dynamic tile counters (keeps the rows in flight inside the XCD's L2).
 * D <= 256; ldh % 4 == 0, ldo % 4 == 0, 16-B aligned tables; pad columns must be zero.        */
int bgnn_adaptedconv_aggregate_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                   const float* a_t2s, const float* a_s2t,
                                   const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                   int64_t row_begin, int64_t row_end, int32_t D, float negative_slope,
                                   float* out, int64_t ldo, float* alpha_opt,
                                   const float* ep_scale_opt, const float* ep_shift_opt, int ep_relu,
                                   float* state_ms_opt, int part, int64_t park_begin, int32_t heads, double* colsum_opt,
                                   uint32_t* tile_queue_opt, void* stream);

/* bgnn_adaptedconv_aggregate_f32 with one more promise from the caller (ABI 113): both tables have `table_rows` rows and every id in
 * `col` is below it (table_rows >= row_end, else BGNN_E_SHAPE).  Results are bit-identical; the promise lets the plain wide launch
 * (heads = 1, part = 0, no alpha, D > 32) address neighbour rows by 32-bit offsets inside one window that holds both tables, when
 * that window is below 4 GB and table_rows <= 2^24 (agg_wide_fast_kernel: C4 hidden conv 1.06 -> see DESIGN 4.1); every other
 * shape runs exactly what bgnn_adaptedconv_aggregate_f32 runs.  Ids >= table_rows read outside the tables (undefined), as they
 * do there.  gather_hint: 0 = unknown, 1 = neighbouring destination rows share neighbours (the gathers live off the L2s), 2 = no
 * neighbour reuse (HBM-bound gathers): only chooses how many blocks of the fast kernel stay resident per CU (results unchanged;
 * DstCSR.gather_hint() measures it once per graph).  BGNN_AGG_FAST=0 in the environment keeps the general kernel. */
int bgnn_adaptedconv_aggregate_bounded_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                           const float* a_t2s, const float* a_s2t,
                                           const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                           int64_t row_begin, int64_t row_end, int32_t D, float negative_slope,
                                           float* out, int64_t ldo, float* alpha_opt,
                                           const float* ep_scale_opt, const float* ep_shift_opt, int ep_relu,
                                           float* state_ms_opt, int part, int64_t park_begin, int32_t heads, double* colsum_opt,
                                           uint32_t* tile_queue_opt, int64_t table_rows, int32_t gather_hint, void* stream);

/* bgnn_adaptedconv_aggregate_bounded_f32 with a tile queue of a stated size: tile_queue_opt holds tile_queue_words uint32 (>= 8, else
 * BGNN_E_WORKSPACE; zeroed here on `stream`, as far as the launch uses it).  With bgnn_aggregate_tile_queue_words() words or more the
 * plain wide launch (agg_wide_fast_kernel) claims SINGLE tiles from striped counters, 8 * NQ of them a cache line apart,
 * instead of chunks of four from the 8 counters every other kernel and entry uses; a smaller queue gets those chunk claims, and no
 * entry writes past the words it was given.  Results are bit-identical either way (column sums: fp32 partials in claim order).
 * Environment (read once): BGNN_AGG_CLAIM=chunk | tile, BGNN_AGG_SUBQUEUES = NQ (1..8, default 4),
 * BGNN_AGG_CLAIM_AHEAD=0 (the claim waited for where it is issued); bgnn_aggregate_tile_queue_words() follows them (8 under BGNN_AGG_CLAIM=chunk).  An additive pair:
 * bgnn_adaptedconv_aggregate_f32, _bounded_f32 and _hub_f32 keep their 8-word contract and their schedule. */
int64_t bgnn_aggregate_tile_queue_words(void);
int bgnn_adaptedconv_aggregate_queued_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                          const float* a_t2s, const float* a_s2t,
                                          const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                          int64_t row_begin, int64_t row_end, int32_t D, float negative_slope,
                                          float* out, int64_t ldo, float* alpha_opt,
                                          const float* ep_scale_opt, const float* ep_shift_opt, int ep_relu,
                                          float* state_ms_opt, int part, int64_t park_begin, int32_t heads, double* colsum_opt,
                                          uint32_t* tile_queue_opt, int64_t tile_queue_words, int64_t table_rows, int32_t gather_hint,
                                          void* stream);

/* The same aggregation for graphs with HUB rows.  A destination row is walked by one lane group, so a row with hundreds of
 * in-edges (the 581 source nodes of the Twitter_Graph stand-in have ~750) is a chain of dependent gather steps that outlives
 * all other rows.  Rows with >= hub_threshold in-edges (hub_rows [n_hubs], ascending) are skipped by the main launch, walked as
 * segments -- seg_bounds [2 n_segments] = (begin, end) offsets into `col`, seg_node [n_segments] = the segment's row,
 * hub_seg_ptr [n_hubs + 1] = the segments of each hub -- whose online-softmax states are parked like two-part rows, and finished
 * by a merge launch (normalise, epilogue, colsum; part-3 state for the heads backward when state_ms_opt is given; alpha_opt [E'],
 * heads = 1: the attention coefficients in CSR order for the backward).  All N rows,
 * wide rows (D > 32, heads = 1) or interleaved narrow heads (heads = 2 | 3, ldh = ldo = 4); other shapes: BGNN_E_SHAPE (use
 * bgnn_adaptedconv_aggregate_f32).  n_hubs = 0 is the plain launch.  ws: bgnn_aggregate_hub_workspace_bytes(n_segments, heads, ldo). */
size_t bgnn_aggregate_hub_workspace_bytes(int64_t n_segments, int32_t heads, int64_t ldo);
int bgnn_adaptedconv_aggregate_hub_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                       const float* a_t2s, const float* a_s2t,
                                       const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                       int64_t N, int32_t D, float negative_slope, float* out, int64_t ldo,
                                       const float* ep_scale_opt, const float* ep_shift_opt, int ep_relu,
                                       float* state_ms_opt, int32_t heads, double* colsum_opt,
                                       uint32_t* tile_queue_opt, int32_t hub_threshold, const int32_t* hub_rows,
                                       int64_t n_hubs, const int32_t* hub_seg_ptr, const int32_t* seg_bounds,
                                       const int32_t* seg_node, int64_t n_segments, float* alpha_opt,
                                       void* ws, size_t ws_bytes, void* stream);

/*  backward of the aggregation above -- what autograd computes through
 * models/KTGNN.py:292-305 when main_graph_knowledge_transfer.py:39-68 calls loss.backward().
 * Inputs: the forward's tables, `out`, `alpha` (CSR order) and grad_out = dL/dout.  Outputs are
 * ACCUMULATED into (caller zero-fills): dh_t2s / dh_s2t [rows of the tables, ldh] and da_t2s / da_s2t [D].
 * Source-side sums use hardware fp32 atomics (order-dependent in the last bits).               */
int bgnn_adaptedconv_aggregate_bwd_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                       const float* a_t2s, const float* a_s2t,
                                       const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                       int64_t row_begin, int64_t row_end, int32_t D, float negative_slope,
                                       const float* out, int64_t ldo, const float* alpha,
                                       const float* grad_out, int64_t ldg,
                                       float* dh_t2s, float* dh_s2t, float* da_t2s, float* da_s2t,
                                       void* stream);

/* Atomic-free ("pull") form of the same backward, 1 <= D <= 256 (ABI 114: one entry for every width, with or without hub rows): the
 * source-side sums are gathered over a by-source view of the edges (t_rowptr [N+1]; t_eid [E'] = position of the edge in the
 * by-destination order; t_dst [E'] = its destination) instead of scattered with float atomics; every dH row is written exactly once
 * (no zero-fill needed, deterministic; pad columns D <= c < ldh are written 0 for D > 128).  All N rows are visited.  ldh / ldo / ldg
 * are multiples of 4 and at least D, else BGNN_E_SHAPE.
 * Hub rows: pass A walks destinations, pass B sources: a destination with >= hub_threshold in-edges / a source with that many
 * out-edges is skipped as a row and walked as segments -- d_* tables over `rowptr` / `col`, s_* tables over the by-source arrays,
 * both in the layout of bgnn_adaptedconv_aggregate_hub_f32 (hub_rows, hub_seg_ptr, seg_bounds = (begin, end) pairs, seg_node) --
 * that ride behind the real rows of the same launch and leave partial row sums, merged in a fixed order.  d_n_hubs = s_n_hubs = 0
 * (tables may then be NULL, hub_threshold is not looked at): no hub rows.  The narrow form (D <= 4 with ldh = ldo = ldg = 4)
 * knows no segments: BGNN_E_SHAPE with hub tables.
 * da: for D <= 128 da_t2s / da_s2t are ACCUMULATED into with float atomics (caller zero-fills; N == 0 leaves them untouched); for
 * D > 128 (a whole wave per row) they are WRITTEN whole, from partial rows summed in a fixed order, so all four outputs of a call
 * are bitwise reproducible (N == 0 writes zeros).  For D > 128 pad columns of the tables must hold finite values.
 * ws: bgnn_aggregate_bwd_pull_workspace_bytes(N, E', ldh, D, d_n_segments, s_n_segments) -- a record per edge (32 bytes, 64 for
 * D > 128), the dstside table, for D > 128 the da partial rows, the hub segments' partial rows; the entry returns
 * BGNN_E_WORKSPACE exactly when ws_bytes is below that figure. */
size_t bgnn_aggregate_bwd_pull_workspace_bytes(int64_t N, int64_t E, int64_t ldh, int32_t D, int64_t d_segments, int64_t s_segments);
int bgnn_adaptedconv_aggregate_bwd_pull_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                            const float* a_t2s, const float* a_s2t,
                                            const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                            const int32_t* t_rowptr, const int32_t* t_eid, const int32_t* t_dst,
                                            int64_t N, int64_t E, int32_t D, float negative_slope,
                                            const float* out, int64_t ldo, const float* alpha,
                                            const float* grad_out, int64_t ldg,
                                            float* dh_t2s, float* dh_s2t, float* da_t2s, float* da_s2t,
                                            int32_t hub_threshold,
                                            const int32_t* d_hub_rows, int64_t d_n_hubs, const int32_t* d_hub_seg_ptr,
                                            const int32_t* d_seg_bounds, const int32_t* d_seg_node, int64_t d_n_segments,
                                            const int32_t* s_hub_rows, int64_t s_n_hubs, const int32_t* s_hub_seg_ptr,
                                            const int32_t* s_seg_bounds, const int32_t* s_seg_node, int64_t s_n_segments,
                                            void* ws, size_t ws_bytes, void* stream);

/* Pull-form backward for `heads` (2 or 3) interleaved narrow convs evaluated together (KT-GNN's classifier stage under
 * autograd: clf_base(x), clf_target(x), clf_target(T(x)), KTGNN.py:432-435, share the graph): tables / out / grad_out / dH are
 * [N][heads][4], a_* and da_* [heads][D] (da accumulated: caller zero-fills), D <= 4.  `state_ms` [N][heads][2] is the finished
 * rows' softmax state (max, sum) that bgnn_adaptedconv_aggregate_f32 leaves with part = 3; alpha is rebuilt from it, no per-edge
 * array is kept by the forward.  log_softmax != 0: `out` holds the fused log-probabilities (ep_relu = 2) and grad_out is
 * dL/dlogp -- the row-local adjoint is applied first.  Every dH row is written exactly once (deterministic).
 * Hub tables and the zero-hubs rule as in bgnn_adaptedconv_aggregate_bwd_pull_f32 (partial rows of heads * 4 floats).
 * ws: bgnn_aggregate_heads_bwd_workspace_bytes(N, E', heads, d_n_segments, s_n_segments), refused exactly below that figure. */
size_t bgnn_aggregate_heads_bwd_workspace_bytes(int64_t N, int64_t E, int32_t heads, int64_t d_segments, int64_t s_segments);
int bgnn_adaptedconv_aggregate_heads_bwd_f32(const float* h_t2s, const float* h_s2t, const float* a_t2s, const float* a_s2t,
                                             const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                             const int32_t* t_rowptr, const int32_t* t_dst,
                                             int64_t N, int64_t E, int32_t D, int32_t heads, float negative_slope,
                                             const float* out, const float* state_ms, const float* grad_out,
                                             int log_softmax, float* dh_t2s, float* dh_s2t, float* da_t2s, float* da_s2t,
                                             int32_t hub_threshold,
                                             const int32_t* d_hub_rows, int64_t d_n_hubs, const int32_t* d_hub_seg_ptr,
                                             const int32_t* d_seg_bounds, const int32_t* d_seg_node, int64_t d_n_segments,
                                             const int32_t* s_hub_rows, int64_t s_n_hubs, const int32_t* s_hub_seg_ptr,
                                             const int32_t* s_seg_bounds, const int32_t* s_seg_node, int64_t s_n_segments,
                                             void* ws, size_t ws_bytes, void* stream);

/* The classifier stage's three-head walk for WIDE classes (KT-GNN trained on office, 31 classes; ABI 113, additive): `heads`
 * (2 or 3) interleaved convs, 4 < D <= 32, tables / out [N][heads][ldh] with ldh = pad4(D), a_* [heads][D].  One CSR walk for all
 * heads (each in-neighbour id read once), per head the GATv2 logit, an online softmax (alpha = p / (s + 1e-16)), the weighted sum
 * and the log_softmax over the D classes (KTGNN.py:435); pad columns of `out` are written 0.  `state_ms` [N][heads][2] receives
 * each row's (max, sum) for the backward; nothing per edge is written.  A row with no in-edges gives log_softmax(0) = -log D.
 * Outside the envelope (D <= 4, D > 32, heads not 2 | 3, ldh != pad4(D)): BGNN_E_SHAPE.  No workspace. */
int bgnn_adaptedconv_aggregate_heads_wide_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                              const float* a_t2s, const float* a_s2t,
                                              const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                              int64_t N, int32_t D, int32_t heads, float negative_slope,
                                              float* out, float* state_ms, void* stream);
/* Its pull-form backward (grad_out = dL/dlogp, [N][heads][ldh]): the row-local log_softmax adjoint first, alpha rebuilt from
 * state_ms; pass A over destinations, pass B over sources (the by-source view t_rowptr / t_dst).  Every dH row (pad columns 0) is
 * written exactly once; da_* [heads][D] are written (not accumulated) from per-block partial sums added in a fixed order, so two
 * identical calls are bitwise equal (N = 0: da_* are written as zeros).  Same envelope.  ws: bgnn_aggregate_heads_wide_bwd_workspace_bytes(N, heads, ldh). */
size_t bgnn_aggregate_heads_wide_bwd_workspace_bytes(int64_t N, int32_t heads, int64_t ldh);
int bgnn_adaptedconv_aggregate_heads_wide_bwd_f32(const float* h_t2s, const float* h_s2t, int64_t ldh,
                                                  const float* a_t2s, const float* a_s2t,
                                                  const int32_t* rowptr, const int32_t* col, const uint8_t* mask,
                                                  const int32_t* t_rowptr, const int32_t* t_dst,
                                                  int64_t N, int32_t D, int32_t heads, float negative_slope,
                                                  const float* out, const float* state_ms, const float* grad_out,
                                                  float* dh_t2s, float* dh_s2t, float* da_t2s, float* da_s2t,
                                                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * GraphSAGE mean aggregation (the --no_dtc model of main_graph_knowledge_transfer.py:326,:414-417):
 *     models/backbones.py:440-498 -- torch_sparse matmul(adj_t, x, reduce='mean') inside each SAGEConv (PyG sage_conv),
 *     F.relu + F.dropout(p=0.5) between convs (:467-469) and F.log_softmax (:471).
 * The caller transforms first (T = x [W_l ; W_r]^T + [0 ; b_l]) and aggregates rows of the output width D:
 *   out[i] = epi( s_i * sum_{t in [rowptr[i], rowptr[i+1])} tbl[col[t]] + root[i] ),  s_i = 1/deg_i if `mean` else 1,
 * a row without edges gives epi(root[i]); root_opt NULL adds nothing, ldr == 0 broadcasts one row.  Duplicate edges count with
 * their multiplicity, self loops as given.  A by-destination CSR (rowptr [n_rows+1], col = sources) averages in-neighbours (forward);
 * the by-source view (t_rowptr, t_dst) averages out-neighbours (get_emb / get_logits, :473-498).  ids in col must be < n_tbl.
 * epilogue: 0 none; 1 ReLU, then dropout with keep probability 1-p_drop (mask = the counter-based hash of bgnn_bn_relu_dropout_f32
 * over element index row * D + column, same seed / seed_dev_opt semantics; p_drop > 0 only with epilogue 1); 2 row log_softmax
 * (D <= 128).  Strides ldt / ldr / ldo are in floats, % 4 == 0 and >= pad4(D); pointers 16-B aligned; pad columns of out are
 * written as 0.  D > 128 runs as 128-column slices.
 * row_id_opt [n_rows] (int64), for a block of rows of a larger graph (a rank's rows of a destination-node partition): every output
 * row's GLOBAL row id; the dropout element index is then row_id[i] * D + column, so a rank draws exactly the masks of the
 * whole-graph call.  NULL (or no dropout): row i; the plain kernels run.
 * bgnn_sage_mean_aggregate_bwd_f32: the atomic-free backward of the same call (mean = 1, root present) -- from the forward's output
 * y and grad_y: g = grad_y (epilogue 0), (y > 0 ? grad_y / (1 - p_drop) : 0) (epilogue 1), grad_y - exp(y) * rowsum(grad_y)
 * (epilogue 2); grad_root[i] = g[i] (n_rows rows) and grad_tbl[j] = sum over the out-edges (j -> i) of g[i] / deg_i, walked over
 * the by-source view (t_rowptr [n_src+1], t_col = destinations) in n_src rows.  Deterministic bits.
 * ws: bgnn_sage_mean_aggregate_bwd_workspace_bytes(n_rows, D). */
int bgnn_sage_mean_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* root_opt, int64_t ldr,
                                 const int32_t* rowptr, const int32_t* col, int64_t n_rows, int32_t D, int mean,
                                 int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                                 const int64_t* row_id_opt, float* out, int64_t ldo, void* stream);
size_t bgnn_sage_mean_aggregate_bwd_workspace_bytes(int64_t n_rows, int32_t D);
int bgnn_sage_mean_aggregate_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy,
                                     const int32_t* rowptr, int64_t n_rows, const int32_t* t_rowptr, const int32_t* t_col,
                                     int64_t n_src, int32_t D, int epilogue, float p_drop,
                                     float* grad_tbl, int64_t ldgt, float* grad_root, int64_t ldgr,
                                     void* ws, size_t ws_bytes, void* stream);
/* bgnn_rows_segment_add_f32: for a CSR of segments (seg_ptr [n_seg+1], idx = rows of src < n_src, row [n_seg]),
 *     dst[row[s]] = (accumulate ? dst[row[s]] : 0) + sum_{k in [seg_ptr[s], seg_ptr[s+1])} src[idx[k]]
 * over D columns (pad columns up to pad4(D) written as 0).  The row ids must be distinct; an id outside [0, n_dst) is skipped
 * (its segment is never written).  No atomics: one lane group
 * owns a segment and sums it in a fixed order, so the result is bit-identical from run to run.  Empty segments give dst[row[s]]
 * (accumulate) or 0.  lds / ldd in floats, % 4 == 0 and >= pad4(D); src / dst 16-B aligned.  This is how the owner of a row
 * folds the gradient rows that come back from the reverse halo exchange (a row sent to k ranks gets k rows back). */
int bgnn_rows_segment_add_f32(const float* src, int64_t lds, int64_t n_src, const int32_t* seg_ptr, const int32_t* idx,
                              const int32_t* row, int64_t n_seg, int32_t D, int accumulate, float* dst, int64_t ldd, int64_t n_dst,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * GCN normalised aggregation (the `gnn='GCN'` baseline of main_graph_knowledge_transfer.py:302):
 *     models/backbones.py:246-300 -- PyG GCNConv: gcn_norm(add_self_loops=True, improved=False) with unit edge weights,
 *     propagate(aggr='add'), + bias; F.relu + F.dropout(p=0.5) between convs (:274-275) and F.log_softmax (:277).
 * The caller transforms first (tbl = x W^T, width D = the conv's output width) and hands a by-destination CSR that already
 * holds exactly one self loop per row (bgnn_build_dst_csr with rewrite_self_loops: add_remaining_self_loops leaves one loop of
 * weight 1 per node however many the input had; duplicate non-loop edges count with their multiplicity, in the sum and in deg):
 *   dinv[i] = 1 / sqrt(rowptr[i+1] - rowptr[i])
 *   out[i]  = epi( dinv[i] * sum_{t in [rowptr[i], rowptr[i+1])} dinv[col[t]] * tbl[col[t]] + bias )
 * dinv [n_dinv >= max(n_rows, n_tbl)] is built once per graph by the caller and gathered per edge.  bias_opt: one row of D
 * floats (16-B aligned) or NULL.  Epilogues, strides, padding, alignment and the dropout hash are those of
 * bgnn_sage_mean_aggregate_f32 (0 none; 1 ReLU then dropout over element index row * D + column with seed / seed_dev_opt;
 * 2 row log_softmax at D <= 128).  D > 128 runs as 128-column slices (epilogue 2 then returns BGNN_E_SHAPE).
 * Hub rows: with n_hubs > 0 the rows listed in hub_rows (exactly the rows of at least hub_threshold edges) are cut into n_seg
 * segments -- hub_seg_ptr [n_hubs+1] indexes a hub's segments, seg_bounds [2 n_seg] holds each segment's (begin, end) offsets
 * into col (`DstCSR.hub_tables`).  One lane group sums a segment into a partial row of ws
 * (bgnn_gcn_aggregate_workspace_bytes(n_seg, D)), then one group per hub adds its partial rows in segment order and applies
 * scale, bias and epilogue: three launches instead of one, and no row is walked by a single group.  n_hubs == 0: one launch.
 * row_id_opt [n_rows] (int64), for a block of rows of a larger graph (a rank's rows of a destination-node partition; tbl and dinv
 * then cover the rank's own rows followed by its halo rows): every output row's GLOBAL row id; the dropout element index is then
 * row_id[i] * D + column, so a rank draws exactly the masks of the whole-graph call -- in the one-launch row kernel, in the finish
 * pass of a hub row (row_id[hub_rows[h]]) and in every 128-column slice at D > 128.  NULL (or no dropout): row i; the plain kernels
 * run.
 * bgnn_gcn_aggregate_bwd_f32: the atomic-free backward.  A row pass writes g [n_rows, ldg] from the forward's output y and
 * grad_y (g = grad_y; (y > 0 ? grad_y / (1 - p_drop) : 0); grad_y - exp(y) * rowsum(grad_y)); the caller takes grad_bias as the
 * column sums of g.  By symmetry of the normalisation grad_tbl[j] = dinv[j] * sum_{i : j -> i} dinv[i] * g[i]: the forward
 * walk without bias or epilogue over the by-source view (t_rowptr [n_src+1], t_col = destinations, self loops included; the
 * hub tables are those of that view).  It takes no ids: the mask is recovered from y > 0, and n_rows (rows of g) and n_src (rows
 * of grad_tbl) are counted separately.  Deterministic bits. */
size_t bgnn_gcn_aggregate_workspace_bytes(int64_t n_seg, int32_t D);
int bgnn_gcn_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* bias_opt, const int32_t* rowptr,
                           const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows, int32_t D,
                           int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                           int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                           const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                           void* ws_opt, size_t ws_bytes, const int64_t* row_id_opt, float* out, int64_t ldo, void* stream);
int bgnn_gcn_aggregate_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, int64_t n_rows,
                               const int32_t* t_rowptr, const int32_t* t_col, const float* dinv, int64_t n_dinv,
                               int64_t n_src, int32_t D, int epilogue, float p_drop,
                               int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                               const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                               void* ws_opt, size_t ws_bytes, float* g, int64_t ldg, float* grad_tbl, int64_t ldgt,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * APPNP propagation (the APPNP_Net baseline, models/backbones.py:110-128: an MLP followed by PyG `APPNP(K=10, alpha=0.1)`,
 * then F.log_softmax): K personalised-PageRank steps over the GCN-normalised graph at class width,
 *     z_0 = h,   z_{k+1} = (1 - alpha) * A^ z_k + alpha * h   (k = 0 .. K-1),   out = epi(z_K),
 * A^ = D^-1/2 (A' + I) D^-1/2 over the CSR of bgnn_gcn_aggregate_f32 (exactly one self loop per row, dinv[i] = 1/sqrt(deg_i)).
 * The graph is square: rowptr [n_rows+1], every id in col < n_rows, h and out have n_rows rows, dinv [n_dinv >= n_rows].
 * One launch per step on `stream` (three with hub tables), ordered by launch order alone; nothing is allocated and the host
 * never waits, so a captured graph records the launches.  Between steps the state is kept pre-scaled, s_k = dinv * z_k, in two
 * [n_rows, pad4(D)] buffers of the workspace that alternate: a step gathers s_k[col[t]] only (the first one reads h and
 * gathers dinv[col[t]] next to it), forms (1 - alpha) * dinv[i] * sum + alpha * h[i] and stores dinv[i] times that; the last
 * step stores the value itself, or its row log_softmax.  1 <= D <= 128 (else BGNN_E_SHAPE), K >= 0 (K == 0: out = epi(h)),
 * 0 <= alpha <= 1 (alpha == 1: out == h bit for bit), epilogue 0 (none) or 2 (row log_softmax).  ld_h / ld_out in floats,
 * % 4 == 0 and >= pad4(D), h / out 16-B aligned and distinct; pad columns of out are written as 0.
 * Hub rows: the argument group and the scheme of bgnn_gcn_aggregate_f32 -- the row kernel skips them, one lane group sums
 * a segment into a partial row of the workspace, one group per hub adds its partial rows in segment order and applies the
 * step's scaling, teleport term, store and epilogue.  No float atomics: bit-identical from run to run.
 * ws: bgnn_appnp_propagate_workspace_bytes(n_rows, D, n_seg) bytes (two state buffers + n_seg partial rows; may be NULL when
 * K <= 1 and n_hubs == 0).
 * The operator is linear in h and A^ is symmetric in its dinv products, so the gradient of z_K with respect to h is the SAME
 * call on the by-source view (t_rowptr, t_dst and that view's hub tables) applied to the gradient at z_K, epilogue 0: there
 * is no _bwd entry.  Under epilogue 2 the caller first forms g = dy - exp(y) * rowsum(dy):
 * bgnn_appnp_log_softmax_bwd_f32 (models/backbones.py:110-128, the backward of :128's F.log_softmax) is the convs' backward
 * row pass under its log_softmax rule, y = the forward's output; g is written once and read by every step as the teleport
 * term.  Leading dimensions and alignment as above, D <= 128; pad columns of g are written as 0. */
size_t bgnn_appnp_propagate_workspace_bytes(int64_t n_rows, int32_t D, int64_t n_seg);
int bgnn_appnp_propagate_f32(const float* h, int64_t ld_h, const int32_t* rowptr, const int32_t* col, const float* dinv,
                             int64_t n_dinv, int64_t n_rows, int32_t D, int32_t K, float alpha, int epilogue,
                             int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                             const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                             void* ws_opt, size_t ws_bytes, float* out, int64_t ld_out, void* stream);
int bgnn_appnp_log_softmax_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, int64_t n_rows, int32_t D,
                                   float* g, int64_t ldg, void* stream);
/* Feature dropout of APPNP_Net (models/backbones.py:110-128: F.dropout(x, 0.5) on the input, F.relu + F.dropout(0.5) on the
 * hidden activation) over a contiguous [n_rows, D] activation of any width, x and y 16-B aligned (y may be x):
 *     y = drop(act(x + bias)),  act = ReLU when relu != 0,  bias_opt [D] or NULL,
 * element e = row * D + column kept when the 16 bits of the shared (seed + *seed_dev_opt, e) hash reach round(p_drop * 65536),
 * kept values scaled by the reciprocal of the quantised keep probability (the contract of bgnn_bn_relu_dropout_f32);
 * 0 <= p_drop < 1.
 * bgnn_feature_dropout_bwd_f32 (models/backbones.py:110-128, the backward of the same two sites):
 * grad_x = grad_y * keep / (1 - p) * [act'], the mask read off y > 0 under ReLU (y required) and redrawn from the seed
 * otherwise (y_opt unused). */
int bgnn_feature_dropout_f32(const float* x, const float* bias_opt, int64_t n_rows, int32_t D, int relu, float p_drop,
                             uint64_t seed, const uint64_t* seed_dev_opt, float* y, void* stream);
int bgnn_feature_dropout_bwd_f32(const float* y_opt, const float* grad_y, int64_t n_rows, int32_t D, int relu, float p_drop,
                                 uint64_t seed, const uint64_t* seed_dev_opt, float* grad_x, void* stream);
/* One step of the APPNP propagation over a RECTANGULAR graph (APPNP_Net, models/backbones.py:110-128, on a destination-node
 * partition: the caller exchanges halo rows between steps, which the K-step entry cannot do):
 *     out[i] = store((1 - alpha) * dinv[i] * sum_{t in row i} w_t * tbl[col[t]] + alpha * h[i]),   i < n_rows,
 * rowptr [n_rows+1] and h / out with n_rows rows (a rank's owned rows), tbl with n_tbl >= n_rows rows (the owned rows, then the
 * halo slots); ids >= n_tbl are never dereferenced.  first != 0: tbl holds h's rows and w_t = dinv[col[t]] (dinv [n_dinv >=
 * n_tbl]); first == 0: tbl holds the scaled state s_k = dinv * z_k and w_t = 1 (dinv [n_dinv >= n_rows]).  store: 0 the next
 * scaled state dinv[i] * z, 1 the value z itself, 2 its row log_softmax; pad columns are written as 0.  It is the launch
 * sequence bgnn_appnp_propagate_f32 runs per step (one launch, three with hub tables: the same argument group, over the n_rows
 * owned rows), through the same code, so K calls on a square graph give that entry's bits.  1 <= D <= 128, 0 <= alpha <= 1,
 * leading dimensions % 4 == 0 and >= pad4(D), tbl / h / out 16-B aligned, out distinct from tbl and h.
 * ws: n_seg * pad4(D) * 4 + 16 bytes for the hub partial rows, provided by the caller (may be NULL when n_hubs == 0).  Nothing
 * is allocated and the host never waits. */
int bgnn_appnp_step_f32(const float* tbl, int64_t ld_tbl, int64_t n_tbl, const float* h, int64_t ld_h, const int32_t* rowptr,
                        const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows, int32_t D, float alpha, int first,
                        int store, int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                        const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                        void* ws_opt, size_t ws_bytes, float* out, int64_t ld_out, void* stream);
/* Feature dropout of APPNP_Net (models/backbones.py:110-128) on a rank's rows of a partitioned activation: the passes of
 * bgnn_feature_dropout_f32 / bgnn_feature_dropout_bwd_f32 with row_ids (int64 [n_rows], the GLOBAL row of every local row):
 * element (r, c) draws the bits the plain pass draws for flat element row_ids[r] * D + c (word pair e >> 2, 16-bit slot e & 3),
 * so every rank drops what the whole-graph call drops in its rows; identity ids give the plain pass bit for bit.  Bias, ReLU,
 * the (seed, seed_dev) pair and the backward's mask off y > 0 as there.  The grid is capped at 4096 blocks of 256 lanes (one
 * quad of four consecutive local elements per lane and trip), the rest is walked by stride. */
int bgnn_feature_dropout_rows_f32(const float* x, const float* bias_opt, const int64_t* row_ids, int64_t n_rows, int32_t D,
                                  int relu, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, float* y, void* stream);
int bgnn_feature_dropout_rows_bwd_f32(const float* y_opt, const float* grad_y, const int64_t* row_ids, int64_t n_rows, int32_t D,
                                      int relu, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, float* grad_x,
                                      void* stream);

/* ------------------------------------------------------------------------------------------
 * GCNII conv (the GCN2 baseline, models/backbones.py:163-197: PyG GCN2Conv(H, alpha, theta, layer, shared_weights=True,
 * normalize=False) over the cached gcn_norm adjacency, followed by F.relu and the next F.dropout of GCN2.forward), one pass:
 *     m_i = (1 - alpha) * dinv[i] * sum_{t in row i} dinv[col[t]] * x[col[t]] + alpha * x0[i]
 *     y_i = drop(relu(m_i @ M)),       M = (1 - beta) * I + beta * weight1,  beta = log(theta / layer + 1)
 * over the CSR of bgnn_gcn_aggregate_f32 (exactly one self loop per row, dinv[i] = 1/sqrt(deg_i)).  The graph is square: rowptr
 * [n_rows+1], every id in col < n_rows, x / x0 / out (and m_out) have n_rows rows, dinv [n_dinv >= n_rows].  M: the caller forms
 * it once per layer call, [pad4(H), pad4(H)] row-major with zero padding, applied untransposed; rows and columns from H on are
 * not read into the product.  1 <= H <= 128 (else BGNN_E_SHAPE), any H in that range; 0 <= alpha <= 1 (alpha == 1: y does
 * not depend on the graph); 0 <= p_drop < 1: element i * H + column is kept by the shared (seed + *seed_dev_opt, element) hash
 * exactly as bgnn_gcn_aggregate_f32's epilogue 1 keeps it, p_drop == 0 draws no mask.  Leading dimensions in floats, % 4 == 0
 * and >= pad4(H) (x may be a view of a wider table), bases 16-B aligned, out and m_out distinct from x and from each other; pad
 * columns of out and m_out are written as 0.
 * m_out_opt: NULL (evaluation) and the mix is never written to memory; else [n_rows, ldm] and m is written exactly once (the
 * backward's operand of grad_weight1).  y has the same bits either way.
 * The product runs inside the tile on the f32-input MFMA (an exact fp32 fmaf chain over k = 0 .. pad4(H)-1); M sits in LDS once
 * per persistent block.
 * Hub rows: the argument group and the scheme of bgnn_gcn_aggregate_f32 -- with tables the row launch skips them, a segment
 * launch writes partial rows to the workspace, a finish launch adds a hub's partial rows in segment order and runs the same
 * mix, product and epilogue on the finished row: a hub's bits do not depend on which block took which segment.  Without tables
 * (n_hubs == 0) the row launch walks every row whole.  No float atomics.
 * ws: bgnn_gcn2_conv_workspace_bytes(n_seg, H) bytes (may be NULL when n_hubs == 0).  Nothing is allocated, the host never waits.
 *
 * bgnn_gcn2_conv_bwd_f32 (models/backbones.py:163-197, the dense half of the same layer's backward), one streaming pass:
 *     gz = grad_y * [y > 0] * keep_scale     (y > 0 <=> kept and positive: the rule of bgnn_gcn_aggregate_bwd_f32; no mask is redrawn)
 *     gm = gz @ M^T,    t = (1 - alpha) * gm,    gx0 = alpha * gm
 * y: the forward's output; gz, t, gx0: [n_rows, ld], pad columns written as 0, pairwise distinct (gz may be grad_y).  The caller
 * finishes with entries that exist: grad_weight1 = beta * m^T gz (bgnn_gram_f32) and grad_x = the walk of bgnn_gcn_aggregate_f32
 * over the by-source view applied to t (the operator is symmetric in its dinv products). */
size_t bgnn_gcn2_conv_workspace_bytes(int64_t n_seg, int32_t H);
int bgnn_gcn2_conv_f32(const float* x, int64_t ldx, const float* x0, int64_t ldx0, const float* M, const int32_t* rowptr,
                       const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows, int32_t H, float alpha,
                       float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                       int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                       const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                       void* ws_opt, size_t ws_bytes, float* m_out_opt, int64_t ldm, float* out, int64_t ldo, void* stream);
int bgnn_gcn2_conv_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, const float* M, int64_t n_rows,
                           int32_t H, float alpha, float p_drop, float* gz, int64_t ldgz, float* t, int64_t ldt,
                           float* gx0, int64_t ldgx0, void* stream);
/* The GCNII conv over a RECTANGULAR graph (GCN2, models/backbones.py:163-197, on a destination-node partition: a rank's owned
 * rows gather from [owned rows ; halo slots]): bgnn_gcn2_conv_f32 with
 *   n_tbl        rows of x, n_tbl >= n_rows; rowptr [n_rows+1], ids in col < n_tbl (ids >= n_tbl are never dereferenced);
 *   row_ids_opt  NULL, or int64 [n_rows]: the GLOBAL id of every output row.  The dropout element of (row i, column) is then
 *                row_ids[i] * H + column -- in the row launch and, for a hub row, in the finish launch through hub_rows -- the rule
 *                of bgnn_gcn_aggregate_f32's row_id_opt: every rank drops what the whole-graph call drops in its rows.
 * x0, m_out and out have n_rows rows; dinv covers the table, n_dinv >= n_tbl (else BGNN_E_SHAPE): the gather reads dinv[col].
 * out and m_out may not overlap x: checked on the byte extents [base, base + ((rows - 1) * ld + pad4(H)) * 4) of the row-strided
 * views, x over its n_tbl rows, so the front rows of the buffer x lives in are refused, and so are two column slices of one
 * buffer; BGNN_E_SHAPE.  Everything else as bgnn_gcn2_conv_f32, which is this entry with n_tbl = n_rows and no ids through the
 * same launch sequence: identity ids on a square graph give its bits. */
int bgnn_gcn2_conv_rows_f32(const float* x, int64_t ldx, int64_t n_tbl, const float* x0, int64_t ldx0, const float* M,
                            const int32_t* rowptr, const int32_t* col, const float* dinv, int64_t n_dinv, int64_t n_rows,
                            const int64_t* row_ids_opt, int32_t H, float alpha, float p_drop, uint64_t seed,
                            const uint64_t* seed_dev_opt, int32_t hub_threshold, const int32_t* hub_rows_opt, int64_t n_hubs,
                            const int32_t* hub_seg_ptr_opt, const int32_t* seg_bounds_opt, int64_t n_seg,
                            void* ws_opt, size_t ws_bytes, float* m_out_opt, int64_t ldm, float* out, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * DeeperGCN softmax aggregation (the DeeperGCN baseline, models/backbones.py:130-161: the message, the aggregation and the root
 * add of PyG GENConv(H, H, aggr='softmax', t=1.0, learn_t=True, num_layers=2, norm='layer') -- everything in front of its MLP),
 * one walk over the by-destination CSR exactly as given (duplicates are separate messages, self loops ordinary edges, none added):
 *     v_j = relu(x_j) + 1e-7
 *     alpha_ij[c] = softmax over the in-edges j of row i of (t * v_j[c])        per destination AND per channel
 *     o_i = sum_j alpha_ij * v_j   (0 for a row without in-edges),      z_i = o_i + x_i   (the raw x_i)
 * x: [n_tbl, ldx] node rows, n_tbl >= n_rows (row i of z adds row i of x), ids in col >= n_tbl are never dereferenced and add
 * nothing; rowptr [n_rows+1] is cut to [0, n_edges] (a malformed rowptr gives a wrong sum, never a stray read).  t: ONE float in
 * DEVICE memory (the learnable temperature; the host never waits for it), any sign or 0 -- the running maximum is over t * v.
 * z: [n_rows, ldz], distinct from x; pad columns H .. pad4(H)-1 are written as 0 whatever x holds there.  Any H >= 1; leading
 * dimensions in floats, % 4 == 0 and >= pad4(H) (x may be a view of a wider table), bases 16-B aligned.  Columns run in
 * independent slices of 128.
 * lse_opt / o_opt: both NULL (evaluation) or both [n_rows, lds] (training): lse_i[c] = log sum_j exp(t * v_j[c]) and o_i[c], pad
 * columns 0; a row without in-edges stores z_i = x_i bit for bit, lse = 0 and o = 0.  z has the same bits either way.
 * Each lane keeps (max, sum, weighted sum) per channel, takes the maximum of a batch of gathered rows first and rescales once per
 * batch; narrow rows merge their sub-groups by a fixed butterfly.  No float atomics, bit-identical from run to run, nothing is
 * allocated.  A hub row is walked by one lane group.
 *
 * bgnn_gen_softmax_aggregate_bwd_f32 (models/backbones.py:130-161, the backward of the same aggregation), one walk over the
 * by-source view (t_rowptr [n_src+1], t_dst: the destinations of every source's out-edges, ids >= n_rows add nothing):
 *     a_ij = exp(t * v_j - lse_i)                                    (= alpha_ij, <= 1 up to rounding: no overflow)
 *     dv_j = sum over the out-edges j -> i of a_ij * g_i * (1 + t * (v_j - o_i))
 *     grad_x[j] = [x_j > 0] * dv_j + g_j   (g_j for j < n_rows)
 *     grad_t    = sum over edges and channels of a_ij * g_i * (v_j - o_i)^2       (the centred form)
 * x: [n_src, ldx]; grad_z (g), lse, o: [n_rows, .] -- the gradient at z and the forward's tables; grad_x: [n_src, ldgx], written
 * once, pad columns 0, distinct from every input; grad_t: one float in device memory, overwritten.  grad_t leaves the walk as one
 * fp64 partial per block and is summed in a fixed order by a second, one-block launch per column slice: no float atomics, and
 * nothing is carried from one call to the next.  ws: bgnn_gen_softmax_aggregate_workspace_bytes(n_src, H) bytes. */
int bgnn_gen_softmax_aggregate_f32(const float* x, int64_t ldx, int64_t n_tbl, const int32_t* rowptr, const int32_t* col,
                                   int64_t n_edges, int64_t n_rows, int32_t H, const float* t, float* lse_opt, float* o_opt,
                                   int64_t lds, float* z, int64_t ldz, void* stream);
size_t bgnn_gen_softmax_aggregate_workspace_bytes(int64_t n_src, int32_t H);
int bgnn_gen_softmax_aggregate_bwd_f32(const float* x, int64_t ldx, int64_t n_src, const float* grad_z, int64_t ldg,
                                       const float* lse, const float* o, int64_t lds, int64_t n_rows, const int32_t* t_rowptr,
                                       const int32_t* t_dst, int64_t n_edges, int32_t H, const float* t, float* grad_x,
                                       int64_t ldgx, float* grad_t, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * GIN sum aggregation (the GINNet baseline, models/backbones.py:26-57: PyG GINConv(Linear(in, out), train_eps=True) after its
 * transform T = x W^T, with the F.relu / F.dropout between convs and the closing F.log_softmax), one walk over the by-destination
 * CSR exactly as given (duplicates are separate messages, self loops ordinary edges, none added or removed):
 *     out_i = epi( (1 + eps) * tbl_i + sum over t in row i of tbl[col[t]] + bias )
 * tbl: [n_tbl, ldt], n_tbl >= n_rows (row i is its own root: no root buffer); ids in col outside [0, n_tbl) are never dereferenced
 * and add nothing; rowptr [n_rows+1] is cut to [0, n_edges] (a malformed rowptr gives a wrong sum, never a stray read).
 * eps: ONE float in DEVICE memory (GINConv's eps, trainable or not; the host never waits for it), or NULL for weight 1 -- the same
 * bits as a device 0.  bias_opt: [>= pad4(D)] floats, 16-B aligned, or NULL.  epilogue: 0 none, 1 ReLU then dropout at p_drop (the
 * (seed + *seed_dev_opt, element index) hash of bgnn_sage_mean_aggregate_f32; row_id_opt: int64 [n_rows], the GLOBAL row of each
 * output row for that hash, or NULL = row i), 2 log_softmax (D <= 128).  out: [n_rows, ldo], distinct from tbl; pad columns
 * D .. pad4(D)-1 are written as 0 whatever tbl holds there.  Leading dimensions in floats, % 4 == 0 and >= pad4(D) (tbl may be a
 * view of a wider table), bases 16-B aligned; BGNN_E_SHAPE / BGNN_E_ALIGN otherwise.  One lane group per row (the mapping of
 * bgnn_sage_mean_aggregate_f32), columns in slices of 128, a hub row walked by one group (the _hub_ entries below segment it).  No float atomics, nothing allocated.
 *
 * bgnn_gin_aggregate_bwd_f32 (models/backbones.py:26-57, the backward of the same aggregation):
 *     g_i        = the gradient at the epilogue's input from (y_i, grad_y_i): y > 0 ? grad_y * keep_scale : 0 (ReLU then dropout),
 *                  grad_y - exp(y) * rowsum(grad_y) (log_softmax), grad_y (none); written to g [n_rows, ldg], pad columns 0
 *     grad_eps   = sum over i < n_rows of <g_i, tbl_i>        (only with grad_eps_opt; tbl_opt is the forward's table)
 *     grad_tbl_j = (1 + eps) * g_j + sum over the out-edges j -> i of g_i        (g_j for j < n_rows)
 * (t_rowptr [n_src+1], t_col): the by-source view of the same edges, ids >= n_rows add nothing.  grad_tbl: [n_src, ldgt], written
 * once, distinct from g, y and grad_y.  grad_eps_opt: one float in device memory, overwritten, or NULL (no eps pass runs; tbl_opt
 * and ws_opt may then be NULL).  grad_eps is formed in fp64: one partial per block of a row pass, summed in a fixed order by a
 * one-block launch -- no float atomics, bit-identical from run to run, nothing carried from one call to the next.  grad_bias is
 * the caller's: the column sums of g.  ws_opt: bgnn_gin_aggregate_bwd_workspace_bytes(n_rows, D) bytes. */
int bgnn_gin_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* eps, const float* bias_opt,
                           const int32_t* rowptr, const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t D, int epilogue,
                           float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, const int64_t* row_id_opt, float* out,
                           int64_t ldo, void* stream);
size_t bgnn_gin_aggregate_bwd_workspace_bytes(int64_t n_rows, int32_t D);
int bgnn_gin_aggregate_bwd_f32(const float* tbl_opt, int64_t ldt, const float* y, int64_t ldy, const float* grad_y, int64_t ldgy,
                               int64_t n_rows, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_edges, int64_t n_src,
                               int32_t D, const float* eps, int epilogue, float p_drop, float* g, int64_t ldg, float* grad_tbl,
                               int64_t ldgt, float* grad_eps_opt, void* ws_opt, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * GIN sum aggregation with segmented hub rows (the GINNet baseline, models/backbones.py:26-57; the ROWS / SEGMENT / FINISH scheme of
 * bgnn_gcn_aggregate_f32 on GIN's sum).  bgnn_gin_aggregate_hub_f32 computes what bgnn_gin_aggregate_f32 computes,
 *     out_i = epi( (1 + eps) * tbl_i + sum over t in row i of tbl[col[t]] + bias ),
 * with the same arguments plus the hub tables of the SAME view, in bgnn_gcn_aggregate_f32's order: hub_rows_opt [n_hubs] the rows
 * of at least hub_threshold (>= 1) edges, hub_seg_ptr_opt [n_hubs+1] the segment range of each hub, seg_bounds_opt [2 n_seg] one
 * (begin, end) pair of edge offsets per segment, n_seg >= n_hubs, ws_opt >= bgnn_gin_aggregate_hub_workspace_bytes(n_seg, D) bytes
 * (BGNN_E_SHAPE / BGNN_E_NULL / BGNN_E_WORKSPACE otherwise).  n_hubs == 0 takes no table and launches what the entry without hubs
 * launches.  With hubs three launches per 128-column slice:
 *   ROWS     the row kernel neither gathers nor stores for a row of at least hub_threshold edges;
 *   SEGMENT  one lane group per segment sums tbl[col[t]] over its pair (cut to [0, n_edges]; ids outside [0, n_tbl) are never
 *            dereferenced) with the row walk's batches and compensated add into one partial row of ws: no own row, bias, epilogue;
 *   FINISH   one lane group per hub adds its partial rows in segment order through the same compensated add (a segment range is
 *            cut to [0, n_seg]), then fma(1 + eps, own, sum) with the own row read from tbl at hub_rows[h] where that is < n_tbl,
 *            then bias and epilogue; under row_id_opt the mask is drawn for row_id[hub_rows[h]]; pad columns leave as 0; a hub
 *            row outside [0, n_rows) is dropped.
 * Every non-hub row carries the bits of the entry without hubs, and so does a hub of ONE segment; a hub's bits do not depend on
 * which block took which segment.  No float atomics, nothing allocated.
 *
 * bgnn_gin_aggregate_bwd_hub_f32 (models/backbones.py:26-57, the backward of the same aggregation): g, grad_eps and
 *     grad_tbl_j = (1 + eps) * g_j + sum over the out-edges j -> i of g_i        (g_j for j < n_rows)
 * as the backward entry without hubs forms them -- pass A and the grad_eps passes are its launches -- with pass B, the walk over
 * the by-source view (t_rowptr, t_col), run through the hub walk above: the tables are those of the by-source view, hub SOURCES
 * j >= n_rows (a rank's halo slots) have no own term.  ws_opt: bgnn_gin_aggregate_bwd_workspace_bytes(n_rows, D) bytes first (only
 * with grad_eps_opt), then bgnn_gin_aggregate_hub_workspace_bytes(n_seg, D) bytes. */
size_t bgnn_gin_aggregate_hub_workspace_bytes(int64_t n_seg, int32_t D);
int bgnn_gin_aggregate_hub_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* eps, const float* bias_opt,
                               const int32_t* rowptr, const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t D, int epilogue,
                               float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, int32_t hub_threshold,
                               const int32_t* hub_rows_opt, int64_t n_hubs, const int32_t* hub_seg_ptr_opt,
                               const int32_t* seg_bounds_opt, int64_t n_seg, void* ws_opt, size_t ws_bytes,
                               const int64_t* row_id_opt, float* out, int64_t ldo, void* stream);
int bgnn_gin_aggregate_bwd_hub_f32(const float* tbl_opt, int64_t ldt, const float* y, int64_t ldy, const float* grad_y, int64_t ldgy,
                                   int64_t n_rows, const int32_t* t_rowptr, const int32_t* t_col, int64_t n_edges, int64_t n_src,
                                   int32_t D, const float* eps, int epilogue, float p_drop, int32_t hub_threshold,
                                   const int32_t* hub_rows_opt, int64_t n_hubs, const int32_t* hub_seg_ptr_opt,
                                   const int32_t* seg_bounds_opt, int64_t n_seg, float* g, int64_t ldg, float* grad_tbl,
                                   int64_t ldgt, float* grad_eps_opt, void* ws_opt, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * JKNet scaled-sum conv (the JKNet baseline, models/backbones.py:60-107: PyG GCNConv handed the already normalised adj_t_cache,
 * which GCNConv.forward normalises a second time, after its transform T = x W^T, with the F.relu / F.dropout after every conv), one
 * walk over the by-destination CSR WITHOUT self loops (loops dropped, none appended, duplicates are separate messages):
 *     out_i = epi( w_i * tbl_i + s_i * sum over t in row i of s[col[t]] * tbl[col[t]] + bias )
 * s, w: [n_tbl] floats each (twice-normalised operator: s_i = dinv_i * d2_i^-1/2, w_i = 1 / d2_i; textbook GCN: s = dinv, w = dinv^2).
 * tbl: [n_tbl, ldt], n_tbl >= n_rows (row i is its own root: no root buffer); ids in col outside [0, n_tbl) are never dereferenced
 * (neither in s nor in tbl) and add nothing; rowptr [n_rows+1] is cut to [0, n_edges].  bias_opt: [>= pad4(D)] floats, 16-B aligned,
 * or NULL.  epilogue: 0 none, 1 ReLU then dropout at p_drop, element index row * D + column under the (seed + *seed_dev_opt) hash
 * of bgnn_gcn_aggregate_f32 (with w = s^2 and the same seed the zero pattern is that entry's); 2 is refused (BGNN_E_SHAPE).  out:
 * [n_rows, ldo], distinct from tbl, MAY BE A COLUMN SLICE OF A WIDER BUFFER (ldo the buffer's row length): only columns
 * 0 .. pad4(D)-1 of the slice are written, the pad columns as 0.  Leading dimensions in floats, % 4 == 0 and >= pad4(D), bases 16-B
 * aligned.  One lane group per row, columns in slices of 128, a hub row walked by one group with compensated batch adds.  No float
 * atomics, nothing allocated.
 *
 * bgnn_jk_gcn_aggregate_bwd_f32 (models/backbones.py:60-107, the backward of the same conv):
 *     g_i        = y > 0 ? grad_y * keep_scale : 0 (ReLU then dropout) | grad_y (none); written to g [n_rows, ldg], pad columns 0
 *     grad_tbl_j = w_j * g_j + s_j * sum over the out-edges j -> i of s_i * g_i
 * (t_rowptr [n_src+1], t_col): the by-source view of the same edges; n_src == n_rows (one node set).  grad_tbl: [n_src, ldgt],
 * written once, distinct from g, y and grad_y.  grad_bias is the caller's: the column sums of g.  Bit-identical from run to run.
 *
 * bgnn_jk_head_f32 (models/backbones.py:60-107: JumpingKnowledge(cat | max), Linear, log_softmax in one pass):
 * x: the layer buffer [n_rows, ldx], layer l in columns [l*Hp, l*Hp + H), Hp = pad4(H), pad columns 0.  mode 0 (cat): the jumped
 * row is the L slices (K = L*Hp); mode 1 (max): their elementwise maximum, the lowest l on ties (K = Hp).  W: [C, ldw >= K] in the
 * SAME padded column layout (pad columns 0), 16-B aligned, ldw % 4 == 0; bias_opt: [C] or NULL.  out [n_rows, ldo >= pad4(C)] =
 * jumped @ W^T + bias, then log_softmax over the C classes when log_softmax != 0; pad columns are written as 0.  The product is the
 * f32-input MFMA (exact fp32 products, four split-K partial sums per class).  Max mode only: win_opt uint8 [n_rows, Hp] (4-B
 * aligned) receives the winning layer per element and jump_opt [n_rows, ldj >= Hp] the jumped row (both or neither may be NULL).
 * Envelope: bgnn_jk_head_supported(L, H, C, mode) != 0 <=> 1 <= L <= 8, 1 <= C <= 32 and W fits 64 KB of LDS (16 or 32 rows of
 * K rounded up to 16 floats); BGNN_E_SHAPE outside it.
 *
 * bgnn_jk_max_route_f32 (models/backbones.py:60-107, the backward of the max jump): grad_x[i, l*Hp + c] = win[i, c] == l ?
 * grad_jump[i, c] : 0 for every l < L and c < Hp; grad_x [n_rows, ldx >= L*Hp] is written whole. */
int bgnn_jk_gcn_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* s, const float* w, const float* bias_opt,
                              const int32_t* rowptr, const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t D, int epilogue,
                              float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, float* out, int64_t ldo, void* stream);
int bgnn_jk_gcn_aggregate_bwd_f32(const float* y, int64_t ldy, const float* grad_y, int64_t ldgy, int64_t n_rows,
                                  const int32_t* t_rowptr, const int32_t* t_col, int64_t n_edges, int64_t n_src, const float* s,
                                  const float* w, int32_t D, int epilogue, float p_drop, float* g, int64_t ldg, float* grad_tbl,
                                  int64_t ldgt, void* stream);
int bgnn_jk_head_supported(int32_t L, int32_t H, int32_t C, int mode);
int bgnn_jk_head_f32(const float* x, int64_t ldx, int64_t n_rows, int32_t L, int32_t H, int mode, const float* W, int64_t ldw,
                     const float* bias_opt, int32_t C, int log_softmax, float* out, int64_t ldo, uint8_t* win_opt, float* jump_opt,
                     int64_t ldj, void* stream);
int bgnn_jk_max_route_f32(const float* grad_jump, int64_t ldj, const uint8_t* win, int64_t n_rows, int32_t L, int32_t H,
                          float* grad_x, int64_t ldx, void* stream);

/* ------------------------------------------------------------------------------------------
 * GAT attention aggregation (the `gnn='GAT'` baseline of main_graph_knowledge_transfer.py:327-328):
 *     models/backbones.py:404-438 -- two PyG GATConv (heads, concat, negative_slope 0.2, attention dropout 0.6, add_self_loops,
 *     bias) with F.elu + F.dropout(p=0.6) between them (:427-428) and F.log_softmax (:430).
 * The caller transforms first (tbl = x W^T, [n, H*C], head h of row n at tbl[n*ldt + h*C]; ldt a multiple of 4, >= pad4(H*C))
 * and hands the by-destination CSR with exactly one self loop per row (bgnn_build_dst_csr with rewrite_self_loops: PyG's
 * remove_self_loops + add_self_loops; duplicate edges stay separate edges).  1 <= H <= 8, 1 <= C <= 128 (else BGNN_E_SHAPE).
 * bgnn_gat_scores_f32: s_src[n,h] = <tbl[n,h,:], att_src[h,:]>, s_dst[n,h] = <tbl[n,h,:], att_dst[h,:]> ([n, H] each; att_* are
 * [H*C] floats) in one read of tbl -- GATConv's (x_src * att_src).sum(-1) / (x_dst * att_dst).sum(-1).
 * bgnn_gat_aggregate_f32, for row i, head h over the edges t of the row, j = col[t]:
 *   z = s_src[j,h] + s_dst[i,h];  e = z > 0 ? z : negative_slope * z;  alpha = softmax_t(e) (row maximum subtracted);
 *   a~ = alpha * m[t,h], m = 0 or 1/(1 - p_att) from the counter hash of bgnn_bn_relu_dropout_f32 at element t*H + h with
 *   seed_att (+ *seed_att_dev_opt) -- t is the edge's position in this CSR, so duplicate edges draw independently;
 *   out[i,h,:] = epi( sum_t a~ * tbl[j,h,:] + bias[h,:] ).
 * Epilogues: 0 none; 1 ELU then dropout at p_drop over element index i*(H*C) + h*C + c with seed (+ *seed_dev_opt); 2 row
 * log_softmax (H == 1 only).  Outputs: state [n_rows, H, 2] = the softmax's (maximum, denominator) per (row, head); the
 * coefficients a~ as [n_edges, H] in CSR order, into alpha_out_opt when given, else into ws
 * (bgnn_gat_aggregate_workspace_bytes(n_edges, n_rows, H)); pre_out_opt [n_rows, ldp]: the conv output before the epilogue
 * (what the backward needs; NULL: not written); out [n_rows, ldo]; pad columns H*C .. pad4(H*C) of out and pre_out leave as 0.
 * Two passes over the scores (state, then coefficients), one gather pass over tbl; rows of any degree, one lane group each.
 * bgnn_gat_aggregate_bwd_f32: the atomic-free backward from the forward's (s_src, s_dst, state, alpha, pre) and grad_y.
 * A row pass writes g [n_rows, ldg] (the gradient at the conv output: ELU' from pre and the feature mask REDRAWN from
 * (seed, element index); grad_y - softmax(pre) * rowsum(grad_y) for epilogue 2) and r[i,h] = <g[i,h,:], pre[i,h,:] - bias[h,:]>;
 * a pass over the by-destination CSR forms per edge da = m * <g[i,h,:], tbl[j,h,:]>, de = alpha * (da - r[i,h]),
 * dz = de * (z > 0 ? 1 : negative_slope) into ws, and ds_dst[i,h] = sum_t dz in the per-side form
 * (1 - negative_slope) (S+ Z- - S- Z+) / (Z+ + Z-), S and Z the row's sums of alpha * da and of alpha over its z > 0 / z <= 0 edges
 * (the row's de sum to zero; summing the stored dz, whose r comes from pre, would leave a rounding of r in every row); a pass over the by-source view (t_rowptr [n_src+1],
 * t_eid = the edge's position in the by-destination order, t_dst = its destination: `DstCSR.transposed()`) forms
 * grad_tbl[j,h,:] = sum a~ * g[i,h,:] and ds_src[j,h] = sum dz.  The caller finishes: grad_bias = column sums of g,
 * grad_tbl += ds_src (x) att_src + ds_dst (x) att_dst, grad_att_src[h,:] = sum_n ds_src[n,h] * tbl[n,h,:] (att_dst likewise).
 * Rows and sources are counted separately: n_rows destination rows (rowptr [n_rows+1]; s_dst, state, pre, grad_y, g and ds_dst are
 * over n_rows, and so is the workspace: bgnn_gat_aggregate_workspace_bytes(n_edges, n_rows, H)) and n_src >= n_rows source rows
 * (tbl, s_src, grad_tbl and ds_src are over n_src, t_rowptr is [n_src+1]); every id in col is < n_src, every id in t_dst < n_rows.
 * On a whole graph n_src == n_rows (self loops make every node both); a rank's extended graph of a partition has its halo slots
 * as further sources without in-edges.
 * row_id_opt / edge_base_opt [n_rows] (int64), of both entries, for a block of rows of a larger graph (a rank's rows of a
 * destination-node partition: tbl and s_src cover the rank's own rows followed by its halo rows, n_src = n_ext in the backward).
 * Both masks are then drawn where the whole-graph call draws them: row_id is every row's GLOBAL id, the feature-dropout element
 * index becomes row_id[i]*(H*C) + h*C + c; edge_base is the position of the row's first edge in the WHOLE graph's by-destination
 * CSR, the attention-dropout element index of edge t of row i becomes (edge_base[i] + (t - rowptr[i])) * H + h -- a rank's rows
 * must keep the whole graph's edge order inside a row.  The backward redraws both masks from the same ids.  The ids feed the hash
 * only and never form an address.  NULL (or no dropout): row i, edge t; the plain kernels run.
 * Deterministic bits.  A row's edge range is cut to [0, n_edges] and ids are
 * checked against their tables: a malformed CSR gives a wrong sum, never a stray access.  The entry points are defined in
 * csrc/bgnn_gat.hip next to their kernels. */
int bgnn_gat_scores_f32(const float* tbl, int64_t ldt, int64_t n, int32_t H, int32_t C, const float* att_src,
                        const float* att_dst, float* s_src, float* s_dst, void* stream);
size_t bgnn_gat_aggregate_workspace_bytes(int64_t n_edges, int64_t n_rows, int32_t H);
int bgnn_gat_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* s_src, const float* s_dst,
                           const float* bias_opt, const int32_t* rowptr, const int32_t* col, int64_t n_edges,
                           int64_t n_rows, int32_t H, int32_t C, float negative_slope, float p_att, uint64_t seed_att,
                           const uint64_t* seed_att_dev_opt, int epilogue, float p_drop, uint64_t seed,
                           const uint64_t* seed_dev_opt, const int64_t* row_id_opt, const int64_t* edge_base_opt, float* state,
                           float* alpha_out_opt, void* ws_opt, size_t ws_bytes, float* pre_out_opt, int64_t ldp, float* out,
                           int64_t ldo, void* stream);
int bgnn_gat_aggregate_bwd_f32(const float* tbl, int64_t ldt, int64_t n_src, const float* s_src, const float* s_dst,
                               const float* bias_opt, const float* state, const float* alpha, const float* pre, int64_t ldp,
                               const float* grad_y, int64_t ldgy, const int32_t* rowptr, const int32_t* col,
                               const int32_t* t_rowptr, const int32_t* t_eid, const int32_t* t_dst, int64_t n_edges,
                               int64_t n_rows, int32_t H, int32_t C, float negative_slope, float p_att, uint64_t seed_att,
                               const uint64_t* seed_att_dev_opt, int epilogue, float p_drop, uint64_t seed,
                               const uint64_t* seed_dev_opt, void* ws, size_t ws_bytes, const int64_t* row_id_opt,
                               const int64_t* edge_base_opt, float* g, int64_t ldg, float* grad_tbl, int64_t ldgt, float* ds_src,
                               float* ds_dst, void* stream);

/* ------------------------------------------------------------------------------------------
 * GATv2 attention conv (the `gnn='GATv2'` baseline of main_graph_knowledge_transfer.py:329-330):
 *     models/backbones.py:302-358 -- PyG GATv2Conv (share_weights=False: lin_l and lin_r with bias; heads, concat,
 *     negative_slope 0.2, attention dropout, add_self_loops, bias) with F.elu + F.dropout between the convs (:354-355) and
 *     log_softmax (:358).
 * The caller transforms first into ONE table tbl = x [W_l ; W_r]^T + [b_l ; b_r]: x_l[n,h,:] at tbl[n*ldt + h*C], x_r[n,h,:] at
 * tbl[n*ldt + P + h*C], P = pad4(H*C); ldt a multiple of 4, >= 2P; n_tbl >= n_rows rows.  The CSR is GAT's: by destination with
 * exactly one self loop per row (bgnn_build_dst_csr with rewrite_self_loops).  1 <= H <= 8, 1 <= C <= 128 (else BGNN_E_SHAPE).
 * bgnn_gatv2_aggregate_f32, for row i, head h over the edges t of the row, j = col[t], in ONE pass (online softmax):
 *   m = x_l[j,h,:] + x_r[i,h,:] (one rounded fp32 add per column);  e = sum_c att[h,c] * (m_c > 0 ? m_c : negative_slope * m_c);
 *   alpha = softmax_t(e);  a~ = alpha * mask[t,h], mask = 0 or 1/(1 - p_att) from the counter hash at element t*H + h with
 *   seed_att (+ *seed_att_dev_opt) -- GAT's contract; the denominator sums every edge;
 *   out[i,h,:] = epi( sum_t a~ * x_l[j,h,:] + bias[h,:] ).
 * att: [H*C] floats, 16-byte aligned.  Epilogues as bgnn_gat_aggregate_f32 (0 none; 1 ELU then dropout at p_drop over element
 * i*(H*C) + h*C + c with seed (+ *seed_dev_opt); 2 row log_softmax, H == 1 only).  Outputs: state [n_rows, H, 2] = (maximum,
 * denominator >= 1); alpha_out_opt [n_edges, H]: the coefficients a~ in CSR order (NULL: not formed; the pass parks the logits
 * there and a sweep over the row's own words finishes them, no second gather); pre_out_opt [n_rows, ldp]: the conv output
 * before the epilogue (NULL: not written); out [n_rows, ldo]; pad columns H*C .. P of out and pre_out leave as 0.
 * bgnn_gatv2_aggregate_bwd_f32: the atomic-free backward from (tbl, att, state, pre) and grad_y.  A row pass writes g [n_rows, ldg] and r[i,h] = <g[i,h,:], pre[i,h,:] - bias[h,:]> as GAT's does; a pass
 * over the by-destination CSR regathers x_l[j], rebuilds e with the forward's own operations, alpha = exp(e - max) / den,
 * da = mask * <g[i,h,:], x_l[j,h,:]>, de = alpha * (da - r); de and a~ go to ws, grad_tbl[i, P + h*C + c] = sum_t de * att[h,c] *
 * leaky'(m_c), and grad_att[h,c] = sum over all edges of de * leaky(m_c): per block partial rows added in a fixed order by a small
 * second kernel; a pass over the by-source view (t_rowptr, t_eid, t_dst: `DstCSR.transposed()`) gathers g[i] and x_r[i]:
 * grad_tbl[j, h*C + c] = sum a~ * g[i,h,c] + de * att[h,c] * leaky'(x_l[j,h,c] + x_r[i,h,c]).  grad_tbl [n_src, ldgt >= 2P] is the
 * whole gradient of tbl (pad columns 0); the caller finishes with grad_bias = column sums of g.
 * Rows and sources are counted separately: n_rows destination rows (rowptr [n_rows+1]; state, pre, grad_y and g are over n_rows,
 * and so is the workspace: bgnn_gatv2_aggregate_workspace_bytes(n_edges, n_rows, H, C)) and n_src >= n_rows source rows (else
 * BGNN_E_SHAPE; tbl and grad_tbl are over n_src, t_rowptr is [n_src+1]); every id in col is < n_src, every id in t_dst < n_rows.
 * On a whole graph n_src == n_rows; a rank's extended graph of a partition has its halo slots as further sources.  The
 * by-destination pass regathers x_l[j] for j < n_src; the by-source pass walks n_src sources and reads x_r and g of rows < n_rows
 * only.  The x_r half of grad_tbl (columns [P, 2P)) is written for rows < n_rows and is 0 for the rows n_rows .. n_src (a halo slot
 * has no in-edges, its x_r is never read); grad_att is the sum over this call's edges.
 * row_id_opt / edge_base_opt [n_rows] (int64), of both entries, for a block of rows of a larger graph (a rank's rows of a
 * destination-node partition: tbl covers the rank's own rows followed by its halo rows).  Both masks are then drawn where the
 * whole-graph call draws them: row_id is every row's GLOBAL id, the feature-dropout element index becomes
 * row_id[i]*(H*C) + h*C + c; edge_base is the position of the row's first edge in the WHOLE graph's by-destination CSR, the
 * attention-dropout element index of edge t of row i becomes (edge_base[i] + (t - rowptr[i])) * H + h -- a rank's rows must keep
 * the whole graph's edge order inside a row.  The two pointers are given together (else BGNN_E_NULL); the ids feed the hash only
 * and never form an address.  The backward redraws both masks from the same ids.  NULL (or no dropout): row i, edge t; the plain
 * kernels run.
 * No float atomics: two identical calls are bitwise equal.  A row's edge range is cut to
 * [0, n_edges] and ids are checked against their tables.  The entry points are defined in csrc/bgnn_gatv2.hip next to their
 * kernels. */
size_t bgnn_gatv2_aggregate_workspace_bytes(int64_t n_edges, int64_t n_rows, int32_t H, int32_t C);
int bgnn_gatv2_aggregate_f32(const float* tbl, int64_t ldt, int64_t n_tbl, const float* att, const float* bias_opt,
                             const int32_t* rowptr, const int32_t* col, int64_t n_edges, int64_t n_rows, int32_t H, int32_t C,
                             float negative_slope, float p_att, uint64_t seed_att, const uint64_t* seed_att_dev_opt,
                             int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt,
                             const int64_t* row_id_opt, const int64_t* edge_base_opt, float* state, float* alpha_out_opt,
                             float* pre_out_opt, int64_t ldp, float* out, int64_t ldo, void* stream);
int bgnn_gatv2_aggregate_bwd_f32(const float* tbl, int64_t ldt, int64_t n_src, const float* att, const float* bias_opt,
                                 const float* state, const float* pre, int64_t ldp, const float* grad_y, int64_t ldgy,
                                 const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_eid,
                                 const int32_t* t_dst, int64_t n_edges, int64_t n_rows, int32_t H, int32_t C,
                                 float negative_slope, float p_att, uint64_t seed_att, const uint64_t* seed_att_dev_opt,
                                 int epilogue, float p_drop, uint64_t seed, const uint64_t* seed_dev_opt, void* ws,
                                 size_t ws_bytes, const int64_t* row_id_opt, const int64_t* edge_base_opt, float* g, int64_t ldg,
                                 float* grad_tbl, int64_t ldgt, float* grad_att, void* stream);

/* ------------------------------------------------------------------------------------------
 * (a2,a3,a5,a6,a7) kNN bridge: pair scoring + per-query top-k.
 *     main_bridged_graph.py:45-67 / :90-111 (batched loop), models/models.py:124-130,:944-954
 *     (scorers), :265-282 (pair_enumeration -- never materialised here), Tensor.topk :60,:104.
 * Selection rule (declared; replaces torch's unspecified tie order): the k candidates with the
 * largest CANONICAL score, ties -> lower candidate index; rows come out sorted by that rule.
 * CANONICAL score = fp64 accumulation in feature-index order of the exact fp32 products
 * (oracle/oracle_c.c orc_cosine_topk / orc_mlp_topk).  Cosine: a cascade of filters with a proof per stage --
 * (0) every fp32 embedding is split exactly into bf16 pieces and the residual norms give a rigorous bound eps on
 * |approximate - exact| score; (1) a FAST pass streams all candidates on the bf16 matrix cores with one piece per
 * candidate, keeping per query the candidates within 2 eps of the running k-th best; (2) the survivors are re-scored
 * in canonical arithmetic and the row is proven (kth_exact > best excluded approximate score + eps) or queued;
 * (3) queued rows go through a PRECISE pass (three piece products, eps ~ 5e-5) and the same proof; (4) rows that are
 * still unproven (exact ties across the boundary) are re-done exhaustively.  mlp: fp32 VALU pass + stages (2), (4), with a
 * bound per QUERY proven from the call's own data: the fp32 chain (one add and two fmas per hidden unit) errs by at most
 * (H + 2) 2^-24 S, S = |b2| + sum_h |w2_h| (|scale_h| |a_h + b_h| + |shift_h|) -- it follows the magnitude of the TERMS, not
 * of the score, which may be small where they cancel -- and eps_q takes S over all candidates from the column maxima of |A|
 * (one reduction per call) and the query's own |B| row, with (H + 4) 1.01 for the constant.  The shortlist margin, the refine
 * stage and the proof read the same eps_q; terms that cancel to within eps_q send the row to stage (4), never to a wrong index.
 * n_fallback_opt (optional, int32[2] on the device): [0] = rows re-done exhaustively, [1] = rows sent to the precise pass.
 * val_out = sigmoid(score) as fp32 if apply_sigmoid (models.py:129,:953) else the fp32 score.
 * k <= 56.  q* must already be L2-normalised by bgnn_l2_normalize_rows_f32 (cosine).
 * bgnn_topk_workspace_bytes depends on the process's BGNN_KNN_FAST_PRODUCTS (read once; =3 gives the fast pass the precise
 * pass's longer shortlists): size the workspace with the figure of the process that makes the call.          */
int bgnn_l2_normalize_rows_f32(const float* q, int64_t n, int32_t d, float eps, float* out, void* stream);
size_t bgnn_topk_workspace_bytes(int64_t Nq, int64_t Nc, int32_t k);
int bgnn_cosine_topk_f32(const float* qn_query, const float* qn_cand, int64_t Nq, int64_t Nc,
                         int32_t d, int32_t k, int apply_sigmoid,
                         int64_t* idx_out /*[Nq,k]*/, float* val_out /*[Nq,k]*/,
                         int32_t* n_fallback_opt, void* ws, size_t ws_bytes, void* stream);
int bgnn_mlp_pair_topk_f32(const float* A_cand /*[Nc,H]*/, const float* B_query /*[Nq,H]*/,
                           const float* bn_scale, const float* bn_shift, const float* w2, float b2,
                           int64_t Nq, int64_t Nc, int32_t H, int32_t k, int apply_sigmoid,
                           int64_t* idx_out, float* val_out, int32_t* n_fallback_opt,
                           void* ws, size_t ws_bytes, void* stream);

/* (a2/a3 tail) edge list from the top-k table: edge (from = idx[q,t] + cand_base, to = q + query_base),
 * main_bridged_graph.py:61-63,:105-107.  edge_index_out is [2, Nq*k].                          */
int bgnn_topk_edges_i64(const int64_t* idx, int64_t Nq, int32_t k, int64_t cand_base, int64_t query_base,
                        int64_t* edge_index_out, void* stream);
/* The same table as a COALESCED edge list (what main_bridged_graph.py:75 / :113 pass on: coalesce(edge_index_added)) in one
 * call: the k candidates of a query are distinct (0 <= idx < Nc, k <= Nc), so the list has no duplicates and coalescing is a
 * stable sort by candidate id of the query-major pairs -- 32-bit pairs over ceil(log2 Nc) bits, exactly Nq * k edges out, no
 * device-to-host read.  Equal to bgnn_coalesce_i64 applied to bgnn_topk_edges_i64's output.  ws:
 * bgnn_topk_edges_coalesced_workspace_bytes(Nq, k). */
size_t bgnn_topk_edges_coalesced_workspace_bytes(int64_t Nq, int32_t k);
int bgnn_topk_edges_coalesced_i64(const int64_t* idx, int64_t Nq, int32_t k, int64_t Nc, int64_t cand_base, int64_t query_base,
                                  int64_t* edge_index_out, void* ws, size_t ws_bytes, void* stream);

/* Packs table rows for a halo send list (bridged_gnn_amd/dist.py; the reference is single-device):
 * dst[r, :row_floats] = src[idx[r], :row_floats].  row_floats % 4 == 0, 16-B aligned tables with ld % 4 == 0; indices
 * are clamped into [0, src_rows).  Narrow rows (the classifier stage's 48-byte rows) are what the library gather is slow at. */
int bgnn_gather_rows_f32(const float* src, int64_t src_rows, int64_t ld_src, const int64_t* idx, int64_t n,
                         int32_t row_floats, float* dst, int64_t ld_dst, void* stream);

/* (a8) torch_geometric.utils.coalesce -- call sites main_bridged_graph.py:75,:113,:193.
 * key = row*num_nodes + col, ascending, duplicates dropped.  In place on [2,E] (row stride E);
 * the first *E_out_dev columns of each row are valid afterwards.                               */
size_t bgnn_coalesce_workspace_bytes(int64_t E);
int bgnn_coalesce_i64(int64_t* edge_index, int64_t E, int64_t num_nodes, int64_t* E_out_dev,
                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Train-mode pair passes of the mlp similarity scorer Similar_v2(mode='mlp')      models/models.py:913-920, :949-951, :967-970
 * under train_adv_few_shot's BCE (scripts.py:36-50), for the similarity-learner training of bridged_gnn_amd/simlearner.py.
 * BN1 (batch statistics) and Linear(2H, 128) are per-node work done by the caller: u_p = A[idx1[p]] + B[idx2[p]] with
 * A [nA, 128] and B [nB, 128] row-strided fp32 tables (16-B aligned, ld >= 128, ld % 4 == 0); idx1 / idx2 int64 [P], out-of-range
 * ids are clamped.  Every column sum is fp64 over a grid fixed by P in a fixed order (no atomics): results are run-to-run
 * identical.  ws: bgnn_pair_mlp_workspace_bytes(P).  P <= 1 is BGNN_E_SHAPE in train mode (torch raises on one value per channel).
 * stats:  stats[0:128] = batch mean of u, stats[128:256] = biased variance (fp64); with run_mean_opt / run_var_opt the
 *         nn.BatchNorm1d running update (momentum, unbiased variance P / (P - 1)) of BN2.
 * loss:   BN2 (stats, eps), ReLU, w2 dot, b2 (device scalar), sigmoid -> p_out [P]; dl_out [P] = d(mean BCE) / d logit along
 *         torch's chain ((p - y) / max((1 - p) p, 1e-12) / P * (1 - p) p: exactly 0 where p is 0 or 1); y uint8 [P] (0 / 1).
 *         sums [392] fp64: [0:128) sum dy, [128:256) sum dy * x2, [256:384) sum dl * h (= dw2), then sum dl (= db2), sum of the
 *         BCE terms (log clamp -100), TP, FP, FN at p > 0.5; dy = dl * w2 * [BN2 output > 0] (sum dy = dbeta2, sum dy x2 = dgamma2).
 * segsum: S[n] = sum over the pairs of node n (CSR rowptr [n_own+1] / perm [P] = pair ids, e.g. bgnn_build_dst_csr(eperm) of the
 *         list by n) of du_p = g2 rstd2 (dy_p - sum dy / P - x2_p sum(dy x2) / P), u_p = own[n] + other[idx_other[p]]; every row
 *         written once (zero rows for nodes without pairs).  Called with (A, B, idx2) for S1 and (B, A, idx1) for S2.
 * eval:   running-statistics form: BN2 as scale2 / shift2, p_out [P]; with y_opt, counts_opt[0:3] = TP, FP, FN (fp64).
 * count:  the running-statistics form over every (i, j) of rows1 [m1] x rows2 [m2] (int64 ids), no pair materialised:
 *         counts [4] int64 = TP, FP, FN, TN of (sigmoid(b2 + sum_c w2[c] relu(scale2[c] (A[rows1[i]][c] + B[rows2[j]][c]) +
 *         shift2[c])) > 0.5 in fp32, eval's predicate) against (lab1[rows1[i]] == lab2[rows2[j]]) (lab1 [nA], lab2 [nB] int64).
 *         BN2 is folded into the tables (scale2 A + shift2, scale2 B) and the columns summed in ascending order, so a pair
 *         whose logit is within fp32 rounding of 0 may be counted differently from eval.  scale2 / shift2 16-B aligned; m1 or
 *         m2 may be 0.  ws: bgnn_pair_mlp_count_workspace_bytes(m1, m2).                                                     */
size_t bgnn_pair_mlp_workspace_bytes(int64_t P);
size_t bgnn_pair_mlp_count_workspace_bytes(int64_t m1, int64_t m2);
int bgnn_pair_mlp_stats_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB, const int64_t* idx1,
                            const int64_t* idx2, int64_t P, float momentum, float* run_mean_opt, float* run_var_opt, double* stats,
                            void* ws, size_t ws_bytes, void* stream);
int bgnn_pair_mlp_loss_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB, const int64_t* idx1,
                           const int64_t* idx2, const uint8_t* y, int64_t P, const double* stats, const float* g2, const float* be2,
                           const float* w2, const float* b2, float eps, float* p_out, float* dl_out, double* sums, void* ws,
                           size_t ws_bytes, void* stream);
int bgnn_pair_mlp_segsum_f32(const float* own, int64_t ld_own, int64_t n_own, const float* other, int64_t ld_other, int64_t n_other,
                             const int32_t* rowptr, const int32_t* perm, const int64_t* idx_other, int64_t P, const float* dl,
                             const double* stats, const double* sums, const float* g2, const float* be2, const float* w2, float eps,
                             float* S, int64_t ld_s, void* stream);
int bgnn_pair_mlp_eval_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB, const int64_t* idx1,
                           const int64_t* idx2, const uint8_t* y_opt, int64_t P, const float* scale2, const float* shift2,
                           const float* w2, const float* b2, float* p_out, double* counts_opt, void* ws, size_t ws_bytes,
                           void* stream);
int bgnn_pair_mlp_count_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB, const int64_t* rows1,
                            int64_t m1, const int64_t* rows2, int64_t m2, const int64_t* lab1, const int64_t* lab2,
                            const float* scale2, const float* shift2, const float* w2, const float* b2, long long* counts, void* ws,
                            size_t ws_bytes, void* stream);


/* ------------------------------------------------------------------------------------------
 * Pair passes of the cosine similarity scorer Similar (v1)                        models/models.py:67-169
 * under train_adv_few_shot's BCE (scripts.py:36-50) and the Cartesian evaluation of eval_within_domain / eval_cross_domain
 * (scripts.py:98-190), for bridged_gnn_amd/simlearner_v1.py.  q = u + biasatt(u), u = lin_self(z) and the row normalisation
 * q^ = q / max(|q|, 1e-8) are per-node work done by the caller: A [nA, 128], B [nB, 128] are normalised row-strided fp32
 * tables (16-B aligned, ld >= 128, ld % 4 == 0); out-of-range ids are clamped.  No atomics: results are run-to-run identical.
 * loss:   cos_p = A[idx1[p]] . B[idx2[p]], p_out [P] = sigmoid(cos_p) (fp32), dl_out [P] = d(mean BCE) / d cos_p along torch's
 *         chain ((p - y) / max((1 - p) p, 1e-12) / P * (1 - p) p); y uint8 [P] (0 / 1).  sums [4] fp64 in a fixed order: sum of
 *         the BCE terms (log clamp -100), TP, FP, FN at p > 0.5.  ws: bgnn_pair_cos_loss_workspace_bytes(P).  P >= 1.
 * segsum: G[n] = sum over the pairs of node n (CSR rowptr [n_own+1] / perm [P] = pair ids, e.g. the pair CSR of the list by n)
 *         of dl[p] * other[idx_other[p]], fp64 accumulation; every row of G [n_own, 128] written once (zero rows for nodes
 *         without pairs).
 * count:  counts [4] int64 = TP, FP, FN, TN of (sigmoid(A[rows1[i]] . B[rows2[j]]) > 0.5 in fp32) against
 *         (lab1[rows1[i]] == lab2[rows2[j]]) over every (i, j) of rows1 [m1] x rows2 [m2] (int64 ids; lab1 [nA], lab2 [nB]
 *         int64), no pair materialised; m1 or m2 may be 0.  ws: bgnn_pair_cos_count_workspace_bytes(m1, m2).             */
size_t bgnn_pair_cos_loss_workspace_bytes(int64_t P);
size_t bgnn_pair_cos_count_workspace_bytes(int64_t m1, int64_t m2);
int bgnn_pair_cos_loss_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB, const int64_t* idx1,
                           const int64_t* idx2, const uint8_t* y, int64_t P, float* p_out, float* dl_out, double* sums, void* ws,
                           size_t ws_bytes, void* stream);
int bgnn_pair_cos_segsum_f32(const float* other, int64_t ld_other, int64_t n_other, const int32_t* rowptr, const int32_t* perm,
                             const int64_t* idx_other, int64_t P, const float* dl, int64_t n_own, float* G, int64_t ld_g,
                             void* stream);
int bgnn_pair_cos_count_f32(const float* A, int64_t lda, int64_t nA, const float* B, int64_t ldb, int64_t nB, const int64_t* rows1,
                            int64_t m1, const int64_t* rows2, int64_t m2, const int64_t* lab1, const int64_t* lab2, long long* counts,
                            void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Step 2's loss and metric counts                              main_graph_knowledge_transfer.py:39-142, :265-300
 * for bridged_gnn_amd/transfer.py.  Tables are fp32 log-probabilities [N, C] with a row stride (ld >= C, unit column stride, no
 * alignment requirement, any C >= 1); y int64 [N]; masks uint8 [N] (0 / 1).  A label outside [0, C) on a selected row selects
 * nothing (the driver refuses such graphs at set-up).  No host synchronisation, no row compaction; scratch and outputs are cleared
 * by kernels, never by a memset node, so every entry may be captured into a HIP graph.
 * loss:      replaces :44-54.  terms [8] fp64 = total, nll(lp_s | train), nll(lp_t | train & ~central), nll(lp_t^ | train & ~central),
 *            KL_batchmean(lp_t^ || lp_t) = sum exp(lp_t)(lp_t - lp_t^) / N, #train, #train & ~central, 0;
 *            total = (2 nll_s + nll_t + nll_t^) / 4 + lambda KL.  An empty selection makes its mean NaN (0 / 0), as F.nll_loss
 *            does.  fp64 sums in a fixed order without atomics: two calls are bitwise equal.  ws: bgnn_step2_loss_workspace_bytes.
 * loss_bwd:  replaces loss.backward() for :54: writes every element of the three gradient tables g_s, g_t, g_h [N, C] (row stride
 *            ld_g), scaled by grad_out[0] (device fp32 scalar); `terms` is the forward's output (the row counts are read from it).
 * nll:       replaces :269 (train_noDTC): terms [2] fp64 = nll(lp | mask), #mask.   nll_bwd: its gradient table.
 * counts:    replaces what :82-105, :125-131 and :285-295 hand to sklearn.  One pass over the rows: per-row argmax of each table
 *            that is needed (ties -> the lowest index), then counts [K, C, C] int64, counts[k][true][predicted], for K <= 8
 *            combinations; byte k of `combos` = table index 0..2 | selection bit 0..7 << 2; sel uint8 [N]: bit b set = the row
 *            is in selection b.  Tables that no combination names may be NULL.
 * auc_count: the rank statistic of roc_auc_score(y, score): out [2] int64 = sum over the rows with pos[r] of
 *            2 #{negatives with a smaller score} + #{negatives with an equal score}, and #positive rows; neg_sorted [>= *n_neg] are
 *            the negatives' scores in ascending order, n_neg a device int64.  AUC = out[0] / (2 out[1] *n_neg).            */
size_t bgnn_step2_loss_workspace_bytes(int64_t N, int32_t C);
int bgnn_step2_loss_f32(const float* lp_s, int64_t ld_s, const float* lp_t, int64_t ld_t, const float* lp_h, int64_t ld_h, int64_t N,
                        int32_t C, const int64_t* y, const uint8_t* train_mask, const uint8_t* central_mask, double lambda,
                        double* terms, void* ws, size_t ws_bytes, void* stream);
int bgnn_step2_loss_bwd_f32(const float* lp_t, int64_t ld_t, const float* lp_h, int64_t ld_h, int64_t N, int32_t C, const int64_t* y,
                            const uint8_t* train_mask, const uint8_t* central_mask, double lambda, const double* terms,
                            const float* grad_out, float* g_s, float* g_t, float* g_h, int64_t ld_g, void* stream);
int bgnn_step2_nll_f32(const float* lp, int64_t ld, int64_t N, int32_t C, const int64_t* y, const uint8_t* mask, double* terms, void* ws,
                       size_t ws_bytes, void* stream);
int bgnn_step2_nll_bwd_f32(int64_t N, int32_t C, const int64_t* y, const uint8_t* mask, const double* terms, const float* grad_out,
                           float* g, int64_t ld_g, void* stream);
int bgnn_step2_counts_f32(const float* t0, int64_t ld0, const float* t1, int64_t ld1, const float* t2, int64_t ld2, int64_t N, int32_t C,
                          const int64_t* y, const uint8_t* sel, uint64_t combos, int32_t K, long long* counts, void* stream);
int bgnn_step2_auc_count_f32(const float* score, const uint8_t* pos, int64_t N, const float* neg_sorted, const int64_t* n_neg,
                             long long* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-tensor Adam with device-resident step and schedule    main_graph_knowledge_transfer.py:205, :67, :353, :274
 * for bridged_gnn_amd/optim.py (`torch.optim.Adam(params, lr, weight_decay)` built at :205 / :353, stepped at :67 / :274, its
 * learning rate moved by the StepLR of :206 / :354).  ONE launch updates every tensor: records [n_tensors][5] int64 = device
 * addresses of parameter, gradient, exp_avg, exp_avg_sq and the element count (fp32 tensors, contiguous, any alignment; a 0
 * gradient address skips the tensor, as torch skips a parameter without .grad); chunk_map [n_chunks][2] int32 = (tensor, chunk
 * within it), one chunk of bgnn_adam_chunk_elems() consecutive elements per block, every chunk of every tensor listed once.
 * step: device int64, the 1-based number of this step; it is read, never written (the caller advances it, inside the same
 * captured graph if there is one).  lr_table: device fp64 [lr_len], the rate of step s is lr_table[min(s, lr_len) - 1].
 * Arithmetic of torch's _single_tensor_adam (amsgrad=False, maximize=False, L2 weight decay added to the gradient, eps added after
 * the bias-corrected square root); bias corrections in fp64 from the step.  No atomics, no scratch, nothing to clear: safe
 * inside a captured HIP graph, where only the addresses are baked in.                                                        */
int64_t bgnn_adam_chunk_elems(void);
int bgnn_adam_step_f32(const void* records, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks, const int64_t* step,
                       const double* lr_table, int64_t lr_len, double beta1, double beta2, double eps, double weight_decay,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Edge-validity filters of step 1    main_bridged_graph.py:123-161 (within a domain), :225-264 (across domains)
 * quantile:   replaces `e_sim.quantile(q)` (:135, :238): torch.quantile's linear interpolation (the order statistics floor / ceil of
 *             q (n - 1), then its lerp) by radix selection over the order-preserving uint32 image of the values, four histogram
 *             passes, no sort.  1 <= n <= 2^31 - 1 (torch stops at 2^24); the position is formed in fp32 as torch forms it while
 *             n - 1 <= 2^24 and in fp64 beyond.  -0 and +0 are one value, returned as +0.  NaN input is out of contract.  out:
 *             one device float; no host synchronisation; two calls are bitwise equal.  ws: 8-byte aligned.
 * inv_norms:  out[i] = 1 / max(|x_i|_2, eps) for a contiguous [N, F] table, any F (what F.cosine_similarity divides a row by,
 *             :149, :252).
 * validity:   replaces :140-150 / :243-253 and the [E, F] gathers of :149 / :252.  edge_index [2, E] int64 (row 0 = `from`, an index
 *             into the *_from tables; row 1 = `to`, an index into the *_to tables; any order, a list sorted by row 0 is gathered
 *             faster); per node: feature row, inverse norm, argmax class, label (-1 = none), and for `to` nodes the train mask.
 *             within = 0: the cross-domain rules (:243-253), within = 1: the single-domain rules (:140-150; pass the same tables
 *             twice).  flags [E]: bit 1 = wrong prediction at `from`, bit 2 = wrong prediction at `to`, bit 3 = predictions
 *             differ, bit 4 = dot . inv_from . inv_to < thres_feat_sim (fp32).  idx_mat / e_sim_mat [n_to, k] (optional): the top-k
 *             tables the list was made from; sim_out[e] = e_sim_mat[to, position of `from` in idx_mat[to]].  counts [8] int64 is
 *             cleared; counts[5] = edges not found in idx_mat, counts[6] = edges with an index outside the tables (flagged, never
 *             dereferenced).
 * rule1:      replaces :136 / :239 and the prints of :138-152 / :241-255: flags[e] |= 1 where sim[e] < *thres (device scalar);
 *             counts[r] += edges with any of bits 0..r set, r = 0..4.                                                           */
size_t bgnn_quantile_workspace_bytes(int64_t n);
int bgnn_quantile_f32(const float* values, int64_t n, double q, float* out, void* ws, size_t ws_bytes, void* stream);
int bgnn_row_inv_norms_f32(const float* x, int64_t N, int32_t F, float eps, float* out, void* stream);
int bgnn_edge_validity_f32(const int64_t* edge_index, int64_t E, const float* x_from, int64_t n_from, const float* inv_from,
                           const int32_t* pred_from, const int32_t* y_from, const float* x_to, int64_t n_to, const float* inv_to,
                           const int32_t* pred_to, const int32_t* y_to, const uint8_t* train_to, int32_t F, int within,
                           float thres_feat_sim, const int64_t* idx_mat_opt, const float* e_sim_mat_opt, int32_t k,
                           float* sim_out_opt, uint8_t* flags, long long* counts, void* stream);
int bgnn_edge_rule1_counts_f32(const float* sim, const float* thres, int64_t E, uint8_t* flags, long long* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_H_ */
