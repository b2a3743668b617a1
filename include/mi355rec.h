/* mi355rec.h -- C ABI of libmi355rec.so: the MI355X (gfx950) embedding + feature-interaction engine.
 *
 * Drop-in boundary.  The reference (PatrickHwang/Explicit-tf2-Recommendation) is pure Python/TF2 and has
 * no FFI of its own; its boundary for this path is the Keras `Layer.__call__` protocol of
 * 2.FM/CustomLayers.py, 3.DCN/CustomLayers.py, 5.DIN/CustomLayers.py as driven by
 * 2.FM/ModelManager.py:87-96,171-181.  Each entry point below replaces the TF op sequence cited next to
 * it; the Python mirror of the Layer classes
 * (explicit-tf2-recommendation_amd/layers.py) is the only caller.
 *
 * This file is also what the Python side is generated from: explicit-tf2-recommendation_amd/_lib.py reads it at import
 * and derives the ctypes signature of every prototype `ret rec_name(args);`, the fields of struct rec_deepfm_lazy_adam
 * and the two tables of constants.  Every `#define REC_<NAME> <integer>` goes to LIMITS: the status codes and the shape
 * limits and launch caps of every kernel family, which the kernel files and the guards of ops.py both take from here.
 * The enumerators of every `enum { ... }` go to ENUMS: the operation codes (REC_ACT_*, REC_EPI_*, REC_DACT_*) and the
 * mode codes (REC_FIBINET_TYPE_*, REC_AUTOINT_RES_*, REC_DIEN_*, REC_SDIM_MODE_*), which the kernels switch on and
 * ops.py binds its names to.  There is no second table to keep in step; the price is a
 * closed set of type spellings, and anything else fails the import and names the declaration:
 *   int, int32_t, int64_t, float, double, size_t by value (with or without a leading const);
 *   a pointer, at any depth and constness, to one of those or to void;  const rec_deepfm_lazy_adam*.
 * Every parameter is named, a prototype without parameters is written (void), and struct fields are plain declarator
 * lists (`float *m, *v; int64_t ld;`).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - all matrices are dense row-major fp32, index tensors are int64 (as the reference's Inputs are,
 *     2.FM/ModelManager.py:92);
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (no allocation, no
 *     synchronisation, graph-capture safe); inputs are borrowed for the duration of the enqueued work;
 *   - return value: 0 ok, <0 argument error (REC_E_*), >0 a hipError_t from the launch;
 *   - `oob_flag` (optional int32*): kernels never read outside a table -- an id outside [0,V) contributes
 *     a zero row and sets *oob_flag = 1, which the Python layer turns into IndexError (the reference
 *     raises InvalidArgumentError on CPU, aliased wrapError at 2.FM/CustomLayers.py:8).
 */
#ifndef MI355REC_H
#define MI355REC_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REC_OK 0
#define REC_E_ARG (-1)
#define REC_E_UNSUPPORTED (-2)
#define REC_E_WORKSPACE (-3)

#define REC_MAX_COLS 128

/* Shape limits of the kernel families: the largest value of each size the entry points accept (beyond it
 * REC_E_UNSUPPORTED, and 0 from the family's rec_*_workspace_bytes).  The kernel files size their arrays and write their
 * checks with these, and ops.py builds its guards and messages from the same values. */
/* AFM (csrc/afm.hip): fields, embedding width, attention width */
#define REC_AFM_MAX_F 64
#define REC_AFM_MAX_E 64
#define REC_AFM_MAX_A 16
/* AutoInt (csrc/autoint.hip): fields (categorical + continuous), embedding width */
#define REC_AUTOINT_MAX_F 64
#define REC_AUTOINT_MAX_E 64
/* FiBiNet (csrc/fibinet.hip): fields, embedding width, continuous features */
#define REC_FIBINET_MAX_F 32
#define REC_FIBINET_MAX_E 64
#define REC_FIBINET_MAX_C 64
/* CIN of xDeepFM (csrc/cin.hip): fields, embedding width, layers, units of a layer */
#define REC_CIN_MAX_F 64
#define REC_CIN_MAX_E 64
#define REC_CIN_MAX_L 8
#define REC_CIN_MAX_H 256
/* field-conv stacks, CCPM and FGCNN alike (csrc/field_conv.h): fields, embedding width, layers, filters, kernel width */
#define REC_FIELD_CONV_MAX_F 64
#define REC_FIELD_CONV_MAX_E 64
#define REC_FIELD_CONV_MAX_L 3
#define REC_FIELD_CONV_MAX_C 16
#define REC_FIELD_CONV_MAX_KW 8
/* ... the workgroups (= workspace slots) of their backward: beyond it a workgroup takes a second tile */
#define REC_FIELD_CONV_BWD_GRID 1024
/* FGCNN (csrc/fgcnn.hip): pooling width */
#define REC_FGCNN_MAX_PW 8
/* MaskNet (csrc/masknet.hip): fields, embedding width; a mask block's x_emb, guided and output widths, reduction rate */
#define REC_MASKNET_MAX_F 64
#define REC_MASKNET_MAX_E 64
#define REC_MASKNET_MAX_D 512
#define REC_MASKNET_MAX_P 512
#define REC_MASKNET_MAX_O 128
#define REC_MASKNET_MAX_R 4
/* DIN attention (csrc/din.hip), forward and backward alike: key width D = E C, hidden units H; beyond D = WIDE_D only
 * H <= WIDE_MAX_H (the backward keeps Eff, the key slabs and the gpre slabs of a workgroup in the LDS of one CU) */
#define REC_DIN_MAX_D 256
#define REC_DIN_MAX_H 64
#define REC_DIN_WIDE_D 128
#define REC_DIN_WIDE_MAX_H 48
/* capsule routing, MIND and ComiRec alike (csrc/capsule.h): routing rounds.  Their key and capsule widths are
 * REC_DIN_MAX_D and their capsules REC_AFM_MAX_A, as SINE's and DMR's widths are */
#define REC_CAPSULE_MAX_R 8
/* SINE (csrc/sine.hip): concepts of the pool; width of a pool row of the aux kernels */
#define REC_SINE_MAX_L 1024
#define REC_SINE_AUX_MAX_D 256
/* CAN (csrc/can.hip): layers of the micro-MLP, and orders alike (its widest layer is REC_AFM_MAX_E) */
#define REC_CAN_MAX_L 4
/* series search, SIM, ETA and SDIM alike (csrc/sim.hip, csrc/eta.hip, csrc/sdim.hip): key width D = E C; selected
 * positions K, which are also the keys of the ESU attention */
#define REC_SEARCH_MAX_D 256
#define REC_SEARCH_MAX_K 16
/* ESU attention (csrc/sim.hip): width of the query and key rows D and of a head dk alike, heads */
#define REC_ESU_MAX_D 64
#define REC_ESU_MAX_H 8
/* ETA (csrc/eta.hip): hash bits */
#define REC_ETA_MAX_M 32
/* SDIM (csrc/sdim.hip): hash bits of all groups together G m, candidates of an example */
#define REC_SDIM_MAX_BITS 32
#define REC_SDIM_MAX_S 16
/* Launch caps: the most dynamic LDS, in bytes, a launch of these kernels asks for; a shape whose LDS formula (given
 * with each family below) passes it is REC_E_UNSUPPORTED.
 * 150 KiB: the one-example and one-tile kernels of MIND, ComiRec, SINE, CAN, DMR, DIEN, the ESU and DIN attentions */
#define REC_TILE_LDS_CAP 153600
/* 156 KiB: the 32-example tiles of POSO-MLP, PLE, MMOE and ContextNet */
#define REC_POSO_LDS_CAP 159744
/* 64 KiB: the series searches of SIM, ETA and SDIM */
#define REC_SEARCH_LDS_CAP 65536

/* activation kinds shared by the dense entry points */
enum { REC_ACT_NONE = 0, REC_ACT_RELU = 1, REC_ACT_SIGMOID = 2, REC_ACT_TANH = 3 };

/* mode codes of the families that take one: `type` of rec_fibinet_* and rec_fibinetplus_*, `res` of rec_autoint_*,
 * `mode` of rec_dien_augru_* (the GRU of rec_dien_gru_* is the same cell's mode 0) and `mode` of rec_sdim_interest_* */
enum { REC_FIBINET_TYPE_ALL = 0, REC_FIBINET_TYPE_EACH = 1, REC_FIBINET_TYPE_INTERACTION = 2 };
enum { REC_AUTOINT_RES_NONE = 0, REC_AUTOINT_RES_ADD = 1, REC_AUTOINT_RES_LEARNED = 2 };
enum { REC_DIEN_GRU = 0, REC_DIEN_AUGRU = 1, REC_DIEN_AGRU = 2 };
enum { REC_SDIM_MODE_REFERENCE = 0, REC_SDIM_MODE_VALID = 1 };

/* epilogues of rec_gemm_f32 */
enum {
  REC_EPI_NONE = 0,      /* C = A.B                                   */
  REC_EPI_BIAS = 1,      /* C = A.B + bias[n]                          */
  REC_EPI_BIAS_RELU = 2, /* C = relu(A.B + bias[n])                    */
  REC_EPI_BIAS_SIGMOID = 3,
  REC_EPI_BIAS_TANH = 4,
  REC_EPI_CROSS = 5,     /* C = e0[m,n] * (A.B + bias[n]) + e1[m,n]    (MatrixCrossLayer, 3.DCN/CustomLayers.py:301-303) */
  REC_EPI_ADD = 6        /* C = A.B + e1[m,n]                          */
};

int rec_version(void);

/* ---- K1  index assembly: expand_dims + concat(axis=1) of F int64 columns (2.FM/CustomLayers.py:138-144).
 * cols_host: HOST array of F device pointers, each a column of `rows` int64 (a [B,1] or [B] tensor; for the
 * DIN series stack, 5.DIN/CustomLayers.py:258, a [B,T] tensor with rows = B*T).  Writes X[r*ldx + col0 + f]. */
int rec_index_pack_i64(const int64_t* const* cols_host, int F, int64_t rows, int64_t* X, int64_t ldx,
                       int64_t col0, void* stream);

/* Staging of input batches for the compiled train loop (2.FM/ModelManager.py:183-199 iterates a tf.data pipeline; here
 * the batches of a chunk of steps are copied into fixed device buffers so that the captured step sees constant addresses):
 * n device arrays of bytes_each bytes (a multiple of 4) -> out[s * bytes_each ...], one launch.  srcs_host: HOST array of
 * n device pointers. */
int rec_block_copy(const void* const* srcs_host, int n, int64_t bytes_each, void* out, void* stream);
/* tf.keras.metrics.AUC(num_thresholds) / Mean(loss) accumulated on the device (2.FM/ModelManager.py:106-107,180-181):
 * hist [2][n_thresholds + 1] int64 += examples per (label > 0.5, number of thresholds strictly below the prediction);
 * *loss_acc (double) += the n_steps per-step losses.  Integer atomics: exact and order-independent. */
int rec_auc_hist_update_f32(const float* prob, const float* label, int64_t n, const float* thresholds, int n_thresholds,
                            int64_t* hist, const float* loss_steps, int n_steps, double* loss_acc, void* stream);

/* Tables: row-major fp32 with a row stride `ld` >= E floats (dense table: ld = E).  The FM-family layers keep
 * `embed` [V,E] and `w` [V,1] of one id in ONE 128-byte line -- fused layout, row = [embed(E) | w | pad] with
 * ld = next_pow2(E+1) >= 16, passed as embed = base, w = base + E, ld_e = ld_w = ld -- because a random row
 * read costs one 128-B line request whatever its size (measured), so the first-order weight is free.
 *
 * ---- K2  Embedding(V,E)(X) -> gather (2.FM/CustomLayers.py:129-134,146-147).  out[i,:] = table[idx[i],:]. */
int rec_emb_gather_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* idx, int64_t n,
                       float* out, int* oob_flag, void* stream);

/* ---- K2+K3 fused: w(X), embed(X), reduce_sum / square / subtract / 0.5*reduce_sum
 * (2.FM/CustomLayers.py:146-153, 289-297).  z[b] = bias + sum_f w[X[b,f]] + 0.5*sum_d(S_d^2 - sum_f e_fd^2).
 * Optional outputs (NULL to skip): prob[b] = sigmoid(z[b]) (FMRankingLayer, :155); emb_out [B,F,E] (the
 * Flatten() input of DeepFM's DNN part, :300); sumvec [B,E] = S (saved for backward). */
int rec_emb_fm_fwd_f32(const float* embed, int64_t ld_e, const float* w, int64_t ld_w, const float* bias,
                       int64_t V, int E, const int64_t* idx, int64_t B, int F, float* z, float* prob,
                       float* emb_out, float* sumvec, int* oob_flag, void* stream);

/* ---- K4 (values): GradientTape gradient of the FM part w.r.t. the gathered rows, as the IndexedSlices
 * values TF produces (2.FM/ModelManager.py:176-177): dvals[b,f,:] = gz[b]*(S[b,:] - e[b,f,:]) + extra[b,f,:].
 * emb_rows (optional): the rows saved by the forward; NULL -> re-gather from `embed`.  extra (optional):
 * gradient arriving through the DNN part. */
int rec_emb_fm_bwd_vals_f32(const float* embed, int64_t ld_e, int64_t V, int E, const int64_t* idx, int64_t B,
                            int F, const float* gz, const float* sumvec, const float* emb_rows,
                            const float* extra, float* dvals, void* stream);

/* ---- K4 (de-duplication): what Keras' optimizer does to an IndexedSlices gradient before applying it
 * (tf.unique + unsorted_segment_sum); here ids come out ASCENDING and rows of one id are added in a fixed
 * order, so results are run-to-run bit-identical.
 * plan: ids[n] -> uniq_ids[n] (first *n_uniq valid, ascending; the tail is padded with uniq_ids[0]),
 *       seg_start[n+1] (row range of each unique id in the sorted order; empty for the tail),
 *       perm[n] (sorted position -> original position), n_uniq (device int64). */
size_t rec_dedup_workspace_bytes(int64_t n);
int rec_dedup_plan_i64(const int64_t* ids, int64_t n, int64_t V, int64_t* uniq_ids, int32_t* seg_start,
                       int32_t* perm, int64_t* n_uniq, void* workspace, size_t workspace_bytes,
                       void* stream);
/* out[u,:] = sum over s in [seg_start[u], seg_start[u+1]) of vals[perm[s] / row_div, :]   for u in [0,n).
 * row_div = 1 for per-lookup values; row_div = F broadcasts a per-example value (the w table, whose
 * per-lookup gradient is gz[b]).  E <= 256 goes through chunk partials (long runs are finished by a whole workgroup);
 * E > 256 (CAN's induction rows) takes one workgroup per output row, a thread per column and every 256th after it, the
 * rows of a run added in sorted order, and does not touch the workspace. */
/* Same outputs as rec_dedup_plan_i64 for ids that arrive as n_lists ascending, duplicate-free lists laid end to end
 * (list_counts [n_lists], int64, on the device; their sum must be n): the owner-side union of what P requesters
 * send after de-duplicating their own batches.  Rank merge by binary search instead of a sort; rows of one id are
 * summed in list order.  workspace: rec_dedup_workspace_bytes(n). */
int rec_dedup_plan_sorted_lists_i64(const int64_t* ids, int64_t n, const int64_t* list_counts, int n_lists,
                                    int64_t V, int64_t* uniq_ids, int32_t* seg_start, int32_t* perm,
                                    int64_t* n_uniq, void* workspace, size_t workspace_bytes, void* stream);
size_t rec_segment_sum_workspace_bytes(int64_t n, int E);
int rec_segment_sum_f32(const float* vals, int E, const int32_t* perm, const int32_t* seg_start, int64_t n,
                        int32_t row_div, float* out, float* workspace, void* stream);

/* ---- K5/K6  dense: C[M,N] = epi(op(A).op(B)), fp32-exact MFMA (v_mfma_f32_32x32x2_f32).
 * op(A) is [M,K]: transA=0 -> A stored [M,K] (lda), transA=1 -> A stored [K,M].  op(B) is [K,N]:
 * transB=0 -> B stored [K,N], transB=1 -> B stored [N,K].  MatMul+BiasAdd+activation of MLPLayer
 * (2.FM/CustomLayers.py:74-81), Keras Dense (3.DCN/CustomLayers.py:158-167), MatrixCrossLayer
 * (3.DCN/CustomLayers.py:301-303, REC_EPI_CROSS with e0=x0, e1=x_l) and their backward GEMMs.
 * split_k > 1 needs workspace of split_k*M*N floats (partials are summed in a fixed order).
 * aux (optional, REC_EPI_CROSS only, leading dimension ldc): receives U = A.B + bias, kept for the backward pass. */
int rec_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                 const float* B, int64_t ldb, float* C, int64_t ldc, int epilogue, const float* bias,
                 const float* e0, int64_t lde0, const float* e1, int64_t lde1, int split_k,
                 float* workspace, float* aux, void* stream);

/* ---- K6 backward, elementwise part of one MatrixCrossLayer layer: h = g*x0 ; gx0 = (accumulate ? gx0 : 0) + g*u
 * (H = G (.) X0 feeds the dW and dX GEMMs; dX0 += G (.) U_l).  n = B*D. */
int rec_crossnet_mat_bwd_elem_f32(const float* g, const float* x0, const float* u, float* h, float* gx0,
                                  int accumulate, int64_t n, void* stream);

/* elementwise helpers of the dense forward / backward */
/* y = act(x + x2)  (x2 optional; tf.nn.sigmoid(fm_part + dnn_part), 2.FM/CustomLayers.py:155,305) */
int rec_act_fwd_f32(int act, const float* x, const float* x2, float* y, int64_t n, void* stream);
/* dpre = dpost * act'(post)   (in place allowed) */
int rec_act_bwd_f32(int act, const float* post, const float* dpost, float* dpre, int64_t n, void* stream);
/* out[j] = sum_i X[i,j]  (bias gradients), deterministic two-stage sum; workspace of
 * rec_colsum_workspace_bytes(M,N) bytes. */
size_t rec_colsum_workspace_bytes(int64_t M, int64_t N);
int rec_colsum_f32(const float* X, int64_t M, int64_t N, int64_t ldx, float* out, float* workspace, void* stream);
/* The same in ONE launch: `counters` = ceil(N/32) ints that are ZERO on entry and zero again on exit (the workgroup that
 * arrives last at a column block's counter adds the partials of all row blocks, in the fixed order of the two-stage
 * form: bit-identical results).  Calls that share counters must not run concurrently. */
int rec_colsum_fused_f32(const float* X, int64_t M, int64_t N, int64_t ldx, float* out, float* workspace, int* counters,
                         void* stream);
/* y = a*x + b*y over n elements */
int rec_axpby_f32(float a, const float* x, float b, float* y, int64_t n, void* stream);
/* dst[r, c0:c0+w] = src[r, 0:w]   (concat / split along the feature axis) */
int rec_copy_cols_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int64_t w,
                      void* stream);

/* ---- K7  CrossLayer, vector mode (3.DCN/CustomLayers.py:195-203): x_{l+1} = x0*(x_l.w_l) + b_l + x_l.
 * w, b: [L,D].  xs (optional) saves x_0..x_{L-1} as [L,B,D] for backward.  y [B,D]. */
int rec_crossnet_vec_fwd_f32(const float* x0, int64_t B, int D, int L, const float* w, const float* b,
                             float* y, float* xs, void* stream);
/* gx0 [B,D], dw [L,D], db [L,D]; workspace: rec_crossnet_vec_bwd_workspace_bytes(B,D,L). */
size_t rec_crossnet_vec_bwd_workspace_bytes(int64_t B, int D, int L);
int rec_crossnet_vec_bwd_f32(const float* x0, int64_t B, int D, int L, const float* w, const float* xs,
                             const float* gy, float* gx0, float* dw, float* db, void* workspace,
                             void* stream);

/* ---- K10  two-tower score (2.FM/CustomLayers.py:233-234): out[b] = (1 - cos(u_b, i_b))/2,
 * l2norm = x*rsqrt(max(sum x^2, 1e-12)). */
int rec_cosine_fwd_f32(const float* u, const float* i, int64_t B, int d, float* out, void* stream);
int rec_cosine_bwd_f32(const float* u, const float* i, int64_t B, int d, const float* gout, float* gu,
                       float* gi, void* stream);

/* ---- K11  reduce_sum(BinaryCrossentropy()(y, p)) and its gradient (2.FM/ModelManager.py:100,175).
 * p: probabilities [n]; y: labels [n].  loss (device scalar) = mean of -(y log(clip(p)+eps) +
 * (1-y) log(1-clip(p)+eps)), eps = 1e-7.  dp (optional) = dL/dp; dz (optional) = dL/dp * p(1-p) (sigmoid head). */
int rec_bce_fwd_bwd_f32(const float* y, const float* p, int64_t n, float* loss, float* dp, float* dz,
                        void* stream);

/* ---- K12  Keras Adam (2.FM/ModelManager.py:104,178-179).  t = 1-based step.
 * dense: m += (g-m)(1-b1); v += (g*g-v)(1-b2); var -= lr_t*m/(sqrt(v)+eps). */
int rec_adam_dense_f32(float* var, float* m, float* v, const float* g, int64_t n, int64_t t, float lr,
                       float b1, float b2, float eps, void* stream);
/* Keras' bias-corrected step size lr * sqrt(1 - b2^t) / (1 - b1^t) in float32 as the entry points above compute it from
 * (t, lr, b1, b2) -- for a caller that keeps the values of steps 1..n in a device table (beyond it the corrections are
 * 1 in float32: b2^t < 2^-24). */
float rec_adam_lr_t_f32(float lr, float b1, float b2, int64_t t);
/* rec_adam_dense_f32 on up to 16 parameters in ONE launch, step size read from device memory (host arrays of device
 * pointers, copied into the kernel arguments). */
int rec_adam_dense_multi_f32(int n_tensors, float* const* var, float* const* m, float* const* v, const float* const* g,
                             const int64_t* numel, const float* lr_t_dev, float b1, float b2, float eps, void* stream);
/* Keras sparse apply = DENSE SWEEP: m*=b1, v*=b2 on all V rows, m[ids]+=(1-b1)g, v[ids]+=(1-b2)g^2, then
 * var -= lr_t*m/(sqrt(v)+eps) on all V rows.  (uniq_ids, g_rows, n_uniq) as produced by the dedup above
 * (cap = allocated rows of uniq_ids/g_rows).  var has row stride ld; m, v are dense [V,E].
 * side: workspace of cap*3*E floats. */
int rec_adam_sparse_keras_f32(float* var, int64_t ld, float* m, float* v, int64_t V, int E,
                              const int64_t* uniq_ids, const float* g_rows, const int64_t* n_uniq, int64_t cap,
                              float* side, int64_t t, float lr, float b1, float b2, float eps, void* stream);
/* The same Keras sparse apply for BOTH tables of an FM-family layer that share the fused rows [embed(E) | w | pad]
 * (fused = row 0 of the [V,ld] array; w = fused + E): one sweep over the lines instead of two -- swept on its own, w
 * costs a full 128-byte line read + write per row.  Elementwise identical to two rec_adam_sparse_keras_f32 calls.
 * side_e [cap,3,E], side_w [cap,3,1]. */
int rec_adam_sparse_keras_pair_f32(float* fused, int64_t ld, float* m_e, float* v_e, float* m_w, float* v_w, int64_t V,
                                   int E, const int64_t* uniq_ids, const float* g_e_rows, const float* g_w_rows,
                                   const int64_t* n_uniq, int64_t cap, float* side_e, float* side_w, int64_t t,
                                   float lr, float b1, float b2, float eps, void* stream);

/* 'lazy' variant (NOT reference semantics): only the touched rows decay and move. */
int rec_adam_rows_f32(float* var, int64_t ld, float* m, float* v, int64_t V, int E, const int64_t* uniq_ids,
                      const float* g_rows, const int64_t* n_uniq, int64_t cap, int64_t t, float lr,
                      float b1, float b2, float eps, void* stream);

/* ---- L2 on the embedding rows a batch used (5.DIN/ModelManager.py:176-190):
 * loss = factor * l2_loss(table[uniq_ids[0..n_uniq)]) with l2_loss(x) = sum(x^2)/2; rows_out [n,E] = its gradient
 * factor * table[uniq_ids[u]] (zero rows on the padded tail u >= n_uniq).  uniq_ids / n_uniq: a rec_dedup_plan. */
size_t rec_l2_rows_workspace_bytes(int64_t n, int E);
int rec_l2_rows_f32(const float* table, int64_t ld, int64_t V, int E, const int64_t* uniq_ids, const int64_t* n_uniq,
                    int64_t n, float factor, float* rows_out, float* loss, float* workspace, void* stream);

/* ---- retrieval after the DSSM towers (2.FM/OfflineLoader.py:129-162, 2.FM/OnlineServer.py:53-75:
 * item vectors L2-normalised, sklearn BallTree(Euclidean).query(raw user vector, k) -- an exact search, i.e. the k
 * smallest ||u - i_hat||_2 ascending).  rec_l2_normalize_rows_f32: y[r,:] = x[r,:] / ||x[r,:]||_2.
 * rec_topk_l2_f32: out_idx [nq,k] (int64, item row numbers; equal distances: the lower index first), out_dist [nq,k]
 * ascending; k <= 64, d <= 64; if n < k the tail is (-1, +inf).  workspace: rec_topk_l2_workspace_bytes(nq, n, k). */
int rec_l2_normalize_rows_f32(const float* x, int64_t n, int d, int64_t ld_in, float* y, int64_t ld_out, void* stream);
size_t rec_topk_l2_workspace_bytes(int64_t nq, int64_t n, int k);
int rec_topk_l2_f32(const float* queries, int64_t nq, int d, int64_t ldq, const float* items, int64_t n, int64_t ldi,
                    int k, int64_t* out_idx, float* out_dist, void* workspace, size_t workspace_bytes, void* stream);

/* ---- (e) row-wise block sharding of a table (no reference counterpart).
 * owner = id / rows_per_shard.  perm[n]: positions grouped by owner, ascending inside a group;
 * send_counts[n_shard] (int64); local_ids[n] = ids[perm] - owner*rows_per_shard. */
size_t rec_shard_bucketize_workspace_bytes(int64_t n, int n_shard);
int rec_shard_bucketize_i64(const int64_t* ids, int64_t n, int64_t rows_per_shard, int n_shard,
                            int64_t* perm, int64_t* send_counts, int64_t* local_ids, int* oob_flag,
                            void* workspace, size_t workspace_bytes, void* stream);
/* De-duplicate-first exchange plan on top of rec_colsort_plan_i64 (columns own ascending id ranges => the batch's
 * unique ids, column after column, are globally ascending and grouped by owner): uidx [F,B] = compact index of every
 * lookup's id in that list (the fused kernel gathers the exchanged rows by it), uid_local [B*F] = id - owner *
 * rows_per_shard (first *n_uniq valid), send_counts [n_shard] (int64) = unique ids per owner. */
int rec_colsort_shard_map_i64(const int32_t* perm, const int64_t* col_uid, const int32_t* col_seg,
                              const int32_t* col_nu, int64_t B, int F, int64_t rows_per_shard, int n_shard,
                              int64_t* uid_local, int64_t* uidx, int64_t* send_counts, int64_t* n_uniq,
                              int* oob_flag, void* stream);
/* The same plan for FIXED-CAPACITY exchanges (constant split sizes: no count exchange, no host read; the whole sharded
 * step can be captured in a hipGraph).  Every owner has a slab of `cap` slots; cap >= the unique ids one batch can hold
 * for one owner = sum over the fields that intersect the owner's block of min(B, overlap) (else *oob_flag is set).
 * msg [n_shard, 2 + cap] int64: word 0 = unique ids for this owner, word 1 = 0, then the owner-local ids, ascending;
 * uidx [F,B] = owner * cap + j (row of the lookup in the [n_shard * cap, .] buffer the rows come back in);
 * slot_map [B*F] int32 (first *n_uniq valid): rank in the batch's ascending unique list -> owner * cap + j. */
int rec_colsort_shard_map_fixed_i64(const int32_t* perm, const int64_t* col_uid, const int32_t* col_seg,
                                    const int32_t* col_nu, int64_t B, int F, int64_t rows_per_shard, int n_shard,
                                    int64_t cap, int64_t* msg, int64_t* uidx, int32_t* slot_map, int64_t* n_uniq,
                                    int* oob_flag, void* stream);
/* The same kind of plan for a GENERIC lookup (any id list, any layer): on top of rec_dedup_plan_i64 of the flat ids
 * (uniq_ids ascending = grouped by owner under the block partition, seg_start, perm, *n_uniq on the device).
 * msg [n_shard, 2 + cap] as above (words beyond an owner's count are left alone: the caller keeps them zero);
 * slot [n] int64: row of every lookup in the [n_shard * cap, E] buffer the rows come back in.  *oob_flag is set when an
 * owner's unique ids exceed cap or an id lies outside [0, n_shard * rows_per_shard).
 * uslot [n] int64: the slot of every UNIQUE id (rank u of the plan -> owner * cap + j; ranks >= *n_uniq ->
 * n_shard * cap, one row past the buffer).  The plan of the ids is then also the plan of the slots (slot is monotone in the
 * id), which is what lets the backward of the lookup reuse the forward's de-duplication: segment sums in the plan's order,
 * scattered by uslot, are the dense gradient of the [n_shard * cap, E] rows buffer. */
int rec_shard_slab_map_uslot_i64(const int64_t* uniq_ids, const int64_t* n_uniq, const int32_t* seg_start,
                                 const int32_t* perm, int64_t n, int64_t rows_per_shard, int n_shard, int64_t cap,
                                 int64_t* msg, int64_t* slot, int64_t* uslot, int* oob_flag, void* stream);
/* Owner side of it.  Gather for n_lists received slabs (msg layout above): out [n_lists * cap, E], row (q, j) written
 * only for j < count_q = the first E floats of the table row (E a multiple of 4 up to 256, E <= ld; the sharded
 * DeepFM step sends E = 20 of the 32 floats of a fused row: [embed 16 | w | pad]); 16-byte aligned operands. */
int rec_emb_gather_lists_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* msg, int n_lists,
                             int64_t cap, float* out, int* oob_flag, void* stream);
/* Union of the n_lists ascending duplicate-free lists of such a message (rank merge, no sort) as a segment plan over
 * the [n_lists * cap, .] payload rows: uniq_ids [n_lists*cap], seg_start [n_lists*cap + 1], perm [n_lists*cap] (payload
 * row of every sorted position), *n_uniq; tails padded as rec_dedup_plan_i64 does (valid id, empty runs), so
 * rec_segment_sum_f32(n = n_lists*cap) follows without a host read.  workspace: rec_dedup_workspace_bytes(n_lists*cap). */
int rec_dedup_plan_sorted_slabs_i64(const int64_t* msg, int n_lists, int64_t cap, int64_t V, int64_t* uniq_ids,
                                    int32_t* seg_start, int32_t* perm, int64_t* n_uniq, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* (The post launch of the fused step writes the row gradients into that layout: rec_deepfm_fused_post_f32 with
 * slot_map, below.) */
/* out[perm[i], :] = in[i, :]   (inverse permutation of received rows) and its transpose */
int rec_permute_rows_f32(const float* in, const int64_t* perm, int64_t n, int E, int scatter, float* out,
                         void* stream);

/* ---- Fused DeepFM train step (2.FM/CustomLayers.py:279-308 under 2.FM/ModelManager.py:171-177) for the reference's
 * default head (embedding_dims 16, mlp_dims [32,8]) on the fused 128-byte row layout: a de-duplication plan of the
 * batch's ids, then two launches on the stream -- the main kernel (index assembly from the F feature columns, gather,
 * FM, MLP on fp32 MFMA, sigmoid, Keras BCE and the whole backward) and the post launch (fixed-order reduction of the
 * main kernel's per-workgroup partials side by side with the segment sums of the de-duplicated table gradients).
 * Outputs: gz [B] = dL/dz, vals [B*F,16] = IndexedSlices values of `embed` (the values of `w` are gz[b]), dense
 * gradients, loss (device scalar, mean BCE), prob [B] (optional), per-unique-id gradient rows.  F <= 28.
 * workspace (main kernel -> post launch): rec_deepfm_fused_workspace_bytes(B, F). */
size_t rec_deepfm_fused_workspace_bytes(int64_t B, int F);

/* Plan.  Uses the DataGenerator contract (2.FM/DataGenerator.py:76-88): column f only holds ids of
 * [col_lo[f], col_lo[f] + 2^key_bits) and columns are given in ascending range order, so duplicates occur only inside
 * a column and each column (B <= 16384 ids; max_key = largest id - col_lo over all columns, bits(max_key) +
 * ceil(log2 B) <= 32) is sorted on its own (one workgroup per column: LDS radix sort + run detection; up to 256 columns
 * per call, so one call may plan several batches).
 * perm [F,B], col_uid [F,B], col_seg [F,B+1], col_nu [F]; an id outside its column's range sets *bad_flag. */
size_t rec_colsort_workspace_bytes(int64_t B, int F);
/* Radix passes of that sort for a batch of B and a largest key max_key: *passes passes of at most *digit_bits bits
 * (<= 10) over the key; the status the plan calls return for (B, max_key) otherwise. */
int rec_colsort_digits(int64_t B, int64_t max_key, int* passes, int* digit_bits);
/* Bitmap path of that sort (columns without a hot bucket are ranked through an LDS bitmap of the launch's key range
 * instead of being sorted): *words = 32-bit bitmap words a launch of (B, max_key) uses = ceil((max_key + 1) / 32), or 0
 * when the launch does not take the path (B > 8192, or a key range beyond 425,984 keys); *slow_cap = the most lookups
 * of a column that may share a 32-key word with a duplicated id (a column with more takes the bucket path).  Statuses
 * as rec_colsort_digits. */
int rec_colsort_bitmap_limits(int64_t B, int64_t max_key, int* words, int* slow_cap);
int rec_colsort_plan_i64(const int64_t* const* cols_host, int F, int64_t B, int64_t V, const int64_t* col_lo,
                         int64_t max_key, int32_t* perm, int64_t* col_uid, int32_t* col_seg, int32_t* col_nu,
                         int* bad_flag, void* workspace, void* stream);
/* The same plan plus its inverse view: dloc [F,B] (int32) = for lookup (column f, example b) the index of its run of
 * equal ids inside the column (0 .. col_nu[f]-1), with the sign bit set unless the lookup is the FIRST member of the run
 * (smallest example index).  What the direct mode of the fused step needs to write value rows straight to their
 * de-duplicated slot (global slot = runs of the columns before + the run index). */
int rec_colsort_plan_dest_i64(const int64_t* const* cols_host, int F, int64_t B, int64_t V, const int64_t* col_lo,
                              int64_t max_key, int32_t* perm, int64_t* col_uid, int32_t* col_seg, int32_t* col_nu,
                              int32_t* dloc, int* bad_flag, void* workspace, void* stream);

/* Main launch (csrc/deepfm_fused3.hip): the two 16-example halves of a workgroup run one phase apart (the backward of
 * one half on the matrix cores while the rows of the other are still landing).  weights: HOST array of 8 device
 * pointers bias, K0 [F*16,32], K0T, b0, K1 [32,8], b1, K2 [8,1], b2; K0T [32, F*16] = the transpose of K0, kept by the
 * caller with rec_deepfm_k0t_f32 (read only when F > 26: otherwise K0 is staged in LDS).  Two optional groups:
 *   dloc, col_nu, g_embed_rows   all NULL: the plan-after form -- any row stride ld >= 20 that is a multiple of 4 (rows
 *       [embed 16 | w | ...]: 32 for a table, 20 for the rows a sharded step received); the plan may be built after
 *       the launch.  All given: direct mode (ld = 32) -- the plan of the batch (rec_colsort_plan_dest_i64) is complete
 *       before the launch, and the IndexedSlices value row of a lookup that heads its run goes straight to
 *       g_embed_rows[slot] (only the other members of a run are written to vals).  Anything else: REC_E_ARG.
 *   step_dev, lr_table, n_table, lr_t_dev   step_dev NULL: off.  Otherwise the optimizer's device-side step counter is
 *       advanced by the kernel's first thread: *step_dev += 1, *lr_t_dev = lr_table[min(*step_dev, n_table) - 1]
 *       (lr_table: rec_adam_lr_t_f32 of steps 1..n_table).  The kernel reads neither word; the launches behind it on the
 *       stream see the new step, so a train step holds no per-step host scalar and can be captured in a hipGraph. */
int rec_deepfm_k0t_f32(const float* K0, int F, float* K0T, void* stream);
int rec_deepfm_fused3_main_f32(const float* table, int64_t ld, int64_t V, const int64_t* const* cols_host, int F,
                               int64_t B, const float* const* weights, const float* label, float* gz, float* vals,
                               float* prob, int* oob_flag, void* workspace, const int32_t* dloc, const int32_t* col_nu,
                               float* g_embed_rows, int64_t* step_dev, const float* lr_table, int64_t n_table,
                               float* lr_t_dev, void* stream);

/* The lazy (touched-rows) Adam of the post launch (optimizer in the backward; arithmetic of
 * rec_adam_rows_f32), applied to each row of both tables the moment its gradient is final.  table: fused rows [V,32] =
 * [embed 16 | w | pad] (ld = 32).  The step size is read from device memory (lr_t_dev, advanced by the main launch on
 * the same stream).  Row strides of the optimizer state: ld_state (floats) for m_e / v_e, ld_wstate for m_w / v_w -- 16
 * and 1 for dense arrays, 32 and 32 for state packed beside the rows ([m 16 | v 16] as one 128-byte row, m_w / v_w in
 * the padding of the fused table row: a touched row then costs two line requests instead of five or six).
 * last == NULL: plain touched-rows Adam, NOT Keras' dense-sweep semantics of 2.FM/ModelManager.py:104,178-179 (opt-in);
 * last != NULL (then step_dev too): the exact lazy evaluation of Keras' Adam below. */
typedef struct rec_deepfm_lazy_adam {
  float* table; int64_t ld, V;
  float *m_e, *v_e, *m_w, *v_w; int64_t ld_state, ld_wstate;
  const float* lr_t_dev; float b1, b2, eps;
  int32_t* last; const int64_t* step_dev;
} rec_deepfm_lazy_adam;
/* Post launch (csrc/deepfm_fused.hip): reduction of the workgroup partials into the dense gradients (grads: HOST array
 * of 7 device pointers dK0, db0, dK1, db1, dK2, db2, dbias) and *loss, side by side with the segment sums of (vals, gz)
 * over the plan, compacted to the global ascending list: uniq_ids [B*F], g_embed_rows [B*F,16], g_w_rows [B*F], n_uniq;
 * the tail is padded like rec_dedup_plan_i64's.  Replaces the 2.FM/ModelManager.py:176-179 IndexedSlices hand-over.
 *   slot_map != NULL (the sharded step; uniq_ids, g_w_rows, n_uniq NULL): per-unique-id sums written as packed rows
 *       [embed 16 | w | 0 0 0] to g_embed_rows [n_shard * cap, 20] at slot_map[rank]; unused slots are left alone.
 *   direct != 0, after a direct-mode main launch: adds the remaining members of runs longer than one in position order
 *       (sums bit-identical to the plain form), writes uniq_ids / g_w_rows / n_uniq and the zero-padded tail.
 *   adam != NULL (direct only): the lazy Adam above on every finished row.
 * slot_map with direct, adam without direct: REC_E_UNSUPPORTED. */
int rec_deepfm_fused_post_f32(int F, int64_t B, const float* gz, const float* vals, float* const* grads, float* loss,
                              void* workspace, const int32_t* perm, const int64_t* col_uid, const int32_t* col_seg,
                              const int32_t* col_nu, int64_t* uniq_ids, float* g_embed_rows, float* g_w_rows,
                              int64_t* n_uniq, const int32_t* slot_map, int direct, const rec_deepfm_lazy_adam* adam,
                              void* stream);
/* Keras Adam evaluated lazily and exactly (2.FM/ModelManager.py:178-179: the sparse apply of IndexedSlices gradients is
 * a dense sweep over every row).  An untouched row's update at step j depends only on the row and lr_j, so rows may skip
 * the sweeps and replay them later with the sweep's own arithmetic: last [V] int32 = the step each row holds (zero at
 * the start).  rec_adam_keras_catchup_f32 brings the unique rows of a batch's plan (col_uid / col_nu of
 * rec_colsort_plan_dest_i64) up to step *step_dev BEFORE the batch reads them; the post launch above, given `last`,
 * applies the touched update of the step that follows and stamps the rows; rec_adam_keras_flush_f32 brings every row up
 * to date (before the parameters are read from outside).  Rounding is pinned in every Adam kernel of this library, so
 * the tables equal those of rec_adam_sparse_keras_pair_f32 bit for bit.  lr_table: rec_adam_lr_t_f32 of steps 1..n. */
int rec_adam_keras_catchup_f32(const int64_t* col_uid, const int32_t* col_nu, int64_t B, int F, float* table, int64_t ld,
                               int64_t V, float* m_e, float* v_e, int64_t ld_state, float* m_w, float* v_w,
                               int64_t ld_wstate, const int32_t* last, const int64_t* step_dev, const float* lr_table,
                               int64_t n_table, float b1, float b2, float eps, void* stream);
int rec_adam_keras_flush_f32(float* table, int64_t ld, int64_t V, float* m_e, float* v_e, int64_t ld_state, float* m_w,
                             float* v_w, int64_t ld_wstate, int32_t* last, const int64_t* step_dev, const float* lr_table,
                             int64_t n_table, float b1, float b2, float eps, void* stream);

/* ---- Fused DSSM two-tower train step (2.FM/CustomLayers.py:208-239 under 2.FM/ModelManager.py:171-177) for the
 * widths mlp_dims [64,32], final_dim 8 (h1, h2, d_out; anything else: REC_E_UNSUPPORTED), E in {8,16,32,64} shared by
 * both towers, 1 <= F_u, F_i <= 8 (csrc/dssm_fused.hip).  Two launches:
 *   main: gather of ids [B,F] (row-major, 64-bit row offsets into table[V, ld], ld >= E a multiple of 4, table 16-byte
 *         aligned; an id outside [0,V) reads a zero row, gets a zero gradient row and sets *oob_flag), both tower MLPs
 *         on fp32 MFMA, score (1 - cos)/2, Keras BCE (mean over B) and the whole backward.  Writes the per-lookup
 *         gradient rows u_vals [B*F_u,E] / i_vals [B*F_i,E] and per-workgroup dense partials + loss terms into the
 *         workspace; user_emb / item_emb [B,8] and score [B] when non-null.  weights: host array of 12 device pointers
 *         (user tower K0 [F_u*E,64], b0, K1 [64,32], b1, Kf [32,8], bf, then the item tower's).  step_dev != NULL: the
 *         optimizer's device-side step counter is advanced as in rec_deepfm_fused3_main_f32.
 *   post: fixed-order reduction of the partials into grads (host array of 12 device pointers, order of `weights`) and
 *         *loss, side by side with the segment sums of u_vals / i_vals over a rec_dedup_plan_i64 of each tower's flat
 *         ids (perm, seg_start, uniq_ids, n_uniq) -> u_rows [B*F_u,E] / i_rows [B*F_i,E] (zero on the padded tail).
 *         adam != NULL (host array: u_table, u_m, u_v, i_table, i_m, i_v; m / v dense [V,E]): the touched-rows Adam update
 *         of rec_adam_rows_f32 on every unique row, step size *lr_t_dev.
 * No float atomics: bit-identical results run to run.  workspace: rec_dssm_fused_workspace_bytes (0: unsupported). */
size_t rec_dssm_fused_workspace_bytes(int64_t B, int E, int F_u, int F_i);
int rec_dssm_fused_main_f32(const float* u_table, int64_t u_ld, int64_t u_V, const int64_t* u_ids, int F_u,
                            const float* i_table, int64_t i_ld, int64_t i_V, const int64_t* i_ids, int F_i, int E,
                            int h1, int h2, int d_out, int64_t B, const float* const* weights, const float* label,
                            float* u_vals, float* i_vals, float* user_emb, float* item_emb, float* score, int* oob_flag,
                            void* workspace, size_t workspace_bytes, int64_t* step_dev, const float* lr_table,
                            int64_t n_table, float* lr_t_dev, void* stream);
int rec_dssm_fused_post_f32(int64_t B, int E, int F_u, int F_i, const void* workspace, size_t workspace_bytes,
                            float* const* grads, float* loss, const float* u_vals, const int32_t* u_perm,
                            const int32_t* u_seg, const int64_t* u_uniq, const int64_t* u_n_uniq, float* u_rows,
                            const float* i_vals, const int32_t* i_perm, const int32_t* i_seg, const int64_t* i_uniq,
                            const int64_t* i_n_uniq, float* i_rows, float* const* adam, int64_t u_ld, int64_t u_V,
                            int64_t i_ld, int64_t i_V, const float* lr_t_dev, float b1, float b2, float eps,
                            void* stream);

/* ---- K8/K9  DIN ActivationUnit + masked sum pooling (5.DIN/CustomLayers.py:163-180, 256-282), factorised:
 *   pre[b,t,:] = c_b + k_t . Eff_b,  Eff_b = (W_k - W_d) + M_b,  M_b[i,o] = sum_j q_j W_o[i,j,o],
 *   c_b = q (W_q + W_d) + b1;  score = act(pre) . w2 + b2;  pooled[b,:] = sum_t mask[b,t] * score[b,t] * k_t.
 * D = E*C (C item features), H = hidden width (36 in the reference), W1 = the Dense(H) kernel [3D + D*D, H].
 * activation kinds for per-feature activations (alpha/mean/var are [H] device vectors; unused ones may be NULL): */
enum { REC_DACT_NONE = 0, REC_DACT_RELU = 1, REC_DACT_SIGMOID = 2, REC_DACT_TANH = 3,
       REC_DACT_DICE = 4,   /* Dice, BN(center=False, scale=False) with moving statistics (5.DIN/CustomLayers.py:183-196) */
       REC_DACT_PRELU = 5 };
/* W1, b1 -> Wcat [D, D*H + H] = [Wo_r | W_q + W_d], Wkd [D,H] = W_k - W_d, bext [D*H + H] = [0 | b1]; then
 * Mext = q . Wcat + bext is ONE rec_gemm_f32 per batch.  prepare_bwd maps (gWcat, gWkd) back onto gW1. */
int rec_din_prepare_f32(const float* W1, const float* b1, int D, int H, float* Wcat, float* Wkd, float* bext,
                        void* stream);
int rec_din_prepare_bwd_f32(const float* gWcat, const float* gWkd, int D, int H, float* gW1, void* stream);
/* series: int64 [B,T,C] (the tf.stack(axis=2) of the behaviour series, :258); key k_t = concat_r embed[series[b,t,r]].
 * mask: reference behaviour (mask_valid = 0) keeps PADDED positions (series[b,t,0] == padding_index, :256,277-278);
 * mask_valid = 1 is the intended form.  scores [B,T] are the raw (unmasked) scores; pooled [B,D].
 * Supported, the same for the forward and the backward: 1 <= D = E C <= REC_DIN_MAX_D (256), 1 <= H <= REC_DIN_MAX_H
 * (64), and D > REC_DIN_WIDE_D (128) only with H <= REC_DIN_WIDE_MAX_H (48): at 129 <= D <= 256 with 49 <= H <= 64 the
 * backward's LDS (156 KiB) is above its launch cap REC_TILE_LDS_CAP (150 KiB), so both directions refuse that corner.
 * Outside: -2 (REC_E_UNSUPPORTED), answered from the sizes alone before a pointer is looked at, also with B == 0.  A
 * size <= 0, ld < E, V <= 0, an unknown act or a NULL pointer: -1. */
int rec_din_attn_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                         int T, const float* Mext, const float* Wkd, int H, int act, const float* alpha,
                         const float* mean, const float* var, const float* w2, const float* b2,
                         int64_t padding_index, int mask_valid, float* scores, float* pooled, int* oob_flag,
                         void* stream);
/* backward: gkeys [B,T,D] (IndexedSlices values of the series lookups), gMext [B, D*H+H], and per-example partials
 * gw2p [B,H], galphap [B,H], gb2p [B] (column sums of these are the parameter gradients).  gscores (optional, [B,T]):
 * a gradient that arrives at the raw scores themselves, added to the one that comes through pooled; NULL = none. */
int rec_din_attn_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                         int T, const float* Mext, const float* Wkd, int H, int act, const float* alpha,
                         const float* mean, const float* var, const float* w2, const float* b2,
                         int64_t padding_index, int mask_valid, const float* scores, const float* gpooled,
                         const float* gscores, float* gkeys, float* gMext, float* gw2p, float* galphap, float* gb2p,
                         void* stream);

/* ---- rows of DIN's final MLP (make_mlp_layer, 5.DIN/CustomLayers.py:142-160) */
/* y = act(x) on [M,N] with per-feature parameters; bwd also returns gy * dy/dalpha per element (column-sum it) */
int rec_feat_act_fwd_f32(int kind, const float* x, const float* alpha, const float* mean, const float* var, float* y,
                         int64_t M, int N, void* stream);
int rec_feat_act_bwd_f32(int kind, const float* x, const float* gy, const float* alpha, const float* mean,
                         const float* var, float* gx, float* ga_elem, int64_t M, int N, void* stream);
/* keras LayerNormalization (epsilon 1e-3): y = xhat*gamma + beta; saves xhat [M,N] and rstd [M] */
int rec_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, int64_t M, int N, float* y,
                          float* xhat, float* rstd, void* stream);
/* the same with a given epsilon (finite, > 0; else -1); rec_layernorm_fwd_f32 is this at 1e-3, bit for bit.  The backward
 * works from xhat and rstd and so serves both */
int rec_layernorm_eps_fwd_f32(const float* x, const float* gamma, const float* beta, int64_t M, int N, float eps,
                              float* y, float* xhat, float* rstd, void* stream);
int rec_layernorm_bwd_f32(const float* gy, const float* xhat, const float* rstd, const float* gamma, int64_t M, int N,
                          float* gx, float* gg_elem, void* stream);
int rec_softmax_fwd_f32(const float* x, int64_t M, int N, float* y, void* stream);
int rec_softmax_bwd_f32(const float* y, const float* gy, int64_t M, int N, float* gx, void* stream);

/* ==== SURVEY.md section 8 row f4: sibling interaction layers that share the gather ======================= */

/* ---- PNN inner product: Embedding -> Flatten ++ IpnLayer (2.FM/CustomLayers.py:729-745, :755-792).
 * out[b, f*E + d] = table[X[b,f], d];  out[b, F*E + p(i,j)] = <e_i, e_j> for i < j in the row-major order of the
 * upper triangle (the order tf.boolean_mask keeps).  ld_out >= F*E + F*(F-1)/2: `out` IS the reference's
 * combined_vector.  Forward and backward accept the same shapes: F <= 255, 4*F*(E+4) + 4*F + F*(F-1) + 16 <= 65536 (the
 * forward's LDS of one example) and 4*F*(2*E + 1 + F) <= 163840 (the backward's, one CU); REC_E_ARG beyond. */
int rec_emb_ipn_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F,
                        float* out, int64_t ld_out, int* oob_flag, void* stream);
/* IndexedSlices values of that lookup: vals[b*F+i, :] = g[b, i*E:(i+1)*E] + sum_{j != i} g[b, F*E + p(i,j)] * e_j,
 * with the rows e read back from the forward output `out`. */
int rec_emb_ipn_bwd_vals_f32(const float* out, int64_t ld_out, const float* g, int64_t ld_g, int64_t B, int F, int E,
                             float* vals, void* stream);

/* ---- NFM bi-interaction pooling (3.DCN/CustomLayers.py:499-501): out[b,d] = 0.5*((sum_f e_fd)^2 - sum_f e_fd^2),
 * written with row stride ld_out (so it can land in the leading columns of [second_order | X_cont]); sumvec [B,E]
 * = sum_f e_f is kept for the backward  vals[b*F+f, d] = g[b,d] * (sumvec[b,d] - e_fd). */
int rec_emb_bi_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F, float* out,
                       int64_t ld_out, float* sumvec, int* oob_flag, void* stream);
int rec_emb_bi_bwd_vals_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F,
                            const float* g, int64_t ld_g, const float* sumvec, float* vals, void* stream);

/* ---- SIM GSU inner-product attention + sum pooling (7.SIM/CustomLayers.py:88-96, 107-118).
 * series int64 [B,T,C]; key k_t = concat_r embed[series[b,t,r]] (D = C*E <= 256); valid[b,t] = series[b,t,0] !=
 * padding_index; scores[b,t] = valid * <q_b, k_t> (the masked scores); pooled[b,:] = sum_t scores[b,t] * k_t. */
int rec_ip_attn_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B, int T,
                        const float* q, int64_t ld_q, int64_t padding_index, float* scores, float* pooled,
                        int64_t ld_pooled, int* oob_flag, void* stream);
/* gkeys [B,T,D] = IndexedSlices values of the series lookups, gq [B,D] = gradient of the target vector. */
int rec_ip_attn_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B, int T,
                        const float* q, int64_t ld_q, int64_t padding_index, const float* scores, const float* gpooled,
                        int64_t ld_gpooled, float* gkeys, float* gq, void* stream);

/* ---- FFM, field-aware second order (FieldAwareInteractionLayer 2.FM/CustomLayers.py:428-462; FFMRankingLayer.call
 * :398-425 computes the same numbers from F separate tables).  v [V, F, E] with row stride ld_v >= F*E floats:
 * v[id, c, :] is the vector id uses against field c (table c of the loop form, row id).
 *   z[b] = bias + sum_a w[X[b,a]] + sum_{a<c} < v[X[b,a], c, :], v[X[b,c], a, :] >,  prob = sigmoid(z).
 * F <= 254 in both directions (4*F + 16 + F*(F-1) bytes of LDS, launched without the opt-in). */
int rec_ffm_fwd_f32(const float* v, int64_t ld_v, const float* w, int64_t ld_w, const float* bias, int64_t V, int E,
                    const int64_t* X, int64_t B, int F, float* z, float* prob, int* oob_flag, void* stream);
/* de-duplicated gradient rows of v on the plan of rec_dedup_plan_i64 over X (n = B*F):
 *   g_rows[u, c, :] = sum over the lookups (b,a) of unique id u of gz[b] * v[X[b,c], a, :]  (c != a);  rows >= n_uniq
 * are zero.  g_rows [B*F, F*E]. */
int rec_ffm_bwd_rows_f32(const float* v, int64_t ld_v, int64_t V, int E, const int64_t* X, int64_t B, int F,
                         const float* gz, const int32_t* perm, const int32_t* seg_start, const int64_t* n_uniq,
                         float* g_rows, void* stream);

/* ---- tf.keras.layers.BatchNormalization on [B,N] (3.DCN/CustomLayers.py:466,504; 2.FM/CustomLayers.py:69,78-79).
 * training != 0: batch mean / biased batch variance, moving statistics updated in place with `momentum`;
 * training == 0: moving statistics.  xhat [B,N] and rstd [N] are saved for the backward (may be NULL at inference).
 * gamma / beta may be NULL (scale / center off).  workspace: rec_batchnorm_workspace_bytes(B, N) device bytes. */
size_t rec_batchnorm_workspace_bytes(int64_t B, int N);
int rec_batchnorm_fwd_f32(const float* x, int64_t ld_x, int64_t B, int N, const float* gamma, const float* beta,
                          float eps, float momentum, int training, float* moving_mean, float* moving_var, float* y,
                          float* xhat, float* rstd, void* workspace, void* stream);
int rec_batchnorm_bwd_f32(const float* g, const float* xhat, const float* rstd, int64_t B, int N, const float* gamma,
                          int training, float* gx, float* ggamma, float* gbeta, void* workspace, void* stream);

/* ---- Compressed Interaction Network of xDeepFM (CINLayer, 3.DCN/CustomLayers.py:377-417; csrc/cin.hip).
 * x0 [B, F, E]; L layers of H_host[k] = cin_size[k] units; W_host: HOST array of L device pointers, W_k
 * [F * H_k, H_{k+1}] row-major (the reference's (1, F*H_k, H_{k+1}) weight; H_0 = F, row m*H_k + n):
 *   X^{k+1}[b,h,e] = sum_{m,n} W_k[m*H_k + n, h] * x0[b,m,e] * X^k[b,n,e]     (X^0 = x0)
 *   cin_part [B, SH] = concat_k sum_e X^{k+1}[b,:,e]      states [B, SH, E] = concat_k X^{k+1}  (SH = sum H_k)
 * The backward takes g = dLoss/dcin_part [B, SH] and writes dx0 [B, F, E] and every dW_k (dW_host: HOST array of L
 * device pointers, shapes of W_k).  No float atomics: bit-identical results run to run.
 * Supported: 1 <= F, E <= 64, 1 <= L <= 8, 1 <= H_k <= 256, B >= 1; otherwise -2 (an H_k < 1 or B < 1 is -1).
 * workspace: rec_cin_workspace_bytes (0: invalid or unsupported shape). */
size_t rec_cin_workspace_bytes(int64_t B, int F, int E, int L, const int* H_host);
int rec_cin_fwd_f32(const float* x0, int64_t B, int F, int E, int L, const int* H_host, const float* const* W_host,
                    float* states, float* cin_part, void* stream);
int rec_cin_bwd_f32(const float* x0, const float* states, const float* g, int64_t B, int F, int E, int L,
                    const int* H_host, const float* const* W_host, float* dx0, float* const* dW_host, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- FiBiNet SENet + bilinear interaction (FiBiNetLayer / SENetLayer / BilinearInteractionLayer,
 * 3.DCN/CustomLayers.py:888-1011; csrc/fibinet.hip).  x_emb [B, F, E], x_cont [B, C] (may be NULL when C == 0),
 * S0 [F, mid], S1 [mid, F], W [nW, E, E] packed (nW = 1 / F-1 / P for type REC_FIBINET_TYPE_ALL / _EACH / _INTERACTION,
 * P = F(F-1)/2 pairs i<j in itertools.combinations order; 'each' uses W[i], 'interaction' W[pair]):
 *   Z = mean_e x_emb      H1 = relu(Z S0) [B, mid]      A = relu(H1 S1) [B, F]
 *   p_ij = (v_i W_ij) * v_j      dnn_in [B, 2PE + C] = [p (raw pairs) | A_i A_j p_ij (SENet pairs) | x_cont],
 *   element (s, pair, e) at column (s P + pair) E + e.  A and H1 are written for the backward.
 * The backward reads the 2PE interaction columns of g = dLoss/d dnn_in [B, 2PE + C] and writes dx_emb [B, F, E],
 * dW [nW, E, E] (summed over the pairs sharing a W), dS0 and dS1.  No float atomics: bit-identical results run to run.
 * Supported: 2 <= F <= 32, 1 <= E <= 64, 0 <= C <= 64, 1 <= mid <= F, B >= 0 (B == 0: nothing is launched);
 * otherwise -2.  A negative size, a type that is none of the three or a NULL pointer: -1.
 * workspace: rec_fibinet_workspace_bytes (0: invalid or unsupported shape). */
size_t rec_fibinet_workspace_bytes(int64_t B, int F, int E, int mid, int type);
int rec_fibinet_fwd_f32(const float* x_emb, const float* x_cont, const float* S0, const float* S1, const float* W,
                        int64_t B, int F, int E, int C, int mid, int type, float* dnn_in, float* A, float* H1,
                        void* stream);
int rec_fibinet_bwd_f32(const float* x_emb, const float* g, const float* A, const float* H1, const float* S0,
                        const float* S1, const float* W, int64_t B, int F, int E, int C, int mid, int type,
                        float* dx_emb, float* dW, float* dS0, float* dS1, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- AutoInt multi-head field attention (TransformerAttentionLayer / AutoIntLayer, 3.DCN/CustomLayers.py:1012-1139;
 * csrc/autoint.hip).  One layer over X [B, F, E], F = Fc + C fields: the Fc categorical rows come from x [B, Fc, E],
 * the C continuous rows (last) are cemb[c, :] * x_cont[b, c] (cemb [C, E], x_cont [B, C]; both may be NULL when C == 0).
 * H heads of width d = E / H, head h owns the columns [h d, (h+1) d):
 *   Q = X Wq, K = X Wk, V = X Wv (each [E, E])      S[h,b,i,j] = scale Q_h[b,i,:] . K_h[b,j,:], scale = 1/sqrt(d) or 1
 *   P = softmax of S over the BATCH axis b (the reference's tf.nn.softmax(axis=1) on (H, B, F, F))
 *   O[b,i,h d + c] = sum_j P[h,b,i,j] V[b,j,h d + c]      Z = O | O + X | O + X Wres  (res REC_AUTOINT_RES_NONE | _ADD | _LEARNED)
 *   y = relu(Z) [B, F, E];  o [B, F, E] = O before the residual (may be NULL);  stats [2, H, F, F] = (max_b S, 1/sum_b
 *   exp(S - max)) for the backward.
 * The backward takes dy = dLoss/dy and writes dx [B, Fc, E] (categorical rows), dWq, dWk, dWv, dWres (res 2), dcemb
 * [C, E] (C > 0).  Every output of one call depends on the whole batch.  No float atomics: bit-identical results run
 * to run; no host synchronisation (graph-capturable).
 * Supported: 1 <= F <= 64, 1 <= E <= 64, 1 <= H <= E with E % H == 0, 0 <= C < F, 0 <= B < 2^31 (B == 0: nothing is
 * launched); otherwise -2.  A negative size, a res that is none of the three, scaling outside 0..1 or a NULL pointer:
 * -1.
 * workspace: rec_autoint_workspace_bytes (0: invalid or unsupported shape), for either direction. */
size_t rec_autoint_workspace_bytes(int64_t B, int F, int E, int H, int C, int res);
int rec_autoint_fwd_f32(const float* x, const float* x_cont, const float* cemb, const float* Wq, const float* Wk,
                        const float* Wv, const float* Wres, int64_t B, int F, int E, int H, int C, int res, int scaling,
                        float* y, float* o, float* stats, void* workspace, size_t workspace_bytes, void* stream);
int rec_autoint_bwd_f32(const float* x, const float* x_cont, const float* cemb, const float* Wq, const float* Wk,
                        const float* Wv, const float* Wres, const float* y, const float* dy, const float* stats,
                        int64_t B, int F, int E, int H, int C, int res, int scaling, float* dx, float* dWq, float* dWk,
                        float* dWv, float* dWres, float* dcemb, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Attentional Factorization Machine, fused with the lookup (InteractionLayer / AttentionLayer /
 * AttentionalFactorizationMachine, 3.DCN/CustomLayers.py:825-885; csrc/afm.hip).  X int64 [B, F], table [V, E] with row
 * stride ld; Wa [E, A], ba [A] (attention_w), hv [A] (attention_h kernel [A, 1]), bh [1]:
 *   e_f = table[X[b,f]]      p_k = e_i * e_j for the P = F(F-1)/2 pairs i < j (i outer, j inner)
 *   s_k = relu(p_k Wa + ba) . hv + bh      a = softmax over the pairs k      o [B, E] = sum_k a_k p_k
 * The forward writes o, stats [B, 2] = (max_k s_k, sum_k exp(s_k - max)) and, when `rows` is not NULL, the gathered rows
 * [B, F, E]; an id outside [0, V) sets *oob_flag (may be NULL) and reads as a zero row.
 * The backward takes dout = dLoss/do [B, E] and writes vals [B*F, E], the IndexedSlices values of the lookup in the
 * order of X, and dWa [E, A], dba [A], dhv [A], dbh [1].  With `rows` (the forward's) it does not touch the table and X
 * (both may then be NULL); with rows == NULL it gathers again.  No float atomics: bit-identical results run to run; no
 * host synchronisation (graph-capturable).
 * Supported: 2 <= F <= 64, 1 <= E <= 64, 1 <= A <= 16, 0 <= B < 2^31 (B == 0: nothing is launched), V < 2^31;
 * otherwise -2.  A negative size, V <= 0, ld < E or a NULL pointer: -1.
 * workspace (backward only): rec_afm_workspace_bytes (0: invalid or unsupported shape). */
size_t rec_afm_workspace_bytes(int64_t B, int F, int E, int A);
int rec_emb_afm_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F, int A,
                        const float* Wa, const float* ba, const float* hv, const float* bh, float* o, float* stats,
                        float* rows, int* oob_flag, void* stream);
int rec_emb_afm_bwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F, int A,
                        const float* Wa, const float* ba, const float* hv, const float* bh, const float* o,
                        const float* stats, const float* rows, const float* dout, float* vals, float* dWa, float* dba,
                        float* dhv, float* dbh, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Convolutional Click Prediction Model, fused with the lookup (KMaxPool / CCPMBaseLayer / CCPMLayer,
 * 3.DCN/CustomLayers.py:621-725; csrc/ccpm.hip).  X int64 [B, F], table [V, E] with row stride ld.  L layers; the HOST
 * int arrays filters_host[L] (C_j), kernel_width_host[L] (kw_j) and pool_k_host[L] (k_j) describe them; params is one
 * flat DEVICE buffer K_1 | b_1 | K_2 | b_2 | ... with K_j [kw_j, 1, C_{j-1}, C_j] row-major (C_0 = 1) and b_j [C_j].
 * With x_0[h, e, 0] = table[X[b,h]][e] (H_0 = F) and for j = 1..L:
 *   y[h, e, co] = tanh(b_j[co] + sum_t sum_ci K_j[t, 0, ci, co] x_{j-1}[h - (kw_j - 1) / 2 + t, e, ci])   zeros outside
 *                 [0, H_{j-1}) (TF's SAME padding: the extra row at the end)
 *   x_j[r, e, co] = the r-th largest y[., e, co] over h: values in descending order, the lower h first on equal values
 *                 (tf.nn.top_k(sorted=True)); H_j = k_j
 * The forward writes out [B, k_L E C_L], out[b, (r E + e) C_L + c] = x_L[r, e, c] (Flatten), and, when `rows` is not
 * NULL, the gathered rows [B, F, E]; an id outside [0, V) sets *oob_flag (may be NULL) and reads as a zero row.
 * The backward takes dout = dLoss/dout and writes vals [B*F, E], the IndexedSlices values of the lookup in the order of
 * X (the gradient reaches the selected positions only), and dparams in the layout of params.  With `rows` (the
 * forward's) it does not touch the table and X (both may then be NULL); with rows == NULL it gathers again.  No float
 * atomics: bit-identical results run to run; no host synchronisation (graph-capturable).
 * Supported: 1 <= F <= 64, 1 <= E <= 64, 1 <= L <= 3, 1 <= C_j <= 16, 1 <= kw_j <= 8, 1 <= k_j, 0 <= B < 2^31
 * (B == 0: nothing is launched), V < 2^31, and a column's working set within the LDS of a CU at 64 threads: with
 * S = F + sum_j k_j C_j, (2 S + F + ceil(S / 4)) * 256 + 4 * sum_j (kw_j C_{j-1} + 1) C_j <= 160 KiB; otherwise -2.
 * A negative size, V <= 0, ld < E, a NULL pointer or k_j > H_{j-1} (top_k over fewer values than k): -1.
 * workspace (backward only): rec_ccpm_workspace_bytes (0: invalid or unsupported shape). */
size_t rec_ccpm_workspace_bytes(int64_t B, int F, int E, int L, const int* filters_host, const int* kernel_width_host,
                                const int* pool_k_host);
int rec_emb_ccpm_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F, int L,
                         const int* filters_host, const int* kernel_width_host, const int* pool_k_host,
                         const float* params, float* out, float* rows, int* oob_flag, void* stream);
int rec_emb_ccpm_bwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F, int L,
                         const int* filters_host, const int* kernel_width_host, const int* pool_k_host,
                         const float* params, const float* rows, const float* dout, float* vals, float* dparams,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- Feature Generation by CNN, fused with the lookup (FGCNNBaseLayer / FGCNNLayer, 3.DCN/CustomLayers.py:728-822;
 * csrc/fgcnn.hip).  X int64 [B, F], table [V, E] with row stride ld.  L layers; the HOST int arrays filters_host[L]
 * (C_j), kernel_width_host[L] (kw_j) and pooling_width_host[L] (pw_j) describe them; params is one flat DEVICE buffer
 * K_1 | b_1 | K_2 | b_2 | ... with K_j [kw_j, 1, C_{j-1}, C_j] row-major (C_0 = 1) and b_j [C_j].
 * With x_0[h, e, 0] = table[X[b,h]][e] (H_0 = F) and for j = 1..L:
 *   y[h, e, co] = tanh(b_j[co] + sum_t sum_ci K_j[t, 0, ci, co] x_{j-1}[h - (kw_j - 1) / 2 + t, e, ci])   zeros outside
 *                 [0, H_{j-1}) (TF's SAME padding: the extra row at the end)
 *   x_j[r, e, co] = max_{q < pw_j} y[r pw_j + q, e, co]      MaxPool2D((pw_j, 1)), stride pw_j, VALID:
 *                 H_j = H_{j-1} / pw_j, the trailing H_{j-1} mod pw_j rows are dropped
 * The forward writes the gathered rows [B, F, E] and EVERY pooled map, pooled_out_host_ptrs[j-1] -> p_j
 * [B, H_j E C_j] with p_j[b, (r E + e) C_j + c] = x_j[r, e, c] (Flatten); pooled_out_host_ptrs is a HOST array of L
 * device pointers.  An id outside [0, V) sets *oob_flag (may be NULL) and reads as a zero row.
 * The backward takes the saved rows, dpooled_host_ptrs[j-1] -> dLoss/dp_j for every j (a HOST array of L device
 * pointers) and drows_direct [B, F, E] = dLoss/drows from the rows' other consumers (may be NULL: zeros).  It writes
 * vals [B*F, E] = drows_direct + dLoss/dx_0, the IndexedSlices values of the lookup in the order of X, and dparams in
 * the layout of params.  The gradient of a pooling goes to the maximum of its window, on equal values to the LOWER
 * row; dropped rows get none.  It reads neither the table nor X, so it takes only the shape.  No float atomics:
 * bit-identical results run to run; no host synchronisation (graph-capturable).
 * Supported: 1 <= F <= 64, 1 <= E <= 64, 1 <= L <= 3, 1 <= C_j <= 16, 1 <= kw_j <= 8, pw_j <= 8, 0 <= B < 2^31
 * (B == 0: nothing is launched), V < 2^31, and the state of one column within the LDS of a CU; otherwise -2.
 * A negative size, V <= 0, ld < E, a NULL pointer, pw_j < 1 or H_j == 0: -1.
 * workspace (backward only): rec_fgcnn_workspace_bytes (0: invalid or unsupported shape). */
size_t rec_fgcnn_workspace_bytes(int64_t B, int F, int E, int L, const int* filters_host, const int* kernel_width_host,
                                 const int* pooling_width_host);
int rec_emb_fgcnn_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F, int L,
                          const int* filters_host, const int* kernel_width_host, const int* pooling_width_host,
                          const float* params, float* rows_out, float* const* pooled_out_host_ptrs, int* oob_flag,
                          void* stream);
int rec_emb_fgcnn_bwd_f32(int E, int64_t B, int F, int L, const int* filters_host, const int* kernel_width_host,
                          const int* pooling_width_host, const float* params, const float* rows,
                          const float* const* dpooled_host_ptrs, const float* drows_direct, float* vals, float* dparams,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- MaskNet (LayerNormInputFeaturesEmbeddingLayer / MaskBlockLayer, 11.FiBiNet++/CustomLayers.py:245-337;
 * csrc/masknet.hip).
 * Input stage, fused with the lookup.  X int64 [B, F], F = Fc + Fk with the Fk key columns of the continuous features
 * LAST; values [B, Fk] (NULL when Fk == 0); table [V, E] with row stride ld; gamma, beta [F, E], one LayerNormalization
 * per field:
 *   r[b,f,:] = table[X[b,f]] for f < Fc      r[b,Fc+j,:] = table[X[b,Fc+j]] * values[b,j]
 *   x_emb [B, F E] = r      x_norm[b,f,:] = (r - mean) * rstd * gamma_f + beta_f   (biased variance over E, epsilon 1e-3)
 *   stats [B, F, 2] = (mean, rstd), for the backward.
 * An id outside [0, V), in a key column too, sets *oob_flag (may be NULL) and reads as a zero row.
 * The backward takes dx_norm [B, F E] and dx_emb [B, F E] = dLoss/dx_emb from the other consumers of x_emb (may be NULL:
 * zeros) and writes vals [B*F, E], the IndexedSlices values of the lookup in the order of X -- the continuous fields'
 * already multiplied by their value (an input: no gradient of its own) -- and dgamma, dbeta [F, E].  It reads neither
 * the table nor X.
 * Mask block.  x_emb [B, D], v [B, P], W1 [D, R P], b1 [R P], W2 [R P, P], b2 [P], W3 [P, O], b3 [O], gamma, beta [O]:
 *   h = relu(x_emb W1 + b1)   m = h W2 + b2   u = v (.) m   z = u W3 + b3   y [B, O] = relu(LayerNorm(z))  (epsilon 1e-3)
 * One launch; the products run on v_mfma_f32_32x32x2_f32 (fp32-exact, as rec_gemm_f32).  The save buffers h [B, R P],
 * m [B, P], xhat [B, O], rstd [B] are all given (training) or all NULL (inference: only y is written; the same y).
 * The backward takes dy [B, O] and the forward's y and save buffers, writes dv [B, P], dx_emb [B, D] (accumulate != 0:
 * added to what dx_emb holds, so the blocks of a stack add into one buffer in call order) and dW1, db1, dW2, db2, dW3,
 * db3, dgamma, dbeta: one launch for the per-example chain, one slot sum for the vectors, and dW1 = x_emb^T dh,
 * dW2 = h^T dm, dW3 = u^T dz on rec_gemm_f32 (split-K over the batch in at most 16 slices, added in order).
 * All four only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  B == 0: nothing is launched.
 * Supported: 1 <= F <= 64, 1 <= E <= 64, 0 <= Fk <= F; 1 <= D, P <= 512, 1 <= O <= 128, 1 <= R <= 4; 0 <= B < 2^31;
 * otherwise -2.  A negative size, V <= 0, ld < E, a NULL pointer or save buffers given in part: -1.
 * workspace: rec_masknet_ln_workspace_bytes for the input stage's backward, rec_masknet_block_workspace_bytes for a
 * block's backward: 4 B (R P + 2 P + O) bytes of per-example gradients, (B / 32) slots of 3 O + P + R P floats and at
 * most 16 copies of the largest weight (0: invalid or unsupported shape). */
size_t rec_masknet_ln_workspace_bytes(int64_t B, int F, int E);
int rec_emb_masknet_ln_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, const float* values,
                               int64_t B, int F, int Fk, const float* gamma, const float* beta, float* x_emb,
                               float* x_norm, float* stats, int* oob_flag, void* stream);
int rec_emb_masknet_ln_bwd_f32(const float* x_emb, const float* stats, const float* values, const float* gamma,
                               const float* dx_norm, const float* dx_emb, int64_t B, int F, int Fk, int E, float* vals,
                               float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
size_t rec_masknet_block_workspace_bytes(int64_t B, int D, int P, int O, int R);
int rec_mask_block_fwd_f32(const float* x_emb, const float* v, const float* W1, const float* b1, const float* W2,
                           const float* b2, const float* W3, const float* b3, const float* gamma, const float* beta,
                           int64_t B, int D, int P, int O, int R, float* y, float* h, float* m, float* xhat, float* rstd,
                           void* stream);
int rec_mask_block_bwd_f32(const float* x_emb, const float* v, const float* W1, const float* W2, const float* W3,
                           const float* gamma, const float* y, const float* h, const float* m, const float* xhat,
                           const float* rstd, const float* dy, int64_t B, int D, int P, int O, int R, float* dv,
                           float* dx_emb, int accumulate, float* dW1, float* db1, float* dW2, float* db2, float* dW3,
                           float* db3, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- ContextNet (ContextualEmbeddingLayer / NonLinearFeedforwardLayer / ContextNetBlockLayer,
 * 11.FiBiNet++/CustomLayers.py:412-531; csrc/contextnet.hip).
 * Input stage, fused with the lookup: MaskNet's without the LayerNorm.  X int64 [B, F], F = Fc + Fk with the Fk key
 * columns LAST; values [B, Fk] (NULL when Fk == 0); table [V, E] with row stride ld:
 *   x[b,f,:] = table[X[b,f]] for f < Fc      x[b,Fc+j,:] = table[X[b,Fc+j]] * values[b,j]      x [B, F E]
 * An id outside [0, V), in a key column too, sets *oob_flag (may be NULL) and reads as a zero row.  The backward takes
 * dx [B, F E] and writes vals [B*F, E], the IndexedSlices values of the lookup in the order of X, the key fields'
 * multiplied by their value (an input: no gradient of its own).  It reads neither the table nor X.
 * Block.  x [B, F E], D = F E, H = R D; Wa [D, H], ba [H], Wb [H, D], bb [D]; per field W1, W2 [F, E, E] and gamma,
 * beta [F, E]:
 *   h = relu(x Wa + ba)   m = h Wb + bb   u = x (.) m
 *   pointwise != 0:  a_f = relu(u_f W1_f)   r_f = a_f W2_f + u_f        pointwise == 0:  r_f = u_f W1_f   (W2 unused: NULL)
 *   y[b,f,:] = LayerNorm(r_f) gamma_f + beta_f   (biased variance over E, epsilon 1e-3)        y [B, F E]
 * One launch; h and m run on v_mfma_f32_32x32x2_f32 (fp32-exact, as rec_gemm_f32), the per-field products out of LDS.
 * The save buffers h [B, H], m [B, D], xhat [B, D], rstd [B, F] and, when pointwise, a [B, D] (ignored otherwise) are
 * all given (training) or all NULL (inference: only y is written; the same y).
 * The backward takes dy [B, D] and the forward's save buffers and writes dx [B, D] (written, never added to) and dWa,
 * dba, dWb, dbb, dW1, dW2 (pointwise only, else may be NULL), dgamma, dbeta: one launch for the per-example chain, one
 * slot sum for the vectors, ONE launch for all per-field weight gradients (dW1_f = u_f^T da_f, dW2_f = a_f^T dr_f over
 * at most 16 batch slices added in order by a second slot sum), and dWa = x^T dh, dWb = h^T dm on rec_gemm_f32 (split-K
 * over the batch in at most 16 slices, added in order): the number of launches does not depend on F.
 * All four only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  B == 0: nothing is launched.
 * Supported: the limits are MaskNet's, this family has no constants of its own: 1 <= F <= REC_MASKNET_MAX_F,
 * 1 <= E <= REC_MASKNET_MAX_E, F E <= REC_MASKNET_MAX_D (the input stage too: it feeds the blocks),
 * 1 <= R <= REC_MASKNET_MAX_R, 0 <= Fk <= F, 0 <= B < 2^31; otherwise -2.  A negative size, V <= 0, ld < E, pointwise other than 0 / 1, a NULL pointer or save buffers given in
 * part: -1.
 * workspace (block backward only): rec_contextnet_block_workspace_bytes: 4 B (R D + 3 D, + D when pointwise) bytes of
 * per-example gradients, (B / 32) slots of 3 D + R D floats, at most 16 copies of the per-field weights and at most 16
 * of Wa (0: invalid or unsupported shape). */
int rec_emb_contextnet_in_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X,
                                  const float* values, int64_t B, int F, int Fk, float* x, int* oob_flag, void* stream);
int rec_emb_contextnet_in_bwd_f32(const float* values, const float* dx, int64_t B, int F, int Fk, int E, float* vals,
                                  void* stream);
size_t rec_contextnet_block_workspace_bytes(int64_t B, int F, int E, int R, int pointwise);
int rec_contextnet_block_fwd_f32(const float* x, const float* Wa, const float* ba, const float* Wb, const float* bb,
                                 const float* W1, const float* W2, const float* gamma, const float* beta, int64_t B,
                                 int F, int E, int R, int pointwise, float* y, float* h, float* m, float* xhat,
                                 float* rstd, float* a, void* stream);
int rec_contextnet_block_bwd_f32(const float* x, const float* Wa, const float* Wb, const float* W1, const float* W2,
                                 const float* gamma, const float* h, const float* m, const float* xhat,
                                 const float* rstd, const float* a, const float* dy, int64_t B, int F, int E, int R,
                                 int pointwise, float* dx, float* dWa, float* dba, float* dWb, float* dbb, float* dW1,
                                 float* dW2, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ---- FiBiNet++ (NormInputFeaturesEmbeddingLayer / SENetPlusLayer / BilinearInteractionPlusLayer / FiBiNetPlusLayer,
 * 11.FiBiNet++/CustomLayers.py:78-242; csrc/fibinetplus.hip).
 * Input stage, fused with the lookup.  X int64 [B, F], F = Fc + Fk with the Fk key columns LAST; values [B, Fk] (NULL
 * when Fk == 0); table [V, E] with row stride ld:
 *   f < Fc:   x[b,f,:] = BatchNorm(table[X[b,f]])  ONE Keras BatchNormalization over the B Fc rows, per channel e: gamma_bn,
 *             beta_bn, moving_mean, moving_var [E], biased variance, epsilon 1e-3, momentum 0.99
 *   j < Fk:   x[b,Fc+j,:] = LayerNorm_j(table[X[b,Fc+j]] * values[b,j])  over E, epsilon 1e-3; gamma_ln, beta_ln [Fk, E]
 * training != 0: batch statistics, and moving <- 0.99 moving + 0.01 batch (the biased batch variance) on the device;
 * training == 0: the moving statistics, nothing updated.  The channel sums are per-workgroup partials in workspace slots
 * added in a fixed order, the variance a second pass over (x - mean)^2.  An id outside [0, V), in a key column too, sets
 * *oob_flag (may be NULL) and reads as a zero row, which takes part in the statistics.  The save buffers xhat [B, F E],
 * rstd_bn [E] (Fc > 0) and rstd_ln [B, Fk] (Fk > 0) are all given or all NULL.
 * The backward takes dx [B, F E] and the save buffers and writes vals [B*F, E], the IndexedSlices values of the lookup in
 * the order of X, the key fields' already multiplied by their value, and dgamma_bn, dbeta_bn [E], dgamma_ln, dbeta_ln
 * [Fk, E]; training != 0: the full BatchNorm backward across the B Fc rows, else g gamma rstd.  It reads neither the
 * table nor X.  workspace (both ways): rec_emb_fibinetplus_in_workspace_bytes.
 * Body.  x [B, F E], D = F E, P = F (F - 1) / 2 pairs (i < j) in itertools.combinations order; W [nW, E, E] with nW = 1
 * (type 0 'all'), F - 1 (type 1 'each': W[i]) or P (type 2 'interaction': W[pair]); Wr [P, O], br, gamma_q, beta_q [O];
 * G groups of width E / G; S0 [2 G F, mid], b0, gamma0, beta0 [mid]; S1 [mid, D], b1, gamma1, beta1 [D]:
 *   p[b,pair] = x_i W x_j^T      q = LayerNorm(p Wr + br)
 *   s[b, f 2G + g] = mean of group g of field f      s[b, f 2G + G + g] = its maximum
 *   h = relu(LayerNorm(s S0 + b0))      A = relu(LayerNorm(h S1 + b1))      out = [q | x (.) A]      out [B, O + D]
 * (every LayerNorm: biased variance, epsilon 1e-3).  One launch: a workgroup owns 16 examples whose x, p, s, h and A live
 * in LDS; nothing between x and out goes to global memory except the save buffers p [B, P], xhat_q [B, O], s [B, 2 G F],
 * xhat0 [B, mid], h [B, mid], xhat1 [B, D], rstd [B, 3] (q, h, A), all given (training) or all NULL (inference: only out
 * is written; the same out).
 * The backward takes dout [B, O + D] and the save buffers and writes dx [B, D] (written, never added to), dW [nW, E, E],
 * dWr, dbr, dgamma_q, dbeta_q, dS0, db0, dgamma0, dbeta0, dS1, db1, dgamma1, dbeta1: one launch for the per-example
 * chain (the gradient of a group maximum goes to its first arg-max element), two slot sums for the vectors, ONE launch
 * for all of dW over at most 16 batch slices added in order by a third slot sum, and dWr = p^T dzq, dS0 = s^T dz0,
 * dS1 = h^T dz1 on rec_gemm_f32 (split-K over the batch in at most 16 slices, added in order): the number of launches
 * does not depend on F or P.
 * All four only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  B == 0: nothing is launched.  A norm over one element returns exactly beta and
 * exactly zero input gradients.
 * Supported: the limits are FiBiNet's and MaskNet's, this family has no constants of its own: 2 <= F <= REC_FIBINET_MAX_F
 * (the input stage alone: 1 <= F),
 * 1 <= E <= REC_FIBINET_MAX_E, F E <= REC_MASKNET_MAX_D, 1 <= O <= REC_MASKNET_MAX_O, 1 <= mid <= REC_MASKNET_MAX_P,
 * G >= 1, 0 <= Fk <= F, type 0 / 1 / 2, 0 <= B < 2^31; otherwise -2.  A negative size, G not dividing E, V <= 0, ld < E,
 * a NULL pointer or save buffers given in part: -1.  A workspace that is too small: -3.
 * workspace (block backward only): rec_fibinetplus_block_workspace_bytes: 4 B (D + mid + O + P) bytes of per-example
 * gradients, (B / 16) slots of 3 (D + mid + O) floats, at most 16 copies of W and at most 16 of the largest of Wr, S0,
 * S1 (0: invalid or unsupported shape). */
size_t rec_emb_fibinetplus_in_workspace_bytes(int64_t B, int F, int Fk, int E);
int rec_emb_fibinetplus_in_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X,
                                   const float* values, const float* gamma_bn, const float* beta_bn,
                                   const float* gamma_ln, const float* beta_ln, int64_t B, int F, int Fk, int training,
                                   float* moving_mean, float* moving_var, float* x, float* xhat, float* rstd_bn,
                                   float* rstd_ln, int* oob_flag, void* workspace, size_t workspace_bytes, void* stream);
int rec_emb_fibinetplus_in_bwd_f32(const float* dx, const float* values, const float* xhat, const float* rstd_bn,
                                   const float* rstd_ln, const float* gamma_bn, const float* gamma_ln, int64_t B, int F,
                                   int Fk, int E, int training, float* vals, float* dgamma_bn, float* dbeta_bn,
                                   float* dgamma_ln, float* dbeta_ln, void* workspace, size_t workspace_bytes,
                                   void* stream);
size_t rec_fibinetplus_block_workspace_bytes(int64_t B, int F, int E, int G, int mid, int O, int type);
int rec_fibinetplus_block_fwd_f32(const float* x, const float* W, const float* Wr, const float* br,
                                  const float* gamma_q, const float* beta_q, const float* S0, const float* b0,
                                  const float* gamma0, const float* beta0, const float* S1, const float* b1,
                                  const float* gamma1, const float* beta1, int64_t B, int F, int E, int G, int mid, int O,
                                  int type, float* out, float* p, float* xhat_q, float* s, float* xhat0, float* h,
                                  float* xhat1, float* rstd, void* stream);
int rec_fibinetplus_block_bwd_f32(const float* x, const float* W, const float* Wr, const float* gamma_q, const float* S0,
                                  const float* gamma0, const float* beta0, const float* S1, const float* gamma1,
                                  const float* beta1, const float* p, const float* xhat_q, const float* s,
                                  const float* xhat0, const float* h, const float* xhat1, const float* rstd,
                                  const float* dout, int64_t B, int F, int E, int G, int mid, int O, int type, float* dx,
                                  float* dW, float* dWr, float* dbr, float* dgamma_q, float* dbeta_q, float* dS0,
                                  float* db0, float* dgamma0, float* dbeta0, float* dS1, float* db1, float* dgamma1,
                                  float* dbeta1, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MMOE / ESMM (MMOELayer / ESMMLayer, 4.MMOE/CustomLayers.py:107-245; csrc/mmoe.hip): n expert MLPs and T gate
 * MLPs over one input, the gate-weighted expert outputs flattened into T towers.
 * x [B, D]; n experts, T tasks, hidden width H1 of experts and gates, expert output width O, tower widths H2 and O2,
 * N1 = (n + T) H1.  Packed weights, all row-major:
 *   W1 [D, N1], b1 [N1]   the first layers side by side: column block i < n (H1 columns) is expert i's, block n + t gate t's
 *   We2 [n, H1, O], be2 [n, O]      Wg2 [T, H1, n], bg2 [T, n]
 *   Wt1 [T, n O, H2], bt1 [T, H2]   Wt2 [T, H2, O2], bt2 [T, O2]   Wt3 [T, O2], bt3 [T]
 * Per example (relu'(0) = 0):
 *   h = relu(x W1 + b1)   e_i = relu(h_i We2[i] + be2[i])   z_t = relu(h_{n+t} Wg2[t] + bg2[t])
 *   g_t = softmax(z_t), applied gate_softmax_passes times (1: MMOE, 2: ESMM)
 *   u_t = concat_i(e_i g_t[i])  [n O]  (flattened, not summed over the experts)
 *   a1_t = relu(u_t Wt1[t] + bt1[t])   a2_t = relu(a1_t Wt2[t] + bt2[t])   p_t = sigmoid(a2_t Wt3[t] + bt3[t])
 *   out[:, t] = p_t;  ctcvr != 0 (T == 2): out[:, 1] = p_0 p_1                                            out [B, T]
 * One launch: a workgroup owns 32 examples, x W1 runs on v_mfma_f32_32x32x2_f32 (fp32-exact, as rec_gemm_f32), everything
 * after h out of LDS.  The save buffers h [B, N1], e [B, n O], z [B, T n], g [B, T n] (the gate after the last softmax),
 * a1 [B, T H2], a2 [B, T O2] and p [B, T] are all given (training) or all NULL (inference: only out is written; the
 * same out).
 * The backward takes dout [B, T] and the save buffers and writes dx [B, D] (written, never added to) and the gradient of
 * every packed weight: one launch for the per-example chain and dx, one slot sum for the bias gradients, ONE launch for
 * dWe2, dWg2, dWt1, dWt2 and dWt3 over at most 16 batch slices added in order by a second slot sum, and dW1 = x^T dZ1
 * on rec_gemm_f32 (split-K over the batch in at most 16 slices, added in order): the number of launches does not depend
 * on n, T or B.
 * Both only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics: bit-identical
 * results run to run.  B == 0: nothing is launched.  With n == 1 the gate is exactly 1 and its gradients exactly 0.
 * Supported: the limits are MaskNet's, this family has no constants of its own: 1 <= D <= REC_MASKNET_MAX_D,
 * N1 <= REC_MASKNET_MAX_P, each of H1, H2, O2, n O and n T <= REC_MASKNET_MAX_O, 1 <= T <= REC_MASKNET_MAX_R, n >= 1,
 * 0 <= B < 2^31; otherwise -2.  A size below 1 (B below 0), gate_softmax_passes other than 1 / 2, ctcvr other than
 * 0 / 1, ctcvr with T != 2, a NULL pointer or save buffers given in part: -1.  A workspace that is too small: -3.
 * workspace (backward only): rec_mmoe_workspace_bytes: 4 B (N1 + n O + T n + T H2 + T O2 + T) bytes of per-example
 * gradients, (B / 32) slots of as many floats, at most 16 copies of the small weights and at most 16 of W1 (0: invalid
 * or unsupported shape). */
size_t rec_mmoe_workspace_bytes(int64_t B, int D, int n, int T, int H1, int O, int H2, int O2);
int rec_mmoe_fwd_f32(const float* x, const float* W1, const float* b1, const float* We2, const float* be2,
                     const float* Wg2, const float* bg2, const float* Wt1, const float* bt1, const float* Wt2,
                     const float* bt2, const float* Wt3, const float* bt3, int64_t B, int D, int n, int T, int H1, int O,
                     int H2, int O2, int gate_softmax_passes, int ctcvr, float* out, float* h, float* e, float* z,
                     float* g, float* a1, float* a2, float* p, void* stream);
int rec_mmoe_bwd_f32(const float* x, const float* W1, const float* We2, const float* Wg2, const float* Wt1,
                     const float* Wt2, const float* Wt3, const float* h, const float* e, const float* z, const float* g,
                     const float* a1, const float* a2, const float* p, const float* dout, int64_t B, int D, int n, int T,
                     int H1, int O, int H2, int O2, int gate_softmax_passes, int ctcvr, float* dx, float* dW1,
                     float* db1, float* dWe2, float* dbe2, float* dWg2, float* dbg2, float* dWt1, float* dbt1,
                     float* dWt2, float* dbt2, float* dWt3, float* dbt3, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- PLE (PLELayer, 4.MMOE/CustomLayers.py:248-384; csrc/ple.hip): one CGC level (customized gate control, one stage
 * of progressive layered extraction) per call each way.
 * T tasks, S specific experts per task, Sh shared experts, ne = T S + Sh experts, ns = S + Sh; hidden width H1 of every
 * MLP, expert output width O, gate MLP output width Og; last != 0: the last level (T outputs and the towers, no shared
 * gate), else a level with a shared output.  Gout = last ? T : T + 1 gates, M = ne + Gout first layers, N1 = M H1,
 * GW = T ns + (last ? 0 : ne) gate columns.
 * xin [B, Gin, Din] with Gin = 1 (level 0: every MLP reads the same row) or Gin = T + 1 (every MLP reads the row of its
 * group: task t is group t, the shared branch group T; Din is the previous level's O).  group(m): expert m < T S reads
 * group m / S, a shared expert and the shared gate read group T, task gate t reads group t.
 * Packed weights, all row-major:
 *   W1 [Din, N1], b1 [N1]   the first layers side by side: column block m < ne is expert m's, block ne + g gate g's
 *   We2 [ne, H1, O], be2 [ne, O]        Wg2 [Gout, H1, Og], bg2 [Gout, Og]
 *   Wg3s [T, Og, ns] (no bias)          Wg3h [Og, ne] (no bias; NULL iff last)
 *   Wtw [T, O], btw [T]                 the sigmoid towers (NULL unless last)
 * Per example (relu'(0) = 0):
 *   h_m = relu(in_group(m) W1_m + b1_m)   e_i = relu(h_i We2[i] + be2[i])   q_g = relu(h_{ne+g} Wg2[g] + bg2[g])
 *   g_t = softmax(softmax(q_t Wg3s[t]))  (twice, as the reference applies it)
 *   y_t = sum_{j<S} g_t[j] e_{t S+j} + sum_{k<Sh} g_t[S+k] e_{T S+k}         (a sum over the experts, not a flatten)
 *   not last:  g_T = softmax(q_T Wg3h) (once),  y_T = sum_i g_T[i] e_i over all experts in order
 *   last:      out[:, t] = sigmoid(y_t . Wtw[t] + btw[t])
 * y [B, Gout, O] is always written; out [B, T] iff last (NULL otherwise).
 * One launch: a workgroup owns 32 examples; the first layers run on v_mfma_f32_32x32x2_f32 (fp32-exact) in chunks of
 * whole MLPs whose second layers are finished before the next chunk, everything narrower out of LDS.  The save buffers
 * h [B, N1], e [B, ne O], q [B, Gout Og] and g [B, GW] (the gates after their last softmax, task gates first) are all
 * given (training) or all NULL (inference: the same y and out).
 * The backward takes the save buffers, y and out as the forward wrote them, dy [B, Gout, O] (may be NULL when last: read
 * as zero) and dout [B, T] (iff last), and writes dxin [B, Gin, Din] (written, never added to) and the gradient of every
 * packed weight (dWg3h iff not last, dWtw and dbtw iff last; NULL otherwise).  Gate logits are not saved: the first
 * softmax of a task gate is recomputed from q with the forward's code.  One launch for the per-example chain and dxin,
 * one slot sum for the bias gradients, ONE launch for dWe2, dWg2, dWg3s, dWg3h, dWtw (and dW1 when Gin > 1) over at most
 * 16 batch slices added in order by a second slot sum; with Gin = 1, dW1 = xin^T dZ1 on rec_gemm_f32 (split-K, slices
 * added in order).
 * All only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics: bit-identical
 * results run to run.  B == 0: nothing is launched.
 * Supported: the limits are MaskNet's, this family has no constants of its own: 1 <= Din <= REC_MASKNET_MAX_D,
 * H1 <= REC_MASKNET_MAX_O, ne O <= REC_MASKNET_MAX_O, (T + 1) Og <= REC_MASKNET_MAX_O, 1 <= T <= REC_MASKNET_MAX_R,
 * S >= 1, Sh >= 1, 0 <= B < 2^31, and two that keep every shape inside the 156 KB of LDS of a workgroup: the gate
 * columns GW <= REC_MASKNET_MAX_O (the gates, their first softmax and their gradients live in LDS next to e and q), and
 * Gin Din <= REC_MASKNET_MAX_O when Gin > 1 (the width of a previous level's y); otherwise -2.  A size below 1 (B below
 * 0), Gin other than 1 / T + 1, last other than 0 / 1, a NULL pointer that must be given or a pointer that must be
 * NULL, or save buffers given in part: -1.  A workspace that is too small: -3.
 * workspace (backward only): rec_ple_cgc_workspace_bytes: 4 B (N1 + ne O + Gout Og + GW + T) bytes of per-example
 * gradients, (B / 32) slots of bias gradients, at most 16 copies of the small weights and, with Gin = 1, at most 16 of
 * W1 (0: invalid or unsupported shape). */
size_t rec_ple_cgc_workspace_bytes(int64_t B, int Din, int Gin, int T, int S, int Sh, int H1, int O, int Og, int last);
int rec_ple_cgc_fwd_f32(const float* xin, const float* W1, const float* b1, const float* We2, const float* be2,
                        const float* Wg2, const float* bg2, const float* Wg3s, const float* Wg3h, const float* Wtw,
                        const float* btw, int64_t B, int Din, int Gin, int T, int S, int Sh, int H1, int O, int Og,
                        int last, float* y, float* out, float* h, float* e, float* q, float* g, void* stream);
int rec_ple_cgc_bwd_f32(const float* xin, const float* W1, const float* We2, const float* Wg2, const float* Wg3s,
                        const float* Wg3h, const float* Wtw, const float* h, const float* e, const float* q,
                        const float* g, const float* y, const float* out, const float* dy, const float* dout, int64_t B,
                        int Din, int Gin, int T, int S, int Sh, int H1, int O, int Og, int last, float* dxin, float* dW1,
                        float* db1, float* dWe2, float* dbe2, float* dWg2, float* dbg2, float* dWg3s, float* dWg3h,
                        float* dWtw, float* dbtw, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MIND (MultiInterestExtractorLayer, LabelAwareAttention, MINDLayer.call, 6.MIND/CustomLayers.py:62-158, 263-285;
 * csrc/mind.hip): capsule routing over a behaviour series, and label-aware attention with the sampled-softmax loss.
 * Both families gather from embed [V, E] with row stride ld >= E; an id outside [0, V) reads as a zero row and sets
 * *oob_flag (may be NULL).
 *
 * Capsule routing.  series int64 [B, T, C] as rec_din_attn_*, D = E C, S [D, Dc], B0 [K, T] (the layer's non-trainable
 * logits, the same for every example), R rounds.  Per example b:
 *   x_t = concat_r embed[series[b,t,r]]  [T, D]    valid_t = series[b,t,0] != padding_index    u = x S  [T, Dc]
 *   L = B0;  R times:  W = softmax_t(valid_t ? L : -FLT_MAX)  [K, T],  c = squash(W u)  [K, Dc],
 *                      and in every round but the last  L += c u^T
 *   out[b] = c                                                                                    out [B, K, Dc]
 * squash(s) = s n / (1 + n^2), n = |s|: at n = 0 it is 0 with a zero gradient, the limit of the reference's
 * n^2 / ((1 + n^2) n), which is 0/0 there.  -FLT_MAX is the lowest finite float: an example with no valid position gets
 * the uniform weights 1 / T over all T positions, padded ones included, and never NaN.  Padding may sit anywhere.
 * The forward is one launch and saves nothing but out.  The backward takes gout [B, K, Dc], runs the rounds again from
 * the ids and differentiates through all of them (no stop_gradient; B0 gets nothing): gkeys [B, T, D], the
 * IndexedSlices values of the series lookups as rec_din_attn_bwd_f32's, and dS [D, Dc], both written, never added to.
 * dS is reduced through one partial per workgroup of a capped grid and a slot sum in wave order.
 * Supported, the same both ways: D = E C <= REC_DIN_MAX_D (256), Dc <= REC_DIN_MAX_D, K <= REC_AFM_MAX_A (16),
 * 1 <= R <= REC_CAPSULE_MAX_R, 0 <= B < 2^31 and the backward's LDS within the launch cap REC_TILE_LDS_CAP (150 KiB):
 *   4 (T (D|1) + 2 T (Dc|1) + (R + 2) K T + 2 K (Dc|1) + T) <= 153600          (x|1: x made odd)
 * e.g. T <= 226 at D = Dc = 48, K = 4, R = 3 and T <= 35 at D = Dc = 256, K = 16, R = 3.
 * workspace (backward only): rec_mind_routing_workspace_bytes: min(B, 1024) partials of D Dc floats (at most 512 when dS
 * has more than four 32 x 32 blocks, 256 when more than sixteen); 0: invalid or unsupported shape.
 *
 * Label-aware attention + loss.  items int64 [B, Ns, C], Dc = E C, m [B, K, Dc] (the capsules after the final MLP),
 * kv int32 [B]: capsule k of example b is valid iff k < kv[b].  Per example:
 *   x_s = concat_r embed[items[b,s,r]]  [Ns, Dc]      sc[k,s] = m_k . x_s
 *   w[:,s] = softmax_k(k < kv ? sc[k,s] : -FLT_MAX)   (kv <= 0: uniform 1 / K)
 *   out[s] = sum_k w[k,s] sc[k,s]   (the unmasked scores: equal to (sum_k w[k,s] m_k) . x_s)          out [B, Ns]
 *   loss = logsumexp_s(out) - out[0]   (softmax cross entropy with the label at sample 0)            loss [B]
 * The forward is one launch for both.  The backward is one launch from gout [B, Ns] and gloss [B], either of which may
 * be NULL (not both): it recomputes the forward and writes gm [B, K, Dc] and gitems [B, Ns, Dc], the IndexedSlices
 * values of the item lookups.  A masked capsule's score is a constant inside the softmax: it receives the direct term
 * w[k,s] alone, which is zero unless every capsule is masked.
 * Supported: Dc = E C <= REC_DIN_MAX_D, K <= REC_AFM_MAX_A, 0 <= B < 2^31 and one example's LDS within the launch cap:
 *   4 ((K + Ns) (Dc|1) + 2 K Ns + 2 Ns) <= 153600
 * (a workgroup holds 4, 2 or 1 examples, as many as fit).  rec_mind_laa_lds_bytes: the dynamic LDS of a launch; 0:
 * invalid or unsupported shape.  There is no workspace.
 *
 * All four only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  Return codes, answered in this order: a size below 1 (B below 0): -1; a shape
 * outside the limits: -2, from the sizes alone; ld < E, V < 1 or a NULL pointer other than oob_flag / one of gout and
 * gloss: -1; a workspace that is too small: -3; then B == 0: 0, nothing is launched or written. */
size_t rec_mind_routing_workspace_bytes(int64_t B, int T, int E, int C, int Dc, int K, int R);
int rec_mind_routing_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                             int T, const float* S, const float* B0, int Dc, int K, int R, int64_t padding_index,
                             float* out, int* oob_flag, void* stream);
int rec_mind_routing_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                             int T, const float* S, const float* B0, int Dc, int K, int R, int64_t padding_index,
                             const float* gout, float* gkeys, float* dS, void* workspace, size_t workspace_bytes,
                             void* stream);
size_t rec_mind_laa_lds_bytes(int Ns, int E, int C, int K);
int rec_mind_laa_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items, int64_t B,
                         int Ns, const float* m, const int32_t* kv, int K, float* out, float* loss, int* oob_flag,
                         void* stream);
int rec_mind_laa_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items, int64_t B,
                         int Ns, const float* m, const int32_t* kv, int K, const float* gout, const float* gloss,
                         float* gm, float* gitems, void* stream);

/* ---- ComiRec (ComiRecDynamicRoutingLayer, ComiRecSelfAttentiveLayer, ComiRecLayer.manually_negative_sampled_call,
 * 6.MIND/CustomLayers.py:528-810; csrc/comirec.hip): dynamic routing with unshared weights, the self-attentive
 * extractor, and hard attention with the sampled-softmax loss.  All three gather from embed [V, E] with row stride
 * ld >= E; an id outside [0, V) reads as a zero row and sets *oob_flag (may be NULL).  series int64 [B, T, C], D = E C.
 * Position t of example b TAKES PART iff (series[b,t,0] == padding_index) == (keep_padding != 0): keep_padding = 1 is
 * the reference read literally (ComiRecLayer hands `series == padding_index` to a mask in which True means "takes
 * part"), keep_padding = 0 routes over the behaviours, as MIND does.  Padding may sit anywhere.  -FLT_MAX is the lowest
 * finite float: a row with no participating position gets the uniform weights 1 / T over all T positions, never NaN.
 * squash(s) = s n / (1 + n^2), n = |s|, 0 with a zero gradient at n = 0, as for MIND.
 *
 * (a) Dynamic routing.  W [K, T, D, Dc] (one matrix per capsule and position), B0 [K, T] (the layer's non-trainable
 * logits), R rounds.  Per example b:
 *   x_t = concat_r embed[series[b,t,r]]      u[k,t,:] = x_t W[k,t]      L = B0
 *   R times:  C = softmax_t(part_t ? L : -FLT_MAX)  [K, T],   c_k = squash(sum_t C[k,t] u[k,t,:]),
 *             and in every round but the last  L[k,t] += c_k . u[k,t,:]
 *   out[b] = c                                                                                    out [B, K, Dc]
 * The backward takes gout [B, K, Dc], recomputes u and the rounds and differentiates through all of them (no
 * stop_gradient; B0 gets nothing): gkeys [B, T, D], the IndexedSlices values of the series lookups, and dW [K, T, D, Dc],
 * both written, never added to.  The batch goes through in slabs of min(2048, max(32, 64 MiB / (4 K T Dc) rounded down
 * to 32)) examples; u [slab, K, T, Dc] lives in the workspace (du overwrites it), the projection and the two backward
 * products run on v_mfma_f32_32x32x2_f32 over 32-example tiles with W[k,t] read once per tile, and dW is reduced through
 * one partial per batch slice (at most 16) and a slot sum in serial order.  One wave owns a row (b, k) through the rounds.
 * Supported, the same both ways: D = E C <= REC_DIN_MAX_D (256), Dc <= REC_DIN_MAX_D, K <= REC_AFM_MAX_A (16),
 * 1 <= R <= REC_CAPSULE_MAX_R, 0 <= B < 2^31 and one row's LDS within the launch cap REC_TILE_LDS_CAP:
 *   4 (T (Dc|1) + (2 R + 3) T + 2 R (Dc|1)) <= 153600                          (x|1: x made odd)
 * e.g. T <= 657 at Dc = 48, R = 3 and T <= 124 at Dc = 256, R = 8.
 * workspace (BOTH directions): rec_comirec_dr_workspace_bytes: u of a slab plus, for the backward, slices K T D Dc
 * floats; the forward accepts one that holds u alone; 0: invalid or unsupported shape.
 *
 * (b) Self-attentive extractor.  W1 [D, Dc], W2 [K, Dc], pos [T, D] or NULL (no positional encoding).  Per example:
 *   h_t = tanh((x_t + pos_t) W1)   sc[k,t] = h_t . W2[k]   A = softmax_t(part_t ? sc : -FLT_MAX)
 *   out[b,k] = sum_t A[k,t] h_t     (the reference weights h, not the raw behaviours)             out [B, K, Dc]
 * One launch forward, one example per workgroup; the backward recomputes it and writes gkeys [B, T, D], dW1 [D, Dc] and
 * dW2 [K, Dc] (pos is a constant), the weight gradients through one partial per workgroup of a capped grid and a slot
 * sum in wave order.  Supported: D, Dc, K, B as above and the backward's LDS within the launch cap:
 *   4 (T (D|1) + 2 T (Dc|1) + 2 K T + 3 K (Dc|1) + T) <= 153600
 * e.g. T <= 242 at D = Dc = 48, K = 4.  workspace (backward only): rec_comirec_sa_workspace_bytes: min(B, 1024)
 * partials of (D + K) Dc floats (at most 512 / 256 when dW1 has more than four / sixteen 32 x 32 blocks).
 *
 * (c) Hard attention + loss.  items int64 [B, Ns, C], Dc = E C, m [B, K, Dc] (the capsules).  Per example:
 *   x_s = concat_r embed[items[b,s,r]]   p[s,k] = m_k . x_s
 *   chosen[s] = the smallest k with p[s,k] = max_k p[s,k]  (tf.argmax)   inner[s] = p[s, chosen[s]]
 *   loss = logsumexp_s(inner) - inner[0]   (softmax cross entropy with the label at sample 0)
 * Forward, one launch: chosen int32 [B, Ns], inner [B, Ns], loss [B].  Backward, one launch, from ginner [B, Ns] and
 * gloss [B], either of which may be NULL (not both), and gsel [B, Ns, Dc] or NULL, the gradient of the selected
 * capsules m[b, chosen[s]] themselves: gm [B, K, Dc] and gitems [B, Ns, Dc].  It reads chosen as the forward wrote it
 * (a value outside [0, K) is clamped) and never recomputes the argmax.  Supported: as rec_mind_laa_*, the same LDS
 * inequality; rec_comirec_select_lds_bytes: the dynamic LDS of a launch; 0: invalid or unsupported.  No workspace.
 *
 * All entry points only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  Return codes, answered in this order: a size below 1 (B below 0): -1; a shape
 * outside the limits: -2, from the sizes alone; ld < E, V < 1 or a NULL pointer other than oob_flag, pos, gsel / one of
 * ginner and gloss: -1; a workspace that is too small: -3; then B == 0: 0, nothing is launched or written. */
size_t rec_comirec_dr_workspace_bytes(int64_t B, int T, int E, int C, int Dc, int K, int R);
int rec_comirec_dr_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                           int T, const float* W, const float* B0, int Dc, int K, int R, int64_t padding_index,
                           int keep_padding, float* out, int* oob_flag, void* workspace, size_t workspace_bytes,
                           void* stream);
int rec_comirec_dr_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                           int T, const float* W, const float* B0, int Dc, int K, int R, int64_t padding_index,
                           int keep_padding, const float* gout, float* gkeys, float* dW, void* workspace,
                           size_t workspace_bytes, void* stream);
size_t rec_comirec_sa_workspace_bytes(int64_t B, int T, int E, int C, int Dc, int K);
int rec_comirec_sa_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                           int T, const float* W1, const float* W2, const float* pos, int Dc, int K,
                           int64_t padding_index, int keep_padding, float* out, int* oob_flag, void* stream);
int rec_comirec_sa_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                           int T, const float* W1, const float* W2, const float* pos, int Dc, int K,
                           int64_t padding_index, int keep_padding, const float* gout, float* gkeys, float* dW1,
                           float* dW2, void* workspace, size_t workspace_bytes, void* stream);
size_t rec_comirec_select_lds_bytes(int Ns, int E, int C, int K);
int rec_comirec_select_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items, int64_t B,
                               int Ns, const float* m, int K, int32_t* chosen, float* inner, float* loss, int* oob_flag,
                               void* stream);
int rec_comirec_select_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items, int64_t B,
                               int Ns, const float* m, int K, const int32_t* chosen, const float* ginner,
                               const float* gloss, const float* gsel, float* gm, float* gitems, void* stream);

/* ---- CAN co-action (CoActionUnit, 7.SIM/CustomLayers.py:285-378; csrc/can.hip): for every example the target item's
 * induction row IS the weights and biases of a small MLP, which is applied to every feed feature of the example raised
 * to the powers 1..O.  Both lookups happen inside the kernel.
 *   feed [Vf, E], row stride ld_f >= E;   ind_host: O pointers (a HOST array of device pointers; one pointer with
 *   shared = 1, read by every order) to tables [Vi, P], row stride ld_i >= P;   iid int64 [B];   fid int64 [B, T].
 * An id outside its table reads as a zero row and sets *oob_flag (may be NULL).  widths[0] = E, widths[l] = E c_l with
 * c_1..c_n = coefs_host (n = n_layers); P = sum_{l<n} (widths[l] widths[l+1] + widths[l+1]); a row holds layer after
 * layer, W_l row-major [widths[l], widths[l+1]] and then B_l.  Per example b, order o = 1..O and position t:
 *   x_0 = feed[fid[b,t]] ** o (elementwise, by repeated multiplication)        v = ind_o[iid[b]]
 *   x_{l+1} = act(x_l W_l + B_l)  for l < La                                  act: REC_ACT_NONE / RELU / SIGMOID / TANH
 *   out[o-1,b,t,:] = (fid[b,t] == padding_index) ? 0 : x_La                    out [O, B, T, Eo], Eo = widths[La]
 * La = min(n_layers, order) is the number of layers APPLIED: the reference zips its layers with a list of `order`
 * activations and so silently drops the layers beyond `order`; that is kept.  The row still has all P floats; the tail
 * no layer reads gets a zero gradient.  Padding may sit anywhere; a padded position still goes through the MLP in the
 * reference and is zeroed afterwards, so it contributes nothing to any gradient.
 * Two output modes, exactly one of out and pool is non-NULL:
 *   out  [O, B, T, Eo]  each order a contiguous [B, T, Eo], as the reference's list;
 *   pool [B, Eo] = sum_o sum_t out[o,b,t,:]  (concat(axis=1) + reduce_sum(axis=1) of CANLayer), added in a fixed order:
 *                 per order min(16, 256 / Eo) interleaved partial sums over t, these in ascending order onto the running
 *                 sum, orders ascending; out is never written.
 * The backward takes gout [O, B, T, Eo] or gpool [B, Eo] (exactly one non-NULL), runs the forward again (nothing is
 * saved) and writes, never adds:
 *   gfeed [B, T, E] = sum_o o feed^(o-1) dx_0(o), feed^0 = 1 exactly; orders ascending; zero at padded positions;
 *   gind [O, B, P]: the IndexedSlices values of each order's induction lookup: dW_l = sum_t x_l^T dz_l and
 *                   dB_l = sum_t dz_l added in position order, the tail beyond the La applied layers written as zeros.
 * One workgroup of 256 threads owns an example through all orders: the feed rows are read once, each induction row once
 * per (example, order), coalesced, into LDS (W_l rows padded to an odd stride); the products are f32 FMA chains out of
 * LDS, four positions per thread forward; dW is accumulated in registers over the positions and each gind row is
 * written once.  Supported, the same both ways: every widths[l] <= REC_AFM_MAX_E (64), 1 <= n_layers <= REC_CAN_MAX_L,
 * 1 <= order <= REC_CAN_MAX_L, T >= 1, 0 <= B < 2^31 and one example's working set within REC_TILE_LDS_CAP:
 *   4 (2 T E + Pv + T sum_{l<=La} (widths[l]|1) + 2 T (wmax|1) + T + 256) <= 153600                (x|1: x made odd)
 *   Pv = sum_{l<La} (widths[l] (widths[l+1]|1) + widths[l+1]),  wmax = max_{l<=La} widths[l]
 * e.g. T <= 276 at E = 16, coefs (1,1,1), order 3 (Pv = 864) and T <= 65 at E = 64, coefs (1,1), order 2 (Pv = 8448).
 * rec_can_lds_bytes: the left-hand side, the dynamic LDS of a backward launch; 0: invalid or unsupported.  No workspace.
 *
 * Both entry points only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  Return codes, answered in this order: a size below 1 (B below 0, a coefficient
 * below 1, coefs_host NULL): -1; a shape outside the limits: -2, from the sizes alone; ld_f < E, ld_i < P, Vf < 1,
 * Vi < 1, an unknown act, a NULL pointer other than oob_flag, or not exactly one of out / pool (gout / gpool): -1; then
 * B == 0: 0, nothing is launched or written. */
size_t rec_can_lds_bytes(int T, int E, int n_layers, const int* coefs_host, int order);
int rec_can_fwd_f32(const float* feed, int64_t ld_f, int64_t Vf, int E, const float* const* ind_host, int shared,
                    int64_t ld_i, int64_t Vi, int n_layers, const int* coefs_host, int order, int act,
                    const int64_t* iid, const int64_t* fid, int64_t B, int T, int64_t padding_index, float* out,
                    float* pool, int* oob_flag, void* stream);
int rec_can_bwd_f32(const float* feed, int64_t ld_f, int64_t Vf, int E, const float* const* ind_host, int shared,
                    int64_t ld_i, int64_t Vi, int n_layers, const int* coefs_host, int order, int act,
                    const int64_t* iid, const int64_t* fid, int64_t B, int T, int64_t padding_index, const float* gout,
                    const float* gpool, float* gfeed, float* gind, void* stream);

/* ---- SINE (SINELayer, 6.MIND/CustomLayers.py:966-1176; csrc/sine.hip): the sparse-interest extractor, whose examples
 * each select K of the L concepts of a pool, and the auxiliary loss of the pool.  The extractor gathers from embed [V, E]
 * with row stride ld >= E; an id outside [0, V) reads as a zero row and sets *oob_flag (may be NULL).  series int64
 * [B, T, C], D = E C, pool [L, D], W1 [D, D], W2 [D], Wk1 [L, D, D], Wk2 [L, D], W3 [D, D], W4 [D].
 * LN(r) = (r - mean) / sqrt(var + ln_eps) over the last axis with the population variance, no gamma, no beta (the
 * reference builds its LayerNormalization inside call: never trained, ln_eps = 1e-3).  Per example b:
 *   x_t = concat_r embed[series[b,t,r]]   pad_t = series[b,t,0] == padding_index
 *   (a) s_t = tanh(x_t W1) . W2 + (pad_t ? -1e9f : 0)    a = softmax_t(s)    z = sum_t a_t x_t
 *   (b) sim_l = z . pool_l    idx = top-K of sim: descending, the lower index first on equal values (tf.math.top_k)
 *       g_k = sigmoid(sim[idx_k])    Cu_k = g_k pool[idx_k]                                                     [K, D]
 *   (c) P[t,:] = softmax_k(LN(x_t W3) . LN(Cu_k))                                                               [T, K]
 *   (d) A[k,:] = softmax_t(tanh(x_t Wk1[idx_k]) . Wk2[idx_k])                                                   [K, T]
 *   (e) Z_k = LN(sum_t P[t,k] A[k,t] x_t)                                                                       [K, D]
 *   (f) Xh_t = sum_k P[t,k] Cu_k    b = softmax_t(tanh(Xh_t W3) . W4)    cap = LN(sum_t b_t Xh_t)
 *   (g) e = softmax_k(cap . Z_k / tau)    out[b] = sum_k e_k Z_k                                          out [B, D]
 * Only (a) masks padded positions; (c), (d) and (f) run over all T, as the reference does.  The mask is the additive
 * -1e9f in fp32: a row padded throughout gets the uniform 1 / T, never NaN.  Padding may sit anywhere.
 * The forward is one launch, one example per workgroup at a time; the 3 + K products [T, D] x [D, D] run on
 * v_mfma_f32_32x32x2_f32, the top-K is K rounds of an arg-max inside the workgroup.  It writes out and chosen int32
 * [B, K] (idx, in descending-similarity order) and saves nothing else.  The backward takes chosen as the forward wrote
 * it (a value outside [0, L) is clamped) and never re-selects; it recomputes (a)-(g) and differentiates through all of
 * it with idx constant, from gout [B, D]: gkeys [B, T, D], the IndexedSlices values of the series lookups, dpool [L, D]
 * (through Cu and through sim), dW1, dW2, dWk1 [L, D, D], dWk2 [L, D], dW3 (both uses) and dW4, every one written, never
 * added to; the rows of dpool, dWk1 and dWk2 that no example chose are zero.  The batch goes through in slabs of
 * min(2048, max(1, 64 MiB / (4 K (D D + 2 D)))) examples: an example-major launch keeps dW1 .. dW4 per workgroup (at most
 * 1024 workgroups; 256 where [D, D] has more than four 32 x 32 blocks) and writes x^T dpre_k, the row of dWk2 and the row
 * of dpool of every pair (b, k) to the scratch; a concept-major launch adds the pairs with chosen == l in ascending
 * (b, k) order, one thread per element (the first slab writes, later slabs add); a slot sum in wave order finishes
 * dW1 .. dW4.  Supported, the same both ways: D = E C <= REC_DIN_MAX_D (256), 1 <= K <= min(L, REC_AFM_MAX_A (16)),
 * L <= REC_SINE_MAX_L, 0 <= B < 2^31 and one example's LDS within the launch cap REC_TILE_LDS_CAP:
 *   4 (4 T (D|1) + 4 K T + L + 5 K (D|1) + 6 T + 8 (D|1) + 128) <= 153600                     (x|1: x made odd)
 * e.g. T <= 164 at D = 48, K = 5, L = 100.  rec_sine_lds_bytes: the left-hand side, the dynamic LDS of a launch; 0:
 * invalid or unsupported.  scratch (backward only): rec_sine_scratch_bytes: the pairs of a slab plus the slots; 0 likewise.
 *
 * aux.  Cc = pool - mean_l(pool), M = Cc Cc^T [L, L]: loss[0] = 0.5 sum_{i != j} M_ij^2; the backward takes gloss [1] ON
 * THE DEVICE and writes dpool = gloss (2 offdiag(M) Cc), pushed back through the centring.  L <= REC_SINE_MAX_L,
 * D <= REC_SINE_AUX_MAX_D.
 *
 * All entry points only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  Return codes, answered in this order: a size below 1 (B below 0), tau <= 0 or
 * ln_eps <= 0: -1; a shape outside the limits: -2, from the sizes alone; ld < E, V < 1 or a NULL pointer other than
 * oob_flag: -1; a scratch that is too small: -3; then B == 0: 0, nothing is launched or written. */
size_t rec_sine_lds_bytes(int T, int E, int C, int L, int K);
size_t rec_sine_scratch_bytes(int64_t B, int T, int E, int C, int L, int K);
int rec_sine_interest_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                              int T, const float* pool, const float* W1, const float* W2, const float* Wk1,
                              const float* Wk2, const float* W3, const float* W4, int L, int K, float tau, float ln_eps,
                              int64_t padding_index, float* out, int32_t* chosen, int* oob_flag, void* stream);
int rec_sine_interest_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                              int T, const float* pool, const float* W1, const float* W2, const float* Wk1,
                              const float* Wk2, const float* W3, const float* W4, int L, int K, float tau, float ln_eps,
                              int64_t padding_index, const int32_t* chosen, const float* gout, float* gkeys,
                              float* dpool, float* dW1, float* dW2, float* dWk1, float* dWk2, float* dW3, float* dW4,
                              void* scratch, size_t scratch_bytes, void* stream);
int rec_sine_aux_fwd_f32(const float* pool, int L, int D, float* loss, void* stream);
int rec_sine_aux_bwd_f32(const float* pool, int L, int D, const float* gloss, float* dpool, void* stream);

/* ---- FinalMLP (FinalMLPLayer / FeatureSelectionLayer / DualPartsInteractionLayer, 8.DMR/CustomLayers.py:319-442;
 * csrc/finalmlp.hip): everything between the three lookups and the output.
 * xs [B, D]: the shared rows, user fields first.  x1 [B, D1]: the rows of gate 1 (fs1_embedding of the ITEM ids),
 * x2 [B, D2]: those of gate 2 (fs2_embedding of the USER ids).  Hg1, Hg2: the hidden width of each gate.  L layers per
 * stream of widths widths1_host / widths2_host (HOST arrays of L ints); n heads, o outputs; d1, d2: the last widths.
 *   hg_s = relu(x_s Wh_s + bh_s)   g_s = 2 sigmoid(hg_s Wo_s + bo_s)   part_s = g_s (.) xs                      s = 1, 2
 *   z_s^0 = part_s W_s^0 + b_s^0   a_s^l = relu(xhat_s^l gamma_s^l + beta_s^l)   z_s^(l+1) = a_s^l W_s^(l+1) + b_s^(l+1)
 *   xhat = (z - mean) rstd, rstd = 1 / sqrt(var + eps), per column: training != 0 the batch mean and the biased batch
 *   variance, and moving <- momentum moving + (1 - momentum) batch on the device (eps and momentum are doubles so that
 *   1 - momentum is rounded to fp32 once, as Keras rounds it); training == 0 the moving statistics,
 *   nothing updated (Keras BatchNormalization; relu'(0) = 0)
 *   out = sigmoid(m_1 W_1 + c_1 + m_2 W_2 + c_2 + sum_h m_1h^T W_12[h] m_2h)      m_s = a_s^(L-1), head h its columns
 *   [h d_s / n, (h + 1) d_s / n)                                                                           out [B, o]
 * params: ONE buffer, row-major tensors laid end to end without padding, in this order:
 *   Wh_1 [D1, Hg1], bh_1 [Hg1], Wo_1 [Hg1, D], bo_1 [D],   Wh_2 [D2, Hg2], bh_2 [Hg2], Wo_2 [Hg2, D], bo_2 [D],
 *   stream 1, l = 0 .. L-1: W [in, w], b [w], gamma [w], beta [w] (in = D, then the width before),   stream 2 likewise,
 *   W_1 [d1, o], c_1 [o], W_2 [d2, o], c_2 [o], W_12 [n, d1 / n, d2 / n, o]
 * dparams: the gradients in the same layout, every float written, never added to.
 * moving_mean_host, moving_var_host: HOST arrays of 2 L device pointers (stream 1 layer 0 .. L-1, then stream 2), each
 * to the [w] floats of that layer; read at enqueue time.
 * Save buffers hg [B, Hg1 + Hg2], g [B, 2 D] (g_1 | g_2), z and a [B, Z] with Z = sum_l (w1_l + w2_l) and the columns
 * layer-major (layer 0: stream 1, stream 2; layer 1: ...), stats [2, Z] (mean row, rstd row): all given or all NULL;
 * training != 0 needs them (z carries the chain from launch to launch).  Inference without them writes out alone, the
 * same out.
 * Forward, training == 0: one launch.  training != 0: 2 L + 1 launches whatever B: a launch ends where the next batch
 * statistic is needed and leaves z^l and, per 32-example tile and column, (count, mean, M2 about that mean); a merge
 * launch folds the tiles in a fixed order with the pairwise update of Chan, Golub and LeVeque (the variance is never
 * formed as E[x^2] - mean^2), writes mean and rstd and moves the moving averages; the last launch runs the head.
 * Every product runs on v_mfma_f32_32x32x2_f32 (fp32-exact, as rec_gemm_f32), the head on the VALU out of LDS.
 * Backward: takes dout [B, o], out and the save buffers, writes dxs [B, D], dx1 [B, D1], dx2 [B, D2] (written, never
 * added to) and dparams.  L + 1 stage launches (head, then layer L-1 .. 0 and the gates), each followed by a slot sum
 * that lands the stage's column sums in dparams (dgamma / dbeta of a layer are the batch sums the next stage's full
 * BatchNorm backward reads); one launch for dW_1, dW_2, dW_12 over at most 16 batch slices added in order by a slot
 * sum; every other weight gradient on rec_gemm_f32 (split-K over the batch in at most 16 slices, added in order).
 * training != 0: the gradient of a bias b_s^l is sum_b dz = 0 identically and is written as exact zeros.
 * All three only enqueue (no allocation, no host synchronisation: graph-capturable) and use no float atomics:
 * bit-identical results run to run.  B == 0: nothing is launched.  B == 1, training: xhat is exactly 0.
 * Supported: the limits are MaskNet's, this family has no constants of its own: each of D, D1, D2
 * <= REC_MASKNET_MAX_D, each of Hg1, Hg2 and every stream width <= REC_MASKNET_MAX_O, 1 <= L <= REC_MASKNET_MAX_R,
 * 1 <= o <= REC_MASKNET_MAX_R, (d2 / n) o <= REC_MASKNET_MAX_O, 0 <= B < 2^31; otherwise -2.  A size below 1 (B below
 * 0), n not dividing d1 and d2, a NULL widths array, training other than 0 / 1, eps <= 0, momentum outside [0, 1], a
 * NULL pointer or save buffers given in part: -1.  A workspace that is too small: -3.
 * workspace (forward when training != 0, and backward): rec_finalmlp_scratch_bytes: 4 B (Z + o + d2 o + 4 D + Hg1 +
 * Hg2) bytes of per-example gradients and operands, (B / 32) slots, at most 16 copies of the head weights and at most
 * 16 of the largest other weight (0: invalid or unsupported shape). */
size_t rec_finalmlp_scratch_bytes(int64_t B, int D, int D1, int D2, int Hg1, int Hg2, int L, const int* widths1_host,
                                    const int* widths2_host, int n, int o);
int rec_finalmlp_fwd_f32(const float* xs, const float* x1, const float* x2, const float* params,
                         float* const* moving_mean_host, float* const* moving_var_host, int64_t B, int D, int D1, int D2,
                         int Hg1, int Hg2, int L, const int* widths1_host, const int* widths2_host, int n, int o,
                         int training, double eps, double momentum, float* out, float* hg, float* g, float* z, float* a,
                         float* stats, void* workspace, size_t workspace_bytes, void* stream);
int rec_finalmlp_bwd_f32(const float* xs, const float* x1, const float* x2, const float* params, const float* hg,
                         const float* g, const float* z, const float* a, const float* stats, const float* out,
                         const float* dout, int64_t B, int D, int D1, int D2, int Hg1, int Hg2, int L,
                         const int* widths1_host, const int* widths2_host, int n, int o, int training, float* dxs,
                         float* dx1, float* dx2, float* dparams, void* workspace, size_t workspace_bytes, void* stream);

/* ---- DMR (DMRI2INetworkLayer / DMRU2INetworkLayer / compute_auxiliary_loss, 8.DMR/CustomLayers.py:203-316;
 * csrc/dmr.hip): both attention units over the looked-up behaviour series and the auxiliary match loss, one launch each
 * way.  series int64 [B, T, C], negatives int64 [B, Nn, C], D = E C; xi [B, D] the candidate item's rows; q [B, H] =
 * xi Wc and P [T, 2H] = pos [Wp_i2i | Wp_u2i], both made by the caller (rec_gemm_f32); We [D, 2H] = [We_i2i | We_u2i];
 * z [2, H] = z_i2i, z_u2i.  Unit 0 is i2i, unit 1 u2i.  Per example, x_t = concat_r embed[series[b,t,r]]:
 *   valid_t = series[b,t,0] != padding_index   n = sum_t valid_t   last = n - 1
 *   h_t = tanh(([q | 0] + x_t We) + P_t)       s[u,t] = z_u . h_t[uH : (u+1)H]
 *   A_u = softmax over the valid t of s[u], 0 elsewhere (all 0 where n = 0)
 *   i2i = [sum_t A_0[t] x_t, sum_valid s[0,t]]                                                         i2i [B, D + 1]
 *   u = sum_t A_1[t] x_t    u2i = [u, u . xi]                                                           u2i [B, D + 1]
 *   lv = A_1[last] x_last   ov = sum_{t < last} A_1[t] x_t   nrm(v) = v / sqrt(max(sum v^2, 1e-12))
 *   cos(p, q) = sum nrm(p) nrm(q)   pos = (1 - cos(lv, ov)) / 2   neg_j = (1 - cos(xneg_j, ov)) / 2
 *   aux = softplus(-pos) + sum_j softplus(neg_j)   (0 where n = 0: the reference fails there)             aux [B]
 * Nothing is saved.  The backward takes g_i2i [B, D + 1], g_u2i [B, D + 1] and g_aux [B], each of which may be NULL
 * (exact zeros), recomputes the forward from the ids and writes, never adds to: gkeys [B, T, D] and gneg [B, Nn, D],
 * the IndexedSlices values of the two lookups; gitem [B, D] (through u . xi only); gq [B, H]; dP [T, 2H], dWe [D, 2H],
 * dz [2, H], summed over the batch through one slot per workgroup of a capped grid and a slot sum in wave order.  The
 * clamp inside nrm has TF's gradient (a constant factor 1e6 where sum v^2 < 1e-12).  One example per workgroup; x We,
 * dh We^T and x^T dh run on v_mfma_f32_32x32x2_f32.  Both only enqueue (no allocation, no host synchronisation:
 * graph-capturable) and use no float atomics: bit-identical results run to run.
 * Supported, the same both ways: D = E C <= REC_DIN_MAX_D (256), H <= REC_DIN_MAX_D, 0 <= B < 2^31 and one example's
 * LDS within the launch cap REC_TILE_LDS_CAP (rec_dmr_lds_bytes; 0: invalid or unsupported):
 *   4 (T ((D|1) + (2H|1) + 7) + Nn ((D|1) + 3) + 8 (D|1) + 5 H + 16) <= 153600                (x|1: x made odd)
 * e.g. T <= 244 at D = H = 48, Nn = 6.  scratch (backward only): rec_dmr_scratch_bytes: min(B, 1024) slots of
 * (D + T + 1) 2H floats (at most 512 / 256 slots when dWe has more than eight / sixteen 32 x 32 blocks); 0: invalid or
 * unsupported.  Return codes, answered in this order: a size below 1 (B below 0): -1; a shape outside the limits: -2,
 * from the sizes alone; ld < E, V < 1 or a NULL pointer other than oob_flag, g_i2i, g_u2i, g_aux: -1; a scratch that is
 * too small: -3; then B == 0: 0, nothing is launched or written. */
size_t rec_dmr_lds_bytes(int T, int E, int C, int H, int Nn);
size_t rec_dmr_scratch_bytes(int64_t B, int T, int E, int C, int H, int Nn);
int rec_dmr_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B, int T,
                    const int64_t* negatives, int Nn, const float* xi, const float* q, const float* P, const float* We,
                    const float* z, int H, int64_t padding_index, float* i2i, float* u2i, float* aux, int* oob_flag,
                    void* stream);
int rec_dmr_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B, int T,
                    const int64_t* negatives, int Nn, const float* xi, const float* q, const float* P, const float* We,
                    const float* z, int H, int64_t padding_index, const float* g_i2i, const float* g_u2i,
                    const float* g_aux, float* gkeys, float* gneg, float* gitem, float* gq, float* dP, float* dWe,
                    float* dz, void* scratch, size_t scratch_bytes, void* stream);

/* ---- PEPNet (PEPNetLayer / PosoForMLPLayer / GateNULayer, 10.POSO/CustomLayers.py:76-119, 371-462; csrc/epnet.hip,
 * csrc/poso.hip).  GateNU(v) = 2 sigmoid(relu(v A + a) Bm + bm).
 * EPNet lookup.  ids int64 [B, F + P] into ONE table [V, E] with row stride ld: F main ids, then P personalisation ids.
 * Packed gate weights, row-major: A [F, P E, Hg], a [F, Hg], Bm [F, Hg, E], bm [F, E].  Per example:
 *   pp = concat_p table[ids[F + p]]  [P E]        gate_f = GateNU_f(pp)  [E]
 *   u[f E + e] = gate_f[e] table[ids[f]][e]  (f < F)      u[F E + k] = pp[k]                            u [B, (F + P) E]
 * u is the gate input of the towers below and its leading F E columns their main input.  An id outside [0, V) reads row
 * 0 and sets *oob_flag (may be NULL).  Nothing is saved: the backward takes du [B, (F + P) E], recomputes the gates from
 * the ids and writes, never adds to: drows [B, F + P, E], the IndexedSlices values of the lookup (main rows du (.) gate,
 * pp rows du plus the gradient through all F gates), and dA, da, dBm, dbm, summed over the batch through one slot per
 * workgroup (at most 256, each walking its tiles of 32 examples in order) and a slot sum in wave order.
 * Supported (the limits are MaskNet's, this family has no constants of its own): 1 <= F <= REC_MASKNET_MAX_F,
 * 1 <= E <= REC_MASKNET_MAX_E, 1 <= Hg <= REC_MASKNET_MAX_E, 1 <= P,
 * P E <= REC_MASKNET_MAX_O, (F + P) E <= REC_MASKNET_MAX_D, 0 <= B < 2^31; otherwise -2.  A size below 1 (B below 0),
 * V < 1, ld < E or a NULL pointer other than oob_flag: -1.  A workspace that is too small: -3.  workspace (backward
 * only): rec_epnet_lookup_scratch_bytes: min(ceil(B / 32), 256) slots of F (P E Hg + Hg + Hg E + E) floats (0: invalid
 * or unsupported shape).
 * POSO-MLP.  x [B, Dm] with row stride ldx and g [B, Dg] with row stride ldg (both may point into one u); T tasks of L
 * chained layers of widths U_i = units_host[i] (a HOST int array, as acts_host: REC_ACT_NONE / _RELU / _SIGMOID);
 * m = gate_hidden_multiple, H_i = m U_i, sumU = sum_i U_i, NG = T m sumU, K_0 = Dm, K_i = U_{i-1}.  Packed weights,
 * row-major, (t, i) task-major:
 *   Wg1 [Dg, NG], bg1 [NG]   the first gate layers side by side; the H_i columns of (t, i) start at m (t sumU + sum_{j<i} U_j)
 *   Wg2   the [H_i, U_i] of every (t, i) one after the other     bg2 [T, sumU]
 *   W     the [K_i, U_i] of every (t, i) one after the other     b [T, sumU]     C [T, L]
 * Per example (relu'(0) = 0), a_t,-1 = x:
 *   h_ti = relu(g Wg1_ti + bg1_ti)   gate_ti = 2 sigmoid(h_ti Wg2_ti + bg2_ti)   d_ti = a_t,i-1 W_ti + b_ti
 *   a_ti = act_i(C_ti (d_ti (.) gate_ti))          out[:, t, :] = a_t,L-1                            out [B, T, U_{L-1}]
 * The reference as written (every layer reads x, only the last one is returned) is L = 1 on the last layer's
 * parameters.  One launch: a workgroup owns 32 examples, every product runs on v_mfma_f32_32x32x2_f32 (fp32-exact).  The
 * save buffers h [B, NG], gate, d_out, a [B, T sumU] are all given (training) or all NULL (inference: only out is
 * written; the same out).  The backward takes dout [B, T, U_{L-1}] and the save buffers and writes, never adds to:
 * dx [B, Dm] and dg [B, Dg] (contiguous, separately: the caller decides what reaches a shared buffer) and the gradient
 * of every packed weight: one launch for the per-example chain, one slot sum (dbg1, dbg2, db, dC), ONE launch for all dW
 * and dWg2 over at most 16 batch slices added in order by a second slot sum, and dWg1 = g^T dZ on rec_gemm_f32 (split-K,
 * slices added in order).  Both only enqueue (no allocation, no host synchronisation: graph-capturable) and use no
 * float atomics: bit-identical results run to run.  B == 0: nothing is launched.
 * Supported: 1 <= T <= REC_MASKNET_MAX_R, 1 <= L <= REC_MASKNET_MAX_R, U_i <= REC_MASKNET_MAX_O, m U_i <= REC_MASKNET_MAX_P,
 * Dm, Dg <= REC_MASKNET_MAX_D, an activation of the three above, 0 <= B < 2^31, and the forward's tile within the LDS of
 * a CU: 132 (even(Dg) + max(even(m Umax), even(Dm)) + (L > 1 ? 2 : 1) even(Umax)) <= REC_POSO_LDS_CAP (every L = 1
 * shape inside the limits does; L > 1 with Dg and max(Dm, m Umax) both near 512 does not); otherwise -2.  A size below
 * 1 (B below 0), ldx < Dm, ldg < Dg, a NULL pointer or save buffers given in part: -1.  A workspace that is too small:
 * -3.  workspace (backward only): rec_poso_mlp_scratch_bytes: 4 B (NG + 2 T sumU) bytes of per-example gradients, (B / 32) slots of
 * NG + 2 T sumU + T L floats, at most 16 copies of W and Wg2 and at most 16 of Wg1 (0: invalid or unsupported shape). */
size_t rec_epnet_lookup_scratch_bytes(int64_t B, int F, int P, int E, int Hg);
int rec_epnet_lookup_fwd_f32(const float* table, int64_t V, int64_t ld, const int64_t* ids, const float* A,
                             const float* a, const float* Bm, const float* bm, int64_t B, int F, int P, int E, int Hg,
                             float* u, int* oob_flag, void* stream);
int rec_epnet_lookup_bwd_f32(const float* table, int64_t V, int64_t ld, const int64_t* ids, const float* A,
                             const float* a, const float* Bm, const float* bm, const float* du, int64_t B, int F, int P,
                             int E, int Hg, float* drows, float* dA, float* da, float* dBm, float* dbm, void* workspace,
                             size_t workspace_bytes, void* stream);
size_t rec_poso_mlp_scratch_bytes(int64_t B, int Dm, int Dg, int T, int L, const int* units_host,
                                    int gate_hidden_multiple);
int rec_poso_mlp_fwd_f32(const float* x, int64_t ldx, const float* g, int64_t ldg, const float* Wg1, const float* bg1,
                         const float* Wg2, const float* bg2, const float* W, const float* b, const float* C, int64_t B,
                         int Dm, int Dg, int T, int L, const int* units_host, const int* acts_host,
                         int gate_hidden_multiple, float* out, float* h, float* gate, float* d_out, float* a,
                         void* stream);
int rec_poso_mlp_bwd_f32(const float* x, int64_t ldx, const float* g, int64_t ldg, const float* Wg1, const float* Wg2,
                         const float* W, const float* C, const float* h, const float* gate, const float* d_out,
                         const float* a, const float* dout, int64_t B, int Dm, int Dg, int T, int L,
                         const int* units_host, const int* acts_host, int gate_hidden_multiple, float* dx, float* dg,
                         float* dWg1, float* dbg1, float* dWg2, float* dbg2, float* dW, float* db, float* dC,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- DIEN (DIENLayer / DienGRU / CustomGRUCell / DienActivationLayer, 5.DIN/CustomLayers.py:292-517; csrc/dien.hip):
 * the interest extractor (a masked tf.keras.layers.GRU fused with the series and negative lookups and the auxiliary
 * loss) and the interest evolution (attention scores fused with an AGRU / AUGRU).  H = D = E C everywhere.  One cell
 * serves all three recurrences: gate blocks [z | r | h] of H columns each, Wx [H, 3H] on the input, Uh [H, 3H] on the
 * state (AGRU: [r | h], [H, 2H]); valid[b,t] = (mask id != padding_index); where it is false h_t = h_{t-1} (h_{-1} = 0),
 * anywhere in the row:
 *   pre = x_t Wx + bx   rec = h Uh + bh   z = sigmoid(pre_z + rec_z)   r = sigmoid(pre_r + rec_r)
 *   hh = tanh(pre_h + r (.) rec_h)
 *   GRU     h_t = z h + (1 - z) hh        kernel = Wx, recurrent_kernel = Uh, bias [2, 3H] = [bx ; bh] (reset_after=True)
 *   AUGRU   h_t = (1 - a z) h + a z hh    Wx = [W_z | W_r | W_h], Uh = [U_z | U_r | U_h], bx = [b_z | b_r | b_h], bh = 0
 *   AGRU    h_t = (1 - a) h + a hh        Wx = [W_r | W_h], Uh = [U_r | U_h], bx = [b_r | b_h]
 * rec_dien_gru_*.  Table mode (embed != NULL; x and mask_ids NULL): x_t = concat_r embed[series[b,t,r]], series int64
 * [B, T, C], the mask ids are series[b,t,0]; an id outside [0, V) reads a zero row and sets *oob_flag (may be NULL).
 * Dense mode (embed NULL): x [B, T, H] and mask_ids int64 [B, T]; negatives must be NULL.  The forward writes
 * gru_output [B, T, H] (every h_t) and / or h_final [B, H]: either may be NULL, not both.  negatives int64 [B, T, C]
 * (table mode, may be NULL): aux [1] = sum over b and t >= 1 of valid[b,t] (ce(sigmoid(x_{t-1} . h_t), 1) +
 * ce(sigmoid(x_{t-1} . neg_t), 0)), ce(v, l) = max(v, 0) - v l + log1p(exp(-|v|)); T = 1 gives 0.  It is summed
 * through one slot per workgroup in the scratch, which only this case needs (the others accept NULL).
 * The backward takes gru_output (the forward's, always [B, T, H]), dgru_output [B, T, H], dh_final [B, H] and gaux [1]
 * (each may be NULL: exact zeros), recomputes the gates and writes, never adds to: dx [B, T, H], the IndexedSlices
 * values of the series lookup (table mode) or the gradient of x; dneg [B, T, H] the values of the negative lookup (with
 * negatives; position 0 is zero); dkernel, drecurrent_kernel [H, 3H], dbias [2, 3H].
 * rec_dien_augru_*.  mode REC_DIEN_AUGRU or REC_DIEN_AGRU.  gru_output [B, T, H] is the input, q [B, H] = X_item W^T (made
 * by the caller, rec_gemm_f32), mask_ids[(b T + t) mask_stride] the mask ids.  product[b,t] = gru_output[b,t] . q[b],
 * e = sel ? exp(product) : 0 with sel = !valid (mask_valid = 0, the reference: only PADDED positions score) or valid
 * (mask_valid = 1), scores = e / sum_t e with NaN -> 0 (a row with nothing selected scores zeros) [B, T], always
 * written; a = scores.  states [B, T, H] (every h_t; may be NULL in inference) and h_final [B, H].  The backward takes
 * scores, states and dh_final and writes dgru_output [B, T, H] (through the cell and through the scores), dq [B, H],
 * dWx, dUh, dbx in the packed layout; rows whose scores were NaN -> 0 get zero through the scores.
 * All four: one recurrence launch that walks t inside the kernel, a workgroup of 4 waves per 32 examples, products on
 * v_mfma_f32_32x32x2_f32 (fp32-exact); the backward adds one slot sum for the bias gradients and three rec_gemm_f32
 * (split-K over B T, slices added in order) for dWx = X^T dpre and dUh = Hprev^T drec out of the scratch.  They only
 * enqueue (graph-capturable) and use no float atomics: bit-identical results run to run.
 * Supported, the same both ways: 1 <= H <= REC_DIN_WIDE_D (128), T >= 1, 0 <= B < 2^31 and the tile's LDS within the
 * launch cap REC_TILE_LDS_CAP (rec_dien_gru_lds_bytes, rec_dien_augru_lds_bytes; 0: invalid or unsupported), He = H
 * made even:
 *   GRU     132 * 8 He + 512 <= 153600                       (every H up to 128, any T)
 *   AUGRU   132 * (7 He + 2 T) + 512, AGRU 132 * (6 He + 2 T) + 512 <= 153600      (T <= 131 at H = 128, <= 243 at 96)
 * scratch: rec_dien_gru_scratch_bytes (backward = 0: the forward's aux slots; 1: the backward's) and
 * rec_dien_augru_scratch_bytes (backward only): B T (6 H or 5 H) floats of per-step gradients and operands, at most
 * 2048 slots of 2 ng H floats, 16 split-K slices of [H, ng H]; 0: invalid or unsupported.
 * Return codes, in this order: a size below 1 (B below 0) or an unknown mode: -1; a shape outside the limits: -2, from
 * the sizes alone; ld < E, V < 1, E C != H, a pointer that must (not) be NULL: -1; a scratch that is too small: -3; then
 * B == 0: 0, nothing is launched or written. */
size_t rec_dien_gru_lds_bytes(int T, int H);
size_t rec_dien_augru_lds_bytes(int T, int H, int mode);
size_t rec_dien_gru_scratch_bytes(int64_t B, int T, int H, int backward);
size_t rec_dien_augru_scratch_bytes(int64_t B, int T, int H, int mode);
int rec_dien_gru_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                         const int64_t* negatives, const float* x, const int64_t* mask_ids, int64_t B, int T, int H,
                         const float* kernel, const float* recurrent_kernel, const float* bias, int64_t padding_index,
                         float* gru_output, float* h_final, float* aux, int* oob_flag, void* scratch,
                         size_t scratch_bytes, void* stream);
int rec_dien_gru_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                         const int64_t* negatives, const float* x, const int64_t* mask_ids, int64_t B, int T, int H,
                         const float* kernel, const float* recurrent_kernel, const float* bias, int64_t padding_index,
                         const float* gru_output, const float* dgru_output, const float* dh_final, const float* gaux,
                         float* dx, float* dneg, float* dkernel, float* drecurrent_kernel, float* dbias, void* scratch,
                         size_t scratch_bytes, void* stream);
int rec_dien_augru_fwd_f32(const float* gru_output, const float* q, const int64_t* mask_ids, int64_t mask_stride,
                           int64_t B, int T, int H, int mode, const float* Wx, const float* Uh, const float* bx,
                           int64_t padding_index, int mask_valid, float* scores, float* states, float* h_final,
                           void* stream);
int rec_dien_augru_bwd_f32(const float* gru_output, const float* q, const int64_t* mask_ids, int64_t mask_stride,
                           int64_t B, int T, int H, int mode, const float* Wx, const float* Uh, const float* bx,
                           int64_t padding_index, int mask_valid, const float* scores, const float* states,
                           const float* dh_final, float* dgru_output, float* dq, float* dWx, float* dUh, float* dbx,
                           void* scratch, size_t scratch_bytes, void* stream);

/* ---- SIM (SIMLayer / ESULayer, 7.SIM/CustomLayers.py:130-282; csrc/sim.hip): the soft search fused with the GSU
 * pooling, and the one-query multi-head attention of the exact search unit.  D = E C.
 * rec_sim_search_*.  key k_t = concat_r embed[series[b,t,r]], valid[b,t] = series[b,t,0] != padding_index.  scores
 * [B,T] = valid <q, k_t> and pooled [B,D] = sum_t scores_t k_t are those of rec_ip_attn_fwd_f32.  The ranked value is
 * <q, k_t> for a valid step and -inf for a padded one (a NaN ranks as -inf); chosen int32 [B,K] holds the K <= T
 * positions in descending order, on equal values the lower index first (tf.argsort(direction='DESCENDING')[:, :K]; it
 * also orders the -inf entries when fewer than K steps are valid).  A score depends on the values of its key and of q
 * only, so steps with the same ids tie bit for bit.  sel [B,K,D] is the key at chosen[b,j], read for padded positions
 * too; sel_valid int32 [B,K] = valid[b, chosen[b,j]].  An id outside [0, V) reads a zero row and sets *oob_flag (may be
 * NULL).  The backward writes, never adds to, gkeys [B,T,D] = scores_t gpooled + valid <gpooled, k_t> q, plus gsel[b,j,:]
 * (may be NULL: none) where chosen[b,j] == t -- the IndexedSlices values of the one series lookup -- and gq [B,D] as
 * rec_ip_attn_bwd_f32 does (the selection sends nothing to q).  One launch each way, one workgroup per example.
 * Supported: D <= REC_SEARCH_MAX_D, K <= REC_SEARCH_MAX_K, V and B < 2^31, 4 (T C + 4 D + T + REC_SEARCH_MAX_K) <=
 * REC_SEARCH_LDS_CAP bytes of LDS (rec_sim_search_lds_bytes:
 * that sum, 0: invalid or unsupported).
 * rec_esu_attn_*.  Keras 2.x MultiHeadAttention (value_dim = key_dim, no dropout) with one query q [B,D] over K dense
 * keys x [B,K,D], mask int32 [B,K] (non-zero = attend), Wq, Wk, Wv [D,H,dk], bq, bk, bv [H,dk], Wo [H,dk,D], bo [D]:
 *   Q_h  = (q Wq_h + bq_h) / sqrt(dk)          K_jh = x_j Wk_h + bk_h          V_jh = x_j Wv_h + bv_h
 *   l_hj = <Q_h, K_jh>      a_hj = float32(l_hj + (1 - mask_j) * (-1e9))       p_h = softmax_j(a_h)
 *   out  = sum_h (sum_j p_hj V_jh) Wo_h + bo
 * The mask is additive in fp32, not a select: a row with every position masked has a_hj = -1e9 exactly for |l| < 32,
 * hence p = 1/K, and the backward is the softmax Jacobian dl_hj = p_hj (g_hj - <p_h, g_h>) for every j, masked or not.
 * out [B,D]; probs [B,H,K] = p (may be NULL).  The kernels use the collapsed form u_h = Wk_h Q_h, l_hj = <x_j, u_h> +
 * <bk_h, Q_h>, sum_j p_hj V_jh = (sum_j p_hj x_j) Wv_h + bv_h; dbk, zero in exact arithmetic, comes out as rounding
 * residue of sum_j dl_hj.  The backward takes gout [B,D] and writes, never adds to, gq [B,D], gx [B,K,D] and the eight
 * weight gradients: one launch for the chain (a workgroup of 4 waves per 32 examples, products on
 * v_mfma_f32_32x32x2_f32), a slot sum for dbq, dbv, dbo and one launch plus a slot sum for the 5 H per-head matrices of
 * dWq, dWk, dWv, dWo, dbk over at most 16 batch slices added in order.  No float atomics: bit-identical run to run.
 * Supported: D, dk <= REC_ESU_MAX_D and even, H <= REC_ESU_MAX_H, K <= REC_SEARCH_MAX_K, B < 2^31 and
 * 132 (max(H dk, H D) + 2 + 2 H K + H) <= REC_TILE_LDS_CAP bytes of LDS (rec_esu_attn_lds_bytes: that product, 0: invalid
 * or unsupported; inside the other limits it is at most 102696).  scratch: rec_esu_attn_scratch_bytes,
 * what the backward needs (the forward needs less): 4 B (4 H dk + 4 H D + H) bytes of per-example operands, (B / 32)
 * slots and at most 16 copies of the weights; 0: invalid or unsupported.
 * Return codes, in this order: a size below 1 (B below 0): -1; a shape outside the limits: -2, from the sizes alone; a
 * leading dimension that is too small or K > T: -1; B == 0: 0, nothing is launched or written; a pointer that must not
 * be NULL: -1; a scratch that is too small: -3. */
size_t rec_sim_search_lds_bytes(int T, int C, int E, int K);
size_t rec_esu_attn_lds_bytes(int K, int D, int H, int dk);
size_t rec_esu_attn_scratch_bytes(int64_t B, int K, int D, int H, int dk);
int rec_sim_search_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                           int T, const float* q, int64_t ld_q, int64_t padding_index, int K, float* scores,
                           float* pooled, int64_t ld_pooled, int* chosen, float* sel, int* sel_valid, int* oob_flag,
                           void* stream);
int rec_sim_search_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                           int T, const float* q, int64_t ld_q, int64_t padding_index, int K, const float* scores,
                           const float* gpooled, int64_t ld_gpooled, const int* chosen, const float* gsel, float* gkeys,
                           float* gq, void* stream);
int rec_esu_attn_fwd_f32(const float* q, int64_t ld_q, const float* x, const int* mask, int64_t B, int K, int D, int H,
                         int dk, const float* Wq, const float* bq, const float* Wk, const float* bk, const float* Wv,
                         const float* bv, const float* Wo, const float* bo, float* out, float* probs, void* scratch,
                         size_t scratch_bytes, void* stream);
int rec_esu_attn_bwd_f32(const float* q, int64_t ld_q, const float* x, const int* mask, int64_t B, int K, int D, int H,
                         int dk, const float* Wq, const float* bq, const float* Wk, const float* bk, const float* Wv,
                         const float* bv, const float* Wo, const float* gout, int64_t ld_gout, float* gq, float* gx,
                         float* dWq, float* dbq, float* dWk, float* dbk, float* dWv, float* dbv, float* dWo, float* dbo,
                         void* scratch, size_t scratch_bytes, void* stream);

/* ---- ETA (ETALayer, 7.SIM/CustomLayers.py:518-626; csrc/eta.hip): the SimHash search of the long behaviour series.
 * D = E C.  key k_t = concat_c embed[series[b,t,c]], valid[b,t] = series[b,t,0] != padding_index (the first column
 * alone).  q [B,D] is the candidate's rows, Hm [D,m] row-major the frozen projection.  The code of a row x is
 * c(x)_j = sign(sum_d x_d Hm[d,j]) in {-1, 0, +1} as tf.sign gives it in fp32: a zero projection gives 0 (a zero row
 * gives m of them), a NaN projection equals nothing.  A code depends on the values of its row and of Hm only -- not on
 * t, T, the lane or ld -- so steps with the same ids get the same codes bit for bit.  scores int32 [B,T] (may be NULL) =
 * #{ j : c(k_t)_j == c(q_b)_j } in [0, m], for every step, padded ones too.  A valid step ranks by its score, a padded
 * one as -inf (the reference adds mask * (-inf), NaN for every valid step; the intent is kept, as rec_sim_search does).
 * chosen int32 [B,K] = argsort(rank, DESCENDING)[:, :K], on equal ranks the lower index first; it also orders the padded
 * steps when fewer than K are valid.  sel [B,K,D] is the key at chosen[b,j], read for padded positions too; sel_valid
 * int32 [B,K] = valid[b, chosen[b,j]]; sel_ids int64 [B,K,C] the ids of the chosen steps as given.  An id outside [0, V)
 * reads a zero row and sets *oob_flag (may be NULL).  One launch, one workgroup per example, a lane per step; no float
 * atomics.  There is no backward entry point: Hm is frozen and sign has no gradient, so the gradient of sel is the sparse
 * row gradient over sel_ids.
 * Supported: m <= REC_ETA_MAX_M, K <= REC_SEARCH_MAX_K, D <= REC_SEARCH_MAX_D, V and B < 2^31,
 * 4 (D MC + T + REC_SEARCH_MAX_K) <= REC_SEARCH_LDS_CAP bytes of LDS with MC = 16 for m <= 16 and 32 beyond
 * (rec_eta_search_lds_bytes: that sum, 0: invalid or unsupported).
 * Return codes, in this order: a size below 1 (B below 0): -1; a shape outside the limits: -2, from the sizes alone;
 * ld < E, ld_q < D or K > T: -1; B == 0: 0, nothing is launched or written; a pointer that must not be NULL: -1. */
size_t rec_eta_search_lds_bytes(int T, int C, int E, int m, int K);
int rec_eta_search_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                           int T, const float* q, int64_t ld_q, const float* Hm, int m, int64_t padding_index, int K,
                           int* scores, int* chosen, float* sel, int* sel_valid, int64_t* sel_ids, int* oob_flag,
                           void* stream);

/* ---- SDIM (SDIMLayer.generate_longterm_interest, once=True, 8.DMR/CustomLayers.py:816-841; csrc/sdim.hip): the
 * hash-bucket interest of the long behaviour series.  D = E C.  key k_l = concat_c embed[series[b,l,c]], pad[b,l] =
 * series[b,l,0] == padding_index (the first column alone).  q [B,S,D] with row stride ld_q holds the S candidates' rows,
 * Hm [D,G,m] row-major (rec_eta_search's [D, G m]) the frozen projection.  Bit j of a row x's code is
 * sum_d x_d Hm[d,j] > 0 (tf.where(sign == 1, 1, 0): a zero and a NaN projection give 0), the projection computed as
 * rec_eta_search computes it -- d in order, the product rounded before the sum, dependent on the values of the row and of
 * Hm only -- so equal ids give equal codes bit for bit; group g's code is bits [g m, (g+1) m).  An id outside [0, V)
 * reads a zero row and sets *oob_flag (may be NULL).
 *   match[s,l,g] = code_g(k_l) == code_g(q[b,s,:])
 *   mode REC_SDIM_MODE_REFERENCE (the text as written: it keeps the PADDED rows and counts every step)
 *                                                                                              w_l = pad[b,l], n_l = 1
 *   mode REC_SDIM_MODE_VALID (the paper's intent)                                              w_l = n_l = !pad[b,l]
 *   Sum[s,g,d] = sum_{l: match} float(w_l) k_l[d], in increasing l from 0, every product and sum rounded to fp32
 *   cnt[s,g]   = sum_{l: match} n_l
 *   mean[s,g,d] = Sum / float(cnt), 0 where that is not finite (an empty bucket, a non-finite sum)
 *   out[b,s,d]  = (mean[s,0,d] + mean[s,1,d] + .. in increasing g) / float(G)
 * The forward writes out [B,S,D] and what makes the backward table-free: codes int32 [B,T] (the steps' packed codes),
 * qcodes int32 [B,S] and cnt int32 [B,S,G].  The backward takes gout [B,S,D] with row stride ld_gout and writes, never
 * adds to, gkeys [B,T,D] -- the IndexedSlices values of the one series lookup, as rec_sim_search_bwd_f32 does:
 *   gkeys[b,l,d] = sum over s, then over g, from 0, of match[s,l,g] ((gout[b,s,d] / float(G)) / float(cnt[s,g]))
 * for a step with w_l = 1 (cnt >= 1 wherever such a step matches) and +0 for a step with w_l = 0.  q and Hm receive no
 * gradient (sign and one_hot carry none); the backward reads neither embed nor Hm.  For an element whose bucket sum was
 * not finite the reference's gradient is zero; this ABI leaves that element's gradient UNDEFINED.  One launch each way,
 * one workgroup per example, no float atomics: bit-identical run to run.
 * Supported: G m <= REC_SDIM_MAX_BITS, S <= REC_SDIM_MAX_S, D <= REC_SEARCH_MAX_D, V and B < 2^31,
 * 4 (D MC + T + 2 ceil(T / 64) + REC_SDIM_MAX_S + 2 (T + T mod 2)) <= REC_SEARCH_LDS_CAP bytes of LDS with MC = 16 for
 * G m <= 16 and 32 beyond (rec_sdim_lds_bytes: the forward's sum, 0: invalid or unsupported; the backward needs less).
 * T >= 65536 is refused as well (16-bit list entries); the LDS rule is the stricter one, which csrc/sdim.hip asserts.
 * Return codes, in this order: a size below 1 (B below 0): -1; a shape outside the limits: -2, from the sizes alone;
 * ld < E, ld_q < D, ld_gout < D or a mode that is neither of the two: -1; B == 0: 0, nothing is launched or written; a
 * pointer that must not be NULL: -1. */
size_t rec_sdim_lds_bytes(int T, int C, int E, int G, int m, int S);
int rec_sdim_interest_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                              int T, const float* q, int64_t ld_q, int S, const float* Hm, int G, int m,
                              int64_t padding_index, int mode, float* out, int* codes, int* qcodes, int* cnt,
                              int* oob_flag, void* stream);
int rec_sdim_interest_bwd_f32(const int64_t* series, int E, int C, int64_t B, int T, int G, int m, int S,
                              int64_t padding_index, int mode, const int* codes, const int* qcodes, const int* cnt,
                              const float* gout, int64_t ld_gout, float* gkeys, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355REC_H */
