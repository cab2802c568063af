/*
 * recman_hip_multitask.h - C ABI of librecman_hip.so, continued: multi-task learning beyond MMoE (csrc/multitask.hip).
 * The conventions of recman_hip.h hold: device pointers, kernels enqueued on `stream`, RM_OK or a negative RM_E* code
 * with rm_last_error() for the message.  Nothing in the reference implements any of it: it knows one label per
 * example.
 *
 * ------------------------------------------------------------------------
 * The grouped gate mixture of one extraction level of PLE / CGC (Progressive Layered Extraction and its one-level
 * form Customized Gate Control, Tang et al., RecSys 2020).  Per example:
 *     T tasks, S task-specific experts per task, C shared experts, N = T S + C experts of width H;
 *     task gate t sees its own S experts and the C shared ones (width W = S + C); with shared_gate = 1 (every level
 *     but the last) one more gate, g = T, sees all N experts.  G = T + shared_gate gates.
 *     p_g = softmax over gate g's logits, max-subtracted;   M_g = sum_{e in gate g} p_ge Z_e
 *   Z [B, ldz]  N H columns used: expert j of task t at column (t S + j) H, shared expert j at (T S + j) H
 *   A [B, lda]  the gate logits, T W + shared_gate N columns: task gate t at columns t W .., its own experts
 *               j = 0..S-1 first, then the C shared ones; the shared gate's N logits from column T W on, in Z's
 *               expert order
 *   M [B, ldm]  G H columns written, gate g at g H (the shared gate is g = T)
 *   P [B, ldp]  or NULL: the gate weights in A's layout, for inspection (M has the same bits either way)
 *   Every operand is a pointer and a row stride in floats: a column range of a wider buffer works; pointers 16-byte
 *   aligned, strides multiples of 4 floats and >= the width; columns outside the range are never read or written.
 * rm_cgc_mix_fwd reads Z and A once and writes M once; p lives in LDS and reaches HBM only through P.
 * rm_cgc_mix_bwd, given dM [B, lddm] = dLoss/dM (G H columns), recomputes p and writes dZ [B, lddz] (all N H columns,
 *   once: every expert is in at least one gate) and dA [B, ldda] (A's layout):
 *     dZ_e = sum_{g with e} p_ge dM_g;   c_ge = <dM_g, Z_e>;   dA_g = p_g o (c_g - <p_g, c_g>)
 *   (exactly 0 for a gate of width 1).  No parameters, so no partial sums; no atomics, no workspace: two runs are
 *   bit-equal.
 * Supported (rm_cgc_mix_supported): 1 <= T <= 8, 1 <= S <= 4, 1 <= C <= 8, N = T S + C <= 32, H a multiple of 4 in
 *   4..512, shared_gate 0 or 1; anything else, a NULL or unaligned pointer, or a stride that is below its width or no
 *   multiple of 4 is RM_EINVAL before any launch, the limits named in the message.  B = 0 is RM_OK.
 * rm_cgc_mix_tile: RM_CGC_TILE the examples a block owns per tile (backward != 0: of rm_cgc_mix_bwd), RM_CGC_CAP the
 *   cap of both grids: a block walks the batch again from B > cap * tile on.  -1 when unsupported.
 *
 * ------------------------------------------------------------------------
 * The entire-space loss head of ESMM (Entire Space Multi-task Model, Ma et al., SIGIR 2018): rm_multitask_loss
 * (recman_hip.h: its arguments, layouts and reductions) with two classification tasks coupled, es_ctr = c and
 * es_cvr = v, c != v.  es_ctr = es_cvr = -1 gives rm_multitask_loss's results, bit for bit.  Every task other than v
 * behaves as in rm_multitask_loss.  Task v is trained through the product pCTCVR = pCTR pCVR over all impressions:
 *     y_c = Y[i, c], y_v = Y[i, v], p = sigmoid(logit)
 *     z_i = 0    if y_c == 0 (whatever y_v is, NaN included)
 *         = y_v  if y_c == 1 and y_v is observed;   unobserved otherwise (y_c NaN, or y_c == 1 with y_v NaN)
 *     q_i = p_c p_v;   l_v,i = Keras binary_crossentropy(z_i, q_i) (the clip and epsilon of every loss head here)
 *     n_v = #observed z;   loss_v = the mean of l_v over them;   loss = sum_t w_t loss_t
 *     dlogit_v,i = w_v / n_v grad_scale dl/dq q (1 - p_v)
 *     dlogit_c,i = task c's own term + w_v / n_v grad_scale dl/dq q (1 - p_c)
 *   The coupled terms are exactly +0.0 where z is unobserved and where q lies in the clip region (q < 1e-7 or
 *   1 - q < 1e-7).  pred[v] stays p_v (pCVR), written for every row.  1 - p is formed as sigmoid(-logit) and 1 - q as
 *   sigmoid(-a) + sigmoid(a) sigmoid(-b), so neither cancels.  Counts and sums are fixed-order two-stage reductions in
 *   double: two runs are bit-equal.  workspace: rm_multitask_loss_es_workspace(B, T) floats, 16-byte aligned (-1:
 *   unsupported T).  An es pair that is not (-1, -1) or two distinct classification tasks below T is RM_EINVAL.
 */
#ifndef RECMAN_HIP_MULTITASK_H
#define RECMAN_HIP_MULTITASK_H

#include "recman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RM_CGC_TILE 0
#define RM_CGC_CAP 1
int rm_cgc_mix_supported(int T, int S, int C, int H, int shared_gate);
int rm_cgc_mix_tile(int T, int S, int C, int H, int shared_gate, int backward, int which);
int rm_cgc_mix_fwd(const float *Z, int64_t ldz, const float *A, int64_t lda, int64_t B, int T, int S, int C, int H,
                   int shared_gate, float *M, int64_t ldm, float *P, int64_t ldp, rm_stream_t stream);
int rm_cgc_mix_bwd(const float *Z, int64_t ldz, const float *A, int64_t lda, const float *dM, int64_t lddm, int64_t B,
                   int T, int S, int C, int H, int shared_gate, float *dZ, int64_t lddz, float *dA, int64_t ldda,
                   rm_stream_t stream);
int64_t rm_multitask_loss_es_workspace(int64_t B, int T);
int rm_multitask_loss_es(const float *logit, const float *Y, const int *task_type, const float *task_weight,
                         float grad_scale, int64_t B, int T, int es_ctr, int es_cvr, float *pred, float *dlogit,
                         int64_t *n_t, float *loss_t, float *loss, float *workspace, rm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECMAN_HIP_MULTITASK_H */
