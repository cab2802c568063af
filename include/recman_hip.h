/*
 * recman_hip.h - C ABI of librecman_hip.so: the MI355X (gfx950) kernels behind
 * recman's CTR forward+backward path (DeepFM / DCN / xDeepFM).
 *
 * The reference (dev-wei/recman) has no native code, no operator registry and no
 * FFI: its seam is the Python layer-callable protocol `Layer(variables, ...)(x)`
 * of recman/tf/core/layers.py, composed by xDeepFM._out (recman/tf/core/xDeepFM.py:47-104),
 * DeepFM._init_graph (DeepFM.py:107-163) and DCN._init_graph (DCN.py:99-149).
 * Each entry point below cites the span of that Python it replaces.  The Python
 * host side that binds these (ctypes) is recman_amd/_lib.py; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless named host_*; the caller owns all
 *    buffers, the library allocates nothing and keeps no global mutable state;
 *  - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream) and return immediately: asynchronous, graph-capturable;
 *  - return value: RM_OK (0) or a negative RM_E* code; rm_last_error() gives a
 *    thread-local message for the last failing call.  No exceptions cross the ABI;
 *  - floats are IEEE fp32, indices are int64 (recman/tf/inputs.py:158,199);
 *  - layouts are row-major; E is [B, F, D] exactly as tf.concat(axis=1) of the
 *    per-field [B,1,D] lookups produces it (layers.py:248-253).
 */
#ifndef RECMAN_HIP_H
#define RECMAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_OK 0
#define RM_EINVAL (-1)  /* bad argument (null pointer, size, alignment)      */
#define RM_ELAUNCH (-2) /* hipLaunch / runtime error, see rm_last_error()    */
#define RM_EUNSUPPORTED (-3)

/* activation ids (layers.py:601,738; tf.nn.leaky_relu alpha = 0.2) */
#define RM_ACT_IDENTITY 0
#define RM_ACT_RELU 1
#define RM_ACT_LEAKY_RELU 2

typedef void *rm_stream_t;

int rm_version(void);
const char *rm_last_error(void);
/* number of compute units of the current device (grid sizing for callers) */
int rm_device_cus(void);
/* Enqueues an empty one-wave kernel named rm_profile_marker_kernel: brackets a stretch of launches so
 * that a rocprofv3 kernel / counter trace can be cut at it (bench.py's PMC child passes).  No memory
 * is touched.  (New: the reference has no profiler hooks beyond tf.summary.trace_on,
 * recman/tf/core/TensorBoardLogger.py:58-69.) */
int rm_profile_marker(int tag, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Embedding gather (+ FM, + sparse/dense linear term), forward.
 * Replaces: FeatEmbedding.__call__ SparseFeat branch + FeatEmbeddingLayer.__call__
 *   (layers.py:117-128, 238-261), FMLayer.__call__ (layers.py:457-478) and
 *   LinearCombiner/LinearLayer resp. SparseLinearCombiner/SparseLinearLayer
 *   (layers.py:281-347, 368-439; one_hot utils.py:51-67) in gather form.
 *
 *   idx        [B,F]  per-field row index (0 = null/unknown, inputs.py:166)
 *   table      [R,D]  all field tables concatenated, row r at table + r*table_ld
 *                     (table_ld >= D floats); field f owns rows
 *                     field_off[f] .. field_off[f]+V_f-1
 *   bias_table [R]    first-order FM bias tables, same row numbering, element r at
 *                     bias_table + r*bias_ld, or NULL
 *   lin_w             sparse part of linear_w (one one-hot block per feature), or
 *                     NULL; element (f, i) at lin_w + (lin_off[f]+i)*lin_ld.
 *                     (the *_ld strides let bias and linear weight live inside the
 *                     embedding row - one HBM sector per lookup instead of three)
 *   lin_w_dense [Dn]  linear weights of the dense columns, lin_w0 [1] the bias
 *   dense      [B,Dn] scaled dense features or NULL (Dn = 0)
 *   mask_b [B,F], mask_e [B,F,D]: FMLayer dropout multipliers (0 or 1/keep,
 *                     layers.py:461,466) or NULL = keep-probability 1
 * outputs (each may be NULL = not wanted):
 *   E        [B,F,D]  gathered rows (the un-dropped embeddings the DNN/CIN/cross use)
 *   fm_sum   [B,D]    S = sum_f mask_e*E  (saved for the backward)
 *   fm_logit [B]      sum_f mask_b*bias + 0.5*sum_k(S_k^2 - sum_f (mask_e*E)_fk^2)
 *   lin_logit[B]      sum_f lin_w[lin_off[f]+idx] + dense . lin_w[dense block] + lin_w0
 * D must be one of 4, 8, 16, 32, 64, 128, 256 (D/4 lanes own an example and must divide the 64-lane wave; anything
 * else is RM_EINVAL); table_ld a multiple of 4; table/E/fm_sum/mask_e 16-byte aligned.
 */
/* flags: RM_EMBED_STREAM_ROWS = load the table rows non-temporally (fused-row layout only).  For ids that
 * touch a row about once per batch (uniformly hashed ids over a table far larger than the caches) the
 * row lines then do not evict E from L2 / the Infinity Cache, which the next kernels read; ids with
 * heavy reuse (Zipf) want the plain, cached loads. */
enum { RM_EMBED_STREAM_ROWS = 1 };
int rm_embed_fwd(const int64_t *idx, const float *table, int64_t table_ld,
                 const int64_t *field_off, const float *bias_table, int64_t bias_ld,
                 const float *lin_w, int64_t lin_ld, const int64_t *lin_off,
                 const float *lin_w_dense, const float *lin_w0, const float *dense, int Dn,
                 const float *mask_b, const float *mask_e, int64_t B, int F, int D,
                 float *E, float *fm_sum, float *fm_logit, float *lin_logit,
                 int flags /* RM_EMBED_* */, rm_stream_t stream);

/* The linear term on its own: (Sparse)LinearCombiner + (Sparse)LinearLayer.__call__ (layers.py:281-347,
 * 368-439; one_hot utils.py:51-67) in gather form, for callers that compose the reference's layer
 * callables one by one (recman_amd/th/layers.py; the engines take it from rm_embed_fwd):
 *   out[b] = sum_f w[lin_off[f] + idx[b,f]] + sum_j dense[b,j] * w_dense[j] + w0[0]
 * w0 may be NULL.  Its backward is rm_scatter_add_rows (g_row form) + rm_linear_dense_bwd. */
int rm_linear_fwd(const int64_t *idx, const int64_t *lin_off, const float *w, const float *dense,
                  const float *w_dense, const float *w0, int64_t B, int F, int Dn, float *out,
                  rm_stream_t stream);

/* Backward of the embedding + FM block w.r.t. the gathered rows: the IndexedSlices
 * values TF's autodiff produces for tf.nn.embedding_lookup (one row per (b,f)
 * occurrence, duplicates NOT merged; the indices are `idx` itself).
 *   d_rows[b,f,:] = dE_up[b,f,:] + g_fm[b] * mask_e[b,f,:] * (S[b,:] - mask_e*E[b,f,:])
 *   d_bias[b,f]   = g_fm[b] * mask_b[b,f]
 * dE_up (upstream gradient from DNN / CIN / cross w.r.t. E) may be NULL; g_fm may
 * be NULL (no FM term: d_rows = dE_up, and d_bias is then NOT written - it keeps its prior content).  d_rows may
 * alias dE_up.  d_bias may be NULL.  D is any multiple of 4 (the pass is elementwise over float4 slices).
 */
int rm_embed_bwd(const float *E, const float *fm_sum, const float *dE_up, const float *g_fm,
                 const float *mask_b, const float *mask_e, int64_t B, int F, int D,
                 float *d_rows, float *d_bias, rm_stream_t stream);

/* Scatter-add of occurrence rows into a dense table gradient (what TF's
 * IndexedSlices densify to once the l2 term touches every row, layers.py:188-193):
 *   d_table[(field_off[f]+idx[b,f])*ld + k] += rows[b,f,k], k < width   (float atomics)
 * `width` = D for embedding tables, 1 for bias tables / linear weights (then
 * field_off = lin_off).  When g_row != NULL, rows is ignored and the added value
 * is g_row[b] (width must be 1): the D=1 linear / bias gradient. */
int rm_scatter_add_rows(const int64_t *idx, const int64_t *field_off, const float *rows,
                        const float *g_row, int64_t B, int F, int width, int64_t ld,
                        float *d_table, rm_stream_t stream);

/* Weighted column sums: d_w_dense[j] = sum_b g[b]*dense[b,j] (j < Dn <= 1023),
 * d_w0 = sum_b g[b].  The dense part of the linear-layer backward, and the gradient of
 * every [*,1] output projection (d cin_w = pooled^T g, d dnn_w = a^T g).  Deterministic
 * two-stage reduction; workspace >= 262144 floats; either output may be NULL. */
int rm_linear_dense_bwd(const float *g, const float *dense, int64_t B, int Dn,
                        float *d_w_dense, float *d_w0, float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * PredictionLayer + create_loss, forward and backward in one pass.
 * Replaces: tf.add_n of the branch logits (xDeepFM.py:99-102, DeepFM.py:149-158,
 *   DCN.py:140-144), PredictionLayer.__call__ (layers.py:796-808), create_loss
 *   (utils.py:192-198: Keras binary_crossentropy on probabilities, clip 1e-7) and
 *   their gradient.
 *   logit_a..d [B]  branch logits (NULL = absent); coef_* multiply them (DCN's
 *                   double-counted dnn logit uses coef 2 under strict_reference)
 *   y   [B] int64 labels (classification) or NULL with y_f [B] float (regression)
 *   task 0 = classification (sigmoid + BCE), 1 = regression (MSE)
 * outputs: logit [B] (sum), pred [B], dlogit [B] = d(mean loss)/d(logit) (NULL ok),
 *   loss [1] (NULL ok; needs workspace >= 1024 floats).
 */
int rm_logit_loss(const float *logit_a, float coef_a, const float *logit_b, float coef_b,
                  const float *logit_c, float coef_c, const float *logit_d, float coef_d,
                  const int64_t *y, const float *y_f, int task, int64_t B, float *logit,
                  float *pred, float *dlogit, float *loss, float *workspace,
                  rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Skinny DNN (every hidden width <= 32, 1..3 hidden layers, FD+Dn <= 448), fused on the
 * f32 MFMA.  Replaces DNNCombiner + DNN.__call__ (layers.py:494-501, 576-609) and their
 * gradient for the reference-default deep_hidden_units (32, 32) (DeepFM.py:37,
 * hparams/xDeepFM.py:27); wider MLPs (DCN's [400,400]) go to rocBLAS/hipBLASLt.
 *   x = [xe | xd] (never concatenated); W[0] [FD+Dn, H0], W[l] [H_{l-1}, H_l], bias[l] [H_l];
 *   w_out [H_last], w0_out [1];  host arrays H / W / bias / h_out / dh / dW have NL entries.
 * rm_mlp_fwd: h_out[l] [B,32] (post-activation, columns >= H_l zero), logit [B].
 * rm_mlp_bwd: g [B] = dLoss/dlogit; writes dLoss/dxe into d_rows [B,FD]; when fm_sum
 *   (S [B,D] from rm_embed_fwd) is given the FM second-order gradient g*(S - E) is added
 *   (xe is E: the whole DeepFM row gradient in one pass, no rm_embed_bwd launch);
 *   dh[l] [B,32] = dLoss/d(pre-activation of layer l); dW[l] / db[l] = weight / bias
 *   gradients, d_w_out [H_last], d_w0_out [1] = gradients of the output projection
 *   (db, d_w_out, d_w0_out may be NULL); d_xd_wsum [Dn] (NULL or Dn <= 32) = sum_b g[b] * xd[b,:],
 *   and d_g_sum [1] (NULL ok) = sum_b g[b]: the gradients of the linear term's dense weights and
 *   bias when the same g drives it (layers.py:330-347; saves the rm_linear_dense_bwd pass).
 *   Deterministic (no float atomics).
 *   workspace: rm_mlp_bwd_workspace(FD, Dn) floats.
 *   flags: RM_MLP_STREAM_DROWS = store d_rows non-temporally - only when NOTHING re-reads it soon (a
 *   bare fwd+bwd); in training the optimizer step gathers it right after: leave it 0.
 *
 * Fused training head (rm_mlp_tail, optional - NULL gives the plain calls above).  When the DNN is
 *   the LAST branch of the model's forward (DeepFM, xDeepFM), everything between its output and its
 *   backward is elementwise per example: final logit = coef_mlp * dnn + coef_a * logit_a + coef_b *
 *   logit_b (xDeepFM.py:99-102), PredictionLayer + loss (layers.py:796-808, utils.py:192-198, the
 *   arithmetic of rm_logit_loss) and the dh chain of the hidden layers.  rm_mlp_fwd with a tail does
 *   all of it in the forward kernel's epilogue, where h_l are still in registers: it writes logit /
 *   pred / dlogit (= dLoss/dlogit * grad_scale, the `g` of the backward), the per-tile loss sums
 *   loss_partial [ceil(B/32)] and dh[l] [B,32].  rm_mlp_bwd with the SAME tail skips its own dh-chain
 *   launch (g = tail->dlogit) and its finishing kernel also reduces loss_partial into loss [1]
 *   (mean over B; no l2 terms).  Saves three launches per step (rm_logit_loss's two kernels and the
 *   chain kernel) - 20 of 237 us on the DeepFM benchmark step. */
typedef struct rm_mlp_tail {
  const float *logit_a; /* other branch logits [B], NULL = absent */
  float coef_a;
  const float *logit_b;
  float coef_b;
  float coef_mlp;       /* coefficient of this MLP's logit in the sum: MUST be 1 - the dh chain and rm_mlp_bwd's
                           d_w_out / d_w0_out take dlogit as dLoss/d(this MLP's logit); anything else is refused
                           (scale the MLP's branch with rm_logit_loss and the plain calls instead) */
  const int64_t *y;     /* labels: int64 (classification) ... */
  const float *y_f;     /* ... or float (regression); exactly one of them */
  int task;             /* 0 = classification (sigmoid + binary cross-entropy), 1 = regression (MSE) */
  float grad_scale;     /* dlogit is multiplied by this (micro-batches / ranks); 1 = plain mean over B */
  float *logit, *pred, *dlogit; /* [B] outputs (logit / pred may be NULL) */
  float *loss_partial;  /* [ceil(B/32)] workspace: per-tile loss sums */
  float *loss;          /* [1], written by rm_mlp_bwd's finishing kernel; NULL = not wanted */
  float *dh[3];         /* dh[l] [B,32] for l < NL (the same buffers rm_mlp_bwd gets as dh) */
} rm_mlp_tail;

#define RM_MLP_STREAM_DROWS 1
int rm_mlp_supported(int FD, int Dn, int NL, const int *H);
int rm_mlp_fwd(const float *xe, const float *xd, int FD, int Dn, int NL, const int *H,
               const float *const *W, const float *const *bias, const float *w_out,
               const float *w0_out, int act, int64_t B, float *const *h_out, float *logit,
               const rm_mlp_tail *tail, rm_stream_t stream);
/* Gather + FM + linear term + skinny MLP (+ training head) in ONE kernel: rm_embed_fwd followed by rm_mlp_fwd
 * on E without the round trip of x through HBM (FeatEmbeddingLayer + FMLayer + LinearLayer + DNNCombiner + DNN of
 * DeepFM._init_graph, recman/tf/core/DeepFM.py:96-150 over layers.py:238-261,457-478,330-347,494-501,576-609).
 * Fused-row layout only: table rows [16 embedding | bias | linear weight | ...] with table_ld = 32 (or 20: the
 * rows a row-sharded table exchanges, idx = positions in the received buffer, field_off = 0), D = 16;
 * Dn <= 16, 16 F + Dn <= 448, hidden widths <= 32 (rm_embed_mlp_fwd_supported).  want_bias / want_lin: the FM
 * bias sum / the sparse part of the linear term are wanted; lin_w_dense [Dn] (NULL: the linear term has no
 * dense part), lin_w0 [1] or NULL; xd [B,Dn] feeds the MLP (and the linear term).  Outputs as the two calls':
 * E [B,F,16] (always written: the backward reads it), fm_sum [B,16], fm_logit [B], lin_logit [B] (NULL = not
 * wanted), h_out / logit / tail as rm_mlp_fwd - tail->logit_a / logit_b must be this call's lin_logit /
 * fm_logit buffers (or NULL).  flags: RM_EMBED_STREAM_ROWS.  No dropout masks (the callers fall back to the
 * two separate entry points). */
int rm_embed_mlp_fwd_supported(int F, int D, int64_t table_ld, int Dn, int NL, const int *H);
int rm_embed_mlp_fwd(const int64_t *idx, const float *table, int64_t table_ld, const int64_t *field_off,
                     int want_bias, int want_lin, const float *lin_w_dense, const float *lin_w0,
                     const float *xd, int Dn, int64_t B, int F, int D, float *E, float *fm_sum,
                     float *fm_logit, float *lin_logit, int flags, int NL, const int *H,
                     const float *const *W, const float *const *bias, const float *w_out,
                     const float *w0_out, int act, float *const *h_out, float *logit,
                     const rm_mlp_tail *tail, rm_stream_t stream);
int64_t rm_mlp_bwd_workspace(int FD, int Dn);
int rm_mlp_bwd(const float *xe, const float *xd, int FD, int Dn, int NL, const int *H,
               const float *const *W, const float *w_out, int act, int64_t B, const float *g,
               const float *const *h, const float *fm_sum, int D, float *d_rows,
               float *const *dh, float *const *dW, float *const *db, float *d_w_out,
               float *d_w0_out, float *d_xd_wsum, float *d_g_sum, float *workspace,
               const rm_mlp_tail *tail, int flags, rm_stream_t stream);

/* DeepFM's WHOLE training step in one kernel + one finishing launch: DeepFM._init_graph forward and the gradient
 * of every variable (recman/tf/core/DeepFM.py:107-180; FeatEmbeddingLayer layers.py:238-261, LinearLayer :330-347,
 * FMLayer :457-478, DNN :576-609, PredictionLayer :796-808, create_loss utils.py:192-198) - what rm_embed_mlp_fwd
 * followed by rm_mlp_bwd compute, without E, S, h_l or dh_l ever reaching HBM (every DeepFM gradient except the
 * parameter reductions is local to the example).  Shapes: fused-row table [R, table_ld] (rows [16 embedding | bias
 * entry | linear weight | ...], table_ld a multiple of 4, >= 20, < 2^30), D = 16, F <= 26, Dn <= 16, NL = 2 hidden layers
 * of width <= 32 (rm_deepfm_step_supported); FM, bias tables, linear term and DNN all on, no dropout masks - the
 * callers use the separate entry points for anything else.
 * In: idx [B,F] int64, field_off [F], dense [B,Dn] (NULL when Dn = 0), labels y (int64) or y_f (float),
 *   W[l] / bias[l] (l < 2), w_out [H1], w0_out [1], lin_w_dense [Dn], lin_w0 [1], act, task (0 classification,
 *   1 regression), grad_scale (dlogit multiplier: micro-batches / ranks; 1 = plain mean over B).
 * Out: d_rows [B,F,16] = dLoss/dE (IndexedSlices form, duplicates not merged), logit / pred / dlogit [B] (dlogit =
 *   dLoss/dlogit: the per-occurrence gradient of the bias-table and sparse linear entries), loss [1] (mean over B,
 *   no l2 terms), dW[l] / db[l] (db may be NULL), d_w_out [H1], d_w0_out [1], d_lin_w_dense [Dn], d_lin_w0 [1].
 * packed_rows > 0 (row-sharded table, recman_amd/dist.py): `table` is the buffer of RECEIVED rows [packed_rows,
 *   20] ([16 embedding | bias | linear | 0 0], table_ld = 20), idx [B,F] = the position of every occurrence in it
 *   (field_off zeros), and d_rows is the send buffer of the backward exchange, [packed_rows, 20]: occurrence (b, f)
 *   writes [dE | dlogit | dlogit * lin_field_mask[f] | 0 0] to row idx[b, f] - what rm_pack_grad_rows builds from
 *   the plain layout (lin_field_mask [F] or NULL: the linear_features subset).  packed_rows = 0: the plain layout.
 * workspace: rm_deepfm_step_workspace(F, Dn) floats.  flags: bit 0 = non-temporal row loads
 *   (RM_EMBED_STREAM_ROWS), bit 1 = non-temporal d_rows stores (only when nothing re-reads them soon), bit 2 = skip
 *   the finishing launch (measurement only: the parameter gradients and the loss are then NOT written).
 * Deterministic (fixed summation orders, no float atomics). */
int rm_deepfm_step_supported(int F, int D, int64_t table_ld, int Dn, int NL, const int *H);
int64_t rm_deepfm_step_workspace(int F, int Dn);
int rm_deepfm_step(const int64_t *idx, const float *table, int64_t table_ld, const int64_t *field_off,
                   const float *dense, int Dn, const int64_t *y, const float *y_f, int64_t B, int F, int D,
                   int NL, const int *H, const float *const *W, const float *const *bias, const float *w_out,
                   const float *w0_out, const float *lin_w_dense, const float *lin_w0, int act, int task,
                   float grad_scale, float *d_rows, float *logit, float *pred, float *dlogit, float *loss,
                   float *const *dW, float *const *db, float *d_w_out, float *d_w0_out, float *d_lin_w_dense,
                   float *d_lin_w0, float *workspace, int64_t packed_rows, const float *lin_field_mask, int flags,
                   rm_stream_t stream);
/* Test aids, not product paths.  rm_debug_lds_fill fills the LDS of every CU with one 32-bit pattern: workgroups of
 * 512 threads that allocate a CU's whole LDS (163,840 bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, so one fits a
 * CU), four times the CU count of them, every word written with ds_write - what the kernel behind it on the stream
 * finds in LDS before it has written it is then known (tests/stale_state.py, tests/test_gpu_stale_lds.py,
 * tests/test_gpu_step_stale_lds.py).  rm_debug_lds_probe is the fill's own check: nblocks workgroups that allocate the
 * whole LDS, write none of it and count the words that differ from pattern; mismatches [nblocks] (device) gets one
 * count per block. */
int rm_debug_lds_fill(unsigned pattern, rm_stream_t stream);
int rm_debug_lds_probe(unsigned pattern, unsigned *mismatches, int nblocks, rm_stream_t stream);

/* Epilogues of the library-GEMM DNN path (wide hidden layers, layers.py:593-601):
 * rm_bias_act: x[b,j] = act(x[b,j] + bias[j]) in place (bias may be NULL = a bias of +0.0: the add is still made,
 *              so x = -0.0 becomes +0.0);
 * rm_act_bwd:  da[b,j] *= act'(a[b,j]) in place, act' read off the post-activation a. */
int rm_bias_act(float *x, const float *bias, int64_t B, int N, int act, rm_stream_t stream);
int rm_act_bwd(float *da, const float *a, int64_t B, int N, int act, rm_stream_t stream);
/* da[b,j] = g[b] * w[j] * act'(a[b,j]) (a = post-activation of the last hidden layer, or NULL for no
 * activation factor): the backward of the [H,1] output projection (layers.py:606-609) and of the last
 * activation in one pass.  N % 4 == 0. */
int rm_outer_actgrad(const float *g, const float *w, const float *a, int64_t B, int N, int act,
                     float *da, rm_stream_t stream);
/* The same pass also reduces the columns of the two arrays it touches: d_w[j] = sum_b g[b] a[b,j]
 * (gradient of dnn_w), d_w0 = sum_b g[b] (dnn_w0), db[j] = sum_b da[b,j] (bias of the last hidden
 * layer) - three reads of a [B,N] array less.  a is required; d_w / d_w0 / db may be NULL;
 * workspace: rm_outer_actgrad_sums_workspace(B, N) floats.  Deterministic. */
int64_t rm_outer_actgrad_sums_workspace(int64_t B, int N);
int rm_outer_actgrad_sums(const float *g, const float *w, const float *a, int64_t B, int N, int act,
                          float *da, float *d_w, float *d_w0, float *db, float *workspace,
                          rm_stream_t stream);

/* out[b] = sum_j X[b,j]*w[j] + w0[0]: the [*,1] output projections (dnn_w/dnn_w0,
 * layers.py:606-609; cin_w/cin_w0, layers.py:757-760).  w0 may be NULL. */
int rm_rowdot(const float *X, const float *w, const float *w0, int64_t B, int P, float *out,
              rm_stream_t stream);

/* ------------------------------------------------------------------------
 * CrossNet (DCN v1, vector form), all L layers fused.
 * Replaces: CrossNet(layer_num, l2_reg)(dnn_input) -> logit [B,1] used at
 *   DCN.py:134-137 - the class itself is ABSENT from the reference
 *   (DCN.py:7 comments the import out); arithmetic per arXiv 1708.05123 eq. (3):
 *   x_{l+1} = x0 * (x_l . w_l) + b_l + x_l,  logit = x_L . w_out
 * x0 = [xe | xd]: xe [B,FD] is the flattened embedding block E, xd [B,Dn] the dense
 * columns (DNNCombiner, layers.py:494-501) - never concatenated in memory.
 *   w, b [L,d], w_out [d], d = FD + Dn, FD % 4 == 0, 0 < FD <= 512, L <= 8.
 * Computed in closed form (exact algebra): x_l = c_l x0 + Bp_l with Bp_l = sum_{j<l} b_j, so
 *   s_l = x_l.w_l = c_l p_l + beta_l,  p_l = x0.w_l,  beta_l = Bp_l.w_l,  c_{l+1} = c_l + s_l,
 *   logit = c_L p_out + beta_out  (p_out = x0.w_out): L+1 dot products per row + a scalar recurrence.
 *   p_out [B, p_ld] (p_ld >= L+1; NULL ok): the row's dot products (p_0..p_{L-1}, x0.w_out), saved
 *   for the backward, which needs nothing else of x0.
 */
int rm_cross_fwd(const float *xe, const float *xd, int FD, int Dn, const float *w,
                 const float *b, const float *w_out, int L, int64_t B, float *logit,
                 float *p_out, int p_ld, rm_stream_t stream);

/* Backward: given g [B] = dLoss/dlogit and p [B, p_ld] from the forward,
 *   d_xe [B,FD] (+ dx_in_e when given): gradient w.r.t. the embedding block of x0
 *       = g c_L w_out + sum_l t_l c_l w_l, optionally summed with another branch's gradient
 *       (t_l = g p_out + sum_{j>l} t_j p_j).  x0 itself is not read; the dense columns are input
 *       data and get no gradient (the reference differentiates variables only, xDeepFM.py:126).
 *   coef [B, 2L+2]: per-example scalars from which the parameter gradients follow
 *       by one skinny GEMM (see recman_amd/engine.py and DESIGN.md):
 *       columns 0..L-1 = t_l*c_l, L = g*c_L, L+1..2L = t_l, 2L+1 = g
 */
int rm_cross_bwd(int FD, int Dn, const float *w, const float *b, const float *w_out, int L,
                 int64_t B, const float *g, const float *p, int p_ld, const float *dx_in_e,
                 float *d_xe, float *coef, rm_stream_t stream);

/* Finishes the CrossNet parameter gradients from P = x0^T @ coef[:, :L+1] ([d, L+1],
 * row-major) and colsum = sum_b coef[:, L+1:] ([L+1]):
 *   d_w[l] = P[:,l] + T_l * Bp_l,  d_w_out = P[:,L] + G * Bp_L,
 *   d_b[l] = G * w_out + sum_{j>l} T_j * w_j,   Bp_l = sum_{j<l} b_j */
int rm_cross_param_grads(const float *P, const float *colsum, const float *w, const float *b,
                         const float *w_out, int L, int d, float *d_w, float *d_b,
                         float *d_w_out, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * AFM attention layer (Attentional Factorization Machines), forward and backward fused.
 * Replaces: AFMLayer(att_factor, att_dropout)(feat_embeds) -> logit [B,1] used at
 *   AFM.py:119-122 - the class itself is ABSENT from the reference (AFM.py:7 comments the
 *   import out); arithmetic per arXiv 1708.04617 eq. (4)-(6).  Per example, over the
 *   P = F(F-1)/2 field pairs i < j (row-major over the upper triangle):
 *     P_ij = E_i * E_j;  z_ij = W^T P_ij + b;  s_ij = h . relu(z_ij);  a = softmax_ij(s)
 *     v = sum_ij a_ij P_ij;  logit = p . (mask * v)
 *   E [B,F,D] (the gathered rows, rm_embed_fwd's E); W [D,T], b [T], h [T], p [D];
 *   mask [B,D] or NULL: the dropout multiplier (0 or 1/keep); logit [B].
 *   stats [B,D+2] or NULL (inference): per example the softmax's (max score, sum of exp(s - max))
 *   and u = mask * v [D] - all the backward keeps of the forward.  The softmax is max-subtracted;
 *   the logits are the same bits with and without stats.
 * Supported: D in {8,16,32,64}, 2 <= F <= 40, 1 <= T <= 64 (rm_afm_supported); anything else is
 *   RM_EINVAL.  The [P,D] pair products, the [P,T] hidden units and the scores never leave the chip.
 * rm_afm_bwd, given g [B] = dLoss/dlogit and the forward's logit and stats, recomputes the forward
 *   per pair and writes  d_rows [B,F,D] = dLoss/dE (+ dE_up [B,F,D] when not NULL; dE_up may BE
 *   d_rows),  dW [D,T], db [T], dh [T], dp [D] (overwritten, summed over the batch):
 *     c = g (mask * p);  ds_ij = a_ij (c . P_ij - g logit);  dz_ij = ds_ij h [z_ij > 0]
 *     dP_ij = a_ij c + W dz_ij;  dE_i += dP_ij E_j;  dE_j += dP_ij E_i
 *     dW = sum P_ij dz_ij^T;  db = sum dz_ij;  dh = sum ds_ij relu(z_ij);  dp = sum g u
 *   workspace: rm_afm_bwd_workspace(B, F, D, T) floats, 16-byte aligned.
 * Deterministic: per-block partial sums added in block order, fixed-order sums inside a block,
 *   no float atomics - two runs on the same inputs are bit-equal.
 */
int rm_afm_supported(int F, int D, int T);
int rm_afm_fwd(const float *E, const float *W, const float *b, const float *h, const float *p,
               const float *mask, int64_t B, int F, int D, int T, float *logit, float *stats,
               rm_stream_t stream);
int64_t rm_afm_bwd_workspace(int64_t B, int F, int D, int T);
int rm_afm_bwd(const float *E, const float *W, const float *b, const float *h, const float *p,
               const float *mask, const float *g, const float *logit, const float *stats,
               const float *dE_up, int64_t B, int F, int D, int T, float *d_rows, float *dW, float *db,
               float *dh, float *dp, float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * AutoInt interacting layer (multi-head self-attention over the fields, arXiv 1810.11921
 * eq. (5)-(8)) and the model's last projection.  Nothing in the reference implements it.
 * One layer maps X [B,F,Din] to Y [B,F,HD], HD = H dk; Wq, Wk, Wv, Wr [Din,HD]; Q, K, V are cut
 * into H column blocks of width dk:
 *     Q = X Wq;  K = X Wk;  V = X Wv;  s^h_mk = <Q^h_m, K^h_k> scale;  a^h_m. = softmax_k(s^h_m.)
 *     O_m = concat_h sum_k a^h_mk V^h_k;  Y_m = relu(O_m + X_m Wr)      (Wr NULL: relu(O_m))
 *   The softmax is max-subtracted and runs over all F fields (k = m included).
 *   stats [B,H,F,2] (rm_autoint_stats_floats(B, F, H) floats) or NULL (inference): per (example,
 *   head, field) the row maximum and the sum of exp(s - max) - all the backward keeps of the
 *   forward besides X and Y.  Y is the same bits with and without stats.  Q, K, V, the scores and
 *   the weights never leave the chip.
 * Supported (rm_autoint_supported): 1 <= F <= 40, Din in {8,16,32,64}, H in {1,2,4,8}, dk >= 4,
 *   H dk in {8,16,32,64}; anything else is RM_EINVAL ("unsupported") before any launch.
 * rm_autoint_layer_bwd, given dY [B,F,HD], recomputes Q, K, V and the weights and writes
 *   dX [B,F,Din] = dLoss/dX (+ dX_up when not NULL; dX_up may BE dX), dWq, dWk, dWv, dWr
 *   (overwritten, summed over the batch; dWr NULL exactly when Wr is):
 *     dP = dY [Y > 0];  da_mk = <dP^h_m, V^h_k>;  ds_mk = a_mk (da_mk - sum_k' a_mk' da_mk')
 *     dQ_m = scale sum_k ds_mk K_k;  dK_k = scale sum_m ds_mk Q_m;  dV_k = sum_m a_mk dP_m
 *     dW* = X^T d*;  dWr = X^T dP;  dX = dQ Wq^T + dK Wk^T + dV Wv^T + dP Wr^T
 *   workspace: rm_autoint_layer_bwd_workspace(B, F, Din, H, dk) floats, 16-byte aligned.
 * rm_autoint_head_fwd:  logit[b] = Y[b,:] . w + w0,  Y [B,K], w [K], w0 [1].
 * rm_autoint_head_bwd, given g [B]:  dY[b,:] = g[b] w,  dw = sum_b g[b] Y[b,:],  dw0 = sum_b g[b];
 *   workspace: rm_autoint_head_bwd_workspace(B, K) floats.
 * Deterministic: per-block partial sums added in block order, fixed-order sums inside a block,
 *   no float atomics - two runs on the same inputs are bit-equal.
 */
int rm_autoint_supported(int F, int Din, int H, int dk);
int64_t rm_autoint_stats_floats(int64_t B, int F, int H);
int rm_autoint_layer_fwd(const float *X, const float *Wq, const float *Wk, const float *Wv,
                         const float *Wr, int64_t B, int F, int Din, int H, int dk, float scale,
                         float *Y, float *stats, rm_stream_t stream);
int64_t rm_autoint_layer_bwd_workspace(int64_t B, int F, int Din, int H, int dk);
int rm_autoint_layer_bwd(const float *X, const float *Wq, const float *Wk, const float *Wv,
                         const float *Wr, const float *Y, const float *stats, const float *dY,
                         int64_t B, int F, int Din, int H, int dk, float scale, float *dX,
                         const float *dX_up, float *dWq, float *dWk, float *dWv, float *dWr,
                         float *workspace, rm_stream_t stream);
int rm_autoint_head_fwd(const float *Y, const float *w, const float *w0, int64_t B, int K,
                        float *logit, rm_stream_t stream);
int64_t rm_autoint_head_bwd_workspace(int64_t B, int K);
int rm_autoint_head_bwd(const float *Y, const float *w, const float *g, int64_t B, int K, float *dY,
                        float *dw, float *dw0, float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * DLRM's dot interaction (arXiv 1906.00091 section 3; the 351-pair layer of MLPerf DLRM at
 * F = 26), forward and backward fused.  Nothing in the reference implements it.  Per example,
 * over the T = F + 1 vectors v_0 = z and v_f = E[f-1] (f = 1..F), P = F(F+1)/2:
 *     X[0:D] = z (the same bits);  X[D + i(i-1)/2 + j] = <v_i, v_j>  for 0 <= j < i <= F
 *   (the strict lower triangle, row-major: (1,0), (2,0), (2,1), (3,0), ...; no diagonal).
 *   E [B,F,D] (the gathered rows, rm_embed_fwd's E) and z [B,D] contiguous, 16-byte aligned;
 *   X [B, ldx], ldx >= D + P, rows need no alignment; columns [D + P, ldx) are set to +0.0.
 *   Every dot product is a k-ordered fmaf chain.
 * Supported: D in {8,16,32,64}, 1 <= F <= 40 (rm_dot_interact_supported); anything else is
 *   RM_EINVAL before any launch.  B = 0 is RM_OK.  The [T,T] Gram matrix never reaches HBM.
 * rm_dot_interact_bwd, given dX [B, ldx] = dLoss/dX (columns >= D + P are never read), writes
 *   d_rows [B,F,D] and dz [B,D] (both fully overwritten, 16-byte aligned):
 *     G_ij = G_ji = dX[D + p(i,j)], G_ii = 0;  dV = G V (summed over j in ascending order)
 *     d_rows[f-1] = dV_f;  dz = dV_0 + dX[0:D]
 * Deterministic: no parameters, so no batch reduction; no atomics, no workspace - two runs on
 *   the same inputs are bit-equal.
 */
int rm_dot_interact_supported(int F, int D);
int rm_dot_interact_fwd(const float *E, const float *z, int64_t B, int F, int D, float *X,
                        int64_t ldx, rm_stream_t stream);
int rm_dot_interact_bwd(const float *E, const float *z, const float *dX, int64_t ldx, int64_t B,
                        int F, int D, float *d_rows, float *dz, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * The core of a DCN-Mix cross layer (DCN-V2, arXiv 2008.13535 eq. 4-5): everything between the
 * layer's projection GEMM and its output GEMM, fused (csrc/cross_mix.hip).  Nothing in the
 * reference implements it.  Per example, E experts of rank r, W = E r, expert i owning columns
 * [i r, i r + r):
 *     a_i = tanh(t_i);  c_i = tanh(a_i C_i);  p = softmax_i(s), max-subtracted;  m_i = p_i c_i
 *   T [B, ldt] (W columns used), S [B, lds] (E columns used), M [B, ldm] (W columns written):
 *   every [B, .] argument is a pointer and a row stride in floats, stride >= width, rows need no
 *   alignment - T | S may be column ranges of one buffer; columns past the width are never read
 *   or written.  C [E, r, r] contiguous.  Each r x r product is a k-ordered fmaf chain.
 * rm_cross_mix_bwd, given dM = dLoss/dM, recomputes a, c and p and writes dT, dS (owned columns
 *   only) and dC [E, r, r] (overwritten; all zero at B = 0):
 *     dc_i = p_i dm_i;  dp_i = <dm_i, c_i>;  ds_i = p_i (dp_i - sum_j p_j dp_j)   (+0.0 at E = 1)
 *     dh_i = dc_i o (1 - c_i^2);  dC_i = sum_b a_i^T dh_i;  da_i = dh_i C_i^T;  dt_i = da_i o (1 - a_i^2)
 *   workspace: rm_cross_mix_bwd_workspace(B, E, r) floats (per-block partial dC, summed in block
 *   order by a finish kernel: no atomics, two runs are bit-equal); -1 for an unsupported shape.
 * Supported: 1 <= E <= 8, r in {8,16,32,64}, E r <= 256 (rm_cross_mix_supported); anything else,
 *   a NULL pointer or a stride below its width is RM_EINVAL before any launch.  B = 0 is RM_OK.
 * a, h, c, p and dh never reach HBM: the forward moves 4 (2 W + E) bytes per example, the
 *   backward reads 4 (2 W + E) and writes 4 (W + E).
 */
int rm_cross_mix_supported(int E, int r);
int rm_cross_mix_fwd(const float *T, int64_t ldt, const float *S, int64_t lds, const float *C, int E,
                     int r, int64_t B, float *M, int64_t ldm, rm_stream_t stream);
int64_t rm_cross_mix_bwd_workspace(int64_t B, int E, int r);
int rm_cross_mix_bwd(const float *T, int64_t ldt, const float *S, int64_t lds, const float *C, int E,
                     int r, int64_t B, const float *dM, int64_t lddm, float *dT, int64_t lddt,
                     float *dS, int64_t ldds, float *dC, float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * FiBiNET's interaction (arXiv 1905.09433): a squeeze-excitation gate over the F embedding rows
 * and a bilinear interaction over every field pair, on the raw and on the re-weighted rows,
 * fused (csrc/fibinet.hip).  Nothing in the reference implements it.  Per example, E [F, D],
 * P = F(F-1)/2, pairs p = (i, j), 0 <= i < j < F, i-major (itertools.combinations order):
 *     z_f = (1/D) sum_d E[f,d];  s = relu(z W1);  a = relu(s W2);  V[f] = a_f E[f]    (no biases)
 *     bilinear(Y, W)[p, d] = (sum_k Y[i,k] W_(i)[k,d]) Y[j,d]
 *     X = [ bilinear(E, Wb) | bilinear(V, Wsb) ]           2 P D columns, pair-major, d fastest
 *   type RM_FIBINET_ALL: W_(i) = W[0], Wb and Wsb [1, D, D];  RM_FIBINET_EACH: W_(i) = W[i] (the
 *   LEFT field selects the matrix), Wb and Wsb [F-1, D, D].  W1 [F, R], W2 [R, F].  All contiguous.
 *   E [B, F, D] contiguous, 16-byte aligned (rm_embed_fwd's E).  X [B, ldx], ldx >= 2 P D, rows
 *   need no alignment; columns [2 P D, ldx) are left untouched.  The gate (z, s, a) and the left
 *   products sum_k Y[i,k] W_(i)[k,d] are summed in ascending order in float64 and rounded to float
 *   once (X keeps the D axis: a cancelling left product times a large row entry would otherwise
 *   carry a relative error of 1e-5 and more); everything else is float32 fmaf chains.
 * rm_fibinet_bwd, given dX [B, lddx] = dLoss/dX (columns >= 2 P D are never read), recomputes z,
 *   s, a, V and the left products and writes dE [B, F, D] (overwritten, 16-byte aligned) and the
 *   four parameter gradients dW1 [F,R], dW2 [R,F], dWb, dWsb (overwritten; all zero at B = 0),
 *   relu'(0) = 0:
 *     dU_i[d] = sum_{j>i} dX[p,d] Y[j,d];  dY_j[d] += sum_{i<j} dX[p,d] U_i[d];  dY_i += dU_i W_(i)^T
 *     dW_(i) += Y_i^T dU_i;  dE = dY(E) + a o dV;  da_f = <dV_f, E_f>;  back through the relus, W2
 *     and W1;  dE[f,d] += dz_f / D
 *   workspace: rm_fibinet_bwd_workspace(B, F, D, R, type) floats (per-block partial gradients,
 *   2 nW D D + 2 F R each over at most 512 blocks - fewer, down to 128, where that would pass
 *   32 MB -, summed in block order by a finish kernel: no
 *   atomics, two runs are bit-equal); 0 at B = 0, -1 for an unsupported shape.
 * rm_fibinet_tile: the examples per tile of the forward (backward = 0) or backward kernel, -1 for
 *   an unsupported shape; both grids are capped at 512 blocks and grid-stride the rest.
 * Supported: D in {8,16,32}, 2 <= F <= 40, 1 <= R <= F, type ALL or EACH (rm_fibinet_supported);
 *   anything else, a NULL pointer or a stride below 2 P D is RM_EINVAL before any launch.  B = 0
 *   is RM_OK.  z, s, a, V and the left products never reach HBM: the forward moves
 *   4 (F D + 2 P D) bytes per example, the backward reads 4 (F D + 2 P D) and writes 4 F D.
 */
#define RM_FIBINET_ALL 0
#define RM_FIBINET_EACH 1
int rm_fibinet_supported(int F, int D, int R, int type);
int rm_fibinet_tile(int F, int D, int R, int type, int backward);
int rm_fibinet_fwd(const float *E, const float *W1, const float *W2, const float *Wb, const float *Wsb,
                   int64_t B, int F, int D, int R, int type, float *X, int64_t ldx, rm_stream_t stream);
int64_t rm_fibinet_bwd_workspace(int64_t B, int F, int D, int R, int type);
int rm_fibinet_bwd(const float *E, const float *W1, const float *W2, const float *Wb, const float *Wsb,
                   const float *dX, int64_t lddx, int64_t B, int F, int D, int R, int type, float *dE,
                   float *dW1, float *dW2, float *dWb, float *dWsb, float *workspace,
                   rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Field-pair weighted FM: FwFM (arXiv 1806.03514), FvFM and FmFM (arXiv 2102.12994), fused
 * (csrc/fmfm.hip).  Nothing in the reference implements them.  Per example, E [F, D],
 * P = F(F-1)/2, pairs p = (i, j), 0 <= i < j < F, i-major (itertools.combinations order):
 *     logit = sum_p E_i W_(p) E_j^T
 *   type RM_FMFM_MATRIX: W_(p) = W[p], W [P, D, D] (the LEFT field i on the rows);
 *   RM_FMFM_VECTOR: W_(p) = diag(W[p]), W [P, D];  RM_FMFM_SCALAR: W_(p) = W[p] I, W [P].
 *   E [B, F, D] contiguous, 16-byte aligned (rm_embed_fwd's E); W contiguous; logit [B] is
 *   overwritten.  The matrix type runs on the exact-f32 MFMA (fmaf chains of length D inside a
 *   pair; pair sums are added in per-lane chains of at most P / 8 and reduced by a tree), the other
 *   two on the vector ALU (chains of at most F - 1 inside, F - 1 outside): no chain over all
 *   P D D products exists.
 * rm_fmfm_bwd, given g [B] = dLoss/dlogit:
 *     dE_i += g W_(p) E_j;  dE_j += g W_(p)^T E_i;  dW[p] = sum_b g_b E_i (x) E_j  (its diagonal for
 *     VECTOR, its trace for SCALAR)
 *   d_rows [B, F, D] = dE_up + dE when dE_up is given (it may be d_rows itself), dE otherwise -
 *   written once; dW (the shape of W) is overwritten.
 *   workspace: rm_fmfm_bwd_workspace(B, F, D, type) floats: the partial dW of at most 64 batch
 *   slices (MATRIX; 512 for VECTOR and SCALAR; fewer where that many sets would pass 32 MB),
 *   summed in slice order by a finish kernel: no atomics, two runs are bit-equal; 0 at B = 0,
 *   -1 for an unsupported shape.
 * rm_fmfm_tile(F, D, type, which): the examples per tile of the forward / dE / dW kernel
 *   (RM_FMFM_TILE_*) and the cap of the forward's and dE's grids and of the dW kernels' batch
 *   slices (RM_FMFM_CAP_*): beyond cap x tile examples a block walks the batch with a grid stride.
 *   -1 for an unsupported shape or `which`.
 * Supported: D in {8,16,32}, 2 <= F <= 40, type MATRIX, VECTOR or SCALAR (rm_fmfm_supported);
 *   anything else or a NULL pointer is RM_EINVAL before any launch.  B = 0 is RM_OK and touches
 *   nothing.  Nothing of size P leaves the chip: the forward reads 4 F D bytes per example and
 *   writes 4; the backward reads E twice (dE kernel, dW kernel: the matrix dW kernel once per
 *   chunk of 64 pairs - 16 at D = 32 -, from L2 after the first) and writes d_rows once.
 */
#define RM_FMFM_MATRIX 0
#define RM_FMFM_VECTOR 1
#define RM_FMFM_SCALAR 2
#define RM_FMFM_TILE_FWD 0
#define RM_FMFM_TILE_DE 1
#define RM_FMFM_TILE_DW 2
#define RM_FMFM_CAP_FWD 3
#define RM_FMFM_CAP_DE 4
#define RM_FMFM_CAP_DW 5
int rm_fmfm_supported(int F, int D, int type);
int rm_fmfm_tile(int F, int D, int type, int which);
int rm_fmfm_fwd(const float *E, const float *W, int type, int64_t B, int F, int D, float *logit,
                rm_stream_t stream);
int64_t rm_fmfm_bwd_workspace(int64_t B, int F, int D, int type);
int rm_fmfm_bwd(const float *E, const float *W, int type, const float *g, const float *dE_up,
                int64_t B, int F, int D, float *d_rows, float *dW, float *workspace,
                rm_stream_t stream);

/* ------------------------------------------------------------------------
 * The product layer of the Product-based Neural Network (PNN, arXiv 1611.00144), fused
 * (csrc/pnn.hip): the kernel-form layer of the widely used open-source PNN (use_inner,
 * use_outter, kernel_type mat / vec / num), NOT the paper's sum-pooled outer-product shortcut.
 * Nothing in the reference implements it.  Per example, E [F, D], P = F(F-1)/2, pairs p = (i, j),
 * 0 <= i < j < F, i-major (itertools.combinations order):
 *     inner[p] = <E_i, E_j>
 *     outer[p] = E_i K_(p) E_j^T
 *   kernel_type RM_PNN_MAT: K_(p) = K[p], K [P, D, D] (the LEFT field i on the rows);
 *   RM_PNN_VEC: K_(p) = diag(K[p]), K [P, D];  RM_PNN_NUM: K_(p) = K[p] I, K [P].
 *     X = [ E flattened (F D columns, the same bits) | inner (P, with RM_PNN_INNER) |
 *           outer (P, with RM_PNN_OUTER) ]                       W = F D + n P columns
 *   products: a non-empty bit set of RM_PNN_INNER and RM_PNN_OUTER.  E [B, F, D] contiguous,
 *   16-byte aligned (rm_embed_fwd's E); K contiguous, may be NULL without OUTER (kernel_type
 *   must still be one of the three).  X [B, ldx], ldx >= W, rows need no alignment; columns
 *   [W, ldx) are set to +0.0.  Every product is accumulated in float64 and rounded to float once
 *   (X keeps every pair: a product of a row of large entries that cancels to below 1 would
 *   otherwise carry an absolute error of 1e-5 and more at D >= 16).  INNER, VEC and NUM products
 *   are k-ordered fma chains of length D on the vector ALU.  A MAT product is U = E_i K[p] on
 *   v_mfma_f64_16x16x4_f64 (per column d a k-ordered chain of length D), then sum_d U[d] E_j[d]:
 *   per lane a chain over four d (eight at D = 32), the four lane groups added by two shuffle
 *   steps.  The backward is float32: fmaf chains, and v_mfma_f32_16x16x4_f32 for MAT.
 * rm_pnn_bwd, given dX [B, lddx] = dLoss/dX (lddx >= W; columns >= W are never read), with G_in
 *   and G_out its two product column blocks:
 *     dE_i += G_in[p] E_j + G_out[p] K_(p) E_j;   dE_j += G_in[p] E_i + G_out[p] K_(p)^T E_i
 *     d_rows [B, F, D] = dX[:, 0:FD] + dE, written once
 *     dK[p] = sum_b G_out[b,p] E_bi (x) E_bj  (its diagonal for VEC, its trace for NUM)
 *   d_rows and dK (the shape of K) are overwritten; dK and the workspace may be NULL without
 *   OUTER.  workspace: rm_pnn_bwd_workspace(B, F, D, products, kernel_type) floats: the partial
 *   dK of at most 64 batch slices (MAT; 512 for VEC and NUM; fewer where that many sets would
 *   pass 32 MB), summed in slice order by a finish kernel: no atomics, two runs are bit-equal;
 *   0 at B = 0 or without OUTER, -1 for an unsupported shape.
 * rm_pnn_tile(F, D, products, kernel_type, which): the examples per tile of the forward / dE /
 *   dK kernel (RM_PNN_TILE_*) and the cap of the forward's and dE's grids and of the dK kernels'
 *   batch slices (RM_PNN_CAP_*): beyond cap x tile examples a block walks the batch with a grid
 *   stride.  The dK entries are 0 without OUTER.  -1 for an unsupported shape or `which`.
 * Supported: D in {8,16,32}, 2 <= F <= 40, products 1..3, kernel_type MAT, VEC or NUM
 *   (rm_pnn_supported); anything else, a NULL pointer or a stride below W is RM_EINVAL before any
 *   launch.  B = 0 is RM_OK and touches nothing.  Nothing of size P D leaves the chip: the
 *   forward reads 4 F D bytes per example and writes 4 ldx; the backward reads E and dX twice
 *   with OUTER (dE kernel, dK kernel: the MAT dK kernel once per chunk of 64 pairs - 16 at
 *   D = 32 -, from L2 after the first), once without, and writes d_rows once.
 */
#define RM_PNN_INNER 1
#define RM_PNN_OUTER 2
#define RM_PNN_MAT 0
#define RM_PNN_VEC 1
#define RM_PNN_NUM 2
#define RM_PNN_TILE_FWD 0
#define RM_PNN_TILE_DE 1
#define RM_PNN_TILE_DK 2
#define RM_PNN_CAP_FWD 3
#define RM_PNN_CAP_DE 4
#define RM_PNN_CAP_DK 5
int rm_pnn_supported(int F, int D, int products, int kernel_type);
int rm_pnn_tile(int F, int D, int products, int kernel_type, int which);
int rm_pnn_fwd(const float *E, const float *K, int products, int kernel_type, int64_t B, int F, int D,
               float *X, int64_t ldx, rm_stream_t stream);
int64_t rm_pnn_bwd_workspace(int64_t B, int F, int D, int products, int kernel_type);
int rm_pnn_bwd(const float *E, const float *K, int products, int kernel_type, const float *dX,
               int64_t lddx, int64_t B, int F, int D, float *d_rows, float *dK, float *workspace,
               rm_stream_t stream);

/* ------------------------------------------------------------------------
 * MaskNet (arXiv 2102.07619): the normalise-and-mask passes around its dense layers, fused
 * (csrc/masknet.hip).  Nothing in the reference implements it.  eps = 1e-5 inside the root,
 * biased variance; a row's mean and centred sum of squares are accumulated in float64 (centred
 * before squaring) and xhat is rounded to float32 once; the rest is float32 fmaf chains.
 *
 * a. Group-LayerNorm times N masks.  Per example, X = E [F, D], gamma / beta [F, D]:
 *     V[f,:] = gamma[f,:] o (E[f,:] - mean_f) / sqrt(var_f + eps) + beta[f,:];   Y_n = M_n o V
 *   X [B, F, D] contiguous, 16-byte aligned (rm_embed_fwd's E); M, Y: host arrays of N device
 *   pointers to [B, F D] buffers of row stride ldm / ldy >= F D floats - any stride and alignment
 *   (float4 accesses when every pointer is 16-byte aligned and the strides are multiples of 4,
 *   per-element ones otherwise); each may be a column range of a wider buffer.  V, the means and
 *   the inverse deviations never reach HBM.
 * rm_masknet_group_bwd, given dY_n (row stride lddy), recomputes the statistics from X:
 *     dM_n = dY_n o V (row stride lddm; dM[n] MAY be dY[n] itself, with lddm = lddy: a thread
 *     reads its elements of dY_n before it writes them; no other overlap is allowed: dM[n] equal
 *     to a mask or to another dY[k] is RM_EINVAL)
 *     dV = sum_n dY_n o M_n;  dgamma = sum_b dV o xhat;  dbeta = sum_b dV   ([F, D], overwritten)
 *     dE = rstd (dxhat - mean(dxhat) - xhat mean(dxhat o xhat)), dxhat = dV o gamma
 *   d_rows [B, F, D] = dE_up + dE when dE_up is given (it may be d_rows itself), dE otherwise -
 *   written once.  workspace: rm_masknet_group_bwd_workspace(B, F, D) floats, 16-byte aligned:
 *   one partial dgamma | dbeta set per (block, example slot) of a grid of at most 512 blocks,
 *   (fewer where the sets would pass 16 MB), summed in a fixed order in float64 by a finish
 *   kernel: no atomics, two runs are bit-equal; 0 at B = 0, -1 for an unsupported shape.
 * normalize = 0 (MaskNet's serial blocks 2..N): X = h_prev [B, H] contiguous, called with F = 1,
 *   D = H, N = 1; gamma, beta, dgamma, dbeta, workspace NULL:
 *     Y = M o X;   dM = dY o X;   d_rows [B, H] = (dE_up +) dY o M
 * Supported (rm_masknet_group_supported(F, D, N, normalize)): normalize = 1: D in {8,16,32},
 *   1 <= F <= 40, 1 <= N <= 8;  normalize = 0: F = 1, N = 1, D a multiple of 4 in 8..2048.
 *   Anything else, a short stride or a NULL pointer is RM_EINVAL before any launch; B = 0 is RM_OK
 *   and touches nothing.
 * rm_masknet_group_tile(F, D, normalize, which): RM_MASKNET_TILE the examples per block pass,
 *   RM_MASKNET_CAP the grid cap - beyond cap x tile examples a block walks the batch with a grid
 *   stride; -1 for an unsupported shape or `which`.
 * Bytes: forward 4 B F D (1 + 2 N) + 8 F D (X and M_n in, Y_n out, the parameters);
 *   backward 4 B F D (2 + 3 N) (+ 4 B F D with dE_up) + the partial sets.
 *
 * b. Row-LayerNorm + ReLU: Z [B, H] contiguous, gamma / beta [H]:
 *     h[b, :] = relu(gamma o (Z[b,:] - mean_b) / sqrt(var_b + eps) + beta)     row stride ldh >= H
 * rm_masknet_row_bwd, given dh (row stride lddh; relu'(0) = 0), recomputes the statistics from Z
 *   (saving mean and rstd would add 8 bytes per row to the forward and save none in the backward,
 *   which reads Z for xhat either way) and writes dZ [B, H] contiguous (neither Z nor dh itself:
 *   RM_EINVAL; no other overlap of an output with an input is supported), dgamma and
 *   dbeta [H] - deterministic as above, workspace rm_masknet_row_bwd_workspace(B, H) floats.
 * Supported (rm_masknet_row_supported): H a multiple of 4 in 8..2048; ldh, lddh multiples of 4;
 *   every pointer 16-byte aligned.  Bytes: forward 8 B H, backward 12 B H + the partial sets.
 */
#define RM_MASKNET_TILE 0
#define RM_MASKNET_CAP 1
int rm_masknet_group_supported(int F, int D, int N, int normalize);
int rm_masknet_group_tile(int F, int D, int normalize, int which);
int rm_masknet_group_fwd(const float *X, const float *gamma, const float *beta, int normalize,
                         const float *const *M, int64_t ldm, int N, int64_t B, int F, int D,
                         float *const *Y, int64_t ldy, rm_stream_t stream);
int64_t rm_masknet_group_bwd_workspace(int64_t B, int F, int D);
int rm_masknet_group_bwd(const float *X, const float *gamma, const float *beta, int normalize,
                         const float *const *M, int64_t ldm, const float *const *dY, int64_t lddy,
                         float *const *dM, int64_t lddm, int N, const float *dE_up, int64_t B, int F,
                         int D, float *d_rows, float *dgamma, float *dbeta, float *workspace,
                         rm_stream_t stream);
int rm_masknet_row_supported(int H);
int rm_masknet_row_tile(int H, int which);
int rm_masknet_row_fwd(const float *Z, const float *gamma, const float *beta, int64_t B, int H,
                       float *h, int64_t ldh, rm_stream_t stream);
int64_t rm_masknet_row_bwd_workspace(int64_t B, int H);
int rm_masknet_row_bwd(const float *Z, const float *gamma, const float *beta, const float *dh,
                       int64_t lddh, int64_t B, int H, float *dZ, float *dgamma, float *dbeta,
                       float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Attention-pooled behaviour sequences: SequenceFeat + DIN's local activation unit (Deep
 * Interest Network, arXiv 1706.06978 section 4.3).  Replaces ASPCombiner / ASPLayer, which
 * DIN.py:6 imports and which exist nowhere in the reference (SequenceFeat.__init__ raises,
 * inputs.py:443).  CSR input: example b owns history ids ids[offsets[b] .. offsets[b+1]),
 * offsets[B] == nnz.  rows [*, LD]: the fused table; a history id addresses row row0 + id
 * (the query feature's block), the example's query is row qrow[b] (absolute).  Per example:
 *     x_l = [q, k_l, q - k_l, q * k_l] (4D, columns 0..D-1 of the rows)
 *     z   = act(.. act(x_l W0 + b0) .. )     n_layers = 1 or 2, widths H[], W0 [4D,H0], W1 [H0,H1]
 *     s_l = z . w + w0;   a_l = s_l (norm = 0)  or  softmax over the example's l (norm = 1, max-
 *     subtracted);   out_b = sum_l a_l k_l;  no history -> 0
 *   act: RM_ASP_RELU / RM_ASP_SIGMOID.
 * rm_asp_fwd writes out [B, LD] (out_b in columns 0..D-1, zeros behind) and scores [nnz] = s_l: the
 *   one per-position value that reaches HBM and all the backward needs (inference passes the same
 *   kind of buffer: one code path, the pooled rows are the same bits).  workspace:
 *   rm_asp_workspace(D, n_layers, H, nnz, 0) floats.
 * rm_asp_bwd, given d_out (the pooled rows' gradient, row b at d_out + b * do_stride, D floats),
 *   recomputes x and the hidden layers and writes  d_keys [nnz, D] (the gradient of every history
 *   occurrence's row), ADDS the query gradient onto d_query[b * dq_stride + 0..D-1] (one example
 *   per lane group), and overwrites dW0, db0, dW1, db1 (NULL with one layer), dw [H_last], dw0 [1].
 *   workspace: rm_asp_workspace(D, n_layers, H, nnz, 1) floats, 16-byte aligned.
 * Supported (rm_asp_supported): D in {8,16,32}, 1 or 2 hidden layers of 1..128 units, max_len
 *   1..256; anything else is RM_EINVAL before any launch.
 * Deterministic: per-block partial sums added in block order, fixed-order sums inside a block,
 *   no float atomics - two runs on the same inputs are bit-equal. */
#define RM_ASP_RELU 0
#define RM_ASP_SIGMOID 1
int rm_asp_supported(int D, int n_layers, const int *H, int max_len);
int64_t rm_asp_workspace(int D, int n_layers, const int *H, int64_t nnz, int backward);
int rm_asp_fwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
               const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz, const float *W0,
               const float *b0, const float *W1, const float *b1, const float *w, const float *w0,
               int n_layers, const int *H, int act, int norm, float *out, float *scores,
               float *workspace, rm_stream_t stream);
int rm_asp_bwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
               const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz, const float *W0,
               const float *b0, const float *W1, const float *b1, const float *w, const float *w0,
               int n_layers, const int *H, int act, int norm, const float *scores, const float *d_out,
               int64_t do_stride, float *d_keys, float *d_query, int64_t dq_stride, float *dW0,
               float *db0, float *dW1, float *db1, float *dw, float *dw0, float *workspace,
               rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Transformer-pooled behaviour sequences: SequenceFeat + one post-norm encoder block (Behavior
 * Sequence Transformer, arXiv 1905.06874).  New: the reference has none.  CSR input and addressing
 * as rm_asp_fwd (rows, LD, row0, offsets, ids oldest first, qrow; only columns 0..D-1 of a row are
 * read).  Per example with n <= max_len history rows k_i and query row q, T = n + 1 tokens, the
 * candidate LAST:
 *     x_i = k_i + P[n - i] (i < n),  x_n = q + P[0]       P = pos [max_len + 1, D]: by distance
 *     Q, K, V = X Wq + bq, X Wk + bk, X Wv + bv            W* [D, D] ([in, out]), dk = D / heads
 *     a^h = softmax_j(Q^h_i . K^h_j / sqrt(dk))            max-subtracted, no mask
 *     O = concat_h(a^h V^h) Wo + bo
 *     Y = LayerNorm(X + O; ln1_gamma, ln1_beta)            eps 1e-5, biased variance, over D
 *     Z = LayerNorm(Y + relu(Y W1 + c1) W2 + c2; ln2_*)    W1 = ffn_w1 [D, Hf], W2 = ffn_w2 [Hf, D]
 *     out_b = (1 / T) sum_i Z_i                            no history: T = 1 and out_b = Z_0, not 0
 *   rm_bst_params: the 17 device pointers, read on the host at call time; the same struct carries
 *   the 17 gradient destinations.
 * rm_bst_fwd writes out [B, LD] (out_b in columns 0..D-1, zeros behind).  It saves nothing: no
 *   per-token value reaches HBM, and inference is the same call (the same bits).  workspace:
 *   rm_bst_workspace(D, heads, Hf, max_len, B, 0) floats.
 * rm_bst_bwd, given d_out (the pooled rows' gradient, row b at d_out + b * do_stride, D floats),
 *   recomputes the block and writes d_keys [nnz, D] (the gradient of every history occurrence's
 *   row), ADDS the candidate's gradient onto d_query[b * dq_stride + 0..D-1] (d_query may be other
 *   columns of the buffer that holds d_out) and overwrites all 17 members of grads (all zero at
 *   B = 0).  workspace: rm_bst_workspace(.., B, 1) floats, 16-byte aligned.
 * Supported (rm_bst_supported): D in {8,16,32}; heads in {1,2,4,8} with D / heads >= 4; Hf a
 *   multiple of 4 in 4..128; max_len 1..63; anything else is RM_EINVAL before any launch.  A
 *   history longer than max_len is a caller error that is made safe: its LAST max_len items are
 *   used (what th.SequenceFeat keeps) and the d_keys rows of the others are written as zeros.
 * Deterministic: a fixed assignment of examples to blocks, per-block partial sums added in block
 *   order, fixed-order sums inside a block, no float atomics - two runs are bit-equal. */
typedef struct rm_bst_params {
  float *wq, *wk, *wv, *wo;             /* [D, D] */
  float *bq, *bk, *bv, *bo;             /* [D] */
  float *ffn_w1, *ffn_b1;               /* [D, Hf], [Hf] */
  float *ffn_w2, *ffn_b2;               /* [Hf, D], [D] */
  float *ln1_gamma, *ln1_beta, *ln2_gamma, *ln2_beta; /* [D] */
  float *pos;                           /* [max_len + 1, D] */
} rm_bst_params;
int rm_bst_supported(int D, int heads, int Hf, int max_len);
int64_t rm_bst_workspace(int D, int heads, int Hf, int max_len, int64_t B, int backward);
int rm_bst_fwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
               const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
               const rm_bst_params *params, int heads, int Hf, int max_len, float *out,
               float *workspace, rm_stream_t stream);
int rm_bst_bwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
               const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
               const rm_bst_params *params, int heads, int Hf, int max_len, const float *d_out,
               int64_t do_stride, float *d_keys, float *d_query, int64_t dq_stride,
               const rm_bst_params *grads, float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Interest-evolution pooling of behaviour sequences: SequenceFeat + a GRU, an attention and an
 * attention-gated GRU over the history (Deep Interest Evolution Network, arXiv 1809.03672).  New:
 * the reference has none.  CSR input and addressing as rm_asp_fwd (rows, LD, row0, offsets, ids
 * oldest first, qrow; only columns 0..D-1 of a row are read).  Matrices are [in, out]; the column
 * blocks of a [D, 3D] matrix are [u | r | c].  Per example with history rows k_1..k_n
 * (n <= max_len) and query row q:
 *     cell(x, h; W, U, b, a):                              one bias; r applied AFTER the product
 *         u = sigmoid(x Wu + h Uu + bu)                    with U (paper eq. 1-4)
 *         r = sigmoid(x Wr + h Ur + br)
 *         c = tanh(x Wc + r * (h Uc) + bc)
 *         u = a u;  return (1 - u) h + u c                 (eq. 15-16; a = 1 in the extractor)
 *     h_0 = 0,  h_t = cell(k_t, h_{t-1}; gru_w, gru_u, gru_b, 1)
 *     s_t = h_t . (att_w q)                                att_w [D, D] (eq. 13)
 *     a = softmax_t(s)                                     max-subtracted, the example's n positions
 *     g_0 = 0,  g_t = cell(h_t, g_{t-1}; augru_w, augru_u, augru_b, a_t)
 *     out_b = g_n                                          n = 0: out_b = 0 and no gradient
 *   The hidden size is D; there is no auxiliary loss, no AIGRU / AGRU variant and no dropout.
 *   sigmoid and tanh stay finite for pre-activations of any size.  The forward forms h_t and s_t in
 *   float64 (|att_w q| multiplies h_t's error into the softmax) and stores h_t rounded to float.
 *   rm_dien_params: the 7 device pointers, read on the host at call time; the same struct carries
 *   the 7 gradient destinations.
 * rm_dien_fwd writes out [B, LD] (out_b in columns 0..D-1, zeros behind) and leaves h_t and a_t in
 *   the workspace; with save != 0 also g_t, which rm_dien_bwd needs.  `out` has the same bits for
 *   save 0 and 1.  workspace: rm_dien_workspace(D, max_len, B, nnz, save) floats.
 * rm_dien_bwd, called after a save forward on the same inputs and workspace, given d_out (the
 *   pooled rows' gradient, row b at d_out + b * do_stride, D floats), writes d_keys [nnz, D] (the
 *   gradient of every history occurrence's row), ADDS the query gradient onto
 *   d_query[b * dq_stride + 0..D-1] (d_query may be other columns of the buffer that holds d_out,
 *   which comes back unchanged) and overwrites all 7 members of grads (all zero at B = 0 or
 *   nnz = 0).  workspace: rm_dien_workspace(.., 1) floats, 16-byte aligned.
 * Supported (rm_dien_supported): D in {8,16,32}; max_len 1..256; anything else is RM_EINVAL before
 *   any launch and a workspace of 0.  A history longer than max_len is a caller error that is made
 *   safe: its LAST max_len items are used (what th.SequenceFeat keeps) and the d_keys rows of the
 *   others are written as zeros; offsets are clamped to [0, nnz], so no loop bound comes from
 *   unchecked input.
 * Deterministic: a fixed assignment of examples (and, for the weight gradients, of positions) to
 *   blocks, per-block partial sums added in block order, fixed-order sums inside a block, no float
 *   atomics - two runs are bit-equal. */
typedef struct rm_dien_params {
  float *gru_w, *gru_u, *gru_b;         /* [D, 3D], [D, 3D], [3D] */
  float *att_w;                         /* [D, D] */
  float *augru_w, *augru_u, *augru_b;   /* [D, 3D], [D, 3D], [3D] */
} rm_dien_params;
int rm_dien_supported(int D, int max_len);
int64_t rm_dien_workspace(int D, int max_len, int64_t B, int64_t nnz, int backward);
int rm_dien_fwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
                const rm_dien_params *params, int max_len, int save, float *out, float *workspace,
                rm_stream_t stream);
int rm_dien_bwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
                const rm_dien_params *params, int max_len, const float *d_out, int64_t do_stride,
                float *d_keys, float *d_query, int64_t dq_stride, const rm_dien_params *grads,
                float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * CIN (xDeepFM), one layer, on the f32-input MFMA.
 * Replaces the loop body of CIN.__call__ (layers.py:714-752):
 *   Z[b,d,i*H+j] = X0[b,i,d] * Xk[b,j,d];  M = Z @ W + bias;  out = act(M)
 *   out laid out [B,N,D] (after the transpose of layers.py:739); Z is never formed.
 *   X0 [B,m,D]; Xk: rows j < H of a [B,*,D] tensor with xk_bstride floats between
 *   examples (the "next hidden" half of the previous layer's map, layers.py:744-746);
 *   W [m*H, N] (cin_filter_k[0]), bias [N].
 *   pooled [B, pool_stride]: when not NULL, sum_d out[b,n,d] for n in [pool_from, N)
 *   is written to pooled[b, pool_col0 + n - pool_from] (the direct-connect half and
 *   the reduce_sum of layers.py:751-755).
 *   filter_ws: scratch of rm_cin_filter_workspace(m,H,N) floats (the filter
 *   re-laid out as MFMA B-operand; rewritten by every call).
 * N <= 128; D a multiple of 4 dividing 256; (m+1+H)*1 KiB + 32 KiB of LDS <= 160 KiB.
 */
int64_t rm_cin_filter_workspace(int m, int H, int N);
int rm_cin_layer_fwd(const float *X0, const float *Xk, int64_t xk_bstride, const float *W,
                     const float *bias, int act, int64_t B, int m, int H, int N, int D,
                     float *out, float *pooled, int pool_stride, int pool_col0, int pool_from,
                     float *filter_ws, rm_stream_t stream);
/* rm_cin_layer_fwd6: the same layer on the bf16 matrix pipe with split fp32 operands (csrc/cin6.hip; the scheme of
 * rm_dense_fwd6): Z = fl(X0 * Xk) is formed in fp32 as the reference does, then split into three bf16 pieces; six
 * exact piece products per k-step, fp32 accumulate - fp32-level error.  Covers H <= 64 (padded to a multiple of 32),
 * N <= 128, D in {16, 32, 64}; RM_EUNSUPPORTED otherwise (run rm_cin_layer_fwd, which is also the better choice
 * for the first layer: its symmetric k' ordering does half the work).
 * filter_ws: rm_cin_filter_workspace6(m, H, N, D) floats (0 = not covered), 16-byte aligned. */
int64_t rm_cin_filter_workspace6(int m, int H, int N, int D);
int rm_cin_layer_fwd6(const float *X0, const float *Xk, int64_t xk_bstride, const float *W, const float *bias,
                      int act, int64_t B, int m, int H, int N, int D, float *out, float *pooled, int pool_stride,
                      int pool_col0, int pool_from, float *filter_ws, rm_stream_t stream);

/* Backward of one CIN layer (three MFMA passes over the same GEMM shape).
 *   out [B,N,D]: the layer's post-activation map (act' is read off its sign);
 *   the gradient w.r.t. out is never materialised by the caller:
 *     n <  pool_from: d_hidden[b,n,d]  (the next layer's dXk, dh_bstride floats per example)
 *     n >= pool_from: g[b] * cin_w_direct[n - pool_from]   (reduce_sum + cin_w, layers.py:754-758)
 *   dX0 [B,m,D] (+= when accumulate_dx0 & 1) = sum_j (dM @ W^T)[.,(i,j)] * Xk[b,j,d]
 *        accumulate_dx0 & 2: the dX pass runs on the bf16 matrix pipe with split fp32 operands (csrc/cin6.hip, the
 *        scheme of rm_cin_layer_fwd6), and the dW pass too, where csrc/cin6.hip covers the layer (H <= 64, 64 < N <=
 *        128, D in {16, 32, 64}; not the first layer, whose symmetric f32 kernels do half the work - & 4: its dX too)
 *   dXk [B,H,D] (dxk_bstride floats per example) = sum_i (dM @ W^T)[.,(i,j)] * X0[b,i,d];
 *        with xk_is_x0 (first layer: Xk is X0 itself) it is added into dX0 instead
 *   dW [m*H,N] = Z^T @ dM,  dbias [N] = colsum(dM)   (dM = d_out * act'(out))
 *   workspace: rm_cin_bwd_workspace(B,m,H,N,D) floats.  D must divide 64. */
int64_t rm_cin_bwd_workspace(int64_t B, int m, int H, int N, int D);
int rm_cin_layer_bwd(const float *X0, const float *Xk, int64_t xk_bstride, int xk_is_x0,
                     const float *W, int act, const float *out, const float *d_hidden,
                     int64_t dh_bstride, const float *g, const float *cin_w_direct, int pool_from,
                     int64_t B, int m, int H, int N, int D, float *dX0, int accumulate_dx0,
                     float *dXk, int64_t dxk_bstride, float *dW, float *dbias, float *workspace,
                     int64_t workspace_floats, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Wide dense layers on the f32 MFMA (hidden widths > 32: DCN's deep_hidden_units (400, 400),
 * DCN.py:33; and the matrix form of the cross layer).  Replaces tf.matmul(x, W) + bias +
 * activation of DNN.__call__ (layers.py:594-602) and the GEMMs of its gradient, with the
 * dense-input piece, bias, activation and activation gradient fused (csrc/gemm.hip).
 *
 * rm_dense_fwd:  C[M,N] = epilogue( [A1 | A2][M, K1+K2] . op(W) )
 *   A1 [M,K1] (float4 loads when its rows are 16-byte aligned: lda1 % 4 == 0; per-element loads
 *   otherwise), A2 [M,K2] or NULL (the 13 dense inputs);
 *   W row-major: [K,N] (w_transposed = 0) or [N,K] (w_transposed = 1, i.e. op(W) = W^T);
 *   epilogue (acc = the GEMM result, b = bias[col] or 0 when bias is NULL):
 *     RM_DENSE_BIAS_ACT     C = act(acc + b)
 *     RM_DENSE_MUL_ACTGRAD  C = (acc + b) * act'(.) taken from the POST-activation values aux1
 *     RM_DENSE_ADD          C = acc + b (+ aux1 when not NULL)
 *     RM_DENSE_CROSS        u = acc + b ; C = aux1 * u + aux2 ; C2 = u when not NULL
 *                           (x_{l+1} = x0 o (W x_l + b) + x_l with aux1 = x0, aux2 = x_l)
 *   filter_ws: rm_dense_filter_workspace(K1+K2, N) floats (the weights re-laid for the kernel).
 * rm_dense_wgrad: dW[K1+K2, N] (+)= [A1 | A2]^T . G[M,N]  (reduction over the batch, split
 *   into slabs + a deterministic second-stage sum); db [N] (NULL ok) = the column sums of G, i.e. the
 *   bias gradient of the same layer, from the G tiles the kernel stages anyway;
 *   workspace: rm_dense_wgrad_workspace floats.
 * Padding (these four entry points): a row stride may exceed the row's width (lda1 > K1, ldc > N, ld_aux1 > N,
 *   ldg > N, lddw > N ...).  The columns between the width and the stride are NEVER read and never written - they
 *   may hold NaN or another tensor's data.  Loads that reach past a row's end (a float4 over a ragged K1, a tile
 *   over a ragged N) select, they do not multiply by zero.  rm_dense_fwd6's last slab of a ragged K re-reads
 *   columns [K - 32, K) of A1 itself, inside the row, against zeroed weights: no pad column either.  Workspaces are
 *   written before they are read and never beyond the size their *_workspace() function reports
 *   (tests/test_gpu_dense.py runs with NaN pads, NaN-filled workspaces and guard bands). */
enum { RM_DENSE_BIAS_ACT = 0, RM_DENSE_MUL_ACTGRAD = 1, RM_DENSE_ADD = 2, RM_DENSE_CROSS = 3 };
int64_t rm_dense_filter_workspace(int K, int N);
int rm_dense_fwd(const float *A1, int64_t lda1, int K1, const float *A2, int64_t lda2, int K2,
                 const float *W, int64_t ldw, int w_transposed, int N, const float *bias, int epilogue,
                 int act, const float *aux1, int64_t ld_aux1, const float *aux2, int64_t ld_aux2,
                 int64_t M, float *C, int64_t ldc, float *C2, int64_t ldc2, float *filter_ws,
                 rm_stream_t stream);
/* rm_dense_fwd6: rm_dense_fwd's GEMM with every fp32 operand SPLIT into three bf16 pieces (x = h + m + l, 8 + 8 + 8
 * significant bits) and six of the nine piece products formed on the bf16 matrix pipe, fp32 accumulate
 * (csrc/gemm6.hip): the kept products are exact in fp32, the dropped ones are below 3 * 2^-24 of |x y| - the
 * result carries fp32-level error (measured against float64 it is SMALLER than the f32-MFMA kernel's, whose
 * k-chunked sums are longer chains).  gfx950 has no tf32; its f32 MFMA runs at 1/16 of the bf16 rate.
 * Arguments as rm_dense_fwd; epilogues RM_DENSE_BIAS_ACT / MUL_ACTGRAD / ADD; A1 rows 16-byte aligned (lda1 % 4 ==
 * 0); K1 % 32 + K2 <= 32 (the ragged end of [A1 | A2] is copied into one padded slab), otherwise
 * RM_EUNSUPPORTED.  dot_w [N] + dot_out [M] (or both NULL; dot_w0 [1] or NULL): also dot_out[b] = C[b, :] . dot_w
 * + dot_w0 from the epilogue's registers - the [*, 1] output projection of the DNN (rm_rowdot) without another
 * pass over C; fixed summation order.  workspace: rm_dense6_workspace(K, N, M) floats, 16-byte aligned. */
int64_t rm_dense6_workspace(int K, int N, int64_t M);
/* rm_dense_wgrad6: rm_dense_wgrad (dW[K,N] (+)= [A1 | A2]^T . G, db[N] = column sums of G or NULL) on the same
 * scheme: both activations split into bf16 pieces on the fly, once per block and 32-row slab, through transposed
 * LDS planes; partial tiles per batch split in the workspace, added in split order (deterministic).  Any K / N /
 * strides.  G2 [M, N2] + dW2 [K, N2] (or NULL / 0): a second piece of gradient columns against the SAME activations in
 * the same pass (DCN: the cross net's coefficient columns beside the first dense layer's dA - x0 read once).
 * workspace: rm_dense_wgrad6_workspace(K, N + N2, M) floats, 16-byte aligned. */
int64_t rm_dense_wgrad6_workspace(int K, int N, int64_t M);
int rm_dense_wgrad6(const float *A1, int64_t lda1, int K1, const float *A2, int64_t lda2, int K2, const float *G,
                    int64_t ldg, int N, const float *G2, int64_t ldg2, int N2, int64_t M, float *dW, int64_t lddw,
                    float *dW2, int64_t lddw2, int accumulate, float *db, float *workspace,
                    int64_t workspace_floats, rm_stream_t stream);
int rm_dense_fwd6(const float *A1, int64_t lda1, int K1, const float *A2, int64_t lda2, int K2, const float *W,
                  int64_t ldw, int w_transposed, int N, const float *bias, int epilogue, int act,
                  const float *aux1, int64_t ld_aux1, int64_t M, float *C, int64_t ldc, const float *dot_w,
                  const float *dot_w0, float *dot_out, float *workspace, rm_stream_t stream);

int64_t rm_dense_wgrad_workspace(int K, int N, int64_t M);
int rm_dense_wgrad(const float *A1, int64_t lda1, int K1, const float *A2, int64_t lda2, int K2,
                   const float *G, int64_t ldg, int N, int64_t M, float *dW, int64_t lddw,
                   int accumulate, float *db, float *workspace, int64_t workspace_floats,
                   rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Multi-valued tag-list features (MultiValCsvFeat, inputs.py:380-425): the sqrtn-pooled
 * lookup tf.nn.embedding_lookup_sparse(..., combiner="sqrtn") of layers.py:144-169 and the
 * multi-hot linear input of utils.py:86-108.  CSR input: example b owns tag ids
 * ids[offsets[b] .. offsets[b+1]) (0 = unknown tag).  rm_pool_rows writes one pooled FUSED
 * row per example: out[b, 0..D) = sum emb / sqrt(n), out[b, D] = sum bias / sqrt(n),
 * out[b, D+1] = sum over known tags (id >= 1) of the linear weight; the gather kernel then
 * reads that row like any other.  rm_pool_rows_bwd scatters a row gradient (d_rows rows of
 * dr_stride floats, g_bias / g_lin [B] or NULL) back to the tag rows of dense gradient
 * buffers d_table [R,D], d_bias [R], d_lin [R] (float atomics; NULL = skip).
 *
 * vals (float [nnz] or NULL): per-id weights.  With vals the pair implements the
 * value-weighted lookup of SparseValueFeat (inputs.py:213-278; `feat_embeds * value`,
 * layers.py:129-142; `one_hot * value`, utils.py:70-71): out[b, 0..D) = sum v*emb,
 * out[b, D] = sum bias (NOT scaled, as layers.py:136-140), out[b, D+1] = sum v*lin; no sqrtn
 * factor and slot 0 is kept.  A SparseValueFeat is the CSR with one id per example. */
int rm_pool_rows(const float *rows, int64_t row0, int LD, int D, const int64_t *offsets,
                 const int64_t *ids, const float *vals, int64_t B, float *out, rm_stream_t stream);
int rm_pool_rows_bwd(const float *d_rows, int64_t dr_stride, const float *g_bias, const float *g_lin,
                     int D, const int64_t *offsets, const int64_t *ids, const float *vals, int64_t B,
                     int64_t row0, float *d_table, float *d_bias, float *d_lin, rm_stream_t stream);
/* The same pooling in PADDED form, for the row-sharded table's fixed-capacity exchange (recman_amd/dist.py): the
 * tags of a feature are T columns of the occurrence matrix - ids[b * ids_ld + t], -1 = no tag - and the row of tag
 * (b, t) is rows[pos[b * pos_ld + t]] (a position among the rows received from their owners; rows are LD floats).
 * vals[b * vals_ld + t] or NULL as above.  rm_pool_rows_padded writes the pooled rows out [B, LD] (same sums,
 * same order as rm_pool_rows); rm_pack_pooled_grad_rows writes each tag's gradient row
 * [d_rows[b] * we | g_bias[b] * wb | g_lin[b] * wl | 0 ..] (width floats; the factors of rm_pool_rows_bwd) at
 * out[pos[b, t]]: the send buffer of the backward all_to_all, every tag its own slot, no atomics. */
int rm_pool_rows_padded(const float *rows, int LD, int D, const int64_t *pos, int64_t pos_ld, const int64_t *ids,
                        int64_t ids_ld, const float *vals, int64_t vals_ld, int64_t B, int T, float *out,
                        rm_stream_t stream);
int rm_pack_pooled_grad_rows(const float *d_rows, int64_t dr_stride, const float *g_bias, const float *g_lin,
                             int D, const int64_t *pos, int64_t pos_ld, const int64_t *ids, int64_t ids_ld,
                             const float *vals, int64_t vals_ld, int64_t B, int T, int width, float *out,
                             rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Optimizer steps.  Replace optimizer.minimize(...) of xDeepFM.py:121-126 / create_optimizer
 * (utils.py:201-213): Keras Adam (kind 0: beta1/beta2, epsilon outside the sqrt), Adagrad (kind 1,
 * accumulator starts at 0.1) or SGD (kind 2).  reset != 0 ignores the stored moments (the reference
 * builds a new optimizer for every batch) AND the step number: the update is a new optimizer's first step (Adam
 * bias correction at t = 1, whatever `step` says); otherwise step >= 1 is the Adam bias-correction step.
 *
 * rm_sparse_optimizer_step: ROW-WISE and LAZY step on table rows, straight from the IndexedSlices
 * form the backward produces (LazyAdam - Keras' sparse Adam decays the moments of EVERY row; the two
 * coincide under `reset` and when every row is touched each step; see csrc/optim.hip).  Only rows
 * occurring in idx are touched; duplicate occurrences are summed in occurrence order (a stable sort,
 * no float atomics: bit-reproducible).  Occurrences with idx < 0 are skipped.
 *   rows [R, ld]: parameter rows [D embedding | bias | lin | m_bias | m_lin | v_bias | v_lin | pad pad ..],
 *                 ld >= D + 8, ld % 4 == 0 (the four moment entries live in the row's padding), 8 <= D <= 64
 *   mom  [R, 2D]: moments of the embedding entries, interleaved per float4 slice
 *                 [m[0:4] v[0:4] | m[4:8] v[4:8] | ..] (Adagrad uses the v halves; SGD: may be NULL)
 *   d_rows [B,F,D], g_bias / g_lin [B] (per-example gradient of column D / D+1, or NULL),
 *   lin_field_mask [F] or NULL (linear_features subsets)
 *   l2_embedding / l2_linear: LAZY l2 (0 = none) - the gradient of FeatEmbedding.l2 / LinearLayer.l2
 *                 (reg * 1/2 |.|^2, layers.py:188-193, 349-354) is added as reg * row (resp. reg * linear entry)
 *                 for the rows this batch touches, once per distinct row and step, inside the same pass (one FMA
 *                 per element, no extra traffic).  The reference's dense term touches EVERY row every step (the
 *                 whole table, 1.7 - 25.6 GB at the BASELINE configs): the two coincide when every row is touched
 *                 each step; DESIGN.md section 6.
 *   workspace: rm_sparse_optimizer_workspace(B * F) BYTES.
 *   max_field_rows: 0, or a promise that lets the sort work per field: field f owns the rows
 *                 [field_off[f], field_off[f+1]) (the last one up to R), ascending and disjoint, none with more
 *                 than max_field_rows rows, F <= 64.  The ids are then sorted as F independent lists of B keys of
 *                 log2(max_field_rows) bits (csrc/optim.hip, "field-segmented sort": 2 passes for < 2^20 rows per
 *                 field instead of 4 over log2(R) bits); an id beyond its own field's rows is skipped like a
 *                 negative one.  0: one sort of all B * F (row, occurrence) pairs, any field_off.
 * rm_sparse_optimizer_prepare: the id-only part of a step (keys + stable sort by table row) on its own,
 *   so that it can be issued before / beside the forward+backward pass; the following step call on the
 *   same ids passes prepared = 1 and the same workspace (ids: idx [n/F, F] + field_off, or row_ids [n]).
 * rm_sparse_optimizer_step_rows: the same step from gradient rows that already carry their table row
 *   (the row-sharded table's owner side): row_ids [n] (< 0: skip), grad_rows [n, gw] with columns
 *   [0, D) embedding gradient, D bias gradient, D+1 linear gradient.
 * rm_dense_optimizer_step: the same update rule on a flat parameter buffer (dense parameters). */
int64_t rm_sparse_optimizer_workspace(int64_t n);
int rm_sparse_optimizer_prepare(const int64_t *idx, const int64_t *field_off, const int64_t *row_ids,
                                int64_t n, int F, int64_t R, int64_t max_field_rows, void *workspace,
                                int64_t ws_bytes, rm_stream_t stream);
int rm_sparse_optimizer_step(const int64_t *idx, const int64_t *field_off, const float *d_rows,
                             const float *g_bias, const float *g_lin, int64_t B, int F, int D,
                             int64_t R, float *rows, int64_t ld, float *mom, int step, int kind,
                             float lr, float beta1, float beta2, float eps, int reset, float l2_embedding,
                             float l2_linear, const float *lin_field_mask, int64_t max_field_rows, int prepared,
                             void *workspace, int64_t ws_bytes, rm_stream_t stream);
int rm_sparse_optimizer_step_rows(const int64_t *row_ids, const float *grad_rows, int64_t gw, int64_t n,
                                  int D, int64_t R, float *rows, int64_t ld, float *mom, int step, int kind,
                                  float lr, float beta1, float beta2, float eps, int reset, float l2_embedding,
                                  float l2_linear, int prepared, void *workspace, int64_t ws_bytes,
                                  rm_stream_t stream);
int rm_dense_optimizer_step(float *p, const float *g, float *m, float *v, int64_t n, int step, int kind,
                            float lr, float beta1, float beta2, float eps, int reset, rm_stream_t stream);

/* The same steps with the update rule(s) given explicitly, and FTRL-Proximal (kind 3) beside Adam, Adagrad and SGD.
 * A rule descriptor is read on the host at call time.  Field by kind ("-": ignored):
 *            kind  lr                   beta1  beta2  eps                 l1   l2   beta
 *   Adam     0     learning rate        yes    yes    outside the sqrt    -    -    -
 *   Adagrad  1     learning rate        -      -      outside the sqrt    -    -    -
 *   SGD      2     learning rate        -      -      -                   -    -    -
 *   FTRL     3     learning rate, > 0   -      -      -                   L1   L2   beta
 * l1, l2 and beta must be >= 0 whatever the kind (leave them 0 for kinds 0 - 2).
 * FTRL is tf.keras.optimizers.Ftrl with learning_rate_power = -0.5, initial accumulator 0.1 and no l2_shrinkage;
 * per element, in float32, every operation rounded on its own:
 *   n_new = n + g*g;  sigma = (sqrt(n_new) - sqrt(n)) / lr;  z = z + g - sigma * p;
 *   q = (sqrt(n_new) + beta) / lr + 2*l2;  p = |z| > l1 ? (copysign(l1, z) - z) / q : 0;  n = n_new
 * with g the summed gradient after the lazy l2 term, and `reset` setting z = 0, n = 0.1 first.  State: z ("linear"
 * in TF) lives in the m slot and n (the accumulator) in the v slot - of mom's interleaved row, of the row's state
 * columns [m_b m_l v_b v_l], of the dense step's m / v arrays.  Keras applies FTRL to IndexedSlices row by row, so
 * the lazy row-wise step is Keras's own semantics for this kind.
 *
 * rm_sparse_optimizer_step_rules / rm_sparse_optimizer_step_rows_rules: emb_rule updates the D embedding entries of
 * a touched row (state: mom, which must be non-NULL unless emb_rule is SGD, and is not touched when it is), side_rule
 * its bias and linear entries (state: the row's columns D+2 .. D+5; a rule changes only the columns it keeps: SGD none,
 * Adagrad v_b v_l).  Both rules see the same `step` and `reset`.  With emb_rule == side_rule of kind 0 - 2 the result
 * is that of rm_sparse_optimizer_step / _step_rows, which run the same code.  Every other argument as above.
 * rm_dense_optimizer_step_rule: one rule on a flat buffer; m is needed for Adam and FTRL (z), v unless SGD (FTRL: n).
 * An invalid rule (kind outside 0..3, negative l1 / l2 / beta, FTRL with lr <= 0, a missing state array) returns
 * RM_EINVAL before anything is launched. */
typedef struct rm_opt_rule {
  int kind;
  float lr;
  float beta1, beta2;
  float eps;
  float l1, l2, beta;
} rm_opt_rule;
int rm_sparse_optimizer_step_rules(const int64_t *idx, const int64_t *field_off, const float *d_rows,
                                   const float *g_bias, const float *g_lin, int64_t B, int F, int D, int64_t R,
                                   float *rows, int64_t ld, float *mom, int step, const rm_opt_rule *emb_rule,
                                   const rm_opt_rule *side_rule, int reset, float l2_embedding, float l2_linear,
                                   const float *lin_field_mask, int64_t max_field_rows, int prepared,
                                   void *workspace, int64_t ws_bytes, rm_stream_t stream);
int rm_sparse_optimizer_step_rows_rules(const int64_t *row_ids, const float *grad_rows, int64_t gw, int64_t n, int D,
                                        int64_t R, float *rows, int64_t ld, float *mom, int step,
                                        const rm_opt_rule *emb_rule, const rm_opt_rule *side_rule, int reset,
                                        float l2_embedding, float l2_linear, int prepared, void *workspace,
                                        int64_t ws_bytes, rm_stream_t stream);
int rm_dense_optimizer_step_rule(float *p, const float *g, float *m, float *v, int64_t n, int step,
                                 const rm_opt_rule *rule, int reset, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Row helpers (owner-side gather and re-ordering for the row-sharded table).
 */
/* Buckets the n = B*F occurrences (b,f) by the owner rank of their global row
 * g = field_off[f] + idx[b,f] (owner g % world, local row g / world) - a deterministic
 * counting sort:  pos[o] = position of occurrence o in the bucketed order,
 * send_ids[pos[o]] = g / world, counts[w] = occurrences owned by rank w.  An EMPTY occurrence (idx < 0: the
 * padding of a multi-valued feature's tag columns, see rm_pool_rows_padded) takes no slot: pos[o] = -1, counted
 * nowhere.  workspace: rm_shard_route_workspace(world) int32 words.  world <= 16. */
int64_t rm_shard_route_workspace(int world);
int rm_shard_route(const int64_t *idx, const int64_t *field_off, int64_t B, int F, int world,
                   int64_t *pos, int64_t *send_ids, int64_t *counts, int32_t *workspace,
                   rm_stream_t stream);
/* Fixed-capacity variant: bucket w occupies slots [w*cap, (w+1)*cap) of pos / send_ids
 * (send_ids has world*cap entries; unused slots hold -1, which rm_gather_rows answers with a
 * zero row).  Every rank then exchanges equal splits: no count exchange, no host sync, and the
 * whole step can be captured in one hipGraph.  A bucket that needs more than cap slots sets
 * *overflow = 1 (sticky; the caller clears it) and the step's result must be discarded. */
int rm_shard_route_padded(const int64_t *idx, const int64_t *field_off, int64_t B, int F, int world,
                          int64_t cap, int64_t *pos, int64_t *send_ids, int64_t *counts,
                          int32_t *overflow, int32_t *workspace, rm_stream_t stream);

/* out[pos[o], :] = [d_rows[o, 0..D) | g_bias[b] | g_lin[b] * lin_field_mask[f] | 0 ..] (width floats per
 * row): the per-occurrence gradient rows of the fused table rows, written straight in bucketed order
 * (the send buffer of the backward all_to_all).  g_bias / g_lin [B] may be NULL (0); lin_field_mask
 * [F] or NULL: the linear_features subset (get_linear_features, utils.py:27-30). */
int rm_pack_grad_rows(const float *d_rows, const float *g_bias, const float *g_lin,
                      const float *lin_field_mask, const int64_t *pos, int64_t B, int F, int D, int width,
                      float *out, rm_stream_t stream);

/* rows_out[i, 0..width) = table[rows[i], 0..width) for i < n (owner-side gather of the requested
 * local rows; table rows are table_ld floats apart - the shard keeps optimizer state behind the
 * exchanged columns -, width % 4 == 0, table_ld % 4 == 0); rows[i] < 0 gives a zero row. */
int rm_gather_rows(const float *table, int64_t table_ld, const int64_t *rows, int64_t n, int width,
                   float *rows_out, rm_stream_t stream);

/* dst[i,:] = src[slot[i],:] (un-route: received rows back into (b,f) order) when
 * inverse == 0;  dst[slot[i],:] = src[i,:] when inverse != 0 (route gradient rows). */
int rm_permute_rows(const float *src, const int64_t *slot, int64_t n, int width, int inverse,
                    float *dst, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Evaluation metrics of a prediction vector (csrc/metrics.hip): what fit() / evaluate() score with.
 * Replaces recman/metrics/roc_auc.py:4-16 and recman/metrics/logloss.py:4-19 (sklearn's roc_auc_score /
 * log_loss on the host) and the scoring of DeepModel.py:72-74,92-131.
 *
 *   scores / pred [n]  fp32 (any finite value for the AUC; probabilities for the log loss)
 *   labels [n]         int64 0 / 1;   1 <= n <= 2^31 - 1
 *   workspace          rm_metric_workspace(n) BYTES, 16-byte aligned; one workspace serves both calls
 *   out                ONE device record, read by the host in one copy
 * rm_roc_auc: the exact Mann-Whitney AUC, ties counted one half: 2U in uint64, one division in double.
 * rm_log_loss: -mean(log(clip(p or 1 - p))) with the clip in fp32 at eps (and 1 - eps), log and sum in
 *   fp64 - sklearn 1.7.2's binary log_loss on float32 input when eps = FLT_EPSILON.  0 < eps < 0.5.
 * Both are deterministic (fixed-order reductions, no float atomics).  Invalid inputs do not fail the call:
 * they set bits of out->flags, and the value is then meaningless.  With one class present (pos or neg 0)
 * RM_METRIC_ONE_CLASS is set and the AUC is NaN. */
#define RM_METRIC_BAD_LABEL 1  /* a label outside {0, 1}                  */
#define RM_METRIC_BAD_SCORE 2  /* a NaN or infinite score                  */
#define RM_METRIC_ONE_CLASS 4  /* every label equal                        */
#define RM_METRIC_PROB_RANGE 8 /* rm_log_loss: a probability outside [0, 1] */
typedef struct rm_metric_result {
  double value;
  int64_t pos;   /* P: labels equal to 1 */
  int64_t neg;   /* N = n - P            */
  int64_t flags; /* RM_METRIC_*          */
} rm_metric_result;
int64_t rm_metric_workspace(int64_t n);
int rm_roc_auc(const float *scores, const int64_t *labels, int64_t n, void *workspace, rm_metric_result *out,
               rm_stream_t stream);
int rm_log_loss(const float *pred, const int64_t *labels, int64_t n, float eps, void *workspace,
                rm_metric_result *out, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Grouped AUC, GAUC (csrc/gauc.hip): the AUC inside each group (user), averaged over the groups that hold
 * both classes - the measure of the DIN paper (arXiv 1706.06978, section 6.2).  New: the reference has none.
 *
 *   scores [n] fp32 finite, labels [n] int64 0 / 1, groups [n] int64 with 0 <= id < 2^32;  1 <= n <= 2^31 - 1
 *   weight_kind        0: w_g = n_g (impressions, the paper)   1: w_g = P_g (clicks)
 *   workspace          rm_group_auc_workspace(n) BYTES, 16-byte aligned
 *   group_ids / group_n / group_pos / group_2u [n] each, or all NULL: per group, in ascending id order, its id,
 *                      examples n_g, positives P_g and 2U_g (the Mann-Whitney count inside the group, ties one
 *                      half; equal scores in different groups never tie).  Only the first out->groups entries
 *                      are written.
 *   out                ONE device record, read by the host in one copy
 * GAUC = sum_g w_g AUC_g / sum_g w_g over the scored groups (P_g > 0 and N_g > 0), AUC_g = 2U_g / (2 P_g N_g).
 * Every per-group integer is exact; the mean is double, summed in ascending id order by a fixed tree (no float
 * atomics): bitwise reproducible and independent of the order of the input.  With no scored group the value is
 * NaN and RM_METRIC_ONE_CLASS is set.  Invalid inputs set bits of out->flags as rm_roc_auc does. */
#define RM_METRIC_BAD_GROUP 16 /* rm_group_auc: a group id outside [0, 2^32) */
typedef struct rm_group_auc_result {
  double value;          /* GAUC, NaN when no group is scored */
  int64_t groups;        /* distinct group ids                */
  int64_t scored_groups; /* those with both classes           */
  int64_t weight;        /* sum of w_g over the scored groups */
  int64_t pos;           /* P over all examples               */
  int64_t flags;         /* RM_METRIC_*                       */
} rm_group_auc_result;
int64_t rm_group_auc_workspace(int64_t n);
int rm_group_auc(const float *scores, const int64_t *labels, const int64_t *groups, int64_t n, int weight_kind,
                 void *workspace, int64_t *group_ids, int64_t *group_n, int64_t *group_pos, uint64_t *group_2u,
                 rm_group_auc_result *out, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Multi-task learning: the gate-softmax + expert mixture of MMoE (Multi-gate Mixture-of-Experts, Ma et al., KDD
 * 2018) for all tasks in one pass, and the loss head for several labels (csrc/multitask.hip).  Nothing in the reference
 * implements them: it knows one label per example (DeepModel.py:31-34).  Per example, E experts of width H, T tasks:
 *     p_t = softmax_e(A_t), max-subtracted;   M_t = sum_e p_te Z_e
 *   Z [B, ldz] (E H columns used, expert e at columns e H ..), A [B, lda] (T E columns, task t at t E ..),
 *   M [B, ldm] (T H columns written, task t at t H ..), P [B, ldp] or NULL (T E columns written: the gate weights,
 *   for inspection at inference).  Every operand is a pointer and a row stride in floats: a column range of a wider
 *   buffer works; pointers 16-byte aligned, strides multiples of 4 floats and >= the width; columns past the width
 *   are never read or written.
 * rm_mmoe_mix_fwd replaces what a composition of softmax, T E scaled adds and T stores of p would move: Z and A are
 *   read once, M is written once, p reaches HBM only when P is given (M has the same bits either way).
 * rm_mmoe_mix_bwd, given dM = dLoss/dM, recomputes p and writes dZ [B, lddz] and dA [B, ldda] once (own columns only):
 *     dZ_e = sum_t p_te dM_t;   c_te = <dM_t, Z_e>;   dA_te = p_te (c_te - sum_e' p_te' c_te')    (exactly 0 at E = 1)
 *   No parameters, so no partial sums; no atomics, no workspace: two runs are bit-equal.
 * Supported (rm_mmoe_mix_supported): 1 <= E <= 16, 1 <= T <= 8, H a multiple of 4 in 4..512; anything else, a NULL
 *   or unaligned pointer, or a stride that is below its width or no multiple of 4 is RM_EINVAL before any launch,
 *   the limits named in the message.  B = 0 is RM_OK.
 * rm_mmoe_mix_tile: RM_MMOE_TILE the examples a block owns per tile (backward != 0: of rm_mmoe_mix_bwd),
 *   RM_MMOE_CAP the cap of both grids: a block walks the batch again from B > cap * tile on.  -1 when unsupported.
 */
#define RM_MMOE_TILE 0
#define RM_MMOE_CAP 1
int rm_mmoe_mix_supported(int E, int T, int H);
int rm_mmoe_mix_tile(int E, int T, int H, int backward, int which);
int rm_mmoe_mix_fwd(const float *Z, int64_t ldz, const float *A, int64_t lda, int64_t B, int E, int T, int H,
                    float *M, int64_t ldm, float *P, int64_t ldp, rm_stream_t stream);
int rm_mmoe_mix_bwd(const float *Z, int64_t ldz, const float *A, int64_t lda, const float *dM, int64_t lddm,
                    int64_t B, int E, int T, int H, float *dZ, int64_t lddz, float *dA, int64_t ldda,
                    rm_stream_t stream);

/* The loss head for T labels per example: rm_logit_loss's arithmetic per task (PredictionLayer + create_loss,
 * layers.py:796-808, utils.py:192-198: Keras binary_crossentropy on clipped probabilities, or MSE), over the
 * examples whose label is OBSERVED - NaN in Y means unobserved (CVR is defined on clicks only).
 *   logit [T, B];  Y [B, T] fp32, NaN = unobserved;  task_type [T] HOST ints (0 classification, 1 regression);
 *   task_weight [T] HOST floats;  1 <= T <= 8, B >= 1
 *   pred   [T, B]  sigmoid(logit) or logit; written for unobserved labels too
 *   dlogit [T, B]  w_t dl_t/dlogit / n_t * grad_scale where the label is observed, +0.0 elsewhere
 *   n_t    [T] int64, the observed labels per task;  loss_t [T] the mean of l_t over them (0 when n_t = 0)
 *   loss   [1]  sum_t w_t loss_t
 * A task with no observed label contributes loss 0 and a zero gradient.  Counts and sums are two-stage reductions
 * in double in a fixed order, no float atomics: two runs are bit-equal.  With Y, dlogit, n_t, loss_t and loss all
 * NULL only pred is written (inference).  workspace: rm_multitask_loss_workspace(B, T) floats, 16-byte aligned
 * (-1: unsupported T). */
int64_t rm_multitask_loss_workspace(int64_t B, int T);
int rm_multitask_loss(const float *logit, const float *Y, const int *task_type, const float *task_weight,
                      float grad_scale, int64_t B, int T, float *pred, float *dlogit, int64_t *n_t, float *loss_t,
                      float *loss, float *workspace, rm_stream_t stream);

/* ------------------------------------------------------------------------
 * Two-tower retrieval: the in-batch softmax loss over the scores of every user row against every item row of the
 * batch (DSSM / YouTube-DNN; the logQ correction of Yi et al., RecSys 2019), forward and backward, and the row
 * normalisation of the tower outputs (csrc/inbatch.hip).  Nothing in the reference implements them: every model of
 * it scores one (user, item) row.  U and V are [B, H] float32, each a pointer and a row stride in floats: a column
 * range of a wider buffer works; pointers 16-byte aligned, strides multiples of 4 floats and >= H; columns outside
 * the range are never read or written.
 *     S_ij    = scale <U_i, V_j> - logq_j                  (logq NULL: 0; applied to the diagonal too)
 *     allowed = (j == i) or item_id NULL or item_id_j != item_id_i       (accidental hits are masked out)
 *     lse_i   = log sum_{j allowed} exp(S_ij)              (max-subtracted, online over the column tiles)
 *     l_i     = lse_i - S_ii = row_loss_i
 *     W       = sum_i w_i (w NULL: all 1; w_i >= 0);   loss = sum_i w_i l_i / W   (W == 0: loss 0)
 *     rank_i  = #{ j allowed, j != i : S_ij > S_ii }       (int32, on the kernel's own float32 S; may be NULL)
 *   backward: P_ij = exp(S_ij - lse_i) for allowed j, else 0;  G_ij = grad_scale w_i / W (P_ij - [i == j])
 *     dU_i = scale sum_j G_ij V_j;   dV_j = scale sum_i G_ij U_i          (W == 0: both exactly 0)
 * S, P and G [B, B] never reach HBM: the products run on the exact-f32 MFMA from tiles in LDS, the backward
 *   recomputes S from U, V and the saved lse.  dU is owned by row tiles, dV by column tiles.  No float atomics; loss
 *   and W are fixed-order two-stage sums in double.
 * col_splits: 0 = the library's choice, 1..RM_IBS_MAX_SPLITS forces it: that many blocks share a row tile's columns
 *   (a small batch has few row tiles).  The splits' partial (max, sum, rank) triples, and the backward's partial
 *   sums, are combined in split order: two runs with the same col_splits are bit-equal.  A split count above the
 *   number of column tiles is valid (the extra splits are empty).
 * rm_inbatch_softmax_tile: RM_IBS_ROWS the rows a block owns, RM_IBS_COLS the rows of a streamed tile,
 *   RM_IBS_MAX_SPLITS; -1 when H is unsupported.  workspace: rm_inbatch_softmax_workspace(B, H) floats, 16-byte
 *   aligned; it covers the largest split count (-1: unsupported).
 * Supported (rm_inbatch_softmax_supported): H a multiple of 4 in 4..256.  An unsupported H, a NULL or unaligned
 *   pointer, a stride below H or no multiple of 4, a split count out of range: RM_EINVAL before any launch, the
 *   limit named in the message.  B = 0 is RM_OK.
 * rm_rownorm_fwd: Y = X / max(|X|_2, eps), inv_norm [B] = 1 / max(|X|_2, eps).  rm_rownorm_bwd: dX = inv_norm
 *   (dY - Y <Y, dY>); dX may alias dY.  Operands and limits as above.
 */
#define RM_IBS_ROWS 0
#define RM_IBS_COLS 1
#define RM_IBS_MAX_SPLITS 2
int rm_inbatch_softmax_supported(int H);
int rm_inbatch_softmax_tile(int H, int which);
int64_t rm_inbatch_softmax_workspace(int64_t B, int H);
int rm_inbatch_softmax_fwd(const float *U, int64_t ldu, const float *V, int64_t ldv, const int64_t *item_id,
                           const float *logq, const float *w, float scale, int64_t B, int H, int col_splits,
                           float *lse, float *row_loss, int32_t *rank, float *loss, float *workspace,
                           rm_stream_t stream);
int rm_inbatch_softmax_bwd(const float *U, int64_t ldu, const float *V, int64_t ldv, const int64_t *item_id,
                           const float *logq, const float *w, float scale, float grad_scale, int64_t B, int H,
                           int col_splits, const float *lse, float *dU, int64_t lddu, float *dV, int64_t lddv,
                           float *workspace, rm_stream_t stream);
int rm_rownorm_fwd(const float *X, int64_t ldx, int64_t B, int H, float eps, float *Y, int64_t ldy, float *inv_norm,
                   rm_stream_t stream);
int rm_rownorm_bwd(const float *Y, int64_t ldy, const float *inv_norm, const float *dY, int64_t lddy, int64_t B,
                   int H, float *dX, int64_t lddx, rm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECMAN_HIP_H */
