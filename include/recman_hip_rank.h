/*
 * recman_hip_rank.h - C ABI of librecman_hip.so, continued: grouped ranking objectives for the single-logit models
 * (csrc/rank.hip).  The conventions of recman_hip.h hold: device pointers, kernels enqueued on `stream`, RM_OK or a
 * negative RM_E* code with rm_last_error() for the message.  Nothing in the reference implements it: it trains against
 * the pointwise losses only.
 *
 * A second loss term next to the pointwise one (rm_logit_loss), over the examples of ONE batch that share a group id:
 * the RankNet / BPR pair loss ("Joint Optimization of Ranking and Calibration", Sheng et al., 2022) or the ListNet /
 * TF-Ranking softmax loss.
 *   logit  [B] float32  s, the summed logit
 *   y      [B] int64    labels in {0, 1}
 *   groups [B] int64    ids in [0, 2^32), or NULL: the whole batch is one group
 * Per group g: n_g examples, P_g positives, N_g negatives.  A group is SCORED when P_g > 0 and N_g > 0 (the rule of
 * rm_group_auc); only scored groups contribute, to the value and to the gradient.
 *   kind RM_RANK_PAIRWISE   L = sum_g c_g sum_{i in g, y_i = 1} sum_{j in g, y_j = 0} softplus(-(s_i - s_j)),
 *                           softplus(-d) = max(-d, 0) + log1p(exp(-|d|))
 *                           dL/ds_i = -c_g sum_j sigmoid(-(s_i - s_j)) (i positive), dL/ds_j = +c_g sum_i sigmoid(-(s_i - s_j))
 *   kind RM_RANK_LISTWISE   L = sum_g c_g sum_{i in g} y_i (lse_g - s_i), lse_g the max-subtracted log-sum-exp of the group
 *                           dL/ds_i = c_g (P_g softmax_g(s)_i - y_i)
 *   norm RM_RANK_NORM_PAIRS pairwise c_g = 1 / Q, Q = sum_scored P_g N_g;  listwise c_g = 1 / P, P = sum_scored P_g
 *   norm RM_RANK_NORM_GROUP pairwise c_g = n_g / (W P_g N_g);  listwise c_g = n_g / (W P_g);  W = sum_scored n_g
 *                           (the pairwise loss is then the smooth surrogate of 1 - GAUC weighted by impressions)
 * c_g is formed in double from the integer counts and rounded to float once for the gradient.
 * Combination, 0 < alpha <= 1:
 *   dlogit_out[i] = grad_scale ((1 - alpha) dlogit_in[i] + alpha dL/ds_i)   (dlogit_in NULL: grad_scale alpha dL/ds_i)
 *   loss_out[0]   = (1 - alpha) loss_in[0] + alpha L, in double, rounded once   (loss_in NULL: alpha L; loss_out NULL:
 *                   not written)
 *   dlogit_out may be dlogit_in, loss_out may be loss_in.  dL/ds is exactly +0.0 for every example of a group that is
 *   not scored; with no scored group L = 0.
 * out (or NULL): the record, written on the device; nothing is read back by the host.
 *   value = L; groups, scored_groups; pairs = Q; pos = P; weight = W; flags = RM_METRIC_BAD_LABEL (a label outside
 *   {0, 1}), RM_METRIC_BAD_GROUP (an id outside [0, 2^32)), RM_METRIC_BAD_SCORE (a NaN or infinite logit).  Invalid
 *   input does not fail the call: it sets its flag, the outputs are then meaningless, and every write stays inside the
 *   buffers (a bad label counts as 0, a bad id is taken modulo 2^32).
 * How: one stable LSD radix sort by (group id, label) - digits that do not vary are skipped - after which a group is
 *   two contiguous runs, negatives then positives; per-group bounds and counts; then one thread per example.  Pairwise:
 *   the thread walks the opposite-class run of its group, streamed through LDS in tiles of RM_RANK_TILE scores, so every
 *   pair is evaluated twice and no atomic is needed; a tile's terms are summed in float32 and the tiles in double.  The
 *   tiles of a block of 256 positions are dealt to RM_RANK_SPLITS blocks (a few positives against a batch of negatives
 *   would otherwise be a few long threads) whose sums are added in split order.
 *   Listwise: (max, sum-exp) per piece of RM_RANK_PIECE sorted positions of a group, the pieces of a group combined in
 *   position order in double.  Loss and counts are fixed-order two-stage reductions (double / int64).  No float atomics:
 *   two runs are bit-equal.  Nothing of size B^2, Q or groups x max_len exists; the workspace is O(B).
 * workspace: rm_rank_loss_workspace(B) BYTES (0 outside the limits), 16-byte aligned; its contents on entry do not
 *   matter.
 * Limits: 1 <= B <= 2^24; kind, norm as above; 0 < alpha <= 1; grad_scale finite; logit, y, dlogit_out and workspace not
 *   NULL; workspace and out 16-byte aligned.  A violation is RM_EINVAL before any launch, the limit named in the message.
 */
#ifndef RECMAN_HIP_RANK_H
#define RECMAN_HIP_RANK_H

#include "recman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RM_RANK_PAIRWISE 0
#define RM_RANK_LISTWISE 1
#define RM_RANK_NORM_PAIRS 0
#define RM_RANK_NORM_GROUP 1
#define RM_RANK_TILE 256
#define RM_RANK_PIECE 256
#define RM_RANK_SPLITS 16
#define RM_RANK_MAX_B (1 << 24)

typedef struct rm_rank_result {
  double value;          /* L, the ranking term alone                */
  int64_t groups;        /* distinct group ids                       */
  int64_t scored_groups; /* ... with both classes                    */
  int64_t pairs;         /* Q = sum of P_g N_g over the scored groups */
  int64_t pos;           /* P = sum of P_g over the scored groups     */
  int64_t weight;        /* W = sum of n_g over the scored groups     */
  int64_t flags;         /* RM_METRIC_*                               */
} rm_rank_result;

int64_t rm_rank_loss_workspace(int64_t B);
int rm_rank_loss(const float *logit, const int64_t *y, const int64_t *groups, int64_t B, int kind, int norm,
                 float alpha, float grad_scale, const float *dlogit_in, float *dlogit_out, const float *loss_in,
                 float *loss_out, rm_rank_result *out, void *workspace, rm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECMAN_HIP_RANK_H */
