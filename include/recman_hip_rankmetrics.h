/*
 * recman_hip_rankmetrics.h - C ABI of librecman_hip.so, continued: grouped top-k ranking metrics of a prediction vector
 * (csrc/rankmetrics.hip): NDCG@k, recall@k and precision@k per group (user, query).  The conventions of recman_hip.h
 * hold: device pointers, kernels enqueued on `stream`, RM_OK or a negative RM_E* code with rm_last_error() for the
 * message.  New: the reference has none.
 *
 * rm_group_gain is an evaluation metric and is never part of a captured training step: like rm_roc_auc and
 * rm_group_auc, the ledger of tests/graph_replay.py files it under NOT_IN_A_STEP.
 *
 *   scores [n] fp32 finite, labels [n] int64 0 / 1, groups [n] int64 with 0 <= id < 2^32, or NULL: all of it is one
 *   group (no id tensor is needed);  1 <= n <= 2^31 - 1
 *   disc [cutoffs[n_cutoffs - 1]]  float64 on the device: the discount of each 0-based rank, non-negative
 *   cutoffs [n_cutoffs]            on the HOST: 1 <= n_cutoffs <= RM_GAIN_MAX_CUTOFFS values k, strictly ascending,
 *                                  1 <= k <= RM_GAIN_MAX_K
 * Inside a group the examples are ordered by score, descending.  Examples of one group with equal scores (-0.0 ==
 * +0.0) form a tie group; equal scores in different groups never tie.  A tie group T takes the ranks [lo, hi) and
 * holds pos_T positives:
 *   gain_g(k)  = sum over T with lo < k of (pos_T / (hi - lo)) * sum_{r = lo}^{min(hi, k) - 1} disc[r]
 *   value_g(k) = gain_g(k) / norm_g(k)
 *   norm RM_GAIN_NORM_IDEAL      sum_{r < min(P_g, k)} disc[r]   (NDCG with binary gains when disc[r] = 1 / log2(r + 2))
 *        RM_GAIN_NORM_POSITIVES  P_g                             (recall when disc = 1)
 *        RM_GAIN_NORM_K          k                               (precision when disc = 1)
 * the expectation of the metric over a uniformly random order inside every tie group - what sklearn's ndcg_score
 * computes with ignore_ties=False, and the counterpart of the AUC's "ties count one half".  A group shorter than k
 * ends early.  A norm of zero (no positive) gives value_g = 0.0.
 *   scored_rule RM_GAIN_SCORED_BOTH_CLASSES  0 < P_g < n_g  (the rule of rm_group_auc and rm_rank_loss)
 *               RM_GAIN_SCORED_HAS_POSITIVE  P_g >= 1
 *   weight_kind RM_GAIN_WEIGHT_GROUPS 1   RM_GAIN_WEIGHT_IMPRESSIONS n_g   RM_GAIN_WEIGHT_CLICKS P_g
 * out->value[c] = sum_g w_g value_g(cutoffs[c]) / sum_g w_g over the scored groups; NaN, with RM_METRIC_ONE_CLASS set,
 * when no group is scored.  Entries past n_cutoffs are NaN.
 *   workspace          rm_group_gain_workspace(n) BYTES, 16-byte aligned; its contents on entry do not matter
 *   group_ids / group_n / group_pos [n] int64 and group_value [n][n_cutoffs] float64, or all four NULL: per group, in
 *                      ascending id order, its id, examples n_g, positives P_g and value_g per cutoff (unscored groups
 *                      too).  Only the first out->groups entries are written.
 *   out                ONE device record, read by the host in one copy
 * How: one stable LSD radix sort by (group id ascending, score descending) - digits that do not vary are skipped - so
 * a group is a contiguous run and a rank is a position minus the group's start; a prefix count of the sorted labels
 * makes pos_T and P_g differences; then one thread per group walks the tie groups of its first min(n_g, kmax)
 * positions (the end of a tie group that runs past them is found by bisection).  Every range sum of disc is formed by
 * adding its entries in rank order, the terms of a group in rank order, the groups in ascending id order by a fixed
 * tree, all in double: value_g(k) is within (3k + 8) 2^-53 relative of the exact rational.  No float atomics; the
 * sorted order is canonical up to the labels inside a tie group, of which only counts are read: two runs are bit-equal
 * and the value does not depend on the order of the input.  Nothing is read back by the host between the kernels.
 * Invalid inputs do not fail the call: they set bits of out->flags as rm_group_auc does (RM_METRIC_BAD_SCORE /
 * _BAD_LABEL / _BAD_GROUP), the value is then meaningless, and every access stays inside the buffers.
 * Limits: n, n_cutoffs and cutoffs as above; norm, scored_rule, weight_kind one of the constants; scores, labels, disc,
 * cutoffs, workspace and out not NULL; workspace and out 16-byte aligned.  A violation is RM_EINVAL before any launch.
 */
#ifndef RECMAN_METRICS_RANK_H
#define RECMAN_METRICS_RANK_H

#include "recman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RM_GAIN_MAX_K 1024
#define RM_GAIN_MAX_CUTOFFS 8
#define RM_GAIN_NORM_IDEAL 0
#define RM_GAIN_NORM_POSITIVES 1
#define RM_GAIN_NORM_K 2
#define RM_GAIN_SCORED_BOTH_CLASSES 0
#define RM_GAIN_SCORED_HAS_POSITIVE 1
#define RM_GAIN_WEIGHT_GROUPS 0
#define RM_GAIN_WEIGHT_IMPRESSIONS 1
#define RM_GAIN_WEIGHT_CLICKS 2

typedef struct rm_group_gain_result {
  double value[RM_GAIN_MAX_CUTOFFS]; /* one per cutoff, NaN when no group is scored */
  int64_t groups;                    /* distinct group ids                          */
  int64_t scored_groups;             /* those the scored rule admits                */
  int64_t weight;                    /* sum of w_g over the scored groups           */
  int64_t pos;                       /* P over all examples                         */
  int64_t flags;                     /* RM_METRIC_*                                 */
} rm_group_gain_result;

int64_t rm_group_gain_workspace(int64_t n);
int rm_group_gain(const float *scores, const int64_t *labels, const int64_t *groups, int64_t n, const double *disc,
                  const int *cutoffs, int n_cutoffs, int norm, int scored_rule, int weight_kind, void *workspace,
                  int64_t *group_ids, int64_t *group_n, int64_t *group_pos, double *group_value,
                  rm_group_gain_result *out, rm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECMAN_METRICS_RANK_H */
