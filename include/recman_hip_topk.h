/*
 * recman_hip_topk.h - C ABI of librecman_hip.so, continued: exact top-k retrieval by inner product over an item
 * catalogue (csrc/topk.hip).  The conventions of recman_hip.h hold: device pointers, kernels enqueued on `stream`,
 * RM_OK or a negative RM_E* code with rm_last_error() for the message.  Nothing in the reference implements it.
 *
 * Q [Nq, H] (the queries, e.g. user embeddings) and C [N, H] (the catalogue, e.g. item embeddings) are float32, each a
 * pointer and a row stride in floats: a column range of a wider buffer works; columns outside it are never read.
 *     s_ij = fl(scale * dot_ij),  dot_ij = <Q_i, C_j> accumulated in fp32 over H in a fixed k-step order on the
 *            exact-f32 MFMA: a pair's score does not depend on the block, tile or split that computes it, and the
 *            returned scores are bit-equal to the values that were compared.
 * Order: by score descending, then by catalogue row ascending; -0.0 == +0.0; a NaN score ranks below every number
 *   and NaN scores are ordered by row among themselves.  This is a total order: the result is unique and
 *   bit-identical for every item_splits and on every run.  A returned NaN score is the quiet NaN 0x7fc00000, a
 *   returned zero is +0.0.
 * Output: row i of out_rows (int64) / out_scores (float32), row stride ldo >= k, holds the best min(k, available)
 *   catalogue rows of query i, sorted; the slots past them hold row -1 and score -inf.  Columns >= k are not written.
 * Exclusions: excl_offsets [Nq + 1] / excl_rows [excl_offsets[Nq]] (both NULL: none) are a CSR over the queries: the
 *   catalogue rows query i must never get back.  Each query's list must be ascending (an unsorted list gives a wrong
 *   result, never an out-of-bounds access); rows outside [0, N) are ignored, duplicates are allowed.  available = N
 *   minus the distinct excluded rows in [0, N).
 * item_splits: 0 = the library's choice, 1..rm_topk_ip_tile(H, RM_TOPK_MAX_SPLITS) forces it: that many blocks
 *   share a query tile's catalogue, each a contiguous range of tiles (a split count above the number of catalogue
 *   tiles is valid; it is clamped).  Stage 1 keeps, per (query, split), a list of candidates in the workspace that
 *   beat the split's running k-th best; stage 2 merges the splits' sorted lists in split order.
 * rm_topk_ip_tile: RM_TOPK_ROWS the query rows a block owns, RM_TOPK_COLS the catalogue rows of a streamed tile,
 *   RM_TOPK_MAX_SPLITS the largest item_splits; -1 when H is unsupported.
 * workspace: rm_topk_ip_workspace(Nq, N, H, k) FLOATS, 16-byte aligned; it covers every split count (-1:
 *   unsupported H or k, or a negative size).
 * Limits (rm_topk_ip_supported(H, k)): H a multiple of 4 in 4..256, k in 1..1024; 0 <= Nq < 2^30 and
 *   0 <= N <= 2^31 - 1; pointers 16-byte aligned; ldq and ldc multiples of 4, >= H (and <= 2^24); ldo >= k;
 *   item_splits 0..max.  A violation is RM_EINVAL before any launch, the limit named in the message.  Nq = 0 is
 *   RM_OK and touches nothing; with N = 0 every slot is padding.
 */
#ifndef RECMAN_HIP_TOPK_H
#define RECMAN_HIP_TOPK_H

#include "recman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RM_TOPK_ROWS 0
#define RM_TOPK_COLS 1
#define RM_TOPK_MAX_SPLITS 2
int rm_topk_ip_supported(int H, int k);
int rm_topk_ip_tile(int H, int which);
int64_t rm_topk_ip_workspace(int64_t Nq, int64_t N, int H, int k);
int rm_topk_ip(const float *Q, int64_t ldq, const float *C, int64_t ldc, int64_t Nq, int64_t N, int H, float scale,
               int k, const int64_t *excl_offsets, const int64_t *excl_rows, int item_splits, int64_t *out_rows,
               float *out_scores, int64_t ldo, void *workspace, rm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECMAN_HIP_TOPK_H */
