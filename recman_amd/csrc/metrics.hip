// Exact binary ROC AUC and log loss of a prediction vector, on the device: the metrics fit() and
// evaluate() score with.  Replaces recman/metrics/roc_auc.py:4-16 and recman/metrics/logloss.py:4-19
// (sklearn.metrics.roc_auc_score / log_loss on the host, DeepModel.py:72-74,92-131); see recman_hip.h.
//
// ROC AUC (Mann-Whitney): sort the scores, group equal scores, and with [a, b) the sorted positions of a
// positive example's group
//     2U = sum_{positives} (a + b + 1) - P (P + 1),   AUC = 2U / (2 P N)
// (a + b + 1 is twice the 1-based mid-rank of the group).  Every term is an integer: 2U is counted in uint64
// and divided once in double, so the result is exact up to that rounding and does not depend on the order of
// anything.  Kernels, in launch order:
//   auc_keys_kernel       validate, score -> order-preserving uint32 key, label -> byte; P; the four
//                         digit histograms of all keys (one read)
//   radix_sort            (rm_radix_sort.h) the stable LSD radix sort of (key, label) by the four bytes of the
//                         key: its plan kernel, then (hist, scan, pass) per digit
//   auc_groups_kernel     per tile: group starts / ends (neighbour keys across the tile edges), the known
//                         part of sum (a + b + 1) and the positives whose group runs past either edge
//   auc_final_kernel      resolves those edge groups with a prefix max / suffix min over the tiles and
//                         writes the record
// One sort path serves every score: the label rides as a byte beside the key.  A keys-only sort of
// (bits << 1 | label) would save 2 B/element per pass (about 15 %) but holds only for scores >= +0.
// Log loss: logloss_kernel (fp32 clip as sklearn 1.7.2, log and sum in fp64, per-block partials) and
// logloss_final_kernel (fixed-order reduction).  No float atomics anywhere: bitwise reproducible.
#include <math.h>

#include "rm_radix_sort.h"

namespace {

constexpr int kLossBlocks = 1024;

// the sorted record: one column, the score key, with the label byte beside it; digit p is byte p of the key
struct AucRecord {
  static constexpr int kCols = 1;
  static constexpr bool kLabel = true;
  static constexpr int kDigits = 4;
  static __device__ __forceinline__ int column(int) { return 0; }
  static __device__ __forceinline__ unsigned extract(unsigned v, int p) { return (v >> (8 * p)) & 255u; }
};

struct AucHeader {
  unsigned long long pos;               // P
  unsigned flags;                       // RM_METRIC_* of the inputs
  unsigned pad;
  SortPlan<AucRecord::kDigits> plan;
};

struct Layout {
  size_t header, hist, part, head, tail, last, first, keys0, keys1, lab0, lab1, total;
  size_t loss_part, loss_pos, loss_flags, loss_total;
};

Layout layout(int64_t n) {
  const size_t tiles = (size_t)((n + kTile - 1) / kTile), un = (size_t)n;
  Layout L;
  size_t o = 0;
  L.header = take(o, sizeof(AucHeader));
  L.hist = take(o, 4 * kRadix * tiles);
  L.part = take(o, 8 * tiles);
  L.head = take(o, 4 * tiles);
  L.tail = take(o, 4 * tiles);
  L.last = take(o, 4 * tiles);
  L.first = take(o, 4 * tiles);
  L.keys0 = take(o, 4 * un);
  L.keys1 = take(o, 4 * un);
  L.lab0 = take(o, un);
  L.lab1 = take(o, un);
  L.total = o;
  o = 0;  // log loss uses the front of the same workspace
  L.loss_part = take(o, 8 * kLossBlocks);
  L.loss_pos = take(o, 8 * kLossBlocks);
  L.loss_flags = take(o, 4 * kLossBlocks);
  L.loss_total = o;
  return L;
}

// ------------------------------------------------------------------------------------------ ROC AUC
__global__ __launch_bounds__(kThreads) void auc_keys_kernel(const float *__restrict__ scores,
                                                            const int64_t *__restrict__ labels, int64_t n,
                                                            unsigned *__restrict__ keys,
                                                            unsigned char *__restrict__ lab,
                                                            AucHeader *__restrict__ hd) {
  constexpr int kDigits = AucRecord::kDigits;
  __shared__ unsigned h[kDigits * kRadix];
  __shared__ unsigned long long smp[kWaves];
  __shared__ unsigned smf[kWaves];
  for (int i = threadIdx.x; i < kDigits * kRadix; i += kThreads) h[i] = 0u;
  __syncthreads();
  unsigned long long pos = 0;
  unsigned flags = 0;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const float s = scores[i];
    const int64_t y = labels[i];
    if (!isfinite(s)) flags |= RM_METRIC_BAD_SCORE;
    if (y != 0 && y != 1) flags |= RM_METRIC_BAD_LABEL;
    const unsigned k = score_key(s);
    keys[i] = k;
    lab[i] = (unsigned char)(y == 1);
    pos += (y == 1);
#pragma unroll
    for (int p = 0; p < kDigits; ++p) atomicAdd(&h[p * kRadix + AucRecord::extract(k, p)], 1u);
  }
  flush_flags(flags, &hd->flags, smf);
  flush_positives(pos, &hd->pos, smp);
  flush_digit_hist(h, &hd->plan);
}

// Per tile of the sorted keys: thread t owns positions c0 + 16 t .. c0 + 16 t + 15.  For a positive at position
// i in group [a, b) it adds a + b + 1 where a (b) lies inside the tile, and counts it in head (tail) where the
// group starts before (ends after) the tile; last / first: the tile's last group start and first group end.
__global__ __launch_bounds__(kThreads) void auc_groups_kernel(
    const AucHeader *__restrict__ hd, const unsigned *__restrict__ keys0, const unsigned *__restrict__ keys1,
    const unsigned char *__restrict__ lab0, const unsigned char *__restrict__ lab1, int64_t n,
    unsigned long long *__restrict__ part, unsigned *__restrict__ head, unsigned *__restrict__ tail,
    int *__restrict__ last, unsigned *__restrict__ first) {
  const int m = hd->plan.m;  // the sorted pairs are in buffer m & 1
  const unsigned *keys = (m & 1) ? keys1 : keys0;
  const unsigned char *lab = (m & 1) ? lab1 : lab0;
  __shared__ unsigned sk[kTile + 2];  // sk[1 + li]; sk[0] / sk[valid + 1]: the neighbours across the edges
  __shared__ unsigned char sl[kTile];
  __shared__ int exs[kThreads];
  __shared__ unsigned exe[kThreads];
  __shared__ int smi[kWaves];
  __shared__ unsigned smu[kWaves];
  __shared__ unsigned long long sml[kWaves];

  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int valid = (int)min((int64_t)kTile, n - c0);
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int li = j * kThreads + tid;
    if (li < valid) {
      sk[1 + li] = keys[c0 + li];
      sl[li] = lab[c0 + li];
    }
  }
  if (tid == 0) sk[0] = c0 > 0 ? keys[c0 - 1] : 0u;
  if (tid == 1) sk[valid + 1] = c0 + valid < n ? keys[c0 + valid] : 0u;
  __syncthreads();

  unsigned sbits = 0u, ebits = 0u, pbits = 0u;
  int agg_s = -1;
  unsigned agg_e = kNoEnd;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    const int li = tid * kItems + q;
    if (li < valid) {
      const int64_t i = c0 + li;
      const bool st = i == 0 || sk[li + 1] != sk[li];
      const bool en = i == n - 1 || sk[li + 1] != sk[li + 2];
      sbits |= (unsigned)st << q;
      ebits |= (unsigned)en << q;
      pbits |= (unsigned)sl[li] << q;
      if (st) agg_s = (int)i;
      if (en && agg_e == kNoEnd) agg_e = (unsigned)(i + 1);
    }
  }
  // last start among the threads before, first end among the threads after
  const int incl_s = block_scan<false>(agg_s, OpMax(), smi);
  const unsigned incl_e = block_scan<true>(agg_e, OpMin(), smu);
  exs[tid] = incl_s;
  exe[tid] = incl_e;
  __syncthreads();
  const int carry_s = tid > 0 ? exs[tid - 1] : -1;
  const unsigned carry_e = tid + 1 < kThreads ? exe[tid + 1] : kNoEnd;

  int a[kItems];
  int run = carry_s;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    if ((sbits >> q) & 1u) run = (int)(c0 + tid * kItems + q);
    a[q] = run;
  }
  unsigned long long acc = 0;
  unsigned nh = 0u, nt = 0u;
  unsigned b = carry_e;
#pragma unroll
  for (int q = kItems - 1; q >= 0; --q) {
    if ((ebits >> q) & 1u) b = (unsigned)(c0 + tid * kItems + q + 1);
    if ((pbits >> q) & 1u) {
      acc += 1ull + (a[q] >= 0 ? (unsigned long long)a[q] : 0ull) + (b != kNoEnd ? (unsigned long long)b : 0ull);
      nh += a[q] < 0;
      nt += b == kNoEnd;
    }
  }
  acc = block_sum(acc, sml);
  nh = block_sum(nh, smu);
  nt = block_sum(nt, smu);
  if (tid == 0) {
    part[blockIdx.x] = acc;
    head[blockIdx.x] = nh;
    tail[blockIdx.x] = nt;
    last[blockIdx.x] = exs[kThreads - 1];
    first[blockIdx.x] = exe[0];
  }
}

__global__ __launch_bounds__(kThreads) void auc_final_kernel(
    const AucHeader *__restrict__ hd, int64_t n, int64_t tiles, const unsigned long long *__restrict__ part,
    const unsigned *__restrict__ head, const unsigned *__restrict__ tail, const int *__restrict__ last,
    const unsigned *__restrict__ first, rm_metric_result *__restrict__ out) {
  __shared__ int smi[kWaves];
  __shared__ unsigned smu[kWaves];
  __shared__ unsigned long long sml[kWaves];
  __shared__ int exs[kThreads];
  __shared__ unsigned exe[kThreads];
  const int tid = threadIdx.x;
  const int64_t seg = (tiles + kThreads - 1) / kThreads;
  const int64_t lo = min((int64_t)tid * seg, tiles), hi = min(lo + seg, tiles);
  int agg_s = -1;
  unsigned agg_e = kNoEnd;
  for (int64_t c = lo; c < hi; ++c) {
    agg_s = max(agg_s, last[c]);
    agg_e = min(agg_e, first[c]);
  }
  exs[tid] = block_scan<false>(agg_s, OpMax(), smi);
  exe[tid] = block_scan<true>(agg_e, OpMin(), smu);
  __syncthreads();
  // a tile's head positives belong to the group of the last start before it, its tail positives to the
  // group of the first end after it (position 0 starts and position n - 1 ends a group: both exist
  // whenever they are needed)
  unsigned long long acc = 0;
  int run = tid > 0 ? exs[tid - 1] : -1;
  for (int64_t c = lo; c < hi; ++c) {
    acc += part[c];
    if (head[c]) acc += (unsigned long long)head[c] * (unsigned long long)run;
    run = max(run, last[c]);
  }
  unsigned runE = tid + 1 < kThreads ? exe[tid + 1] : kNoEnd;
  for (int64_t c = hi - 1; c >= lo; --c) {
    if (tail[c]) acc += (unsigned long long)tail[c] * (unsigned long long)runE;
    runE = min(runE, first[c]);
  }
  acc = block_sum(acc, sml);
  if (tid == 0) {
    const unsigned long long P = hd->pos, N = (unsigned long long)n - P;
    long long flags = hd->flags;
    double v;
    if (P == 0 || N == 0) {
      flags |= RM_METRIC_ONE_CLASS;
      v = __builtin_nan("");
    } else {
      const unsigned long long two_u = acc - P * (P + 1ull);
      v = (double)two_u / (2.0 * (double)P * (double)N);
    }
    out->value = v;
    out->pos = (int64_t)P;
    out->neg = (int64_t)N;
    out->flags = flags;
  }
}

// ----------------------------------------------------------------------------------------- log loss
// sklearn 1.7.2 binary log_loss on float32 y_pred: p and 1 - p clipped in fp32 to [eps, 1 - eps], the log of
// the one the label selects taken in fp64, summed in fp64, divided by n.  Probabilities outside [0, 1] are
// flagged (sklearn raises on them).
__global__ __launch_bounds__(kThreads) void logloss_kernel(const float *__restrict__ pred,
                                                           const int64_t *__restrict__ labels, int64_t n,
                                                           float eps, double *__restrict__ part,
                                                           unsigned long long *__restrict__ pos,
                                                           unsigned *__restrict__ flags) {
  __shared__ double smd[kWaves];
  __shared__ unsigned long long sml[kWaves];
  __shared__ unsigned smu[kWaves];
  const float hi = 1.0f - eps;
  double acc = 0.0;
  unsigned long long np = 0;
  unsigned f = 0;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const float x = pred[i];
    const int64_t y = labels[i];
    if (!isfinite(x)) f |= RM_METRIC_BAD_SCORE;
    if (x < 0.0f || x > 1.0f) f |= RM_METRIC_PROB_RANGE;
    if (y != 0 && y != 1) f |= RM_METRIC_BAD_LABEL;
    const float c = fminf(fmaxf(x, eps), hi);
    const float v = y == 1 ? c : 1.0f - c;
    acc += log((double)v);
    np += (y == 1);
  }
  acc = block_sum(acc, smd);
  np = block_sum(np, sml);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) f |= __shfl_xor(f, o, 64);
  if ((threadIdx.x & 63) == 0) smu[threadIdx.x >> 6] = f;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) f |= smu[w];
    part[blockIdx.x] = acc;
    pos[blockIdx.x] = np;
    flags[blockIdx.x] = f;
  }
}

__global__ __launch_bounds__(kThreads) void logloss_final_kernel(const double *__restrict__ part,
                                                                 const unsigned long long *__restrict__ pos,
                                                                 const unsigned *__restrict__ flags, int nb,
                                                                 int64_t n, rm_metric_result *__restrict__ out) {
  __shared__ double smd[kWaves];
  __shared__ unsigned long long sml[kWaves];
  __shared__ unsigned smu[kWaves];
  double s = 0.0;
  unsigned long long p = 0;
  unsigned f = 0;
  for (int b = threadIdx.x; b < nb; b += kThreads) {
    s += part[b];
    p += pos[b];
    f |= flags[b];
  }
  s = block_sum(s, smd);
  p = block_sum(p, sml);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) f |= __shfl_xor(f, o, 64);
  if ((threadIdx.x & 63) == 0) smu[threadIdx.x >> 6] = f;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) f |= smu[w];
    const unsigned long long N = (unsigned long long)n - p;
    if (p == 0 || N == 0) f |= RM_METRIC_ONE_CLASS;
    out->value = -s / (double)n;
    out->pos = (int64_t)p;
    out->neg = (int64_t)N;
    out->flags = (int64_t)f;
  }
}

}  // namespace

extern "C" int64_t rm_metric_workspace(int64_t n) {
  if (n < 1 || n > 0x7FFFFFFFll) return 0;
  const Layout L = layout(n);
  return (int64_t)(L.total > L.loss_total ? L.total : L.loss_total);
}

extern "C" int rm_roc_auc(const float *scores, const int64_t *labels, int64_t n, void *workspace,
                          rm_metric_result *out, rm_stream_t stream) {
  RM_REQUIRE(n >= 1 && n <= 0x7FFFFFFFll, "rm_roc_auc: n = %lld outside [1, 2^31 - 1]", (long long)n);
  RM_REQUIRE(scores && labels && workspace && out, "rm_roc_auc: NULL pointer");
  RM_REQUIRE(rm_aligned16(workspace) && rm_aligned16(out), "rm_roc_auc: workspace / out not 16-byte aligned");
  const Layout L = layout(n);
  char *ws = (char *)workspace;
  AucHeader *hd = (AucHeader *)(ws + L.header);
  unsigned *hist = (unsigned *)(ws + L.hist);
  unsigned long long *part = (unsigned long long *)(ws + L.part);
  unsigned *head = (unsigned *)(ws + L.head), *tail = (unsigned *)(ws + L.tail);
  int *last = (int *)(ws + L.last);
  unsigned *first = (unsigned *)(ws + L.first);
  unsigned *k0 = (unsigned *)(ws + L.keys0), *k1 = (unsigned *)(ws + L.keys1);
  unsigned char *l0 = (unsigned char *)(ws + L.lab0), *l1 = (unsigned char *)(ws + L.lab1);
  const int64_t tiles = (n + kTile - 1) / kTile;
  hipStream_t s = (hipStream_t)stream;

  if (hipMemsetAsync(hd, 0, sizeof(AucHeader), s) != hipSuccess) {
    rm_set_error("rm_roc_auc: hipMemsetAsync failed");
    return RM_ELAUNCH;
  }
  hipLaunchKernelGGL(auc_keys_kernel, dim3(rm_grid_cap((n + kThreads - 1) / kThreads, kKeyBlocks)),
                     dim3(kThreads), 0, s, scores, labels, n, k0, l0, hd);
  radix_sort<AucRecord>(&hd->plan, {{{k0}, {k1}}, {l0, l1}}, n, hist, s);
  hipLaunchKernelGGL(auc_groups_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, hd, k0, k1, l0, l1, n, part,
                     head, tail, last, first);
  hipLaunchKernelGGL(auc_final_kernel, dim3(1), dim3(kThreads), 0, s, hd, n, tiles, part, head, tail, last, first,
                     out);
  RM_CHECK_LAUNCH("rm_roc_auc");
  return RM_OK;
}

extern "C" int rm_log_loss(const float *pred, const int64_t *labels, int64_t n, float eps, void *workspace,
                           rm_metric_result *out, rm_stream_t stream) {
  RM_REQUIRE(n >= 1 && n <= 0x7FFFFFFFll, "rm_log_loss: n = %lld outside [1, 2^31 - 1]", (long long)n);
  RM_REQUIRE(pred && labels && workspace && out, "rm_log_loss: NULL pointer");
  RM_REQUIRE(rm_aligned16(workspace) && rm_aligned16(out), "rm_log_loss: workspace / out not 16-byte aligned");
  RM_REQUIRE(eps > 0.0f && eps < 0.5f, "rm_log_loss: eps must lie in (0, 0.5)");
  const Layout L = layout(n);
  char *ws = (char *)workspace;
  double *part = (double *)(ws + L.loss_part);
  unsigned long long *pos = (unsigned long long *)(ws + L.loss_pos);
  unsigned *flags = (unsigned *)(ws + L.loss_flags);
  const int nb = rm_grid_cap((n + kThreads - 1) / kThreads, kLossBlocks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(logloss_kernel, dim3(nb), dim3(kThreads), 0, s, pred, labels, n, eps, part, pos, flags);
  hipLaunchKernelGGL(logloss_final_kernel, dim3(1), dim3(kThreads), 0, s, part, pos, flags, nb, n, out);
  RM_CHECK_LAUNCH("rm_log_loss");
  return RM_OK;
}
