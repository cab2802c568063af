// The one device-wide sort of the metric family (metrics.hip, gauc.hip, rankmetrics.hip, rank.hip): a stable LSD
// radix sort by 8-bit digits over tiles of 4096 records, which skips every digit that is the same in all records.
//
// A record is one or two uint32 columns and, where the user has one, a label byte that rides along.  A user
// describes its record with a policy R:
//   R::kCols            1 or 2: the uint32 columns
//   R::kLabel           whether a label byte rides along
//   R::kDigits          how many 8-bit digits the sort order has, the least significant first
//   R::column(p)        the column that alone holds digit p (sort_hist_kernel reads only that one)
//   R::extract(v, p)    digit p of a value v of that column
// A column or label the record lacks costs nothing: no registers, no LDS, no loads or stores.
//
// The user's keys kernel writes the records into buffer 0 and counts every digit of every record into
// SortPlan::ghist (flush_digit_hist); radix_sort() then issues, on the stream,
//   sort_plan_kernel      which of the digits vary (a constant digit's pass is skipped) and the global digit bases
//                         of each pass that runs
//   per pass:
//     sort_hist_kernel      per-tile digit counts
//     sort_scan_kernel      device-wide exclusive scan of the counts, digit-major
//     sort_pass_kernel      stable tile-local ranking (wave match + per-wave counters) staged through LDS, then a
//                           scatter in runs of equal digits
// A pass past SortPlan::m returns at once, and pass `slot` reads buffer slot & 1 and writes the other: afterwards
// the sorted records are in buffer m & 1.  Nothing is read back by the host.
#pragma once
#include <math.h>

#include "rm_metric_common.h"

namespace {

template <int kDigits>
struct SortPlan {
  unsigned ghist[kDigits][kRadix];  // count of every value of digit p over all records (the keys kernel)
  int m;                            // passes that run (digits that vary)
  int digit[kDigits];               // which digit each of them sorts by, low first
  unsigned base[kDigits][kRadix];   // exclusive scan of the pass's global digit counts
};

// the two ping-pong buffers of a record's columns (and labels)
template <class R, bool = R::kLabel>
struct SortBuffers {
  unsigned *col[2][R::kCols];
  unsigned char *lab[2];
};
template <class R>
struct SortBuffers<R, false> {
  unsigned *col[2][R::kCols];
};

// a tile of records in LDS, between the ranking and the scatter
template <class R, bool = R::kLabel>
struct SortStage {
  unsigned col[R::kCols][kTile];
  unsigned char lab[kTile];
};
template <class R>
struct SortStage<R, false> {
  unsigned col[R::kCols][kTile];
};

template <class R>
__device__ __forceinline__ unsigned record_digit(const unsigned (&v)[R::kCols], int p) {
  unsigned x = v[0];
  if constexpr (R::kCols == 2) x = R::column(p) ? v[1] : v[0];
  return R::extract(x, p);
}

// ------------------------------------------------------------------------------ the tail of a keys kernel
// OR of `flags` over the block into *out (untouched when nothing is set); sm: kWaves entries
__device__ __forceinline__ void flush_flags(unsigned flags, unsigned *out, unsigned *sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = flags;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned f = 0;
    for (int w = 0; w < kWaves; ++w) f |= sm[w];
    if (f) atomicOr(out, f);
  }
}

// sum of `pos` over the block added to *out; sm: kWaves entries
__device__ __forceinline__ void flush_positives(unsigned long long pos, unsigned long long *out,
                                                unsigned long long *sm) {
  pos = block_sum(pos, sm);
  if (threadIdx.x == 0 && pos) atomicAdd(out, pos);
}

// the block's digit counts h[kDigits * kRadix] (LDS, complete: a barrier lies behind the last count) into the plan
template <int kDigits>
__device__ __forceinline__ void flush_digit_hist(const unsigned *h, SortPlan<kDigits> *plan) {
  for (int i = threadIdx.x; i < kDigits * kRadix; i += kThreads)
    if (h[i]) atomicAdd(&plan->ghist[i / kRadix][i % kRadix], h[i]);
}

// ----------------------------------------------------------------------------------------------- the sort
template <int kDigits>
__global__ __launch_bounds__(kThreads) void sort_plan_kernel(SortPlan<kDigits> *__restrict__ plan, int64_t n) {
  __shared__ unsigned sm[kWaves];
  const int d = threadIdx.x;
  int m = 0;
  for (int p = 0; p < kDigits; ++p) {
    const unsigned c = plan->ghist[p][d];
    if (__syncthreads_or(c == (unsigned)n)) continue;  // one digit value in every record: nothing to sort
    const unsigned incl = block_scan<false>(c, OpAdd(), sm);
    plan->base[m][d] = incl - c;
    if (d == 0) plan->digit[m] = p;
    ++m;
  }
  if (d == 0) plan->m = m;
}

template <class R>
__global__ __launch_bounds__(kThreads) void sort_hist_kernel(const SortPlan<R::kDigits> *__restrict__ plan, int slot,
                                                             const SortBuffers<R> b, int64_t n, int64_t tiles,
                                                             unsigned *__restrict__ hist) {
  if (slot >= plan->m) return;
  const int p = plan->digit[slot];
  const unsigned *src = (slot & 1) ? b.col[1][0] : b.col[0][0];
  if constexpr (R::kCols == 2) {
    if (R::column(p)) src = (slot & 1) ? b.col[1][1] : b.col[0][1];
  }
  __shared__ unsigned h[kRadix];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * kTile;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t i = t0 + j * kThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[R::extract(src[i], p)], 1u);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// In place, by one block: row[t] -> start + row[0] + ... + row[t - 1].  Thread k takes a contiguous segment of the
// row; returns the inclusive sum over the segments up to the caller's (the last thread: the row's sum, without
// start).  sm: kWaves entries.
__device__ __forceinline__ unsigned scan_row(unsigned *__restrict__ row, int64_t tiles, unsigned start,
                                             unsigned *sm) {
  const int64_t seg = (tiles + kThreads - 1) / kThreads;
  const int64_t lo = min((int64_t)threadIdx.x * seg, tiles), hi = min(lo + seg, tiles);
  unsigned s = 0;
  for (int64_t i = lo; i < hi; ++i) s += row[i];
  const unsigned incl = block_scan<false>(s, OpAdd(), sm);
  unsigned run = start + incl - s;
  for (int64_t i = lo; i < hi; ++i) {
    const unsigned c = row[i];
    row[i] = run;
    run += c;
  }
  return incl;
}

// one block per digit value: its row of per-tile counts -> global positions (base of the value + the counts of
// the tiles before)
template <int kDigits>
__global__ __launch_bounds__(kThreads) void sort_scan_kernel(const SortPlan<kDigits> *__restrict__ plan, int slot,
                                                             int64_t tiles, unsigned *__restrict__ hist) {
  if (slot >= plan->m) return;
  __shared__ unsigned sm[kWaves];
  const int d = blockIdx.x;
  scan_row(hist + (int64_t)d * tiles, tiles, plan->base[slot][d], sm);
}

// One LSD pass over a tile of 4096 records.  Wave w holds tile positions [1024 w, 1024 w + 1024), item j of lane l
// at 1024 w + 64 j + l: the tile order is (wave, item, lane), which the ranking keeps.  Past the end of the array a
// slot holds 0xFFFFFFFF in every column: the largest value of every digit, at the tile's last positions, so it
// ranks after every real record and is never written.
template <class R>
__global__ __launch_bounds__(kThreads) void sort_pass_kernel(const SortPlan<R::kDigits> *__restrict__ plan, int slot,
                                                             const SortBuffers<R> b, int64_t n, int64_t tiles,
                                                             const unsigned *__restrict__ hist) {
  if (slot >= plan->m) return;
  const int p = plan->digit[slot];
  constexpr int kCols = R::kCols;
  const unsigned *src[kCols];
  unsigned *dst[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    src[c] = (slot & 1) ? b.col[1][c] : b.col[0][c];
    dst[c] = (slot & 1) ? b.col[0][c] : b.col[1][c];
  }
  const unsigned char *src_l = nullptr;
  unsigned char *dst_l = nullptr;
  if constexpr (R::kLabel) {
    src_l = (slot & 1) ? b.lab[1] : b.lab[0];
    dst_l = (slot & 1) ? b.lab[0] : b.lab[1];
  }

  __shared__ unsigned wcnt[kWaves][kRadix];  // per-wave digit counters, then per-wave digit offsets
  __shared__ unsigned tstart[kRadix];        // first tile rank of each digit
  __shared__ unsigned gofs[kRadix];          // global position of that rank
  __shared__ SortStage<R> st;
  __shared__ unsigned sm[kWaves];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = tid; i < kWaves * kRadix; i += kThreads) (&wcnt[0][0])[i] = 0u;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * kTile;
  const int valid = (int)min((int64_t)kTile, n - t0);
  const unsigned long long below_mask = (1ull << lane) - 1ull;

  unsigned v[kItems][kCols], r[kItems], lbits = 0u;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int li = w * (kTile / kWaves) + j * 64 + lane;
    unsigned y = 0u;
#pragma unroll
    for (int c = 0; c < kCols; ++c) v[j][c] = 0xFFFFFFFFu;
    if (li < valid) {
#pragma unroll
      for (int c = 0; c < kCols; ++c) v[j][c] = src[c][t0 + li];
      if constexpr (R::kLabel) y = src_l[t0 + li];
    }
    lbits |= y << j;
    const unsigned d = record_digit<R>(v[j], p);
    unsigned long long peers = ~0ull;  // lanes with the same digit
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool bit = (d >> q) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const unsigned before = (unsigned)__popcll(peers & below_mask);
    const int leader = __ffsll((long long)peers) - 1;
    unsigned old = 0u;
    if (before == 0u) old = atomicAdd(&wcnt[w][d], (unsigned)__popcll(peers));
    r[j] = (unsigned)__shfl((int)old, leader, 64) + before;
  }
  __syncthreads();
  {
    const int d = tid;
    unsigned run = 0u;
#pragma unroll
    for (int u = 0; u < kWaves; ++u) {
      const unsigned c = wcnt[u][d];
      wcnt[u][d] = run;
      run += c;
    }
    const unsigned incl = block_scan<false>(run, OpAdd(), sm);
    tstart[d] = incl - run;
    gofs[d] = hist[(int64_t)d * tiles + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const unsigned d = record_digit<R>(v[j], p);
    const unsigned rank = tstart[d] + wcnt[w][d] + r[j];
#pragma unroll
    for (int c = 0; c < kCols; ++c) st.col[c][rank] = v[j][c];
    if constexpr (R::kLabel) st.lab[rank] = (unsigned char)((lbits >> j) & 1u);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int li = j * kThreads + tid;
    if (li < valid) {
      unsigned x[kCols];
#pragma unroll
      for (int c = 0; c < kCols; ++c) x[c] = st.col[c][li];
      const unsigned d = record_digit<R>(x, p);
      const int64_t at = (int64_t)gofs[d] + (li - (int)tstart[d]);
#pragma unroll
      for (int c = 0; c < kCols; ++c) dst[c][at] = x[c];
      if constexpr (R::kLabel) dst_l[at] = st.lab[li];
    }
  }
}

// Sorts the n records of buffer 0 (whose digit counts are in plan->ghist): the plan, then `passes` x (hist, scan,
// pass).  `passes` below R::kDigits is for a caller that knows the digits from `passes` up to be constant.  hist:
// kRadix x tiles counters.
template <class R>
void radix_sort(SortPlan<R::kDigits> *plan, const SortBuffers<R> &b, int64_t n, unsigned *hist, hipStream_t s,
                int passes = R::kDigits) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  hipLaunchKernelGGL(sort_plan_kernel<R::kDigits>, dim3(1), dim3(kThreads), 0, s, plan, n);
  for (int slot = 0; slot < passes; ++slot) {
    hipLaunchKernelGGL(sort_hist_kernel<R>, dim3((unsigned)tiles), dim3(kThreads), 0, s, plan, slot, b, n, tiles,
                       hist);
    hipLaunchKernelGGL(sort_scan_kernel<R::kDigits>, dim3(kRadix), dim3(kThreads), 0, s, plan, slot, tiles, hist);
    hipLaunchKernelGGL(sort_pass_kernel<R>, dim3((unsigned)tiles), dim3(kThreads), 0, s, plan, slot, b, n, tiles,
                       hist);
  }
}

// ------------------------------------------------------- the (score key, group, label) record of gauc / rankmetrics
// digits 0..3: the bytes of the score key, 4..7: those of the group id - sorted by (group, key)
struct GroupedScoreRecord {
  static constexpr int kCols = 2;  // 0 the key, 1 the group
  static constexpr bool kLabel = true;
  static constexpr int kDigits = 8;
  static __device__ __forceinline__ int column(int p) { return p >> 2; }
  static __device__ __forceinline__ unsigned extract(unsigned v, int p) { return (v >> (8 * (p & 3))) & 255u; }
};

struct GroupedScoreHeader {
  unsigned long long pos;  // P over all examples
  unsigned flags;          // RM_METRIC_* of the inputs
  unsigned groups;         // distinct group ids (the user's carry kernel)
  SortPlan<GroupedScoreRecord::kDigits> plan;
};

// validate; score -> order-preserving uint32 key (kDescending: its complement, so that ascending in the key is
// descending in the score), label -> byte, group -> uint32 (0 when there is no id column); P; the eight digit
// histograms in one read
template <bool kDescending>
__global__ __launch_bounds__(kThreads) void grouped_keys_kernel(
    const float *__restrict__ scores, const int64_t *__restrict__ labels, const int64_t *__restrict__ groups,
    int64_t n, unsigned *__restrict__ keys, unsigned *__restrict__ grp, unsigned char *__restrict__ lab,
    GroupedScoreHeader *__restrict__ hd) {
  using R = GroupedScoreRecord;
  __shared__ unsigned h[R::kDigits * kRadix];
  __shared__ unsigned long long smp[kWaves];
  __shared__ unsigned smf[kWaves];
  for (int i = threadIdx.x; i < R::kDigits * kRadix; i += kThreads) h[i] = 0u;
  __syncthreads();
  unsigned long long pos = 0;
  unsigned flags = 0;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const float s = scores[i];
    const int64_t y = labels[i];
    const int64_t gid = groups ? groups[i] : 0;
    if (!isfinite(s)) flags |= RM_METRIC_BAD_SCORE;
    if (y != 0 && y != 1) flags |= RM_METRIC_BAD_LABEL;
    if (gid < 0 || gid > 0xFFFFFFFFll) flags |= RM_METRIC_BAD_GROUP;
    const unsigned v[2] = {kDescending ? ~score_key(s) : score_key(s), (unsigned)gid};
    keys[i] = v[0];
    grp[i] = v[1];
    lab[i] = (unsigned char)(y == 1);
    pos += (y == 1);
#pragma unroll
    for (int p = 0; p < R::kDigits; ++p) atomicAdd(&h[p * kRadix + record_digit<R>(v, p)], 1u);
  }
  flush_flags(flags, &hd->flags, smf);
  flush_positives(pos, &hd->pos, smp);
  flush_digit_hist(h, &hd->plan);
}

}  // namespace
