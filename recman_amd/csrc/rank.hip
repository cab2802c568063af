// Grouped ranking objectives next to the pointwise loss: the RankNet / BPR pair loss and the ListNet softmax loss over
// the examples of a batch that share a group id; see recman_hip_rank.h.  With the examples sorted by (group, label) a
// group g is the sorted positions [s, e): its negatives [s, m), then its positives [m, e).  Kernels, in launch order:
//   rank_keys_kernel      validate; group -> uint32, (label << 31 | example) -> uint32 payload; the five digit
//                         histograms (the label bit, four of the group) in one read
//   radix_sort            (rm_radix_sort.h) the stable LSD radix sort of (group, payload), the label first, then the
//                         group digits: its plan kernel, then (hist, scan, pass) per digit
//   rank_marks_kernel     per tile of the sorted order: the number of group starts
//   rank_carry_kernel     over the tiles: the slot of each tile's first start (exclusive sum); the number of groups
//   rank_bounds_kernel    per sorted position: its group's slot and its logit; per group s, m, e - each written by the
//                         one position that knows it (the start; the first positive, or the last position when it is a
//                         negative; the last position)
//   rank_pieces_kernel    (listwise) per piece = (group, chunk of 256 sorted positions): max and sum-exp, float32, by
//                         the thread at the piece's first position
//   rank_groups_kernel    per group: n, P, N, scored; (listwise) its pieces combined in position order, the sum in
//                         double; per-block partials of Q, P, W and the scored count
//   rank_totals_kernel    fixed-order sum of the partials into the header
//   rank_pair_kernel      (pairwise) one thread per sorted position and split: its sum of sigmoid(-d) and, for a
//                         positive, of softplus(-d) over its share of the opposite-class run of its group, streamed
//                         through LDS; a tile in float32, the tiles in double; per-block loss partials
//   rank_pair_finish_kernel / rank_list_kernel
//                         one thread per sorted position: c_g in double, rounded once; its own dL/ds (pairwise: the
//                         splits added in order) combined with dlogit_in into dlogit_out at its example; (listwise) a
//                         positive's loss share, in double, per-block partials
//   rank_final_kernel     fixed-order sum of the loss partials, loss_out, the record
// No float atomics; nothing is read back by the host between the kernels.
#include <math.h>

#include "../../include/recman_hip_rank.h"
#include "rm_radix_sort.h"

namespace {

constexpr int kReduceBlocks = 1024;
constexpr int kPairTile = RM_RANK_TILE;  // scores of an LDS tile of the opposite-class run
constexpr int kPiece = RM_RANK_PIECE;    // sorted positions of a listwise piece (= kThreads)
constexpr int kSplits = RM_RANK_SPLITS;  // blocks that share the opposite-class runs of one block of positions
constexpr unsigned kExample = 0x7FFFFFFFu;
static_assert(kPiece == kThreads, "a piece is what one block of rank_pieces_kernel holds");

// the sorted record: two columns, the group id and the payload; digit 0 is the label bit of the payload, digits
// 1..4 the bytes of the group id (low first)
struct RankRecord {
  static constexpr int kCols = 2;  // 0 the group, 1 the payload
  static constexpr bool kLabel = false;
  static constexpr int kDigits = 5;
  static __device__ __forceinline__ int column(int p) { return p == 0; }
  static __device__ __forceinline__ unsigned extract(unsigned v, int p) {
    return (v >> (p == 0 ? 31 : 8 * (p - 1))) & (p == 0 ? 1u : 255u);
  }
};

struct RankHeader {
  unsigned flags;                   // RM_METRIC_* of the inputs
  unsigned groups;                  // distinct group ids (rank_carry_kernel)
  long long pairs, pos, weight, scored;  // Q, P, W and the scored groups (rank_totals_kernel)
  SortPlan<RankRecord::kDigits> plan;
};

struct Layout {
  size_t header, hist, cnt, grp0, grp1, pay0, pay1, slot, ss, gs, gm, ge, pm, ps, gmax, gsum;
  size_t rq, rp, rw, rs, pg, lpart, total;
};

inline size_t pair_blocks(int64_t n) { return (size_t)((n + kThreads - 1) / kThreads); }

Layout layout(int64_t n) {
  const size_t tiles = (size_t)((n + kTile - 1) / kTile), un = (size_t)n;
  Layout L;
  size_t o = 0;
  L.header = take(o, sizeof(RankHeader));
  L.hist = take(o, 4 * kRadix * tiles);
  L.cnt = take(o, 4 * tiles);
  L.grp0 = take(o, 4 * un);
  L.grp1 = take(o, 4 * un);
  L.pay0 = take(o, 4 * un);
  L.pay1 = take(o, 4 * un);
  L.slot = take(o, 4 * un);
  L.ss = take(o, 4 * un);
  L.gs = take(o, 4 * un);
  L.gm = take(o, 4 * un);
  L.ge = take(o, 4 * un);
  L.pm = take(o, 4 * un);
  L.ps = take(o, 4 * un);
  L.gmax = take(o, 4 * un);
  L.gsum = take(o, 8 * un);
  L.rq = take(o, 8 * kReduceBlocks);
  L.rp = take(o, 8 * kReduceBlocks);
  L.rw = take(o, 8 * kReduceBlocks);
  L.rs = take(o, 8 * kReduceBlocks);
  L.pg = take(o, 4 * un * kSplits);
  L.lpart = take(o, 8 * pair_blocks(n) * kSplits);
  L.total = o;
  return L;
}

__global__ __launch_bounds__(kThreads) void rank_keys_kernel(
    const float *__restrict__ logit, const int64_t *__restrict__ labels, const int64_t *__restrict__ groups,
    int64_t n, unsigned *__restrict__ grp, unsigned *__restrict__ pay, RankHeader *__restrict__ hd) {
  constexpr int kDigits = RankRecord::kDigits;
  __shared__ unsigned h[kDigits * kRadix];
  __shared__ unsigned smf[kWaves];
  for (int i = threadIdx.x; i < kDigits * kRadix; i += kThreads) h[i] = 0u;
  __syncthreads();
  unsigned flags = 0;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const float s = logit[i];
    const int64_t y = labels[i];
    const int64_t gid = groups ? groups[i] : 0;
    if (!isfinite(s)) flags |= RM_METRIC_BAD_SCORE;
    if (y != 0 && y != 1) flags |= RM_METRIC_BAD_LABEL;
    if (gid < 0 || gid > 0xFFFFFFFFll) flags |= RM_METRIC_BAD_GROUP;
    const unsigned v[2] = {(unsigned)gid, ((unsigned)(y == 1) << 31) | (unsigned)i};
    grp[i] = v[0];
    pay[i] = v[1];
#pragma unroll
    for (int p = 0; p < kDigits; ++p) atomicAdd(&h[p * kRadix + record_digit<RankRecord>(v, p)], 1u);
  }
  flush_flags(flags, &hd->flags, smf);
  flush_digit_hist(h, &hd->plan);
}

// Thread t owns tile positions 16 t .. 16 t + 15.  Position i starts a group when i == 0 or its id differs from
// i - 1's.
__global__ __launch_bounds__(kThreads) void rank_marks_kernel(const RankHeader *__restrict__ hd,
                                                              const unsigned *__restrict__ grp0,
                                                              const unsigned *__restrict__ grp1, int64_t n,
                                                              unsigned *__restrict__ cnt) {
  const unsigned *grp = (hd->plan.m & 1) ? grp1 : grp0;  // the sorted pairs are in buffer m & 1
  __shared__ unsigned smu[kWaves];
  const int64_t c0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
  unsigned c = 0u;
  if (c0 < n) {
    unsigned prev = c0 > 0 ? grp[c0 - 1] : 0u;
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
      const int64_t i = c0 + q;
      if (i < n) {
        const unsigned g = grp[i];
        c += (i == 0 || g != prev);
        prev = g;
      }
    }
  }
  c = block_sum(c, smu);
  if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

// In place, over the tiles: cnt -> the number of group starts before the tile; the number of groups.
__global__ __launch_bounds__(kThreads) void rank_carry_kernel(RankHeader *__restrict__ hd, int64_t tiles,
                                                              unsigned *__restrict__ cnt) {
  __shared__ unsigned smu[kWaves];
  const unsigned ic = scan_row(cnt, tiles, 0u, smu);
  if (threadIdx.x == kThreads - 1) hd->groups = ic;
}

__global__ __launch_bounds__(kThreads) void rank_bounds_kernel(
    const RankHeader *__restrict__ hd, const unsigned *__restrict__ grp0, const unsigned *__restrict__ grp1,
    const unsigned *__restrict__ pay0, const unsigned *__restrict__ pay1, const float *__restrict__ logit, int64_t n,
    const unsigned *__restrict__ cnt, unsigned *__restrict__ slot_of, float *__restrict__ ss,
    unsigned *__restrict__ gs, unsigned *__restrict__ gm, unsigned *__restrict__ ge) {
  const int m = hd->plan.m;
  const unsigned *grp = (m & 1) ? grp1 : grp0, *pay = (m & 1) ? pay1 : pay0;
  __shared__ unsigned smu[kWaves];
  const int64_t c0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
  unsigned g[kItems + 2], lab[kItems + 1];  // [q + 1] = position c0 + q; [0] / [kItems + 1] its neighbours
  unsigned c = 0u;
  if (c0 < n) {
    g[0] = c0 > 0 ? grp[c0 - 1] : 0u;
    lab[0] = c0 > 0 ? pay[c0 - 1] >> 31 : 0u;
#pragma unroll
    for (int q = 0; q < kItems + 1; ++q) {
      const int64_t i = c0 + q;
      g[q + 1] = i < n ? grp[i] : 0u;
    }
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
      const int64_t i = c0 + q;
      if (i < n) c += (i == 0 || g[q + 1] != g[q]);
    }
  }
  const unsigned incl = block_scan<false>(c, OpAdd(), smu);
  if (c0 >= n) return;
  int64_t slot = (int64_t)cnt[blockIdx.x] + (incl - c) - 1;  // of the group open at this thread's first position
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    const int64_t i = c0 + q;
    if (i < n) {
      const unsigned py = pay[i], y = py >> 31;
      lab[q + 1] = y;
      const bool start = i == 0 || g[q + 1] != g[q];
      const bool last = i == n - 1 || g[q + 2] != g[q + 1];
      slot += start;
      slot_of[i] = (unsigned)slot;
      ss[i] = logit[py & kExample];
      if (start) gs[slot] = (unsigned)i;
      if (y && (start || !lab[q])) gm[slot] = (unsigned)i;  // the first positive
      if (last) {
        ge[slot] = (unsigned)(i + 1);
        if (!y) gm[slot] = (unsigned)(i + 1);  // no positive
      }
    }
  }
}

// One block per chunk of kPiece sorted positions; the thread at the first position of a piece (a group's part of the
// chunk) walks it: its max, then its sum of exp(s - max).
__global__ __launch_bounds__(kThreads) void rank_pieces_kernel(const unsigned *__restrict__ slot_of,
                                                               const float *__restrict__ ss, int64_t n,
                                                               float *__restrict__ pm, float *__restrict__ ps) {
  __shared__ unsigned sl[kPiece];
  __shared__ float sv[kPiece];
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * kPiece;
  const int valid = (int)min((int64_t)kPiece, n - c0);
  if (tid < valid) {
    sl[tid] = slot_of[c0 + tid];
    sv[tid] = ss[c0 + tid];
  }
  __syncthreads();
  if (tid >= valid) return;
  const unsigned mine = sl[tid];
  if (tid > 0 && sl[tid - 1] == mine) return;
  float mx = sv[tid];
  int end = tid + 1;
  while (end < valid && sl[end] == mine) {
    mx = fmaxf(mx, sv[end]);
    ++end;
  }
  float sum = 0.f;
  for (int k = tid; k < end; ++k) sum += expf(sv[k] - mx);
  pm[c0 + tid] = mx;
  ps[c0 + tid] = sum;
}

// Block k takes the slots [k chunk, (k + 1) chunk).
template <bool kList>
__global__ __launch_bounds__(kThreads) void rank_groups_kernel(
    const RankHeader *__restrict__ hd, const unsigned *__restrict__ gs, const unsigned *__restrict__ gm,
    const unsigned *__restrict__ ge, const float *__restrict__ pm, const float *__restrict__ ps,
    float *__restrict__ gmax, double *__restrict__ gsum, long long *__restrict__ rq, long long *__restrict__ rp,
    long long *__restrict__ rw, long long *__restrict__ rs) {
  __shared__ long long sml[kWaves];
  const int64_t G = hd->groups;
  const int64_t chunk = (G + gridDim.x - 1) / gridDim.x;
  const int64_t lo = min((int64_t)blockIdx.x * chunk, G), hi = min(lo + chunk, G);
  long long q = 0, p = 0, w = 0, sc = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const long long s = gs[i], m = gm[i], e = ge[i];
    const long long N = m - s, P = e - m;
    if (P > 0 && N > 0) {
      q += P * N;
      p += P;
      w += e - s;
      ++sc;
      if (kList) {
        // the pieces start at s and at every multiple of kPiece inside (s, e)
        float mx = pm[s];
        for (long long k = (s / kPiece + 1) * kPiece; k < e; k += kPiece) mx = fmaxf(mx, pm[k]);
        double sum = (double)ps[s] * (double)expf(pm[s] - mx);
        for (long long k = (s / kPiece + 1) * kPiece; k < e; k += kPiece)
          sum += (double)ps[k] * (double)expf(pm[k] - mx);
        gmax[i] = mx;
        gsum[i] = sum;
      }
    }
  }
  q = block_sum(q, sml);
  p = block_sum(p, sml);
  w = block_sum(w, sml);
  sc = block_sum(sc, sml);
  if (threadIdx.x == 0) {
    rq[blockIdx.x] = q;
    rp[blockIdx.x] = p;
    rw[blockIdx.x] = w;
    rs[blockIdx.x] = sc;
  }
}

__global__ __launch_bounds__(kThreads) void rank_totals_kernel(RankHeader *__restrict__ hd, int nb,
                                                               const long long *__restrict__ rq,
                                                               const long long *__restrict__ rp,
                                                               const long long *__restrict__ rw,
                                                               const long long *__restrict__ rs) {
  __shared__ long long sml[kWaves];
  long long q = 0, p = 0, w = 0, sc = 0;
  for (int b = threadIdx.x; b < nb; b += kThreads) {
    q += rq[b];
    p += rp[b];
    w += rw[b];
    sc += rs[b];
  }
  q = block_sum(q, sml);
  p = block_sum(p, sml);
  w = block_sum(w, sml);
  sc = block_sum(sc, sml);
  if (threadIdx.x == 0) {
    hd->pairs = q;
    hd->pos = p;
    hd->weight = w;
    hd->scored = sc;
  }
}

// c_g of a scored group, in double
__device__ __forceinline__ double coef(const RankHeader *__restrict__ hd, int kind, int norm, long long n_g,
                                       long long P, long long N) {
  if (norm == RM_RANK_NORM_PAIRS) return 1.0 / (double)(kind == RM_RANK_PAIRWISE ? hd->pairs : hd->pos);
  const double den = (double)hd->weight * (double)P * (kind == RM_RANK_PAIRWISE ? (double)N : 1.0);
  return (double)n_g / den;
}

// dlogit_out at the example of a sorted position
__device__ __forceinline__ void write_example(unsigned example, float grad, float alpha, float grad_scale,
                                              const float *dlogit_in, float *dlogit_out) {
  float v = alpha * grad;
  if (dlogit_in) v = (1.0f - alpha) * dlogit_in[example] + v;
  dlogit_out[example] = grad_scale * v;
}

// What a thread of the pairwise kernels knows of its sorted position i: its example, class and logit, the
// opposite-class run [a, b) of its group (empty when the group is not scored) and c_g.
struct PairSide {
  unsigned example;
  bool positive;
  int a, b;
  float sx;
  double cd;
};

__device__ __forceinline__ PairSide pair_side(const RankHeader *__restrict__ hd, const unsigned *__restrict__ pay,
                                              const unsigned *__restrict__ slot_of, const float *__restrict__ ss,
                                              const unsigned *__restrict__ gs, const unsigned *__restrict__ gm,
                                              const unsigned *__restrict__ ge, int64_t i, int norm) {
  PairSide t{0u, false, 0x7FFFFFFF, 0, 0.f, 0.0};
  const unsigned py = pay[i], slot = slot_of[i];
  t.example = py & kExample;
  t.positive = py >> 31;
  t.sx = ss[i];
  const int s = (int)gs[slot], m = (int)gm[slot], e = (int)ge[slot];
  if (m > s && e > m) {
    t.a = t.positive ? s : m;
    t.b = t.positive ? m : e;
    t.cd = coef(hd, RM_RANK_PAIRWISE, norm, e - s, e - m, m - s);
  }
  return t;
}

// Thread t of block (x, y) owns sorted position i = 256 x + t; a positive walks its group's negatives [s, m), a
// negative its positives [m, e).  The blocks (x, 0 .. kSplits - 1) share the union [lo, hi) of their threads' runs,
// streamed through LDS kPairTile scores at a time: block (x, y) takes the tiles y, y + kSplits, .. (a tile none of its
// threads needs is skipped), so one long run - a few positives against a whole batch of negatives - is spread over
// kSplits blocks.  A thread reads the part of the tile inside its own run: the whole wave the same address when it
// shares a group (a broadcast), else a few short runs.  It leaves its sum of sigmoid(-d) over its tiles in
// pg[y][i] and its loss share in the block's partial; rank_pair_finish_kernel adds the splits in order.
__global__ __launch_bounds__(kThreads) void rank_pair_kernel(
    const RankHeader *__restrict__ hd, const unsigned *__restrict__ pay0, const unsigned *__restrict__ pay1,
    const unsigned *__restrict__ slot_of, const float *__restrict__ ss, const unsigned *__restrict__ gs,
    const unsigned *__restrict__ gm, const unsigned *__restrict__ ge, int64_t n, int norm, float *__restrict__ pg,
    double *__restrict__ lpart) {
  __shared__ float tile[kPairTile];
  __shared__ int smi[kWaves];
  __shared__ int bounds[2];
  __shared__ double smd[kWaves];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
  PairSide t{0u, false, 0x7FFFFFFF, 0, 0.f, 0.0};
  if (i < n) t = pair_side(hd, (hd->plan.m & 1) ? pay1 : pay0, slot_of, ss, gs, gm, ge, i, norm);
  const int a = t.a, b = t.b;
  const int lo = block_scan<false>(a, OpMin(), smi), hi = block_scan<false>(b, OpMax(), smi);
  if (tid == kThreads - 1) {
    bounds[0] = lo;
    bounds[1] = hi;
  }
  __syncthreads();
  const int blo = bounds[0], bhi = bounds[1];
  const float sgn = t.positive ? 1.0f : -1.0f, sx = t.sx;
  const bool positive = t.positive;
  double gsum = 0.0, lsum = 0.0;
  for (int64_t t0 = (int64_t)blo + (int64_t)blockIdx.y * kPairTile; t0 < bhi; t0 += (int64_t)kSplits * kPairTile) {
    const int ja = (int)(max((int64_t)a, t0) - t0), jb = (int)(min((int64_t)b, t0 + kPairTile) - t0);
    if (!__syncthreads_or(ja < jb)) continue;  // (also the barrier between two tiles)
    for (int k = tid; k < kPairTile; k += kThreads) tile[k] = t0 + k < bhi ? ss[t0 + k] : 0.f;
    __syncthreads();
    float gacc = 0.f, lacc = 0.f;
#pragma unroll 4
    for (int j = ja; j < jb; ++j) {
      const float d = sgn * (sx - tile[j]);  // positive minus negative
      // exp by the hardware's 2^x, the reciprocal by its rcp, log1p(e) as log(1 + e) for e >= 1/64 and as its
      // cubic e (1 - e (1/2 - e / 3)) below (relative error < e^3 / 4 < 1e-6): DESIGN.md says what this costs
      const float ex = __expf(-fabsf(d));
      const float r = __frcp_rn(1.0f + ex);
      gacc += d >= 0.f ? ex * r : r;  // sigmoid(-d)
      if (positive)
        lacc += fmaxf(-d, 0.f) +
                (ex < 0.015625f ? ex * (1.0f - ex * (0.5f - ex * (1.0f / 3.0f))) : __logf(1.0f + ex));
    }
    gsum += (double)gacc;
    lsum += (double)lacc;
  }
  if (i < n) pg[(int64_t)blockIdx.y * n + i] = (float)gsum;
  const double share = block_sum(t.cd * lsum, smd);
  if (tid == 0) lpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = share;
}

// The splits of a position's sum in order, in double; then its dL/ds and dlogit_out at its example.
__global__ __launch_bounds__(kThreads) void rank_pair_finish_kernel(
    const RankHeader *__restrict__ hd, const unsigned *__restrict__ pay0, const unsigned *__restrict__ pay1,
    const unsigned *__restrict__ slot_of, const float *__restrict__ ss, const unsigned *__restrict__ gs,
    const unsigned *__restrict__ gm, const unsigned *__restrict__ ge, int64_t n, int norm,
    const float *__restrict__ pg, float alpha, float grad_scale, const float *dlogit_in, float *dlogit_out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const PairSide t = pair_side(hd, (hd->plan.m & 1) ? pay1 : pay0, slot_of, ss, gs, gm, ge, i, norm);
  float grad = 0.f;  // (a position with an empty run keeps the exact +0.0: -1 * 0.0 would be -0.0)
  if (t.a < t.b) {
    double sum = 0.0;
#pragma unroll
    for (int y = 0; y < kSplits; ++y) sum += (double)pg[(int64_t)y * n + i];
    grad = (t.positive ? -1.0f : 1.0f) * ((float)t.cd * (float)sum);
  }
  write_example(t.example, grad, alpha, grad_scale, dlogit_in, dlogit_out);
}

__global__ __launch_bounds__(kThreads) void rank_list_kernel(
    const RankHeader *__restrict__ hd, const unsigned *__restrict__ pay0, const unsigned *__restrict__ pay1,
    const unsigned *__restrict__ slot_of, const float *__restrict__ ss, const unsigned *__restrict__ gs,
    const unsigned *__restrict__ gm, const unsigned *__restrict__ ge, const float *__restrict__ gmax,
    const double *__restrict__ gsum, int64_t n, int norm, float alpha, float grad_scale, const float *dlogit_in,
    float *dlogit_out, double *__restrict__ lpart) {
  __shared__ double smd[kWaves];
  const unsigned *pay = (hd->plan.m & 1) ? pay1 : pay0;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < n;
  unsigned example = 0u;
  float grad = 0.f;
  double share = 0.0;
  if (live) {
    const unsigned py = pay[i], slot = slot_of[i];
    example = py & kExample;
    const int s = (int)gs[slot], m = (int)gm[slot], e = (int)ge[slot];
    if (m > s && e > m) {
      const bool positive = py >> 31;
      const double cd = coef(hd, RM_RANK_LISTWISE, norm, e - s, e - m, m - s);
      const float sx = ss[i], mx = gmax[slot];
      const double sum = gsum[slot];
      const float soft = expf(sx - mx) / (float)sum;
      grad = (float)cd * ((float)(e - m) * soft - (positive ? 1.0f : 0.0f));
      if (positive) share = cd * (((double)mx - (double)sx) + log(sum));
    }
  }
  if (live) write_example(example, grad, alpha, grad_scale, dlogit_in, dlogit_out);
  share = block_sum(share, smd);
  if (threadIdx.x == 0) lpart[blockIdx.x] = share;
}

__global__ __launch_bounds__(kThreads) void rank_final_kernel(const RankHeader *__restrict__ hd, int64_t nb,
                                                              const double *__restrict__ lpart, float alpha,
                                                              const float *loss_in, float *loss_out,
                                                              rm_rank_result *__restrict__ out) {
  __shared__ double smd[kWaves];
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < nb; b += kThreads) acc += lpart[b];
  acc = block_sum(acc, smd);
  if (threadIdx.x == 0) {
    if (loss_out) {
      double v = (double)alpha * acc;
      if (loss_in) v += (1.0 - (double)alpha) * (double)loss_in[0];
      loss_out[0] = (float)v;
    }
    if (out) {
      out->value = acc;
      out->groups = (int64_t)hd->groups;
      out->scored_groups = hd->scored;
      out->pairs = hd->pairs;
      out->pos = hd->pos;
      out->weight = hd->weight;
      out->flags = (int64_t)hd->flags;
    }
  }
}

}  // namespace

extern "C" int64_t rm_rank_loss_workspace(int64_t B) {
  if (B < 1 || B > RM_RANK_MAX_B) return 0;
  return (int64_t)layout(B).total;
}

extern "C" int rm_rank_loss(const float *logit, const int64_t *y, const int64_t *groups, int64_t B, int kind,
                            int norm, float alpha, float grad_scale, const float *dlogit_in, float *dlogit_out,
                            const float *loss_in, float *loss_out, rm_rank_result *out, void *workspace,
                            rm_stream_t stream) {
  RM_REQUIRE(B >= 1 && B <= RM_RANK_MAX_B, "rm_rank_loss: B = %lld outside [1, 2^24]", (long long)B);
  RM_REQUIRE(kind == RM_RANK_PAIRWISE || kind == RM_RANK_LISTWISE, "rm_rank_loss: kind %d (0 pairwise, 1 listwise)",
             kind);
  RM_REQUIRE(norm == RM_RANK_NORM_PAIRS || norm == RM_RANK_NORM_GROUP, "rm_rank_loss: norm %d (0 pairs, 1 group)",
             norm);
  RM_REQUIRE(alpha > 0.f && alpha <= 1.f, "rm_rank_loss: alpha = %g outside (0, 1]", (double)alpha);
  RM_REQUIRE(isfinite(grad_scale), "rm_rank_loss: grad_scale is not finite");
  RM_REQUIRE(logit && y && dlogit_out && workspace, "rm_rank_loss: NULL pointer (logit, y, dlogit_out, workspace)");
  RM_REQUIRE(rm_aligned16(workspace) && rm_aligned16(out), "rm_rank_loss: workspace / out not 16-byte aligned");
  const int64_t n = B;
  const Layout L = layout(n);
  char *ws = (char *)workspace;
  RankHeader *hd = (RankHeader *)(ws + L.header);
  unsigned *hist = (unsigned *)(ws + L.hist), *cnt = (unsigned *)(ws + L.cnt);
  unsigned *g0 = (unsigned *)(ws + L.grp0), *g1 = (unsigned *)(ws + L.grp1);
  unsigned *p0 = (unsigned *)(ws + L.pay0), *p1 = (unsigned *)(ws + L.pay1);
  unsigned *slot_of = (unsigned *)(ws + L.slot);
  float *ss = (float *)(ws + L.ss);
  unsigned *gs = (unsigned *)(ws + L.gs), *gm = (unsigned *)(ws + L.gm), *ge = (unsigned *)(ws + L.ge);
  float *pm = (float *)(ws + L.pm), *ps = (float *)(ws + L.ps), *gmax = (float *)(ws + L.gmax);
  double *gsum = (double *)(ws + L.gsum), *lpart = (double *)(ws + L.lpart);
  float *pg = (float *)(ws + L.pg);
  long long *rq = (long long *)(ws + L.rq), *rp = (long long *)(ws + L.rp), *rw = (long long *)(ws + L.rw);
  long long *rs = (long long *)(ws + L.rs);
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t blocks = (int64_t)pair_blocks(n);
  const int nb = rm_grid_cap(blocks, kReduceBlocks);
  hipStream_t s = (hipStream_t)stream;

  if (hipMemsetAsync(hd, 0, sizeof(RankHeader), s) != hipSuccess) {
    rm_set_error("rm_rank_loss: hipMemsetAsync failed");
    return RM_ELAUNCH;
  }
  hipLaunchKernelGGL(rank_keys_kernel, dim3(rm_grid_cap(blocks, kKeyBlocks)), dim3(kThreads), 0, s, logit, y, groups,
                     n, g0, p0, hd);
  // (without ids only the label digit can vary: the four group passes are not enqueued at all)
  radix_sort<RankRecord>(&hd->plan, {{{g0, p0}, {g1, p1}}}, n, hist, s, groups ? RankRecord::kDigits : 1);
  hipLaunchKernelGGL(rank_marks_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, hd, g0, g1, n, cnt);
  hipLaunchKernelGGL(rank_carry_kernel, dim3(1), dim3(kThreads), 0, s, hd, tiles, cnt);
  hipLaunchKernelGGL(rank_bounds_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, hd, g0, g1, p0, p1, logit, n,
                     cnt, slot_of, ss, gs, gm, ge);
  if (kind == RM_RANK_LISTWISE) {
    hipLaunchKernelGGL(rank_pieces_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, slot_of, ss, n, pm, ps);
    hipLaunchKernelGGL(rank_groups_kernel<true>, dim3(nb), dim3(kThreads), 0, s, hd, gs, gm, ge, pm, ps, gmax, gsum,
                       rq, rp, rw, rs);
  } else {
    hipLaunchKernelGGL(rank_groups_kernel<false>, dim3(nb), dim3(kThreads), 0, s, hd, gs, gm, ge, pm, ps, gmax, gsum,
                       rq, rp, rw, rs);
  }
  hipLaunchKernelGGL(rank_totals_kernel, dim3(1), dim3(kThreads), 0, s, hd, nb, rq, rp, rw, rs);
  if (kind == RM_RANK_LISTWISE) {
    hipLaunchKernelGGL(rank_list_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, hd, p0, p1, slot_of, ss, gs, gm,
                       ge, gmax, gsum, n, norm, alpha, grad_scale, dlogit_in, dlogit_out, lpart);
  } else {
    hipLaunchKernelGGL(rank_pair_kernel, dim3((unsigned)blocks, kSplits), dim3(kThreads), 0, s, hd, p0, p1, slot_of,
                       ss, gs, gm, ge, n, norm, pg, lpart);
    hipLaunchKernelGGL(rank_pair_finish_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, hd, p0, p1, slot_of, ss,
                       gs, gm, ge, n, norm, pg, alpha, grad_scale, dlogit_in, dlogit_out);
  }
  hipLaunchKernelGGL(rank_final_kernel, dim3(1), dim3(kThreads), 0, s, hd,
                     kind == RM_RANK_LISTWISE ? blocks : blocks * kSplits, lpart, alpha, loss_in, loss_out, out);
  RM_CHECK_LAUNCH("rm_rank_loss");
  return RM_OK;
}
