// Grouped top-k ranking metrics (NDCG@k, recall@k, precision@k) of a prediction vector, on the device: any top-k
// measure that is linear in the labels, exact under ties, for up to RM_GAIN_MAX_CUTOFFS cutoffs in one sort; see
// recman_hip_rankmetrics.h.  With the examples sorted by (group ascending, score descending) a group is a contiguous
// run [s, e), the rank of position i is i - s, and with L the exclusive prefix count of the sorted labels a tie group
// at ranks [lo, hi) holds pos_T = L[s + hi] - L[s + lo] positives and the group P_g = L[e] - L[s]:
//     gain_g(k) = sum_{T, lo < k} (pos_T / (hi - lo)) (disc[lo] + ... + disc[min(hi, k) - 1])
// Kernels, in launch order:
//   grouped_keys_kernel   (rm_radix_sort.h, descending) validate; score -> ~(order-preserving uint32 key), so that
//                         ascending is score descending; label -> byte, group -> uint32 (0 when there is no id
//                         column); P; the eight digit histograms
//   radix_sort            (rm_radix_sort.h) the stable LSD radix sort of (key, group, label), score digits first, then
//                         group digits: its plan kernel, then (hist, scan, pass) per digit
//   gain_count_kernel     per tile of the sorted order: its group starts and its positives
//   gain_carry_kernel     over the tiles: exclusive sums of both; the number of groups
//   gain_starts_kernel    per tile: the start position and id of every group (slot = ascending id) and L
//   gain_groups_kernel    one thread per group: walks the tie groups of the first min(n_g, kmax) ranks (a tie group
//                         that runs past them ends where a bisection of the group's sorted keys says), adds disc
//                         (staged in LDS) entry by entry, the terms in rank order; value_g per cutoff; the optional
//                         per-group outputs; per-block partials over contiguous ranges of slots
//   gain_final_kernel     fixed-order sum of the partials, the record
// Only counts are read from inside a tie group, and every sum is a fixed function of the sorted position: no float
// atomics, bit-equal runs, independent of the input order.  Nothing is read back by the host between the kernels.
#include <math.h>

#include "../../include/recman_hip_rankmetrics.h"
#include "rm_radix_sort.h"

namespace {

constexpr int kReduceBlocks = 1024;
constexpr int kCut = RM_GAIN_MAX_CUTOFFS;

using GainHeader = GroupedScoreHeader;  // groups: written by gain_carry_kernel

// the cutoffs (k[c] = 0 past n_cut: no rank reaches it) and the three choices, by value
struct GainParams {
  int k[kCut];
  int n_cut, kmax, norm, rule, weight;
};

struct Layout {
  size_t header, hist, tcnt, tpos, keys0, keys1, grp0, grp1, lab0, lab1, gstart, gid, lpre, rsum, rwt, rsc, total;
};

Layout layout(int64_t n) {
  const size_t tiles = (size_t)((n + kTile - 1) / kTile), un = (size_t)n;
  Layout L;
  size_t o = 0;
  L.header = take(o, sizeof(GainHeader));
  L.hist = take(o, 4 * kRadix * tiles);
  L.tcnt = take(o, 4 * tiles);
  L.tpos = take(o, 4 * tiles);
  L.keys0 = take(o, 4 * un);
  L.keys1 = take(o, 4 * un);
  L.grp0 = take(o, 4 * un);
  L.grp1 = take(o, 4 * un);
  L.lab0 = take(o, un);
  L.lab1 = take(o, un);
  L.gstart = take(o, 4 * (un + 1));
  L.gid = take(o, 4 * un);
  L.lpre = take(o, 4 * (un + 1));
  L.rsum = take(o, 8 * kCut * kReduceBlocks);
  L.rwt = take(o, 8 * kReduceBlocks);
  L.rsc = take(o, 8 * kReduceBlocks);
  L.total = o;
  return L;
}

// Position i of the sorted order starts a group when i == 0 or its group id differs from i - 1's.
__global__ __launch_bounds__(kThreads) void gain_count_kernel(
    const GainHeader *__restrict__ hd, const unsigned *__restrict__ grp0, const unsigned *__restrict__ grp1,
    const unsigned char *__restrict__ lab0, const unsigned char *__restrict__ lab1, int64_t n,
    unsigned *__restrict__ tcnt, unsigned *__restrict__ tpos) {
  const int m = hd->plan.m;  // the sorted triples are in buffer m & 1
  const unsigned *grp = (m & 1) ? grp1 : grp0;
  const unsigned char *lab = (m & 1) ? lab1 : lab0;
  __shared__ unsigned sm[kWaves];
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  unsigned c = 0u, p = 0u;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int64_t i = c0 + j * kThreads + threadIdx.x;
    if (i < n) {
      c += (i == 0 || grp[i] != grp[i - 1]);
      p += lab[i];
    }
  }
  c = block_sum(c, sm);
  p = block_sum(p, sm);
  if (threadIdx.x == 0) {
    tcnt[blockIdx.x] = c;
    tpos[blockIdx.x] = p;
  }
}

// In place, over the tiles: tcnt -> group starts before the tile, tpos -> positives before the tile.
__global__ __launch_bounds__(kThreads) void gain_carry_kernel(GainHeader *__restrict__ hd, int64_t tiles,
                                                              unsigned *__restrict__ tcnt,
                                                              unsigned *__restrict__ tpos) {
  __shared__ unsigned sm[kWaves];
  const unsigned ic = scan_row(tcnt, tiles, 0u, sm);
  scan_row(tpos, tiles, 0u, sm);
  if (threadIdx.x == kThreads - 1) hd->groups = ic;
}

// Thread t owns tile positions 16 t .. 16 t + 15.  gstart[slot] / gid[slot]: the first position and the id of the
// slot-th group; gstart[groups] = n.  lpre[i]: positives at the sorted positions before i; lpre[n] = P.
__global__ __launch_bounds__(kThreads) void gain_starts_kernel(
    const GainHeader *__restrict__ hd, const unsigned *__restrict__ grp0, const unsigned *__restrict__ grp1,
    const unsigned char *__restrict__ lab0, const unsigned char *__restrict__ lab1, int64_t n,
    const unsigned *__restrict__ tcnt, const unsigned *__restrict__ tpos, unsigned *__restrict__ gstart,
    unsigned *__restrict__ gid, unsigned *__restrict__ lpre) {
  const int m = hd->plan.m;
  const unsigned *grp = (m & 1) ? grp1 : grp0;
  const unsigned char *lab = (m & 1) ? lab1 : lab0;
  __shared__ unsigned sm[kWaves];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kTile + tid * kItems;
  unsigned g[kItems], gbits = 0u, pbits = 0u, c = 0u, p = 0u;
  unsigned prev = (i0 > 0 && i0 < n) ? grp[i0 - 1] : 0u;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    const int64_t i = i0 + q;
    g[q] = 0u;
    if (i < n) {
      g[q] = grp[i];
      const unsigned gs = (i == 0 || g[q] != prev), y = lab[i];
      prev = g[q];
      gbits |= gs << q;
      pbits |= y << q;
      c += gs;
      p += y;
    }
  }
  unsigned slot = tcnt[blockIdx.x] + block_scan<false>(c, OpAdd(), sm) - c;
  unsigned pre = tpos[blockIdx.x] + block_scan<false>(p, OpAdd(), sm) - p;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    const int64_t i = i0 + q;
    if (i < n) {
      if ((gbits >> q) & 1u) {
        gstart[slot] = (unsigned)i;
        gid[slot] = g[q];
        ++slot;
      }
      lpre[i] = pre;
      pre += (pbits >> q) & 1u;
      if (i == n - 1) {
        gstart[slot] = (unsigned)n;
        lpre[n] = pre;
      }
    }
  }
}

// Block b takes the slots [b chunk, (b + 1) chunk): ascending group id, one thread per group.  Roundings of
// value_g(k): pos_T / len (1), a range sum of at most k non-negative entries (k - 1), the product (1), at most k
// terms of a group (k - 1), the ideal sum (k - 1), the division (1): (3k + 8) 2^-53 covers them.
__global__ __launch_bounds__(kThreads) void gain_groups_kernel(
    const GainHeader *__restrict__ hd, const GainParams pr, const unsigned *__restrict__ keys0,
    const unsigned *__restrict__ keys1, const unsigned *__restrict__ gstart, const unsigned *__restrict__ gid,
    const unsigned *__restrict__ lpre, const double *__restrict__ disc, int64_t *__restrict__ out_ids,
    int64_t *__restrict__ out_n, int64_t *__restrict__ out_pos, double *__restrict__ out_val,
    double *__restrict__ rsum, long long *__restrict__ rwt, long long *__restrict__ rsc) {
  __shared__ double smd[kWaves];
  __shared__ long long sml[kWaves];
  __shared__ double sdisc[RM_GAIN_MAX_K];  // the discounts of the ranks that count
  const unsigned *keys = (hd->plan.m & 1) ? keys1 : keys0;
  const int64_t G = hd->groups;
  const int64_t chunk = (G + gridDim.x - 1) / gridDim.x;
  const int64_t lo = min((int64_t)blockIdx.x * chunk, G), hi = min(lo + chunk, G);
  const unsigned kmax = (unsigned)pr.kmax;
  for (unsigned r = threadIdx.x; r < kmax; r += kThreads) sdisc[r] = disc[r];
  __syncthreads();
  double sum[kCut];
#pragma unroll
  for (int c = 0; c < kCut; ++c) sum[c] = 0.0;
  long long wt = 0, sc = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const unsigned s = gstart[i], e = gstart[i + 1], ng = e - s;
    const unsigned ps = lpre[s], P = lpre[e] - ps;
    const unsigned limit = min(ng, kmax);
    double acc[kCut], nrm[kCut];
#pragma unroll
    for (int c = 0; c < kCut; ++c) {
      acc[c] = 0.0;
      nrm[c] = pr.norm == RM_GAIN_NORM_POSITIVES ? (double)P : pr.norm == RM_GAIN_NORM_K ? (double)pr.k[c] : 0.0;
    }
    if (P) {
      // la = L at the tie group's start; the key and L at s + b are loaded together, one round trip per rank
      unsigned a = 0u, key = keys[s], la = ps;
      while (a < limit) {
        unsigned b = a + 1u, nk = 0u, lb = 0u;
        for (;;) {
          const bool inside = b < ng;
          if (inside) nk = keys[s + b];
          lb = lpre[s + b];
          if (!inside || b >= limit || nk != key) break;
          ++b;
        }
        if (b == limit && b < ng && nk == key) {
          // the tie group runs past the last rank that counts: its end is the first other key of the group
          unsigned l = b + 1u, h = ng;
          while (l < h) {
            const unsigned mid = l + ((h - l) >> 1);
            if (keys[s + mid] == key) {
              l = mid + 1u;
            } else {
              h = mid;
            }
          }
          b = l;
          lb = lpre[s + b];
        }
        const unsigned pos_t = lb - la;
        if (pos_t) {
          const double frac = (double)pos_t / (double)(b - a);
          const unsigned top = min(b, kmax);
          double rs = 0.0;
          for (unsigned r = a; r < top; ++r) {
            rs += sdisc[r];
#pragma unroll
            for (int c = 0; c < kCut; ++c)
              if (r + 1u == min(b, (unsigned)pr.k[c])) acc[c] += frac * rs;
          }
        }
        a = b;
        key = nk;
        la = lb;
      }
      if (pr.norm == RM_GAIN_NORM_IDEAL) {
        const unsigned top = min(P, kmax);
        double rs = 0.0;
        for (unsigned r = 0u; r < top; ++r) {
          rs += sdisc[r];
#pragma unroll
          for (int c = 0; c < kCut; ++c)
            if (r + 1u == min(P, (unsigned)pr.k[c])) nrm[c] = rs;
        }
      }
    }
    const bool scored = pr.rule == RM_GAIN_SCORED_HAS_POSITIVE ? P > 0u : (P > 0u && P < ng);
    const long long wg = pr.weight == RM_GAIN_WEIGHT_GROUPS ? 1ll : (long long)(pr.weight == RM_GAIN_WEIGHT_CLICKS ? P : ng);
    if (out_ids) {
      out_ids[i] = (int64_t)gid[i];
      out_n[i] = (int64_t)ng;
      out_pos[i] = (int64_t)P;
    }
#pragma unroll
    for (int c = 0; c < kCut; ++c) {
      const double v = nrm[c] > 0.0 ? acc[c] / nrm[c] : 0.0;
      if (out_val && c < pr.n_cut) out_val[i * pr.n_cut + c] = v;
      if (scored) sum[c] += (double)wg * v;
    }
    if (scored) {
      wt += wg;
      ++sc;
    }
  }
#pragma unroll
  for (int c = 0; c < kCut; ++c) {
    const double t = block_sum(sum[c], smd);
    if (threadIdx.x == 0) rsum[(int64_t)blockIdx.x * kCut + c] = t;
  }
  wt = block_sum(wt, sml);
  sc = block_sum(sc, sml);
  if (threadIdx.x == 0) {
    rwt[blockIdx.x] = wt;
    rsc[blockIdx.x] = sc;
  }
}

__global__ __launch_bounds__(kThreads) void gain_final_kernel(const GainHeader *__restrict__ hd, int nb, int n_cut,
                                                              const double *__restrict__ rsum,
                                                              const long long *__restrict__ rwt,
                                                              const long long *__restrict__ rsc,
                                                              rm_group_gain_result *__restrict__ out) {
  __shared__ double smd[kWaves];
  __shared__ long long sml[kWaves];
  double acc[kCut];
#pragma unroll
  for (int c = 0; c < kCut; ++c) acc[c] = 0.0;
  long long wt = 0, sc = 0;
  for (int b = threadIdx.x; b < nb; b += kThreads) {
#pragma unroll
    for (int c = 0; c < kCut; ++c) acc[c] += rsum[(int64_t)b * kCut + c];
    wt += rwt[b];
    sc += rsc[b];
  }
#pragma unroll
  for (int c = 0; c < kCut; ++c) acc[c] = block_sum(acc[c], smd);
  wt = block_sum(wt, sml);
  sc = block_sum(sc, sml);
  if (threadIdx.x == 0) {
    long long flags = hd->flags;
    if (sc == 0) flags |= RM_METRIC_ONE_CLASS;
#pragma unroll
    for (int c = 0; c < kCut; ++c)
      out->value[c] = (sc == 0 || c >= n_cut) ? __builtin_nan("") : acc[c] / (double)wt;
    out->groups = (int64_t)hd->groups;
    out->scored_groups = sc;
    out->weight = wt;
    out->pos = (int64_t)hd->pos;
    out->flags = flags;
  }
}

}  // namespace

extern "C" int64_t rm_group_gain_workspace(int64_t n) {
  if (n < 1 || n > 0x7FFFFFFFll) return 0;
  return (int64_t)layout(n).total;
}

extern "C" int rm_group_gain(const float *scores, const int64_t *labels, const int64_t *groups, int64_t n,
                             const double *disc, const int *cutoffs, int n_cutoffs, int norm, int scored_rule,
                             int weight_kind, void *workspace, int64_t *group_ids, int64_t *group_n,
                             int64_t *group_pos, double *group_value, rm_group_gain_result *out, rm_stream_t stream) {
  RM_REQUIRE(n >= 1 && n <= 0x7FFFFFFFll, "rm_group_gain: n = %lld outside [1, 2^31 - 1]", (long long)n);
  RM_REQUIRE(scores && labels && disc && cutoffs && workspace && out, "rm_group_gain: NULL pointer");
  RM_REQUIRE(n_cutoffs >= 1 && n_cutoffs <= RM_GAIN_MAX_CUTOFFS, "rm_group_gain: n_cutoffs = %d outside [1, %d]",
             n_cutoffs, RM_GAIN_MAX_CUTOFFS);
  GainParams pr;
  for (int c = 0; c < kCut; ++c) pr.k[c] = 0;
  for (int c = 0; c < n_cutoffs; ++c) {
    RM_REQUIRE(cutoffs[c] >= 1 && cutoffs[c] <= RM_GAIN_MAX_K, "rm_group_gain: cutoff %d outside [1, %d]",
               cutoffs[c], RM_GAIN_MAX_K);
    RM_REQUIRE(c == 0 || cutoffs[c] > cutoffs[c - 1], "rm_group_gain: cutoffs must be strictly ascending");
    pr.k[c] = cutoffs[c];
  }
  RM_REQUIRE(norm == RM_GAIN_NORM_IDEAL || norm == RM_GAIN_NORM_POSITIVES || norm == RM_GAIN_NORM_K,
             "rm_group_gain: norm %d (0 ideal, 1 positives, 2 k)", norm);
  RM_REQUIRE(scored_rule == RM_GAIN_SCORED_BOTH_CLASSES || scored_rule == RM_GAIN_SCORED_HAS_POSITIVE,
             "rm_group_gain: scored_rule %d (0 both classes, 1 has a positive)", scored_rule);
  RM_REQUIRE(weight_kind == RM_GAIN_WEIGHT_GROUPS || weight_kind == RM_GAIN_WEIGHT_IMPRESSIONS ||
                 weight_kind == RM_GAIN_WEIGHT_CLICKS,
             "rm_group_gain: weight_kind %d (0 groups, 1 impressions, 2 clicks)", weight_kind);
  const int outs =
      (group_ids != nullptr) + (group_n != nullptr) + (group_pos != nullptr) + (group_value != nullptr);
  RM_REQUIRE(outs == 0 || outs == 4, "rm_group_gain: the four per-group arrays come together or not at all");
  RM_REQUIRE(rm_aligned16(workspace) && rm_aligned16(out), "rm_group_gain: workspace / out not 16-byte aligned");
  pr.n_cut = n_cutoffs;
  pr.kmax = cutoffs[n_cutoffs - 1];
  pr.norm = norm;
  pr.rule = scored_rule;
  pr.weight = weight_kind;
  const Layout L = layout(n);
  char *ws = (char *)workspace;
  GainHeader *hd = (GainHeader *)(ws + L.header);
  unsigned *hist = (unsigned *)(ws + L.hist);
  unsigned *tcnt = (unsigned *)(ws + L.tcnt), *tpos = (unsigned *)(ws + L.tpos);
  unsigned *k0 = (unsigned *)(ws + L.keys0), *k1 = (unsigned *)(ws + L.keys1);
  unsigned *g0 = (unsigned *)(ws + L.grp0), *g1 = (unsigned *)(ws + L.grp1);
  unsigned char *l0 = (unsigned char *)(ws + L.lab0), *l1 = (unsigned char *)(ws + L.lab1);
  unsigned *gstart = (unsigned *)(ws + L.gstart), *gid = (unsigned *)(ws + L.gid), *lpre = (unsigned *)(ws + L.lpre);
  double *rsum = (double *)(ws + L.rsum);
  long long *rwt = (long long *)(ws + L.rwt), *rsc = (long long *)(ws + L.rsc);
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int nb = rm_grid_cap((n + kThreads - 1) / kThreads, kReduceBlocks);
  hipStream_t s = (hipStream_t)stream;

  if (hipMemsetAsync(hd, 0, sizeof(GainHeader), s) != hipSuccess) {
    rm_set_error("rm_group_gain: hipMemsetAsync failed");
    return RM_ELAUNCH;
  }
  hipLaunchKernelGGL(grouped_keys_kernel<true>, dim3(rm_grid_cap((n + kThreads - 1) / kThreads, kKeyBlocks)),
                     dim3(kThreads), 0, s, scores, labels, groups, n, k0, g0, l0, hd);
  radix_sort<GroupedScoreRecord>(&hd->plan, {{{k0, g0}, {k1, g1}}, {l0, l1}}, n, hist, s);
  hipLaunchKernelGGL(gain_count_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, hd, g0, g1, l0, l1, n, tcnt,
                     tpos);
  hipLaunchKernelGGL(gain_carry_kernel, dim3(1), dim3(kThreads), 0, s, hd, tiles, tcnt, tpos);
  hipLaunchKernelGGL(gain_starts_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, hd, g0, g1, l0, l1, n, tcnt,
                     tpos, gstart, gid, lpre);
  hipLaunchKernelGGL(gain_groups_kernel, dim3(nb), dim3(kThreads), 0, s, hd, pr, k0, k1, gstart, gid, lpre, disc,
                     group_ids, group_n, group_pos, group_value, rsum, rwt, rsc);
  hipLaunchKernelGGL(gain_final_kernel, dim3(1), dim3(kThreads), 0, s, hd, nb, n_cutoffs, rsum, rwt, rsc, out);
  RM_CHECK_LAUNCH("rm_group_gain");
  return RM_OK;
}
