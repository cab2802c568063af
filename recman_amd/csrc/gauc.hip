// Grouped AUC (GAUC, arXiv 1706.06978 section 6.2) of a prediction vector, on the device: the AUC inside each
// group (user), averaged over the groups that hold both classes, weighted by impressions or clicks; see
// recman_hip.h.  With the examples sorted by (group, score), [a, b) the sorted positions of a positive's tie
// group (equal group AND score) and s the first position of its group
//     2U_g = sum_{positives of g} (a + b + 1 - 2 s) - P_g (P_g + 1),   AUC_g = 2U_g / (2 P_g N_g)
// Every per-group quantity is an integer (2U_g in uint64); only the weighted mean is floating point: double,
// summed in group-id order by a fixed tree.  Kernels, in launch order:
//   grouped_keys_kernel   (rm_radix_sort.h, ascending) validate; score -> order-preserving uint32 key, label ->
//                         byte, group -> uint32; P; the eight digit histograms (four of the key, four of the
//                         group) in one read
//   radix_sort            (rm_radix_sort.h) the stable LSD radix sort of (key, group, label), score digits first,
//                         then group digits: its plan kernel, then (hist, scan, pass) per digit
//   gauc_marks_kernel     per tile of the sorted order: group starts (count, last), last tie-group start, first
//                         tie-group end
//   gauc_carry_kernel     over the tiles: the slot of each tile's first group (exclusive sum of the starts), and
//                         what crosses its edges - the last group / tie start before it (prefix max) and the
//                         first tie end after it (suffix min); the number of groups
//   gauc_zero_kernel      clears the per-group sums of the groups that exist
//   gauc_segments_kernel  per tile: a, b, s of every element, then one (n, P, sum) piece per group of the tile
//                         from a segmented scan over the threads; pieces are added to the group's slot with
//                         INTEGER atomics (a group that crosses tiles gets one piece per tile: order-free, exact)
//   gauc_reduce_kernel    per group AUC_g (double), w_g, scored or not; the optional int64 per-group outputs;
//                         per-block partials over contiguous ranges of slots (ascending group id)
//   gauc_final_kernel     fixed-order sum of the partials, the record
// No float atomics; nothing is read back by the host between the kernels.
#include <math.h>

#include "rm_radix_sort.h"

namespace {

constexpr int kReduceBlocks = 1024;

using GaucHeader = GroupedScoreHeader;  // groups: written by gauc_carry_kernel

struct Layout {
  size_t header, hist, cnt, lastg, lastt, firste, keys0, keys1, grp0, grp1, lab0, lab1, gid, gnp, gu;
  size_t rsum, rwt, rsc, rmin, rmax, total;
};

Layout layout(int64_t n) {
  const size_t tiles = (size_t)((n + kTile - 1) / kTile), un = (size_t)n;
  Layout L;
  size_t o = 0;
  L.header = take(o, sizeof(GaucHeader));
  L.hist = take(o, 4 * kRadix * tiles);
  L.cnt = take(o, 4 * tiles);
  L.lastg = take(o, 4 * tiles);
  L.lastt = take(o, 4 * tiles);
  L.firste = take(o, 4 * tiles);
  L.keys0 = take(o, 4 * un);
  L.keys1 = take(o, 4 * un);
  L.grp0 = take(o, 4 * un);
  L.grp1 = take(o, 4 * un);
  L.lab0 = take(o, un);
  L.lab1 = take(o, un);
  L.gid = take(o, 4 * un);
  L.gnp = take(o, 8 * un);
  L.gu = take(o, 8 * un);
  L.rsum = take(o, 8 * kReduceBlocks);
  L.rwt = take(o, 8 * kReduceBlocks);
  L.rsc = take(o, 8 * kReduceBlocks);
  L.rmin = take(o, 8 * kReduceBlocks);
  L.rmax = take(o, 8 * kReduceBlocks);
  L.total = o;
  return L;
}

// A tile of the sorted order in LDS with its two neighbours across the edges: sk / sg[1 + li].  Position i starts
// a group when i == 0 or its group id differs from i - 1's, a tie group when it starts a group or its key
// differs; it ends a tie group when i == n - 1 or i + 1 starts one.
struct TileEdges {
  bool first, last;  // the tile holds position 0 / n - 1
};

__device__ __forceinline__ TileEdges load_tile(const unsigned *__restrict__ keys, const unsigned *__restrict__ grp,
                                               int64_t n, int64_t c0, int valid, unsigned *sk, unsigned *sg) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int li = j * kThreads + tid;
    if (li < valid) {
      sk[1 + li] = keys[c0 + li];
      sg[1 + li] = grp[c0 + li];
    }
  }
  if (tid == 0 && c0 > 0) {
    sk[0] = keys[c0 - 1];
    sg[0] = grp[c0 - 1];
  }
  if (tid == 1 && c0 + valid < n) {
    sk[valid + 1] = keys[c0 + valid];
    sg[valid + 1] = grp[c0 + valid];
  }
  __syncthreads();
  return TileEdges{c0 == 0, c0 + valid == n};
}

// Thread t owns tile positions 16 t .. 16 t + 15.
__global__ __launch_bounds__(kThreads) void gauc_marks_kernel(
    const GaucHeader *__restrict__ hd, const unsigned *__restrict__ keys0, const unsigned *__restrict__ keys1,
    const unsigned *__restrict__ grp0, const unsigned *__restrict__ grp1, int64_t n, unsigned *__restrict__ cnt,
    int *__restrict__ lastg, int *__restrict__ lastt, unsigned *__restrict__ firste) {
  const int m = hd->plan.m;  // the sorted triples are in buffer m & 1
  __shared__ unsigned sk[kTile + 2], sg[kTile + 2];
  __shared__ int smi[kWaves];
  __shared__ unsigned smu[kWaves];
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int valid = (int)min((int64_t)kTile, n - c0);
  const TileEdges ed = load_tile((m & 1) ? keys1 : keys0, (m & 1) ? grp1 : grp0, n, c0, valid, sk, sg);

  unsigned c = 0u;
  int lg = -1, lt = -1;
  unsigned fe = kNoEnd;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    const int li = tid * kItems + q;
    if (li < valid) {
      const bool gs = (ed.first && li == 0) || sg[li + 1] != sg[li];
      const bool ts = gs || sk[li + 1] != sk[li];
      const bool te = (ed.last && li == valid - 1) || sg[li + 1] != sg[li + 2] || sk[li + 1] != sk[li + 2];
      c += gs;
      if (gs) lg = (int)(c0 + li);
      if (ts) lt = (int)(c0 + li);
      if (te && fe == kNoEnd) fe = (unsigned)(c0 + li + 1);
    }
  }
  c = block_sum(c, smu);
  // (max / min are order-free: a plain reduction through the scan helper's last / first thread)
  lg = block_scan<false>(lg, OpMax(), smi);
  lt = block_scan<false>(lt, OpMax(), smi);
  fe = block_scan<true>(fe, OpMin(), smu);
  if (tid == kThreads - 1) {
    cnt[blockIdx.x] = c;
    lastg[blockIdx.x] = lg;
    lastt[blockIdx.x] = lt;
  }
  if (tid == 0) firste[blockIdx.x] = fe;
}

// In place, over the tiles: cnt -> slot of the group open at the tile's start + 1 (exclusive sum of the group
// starts), lastg / lastt -> the last group / tie start BEFORE the tile, firste -> the first tie end AFTER it.
// Position 0 starts and position n - 1 ends a group, so each exists wherever it is needed.
__global__ __launch_bounds__(kThreads) void gauc_carry_kernel(GaucHeader *__restrict__ hd, int64_t tiles,
                                                              unsigned *__restrict__ cnt, int *__restrict__ lastg,
                                                              int *__restrict__ lastt,
                                                              unsigned *__restrict__ firste) {
  __shared__ int smi[kWaves];
  __shared__ unsigned smu[kWaves];
  __shared__ unsigned exe[kThreads];
  __shared__ int exg[kThreads], ext[kThreads];
  const int tid = threadIdx.x;
  const int64_t seg = (tiles + kThreads - 1) / kThreads;
  const int64_t lo = min((int64_t)tid * seg, tiles), hi = min(lo + seg, tiles);
  unsigned c = 0u;
  int lg = -1, lt = -1;
  unsigned fe = kNoEnd;
  for (int64_t t = lo; t < hi; ++t) {
    c += cnt[t];
    lg = max(lg, lastg[t]);
    lt = max(lt, lastt[t]);
    fe = min(fe, firste[t]);
  }
  const unsigned ic = block_scan<false>(c, OpAdd(), smu);
  const int ig = block_scan<false>(lg, OpMax(), smi);
  const int it = block_scan<false>(lt, OpMax(), smi);
  exe[tid] = block_scan<true>(fe, OpMin(), smu);
  __syncthreads();
  if (tid == kThreads - 1) hd->groups = ic;
  // exclusive values at this thread's first tile (a max has no inverse: the inclusive scan of the thread before)
  unsigned rc = ic - c;
  exg[tid] = ig;
  ext[tid] = it;
  __syncthreads();
  int rg = tid > 0 ? exg[tid - 1] : -1, rt = tid > 0 ? ext[tid - 1] : -1;
  for (int64_t t = lo; t < hi; ++t) {
    const unsigned ct = cnt[t];
    const int g = lastg[t], s = lastt[t];
    cnt[t] = rc;
    lastg[t] = rg;
    lastt[t] = rt;
    rc += ct;
    rg = max(rg, g);
    rt = max(rt, s);
  }
  unsigned re = tid + 1 < kThreads ? exe[tid + 1] : kNoEnd;
  for (int64_t t = hi - 1; t >= lo; --t) {
    const unsigned e = firste[t];
    firste[t] = re;
    re = min(re, e);
  }
}

__global__ __launch_bounds__(kThreads) void gauc_zero_kernel(const GaucHeader *__restrict__ hd,
                                                             unsigned long long *__restrict__ gnp,
                                                             unsigned long long *__restrict__ gu) {
  const int64_t G = hd->groups, stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < G; i += stride) {
    gnp[i] = 0ull;
    gu[i] = 0ull;
  }
}

// One piece (examples << 32 | positives, sum of a + b + 1 - 2 s over the positives) of a group.
struct Piece {
  unsigned long long np, u;
};

__device__ __forceinline__ void add_piece(unsigned long long *__restrict__ gnp, unsigned long long *__restrict__ gu,
                                          int64_t slot, Piece p) {
  if (p.np == 0ull) return;
  atomicAdd(&gnp[slot], p.np);
  if (p.u) atomicAdd(&gu[slot], p.u);
}

__global__ __launch_bounds__(kThreads) void gauc_segments_kernel(
    const GaucHeader *__restrict__ hd, const unsigned *__restrict__ keys0, const unsigned *__restrict__ keys1,
    const unsigned *__restrict__ grp0, const unsigned *__restrict__ grp1, const unsigned char *__restrict__ lab0,
    const unsigned char *__restrict__ lab1, int64_t n, const unsigned *__restrict__ cnt,
    const int *__restrict__ lastg, const int *__restrict__ lastt, const unsigned *__restrict__ firste,
    unsigned *__restrict__ gid, unsigned long long *__restrict__ gnp, unsigned long long *__restrict__ gu) {
  const int m = hd->plan.m;
  const unsigned char *lab = (m & 1) ? lab1 : lab0;
  __shared__ unsigned sk[kTile + 2], sg[kTile + 2];
  __shared__ int smi[kWaves];
  __shared__ unsigned smu[kWaves];
  __shared__ int exg[kThreads], ext[kThreads];
  __shared__ unsigned exe[kThreads], exc[kThreads];
  __shared__ unsigned long long xnp[kThreads], xu[kThreads];
  __shared__ unsigned long long wnp[kWaves], wu[kWaves];
  __shared__ unsigned wf[kWaves];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int valid = (int)min((int64_t)kTile, n - c0);
  const TileEdges ed = load_tile((m & 1) ? keys1 : keys0, (m & 1) ? grp1 : grp0, n, c0, valid, sk, sg);

  unsigned gbits = 0u, sbits = 0u, ebits = 0u, pbits = 0u, c = 0u;
  int lg = -1, lt = -1;
  unsigned fe = kNoEnd;
  {
    // the thread's 16 label bytes: positions c0 + 16 tid .. (16-byte aligned whenever whole)
    unsigned char y[kItems];
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
      const int li = tid * kItems + q;
      y[q] = li < valid ? lab[c0 + li] : (unsigned char)0;
    }
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
      const int li = tid * kItems + q;
      if (li < valid) {
        const bool gs = (ed.first && li == 0) || sg[li + 1] != sg[li];
        const bool ts = gs || sk[li + 1] != sk[li];
        const bool te = (ed.last && li == valid - 1) || sg[li + 1] != sg[li + 2] || sk[li + 1] != sk[li + 2];
        gbits |= (unsigned)gs << q;
        sbits |= (unsigned)ts << q;
        ebits |= (unsigned)te << q;
        pbits |= (unsigned)y[q] << q;
        c += gs;
        if (gs) lg = (int)(c0 + li);
        if (ts) lt = (int)(c0 + li);
        if (te && fe == kNoEnd) fe = (unsigned)(c0 + li + 1);
      }
    }
  }
  // what the threads before / after contribute, seeded with what crosses the tile's edges
  exc[tid] = block_scan<false>(c, OpAdd(), smu);
  exg[tid] = block_scan<false>(lg, OpMax(), smi);
  ext[tid] = block_scan<false>(lt, OpMax(), smi);
  exe[tid] = block_scan<true>(fe, OpMin(), smu);
  __syncthreads();
  const int64_t slot0 = (int64_t)cnt[blockIdx.x] - 1;  // slot of the group open at the tile's start
  int64_t slot = slot0 + (tid > 0 ? exc[tid - 1] : 0u);  // ... at this thread's start
  int run_s = max(lastg[blockIdx.x], tid > 0 ? exg[tid - 1] : -1);
  int run_a = max(lastt[blockIdx.x], tid > 0 ? ext[tid - 1] : -1);
  unsigned run_b = min(firste[blockIdx.x], tid + 1 < kThreads ? exe[tid + 1] : kNoEnd);

  unsigned b[kItems];
#pragma unroll
  for (int q = kItems - 1; q >= 0; --q) {
    if ((ebits >> q) & 1u) run_b = (unsigned)(c0 + tid * kItems + q + 1);
    b[q] = run_b;
  }
  // the thread's pieces: `head` closes the group open at its start (when a group starts inside the thread),
  // pieces between two starts inside the thread are whole, `run` is what stays open at its end
  Piece head{0ull, 0ull}, run{0ull, 0ull};
  bool seen = false;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    const int li = tid * kItems + q;
    if (li < valid) {
      const int i = (int)(c0 + li);
      if ((gbits >> q) & 1u) {
        if (!seen) {
          head = run;
          seen = true;
        } else {
          add_piece(gnp, gu, slot, run);
        }
        run = Piece{0ull, 0ull};
        ++slot;
        run_s = i;
        gid[slot] = sg[li + 1];
      }
      if ((sbits >> q) & 1u) run_a = i;
      const unsigned y = (pbits >> q) & 1u;
      run.np += (1ull << 32) | y;
      if (y) run.u += (unsigned long long)(run_a - run_s) + (unsigned long long)(b[q] - (unsigned)run_s) + 1ull;
    }
  }
  // inclusive segmented sum of `run` over the threads; a thread that saw a group start begins a segment
  Piece v = run;
  unsigned f = seen;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long np2 = __shfl_up(v.np, o, 64), u2 = __shfl_up(v.u, o, 64);
    const unsigned f2 = __shfl_up(f, o, 64);
    if (lane >= o) {
      if (!f) {
        v.np += np2;
        v.u += u2;
      }
      f |= f2;
    }
  }
  if (lane == 63) {
    wnp[w] = v.np;
    wu[w] = v.u;
    wf[w] = f;
  }
  __syncthreads();
  for (int i = w - 1; i >= 0 && !f; --i) {
    v.np += wnp[i];
    v.u += wu[i];
    f |= wf[i];
  }
  xnp[tid] = v.np;
  xu[tid] = v.u;
  __syncthreads();
  if (seen) {  // the group open at this thread's start ends here: the threads before + head
    Piece p = head;
    if (tid > 0) {
      p.np += xnp[tid - 1];
      p.u += xu[tid - 1];
    }
    add_piece(gnp, gu, slot0 + (tid > 0 ? exc[tid - 1] : 0u), p);
  }
  if (tid == kThreads - 1) add_piece(gnp, gu, slot0 + exc[kThreads - 1], v);  // what stays open at the tile's end
}

// Block k takes the slots [k chunk, (k + 1) chunk): ascending group id.  AUC_g in double from integers (three
// roundings), w_g AUC_g one more; the block's sum runs in a fixed order.
__global__ __launch_bounds__(kThreads) void gauc_reduce_kernel(
    const GaucHeader *__restrict__ hd, int weight_kind, const unsigned *__restrict__ gid,
    const unsigned long long *__restrict__ gnp, const unsigned long long *__restrict__ gu,
    int64_t *__restrict__ out_ids, int64_t *__restrict__ out_n, int64_t *__restrict__ out_pos,
    unsigned long long *__restrict__ out_2u, double *__restrict__ rsum, long long *__restrict__ rwt,
    long long *__restrict__ rsc, double *__restrict__ rmin, double *__restrict__ rmax) {
  __shared__ double smd[kWaves];
  __shared__ long long sml[kWaves];
  const int64_t G = hd->groups;
  const int64_t chunk = (G + gridDim.x - 1) / gridDim.x;
  const int64_t lo = min((int64_t)blockIdx.x * chunk, G), hi = min(lo + chunk, G);
  double acc = 0.0, lo_v = 2.0, hi_v = -1.0;
  long long wt = 0, sc = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const unsigned long long np = gnp[i];
    const unsigned long long ng = np >> 32, P = np & 0xFFFFFFFFull, N = ng - P;
    const unsigned long long two_u = gu[i] - P * (P + 1ull);
    if (out_ids) {
      out_ids[i] = (int64_t)gid[i];
      out_n[i] = (int64_t)ng;
      out_pos[i] = (int64_t)P;
      out_2u[i] = two_u;
    }
    if (P && N) {
      const double auc = (double)two_u / (double)(2ull * P * N);
      const long long wg = (long long)(weight_kind ? P : ng);
      acc += (double)wg * auc;
      wt += wg;
      ++sc;
      lo_v = fmin(lo_v, auc);
      hi_v = fmax(hi_v, auc);
    }
  }
  acc = block_sum(acc, smd);
  wt = block_sum(wt, sml);
  sc = block_sum(sc, sml);
  lo_v = block_scan<false>(lo_v, OpMin(), smd);
  hi_v = block_scan<false>(hi_v, OpMax(), smd);
  if (threadIdx.x == kThreads - 1) {
    rsum[blockIdx.x] = acc;
    rwt[blockIdx.x] = wt;
    rsc[blockIdx.x] = sc;
    rmin[blockIdx.x] = lo_v;
    rmax[blockIdx.x] = hi_v;
  }
}

__global__ __launch_bounds__(kThreads) void gauc_final_kernel(
    const GaucHeader *__restrict__ hd, int nb, const double *__restrict__ rsum, const long long *__restrict__ rwt,
    const long long *__restrict__ rsc, const double *__restrict__ rmin, const double *__restrict__ rmax,
    rm_group_auc_result *__restrict__ out) {
  __shared__ double smd[kWaves];
  __shared__ long long sml[kWaves];
  double acc = 0.0, lo_v = 2.0, hi_v = -1.0;
  long long wt = 0, sc = 0;
  for (int b = threadIdx.x; b < nb; b += kThreads) {
    acc += rsum[b];
    wt += rwt[b];
    sc += rsc[b];
    lo_v = fmin(lo_v, rmin[b]);
    hi_v = fmax(hi_v, rmax[b]);
  }
  acc = block_sum(acc, smd);
  wt = block_sum(wt, sml);
  sc = block_sum(sc, sml);
  lo_v = block_scan<false>(lo_v, OpMin(), smd);
  hi_v = block_scan<false>(hi_v, OpMax(), smd);
  if (threadIdx.x == kThreads - 1) {
    long long flags = hd->flags;
    double v;
    if (sc == 0) {
      flags |= RM_METRIC_ONE_CLASS;
      v = __builtin_nan("");
    } else {
      // a weighted mean lies between its smallest and largest term: the clamp only removes rounding (one scored
      // group, or every AUC_g equal, gives that value exactly)
      v = fmin(fmax(acc / (double)wt, lo_v), hi_v);
    }
    out->value = v;
    out->groups = (int64_t)hd->groups;
    out->scored_groups = sc;
    out->weight = wt;
    out->pos = (int64_t)hd->pos;
    out->flags = flags;
  }
}

}  // namespace

extern "C" int64_t rm_group_auc_workspace(int64_t n) {
  if (n < 1 || n > 0x7FFFFFFFll) return 0;
  return (int64_t)layout(n).total;
}

extern "C" int rm_group_auc(const float *scores, const int64_t *labels, const int64_t *groups, int64_t n,
                            int weight_kind, void *workspace, int64_t *group_ids, int64_t *group_n,
                            int64_t *group_pos, uint64_t *group_2u, rm_group_auc_result *out, rm_stream_t stream) {
  RM_REQUIRE(n >= 1 && n <= 0x7FFFFFFFll, "rm_group_auc: n = %lld outside [1, 2^31 - 1]", (long long)n);
  RM_REQUIRE(scores && labels && groups && workspace && out, "rm_group_auc: NULL pointer");
  RM_REQUIRE(weight_kind == 0 || weight_kind == 1, "rm_group_auc: weight_kind %d (0 impressions, 1 clicks)",
             weight_kind);
  const int outs = (group_ids != nullptr) + (group_n != nullptr) + (group_pos != nullptr) + (group_2u != nullptr);
  RM_REQUIRE(outs == 0 || outs == 4, "rm_group_auc: the four per-group arrays come together or not at all");
  RM_REQUIRE(rm_aligned16(workspace) && rm_aligned16(out), "rm_group_auc: workspace / out not 16-byte aligned");
  const Layout L = layout(n);
  char *ws = (char *)workspace;
  GaucHeader *hd = (GaucHeader *)(ws + L.header);
  unsigned *hist = (unsigned *)(ws + L.hist);
  unsigned *cnt = (unsigned *)(ws + L.cnt), *firste = (unsigned *)(ws + L.firste);
  int *lastg = (int *)(ws + L.lastg), *lastt = (int *)(ws + L.lastt);
  unsigned *k0 = (unsigned *)(ws + L.keys0), *k1 = (unsigned *)(ws + L.keys1);
  unsigned *g0 = (unsigned *)(ws + L.grp0), *g1 = (unsigned *)(ws + L.grp1);
  unsigned char *l0 = (unsigned char *)(ws + L.lab0), *l1 = (unsigned char *)(ws + L.lab1);
  unsigned *gid = (unsigned *)(ws + L.gid);
  unsigned long long *gnp = (unsigned long long *)(ws + L.gnp), *gu = (unsigned long long *)(ws + L.gu);
  double *rsum = (double *)(ws + L.rsum), *rmin = (double *)(ws + L.rmin), *rmax = (double *)(ws + L.rmax);
  long long *rwt = (long long *)(ws + L.rwt), *rsc = (long long *)(ws + L.rsc);
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int nb = rm_grid_cap((n + kThreads - 1) / kThreads, kReduceBlocks);
  hipStream_t s = (hipStream_t)stream;

  if (hipMemsetAsync(hd, 0, sizeof(GaucHeader), s) != hipSuccess) {
    rm_set_error("rm_group_auc: hipMemsetAsync failed");
    return RM_ELAUNCH;
  }
  hipLaunchKernelGGL(grouped_keys_kernel<false>, dim3(rm_grid_cap((n + kThreads - 1) / kThreads, kKeyBlocks)),
                     dim3(kThreads), 0, s, scores, labels, groups, n, k0, g0, l0, hd);
  radix_sort<GroupedScoreRecord>(&hd->plan, {{{k0, g0}, {k1, g1}}, {l0, l1}}, n, hist, s);
  hipLaunchKernelGGL(gauc_marks_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, hd, k0, k1, g0, g1, n, cnt,
                     lastg, lastt, firste);
  hipLaunchKernelGGL(gauc_carry_kernel, dim3(1), dim3(kThreads), 0, s, hd, tiles, cnt, lastg, lastt, firste);
  hipLaunchKernelGGL(gauc_zero_kernel, dim3(nb), dim3(kThreads), 0, s, hd, gnp, gu);
  hipLaunchKernelGGL(gauc_segments_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, s, hd, k0, k1, g0, g1, l0,
                     l1, n, cnt, lastg, lastt, firste, gid, gnp, gu);
  hipLaunchKernelGGL(gauc_reduce_kernel, dim3(nb), dim3(kThreads), 0, s, hd, weight_kind, gid, gnp, gu, group_ids,
                     group_n, group_pos, (unsigned long long *)group_2u, rsum, rwt, rsc, rmin, rmax);
  hipLaunchKernelGGL(gauc_final_kernel, dim3(1), dim3(kThreads), 0, s, hd, nb, rsum, rwt, rsc, rmin, rmax, out);
  RM_CHECK_LAUNCH("rm_group_auc");
  return RM_OK;
}
