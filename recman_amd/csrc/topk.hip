// Exact top-k retrieval by inner product over an item catalogue (see recman_hip_topk.h).  Nothing in the reference
// implements it.
//
// The [Nq, N] scores never reach HBM.  Two kernels:
//   stage 1 (topk_scan_kernel)   grid = query tiles x splits.  A block owns 64 query rows in registers (4 waves x 16)
//       and streams its split's contiguous range of catalogue tiles through double-buffered LDS on the exact-f32 MFMA
//       (v_mfma_f32_16x16x4_f32), the layout of inbatch.hip's score kernels: the query rows are the B operand (lane l
//       holds Q[l & 15][4 kk + (l >> 4)]), the tile is computed TRANSPOSED, so accumulator register r of lane l holds
//       (catalogue row 4 (l >> 4) + r of the 16-row sub-tile, query l & 15): a lane's query is fixed and the query's
//       threshold tau is one register (the same in its four lanes).
//       Each score becomes a 64-bit key (score_key(s) << 32) | (0xFFFFFFFF - row), NaN mapped to score key 0: one
//       unsigned compare applies the whole order (score descending, row ascending, NaN last), and keys are unique.
//       A key above tau that a binary search of the query's exclusion list (only on this rare path) does not reject
//       is appended to the (query, split) list in the workspace; its count lives in LDS (the block owns the pair, a
//       wave its 16 queries: no global atomics).  The list holds cap = 2 max(64, pow2(k)) keys; before a tile that
//       could overflow it (count > cap - tile rows), the wave selects the k-th key in LDS (bit by bit from the top:
//       counts of the keys at or above a candidate), keeps the best k, unordered, and raises tau to that key.  After
//       the last tile every list is sorted (bitonic in LDS, wave-synchronous) and cut to <= k keys.
//   stage 2 (topk_merge_kernel)  a block per query merges the splits' sorted lists in split order: an entry's place
//       in the merge of two sorted lists is its own index plus the number of keys above it in the other list (keys
//       are unique), so each merge step is one binary search per entry, in LDS.
// A pair's score is the same MFMA chain over the same k-steps wherever it is computed: the result does not depend on
// item_splits or on the run.
#include "rm_launch.h"
#include "rm_metric_common.h"  // score_key, kThreads = 256

#include "../../include/recman_hip_topk.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kQRows = 64;        // query rows per block (4 waves x 16)
constexpr int kTkMaxSplits = 64;
constexpr int kTkMaxK = 1024;
constexpr int kTkFill = 512;      // the library's split choice aims at two blocks on each of the 256 CUs
constexpr int kMergeBlocks = 256 * 16;
constexpr int64_t kTkMaxRows = ((int64_t)1 << 31) - 1;  // N
constexpr int64_t kTkMaxQueries = (int64_t)1 << 30;    // Nq (query indices stay ints)

// the template width (k-steps of 4) that holds H: HP = 4 NK
inline int tk_nk(int H) {
  const int widths[] = {4, 8, 12, 16, 24, 32, 48, 64};
  for (int nk : widths)
    if (4 * nk >= H) return nk;
  return -1;
}
inline int tk_cols(int nk) { return 4 * nk <= 128 ? 64 : 32; }
inline int64_t tk_tiles(int64_t N, int cols) { return (N + cols - 1) / cols; }
// keys a (query, split) list holds: at least k + a tile's rows (64) after a cut, a power of two for the sort
inline int tk_cap(int k) {
  int p = 64;
  while (p < k) p <<= 1;
  return 2 * p;
}
inline bool tk_supported(int H, int k) { return H >= 4 && H <= 256 && H % 4 == 0 && k >= 1 && k <= kTkMaxK; }

// the split count launched: item_splits (0: enough blocks to fill the device), never above the catalogue's tiles
inline int tk_splits(int64_t Nq, int64_t N, int cols, int item_splits) {
  int64_t s = item_splits;
  if (s == 0) {
    const int64_t qt = (Nq + kQRows - 1) / kQRows;
    s = (kTkFill + qt - 1) / qt;
    if (s > kTkMaxSplits) s = kTkMaxSplits;
  }
  const int64_t tiles = tk_tiles(N, cols);
  if (s > tiles) s = tiles;
  return (int)(s < 1 ? 1 : s);
}

// workspace, in floats: the lists [Nq, S, cap] of u64 keys, then the counts [Nq, S] int32; S = the largest split
// count tk_splits can return for N
inline int64_t tk_max_splits(int64_t N, int cols) {
  const int64_t t = tk_tiles(N, cols);
  return t < 1 ? 1 : (t < kTkMaxSplits ? t : kTkMaxSplits);
}
inline int64_t tk_ws_floats(int64_t Nq, int64_t N, int H, int k) {
  const int64_t lists = Nq * tk_max_splits(N, tk_cols(tk_nk(H)));
  return 2 * lists * tk_cap(k) + (lists + 3) / 4 * 4;
}

struct TkArgs {
  const float *Q;  // [Nq, ldq]
  int64_t ldq;
  const float *C;  // [N, ldc]
  int64_t ldc;
  int Nq, N, H;
  float scale;
  int k, cap;
  const int64_t *eoff, *erows;  // or NULL
  int tiles_per_split, splits;
  u64 *lists;
  int *counts;
};

__device__ __forceinline__ u64 tk_key(float s, unsigned row) {
  const unsigned k32 = s != s ? 0u : score_key(s);
  return ((u64)k32 << 32) | (u64)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ float tk_key_score(u64 key) {
  const unsigned k32 = (unsigned)(key >> 32);
  if (k32 == 0u) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k32 & 0x80000000u) ? (k32 & 0x7FFFFFFFu) : ~k32);
}
__device__ __forceinline__ int64_t tk_key_row(u64 key) { return (int64_t)(0xFFFFFFFFu - (unsigned)key); }

// the lanes of one wave: what one lane wrote (LDS or global) is seen by the others after it
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// bitonic sort of s[0, P) descending by one wave (P a power of two >= 2)
__device__ void wave_sort_desc(u64 *s, int P, int lane) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = lane; i < P / 2; i += 64) {
        const int pos = 2 * i - (i & (stride - 1)), oth = pos + stride;
        const u64 x = s[pos], y = s[oth];
        const bool desc = (pos & size) == 0;
        if (desc ? x < y : x > y) {
          s[pos] = y;
          s[oth] = x;
        }
      }
      wave_sync();
    }
  }
}

// the number of keys above `key` in the descending arr[0, n)
__device__ __forceinline__ int count_above(const u64 *arr, int n, u64 key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (arr[mid] > key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <int NK>
__global__ __launch_bounds__(kThreads, 2) void topk_scan_kernel(TkArgs a) {
  constexpr int HP = 4 * NK, LDV = HP + 4, COLS = HP <= 128 ? 64 : 32;
  constexpr int NPF = COLS * NK / kThreads;  // float4 loads per thread and tile
  extern __shared__ float smem[];
  // LDS: two tiles, the 64 list counts, per wave a sort buffer of cap keys
  float *const tiles = smem;
  int *const scnt = reinterpret_cast<int *>(smem + 2 * COLS * LDV);
  u64 *const sorts = reinterpret_cast<u64 *>(scnt + kQRows);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
  const int N = a.N, H = a.H, split = blockIdx.y;
  const int q0 = blockIdx.x * kQRows + wave * 16;  // the wave's first query
  const int own = q0 + lo;
  const bool own_ok = own < a.Nq;
  const int64_t ntiles = ((int64_t)N + COLS - 1) / COLS;
  const int64_t t0 = (int64_t)split * a.tiles_per_split;
  const int64_t t1 = min(t0 + a.tiles_per_split, ntiles);
  u64 *const sw = sorts + (int64_t)wave * a.cap;
  auto list_of = [&](int q) { return a.lists + ((int64_t)q * a.splits + split) * a.cap; };
  u64 *const mine = list_of(own_ok ? own : 0);

  // the own query rows as B operands
  float x[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
    const int c = 4 * kk + hi;
    x[kk] = (own_ok && c < H) ? a.Q[(int64_t)own * a.ldq + c] : 0.f;
  }
  int64_t e0 = 0, e1 = 0;  // the own query's exclusion list
  if (own_ok && a.eoff) {
    e0 = a.eoff[own];
    e1 = a.eoff[own + 1];
    if (e1 < e0) e1 = e0;
  }
  u64 tau = 0;  // a key must be above it to enter the list (0: below every key)
  if (tid < kQRows) scnt[tid] = 0;

  // list q0 + qi cut to its best k, tau of its lanes raised to a key no better than the k-th.  In the stream (c > k:
  // c > cap - COLS >= k) the k-th key is selected bit by bit from the top (the largest t with #{key >= t} >= k; at
  // #{key >= t} == k the keys >= t are the best k already) and the keys >= t are compacted, unordered.  The final
  // cut sorts the list (stage 2 merges sorted lists) and stores its count.
  auto cut = [&](int qi, bool final) {
    u64 *const L = list_of(q0 + qi);
    wave_sync();
    const int c = scnt[wave * 16 + qi];
    const int n = min(c, a.k);
    u64 kth = 0;
    if (final) {
      int P = 64;
      while (P < c) P <<= 1;
      for (int i = lane; i < P; i += 64) sw[i] = i < c ? L[i] : 0ull;
      wave_sync();
      wave_sort_desc(sw, P, lane);
      for (int i = lane; i < n; i += 64) L[i] = sw[i];
      if (lane == 0) a.counts[(int64_t)(q0 + qi) * a.splits + split] = n;
    } else {
      for (int i = lane; i < c; i += 64) sw[i] = L[i];
      wave_sync();
      for (int b = 63; b >= 0; --b) {
        const u64 cand = kth | (1ull << b);
        int m = 0;
        for (int i = lane; i < c; i += 64) m += sw[i] >= cand ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
        if (m >= a.k) kth = cand;
        if (m == a.k) break;
      }
      int base = 0;
      for (int i0 = 0; i0 < c; i0 += 64) {
        const int i = i0 + lane;
        const bool keep = i < c && sw[i] >= kth;
        const u64 mask = __ballot(keep);
        if (keep) L[base + __popcll(mask & ((1ull << lane) - 1ull))] = sw[i];
        base += __popcll(mask);
      }
    }
    wave_sync();
    if (lane == 0) scnt[wave * 16 + qi] = n;
    if (lo == qi && kth > tau) tau = kth;
    wave_sync();
  };

  auto excluded = [&](int64_t g) {
    int64_t l = e0, h = e1;
    while (l < h) {
      const int64_t mid = (l + h) >> 1;
      if (a.erows[mid] < g) l = mid + 1;
      else h = mid;
    }
    return l < e1 && a.erows[l] == g;
  };

  // the prefetch registers of one tile
  float4 pf[NPF];
  auto fetch = [&](int64_t t) {
#pragma unroll
    for (int p = 0; p < NPF; ++p) {
      const int q = tid + kThreads * p, row = q / NK, c4 = q % NK;
      const int64_t g = t * COLS + row;
      pf[p] = (g < N && 4 * c4 < H) ? *reinterpret_cast<const float4 *>(a.C + g * a.ldc + 4 * c4)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int p = 0; p < NPF; ++p) {
      const int q = tid + kThreads * p, row = q / NK, c4 = q % NK;
      *reinterpret_cast<float4 *>(tiles + buf * (COLS * LDV) + row * LDV + 4 * c4) = pf[p];
    }
  };

  if (t0 < t1) {
    fetch(t0);
    stash(0);
  }
  __syncthreads();
  for (int64_t t = t0; t < t1; ++t) {
    const int buf = (int)((t - t0) & 1);
    {
      // a tile adds at most COLS keys to a list: cut the wave's lists that it could overflow
      const int c = scnt[wave * 16 + lo];
      u64 need = __ballot(hi == 0 && own_ok && c > a.cap - COLS);
      while (need) {
        const int qi = __builtin_ctzll(need);
        need &= need - 1;
        cut(qi, false);
      }
    }
    if (t + 1 < t1) fetch(t + 1);
    const float *ys = tiles + buf * (COLS * LDV);
#pragma unroll 1
    for (int sub = 0; sub < COLS / 16; sub += 2) {
      // two 16-row sub-tiles of the catalogue: two independent accumulator chains
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const float *y0 = ys + (sub * 16 + lo) * LDV + hi, *y1 = y0 + 16 * LDV;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y0[4 * kk], x[kk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y1[4 * kk], x[kk], acc1, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int sl = (sub + (q >> 2)) * 16 + 4 * hi + (q & 3);  // the catalogue row inside the tile
        const int64_t g = t * COLS + sl;
        const float raw = q < 4 ? acc0[q & 3] : acc1[q & 3];
        const u64 key = tk_key(a.scale * raw, (unsigned)g);
        if (own_ok && g < N && key > tau && !(e1 > e0 && excluded(g))) {
          const int slot = atomicAdd(&scnt[wave * 16 + lo], 1);
          mine[slot] = key;
        }
      }
    }
    if (t + 1 < t1) stash(buf ^ 1);
    __syncthreads();
  }
  for (int qi = 0; qi < 16; ++qi)
    if (q0 + qi < a.Nq) cut(qi, true);
}

template <int NK>
constexpr size_t tk_tile_lds() {
  constexpr int HP = 4 * NK, LDV = HP + 4, COLS = HP <= 128 ? 64 : 32;
  return (size_t)(2 * COLS * LDV + kQRows) * sizeof(float);
}
template <int NK>
size_t tk_scan_lds(int cap) {
  return tk_tile_lds<NK>() + (size_t)(kThreads / 64) * cap * sizeof(u64);
}

template <int NK>
void tk_launch_nk(dim3 grid, hipStream_t st, const TkArgs &a) {
  rm_launch_lds(topk_scan_kernel<NK>, grid, dim3(kThreads), tk_scan_lds<NK>(a.cap), st, a);
}

void tk_launch(int nk, dim3 grid, hipStream_t st, const TkArgs &a) {
  switch (nk) {
    case 4: tk_launch_nk<4>(grid, st, a); break;
    case 8: tk_launch_nk<8>(grid, st, a); break;
    case 12: tk_launch_nk<12>(grid, st, a); break;
    case 16: tk_launch_nk<16>(grid, st, a); break;
    case 24: tk_launch_nk<24>(grid, st, a); break;
    case 32: tk_launch_nk<32>(grid, st, a); break;
    case 48: tk_launch_nk<48>(grid, st, a); break;
    default: tk_launch_nk<64>(grid, st, a); break;
  }
}

// stage 2: per query the splits' sorted lists merged in split order into the best k; then the padding
__global__ __launch_bounds__(kThreads) void topk_merge_kernel(const u64 *__restrict__ lists,
                                                              const int *__restrict__ counts, int splits, int cap,
                                                              int Nq, int k, int64_t *__restrict__ out_rows,
                                                              float *__restrict__ out_scores, int64_t ldo) {
  extern __shared__ float smem[];
  u64 *const buf0 = reinterpret_cast<u64 *>(smem), *const buf1 = buf0 + k, *const lst = buf1 + k;
  const int tid = threadIdx.x;
  for (int q = blockIdx.x; q < Nq; q += gridDim.x) {
    u64 *cur = buf0, *nxt = buf1;
    int na = 0;
    for (int s = 0; s < splits; ++s) {
      const int64_t at = (int64_t)q * splits + s;
      const int nb = counts[at];
      if (nb <= 0) continue;
      const u64 *L = lists + at * cap;
      for (int j = tid; j < nb; j += kThreads) lst[j] = L[j];
      __syncthreads();
      for (int i = tid; i < na; i += kThreads) {
        const u64 v = cur[i];
        const int p = i + count_above(lst, nb, v);
        if (p < k) nxt[p] = v;
      }
      for (int j = tid; j < nb; j += kThreads) {
        const u64 v = lst[j];
        const int p = j + count_above(cur, na, v);
        if (p < k) nxt[p] = v;
      }
      na = min(na + nb, k);
      u64 *const tmp = cur;
      cur = nxt;
      nxt = tmp;
      __syncthreads();
    }
    for (int i = tid; i < k; i += kThreads) {
      const bool live = i < na;
      const u64 v = live ? cur[i] : 0ull;
      out_rows[(int64_t)q * ldo + i] = live ? tk_key_row(v) : (int64_t)-1;
      out_scores[(int64_t)q * ldo + i] = live ? tk_key_score(v) : -INFINITY;
    }
    __syncthreads();
  }
}

#define TK_LIMITS                                                                                                   \
  "H a multiple of 4 in 4..256, k in 1..1024, 0 <= Nq < 2^30, 0 <= N <= 2^31 - 1, pointers 16-byte aligned, ldq " \
  "and ldc multiples of 4 and >= H, ldo >= k, item_splits 0..64"

int tk_operand(const char *fn, const char *name, const char *ldname, const void *p, int64_t ld, int H) {
  RM_REQUIRE(p != nullptr, "%s: %s is NULL", fn, name);
  RM_REQUIRE(ld >= H, "%s: %s=%lld < H=%d (limits: " TK_LIMITS ")", fn, ldname, (long long)ld, H);
  RM_REQUIRE(ld % 4 == 0 && rm_aligned16(p) && ld <= kRmMaxStride,
             "%s: %s must be 16-byte aligned and %s=%lld a multiple of 4 floats (limits: " TK_LIMITS ")", fn, name,
             ldname, (long long)ld);
  return RM_OK;
}

}  // namespace

extern "C" int rm_topk_ip_supported(int H, int k) { return tk_supported(H, k) ? 1 : 0; }

extern "C" int rm_topk_ip_tile(int H, int which) {
  if (!tk_supported(H, 1)) return -1;
  switch (which) {
    case RM_TOPK_ROWS: return kQRows;
    case RM_TOPK_COLS: return tk_cols(tk_nk(H));
    case RM_TOPK_MAX_SPLITS: return kTkMaxSplits;
    default: return -1;
  }
}

extern "C" int64_t rm_topk_ip_workspace(int64_t Nq, int64_t N, int H, int k) {
  if (!tk_supported(H, k) || Nq < 0 || Nq >= kTkMaxQueries || N < 0 || N > kTkMaxRows) return -1;
  return tk_ws_floats(Nq, N, H, k);
}

extern "C" int rm_topk_ip(const float *Q, int64_t ldq, const float *C, int64_t ldc, int64_t Nq, int64_t N, int H,
                          float scale, int k, const int64_t *excl_offsets, const int64_t *excl_rows, int item_splits,
                          int64_t *out_rows, float *out_scores, int64_t ldo, void *workspace, rm_stream_t stream) {
  const char *fn = "rm_topk_ip";
  RM_REQUIRE(k >= 1 && k <= kTkMaxK, "%s: k=%d out of range (limits: " TK_LIMITS ")", fn, k);
  RM_REQUIRE(tk_supported(H, k), "%s: H=%d unsupported (limits: " TK_LIMITS ")", fn, H);
  RM_REQUIRE(Nq >= 0 && Nq < kTkMaxQueries, "%s: bad Nq=%lld (limits: " TK_LIMITS ")", fn, (long long)Nq);
  RM_REQUIRE(N >= 0 && N <= kTkMaxRows, "%s: bad N=%lld (limits: " TK_LIMITS ")", fn, (long long)N);
  RM_REQUIRE(item_splits >= 0 && item_splits <= kTkMaxSplits,
             "%s: item_splits=%d out of range (limits: " TK_LIMITS ")", fn, item_splits);
  if (Nq == 0) return RM_OK;
  if (N > 0) {
    if (int rc = tk_operand(fn, "Q", "ldq", Q, ldq, H)) return rc;
    if (int rc = tk_operand(fn, "C", "ldc", C, ldc, H)) return rc;
  }
  RM_REQUIRE(ldo >= k && ldo <= kRmMaxStride, "%s: ldo=%lld < k=%d or too large (limits: " TK_LIMITS ")", fn,
             (long long)ldo, k);
  RM_REQUIRE(out_rows && out_scores && rm_aligned16(out_rows) && rm_aligned16(out_scores),
             "%s: out_rows or out_scores is NULL or not 16-byte aligned", fn);
  RM_REQUIRE(workspace && rm_aligned16(workspace), "%s: the workspace is NULL or not 16-byte aligned", fn);
  RM_REQUIRE(excl_offsets || !excl_rows, "%s: excl_rows given without excl_offsets", fn);
  RM_REQUIRE(!excl_offsets || excl_rows, "%s: excl_offsets given without excl_rows", fn);
  const int nk = tk_nk(H), cols = tk_cols(nk), cap = tk_cap(k);
  hipStream_t st = (hipStream_t)stream;
  u64 *lists = reinterpret_cast<u64 *>(workspace);
  int splits = 0;
  int *counts = nullptr;
  if (N > 0) {
    splits = tk_splits(Nq, N, cols, item_splits);
    const int64_t tiles = tk_tiles(N, cols);
    counts = reinterpret_cast<int *>(lists + Nq * splits * (int64_t)cap);
    TkArgs a = {};
    a.Q = Q; a.ldq = ldq; a.C = C; a.ldc = ldc;
    a.Nq = (int)Nq; a.N = (int)N; a.H = H;
    a.scale = scale; a.k = k; a.cap = cap;
    a.eoff = excl_offsets; a.erows = excl_rows;
    a.tiles_per_split = (int)((tiles + splits - 1) / splits);
    a.splits = splits;
    a.lists = lists; a.counts = counts;
    tk_launch(nk, dim3((unsigned)((Nq + kQRows - 1) / kQRows), (unsigned)splits), st, a);
  }
  rm_launch_lds(topk_merge_kernel, dim3(rm_grid_cap(Nq, kMergeBlocks)), dim3(kThreads),
                (size_t)3 * k * sizeof(u64), st, (const u64 *)lists, (const int *)counts, splits, cap, (int)Nq, k,
                out_rows, out_scores, ldo);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
