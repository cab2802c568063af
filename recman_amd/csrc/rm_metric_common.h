// Device helpers shared by the translation units that sort a batch or a prediction vector (metrics.hip, gauc.hip,
// rankmetrics.hip, rank.hip): the tile geometry, the order-preserving score key and the fixed-order block
// reductions / scans.  The sort itself, the one radix sort of all four, is in rm_radix_sort.h.
#pragma once
#include "rm_common.h"

namespace {

constexpr int kThreads = 256;             // 4 waves: every kernel here
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 16;                // keys per thread of a sort / group tile
constexpr int kTile = kThreads * kItems;  // 4096
constexpr int kRadix = 256;               // 8-bit digits
constexpr int kKeyBlocks = 1024;          // grid cap of the grid-stride passes
constexpr unsigned kNoEnd = 0xFFFFFFFFu;  // "group end not in this tile" (ends are <= n <= 2^31 - 1)

inline size_t take(size_t &o, size_t bytes) {
  const size_t at = o;
  o += (bytes + 255) & ~size_t(255);
  return at;
}

// order-preserving key of a float; -0.0 is canonicalised to +0.0 (they compare equal and must tie)
__device__ __forceinline__ unsigned score_key(float s) {
  unsigned b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide sum in a fixed order (every lane of the block gets it); sm: kWaves entries
template <typename T>
__device__ T block_sum(T v, T *sm) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = sm[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s += sm[w];
  __syncthreads();
  return s;
}

// block-wide inclusive scan (kRev: from the last thread down) of a commutative, associative op
template <bool kRev, typename T, typename Op>
__device__ T block_scan(T v, Op op, T *sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = kRev ? __shfl_down(v, o, 64) : __shfl_up(v, o, 64);
    if (kRev ? lane + o < 64 : lane >= o) v = op(v, u);
  }
  if (lane == (kRev ? 0 : 63)) sm[w] = v;
  __syncthreads();
  if (kRev) {
    for (int i = w + 1; i < kWaves; ++i) v = op(v, sm[i]);
  } else {
    for (int i = 0; i < w; ++i) v = op(v, sm[i]);
  }
  __syncthreads();
  return v;
}

struct OpAdd {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct OpMin {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};

}  // namespace
