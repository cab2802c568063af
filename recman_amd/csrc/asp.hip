// Attention-pooled behaviour sequences - SequenceFeat + the DIN local activation unit (Deep Interest Network,
// arXiv 1706.06978, section 4.3).  The reference has no code for it (recman/tf/core/DIN.py:6 imports ASPCombiner /
// ASPLayer, which exist nowhere; SequenceFeat.__init__ raises, inputs.py:443).  Per example b with query row q
// (columns 0..D-1 of the candidate item's table row) and history rows k_1..k_n of the SAME table block (CSR):
//     x_l = [q, k_l, q - k_l, q * k_l]  (4D)      z = act(.. act(x_l W0 + b0) .. W_{m-1} + b_{m-1}),  m = 1 or 2
//     s_l = z . w + w0        a_l = s_l  or  softmax_{l <= n}(s_l)  (max-subtracted)        out_b = sum_l a_l k_l
// rm_asp_fwd writes out_b into a fused scratch row (columns 0..D-1, zeros behind: no linear / FM-bias term) that the
// gather kernel reads like any table row.  x and the hidden activations never reach HBM: the only per-position value
// that does is the score s_l (one float), which is also all the backward keeps.
//
// Mapping.  The two small GEMMs run on the f32 MFMA (v_mfma_f32_32x32x2_f32: exact f32 fma chains) with POSITIONS as
// the M dimension: the nnz history positions of the batch are cut into tiles of TP = 64 (or 32) consecutive CSR
// positions - whatever example they belong to (binary search in `offsets`), so ragged lengths cost nothing - one
// 256-thread block per tile, grid-stride.  A tile's x [TP, 4D], z1 [TP, H1p] and z2 [TP, H2p] live in LDS (odd row
// strides); the weights, padded to multiples of 32 units with zeros (inert: a padded unit feeds zero weights), are
// copied into LDS once per block when they fit beside the tile (they do for the default (80, 40), D = 16) and are
// read through the caches otherwise.  Every wave owns 32x32 output tiles of a product; A and B operands come from
// LDS one float per lane and MFMA (64 cycles each: two 4-byte LDS reads per MFMA are far from the LDS limit).
//   forward : asp_score_kernel (tiles: x -> z1 -> z2 -> s_l)  +  asp_pool_kernel (16 lanes per example: softmax
//             over the example's scores, out = sum a_l k_l).
//   backward: asp_bwd_example_kernel (16 lanes per example: ds_l from the pooled row's gradient, and the direct key
//             gradient a_l * d_out),  asp_bwd_tile_kernel (tiles: recompute x, z1, z2; dz2, dz1, dx on the MFMA;
//             dW1 += z1^T dz2 and dW0 += x^T dz1 accumulate in registers over all tiles of the block; per position
//             the key gradient is added to d_keys and the query gradient goes to a [nnz, D] workspace),
//             asp_bwd_query_kernel (16 lanes per example: sums its positions' query gradients in list order and ADDS
//             them onto d_query),  asp_finish_kernel (per-block partials summed in block order).
// Under the softmax sum_l ds_l is zero per example, so dw, dw0 and the bias gradients are what is left of a
// cancellation: the sums behind ds_l, those per-thread sums, the query sums and the finish pass are kept in double.
// No float atomics anywhere, every sum in a fixed order: two runs are bit-equal.
#include <math.h>

#include "rm_launch.h"

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kMaxH = 128, kMaxLen = 256;
constexpr int kMaxBlocks = 512;           // two blocks per CU
constexpr size_t kLdsMax = 160 * 1024;    // per CU (and per block) on gfx950

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline int rup32(int v) { return (v + 31) / 32 * 32; }
inline int64_t rup4(int64_t v) { return (v + 3) / 4 * 4; }

struct AspDims {
  int D, K0, nl, H1, H2, H1p, H2p, HL, HLp;  // K0 = 4 D; HL = width of the last hidden layer
  int S0, S1, SX;                            // LDS row strides of x, z1 and z2 / dx (odd)
  int ldw0, ldw1;                            // row strides of the packed W0 [K0, H1p], W1 [H1p, H2p] (odd)
  int oW0, ob0, oW1, ob1, ow, ow0, nparam;   // offsets in the packed parameter block (floats)
  int pW0, pW1, pb0, pb1, pw, pw0, plo, npart;  // a block's partial sums: dW0 [K0, H1p], dW1 [H1p, H2p], db0, ..; the
                                                // sums kept in double (pb0 .. pw0) have their low halves behind plo
};

AspDims asp_dims(int D, int nl, const int *H) {
  AspDims d;
  d.D = D; d.K0 = 4 * D; d.nl = nl;
  d.H1 = H[0]; d.H2 = nl == 2 ? H[1] : 0;
  d.H1p = rup32(d.H1); d.H2p = nl == 2 ? rup32(d.H2) : 0;
  d.HL = nl == 2 ? d.H2 : d.H1; d.HLp = nl == 2 ? d.H2p : d.H1p;
  d.S0 = d.K0 + 1; d.S1 = d.H1p + 1; d.SX = (d.K0 > d.H2p ? d.K0 : d.H2p) + 1;
  d.ldw0 = d.H1p + 1; d.ldw1 = d.H2p + 1;
  d.oW0 = 0; d.ob0 = d.K0 * d.ldw0; d.oW1 = d.ob0 + d.H1p;
  d.ob1 = d.oW1 + (nl == 2 ? d.H1p * d.ldw1 : 0); d.ow = d.ob1 + d.H2p; d.ow0 = d.ow + d.HLp;
  d.nparam = (int)rup4(d.ow0 + 1);
  d.pW0 = 0; d.pW1 = d.K0 * d.H1p; d.pb0 = d.pW1 + d.H1p * d.H2p; d.pb1 = d.pb0 + d.H1p; d.pw = d.pb1 + d.H2p;
  d.pw0 = d.pw + d.HLp; d.plo = d.pw0 + 1; d.npart = (int)rup4(d.plo + d.plo - d.pb0);
  return d;
}

struct AspCfg {
  int TP;
  bool wlds;
  size_t smem;
};
AspCfg asp_cfg(const AspDims &d) {
  auto buf = [&](int TP) { return (size_t)TP * (d.S0 + d.S1 + d.SX + 2); };  // + ds [TP] + example index [TP]
  if (4 * (buf(64) + d.nparam) <= kLdsMax) return {64, true, 4 * (buf(64) + d.nparam)};
  if (4 * (buf(32) + d.nparam) <= kLdsMax) return {32, true, 4 * (buf(32) + d.nparam)};
  return {64, false, 4 * buf(64)};
}

inline bool asp_shape_ok(int D, int nl, const int *H, int max_len) {
  if (!(D == 8 || D == 16 || D == 32) || !(nl == 1 || nl == 2) || H == nullptr) return false;
  for (int i = 0; i < nl; ++i)
    if (H[i] < 1 || H[i] > kMaxH) return false;
  return max_len >= 1 && max_len <= kMaxLen;
}

__device__ __forceinline__ float asp_act(float x, int act) { return act == 0 ? fmaxf(x, 0.f) : 1.f / (1.f + expf(-x)); }
// derivative from the POST-activation value
__device__ __forceinline__ float asp_actg(float y, int act) { return act == 0 ? (y > 0.f ? 1.f : 0.f) : y * (1.f - y); }

// W0 [4D,H1], b0, W1 [H1,H2], b1, w [HL], w0 -> the padded block (zeros in the padding)
__global__ void asp_pack_kernel(AspDims d, const float *__restrict__ W0, const float *__restrict__ b0,
                                const float *__restrict__ W1, const float *__restrict__ b1,
                                const float *__restrict__ w, const float *__restrict__ w0, float *__restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d.nparam) return;
  float v = 0.f;
  if (e < d.ob0) {
    const int r = e / d.ldw0, c = e - r * d.ldw0;
    if (c < d.H1) v = W0[r * d.H1 + c];
  } else if (e < d.oW1) {
    if (e - d.ob0 < d.H1) v = b0[e - d.ob0];
  } else if (e < d.ob1) {
    const int q = e - d.oW1, r = q / d.ldw1, c = q - r * d.ldw1;
    if (r < d.H1 && c < d.H2) v = W1[r * d.H2 + c];
  } else if (e < d.ow) {
    if (e - d.ob1 < d.H2) v = b1[e - d.ob1];
  } else if (e < d.ow0) {
    if (e - d.ow < d.HL) v = w[e - d.ow];
  } else if (e == d.ow0) {
    v = w0[0];
  }
  out[e] = v;
}

// C[m, n] = sum_k A(m, k) B(k, n) over Mt x Nt tiles of 32 x 32, K a multiple of 2; element (m, k) of A sits at
// A[m a_m + k a_k], (k, n) of B at Bm[k b_k + n b_n].  A wave owns tiles wave, wave + 4, ..; epi(m, n, value).
// (v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][l >> 5], B[l >> 5][l & 31]; C column l & 31, rows
// (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).)
template <class Epi>
__device__ __forceinline__ void asp_gemm(int Mt, int Nt, int K, const float *A, int a_m, int a_k, const float *Bm,
                                         int b_k, int b_n, Epi epi) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int t = wave; t < Mt * Nt; t += kWaves) {
    const int mi = t / Nt, ni = t - mi * Nt;
    const float *ap = A + (mi * 32 + r) * a_m + h * a_k;
    const float *bp = Bm + h * b_k + (ni * 32 + r) * b_n;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k * a_k], bp[k * b_k], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) epi(mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * h, ni * 32 + r, acc[i]);
  }
}

// the same product ADDED onto accumulators that live in registers across calls: slot s = tile wave + 4 s (<= 16 tiles)
__device__ __forceinline__ void asp_gemm_acc(int Mt, int Nt, int K, const float *A, int a_m, int a_k, const float *Bm,
                                             int b_k, int b_n, f32x16 (&acc)[4]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int t = wave + kWaves * s;
    if (t < Mt * Nt) {
      const int mi = t / Nt, ni = t - mi * Nt;
      const float *ap = A + (mi * 32 + r) * a_m + h * a_k;
      const float *bp = Bm + h * b_k + (ni * 32 + r) * b_n;
      f32x16 c = acc[s];

      for (int k = 0; k < K; k += 2) c = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k * a_k], bp[k * b_k], c, 0, 0, 0);
      acc[s] = c;
    }
  }
}

__device__ __forceinline__ void asp_store_acc(int Mt, int Nt, int ld, const f32x16 (&acc)[4], float *out) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int t = wave + kWaves * s;
    if (t < Mt * Nt) {
      const int mi = t / Nt, ni = t - mi * Nt;
#pragma unroll
      for (int i = 0; i < 16; ++i) out[(mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * ld + ni * 32 + r] = acc[s][i];
    }
  }
}

struct AspIn {
  const float *rows;
  int64_t LD, row0;
  const int64_t *offsets, *ids, *qrow;
  int64_t B, nnz;
};

// LDS carve-up: x [TP][S0] | z1 [TP][S1] | zx [TP][SX] | ds [TP] | example index [TP] | (weights)
struct AspLds {
  float *xs, *z1, *zx, *dsl;
  int *exs;
  const float *P;
};
template <bool WLDS>
__device__ __forceinline__ AspLds asp_lds(const AspDims &d, int TP, float *sm, const float *params) {
  AspLds l;
  l.xs = sm;
  l.z1 = l.xs + TP * d.S0;
  l.zx = l.z1 + TP * d.S1;
  l.dsl = l.zx + TP * d.SX;
  l.exs = reinterpret_cast<int *>(l.dsl + TP);
  if constexpr (WLDS) {
    float *w = l.dsl + 2 * TP;
    for (int i = threadIdx.x; i < d.nparam; i += kThreads) w[i] = params[i];
    l.P = w;  // (the first barrier of the tile loop publishes it)
  } else {
    l.P = params;
  }
  return l;
}

// one tile: example index of every position, x, z1 (and z2 into zx) in LDS; ends on a barrier
__device__ __forceinline__ void asp_tile_forward(const AspDims &d, int TP, int64_t pos0, const AspIn &in,
                                                 const AspLds &l, int act) {
  const int tid = threadIdx.x, D = d.D;
  __syncthreads();
  for (int p = tid; p < TP; p += kThreads) {
    const int64_t pos = pos0 + p;
    int e = -1;
    if (pos < in.nnz) {  // the largest b with offsets[b] <= pos (empty examples are skipped)
      int64_t lo = 0, hi = in.B - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (in.offsets[mid] <= pos) lo = mid; else hi = mid - 1;
      }
      e = (int)lo;
    }
    l.exs[p] = e;
  }
  __syncthreads();
  for (int i = tid; i < TP * D; i += kThreads) {
    const int p = i / D, c = i - p * D, e = l.exs[p];
    float q = 0.f, k = 0.f;
    if (e >= 0) {
      k = in.rows[(in.row0 + in.ids[pos0 + p]) * in.LD + c];
      q = in.rows[in.qrow[e] * in.LD + c];
    }
    float *x = l.xs + p * d.S0;
    x[c] = q; x[D + c] = k; x[2 * D + c] = q - k; x[3 * D + c] = q * k;
  }
  __syncthreads();
  const float *P = l.P;
  float *z1 = l.z1, *zx = l.zx;
  const int S1 = d.S1, SX = d.SX;
  asp_gemm(TP / 32, d.H1p / 32, d.K0, l.xs, d.S0, 1, P + d.oW0, d.ldw0, 1,
           [&](int m, int n, float v) { z1[m * S1 + n] = asp_act(v + P[d.ob0 + n], act); });
  __syncthreads();
  if (d.nl == 2) {
    asp_gemm(TP / 32, d.H2p / 32, d.H1p, z1, S1, 1, P + d.oW1, d.ldw1, 1,
             [&](int m, int n, float v) { zx[m * SX + n] = asp_act(v + P[d.ob1 + n], act); });
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <bool WLDS>
__global__ __launch_bounds__(kThreads) void asp_score_kernel(AspDims d, int TP, AspIn in,
                                                             const float *__restrict__ params, int act,
                                                             float *__restrict__ scores) {
  extern __shared__ float sm[];
  const AspLds l = asp_lds<WLDS>(d, TP, sm, params);
  const int tid = threadIdx.x;
  const float *zl = d.nl == 2 ? l.zx : l.z1;
  const int SL = d.nl == 2 ? d.SX : d.S1;
  const int per = kThreads / TP;  // lanes per position: 4 or 8
  const int64_t tiles = (in.nnz + TP - 1) / TP;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t pos0 = tile * TP;
    asp_tile_forward(d, TP, pos0, in, l, act);
    const int p = tid / per, j = tid - p * per;
    float s = 0.f;
    for (int u = j; u < d.HLp; u += per) s = fmaf(zl[p * SL + u], l.P[d.ow + u], s);
    for (int o = per >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (j == 0 && l.exs[p] >= 0) scores[pos0 + p] = s + l.P[d.ow0];
  }
}

// softmax statistics of one example's scores (every lane of the group computes them): a_l = exp(s_l - m) / den
__device__ __forceinline__ void asp_softmax_stats(const float *__restrict__ scores, int64_t s, int64_t e, float *m,
                                                  float *den) {
  float mx = -INFINITY, dn = 0.f;
  for (int64_t t = s; t < e; ++t) mx = fmaxf(mx, scores[t]);
  for (int64_t t = s; t < e; ++t) dn += expf(scores[t] - mx);
  *m = mx;
  *den = dn;
}

// 16 lanes per example: lane k handles columns k and k + 16 of the fused row
__global__ __launch_bounds__(kThreads) void asp_pool_kernel(AspIn in, int D, int norm,
                                                            const float *__restrict__ scores,
                                                            float *__restrict__ out) {
  const int lane = threadIdx.x & 15;
  const int64_t b = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 4;
  if (b >= in.B) return;
  const int64_t s = in.offsets[b], e = in.offsets[b + 1];
  float m = 0.f, den = 1.f;
  if (norm && e > s) asp_softmax_stats(scores, s, e, &m, &den);
  float acc0 = 0.f, acc1 = 0.f;
  for (int64_t t = s; t < e; ++t) {
    const float a = norm ? expf(scores[t] - m) / den : scores[t];
    const float *k = in.rows + (in.row0 + in.ids[t]) * in.LD;
    if (lane < D) acc0 = fmaf(a, k[lane], acc0);
    if (lane + 16 < D) acc1 = fmaf(a, k[lane + 16], acc1);
  }
  for (int c = lane; c < in.LD; c += 16)  // zeros behind column D: no FM-bias and no linear entry
    out[b * in.LD + c] = c >= D ? 0.f : (c == lane ? acc0 : acc1);
}

// ----------------------------------------------------------------------------------------------- backward
__device__ __forceinline__ float asp_group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ds_l and the direct key gradient a_l * d_out: 16 lanes per example
__global__ __launch_bounds__(kThreads) void asp_bwd_example_kernel(AspIn in, int D, int norm,
                                                                   const float *__restrict__ scores,
                                                                   const float *__restrict__ d_out, int64_t do_stride,
                                                                   float *__restrict__ ds, float *__restrict__ d_keys) {
  const int lane = threadIdx.x & 15;
  const int64_t b = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 4;
  if (b >= in.B) return;  // (the 16 lanes of a group share b)
  const int64_t s = in.offsets[b], e = in.offsets[b + 1];
  if (e <= s) return;
  const float g0 = lane < D ? d_out[b * do_stride + lane] : 0.f;
  const float g1 = lane + 16 < D ? d_out[b * do_stride + lane + 16] : 0.f;
  // ds_l = a_l (da_l - sum_j a_j da_j) sums to ZERO over the example, and the parameter gradients built from it
  // (dw, the bias gradients) are what is left of that cancellation: the weights a_l and the inner sum are kept in
  // double, so the residue of sum_l ds_l is the rounding of the stored floats and not that of a 256-term float chain
  float m = 0.f;
  double den = 1.0, tsum = 0.0;
  if (norm) {
    float denf;
    asp_softmax_stats(scores, s, e, &m, &denf);
    den = 0.0;
    for (int64_t t = s; t < e; ++t) den += (double)expf(scores[t] - m);
    for (int64_t t = s; t < e; ++t) {
      const float *k = in.rows + (in.row0 + in.ids[t]) * in.LD;
      const float da = asp_group16_sum((lane < D ? g0 * k[lane] : 0.f) + (lane + 16 < D ? g1 * k[lane + 16] : 0.f));
      tsum += (double)expf(scores[t] - m) / den * (double)da;
    }
  }
  for (int64_t t = s; t < e; ++t) {
    const float *k = in.rows + (in.row0 + in.ids[t]) * in.LD;
    const float da = asp_group16_sum((lane < D ? g0 * k[lane] : 0.f) + (lane + 16 < D ? g1 * k[lane + 16] : 0.f));
    const double ad = norm ? (double)expf(scores[t] - m) / den : (double)scores[t];
    const float a = (float)ad;
    if (lane == 0) ds[t] = norm ? (float)(ad * ((double)da - tsum)) : da;
    if (lane < D) d_keys[t * D + lane] = a * g0;
    if (lane + 16 < D) d_keys[t * D + lane + 16] = a * g1;
  }
}

// a double partial sum as two floats of the block's partials: the high half at e, the low half behind plo
__device__ __forceinline__ void asp_store_double(float *out, const AspDims &d, int e, double v) {
  const float hi = (float)v;
  out[e] = hi;
  out[d.plo + e - d.pb0] = (float)(v - (double)hi);
}

template <bool WLDS>
__global__ __launch_bounds__(kThreads) void asp_bwd_tile_kernel(AspDims d, int TP, AspIn in,
                                                                const float *__restrict__ params, int act,
                                                                const float *__restrict__ ds,
                                                                float *__restrict__ d_keys, float *__restrict__ d_q,
                                                                float *__restrict__ part) {
  extern __shared__ float sm[];
  const AspLds l = asp_lds<WLDS>(d, TP, sm, params);
  const int tid = threadIdx.x, D = d.D;
  const float *P = l.P;
  float *xs = l.xs, *z1 = l.z1, *zx = l.zx, *dsl = l.dsl;
  const int S0 = d.S0, S1 = d.S1, SX = d.SX;
  float *zl = d.nl == 2 ? zx : z1;
  const int SL = d.nl == 2 ? SX : S1;

  f32x16 accW0[4], accW1[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < 16; ++i) accW0[s][i] = accW1[s][i] = 0.f;
  // thread u: unit u of the layer.  These sums run over every position of the batch and nearly cancel (sum_l ds_l is
  // zero per example under the softmax): they are kept in double, a few fma per thread and tile
  double dw_acc = 0.0, dbl_acc = 0.0, db0_acc = 0.0, dw0_acc = 0.0;

  const int64_t tiles = (in.nnz + TP - 1) / TP;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t pos0 = tile * TP;
    asp_tile_forward(d, TP, pos0, in, l, act);
    for (int p = tid; p < TP; p += kThreads) dsl[p] = l.exs[p] >= 0 ? ds[pos0 + p] : 0.f;
    __syncthreads();
    // the last layer: dw += ds z, dz = ds w act'(z) in place, its bias gradient
    if (tid < d.HLp) {
      const float wu = P[d.ow + tid];
      for (int p = 0; p < TP; ++p) {
        const float y = zl[p * SL + tid], s = dsl[p];
        dw_acc = fma((double)s, (double)y, dw_acc);
        const float dz = s * wu * asp_actg(y, act);
        zl[p * SL + tid] = dz;
        dbl_acc += (double)dz;
      }
    } else if (tid == kThreads - 1) {
      for (int p = 0; p < TP; ++p) dw0_acc += (double)dsl[p];
    }
    __syncthreads();
    if (d.nl == 2) {
      // dW1 += z1^T dz2;  then dz1 = (dz2 W1^T) o act'(z1) in place
      asp_gemm_acc(d.H1p / 32, d.H2p / 32, TP, z1, 1, S1, zx, SX, 1, accW1);
      __syncthreads();
      asp_gemm(TP / 32, d.H1p / 32, d.H2p, zx, SX, 1, P + d.oW1, 1, d.ldw1,
               [&](int m, int n, float v) { z1[m * S1 + n] = v * asp_actg(z1[m * S1 + n], act); });
      __syncthreads();
      if (tid < d.H1p)
        for (int p = 0; p < TP; ++p) db0_acc += (double)z1[p * S1 + tid];
    }
    // dW0 += x^T dz1;  dx = dz1 W0^T -> zx (nobody reads dz2 any more)
    asp_gemm_acc(d.K0 / 32, d.H1p / 32, TP, xs, 1, S0, z1, S1, 1, accW0);
    asp_gemm(TP / 32, d.K0 / 32, d.H1p, z1, S1, 1, P + d.oW0, 1, d.ldw0,
             [&](int m, int n, float v) { zx[m * SX + n] = v; });
    __syncthreads();
    // x = [q, k, q - k, q k]: dk = dx_k - dx_d + q dx_p, dq = dx_q + dx_d + k dx_p
    for (int i = tid; i < TP * D; i += kThreads) {
      const int p = i / D, c = i - p * D;
      if (l.exs[p] < 0) continue;
      const float *x = xs + p * S0, *g = zx + p * SX;
      const float q = x[c], k = x[D + c];
      const float dk = g[D + c] - g[2 * D + c] + q * g[3 * D + c];
      const float dq = g[c] + g[2 * D + c] + k * g[3 * D + c];
      d_keys[(pos0 + p) * D + c] += dk;
      d_q[(pos0 + p) * D + c] = dq;
    }
  }
  float *out = part + (int64_t)blockIdx.x * d.npart;
  asp_store_acc(d.K0 / 32, d.H1p / 32, d.H1p, accW0, out + d.pW0);
  if (d.nl == 2) {
    asp_store_acc(d.H1p / 32, d.H2p / 32, d.H2p, accW1, out + d.pW1);
    if (tid < d.H1p) asp_store_double(out, d, d.pb0 + tid, db0_acc);
    if (tid < d.H2p) asp_store_double(out, d, d.pb1 + tid, dbl_acc);
  } else if (tid < d.H1p) {
    asp_store_double(out, d, d.pb0 + tid, dbl_acc);
  }
  if (tid < d.HLp) asp_store_double(out, d, d.pw + tid, dw_acc);
  if (tid == kThreads - 1) asp_store_double(out, d, d.pw0, dw0_acc);
}

// 16 lanes per example: the query gradient = sum of its positions' contributions in list order, ADDED onto d_query
__global__ __launch_bounds__(kThreads) void asp_bwd_query_kernel(const int64_t *__restrict__ offsets, int64_t B, int D,
                                                                 const float *__restrict__ d_q,
                                                                 float *__restrict__ d_query, int64_t dq_stride) {
  const int lane = threadIdx.x & 15;
  const int64_t b = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 4;
  if (b >= B) return;
  const int64_t s = offsets[b], e = offsets[b + 1];
  if (e <= s) return;
  for (int c = lane; c < D; c += 16) {
    double acc = 0.0;
    for (int64_t t = s; t < e; ++t) acc += (double)d_q[t * D + c];
    d_query[b * dq_stride + c] += (float)acc;
  }
}

// fixed-order sum (in double) of the per-block partials, padding dropped
__global__ void asp_finish_kernel(AspDims d, const float *__restrict__ part, int nblk, float *__restrict__ dW0,
                                  float *__restrict__ db0, float *__restrict__ dW1, float *__restrict__ db1,
                                  float *__restrict__ dw, float *__restrict__ dw0) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d.plo) return;
  float *dst = nullptr;
  if (e < d.pW1) {
    const int r = e / d.H1p, c = e - r * d.H1p;
    if (c < d.H1) dst = dW0 + r * d.H1 + c;
  } else if (e < d.pb0) {
    const int q = e - d.pW1, r = q / d.H2p, c = q - r * d.H2p;
    if (r < d.H1 && c < d.H2) dst = dW1 + r * d.H2 + c;
  } else if (e < d.pb1) {
    if (e - d.pb0 < d.H1) dst = db0 + (e - d.pb0);
  } else if (e < d.pw) {
    if (e - d.pb1 < d.H2) dst = db1 + (e - d.pb1);
  } else if (e < d.pw0) {
    if (e - d.pw < d.HL) dst = dw + (e - d.pw);
  } else if (e == d.pw0) {
    dst = dw0;
  }
  if (dst == nullptr) return;
  const int lo = e >= d.pb0 ? d.plo + e - d.pb0 : -1;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) {
    const float *pk = part + (int64_t)k * d.npart;
    s += lo >= 0 ? (double)pk[e] + (double)pk[lo] : (double)pk[e];
  }
  *dst = (float)s;
}

inline int asp_blocks(int64_t nnz, int TP) { return rm_grid_cap((nnz + TP - 1) / TP, kMaxBlocks); }

int asp_check(const char *fn, int D, int nl, const int *H, int act, int64_t B, int64_t nnz, int64_t LD) {
  RM_REQUIRE(asp_shape_ok(D, nl, H, 1), "%s: unsupported shape (D=%d in {8,16,32}, 1 or 2 hidden layers of 1..%d units)",
             fn, D, kMaxH);
  RM_REQUIRE(act == RM_ASP_RELU || act == RM_ASP_SIGMOID, "%s: unsupported activation %d", fn, act);
  return rm_seq_check_sizes(fn, D, B, nnz, LD);
}

void asp_pack(const AspDims &d, const float *W0, const float *b0, const float *W1, const float *b1, const float *w,
              const float *w0, float *out, hipStream_t st) {
  hipLaunchKernelGGL(asp_pack_kernel, dim3((d.nparam + 255) / 256), dim3(256), 0, st, d, W0, b0, W1, b1, w, w0, out);
}

}  // namespace

extern "C" int rm_asp_supported(int D, int n_layers, const int *H, int max_len) {
  return asp_shape_ok(D, n_layers, H, max_len) ? 1 : 0;
}

extern "C" int64_t rm_asp_workspace(int D, int n_layers, const int *H, int64_t nnz, int backward) {
  if (!asp_shape_ok(D, n_layers, H, 1) || nnz < 0) return 0;
  const AspDims d = asp_dims(D, n_layers, H);
  if (!backward) return d.nparam;
  const AspCfg c = asp_cfg(d);
  return d.nparam + rup4(nnz) + rup4(nnz * D) + (int64_t)asp_blocks(nnz, c.TP) * d.npart;
}

extern "C" int rm_asp_fwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                          const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz, const float *W0,
                          const float *b0, const float *W1, const float *b1, const float *w, const float *w0,
                          int n_layers, const int *H, int act, int norm, float *out, float *scores, float *workspace,
                          rm_stream_t stream) {
  int rc = asp_check("rm_asp_fwd", D, n_layers, H, act, B, nnz, LD);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  if ((rc = rm_seq_check_fwd("rm_asp_fwd", rows, offsets, ids, qrow, nnz, out, workspace)) != RM_OK) return rc;
  RM_REQUIRE(W0 && b0 && w && w0 && (n_layers == 1 || (W1 && b1)) && (nnz == 0 || scores), "rm_asp_fwd: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const AspDims d = asp_dims(D, n_layers, H);
  const AspIn in{rows, LD, row0, offsets, ids, qrow, B, nnz};
  if (nnz > 0) {
    asp_pack(d, W0, b0, W1, b1, w, w0, workspace, st);
    const AspCfg c = asp_cfg(d);
    dim3 grid(asp_blocks(nnz, c.TP));
#define RM_ASP_SCORE(WL_) \
  rm_launch_lds(asp_score_kernel<WL_>, grid, dim3(kThreads), c.smem, st, d, c.TP, in, workspace, act, scores)
    if (c.wlds) RM_ASP_SCORE(true); else RM_ASP_SCORE(false);
#undef RM_ASP_SCORE
    RM_CHECK_LAUNCH("rm_asp_fwd (scores)");
  }
  hipLaunchKernelGGL(asp_pool_kernel, dim3((unsigned)((B * 16 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, in,
                     D, norm ? 1 : 0, (const float *)scores, out);
  RM_CHECK_LAUNCH("rm_asp_fwd (pool)");
  return RM_OK;
}

extern "C" int rm_asp_bwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                          const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz, const float *W0,
                          const float *b0, const float *W1, const float *b1, const float *w, const float *w0,
                          int n_layers, const int *H, int act, int norm, const float *scores, const float *d_out,
                          int64_t do_stride, float *d_keys, float *d_query, int64_t dq_stride, float *dW0, float *db0,
                          float *dW1, float *db1, float *dw, float *dw0, float *workspace, rm_stream_t stream) {
  int rc = asp_check("rm_asp_bwd", D, n_layers, H, act, B, nnz, LD);
  if (rc != RM_OK) return rc;
  if ((rc = rm_seq_check_bwd("rm_asp_bwd", D, rows, offsets, ids, qrow, B, nnz, d_out, do_stride, d_keys, d_query,
                             dq_stride, workspace)) != RM_OK)
    return rc;
  RM_REQUIRE(W0 && b0 && w && w0 && dW0 && db0 && dw && dw0 && (n_layers == 1 || (W1 && b1 && dW1 && db1)) &&
                 (nnz == 0 || scores), "rm_asp_bwd: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const AspDims d = asp_dims(D, n_layers, H);
  const AspCfg c = asp_cfg(d);
  float *ds = workspace + d.nparam, *d_q = ds + rup4(nnz), *part = d_q + rup4(nnz * D);
  const int nblk = nnz > 0 ? asp_blocks(nnz, c.TP) : 0;
  if (nnz > 0) {
    const AspIn in{rows, LD, row0, offsets, ids, qrow, B, nnz};
    asp_pack(d, W0, b0, W1, b1, w, w0, workspace, st);
    const dim3 egrid((unsigned)((B * 16 + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(asp_bwd_example_kernel, egrid, dim3(kThreads), 0, st, in, D, norm ? 1 : 0, scores, d_out,
                       do_stride, ds, d_keys);
    RM_CHECK_LAUNCH("rm_asp_bwd (examples)");
#define RM_ASP_BWD(WL_)                                                                                         \
  rm_launch_lds(asp_bwd_tile_kernel<WL_>, dim3(nblk), dim3(kThreads), c.smem, st, d, c.TP, in, workspace, act, ds, \
                d_keys, d_q, part)
    if (c.wlds) RM_ASP_BWD(true); else RM_ASP_BWD(false);
#undef RM_ASP_BWD
    RM_CHECK_LAUNCH("rm_asp_bwd (tiles)");
    hipLaunchKernelGGL(asp_bwd_query_kernel, egrid, dim3(kThreads), 0, st, offsets, B, D, (const float *)d_q, d_query,
                       dq_stride);
    RM_CHECK_LAUNCH("rm_asp_bwd (query)");
  }
  hipLaunchKernelGGL(asp_finish_kernel, dim3((d.npart + 255) / 256), dim3(256), 0, st, d, (const float *)part, nblk,
                     dW0, db0, dW1, db1, dw, dw0);
  RM_CHECK_LAUNCH("rm_asp_bwd (finish)");
  return RM_OK;
}
