// Transformer-pooled behaviour sequences - SequenceFeat + one post-norm encoder block (Behavior Sequence Transformer,
// arXiv 1905.06874).  Nothing in the reference implements it.  Per example b with query row q (columns 0..D-1 of the
// candidate item's table row) and history rows k_0..k_{n-1} of the SAME table block (CSR, oldest first), T = n + 1 tokens:
//     x_i = k_i + P[n - i]  (i < n),   x_n = q + P[0]                       P [max_len + 1, D]: distance from the candidate
//     Q, K, V = X Wq + bq, ..;   a^h = softmax_j(Q^h_i . K^h_j / sqrt(dk))  (max-subtracted);   O = concat_h(a^h V^h) Wo + bo
//     Y = LN(X + O; g1, b1);   Z = LN(Y + relu(Y W1 + c1) W2 + c2; g2, b2)   (eps 1e-5, biased variance)
//     out_b = (1 / T) sum_i Z_i                                              (no history: T = 1, out_b = Z_0)
// rm_bst_fwd writes out_b into a fused scratch row (columns 0..D-1, zeros behind) that the gather kernel reads like any
// table row.  Nothing per token reaches HBM: the forward saves nothing and the backward recomputes the block.
//
// Mapping.  One 256-thread block owns a contiguous chunk of examples (a FIXED assignment: chunk = ceil(B / blocks)) and
// walks it in steps; a step packs whole consecutive examples while their tokens fit a tile of 64 rows (wave 0: the
// lengths from `offsets`, a prefix sum by shuffles, no host sync).  The tile's X, Q, K, V, the attention output, both
// LayerNorm inputs, Y, the hidden activations [64, Hf] and one gradient buffer live in LDS (row strides D + 1 and
// Hf + 1: odd, so column walks of a transposed product are conflict-free); the weights, packed with the same odd
// strides, are copied into LDS once per block when they fit beside the tile (every shape but D = 32 with Hf > 116) and
// are read through the caches otherwise.  The small products run on the vector ALU, one output element per thread and
// pass, two LDS reads per multiply-add.  The matrix pipe is NOT used: v_mfma_f32_16x16x4_f32 with tokens on M would
// cut the LDS reads per multiply-add sixteen-fold, and LDS reads are what bounds these kernels - it was left out to
// keep one code path for every step height (1..64 ragged rows) and every Hf, and is the first thing to do next
// (profiles/bst.md).  Attention: one thread per (token, head), two passes over the example's keys, the head's dk
// outputs in registers.
//   forward : bst_pack_kernel + bst_fwd_kernel.
//   backward: bst_pack_kernel + bst_bwd_kernel (recompute; dZ .. dX in LDS; every parameter gradient accumulates in
//             registers over all tiles of the block and is written once as the block's partial) + rm_sum_partials (partials summed in block order).
// LayerNorm statistics: float32, two passes over the D <= 32 values of a row (mean, then the centred squares).
// No float atomics anywhere, every sum in a fixed order: two runs are bit-equal.
#include <math.h>

#include "rm_launch.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;                // token rows per step (max_len + 1 <= 64)
constexpr int kMaxHeads = 8;
constexpr int kMaxBlocks = 512;          // two blocks per CU
constexpr int kMinChunk = 16;            // examples per block at least
constexpr size_t kLdsMax = 160 * 1024;   // per CU (and per block) on gfx950
constexpr float kLnEps = 1e-5f;

inline int64_t rup4(int64_t v) { return (v + 3) / 4 * 4; }

struct BstDims {
  int D, h, dk, Hf, ML;  // ML = max_len
  int SD, SH;            // row strides D + 1 and Hf + 1
  // the packed parameter block (floats): Wq Wk Wv Wo [D][SD], W1 [D][SH], W2 [Hf][SD], then the vectors
  int oWq, oWk, oWv, oWo, oW1, oW2, obq, obk, obv, obo, oc1, oc2, og1, ob1, og2, ob2, nparam;
  // the five sets of partial sums of a block: (dWq dWk dWv dWo) (dbq dbk dbv dbo) (dW1 dc1 dW2 dc2) (dg1 db1 dg2 db2) (dP)
  int nA, nB, nC, nG, nP;
};

__host__ __device__ inline BstDims bst_dims(int D, int h, int Hf, int ML) {
  BstDims d;
  d.D = D; d.h = h; d.dk = D / h; d.Hf = Hf; d.ML = ML;
  d.SD = D + 1; d.SH = Hf + 1;
  d.oWq = 0; d.oWk = D * d.SD; d.oWv = 2 * D * d.SD; d.oWo = 3 * D * d.SD;
  d.oW1 = 4 * D * d.SD; d.oW2 = d.oW1 + D * d.SH;
  d.obq = d.oW2 + Hf * d.SD; d.obk = d.obq + D; d.obv = d.obk + D; d.obo = d.obv + D;
  d.oc1 = d.obo + D; d.oc2 = d.oc1 + Hf;
  d.og1 = d.oc2 + D; d.ob1 = d.og1 + D; d.og2 = d.ob1 + D; d.ob2 = d.og2 + D;
  d.nparam = (d.ob2 + D + 3) / 4 * 4;
  d.nA = 4 * D * D; d.nB = 4 * D; d.nC = 2 * D * Hf + Hf + D; d.nG = 4 * D; d.nP = (ML + 1) * D;
  return d;
}

inline bool bst_shape_ok(int D, int h, int Hf, int ML) {
  if (!(D == 8 || D == 16 || D == 32)) return false;
  if (!(h == 1 || h == 2 || h == 4 || h == 8) || D / h < 4) return false;
  if (Hf < 4 || Hf > 128 || Hf % 4) return false;
  return ML >= 1 && ML <= kTile - 1;
}

// floats of LDS of the tile: 9 buffers [64][SD], the hidden activations [64][SH], rstd1, rstd2, the softmax
// maxima, denominators and the deltas [64][8], then the tile's bookkeeping (ints)
inline size_t bst_tile_floats(const BstDims &d) {
  return (size_t)9 * kTile * d.SD + (size_t)kTile * d.SH + 2 * kTile + 3 * kTile * kMaxHeads + 2 * kTile /* ex_off */ +
         4 * kTile + 4;
}
struct BstCfg {
  bool wlds;
  size_t smem;
};
BstCfg bst_cfg(const BstDims &d) {
  const size_t tile = rup4((int64_t)bst_tile_floats(d));
  if (4 * (tile + d.nparam) <= kLdsMax) return {true, 4 * (tile + d.nparam)};
  return {false, 4 * tile};
}

inline int bst_blocks(int64_t B) { return rm_grid_cap((B + kMinChunk - 1) / kMinChunk, kMaxBlocks); }

// the 16 packed parameters: source, rows x cols, at off[] with row stride ld
struct BstPack {
  const float *src[16];
  int off[16], cols[16], ld[16], len[16];
};

__global__ void bst_pack_kernel(BstPack p, int nparam, float *__restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nparam) return;
  float v = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    if (e >= p.off[s] && e < p.off[s] + p.len[s]) {
      const int q = e - p.off[s], r = q / p.ld[s], c = q - r * p.ld[s];
      if (c < p.cols[s]) v = p.src[s][r * p.cols[s] + c];
    }
  }
  out[e] = v;
}

struct BstIn {
  const float *rows;
  int64_t LD, row0;
  const int64_t *offsets, *ids, *qrow;
  int64_t B;
  const float *P;  // the position table [ML + 1, D]
};

struct BstLds {
  float *X, *Q, *K, *V, *A, *N1, *Y, *N2, *G, *HH;  // N1 / N2: the LayerNorm inputs, then their normalised values
  float *rstd1, *rstd2, *sm, *sden, *sdel;
  long long *ex_off;                                // CSR start of every example of the tile
  int *ex_n, *ex_t0, *ex_cut, *row_ex, *misc;       // history length, first row, items cut off an over-long history;
                                                    // the example of every row; {nex, R}
  const float *W;                                   // the packed parameters
};

// the packed parameters: copied behind the tile (WLDS) or read where they are
template <bool WLDS>
__device__ __forceinline__ const float *bst_stage_weights(int nparam, float *sm, const float *params, size_t tile_floats) {
  if constexpr (WLDS) {
    float *w = sm + tile_floats;
    for (int i = threadIdx.x; i < nparam; i += kThreads) w[i] = params[i];
    return w;  // (the first barrier of the tile loop publishes it)
  } else {
    return params;
  }
}

__device__ __forceinline__ BstLds bst_lds(const BstDims &d, float *sm, const float *W) {
  BstLds l;
  const int nb = kTile * d.SD;
  l.X = sm; l.Q = l.X + nb; l.K = l.Q + nb; l.V = l.K + nb; l.A = l.V + nb; l.N1 = l.A + nb; l.Y = l.N1 + nb;
  l.N2 = l.Y + nb; l.G = l.N2 + nb; l.HH = l.G + nb;
  l.rstd1 = l.HH + kTile * d.SH; l.rstd2 = l.rstd1 + kTile;
  l.sm = l.rstd2 + kTile; l.sden = l.sm + kTile * kMaxHeads; l.sdel = l.sden + kTile * kMaxHeads;
  float *p = l.sdel + kTile * kMaxHeads;
  // (every buffer above is a multiple of 64 floats: p is 8-byte aligned)
  l.ex_off = reinterpret_cast<long long *>(p);
  l.ex_n = reinterpret_cast<int *>(p + 2 * kTile);
  l.ex_t0 = l.ex_n + kTile; l.ex_cut = l.ex_t0 + kTile; l.row_ex = l.ex_cut + kTile; l.misc = l.row_ex + kTile;
  l.W = W;
  return l;
}

// The shape, re-derived at the top of every step from values the compiler cannot see through: offsets, strides and
// LDS pointers are then a few scalar operations per step instead of a hundred registers held across the tile loop
// (which the compiler spilled).
#define RM_BST_STEP_SHAPE()                                      \
  int D_ = D0, Hf_ = Hf0;                                        \
  asm volatile("" : "+s"(D_), "+s"(Hf_));                        \
  const BstDims d = bst_dims(D_, heads, Hf_, ML);                \
  const BstLds l = bst_lds(d, sm, W)

// out(r, n) = sum_k A[r sa + k] W[k sw + n] for r < R, n < N: one element per thread and pass
template <class Epi>
__device__ __forceinline__ void bst_mm(int R, int N, int K, const float *A, int sa, const float *W, int sw, Epi epi) {
  for (int e = threadIdx.x; e < R * N; e += kThreads) {
    const int r = e / N, n = e - r * N;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf(A[r * sa + k], W[k * sw + n], s);
    epi(r, n, s);
  }
}
// out(r, n) = sum_k A[r sa + k] W[n sw + k]  (the product with W^T)
template <class Epi>
__device__ __forceinline__ void bst_mmT(int R, int N, int K, const float *A, int sa, const float *W, int sw, Epi epi) {
  for (int e = threadIdx.x; e < R * N; e += kThreads) {
    const int r = e / N, n = e - r * N;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf(A[r * sa + k], W[n * sw + k], s);
    epi(r, n, s);
  }
}
// acc[s] += sum_{r < R} A[r sa + i] G[r sg + j] for element e = tid + 256 s = i NJ + j < NI NJ (a weight gradient);
// the threads of slot 0 with e < NJ also add the column sum of G (the bias gradient) onto *col
template <int S>
__device__ __forceinline__ void bst_wgrad(float (&acc)[S], float *col, int R, int NI, int NJ, const float *A, int sa,
                                          const float *G, int sg) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int e = threadIdx.x + kThreads * s;
    if (e < NI * NJ) {
      const int i = e / NJ, j = e - i * NJ;
      float t = 0.f, cs = 0.f;
      for (int r = 0; r < R; ++r) {
        const float g = G[r * sg + j];
        t = fmaf(A[r * sa + i], g, t);
        cs += g;
      }
      acc[s] += t;
      if (s == 0 && e < NJ) *col += cs;
    }
  }
}

__device__ __forceinline__ float bst_sum4(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// LayerNorm of the rows of N (in place: N becomes the normalised rows), 4 lanes per row; Yout = N gamma + beta
__device__ __forceinline__ void bst_layernorm(int R, int D, int SD, float *N, float *rstd, const float *gamma,
                                              const float *beta, float *Yout) {
  const int r = threadIdx.x >> 2, l = threadIdx.x & 3;
  const bool on = r < R;
  float s = 0.f;
  if (on)
    for (int c = l; c < D; c += 4) s += N[r * SD + c];
  const float mean = bst_sum4(s) / (float)D;
  float v = 0.f;
  if (on)
    for (int c = l; c < D; c += 4) {
      const float t = N[r * SD + c] - mean;
      v = fmaf(t, t, v);
    }
  const float rs = 1.0f / sqrtf(bst_sum4(v) / (float)D + kLnEps);
  if (on) {
    for (int c = l; c < D; c += 4) {
      const float xh = (N[r * SD + c] - mean) * rs;
      N[r * SD + c] = xh;
      Yout[r * SD + c] = fmaf(xh, gamma[c], beta[c]);
    }
    if (l == 0) rstd[r] = rs;
  }
}

// G (the gradient of the LayerNorm's output) -> the gradient of its input, in place; xh: the normalised rows
__device__ __forceinline__ void bst_layernorm_bwd(int R, int D, int SD, float *G, const float *xh, const float *rstd,
                                                  const float *gamma) {
  const int r = threadIdx.x >> 2, l = threadIdx.x & 3;
  const bool on = r < R;
  float s1 = 0.f, s2 = 0.f;
  if (on)
    for (int c = l; c < D; c += 4) {
      const float t = G[r * SD + c] * gamma[c];
      s1 += t;
      s2 = fmaf(t, xh[r * SD + c], s2);
    }
  const float m1 = bst_sum4(s1) / (float)D, m2 = bst_sum4(s2) / (float)D;
  if (on) {
    const float rs = rstd[r];
    for (int c = l; c < D; c += 4) {
      const float t = G[r * SD + c] * gamma[c];
      G[r * SD + c] = rs * (t - m1 - xh[r * SD + c] * m2);
    }
  }
}

// One step: packs examples from b_cur on (below b_end) into the tile and runs the block's forward on them.
// Leaves X, Q, K, V, A, N1 = xhat1, Y, HH, N2 = xhat2, the statistics, and Z (the block's output rows) in G.
// Returns the number of examples taken (>= 1); ends on a barrier.
template <int DK>
__device__ __forceinline__ int bst_tile_forward(const BstDims &d, const BstIn &in, const BstLds &l, int64_t b_cur,
                                                int64_t b_end) {
  const int tid = threadIdx.x, D = d.D, SD = d.SD, SH = d.SH, Hf = d.Hf;
  const float *W = l.W;
  __syncthreads();  // the previous step is done with the tile
  if (tid < kTile) {
    const int64_t b = b_cur + tid;
    const bool live = b < b_end;
    int n = 0, cut = 0;
    long long o0 = 0;
    if (live) {
      o0 = in.offsets[b];
      const long long len = in.offsets[b + 1] - o0;
      n = len < 0 ? 0 : (len > d.ML ? d.ML : (int)len);
      cut = len > d.ML ? (int)(len - d.ML) : 0;  // a longer history keeps its LAST max_len items (as th.SequenceFeat)
      o0 += cut;
    }
    const int T = live ? n + 1 : 0;
    int incl = T;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (tid >= o) incl += v;
    }
    const bool ok = live && incl <= kTile;  // (T >= 1: incl grows strictly, the set is a prefix; T <= 64: never empty)
    const int nex = __popcll(__ballot(ok));
    if (ok) {
      l.ex_n[tid] = n; l.ex_t0[tid] = incl - T; l.ex_off[tid] = o0; l.ex_cut[tid] = cut;
      for (int i = 0; i < T; ++i) l.row_ex[incl - T + i] = tid;
    }
    if (tid == nex - 1) { l.misc[0] = nex; l.misc[1] = incl; }
  }
  __syncthreads();
  const int nex = l.misc[0], R = l.misc[1];
  // X: the rows plus their position rows
  for (int e = tid; e < R * D; e += kThreads) {
    const int r = e / D, c = e - r * D, ex = l.row_ex[r];
    const int n = l.ex_n[ex], i = r - l.ex_t0[ex];
    const int64_t src = i < n ? in.row0 + in.ids[l.ex_off[ex] + i] : in.qrow[b_cur + ex];
    l.X[r * SD + c] = in.rows[src * in.LD + c] + in.P[(n - i) * D + c];
  }
  __syncthreads();
  bst_mm(R, D, D, l.X, SD, W + d.oWq, SD, [&](int r, int n, float v) { l.Q[r * SD + n] = v + W[d.obq + n]; });
  bst_mm(R, D, D, l.X, SD, W + d.oWk, SD, [&](int r, int n, float v) { l.K[r * SD + n] = v + W[d.obk + n]; });
  bst_mm(R, D, D, l.X, SD, W + d.oWv, SD, [&](int r, int n, float v) { l.V[r * SD + n] = v + W[d.obv + n]; });
  __syncthreads();
  // attention: one thread per (token, head)
  const float scale = 1.0f / sqrtf((float)DK);
  for (int w = tid; w < R * d.h; w += kThreads) {
    const int hd = w / R, r = w - hd * R, ex = l.row_ex[r];
    const int t0 = l.ex_t0[ex], T = l.ex_n[ex] + 1;
    const float *q = l.Q + r * SD + hd * DK;
    float m = -INFINITY;
    for (int j = 0; j < T; ++j) {
      const float *k = l.K + (t0 + j) * SD + hd * DK;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < DK; ++c) s = fmaf(q[c], k[c], s);
      m = fmaxf(m, s * scale);
    }
    float den = 0.f, acc[DK];
#pragma unroll
    for (int c = 0; c < DK; ++c) acc[c] = 0.f;
    for (int j = 0; j < T; ++j) {
      const float *k = l.K + (t0 + j) * SD + hd * DK, *v = l.V + (t0 + j) * SD + hd * DK;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < DK; ++c) s = fmaf(q[c], k[c], s);
      const float p = expf(s * scale - m);
      den += p;
#pragma unroll
      for (int c = 0; c < DK; ++c) acc[c] = fmaf(p, v[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < DK; ++c) l.A[r * SD + hd * DK + c] = acc[c] / den;
    l.sm[r * kMaxHeads + hd] = m;
    l.sden[r * kMaxHeads + hd] = den;
  }
  __syncthreads();
  bst_mm(R, D, D, l.A, SD, W + d.oWo, SD,
         [&](int r, int n, float v) { l.N1[r * SD + n] = l.X[r * SD + n] + (v + W[d.obo + n]); });
  __syncthreads();
  bst_layernorm(R, D, SD, l.N1, l.rstd1, W + d.og1, W + d.ob1, l.Y);
  __syncthreads();
  bst_mm(R, Hf, D, l.Y, SD, W + d.oW1, SH, [&](int r, int n, float v) { l.HH[r * SH + n] = fmaxf(v + W[d.oc1 + n], 0.f); });
  __syncthreads();
  bst_mm(R, D, Hf, l.HH, SH, W + d.oW2, SD,
         [&](int r, int n, float v) { l.N2[r * SD + n] = l.Y[r * SD + n] + (v + W[d.oc2 + n]); });
  __syncthreads();
  bst_layernorm(R, D, SD, l.N2, l.rstd2, W + d.og2, W + d.ob2, l.G);  // (Z: the backward overwrites it)
  __syncthreads();
  return nex;
}

// ------------------------------------------------------------------------------------------------ forward
template <int DK, bool WLDS>
__global__ __launch_bounds__(kThreads) void bst_fwd_kernel(int D0, int heads, int Hf0, int ML, int nparam, BstIn in,
                                                           const float *__restrict__ params, int64_t chunk,
                                                           size_t tile_floats, float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const float *W = bst_stage_weights<WLDS>(nparam, sm, params, tile_floats);
  const int tid = threadIdx.x;
  const int LD = (int)in.LD;
  int64_t b = (int64_t)blockIdx.x * chunk;
  const int64_t b_end = b + chunk < in.B ? b + chunk : in.B;
  while (b < b_end) {
    RM_BST_STEP_SHAPE();
    const int D = d.D, SD = d.SD;
    const int nex = bst_tile_forward<DK>(d, in, l, b, b_end);
    for (int e = tid; e < nex * LD; e += kThreads) {  // the mean over the example's tokens; zeros behind column D
      const int ex = e / LD, c = e - ex * LD;
      float s = 0.f;
      if (c < D) {
        const int t0 = l.ex_t0[ex], T = l.ex_n[ex] + 1;
        for (int i = 0; i < T; ++i) s += l.G[(t0 + i) * SD + c];
        s /= (float)T;
      }
      out[(b + ex) * in.LD + c] = s;
    }
    b += nex;
  }
}

// ----------------------------------------------------------------------------------------------- backward
struct BstBwd {
  const float *d_out;
  int64_t do_stride;
  float *d_keys, *d_query;
  int64_t dq_stride;
  float *part;  // this launch's partial sets: [blocks][nA], [blocks][nB], [blocks][nC], [blocks][nG], [blocks][nP]
};

// (two waves per SIMD, so that two blocks share a CU where their LDS allows it - the default shape; dk = 32 means
// D = 32, whose tile leaves room for one block only, and its registers would not fit the half file without scratch)
template <int DK, bool WLDS>
__global__ __launch_bounds__(kThreads, DK == 32 ? 1 : 2) void bst_bwd_kernel(int D0, int heads, int Hf0, int ML, int nparam, BstIn in,
                                                           const float *__restrict__ params, int64_t chunk,
                                                           size_t tile_floats, BstBwd o) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const float *W = bst_stage_weights<WLDS>(nparam, sm, params, tile_floats);
  const int tid = threadIdx.x;
  const float scale = 1.0f / sqrtf((float)DK);

  // element tid + 256 s of a matrix: D D <= 4 slots, D Hf <= 16, (ML + 1) D <= 8
  float aWq[4], aWk[4], aWv[4], aWo[4], aW1[16], aW2[16], aP[8];
#pragma unroll
  for (int s = 0; s < 4; ++s) aWq[s] = aWk[s] = aWv[s] = aWo[s] = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) aW1[s] = aW2[s] = 0.f;
#pragma unroll
  for (int s = 0; s < 8; ++s) aP[s] = 0.f;
  // thread c < D: column c of the D-vectors; thread u < Hf: unit u of dc1
  float vbq = 0.f, vbk = 0.f, vbv = 0.f, vbo = 0.f, vc1 = 0.f, vc2 = 0.f, vg1 = 0.f, vb1 = 0.f, vg2 = 0.f, vb2 = 0.f;

  int64_t b = (int64_t)blockIdx.x * chunk;
  const int64_t b_end = b + chunk < in.B ? b + chunk : in.B;
  while (b < b_end) {
    RM_BST_STEP_SHAPE();
    const int D = d.D, SD = d.SD, SH = d.SH, Hf = d.Hf;
    const int nex = bst_tile_forward<DK>(d, in, l, b, b_end);
    const int R = l.misc[1];
    // G = dZ: the pooled row's gradient over the example's T tokens
    for (int e = tid; e < R * D; e += kThreads) {
      const int r = e / D, c = e - r * D, ex = l.row_ex[r];
      l.G[r * SD + c] = o.d_out[(b + ex) * o.do_stride + c] / (float)(l.ex_n[ex] + 1);
    }
    __syncthreads();
    if (tid < D) {  // dg2, db2
      float sg = 0.f, sb = 0.f;
      for (int r = 0; r < R; ++r) {
        const float g = l.G[r * SD + tid];
        sg = fmaf(g, l.N2[r * SD + tid], sg);
        sb += g;
      }
      vg2 += sg; vb2 += sb;
    }
    __syncthreads();
    bst_layernorm_bwd(R, D, SD, l.G, l.N2, l.rstd2, W + d.og2);  // G = dS2 (= the residual's share of dY)
    __syncthreads();
    bst_wgrad(aW2, &vc2, R, Hf, D, l.HH, SH, l.G, SD);
    __syncthreads();
    // HH = d(hidden pre-activation) in place
    bst_mmT(R, Hf, D, l.G, SD, W + d.oW2, SD,
            [&](int r, int n, float v) { l.HH[r * SH + n] = l.HH[r * SH + n] > 0.f ? v : 0.f; });
    __syncthreads();
    bst_wgrad(aW1, &vc1, R, D, Hf, l.Y, SD, l.HH, SH);
    bst_mmT(R, D, Hf, l.HH, SH, W + d.oW1, SH, [&](int r, int n, float v) { l.G[r * SD + n] += v; });  // G = dY
    __syncthreads();
    if (tid < D) {  // dg1, db1
      float sg = 0.f, sb = 0.f;
      for (int r = 0; r < R; ++r) {
        const float g = l.G[r * SD + tid];
        sg = fmaf(g, l.N1[r * SD + tid], sg);
        sb += g;
      }
      vg1 += sg; vb1 += sb;
    }
    __syncthreads();
    bst_layernorm_bwd(R, D, SD, l.G, l.N1, l.rstd1, W + d.og1);  // G = dS1 (= the residual's share of dX)
    __syncthreads();
    bst_wgrad(aWo, &vbo, R, D, D, l.A, SD, l.G, SD);
    float *dA = l.N2;  // (xhat2 is used up)
    bst_mmT(R, D, D, l.G, SD, W + d.oWo, SD, [&](int r, int n, float v) { dA[r * SD + n] = v; });
    __syncthreads();
    // delta_i^h = sum_j a_ij (dA_i . V_j) = dA_i^h . A_i^h
    for (int w = tid; w < R * d.h; w += kThreads) {
      const int hd = w / R, r = w - hd * R;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < DK; ++c) s = fmaf(dA[r * SD + hd * DK + c], l.A[r * SD + hd * DK + c], s);
      l.sdel[r * kMaxHeads + hd] = s;
    }
    __syncthreads();
    float *dQ = l.N1, *dK = l.Y, *dV = l.A;  // (xhat1, Y and the attention output are used up)
    for (int w = tid; w < R * d.h; w += kThreads) {
      const int hd = w / R, r = w - hd * R, ex = l.row_ex[r];
      const int t0 = l.ex_t0[ex], T = l.ex_n[ex] + 1, hc = hd * DK;
      {  // token r as the query: dQ_r = scale sum_j ds_rj K_j,  ds_rj = a_rj (dA_r . V_j - delta_r)
        const float *q = l.Q + r * SD + hc, *da = dA + r * SD + hc;
        const float m = l.sm[r * kMaxHeads + hd], den = l.sden[r * kMaxHeads + hd], del = l.sdel[r * kMaxHeads + hd];
        float acc[DK];
#pragma unroll
        for (int c = 0; c < DK; ++c) acc[c] = 0.f;
        for (int j = 0; j < T; ++j) {
          const float *k = l.K + (t0 + j) * SD + hc, *v = l.V + (t0 + j) * SD + hc;
          float s = 0.f, dp = 0.f;
#pragma unroll
          for (int c = 0; c < DK; ++c) {
            s = fmaf(q[c], k[c], s);
            dp = fmaf(da[c], v[c], dp);
          }
          const float ds = expf(s * scale - m) / den * (dp - del);
#pragma unroll
          for (int c = 0; c < DK; ++c) acc[c] = fmaf(ds, k[c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < DK; ++c) dQ[r * SD + hc + c] = acc[c] * scale;
      }
      {  // token r as the key: dK_r = scale sum_i ds_ir Q_i,  dV_r = sum_i a_ir dA_i
        const float *k = l.K + r * SD + hc, *v = l.V + r * SD + hc;
        float ak[DK], av[DK];
#pragma unroll
        for (int c = 0; c < DK; ++c) ak[c] = av[c] = 0.f;
        for (int i = 0; i < T; ++i) {
          const int ri = t0 + i;
          const float *q = l.Q + ri * SD + hc, *da = dA + ri * SD + hc;
          float s = 0.f, dp = 0.f;
#pragma unroll
          for (int c = 0; c < DK; ++c) {
            s = fmaf(q[c], k[c], s);
            dp = fmaf(da[c], v[c], dp);
          }
          const float a = expf(s * scale - l.sm[ri * kMaxHeads + hd]) / l.sden[ri * kMaxHeads + hd];
          const float ds = a * (dp - l.sdel[ri * kMaxHeads + hd]);
#pragma unroll
          for (int c = 0; c < DK; ++c) {
            ak[c] = fmaf(ds, q[c], ak[c]);
            av[c] = fmaf(a, da[c], av[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < DK; ++c) {
          dK[r * SD + hc + c] = ak[c] * scale;
          dV[r * SD + hc + c] = av[c];
        }
      }
    }
    __syncthreads();
    bst_wgrad(aWq, &vbq, R, D, D, l.X, SD, dQ, SD);
    bst_wgrad(aWk, &vbk, R, D, D, l.X, SD, dK, SD);
    bst_wgrad(aWv, &vbv, R, D, D, l.X, SD, dV, SD);
    bst_mmT(R, D, D, dQ, SD, W + d.oWq, SD, [&](int r, int n, float v) { l.G[r * SD + n] += v; });
    bst_mmT(R, D, D, dK, SD, W + d.oWk, SD, [&](int r, int n, float v) { l.G[r * SD + n] += v; });
    bst_mmT(R, D, D, dV, SD, W + d.oWv, SD, [&](int r, int n, float v) { l.G[r * SD + n] += v; });  // G = dX
    __syncthreads();
    // dX: history tokens -> d_keys, the candidate -> ADDED onto d_query; every token -> its position row
    for (int e = tid; e < R * D; e += kThreads) {
      const int r = e / D, c = e - r * D, ex = l.row_ex[r];
      const int n = l.ex_n[ex], i = r - l.ex_t0[ex];
      const float g = l.G[r * SD + c];
      if (i < n) o.d_keys[(l.ex_off[ex] + i) * D + c] = g;
      else o.d_query[(b + ex) * o.dq_stride + c] += g;
    }
    if (tid < nex && l.ex_cut[tid] > 0) {  // the occurrences cut off an over-long history: zero key gradients
      const int cut = l.ex_cut[tid];
      float *z = o.d_keys + (l.ex_off[tid] - cut) * D;
      for (int i = 0; i < cut * D; ++i) z[i] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int e = tid + kThreads * s;
      if (e < d.nP) {
        const int dist = e / D, c = e - dist * D;
        float t = 0.f;
        for (int ex = 0; ex < nex; ++ex) {
          const int n = l.ex_n[ex];
          if (dist <= n) t += l.G[(l.ex_t0[ex] + n - dist) * SD + c];
        }
        aP[s] += t;
      }
    }
    b += nex;
  }
  // the block's partial sums
  const BstDims d = bst_dims(D0, heads, Hf0, ML);
  const int D = D0, Hf = Hf0, DD = D * D, DH = D * Hf;
  const int64_t nblk = gridDim.x, blk = blockIdx.x;
  float *pA = o.part + blk * d.nA, *pB = o.part + nblk * d.nA + blk * d.nB;
  float *pC = o.part + nblk * (d.nA + d.nB) + blk * d.nC, *pG = o.part + nblk * (d.nA + d.nB + d.nC) + blk * d.nG;
  float *pP = o.part + nblk * (d.nA + d.nB + d.nC + d.nG) + blk * d.nP;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = tid + kThreads * s;
    if (e < DD) {
      pA[e] = aWq[s]; pA[DD + e] = aWk[s]; pA[2 * DD + e] = aWv[s]; pA[3 * DD + e] = aWo[s];
    }
  }
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int e = tid + kThreads * s;
    if (e < DH) {
      pC[e] = aW1[s];
      pC[DH + Hf + e] = aW2[s];
    }
  }
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int e = tid + kThreads * s;
    if (e < d.nP) pP[e] = aP[s];
  }
  if (tid < Hf) pC[DH + tid] = vc1;
  if (tid < D) {
    pB[tid] = vbq; pB[D + tid] = vbk; pB[2 * D + tid] = vbv; pB[3 * D + tid] = vbo;
    pC[2 * DH + Hf + tid] = vc2;
    pG[tid] = vg1; pG[D + tid] = vb1; pG[2 * D + tid] = vg2; pG[3 * D + tid] = vb2;
  }
}

int bst_check(const char *fn, int D, int h, int Hf, int ML, int64_t B, int64_t nnz, int64_t LD) {
  RM_REQUIRE(bst_shape_ok(D, h, Hf, ML),
             "%s: unsupported shape D=%d heads=%d Hf=%d max_len=%d (D in {8,16,32}, heads in {1,2,4,8} with D / heads >= 4, "
             "Hf a multiple of 4 in 4..128, max_len 1..63)", fn, D, h, Hf, ML);
  return rm_seq_check_sizes(fn, D, B, nnz, LD);
}

int bst_params_ok(const char *fn, const char *what, const rm_bst_params *p) {
  RM_REQUIRE(p && p->wq && p->wk && p->wv && p->wo && p->bq && p->bk && p->bv && p->bo && p->ffn_w1 && p->ffn_b1 &&
                 p->ffn_w2 && p->ffn_b2 && p->ln1_gamma && p->ln1_beta && p->ln2_gamma && p->ln2_beta && p->pos,
             "%s: %s has a NULL member", fn, what);
  return RM_OK;
}

void bst_pack(const BstDims &d, const rm_bst_params *p, float *out, hipStream_t st) {
  const int D = d.D, Hf = d.Hf;
  BstPack k;
  auto set = [&](int s, const float *src, int off, int rows, int cols, int ld) {
    k.src[s] = src; k.off[s] = off; k.cols[s] = cols; k.ld[s] = ld; k.len[s] = rows * ld;
  };
  set(0, p->wq, d.oWq, D, D, d.SD); set(1, p->wk, d.oWk, D, D, d.SD); set(2, p->wv, d.oWv, D, D, d.SD);
  set(3, p->wo, d.oWo, D, D, d.SD); set(4, p->ffn_w1, d.oW1, D, Hf, d.SH); set(5, p->ffn_w2, d.oW2, Hf, D, d.SD);
  set(6, p->bq, d.obq, 1, D, D); set(7, p->bk, d.obk, 1, D, D); set(8, p->bv, d.obv, 1, D, D);
  set(9, p->bo, d.obo, 1, D, D); set(10, p->ffn_b1, d.oc1, 1, Hf, Hf); set(11, p->ffn_b2, d.oc2, 1, D, D);
  set(12, p->ln1_gamma, d.og1, 1, D, D); set(13, p->ln1_beta, d.ob1, 1, D, D);
  set(14, p->ln2_gamma, d.og2, 1, D, D); set(15, p->ln2_beta, d.ob2, 1, D, D);
  hipLaunchKernelGGL(bst_pack_kernel, dim3((d.nparam + 255) / 256), dim3(256), 0, st, k, d.nparam, out);
}

}  // namespace

extern "C" int rm_bst_supported(int D, int heads, int Hf, int max_len) { return bst_shape_ok(D, heads, Hf, max_len) ? 1 : 0; }

extern "C" int64_t rm_bst_workspace(int D, int heads, int Hf, int max_len, int64_t B, int backward) {
  if (!bst_shape_ok(D, heads, Hf, max_len) || B < 0) return 0;
  const BstDims d = bst_dims(D, heads, Hf, max_len);
  if (!backward) return d.nparam;
  return d.nparam + (int64_t)bst_blocks(B) * (d.nA + d.nB + d.nC + d.nG + d.nP);
}

#define RM_BST_LAUNCH(KERNEL_, ...)                                                                              \
  do {                                                                                                           \
    const dim3 grid_(nblk), block_(kThreads);                                                                    \
    if (c.wlds) {                                                                                                \
      switch (d.dk) {                                                                                            \
        case 4: rm_launch_lds(KERNEL_<4, true>, grid_, block_, c.smem, st, __VA_ARGS__); break;                 \
        case 8: rm_launch_lds(KERNEL_<8, true>, grid_, block_, c.smem, st, __VA_ARGS__); break;                 \
        case 16: rm_launch_lds(KERNEL_<16, true>, grid_, block_, c.smem, st, __VA_ARGS__); break;               \
        default: rm_launch_lds(KERNEL_<32, true>, grid_, block_, c.smem, st, __VA_ARGS__); break;               \
      }                                                                                                          \
    } else {                                                                                                     \
      switch (d.dk) {                                                                                            \
        case 4: rm_launch_lds(KERNEL_<4, false>, grid_, block_, c.smem, st, __VA_ARGS__); break;                \
        case 8: rm_launch_lds(KERNEL_<8, false>, grid_, block_, c.smem, st, __VA_ARGS__); break;                \
        case 16: rm_launch_lds(KERNEL_<16, false>, grid_, block_, c.smem, st, __VA_ARGS__); break;              \
        default: rm_launch_lds(KERNEL_<32, false>, grid_, block_, c.smem, st, __VA_ARGS__); break;              \
      }                                                                                                          \
    }                                                                                                            \
  } while (0)

extern "C" int rm_bst_fwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                          const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
                          const rm_bst_params *params, int heads, int Hf, int max_len, float *out, float *workspace,
                          rm_stream_t stream) {
  int rc = bst_check("rm_bst_fwd", D, heads, Hf, max_len, B, nnz, LD);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  if ((rc = bst_params_ok("rm_bst_fwd", "params", params)) != RM_OK) return rc;
  if ((rc = rm_seq_check_fwd("rm_bst_fwd", rows, offsets, ids, qrow, nnz, out, workspace)) != RM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const BstDims d = bst_dims(D, heads, Hf, max_len);
  const BstCfg c = bst_cfg(d);
  const BstIn in{rows, LD, row0, offsets, ids, qrow, B, params->pos};
  bst_pack(d, params, workspace, st);
  RM_CHECK_LAUNCH("rm_bst_fwd (pack)");
  const int nblk = bst_blocks(B);
  const int64_t chunk = (B + nblk - 1) / nblk;
  const size_t tile = (size_t)rup4((int64_t)bst_tile_floats(d));
  RM_BST_LAUNCH(bst_fwd_kernel, D, heads, Hf, max_len, d.nparam, in, (const float *)workspace, chunk, tile, out);
  RM_CHECK_LAUNCH("rm_bst_fwd");
  return RM_OK;
}

extern "C" int rm_bst_bwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                          const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
                          const rm_bst_params *params, int heads, int Hf, int max_len, const float *d_out,
                          int64_t do_stride, float *d_keys, float *d_query, int64_t dq_stride,
                          const rm_bst_params *grads, float *workspace, rm_stream_t stream) {
  int rc = bst_check("rm_bst_bwd", D, heads, Hf, max_len, B, nnz, LD);
  if (rc != RM_OK) return rc;
  if ((rc = bst_params_ok("rm_bst_bwd", "params", params)) != RM_OK) return rc;
  if ((rc = bst_params_ok("rm_bst_bwd", "grads", grads)) != RM_OK) return rc;
  if ((rc = rm_seq_check_bwd("rm_bst_bwd", D, rows, offsets, ids, qrow, B, nnz, d_out, do_stride, d_keys, d_query,
                             dq_stride, workspace)) != RM_OK)
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const BstDims d = bst_dims(D, heads, Hf, max_len);
  const BstCfg c = bst_cfg(d);
  const int nblk = B > 0 ? bst_blocks(B) : 0;
  float *partA = workspace + d.nparam, *partB = partA + (int64_t)nblk * d.nA, *partC = partB + (int64_t)nblk * d.nB;
  float *partG = partC + (int64_t)nblk * d.nC, *partP = partG + (int64_t)nblk * d.nG;
  if (B > 0) {
    const BstIn in{rows, LD, row0, offsets, ids, qrow, B, params->pos};
    bst_pack(d, params, workspace, st);
    RM_CHECK_LAUNCH("rm_bst_bwd (pack)");
    const int64_t chunk = (B + nblk - 1) / nblk;
    const size_t tile = (size_t)rup4((int64_t)bst_tile_floats(d));
    const BstBwd o{d_out, do_stride, d_keys, d_query, dq_stride, partA};
    RM_BST_LAUNCH(bst_bwd_kernel, D, heads, Hf, max_len, d.nparam, in, (const float *)workspace, chunk, tile, o);
    RM_CHECK_LAUNCH("rm_bst_bwd");
  }
  const int DD = D * D, DH = D * Hf;
  rm_sum_partials(partA, nblk, d.nA, rm_sum_dsts(grads->wq, DD, grads->wk, DD, grads->wv, DD, grads->wo, DD), st);
  rm_sum_partials(partB, nblk, d.nB, rm_sum_dsts(grads->bq, D, grads->bk, D, grads->bv, D, grads->bo, D), st);
  rm_sum_partials(partC, nblk, d.nC, rm_sum_dsts(grads->ffn_w1, DH, grads->ffn_b1, Hf, grads->ffn_w2, DH, grads->ffn_b2, D),
                  st);
  rm_sum_partials(partG, nblk, d.nG,
                  rm_sum_dsts(grads->ln1_gamma, D, grads->ln1_beta, D, grads->ln2_gamma, D, grads->ln2_beta, D), st);
  rm_sum_partials(partP, nblk, d.nP, rm_sum_dsts(grads->pos, d.nP), st);
  RM_CHECK_LAUNCH("rm_bst_bwd (finish)");
  return RM_OK;
}
