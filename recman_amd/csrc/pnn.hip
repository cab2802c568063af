// The product layer of the Product-based Neural Network (PNN, arXiv 1611.00144) in its kernel form - the IPNN inner
// products and the OPNN products through one kernel per field pair (mat / vec / num), NOT the paper's sum-pooled
// outer-product shortcut -, forward and backward.  Nothing in the reference implements it.  Per example, E [F,D],
// P = F(F-1)/2 pairs p = (i, j), i < j, i-major (itertools.combinations order):
//     inner[p] = <E_i, E_j>
//     outer[p] = E_i K_(p) E_j^T     K_(p) = K[p] (mat, K [P,D,D], the LEFT field on the rows), diag(K[p]) (vec, K [P,D])
//                                    or K[p] I (num, K [P])
//     X = [ E flattened (F D columns, the same bits) | inner (P) | outer (P) ]
//   backward, G_in / G_out = the product column blocks of dX:  dE_i += G_in[p] E_j + G_out[p] K_(p) E_j,
//   dE_j += G_in[p] E_i + G_out[p] K_(p)^T E_i,  d_rows = dX[:, 0:FD] + dE,  dK[p] = sum_b G_out[b,p] E_bi (x) E_bj (its
//   diagonal for vec, its trace for num).
// Unlike the field-pair weighted FM (fmfm.hip), which sums the same per-pair terms to one logit on chip, every pair
// term leaves the chip as a DNN input, and the backward has one upstream gradient per (example, pair).
//
// All kernels: a 512-thread block (eight waves) owns a tile of G = 16..64 whole examples in LDS and walks the batch
// with a grid stride; an example's F D floats are padded to a stride = 4 mod 32 floats (= 16 mod 64 in the mat dK
// kernel).  Beside the tile the forward keeps one [G][P] block of products (row stride P | 1: a wave writes one pair
// of 64 examples without a bank conflict), so that both the row copy and the product blocks go out as contiguous
// runs at any row stride; the backward kernels keep G_in / G_out there.  Nothing of size P D reaches HBM.
//   forward, in float64 rounded to float once (X keeps every pair: a product of a row of large entries that cancels to
//     below 1 is held to 1e-5 absolute, and a float32 chain - on the vector ALU or inside the f32 MFMA - misses that
//     at D >= 16, by 1.2e-5 .. 1.7e-5 on the tests' E x 8 row): E -> LDS once; the row copy; the inner products (a
//     thread per (pair, example), a k-ordered fma chain); the outer products: vec / num on the same vector-ALU path,
//     mat on v_mfma_f64_16x16x4_f64 - a wave takes pairs w, w + 8, ..., loads the weight fragment of the next pair
//     from L2 while this one's 16-example sub-tiles run, U^T = K[p]^T E_i^T in the accumulators (d on the rows, an
//     example per lane: the operands of fmfm.hip's forward, swapped), times E_j: four d in the lane's registers, the
//     four lane groups added by two shuffles (at D = 8 two pairs share an MFMA) - not a 16-lane butterfly per pair.
//     The backward kernels stay on the f32 MFMA and float32 chains: their gradients meet 2e-5 with room.
//   dE, mat: a wave takes an output field f for two sub-tiles and runs ONE accumulator chain over the input fields,
//     dE_f = sum_{j>f} (G_out[p] E_j) K[f,j]^T + sum_{j<f} (G_out[p] E_j) K[j,f]: the per-example scale is applied to
//     the A operand (a lane's example row) before the product.  (At D = 8 the upper eight columns stay empty: two
//     output fields cannot share an A operand that carries the scale of one of them.)  The inner part is a vector-ALU
//     chain over j in the epilogue; d_rows = dX[:, f] + both is written once.  vec / num / inner only: a thread per
//     (example, field, d).  Where E, G_in and G_out of 16 examples would pass the LDS (both products at F >= 37,
//     D = 32), G_in is read from dX through L2 instead.
//   dK, mat: the block grid is (pair chunks) x (batch slices); a wave keeps the accumulators of NP pairs for its whole
//     slice, K = examples on the MFMA (A = E_i^T, B = G_out[.,p] E_j), and leaves them in the slice's part of the
//     workspace.  vec / num: a block per slice, a thread per (pair, d).  rm_sum_partials sums the slices in order.
// Determinism: no atomics anywhere; two runs are bit-equal.
#include "rm_launch.h"

namespace {

constexpr int kMaxF = 40;
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kNone = 3;          // "no outer block" as a kernel-type template argument
constexpr int kMatBlocks = 512;   // grid caps of the forward and dE kernels with the mat kernel type ...
constexpr int kVaBlocks = 1024;   // ... and without
constexpr int kDkSlices = 64;     // batch slices of the mat dK kernel, 512 of the vec / num one ...
constexpr int kVaDkSlices = 512;
constexpr int kDkWsFloats = 8 << 20;  // ... fewer where that many sets of partials would pass 32 MB of workspace
constexpr int kLdsBudget = 128 * 1024;   // mat forward, dE: one block per CU
constexpr int kDkLdsBudget = 64 * 1024;  // dK kernels: two blocks per CU (a 128 KB tile made the vec / num one slower)
constexpr int kVaLdsBudget = 64 * 1024;  // vector-ALU forward, dE
constexpr int kLdsMax = 156 * 1024;      // what a block may take at all (160 KB per CU)
constexpr int kMaxG = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

inline bool pn_ok(int F, int D, int products, int kt) {
  return (D == 8 || D == 16 || D == 32) && F >= 2 && F <= kMaxF && products >= 1 && products <= 3 &&
         kt >= RM_PNN_MAT && kt <= RM_PNN_NUM;
}
inline int pn_pairs(int F) { return F * (F - 1) / 2; }
inline int pn_ksize(int F, int D, int kt) { return pn_pairs(F) * (kt == RM_PNN_MAT ? D * D : kt == RM_PNN_VEC ? D : 1); }
inline int pn_width(int F, int D, int products) {
  return F * D + ((products & RM_PNN_INNER) ? pn_pairs(F) : 0) + ((products & RM_PNN_OUTER) ? pn_pairs(F) : 0);
}
// floats between two examples of the LDS tile: F D rounded up to rem (mod mod)
inline int pn_stride(int F, int D, int rem, int mod) {
  const int fd = F * D;
  return fd + ((rem - fd % mod) + mod) % mod;
}
// the pair units the mat forward and dK kernels walk: pairs, or at D = 8 two pairs that share the left field
inline int pn_units(int F, int D) {
  if (D != 8) return pn_pairs(F);
  int n = 0;
  for (int i = 0; i < F - 1; ++i) n += (F - i) / 2;
  return n;
}
inline int pn_dk_np(int D) { return D == 32 ? 2 : 8; }

struct PnPlan {
  int G, ES, PS;
  bool gl;  // dE: G_in stays in dX (read through L2), only G_out is staged
  size_t smem;
};
// which: 0 forward, 1 dE, 2 dK.  LDS: the tile, one or two [G][PS] blocks, the pair table and the unit table
inline PnPlan pn_plan(int F, int D, int products, int kt, int which) {
  const bool mat = (products & RM_PNN_OUTER) && kt == RM_PNN_MAT;
  const int P = pn_pairs(F);
  PnPlan p;
  p.PS = P | 1;
  p.ES = (which == 2 && mat) ? pn_stride(F, D, 16, 64) : pn_stride(F, D, 4, 32);
  int nb = (which == 1 && products == 3) ? 2 : 1;
  const int budget = which == 2 ? kDkLdsBudget : (mat ? kLdsBudget : kVaLdsBudget);
  int g = budget / ((p.ES + nb * p.PS) * (int)sizeof(float)) / 16 * 16;
  p.G = g < 16 ? 16 : (g > kMaxG ? kMaxG : g);
  p.gl = false;
  if (((size_t)p.G * (p.ES + nb * p.PS) + 2 * P) * sizeof(float) > (size_t)kLdsMax) {  // (16 examples, two blocks)
    nb = 1;
    p.gl = true;
  }
  p.smem = ((size_t)p.G * (p.ES + nb * p.PS) + 2 * P) * sizeof(float);
  return p;
}
inline bool pn_mat(int products, int kt) { return (products & RM_PNN_OUTER) && kt == RM_PNN_MAT; }
inline int pn_fwd_cap(int products, int kt) { return pn_mat(products, kt) ? kMatBlocks : kVaBlocks; }
inline int pn_dk_cap(int F, int D, int kt) {
  const int cap = kDkWsFloats / pn_ksize(F, D, kt), most = kt == RM_PNN_MAT ? kDkSlices : kVaDkSlices;
  return cap > most ? most : (cap < 1 ? 1 : cap);
}
inline int pn_dk_slices(int64_t B, int F, int D, int kt, int G) { return rm_grid_cap((B + G - 1) / G, pn_dk_cap(F, D, kt)); }
inline int pn_dk_chunks(int F, int D) {
  const int per = kWaves * pn_dk_np(D);
  return (pn_units(F, D) + per - 1) / per;
}

__device__ __forceinline__ int pn_pair(int F, int i, int j) { return i * F - i * (i + 1) / 2 + j - i - 1; }

// the pair (unit) table -> T: i | j << 8 (| 1 << 16: a lone last pair of a D = 8 unit).  PACK: two pairs per unit
template <bool PACK>
__device__ __forceinline__ void pn_table(int F, int *T) {
  for (int q = threadIdx.x; q < F * F; q += blockDim.x) {
    const int i = q / F, j = q - i * F;
    if (i >= j) continue;
    if (PACK) {
      const int rel = j - i - 1;
      if (rel & 1) continue;
      int at = 0;
      for (int t = 0; t < i; ++t) at += (F - t) / 2;
      T[at + rel / 2] = i | (j << 8) | ((j == F - 1) << 16);
    } else {
      T[pn_pair(F, i, j)] = i | (j << 8);
    }
  }
}

// E of the n examples from `base` on -> LDS [npad][ES]; rows n .. npad - 1 are zeros
__device__ __forceinline__ void pn_stage(const float *__restrict__ E, int64_t base, int n, int npad, int FD, int ES,
                                         float *Es) {
  const int Q = FD / 4;
  for (int q = threadIdx.x; q < npad * Q; q += blockDim.x) {
    const int r = q / Q, c = q - r * Q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < n) v = *reinterpret_cast<const float4 *>(E + (base + r) * FD + 4 * c);
    *reinterpret_cast<float4 *>(Es + r * ES + 4 * c) = v;
  }
}

// P columns of dX from column `col` on -> LDS [npad][PS]; rows n .. npad - 1 are zeros.  Rows of dX need no alignment
__device__ __forceinline__ void pn_stage_g(const float *__restrict__ dX, int64_t lddx, int col, int64_t base, int n,
                                           int npad, int P, int PS, float *Gs) {
  for (int q = threadIdx.x; q < npad * P; q += blockDim.x) {
    const int r = q / P, c = q - r * P;
    Gs[r * PS + c] = r < n ? dX[(base + r) * lddx + col + c] : 0.f;
  }
}

// a [n][P] block of products, LDS -> P columns of X from column `col` on: contiguous runs at any row stride
__device__ __forceinline__ void pn_put(const float *Os, int PS, int n, int P, float *__restrict__ X, int64_t ldx,
                                       int64_t base, int col) {
  for (int q = threadIdx.x; q < n * P; q += blockDim.x) {
    const int r = q / P, c = q - r * P;
    X[(base + r) * ldx + col + c] = Os[r * PS + c];
  }
}

// ---------------------------------------------------------------------------------------- forward
// The vector-ALU products of a tile -> Os: a thread per (pair, example), examples on consecutive lanes (LDS rows
// 4 mod 32 apart: 16-byte reads without a conflict; Os rows an odd stride apart).  KT = kNone: the inner product
template <int D, int KT>
__device__ __forceinline__ void pn_valu_products(const float *Es, const int *T, const float *__restrict__ K, int n,
                                                 int P, int ES, int PS, float *Os) {
  const int sh = n <= 16 ? 4 : (n <= 32 ? 5 : 6);
  for (int q = threadIdx.x; q < (P << sh); q += kThreads) {
    const int p = q >> sh, m = q & ((1 << sh) - 1);
    if (m >= n) continue;
    const int t = T[p];
    const float *ei = Es + m * ES + (t & 255) * D, *ej = Es + m * ES + ((t >> 8) & 255) * D;
    // float64 accumulation, rounded to float once: a product of a row of large entries that cancels to below 1 is
    // held to 1e-5 absolute, which a float32 chain over D terms of size 10 misses
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < D; k += 4) {
      const float4 a = *reinterpret_cast<const float4 *>(ei + k), b = *reinterpret_cast<const float4 *>(ej + k);
      if (KT == RM_PNN_VEC) {
        const float *w = K + p * D + k;
        acc = fma((double)a.x * (double)w[0], (double)b.x, acc);
        acc = fma((double)a.y * (double)w[1], (double)b.y, acc);
        acc = fma((double)a.z * (double)w[2], (double)b.z, acc);
        acc = fma((double)a.w * (double)w[3], (double)b.w, acc);
      } else {
        acc = fma((double)a.x, (double)b.x, acc);
        acc = fma((double)a.y, (double)b.y, acc);
        acc = fma((double)a.z, (double)b.z, acc);
        acc = fma((double)a.w, (double)b.w, acc);
      }
    }
    if (KT == RM_PNN_NUM) acc *= (double)K[p];
    Os[m * PS + p] = (float)acc;
  }
}

// KK consecutive floats of the tile: the A operands of a lane's KK k-steps in one LDS read
template <int KK>
__device__ __forceinline__ void pn_lds_a(const float *p, float (&a)[KK]) {
  if (KK == 2) {
    const float2 v = *reinterpret_cast<const float2 *>(p);
    a[0] = v.x; a[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < KK / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4 *>(p + 4 * q);
      a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
  }
}

// k-step kk of lane group lq = lane / 16 carries k = KK lq + kk (a lane's KK operands of E are consecutive floats of its
// example's row).  The weight fragments of unit t: K[p][k][d], d on the lane; at D = 8 the upper eight d are the next
// pair's.  The forward passes them as the A operand (U^T = K^T E_i^T: d on the accumulator rows, examples on the lanes),
// converted to float64 at the MFMA
template <int D, int KK, int CB>
__device__ __forceinline__ void pn_fwd_b(const float *__restrict__ K, int F, int t, int lr, int lq, float (&b)[CB][KK]) {
  const int i = t & 255, j = (t >> 8) & 255, lone = t >> 16, p = pn_pair(F, i, j);
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int k = KK * lq + kk;
      if (D == 8) {
        const int h = lr >> 3;
        b[cb][kk] = (h && lone) ? 0.f : K[(p + h) * D * D + k * D + (lr & 7)];
      } else {
        b[cb][kk] = K[p * D * D + k * D + 16 * cb + lr];
      }
    }
}

// The mat products of a tile -> Os
template <int D>
__device__ __forceinline__ void pn_mat_products(const float *Es, const int *TU, const float *__restrict__ K, int F,
                                                int nsub, int NU, int ES, int PS, float *Os) {
  constexpr int KK = D >= 16 ? D / 4 : 2, CB = D == 32 ? 2 : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  // the next unit's weight fragment is on its way from L2 while this one's sub-tiles run
  float b[CB][KK], bn[CB][KK];
  int t = 0;
  if (wave < NU) {
    t = TU[wave];
    pn_fwd_b<D, KK, CB>(K, F, t, lr, lq, b);
  }
  for (int u = wave; u < NU; u += kWaves) {
    const int tn = u + kWaves < NU ? TU[u + kWaves] : t;
    pn_fwd_b<D, KK, CB>(K, F, tn, lr, lq, bn);
    const int i = t & 255, j = (t >> 8) & 255, lone = t >> 16, p = pn_pair(F, i, j);
    // accumulator register r of block cb is row d = 16 cb + lq + 4 r (the f64 MFMA's own C/D map), column = example lr
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s >= nsub) break;
      f64x4 acc[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) acc[cb] = f64x4{0.0, 0.0, 0.0, 0.0};
      const float *row = Es + (16 * s + lr) * ES;  // this lane's example
      float a[KK];
      pn_lds_a<KK>(row + i * D + KK * lq, a);
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)b[cb][kk], (double)a[kk], acc[cb], 0, 0, 0);
      if (D == 8) {  // rows 0..7: pair p (registers 0, 1: d = lq, lq + 4), rows 8..15: pair p + 1 (registers 2, 3)
        const float *e0 = row + j * D + lq, *e1 = row + (lone ? j : j + 1) * D + lq;
        double v0 = 0.0, v1 = 0.0;
        v0 = fma(acc[0][0], (double)e0[0], v0);
        v0 = fma(acc[0][1], (double)e0[4], v0);
        v1 = fma(acc[0][2], (double)e1[0], v1);
        v1 = fma(acc[0][3], (double)e1[4], v1);
        v0 += __shfl_xor(v0, 16, 64);
        v1 += __shfl_xor(v1, 16, 64);
        v0 += __shfl_xor(v0, 32, 64);
        v1 += __shfl_xor(v1, 32, 64);
        if (lq == 0) {
          Os[(16 * s + lr) * PS + p] = (float)v0;
          if (!lone) Os[(16 * s + lr) * PS + p + 1] = (float)v1;
        }
      } else {
        double v = 0.0;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const float *ev = row + j * D + 16 * cb + lq;
#pragma unroll
          for (int r = 0; r < 4; ++r) v = fma(acc[cb][r], (double)ev[4 * r], v);
        }
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lq == 0) Os[(16 * s + lr) * PS + p] = (float)v;
      }
    }
    t = tn;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) b[cb][kk] = bn[cb][kk];
  }
}

template <int D, int KT>
__global__ __launch_bounds__(kThreads) void pnn_fwd_kernel(const float *__restrict__ E, const float *__restrict__ K,
                                                           int inner, int64_t B, int F, int G, int ES, int PS, int NU,
                                                           float *__restrict__ X, int64_t ldx) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int P = F * (F - 1) / 2, FD = F * D, W = FD + (inner ? P : 0) + (KT != kNone ? P : 0);
  float *Es = sm;           // [G][ES]
  float *Os = Es + G * ES;  // [G][PS]: one block of products
  int *T = reinterpret_cast<int *>(Os + G * PS), *TU = T + P;
  const int pad = (int)(ldx - W);
  pn_table<false>(F, T);
  if (KT == RM_PNN_MAT) pn_table<D == 8>(F, TU);
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G), nsub = (n + 15) / 16;
    __syncthreads();
    pn_stage(E, base, n, nsub * 16, FD, ES, Es);
    __syncthreads();
    for (int q = threadIdx.x; q < n * FD; q += kThreads) {  // the row copy
      const int r = q / FD, c = q - r * FD;
      X[(base + r) * ldx + c] = Es[r * ES + c];
    }
    for (int q = threadIdx.x; q < n * pad; q += kThreads) {  // the pad columns
      const int r = q / pad, c = q - r * pad;
      X[(base + r) * ldx + W + c] = 0.f;
    }
    int col = FD;
    if (inner) {
      pn_valu_products<D, kNone>(Es, T, K, n, P, ES, PS, Os);
      __syncthreads();
      pn_put(Os, PS, n, P, X, ldx, base, col);
      col += P;
      if (KT != kNone) __syncthreads();
    }
    if (KT != kNone) {
      if (KT == RM_PNN_MAT)
        pn_mat_products<D>(Es, TU, K, F, nsub, NU, ES, PS, Os);
      else
        pn_valu_products<D, KT>(Es, T, K, n, P, ES, PS, Os);
      __syncthreads();
      pn_put(Os, PS, n, P, X, ldx, base, col);
    }
  }
}

// ---------------------------------------------------------------------------------------- dE
// G_in of example m of the tile, pair p: from LDS, or (GL) from dX
template <bool GL>
__device__ __forceinline__ float pn_gin(const float *Gi, int PS, const float *__restrict__ dX, int64_t lddx,
                                        int64_t base, int FD, int m, int p) {
  return GL ? dX[(base + m) * lddx + FD + p] : Gi[m * PS + p];
}

// B[k][c] of the product that adds input field j to output field f: K[f,j]^T for j > f, K[j,f] for j < f
template <int D>
__device__ __forceinline__ float pn_de_b1(const float *__restrict__ K, int F, int f, int j, int k, int c) {
  if (f == j) return 0.f;
  if (j > f) return K[pn_pair(F, f, j) * D * D + c * D + k];
  return K[pn_pair(F, j, f) * D * D + k * D + c];
}
template <int D, int KK, int CB>
__device__ __forceinline__ void pn_de_b(const float *__restrict__ K, int F, int f, int j, int lr, int lq,
                                        float (&b)[CB][KK]) {
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      b[cb][kk] = (D == 8 && lr >= 8) ? 0.f : pn_de_b1<D>(K, F, f, j, KK * lq + kk, D == 8 ? lr : 16 * cb + lr);
}

template <int D, bool GL>
__global__ __launch_bounds__(kThreads) void pnn_de_mat_kernel(const float *__restrict__ E, const float *__restrict__ K,
                                                              const float *__restrict__ dX, int64_t lddx, int inner,
                                                              int64_t B, int F, int G, int ES, int PS,
                                                              float *__restrict__ d_rows) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int KK = D >= 16 ? D / 4 : 2, CB = D == 32 ? 2 : 1;
  const int P = F * (F - 1) / 2, FD = F * D;
  float *Es = sm;           // [G][ES]
  float *Go = Es + G * ES;  // [G][PS]
  float *Gi = Go + G * PS;  // [G][PS] (inner, not GL)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G), nsub = (n + 15) / 16;
    __syncthreads();
    pn_stage(E, base, n, nsub * 16, FD, ES, Es);
    pn_stage_g(dX, lddx, FD + (inner ? P : 0), base, n, nsub * 16, P, PS, Go);
    if (inner && !GL) pn_stage_g(dX, lddx, FD, base, n, nsub * 16, P, PS, Gi);
    __syncthreads();
    const int NH = (nsub + 1) / 2;  // output fields times halves of the tile (two sub-tiles each): the units
    for (int u = wave; u < F * NH; u += kWaves) {
      const int f = u % F, s0 = 2 * (u / F), ns = nsub - s0 < 2 ? nsub - s0 : 2;
      f32x4 acc[2][CB];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[s][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      // (field f itself contributes a zero fragment: one product in F, and no branch in the chain)
      // a ring of four weight fragments: the loads of fields j + 1 .. j + 3 are on their way from L2 while field j's
      // products run
      float b[4][CB][KK];
#pragma unroll
      for (int q = 0; q < 3; ++q) pn_de_b<D, KK, CB>(K, F, f, q < F ? q : F - 1, lr, lq, b[q]);
      for (int j0 = 0; j0 < F; j0 += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = j0 + q;
          if (j >= F) break;
          pn_de_b<D, KK, CB>(K, F, f, j + 3 < F ? j + 3 : F - 1, lr, lq, b[(q + 3) & 3]);
          const int p = j == f ? 0 : (j > f ? pn_pair(F, f, j) : pn_pair(F, j, f));
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            if (s >= ns) break;
            float a[KK];
            pn_lds_a<KK>(Es + (16 * (s0 + s) + lr) * ES + j * D + KK * lq, a);
            // this lane's example, this pair; field f itself adds nothing, whatever pair 0's gradient holds
            const float sc = j == f ? 0.f : Go[(16 * (s0 + s) + lr) * PS + p];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
              for (int cb = 0; cb < CB; ++cb)
                acc[s][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc * a[kk], b[q][cb][kk], acc[s][cb], 0, 0, 0);
          }
        }
      }
      if (D != 8 || lr < 8) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (s >= ns) break;
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int m = 16 * (s0 + s) + 4 * lq + r, d = 16 * cb + lr;
              if (m < n) {
                float in = 0.f;
                if (inner) {  // sum_{j != f} G_in[p(f,j)] E_j[d], j ascending
                  const float *e = Es + m * ES + d;
                  int p = f - 1;  // p(0, f); p(j + 1, f) = p(j, f) + F - j - 2
                  for (int j = 0; j < f; ++j) {
                    in = fmaf(pn_gin<GL>(Gi, PS, dX, lddx, base, FD, m, p), e[j * D], in);
                    p += F - j - 2;
                  }
                  p = pn_pair(F, f, f + 1);
                  for (int j = f + 1; j < F; ++j, ++p)
                    in = fmaf(pn_gin<GL>(Gi, PS, dX, lddx, base, FD, m, p), e[j * D], in);
                }
                d_rows[(base + m) * FD + f * D + d] = dX[(base + m) * lddx + f * D + d] + (acc[s][cb][r] + in);
              }
            }
        }
      }
    }
  }
}

// inner only, vec, num: dE_f[d] = sum_{j != f} (G_in[p] + G_out[p] k_p[d]) E_j[d]: a thread per (example, field, d)
template <int D, int KT, bool GL>
__global__ __launch_bounds__(kThreads) void pnn_de_valu_kernel(const float *__restrict__ E, const float *__restrict__ K,
                                                               const float *__restrict__ dX, int64_t lddx, int inner,
                                                               int64_t B, int F, int G, int ES, int PS,
                                                               float *__restrict__ d_rows) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int P = F * (F - 1) / 2, FD = F * D;
  float *Es = sm;
  float *Go = Es + G * ES;                       // (outer)
  float *Gi = KT == kNone ? Go : Go + G * PS;    // (inner, not GL)
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    pn_stage(E, base, n, n, FD, ES, Es);
    if (KT != kNone) pn_stage_g(dX, lddx, FD + (inner ? P : 0), base, n, n, P, PS, Go);
    if (inner && !GL) pn_stage_g(dX, lddx, FD, base, n, n, P, PS, Gi);
    __syncthreads();
    for (int q = threadIdx.x; q < n * FD; q += kThreads) {
      const int d = q % D, mf = q / D, m = mf / F, f = mf - m * F;
      const float *e = Es + m * ES + d;
      const float *go = Go + m * PS;
      float in = 0.f, out = 0.f;
      int p = f - 1;  // p(0, f); p(j + 1, f) = p(j, f) + F - j - 2
      for (int j = 0; j < F; ++j) {
        if (j == f) {
          p = pn_pair(F, f, f + 1);
          continue;
        }
        const float ej = e[j * D];
        if (inner) in = fmaf(pn_gin<GL>(Gi, PS, dX, lddx, base, FD, m, p), ej, in);
        if (KT == RM_PNN_VEC) out = fmaf(go[p] * K[p * D + d], ej, out);
        if (KT == RM_PNN_NUM) out = fmaf(go[p] * K[p], ej, out);
        p += j < f ? F - j - 2 : 1;
      }
      d_rows[(base + m) * FD + f * D + d] = dX[(base + m) * lddx + f * D + d] + (in + out);
    }
  }
}

// ---------------------------------------------------------------------------------------- dK
template <int D>
__global__ __launch_bounds__(kThreads) void pnn_dk_mat_kernel(const float *__restrict__ E, const float *__restrict__ dX,
                                                              int64_t lddx, int col, int64_t B, int F, int G, int ES,
                                                              int PS, int NU, int NC, int NS, float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NP = D == 32 ? 2 : 8, RB = D == 32 ? 2 : 1, DD = D * D;
  const int P = F * (F - 1) / 2;
  float *Es = sm;           // [G][ES]
  float *Go = Es + G * ES;  // [G][PS]
  int *T = reinterpret_cast<int *>(Go + G * PS);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  const int chunk = blockIdx.x % NC, slice = blockIdx.x / NC;
  pn_table<D == 8>(F, T);
  __syncthreads();
  // this wave's units: round-robin over (chunk, wave) so that the chunks carry equal loads
  int io[NP], jo[NP], po[NP], tu[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int u = (q * NC + chunk) * kWaves + wave;
    tu[q] = u < NU ? T[u] : -1;
    const int t = tu[q] < 0 ? 0 : tu[q], i = t & 255, j = (t >> 8) & 255, lone = t >> 16;
    if (D == 8) {
      const int h = (lr >> 3) && !lone;
      io[q] = i * D + (lr & 7);
      jo[q] = (j + h) * D + (lr & 7);
      po[q] = pn_pair(F, i, j) + h;
    } else {
      io[q] = i * D + lr;
      jo[q] = j * D + lr;
      po[q] = pn_pair(F, i, j);
    }
  }
  f32x4 acc[NP][RB][RB];
#pragma unroll
  for (int q = 0; q < NP; ++q)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int cb = 0; cb < RB; ++cb) acc[q][rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (B + G - 1) / G;
  for (int64_t tile = slice; tile < ntiles; tile += NS) {
    const int64_t base = tile * G;
    const int n = (int)(B - base < G ? B - base : G), npad = (n + 3) & ~3;
    __syncthreads();
    pn_stage(E, base, n, npad, F * D, ES, Es);
    pn_stage_g(dX, lddx, col, base, n, npad, P, PS, Go);
    __syncthreads();
    for (int ks = 0; ks < npad / 4; ++ks) {
      const int bb = 4 * ks + lq;
      const float *row = Es + bb * ES, *grow = Go + bb * PS;
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        if (tu[q] < 0) continue;  // (the same for the whole wave)
        const float gq = grow[po[q]];
        float a[RB], b[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          a[rb] = (D == 8 && lr >= 8) ? 0.f : row[io[q] + 16 * rb];
          b[rb] = gq * row[jo[q] + 16 * rb];  // the scale of this lane's example and pair, before the product
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int cb = 0; cb < RB; ++cb)
            acc[q][rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb], b[cb], acc[q][rb][cb], 0, 0, 0);
      }
    }
  }
  float *mine = part + (int64_t)slice * P * DD;
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    if (tu[q] < 0) continue;
    const int t = tu[q], i = t & 255, j = (t >> 8) & 255, lone = t >> 16, p = pn_pair(F, i, j);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int cb = 0; cb < RB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * rb + 4 * lq + r;
          if (D == 8) {
            const int h = lr >> 3;
            if (k < 8 && !(h && lone)) mine[(p + h) * DD + k * D + (lr & 7)] = acc[q][rb][cb][r];
          } else {
            mine[p * DD + k * D + 16 * cb + lr] = acc[q][rb][cb][r];
          }
        }
  }
}

// dk[p,d] = sum_b G_out[b,p] E_i[b,d] E_j[b,d] (summed over d for num): a block per batch slice, a thread per (pair, d)
template <int D, bool VEC>
__global__ __launch_bounds__(kThreads) void pnn_dk_valu_kernel(const float *__restrict__ E, const float *__restrict__ dX,
                                                               int64_t lddx, int col, int64_t B, int F, int G, int ES,
                                                               int PS, int NS, float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int P = F * (F - 1) / 2, N = VEC ? P * D : P;
  float *Es = sm;
  float *Go = Es + G * ES;
  int *T = reinterpret_cast<int *>(Go + G * PS);
  float *mine = part + (int64_t)blockIdx.x * N;
  pn_table<false>(F, T);
  const int64_t ntiles = (B + G - 1) / G;
  bool first = true;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += NS, first = false) {
    const int64_t base = tile * G;
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    pn_stage(E, base, n, n, F * D, ES, Es);
    pn_stage_g(dX, lddx, col, base, n, n, P, PS, Go);
    __syncthreads();
    for (int o0 = 0; o0 < P * D; o0 += kThreads) {
      const int o = o0 + threadIdx.x;
      const bool valid = o < P * D;
      const int p = valid ? o / D : 0, d = o % D, t = T[p];
      const float *ei = Es + (t & 255) * D + d, *ej = Es + ((t >> 8) & 255) * D + d, *gp = Go + p;
      float s = 0.f;
      for (int b = 0; b < n; ++b) s = fmaf(gp[b * PS] * ei[b * ES], ej[b * ES], s);
      if (!VEC) s = rm_group_sum<D>(valid ? s : 0.f);
      if (valid && (VEC || d == 0)) {  // (an element is always this thread's own)
        const int at = VEC ? o : p;
        mine[at] = first ? s : mine[at] + s;
      }
    }
  }
}

int pn_check(const char *fn, int64_t B, int F, int D, int products, int kt) {
  RM_REQUIRE(B >= 0, "%s: bad batch size", fn);
  RM_REQUIRE(D == 8 || D == 16 || D == 32, "%s: D=%d unsupported (8, 16, 32)", fn, D);
  RM_REQUIRE(F >= 2 && F <= kMaxF, "%s: F=%d unsupported (2..%d)", fn, F, kMaxF);
  RM_REQUIRE(products >= 1 && products <= 3, "%s: products=%d unsupported (RM_PNN_INNER | RM_PNN_OUTER, not empty)", fn,
             products);
  RM_REQUIRE(kt >= RM_PNN_MAT && kt <= RM_PNN_NUM,
             "%s: kernel_type=%d unsupported (RM_PNN_MAT, RM_PNN_VEC, RM_PNN_NUM)", fn, kt);
  return RM_OK;
}

}  // namespace

extern "C" int rm_pnn_supported(int F, int D, int products, int kernel_type) {
  return pn_ok(F, D, products, kernel_type) ? 1 : 0;
}

extern "C" int rm_pnn_tile(int F, int D, int products, int kernel_type, int which) {
  if (!pn_ok(F, D, products, kernel_type)) return -1;
  const bool outer = products & RM_PNN_OUTER;
  switch (which) {
    case RM_PNN_TILE_FWD: return pn_plan(F, D, products, kernel_type, 0).G;
    case RM_PNN_TILE_DE: return pn_plan(F, D, products, kernel_type, 1).G;
    case RM_PNN_TILE_DK: return outer ? pn_plan(F, D, products, kernel_type, 2).G : 0;
    case RM_PNN_CAP_FWD:
    case RM_PNN_CAP_DE: return pn_fwd_cap(products, kernel_type);
    case RM_PNN_CAP_DK: return outer ? pn_dk_cap(F, D, kernel_type) : 0;
    default: return -1;
  }
}

extern "C" int rm_pnn_fwd(const float *E, const float *K, int products, int kernel_type, int64_t B, int F, int D,
                          float *X, int64_t ldx, rm_stream_t stream) {
  const char *fn = "rm_pnn_fwd";
  int rc = pn_check(fn, B, F, D, products, kernel_type);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  const bool inner = products & RM_PNN_INNER, outer = products & RM_PNN_OUTER;
  RM_REQUIRE_PTR(fn, E);
  if (outer) RM_REQUIRE_PTR(fn, K);
  RM_REQUIRE_PTR(fn, X);
  RM_REQUIRE_STRIDE(fn, "ldx", ldx, pn_width(F, D, products), "W = F D + n P");
  RM_REQUIRE(rm_aligned16(E), "%s: E must be 16-byte aligned", fn);
  const PnPlan p = pn_plan(F, D, products, kernel_type, 0);
  const dim3 grid(rm_grid_cap((B + p.G - 1) / p.G, pn_fwd_cap(products, kernel_type))), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  const int kt = outer ? kernel_type : kNone, in = inner ? 1 : 0;
#define RM_PN_FWD1(D_, KT_) \
  rm_launch_lds(pnn_fwd_kernel<D_, KT_>, grid, block, p.smem, st, E, K, in, B, F, p.G, p.ES, p.PS, pn_units(F, D_), X, ldx)
#define RM_PN_FWD(D_)                                  \
  if (kt == RM_PNN_MAT) RM_PN_FWD1(D_, RM_PNN_MAT);    \
  else if (kt == RM_PNN_VEC) RM_PN_FWD1(D_, RM_PNN_VEC); \
  else if (kt == RM_PNN_NUM) RM_PN_FWD1(D_, RM_PNN_NUM); \
  else RM_PN_FWD1(D_, kNone);
  switch (D) {
    case 8: RM_PN_FWD(8) break;
    case 16: RM_PN_FWD(16) break;
    default: RM_PN_FWD(32) break;
  }
#undef RM_PN_FWD
#undef RM_PN_FWD1
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int64_t rm_pnn_bwd_workspace(int64_t B, int F, int D, int products, int kernel_type) {
  if (!pn_ok(F, D, products, kernel_type) || B < 0) return -1;
  if (B == 0 || !(products & RM_PNN_OUTER)) return 0;
  return (int64_t)pn_dk_slices(B, F, D, kernel_type, pn_plan(F, D, products, kernel_type, 2).G) *
         pn_ksize(F, D, kernel_type);
}

extern "C" int rm_pnn_bwd(const float *E, const float *K, int products, int kernel_type, const float *dX, int64_t lddx,
                          int64_t B, int F, int D, float *d_rows, float *dK, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_pnn_bwd";
  int rc = pn_check(fn, B, F, D, products, kernel_type);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  const bool inner = products & RM_PNN_INNER, outer = products & RM_PNN_OUTER;
  RM_REQUIRE_PTR(fn, E);
  if (outer) RM_REQUIRE_PTR(fn, K);
  RM_REQUIRE_PTR(fn, dX);
  RM_REQUIRE_PTR(fn, d_rows);
  if (outer) {
    RM_REQUIRE_PTR(fn, dK);
    RM_REQUIRE_PTR(fn, workspace);
  }
  RM_REQUIRE_STRIDE(fn, "lddx", lddx, pn_width(F, D, products), "W = F D + n P");
  RM_REQUIRE(rm_aligned16(E), "%s: E must be 16-byte aligned", fn);
  hipStream_t st = (hipStream_t)stream;
  const PnPlan pe = pn_plan(F, D, products, kernel_type, 1);
  const dim3 block(kThreads), ge(rm_grid_cap((B + pe.G - 1) / pe.G, pn_fwd_cap(products, kernel_type)));
  const int kt = outer ? kernel_type : kNone, in = inner ? 1 : 0;
#define RM_PN_DE_ARGS ge, block, pe.smem, st, E, K, dX, lddx, in, B, F, pe.G, pe.ES, pe.PS, d_rows
#define RM_PN_DE(D_)                                                                        \
  if (kt == RM_PNN_MAT) {                                                                   \
    if (pe.gl) rm_launch_lds(pnn_de_mat_kernel<D_, true>, RM_PN_DE_ARGS);                   \
    else rm_launch_lds(pnn_de_mat_kernel<D_, false>, RM_PN_DE_ARGS);                        \
  } else if (kt == RM_PNN_VEC) {                                                            \
    if (pe.gl) rm_launch_lds(pnn_de_valu_kernel<D_, RM_PNN_VEC, true>, RM_PN_DE_ARGS);      \
    else rm_launch_lds(pnn_de_valu_kernel<D_, RM_PNN_VEC, false>, RM_PN_DE_ARGS);           \
  } else if (kt == RM_PNN_NUM) {                                                            \
    if (pe.gl) rm_launch_lds(pnn_de_valu_kernel<D_, RM_PNN_NUM, true>, RM_PN_DE_ARGS);      \
    else rm_launch_lds(pnn_de_valu_kernel<D_, RM_PNN_NUM, false>, RM_PN_DE_ARGS);           \
  } else {                                                                                  \
    rm_launch_lds(pnn_de_valu_kernel<D_, kNone, false>, RM_PN_DE_ARGS);                     \
  }
  switch (D) {
    case 8: RM_PN_DE(8) break;
    case 16: RM_PN_DE(16) break;
    default: RM_PN_DE(32) break;
  }
#undef RM_PN_DE
#undef RM_PN_DE_ARGS
  RM_CHECK_LAUNCH(fn);
  if (!outer) return RM_OK;
  const PnPlan pk = pn_plan(F, D, products, kernel_type, 2);
  const int NS = pn_dk_slices(B, F, D, kernel_type, pk.G), N = pn_ksize(F, D, kernel_type);
  const int col = F * D + (inner ? pn_pairs(F) : 0);  // G_out's first column
#define RM_PN_DK(D_)                                                                                               \
  if (kt == RM_PNN_MAT) {                                                                                          \
    const int NC = pn_dk_chunks(F, D_);                                                                            \
    rm_launch_lds(pnn_dk_mat_kernel<D_>, dim3(NC * NS), block, pk.smem, st, E, dX, lddx, col, B, F, pk.G, pk.ES,   \
                  pk.PS, pn_units(F, D_), NC, NS, workspace);                                                      \
  } else if (kt == RM_PNN_VEC) {                                                                                   \
    rm_launch_lds(pnn_dk_valu_kernel<D_, true>, dim3(NS), block, pk.smem, st, E, dX, lddx, col, B, F, pk.G, pk.ES, \
                  pk.PS, NS, workspace);                                                                           \
  } else {                                                                                                         \
    rm_launch_lds(pnn_dk_valu_kernel<D_, false>, dim3(NS), block, pk.smem, st, E, dX, lddx, col, B, F, pk.G,       \
                  pk.ES, pk.PS, NS, workspace);                                                                    \
  }
  switch (D) {
    case 8: RM_PN_DK(8) break;
    case 16: RM_PN_DK(16) break;
    default: RM_PN_DK(32) break;
  }
#undef RM_PN_DK
  RM_CHECK_LAUNCH(fn);
  rm_sum_partials(workspace, NS, N, rm_sum_dsts(dK, N), st);  // dK = the slices' partials, in slice order
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
