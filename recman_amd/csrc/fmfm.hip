// Field-pair weighted FM: FwFM (arXiv 1806.03514, a scalar per field pair), FvFM (a vector per pair) and FmFM
// (arXiv 2102.12994, a matrix per pair), forward and backward.  Nothing in the reference implements them.  Per
// example, E [F,D], P = F(F-1)/2 pairs p = (i, j), i < j, i-major (itertools.combinations order):
//     logit = sum_p E_i W_(p) E_j^T     W_(p) = M[p] (matrix, W [P,D,D], the LEFT field on the rows),
//                                              diag(w[p]) (vector, W [P,D]) or r[p] I (scalar, W [P])
//   backward, g = dLoss/dlogit:  dE_i += g W_(p) E_j,  dE_j += g W_(p)^T E_i,  dM[p] = sum_b g_b E_i (x) E_j (the
//   diagonal of it for vector, its trace for scalar).
// The output is ONE float per example: the pair products are reduced on chip and nothing of size P leaves the CU.
//
// Matrix type: the exact-f32 MFMA (v_mfma_f32_16x16x4_f32; bit-for-bit a k-ordered fmaf chain).  A 512-thread block
// (eight waves) owns a tile of G = 16..64 whole examples in LDS (what 128 KB hold in the forward and dE kernels: one
// block per CU; 64 KB in the dM kernel: two; never fewer than 16 examples) and walks the batch with a grid stride; an
// example's F D floats are padded to a stride = 4 mod 32 floats (forward, dE), = 16 mod 64 in the dM kernel, whose
// operands are both 4 examples x 16 d per instruction.  The weights (333 KB at F = 26, D = 16; 3.2 MB at F = 40,
// D = 32) stay in L2: a wave loads one weight fragment (D D / 64 registers), the next ones already on their way, and
// uses it on several 16-example sub-tiles before it moves on: weight traffic per block and tile is P D D floats
// against G F D of E.  The k order of a chain is chosen so that a lane's A operands are consecutive floats (fm_lds_a).
//   forward: a wave takes pairs w, w + 8, ...; U = E_i M[p] is D/4 x D/16 MFMAs per sub-tile, multiplied by E_j in
//     the accumulator layout (column = d on the lane, four examples in the registers) into per-lane sums (one per
//     example row: chains of P / 8 pair sums), reduced over the 16 lanes of a row by butterfly, over the eight waves
//     as a tree.  At D = 8 two pairs (i, j), (i, j + 1) fill the 16 columns of one MFMA; a lone last pair
//     multiplies zeros in the upper half.  No chain is longer than D (inside the MFMA) + P / 8.
//   dE: a wave takes a whole output field f for two sub-tiles and runs ONE accumulator chain over the input fields,
//     dE_f = sum_{j>f} E_j M[f,j]^T + sum_{j<f} E_j M[j,f]  (K = (F - 1) D), so no two waves add to the same element:
//     d_rows = dE_up + g acc is written once, without atomics.  At D = 8 two output fields share an MFMA.
//   dM: the block grid is (pair chunks) x (batch slices): a wave keeps the accumulators of NP pairs (8 at D = 8 / 16,
//     2 at D = 32: 32 registers) for its whole slice, K = examples on the MFMA (A = g E_i^T, B = E_j), and leaves
//     them in the slice's part of the workspace; rm_sum_partials sums the slices in slice order.  E is read
//     ceil(units / (8 NP)) times (6 at F = 26, D = 16), from L2 after the first.
// Vector and scalar types: one templated vector-ALU path (weight index p D + d or p), a thread per (example, d) in the
// forward (inner chain over j, outer over i, butterfly over d), per (example, field, d) for dE, per (pair, d) and batch
// slice for dW - 16-example tiles (the loops are latency-bound: they want waves, not a large tile), the same workspace
// layout and sum.
// Determinism: no atomics anywhere; per-slice partials are summed in slice order: two runs are bit-equal.
#include "rm_launch.h"

namespace {

constexpr int kMaxF = 40;
constexpr int kThreads = 512;     // forward, dE and the vector-ALU kernels: eight waves on one tile, one block per CU
constexpr int kWaves = kThreads / 64;
constexpr int kDwThreads = 512;   // the dM kernel: eight waves, two blocks per CU
constexpr int kDwWaves = kDwThreads / 64;
constexpr int kFwdBlocks = 512;   // grid caps of the matrix forward and dE kernels ...
constexpr int kDeBlocks = 512;
constexpr int kVsBlocks = 2048;   // ... and of the vector / scalar ones (16-example tiles, four blocks per CU)
constexpr int kDwSlices = 64;     // batch slices of the dM kernel, 512 of the vector / scalar dW kernel ...
constexpr int kVsDwSlices = 512;
constexpr int kDwWsFloats = 8 << 20;  // ... fewer where that many sets of partials would pass 32 MB of workspace
constexpr int kLdsBudget = 128 * 1024;   // forward, dE
constexpr int kDwLdsBudget = 64 * 1024;  // dM kernel
constexpr int kVsLdsBudget = 32 * 1024;  // vector / scalar kernels: latency-bound loops want waves, not a large tile
constexpr int kMaxG = 64;
constexpr int kAux = 512;         // floats of LDS beside the tile: the waves' sums per example / g

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline bool fm_ok(int F, int D, int type) {
  return (D == 8 || D == 16 || D == 32) && F >= 2 && F <= kMaxF && type >= RM_FMFM_MATRIX && type <= RM_FMFM_SCALAR;
}
inline int fm_pairs(int F) { return F * (F - 1) / 2; }
inline int fm_wsize(int F, int D, int type) {
  return fm_pairs(F) * (type == RM_FMFM_MATRIX ? D * D : type == RM_FMFM_VECTOR ? D : 1);
}
// floats between two examples of the LDS tile: F D rounded up to rem (mod mod)
inline int fm_stride(int F, int D, int rem, int mod) {
  const int fd = F * D;
  return fd + ((rem - fd % mod) + mod) % mod;
}
// the pair units an MFMA kernel walks: pairs, or at D = 8 two pairs that share the left field
inline int fm_units(int F, int D) {
  if (D != 8) return fm_pairs(F);
  int n = 0;
  for (int i = 0; i < F - 1; ++i) n += (F - i) / 2;
  return n;
}
// pairs (units) a wave of the dM kernel keeps in registers
inline int fm_dw_np(int D) { return D == 32 ? 2 : 8; }

struct FmPlan {
  int G, ES;
  size_t smem;
};
// which: 0 forward, 1 dE, 2 dW.  LDS: the tile, kAux floats (wave partials / g), the unit table
inline FmPlan fm_plan(int F, int D, int type, int which) {
  FmPlan p;
  p.ES = (which == 2 && type == RM_FMFM_MATRIX) ? fm_stride(F, D, 16, 64) : fm_stride(F, D, 4, 32);
  const int budget = type != RM_FMFM_MATRIX ? kVsLdsBudget : (which == 2 ? kDwLdsBudget : kLdsBudget);
  int g = budget / (p.ES * (int)sizeof(float)) / 16 * 16;
  p.G = g < 16 ? 16 : (g > kMaxG ? kMaxG : g);
  p.smem = ((size_t)p.G * p.ES + kAux + fm_pairs(F)) * sizeof(float);
  return p;
}
inline int fm_fwd_cap(int type) { return type == RM_FMFM_MATRIX ? kFwdBlocks : kVsBlocks; }
inline int fm_de_cap(int type) { return type == RM_FMFM_MATRIX ? kDeBlocks : kVsBlocks; }
inline int fm_dw_cap(int F, int D, int type) {
  const int cap = kDwWsFloats / fm_wsize(F, D, type), most = type == RM_FMFM_MATRIX ? kDwSlices : kVsDwSlices;
  return cap > most ? most : (cap < 1 ? 1 : cap);
}
inline int fm_dw_slices(int64_t B, int F, int D, int type, int G) {
  return rm_grid_cap((B + G - 1) / G, fm_dw_cap(F, D, type));
}
inline int fm_dw_chunks(int F, int D) {
  const int per = kDwWaves * fm_dw_np(D);
  return (fm_units(F, D) + per - 1) / per;
}

__device__ __forceinline__ int fm_pair(int F, int i, int j) { return i * F - i * (i + 1) / 2 + j - i - 1; }

// the unit table -> T: i | j << 8 (| 1 << 16: a lone last pair of a D = 8 unit).  PACK: two pairs per unit
template <bool PACK>
__device__ __forceinline__ void fm_table(int F, int *T) {
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
      T[fm_pair(F, i, j)] = i | (j << 8);
    }
  }
}

// E of the n examples from `base` on -> LDS [npad][ES]; rows n .. npad - 1 are zeros
__device__ __forceinline__ void fm_stage(const float *__restrict__ E, int64_t base, int n, int npad, int FD, int ES,
                                         float *Es) {
  const int Q = FD / 4;
  for (int q = threadIdx.x; q < npad * Q; q += blockDim.x) {
    const int r = q / Q, c = q - r * Q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < n) v = *reinterpret_cast<const float4 *>(E + (base + r) * FD + 4 * c);
    *reinterpret_cast<float4 *>(Es + r * ES + 4 * c) = v;
  }
}

// g of the tile -> Gs [npad], zeros past n
__device__ __forceinline__ void fm_stage_g(const float *__restrict__ g, int64_t base, int n, int npad, float *Gs) {
  for (int q = threadIdx.x; q < npad; q += blockDim.x) Gs[q] = q < n ? g[base + q] : 0.f;
}

// ---------------------------------------------------------------------------------------- matrix: forward
// KK consecutive floats of the tile: the A operands of a lane's KK k-steps in one LDS read
template <int KK>
__device__ __forceinline__ void fm_lds_a(const float *p, float (&a)[KK]) {
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

// The k order of an MFMA chain is free as long as A and B agree: k-step kk of lane group lq = lane / 16 carries
// k = KK lq + kk, so that a lane's KK A operands are consecutive floats of its example's row (one 8- or 16-byte LDS
// read instead of KK 4-byte ones) and the transposed weight fragments of the dE kernel are consecutive too.
// The B fragments of unit u: M[p][k][column]; at D = 8 the upper eight columns are the next pair's
template <int D, int KK, int CB>
__device__ __forceinline__ void fm_fwd_b(const float *__restrict__ W, int F, int t, int lr, int lq, float (&b)[CB][KK]) {
  const int i = t & 255, j = (t >> 8) & 255, lone = t >> 16, p = fm_pair(F, i, j);
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int k = KK * lq + kk;
      if (D == 8) {
        const int h = lr >> 3;
        b[cb][kk] = (h && lone) ? 0.f : W[(p + h) * D * D + k * D + (lr & 7)];
      } else {
        b[cb][kk] = W[p * D * D + k * D + 16 * cb + lr];
      }
    }
}

template <int D>
__global__ __launch_bounds__(kThreads) void fmfm_fwd_kernel(const float *__restrict__ E, const float *__restrict__ W,
                                                            int64_t B, int F, int G, int ES, int NU,
                                                            float *__restrict__ logit) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int KK = D >= 16 ? D / 4 : 2, CB = D == 32 ? 2 : 1;
  float *Es = sm;             // [G][ES]
  float *Ps = Es + G * ES;    // [kWaves][64]: the waves' sums per example
  int *T = reinterpret_cast<int *>(Ps + kAux);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  fm_table<D == 8>(F, T);
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G), nsub = (n + 15) / 16;
    __syncthreads();
    fm_stage(E, base, n, nsub * 16, F * D, ES, Es);
    __syncthreads();
    float sum[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[s][r] = 0.f;
    // the next unit's weight fragment is on its way from L2 while this one's sub-tiles run
    float b[CB][KK], bn[CB][KK];
    int t = 0;
    if (wave < NU) {  // (a wave without a unit loads nothing: entry 0 of an empty table names no pair)
      t = T[wave];
      fm_fwd_b<D, KK, CB>(W, F, t, lr, lq, b);
    }
    for (int u = wave; u < NU; u += kWaves) {
      const int tn = u + kWaves < NU ? T[u + kWaves] : t;
      fm_fwd_b<D, KK, CB>(W, F, tn, lr, lq, bn);
      const int i = t & 255, j = (t >> 8) & 255;
      int jj[CB], dc[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        jj[cb] = D == 8 ? min(j + (lr >> 3), F - 1) : j;
        dc[cb] = D == 8 ? (lr & 7) : 16 * cb + lr;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s >= nsub) break;
        f32x4 acc[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        float a[KK];
        fm_lds_a<KK>(Es + (16 * s + lr) * ES + i * D + KK * lq, a);
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[cb][kk], acc[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          const float *ev = Es + (16 * s + 4 * lq) * ES + jj[cb] * D + dc[cb];
#pragma unroll
          for (int r = 0; r < 4; ++r) sum[s][r] = fmaf(acc[cb][r], ev[r * ES], sum[s][r]);
        }
      }
      t = tn;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) b[cb][kk] = bn[cb][kk];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = rm_group_sum<16>(sum[s][r]);
        if (lr == 0) Ps[wave * 64 + 16 * s + 4 * lq + r] = v;
      }
    __syncthreads();
    if ((int)threadIdx.x < n) {
      const float *ps = Ps + threadIdx.x;  // the eight waves' sums, as a tree
      logit[base + threadIdx.x] = ((ps[0] + ps[64]) + (ps[128] + ps[192])) + ((ps[256] + ps[320]) + (ps[384] + ps[448]));
    }
  }
}

// ---------------------------------------------------------------------------------------- matrix: dE
// B[k][c] of the product that adds input field j to output field f: M[f,j]^T for j > f, M[j,f] for j < f
template <int D>
__device__ __forceinline__ float fm_de_b1(const float *__restrict__ W, int F, int f, int j, int k, int c) {
  if (f >= F || f == j) return 0.f;
  if (j > f) return W[fm_pair(F, f, j) * D * D + c * D + k];
  return W[fm_pair(F, j, f) * D * D + k * D + c];
}
template <int D, int KK, int CB>
__device__ __forceinline__ void fm_de_b(const float *__restrict__ W, int F, int f, int j, int lr, int lq,
                                        float (&b)[CB][KK]) {
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) b[cb][kk] = fm_de_b1<D>(W, F, f, j, KK * lq + kk, D == 8 ? (lr & 7) : 16 * cb + lr);
}

template <int D>
__global__ __launch_bounds__(kThreads) void fmfm_de_kernel(const float *__restrict__ E, const float *__restrict__ W,
                                                           const float *__restrict__ g, const float *dE_up, int64_t B,
                                                           int F, int G, int ES, float *d_rows) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int KK = D >= 16 ? D / 4 : 2, CB = D == 32 ? 2 : 1;
  float *Es = sm;           // [G][ES]
  float *Gs = Es + G * ES;  // [G]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  const int NF = D == 8 ? (F + 1) / 2 : F;  // output fields (at D = 8: pairs of them) ...
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G), nsub = (n + 15) / 16;
    __syncthreads();
    fm_stage(E, base, n, nsub * 16, F * D, ES, Es);
    fm_stage_g(g, base, n, nsub * 16, Gs);
    __syncthreads();
    const int NH = (nsub + 1) / 2;  // ... times halves of the tile (two sub-tiles each): the units
    for (int u = wave; u < NF * NH; u += kWaves) {
      const int uf = u % NF, s0 = 2 * (u / NF), ns = nsub - s0 < 2 ? nsub - s0 : 2;
      const int f = D == 8 ? 2 * uf + (lr >> 3) : uf;  // this lane's output field
      f32x4 acc[2][CB];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[s][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      // (at D >= 16 field f itself contributes a zero fragment: one product in F, and no branch in the chain)
      // a ring of four weight fragments: the loads of fields j + 1 .. j + 3 are on their way from L2 while field j's
      // products run (two sub-tiles are 8 D / 16 MFMAs: far less than one L2 round trip)
      float b[4][CB][KK];
#pragma unroll
      for (int q = 0; q < 3; ++q) fm_de_b<D, KK, CB>(W, F, f, q < F ? q : F - 1, lr, lq, b[q]);
      for (int j0 = 0; j0 < F; j0 += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = j0 + q;
          if (j >= F) break;
          fm_de_b<D, KK, CB>(W, F, f, j + 3 < F ? j + 3 : F - 1, lr, lq, b[(q + 3) & 3]);
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            if (s >= ns) break;
            float a[KK];
            fm_lds_a<KK>(Es + (16 * (s0 + s) + lr) * ES + j * D + KK * lq, a);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
              for (int cb = 0; cb < CB; ++cb)
                acc[s][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[q][cb][kk], acc[s][cb], 0, 0, 0);
          }
        }
      }
      if (f < F) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (s >= ns) break;
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int m = 16 * (s0 + s) + 4 * lq + r;
              if (m < n) {
                const int64_t at = ((base + m) * F + f) * D + (D == 8 ? (lr & 7) : 16 * cb + lr);
                const float v = Gs[m] * acc[s][cb][r];
                d_rows[at] = dE_up ? dE_up[at] + v : v;
              }
            }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- matrix: dM
template <int D>
__global__ __launch_bounds__(kDwThreads) void fmfm_dw_kernel(const float *__restrict__ E, const float *__restrict__ g,
                                                           int64_t B, int F, int G, int ES, int NU, int NC, int NS,
                                                           float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int NP = D == 32 ? 2 : 8, RB = D == 32 ? 2 : 1, DD = D * D;
  float *Es = sm;           // [G][ES]
  float *Gs = Es + G * ES;  // [G]
  int *T = reinterpret_cast<int *>(Gs + kAux);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lq = lane >> 4;
  const int chunk = blockIdx.x % NC, slice = blockIdx.x / NC;
  const int P = F * (F - 1) / 2;
  fm_table<D == 8>(F, T);
  __syncthreads();
  // this wave's units: round-robin over (chunk, wave) so that the chunks carry equal loads
  int io[NP], jo[NP], tu[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int u = (q * NC + chunk) * kDwWaves + wave;
    tu[q] = u < NU ? T[u] : -1;
    const int t = tu[q] < 0 ? 0 : tu[q], i = t & 255, j = (t >> 8) & 255;
    if (D == 8) {
      io[q] = i * D + (lr & 7);
      jo[q] = min(j + (lr >> 3), F - 1) * D + (lr & 7);
    } else {
      io[q] = i * D + lr;
      jo[q] = j * D + lr;
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
    fm_stage(E, base, n, npad, F * D, ES, Es);
    fm_stage_g(g, base, n, npad, Gs);
    __syncthreads();
    for (int ks = 0; ks < npad / 4; ++ks) {
      const int bb = 4 * ks + lq;
      const float gb = (D == 8 && lr >= 8) ? 0.f : Gs[bb];
      const float *row = Es + bb * ES;
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        if (tu[q] < 0) continue;  // (the same for the whole wave)
        float a[RB], b[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          a[rb] = gb * row[io[q] + 16 * rb];
          b[rb] = row[jo[q] + 16 * rb];
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
    const int t = tu[q], i = t & 255, j = (t >> 8) & 255, lone = t >> 16, p = fm_pair(F, i, j);
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

// ---------------------------------------------------------------------------------------- vector / scalar
// logit = sum_i E_i[d] (sum_{j>i} w[p,d] E_j[d]) summed over d: a thread per (example, d)
template <int D, bool VEC>
__global__ __launch_bounds__(kThreads) void fmfm_vs_fwd_kernel(const float *__restrict__ E,
                                                               const float *__restrict__ W, int64_t B, int F, int G,
                                                               int ES, float *__restrict__ logit) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *Es = sm;
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    fm_stage(E, base, n, n, F * D, ES, Es);
    __syncthreads();
    for (int q0 = 0; q0 < n * D; q0 += kThreads) {
      const int q = q0 + threadIdx.x;
      const bool valid = q < n * D;
      const int m = valid ? q / D : 0, d = q % D;
      const float *e = Es + m * ES + d;
      const float *w = W + (VEC ? d : 0);
      float tot = 0.f;
      int p = 0;
      for (int i = 0; i < F - 1; ++i) {
        float in = 0.f;
        for (int j = i + 1; j < F; ++j, ++p) in = fmaf(w[VEC ? p * D : p], e[j * D], in);
        tot = fmaf(e[i * D], in, tot);
      }
      tot = rm_group_sum<D>(valid ? tot : 0.f);
      if (valid && d == 0) logit[base + m] = tot;
    }
  }
}

// dE_f[d] = g sum_{j != f} w[p(f,j), d] E_j[d]: a thread per (example, field, d)
template <int D, bool VEC>
__global__ __launch_bounds__(kThreads) void fmfm_vs_de_kernel(const float *__restrict__ E, const float *__restrict__ W,
                                                              const float *__restrict__ g, const float *dE_up,
                                                              int64_t B, int F, int G, int ES, float *d_rows) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *Es = sm;
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    fm_stage(E, base, n, n, F * D, ES, Es);
    __syncthreads();
    for (int q = threadIdx.x; q < n * F * D; q += kThreads) {
      const int d = q % D, mf = q / D, m = mf / F, f = mf - m * F;
      const float *e = Es + m * ES + d;
      const float *w = W + (VEC ? d : 0);
      float acc = 0.f;
      int p = f - 1;  // p(0, f); p(j + 1, f) = p(j, f) + F - j - 2
      for (int j = 0; j < f; ++j) {
        acc = fmaf(w[VEC ? p * D : p], e[j * D], acc);
        p += F - j - 2;
      }
      p = fm_pair(F, f, f + 1);
      for (int j = f + 1; j < F; ++j, ++p) acc = fmaf(w[VEC ? p * D : p], e[j * D], acc);
      const int64_t at = (base + m) * F * D + (int64_t)f * D + d;
      const float v = g[base + m] * acc;
      d_rows[at] = dE_up ? dE_up[at] + v : v;
    }
  }
}

// dw[p,d] = sum_b g_b E_i[b,d] E_j[b,d] (summed over d for scalar): a block per batch slice, a thread per (pair, d)
template <int D, bool VEC>
__global__ __launch_bounds__(kThreads) void fmfm_vs_dw_kernel(const float *__restrict__ E, const float *__restrict__ g,
                                                              int64_t B, int F, int G, int ES, int NS,
                                                              float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *Es = sm;
  float *Gs = Es + G * ES;
  int *T = reinterpret_cast<int *>(Gs + kAux);
  const int P = F * (F - 1) / 2, N = VEC ? P * D : P;
  float *mine = part + (int64_t)blockIdx.x * N;
  fm_table<false>(F, T);
  const int64_t ntiles = (B + G - 1) / G;
  bool first = true;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += NS, first = false) {
    const int64_t base = tile * G;
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    fm_stage(E, base, n, n, F * D, ES, Es);
    fm_stage_g(g, base, n, n, Gs);
    __syncthreads();
    for (int o0 = 0; o0 < P * D; o0 += kThreads) {
      const int o = o0 + threadIdx.x;
      const bool valid = o < P * D;
      const int p = valid ? o / D : 0, d = o % D, t = T[p];
      const float *ei = Es + (t & 255) * D + d, *ej = Es + ((t >> 8) & 255) * D + d;
      float s = 0.f;
      for (int b = 0; b < n; ++b) s = fmaf(Gs[b] * ei[b * ES], ej[b * ES], s);
      if (!VEC) s = rm_group_sum<D>(valid ? s : 0.f);
      if (valid && (VEC || d == 0)) {  // (an element is always this thread's own)
        const int at = VEC ? o : p;
        mine[at] = first ? s : mine[at] + s;
      }
    }
  }
}

int fm_check(const char *fn, int64_t B, int F, int D, int type) {
  RM_REQUIRE(B >= 0, "%s: bad batch size", fn);
  RM_REQUIRE(D == 8 || D == 16 || D == 32, "%s: D=%d unsupported (8, 16, 32)", fn, D);
  RM_REQUIRE(F >= 2 && F <= kMaxF, "%s: F=%d unsupported (2..%d)", fn, F, kMaxF);
  RM_REQUIRE(type >= RM_FMFM_MATRIX && type <= RM_FMFM_SCALAR,
             "%s: type=%d unsupported (RM_FMFM_MATRIX, RM_FMFM_VECTOR, RM_FMFM_SCALAR)", fn, type);
  return RM_OK;
}

}  // namespace

extern "C" int rm_fmfm_supported(int F, int D, int type) { return fm_ok(F, D, type) ? 1 : 0; }

extern "C" int rm_fmfm_tile(int F, int D, int type, int which) {
  if (!fm_ok(F, D, type)) return -1;
  switch (which) {
    case RM_FMFM_TILE_FWD: return fm_plan(F, D, type, 0).G;
    case RM_FMFM_TILE_DE: return fm_plan(F, D, type, 1).G;
    case RM_FMFM_TILE_DW: return fm_plan(F, D, type, 2).G;
    case RM_FMFM_CAP_FWD: return fm_fwd_cap(type);
    case RM_FMFM_CAP_DE: return fm_de_cap(type);
    case RM_FMFM_CAP_DW: return fm_dw_cap(F, D, type);
    default: return -1;
  }
}

extern "C" int rm_fmfm_fwd(const float *E, const float *W, int type, int64_t B, int F, int D, float *logit,
                           rm_stream_t stream) {
  const char *fn = "rm_fmfm_fwd";
  int rc = fm_check(fn, B, F, D, type);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  RM_REQUIRE_PTR(fn, E);
  RM_REQUIRE_PTR(fn, W);
  RM_REQUIRE_PTR(fn, logit);
  RM_REQUIRE(rm_aligned16(E), "%s: E must be 16-byte aligned", fn);
  const FmPlan p = fm_plan(F, D, type, 0);
  const dim3 grid(rm_grid_cap((B + p.G - 1) / p.G, fm_fwd_cap(type))), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
#define RM_FM_FWD(D_)                                                                                           \
  if (type == RM_FMFM_MATRIX)                                                                                   \
    rm_launch_lds(fmfm_fwd_kernel<D_>, grid, block, p.smem, st, E, W, B, F, p.G, p.ES, fm_units(F, D_), logit); \
  else if (type == RM_FMFM_VECTOR)                                                                              \
    rm_launch_lds(fmfm_vs_fwd_kernel<D_, true>, grid, block, p.smem, st, E, W, B, F, p.G, p.ES, logit);         \
  else                                                                                                          \
    rm_launch_lds(fmfm_vs_fwd_kernel<D_, false>, grid, block, p.smem, st, E, W, B, F, p.G, p.ES, logit);
  switch (D) {
    case 8: RM_FM_FWD(8) break;
    case 16: RM_FM_FWD(16) break;
    default: RM_FM_FWD(32) break;
  }
#undef RM_FM_FWD
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int64_t rm_fmfm_bwd_workspace(int64_t B, int F, int D, int type) {
  if (!fm_ok(F, D, type) || B < 0) return -1;
  if (B == 0) return 0;
  return (int64_t)fm_dw_slices(B, F, D, type, fm_plan(F, D, type, 2).G) * fm_wsize(F, D, type);
}

extern "C" int rm_fmfm_bwd(const float *E, const float *W, int type, const float *g, const float *dE_up, int64_t B,
                           int F, int D, float *d_rows, float *dW, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_fmfm_bwd";
  int rc = fm_check(fn, B, F, D, type);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  RM_REQUIRE_PTR(fn, E);
  RM_REQUIRE_PTR(fn, W);
  RM_REQUIRE_PTR(fn, g);
  RM_REQUIRE_PTR(fn, d_rows);
  RM_REQUIRE_PTR(fn, dW);
  RM_REQUIRE_PTR(fn, workspace);
  RM_REQUIRE(rm_aligned16(E), "%s: E must be 16-byte aligned", fn);
  hipStream_t st = (hipStream_t)stream;
  const FmPlan pe = fm_plan(F, D, type, 1), pw = fm_plan(F, D, type, 2);
  const dim3 block(kThreads), ge(rm_grid_cap((B + pe.G - 1) / pe.G, fm_de_cap(type)));
  const int NS = fm_dw_slices(B, F, D, type, pw.G), N = fm_wsize(F, D, type);
#define RM_FM_BWD(D_)                                                                                              \
  if (type == RM_FMFM_MATRIX) {                                                                                    \
    const int NC = fm_dw_chunks(F, D_);                                                                            \
    rm_launch_lds(fmfm_de_kernel<D_>, ge, block, pe.smem, st, E, W, g, dE_up, B, F, pe.G, pe.ES, d_rows);          \
    rm_launch_lds(fmfm_dw_kernel<D_>, dim3(NC * NS), dim3(kDwThreads), pw.smem, st, E, g, B, F, pw.G, pw.ES,       \
                  fm_units(F, D_), NC, NS, workspace);                                                             \
  } else if (type == RM_FMFM_VECTOR) {                                                                             \
    rm_launch_lds(fmfm_vs_de_kernel<D_, true>, ge, block, pe.smem, st, E, W, g, dE_up, B, F, pe.G, pe.ES, d_rows); \
    rm_launch_lds(fmfm_vs_dw_kernel<D_, true>, dim3(NS), block, pw.smem, st, E, g, B, F, pw.G, pw.ES, NS,          \
                  workspace);                                                                                      \
  } else {                                                                                                         \
    rm_launch_lds(fmfm_vs_de_kernel<D_, false>, ge, block, pe.smem, st, E, W, g, dE_up, B, F, pe.G, pe.ES,         \
                  d_rows);                                                                                         \
    rm_launch_lds(fmfm_vs_dw_kernel<D_, false>, dim3(NS), block, pw.smem, st, E, g, B, F, pw.G, pw.ES, NS,         \
                  workspace);                                                                                      \
  }
  switch (D) {
    case 8: RM_FM_BWD(8) break;
    case 16: RM_FM_BWD(16) break;
    default: RM_FM_BWD(32) break;
  }
#undef RM_FM_BWD
  RM_CHECK_LAUNCH(fn);
  rm_sum_partials(workspace, NS, N, rm_sum_dsts(dW, N), st);  // dW = the slices' partials, in slice order
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
