// FiBiNET's interaction (arXiv 1905.09433): a squeeze-excitation gate over the F embedding rows of an example and a
// bilinear interaction over every field pair, on the raw rows and on the re-weighted rows, forward and backward.
// Nothing in the reference implements it.  Per example, E [F,D], R = the gate's hidden width, P = F(F-1)/2:
//     z_f = mean_d E[f,d]   s = relu(z W1)   a = relu(s W2)   V[f] = a_f E[f]                (W1 [F,R], W2 [R,F])
//     pairs p = (i, j), i < j, i-major;  bilinear(Y, W)[p, d] = (sum_k Y[i,k] W_(i)[k,d]) Y[j,d]
//     W_(i) = W[0] (type "all", W [1,D,D]) or W[i] (type "each", W [F-1,D,D]: the LEFT field selects the matrix)
//     X = [ bilinear(E, Wb) | bilinear(V, Wsb) ]                                  (2 P D columns, pair-major, d fastest)
//   backward (z, s, a, V, U = Y W_(.) recomputed), per branch:
//     dU_i[d] = sum_{j>i} dX[p,d] Y[j,d]   dY_j[d] = sum_{i<j} dX[p,d] U_i[d]   dY_i += dU_i W_(i)^T   dW_(i) += Y_i^T dU_i
//     dE = dY(E branch) + a o dV;  da_f = <dV_f, E_f>;  through the two relus (relu'(0) = 0), W2 and W1;  dE[f,d] += dz_f / D
// Composed from library ops this is two gathers and a product per branch over [B,P,D] arrays.  Here the forward
// reads E once and writes X once; the backward reads E once, dX once from HBM (and a second time out of the caches)
// and writes dE once.  a is recomputed in the backward, not stored: it costs 2 F R multiply-adds per example.
//
// Mapping.  A 256-thread block owns a tile of G whole examples and walks the batch with a grid stride (forward and
// backward grids capped at 512 blocks: two blocks per CU; the backward at fewer, down to 128, where 512 partial
// gradient sets would pass 32 MB of workspace).  LDS budget: 80 KB per block, so two blocks share a CU's
// 160 KB.  Both bilinear weight sets go to LDS once per block when they take at most 56 KB (always for "all"; "each"
// up to F = 27 at D = 16, any F at D = 8, F <= 7 at D = 32) - rows padded to D + 1 floats so that the backward's
// transposed read is conflict-free; larger sets ("each" at D = 32: up to 312 KB) are read through the caches.  The
// gate's two small matrices are always read through the caches.  The tile takes what is left, at most 16 examples.
//   forward:  E of the tile -> LDS (rows of D + 4 floats); z, s, a per example; U = E W_(.) and U' = V W'_(.) for
//     every left field, k ascending (see Precision) -> LDS; then the tile's X rows are ONE contiguous run of n ldx
//     floats: thread k handles floats k, k + 256, ... of it, finds (branch, pair, d) of its column (the pair's
//     fields from a table in LDS) and stores U_i[d] Y_j[d].  Columns from 2 P D on are not written.
//   backward: the same staging, then a work item (example, field f, four d) forms dU_f (over the pairs f leads) and
//     the direct part of dY_f (over the pairs f ends): F - 1 reads of dX whatever f is, 16 bytes each where dX's
//     rows are 16-byte aligned (any stride works: four 4-byte loads otherwise).  dU and dY meet in LDS;
//     a second pass adds dU W^T, folds the gated branch into dE and sums <dV_f, E_f> over a field's D lanes; the
//     gate's backward runs per example; dE leaves as float4.  The tile's addends to the four parameter gradients go
//     into the block's own accumulators - in LDS when they fit what the budget leaves, else in the block's slice of
//     the workspace (each element always touched by the same thread) - and rm_sum_partials sums the blocks' partials
//     in block order.  No atomics: two runs are bit-equal.
// Precision.  X keeps the D axis, so a left product U_i[d] that cancels is multiplied by a row entry that need not be
// small: summed in float32, a pair whose |X| is far above 1 (an example with large rows) carries the cancellation as
// a relative error of 1e-5 and more - the float32 restatement on the CPU does.  The gate (z, s, a) and the left
// products are therefore summed in float64 and rounded to float once: 2 F D D float64 multiply-adds per example
// (13 312 at F = 26, D = 16) beside 2 P D floats written (10 400).  Everything else is float32 fmaf chains.
// Everything is vector-ALU work: D x D products per field against 2 P D floats of X / dX per example.
#include "rm_launch.h"

namespace {

constexpr int kMaxF = 40;
constexpr int kThreads = 256;
constexpr int kFwdBlocks = 512;  // two four-wave blocks per CU
constexpr int kBwdBlocks = 512;  // each block leaves 2 nW D D + 2 F R floats of partial gradients ...
constexpr int kBwdWsFloats = 8 << 20;  // ... in at most 32 MB of workspace: fewer blocks for the largest weight sets
constexpr int kBwdMinBlocks = 128;     // (but never fewer than this: 41 MB at F = 40, D = 32, "each")
constexpr int kLdsBudget = 80 * 1024;
constexpr int kWeightLds = 56 * 1024;
constexpr int kMaxG = 16;

inline bool fib_d_ok(int D) { return D == 8 || D == 16 || D == 32; }
inline bool fib_ok(int F, int D, int R, int type) {
  return fib_d_ok(D) && F >= 2 && F <= kMaxF && R >= 1 && R <= F && (type == RM_FIBINET_ALL || type == RM_FIBINET_EACH);
}
inline int fib_pairs(int F) { return F * (F - 1) / 2; }
inline int fib_nw(int F, int type) { return type == RM_FIBINET_EACH ? F - 1 : 1; }
inline int fib_params(int F, int D, int R, int type) { return 2 * fib_nw(F, type) * D * D + 2 * F * R; }

struct FibPlan {
  int G;        // examples per tile
  bool w_lds;   // the bilinear weights live in LDS
  bool a_lds;   // the backward's gradient accumulators live in LDS
  size_t smem;
};

inline int fib_clamp_tile(int bytes_left, int ex_floats) {
  const int g = bytes_left / (ex_floats * (int)sizeof(float));
  return g < 1 ? 1 : (g > kMaxG ? kMaxG : g);
}

// forward: per example E [F][D+4], U and U' [2][F][D], z [F] and s [R] as doubles, a [F]; per block the pair table
// and the weights
inline FibPlan fib_plan_fwd(int F, int D, int R, int type) {
  FibPlan p;
  const int wl = 2 * fib_nw(F, type) * D * (D + 1) * (int)sizeof(float);
  p.w_lds = wl <= kWeightLds;
  p.a_lds = false;
  const int fixed = fib_pairs(F) * (int)sizeof(int) + (p.w_lds ? wl : 0);
  const int ex = F * (D + 4) + 2 * F * D + 3 * F + 2 * R;
  p.G = fib_clamp_tile(kLdsBudget - fixed, ex);
  p.smem = (size_t)fixed + (size_t)p.G * ex * sizeof(float);
  return p;
}

// backward: per example E [F][D+4], dY, U, dU [2][F][D] each, z [F] and s [R] as doubles, a, da, dz [F], ds [R];
// per block the accumulators first (one tile must still fit), then the weights
inline FibPlan fib_plan_bwd(int F, int D, int R, int type) {
  FibPlan p;
  const int ex = F * (D + 4) + 6 * F * D + 5 * F + 3 * R;
  const int exb = ex * (int)sizeof(float);
  const int al = fib_params(F, D, R, type) * (int)sizeof(float);
  const int wl = 2 * fib_nw(F, type) * D * (D + 1) * (int)sizeof(float);
  int left = kLdsBudget;
  p.a_lds = al <= kWeightLds && left - al >= exb;
  if (p.a_lds) left -= al;
  p.w_lds = wl <= kWeightLds && left - wl >= exb;
  if (p.w_lds) left -= wl;
  p.G = fib_clamp_tile(left, ex);
  p.smem = (size_t)(kLdsBudget - left) + (size_t)p.G * exb;
  return p;
}

inline int fib_blocks(int64_t B, int G, int cap) { return rm_grid_cap((B + G - 1) / G, cap); }
// the backward's grid cap for a shape
inline int fib_bwd_cap(int F, int D, int R, int type) {
  const int c = kBwdWsFloats / fib_params(F, D, R, type);
  return c > kBwdBlocks ? kBwdBlocks : (c < kBwdMinBlocks ? kBwdMinBlocks : c);
}

// E of the n examples from `base` on -> LDS [n][F][D + 4]
template <int D>
__device__ __forceinline__ void fib_stage_e(const float *__restrict__ E, int64_t base, int n, int F, float *Es) {
  constexpr int DS = D + 4, Q = D / 4;
  for (int q = threadIdx.x; q < n * F * Q; q += kThreads) {
    const int r = q / Q, c = q - r * Q;  // r = g F + f
    *reinterpret_cast<float4 *>(Es + r * DS + 4 * c) =
        *reinterpret_cast<const float4 *>(E + (base * F + r) * D + 4 * c);
  }
}

// both bilinear sets [nW][D][D] -> LDS [2][nW][D][D + 1]
template <int D>
__device__ __forceinline__ void fib_stage_w(const float *__restrict__ Wb, const float *__restrict__ Wsb, int nW,
                                            float *Ws) {
  const int N = nW * D * D;
  for (int q = threadIdx.x; q < 2 * N; q += kThreads) {
    const int br = q >= N, o = q - br * N, row = o / D, d = o - row * D;
    Ws[(br * nW * D + row) * (D + 1) + d] = br ? Wsb[o] : Wb[o];
  }
}

// the gate of the tile, carried in float64 (see the note on precision above): z -> Zd [n][F], s -> Sd [n][R],
// a -> As [n][F], rounded to float once
template <int D>
__device__ __forceinline__ void fib_gate(const float *Es, const float *__restrict__ W1, const float *__restrict__ W2,
                                         int n, int F, int R, double *Zd, double *Sd, float *As) {
  constexpr int DS = D + 4;
  for (int q = threadIdx.x; q < n * F; q += kThreads) {
    double sum = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) sum += (double)Es[q * DS + d];
    Zd[q] = sum * (1.0 / D);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < n * R; q += kThreads) {
    const int g = q / R, r = q - g * R;
    double acc = 0.0;
    for (int f = 0; f < F; ++f) acc = fma(Zd[g * F + f], (double)W1[f * R + r], acc);
    Sd[q] = acc > 0.0 ? acc : 0.0;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < n * F; q += kThreads) {
    const int g = q / F, f = q - g * F;
    double acc = 0.0;
    for (int r = 0; r < R; ++r) acc = fma(Sd[g * R + r], (double)W2[r * F + f], acc);
    As[q] = acc > 0.0 ? (float)acc : 0.f;
  }
  __syncthreads();
}

// U_i = Y_i W_(i) of the tile for both branches and every left field i < F - 1 -> Us [2][G][F][D]: k ascending,
// summed in float64 and rounded to float once
template <int D, int WS>
__device__ __forceinline__ void fib_left(const float *Es, const float *As, const float *wb, const float *wsb, int n,
                                         int F, int G, int nW, float *Us) {
  constexpr int DS = D + 4;
  const int per = n * (F - 1) * D;
  for (int q = threadIdx.x; q < 2 * per; q += kThreads) {
    const int br = q >= per, o = q - br * per, d = o % D, gi = o / D, g = gi / (F - 1), i = gi - g * (F - 1);
    const float *w = (br ? wsb : wb) + (nW == 1 ? 0 : i) * D * WS + d;
    const float *e = Es + (g * F + i) * DS;
    const double a = br ? (double)As[g * F + i] : 1.0;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) acc = fma(a * (double)e[k], (double)w[k * WS], acc);
    Us[((br * G + g) * F + i) * D + d] = (float)acc;
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <int D, bool WL>
__global__ __launch_bounds__(kThreads) void fibinet_fwd_kernel(const float *__restrict__ E,
                                                               const float *__restrict__ W1,
                                                               const float *__restrict__ W2,
                                                               const float *__restrict__ Wb,
                                                               const float *__restrict__ Wsb, int64_t B, int F, int R,
                                                               int nW, int G, float *__restrict__ X, int64_t ldx) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int DS = D + 4, WS = WL ? D + 1 : D;
  const int P = F * (F - 1) / 2, PD = P * D;
  float *Es = sm;                                  // [G][F][DS]
  float *Us = Es + G * F * DS;                     // [2][G][F][D]
  double *Zd = reinterpret_cast<double *>(Us + 2 * G * F * D);  // [G][F]
  double *Sd = Zd + G * F;                                      // [G][R]
  float *As = reinterpret_cast<float *>(Sd + G * R);            // [G][F]
  int *Pij = reinterpret_cast<int *>(As + G * F);  // [P]: i | j << 8
  float *Ws = reinterpret_cast<float *>(Pij + P);  // [2][nW][D][D + 1] (WL)
  for (int q = threadIdx.x; q < F * F; q += kThreads) {
    const int i = q / F, j = q - i * F;
    if (i < j) Pij[i * F - i * (i + 1) / 2 + j - i - 1] = i | (j << 8);
  }
  if (WL) fib_stage_w<D>(Wb, Wsb, nW, Ws);
  const float *wb = WL ? Ws : Wb;
  const float *wsb = WL ? Ws + nW * D * WS : Wsb;
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    fib_stage_e<D>(E, base, n, F, Es);
    __syncthreads();
    fib_gate<D>(Es, W1, W2, n, F, R, Zd, Sd, As);
    fib_left<D, WS>(Es, As, wb, wsb, n, F, G, nW, Us);
    __syncthreads();
    float *Xt = X + base * ldx;  // the tile's rows: n * ldx contiguous floats
    const int64_t total = (int64_t)n * ldx;
    int64_t g64 = threadIdx.x / ldx;
    int g = (int)g64;
    int64_t c = threadIdx.x - g64 * ldx;
    for (int64_t q = threadIdx.x; q < total; q += kThreads) {
      if (c < 2 * PD) {
        const int cc = (int)c, br = cc >= PD, o = cc - br * PD, p = o / D, d = o - p * D;
        const int ij = Pij[p], i = ij & 255, j = ij >> 8;
        float y = Es[(g * F + j) * DS + d];
        if (br) y *= As[g * F + j];
        Xt[q] = Us[((br * G + g) * F + i) * D + d] * y;
      }
      c += kThreads;
      while (c >= ldx) { c -= ldx; ++g; }
    }
  }
}

// four consecutive floats: one 16-byte load where the address allows it
__device__ __forceinline__ float4 fib_ld4(const float *p, bool v4) {
  if (v4) return *reinterpret_cast<const float4 *>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

// ------------------------------------------------------------------------------------------------ backward
template <int D, bool WL, bool AL>
__global__ __launch_bounds__(kThreads) void fibinet_bwd_kernel(const float *__restrict__ E,
                                                               const float *__restrict__ W1,
                                                               const float *__restrict__ W2,
                                                               const float *__restrict__ Wb,
                                                               const float *__restrict__ Wsb,
                                                               const float *__restrict__ dX, int64_t lddx, int64_t B,
                                                               int F, int R, int nW, int G, float *__restrict__ dE,
                                                               float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int DS = D + 4, Q = D / 4, WS = WL ? D + 1 : D, DD = D * D;
  const int P = F * (F - 1) / 2, PD = P * D;
  const int GFD = G * F * D, NW = nW * DD, Ntot = 2 * NW + 2 * F * R;
  float *Es = sm;              // [G][F][DS]
  float *dYs = Es + G * F * DS;  // [2][G][F][D]: the direct part of dY; branch 0 ends as dE without the gate's part
  float *Us = dYs + 2 * GFD;   // [2][G][F][D]
  float *dUs = Us + 2 * GFD;   // [2][G][F][D]
  double *Zd = reinterpret_cast<double *>(dUs + 2 * GFD);  // [G][F]
  double *Sd = Zd + G * F;                                 // [G][R]
  float *As = reinterpret_cast<float *>(Sd + G * R);       // [G][F]
  float *dAs = As + G * F;     // [G][F]: da, then the gradient of a's pre-activation
  float *dZs = dAs + G * F;    // [G][F]: dz / D
  float *dSs = dZs + G * F;    // [G][R]: the gradient of s' pre-activation
  float *Acc = dSs + G * R;    // [Ntot] (AL)
  float *Ws = Acc + (AL ? Ntot : 0);  // [2][nW][D][D + 1] (WL)
  float *acc = AL ? Acc : part + (int64_t)blockIdx.x * Ntot;  // [dWb | dWsb | dW1 | dW2]
  const bool v4 = (lddx & 3) == 0 && (reinterpret_cast<uintptr_t>(dX) & 15) == 0;  // dX's pair rows are 16-byte aligned
  for (int o = threadIdx.x; o < Ntot; o += kThreads) acc[o] = 0.f;
  if (WL) fib_stage_w<D>(Wb, Wsb, nW, Ws);
  const float *wb = WL ? Ws : Wb;
  const float *wsb = WL ? Ws + nW * D * WS : Wsb;

  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    fib_stage_e<D>(E, base, n, F, Es);
    __syncthreads();
    fib_gate<D>(Es, W1, W2, n, F, R, Zd, Sd, As);
    fib_left<D, WS>(Es, As, wb, wsb, n, F, G, nW, Us);
    __syncthreads();
    // dU_f over the pairs f leads, the direct part of dY_f over the pairs f ends; an item takes four d of one
    // (branch, example, field): 16-byte loads of dX where its rows allow, several of them in flight
    {
      const int per = n * F * Q;
      for (int q = threadIdx.x; q < 2 * per; q += kThreads) {
        const int br = q >= per, o = q - br * per, c = o % Q, gf = o / Q, g = gf / F, f = gf - g * F;
        const float *dx = dX + (base + g) * lddx + br * PD + 4 * c;
        const float *es = Es + g * F * DS + 4 * c;
        const float *as = As + g * F;
        const float *us = Us + (br * G + g) * F * D + 4 * c;
        float4 du = make_float4(0.f, 0.f, 0.f, 0.f), dy = du;
        const int pf = f * F - f * (f + 1) / 2 - f - 1;  // p(f, j) = pf + j
#pragma unroll 4
        for (int j = f + 1; j < F; ++j) {
          const float4 x = fib_ld4(dx + (pf + j) * D, v4);
          float4 y = *reinterpret_cast<const float4 *>(es + j * DS);
          if (br) {
            const float a = as[j];
            y.x *= a; y.y *= a; y.z *= a; y.w *= a;
          }
          du.x = fmaf(x.x, y.x, du.x); du.y = fmaf(x.y, y.y, du.y);
          du.z = fmaf(x.z, y.z, du.z); du.w = fmaf(x.w, y.w, du.w);
        }
#pragma unroll 4
        for (int i = 0; i < f; ++i) {
          const float4 x = fib_ld4(dx + (i * F - i * (i + 1) / 2 + f - i - 1) * D, v4);
          const float4 u = *reinterpret_cast<const float4 *>(us + i * D);
          dy.x = fmaf(x.x, u.x, dy.x); dy.y = fmaf(x.y, u.y, dy.y);
          dy.z = fmaf(x.z, u.z, dy.z); dy.w = fmaf(x.w, u.w, dy.w);
        }
        const int at = ((br * G + g) * F + f) * D + 4 * c;
        *reinterpret_cast<float4 *>(dUs + at) = du;
        *reinterpret_cast<float4 *>(dYs + at) = dy;
      }
    }
    __syncthreads();
    // dY_f += dU_f W_(f)^T (d ascending); dE = dY + a dV; da_f = <dV_f, E_f> over the field's D lanes
    {
      const int items = n * F * D;  // a multiple of D: the D lanes of one (example, field) stay together
      for (int q0 = 0; q0 < items; q0 += kThreads) {
        const int q = q0 + threadIdx.x;
        const bool valid = q < items;
        const int qq = valid ? q : 0;
        const int k = qq % D, gf = qq / D, g = gf / F, f = gf - g * F;
        float t0 = dYs[qq], t1 = dYs[GFD + qq];  // qq = (g F + f) D + k
        if (f < F - 1) {
          const int m = nW == 1 ? 0 : f;
          const float *w0 = wb + (m * D + k) * WS, *w1 = wsb + (m * D + k) * WS;
          const float *u0 = dUs + (g * F + f) * D, *u1 = u0 + GFD;
#pragma unroll
          for (int d = 0; d < D; ++d) {
            t0 = fmaf(u0[d], w0[d], t0);
            t1 = fmaf(u1[d], w1[d], t1);
          }
        }
        const float e = Es[(g * F + f) * DS + k];
        const float da = rm_group_sum<D>(valid ? t1 * e : 0.f);
        if (valid) {
          dYs[qq] = fmaf(As[g * F + f], t1, t0);
          if (k == 0) dAs[g * F + f] = da;
        }
      }
    }
    __syncthreads();
    // the gate's backward: relu'(0) = 0
    for (int q = threadIdx.x; q < n * F; q += kThreads) dAs[q] = As[q] > 0.f ? dAs[q] : 0.f;
    __syncthreads();
    for (int q = threadIdx.x; q < n * R; q += kThreads) {
      const int g = q / R, r = q - g * R;
      float s = 0.f;
      for (int f = 0; f < F; ++f) s = fmaf(dAs[g * F + f], W2[r * F + f], s);
      dSs[q] = Sd[q] > 0.0 ? s : 0.f;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n * F; q += kThreads) {
      const int g = q / F, f = q - g * F;
      float s = 0.f;
      for (int r = 0; r < R; ++r) s = fmaf(dSs[g * R + r], W1[f * R + r], s);
      dZs[q] = s * (1.f / D);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n * F * Q; q += kThreads) {
      const int r = q / Q, c = q - r * Q;  // r = g F + f
      float4 v = *reinterpret_cast<const float4 *>(dYs + r * D + 4 * c);
      const float dz = dZs[r];
      v.x += dz; v.y += dz; v.z += dz; v.w += dz;
      *reinterpret_cast<float4 *>(dE + (base * F + r) * D + 4 * c) = v;
    }
    // the tile's addends to the parameter gradients, examples (and, for "all", fields) in ascending order
    for (int o = threadIdx.x; o < Ntot; o += kThreads) {
      float sum = 0.f;
      if (o < 2 * NW) {
        const int br = o >= NW, oo = o - br * NW, m = oo / DD, kd = oo - m * DD, k = kd / D, d = kd - k * D;
        const int i0 = nW == 1 ? 0 : m, i1 = nW == 1 ? F - 1 : m + 1;
        for (int i = i0; i < i1; ++i)
          for (int g = 0; g < n; ++g) {
            float y = Es[(g * F + i) * DS + k];
            if (br) y *= As[g * F + i];
            sum = fmaf(y, dUs[((br * G + g) * F + i) * D + d], sum);
          }
      } else if (o < 2 * NW + F * R) {
        const int oo = o - 2 * NW, f = oo / R, r = oo - f * R;  // dW1[f][r] = sum z_f ds_r
        for (int g = 0; g < n; ++g) sum = fmaf((float)Zd[g * F + f], dSs[g * R + r], sum);
      } else {
        const int oo = o - 2 * NW - F * R, r = oo / F, f = oo - r * F;  // dW2[r][f] = sum s_r da_f
        for (int g = 0; g < n; ++g) sum = fmaf((float)Sd[g * R + r], dAs[g * F + f], sum);
      }
      acc[o] += sum;
    }
  }
  if (AL) {  // (a thread reads back only what it wrote itself)
    float *mine = part + (int64_t)blockIdx.x * Ntot;
    for (int o = threadIdx.x; o < Ntot; o += kThreads) mine[o] = acc[o];
  }
}

int fib_check(const char *fn, int64_t B, int F, int D, int R, int type, const char *ldname, int64_t ld) {
  RM_REQUIRE(B >= 0, "%s: bad batch size", fn);
  RM_REQUIRE(fib_d_ok(D), "%s: D=%d unsupported (8, 16, 32)", fn, D);
  RM_REQUIRE(F >= 2 && F <= kMaxF, "%s: F=%d unsupported (2..%d)", fn, F, kMaxF);
  RM_REQUIRE(R >= 1 && R <= F, "%s: R=%d unsupported (1..F)", fn, R);
  RM_REQUIRE(type == RM_FIBINET_ALL || type == RM_FIBINET_EACH, "%s: type=%d unsupported (RM_FIBINET_ALL, RM_FIBINET_EACH)",
             fn, type);
  RM_REQUIRE_STRIDE(fn, ldname, ld, 2 * fib_pairs(F) * D, "2 P D");
  return RM_OK;
}

}  // namespace

extern "C" int rm_fibinet_supported(int F, int D, int R, int type) { return fib_ok(F, D, R, type) ? 1 : 0; }

extern "C" int rm_fibinet_tile(int F, int D, int R, int type, int backward) {
  if (!fib_ok(F, D, R, type)) return -1;
  return backward ? fib_plan_bwd(F, D, R, type).G : fib_plan_fwd(F, D, R, type).G;
}

extern "C" int rm_fibinet_fwd(const float *E, const float *W1, const float *W2, const float *Wb, const float *Wsb,
                              int64_t B, int F, int D, int R, int type, float *X, int64_t ldx, rm_stream_t stream) {
  const char *fn = "rm_fibinet_fwd";
  int rc = fib_check(fn, B, F, D, R, type, "ldx", ldx);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  RM_REQUIRE_PTR(fn, E);
  RM_REQUIRE_PTR(fn, W1);
  RM_REQUIRE_PTR(fn, W2);
  RM_REQUIRE_PTR(fn, Wb);
  RM_REQUIRE_PTR(fn, Wsb);
  RM_REQUIRE_PTR(fn, X);
  RM_REQUIRE(rm_aligned16(E), "%s: E must be 16-byte aligned", fn);
  const FibPlan p = fib_plan_fwd(F, D, R, type);
  const int nW = fib_nw(F, type);
  dim3 grid(fib_blocks(B, p.G, kFwdBlocks));
  hipStream_t st = (hipStream_t)stream;
#define RM_FIB_FWD2(D_, WL_)                                                                                       \
  rm_launch_lds(fibinet_fwd_kernel<D_, WL_>, grid, dim3(kThreads), p.smem, st, E, W1, W2, Wb, Wsb, B, F, R, nW, p.G, \
                X, ldx);
#define RM_FIB_FWD(D_) \
  if (p.w_lds) RM_FIB_FWD2(D_, true) else RM_FIB_FWD2(D_, false)
  switch (D) {
    case 8: RM_FIB_FWD(8) break;
    case 16: RM_FIB_FWD(16) break;
    default: RM_FIB_FWD(32) break;
  }
#undef RM_FIB_FWD
#undef RM_FIB_FWD2
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int64_t rm_fibinet_bwd_workspace(int64_t B, int F, int D, int R, int type) {
  if (!fib_ok(F, D, R, type) || B < 0) return -1;
  if (B == 0) return 0;
  return (int64_t)fib_blocks(B, fib_plan_bwd(F, D, R, type).G, fib_bwd_cap(F, D, R, type)) * fib_params(F, D, R, type);
}

extern "C" int rm_fibinet_bwd(const float *E, const float *W1, const float *W2, const float *Wb, const float *Wsb,
                              const float *dX, int64_t lddx, int64_t B, int F, int D, int R, int type, float *dE,
                              float *dW1, float *dW2, float *dWb, float *dWsb, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_fibinet_bwd";
  int rc = fib_check(fn, B, F, D, R, type, "lddx", lddx);
  if (rc != RM_OK) return rc;
  RM_REQUIRE_PTR(fn, dW1);
  RM_REQUIRE_PTR(fn, dW2);
  RM_REQUIRE_PTR(fn, dWb);
  RM_REQUIRE_PTR(fn, dWsb);
  const int nW = fib_nw(F, type), NW = nW * D * D, FR = F * R;
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {  // the sums over an empty batch
    const char *what = "the parameter gradients";
    float *const grads[4] = {dW1, dW2, dWb, dWsb};
    for (int k = 0; k < 4; ++k)
      if (rm_clear_async(fn, what, grads[k], k < 2 ? FR : NW, st) != RM_OK) return RM_ELAUNCH;
    return RM_OK;
  }
  RM_REQUIRE_PTR(fn, E);
  RM_REQUIRE_PTR(fn, W1);
  RM_REQUIRE_PTR(fn, W2);
  RM_REQUIRE_PTR(fn, Wb);
  RM_REQUIRE_PTR(fn, Wsb);
  RM_REQUIRE_PTR(fn, dX);
  RM_REQUIRE_PTR(fn, dE);
  RM_REQUIRE_PTR(fn, workspace);
  RM_REQUIRE(rm_aligned16(E) && rm_aligned16(dE), "%s: E and dE must be 16-byte aligned", fn);
  const FibPlan p = fib_plan_bwd(F, D, R, type);
  const int nblk = fib_blocks(B, p.G, fib_bwd_cap(F, D, R, type));
#define RM_FIB_BWD3(D_, WL_, AL_)                                                                                  \
  rm_launch_lds(fibinet_bwd_kernel<D_, WL_, AL_>, dim3(nblk), dim3(kThreads), p.smem, st, E, W1, W2, Wb, Wsb, dX, lddx, \
                B, F, R, nW, p.G, dE, workspace);
#define RM_FIB_BWD(D_)                                     \
  if (p.w_lds && p.a_lds) RM_FIB_BWD3(D_, true, true)      \
  else if (p.w_lds) RM_FIB_BWD3(D_, true, false)           \
  else if (p.a_lds) RM_FIB_BWD3(D_, false, true)           \
  else RM_FIB_BWD3(D_, false, false)
  switch (D) {
    case 8: RM_FIB_BWD(8) break;
    case 16: RM_FIB_BWD(16) break;
    default: RM_FIB_BWD(32) break;
  }
#undef RM_FIB_BWD
#undef RM_FIB_BWD3
  RM_CHECK_LAUNCH(fn);
  // the four gradients = the blocks' partials [dWb | dWsb | dW1 | dW2], summed in block order
  rm_sum_partials(workspace, nblk, 2 * NW + 2 * FR, rm_sum_dsts(dWb, NW, dWsb, NW, dW1, FR, dW2, FR), st);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
