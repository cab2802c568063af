// MaskNet (arXiv 2102.07619): the normalise-and-mask passes around its dense layers, forward and backward.
// Nothing in the reference implements it.  Two kernel families:
//
// a. Group-LayerNorm times N masks (rm_masknet_group_fwd / _bwd).  Per example, E [F, D]:
//        V[f,:] = gamma[f,:] o (E[f,:] - mean_f) / sqrt(var_f + eps) + beta[f,:]      (biased variance over the D
//        Y_n    = M_n o V,  n < N                                                      entries of row f, eps = 1e-5)
//    backward, with dV = sum_n dY_n o M_n and xhat the normalised row:
//        dM_n = dY_n o V;   dgamma = sum_b dV o xhat;   dbeta = sum_b dV
//        dE   = rstd (dxhat - mean_D(dxhat) - xhat mean_D(dxhat o xhat)),  dxhat = dV o gamma
//    normalize = 0 (serial blocks 2..N; X = h_prev [B, H], one mask, no parameters):
//        Y = M o X;   dM = dY o X;   dX = dY o M
// b. Row-LayerNorm + ReLU (rm_masknet_row_fwd / _bwd): h = relu(gamma o xhat(Z) + beta) over the H columns of a row,
//    backward with relu'(0) = 0.
//
// Composed from library ops each of these is five to ten elementwise / reduction passes with V, xhat, the means and
// the inverse deviations in HBM between them.  Here E (Z) is read once per pass, the statistics live in registers:
// V, xhat, mean and rstd never reach HBM; the backward recomputes them from E (Z).
//
// Mapping.  256-thread blocks; a thread owns one float4 (four consecutive columns) of one row.
//   group kernels: C4 = F D / 4 float4 columns per example.  A block pass covers `tile` = 256 / C4 whole examples
//     (thread t -> example t / C4, column t % C4; threads past tile * C4 idle), or one example in two column chunks
//     when C4 > 256.  The D / 4 lanes of a field row are consecutive and aligned, so a row's sums are butterfly
//     shuffles inside that lane group.
//   row kernels: the H / 4 float4 of a row go to a group of L = 2..64 lanes (the next power of two), NV = 1..8 float4
//     per lane when H > 256; a block pass covers 256 / L rows.
//   A thread keeps its columns over the whole grid-stride loop, so the gain / bias gradients accumulate in its
//   registers; at the end every (block, example slot) writes one partial set to the workspace and a finish kernel
//   sums the sets in a fixed order (in float64, rounded once): no atomics, two runs are bit-equal.
//
// Numerics.  A row's mean and its centred sum of squares are accumulated in float64 (the input is centred BEFORE it
// is squared), rstd = 1 / sqrt(ss / D + eps) and xhat = (x - mean) rstd are formed in float64 and rounded once;
// everything behind xhat is float32 fmaf chains (the backward's two row means included).  float32 statistics lose
// 1e-3 on a row whose mean is 50 times its spread.
#include "rm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 512;           // 2 four-wave blocks per CU
constexpr int kMaxN = 8;
constexpr int kMaxF = 40;
constexpr int kMinH = 8, kMaxH = 2048;
constexpr double kEps = 1e-5;
constexpr int64_t kWsCapFloats = 4 << 20;  // the partial sets stay under 16 MB

struct InPtrs { const float *p[kMaxN]; };
struct OutPtrs { float *p[kMaxN]; };

inline bool group_ok(int F, int D, int N, int normalize) {
  if (normalize) return (D == 8 || D == 16 || D == 32) && F >= 1 && F <= kMaxF && N >= 1 && N <= kMaxN;
  return F == 1 && D % 4 == 0 && D >= kMinH && D <= kMaxH && N == 1;
}
inline bool row_ok(int H) { return H % 4 == 0 && H >= kMinH && H <= kMaxH; }

// group kernels: examples per block pass and column chunks per thread
inline int group_tile(int C4) { return C4 <= kThreads ? kThreads / C4 : 1; }
inline int group_chunks(int C4) { return (C4 + kThreads - 1) / kThreads; }
// row kernels: lanes per row (power of two) and float4 per lane
inline int row_lanes(int H) {
  const int h4 = H / 4;
  int L = 2;
  while (L < h4 && L < 64) L *= 2;
  return L;
}
inline int row_nv(int H) {
  const int per = (H / 4 + 63) / 64;
  int nv = 1;
  while (nv < per) nv *= 2;
  return nv;
}
inline int row_tile(int H) { return kThreads / row_lanes(H); }
// grid cap: at most kMaxBlocks, fewer where that many blocks' partial sets would pass kWsCapFloats
inline int grid_cap(int64_t floats_per_block) {
  int64_t c = kWsCapFloats / (floats_per_block > 0 ? floats_per_block : 1);
  return (int)(c < 1 ? 1 : (c > kMaxBlocks ? kMaxBlocks : c));
}
inline int group_cap(int F, int D) { return grid_cap((int64_t)group_tile(F * D / 4) * 2 * F * D); }
inline int row_cap(int H) { return grid_cap((int64_t)row_tile(H) * 2 * H); }

__device__ __forceinline__ float4 ld4(const float *p, int vec) {
  if (vec) return *reinterpret_cast<const float4 *>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void st4(float *p, float4 v, int vec) {
  if (vec) {
    *reinterpret_cast<float4 *>(p) = v;
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float hsum4(float4 a) { return (a.x + a.y) + (a.z + a.w); }

// butterfly sums inside aligned groups of `lanes` lanes (a power of two <= 64): every lane gets the same bits
__device__ __forceinline__ double group_sum_d(double v, int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float group_sum_f(float v, int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LN backward of one float4: rstd (dxhat - m1 - xhat m2)
__device__ __forceinline__ float4 ln_dx(float4 dxh, float4 xh, float m1, float m2, float rstd) {
  return make_float4(rstd * fmaf(-xh.x, m2, dxh.x - m1), rstd * fmaf(-xh.y, m2, dxh.y - m1),
                     rstd * fmaf(-xh.z, m2, dxh.z - m1), rstd * fmaf(-xh.w, m2, dxh.w - m1));
}

// ---------------------------------------------------------------------------------- group kernels
// the normalised float4 of a row spread over Q lanes: float64 mean and centred sum of squares, rounded once
template <int Q>
__device__ __forceinline__ float4 group_xhat(float4 x, float *rstd_out) {
  constexpr double inv_d = 1.0 / (4 * Q);
  const double mean = group_sum_d(((double)x.x + (double)x.y) + ((double)x.z + (double)x.w), Q) * inv_d;
  const double c0 = (double)x.x - mean, c1 = (double)x.y - mean, c2 = (double)x.z - mean, c3 = (double)x.w - mean;
  const double ss = group_sum_d((c0 * c0 + c1 * c1) + (c2 * c2 + c3 * c3), Q);
  const double rstd = 1.0 / sqrt(ss * inv_d + kEps);
  *rstd_out = (float)rstd;
  return make_float4((float)(c0 * rstd), (float)(c1 * rstd), (float)(c2 * rstd), (float)(c3 * rstd));
}

// NORM = 1: D = 4 Q, LayerNorm per field row.  NORM = 0: V = X (Q unused).
template <int Q, int NORM>
__global__ __launch_bounds__(kThreads) void masknet_group_fwd_kernel(
    const float *__restrict__ X, const float *__restrict__ gamma, const float *__restrict__ beta, InPtrs M,
    int64_t ldm, OutPtrs Y, int64_t ldy, int N, int64_t B, int C4, int tile, int chunks, int vec) {
  for (int j = 0; j < chunks; ++j) {
    const int s = threadIdx.x + j * kThreads;
    const int e = s / C4, col4 = s - e * C4;
    const bool on = s < tile * C4;
    float4 g = zero4(), bt = zero4();
    if (NORM && on) {
      g = *reinterpret_cast<const float4 *>(gamma + 4 * col4);
      bt = *reinterpret_cast<const float4 *>(beta + 4 * col4);
    }
    for (int64_t base = (int64_t)blockIdx.x * tile; base < B; base += (int64_t)gridDim.x * tile) {
      const int64_t ex = base + e;
      const bool act = on && ex < B;
      float4 v = act ? *reinterpret_cast<const float4 *>(X + (ex * C4 + col4) * 4) : zero4();
      if (NORM) {
        float rstd;
        v = fma4(g, group_xhat<Q>(v, &rstd), bt);
      }
      if (act) {
        for (int n = 0; n < N; ++n) {
          const float4 m = ld4(M.p[n] + ex * ldm + 4 * col4, vec);
          st4(Y.p[n] + ex * ldy + 4 * col4, mul4(m, v), vec);
        }
      }
    }
  }
}

// dM_n may be dY_n (a thread reads its float4 of dY_n before it writes that of dM_n); d_rows may be dE_up.
template <int Q, int NORM>
__global__ __launch_bounds__(kThreads) void masknet_group_bwd_kernel(
    const float *__restrict__ X, const float *__restrict__ gamma, const float *__restrict__ beta, InPtrs M,
    int64_t ldm, InPtrs dY, int64_t lddy, OutPtrs dM, int64_t lddm, int N, const float *dE_up, int64_t B, int C4,
    int tile, int chunks, int vec, float *d_rows, float *__restrict__ ws) {
  constexpr float inv_d = 1.f / (4 * Q);
  for (int j = 0; j < chunks; ++j) {
    const int s = threadIdx.x + j * kThreads;
    const int e = s / C4, col4 = s - e * C4;
    const bool on = s < tile * C4;
    float4 g = zero4(), bt = zero4();
    if (NORM && on) {
      g = *reinterpret_cast<const float4 *>(gamma + 4 * col4);
      bt = *reinterpret_cast<const float4 *>(beta + 4 * col4);
    }
    float4 acc_g = zero4(), acc_b = zero4();
    for (int64_t base = (int64_t)blockIdx.x * tile; base < B; base += (int64_t)gridDim.x * tile) {
      const int64_t ex = base + e;
      const bool act = on && ex < B;
      const float4 x = act ? *reinterpret_cast<const float4 *>(X + (ex * C4 + col4) * 4) : zero4();
      float4 xh = zero4(), v = x;
      float rstd = 0.f;
      if (NORM) {
        xh = group_xhat<Q>(x, &rstd);
        v = fma4(g, xh, bt);
      }
      float4 dv = zero4();
      if (act) {
        for (int n = 0; n < N; ++n) {
          const float4 dy = ld4(dY.p[n] + ex * lddy + 4 * col4, vec);
          const float4 m = ld4(M.p[n] + ex * ldm + 4 * col4, vec);
          dv = fma4(dy, m, dv);
          st4(dM.p[n] + ex * lddm + 4 * col4, mul4(dy, v), vec);
        }
      }
      float4 dx = dv;
      if (NORM) {
        acc_b = add4(acc_b, dv);
        acc_g = fma4(dv, xh, acc_g);
        const float4 dxh = mul4(dv, g);
        const float m1 = group_sum_f(hsum4(dxh), Q) * inv_d;
        const float m2 = group_sum_f(hsum4(mul4(dxh, xh)), Q) * inv_d;
        dx = ln_dx(dxh, xh, m1, m2, rstd);
      }
      if (act) {
        const int64_t o = (ex * C4 + col4) * 4;
        if (dE_up) dx = add4(*reinterpret_cast<const float4 *>(dE_up + o), dx);
        *reinterpret_cast<float4 *>(d_rows + o) = dx;
      }
    }
    if (NORM && on) {
      // partial set (block, example slot): [2][4 C4] = dgamma | dbeta
      float *p = ws + ((int64_t)blockIdx.x * tile + e) * 8 * C4 + 4 * col4;
      *reinterpret_cast<float4 *>(p) = acc_g;
      *reinterpret_cast<float4 *>(p + 4 * C4) = acc_b;
    }
  }
}

// dgamma | dbeta [W] = the partial sets [nsets][2][W] summed in float64 and rounded once: a block owns kFinCols columns,
// its kFinSlices thread rows each sum a contiguous range of sets in set order, thread row 0 adds the slice sums in slice
// order - a fixed order whatever the launch
constexpr int kFinCols = 16, kFinSlices = kThreads / kFinCols;
__global__ __launch_bounds__(kThreads) void masknet_finish_kernel(const float *__restrict__ ws, int nsets, int W,
                                                                  float *__restrict__ dgamma,
                                                                  float *__restrict__ dbeta) {
  __shared__ double part[kFinSlices][kFinCols];
  const int col = threadIdx.x % kFinCols, slice = threadIdx.x / kFinCols;
  const int c = blockIdx.x * kFinCols + col;
  const int per = (nsets + kFinSlices - 1) / kFinSlices;
  const int s0 = slice * per, s1 = s0 + per < nsets ? s0 + per : nsets;
  double acc = 0.0;
  if (c < 2 * W) {
#pragma unroll 4
    for (int s = s0; s < s1; ++s) acc += (double)ws[(int64_t)s * 2 * W + c];
  }
  part[slice][col] = acc;
  __syncthreads();
  if (slice == 0 && c < 2 * W) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kFinSlices; ++k) t += part[k][col];
    if (c < W) dgamma[c] = (float)t;
    else dbeta[c - W] = (float)t;
  }
}

// ------------------------------------------------------------------------------------ row kernels
// a row's float4 j of lane `lane` is column block lane + j L; xh <- xhat, returns rstd
template <int NV>
__device__ __forceinline__ float row_xhat(const float4 (&x)[NV], const bool (&on)[NV], int L, int H, float4 (&xh)[NV]) {
  const double inv_h = 1.0 / (double)H;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j) s += ((double)x[j].x + (double)x[j].y) + ((double)x[j].z + (double)x[j].w);
  const double mean = group_sum_d(s, L) * inv_h;
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const double c0 = (double)x[j].x - mean, c1 = (double)x[j].y - mean, c2 = (double)x[j].z - mean,
                 c3 = (double)x[j].w - mean;
    ss += on[j] ? (c0 * c0 + c1 * c1) + (c2 * c2 + c3 * c3) : 0.0;
  }
  const double rstd = 1.0 / sqrt(group_sum_d(ss, L) * inv_h + kEps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const double c0 = (double)x[j].x - mean, c1 = (double)x[j].y - mean, c2 = (double)x[j].z - mean,
                 c3 = (double)x[j].w - mean;
    xh[j] = on[j] ? make_float4((float)(c0 * rstd), (float)(c1 * rstd), (float)(c2 * rstd), (float)(c3 * rstd))
                  : zero4();
  }
  return (float)rstd;
}

template <int NV>
__global__ __launch_bounds__(kThreads) void masknet_row_fwd_kernel(const float *__restrict__ Z,
                                                                   const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta, int64_t B, int H,
                                                                   int L, float *__restrict__ h, int64_t ldh) {
  const int H4 = H / 4, tile = kThreads / L;
  const int grp = threadIdx.x / L, lane = threadIdx.x - grp * L;
  float4 g[NV], bt[NV];
  bool on[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int col4 = lane + j * L;
    on[j] = col4 < H4;
    g[j] = on[j] ? *reinterpret_cast<const float4 *>(gamma + 4 * col4) : zero4();
    bt[j] = on[j] ? *reinterpret_cast<const float4 *>(beta + 4 * col4) : zero4();
  }
  for (int64_t base = (int64_t)blockIdx.x * tile; base < B; base += (int64_t)gridDim.x * tile) {
    const int64_t row = base + grp;
    const bool act = row < B;
    float4 x[NV], xh[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j)
      x[j] = (act && on[j]) ? *reinterpret_cast<const float4 *>(Z + (row * H4 + lane + j * L) * 4) : zero4();
    row_xhat<NV>(x, on, L, H, xh);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (act && on[j]) {
        const float4 v = fma4(g[j], xh[j], bt[j]);
        *reinterpret_cast<float4 *>(h + row * ldh + 4 * (lane + j * L)) =
            make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f, v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
      }
    }
  }
}

template <int NV>
__global__ __launch_bounds__(kThreads) void masknet_row_bwd_kernel(const float *__restrict__ Z,
                                                                   const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta,
                                                                   const float *__restrict__ dh, int64_t lddh,
                                                                   int64_t B, int H, int L, float *__restrict__ dZ,
                                                                   float *__restrict__ ws) {
  const int H4 = H / 4, tile = kThreads / L;
  const int grp = threadIdx.x / L, lane = threadIdx.x - grp * L;
  const float inv_h = 1.f / (float)H;
  float4 g[NV], bt[NV], acc_g[NV], acc_b[NV];
  bool on[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int col4 = lane + j * L;
    on[j] = col4 < H4;
    g[j] = on[j] ? *reinterpret_cast<const float4 *>(gamma + 4 * col4) : zero4();
    bt[j] = on[j] ? *reinterpret_cast<const float4 *>(beta + 4 * col4) : zero4();
    acc_g[j] = zero4();
    acc_b[j] = zero4();
  }
  for (int64_t base = (int64_t)blockIdx.x * tile; base < B; base += (int64_t)gridDim.x * tile) {
    const int64_t row = base + grp;
    const bool act = row < B;
    float4 x[NV], xh[NV], dxh[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j)
      x[j] = (act && on[j]) ? *reinterpret_cast<const float4 *>(Z + (row * H4 + lane + j * L) * 4) : zero4();
    const float rstd = row_xhat<NV>(x, on, L, H, xh);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      float4 dy = (act && on[j]) ? *reinterpret_cast<const float4 *>(dh + row * lddh + 4 * (lane + j * L)) : zero4();
      const float4 v = fma4(g[j], xh[j], bt[j]);
      // relu'(0) = 0
      dy = make_float4(v.x > 0.f ? dy.x : 0.f, v.y > 0.f ? dy.y : 0.f, v.z > 0.f ? dy.z : 0.f, v.w > 0.f ? dy.w : 0.f);
      acc_b[j] = add4(acc_b[j], dy);
      acc_g[j] = fma4(dy, xh[j], acc_g[j]);
      dxh[j] = mul4(dy, g[j]);
      s1 += hsum4(dxh[j]);
      s2 += hsum4(mul4(dxh[j], xh[j]));
    }
    const float m1 = group_sum_f(s1, L) * inv_h, m2 = group_sum_f(s2, L) * inv_h;
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (act && on[j])
        *reinterpret_cast<float4 *>(dZ + (row * H4 + lane + j * L) * 4) = ln_dx(dxh[j], xh[j], m1, m2, rstd);
  }
  // partial set (block, row slot): [2][H] = dgamma | dbeta
  float *p = ws + ((int64_t)blockIdx.x * tile + grp) * 2 * H;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (on[j]) {
      *reinterpret_cast<float4 *>(p + 4 * (lane + j * L)) = acc_g[j];
      *reinterpret_cast<float4 *>(p + H + 4 * (lane + j * L)) = acc_b[j];
    }
  }
}

// ------------------------------------------------------------------------------------------ host
int group_check(const char *fn, int64_t B, int F, int D, int N, int normalize) {
  RM_REQUIRE(B >= 0 && B <= ((int64_t)1 << 40), "%s: bad batch size", fn);
  RM_REQUIRE(normalize == 0 || normalize == 1, "%s: normalize=%d is not 0 or 1", fn, normalize);
  if (normalize) {
    RM_REQUIRE(D == 8 || D == 16 || D == 32, "%s: D=%d unsupported (8, 16, 32)", fn, D);
    RM_REQUIRE(F >= 1 && F <= kMaxF, "%s: F=%d unsupported (1..%d)", fn, F, kMaxF);
    RM_REQUIRE(N >= 1 && N <= kMaxN, "%s: N=%d masks unsupported (1..%d)", fn, N, kMaxN);
  } else {
    RM_REQUIRE(group_ok(F, D, N, 0),
               "%s: normalize=0 takes F=1, N=1 and a width D=%d that is a multiple of 4 in %d..%d (F=%d, N=%d)", fn, D,
               kMinH, kMaxH, F, N);
  }
  return RM_OK;
}

bool all_aligned(const float *const *p, int N) {
  for (int n = 0; n < N; ++n)
    if (!rm_aligned16(p[n])) return false;
  return true;
}

void finish(int nsets, int W, float *ws, float *dgamma, float *dbeta, hipStream_t st) {
  hipLaunchKernelGGL(masknet_finish_kernel, dim3((2 * W + kFinCols - 1) / kFinCols), dim3(kThreads), 0, st, ws, nsets,
                     W, dgamma, dbeta);
}

}  // namespace

extern "C" int rm_masknet_group_supported(int F, int D, int N, int normalize) {
  return (normalize == 0 || normalize == 1) && group_ok(F, D, N, normalize) ? 1 : 0;
}

extern "C" int rm_masknet_group_tile(int F, int D, int normalize, int which) {
  if (!rm_masknet_group_supported(F, D, 1, normalize)) return -1;
  if (which == RM_MASKNET_TILE) return group_tile(F * D / 4);
  if (which == RM_MASKNET_CAP) return group_cap(F, D);
  return -1;
}

extern "C" int rm_masknet_group_fwd(const float *X, const float *gamma, const float *beta, int normalize,
                                    const float *const *M, int64_t ldm, int N, int64_t B, int F, int D,
                                    float *const *Y, int64_t ldy, rm_stream_t stream) {
  const char *fn = "rm_masknet_group_fwd";
  int rc = group_check(fn, B, F, D, N, normalize);
  if (rc != RM_OK) return rc;
  const int W = F * D, C4 = W / 4;
  RM_REQUIRE(ldm >= W && ldy >= W, "%s: row strides ldm=%lld, ldy=%lld must be at least F D = %d", fn, (long long)ldm,
             (long long)ldy, W);
  if (B == 0) return RM_OK;
  RM_REQUIRE(X && M && Y && (!normalize || (gamma && beta)), "%s: NULL argument", fn);
  InPtrs m;
  OutPtrs y;
  for (int n = 0; n < kMaxN; ++n) {
    m.p[n] = n < N ? M[n] : nullptr;
    y.p[n] = n < N ? Y[n] : nullptr;
    RM_REQUIRE(n >= N || (m.p[n] && y.p[n]), "%s: NULL mask or output %d", fn, n);
  }
  RM_REQUIRE(rm_aligned16(X) && (!normalize || (rm_aligned16(gamma) && rm_aligned16(beta))),
             "%s: X, gamma and beta must be 16-byte aligned", fn);
  const int vec = ldm % 4 == 0 && ldy % 4 == 0 && all_aligned(M, N) && all_aligned(Y, N);
  const int tile = group_tile(C4), chunks = group_chunks(C4);
  dim3 grid(rm_grid_cap((B + tile - 1) / tile, group_cap(F, D)));
  hipStream_t st = (hipStream_t)stream;
#define RM_MASK_FWD(Q_, NORM_)                                                                                    \
  hipLaunchKernelGGL((masknet_group_fwd_kernel<Q_, NORM_>), grid, dim3(kThreads), 0, st, X, gamma, beta, m, ldm, y, \
                     ldy, N, B, C4, tile, chunks, vec)
  if (!normalize) RM_MASK_FWD(1, 0);
  else if (D == 8) RM_MASK_FWD(2, 1);
  else if (D == 16) RM_MASK_FWD(4, 1);
  else RM_MASK_FWD(8, 1);
#undef RM_MASK_FWD
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int64_t rm_masknet_group_bwd_workspace(int64_t B, int F, int D) {
  if (B < 0 || !group_ok(F, D, 1, 1)) return -1;
  if (B == 0) return 0;
  const int tile = group_tile(F * D / 4);
  return (int64_t)rm_grid_cap((B + tile - 1) / tile, group_cap(F, D)) * tile * 2 * F * D;
}

extern "C" int rm_masknet_group_bwd(const float *X, const float *gamma, const float *beta, int normalize,
                                    const float *const *M, int64_t ldm, const float *const *dY, int64_t lddy,
                                    float *const *dM, int64_t lddm, int N, const float *dE_up, int64_t B, int F, int D,
                                    float *d_rows, float *dgamma, float *dbeta, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_masknet_group_bwd";
  int rc = group_check(fn, B, F, D, N, normalize);
  if (rc != RM_OK) return rc;
  const int W = F * D, C4 = W / 4;
  RM_REQUIRE(ldm >= W && lddy >= W && lddm >= W,
             "%s: row strides ldm=%lld, lddy=%lld, lddm=%lld must be at least F D = %d", fn, (long long)ldm,
             (long long)lddy, (long long)lddm, W);
  if (B == 0) return RM_OK;
  RM_REQUIRE(X && M && dY && dM && d_rows && (!normalize || (gamma && beta && dgamma && dbeta && workspace)),
             "%s: NULL argument", fn);
  InPtrs m, dy;
  OutPtrs dm;
  for (int n = 0; n < kMaxN; ++n) {
    m.p[n] = n < N ? M[n] : nullptr;
    dy.p[n] = n < N ? dY[n] : nullptr;
    dm.p[n] = n < N ? dM[n] : nullptr;
    RM_REQUIRE(n >= N || (m.p[n] && dy.p[n] && dm.p[n]), "%s: NULL mask or gradient %d", fn, n);
    RM_REQUIRE(n >= N || dm.p[n] != dy.p[n] || lddm == lddy, "%s: dM over dY needs lddm = lddy", fn);
  }
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < N; ++k)
      RM_REQUIRE(dM[n] != M[k] && (k == n || dM[n] != dY[k]), "%s: dM[%d] may overlap dY[%d] only", fn, n, n);
  RM_REQUIRE(rm_aligned16(X) && rm_aligned16(d_rows) && rm_aligned16(dE_up) &&
                 (!normalize || (rm_aligned16(gamma) && rm_aligned16(beta) && rm_aligned16(workspace))),
             "%s: X, d_rows, dE_up, gamma, beta and the workspace must be 16-byte aligned", fn);
  const int vec = ldm % 4 == 0 && lddy % 4 == 0 && lddm % 4 == 0 && all_aligned(M, N) && all_aligned(dY, N) &&
                  all_aligned(dM, N);
  const int tile = group_tile(C4), chunks = group_chunks(C4);
  dim3 grid(rm_grid_cap((B + tile - 1) / tile, group_cap(F, D)));
  hipStream_t st = (hipStream_t)stream;
#define RM_MASK_BWD(Q_, NORM_)                                                                                     \
  hipLaunchKernelGGL((masknet_group_bwd_kernel<Q_, NORM_>), grid, dim3(kThreads), 0, st, X, gamma, beta, m, ldm, dy, \
                     lddy, dm, lddm, N, dE_up, B, C4, tile, chunks, vec, d_rows, workspace)
  if (!normalize) RM_MASK_BWD(1, 0);
  else if (D == 8) RM_MASK_BWD(2, 1);
  else if (D == 16) RM_MASK_BWD(4, 1);
  else RM_MASK_BWD(8, 1);
#undef RM_MASK_BWD
  RM_CHECK_LAUNCH(fn);
  if (normalize) {
    finish((int)grid.x * tile, W, workspace, dgamma, dbeta, st);
    RM_CHECK_LAUNCH(fn);
  }
  return RM_OK;
}

extern "C" int rm_masknet_row_supported(int H) { return row_ok(H) ? 1 : 0; }

extern "C" int rm_masknet_row_tile(int H, int which) {
  if (!row_ok(H)) return -1;
  if (which == RM_MASKNET_TILE) return row_tile(H);
  if (which == RM_MASKNET_CAP) return row_cap(H);
  return -1;
}

extern "C" int rm_masknet_row_fwd(const float *Z, const float *gamma, const float *beta, int64_t B, int H, float *h,
                                  int64_t ldh, rm_stream_t stream) {
  const char *fn = "rm_masknet_row_fwd";
  RM_REQUIRE(B >= 0 && B <= ((int64_t)1 << 40), "%s: bad batch size", fn);
  RM_REQUIRE(row_ok(H), "%s: H=%d unsupported (a multiple of 4 in %d..%d)", fn, H, kMinH, kMaxH);
  RM_REQUIRE(ldh >= H && ldh % 4 == 0, "%s: ldh=%lld must be a multiple of 4 and at least H = %d", fn, (long long)ldh,
             H);
  if (B == 0) return RM_OK;
  RM_REQUIRE(Z && gamma && beta && h, "%s: NULL argument", fn);
  RM_REQUIRE(rm_aligned16(Z) && rm_aligned16(gamma) && rm_aligned16(beta) && rm_aligned16(h),
             "%s: Z, gamma, beta and h must be 16-byte aligned", fn);
  const int L = row_lanes(H), tile = kThreads / L;
  dim3 grid(rm_grid_cap((B + tile - 1) / tile, row_cap(H)));
  hipStream_t st = (hipStream_t)stream;
#define RM_ROW_FWD(NV_) \
  hipLaunchKernelGGL((masknet_row_fwd_kernel<NV_>), grid, dim3(kThreads), 0, st, Z, gamma, beta, B, H, L, h, ldh)
  switch (row_nv(H)) {
    case 1: RM_ROW_FWD(1); break;
    case 2: RM_ROW_FWD(2); break;
    case 4: RM_ROW_FWD(4); break;
    default: RM_ROW_FWD(8); break;
  }
#undef RM_ROW_FWD
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int64_t rm_masknet_row_bwd_workspace(int64_t B, int H) {
  if (B < 0 || !row_ok(H)) return -1;
  if (B == 0) return 0;
  const int tile = row_tile(H);
  return (int64_t)rm_grid_cap((B + tile - 1) / tile, row_cap(H)) * tile * 2 * H;
}

extern "C" int rm_masknet_row_bwd(const float *Z, const float *gamma, const float *beta, const float *dh, int64_t lddh,
                                  int64_t B, int H, float *dZ, float *dgamma, float *dbeta, float *workspace,
                                  rm_stream_t stream) {
  const char *fn = "rm_masknet_row_bwd";
  RM_REQUIRE(B >= 0 && B <= ((int64_t)1 << 40), "%s: bad batch size", fn);
  RM_REQUIRE(row_ok(H), "%s: H=%d unsupported (a multiple of 4 in %d..%d)", fn, H, kMinH, kMaxH);
  RM_REQUIRE(lddh >= H && lddh % 4 == 0, "%s: lddh=%lld must be a multiple of 4 and at least H = %d", fn,
             (long long)lddh, H);
  if (B == 0) return RM_OK;
  RM_REQUIRE(Z && gamma && beta && dh && dZ && dgamma && dbeta && workspace, "%s: NULL argument", fn);
  RM_REQUIRE(dZ != Z, "%s: dZ must not be Z", fn);
  RM_REQUIRE(dZ != dh, "%s: dZ must not be dh", fn);
  RM_REQUIRE(rm_aligned16(Z) && rm_aligned16(gamma) && rm_aligned16(beta) && rm_aligned16(dh) && rm_aligned16(dZ) &&
                 rm_aligned16(workspace),
             "%s: Z, gamma, beta, dh, dZ and the workspace must be 16-byte aligned", fn);
  const int L = row_lanes(H), tile = kThreads / L;
  dim3 grid(rm_grid_cap((B + tile - 1) / tile, row_cap(H)));
  hipStream_t st = (hipStream_t)stream;
#define RM_ROW_BWD(NV_)                                                                                          \
  hipLaunchKernelGGL((masknet_row_bwd_kernel<NV_>), grid, dim3(kThreads), 0, st, Z, gamma, beta, dh, lddh, B, H, L, \
                     dZ, workspace)
  switch (row_nv(H)) {
    case 1: RM_ROW_BWD(1); break;
    case 2: RM_ROW_BWD(2); break;
    case 4: RM_ROW_BWD(4); break;
    default: RM_ROW_BWD(8); break;
  }
#undef RM_ROW_BWD
  RM_CHECK_LAUNCH(fn);
  finish((int)grid.x * tile, H, workspace, dgamma, dbeta, st);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
