// DLRM's dot interaction (arXiv 1906.00091 section 3, the MLPerf recommendation model), forward and backward.
// Nothing in the reference implements it.  Per example, over the T = F + 1 vectors v_0 = z (the bottom tower's
// output) and v_f = E[f-1] (the gathered rows), all of width D:
//     X[0:D] = z;   X[D + i(i-1)/2 + j] = <v_i, v_j>  for 0 <= j < i <= F      (strict lower triangle, row-major)
//     backward:  G_ij = G_ji = dX[D + p(i,j)], G_ii = 0;  dV = G V;  d_rows[f-1] = dV_f;  dz = dV_0 + dX[0:D]
// Composed from library ops this is cat + bmm + a triangular gather: the [T,T] Gram matrix and the concatenated
// input cross HBM several times.  Here the forward reads E and z once and writes X once; the backward reads E, z
// and dX once and writes d_rows and dz once.
//
// Mapping.  A 256-thread block owns a tile of G consecutive examples (G: as many as fit 16 KB of LDS, at most 16)
// and walks the batch with a grid stride (the grid is capped at 2048 blocks, so the stride loop starts at
// B > 2048 G).  The tile's V = [z | E] goes to LDS with float4 loads (row stride D + 4 floats: 16-byte rows,
// conflict-free float4 reads for consecutive rows).
//   forward:  the tile's X rows are ONE contiguous run of G ldx floats; thread k writes floats k, k + 256, ... of
//     it, so every store instruction covers 256 consecutive bytes per wave whatever ldx is (rows need no
//     alignment).  A thread finds (i, j) of its column from the triangular root and forms the dot product as a
//     k-ordered fmaf chain over two float4 row reads per four terms.  Columns [D + P, ldx) get +0.0.
//   backward: the tile's dX columns [0, D + P) go to LDS too (columns past them are never read); a thread owns
//     four columns of one dV row and sums g_ij v_j over j in ascending order, skipping j = i.  d_rows and dz are
//     written as float4.
// No parameters, so no batch reduction: no atomics, no workspace, two runs are bit-equal.
#include "rm_launch.h"

namespace {

constexpr int kMaxF = 40;
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // 8 four-wave blocks per CU
constexpr int kLdsBudget = 16 * 1024;
constexpr int kMaxG = 16;

inline bool dot_d_ok(int D) { return D == 8 || D == 16 || D == 32 || D == 64; }
inline bool dot_ok(int F, int D) { return dot_d_ok(D) && F >= 1 && F <= kMaxF; }
inline int dot_pairs(int F) { return F * (F + 1) / 2; }
// examples per tile: ex_floats = LDS floats one example needs
inline int dot_tile(int ex_floats) {
  const int g = kLdsBudget / (ex_floats * (int)sizeof(float));
  return g < 1 ? 1 : (g > kMaxG ? kMaxG : g);
}

// V = [z | E] of the n examples from `base` on -> LDS [n][T][D + 4]
template <int D>
__device__ __forceinline__ void stage_v(const float *__restrict__ E, const float *__restrict__ z, int64_t base,
                                        int n, int F, float *Vs) {
  constexpr int DS = D + 4, Q = D / 4;
  const int T = F + 1;
  for (int q = threadIdx.x; q < n * T * Q; q += kThreads) {
    const int g = q / (T * Q), r = q - g * T * Q, t = r / Q, c = r - t * Q;
    const int64_t e = base + g;
    const float *src = t == 0 ? z + e * D + 4 * c : E + (e * F + (t - 1)) * D + 4 * c;
    *reinterpret_cast<float4 *>(Vs + (g * T + t) * DS + 4 * c) = *reinterpret_cast<const float4 *>(src);
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <int D>
__global__ __launch_bounds__(kThreads) void dot_fwd_kernel(const float *__restrict__ E, const float *__restrict__ z,
                                                           int64_t B, int F, int G, float *__restrict__ X,
                                                           int ldx) {
  extern __shared__ float sm[];
  constexpr int DS = D + 4;
  const int T = F + 1, W = D + F * T / 2;
  float *Vs = sm;  // [G][T][DS]
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    stage_v<D>(E, z, base, n, F, Vs);
    __syncthreads();
    float *Xt = X + base * ldx;  // the tile's rows: n * ldx contiguous floats
    const int total = n * ldx;
    int g = threadIdx.x / ldx, c = threadIdx.x - g * ldx;
    for (int q = threadIdx.x; q < total; q += kThreads) {
      float out = 0.f;
      if (c < D) {
        out = Vs[g * T * DS + c];
      } else if (c < W) {
        const int p = c - D;
        // p = i(i-1)/2 + j, 0 <= j < i: i from the triangular root (p < 2^10: exact in float), then settled
        int i = (int)((1.f + sqrtf((float)(8 * p + 1))) * 0.5f);
        while (i * (i - 1) / 2 > p) --i;
        while ((i + 1) * i / 2 <= p) ++i;
        const int j = p - i * (i - 1) / 2;
        const float *vi = Vs + (g * T + i) * DS, *vj = Vs + (g * T + j) * DS;
#pragma unroll
        for (int k = 0; k < D / 4; ++k) {
          const float4 a = *reinterpret_cast<const float4 *>(vi + 4 * k);
          const float4 b = *reinterpret_cast<const float4 *>(vj + 4 * k);
          out = fmaf(a.x, b.x, out); out = fmaf(a.y, b.y, out);
          out = fmaf(a.z, b.z, out); out = fmaf(a.w, b.w, out);
        }
      }
      Xt[q] = out;
      c += kThreads;
      while (c >= ldx) { c -= ldx; ++g; }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
template <int D>
__global__ __launch_bounds__(kThreads) void dot_bwd_kernel(const float *__restrict__ E, const float *__restrict__ z,
                                                           const float *__restrict__ dX, int ldx, int64_t B, int F,
                                                           int G, float *__restrict__ d_rows,
                                                           float *__restrict__ dz) {
  extern __shared__ float sm[];
  constexpr int DS = D + 4, Q = D / 4;
  const int T = F + 1, W = D + F * T / 2;
  float *Vs = sm;                // [G][T][DS]
  float *Gs = Vs + G * T * DS;   // [G][W]: dX's columns [0, W)
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    __syncthreads();
    stage_v<D>(E, z, base, n, F, Vs);
    {
      int g = threadIdx.x / W, c = threadIdx.x - g * W;
      for (int q = threadIdx.x; q < n * W; q += kThreads) {
        Gs[q] = dX[(base + g) * ldx + c];
        c += kThreads;
        while (c >= W) { c -= W; ++g; }
      }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n * T * Q; q += kThreads) {
      const int g = q / (T * Q), r = q - g * T * Q, i = r / Q, c = r - i * Q;
      const float *gs = Gs + g * W + D;
      const float *vs = Vs + g * T * DS + 4 * c;
      const int tri_i = i * (i - 1) / 2;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int tri_j = 0;  // j(j-1)/2
      for (int j = 0; j < T; ++j) {
        if (j != i) {
          const float gij = gs[j < i ? tri_i + j : tri_j + i];
          const float4 v = *reinterpret_cast<const float4 *>(vs + j * DS);
          acc.x = fmaf(gij, v.x, acc.x); acc.y = fmaf(gij, v.y, acc.y);
          acc.z = fmaf(gij, v.z, acc.z); acc.w = fmaf(gij, v.w, acc.w);
        }
        tri_j += j;
      }
      const int64_t e = base + g;
      if (i == 0) {
        const float *pz = Gs + g * W + 4 * c;  // the pass-through gradient of X[0:D] = z
        acc.x += pz[0]; acc.y += pz[1]; acc.z += pz[2]; acc.w += pz[3];
        *reinterpret_cast<float4 *>(dz + e * D + 4 * c) = acc;
      } else {
        *reinterpret_cast<float4 *>(d_rows + (e * F + (i - 1)) * D + 4 * c) = acc;
      }
    }
  }
}

int dot_check(const char *fn, int64_t B, int F, int D, int64_t ldx) {
  RM_REQUIRE(B >= 0, "%s: bad batch size", fn);
  RM_REQUIRE(dot_d_ok(D), "%s: D=%d unsupported (8, 16, 32, 64)", fn, D);
  RM_REQUIRE(F >= 1 && F <= kMaxF, "%s: F=%d unsupported (1..%d)", fn, F, kMaxF);
  RM_REQUIRE_STRIDE(fn, "ldx", ldx, D + dot_pairs(F), "D + F(F+1)/2");
  return RM_OK;
}

}  // namespace

extern "C" int rm_dot_interact_supported(int F, int D) { return dot_ok(F, D) ? 1 : 0; }

extern "C" int rm_dot_interact_fwd(const float *E, const float *z, int64_t B, int F, int D, float *X, int64_t ldx,
                                   rm_stream_t stream) {
  int rc = dot_check("rm_dot_interact_fwd", B, F, D, ldx);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  RM_REQUIRE(E && z && X, "rm_dot_interact_fwd: NULL argument");
  RM_REQUIRE(rm_aligned16(E) && rm_aligned16(z), "rm_dot_interact_fwd: E and z must be 16-byte aligned");
  const int ex_floats = (F + 1) * (D + 4);
  const int G = dot_tile(ex_floats);
  const size_t smem = (size_t)G * ex_floats * sizeof(float);
  dim3 grid(rm_grid_cap((B + G - 1) / G, kMaxBlocks));
  hipStream_t st = (hipStream_t)stream;
#define RM_DOT_FWD(D_) \
  hipLaunchKernelGGL((dot_fwd_kernel<D_>), grid, dim3(kThreads), smem, st, E, z, B, F, G, X, (int)ldx)
  switch (D) {
    case 8: RM_DOT_FWD(8); break;
    case 16: RM_DOT_FWD(16); break;
    case 32: RM_DOT_FWD(32); break;
    default: RM_DOT_FWD(64); break;
  }
#undef RM_DOT_FWD
  RM_CHECK_LAUNCH("rm_dot_interact_fwd");
  return RM_OK;
}

extern "C" int rm_dot_interact_bwd(const float *E, const float *z, const float *dX, int64_t ldx, int64_t B, int F,
                                   int D, float *d_rows, float *dz, rm_stream_t stream) {
  int rc = dot_check("rm_dot_interact_bwd", B, F, D, ldx);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  RM_REQUIRE(E && z && dX && d_rows && dz, "rm_dot_interact_bwd: NULL argument");
  RM_REQUIRE(rm_aligned16(E) && rm_aligned16(z) && rm_aligned16(d_rows) && rm_aligned16(dz),
             "rm_dot_interact_bwd: E, z, d_rows and dz must be 16-byte aligned");
  const int ex_floats = (F + 1) * (D + 4) + D + dot_pairs(F);
  const int G = dot_tile(ex_floats);
  const size_t smem = (size_t)G * ex_floats * sizeof(float);
  dim3 grid(rm_grid_cap((B + G - 1) / G, kMaxBlocks));
  hipStream_t st = (hipStream_t)stream;
#define RM_DOT_BWD(D_) \
  hipLaunchKernelGGL((dot_bwd_kernel<D_>), grid, dim3(kThreads), smem, st, E, z, dX, (int)ldx, B, F, G, d_rows, dz)
  switch (D) {
    case 8: RM_DOT_BWD(8); break;
    case 16: RM_DOT_BWD(16); break;
    case 32: RM_DOT_BWD(32); break;
    default: RM_DOT_BWD(64); break;
  }
#undef RM_DOT_BWD
  RM_CHECK_LAUNCH("rm_dot_interact_bwd");
  return RM_OK;
}
