// The core of a DCN-Mix cross layer (DCN-V2, arXiv 2008.13535 eq. 4-5): what sits between the layer's two skinny
// GEMMs.  Nothing in the reference implements it.  Per example, with E experts of rank r (W = E r):
//     a_i = tanh(t_i)   c_i = tanh(a_i C_i)   p = softmax_i(s) (max-subtracted)   m = [p_1 c_1 | ... | p_E c_E]
//   backward (a, c, p recomputed from t, s, C):
//     dc_i = p_i dm_i   dp_i = <dm_i, c_i>   ds_i = p_i (dp_i - sum_j p_j dp_j)
//     dh_i = dc_i o (1 - c_i^2)   dC_i = sum_b a_i^T dh_i   da_i = dh_i C_i^T   dt_i = da_i o (1 - a_i^2)
// Composed from library ops this is two tanh, a bmm per direction, a softmax and a dozen elementwise passes over
// [B, W] arrays.  Here the forward reads t, s once and writes m once (4 (2 W + E) bytes per example); the backward
// reads t, s, dm once and writes dt, ds once; a, h, c, p, dh live in registers and LDS only.
//
// Mapping.  A 256-thread block owns a tile of G whole examples (G W <= 4096 floats, G <= 64, a multiple of 4) and
// walks the batch with a grid stride.  C goes to LDS once per block, rows padded to r + 1 floats: the forward reads
// it along k (consecutive lanes, consecutive banks), the backward's da = dh C^T along j (stride r + 1: odd, so
// conflict-free), and r (r + 1) floats per expert keep neighbouring experts of a narrow rank off each other's banks.
//   a = tanh(t) of the tile goes to LDS; one thread per example forms p.  A work item is (4 examples, one column):
//   it reads one C value and four broadcast float4 of a per four k-steps, so every r x r product is a k-ordered
//   fmaf chain on the vector ALU.  (The f32 MFMA runs at the vector ALU's rate on gfx950 and these products are a
//   few flop per byte moved: the matrix pipe would buy no time here, and block-diagonal r = 8 tiles do not fill a
//   32x32x2 instruction.)  Every [B, .] argument is a pointer and a row stride; only owned columns are written.
//   backward: after h and c are rebuilt the r lanes of one (example, expert) sum <dm_i, c_i> with a butterfly,
//   dh goes to LDS beside a, and three passes over the tile follow: ds, dt (through da) and the tile's addend to
//   dC, which a thread keeps in registers for its fixed (j, k) positions across all of the block's tiles.
//   dC is deterministic: per-block partials in the workspace, summed in block order (rm_sum_partials); no atomics.
#include "rm_launch.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFwdBlocks = 2048;   // 8 four-wave blocks per CU
constexpr int kBwdBlocks = 512;    // each block leaves E r r floats of partial dC: at most 32 MB of workspace
constexpr int kTileFloats = 4096;  // t values of one tile (16 KB of LDS)
constexpr int kMaxG = 64;
constexpr int kGE = 4;             // examples per work item

inline bool mix_r_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }
inline bool mix_ok(int E, int r) { return E >= 1 && E <= 8 && mix_r_ok(r) && E * r <= 256; }
// examples per tile: a multiple of kGE, 16 (W = 256) .. 64
inline int mix_tile(int W) {
  int g = kTileFloats / W;
  g = g > kMaxG ? kMaxG : g;
  return g / kGE * kGE;
}
inline int mix_blocks(int64_t B, int G, int cap) { return rm_grid_cap((B + G - 1) / G, cap); }

__device__ __forceinline__ float mix_tanh(float x) { return 1.f - 2.f / (expf(2.f * x) + 1.f); }

// C [E][r][r] -> LDS [E][r][r + 1]
template <int R>
__device__ __forceinline__ void stage_c(const float *__restrict__ C, int E, float *Cs) {
  for (int q = threadIdx.x; q < E * R * R; q += kThreads) {
    const int i = q / (R * R), rem = q - i * R * R, j = rem / R, k = rem - j * R;
    Cs[i * R * (R + 1) + j * (R + 1) + k] = C[q];
  }
}

// the tile's a = tanh(t) -> As [n4][W] (rows n .. n4 - 1 zero) and p = softmax(s) -> Ps [n][E]
__device__ __forceinline__ void stage_ap(const float *__restrict__ T, int64_t ldt, const float *__restrict__ S,
                                         int64_t lds, int64_t base, int n, int n4, int E, int W, float *As,
                                         float *Ps) {
  int g = threadIdx.x / W, c = threadIdx.x - g * W;
  for (int q = threadIdx.x; q < n4 * W; q += kThreads) {
    As[q] = g < n ? mix_tanh(T[(base + g) * ldt + c]) : 0.f;
    c += kThreads;
    while (c >= W) { c -= W; ++g; }
  }
  if ((int)threadIdx.x < n) {
    const float *s = S + (base + threadIdx.x) * lds;
    float v[8];
    float mx = s[0];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = i < E ? s[i] : 0.f;
      if (i < E) mx = fmaxf(mx, v[i]);
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = i < E ? expf(v[i] - mx) : 0.f;
      sum += v[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < E) Ps[threadIdx.x * E + i] = v[i] / sum;
  }
}

// h[e] = sum_j a[g0 + e][i r + j] C_i[j][k], j ascending, for the item's kGE examples
template <int R>
__device__ __forceinline__ void item_h(const float *As, const float *Cs, int W, int g0, int i, int k, float *h) {
  const float *a0 = As + g0 * W + i * R;
  const float *c0 = Cs + i * R * (R + 1) + k;
#pragma unroll
  for (int e = 0; e < kGE; ++e) h[e] = 0.f;
#pragma unroll 2
  for (int j = 0; j < R; j += 4) {
    const float w0 = c0[j * (R + 1)], w1 = c0[(j + 1) * (R + 1)], w2 = c0[(j + 2) * (R + 1)],
                w3 = c0[(j + 3) * (R + 1)];
#pragma unroll
    for (int e = 0; e < kGE; ++e) {
      const float4 a = *reinterpret_cast<const float4 *>(a0 + e * W + j);
      h[e] = fmaf(a.x, w0, h[e]); h[e] = fmaf(a.y, w1, h[e]);
      h[e] = fmaf(a.z, w2, h[e]); h[e] = fmaf(a.w, w3, h[e]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <int R>
__global__ __launch_bounds__(kThreads) void cross_mix_fwd_kernel(const float *__restrict__ T, int64_t ldt,
                                                                 const float *__restrict__ S, int64_t lds,
                                                                 const float *__restrict__ C, int E, int64_t B, int G,
                                                                 float *__restrict__ M, int64_t ldm) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int W = E * R;
  float *As = sm;                       // [G][W]
  float *Cs = As + G * W;               // [E][R][R + 1]
  float *Ps = Cs + E * R * (R + 1);     // [G][E]
  stage_c<R>(C, E, Cs);
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    const int n4 = (n + kGE - 1) / kGE * kGE;
    __syncthreads();
    stage_ap(T, ldt, S, lds, base, n, n4, E, W, As, Ps);
    __syncthreads();
    const int items = n4 / kGE * W;
    for (int q = threadIdx.x; q < items; q += kThreads) {
      const int eg = q / W, col = q - eg * W, i = col / R, k = col - i * R, g0 = eg * kGE;
      float h[kGE];
      item_h<R>(As, Cs, W, g0, i, k, h);
#pragma unroll
      for (int e = 0; e < kGE; ++e)
        if (g0 + e < n) M[(base + g0 + e) * ldm + col] = Ps[(g0 + e) * E + i] * mix_tanh(h[e]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
template <int R>
__global__ __launch_bounds__(kThreads) void cross_mix_bwd_kernel(const float *__restrict__ T, int64_t ldt,
                                                                 const float *__restrict__ S, int64_t lds,
                                                                 const float *__restrict__ C, int E, int64_t B, int G,
                                                                 const float *__restrict__ dM, int64_t lddm,
                                                                 float *__restrict__ dT, int64_t lddt,
                                                                 float *__restrict__ dS, int64_t ldds,
                                                                 float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int CS = R * (R + 1);
  constexpr int JS = kThreads / R;                       // rows of C_i one sweep of the block covers
  constexpr int U = R * R > kThreads ? R * R / kThreads : 1;  // dC_i positions per thread
  constexpr int EMAX = 256 / R < 8 ? 256 / R : 8;
  const int W = E * R;
  float *As = sm;               // [G][W]
  float *Dh = As + G * W;       // [G][W]
  float *Cs = Dh + G * W;       // [E][R][R + 1]
  float *Ps = Cs + E * CS;      // [G][E]
  float *Dp = Ps + G * E;       // [G][E]
  stage_c<R>(C, E, Cs);
  const int kc = threadIdx.x % R, jc = threadIdx.x / R;  // this thread's dC_i positions: (jc + JS u, kc)
  float acc[EMAX][U];
#pragma unroll
  for (int i = 0; i < EMAX; ++i)
#pragma unroll
    for (int u = 0; u < U; ++u) acc[i][u] = 0.f;

  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    const int n = (int)(B - base < G ? B - base : G);
    const int n4 = (n + kGE - 1) / kGE * kGE;
    __syncthreads();
    stage_ap(T, ldt, S, lds, base, n, n4, E, W, As, Ps);
    __syncthreads();
    const int items = n4 / kGE * W;  // a multiple of R: the R lanes of one (examples, expert) stay together
    // c rebuilt; dp = <dm_i, c_i> over the expert's R lanes; dh -> LDS
    for (int q0 = 0; q0 < items; q0 += kThreads) {
      const int q = q0 + threadIdx.x;
      const bool valid = q < items;
      const int qq = valid ? q : 0;
      const int eg = qq / W, col = qq - eg * W, i = col / R, k = col - i * R, g0 = eg * kGE;
      float h[kGE];
      item_h<R>(As, Cs, W, g0, i, k, h);
#pragma unroll
      for (int e = 0; e < kGE; ++e) {
        const int g = g0 + e;
        const bool live = valid && g < n;
        const float c = mix_tanh(h[e]);
        const float dm = live ? dM[(base + g) * lddm + col] : 0.f;
        const float p = live ? Ps[g * E + i] : 0.f;
        const float dp = rm_group_sum<R>(dm * c);
        if (valid) {
          Dh[g * W + col] = (p * dm) * (1.f - c * c);
          if (k == 0 && g < n) Dp[g * E + i] = dp;
        }
      }
    }
    __syncthreads();
    // ds_i = p_i (dp_i - sum_j p_j dp_j)
    for (int q = threadIdx.x; q < n * E; q += kThreads) {
      const int g = q / E;
      float sum = 0.f;
      for (int j = 0; j < E; ++j) sum = fmaf(Ps[g * E + j], Dp[g * E + j], sum);
      dS[(base + g) * ldds + (q - g * E)] = Ps[q] * (Dp[q] - sum);
    }
    // da_i = dh_i C_i^T (k ascending), dt = da o (1 - a^2)
    for (int q = threadIdx.x; q < items; q += kThreads) {
      const int eg = q / W, col = q - eg * W, i = col / R, j = col - i * R, g0 = eg * kGE;
      const float *d0 = Dh + g0 * W + i * R;
      const float *c0 = Cs + i * CS + j * (R + 1);
      float da[kGE];
#pragma unroll
      for (int e = 0; e < kGE; ++e) da[e] = 0.f;
#pragma unroll 2
      for (int k = 0; k < R; k += 4) {
        const float w0 = c0[k], w1 = c0[k + 1], w2 = c0[k + 2], w3 = c0[k + 3];
#pragma unroll
        for (int e = 0; e < kGE; ++e) {
          const float4 d = *reinterpret_cast<const float4 *>(d0 + e * W + k);
          da[e] = fmaf(d.x, w0, da[e]); da[e] = fmaf(d.y, w1, da[e]);
          da[e] = fmaf(d.z, w2, da[e]); da[e] = fmaf(d.w, w3, da[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < kGE; ++e)
        if (g0 + e < n) {
          const float a = As[(g0 + e) * W + col];
          dT[(base + g0 + e) * lddt + col] = da[e] * (1.f - a * a);
        }
    }
    // dC_i[j][k] += sum_g a[g][i r + j] dh[g][i r + k], g ascending
    if (R >= 16 || jc < R) {
#pragma unroll
      for (int i = 0; i < EMAX; ++i) {
        if (i < E) {
          for (int g = 0; g < n; ++g) {
            const float d = Dh[g * W + i * R + kc];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[i][u] = fmaf(As[g * W + i * R + jc + JS * u], d, acc[i][u]);
          }
        }
      }
    }
  }
  if (R >= 16 || jc < R) {
    float *mine = part + (int64_t)blockIdx.x * E * R * R;
#pragma unroll
    for (int i = 0; i < EMAX; ++i)
      if (i < E) {
#pragma unroll
        for (int u = 0; u < U; ++u) mine[i * R * R + (jc + JS * u) * R + kc] = acc[i][u];
      }
  }
}

int mix_check(const char *fn, int E, int r, int64_t B) {
  RM_REQUIRE(mix_r_ok(r), "%s: r=%d unsupported (8, 16, 32, 64)", fn, r);
  RM_REQUIRE(E >= 1 && E <= 8, "%s: E=%d unsupported (1..8)", fn, E);
  RM_REQUIRE(E * r <= 256, "%s: E r = %d unsupported (at most 256)", fn, E * r);
  RM_REQUIRE(B >= 0, "%s: bad batch size", fn);
  return RM_OK;
}

#define RM_MIX_STRIDE(fn, name, ld, width)                                                                  \
  RM_REQUIRE((ld) >= (width) && (ld) <= kRmMaxStride, "%s: %s=%lld must be in [%d, 2^24]", fn, name, (long long)(ld), \
             (int)(width))

}  // namespace

extern "C" int rm_cross_mix_supported(int E, int r) { return mix_ok(E, r) ? 1 : 0; }

extern "C" int rm_cross_mix_fwd(const float *T, int64_t ldt, const float *S, int64_t lds, const float *C, int E, int r,
                                int64_t B, float *M, int64_t ldm, rm_stream_t stream) {
  const char *fn = "rm_cross_mix_fwd";
  int rc = mix_check(fn, E, r, B);
  if (rc != RM_OK) return rc;
  const int W = E * r;
  RM_MIX_STRIDE(fn, "ldt", ldt, W);
  RM_MIX_STRIDE(fn, "lds", lds, E);
  RM_MIX_STRIDE(fn, "ldm", ldm, W);
  if (B == 0) return RM_OK;
  RM_REQUIRE_PTR(fn, T);
  RM_REQUIRE_PTR(fn, S);
  RM_REQUIRE_PTR(fn, C);
  RM_REQUIRE_PTR(fn, M);
  const int G = mix_tile(W);
  const size_t smem = ((size_t)G * W + (size_t)E * r * (r + 1) + (size_t)G * E) * sizeof(float);
  dim3 grid(mix_blocks(B, G, kFwdBlocks));
  hipStream_t st = (hipStream_t)stream;
#define RM_MIX_FWD(R_) \
  rm_launch_lds(cross_mix_fwd_kernel<R_>, grid, dim3(kThreads), smem, st, T, ldt, S, lds, C, E, B, G, M, ldm);
  switch (r) {
    case 8: RM_MIX_FWD(8) break;
    case 16: RM_MIX_FWD(16) break;
    case 32: RM_MIX_FWD(32) break;
    default: RM_MIX_FWD(64) break;
  }
#undef RM_MIX_FWD
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int64_t rm_cross_mix_bwd_workspace(int64_t B, int E, int r) {
  if (!mix_ok(E, r) || B < 0) return -1;
  if (B == 0) return 0;
  return (int64_t)mix_blocks(B, mix_tile(E * r), kBwdBlocks) * E * r * r;
}

extern "C" int rm_cross_mix_bwd(const float *T, int64_t ldt, const float *S, int64_t lds, const float *C, int E, int r,
                                int64_t B, const float *dM, int64_t lddm, float *dT, int64_t lddt, float *dS,
                                int64_t ldds, float *dC, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_cross_mix_bwd";
  int rc = mix_check(fn, E, r, B);
  if (rc != RM_OK) return rc;
  const int W = E * r, N = E * r * r;
  RM_MIX_STRIDE(fn, "ldt", ldt, W);
  RM_MIX_STRIDE(fn, "lds", lds, E);
  RM_MIX_STRIDE(fn, "lddm", lddm, W);
  RM_MIX_STRIDE(fn, "lddt", lddt, W);
  RM_MIX_STRIDE(fn, "ldds", ldds, E);
  RM_REQUIRE_PTR(fn, dC);
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) return rm_clear_async(fn, "dC", dC, N, st);  // the sum over an empty batch
  RM_REQUIRE_PTR(fn, T);
  RM_REQUIRE_PTR(fn, S);
  RM_REQUIRE_PTR(fn, C);
  RM_REQUIRE_PTR(fn, dM);
  RM_REQUIRE_PTR(fn, dT);
  RM_REQUIRE_PTR(fn, dS);
  RM_REQUIRE_PTR(fn, workspace);
  const int G = mix_tile(W);
  const size_t smem = ((size_t)2 * G * W + (size_t)E * r * (r + 1) + (size_t)2 * G * E) * sizeof(float);
  const int nblk = mix_blocks(B, G, kBwdBlocks);
#define RM_MIX_BWD(R_)                                                                                         \
  rm_launch_lds(cross_mix_bwd_kernel<R_>, dim3(nblk), dim3(kThreads), smem, st, T, ldt, S, lds, C, E, B, G, dM, lddm, \
                dT, lddt, dS, ldds, workspace);
  switch (r) {
    case 8: RM_MIX_BWD(8) break;
    case 16: RM_MIX_BWD(16) break;
    case 32: RM_MIX_BWD(32) break;
    default: RM_MIX_BWD(64) break;
  }
#undef RM_MIX_BWD
  RM_CHECK_LAUNCH(fn);
  rm_sum_partials(workspace, nblk, N, rm_sum_dsts(dC, N), st);  // dC = the blocks' partials, in block order
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
