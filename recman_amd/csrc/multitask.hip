// Multi-task learning (see recman_hip.h and recman_hip_multitask.h): the gate softmax + expert mixture of all tasks,
// forward and backward - MMoE's (Ma et al., KDD 2018) and the grouped one of an extraction level of PLE / CGC (Tang et
// al., RecSys 2020) - and the loss head for several labels, plain and with ESMM's entire-space pair (Ma et al., SIGIR
// 2018).  Nothing in the reference implements them.
//
// Mixture kernels.  Per example: Z [N, H] expert outputs (N = T S + C: S own experts per task, then C shared ones),
//   A the gate logits (T task gates of width W = S + C, then - with shared_gate - one gate over all N), M [gates, H].
//   MMoE is the same mixture with S = 0, C = E and no shared gate: Z [E, H], A [T, E], M [T, H] = softmax(A_t) Z.  The
//   kernels are compiled once for each (Grouped = false: S and the shared gate are 0 at compile time, so the own-expert
//   loops, the shared gate's accumulators and every test of shared_gate are not there).
//   A lane group of G lanes owns an example, G = the power of two >= H / 4, at most 64: lane i of the group holds the
//   16-byte column vectors i (and i + 64 when H > 256) of every row it touches.  A block of W waves (W = 4; halved
//   while the gate weights of its tile would pass 64 KB of LDS) owns a TILE of W * 64 / G examples and walks tiles
//   blockIdx.x, blockIdx.x + gridDim.x, ..; the grid is min(tiles, kMixBlocks = 1024) blocks.  (E = 2, T = 2, H = 8:
//   G = 2, a tile of 128 examples, so from B > 128 * 1024 on a block walks more than one tile - rm_mmoe_mix_tile.)
//   The gate weights of a tile live in LDS only: the group's lanes load the example's logits (consecutive addresses),
//   one lane per gate turns its logits into the softmax (max-subtracted), every lane then reads p_ge as a broadcast.
//   An expert belongs to one task gate (its own) or to all of them (a shared one), and to the shared gate.  The
//   experts are walked once in Z's order - the T groups of S (the task index unrolled, so every accumulator stays in a
//   register), then the C shared ones - and every Z column vector is loaded once, the next expert's in flight while
//   this one is mixed.  The accumulation order is fixed, there is no atomic and no workspace: two runs are bit-equal.
//   The backward forms c_ge = <dM_g, Z_e> by a butterfly over the group's lanes (in-wave shuffles).
//   The row strides reach the kernels as ints (mix_operand bounds them by kRmMaxStride = 2^24; a row's offset b * ld is
//   formed in 64 bits).
#include "rm_launch.h"

#include "../../include/recman_hip_multitask.h"

namespace {

constexpr int kMixBlocks = 1024;      // grid cap of both mixture kernels
constexpr int kMixThreads = 256;      // at most; a block is W waves
constexpr int kMixLdsBytes = 64 * 1024;
constexpr int kMaxE = 16, kMaxT = 8, kMaxS = 4, kMaxC = 8, kMaxN = 32, kMaxH = 512;

#define MMOE_LIMITS \
  "1 <= E <= 16 experts, 1 <= T <= 8 tasks, H a multiple of 4 in 4..512, row strides multiples of 4 floats"
#define CGC_LIMITS                                                                                                  \
  "1 <= T <= 8 tasks, 1 <= S <= 4 task experts, 1 <= C <= 8 shared experts, N = T S + C <= 32, H a multiple of 4 " \
  "in 4..512, shared_gate 0 or 1, row strides multiples of 4 floats"

// What an entry point mixes.  MMoE: S = 0, C = E, sg = 0.
struct MixShape {
  bool grouped;
  int T, S, C, H, sg;
  int experts() const { return T * S + C; }
  int logits() const { return T * (S + C) + (sg ? experts() : 0); }  // gate logits per example
  int gates() const { return T + sg; }
  const char *limits() const { return grouped ? CGC_LIMITS : MMOE_LIMITS; }
};

struct MixGeom {
  int lg;       // log2 G
  int chunks;   // 16-byte column vectors per lane (1 or 2)
  int waves;    // waves per block
  int tile;     // examples per block and tile
  int pstride;  // floats per example in LDS (the gate logits, made odd: groups land on different banks)
  size_t lds;   // bytes
};

inline MixGeom mix_geom(const MixShape &s, bool backward) {
  MixGeom g;
  const int h4 = s.H / 4;
  g.lg = 0;
  while ((1 << g.lg) < h4 && g.lg < 6) ++g.lg;
  g.chunks = (h4 + 63) / 64;
  g.pstride = s.logits() | 1;
  const int per_wave = 64 >> g.lg;
  g.waves = kMixThreads / 64;
  const int copies = backward ? 2 : 1;
  while (g.waves > 1 && (size_t)g.waves * per_wave * g.pstride * copies * sizeof(float) > (size_t)kMixLdsBytes)
    g.waves /= 2;
  g.tile = g.waves * per_wave;
  g.lds = (size_t)g.tile * g.pstride * copies * sizeof(float);
  return g;
}

// A run-time loop that stays one: not unrolled, and not versioned into an interleaved copy and a remainder either (the
// copies of the short logit loops held the scalar registers that made one backward instantiation spill).
#define RM_PLAIN_LOOP _Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void fma4(float4 &a, float s, const float4 &v) {
  a.x = fmaf(s, v.x, a.x); a.y = fmaf(s, v.y, a.y); a.z = fmaf(s, v.z, a.z); a.w = fmaf(s, v.w, a.w);
}
__device__ __forceinline__ float dot4(const float4 &a, const float4 &b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// the example's AW logits -> LDS (consecutive lanes, consecutive addresses)
__device__ __forceinline__ void stage_logits(const float *__restrict__ A, int lda, int64_t b, bool live, int li,
                                             int G, int AW, float *__restrict__ sp) {
  if (live)
    RM_PLAIN_LOOP
    for (int q = li; q < AW; q += G) sp[q] = A[b * lda + q];
}

// one lane per gate: its logits in LDS (W of them at g W for a task gate, N at T W for the shared gate) become the
// softmax weights, in place
__device__ __forceinline__ void softmax_gates(bool live, int li, int G, int T, int W, int N, int sg,
                                              float *__restrict__ sp) {
  if (!live) return;
  RM_PLAIN_LOOP
  for (int g = li; g < T + sg; g += G) {
    float *s = sp + (g < T ? g * W : T * W);
    const int n = g < T ? W : N;
    float mx = s[0];
    RM_PLAIN_LOOP
    for (int e = 1; e < n; ++e) mx = fmaxf(mx, s[e]);
    float sum = 0.f;
    RM_PLAIN_LOOP
    for (int e = 0; e < n; ++e) {
      const float v = expf(s[e] - mx);
      s[e] = v;
      sum += v;
    }
    RM_PLAIN_LOOP
    for (int e = 0; e < n; ++e) s[e] = s[e] / sum;
  }
}

// T: the tasks (the columns of M of their gates and - Grouped - of the shared gate live in registers); CH: 16-byte
// column vectors per lane; Grouped = false: MMoE, whatever S_ and sg_ say
template <int T, int CH, bool Grouped>
__global__ __launch_bounds__(kMixThreads) void mix_fwd_kernel(
    const float *__restrict__ Z, int ldz, const float *__restrict__ A, int lda, int64_t B, int S_, int C, int H,
    int sg_, float *__restrict__ M, int ldm, float *__restrict__ P, int ldp, int lg) {
  extern __shared__ float smem[];
  constexpr int TG = T + (Grouped ? 1 : 0);  // the gates that may be there
  const int S = Grouped ? S_ : 0, sg = Grouped ? sg_ : 0;
  const int G = 1 << lg, li = threadIdx.x & (G - 1), ex = threadIdx.x >> lg;
  const int tile = blockDim.x >> lg, W = S + C, N = T * S + C, AW = T * W + (sg ? N : 0), h4 = H >> 2;
  const int pstride = AW | 1;  // MixGeom::pstride
  float *sp = smem + ex * pstride;
  const float *psh = sp + T * W;  // the shared gate's weights, in Z's expert order
  for (int64_t b0 = (int64_t)blockIdx.x * tile; b0 < B; b0 += (int64_t)gridDim.x * tile) {  // the block's tiles
    const int64_t b = b0 + ex;
    const bool live = b < B;
    const float *zrow = Z + b * ldz;
    float *mrow = M + b * ldm;
    bool on[CH];
    float4 z[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      on[c] = live && (li + 64 * c) < h4;
      z[c] = on[c] ? ld4(zrow + 4 * (li + 64 * c)) : zero4();
    }
    stage_logits(A, lda, b, live, li, G, AW, sp);
    __syncthreads();
    softmax_gates(live, li, G, T, W, N, sg, sp);
    __syncthreads();
    float4 acc[TG][CH];
#pragma unroll
    for (int t = 0; t < TG; ++t)
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[t][c] = zero4();
    int e = 0;  // the expert whose columns z holds
    if (Grouped) {
#pragma unroll
      for (int t = 0; t < T; ++t) {  // task t's own experts: its gate and the shared gate
        RM_PLAIN_LOOP
        for (int j = 0; j < S; ++j, ++e) {
          float4 zn[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c)  // the next expert's columns are in flight while this one is mixed
            zn[c] = (on[c] && e + 1 < N) ? ld4(zrow + (e + 1) * H + 4 * (li + 64 * c)) : z[c];
          const float p = live ? sp[t * W + j] : 0.f;
#pragma unroll
          for (int c = 0; c < CH; ++c) fma4(acc[t][c], p, z[c]);
          if (sg) {
            const float ps = live ? psh[e] : 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) fma4(acc[TG - 1][c], ps, z[c]);
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) z[c] = zn[c];
        }
      }
    }
    RM_PLAIN_LOOP
    for (int j = 0; j < C; ++j, ++e) {  // the shared experts: every gate
      float4 zn[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c)
        zn[c] = (on[c] && e + 1 < N) ? ld4(zrow + (e + 1) * H + 4 * (li + 64 * c)) : z[c];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float p = live ? sp[t * W + S + j] : 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) fma4(acc[t][c], p, z[c]);
      }
      if (Grouped && sg) {
        const float ps = live ? psh[e] : 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) fma4(acc[TG - 1][c], ps, z[c]);
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) z[c] = zn[c];
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (on[c]) st4(mrow + (t * H + 4 * (li + 64 * c)), acc[t][c]);
    if (Grouped && sg)
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (on[c]) st4(mrow + (T * H + 4 * (li + 64 * c)), acc[TG - 1][c]);
    if (P != nullptr && live)
      RM_PLAIN_LOOP
      for (int q = li; q < AW; q += G) P[b * ldp + q] = sp[q];
    __syncthreads();  // the tile's weights are read: the next tile may overwrite them
  }
}

template <int T, int CH, bool Grouped>
__global__ __launch_bounds__(kMixThreads) void mix_bwd_kernel(
    const float *__restrict__ Z, int ldz, const float *__restrict__ A, int lda, const float *__restrict__ dM, int lddm,
    int64_t B, int S_, int C, int H, int sg_, float *__restrict__ dZ, int lddz, float *__restrict__ dA, int ldda,
    int lg) {
  extern __shared__ float smem[];
  constexpr int TG = T + (Grouped ? 1 : 0);
  const int S = Grouped ? S_ : 0, sg = Grouped ? sg_ : 0;
  const int G = 1 << lg, li = threadIdx.x & (G - 1), ex = threadIdx.x >> lg;
  const int tile = blockDim.x >> lg, W = S + C, N = T * S + C, AW = T * W + (sg ? N : 0), h4 = H >> 2;
  const int pstride = AW | 1;  // MixGeom::pstride
  float *sp = smem + ex * pstride;                       // p_ge
  float *sc = smem + (tile + ex) * pstride;              // c_ge, then dA_ge
  const float *psh = sp + T * W;
  float *csh = sc + T * W;
  for (int64_t b0 = (int64_t)blockIdx.x * tile; b0 < B; b0 += (int64_t)gridDim.x * tile) {  // the block's tiles
    const int64_t b = b0 + ex;
    const bool live = b < B;
    const float *zrow = Z + b * ldz, *dmrow = dM + b * lddm;
    float *dzrow = dZ + b * lddz;
    bool on[CH];
    float4 z[CH], dm[TG][CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      on[c] = live && (li + 64 * c) < h4;
      z[c] = on[c] ? ld4(zrow + 4 * (li + 64 * c)) : zero4();
    }
#pragma unroll
    for (int t = 0; t < TG; ++t)
#pragma unroll
      for (int c = 0; c < CH; ++c)
        dm[t][c] = (on[c] && (t < T || sg)) ? ld4(dmrow + (t * H + 4 * (li + 64 * c))) : zero4();
    stage_logits(A, lda, b, live, li, G, AW, sp);
    __syncthreads();
    softmax_gates(live, li, G, T, W, N, sg, sp);
    __syncthreads();
    int e = 0;
    if (Grouped) {
#pragma unroll
      for (int t = 0; t < T; ++t) {  // task t's own experts
        RM_PLAIN_LOOP
        for (int j = 0; j < S; ++j, ++e) {
          float4 zn[CH], dz[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c)
            zn[c] = (on[c] && e + 1 < N) ? ld4(zrow + (e + 1) * H + 4 * (li + 64 * c)) : z[c];
          const float p = live ? sp[t * W + j] : 0.f;
          float dot = 0.f, dots = 0.f;
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            dz[c] = zero4();
            fma4(dz[c], p, dm[t][c]);
            dot = dot4(dm[t][c], z[c], dot);
          }
          if (sg) {
            const float ps = live ? psh[e] : 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
              fma4(dz[c], ps, dm[TG - 1][c]);
              dots = dot4(dm[TG - 1][c], z[c], dots);
            }
          }
          // c_ge: the lanes' partial dot products summed over the group (a butterfly: every lane gets the total)
          RM_PLAIN_LOOP
          for (int o = G >> 1; o > 0; o >>= 1) {
            dot += __shfl_xor(dot, o, 64);
            dots += __shfl_xor(dots, o, 64);
          }
          if (live && li == 0) {
            sc[t * W + j] = dot;
            if (sg) csh[e] = dots;
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            if (on[c]) st4(dzrow + (e * H + 4 * (li + 64 * c)), dz[c]);
            z[c] = zn[c];
          }
        }
      }
    }
    RM_PLAIN_LOOP
    for (int j = 0; j < C; ++j, ++e) {  // the shared experts
      float4 zn[CH], dz[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        zn[c] = (on[c] && e + 1 < N) ? ld4(zrow + (e + 1) * H + 4 * (li + 64 * c)) : z[c];
        dz[c] = zero4();
      }
      float dot[TG];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        dot[t] = 0.f;
        const float p = live ? sp[t * W + S + j] : 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          fma4(dz[c], p, dm[t][c]);
          dot[t] = dot4(dm[t][c], z[c], dot[t]);
        }
      }
      if (Grouped) dot[TG - 1] = 0.f;
      if (Grouped && sg) {
        const float ps = live ? psh[e] : 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          fma4(dz[c], ps, dm[TG - 1][c]);
          dot[TG - 1] = dot4(dm[TG - 1][c], z[c], dot[TG - 1]);
        }
      }
      RM_PLAIN_LOOP
      for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
        for (int t = 0; t < TG; ++t) dot[t] += __shfl_xor(dot[t], o, 64);
      }
      if (live && li == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) sc[t * W + S + j] = dot[t];
        if (Grouped && sg) csh[e] = dot[TG - 1];
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (on[c]) st4(dzrow + (e * H + 4 * (li + 64 * c)), dz[c]);
        z[c] = zn[c];
      }
    }
    __syncthreads();
    // one lane per gate: dA_ge = p_ge (c_ge - sum_e' p_ge' c_ge'), in place over c
    if (live)
      RM_PLAIN_LOOP
      for (int g = li; g < T + sg; g += G) {
        const int off = g < T ? g * W : T * W, n = g < T ? W : N;
        const float *p = sp + off;
        float *c = sc + off;
        float s = 0.f;
        RM_PLAIN_LOOP
        for (int k = 0; k < n; ++k) s = fmaf(p[k], c[k], s);
        RM_PLAIN_LOOP
        for (int k = 0; k < n; ++k) c[k] = p[k] * (c[k] - s);
      }
    __syncthreads();
    if (live)
      RM_PLAIN_LOOP
      for (int q = li; q < AW; q += G) dA[b * ldda + q] = sc[q];
  }
}

// a [B, width] operand: 16-byte aligned rows (pointer and stride), stride >= width
int mix_operand(const char *fn, const MixShape &s, const char *name, const void *p, int64_t ld, int width) {
  RM_REQUIRE(p != nullptr, "%s: %s is NULL", fn, name);
  RM_REQUIRE(ld >= width, "%s: row stride of %s = %lld < its %d columns", fn, name, (long long)ld, width);
  RM_REQUIRE(ld % 4 == 0 && rm_aligned16(p) && ld <= kRmMaxStride,
             "%s: %s must be 16-byte aligned with a row stride that is a multiple of 4 floats (got stride %lld; "
             "limits: %s)", fn, name, (long long)ld, s.limits());
  return RM_OK;
}

#define MIX_CASE(KERNEL, GROUPED, t, chunks, ...)                         \
  case t:                                                                 \
    if ((chunks) == 1) rm_launch_lds(KERNEL<t, 1, GROUPED>, __VA_ARGS__); \
    else rm_launch_lds(KERNEL<t, 2, GROUPED>, __VA_ARGS__);               \
    break;
#define MIX_SWITCH(KERNEL, GROUPED, T, chunks, ...)     \
  switch (T) {                                          \
    MIX_CASE(KERNEL, GROUPED, 1, chunks, __VA_ARGS__)   \
    MIX_CASE(KERNEL, GROUPED, 2, chunks, __VA_ARGS__)   \
    MIX_CASE(KERNEL, GROUPED, 3, chunks, __VA_ARGS__)   \
    MIX_CASE(KERNEL, GROUPED, 4, chunks, __VA_ARGS__)   \
    MIX_CASE(KERNEL, GROUPED, 5, chunks, __VA_ARGS__)   \
    MIX_CASE(KERNEL, GROUPED, 6, chunks, __VA_ARGS__)   \
    MIX_CASE(KERNEL, GROUPED, 7, chunks, __VA_ARGS__)   \
    default:                                            \
      MIX_CASE(KERNEL, GROUPED, 8, chunks, __VA_ARGS__) \
  }
#define MIX_DISPATCH(KERNEL, shape, chunks, ...)                           \
  do {                                                                     \
    if ((shape).grouped) MIX_SWITCH(KERNEL, true, (shape).T, chunks, __VA_ARGS__) \
    else MIX_SWITCH(KERNEL, false, (shape).T, chunks, __VA_ARGS__)         \
  } while (0)

// The forward of both entry points, whose own limits `s` has passed.
int mix_fwd(const char *fn, const MixShape &s, const float *Z, int64_t ldz, const float *A, int64_t lda, int64_t B,
            float *M, int64_t ldm, float *P, int64_t ldp, rm_stream_t stream) {
  RM_REQUIRE(B >= 0 && B < ((int64_t)1 << 40), "%s: bad B=%lld", fn, (long long)B);
  if (B == 0) return RM_OK;
  if (int rc = mix_operand(fn, s, "Z", Z, ldz, s.experts() * s.H)) return rc;
  if (int rc = mix_operand(fn, s, "A", A, lda, s.logits())) return rc;
  if (int rc = mix_operand(fn, s, "M", M, ldm, s.gates() * s.H)) return rc;
  if (P != nullptr)
    if (int rc = mix_operand(fn, s, "P", P, ldp, s.logits())) return rc;
  const MixGeom g = mix_geom(s, false);
  const int64_t ntiles = (B + g.tile - 1) / g.tile;
  MIX_DISPATCH(mix_fwd_kernel, s, g.chunks, dim3(rm_grid_cap(ntiles, kMixBlocks)), dim3(g.waves * 64), g.lds,
               (hipStream_t)stream, Z, (int)ldz, A, (int)lda, B, s.S, s.C, s.H, s.sg, M, (int)ldm, P, (int)ldp, g.lg);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

int mix_bwd(const char *fn, const MixShape &s, const float *Z, int64_t ldz, const float *A, int64_t lda,
            const float *dM, int64_t lddm, int64_t B, float *dZ, int64_t lddz, float *dA, int64_t ldda,
            rm_stream_t stream) {
  RM_REQUIRE(B >= 0 && B < ((int64_t)1 << 40), "%s: bad B=%lld", fn, (long long)B);
  if (B == 0) return RM_OK;
  if (int rc = mix_operand(fn, s, "Z", Z, ldz, s.experts() * s.H)) return rc;
  if (int rc = mix_operand(fn, s, "A", A, lda, s.logits())) return rc;
  if (int rc = mix_operand(fn, s, "dM", dM, lddm, s.gates() * s.H)) return rc;
  if (int rc = mix_operand(fn, s, "dZ", dZ, lddz, s.experts() * s.H)) return rc;
  if (int rc = mix_operand(fn, s, "dA", dA, ldda, s.logits())) return rc;
  const MixGeom g = mix_geom(s, true);
  const int64_t ntiles = (B + g.tile - 1) / g.tile;
  MIX_DISPATCH(mix_bwd_kernel, s, g.chunks, dim3(rm_grid_cap(ntiles, kMixBlocks)), dim3(g.waves * 64), g.lds,
               (hipStream_t)stream, Z, (int)ldz, A, (int)lda, dM, (int)lddm, B, s.S, s.C, s.H, s.sg, dZ, (int)lddz, dA,
               (int)ldda, g.lg);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

// the limits of the two entry-point families, each with its own message
int mmoe_shape(const char *fn, int E, int T, int H, MixShape *s) {
  RM_REQUIRE(rm_mmoe_mix_supported(E, T, H), "%s: E=%d, T=%d, H=%d unsupported (" MMOE_LIMITS ")", fn, E, T, H);
  *s = MixShape{false, T, 0, E, H, 0};
  return RM_OK;
}

int cgc_shape(const char *fn, int T, int S, int C, int H, int sg, MixShape *s) {
  RM_REQUIRE(rm_cgc_mix_supported(T, S, C, H, sg), "%s: T=%d, S=%d, C=%d, H=%d, shared_gate=%d unsupported (" CGC_LIMITS
             ")", fn, T, S, C, H, sg);
  *s = MixShape{true, T, S, C, H, sg};
  return RM_OK;
}

// ------------------------------------------------------------------------------------------------ the loss head
// Three stages.  EntireSpace: task v is scored through q = p_c p_v against z (ESMM); without it c and v are not read.
constexpr int kLossBlock = 256;
constexpr int kLossBlocks = 256;  // per task

struct LossTasks {
  int type[kMaxT];
  float w[kMaxT];
  int c, v;
};

static int loss_blocks(int64_t B) { return rm_grid_cap((B + kLossBlock - 1) / kLossBlock, kLossBlocks); }

__device__ __forceinline__ float es_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// z of one example from its two labels; false: unobserved
__device__ __forceinline__ bool es_label(float yc, float yv, float *z) {
  if (yc == 0.f) {
    *z = 0.f;
    return true;
  }
  *z = yv;
  return yc == 1.f && yv == yv;
}

// The coupled term of one example with z observed: a, b the logits of c and v.  Returns l = Keras BCE(z, q), q =
// p_c p_v; *inside: q is outside the clip region; *gq = dl/dq * q there.  1 - q = (1 - p_c) + p_c (1 - p_v) with
// 1 - p = sigmoid(-logit): no cancellation.
__device__ __forceinline__ float es_point(float a, float b, float z, bool *inside, float *gq) {
  constexpr float kEps = 1e-7f;  // Keras backend epsilon()
  const float pc = es_sigmoid(a), pv = es_sigmoid(b);
  const float q = pc * pv, r = es_sigmoid(-a) + pc * es_sigmoid(-b);
  const bool low = q < kEps, high = r < kEps;
  const float qc = low ? kEps : (high ? 1.0f - kEps : q);
  const float rc = low ? 1.0f - kEps : (high ? kEps : r);
  const float u = qc + kEps, w = rc + kEps;
  *inside = !low && !high;
  *gq = -(z / u - (1.0f - z) / w) * q;
  return -(z * logf(u) + (1.0f - z) * logf(w));
}

// stage 1, grid (nblk, T): pred, and per block the observed count and the loss sum of its examples, in double
// (Y == NULL: inference, pred only)
template <bool EntireSpace>
__global__ __launch_bounds__(kLossBlock) void mt_loss_partial_kernel(const float *__restrict__ logit,
                                                                     const float *__restrict__ Y, LossTasks tasks,
                                                                     int64_t B, int T, float *__restrict__ pred,
                                                                     double *__restrict__ part) {
  __shared__ double sm[2 * kLossBlock / 64];
  const int t = blockIdx.y, type = tasks.type[t];
  const bool coupled = EntireSpace && t == tasks.v;
  double sum = 0.0, cnt = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
    const float x = logit[(int64_t)t * B + i];
    const float y = Y ? Y[i * T + t] : 0.f;
    float p, dz, l;
    bool seen;
    if (coupled) {
      float z, gq;
      bool inside;
      seen = es_label(Y[i * T + tasks.c], y, &z);
      p = es_sigmoid(x);
      l = seen ? es_point(logit[(int64_t)tasks.c * B + i], x, z, &inside, &gq) : 0.f;
    } else {
      seen = Y && y == y;
      l = rm_loss_point(x, seen ? y : 0.f, type, &p, &dz);
    }
    pred[(int64_t)t * B + i] = p;
    if (seen) {
      sum += (double)l;
      cnt += 1.0;
    }
  }
  // fixed order: a butterfly inside the wave, the waves in index order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sm[2 * (threadIdx.x >> 6)] = sum;
    sm[2 * (threadIdx.x >> 6) + 1] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0 && part) {
    double s = 0.0, c = 0.0;
    for (int w = 0; w < kLossBlock / 64; ++w) {
      s += sm[2 * w];
      c += sm[2 * w + 1];
    }
    part[2 * ((int64_t)t * gridDim.x + blockIdx.x)] = s;
    part[2 * ((int64_t)t * gridDim.x + blockIdx.x) + 1] = c;
  }
}

// stage 2, one wave: per task the blocks' partials in block order; n_t, loss_t, loss and each task's gradient scale
__global__ void mt_loss_finish_kernel(const double *__restrict__ part, int nblk, LossTasks tasks, int T,
                                      float grad_scale, int64_t *__restrict__ n_t, float *__restrict__ loss_t,
                                      float *__restrict__ loss, float *__restrict__ scale) {
  double total = 0.0;
  for (int t = 0; t < T; ++t) {
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) {
      s += part[2 * ((int64_t)t * nblk + i)];
      c += part[2 * ((int64_t)t * nblk + i) + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s += __shfl_xor(s, o, 64);
      c += __shfl_xor(c, o, 64);
    }
    const double mean = c > 0.0 ? s / c : 0.0;
    total += (double)tasks.w[t] * mean;
    if (threadIdx.x == 0) {
      if (n_t) n_t[t] = (int64_t)c;
      if (loss_t) loss_t[t] = (float)mean;
      scale[t] = c > 0.0 ? (float)((double)tasks.w[t] * (double)grad_scale / c) : 0.f;
    }
  }
  if (threadIdx.x == 0 && loss) loss[0] = (float)total;
}

// stage 3, grid (nblk, T): dlogit = dl/dlogit * w_t * grad_scale / n_t where the label is observed, +0.0 elsewhere.
// EntireSpace: task v's gradient through q, task c's own term plus its share of q's; +0.0 where a term's label is
// unobserved or q is clipped
template <bool EntireSpace>
__global__ __launch_bounds__(kLossBlock) void mt_loss_grad_kernel(const float *__restrict__ logit,
                                                                  const float *__restrict__ Y, LossTasks tasks,
                                                                  int64_t B, int T, const float *__restrict__ scale,
                                                                  float *__restrict__ dlogit) {
  const int t = blockIdx.y, type = tasks.type[t];
  const float sc = scale[t], scv = EntireSpace ? scale[tasks.v] : 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
    const float y = Y[i * T + t];
    float p, dz = 0.f;
    if ((!EntireSpace || t != tasks.v) && y == y) {
      (void)rm_loss_point(logit[(int64_t)t * B + i], y, type, &p, &dz);
      dz *= sc;
    }
    if (EntireSpace && (t == tasks.v || t == tasks.c)) {
      const float x = logit[(int64_t)t * B + i];
      const float yc = t == tasks.c ? y : Y[i * T + tasks.c], yv = t == tasks.v ? y : Y[i * T + tasks.v];
      const float a = t == tasks.c ? x : logit[(int64_t)tasks.c * B + i];
      const float b = t == tasks.v ? x : logit[(int64_t)tasks.v * B + i];
      float z, gq;
      bool inside;
      if (es_label(yc, yv, &z)) {
        (void)es_point(a, b, z, &inside, &gq);
        if (inside) dz += scv * gq * es_sigmoid(-x);  // q (1 - p) of the own logit
      }
    }
    dlogit[(int64_t)t * B + i] = dz;
  }
}

// Both loss entry points.  c = v = -1: no pair.  Without the pair, and at inference (pred[v] stays p_v), the pair's
// entry point is rm_multitask_loss itself: the same kernels, the same bits, its name in the messages.
int loss_head(const char *fn, const float *logit, const float *Y, const int *task_type, const float *task_weight,
              float grad_scale, int64_t B, int T, int c, int v, float *pred, float *dlogit, int64_t *n_t,
              float *loss_t, float *loss, float *workspace, rm_stream_t stream) {
  RM_REQUIRE(B > 0, "%s: B must be > 0 (got %lld)", fn, (long long)B);
  RM_REQUIRE(T >= 1 && T <= kMaxT, "%s: T=%d tasks unsupported (1 <= T <= 8)", fn, T);
  RM_REQUIRE(logit && pred && task_type, "%s: NULL argument", fn);
  const bool plain = c == -1 && v == -1;
  RM_REQUIRE(plain || (c >= 0 && c < T && v >= 0 && v < T && c != v && task_type[c] == 0 && task_type[v] == 0),
             "%s: es_ctr=%d, es_cvr=%d must be two distinct classification tasks below T=%d, or both -1", fn, c, v, T);
  const bool train = dlogit || n_t || loss_t || loss;
  const bool es = !plain && train;
  if (!es) fn = "rm_multitask_loss";
  RM_REQUIRE(!train || (Y && task_weight && workspace && rm_aligned16(workspace)),
             "%s: labels, task weights and a 16-byte aligned workspace are needed for the loss and its gradient", fn);
  LossTasks tasks;
  tasks.c = c;
  tasks.v = v;
  for (int t = 0; t < kMaxT; ++t) {
    tasks.type[t] = t < T ? task_type[t] : 0;
    tasks.w[t] = (t < T && task_weight) ? task_weight[t] : 0.f;
    RM_REQUIRE(tasks.type[t] == 0 || tasks.type[t] == 1, "%s: task type must be 0 (classification) or 1", fn);
  }
  const int nblk = loss_blocks(B);
  hipStream_t st = (hipStream_t)stream;
  double *part = train ? reinterpret_cast<double *>(workspace) : nullptr;
  float *scale = train ? workspace + 4 * (int64_t)T * nblk : nullptr;
  hipLaunchKernelGGL(es ? mt_loss_partial_kernel<true> : mt_loss_partial_kernel<false>, dim3(nblk, T),
                     dim3(kLossBlock), 0, st, logit, train ? Y : nullptr, tasks, B, T, pred, part);
  if (train) {
    hipLaunchKernelGGL(mt_loss_finish_kernel, dim3(1), dim3(64), 0, st, part, nblk, tasks, T, grad_scale, n_t, loss_t,
                       loss, scale);
    if (dlogit)
      hipLaunchKernelGGL(es ? mt_loss_grad_kernel<true> : mt_loss_grad_kernel<false>, dim3(nblk, T), dim3(kLossBlock),
                         0, st, logit, Y, tasks, B, T, scale, dlogit);
  }
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

}  // namespace

extern "C" int rm_mmoe_mix_supported(int E, int T, int H) {
  return E >= 1 && E <= kMaxE && T >= 1 && T <= kMaxT && H >= 4 && H <= kMaxH && H % 4 == 0;
}

extern "C" int rm_cgc_mix_supported(int T, int S, int C, int H, int shared_gate) {
  return T >= 1 && T <= kMaxT && S >= 1 && S <= kMaxS && C >= 1 && C <= kMaxC && T * S + C <= kMaxN && H >= 4 &&
         H <= kMaxH && H % 4 == 0 && (shared_gate == 0 || shared_gate == 1);
}

extern "C" int rm_mmoe_mix_tile(int E, int T, int H, int backward, int which) {
  if (!rm_mmoe_mix_supported(E, T, H)) return -1;
  return which == RM_MMOE_CAP ? kMixBlocks : mix_geom(MixShape{false, T, 0, E, H, 0}, backward != 0).tile;
}

extern "C" int rm_cgc_mix_tile(int T, int S, int C, int H, int shared_gate, int backward, int which) {
  if (!rm_cgc_mix_supported(T, S, C, H, shared_gate)) return -1;
  return which == RM_CGC_CAP ? kMixBlocks : mix_geom(MixShape{true, T, S, C, H, shared_gate}, backward != 0).tile;
}

extern "C" int rm_mmoe_mix_fwd(const float *Z, int64_t ldz, const float *A, int64_t lda, int64_t B, int E, int T,
                               int H, float *M, int64_t ldm, float *P, int64_t ldp, rm_stream_t stream) {
  MixShape s;
  if (int rc = mmoe_shape("rm_mmoe_mix_fwd", E, T, H, &s)) return rc;
  return mix_fwd("rm_mmoe_mix_fwd", s, Z, ldz, A, lda, B, M, ldm, P, ldp, stream);
}

extern "C" int rm_mmoe_mix_bwd(const float *Z, int64_t ldz, const float *A, int64_t lda, const float *dM,
                               int64_t lddm, int64_t B, int E, int T, int H, float *dZ, int64_t lddz, float *dA,
                               int64_t ldda, rm_stream_t stream) {
  MixShape s;
  if (int rc = mmoe_shape("rm_mmoe_mix_bwd", E, T, H, &s)) return rc;
  return mix_bwd("rm_mmoe_mix_bwd", s, Z, ldz, A, lda, dM, lddm, B, dZ, lddz, dA, ldda, stream);
}

extern "C" int rm_cgc_mix_fwd(const float *Z, int64_t ldz, const float *A, int64_t lda, int64_t B, int T, int S, int C,
                              int H, int shared_gate, float *M, int64_t ldm, float *P, int64_t ldp,
                              rm_stream_t stream) {
  MixShape s;
  if (int rc = cgc_shape("rm_cgc_mix_fwd", T, S, C, H, shared_gate, &s)) return rc;
  return mix_fwd("rm_cgc_mix_fwd", s, Z, ldz, A, lda, B, M, ldm, P, ldp, stream);
}

extern "C" int rm_cgc_mix_bwd(const float *Z, int64_t ldz, const float *A, int64_t lda, const float *dM, int64_t lddm,
                              int64_t B, int T, int S, int C, int H, int shared_gate, float *dZ, int64_t lddz,
                              float *dA, int64_t ldda, rm_stream_t stream) {
  MixShape s;
  if (int rc = cgc_shape("rm_cgc_mix_bwd", T, S, C, H, shared_gate, &s)) return rc;
  return mix_bwd("rm_cgc_mix_bwd", s, Z, ldz, A, lda, dM, lddm, B, dZ, lddz, dA, ldda, stream);
}

// floats: the per-block (sum, count) pairs in double, then T gradient scales
extern "C" int64_t rm_multitask_loss_workspace(int64_t B, int T) {
  if (B < 1 || T < 1 || T > kMaxT) return -1;
  return 4 * (int64_t)T * loss_blocks(B) + 2 * kMaxT;
}

extern "C" int64_t rm_multitask_loss_es_workspace(int64_t B, int T) { return rm_multitask_loss_workspace(B, T); }

extern "C" int rm_multitask_loss(const float *logit, const float *Y, const int *task_type, const float *task_weight,
                                 float grad_scale, int64_t B, int T, float *pred, float *dlogit, int64_t *n_t,
                                 float *loss_t, float *loss, float *workspace, rm_stream_t stream) {
  return loss_head("rm_multitask_loss", logit, Y, task_type, task_weight, grad_scale, B, T, -1, -1, pred, dlogit, n_t,
                   loss_t, loss, workspace, stream);
}

extern "C" int rm_multitask_loss_es(const float *logit, const float *Y, const int *task_type, const float *task_weight,
                                    float grad_scale, int64_t B, int T, int es_ctr, int es_cvr, float *pred,
                                    float *dlogit, int64_t *n_t, float *loss_t, float *loss, float *workspace,
                                    rm_stream_t stream) {
  return loss_head("rm_multitask_loss_es", logit, Y, task_type, task_weight, grad_scale, B, T, es_ctr, es_cvr, pred,
                   dlogit, n_t, loss_t, loss, workspace, stream);
}
