// Multi-gate mixture-of-experts (MMoE, Ma et al., KDD 2018): the gate softmax + expert mixture of all tasks, forward
// and backward, and the loss head for several labels (see recman_hip.h).  Nothing in the reference implements them.
//
// Mixture kernels.  Per example: Z [E, H] expert outputs, A [T, E] gate logits, M [T, H] = softmax(A_t) Z.
//   A lane group of G lanes owns an example, G = the power of two >= H / 4, at most 64: lane i of the group holds the
//   16-byte column vectors i (and i + 64 when H > 256) of every row it touches.  A block of W waves (W = 4; halved
//   while the gate weights of its tile would pass 64 KB of LDS) owns a TILE of W * 64 / G examples and walks tiles
//   blockIdx.x, blockIdx.x + gridDim.x, ..; the grid is min(tiles, kMixBlocks = 1024) blocks.  (E = 2, T = 2, H = 8:
//   G = 2, a tile of 128 examples, so from B > 128 * 1024 on a block walks more than one tile - rm_mmoe_mix_tile.)
//   The gate weights of a tile live in LDS only: the group's lanes load the example's T E logits (consecutive
//   addresses), one lane per task turns its E logits into p_t = softmax (max-subtracted), every lane then reads p_te
//   as a broadcast.  The accumulation order over e is fixed, there is no atomic, no workspace: two runs are bit-equal.
//   The backward forms c_te = <dM_t, Z_e> by a butterfly over the group's lanes (in-wave shuffles).
#include "rm_launch.h"

namespace {

constexpr int kMixBlocks = 1024;      // grid cap of both mixture kernels
constexpr int kMixThreads = 256;      // at most; a block is W waves
constexpr int kMixLdsBytes = 64 * 1024;
constexpr int kMaxE = 16, kMaxT = 8, kMaxH = 512;

struct MixGeom {
  int lg;       // log2 G
  int chunks;   // 16-byte column vectors per lane (1 or 2)
  int waves;    // waves per block
  int tile;     // examples per block and tile
  int pstride;  // floats per example in LDS (T E, made odd: groups land on different banks)
  size_t lds;   // bytes
};

inline MixGeom mix_geom(int E, int T, int H, bool backward) {
  MixGeom g;
  const int h4 = H / 4;
  g.lg = 0;
  while ((1 << g.lg) < h4 && g.lg < 6) ++g.lg;
  g.chunks = (h4 + 63) / 64;
  g.pstride = (T * E) | 1;
  const int per_wave = 64 >> g.lg;
  g.waves = kMixThreads / 64;
  const int copies = backward ? 2 : 1;
  while (g.waves > 1 && (size_t)g.waves * per_wave * g.pstride * copies * sizeof(float) > (size_t)kMixLdsBytes)
    g.waves /= 2;
  g.tile = g.waves * per_wave;
  g.lds = (size_t)g.tile * g.pstride * copies * sizeof(float);
  return g;
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void fma4(float4 &a, float s, const float4 &v) {
  a.x = fmaf(s, v.x, a.x); a.y = fmaf(s, v.y, a.y); a.z = fmaf(s, v.z, a.z); a.w = fmaf(s, v.w, a.w);
}
__device__ __forceinline__ float dot4(const float4 &a, const float4 &b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// the example's T E logits -> LDS (consecutive lanes, consecutive addresses)
__device__ __forceinline__ void stage_logits(const float *__restrict__ A, int64_t lda, int64_t b, bool live, int li,
                                             int G, int TE, float *__restrict__ sp) {
  if (live)
    #pragma nounroll
    for (int q = li; q < TE; q += G) sp[q] = A[b * lda + q];
}

// one lane per task: its E logits in LDS become the softmax weights, in place
__device__ __forceinline__ void softmax_tasks(bool live, int li, int G, int E, int T, float *__restrict__ sp) {
  if (!live) return;
  #pragma nounroll
  for (int t = li; t < T; t += G) {
    float *s = sp + t * E;
    float mx = s[0];
    #pragma nounroll
    for (int e = 1; e < E; ++e) mx = fmaxf(mx, s[e]);
    float sum = 0.f;
    #pragma nounroll
    for (int e = 0; e < E; ++e) {
      const float v = expf(s[e] - mx);
      s[e] = v;
      sum += v;
    }
    #pragma nounroll
    for (int e = 0; e < E; ++e) s[e] = s[e] / sum;
  }
}

// T: the tasks (their columns of M / dM live in registers); C: 16-byte column vectors per lane
template <int T, int C>
__global__ __launch_bounds__(kMixThreads) void mmoe_mix_fwd_kernel(
    const float *__restrict__ Z, int64_t ldz, const float *__restrict__ A, int64_t lda, int64_t B, int E, int H,
    float *__restrict__ M, int64_t ldm, float *__restrict__ P, int64_t ldp, int lg, int pstride) {
  extern __shared__ float smem[];
  const int G = 1 << lg, li = threadIdx.x & (G - 1), ex = threadIdx.x >> lg;
  const int tile = blockDim.x >> lg, TE = T * E, h4 = H >> 2;
  float *sp = smem + ex * pstride;
  const int64_t ntiles = (B + tile - 1) / tile;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t b = tl * tile + ex;
    const bool live = b < B;
    const float *zrow = Z + b * ldz;
    float *mrow = M + b * ldm;
    bool on[C];
    float4 z[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      on[c] = live && (li + 64 * c) < h4;
      z[c] = on[c] ? ld4(zrow + 4 * (li + 64 * c)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    stage_logits(A, lda, b, live, li, G, TE, sp);
    __syncthreads();
    softmax_tasks(live, li, G, E, T, sp);
    __syncthreads();
    float4 acc[T][C];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[t][c] = make_float4(0.f, 0.f, 0.f, 0.f);
    #pragma nounroll
    for (int e = 0; e < E; ++e) {
      float4 zn[C];
#pragma unroll
      for (int c = 0; c < C; ++c)  // the next expert's columns are in flight while this one is mixed
        zn[c] = (on[c] && e + 1 < E) ? ld4(zrow + (e + 1) * H + 4 * (li + 64 * c)) : z[c];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float p = live ? sp[t * E + e] : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) fma4(acc[t][c], p, z[c]);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) z[c] = zn[c];
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (on[c]) st4(mrow + (t * H + 4 * (li + 64 * c)), acc[t][c]);
    if (P != nullptr && live)
      #pragma nounroll
      for (int q = li; q < TE; q += G) P[b * ldp + q] = sp[q];
    __syncthreads();  // the tile's weights are read: the next tile may overwrite them
  }
}

template <int T, int C>
__global__ __launch_bounds__(kMixThreads) void mmoe_mix_bwd_kernel(
    const float *__restrict__ Z, int64_t ldz, const float *__restrict__ A, int64_t lda, const float *__restrict__ dM,
    int64_t lddm, int64_t B, int E, int H, float *__restrict__ dZ, int64_t lddz, float *__restrict__ dA,
    int64_t ldda, int lg, int pstride) {
  extern __shared__ float smem[];
  const int G = 1 << lg, li = threadIdx.x & (G - 1), ex = threadIdx.x >> lg;
  const int tile = blockDim.x >> lg, TE = T * E, h4 = H >> 2;
  float *sp = smem + ex * pstride;                       // p_te
  float *sc = smem + (tile + ex) * pstride;              // c_te, then dA_te
  const int64_t ntiles = (B + tile - 1) / tile;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t b = tl * tile + ex;
    const bool live = b < B;
    const float *zrow = Z + b * ldz, *dmrow = dM + b * lddm;
    float *dzrow = dZ + b * lddz;
    bool on[C];
    float4 z[C], dm[T][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      on[c] = live && (li + 64 * c) < h4;
      z[c] = on[c] ? ld4(zrow + 4 * (li + 64 * c)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int c = 0; c < C; ++c)
        dm[t][c] = on[c] ? ld4(dmrow + (t * H + 4 * (li + 64 * c)))
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    stage_logits(A, lda, b, live, li, G, TE, sp);
    __syncthreads();
    softmax_tasks(live, li, G, E, T, sp);
    __syncthreads();
    #pragma nounroll
    for (int e = 0; e < E; ++e) {
      float4 zn[C];
#pragma unroll
      for (int c = 0; c < C; ++c)
        zn[c] = (on[c] && e + 1 < E) ? ld4(zrow + (e + 1) * H + 4 * (li + 64 * c)) : z[c];
      float4 dz[C];
#pragma unroll
      for (int c = 0; c < C; ++c) dz[c] = make_float4(0.f, 0.f, 0.f, 0.f);
      float dot[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        dot[t] = 0.f;
        const float p = live ? sp[t * E + e] : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          fma4(dz[c], p, dm[t][c]);
          dot[t] = dot4(dm[t][c], z[c], dot[t]);
        }
      }
      // c_te: the lanes' partial dot products summed over the group (a butterfly: every lane gets the total)
      #pragma nounroll
      for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
        for (int t = 0; t < T; ++t) dot[t] += __shfl_xor(dot[t], o, 64);
      }
      if (live && li == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) sc[t * E + e] = dot[t];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (on[c]) st4(dzrow + (e * H + 4 * (li + 64 * c)), dz[c]);
        z[c] = zn[c];
      }
    }
    __syncthreads();
    // one lane per task: dA_te = p_te (c_te - sum_e' p_te' c_te'), in place over c
    if (live)
      #pragma nounroll
      for (int t = li; t < T; t += G) {
        const float *p = sp + t * E;
        float *c = sc + t * E;
        float s = 0.f;
        #pragma nounroll
        for (int e = 0; e < E; ++e) s = fmaf(p[e], c[e], s);
        #pragma nounroll
        for (int e = 0; e < E; ++e) c[e] = p[e] * (c[e] - s);
      }
    __syncthreads();
    if (live)
      #pragma nounroll
      for (int q = li; q < TE; q += G) dA[b * ldda + q] = sc[q];
  }
}

int mix_check(const char *fn, int E, int T, int H, int64_t B) {
  RM_REQUIRE(rm_mmoe_mix_supported(E, T, H),
             "%s: E=%d, T=%d, H=%d unsupported (1 <= E <= 16 experts, 1 <= T <= 8 tasks, H a multiple of 4 in "
             "4..512, row strides multiples of 4 floats)", fn, E, T, H);
  RM_REQUIRE(B >= 0 && B < ((int64_t)1 << 40), "%s: bad B=%lld", fn, (long long)B);
  return RM_OK;
}

// a [B, width] operand: 16-byte aligned rows (pointer and stride), stride >= width
int mix_operand(const char *fn, const char *name, const void *p, int64_t ld, int width) {
  RM_REQUIRE(p != nullptr, "%s: %s is NULL", fn, name);
  RM_REQUIRE(ld >= width, "%s: row stride of %s = %lld < its %d columns", fn, name, (long long)ld, width);
  RM_REQUIRE(ld % 4 == 0 && rm_aligned16(p) && ld <= kRmMaxStride,
             "%s: %s must be 16-byte aligned with a row stride that is a multiple of 4 floats (got stride %lld; "
             "limits: 1 <= E <= 16, 1 <= T <= 8, H a multiple of 4 in 4..512, row strides multiples of 4 floats)",
             fn, name, (long long)ld);
  return RM_OK;
}

#define MIX_CASE(KERNEL, t, chunks, ...)                       \
  case t:                                                      \
    if ((chunks) == 1) rm_launch_lds(KERNEL<t, 1>, __VA_ARGS__);      \
    else rm_launch_lds(KERNEL<t, 2>, __VA_ARGS__);                 \
    break;
#define MIX_DISPATCH(KERNEL, T, chunks, ...)     \
  switch (T) {                                   \
    MIX_CASE(KERNEL, 1, chunks, __VA_ARGS__)     \
    MIX_CASE(KERNEL, 2, chunks, __VA_ARGS__)     \
    MIX_CASE(KERNEL, 3, chunks, __VA_ARGS__)     \
    MIX_CASE(KERNEL, 4, chunks, __VA_ARGS__)     \
    MIX_CASE(KERNEL, 5, chunks, __VA_ARGS__)     \
    MIX_CASE(KERNEL, 6, chunks, __VA_ARGS__)     \
    MIX_CASE(KERNEL, 7, chunks, __VA_ARGS__)     \
    default:                                     \
      MIX_CASE(KERNEL, 8, chunks, __VA_ARGS__)   \
  }

// ------------------------------------------------------------------------------------------------ the loss head
constexpr int kLossBlock = 256;
constexpr int kLossBlocks = 256;  // per task

struct LossTasks {
  int type[kMaxT];
  float w[kMaxT];
};

static int loss_blocks(int64_t B) { return rm_grid_cap((B + kLossBlock - 1) / kLossBlock, kLossBlocks); }

// stage 1, grid (nblk, T): pred, and per block the observed count and the loss sum of its examples, in double
__global__ __launch_bounds__(kLossBlock) void mt_loss_partial_kernel(const float *__restrict__ logit,
                                                                     const float *__restrict__ Y, LossTasks tasks,
                                                                     int64_t B, int T, float *__restrict__ pred,
                                                                     double *__restrict__ part) {
  __shared__ double sm[2 * kLossBlock / 64];
  const int t = blockIdx.y, type = tasks.type[t];
  double sum = 0.0, cnt = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
    const float z = logit[(int64_t)t * B + i];
    const float y = Y ? Y[i * T + t] : 0.f;
    const bool seen = Y && y == y;
    float p, dz;
    const float l = rm_loss_point(z, seen ? y : 0.f, type, &p, &dz);
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

// stage 3, grid (nblk, T): dlogit = dl/dlogit * w_t * grad_scale / n_t where the label is observed, +0.0 elsewhere
__global__ __launch_bounds__(kLossBlock) void mt_loss_grad_kernel(const float *__restrict__ logit,
                                                                  const float *__restrict__ Y, LossTasks tasks,
                                                                  int64_t B, int T, const float *__restrict__ scale,
                                                                  float *__restrict__ dlogit) {
  const int t = blockIdx.y, type = tasks.type[t];
  const float sc = scale[t];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += stride) {
    const float y = Y[i * T + t];
    float p, dz = 0.f;
    if (y == y) {
      (void)rm_loss_point(logit[(int64_t)t * B + i], y, type, &p, &dz);
      dz *= sc;
    }
    dlogit[(int64_t)t * B + i] = dz;
  }
}

}  // namespace

extern "C" int rm_mmoe_mix_supported(int E, int T, int H) {
  return E >= 1 && E <= kMaxE && T >= 1 && T <= kMaxT && H >= 4 && H <= kMaxH && H % 4 == 0;
}

extern "C" int rm_mmoe_mix_tile(int E, int T, int H, int backward, int which) {
  if (!rm_mmoe_mix_supported(E, T, H)) return -1;
  return which == RM_MMOE_CAP ? kMixBlocks : mix_geom(E, T, H, backward != 0).tile;
}

extern "C" int rm_mmoe_mix_fwd(const float *Z, int64_t ldz, const float *A, int64_t lda, int64_t B, int E, int T,
                               int H, float *M, int64_t ldm, float *P, int64_t ldp, rm_stream_t stream) {
  const char *fn = "rm_mmoe_mix_fwd";
  if (int rc = mix_check(fn, E, T, H, B)) return rc;
  if (B == 0) return RM_OK;
  if (int rc = mix_operand(fn, "Z", Z, ldz, E * H)) return rc;
  if (int rc = mix_operand(fn, "A", A, lda, T * E)) return rc;
  if (int rc = mix_operand(fn, "M", M, ldm, T * H)) return rc;
  if (P != nullptr)
    if (int rc = mix_operand(fn, "P", P, ldp, T * E)) return rc;
  const MixGeom g = mix_geom(E, T, H, false);
  const int64_t ntiles = (B + g.tile - 1) / g.tile;
  MIX_DISPATCH(mmoe_mix_fwd_kernel, T, g.chunks, dim3(rm_grid_cap(ntiles, kMixBlocks)), dim3(g.waves * 64), g.lds,
               (hipStream_t)stream, Z, ldz, A, lda, B, E, H, M, ldm, P, ldp, g.lg, g.pstride);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int rm_mmoe_mix_bwd(const float *Z, int64_t ldz, const float *A, int64_t lda, const float *dM,
                               int64_t lddm, int64_t B, int E, int T, int H, float *dZ, int64_t lddz, float *dA,
                               int64_t ldda, rm_stream_t stream) {
  const char *fn = "rm_mmoe_mix_bwd";
  if (int rc = mix_check(fn, E, T, H, B)) return rc;
  if (B == 0) return RM_OK;
  if (int rc = mix_operand(fn, "Z", Z, ldz, E * H)) return rc;
  if (int rc = mix_operand(fn, "A", A, lda, T * E)) return rc;
  if (int rc = mix_operand(fn, "dM", dM, lddm, T * H)) return rc;
  if (int rc = mix_operand(fn, "dZ", dZ, lddz, E * H)) return rc;
  if (int rc = mix_operand(fn, "dA", dA, ldda, T * E)) return rc;
  const MixGeom g = mix_geom(E, T, H, true);
  const int64_t ntiles = (B + g.tile - 1) / g.tile;
  MIX_DISPATCH(mmoe_mix_bwd_kernel, T, g.chunks, dim3(rm_grid_cap(ntiles, kMixBlocks)), dim3(g.waves * 64), g.lds,
               (hipStream_t)stream, Z, ldz, A, lda, dM, lddm, B, E, H, dZ, lddz, dA, ldda, g.lg, g.pstride);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

// floats: the per-block (sum, count) pairs in double, then T gradient scales
extern "C" int64_t rm_multitask_loss_workspace(int64_t B, int T) {
  if (B < 1 || T < 1 || T > kMaxT) return -1;
  return 4 * (int64_t)T * loss_blocks(B) + 2 * kMaxT;
}

extern "C" int rm_multitask_loss(const float *logit, const float *Y, const int *task_type, const float *task_weight,
                                 float grad_scale, int64_t B, int T, float *pred, float *dlogit, int64_t *n_t,
                                 float *loss_t, float *loss, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_multitask_loss";
  RM_REQUIRE(B > 0, "%s: B must be > 0 (got %lld)", fn, (long long)B);
  RM_REQUIRE(T >= 1 && T <= kMaxT, "%s: T=%d tasks unsupported (1 <= T <= 8)", fn, T);
  RM_REQUIRE(logit && pred && task_type, "%s: NULL argument", fn);
  const bool train = dlogit || n_t || loss_t || loss;
  RM_REQUIRE(!train || (Y && task_weight && workspace && rm_aligned16(workspace)),
             "%s: labels, task weights and a 16-byte aligned workspace are needed for the loss and its gradient", fn);
  LossTasks tasks;
  for (int t = 0; t < kMaxT; ++t) {
    tasks.type[t] = t < T ? task_type[t] : 0;
    tasks.w[t] = (t < T && task_weight) ? task_weight[t] : 0.f;
    RM_REQUIRE(tasks.type[t] == 0 || tasks.type[t] == 1, "%s: task type must be 0 (classification) or 1", fn);
  }
  const int nblk = loss_blocks(B);
  hipStream_t st = (hipStream_t)stream;
  double *part = train ? reinterpret_cast<double *>(workspace) : nullptr;
  float *scale = train ? workspace + 4 * (int64_t)T * nblk : nullptr;
  hipLaunchKernelGGL(mt_loss_partial_kernel, dim3(nblk, T), dim3(kLossBlock), 0, st, logit, train ? Y : nullptr,
                     tasks, B, T, pred, part);
  if (train) {
    hipLaunchKernelGGL(mt_loss_finish_kernel, dim3(1), dim3(64), 0, st, part, nblk, tasks, T, grad_scale, n_t, loss_t,
                       loss, scale);
    if (dlogit)
      hipLaunchKernelGGL(mt_loss_grad_kernel, dim3(nblk, T), dim3(kLossBlock), 0, st, logit, Y, tasks, B, T, scale,
                         dlogit);
  }
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
