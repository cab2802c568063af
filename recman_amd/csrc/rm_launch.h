// Host-side launch scaffolding shared by the model kernel files (afm, autoint, dot_interact, cross_mix, fibinet,
// fmfm, pnn, masknet, asp, bst) and the one fixed-order sum of per-block partials (reduce.hip).
#pragma once
#include "rm_common.h"

// a required pointer argument of the entry point `fn`
#define RM_REQUIRE_PTR(fn, p) RM_REQUIRE(p, "%s: " #p " is NULL", fn)

// Row strides reach the kernels' int offsets: at most 2^24 floats.
constexpr int64_t kRmMaxStride = 1 << 24;

// The row stride `ld` (argument `name`) of rows of `width` floats; `what` spells the width in the message.
#define RM_REQUIRE_STRIDE(fn, name, ld, width, what)                                                     \
  do {                                                                                                   \
    RM_REQUIRE((ld) >= (width), "%s: %s=%lld < " what " = %d", fn, name, (long long)(ld), (int)(width)); \
    RM_REQUIRE((ld) <= kRmMaxStride, "%s: %s=%lld too large", fn, name, (long long)(ld));                \
  } while (0)

// Launches a kernel that needs `smem` bytes of dynamic LDS: the limit is raised on every launch (a set attribute,
// no allocation), then the kernel goes out.  The caller checks the launch (RM_CHECK_LAUNCH).
template <typename K, typename... Args>
inline void rm_launch_lds(K kernel, dim3 grid, dim3 block, size_t smem, hipStream_t st, Args... args) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)smem);
  hipLaunchKernelGGL(kernel, grid, block, smem, st, args...);
}

// +0.0f into `floats` floats at p on the stream: the parameter gradients of an empty batch (`what` names them).
inline int rm_clear_async(const char *fn, const char *what, float *p, int64_t floats, hipStream_t st) {
  if (hipMemsetAsync(p, 0, (size_t)floats * sizeof(float), st) == hipSuccess) return RM_OK;
  rm_set_error("%s: clearing %s failed", fn, what);
  return RM_ELAUNCH;
}

// Up to four destination arrays that split [0, N): array k owns [end[k-1], end[k]) (end[-1] = 0).
struct RmSumDsts {
  float *p[4];
  int end[4];
};
inline RmSumDsts rm_sum_dsts(float *a, int na, float *b = nullptr, int nb = 0, float *c = nullptr, int nc = 0,
                             float *d = nullptr, int nd = 0) {
  return RmSumDsts{{a, b, c, d}, {na, na + nb, na + nb + nc, na + nb + nc + nd}};
}

// dst[o] = the sum of part[b * N + o] over b = 0 .. nsets-1, in that order, from +0.0f (nsets == 0: all +0.0f),
// for every o < N = dsts.end[3] (reduce.hip).  The caller checks the launch.
void rm_sum_partials(const float *part, int nsets, int N, RmSumDsts dsts, hipStream_t st);
