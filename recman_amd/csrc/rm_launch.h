// Host-side launch scaffolding shared by the model kernel files (afm, autoint, dot_interact, cross_mix, fibinet,
// fmfm, pnn, masknet, asp, bst, dien), the argument checks the three sequence pooling units (asp, bst, dien) share,
// and the one fixed-order sum of per-block partials (reduce.hip).
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

// The sequence pooling units (asp, bst, dien) begin their entry points with the same arguments - rows, LD, D, row0,
// offsets, ids, qrow, B, nnz - and check them here, after the file's own shape check.
// The sizes: the kernels narrow the example index to int and index the table's rows with LD.
inline int rm_seq_check_sizes(const char *fn, int D, int64_t B, int64_t nnz, int64_t LD) {
  RM_REQUIRE(B >= 0 && B < ((int64_t)1 << 31) && nnz >= 0, "%s: bad sizes", fn);
  RM_REQUIRE_STRIDE(fn, "LD", LD, D, "D");
  return RM_OK;
}

// The pointers of a forward over B > 0 examples (B == 0 returns before it reads any).
inline int rm_seq_check_fwd(const char *fn, const float *rows, const int64_t *offsets, const int64_t *ids,
                            const int64_t *qrow, int64_t nnz, const float *out, const float *workspace) {
  RM_REQUIRE(rows && offsets && qrow && out && workspace && (nnz == 0 || ids), "%s: NULL argument", fn);
  return RM_OK;
}

// The pointers of a backward (the workspace always: the parameter gradients of an empty batch are summed from it)
// and the row strides of its two [B, D] gradient views.
inline int rm_seq_check_bwd(const char *fn, int D, const float *rows, const int64_t *offsets, const int64_t *ids,
                            const int64_t *qrow, int64_t B, int64_t nnz, const float *d_out, int64_t do_stride,
                            const float *d_keys, const float *d_query, int64_t dq_stride, const float *workspace) {
  RM_REQUIRE_PTR(fn, workspace);
  RM_REQUIRE(B == 0 || (rows && offsets && qrow && d_out && d_query), "%s: NULL argument", fn);
  RM_REQUIRE(nnz == 0 || (ids && d_keys), "%s: NULL argument", fn);
  if (B > 0) {
    RM_REQUIRE_STRIDE(fn, "do_stride", do_stride, D, "D");
    RM_REQUIRE_STRIDE(fn, "dq_stride", dq_stride, D, "D");
  }
  return RM_OK;
}

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
