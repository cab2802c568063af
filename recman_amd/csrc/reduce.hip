// The fixed-order sum of per-block partial gradients (gfx950): the second stage of every model backward whose
// blocks (or batch slices) each write one full set of N partial sums, [nsets][N], into the workspace.
//
// Determinism: element o is summed by one thread, over the sets in ascending order, in one float accumulator
// that starts at +0.0f - no float atomics, so two runs are bit-equal, and neither the block size nor the grid
// enters the arithmetic.  Callers: rm_afm_bwd, rm_autoint_head_bwd (over its kSeg segments), rm_cross_mix_bwd,
// rm_fibinet_bwd, rm_fmfm_bwd, rm_pnn_bwd, rm_bst_bwd (five sets: its 17 destinations).
//
// Second stages that are NOT this kernel, on purpose:
//  - autoint_seg_kernel / autoint_finish_kernel (autoint.hip): a segmented first stage (sets split into kSeg
//    runs) and a destination layout interleaved by column block.
//  - masknet_finish_kernel (masknet.hip): float64 accumulator, sums a slice of the sets per thread.
//  - asp_finish_kernel (asp.hip): float64 accumulator, partials in a padded layout.
//  - the reduce kernels of mlp.hip, gemm*.hip, cin*.hip, loss.hip and embed.hip: tuned with their producers,
//    with other summation orders.
#include "rm_launch.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void rm_sum_partials_kernel(const float *__restrict__ part, int nsets, int N,
                                                                   RmSumDsts d) {
  const int o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= N) return;
  float s = 0.f;
  for (int b = 0; b < nsets; ++b) s += part[(int64_t)b * N + o];
  if (o < d.end[0]) d.p[0][o] = s;
  else if (o < d.end[1]) d.p[1][o - d.end[0]] = s;
  else if (o < d.end[2]) d.p[2][o - d.end[1]] = s;
  else d.p[3][o - d.end[2]] = s;
}

}  // namespace

void rm_sum_partials(const float *part, int nsets, int N, RmSumDsts dsts, hipStream_t st) {
  hipLaunchKernelGGL(rm_sum_partials_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, st, part, nsets,
                     N, dsts);
}
