// Interest-evolution pooling of behaviour sequences - SequenceFeat + a GRU, an attention and an attention-gated GRU
// (AUGRU) over the history (Deep Interest Evolution Network, arXiv 1809.03672; hidden size = D, no auxiliary loss).
// Nothing in the reference implements it.  Per example b with query row q (columns 0..D-1 of the candidate item's
// table row) and history rows k_1..k_n of the SAME table block (CSR, oldest first), matrices [in, out], the column
// blocks of a [D, 3D] matrix [u | r | c]:
//     cell(x, h; W, U, b, a):  u = sigmoid(x Wu + h Uu + bu),  r = sigmoid(x Wr + h Ur + br),
//                              c = tanh(x Wc + r * (h Uc) + bc),  u = a u,  return (1 - u) h + u c
//     h_0 = 0,  h_t = cell(k_t, h_{t-1}; gru_*, 1)                        the interest extractor
//     s_t = h_t . (att_w q),  a = softmax_t(s)  (max-subtracted, over the example's own n positions)
//     g_0 = 0,  g_t = cell(h_t, g_{t-1}; augru_*, a_t)                    the interest evolution
//     out_b = g_n                                                         (n = 0: out_b = 0, no gradient)
// rm_dien_fwd writes out_b into a fused scratch row (columns 0..D-1, zeros behind) that the gather kernel reads like
// any table row.
//
// Mapping.  D consecutive lanes own one example, lane j its column j of every D-vector; a 256-thread block holds
// 256 / D examples and grid-strides over the batch (a FIXED assignment: example b belongs to group b mod the number
// of groups).  The four [D, 3D] matrices (row stride 3D + 1: odd, so the column walk of the forward products and the
// row walk of the transposed products of the backward are both conflict-free), the two biases and att_w (row stride
// D + 1) are copied into LDS once per block: 53.4 KiB at D = 32.  A product reads its weight from LDS and its vector
// element from the owning lane by a shuffle inside the group; the state never leaves registers.  Every loop over time
// runs to the example's OWN length (clamped to max_len), so padding is never processed and lanes of a shorter example
// just wait; there is no block barrier after the weights are staged.  The products run on the vector ALU: the matrix
// pipe is NOT used (profiles/dien.md says what v_mfma_f32_16x16x4_f32 with 16 examples on N would save).
//   forward : dien_fwd_kernel.  Pass 1: the extractor IN FLOAT64 (see dien_gates64); h_t rounded -> workspace, s_t
//             from the unrounded state -> the group's LDS slab (max_len doubles), its running maximum.  Pass 2: the
//             softmax denominator.  Pass 3: the AUGRU in float32 on the rounded h_t; a_t and, with save, g_t ->
//             workspace.  `out` does not depend on save.
//   backward: dien_bwd_kernel walks time backwards twice per example (AUGRU, then the extractor with the softmax's
//             share folded in), recomputing the gates of a step from the saved states.  It writes d_keys, adds the
//             query gradient, and leaves the pre-activation gradients of every position [nnz, 4, D] per GRU and
//             d(att_w q) [B, D] in the workspace; dien_wgrad_kernel / dien_attw_kernel then form the weight
//             gradients as products with the positions (examples) on K: a block owns a fixed chunk of examples, a
//             thread fixed elements, the block's sums are one partial set, and rm_sum_partials adds the sets in block
//             order.
// No float atomics anywhere, every sum in a fixed order: two runs are bit-equal.
#include <math.h>

#include "rm_launch.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLen = 256;
constexpr int kSeqBlocks = 1024;   // four blocks per CU: two resident at D = 32, more below
constexpr int kWgBlocks = 512;     // blocks of the weight-gradient kernels at most
constexpr int kWgTile = 32;        // positions per LDS tile
constexpr int kWgMinChunk = 16;    // examples per block at least
constexpr int kAttBlocks = 256;
constexpr int kAttTile = 64;       // examples per LDS tile (and per block at least)

inline int64_t rup4(int64_t v) { return (v + 3) / 4 * 4; }

inline bool dien_shape_ok(int D, int ML) { return (D == 8 || D == 16 || D == 32) && ML >= 1 && ML <= kMaxLen; }

// floats of one partial set of a GRU: dW [D, 3D], dU [D, 3D], db [3D] (a multiple of 4 at every D)
inline int dien_gru_floats(int D) { return 6 * D * D + 3 * D; }
inline int dien_seq_blocks(int64_t B, int D) { return rm_grid_cap((B + kThreads / D - 1) / (kThreads / D), kSeqBlocks); }
inline int dien_wg_blocks(int64_t B) { return rm_grid_cap((B + kWgMinChunk - 1) / kWgMinChunk, kWgBlocks); }
inline int dien_att_blocks(int64_t B) { return rm_grid_cap((B + kAttTile - 1) / kAttTile, kAttBlocks); }

// The workspace (offsets in floats, every region a multiple of 4): h_t [nnz, D] and a_t [nnz] (every forward);
// g_t [nnz, D] (save); the pre-activation gradients of the extractor and of the AUGRU [nnz, 4, D] each, the
// positions' flags [nnz] (int: 0 unused, 1 first step of its example, 2 later step), d(att_w q) [B, D] and the
// partial sets (backward).
struct DienWs {
  int64_t h, a, g, ga, gb, flag, dp, part_gru, part_augru, part_att, fwd_total, total;
};
inline DienWs dien_ws(int D, int64_t B, int64_t nnz) {
  DienWs w;
  w.h = 0;
  w.a = w.h + rup4(nnz * D);
  w.fwd_total = w.a + rup4(nnz) + 4;
  w.g = w.fwd_total;
  w.ga = w.g + rup4(nnz * D);
  w.gb = w.ga + nnz * 4 * D;
  w.flag = w.gb + nnz * 4 * D;
  w.dp = w.flag + rup4(nnz);
  w.part_gru = w.dp + rup4(B * D);
  w.part_augru = w.part_gru + (int64_t)dien_wg_blocks(B) * dien_gru_floats(D);
  w.part_att = w.part_augru + (int64_t)dien_wg_blocks(B) * dien_gru_floats(D);
  w.total = w.part_att + (int64_t)dien_att_blocks(B) * D * D;
  return w;
}

template <int D>
struct DienLds {
  static constexpr int S = 3 * D + 1, SA = D + 1;
  static constexpr int W1 = 0, U1 = D * S, W2 = 2 * D * S, U2 = 3 * D * S, B1 = 4 * D * S, B2 = B1 + 3 * D,
                       AW = B2 + 3 * D, N = AW + D * SA;
  static constexpr int SC = (N + 1) / 2 * 2;  // the forward's scores (doubles) start here, 8-byte aligned
};

struct DienIn {
  const float *rows;
  int64_t LD, row0;
  const int64_t *offsets, *ids, *qrow;
  int64_t B, nnz;
  int ML;
};

// the seven parameters -> LDS; ends on a barrier
template <int D>
__device__ __forceinline__ void dien_stage(float *sm, const rm_dien_params &p) {
  using L = DienLds<D>;
  for (int e = threadIdx.x; e < 3 * D * D; e += kThreads) {
    const int r = e / (3 * D), c = e - r * (3 * D), o = r * L::S + c;
    sm[L::W1 + o] = p.gru_w[e];
    sm[L::U1 + o] = p.gru_u[e];
    sm[L::W2 + o] = p.augru_w[e];
    sm[L::U2 + o] = p.augru_u[e];
  }
  for (int e = threadIdx.x; e < 3 * D; e += kThreads) {
    sm[L::B1 + e] = p.gru_b[e];
    sm[L::B2 + e] = p.augru_b[e];
  }
  for (int e = threadIdx.x; e < D * D; e += kThreads) {
    const int r = e / D, c = e - r * D;
    sm[L::AW + r * L::SA + c] = p.att_w[e];
  }
  __syncthreads();
}

// The example's positions [o0, o0 + n): its CSR span cut to the array and to its LAST max_len items (what
// th.SequenceFeat keeps); n <= max_len whatever `offsets` holds.
__device__ __forceinline__ void dien_span(const DienIn &in, int64_t b, int64_t *o0, int *n) {
  long long s = in.offsets[b], e = in.offsets[b + 1];
  s = s < 0 ? 0 : (s > in.nnz ? in.nnz : s);
  e = e < s ? s : (e > in.nnz ? in.nnz : e);
  if (e - s > in.ML) s = e - in.ML;
  *o0 = s;
  *n = (int)(e - s);
}

// Finite and correct at both ends: exp -> inf gives 0 or 1; t = expm1(-2 |x|) lies in [-1, 0], so -t / (t + 2) is
// |tanh x| without overflow - and without the cancellation of 1 - 2 / (e^2x + 1) near 0, whose absolute error of one
// ulp of 1 in h_t the score h_t . (att_w q) multiplies by |att_w q|.
__device__ __forceinline__ float dien_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float dien_tanh(float x) {
  const float t = expm1f(-2.0f * fabsf(x));
  return copysignf(-t / (t + 2.0f), x);
}

// The weights do not change from one time step to the next, so the compiler would hoist every LDS read of a step out
// of the time loop into registers (hundreds of them: it spilled).  The lane's column goes through an empty asm in
// every step instead: the reads stay in the loop.
#define RM_DIEN_OPAQUE(v_) asm volatile("" : "+v"(v_))

// The gates of one step for column j: u0 (before the attention weight), r, c and hc = (h Uc)_j.
template <int D>
__device__ __forceinline__ void dien_gates(const float *W, const float *U, const float *bias, int j, float x, float h,
                                           float *u0, float *r, float *c, float *hc) {
  constexpr int S = DienLds<D>::S;
  RM_DIEN_OPAQUE(j);
  float pu = bias[j], pr = bias[D + j], pc = bias[2 * D + j], ph = 0.f;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float xk = __shfl(x, k, D), hk = __shfl(h, k, D);
    const float *w = W + k * S + j, *u = U + k * S + j;
    pu = fmaf(xk, w[0], pu);
    pr = fmaf(xk, w[D], pr);
    pc = fmaf(xk, w[2 * D], pc);
    pu = fmaf(hk, u[0], pu);
    pr = fmaf(hk, u[D], pr);
    ph = fmaf(hk, u[2 * D], ph);
  }
  *u0 = dien_sigmoid(pu);
  *r = dien_sigmoid(pr);
  *c = dien_tanh(fmaf(*r, ph, pc));
  *hc = ph;
}

// The transposed products of one step for row j: dx_j = sum_k W[j, k] dP_k and dh_j = sum_k U[j, k] dP'_k, where dP =
// [dpu | dpr | dpc] and dP' = [dpu | dpr | dhc].
template <int D>
__device__ __forceinline__ void dien_back(const float *W, const float *U, int j, float dpu, float dpr, float dpc,
                                          float dhc, float *dx, float *dh) {
  constexpr int S = DienLds<D>::S;
  RM_DIEN_OPAQUE(j);
  const float *w = W + j * S, *u = U + j * S;
  float sx = 0.f, sh = 0.f;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float a = __shfl(dpu, k, D), b = __shfl(dpr, k, D), c = __shfl(dpc, k, D), d = __shfl(dhc, k, D);
    sx = fmaf(w[k], a, sx);
    sx = fmaf(w[D + k], b, sx);
    sx = fmaf(w[2 * D + k], c, sx);
    sh = fmaf(u[k], a, sh);
    sh = fmaf(u[D + k], b, sh);
    sh = fmaf(u[2 * D + k], d, sh);
  }
  *dx = sx;
  *dh = sh;
}

// sum_j a_j b_j over the example's lanes, the same bits in every lane and at every call site: the product is rounded
// on its own (contracted into the first add of the butterfly, the two partners of a pair would get different sums)
template <int D>
__device__ __forceinline__ float dien_dot(float a, float b) {
  float v;
  {
#pragma clang fp contract(off)
    v = a * b;
  }
  return rm_group_sum<D>(v);
}

// The score path of the forward - the extractor's recurrence and s_t = h_t . (att_w q) - runs in float64.  With a
// large att_w, |att_w q| reaches 1e3 .. 1e4 and a score as much: an ABSOLUTE error e of the score is the RELATIVE
// error e of the softmax weight of every position near the maximum, and of every gradient that passes the softmax.
// One ulp of a float32 score is 1e-4 .. 1e-3 there, and so is |att_w q| times the few ulps that a float32 recurrence
// leaves in h_t - or even the one rounding of a stored h_t.  So the state is carried, and the score taken from it,
// unrounded; nothing downstream of the softmax weight multiplies an error like that, and the AUGRU and the whole
// backward stay in float32 on the rounded h_t.
__device__ __forceinline__ double dien_sigmoid64(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ double dien_tanh64(double x) {
  const double t = expm1(-2.0 * fabs(x));
  return copysign(-t / (t + 2.0), x);
}
// dien_gates for the forward's extractor: the same sums, float64 state in, float64 gates out
template <int D>
__device__ __forceinline__ void dien_gates64(const float *W, const float *U, const float *bias, int j, float x,
                                             double h, double *u0, double *r, double *c) {
  constexpr int S = DienLds<D>::S;
  RM_DIEN_OPAQUE(j);
  double pu = bias[j], pr = bias[D + j], pc = bias[2 * D + j], ph = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double xk = __shfl(x, k, D), hk = __shfl(h, k, D);
    const float *w = W + k * S + j, *u = U + k * S + j;
    pu = fma(xk, (double)w[0], pu);
    pr = fma(xk, (double)w[D], pr);
    pc = fma(xk, (double)w[2 * D], pc);
    pu = fma(hk, (double)u[0], pu);
    pr = fma(hk, (double)u[D], pr);
    ph = fma(hk, (double)u[2 * D], ph);
  }
  *u0 = dien_sigmoid64(pu);
  *r = dien_sigmoid64(pr);
  *c = dien_tanh64(fma(*r, ph, pc));
}
// p_j = (att_w q)_j
template <int D>
__device__ __forceinline__ double dien_attq(const float *AW, int j, float q) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) s = fma((double)AW[j * (D + 1) + k], (double)__shfl(q, k, D), s);
  return s;
}
// s = sum_j h_j p_j over the example's lanes (the same bits in every lane)
template <int D>
__device__ __forceinline__ double dien_score(double h, double p) {
  double v;
  {
#pragma clang fp contract(off)
    v = h * p;
  }
#pragma unroll
  for (int o = D / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ forward
template <int D>
__global__ __launch_bounds__(kThreads) void dien_fwd_kernel(DienIn in, rm_dien_params p, int save, float *out,
                                                            float *hws, float *aws, float *gws) {
  using L = DienLds<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  dien_stage<D>(sm, p);
  constexpr int kEx = kThreads / D;
  const int j = threadIdx.x & (D - 1), grp = threadIdx.x / D;
  // the group's scores, position t < n <= max_len.  Every lane of the group holds the same bits of s_t and writes
  // them, so a lane reads back what it wrote itself (the LDS serves a wave in order; a group lies inside one wave).
  double *sc = reinterpret_cast<double *>(sm + L::SC) + (size_t)grp * in.ML;
  for (int64_t b = (int64_t)blockIdx.x * kEx + grp; b < in.B; b += (int64_t)gridDim.x * kEx) {
    int64_t o0;
    int n;
    dien_span(in, b, &o0, &n);
    float g = 0.f;
    if (n > 0) {
      const double pj = dien_attq<D>(sm + L::AW, j, in.rows[in.qrow[b] * in.LD + j]);
      double h = 0.0, m = -INFINITY;
      float xn = in.rows[(in.row0 + in.ids[o0]) * in.LD + j];
      for (int t = 0; t < n; ++t) {
        const float x = xn;
        if (t + 1 < n) xn = in.rows[(in.row0 + in.ids[o0 + t + 1]) * in.LD + j];
        double u, r, c;
        dien_gates64<D>(sm + L::W1, sm + L::U1, sm + L::B1, j, x, h, &u, &r, &c);
        h = (1.0 - u) * h + u * c;
        hws[(o0 + t) * D + j] = (float)h;
        const double s = dien_score<D>(h, pj);
        sc[t] = s;
        m = fmax(m, s);
      }
      float den = 0.f;
      for (int t = 0; t < n; ++t) den += expf((float)(sc[t] - m));
      for (int t = 0; t < n; ++t) {
        const float x = hws[(o0 + t) * D + j];
        const float a = expf((float)(sc[t] - m)) / den;
        float u, r, c, hc;
        dien_gates<D>(sm + L::W2, sm + L::U2, sm + L::B2, j, x, g, &u, &r, &c, &hc);
        u *= a;
        g = (1.0f - u) * g + u * c;
        if (save) gws[(o0 + t) * D + j] = g;
        if (j == 0) aws[o0 + t] = a;
      }
    }
    float *o = out + b * in.LD;
    o[j] = g;
    for (int c = D + j; c < in.LD; c += D) o[c] = 0.f;
  }
}

// ----------------------------------------------------------------------------------------------- backward
struct DienBwd {
  const float *d_out;
  int64_t do_stride;
  float *d_keys, *d_query;
  int64_t dq_stride;
  const float *hws, *aws, *gws;
  float *ga, *gb, *dp;  // the extractor's and the AUGRU's pre-activation gradients, d(att_w q)
  int *flag;
};

template <int D>
__global__ __launch_bounds__(kThreads) void dien_bwd_kernel(DienIn in, rm_dien_params p, DienBwd o) {
  using L = DienLds<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  dien_stage<D>(sm, p);
  constexpr int kEx = kThreads / D;
  const int j = threadIdx.x & (D - 1), grp = threadIdx.x / D;
  for (int64_t b = (int64_t)blockIdx.x * kEx + grp; b < in.B; b += (int64_t)gridDim.x * kEx) {
    int64_t o0;
    int n;
    dien_span(in, b, &o0, &n);
    if (n == 0) {
      o.dp[b * D + j] = 0.f;
      continue;
    }
    const float pj = (float)dien_attq<D>(sm + L::AW, j, in.rows[in.qrow[b] * in.LD + j]);
    // the AUGRU, last step first.  dx_t and da_t are parked in the extractor's slots of the position (every lane its
    // own copy of da_t, read back by the same lane below); dot = sum_t a_t da_t
    float dg = o.d_out[b * o.do_stride + j], dot = 0.f;
    for (int t = n - 1; t >= 0; --t) {
      const int64_t pos = o0 + t;
      const float x = o.hws[pos * D + j], gp = t > 0 ? o.gws[(pos - 1) * D + j] : 0.f, a = o.aws[pos];
      float u0, r, c, hc;
      dien_gates<D>(sm + L::W2, sm + L::U2, sm + L::B2, j, x, gp, &u0, &r, &c, &hc);
      const float u = a * u0;
      const float du = dg * (c - gp), dpc = dg * u * (1.0f - c * c);
      const float da = dien_dot<D>(du, u0);
      const float dpu = du * a * u0 * (1.0f - u0), dpr = dpc * hc * r * (1.0f - r), dhc = dpc * r;
      float *G = o.gb + pos * 4 * D;
      G[j] = dpu; G[D + j] = dpr; G[2 * D + j] = dpc; G[3 * D + j] = dhc;
      float dx, dh;
      dien_back<D>(sm + L::W2, sm + L::U2, j, dpu, dpr, dpc, dhc, &dx, &dh);
      dot = fmaf(a, da, dot);
      o.ga[pos * 4 * D + j] = dx;
      o.ga[pos * 4 * D + D + j] = da;
      dg = fmaf(dg, 1.0f - u, dh);
    }
    // the extractor, last step first.  s_t = h_t . p under the softmax: ds_t = a_t (da_t - dot) (exactly zero with one
    // position, where a = 1), dh_t += ds_t p, dp = sum_t ds_t h_t
    float dhn = 0.f, dpj = 0.f;
    for (int t = n - 1; t >= 0; --t) {
      const int64_t pos = o0 + t;
      float *G = o.ga + pos * 4 * D;
      const float ds = o.aws[pos] * (G[D + j] - dot);
      const float dh = dhn + fmaf(ds, pj, G[j]);
      dpj = fmaf(ds, o.hws[pos * D + j], dpj);
      const float x = in.rows[(in.row0 + in.ids[pos]) * in.LD + j], hp = t > 0 ? o.hws[(pos - 1) * D + j] : 0.f;
      float u, r, c, hc;
      dien_gates<D>(sm + L::W1, sm + L::U1, sm + L::B1, j, x, hp, &u, &r, &c, &hc);
      const float du = dh * (c - hp), dpc = dh * u * (1.0f - c * c);
      const float dpu = du * u * (1.0f - u), dpr = dpc * hc * r * (1.0f - r), dhc = dpc * r;
      G[j] = dpu; G[D + j] = dpr; G[2 * D + j] = dpc; G[3 * D + j] = dhc;
      float dx, dhh;
      dien_back<D>(sm + L::W1, sm + L::U1, j, dpu, dpr, dpc, dhc, &dx, &dhh);
      o.d_keys[pos * D + j] = dx;
      if (j == 0) o.flag[pos] = t > 0 ? 2 : 1;
      dhn = fmaf(dh, 1.0f - u, dhh);
    }
    o.dp[b * D + j] = dpj;
    {
      float dq = 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) dq = fmaf(sm[L::AW + k * L::SA + j], __shfl(dpj, k, D), dq);
      o.d_query[b * o.dq_stride + j] += dq;
    }
  }
}

// One GRU's weight gradients over the positions of a fixed chunk of examples: dW = X^T dP, dU = Hprev^T dP', db = 1^T dP with
// dP = [dpu | dpr | dpc], dP' = [dpu | dpr | dhc] of G [nnz, 4, D].  X is hws (xsrc) or the gathered table rows
// (xsrc == nullptr); Hprev is prev[pos - 1] on a later step of an example (flag 2), zero on its first (flag 1);
// a position with flag 0 belongs to no example's used history and adds exact zeros.  Every element is ONE chain of
// multiply-adds over the block's positions in order, so neither the tile size nor unused positions between the
// examples change a bit of it.  part[block]: [dW | dU | db], element tid + 256 s in accumulator s.
template <int D>
__global__ __launch_bounds__(kThreads) void dien_wgrad_kernel(const float *__restrict__ xsrc, const float *__restrict__ rows,
                                                              int64_t LD, int64_t row0, const int64_t *__restrict__ ids,
                                                              const float *__restrict__ prev, const float *__restrict__ G,
                                                              const int *__restrict__ flag, int64_t nnz,
                                                              const int64_t *__restrict__ offsets, int64_t B,
                                                              int64_t chunk, float *__restrict__ part) {
  constexpr int SA = 2 * D + 1, SG = 4 * D, N = 6 * D * D + 3 * D, NS = (N + kThreads - 1) / kThreads;
  __shared__ float sA[kWgTile * SA], sG[kWgTile * SG];
  __shared__ int sF[kWgTile];
  const int tid = threadIdx.x;
  float acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.f;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
  long long p0 = b0 < b1 ? offsets[b0] : 0, p1 = b0 < b1 ? offsets[b1] : 0;
  p0 = p0 < 0 ? 0 : (p0 > nnz ? nnz : p0);
  p1 = p1 < p0 ? p0 : (p1 > nnz ? nnz : p1);
  for (int64_t t0 = p0; t0 < p1; t0 += kWgTile) {
    __syncthreads();  // the previous tile is used up
    if (tid < kWgTile) sF[tid] = t0 + tid < p1 ? flag[t0 + tid] : 0;
    __syncthreads();
    for (int e = tid; e < kWgTile * 2 * D; e += kThreads) {
      const int r = e / (2 * D), c = e - r * (2 * D), f = sF[r];
      const int64_t pos = t0 + r;
      float v = 0.f;
      if (c < D) {
        if (f == 1 || f == 2) v = xsrc ? xsrc[pos * D + c] : rows[(row0 + ids[pos]) * LD + c];
      } else if (f == 2) {
        v = prev[(pos - 1) * D + (c - D)];
      }
      sA[r * SA + c] = v;
    }
    if (tid < kWgTile) sA[tid * SA + 2 * D] = (sF[tid] == 1 || sF[tid] == 2) ? 1.f : 0.f;
    for (int e = tid; e < kWgTile * SG; e += kThreads) {
      const int f = sF[e / SG];
      sG[e] = (f == 1 || f == 2) ? G[t0 * SG + e] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int e = tid + kThreads * s;
      if (e < N) {
        int acol, gcol;
        if (e < 3 * D * D) {
          acol = e / (3 * D);
          gcol = e - acol * (3 * D);
        } else if (e < 6 * D * D) {
          const int e2 = e - 3 * D * D, i = e2 / (3 * D), c = e2 - i * (3 * D);
          acol = D + i;
          gcol = c < 2 * D ? c : c + D;
        } else {
          acol = 2 * D;
          gcol = e - 6 * D * D;
        }
        float t = acc[s];
#pragma unroll 8
        for (int r = 0; r < kWgTile; ++r) t = fmaf(sA[r * SA + acol], sG[r * SG + gcol], t);
        acc[s] = t;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int e = tid + kThreads * s;
    if (e < N) part[(int64_t)blockIdx.x * N + e] = acc[s];
  }
}

// d att_w [i, j] = sum_b dp[b, i] q[b, j] over a fixed chunk of examples; part[block]: [D, D]
template <int D>
__global__ __launch_bounds__(kThreads) void dien_attw_kernel(const float *__restrict__ dp, const float *__restrict__ rows,
                                                             int64_t LD, const int64_t *__restrict__ qrow, int64_t B,
                                                             int64_t chunk, float *__restrict__ part) {
  constexpr int SP = D + 1, N = D * D, NS = (N + kThreads - 1) / kThreads;
  __shared__ float sP[kAttTile * SP], sQ[kAttTile * D];
  const int tid = threadIdx.x;
  float acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.f;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
  for (int64_t t0 = b0; t0 < b1; t0 += kAttTile) {
    __syncthreads();
    for (int e = tid; e < kAttTile * D; e += kThreads) {
      const int r = e / D, c = e - r * D;
      const int64_t b = t0 + r;
      const bool on = b < b1;
      sP[r * SP + c] = on ? dp[b * D + c] : 0.f;
      sQ[r * D + c] = on ? rows[qrow[b] * LD + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int e = tid + kThreads * s;
      if (e < N) {
        const int i = e / D, c = e - i * D;
        float t = 0.f;
#pragma unroll 8
        for (int r = 0; r < kAttTile; ++r) t = fmaf(sP[r * SP + i], sQ[r * D + c], t);
        acc[s] += t;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int e = tid + kThreads * s;
    if (e < N) part[(int64_t)blockIdx.x * N + e] = acc[s];
  }
}

int dien_check(const char *fn, int D, int ML, int64_t B, int64_t nnz, int64_t LD) {
  RM_REQUIRE(dien_shape_ok(D, ML), "%s: unsupported shape D=%d max_len=%d (D in {8,16,32}, max_len 1..256)", fn, D, ML);
  RM_REQUIRE(nnz < ((int64_t)1 << 40), "%s: bad sizes", fn);
  return rm_seq_check_sizes(fn, D, B, nnz, LD);
}

int dien_params_ok(const char *fn, const char *what, const rm_dien_params *p) {
  RM_REQUIRE(p && p->gru_w && p->gru_u && p->gru_b && p->att_w && p->augru_w && p->augru_u && p->augru_b,
             "%s: %s has a NULL member", fn, what);
  return RM_OK;
}

}  // namespace

extern "C" int rm_dien_supported(int D, int max_len) { return dien_shape_ok(D, max_len) ? 1 : 0; }

extern "C" int64_t rm_dien_workspace(int D, int max_len, int64_t B, int64_t nnz, int backward) {
  if (!dien_shape_ok(D, max_len) || B < 0 || nnz < 0) return 0;
  const DienWs w = dien_ws(D, B, nnz);
  return backward ? w.total : w.fwd_total;
}

#define RM_DIEN_LAUNCH(KERNEL_, grid_, smem_, ...)                                                         \
  do {                                                                                                     \
    switch (D) {                                                                                           \
      case 8: rm_launch_lds(KERNEL_<8>, dim3(grid_), dim3(kThreads), smem_, st, __VA_ARGS__); break;       \
      case 16: rm_launch_lds(KERNEL_<16>, dim3(grid_), dim3(kThreads), smem_, st, __VA_ARGS__); break;     \
      default: rm_launch_lds(KERNEL_<32>, dim3(grid_), dim3(kThreads), smem_, st, __VA_ARGS__); break;     \
    }                                                                                                      \
  } while (0)

#define RM_DIEN_LAUNCH_PLAIN(KERNEL_, grid_, ...)                                                     \
  do {                                                                                                \
    switch (D) {                                                                                      \
      case 8: hipLaunchKernelGGL(KERNEL_<8>, dim3(grid_), dim3(kThreads), 0, st, __VA_ARGS__); break;   \
      case 16: hipLaunchKernelGGL(KERNEL_<16>, dim3(grid_), dim3(kThreads), 0, st, __VA_ARGS__); break; \
      default: hipLaunchKernelGGL(KERNEL_<32>, dim3(grid_), dim3(kThreads), 0, st, __VA_ARGS__); break; \
    }                                                                                                 \
  } while (0)

static size_t dien_smem(int D) {
  return sizeof(float) * (size_t)(D == 8 ? DienLds<8>::N : D == 16 ? DienLds<16>::N : DienLds<32>::N);
}
// the forward's: the parameters and max_len float64 scores per example of a block (69.4 KiB at most: D = 32, 256)
static size_t dien_fwd_smem(int D, int ML) {
  const size_t sc = (size_t)(D == 8 ? DienLds<8>::SC : D == 16 ? DienLds<16>::SC : DienLds<32>::SC);
  return sizeof(float) * sc + sizeof(double) * (size_t)(kThreads / D) * (size_t)ML;
}

extern "C" int rm_dien_fwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                           const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
                           const rm_dien_params *params, int max_len, int save, float *out, float *workspace,
                           rm_stream_t stream) {
  int rc = dien_check("rm_dien_fwd", D, max_len, B, nnz, LD);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  if ((rc = dien_params_ok("rm_dien_fwd", "params", params)) != RM_OK) return rc;
  if ((rc = rm_seq_check_fwd("rm_dien_fwd", rows, offsets, ids, qrow, nnz, out, workspace)) != RM_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const DienWs w = dien_ws(D, B, nnz);
  const DienIn in{rows, LD, row0, offsets, ids, qrow, B, nnz, max_len};
  RM_DIEN_LAUNCH(dien_fwd_kernel, dien_seq_blocks(B, D), dien_fwd_smem(D, max_len), in, *params, save ? 1 : 0, out,
                 workspace + w.h, workspace + w.a, workspace + w.g);
  RM_CHECK_LAUNCH("rm_dien_fwd");
  return RM_OK;
}

extern "C" int rm_dien_bwd(const float *rows, int64_t LD, int D, int64_t row0, const int64_t *offsets,
                           const int64_t *ids, const int64_t *qrow, int64_t B, int64_t nnz,
                           const rm_dien_params *params, int max_len, const float *d_out, int64_t do_stride,
                           float *d_keys, float *d_query, int64_t dq_stride, const rm_dien_params *grads,
                           float *workspace, rm_stream_t stream) {
  int rc = dien_check("rm_dien_bwd", D, max_len, B, nnz, LD);
  if (rc != RM_OK) return rc;
  if ((rc = dien_params_ok("rm_dien_bwd", "params", params)) != RM_OK) return rc;
  if ((rc = dien_params_ok("rm_dien_bwd", "grads", grads)) != RM_OK) return rc;
  if ((rc = rm_seq_check_bwd("rm_dien_bwd", D, rows, offsets, ids, qrow, B, nnz, d_out, do_stride, d_keys, d_query,
                              dq_stride, workspace)) != RM_OK)
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const DienWs w = dien_ws(D, B, nnz);
  const bool work = B > 0 && nnz > 0;
  const int nwg = work ? dien_wg_blocks(B) : 0, natt = work ? dien_att_blocks(B) : 0;
  const int NG = dien_gru_floats(D);
  if (nnz > 0 && (rc = rm_clear_async("rm_dien_bwd", "d_keys", d_keys, nnz * D, st)) != RM_OK) return rc;
  if (work) {
    int *flag = reinterpret_cast<int *>(workspace + w.flag);
    if ((rc = rm_clear_async("rm_dien_bwd", "the flags", workspace + w.flag, nnz, st)) != RM_OK) return rc;
    const DienIn in{rows, LD, row0, offsets, ids, qrow, B, nnz, max_len};
    const DienBwd o{d_out, do_stride, d_keys, d_query, dq_stride, workspace + w.h, workspace + w.a, workspace + w.g,
                    workspace + w.ga, workspace + w.gb, workspace + w.dp, flag};
    RM_DIEN_LAUNCH(dien_bwd_kernel, dien_seq_blocks(B, D), dien_smem(D), in, *params, o);
    RM_CHECK_LAUNCH("rm_dien_bwd");
    const int64_t chunk = (B + nwg - 1) / nwg, achunk = (B + natt - 1) / natt;
    const float *hws = workspace + w.h, *gws = workspace + w.g, *ga = workspace + w.ga, *gb = workspace + w.gb;
    RM_DIEN_LAUNCH_PLAIN(dien_wgrad_kernel, nwg, (const float *)nullptr, rows, LD, row0, ids, hws, ga, (const int *)flag,
                         nnz, offsets, B, chunk, workspace + w.part_gru);
    RM_DIEN_LAUNCH_PLAIN(dien_wgrad_kernel, nwg, hws, rows, LD, row0, ids, gws, gb, (const int *)flag, nnz, offsets, B,
                         chunk, workspace + w.part_augru);
    RM_DIEN_LAUNCH_PLAIN(dien_attw_kernel, natt, (const float *)(workspace + w.dp), rows, LD, qrow, B, achunk,
                         workspace + w.part_att);
    RM_CHECK_LAUNCH("rm_dien_bwd (weight gradients)");
  }
  const int M = 3 * D * D;
  rm_sum_partials(workspace + w.part_gru, nwg, NG, rm_sum_dsts(grads->gru_w, M, grads->gru_u, M, grads->gru_b, 3 * D),
                  st);
  rm_sum_partials(workspace + w.part_augru, nwg, NG,
                  rm_sum_dsts(grads->augru_w, M, grads->augru_u, M, grads->augru_b, 3 * D), st);
  rm_sum_partials(workspace + w.part_att, natt, D * D, rm_sum_dsts(grads->att_w, D * D), st);
  RM_CHECK_LAUNCH("rm_dien_bwd (finish)");
  return RM_OK;
}
