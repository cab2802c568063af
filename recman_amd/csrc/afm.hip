// AFM attention layer (Attentional Factorization Machines, arXiv 1708.04617 eq. (4)-(6)), forward and backward.
// The class is ABSENT from the reference (recman/tf/core/AFM.py:7 has the import commented out; used at
// AFM.py:119-122).  Per example, over the P = F(F-1)/2 field pairs (i < j) of E [F,D]:
//     P_ij = E_i * E_j,  z_ij = W^T P_ij + b,  s_ij = h . relu(z_ij),  a = softmax_ij(s),
//     v = sum_ij a_ij P_ij,  logit = p . (m * v)                 (m: dropout multiplier, absent = 1)
// Nothing of size [P, D] or [P, T] ever reaches HBM: the forward reads E once and writes logit + a record of D + 2
// floats per example (the softmax's max and denominator, u = m * v); the backward re-reads E, recomputes z, and
// writes d_rows once.
//
// Mapping.  One 64-lane wave per block; the wave is cut into G = 64 / GW lane groups (GW = 16, 32 or 64, the
// smallest that holds F lanes), one EXAMPLE per group, its rows staged in LDS (row stride D + 4 floats: 16-byte
// rows, conflict-free float4 reads for consecutive fields).  The pairs are walked in F/2 passes; in pass k the
// group's lanes cover two rows of the pair triangle at once,
//     lanes [0, F-1-k)   : row iA = k      -> pairs (iA, iA+1+lane)
//     lanes [F-1-k, F)   : row iB = F-2-k  -> pairs (iB, iB+1+(lane-(F-1-k)))       (off when iB == iA)
// so F of the GW lanes work in every pass and each pair is visited exactly once.  A lane forms its pair product
// in registers (D floats) and runs the D x T score product on the VALU with W, b, h as wave-uniform (scalar)
// operands (scalar loads issued row by row next to their use).  The softmax is online per lane (running max / sum /
// weighted logit) and merged over the group with xor butterflies - fixed order.
//
// Backward, per pass: a = exp(s - max) / denom from the saved pair of numbers, ds, dz = ds h [z > 0],
// dP = a c + W dz in registers.  dE_j += dP E_i goes to the group's LDS copy of dE row by row (row A's lanes, then
// row B's: no two lanes of a step share a j); dE_i = sum_j dP E_j is summed by D lanes over the step's lanes through
// LDS, in lane order.  The parameter gradients dW = sum P dz^T, db = sum dz, dh = sum ds relu(z) are a small GEMM
// over the pass's pairs: every lane owns D T / 64 elements of dW (+ a db / dh column) in registers for the whole
// kernel, the pass's P and dz rows go through LDS.  Per-block partial sums land in the workspace and one
// finishing kernel (rm_sum_partials) adds them in block order: no float atomics anywhere, two runs are bit-equal.
#include <math.h>

#include <type_traits>

#include "rm_launch.h"

namespace {

constexpr int kMaxF = 40;
constexpr int kMaxT = 64;
constexpr int kMaxBlocks = 2048;  // 8 single-wave blocks per CU

inline int afm_gw(int F) { return F <= 16 ? 16 : (F <= 32 ? 32 : 64); }
inline bool afm_d_ok(int D) { return D == 8 || D == 16 || D == 32 || D == 64; }
// the backward's T tiling: chunks of TC hidden units, NC of them (T padded with zero columns)
inline int afm_tc(int T) { return T <= 8 ? 8 : 16; }
inline int afm_nc(int T) { return T <= 8 ? 1 : (T + 15) / 16; }
inline int64_t afm_param_floats(int D, int T) { return ((int64_t)(2 * D + 2) * afm_tc(T) * afm_nc(T) + 3) / 4 * 4; }
inline int64_t afm_part_floats(int D, int T) { return (int64_t)D * T + 2 * T + D; }
inline int afm_blocks(int64_t B, int F) {
  const int G = 64 / afm_gw(F);
  return rm_grid_cap((B + G - 1) / G, kMaxBlocks);
}

__device__ __forceinline__ float group_sum(float v, int gw) {
  for (int o = gw >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float group_max(float v, int gw) {
  for (int o = gw >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// A wave-uniform pointer the compiler must treat as freshly made: the loads behind it stay where they are written
// (scalar loads right in front of their use).  Without it every W element is hoisted out of the pass loop as a
// loop invariant - thousands of scalar registers, spilled lane by lane into vector registers.
// (Returned in the constant address space: read-only data at a uniform address is then always a scalar load.)
typedef const float __attribute__((address_space(4))) *afm_cptr;
__device__ __forceinline__ afm_cptr fresh(const float *p) {
  asm volatile("" : "+s"(p));
  return (afm_cptr)p;
}

// f(integral_constant<0>) ... f(integral_constant<N-1>): a loop whose index is a constant in every body (register
// arrays indexed by it stay registers even where the unroller would give up, e.g. around a barrier)
template <int I, int N, class Fn>
__device__ __forceinline__ void static_for(Fn &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// which pair a lane holds in pass `pass` (see the header comment)
struct PairSlot {
  int i, j;
  bool inA, inB;
};
__device__ __forceinline__ PairSlot pair_slot(int pass, int lg, int F) {
  PairSlot s;
  const int iA = pass, iB = F - 2 - pass, nA = F - 1 - iA;
  s.inA = lg < nA;
  s.inB = !s.inA && lg < F && iB != iA;
  s.i = s.inA ? iA : iB;
  s.j = s.inA ? iA + 1 + lg : iB + 1 + (lg - nA);
  if (!(s.inA || s.inB)) s.i = s.j = 0;
  return s;
}

// E rows (and, for the backward, the upstream dE rows) of the G examples from `base` on -> LDS, zero past the batch
template <int D>
__device__ __forceinline__ void stage_rows(const float *__restrict__ src, int64_t base, int64_t B, int G, int F,
                                           float *dst) {
  constexpr int DS = D + 4, Q = D / 4;
  for (int q = threadIdx.x; q < G * F * Q; q += 64) {
    const int gq = q / (F * Q), r = q - gq * F * Q, f = r / Q, c = r - f * Q;
    const int64_t e = base + gq;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src != nullptr && e < B) v = *reinterpret_cast<const float4 *>(src + (e * F + f) * D + 4 * c);
    *reinterpret_cast<float4 *>(dst + (gq * F + f) * DS + 4 * c) = v;
  }
}

// pm[d] = p[d] * mask[e, d] per example of the group
__device__ __forceinline__ void stage_pm(const float *__restrict__ p, const float *__restrict__ mask, int64_t base,
                                         int64_t B, int G, int D, float *pm) {
  for (int q = threadIdx.x; q < G * D; q += 64) {
    const int gq = q / D, d = q - gq * D;
    const int64_t e = base + gq;
    float v = 0.f;
    if (e < B) v = p[d] * (mask != nullptr ? mask[e * D + d] : 1.f);
    pm[q] = v;
  }
}

template <int D>
__device__ __forceinline__ void pair_product(const float *ei, const float *ej, float (&P)[D]) {
#pragma unroll
  for (int q = 0; q < D / 4; ++q) {
    const float4 a = *reinterpret_cast<const float4 *>(ei + 4 * q);
    const float4 b = *reinterpret_cast<const float4 *>(ej + 4 * q);
    P[4 * q] = a.x * b.x; P[4 * q + 1] = a.y * b.y; P[4 * q + 2] = a.z * b.z; P[4 * q + 3] = a.w * b.w;
  }
}

template <int D>
__device__ __forceinline__ float dot_lds(const float *x, const float (&P)[D]) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < D / 4; ++q) {
    const float4 a = *reinterpret_cast<const float4 *>(x + 4 * q);
    s = fmaf(a.x, P[4 * q], s); s = fmaf(a.y, P[4 * q + 1], s);
    s = fmaf(a.z, P[4 * q + 2], s); s = fmaf(a.w, P[4 * q + 3], s);
  }
  return s;
}

// ------------------------------------------------------------------------------------------------ forward
template <int D>
__global__ __launch_bounds__(64) void afm_fwd_kernel(const float *__restrict__ E, const float *__restrict__ W,
                                                     const float *__restrict__ bb, const float *__restrict__ h,
                                                     const float *__restrict__ p, const float *__restrict__ mask,
                                                     int64_t B, int F, int T, int GW, float *__restrict__ logit,
                                                     float *__restrict__ stats) {
  extern __shared__ float sm[];
  constexpr int DS = D + 4;
  const int lane = threadIdx.x, G = 64 / GW, grp = lane / GW, lg = lane % GW;
  float *Es = sm;               // [G][F][DS]
  float *pm = Es + G * F * DS;  // [G][D]
  const int NP = F / 2;         // = ceil((F - 1) / 2) passes
  const int T8 = T & ~7;
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    __syncthreads();
    stage_rows<D>(E, base, B, G, F, Es);
    stage_pm(p, mask, base, B, G, D, pm);
    __syncthreads();
    const int64_t ex = base + grp;
    const bool ex_ok = ex < B;
    // online softmax of this lane's pairs: running max, sum of exponentials, sum of exp * (pm . P)
    float m_run = -INFINITY, l_run = 0.f, w_run = 0.f;
    float v[D];  // training only: sum of exp * P, for the record the backward reads
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = 0.f;
    for (int pass = 0; pass < NP; ++pass) {
      const PairSlot ps = pair_slot(pass, lg, F);
      const bool active = (ps.inA || ps.inB) && ex_ok;
      float P[D];
      pair_product<D>(Es + (grp * F + ps.i) * DS, Es + (grp * F + ps.j) * DS, P);
      float s = 0.f;
      for (int t0 = 0; t0 < T8; t0 += 8) {
        float z[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) z[t] = bb[t0 + t];
        const afm_cptr wc = fresh(W + t0);
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const afm_cptr w = wc + d * T;
#pragma unroll
          for (int t = 0; t < 8; ++t) z[t] = fmaf(P[d], w[t], z[t]);
          if ((d & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // a few rows of W in scalar registers at a time
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) s = fmaf(h[t0 + t], fmaxf(z[t], 0.f), s);
      }
      for (int t = T8; t < T; ++t) {
        float z = bb[t];
        const afm_cptr w = fresh(W + t);
#pragma unroll
        for (int d = 0; d < D; ++d) z = fmaf(P[d], w[d * T], z);
        s = fmaf(h[t], fmaxf(z, 0.f), s);
      }
      if (active) {
        const float qq = dot_lds<D>(pm + grp * D, P);
        const float mn = fmaxf(m_run, s);
        const float sc = expf(m_run - mn);  // 0 on the first pair (m_run = -inf)
        const float e = expf(s - mn);
        l_run = fmaf(l_run, sc, e);
        w_run = fmaf(w_run, sc, e * qq);
        m_run = mn;
        if (stats != nullptr) {
#pragma unroll
          for (int d = 0; d < D; ++d) v[d] = fmaf(v[d], sc, e * P[d]);
        }
      }
    }
    const float M = group_max(m_run, GW);
    const float sc = m_run == -INFINITY ? 0.f : expf(m_run - M);
    const float l = group_sum(l_run * sc, GW);
    const float w = group_sum(w_run * sc, GW);
    if (ex_ok && lg == 0) {
      logit[ex] = w / l;
    }
    if (stats != nullptr) {
      // the record: [max score | denominator | u = mask * v (D)], v = sum_ij a_ij P_ij
      float *rec = stats + (ex_ok ? ex : 0) * (D + 2);
      const float il = 1.f / l;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const float vd = group_sum(v[d] * sc, GW) * il;
        if (ex_ok && lg == (d & 15)) rec[2 + d] = vd * (mask != nullptr ? mask[ex * D + d] : 1.f);
      }
      if (ex_ok && lg == 0) {
        rec[0] = M;
        rec[1] = l;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- backward
// W [D,T], b, h [T] -> Wp [D][TP] | bp [TP] | hp [TP] | Wp^T [TP][D], zero past T (exact: relu(0) * 0 = 0)
__global__ void afm_pack_kernel(const float *__restrict__ W, const float *__restrict__ b,
                                const float *__restrict__ h, int D, int T, int TP, float *__restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (D + 2) * TP) return;
  const int r = e / TP, t = e - r * TP;
  float v = 0.f;
  if (t < T) v = r < D ? W[r * T + t] : (r == D ? b[t] : h[t]);
  out[e] = v;
  if (r < D) out[(D + 2) * TP + t * D + r] = v;
}

template <int D, int TC, int NC>
__global__ __launch_bounds__(64) void afm_bwd_kernel(
    const float *__restrict__ E, const float *__restrict__ params, const float *__restrict__ p,
    const float *__restrict__ mask, const float *__restrict__ g, const float *__restrict__ logit,
    const float *__restrict__ stats, const float *dE_up, int64_t B, int F, int T, int GW, float *d_rows,
    float *__restrict__ part) {
  extern __shared__ float sm[];
  constexpr int DS = D + 4, TP = TC * NC, PS = D + 1, ZS = TC + 1;
  constexpr int ND = 64 / TC;  // lane = (dg, t): t = lane % TC, dg = lane / TC owns rows d = dg + ND k of dW
  constexpr int KD = D / ND;
  const float *__restrict__ Wp = params;
  const float *__restrict__ bp = params + D * TP;
  const float *__restrict__ hp = params + (D + 1) * TP;
  const float *__restrict__ WpT = params + (D + 2) * TP;
  const int lane = threadIdx.x, G = 64 / GW, grp = lane / GW, lg = lane % GW;
  float *Es = sm;                 // [G][F][DS]  the examples' rows
  float *dEs = Es + G * F * DS;   // [G][F][DS]  their gradient
  float *pm = dEs + G * F * DS;   // [G][D]      p * mask
  float *Pb = pm + G * D;         // [64][PS]    the pass's pair products; then the dE_i contributions
  float *zb = Pb + 64 * PS;       // [64][ZS]    dz of the current chunk
  float *rb = zb + 64 * ZS;       // [64][ZS]    ds * relu(z)
  const int NP = F / 2;
  const int tq = lane % TC, dg = lane / TC;

  float acc[NC][KD], dbacc[NC], dhacc[NC], dpacc = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dbacc[c] = dhacc[c] = 0.f;
#pragma unroll
    for (int k = 0; k < KD; ++k) acc[c][k] = 0.f;
  }

  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    __syncthreads();
    stage_rows<D>(E, base, B, G, F, Es);
    stage_rows<D>(dE_up, base, B, G, F, dEs);
    stage_pm(p, mask, base, B, G, D, pm);
    __syncthreads();
    const int64_t ex = base + grp;
    const bool ex_ok = ex < B;
    const float gg = ex_ok ? g[ex] : 0.f;
    const float lo = ex_ok ? logit[ex] : 0.f;
    const float M = ex_ok ? stats[(D + 2) * ex] : 0.f;
    const float invl = ex_ok ? 1.f / stats[(D + 2) * ex + 1] : 0.f;

    for (int pass = 0; pass < NP; ++pass) {
      const PairSlot ps = pair_slot(pass, lg, F);
      const bool active = (ps.inA || ps.inB) && ex_ok;
      const float *ei = Es + (grp * F + ps.i) * DS, *ej = Es + (grp * F + ps.j) * DS;
      float P[D], dP[D], z[NC][TC];
      pair_product<D>(ei, ej, P);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const afm_cptr bc = fresh(bp) + c * TC;
#pragma unroll
        for (int t = 0; t < TC; ++t) z[c][t] = bc[t];
      }
#pragma unroll
      for (int d = 0; d < D; ++d)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const afm_cptr w = fresh(Wp) + (d * TP + c * TC);
#pragma unroll
          for (int t = 0; t < TC; ++t) z[c][t] = fmaf(P[d], w[t], z[c][t]);
          __builtin_amdgcn_sched_barrier(0);  // one row of W in scalar registers at a time
        }
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const afm_cptr hc = fresh(hp) + c * TC;
#pragma unroll
        for (int t = 0; t < TC; ++t) s = fmaf(hc[t], fmaxf(z[c][t], 0.f), s);
      }
      const float a = active ? expf(s - M) * invl : 0.f;
      // ds = a (c . P - g logit) = a g (pm . P - logit): the same dot product, in the same order, as the forward's -
      // with a single pair it IS the logit and ds is exactly 0
      const float ac = a * gg;
      const float ds = ac * (dot_lds<D>(pm + grp * D, P) - lo);
#pragma unroll
      for (int d4 = 0; d4 < D / 4; ++d4) {
        const float4 m4 = *reinterpret_cast<const float4 *>(pm + grp * D + 4 * d4);
        dP[4 * d4] = ac * m4.x; dP[4 * d4 + 1] = ac * m4.y; dP[4 * d4 + 2] = ac * m4.z; dP[4 * d4 + 3] = ac * m4.w;
      }
#pragma unroll
      for (int d = 0; d < D; ++d) Pb[lane * PS + d] = P[d];
      static_for<0, NC>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
#pragma unroll
        for (int t = 0; t < TC; ++t) {
          const float u = z[c][t] > 0.f ? ds : 0.f;
          const float dz = u * fresh(hp)[c * TC + t];
          zb[lane * ZS + t] = dz;
          rb[lane * ZS + t] = u * z[c][t];
          const afm_cptr w = fresh(WpT) + (c * TC + t) * D;
#pragma unroll
          for (int d = 0; d < D; ++d) dP[d] = fmaf(w[d], dz, dP[d]);
          // (dP is next read behind the barrier below: without this pin the products are sunk there and
          // every row of W^T waits for them in spilled scalar registers)
#pragma unroll
          for (int d = 0; d < D; ++d) asm volatile("" : "+v"(dP[d]));
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // dW[dg + ND k][c TC + tq] += sum over the pass's pairs of P[d] dz[t]; db, dh columns beside it
        for (int gq = 0; gq < G; ++gq) {
          for (int l = 0; l < F; ++l) {
            const int pr = gq * GW + l;
            const float dz = zb[pr * ZS + tq];
            dbacc[c] += dz;
            dhacc[c] += rb[pr * ZS + tq];
#pragma unroll
            for (int k = 0; k < KD; ++k) acc[c][k] = fmaf(Pb[pr * PS + dg + ND * k], dz, acc[c][k]);
          }
        }
        __syncthreads();
      });
      // dE: the lane's own j row by row (A, then B), the rows iA / iB through LDS
      {
        float *dj = dEs + (grp * F + ps.j) * DS;
#pragma unroll
        for (int q4 = 0; q4 < D / 4; ++q4) {
          const float4 xj = *reinterpret_cast<const float4 *>(ej + 4 * q4);
          Pb[lane * PS + 4 * q4] = active ? dP[4 * q4] * xj.x : 0.f;
          Pb[lane * PS + 4 * q4 + 1] = active ? dP[4 * q4 + 1] * xj.y : 0.f;
          Pb[lane * PS + 4 * q4 + 2] = active ? dP[4 * q4 + 2] * xj.z : 0.f;
          Pb[lane * PS + 4 * q4 + 3] = active ? dP[4 * q4 + 3] * xj.w : 0.f;
        }
        if (active && ps.inA) {
#pragma unroll
          for (int q4 = 0; q4 < D / 4; ++q4) {
            const float4 xi = *reinterpret_cast<const float4 *>(ei + 4 * q4);
            float4 o = *reinterpret_cast<float4 *>(dj + 4 * q4);
            o.x = fmaf(dP[4 * q4], xi.x, o.x); o.y = fmaf(dP[4 * q4 + 1], xi.y, o.y);
            o.z = fmaf(dP[4 * q4 + 2], xi.z, o.z); o.w = fmaf(dP[4 * q4 + 3], xi.w, o.w);
            *reinterpret_cast<float4 *>(dj + 4 * q4) = o;
          }
        }
        __syncthreads();
        if (active && ps.inB) {
#pragma unroll
          for (int q4 = 0; q4 < D / 4; ++q4) {
            const float4 xi = *reinterpret_cast<const float4 *>(ei + 4 * q4);
            float4 o = *reinterpret_cast<float4 *>(dj + 4 * q4);
            o.x = fmaf(dP[4 * q4], xi.x, o.x); o.y = fmaf(dP[4 * q4 + 1], xi.y, o.y);
            o.z = fmaf(dP[4 * q4 + 2], xi.z, o.z); o.w = fmaf(dP[4 * q4 + 3], xi.w, o.w);
            *reinterpret_cast<float4 *>(dj + 4 * q4) = o;
          }
        }
        // (rows iA and iB are no lane's j in this step: j > iB >= iA)
        const int iA = pass, iB = F - 2 - pass, nA = F - 1 - iA;
        for (int item = lane; item < G * 2 * D; item += 64) {
          const int d = item % D, seg = (item / D) & 1, gq = item / (2 * D);
          if (seg == 1 && iB == iA) continue;
          const int l0 = seg == 0 ? 0 : nA, l1 = seg == 0 ? nA : F;
          float sum = 0.f;
          for (int l = l0; l < l1; ++l) sum += Pb[(gq * GW + l) * PS + d];
          dEs[(gq * F + (seg == 0 ? iA : iB)) * DS + d] += sum;
        }
        __syncthreads();
      }
    }
    // d p += g * u, u = mask * v from the forward's record
    if (lane < D) {
      for (int gq = 0; gq < G; ++gq) {
        const int64_t e = base + gq;
        if (e >= B) break;
        dpacc = fmaf(g[e], stats[(D + 2) * e + 2 + lane], dpacc);
      }
    }
    constexpr int Q = D / 4;
    for (int q = lane; q < G * F * Q; q += 64) {
      const int gq = q / (F * Q), r = q - gq * F * Q, f = r / Q, c = r - f * Q;
      const int64_t e = base + gq;
      if (e < B)
        *reinterpret_cast<float4 *>(d_rows + (e * F + f) * D + 4 * c) =
            *reinterpret_cast<const float4 *>(dEs + (gq * F + f) * DS + 4 * c);
    }
  }
  // this block's partial sums: [dW (D x T) | db (T) | dh (T) | dp (D)]
  float *out = part + (int64_t)blockIdx.x * ((int64_t)D * T + 2 * T + D);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int t = c * TC + tq;
    if (t < T) {
#pragma unroll
      for (int k = 0; k < KD; ++k) out[(dg + ND * k) * T + t] = acc[c][k];
      if (dg == 0) {
        out[D * T + t] = dbacc[c];
        out[D * T + T + t] = dhacc[c];
      }
    }
  }
  if (lane < D) out[D * T + 2 * T + lane] = dpacc;
}

int afm_check(const char *fn, int64_t B, int F, int D, int T) {
  RM_REQUIRE(B >= 0, "%s: bad batch size", fn);
  RM_REQUIRE(afm_d_ok(D), "%s: D=%d unsupported (8, 16, 32, 64)", fn, D);
  RM_REQUIRE(F >= 2 && F <= kMaxF, "%s: F=%d unsupported (2..%d)", fn, F, kMaxF);
  RM_REQUIRE(T >= 1 && T <= kMaxT, "%s: T=%d unsupported (1..%d)", fn, T, kMaxT);
  return RM_OK;
}

}  // namespace

extern "C" int rm_afm_supported(int F, int D, int T) {
  return afm_d_ok(D) && F >= 2 && F <= kMaxF && T >= 1 && T <= kMaxT ? 1 : 0;
}

extern "C" int rm_afm_fwd(const float *E, const float *W, const float *b, const float *h, const float *p,
                          const float *mask, int64_t B, int F, int D, int T, float *logit, float *stats,
                          rm_stream_t stream) {
  int rc = afm_check("rm_afm_fwd", B, F, D, T);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  RM_REQUIRE(E && W && b && h && p && logit, "rm_afm_fwd: NULL argument");
  RM_REQUIRE(rm_aligned16(E), "rm_afm_fwd: E unaligned");
  const int GW = afm_gw(F), G = 64 / GW;
  const size_t smem = (size_t)(G * F * (D + 4) + G * D) * sizeof(float);
  dim3 grid(rm_grid_cap((B + G - 1) / G, 256 * 16));
  hipStream_t st = (hipStream_t)stream;
#define RM_AFM_FWD(D_) \
  hipLaunchKernelGGL((afm_fwd_kernel<D_>), grid, dim3(64), smem, st, E, W, b, h, p, mask, B, F, T, GW, logit, stats)
  switch (D) {
    case 8: RM_AFM_FWD(8); break;
    case 16: RM_AFM_FWD(16); break;
    case 32: RM_AFM_FWD(32); break;
    default: RM_AFM_FWD(64); break;
  }
#undef RM_AFM_FWD
  RM_CHECK_LAUNCH("rm_afm_fwd");
  return RM_OK;
}

extern "C" int64_t rm_afm_bwd_workspace(int64_t B, int F, int D, int T) {
  if (!rm_afm_supported(F, D, T) || B < 0) return 0;
  return afm_param_floats(D, T) + (int64_t)afm_blocks(B, F) * afm_part_floats(D, T);
}

extern "C" int rm_afm_bwd(const float *E, const float *W, const float *b, const float *h, const float *p,
                          const float *mask, const float *g, const float *logit, const float *stats,
                          const float *dE_up, int64_t B, int F, int D, int T, float *d_rows, float *dW, float *db,
                          float *dh, float *dp, float *workspace, rm_stream_t stream) {
  int rc = afm_check("rm_afm_bwd", B, F, D, T);
  if (rc != RM_OK) return rc;
  RM_REQUIRE(W && b && h && p && dW && db && dh && dp && workspace, "rm_afm_bwd: NULL argument");
  RM_REQUIRE(B == 0 || (E && g && logit && stats && d_rows), "rm_afm_bwd: NULL argument");
  RM_REQUIRE(rm_aligned16(E) && rm_aligned16(d_rows) && rm_aligned16(dE_up) && rm_aligned16(workspace),
             "rm_afm_bwd: E, dE_up, d_rows and workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int TC = afm_tc(T), NC = afm_nc(T), TP = TC * NC;
  const int nblk = B == 0 ? 0 : afm_blocks(B, F);
  float *part = workspace + afm_param_floats(D, T);
  if (B > 0) {
    hipLaunchKernelGGL(afm_pack_kernel, dim3(((D + 2) * TP + 255) / 256), dim3(256), 0, st, W, b, h, D, T, TP,
                       workspace);
    const int GW = afm_gw(F), G = 64 / GW;
    const size_t smem =
        (size_t)(2 * G * F * (D + 4) + G * D + 64 * (D + 1) + 2 * 64 * (TC + 1)) * sizeof(float);
    dim3 grid(nblk);
#define RM_AFM_BWD(D_, TC_, NC_)                                                                               \
  hipLaunchKernelGGL((afm_bwd_kernel<D_, TC_, NC_>), grid, dim3(64), smem, st, E, (const float *)workspace, p, \
                     mask, g, logit, stats, dE_up, B, F, T, GW, d_rows, part)
#define RM_AFM_BWD_T(D_)                     \
  if (TC == 8) RM_AFM_BWD(D_, 8, 1);         \
  else if (NC == 1) RM_AFM_BWD(D_, 16, 1);   \
  else if (NC == 2) RM_AFM_BWD(D_, 16, 2);   \
  else if (NC == 3) RM_AFM_BWD(D_, 16, 3);   \
  else RM_AFM_BWD(D_, 16, 4)
    switch (D) {
      case 8: RM_AFM_BWD_T(8); break;
      case 16: RM_AFM_BWD_T(16); break;
      case 32: RM_AFM_BWD_T(32); break;
      default: RM_AFM_BWD_T(64); break;
    }
#undef RM_AFM_BWD_T
#undef RM_AFM_BWD
    RM_CHECK_LAUNCH("rm_afm_bwd");
  }
  // fixed-order sum of the per-block partials (B == 0: no blocks, all +0.0)
  rm_sum_partials(part, nblk, D * T + 2 * T + D, rm_sum_dsts(dW, D * T, db, T, dh, T, dp, D), st);
  RM_CHECK_LAUNCH("rm_afm_bwd (finish)");
  return RM_OK;
}
