// AutoInt interacting layer (multi-head self-attention over the fields, arXiv 1810.11921 eq. (5)-(8)), forward and
// backward, and the model's last projection.  Nothing in the reference implements it; the contract is the paper's:
//     Q = X Wq, K = X Wk, V = X Wv                         X [B,F,Din], W* [Din,HD], HD = H dk
//     s^h_mk = <Q^h_m, K^h_k> c,  a^h_m. = softmax_k(s^h_m.),  O_m = concat_h sum_k a^h_mk V^h_k
//     Y_m = relu(O_m + X_m Wr)   (Wr absent: relu(O_m))
// Q, K, V, the [F,F] scores and the softmax weights never reach HBM: per example the forward reads X and writes Y
// (+ 2 floats per (head, field): the softmax's max and denominator), the backward reads X, Y, dY and writes dX.
//
// Mapping.  A block of 256 threads owns a tile of G whole examples, R = G F field rows:
//   1. the four weight matrices sit side by side in LDS, Ws [Din][4 HD] (staged once per block); the tile's X rows
//      are staged row-major;
//   2. projection P = X Ws on the vector ALU: a thread forms a 2 x 4 block of P (two rows, four columns) from float4
//      LDS reads, k ascending in one fmaf chain per element - the backward recomputes the SAME chain, so its Q, K, V
//      (and with them the scores) are the forward's bits;
//   3. attention: one thread per (example, head, field m).  Its Q chunk lives in registers, K and V rows are LDS
//      broadcasts (the lanes of a wave are consecutive m of one (example, head)).  Two passes over k: the row maximum,
//      then exp(s - max), the denominator and the weighted sum of V.  O overwrites the thread's own Q chunk;
//   4. Y = relu(O + R) leaves through coalesced float4 stores.
// Backward, per tile: dP = dY [Y > 0] (= dO, and the residual's gradient); Q, K, V recomputed;
//   A. thread (e, h, m): delta_m = sum_k a_mk <dO_m, V_k>, then dQ_m = c sum_k ds_mk K_k, ds = a (da - delta);
//   B. thread (e, h, k): dK_k = c sum_m ds_mk Q_m, dV_k = sum_m a_mk dO_m - the same scores, m ascending;
//   C. dW* += X^T [dQ|dK|dV|dP]: every thread owns NI x 4 elements of the [Din][4 HD] gradient in registers for the
//      whole kernel; dX = [dQ|dK|dV|dP] Ws^T (+ dX_up) goes through LDS and leaves coalesced.
// Per-block partial sums of the parameter gradients land in the workspace; two small kernels add them in block order
// (16 segments, then the segments): no float atomics anywhere, two runs are bit-equal.
#include <math.h>

#include "rm_launch.h"

namespace {

constexpr int kMaxF = 40;
constexpr int kThreads = 256;
constexpr int kSeg = 16;                  // segments of the finishing sum
constexpr int kLdsBudget = 76 * 1024;     // two blocks per CU where the shape allows it
constexpr int64_t kPartFloats = 4 << 20;  // cap on the per-block partials of the backward (16 MiB)

inline bool ai_pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }
inline bool ai_ok(int F, int Din, int H, int dk) {
  if (F < 1 || F > kMaxF || !ai_pow2_in(Din, 8, 64) || !ai_pow2_in(H, 1, 8) || dk < 4 || dk > 64) return false;
  return ai_pow2_in(H * dk, 8, 64);
}
inline int ai_rp(int G, int F) { return (G * F + 1) & ~1; }
inline int64_t ai_fwd_floats(int G, int F, int Din, int HD) {
  return (int64_t)Din * 4 * HD + (int64_t)ai_rp(G, F) * ((Din + 4) + (4 * HD + 4));
}
inline int64_t ai_bwd_floats(int G, int F, int Din, int H, int HD) {
  return (int64_t)Din * 4 * HD + (int64_t)ai_rp(G, F) * ((Din + 4) + (3 * HD + 4) + (4 * HD + 4)) +
         (((int64_t)G * F * H * 3 + 3) & ~(int64_t)3);
}
// examples per tile: one (example, head, field) item per thread where LDS allows
inline int ai_pick_g(int F, int Din, int H, int HD, bool bwd) {
  int G = kThreads / (H * F);
  if (G < 1) G = 1;
  while (G > 1 && 4 * (bwd ? ai_bwd_floats(G, F, Din, H, HD) : ai_fwd_floats(G, F, Din, HD)) > kLdsBudget) --G;
  return G;
}
inline int ai_bwd_blocks(int64_t B, int F, int Din, int H, int HD) {
  const int G = ai_pick_g(F, Din, H, HD, true);
  int64_t cap = kPartFloats / ((int64_t)Din * 4 * HD);
  cap = cap < 256 ? 256 : (cap > 1024 ? 1024 : cap);
  return rm_grid_cap((B + G - 1) / G, (int)cap);
}
inline int ai_head_blocks(int64_t B) { return rm_grid_cap((B + 31) / 32, 1024); }

__device__ __forceinline__ void fma4(float4 &a, float s, const float4 &w) {
  a.x = fmaf(s, w.x, a.x); a.y = fmaf(s, w.y, a.y); a.z = fmaf(s, w.z, a.z); a.w = fmaf(s, w.w, a.w);
}
__device__ __forceinline__ float dot4(const float4 &a, const float4 &b, float s) {
  s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
  return s;
}
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }

// Wq | Wk | Wv | Wr [Din][HD] each -> Ws [Din][4 HD]; an absent matrix is zeros
__device__ __forceinline__ void ai_stage_w(const float *__restrict__ Wq, const float *__restrict__ Wk,
                                           const float *__restrict__ Wv, const float *__restrict__ Wr, int Din,
                                           int HD, float *Ws) {
  const int NC = 4 * HD, q4 = HD / 4;
  for (int q = threadIdx.x; q < Din * HD; q += kThreads) {
    const int i = q / HD, c = q - i * HD, blk = c / q4, j4 = c - blk * q4;
    const float *W = blk == 0 ? Wq : (blk == 1 ? Wk : (blk == 2 ? Wv : Wr));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (W != nullptr) v = ld4(W + i * HD + 4 * j4);
    st4(Ws + i * NC + blk * HD + 4 * j4, v);
  }
}

// rows [row0, row0 + R) of src [rows_total][W] -> dst [RP][DS]; zero past the batch and in the padding row
__device__ __forceinline__ void ai_stage_rows(const float *__restrict__ src, int64_t row0, int64_t rows_total, int R,
                                              int RP, int W, float *dst, int DS) {
  const int w4 = W / 4;
  for (int q = threadIdx.x; q < RP * w4; q += kThreads) {
    const int r = q / w4, c = q - r * w4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < R && row0 + r < rows_total) v = ld4(src + (row0 + r) * W + 4 * c);
    st4(dst + r * DS + 4 * c, v);
  }
}

// Ps[r][0 .. 4 nc4) = Xs[r][:] Ws[:][0 .. 4 nc4): a 2 x 4 block per thread, k ascending
__device__ __forceinline__ void ai_project(const float *Xs, int XS, const float *Ws, int NC, int Din, int nc4,
                                           float *Ps, int PS, int RP) {
  const int units = (RP / 2) * nc4;
  for (int u = threadIdx.x; u < units; u += kThreads) {
    const int ru = u / nc4, cg = u - ru * nc4;
    const float *x0 = Xs + 2 * ru * XS, *x1 = x0 + XS, *w = Ws + 4 * cg;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    for (int k = 0; k < Din; k += 4) {
      const float4 xa = ld4(x0 + k), xb = ld4(x1 + k);
      const float4 w0 = ld4(w + k * NC), w1 = ld4(w + (k + 1) * NC), w2 = ld4(w + (k + 2) * NC),
                   w3 = ld4(w + (k + 3) * NC);
      fma4(a0, xa.x, w0); fma4(a0, xa.y, w1); fma4(a0, xa.z, w2); fma4(a0, xa.w, w3);
      fma4(a1, xb.x, w0); fma4(a1, xb.y, w1); fma4(a1, xb.z, w2); fma4(a1, xb.w, w3);
    }
    st4(Ps + 2 * ru * PS + 4 * cg, a0);
    st4(Ps + (2 * ru + 1) * PS + 4 * cg, a1);
  }
}

template <int DK>
__device__ __forceinline__ void ld_chunk(const float *p, float (&v)[DK]) {
#pragma unroll
  for (int q = 0; q < DK / 4; ++q) {
    const float4 t = ld4(p + 4 * q);
    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
  }
}
template <int DK>
__device__ __forceinline__ void st_chunk(float *p, const float (&v)[DK], float c) {
#pragma unroll
  for (int q = 0; q < DK / 4; ++q)
    st4(p + 4 * q, make_float4(v[4 * q] * c, v[4 * q + 1] * c, v[4 * q + 2] * c, v[4 * q + 3] * c));
}
// sum_j a[j] b[j], j ascending, one fmaf chain (the products commute: dot(q, K row) and dot(k, Q row) are equal bits)
template <int DK>
__device__ __forceinline__ float dot_chunk(const float (&a)[DK], const float *b) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < DK / 4; ++q) {
    const float4 t = ld4(b + 4 * q);
    s = fmaf(a[4 * q], t.x, s); s = fmaf(a[4 * q + 1], t.y, s);
    s = fmaf(a[4 * q + 2], t.z, s); s = fmaf(a[4 * q + 3], t.w, s);
  }
  return s;
}
template <int DK>
__device__ __forceinline__ void axpy_chunk(float a, const float *x, float (&y)[DK]) {
#pragma unroll
  for (int q = 0; q < DK / 4; ++q) {
    const float4 t = ld4(x + 4 * q);
    y[4 * q] = fmaf(a, t.x, y[4 * q]); y[4 * q + 1] = fmaf(a, t.y, y[4 * q + 1]);
    y[4 * q + 2] = fmaf(a, t.z, y[4 * q + 2]); y[4 * q + 3] = fmaf(a, t.w, y[4 * q + 3]);
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <int DK>
__global__ __launch_bounds__(kThreads) void autoint_fwd_kernel(
    const float *__restrict__ X, const float *__restrict__ Wq, const float *__restrict__ Wk,
    const float *__restrict__ Wv, const float *__restrict__ Wr, int64_t B, int F, int Din, int H, int G, float scale,
    float *__restrict__ Y, float *__restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int HD = H * DK, NC = 4 * HD, XS = Din + 4, PS = NC + 4;
  const int R = G * F, RP = (R + 1) & ~1;
  float *Ws = sm;             // [Din][NC]
  float *Xs = Ws + Din * NC;  // [RP][XS]
  float *Ps = Xs + RP * XS;   // [RP][PS]  Q | K | V | R; O takes Q's place
  ai_stage_w(Wq, Wk, Wv, Wr, Din, HD, Ws);
  const int64_t rows_total = B * F;
  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    __syncthreads();
    ai_stage_rows(X, base * F, rows_total, R, RP, Din, Xs, XS);
    __syncthreads();
    ai_project(Xs, XS, Ws, NC, Din, HD, Ps, PS, RP);
    __syncthreads();
    for (int item = threadIdx.x; item < G * H * F; item += kThreads) {
      const int gh = item / F, m = item - gh * F, g = gh / H, h = gh - g * H;
      if (base + g >= B) continue;
      float *qp = Ps + (g * F + m) * PS + h * DK;
      const float *kb = Ps + g * F * PS + HD + h * DK, *vb = kb + HD;
      float q[DK], o[DK];
      ld_chunk<DK>(qp, q);
      float mx = -INFINITY;
      for (int k = 0; k < F; ++k) mx = fmaxf(mx, dot_chunk<DK>(q, kb + k * PS) * scale);
#pragma unroll
      for (int j = 0; j < DK; ++j) o[j] = 0.f;
      float l = 0.f;
      for (int k = 0; k < F; ++k) {
        const float e = expf(dot_chunk<DK>(q, kb + k * PS) * scale - mx);
        l += e;
        axpy_chunk<DK>(e, vb + k * PS, o);
      }
      st_chunk<DK>(qp, o, 1.f / l);
      if (stats != nullptr) {
        float *rec = stats + 2 * ((base * H * F) + item);
        rec[0] = mx;
        rec[1] = l;
      }
    }
    __syncthreads();
    const int h4 = HD / 4;
    for (int q = threadIdx.x; q < R * h4; q += kThreads) {
      const int r = q / h4, c = q - r * h4;
      if (base * F + r >= rows_total) break;
      const float4 o = ld4(Ps + r * PS + 4 * c), rr = ld4(Ps + r * PS + 3 * HD + 4 * c);
      st4(Y + (base * F + r) * HD + 4 * c, make_float4(fmaxf(o.x + rr.x, 0.f), fmaxf(o.y + rr.y, 0.f),
                                                       fmaxf(o.z + rr.z, 0.f), fmaxf(o.w + rr.w, 0.f)));
    }
  }
}

// ----------------------------------------------------------------------------------------------- backward
template <int DK, int NI>
__global__ __launch_bounds__(kThreads) void autoint_bwd_kernel(
    const float *__restrict__ X, const float *__restrict__ Wq, const float *__restrict__ Wk,
    const float *__restrict__ Wv, const float *__restrict__ Wr, const float *__restrict__ Y,
    const float *__restrict__ stats, const float *__restrict__ dY, int64_t B, int F, int Din, int H, int G,
    float scale, float *dX, const float *dX_up, float *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int HD = H * DK, NC = 4 * HD, XS = Din + 4, QS = 3 * HD + 4, PS = NC + 4;
  const int R = G * F, RP = (R + 1) & ~1;
  float *Ws = sm;             // [Din][NC]
  float *Xs = Ws + Din * NC;  // [RP][XS]   X; later the tile's dX
  float *Ps = Xs + RP * XS;   // [RP][QS]   Q | K | V
  float *Gs = Ps + RP * QS;   // [RP][PS]   dQ | dK | dV | dP
  float *st = Gs + RP * PS;   // [G H F][3] max, 1 / denominator, delta
  ai_stage_w(Wq, Wk, Wv, Wr, Din, HD, Ws);
  const int64_t rows_total = B * F;
  const int ncg = Wr != nullptr ? NC : 3 * HD;  // columns of [dQ|dK|dV|dP] that reach dX
  // this thread's share of d[Wq|Wk|Wv|Wr] [Din][NC]: rows ig + IT n, columns 4 jg .. 4 jg + 3
  const int IT = kThreads / HD, jg = threadIdx.x % HD, ig = threadIdx.x / HD;
  float4 acc[NI];
#pragma unroll
  for (int n = 0; n < NI; ++n) acc[n] = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int64_t base = (int64_t)blockIdx.x * G; base < B; base += (int64_t)gridDim.x * G) {
    __syncthreads();
    ai_stage_rows(X, base * F, rows_total, R, RP, Din, Xs, XS);
    {
      const int h4 = HD / 4;
      for (int q = threadIdx.x; q < RP * h4; q += kThreads) {
        const int r = q / h4, c = q - r * h4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < R && base * F + r < rows_total) {
          const float4 y = ld4(Y + (base * F + r) * HD + 4 * c), d = ld4(dY + (base * F + r) * HD + 4 * c);
          v = make_float4(y.x > 0.f ? d.x : 0.f, y.y > 0.f ? d.y : 0.f, y.z > 0.f ? d.z : 0.f,
                          y.w > 0.f ? d.w : 0.f);
        }
        st4(Gs + r * PS + 3 * HD + 4 * c, v);
      }
      // the padding row of dQ | dK | dV (no item writes it)
      if (RP > R)
        for (int c = threadIdx.x; c < 3 * HD; c += kThreads) Gs[R * PS + c] = 0.f;
      for (int it = threadIdx.x; it < G * H * F; it += kThreads) {
        const bool ok = base + it / (H * F) < B;
        st[3 * it] = ok ? stats[2 * (base * H * F + it)] : 0.f;
        st[3 * it + 1] = ok ? 1.f / stats[2 * (base * H * F + it) + 1] : 0.f;
      }
    }
    __syncthreads();
    ai_project(Xs, XS, Ws, NC, Din, 3 * HD / 4, Ps, QS, RP);
    __syncthreads();
    // A: rows m.  delta_m = sum_k a_mk da_mk, dQ_m = c sum_k a_mk (da_mk - delta_m) K_k
    for (int item = threadIdx.x; item < G * H * F; item += kThreads) {
      const int gh = item / F, m = item - gh * F, g = gh / H, h = gh - g * H;
      const int r = g * F + m;
      float dq[DK];
#pragma unroll
      for (int j = 0; j < DK; ++j) dq[j] = 0.f;
      if (base + g < B) {
        const float *kb = Ps + g * F * QS + HD + h * DK, *vb = kb + HD;
        float q[DK], dO[DK];
        ld_chunk<DK>(Ps + r * QS + h * DK, q);
        ld_chunk<DK>(Gs + r * PS + 3 * HD + h * DK, dO);
        const float mx = st[3 * item], il = st[3 * item + 1];
        float delta = 0.f;
        for (int k = 0; k < F; ++k) {
          const float a = expf(dot_chunk<DK>(q, kb + k * QS) * scale - mx) * il;
          delta = fmaf(a, dot_chunk<DK>(dO, vb + k * QS), delta);
        }
        st[3 * item + 2] = delta;
        for (int k = 0; k < F; ++k) {
          const float a = expf(dot_chunk<DK>(q, kb + k * QS) * scale - mx) * il;
          const float ds = a * (dot_chunk<DK>(dO, vb + k * QS) - delta);
          axpy_chunk<DK>(ds, kb + k * QS, dq);
        }
      }
      st_chunk<DK>(Gs + r * PS + h * DK, dq, scale);
    }
    __syncthreads();
    // B: columns k.  dK_k = c sum_m ds_mk Q_m, dV_k = sum_m a_mk dO_m
    for (int item = threadIdx.x; item < G * H * F; item += kThreads) {
      const int gh = item / F, k = item - gh * F, g = gh / H, h = gh - g * H;
      const int r = g * F + k;
      float dk[DK], dv[DK];
#pragma unroll
      for (int j = 0; j < DK; ++j) dk[j] = dv[j] = 0.f;
      if (base + g < B) {
        const float *qb = Ps + g * F * QS + h * DK, *ob = Gs + g * F * PS + 3 * HD + h * DK;
        const float *sb = st + 3 * (gh * F);
        float kk[DK], vv[DK];
        ld_chunk<DK>(Ps + r * QS + HD + h * DK, kk);
        ld_chunk<DK>(Ps + r * QS + 2 * HD + h * DK, vv);
        for (int m = 0; m < F; ++m) {
          const float a = expf(dot_chunk<DK>(kk, qb + m * QS) * scale - sb[3 * m]) * sb[3 * m + 1];
          const float ds = a * (dot_chunk<DK>(vv, ob + m * PS) - sb[3 * m + 2]);
          axpy_chunk<DK>(ds, qb + m * QS, dk);
          axpy_chunk<DK>(a, ob + m * PS, dv);
        }
      }
      st_chunk<DK>(Gs + r * PS + HD + h * DK, dk, scale);
      st_chunk<DK>(Gs + r * PS + 2 * HD + h * DK, dv, 1.f);
    }
    __syncthreads();
    // C1: d[Wq|Wk|Wv|Wr] += X^T [dQ|dK|dV|dP], rows ascending
    if (ig < Din) {
      for (int r = 0; r < RP; ++r) {
        const float4 gv = ld4(Gs + r * PS + 4 * jg);
#pragma unroll
        for (int n = 0; n < NI; ++n) fma4(acc[n], Xs[r * XS + ig + IT * n], gv);
      }
    }
    __syncthreads();
    // C2: dX = [dQ|dK|dV|dP] Ws^T, into X's place
    {
      const int d4 = Din / 4;
      for (int u = threadIdx.x; u < R * d4; u += kThreads) {
        const int i4 = u / R, r = u - i4 * R;
        const float *gr = Gs + r * PS, *w = Ws + 4 * i4 * NC;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < ncg; j += 4) {
          const float4 gv = ld4(gr + j);
          o.x = dot4(gv, ld4(w + j), o.x);
          o.y = dot4(gv, ld4(w + NC + j), o.y);
          o.z = dot4(gv, ld4(w + 2 * NC + j), o.z);
          o.w = dot4(gv, ld4(w + 3 * NC + j), o.w);
        }
        st4(Xs + r * XS + 4 * i4, o);
      }
    }
    __syncthreads();
    {
      const int d4 = Din / 4;
      for (int q = threadIdx.x; q < R * d4; q += kThreads) {
        const int r = q / d4, c = q - r * d4;
        if (base * F + r >= rows_total) break;
        float4 o = ld4(Xs + r * XS + 4 * c);
        const int64_t at = (base * F + r) * Din + 4 * c;
        if (dX_up != nullptr) {
          const float4 up = ld4(dX_up + at);
          o.x += up.x; o.y += up.y; o.z += up.z; o.w += up.w;
        }
        st4(dX + at, o);
      }
    }
  }
  if (ig < Din) {
    float *out = part + (int64_t)blockIdx.x * Din * NC;
#pragma unroll
    for (int n = 0; n < NI; ++n) st4(out + (ig + IT * n) * NC + 4 * jg, acc[n]);
  }
}

// fixed-order sum of per-block partials, first stage: segment s adds its blocks for every element
__global__ void autoint_seg_kernel(const float *__restrict__ part, int nblk, int n, float *__restrict__ seg) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int per = (nblk + kSeg - 1) / kSeg, k0 = blockIdx.y * per, k1 = min(nblk, k0 + per);
  float s = 0.f;
  for (int k = k0; k < k1; ++k) s += part[(int64_t)k * n + e];
  seg[(int64_t)blockIdx.y * n + e] = s;
}
// second stage of the layer: segments in order -> dWq, dWk, dWv, dWr [Din][HD]
__global__ void autoint_finish_kernel(const float *__restrict__ seg, int Din, int HD, float *__restrict__ dWq,
                                      float *__restrict__ dWk, float *__restrict__ dWv, float *__restrict__ dWr) {
  const int n = Din * 4 * HD, e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int k = 0; k < kSeg; ++k) s += seg[(int64_t)k * n + e];
  const int i = e / (4 * HD), c = e - i * 4 * HD, blk = c / HD, j = c - blk * HD;
  float *dst = blk == 0 ? dWq : (blk == 1 ? dWk : (blk == 2 ? dWv : dWr));
  if (dst != nullptr) dst[i * HD + j] = s;
}

// ---------------------------------------------------------------------------------------- the last projection
// logit[b] = Y[b,:] . w + w0: one wave per example, lane-strided partial sums, butterfly
__global__ __launch_bounds__(kThreads) void autoint_head_fwd_kernel(const float *__restrict__ Y,
                                                                    const float *__restrict__ w,
                                                                    const float *__restrict__ w0, int64_t B, int K,
                                                                    float *__restrict__ logit) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t b = (int64_t)blockIdx.x * 4 + wv; b < B; b += (int64_t)gridDim.x * 4) {
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s = fmaf(Y[b * K + k], w[k], s);
    s = rm_wave_sum(s);
    if (lane == 0) logit[b] = s + w0[0];
  }
}
// dY[b,:] = g[b] w;  per-block partials of dw = sum_b g[b] Y[b,:] and dw0 = sum_b g[b] (element K), b ascending
__global__ __launch_bounds__(kThreads) void autoint_head_bwd_kernel(const float *__restrict__ Y,
                                                                    const float *__restrict__ w,
                                                                    const float *__restrict__ g, int64_t B, int K,
                                                                    float *__restrict__ dY,
                                                                    float *__restrict__ part) {
  const int64_t chunk = (B + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = blockIdx.x * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
  float *out = part + (int64_t)blockIdx.x * (K + 1);
  for (int k = threadIdx.x; k <= K; k += kThreads) {
    float s = 0.f;
    if (k < K) {
      const float wk = w[k];
      for (int64_t b = b0; b < b1; ++b) {
        const float gb = g[b];
        dY[b * K + k] = gb * wk;
        s = fmaf(gb, Y[b * K + k], s);
      }
    } else {
      for (int64_t b = b0; b < b1; ++b) s += g[b];
    }
    out[k] = s;
  }
}

int ai_check(const char *fn, int64_t B, int F, int Din, int H, int dk) {
  RM_REQUIRE(B >= 0 && B < ((int64_t)1 << 40), "%s: bad batch size", fn);
  RM_REQUIRE(ai_ok(F, Din, H, dk),
             "%s: F=%d Din=%d H=%d dk=%d unsupported (1 <= F <= %d, Din in {8,16,32,64}, H in {1,2,4,8}, dk >= 4, "
             "H dk in {8,16,32,64})", fn, F, Din, H, dk, kMaxF);
  return RM_OK;
}

}  // namespace

extern "C" int rm_autoint_supported(int F, int Din, int H, int dk) { return ai_ok(F, Din, H, dk) ? 1 : 0; }

extern "C" int64_t rm_autoint_stats_floats(int64_t B, int F, int H) {
  return B < 0 || F < 1 || H < 1 ? 0 : 2 * B * F * H;
}

extern "C" int rm_autoint_layer_fwd(const float *X, const float *Wq, const float *Wk, const float *Wv,
                                    const float *Wr, int64_t B, int F, int Din, int H, int dk, float scale,
                                    float *Y, float *stats, rm_stream_t stream) {
  int rc = ai_check("rm_autoint_layer_fwd", B, F, Din, H, dk);
  if (rc != RM_OK) return rc;
  if (B == 0) return RM_OK;
  RM_REQUIRE(X && Wq && Wk && Wv && Y, "rm_autoint_layer_fwd: NULL argument");
  RM_REQUIRE(rm_aligned16(X) && rm_aligned16(Wq) && rm_aligned16(Wk) && rm_aligned16(Wv) && rm_aligned16(Wr) &&
                 rm_aligned16(Y),
             "rm_autoint_layer_fwd: X, the weights and Y must be 16-byte aligned");
  const int HD = H * dk, G = ai_pick_g(F, Din, H, HD, false);
  const size_t smem = (size_t)ai_fwd_floats(G, F, Din, HD) * sizeof(float);
  dim3 grid(rm_grid_cap((B + G - 1) / G, 256 * 8));
  hipStream_t st = (hipStream_t)stream;
#define RM_AI_FWD(DK_)                                                                                          \
  rm_launch_lds(autoint_fwd_kernel<DK_>, grid, dim3(kThreads), smem, st, X, Wq, Wk, Wv, Wr, B, F, Din, H, G, scale, Y, \
                stats)
  switch (dk) {
    case 4: RM_AI_FWD(4); break;
    case 8: RM_AI_FWD(8); break;
    case 16: RM_AI_FWD(16); break;
    case 32: RM_AI_FWD(32); break;
    default: RM_AI_FWD(64); break;
  }
#undef RM_AI_FWD
  RM_CHECK_LAUNCH("rm_autoint_layer_fwd");
  return RM_OK;
}

extern "C" int64_t rm_autoint_layer_bwd_workspace(int64_t B, int F, int Din, int H, int dk) {
  if (!ai_ok(F, Din, H, dk) || B < 0) return 0;
  const int HD = H * dk;
  return ((int64_t)ai_bwd_blocks(B, F, Din, H, HD) + kSeg) * Din * 4 * HD;
}

extern "C" int rm_autoint_layer_bwd(const float *X, const float *Wq, const float *Wk, const float *Wv,
                                    const float *Wr, const float *Y, const float *stats, const float *dY, int64_t B,
                                    int F, int Din, int H, int dk, float scale, float *dX, const float *dX_up,
                                    float *dWq, float *dWk, float *dWv, float *dWr, float *workspace,
                                    rm_stream_t stream) {
  int rc = ai_check("rm_autoint_layer_bwd", B, F, Din, H, dk);
  if (rc != RM_OK) return rc;
  RM_REQUIRE(Wq && Wk && Wv && dWq && dWk && dWv && workspace, "rm_autoint_layer_bwd: NULL argument");
  RM_REQUIRE((Wr == nullptr) == (dWr == nullptr), "rm_autoint_layer_bwd: Wr and dWr go together");
  RM_REQUIRE(B == 0 || (X && Y && stats && dY && dX), "rm_autoint_layer_bwd: NULL argument");
  RM_REQUIRE(rm_aligned16(X) && rm_aligned16(Wq) && rm_aligned16(Wk) && rm_aligned16(Wv) && rm_aligned16(Wr) &&
                 rm_aligned16(Y) && rm_aligned16(dY) && rm_aligned16(dX) && rm_aligned16(dX_up) &&
                 rm_aligned16(workspace),
             "rm_autoint_layer_bwd: X, the weights, Y, dY, dX, dX_up and workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int HD = H * dk, n = Din * 4 * HD;
  const int nblk = B == 0 ? 0 : ai_bwd_blocks(B, F, Din, H, HD);
  float *part = workspace, *seg = workspace + (int64_t)nblk * n;
  if (B > 0) {
    const int G = ai_pick_g(F, Din, H, HD, true);
    const size_t smem = (size_t)ai_bwd_floats(G, F, Din, H, HD) * sizeof(float);
    const int NI = Din * HD >= kThreads ? Din * HD / kThreads : 1;
    dim3 grid(nblk);
#define RM_AI_BWD(DK_, NI_)                                                                                        \
  rm_launch_lds(autoint_bwd_kernel<DK_, NI_>, grid, dim3(kThreads), smem, st, X, Wq, Wk, Wv, Wr, Y, stats, dY, B, F, \
                Din, H, G, scale, dX, dX_up, part)
#define RM_AI_BWD_N(DK_)                     \
  switch (NI) {                              \
    case 1: RM_AI_BWD(DK_, 1); break;        \
    case 2: RM_AI_BWD(DK_, 2); break;        \
    case 4: RM_AI_BWD(DK_, 4); break;        \
    case 8: RM_AI_BWD(DK_, 8); break;        \
    default: RM_AI_BWD(DK_, 16); break;      \
  }
    switch (dk) {
      case 4: RM_AI_BWD_N(4); break;
      case 8: RM_AI_BWD_N(8); break;
      case 16: RM_AI_BWD_N(16); break;
      case 32: RM_AI_BWD_N(32); break;
      default: RM_AI_BWD_N(64); break;
    }
#undef RM_AI_BWD_N
#undef RM_AI_BWD
    RM_CHECK_LAUNCH("rm_autoint_layer_bwd");
  }
  hipLaunchKernelGGL(autoint_seg_kernel, dim3((n + 255) / 256, kSeg), dim3(256), 0, st, part, nblk, n, seg);
  hipLaunchKernelGGL(autoint_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, st, seg, Din, HD, dWq, dWk, dWv,
                     dWr);
  RM_CHECK_LAUNCH("rm_autoint_layer_bwd (finish)");
  return RM_OK;
}

extern "C" int rm_autoint_head_fwd(const float *Y, const float *w, const float *w0, int64_t B, int K, float *logit,
                                   rm_stream_t stream) {
  RM_REQUIRE(B >= 0 && K >= 1, "rm_autoint_head_fwd: bad size");
  if (B == 0) return RM_OK;
  RM_REQUIRE(Y && w && w0 && logit, "rm_autoint_head_fwd: NULL argument");
  hipLaunchKernelGGL(autoint_head_fwd_kernel, dim3(rm_grid_cap((B + 3) / 4, 256 * 16)), dim3(kThreads), 0,
                     (hipStream_t)stream, Y, w, w0, B, K, logit);
  RM_CHECK_LAUNCH("rm_autoint_head_fwd");
  return RM_OK;
}

extern "C" int64_t rm_autoint_head_bwd_workspace(int64_t B, int K) {
  if (B < 0 || K < 1) return 0;
  return ((int64_t)ai_head_blocks(B) + kSeg) * (K + 1);
}

extern "C" int rm_autoint_head_bwd(const float *Y, const float *w, const float *g, int64_t B, int K, float *dY,
                                   float *dw, float *dw0, float *workspace, rm_stream_t stream) {
  RM_REQUIRE(B >= 0 && K >= 1, "rm_autoint_head_bwd: bad size");
  RM_REQUIRE(w && dw && dw0 && workspace, "rm_autoint_head_bwd: NULL argument");
  RM_REQUIRE(B == 0 || (Y && g && dY), "rm_autoint_head_bwd: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = B == 0 ? 0 : ai_head_blocks(B), n = K + 1;
  float *part = workspace, *seg = workspace + (int64_t)nblk * n;
  if (B > 0) {
    hipLaunchKernelGGL(autoint_head_bwd_kernel, dim3(nblk), dim3(kThreads), 0, st, Y, w, g, B, K, dY, part);
    RM_CHECK_LAUNCH("rm_autoint_head_bwd");
  }
  hipLaunchKernelGGL(autoint_seg_kernel, dim3((n + 255) / 256, kSeg), dim3(256), 0, st, part, nblk, n, seg);
  rm_sum_partials(seg, kSeg, n, rm_sum_dsts(dw, K, dw0, 1), st);  // the segments, in order
  RM_CHECK_LAUNCH("rm_autoint_head_bwd (finish)");
  return RM_OK;
}
