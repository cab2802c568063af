// Two-tower retrieval: the in-batch softmax loss over the score matrix S = scale U V^T - logq, forward and backward,
// and the row normalisation of the tower outputs (see recman_hip.h).  Nothing in the reference implements them.
//
// S, the softmax P and its gradient G [B, B] never reach HBM: the forward keeps (max, sum, rank) per row, the backward
// recomputes S from U, V and the saved lse.  One kernel template serves the three passes:
//   MODE 0  forward      own = 64 rows of U,  streamed = tiles of V   -> per row (max, sum, rank) of its columns
//   MODE 1  backward dU  own = 64 rows of U,  streamed = tiles of V   -> dU of the own rows
//   MODE 2  backward dV  own = 64 rows of V,  streamed = tiles of U   -> dV of the own rows
// A block is 4 waves, a wave owns 16 rows.  The own rows sit in registers as the B operand of the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32: lane l holds X[own = l & 15][k = 4 kk + (l >> 4)] for k-step kk), the streamed operand goes
// through LDS in tiles of COLS rows, double-buffered: the next tile's global loads are in flight while this one is
// multiplied, one barrier per tile.  The tile is computed TRANSPOSED, T = Y_tile X^T: accumulator register r of lane l
// holds (streamed = 4 (l >> 4) + r, own = l & 15).  So
//   - the reductions over the streamed index (max, sum, rank) are in-lane over registers and tiles; the four lane
//     groups of a row are combined once at the end (two shuffles);
//   - the register is, as it stands, the A operand (row = own = l & 15, k = l >> 4) of the second product
//     dOwn = G Y if step r's B operand supplies Y[4 (l >> 4) + r]: the reduction index is permuted, nothing moves.
// LDS rows are padded to HP + 4 floats (HP = H rounded up to the template's width, zero-filled): both operand reads
// (16 rows x 4 columns, 4 rows x 16 columns) then touch 64 different banks.
// Column splits: grid.y blocks share a row tile's streamed range.  The forward's partial (max, sum, rank) triples are
// combined in split order by the finish pass, the backward's partial sums by a sum pass in split order (one split
// writes its rows directly).  No atomics; loss and W are fixed-order two-stage sums in double: two runs with the same
// split count are bit-equal.
#include "rm_launch.h"

#include <math.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kRows = 64;        // own rows per block (4 waves x 16)
constexpr int kThreads = 256;
constexpr int kMaxSplits = 8;
constexpr int kFinBlocks = 256;  // blocks of the finish / weight-sum passes (their partials are summed by one block)
constexpr int kFinThreads = 256;
constexpr int kMinH = 4, kMaxH = 256;
constexpr int kFillBlocks = 512;  // the library's split choice aims at two blocks on each of the 256 CUs

// the template width (k-steps of 4) that holds H: HP = 4 NK is a multiple of 16
inline int ibs_nk(int H) {
  const int widths[] = {4, 8, 12, 16, 24, 32, 48, 64};
  for (int nk : widths)
    if (4 * nk >= H) return nk;
  return -1;
}
inline int ibs_cols(int nk) { return 4 * nk <= 128 ? 64 : 32; }
inline int64_t ibs_tiles(int64_t B, int cols) { return (B + cols - 1) / cols; }

inline int ibs_splits(int64_t B, int cols, int col_splits) {
  const int64_t tiles = ibs_tiles(B, cols);
  int64_t s = col_splits;
  if (s == 0) {
    const int64_t row_tiles = (B + kRows - 1) / kRows;
    s = (kFillBlocks + row_tiles - 1) / row_tiles;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s > tiles) s = tiles;
  }
  return (int)(s < 1 ? 1 : s);
}

// workspace, in floats: [0] doubles (2 kFinBlocks partial pairs, then W), then diag [B], and per split max [S B],
// sum [S B], rank [S B] (int32); the backward's partial rows [S, B, H] follow
constexpr int64_t kWsDoubles = 2 * kFinBlocks + 2;
inline int64_t ibs_round4(int64_t n) { return (n + 3) / 4 * 4; }
struct IbsWs {
  double *dbl;
  float *diag, *pm, *ps;
  int *pr;
  float *rows;
};
inline IbsWs ibs_ws(float *ws, int64_t B) {
  IbsWs w;
  w.dbl = reinterpret_cast<double *>(ws);
  const int64_t b4 = ibs_round4(B);
  w.diag = ws + 2 * kWsDoubles;
  w.pm = w.diag + b4;
  w.ps = w.pm + kMaxSplits * b4;
  w.pr = reinterpret_cast<int *>(w.ps + kMaxSplits * b4);
  w.rows = w.ps + 2 * kMaxSplits * b4;
  return w;
}

struct IbsArgs {
  const float *X;  // own operand [B, ldx]
  int64_t ldx;
  const float *Y;  // streamed operand [B, ldy]
  int64_t ldy;
  const int64_t *ids;  // or NULL
  const float *logq;   // or NULL
  const float *w;      // or NULL
  const float *lse;    // backward
  const double *Wsum;  // backward, w != NULL: the sum of w
  float scale, coef;   // coef = scale * grad_scale (the backward's row factor is coef * w_i / W)
  int B, H;
  int tiles_per_split;
  // MODE 0: per split max / sum / rank, and diag
  float *pm, *ps, *diag;
  int *pr;
  int64_t pstride;
  // MODE 1 / 2: the own rows' gradient (or this split's partial rows)
  float *dOwn;
  int64_t lddo;
  int64_t dsplit;  // floats between two splits' rows (0: one split, written in place)
};

template <int NK, int MODE>
__global__ __launch_bounds__(kThreads, 2) void ibs_kernel(IbsArgs a) {
  constexpr int HP = 4 * NK, LDV = HP + 4, COLS = HP <= 128 ? 64 : 32;
  constexpr int NPF = COLS * NK / kThreads;  // float4 loads per thread and tile
  constexpr int NH = HP / 16;
  extern __shared__ float smem[];
  // LDS: two tiles, then per buffer logq_j (MODE 0 / 1) or lse_i (MODE 2), the row factor c_i (MODE 2), the ids
  float *const tiles = smem, *const sa = smem + 2 * COLS * LDV, *const sb = sa + 2 * COLS;
  int64_t *const sid = reinterpret_cast<int64_t *>(sb + 2 * COLS);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
  const int B = a.B, H = a.H;
  const int own = blockIdx.x * kRows + wave * 16 + lo;
  const bool own_ok = own < B;
  const bool has_id = a.ids != nullptr;
  const int t0 = blockIdx.y * a.tiles_per_split;
  const int ntiles = (B + COLS - 1) / COLS;
  const int t1 = min(t0 + a.tiles_per_split, ntiles);

  float inv_w = 0.f;  // MODE 1 / 2: coef / W (0 when W == 0)
  if (MODE != 0) {
    const double W = a.w ? a.Wsum[0] : (double)B;
    inv_w = W > 0.0 ? (float)((double)a.coef / W) : 0.f;
  }

  // the own rows as B operands
  float x[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
    const int c = 4 * kk + hi;
    x[kk] = (own_ok && c < H) ? a.X[(int64_t)own * a.ldx + c] : 0.f;
  }
  const int64_t own_id = (has_id && own_ok) ? a.ids[own] : 0;
  // per own row: MODE 0 the diagonal score, MODE 1 lse_i and c_i, MODE 2 logq_j
  float own_a = 0.f, own_c = 0.f;
  if (MODE == 0) {
    // S_ii by the same instruction chain as the tile: the 16 own rows against themselves, the diagonal picked out
    // (x is +0.0 past H and for rows past B: there the load is clamped onto an element of the range, not masked)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float *yrow = a.Y + (int64_t)(own_ok ? own : 0) * a.ldy;
#pragma unroll
    for (int kk = 0; kk < NK; ++kk)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(yrow[min(4 * kk + hi, H - 1)], x[kk], acc, 0, 0, 0);
    // row own = lo sits in lane group lo >> 2, register lo & 3
    const int r = lo & 3;
    const float mine = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    const float d = __shfl(mine, (lo >> 2) * 16 + lo, 64);
    own_a = a.scale * d - ((a.logq && own_ok) ? a.logq[own] : 0.f);
    if (blockIdx.y == 0 && own_ok && hi == 0) a.diag[own] = own_a;
  } else if (MODE == 1) {
    own_a = own_ok ? a.lse[own] : 0.f;
    own_c = own_ok ? (a.w ? a.w[own] : 1.f) * inv_w : 0.f;
  } else {
    own_a = (a.logq && own_ok) ? a.logq[own] : 0.f;
  }

  float m = -INFINITY, s = 0.f;
  int rank = 0;
  f32x4 dacc[MODE == 0 ? 1 : NH];
  if (MODE != 0) {
#pragma unroll
    for (int hc = 0; hc < NH; ++hc) dacc[hc] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // the prefetch registers of one tile
  float4 pf[NPF];
  float pa = 0.f, pb = 0.f;
  int64_t pid = 0;
  auto fetch = [&](int t) {
#pragma unroll
    for (int p = 0; p < NPF; ++p) {
      const int q = tid + kThreads * p, row = q / NK, c4 = q % NK;
      const int g = t * COLS + row;
      pf[p] = (g < B && 4 * c4 < H) ? *reinterpret_cast<const float4 *>(a.Y + (int64_t)g * a.ldy + 4 * c4)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid < COLS) {
      const int g = t * COLS + tid;
      const bool ok = g < B;
      if (MODE == 2) {
        pa = ok ? a.lse[g] : 0.f;
        pb = ok ? (a.w ? a.w[g] : 1.f) * inv_w : 0.f;
      } else {
        pa = (ok && a.logq) ? a.logq[g] : 0.f;
      }
      pid = (ok && has_id) ? a.ids[g] : 0;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int p = 0; p < NPF; ++p) {
      const int q = tid + kThreads * p, row = q / NK, c4 = q % NK;
      *reinterpret_cast<float4 *>(tiles + buf * (COLS * LDV) + row * LDV + 4 * c4) = pf[p];
    }
    if (tid < COLS) {
      sa[buf * COLS + tid] = pa;
      sb[buf * COLS + tid] = pb;
      sid[buf * COLS + tid] = pid;
    }
  };

  if (t0 < t1) {
    fetch(t0);
    stash(0);
  }
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    if (t + 1 < t1) fetch(t + 1);
    const float *ys = tiles + buf * (COLS * LDV);
#pragma unroll 1
    for (int sub = 0; sub < COLS / 16; sub += 2) {
      // two 16-row sub-tiles of the streamed operand: two independent accumulator chains
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const float *y0 = ys + (sub * 16 + lo) * LDV + hi, *y1 = y0 + 16 * LDV;
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y0[4 * kk], x[kk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y1[4 * kk], x[kk], acc1, 0, 0, 0);
      }
      float v[8];
      bool ok[8], diag[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int sl = (sub + (q >> 2)) * 16 + 4 * hi + (q & 3);  // the streamed row inside the tile
        const int g = t * COLS + sl;
        const float raw = q < 4 ? acc0[q & 3] : acc1[q & 3];
        diag[q] = g == own;
        ok[q] = g < B && own_ok && (diag[q] || !has_id || sid[buf * COLS + sl] != own_id);
        if (MODE == 2) {
          // own = j, streamed = i
          const float S = a.scale * raw - own_a;
          const float p = ok[q] ? expf(S - sa[buf * COLS + sl]) : 0.f;
          v[q] = sb[buf * COLS + sl] * (p - (diag[q] ? 1.f : 0.f));
        } else {
          const float S = a.scale * raw - sa[buf * COLS + sl];
          if (MODE == 0) {
            v[q] = S;
          } else {
            const float p = ok[q] ? expf(S - own_a) : 0.f;
            v[q] = own_c * (p - (diag[q] ? 1.f : 0.f));
          }
        }
      }
      if (MODE == 0) {
        float tm = -INFINITY;
#pragma unroll
        for (int q = 0; q < 8; ++q) tm = ok[q] ? fmaxf(tm, v[q]) : tm;
        if (tm > -INFINITY) {
          const float mn = fmaxf(m, tm);
          float add = 0.f;
#pragma unroll
          for (int q = 0; q < 8; ++q) add += ok[q] ? expf(v[q] - mn) : 0.f;
          s = s * expf(m - mn) + add;
          m = mn;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) rank += (ok[q] && !diag[q] && v[q] > own_a) ? 1 : 0;
      } else {
        // dOwn += G Y: the accumulator registers are the A operand as they stand
        const float *b0 = ys + (sub * 16 + 4 * hi) * LDV + lo, *b1 = b0 + 16 * LDV;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int hc = 0; hc < NH; ++hc)
            dacc[hc] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[r], b0[r * LDV + 16 * hc], dacc[hc], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int hc = 0; hc < NH; ++hc)
            dacc[hc] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[4 + r], b1[r * LDV + 16 * hc], dacc[hc], 0, 0, 0);
        }
      }
    }
    if (t + 1 < t1) stash(buf ^ 1);
    __syncthreads();
  }

  if (MODE == 0) {
    // the four lane groups of a row, then one lane writes the split's triple
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float mo = __shfl_xor(m, o, 64), so = __shfl_xor(s, o, 64);
      rank += __shfl_xor(rank, o, 64);
      const float mn = fmaxf(m, mo);
      const float mine = m > -INFINITY ? s * expf(m - mn) : 0.f, other = mo > -INFINITY ? so * expf(mo - mn) : 0.f;
      s = mine + other;
      m = mn;
    }
    if (own_ok && hi == 0) {
      const int64_t o = (int64_t)blockIdx.y * a.pstride + own;
      a.pm[o] = m;
      a.ps[o] = s;
      a.pr[o] = rank;
    }
  } else {
    float *dst = a.dOwn + (int64_t)blockIdx.y * a.dsplit;
    const int row0 = blockIdx.x * kRows + wave * 16 + 4 * hi;
#pragma unroll
    for (int hc = 0; hc < NH; ++hc) {
      const int c = 16 * hc + lo;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row0 + r < B && c < H) dst[(int64_t)(row0 + r) * a.lddo + c] = dacc[hc][r];
    }
  }
}

template <int NK>
constexpr size_t ibs_lds() {
  constexpr int HP = 4 * NK, LDV = HP + 4, COLS = HP <= 128 ? 64 : 32;
  return (size_t)(2 * COLS * LDV + 4 * COLS) * sizeof(float) + (size_t)2 * COLS * sizeof(int64_t);
}

template <int NK>
void ibs_launch_nk(int mode, dim3 grid, hipStream_t st, const IbsArgs &a) {
  if (mode == 0) rm_launch_lds(ibs_kernel<NK, 0>, grid, dim3(kThreads), ibs_lds<NK>(), st, a);
  else if (mode == 1) rm_launch_lds(ibs_kernel<NK, 1>, grid, dim3(kThreads), ibs_lds<NK>(), st, a);
  else rm_launch_lds(ibs_kernel<NK, 2>, grid, dim3(kThreads), ibs_lds<NK>(), st, a);
}

void ibs_launch(int nk, int mode, dim3 grid, hipStream_t st, const IbsArgs &a) {
  switch (nk) {
    case 4: ibs_launch_nk<4>(mode, grid, st, a); break;
    case 8: ibs_launch_nk<8>(mode, grid, st, a); break;
    case 12: ibs_launch_nk<12>(mode, grid, st, a); break;
    case 16: ibs_launch_nk<16>(mode, grid, st, a); break;
    case 24: ibs_launch_nk<24>(mode, grid, st, a); break;
    case 32: ibs_launch_nk<32>(mode, grid, st, a); break;
    case 48: ibs_launch_nk<48>(mode, grid, st, a); break;
    default: ibs_launch_nk<64>(mode, grid, st, a); break;
  }
}

// fixed order: a butterfly inside the wave, the waves in index order; thread 0 gets the block's sums
__device__ __forceinline__ void block_sum2(double &a, double &b, double *sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sm[2 * (threadIdx.x >> 6)] = a;
    sm[2 * (threadIdx.x >> 6) + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0.0;
    b = 0.0;
    for (int w = 0; w < kFinThreads / 64; ++w) {
      a += sm[2 * w];
      b += sm[2 * w + 1];
    }
  }
}

// finish, stage 1: the splits' triples of a row in split order -> lse, row_loss, rank; per block the sums of
// w_i l_i and w_i in double
__global__ __launch_bounds__(kFinThreads) void ibs_finish_kernel(const float *__restrict__ pm,
                                                                 const float *__restrict__ ps,
                                                                 const int *__restrict__ pr, int64_t pstride,
                                                                 const float *__restrict__ diag,
                                                                 const float *__restrict__ w, int B, int splits,
                                                                 float *__restrict__ lse, float *__restrict__ row_loss,
                                                                 int *__restrict__ rank, double *__restrict__ part) {
  __shared__ double sm[2 * kFinThreads / 64];
  double sl = 0.0, sw = 0.0;
  for (int i = blockIdx.x * kFinThreads + threadIdx.x; i < B; i += gridDim.x * kFinThreads) {
    float M = -INFINITY;
    for (int q = 0; q < splits; ++q) M = fmaxf(M, pm[q * pstride + i]);
    float sum = 0.f;
    int rk = 0;
    for (int q = 0; q < splits; ++q) {
      const float mq = pm[q * pstride + i];
      if (mq > -INFINITY) sum += ps[q * pstride + i] * expf(mq - M);
      rk += pr[q * pstride + i];
    }
    const float l = M + logf(sum);
    const float rl = l - diag[i];
    lse[i] = l;
    row_loss[i] = rl;
    if (rank) rank[i] = rk;
    const float wi = w ? w[i] : 1.f;
    sl += (double)wi * (double)rl;
    sw += (double)wi;
  }
  block_sum2(sl, sw, sm);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = sl;
    part[2 * blockIdx.x + 1] = sw;
  }
}

// per block the sum of w_i in double (the backward's W)
__global__ __launch_bounds__(kFinThreads) void ibs_wsum_kernel(const float *__restrict__ w, int B,
                                                               double *__restrict__ part) {
  __shared__ double sm[2 * kFinThreads / 64];
  double sw = 0.0, zero = 0.0;
  for (int i = blockIdx.x * kFinThreads + threadIdx.x; i < B; i += gridDim.x * kFinThreads) sw += (double)w[i];
  block_sum2(zero, sw, sm);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = 0.0;
    part[2 * blockIdx.x + 1] = sw;
  }
}

// stage 2, one block: the blocks' partials in block order; loss = sum w l / W (W == 0: 0), W kept for the backward
__global__ __launch_bounds__(kFinThreads) void ibs_total_kernel(const double *__restrict__ part, int nblk,
                                                                float *__restrict__ loss, double *__restrict__ Wout) {
  __shared__ double sm[2 * kFinThreads / 64];
  double sl = 0.0, sw = 0.0;
  for (int i = threadIdx.x; i < nblk; i += kFinThreads) {
    sl += part[2 * i];
    sw += part[2 * i + 1];
  }
  block_sum2(sl, sw, sm);
  if (threadIdx.x == 0) {
    if (loss) loss[0] = sw > 0.0 ? (float)(sl / sw) : 0.f;
    Wout[0] = sw;
  }
}

// dst[i, :H] = the splits' partial rows summed in split order
__global__ __launch_bounds__(256) void ibs_sum_rows_kernel(const float *__restrict__ part, int64_t dsplit, int splits,
                                                           int B, int H, float *__restrict__ dst, int64_t ldd) {
  const int h4 = H >> 2;
  const int64_t n = (int64_t)B * h4;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q / h4;
    const int c = (int)(q % h4) * 4;
    float4 acc = *reinterpret_cast<const float4 *>(part + i * H + c);
    for (int sp = 1; sp < splits; ++sp) {
      const float4 v = *reinterpret_cast<const float4 *>(part + sp * dsplit + i * H + c);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4 *>(dst + i * ldd + c) = acc;
  }
}

// ------------------------------------------------------------------------------------------------ row normalisation
// a group of 16 lanes per row, 16-byte column vectors; the squared norm and <Y, dY> in double, summed by a butterfly
__global__ __launch_bounds__(256) void rownorm_fwd_kernel(const float *__restrict__ X, int64_t ldx, int64_t B, int H,
                                                          float eps, float *__restrict__ Y, int64_t ldy,
                                                          float *__restrict__ inv_norm) {
  const int li = threadIdx.x & 15, h4 = H >> 2;
  const int64_t groups = (int64_t)gridDim.x * 16;
  const int64_t rounds = (B + groups - 1) / groups;
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const int64_t b = rd * groups + (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = b < B;
    double ss = 0.0;
    if (live)
      for (int c = li; c < h4; c += 16) {
        const float4 v = *reinterpret_cast<const float4 *>(X + b * ldx + 4 * c);
        ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
      }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float inv = 1.0f / fmaxf((float)sqrt(ss), eps);
    if (live) {
      for (int c = li; c < h4; c += 16) {
        float4 v = *reinterpret_cast<const float4 *>(X + b * ldx + 4 * c);
        v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
        *reinterpret_cast<float4 *>(Y + b * ldy + 4 * c) = v;
      }
      if (li == 0) inv_norm[b] = inv;
    }
  }
}

__global__ __launch_bounds__(256) void rownorm_bwd_kernel(const float *__restrict__ Y, int64_t ldy,
                                                          const float *__restrict__ inv_norm, const float *dY,
                                                          int64_t lddy, int64_t B, int H, float *dX, int64_t lddx) {
  const int li = threadIdx.x & 15, h4 = H >> 2;
  const int64_t groups = (int64_t)gridDim.x * 16;
  const int64_t rounds = (B + groups - 1) / groups;
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const int64_t b = rd * groups + (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = b < B;
    double dot = 0.0;
    if (live)
      for (int c = li; c < h4; c += 16) {
        const float4 y = *reinterpret_cast<const float4 *>(Y + b * ldy + 4 * c);
        const float4 g = *reinterpret_cast<const float4 *>(dY + b * lddy + 4 * c);
        dot += (double)y.x * g.x + (double)y.y * g.y + (double)y.z * g.z + (double)y.w * g.w;
      }
    // every lane of the row has read its dY before the first write below (dX may alias dY): the butterfly joins them
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (live) {
      const float d = (float)dot, inv = inv_norm[b];
      for (int c = li; c < h4; c += 16) {
        const float4 y = *reinterpret_cast<const float4 *>(Y + b * ldy + 4 * c);
        float4 g = *reinterpret_cast<const float4 *>(dY + b * lddy + 4 * c);
        g.x = inv * (g.x - y.x * d); g.y = inv * (g.y - y.y * d);
        g.z = inv * (g.z - y.z * d); g.w = inv * (g.w - y.w * d);
        *reinterpret_cast<float4 *>(dX + b * lddx + 4 * c) = g;
      }
    }
  }
}

#define IBS_LIMITS "H a multiple of 4 in 4..256, pointers 16-byte aligned, row strides multiples of 4 floats and >= H, " \
                   "col_splits 0..8"

int ibs_operand(const char *fn, const char *name, const void *p, int64_t ld, int H) {
  RM_REQUIRE(p != nullptr, "%s: %s is NULL", fn, name);
  RM_REQUIRE(ld >= H, "%s: row stride of %s = %lld < H = %d (limits: " IBS_LIMITS ")", fn, name, (long long)ld, H);
  RM_REQUIRE(ld % 4 == 0 && rm_aligned16(p) && ld <= kRmMaxStride,
             "%s: %s must be 16-byte aligned with a row stride that is a multiple of 4 floats (got stride %lld; "
             "limits: " IBS_LIMITS ")", fn, name, (long long)ld);
  return RM_OK;
}

int ibs_check(const char *fn, int64_t B, int H, int col_splits) {
  RM_REQUIRE(rm_inbatch_softmax_supported(H), "%s: H=%d unsupported (limits: " IBS_LIMITS ")", fn, H);
  RM_REQUIRE(B >= 0 && B < ((int64_t)1 << 30), "%s: bad B=%lld (0 <= B < 2^30)", fn, (long long)B);
  RM_REQUIRE(col_splits >= 0 && col_splits <= kMaxSplits, "%s: col_splits=%d out of range (limits: " IBS_LIMITS ")",
             fn, col_splits);
  return RM_OK;
}

int fin_blocks(int64_t B) { return rm_grid_cap((B + kFinThreads - 1) / kFinThreads, kFinBlocks); }

}  // namespace

extern "C" int rm_inbatch_softmax_supported(int H) { return H >= kMinH && H <= kMaxH && H % 4 == 0; }

extern "C" int rm_inbatch_softmax_tile(int H, int which) {
  if (!rm_inbatch_softmax_supported(H)) return -1;
  switch (which) {
    case RM_IBS_ROWS: return kRows;
    case RM_IBS_COLS: return ibs_cols(ibs_nk(H));
    case RM_IBS_MAX_SPLITS: return kMaxSplits;
    default: return -1;
  }
}

extern "C" int64_t rm_inbatch_softmax_workspace(int64_t B, int H) {
  if (!rm_inbatch_softmax_supported(H) || B < 0 || B >= ((int64_t)1 << 30)) return -1;
  const int64_t b4 = ibs_round4(B);
  return 2 * kWsDoubles + b4 + 3 * kMaxSplits * b4 + (int64_t)kMaxSplits * b4 * H;
}

extern "C" int rm_inbatch_softmax_fwd(const float *U, int64_t ldu, const float *V, int64_t ldv,
                                      const int64_t *item_id, const float *logq, const float *w, float scale,
                                      int64_t B, int H, int col_splits, float *lse, float *row_loss, int32_t *rank,
                                      float *loss, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_inbatch_softmax_fwd";
  if (int rc = ibs_check(fn, B, H, col_splits)) return rc;
  if (B == 0) return RM_OK;
  if (int rc = ibs_operand(fn, "U", U, ldu, H)) return rc;
  if (int rc = ibs_operand(fn, "V", V, ldv, H)) return rc;
  RM_REQUIRE(lse && row_loss && loss, "%s: lse, row_loss or loss is NULL", fn);
  RM_REQUIRE(workspace && rm_aligned16(workspace), "%s: the workspace is NULL or not 16-byte aligned", fn);
  const int nk = ibs_nk(H), cols = ibs_cols(nk);
  const int splits = ibs_splits(B, cols, col_splits);
  const int64_t tiles = ibs_tiles(B, cols);
  const IbsWs ws = ibs_ws(workspace, B);
  hipStream_t st = (hipStream_t)stream;
  IbsArgs a = {};
  a.X = U; a.ldx = ldu; a.Y = V; a.ldy = ldv;
  a.ids = item_id; a.logq = logq; a.w = w;
  a.scale = scale;
  a.B = (int)B; a.H = H;
  a.tiles_per_split = (int)((tiles + splits - 1) / splits);
  a.pm = ws.pm; a.ps = ws.ps; a.pr = ws.pr; a.diag = ws.diag;
  a.pstride = ibs_round4(B);
  ibs_launch(nk, 0, dim3((unsigned)((B + kRows - 1) / kRows), splits), st, a);
  const int nblk = fin_blocks(B);
  hipLaunchKernelGGL(ibs_finish_kernel, dim3(nblk), dim3(kFinThreads), 0, st, ws.pm, ws.ps, ws.pr, a.pstride, ws.diag,
                     w, (int)B, splits, lse, row_loss, rank, ws.dbl);
  hipLaunchKernelGGL(ibs_total_kernel, dim3(1), dim3(kFinThreads), 0, st, ws.dbl, nblk, loss,
                     ws.dbl + 2 * kFinBlocks);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int rm_inbatch_softmax_bwd(const float *U, int64_t ldu, const float *V, int64_t ldv,
                                      const int64_t *item_id, const float *logq, const float *w, float scale,
                                      float grad_scale, int64_t B, int H, int col_splits, const float *lse, float *dU,
                                      int64_t lddu, float *dV, int64_t lddv, float *workspace, rm_stream_t stream) {
  const char *fn = "rm_inbatch_softmax_bwd";
  if (int rc = ibs_check(fn, B, H, col_splits)) return rc;
  if (B == 0) return RM_OK;
  if (int rc = ibs_operand(fn, "U", U, ldu, H)) return rc;
  if (int rc = ibs_operand(fn, "V", V, ldv, H)) return rc;
  if (int rc = ibs_operand(fn, "dU", dU, lddu, H)) return rc;
  if (int rc = ibs_operand(fn, "dV", dV, lddv, H)) return rc;
  RM_REQUIRE(lse, "%s: lse is NULL", fn);
  RM_REQUIRE(workspace && rm_aligned16(workspace), "%s: the workspace is NULL or not 16-byte aligned", fn);
  const int nk = ibs_nk(H), cols = ibs_cols(nk);
  const int splits = ibs_splits(B, cols, col_splits);
  const int64_t tiles = ibs_tiles(B, cols);
  const IbsWs ws = ibs_ws(workspace, B);
  hipStream_t st = (hipStream_t)stream;
  double *Wsum = ws.dbl + 2 * kFinBlocks;
  if (w) {
    const int nblk = fin_blocks(B);
    hipLaunchKernelGGL(ibs_wsum_kernel, dim3(nblk), dim3(kFinThreads), 0, st, w, (int)B, ws.dbl);
    hipLaunchKernelGGL(ibs_total_kernel, dim3(1), dim3(kFinThreads), 0, st, ws.dbl, nblk, (float *)nullptr, Wsum);
  }
  IbsArgs a = {};
  a.ids = item_id; a.logq = logq; a.w = w; a.lse = lse; a.Wsum = Wsum;
  a.scale = scale;
  a.coef = scale * grad_scale;
  a.B = (int)B; a.H = H;
  a.tiles_per_split = (int)((tiles + splits - 1) / splits);
  const dim3 grid((unsigned)((B + kRows - 1) / kRows), splits);
  const int64_t dsplit = (int64_t)ibs_round4(B) * H;
  const int sum_blocks = rm_grid_cap((B * (H / 4) + 255) / 256);
  for (int mode = 1; mode <= 2; ++mode) {
    float *dst = mode == 1 ? dU : dV;
    const int64_t ldd = mode == 1 ? lddu : lddv;
    a.X = mode == 1 ? U : V; a.ldx = mode == 1 ? ldu : ldv;
    a.Y = mode == 1 ? V : U; a.ldy = mode == 1 ? ldv : ldu;
    if (splits == 1) {
      a.dOwn = dst; a.lddo = ldd; a.dsplit = 0;
    } else {
      a.dOwn = ws.rows; a.lddo = H; a.dsplit = dsplit;
    }
    ibs_launch(nk, mode, grid, st, a);
    if (splits > 1)
      hipLaunchKernelGGL(ibs_sum_rows_kernel, dim3(sum_blocks), dim3(256), 0, st, ws.rows, dsplit, splits, (int)B, H,
                         dst, ldd);
  }
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int rm_rownorm_fwd(const float *X, int64_t ldx, int64_t B, int H, float eps, float *Y, int64_t ldy,
                              float *inv_norm, rm_stream_t stream) {
  const char *fn = "rm_rownorm_fwd";
  if (int rc = ibs_check(fn, B, H, 0)) return rc;
  RM_REQUIRE(eps > 0.f, "%s: eps=%g must be > 0", fn, (double)eps);
  if (B == 0) return RM_OK;
  if (int rc = ibs_operand(fn, "X", X, ldx, H)) return rc;
  if (int rc = ibs_operand(fn, "Y", Y, ldy, H)) return rc;
  RM_REQUIRE_PTR(fn, inv_norm);
  hipLaunchKernelGGL(rownorm_fwd_kernel, dim3(rm_grid_cap((B + 15) / 16)), dim3(256), 0, (hipStream_t)stream, X, ldx,
                     B, H, eps, Y, ldy, inv_norm);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}

extern "C" int rm_rownorm_bwd(const float *Y, int64_t ldy, const float *inv_norm, const float *dY, int64_t lddy,
                              int64_t B, int H, float *dX, int64_t lddx, rm_stream_t stream) {
  const char *fn = "rm_rownorm_bwd";
  if (int rc = ibs_check(fn, B, H, 0)) return rc;
  if (B == 0) return RM_OK;
  if (int rc = ibs_operand(fn, "Y", Y, ldy, H)) return rc;
  if (int rc = ibs_operand(fn, "dY", dY, lddy, H)) return rc;
  if (int rc = ibs_operand(fn, "dX", dX, lddx, H)) return rc;
  RM_REQUIRE_PTR(fn, inv_norm);
  hipLaunchKernelGGL(rownorm_bwd_kernel, dim3(rm_grid_cap((B + 15) / 16)), dim3(256), 0, (hipStream_t)stream, Y, ldy,
                     inv_norm, dY, lddy, B, H, dX, lddx);
  RM_CHECK_LAUNCH(fn);
  return RM_OK;
}
