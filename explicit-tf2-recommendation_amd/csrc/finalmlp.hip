// FinalMLP (FinalMLPLayer / FeatureSelectionLayer / DualPartsInteractionLayer, 8.DMR/CustomLayers.py:319-442) on gfx950:
// two gated copies of one embedding row, one BatchNorm-MLP stream over each, a bilinear head over the two streams.
//
// xs [B, D] (the shared rows), x_s [B, Dx_s] (the rows of gate s: s = 0 reads the item ids, s = 1 the user ids):
//   hg_s = relu(x_s Wh_s + bh_s)   g_s = 2 sigmoid(hg_s Wo_s + bo_s)   part_s = g_s (.) xs
//   z_s^0 = part_s W_s^0 + b_s^0   a_s^l = relu(BatchNorm(z_s^l) gamma_s^l + beta_s^l)   z_s^{l+1} = a_s^l W_s^{l+1} + b_s^{l+1}
//   out = sigmoid(m_0 W_1 + c_1 + m_1 W_2 + c_2 + sum_h m_0h^T W_12[h] m_1h),  m_s = a_s^{L-1}
// All parameters arrive in ONE packed buffer (the layout is FmOff below and in include/mi355rec.h), their gradients
// leave in one buffer of the same layout.
// A workgroup of 4 waves owns 32 examples (mfma_tile.h); every product runs on v_mfma_f32_32x32x2_f32 out of a k-major
// LDS operand, the head on the VALU out of LDS (its heads are d/n x d/n, 8 x 8 at the default).
// Forward, moving statistics: one launch.  Forward, batch statistics: the statistic of a layer is a grid-wide barrier,
// so launch `start` (-1, 0, ..., L - 1) ends where the next statistic is needed: it writes z^{start+1} and, per tile and
// column, (count, mean, M2 about that mean, two passes over LDS); a one-wave-per-column launch merges the tiles in a
// fixed order (Chan's update: the variance is never E[x^2] - mean^2), writes mean and rstd and moves the moving
// averages; the last launch runs the head: 2 L + 1 launches whatever B.
// Backward, stage L (head), L - 1, ..., 0: stage l turns dy^l (the gradient of the BatchNorm output) into dz^l with
// the batch sums of dy and dy xhat that the slot sum after stage l + 1 left in dbeta / dgamma, multiplies by W^l^T
// (MFMA) and masks with a^{l-1} > 0; stage 0 goes on through the gates to dxs, dx_0, dx_1.  The bias in front of a
// batch-statistics BatchNorm has the gradient sum_b dz = 0 identically: those are written as exact zeros.  W_1, W_2 and
// W_12 go to the small weight-gradient launch of tile_ops.h, every other weight gradient to rec_gemm_f32 (split-K,
// slices added in order).  No float atomics, no value with two writers; nothing allocates or synchronises.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

namespace {

// the limits are MaskNet's: the header gains no constant for this family
constexpr int FM_MAXD = REC_MASKNET_MAX_D, FM_MAXW = REC_MASKNET_MAX_O, FM_MAXL = REC_MASKNET_MAX_R;
constexpr int FM_MAXOUT = REC_MASKNET_MAX_R;
constexpr int FM_NTHR = 256;
constexpr int FM_G = FM_NTHR / MB_T;             // column groups of the VALU stages

static_assert(FM_MAXD <= 128 * MB_NJ, "accumulator blocks per wave");
static_assert(FM_MAXOUT <= FM_G, "one thread per (example, output)");

struct FmDims {
  int D, Dx[2], Hg[2], L, w[2][FM_MAXL], n, o;
  __host__ __device__ int HG() const { return Hg[0] + Hg[1]; }
  __host__ __device__ int Wl(int l) const { return w[0][l] + w[1][l]; }
  // column of (stream s, layer l) in z, a and stats: layer-major, stream 0 first
  __host__ __device__ int zoff(int s, int l) const {
    int at = 0;
    for (int i = 0; i < l; ++i) at += w[0][i] + w[1][i];
    return s ? at + w[0][l] : at;
  }
  __host__ __device__ int Z() const { return zoff(0, L); }
  __host__ __device__ int wmax() const {
    int m = 1;
    for (int l = 0; l < L; ++l) m = m > w[0][l] ? (m > w[1][l] ? m : w[1][l]) : (w[0][l] > w[1][l] ? w[0][l] : w[1][l]);
    return m;
  }
  __host__ __device__ int hd(int s) const { return w[s][L - 1] / n; }
};

// offsets (floats) into the packed parameters, in the order they are packed
struct FmOff {
  int Wh[2], bh[2], Wo[2], bo[2];
  int W[2][FM_MAXL], b[2][FM_MAXL], gamma[2][FM_MAXL], beta[2][FM_MAXL];
  int W1, c1, W2, c2, W12, total;
};
static FmOff fm_off(const FmDims& d) {
  FmOff p{};
  int at = 0;
  auto take = [&](int n) { const int q = at; at += n; return q; };
  for (int s = 0; s < 2; ++s) {
    p.Wh[s] = take(d.Dx[s] * d.Hg[s]);
    p.bh[s] = take(d.Hg[s]);
    p.Wo[s] = take(d.Hg[s] * d.D);
    p.bo[s] = take(d.D);
  }
  for (int s = 0; s < 2; ++s)
    for (int l = 0; l < d.L; ++l) {
      const int in = l ? d.w[s][l - 1] : d.D, w = d.w[s][l];
      p.W[s][l] = take(in * w);
      p.b[s][l] = take(w);
      p.gamma[s][l] = take(w);
      p.beta[s][l] = take(w);
    }
  const int d1 = d.w[0][d.L - 1], d2 = d.w[1][d.L - 1];
  p.W1 = take(d1 * d.o);
  p.c1 = take(d.o);
  p.W2 = take(d2 * d.o);
  p.c2 = take(d.o);
  p.W12 = take(d1 * (d2 / d.n) * d.o);
  p.total = at;
  return p;
}

__host__ __device__ inline int fm_max(int a, int b) { return a > b ? a : b; }

// rows of LDS ([.][33] floats each):
//   forward   R [max(even(D), even(Dx), 2 We)] | hgs [even(max Hg)] | zb [2 We] | hdp [FM_G o]
//   backward  A [2 We] | R [max(even(D), 2 We)] | H [even(max Hg)] | dls [o] | ps [o]
// with We = even(the widest stream layer)
__host__ __device__ inline int fm_rrows(const FmDims& d, int bwd) {
  const int We = mb_even(d.wmax());
  int r = fm_max(mb_even(d.D), 2 * We);
  if (!bwd) r = fm_max(r, fm_max(mb_even(d.Dx[0]), mb_even(d.Dx[1])));
  return r;
}
__host__ __device__ inline int fm_hrows(const FmDims& d) { return mb_even(fm_max(d.Hg[0], d.Hg[1])); }
__host__ __device__ inline size_t fm_lds_floats(const FmDims& d, int bwd) {
  const int We = mb_even(d.wmax());
  const int rows = fm_rrows(d, bwd) + fm_hrows(d) + 2 * We + (bwd ? 2 * d.o : FM_G * d.o);
  return (size_t)rows * MB_LD;
}
constexpr size_t FM_LDS_CAP = 128 * 1024;
static_assert(sizeof(float) * (FM_MAXD + FM_MAXW + 2 * FM_MAXW + FM_G * FM_MAXOUT) * MB_LD <= FM_LDS_CAP &&
                  FM_LDS_CAP <= REC_LDS_CU_BYTES,
              "both directions of the largest shape fit the LDS of a CU");

using Tile = TileOps<MB_T, MB_LD, FM_NTHR>;

// the operand row behind an odd K is read by the MFMA loop (against a zero weight): keep it finite
__device__ __forceinline__ void fm_pad(float* buf, int K, int tid) {
  if ((K & 1) && tid < MB_LD) buf[K * MB_LD + tid] = 0.f;
}

// epi(col, row, value) for every element of As [32, K] . Bm [K, N] (mb_mma's operands)
template <bool TRANS, class Epi>
__device__ __forceinline__ void fm_product(const float* As, int K, const float* __restrict__ W, int64_t ldw, int N,
                                           int wave, int lo, int hi, Epi epi) {
  f32x16 acc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
  mb_mma<TRANS>(acc, As, K, W, ldw, 0, N, wave, lo, hi);
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int col = (wave + 4 * j) * 32 + lo;
    if ((wave + 4 * j) * 32 < N && col < N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) epi(col, mb_row(r, hi), acc[j][r]);
    }
  }
}

// the same for N <= 128: one 32-column block per wave, one accumulator
template <bool TRANS, class Epi>
__device__ __forceinline__ void fm_product1(const float* As, int K, const float* __restrict__ W, int64_t ldw, int N,
                                            int wave, int lo, int hi, Epi epi) {
  if (wave * 32 >= N) return;                    // uniform over the wave
  f32x16 acc;
  mb_zero(acc);
  mb_mma1<TRANS>(acc, As, K, W, ldw, 0, N, wave * 32, lo, hi);
  const int col = wave * 32 + lo;
  if (col < N) {
#pragma unroll
    for (int r = 0; r < 16; ++r) epi(col, mb_row(r, hi), acc[r]);
  }
}

// merge (nb, meanb, M2b) into (n, mean, M2): Chan, Golub and LeVeque's pairwise update
__device__ __forceinline__ void fm_chan(float& n, float& mean, float& M2, float nb, float meanb, float M2b) {
  if (nb == 0.f) return;
  const float nt = n + nb, dlt = meanb - mean;
  mean += dlt * (nb / nt);
  M2 += M2b + dlt * dlt * (n * nb / nt);
  n = nt;
}

struct FmFwd {
  const float *xs, *x[2], *P;
  const float *mm[2][FM_MAXL], *mv[2][FM_MAXL];  // the moving statistics (read when training == 0)
  float *out, *hg, *g, *z, *a, *stats;           // the save buffers: all or none
  float* tstat;                                  // [tiles][Wl][3] of the layer this launch produces
  int64_t B;
  int training, start;
  float eps;
};

__global__ __launch_bounds__(FM_NTHR) void finalmlp_fwd_kernel(FmDims d, FmOff po, FmFwd f) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = d.D, L = d.L, Z = d.Z(), HG = d.HG(), o = d.o, We = mb_even(d.wmax());
  float* R = lds;
  float* hgs = R + fm_rrows(d, 0) * MB_LD;
  float* zb = hgs + fm_hrows(d) * MB_LD;
  float* hdp = zb + 2 * We * MB_LD;
  float *cur0 = zb, *cur1 = zb + We * MB_LD, *alt0 = R, *alt1 = R + We * MB_LD;
  const int64_t r0 = (int64_t)blockIdx.x * MB_T, B = f.B;
  const float* __restrict__ P = f.P;
  int l;
  bool fresh;

  if (f.start < 0) {
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      const int Dx = s ? d.Dx[1] : d.Dx[0], Hg = s ? d.Hg[1] : d.Hg[0], w0 = s ? d.w[1][0] : d.w[0][0];
      const float* __restrict__ xg = s ? f.x[1] : f.x[0];
      const float* __restrict__ Wh = P + (s ? po.Wh[1] : po.Wh[0]);
      const float* __restrict__ bh = P + (s ? po.bh[1] : po.bh[0]);
      const float* __restrict__ Wo = P + (s ? po.Wo[1] : po.Wo[0]);
      const float* __restrict__ bo = P + (s ? po.bo[1] : po.bo[0]);
      const float* __restrict__ W0 = P + (s ? po.W[1][0] : po.W[0][0]);
      const float* __restrict__ b0 = P + (s ? po.b[1][0] : po.b[0][0]);
      const float* __restrict__ xsg = f.xs;
      float* __restrict__ shg = f.hg ? f.hg + (s ? d.Hg[0] : 0) : nullptr;
      float* __restrict__ sg = f.g ? f.g + s * D : nullptr;
      float* zs = s ? cur1 : cur0;
      Tile::rows_in(R, xg, r0, B, Dx, 0, Dx, tid);
      fm_pad(R, Dx, tid);
      __syncthreads();
      fm_product1<false>(R, Dx, Wh, Hg, Hg, wave, lo, hi, [=](int col, int row, float v) {
        const float hv = fmaxf(v + bh[col], 0.f);
        hgs[col * MB_LD + row] = hv;
        if (shg && r0 + row < B) shg[(r0 + row) * HG + col] = hv;
      });
      fm_pad(hgs, Hg, tid);
      __syncthreads();                           // and every read of the x tile lies before it: R may be written
      fm_product<false>(hgs, Hg, Wo, D, D, wave, lo, hi,
                        [=](int col, int row, float v) { R[col * MB_LD + row] = v + bo[col]; });
      __syncthreads();
      for (int i = tid; i < MB_T * D; i += FM_NTHR) {          // g = 2 sigmoid, part = g (.) xs, rows of the batch
        const int row = i / D, c = i - row * D;
        float pv = 0.f;
        if (r0 + row < B) {
          const float gv = 2.f * sigmoid_acc(R[c * MB_LD + row]);
          pv = gv * xsg[(r0 + row) * D + c];
          if (sg) sg[(r0 + row) * 2 * D + c] = gv;
        }
        R[c * MB_LD + row] = pv;
      }
      fm_pad(R, D, tid);
      __syncthreads();
      fm_product1<false>(R, D, W0, w0, w0, wave, lo, hi,
                         [=](int col, int row, float v) { zs[col * MB_LD + row] = v + b0[col]; });
      __syncthreads();                           // R and hgs are rewritten by the next stream
    }
    l = 0;
    fresh = true;
  } else {
    l = f.start;
    Tile::rows_in(cur0, f.z, r0, B, Z, d.zoff(0, l), d.w[0][l], tid);
    Tile::rows_in(cur1, f.z, r0, B, Z, d.zoff(1, l), d.w[1][l], tid);
    __syncthreads();
    fresh = false;
  }

  for (;;) {
    if (fresh && f.z) {
      Tile::rows_out(f.z, cur0, r0, B, Z, d.zoff(0, l), d.w[0][l], tid);
      Tile::rows_out(f.z, cur1, r0, B, Z, d.zoff(1, l), d.w[1][l], tid);
    }
    if (fresh && f.training) {                   // (count, mean, M2) of the tile's valid rows, per column
      const int w0 = d.w[0][l], Wl = d.Wl(l);
      const int cnt = B - r0 < MB_T ? (int)(B - r0) : MB_T;
      for (int c = tid; c < Wl; c += FM_NTHR) {
        const float* col = c < w0 ? cur0 + c * MB_LD : cur1 + (c - w0) * MB_LD;
        // the mean about the first row: a column whose mean is far above its spread loses nothing in the sum, and a
        // constant column has exactly its value as mean and M2 = 0
        const float x0 = col[0];
        float s = 0.f, m2 = 0.f;
        for (int r = 0; r < cnt; ++r) s += col[r] - x0;
        const float mean = x0 + s / (float)cnt;
        for (int r = 0; r < cnt; ++r) {
          const float dv = col[r] - mean;
          m2 += dv * dv;
        }
        float* t = f.tstat + ((int64_t)blockIdx.x * Wl + c) * 3;
        t[0] = (float)cnt;
        t[1] = mean;
        t[2] = m2;
      }
      return;
    }
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {                // a = relu(xhat gamma + beta) in place
      float* zs = s ? cur1 : cur0;
      const int w = d.w[s][l], zo = d.zoff(s, l);
      const float* __restrict__ mmp = f.mm[s][l];
      const float* __restrict__ mvp = f.mv[s][l];
      const float* __restrict__ gam = P + po.gamma[s][l];
      const float* __restrict__ bet = P + po.beta[s][l];
      for (int i = tid; i < MB_T * w; i += FM_NTHR) {
        const int row = i / w, c = i - row * w;
        float mean, rstd;
        if (f.training) {
          mean = f.stats[zo + c];
          rstd = f.stats[Z + zo + c];
        } else {
          mean = mmp[c];
          rstd = 1.0f / sqrtf(mvp[c] + f.eps);
          if (f.stats && blockIdx.x == 0 && row == 0) {
            f.stats[zo + c] = mean;
            f.stats[Z + zo + c] = rstd;
          }
        }
        const float xh = (zs[c * MB_LD + row] - mean) * rstd;
        const float av = fmaxf(xh * gam[c] + bet[c], 0.f);
        zs[c * MB_LD + row] = av;
        if (f.a && r0 + row < B) f.a[(r0 + row) * Z + zo + c] = av;
      }
      fm_pad(zs, w, tid);
    }
    __syncthreads();
    if (l == L - 1) break;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      const float* as = s ? cur1 : cur0;
      float* zs = s ? alt1 : alt0;
      const int w = d.w[s][l + 1];
      const float* __restrict__ bn = P + po.b[s][l + 1];
      fm_product1<false>(as, d.w[s][l], P + po.W[s][l + 1], w, w, wave, lo, hi,
                         [=](int col, int row, float v) { zs[col * MB_LD + row] = v + bn[col]; });
    }
    __syncthreads();
    float* t0 = cur0;
    float* t1 = cur1;
    cur0 = alt0;
    cur1 = alt1;
    alt0 = t0;
    alt1 = t1;
    ++l;
    fresh = true;
  }

  // the head: thread (example b, group g) owns the heads g, g + 8, ... and the rows g, g + 8, ... of W_1 and W_2
  const int b = tid & (MB_T - 1), g = tid >> 5;
  const int d1 = d.w[0][L - 1], d2 = d.w[1][L - 1], n = d.n, h1 = d.hd(0), h2 = d.hd(1);
  const float* a1 = cur0 + b;
  const float* a2 = cur1 + b;
  for (int oo = 0; oo < o; ++oo) {
    float acc = 0.f;
    for (int h = g; h < n; h += FM_G)
      for (int x = 0; x < h1; ++x) {
        const float* W = P + po.W12 + ((int64_t)(h * h1 + x) * h2) * o + oo;
        float t = 0.f;
        for (int y = 0; y < h2; ++y) t = fmaf(W[y * o], a2[(h * h2 + y) * MB_LD], t);
        acc = fmaf(a1[(h * h1 + x) * MB_LD], t, acc);
      }
    for (int k = g; k < d1; k += FM_G) acc = fmaf(a1[k * MB_LD], P[po.W1 + k * o + oo], acc);
    for (int k = g; k < d2; k += FM_G) acc = fmaf(a2[k * MB_LD], P[po.W2 + k * o + oo], acc);
    hdp[(g * o + oo) * MB_LD + b] = acc;
  }
  __syncthreads();
  if (g < o && r0 + b < B) {
    float acc = 0.f;
    for (int q = 0; q < FM_G; ++q) acc += hdp[(q * o + g) * MB_LD + b];
    f.out[(r0 + b) * o + g] = sigmoid_acc(acc + P[po.c1 + g] + P[po.c2 + g]);
  }
}

// One wave per column of layer l: lane i merges the tiles i, i + 64, ... in order, a shift-down tree merges the lanes,
// lane 0 writes mean and rstd and moves the moving averages.
__global__ __launch_bounds__(64) void finalmlp_merge_kernel(const float* __restrict__ tstat, int tiles, int Wl, int w0,
                                                            float eps, float momentum, float rest, float* mm0, float* mv0,
                                                            float* mm1, float* mv1, float* __restrict__ stats, int zo,
                                                            int Z) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float n = 0.f, mean = 0.f, M2 = 0.f;
  for (int t = lane; t < tiles; t += 64) {
    const float* p = tstat + ((int64_t)t * Wl + c) * 3;
    fm_chan(n, mean, M2, p[0], p[1], p[2]);
  }
  for (int sh = 32; sh > 0; sh >>= 1) {
    const float nb = __shfl_down(n, sh, 64), mb = __shfl_down(mean, sh, 64), qb = __shfl_down(M2, sh, 64);
    if (lane + sh < 64) fm_chan(n, mean, M2, nb, mb, qb);
  }
  if (lane == 0) {
    const float var = M2 / n;
    stats[zo + c] = mean;
    stats[Z + zo + c] = 1.0f / sqrtf(var + eps);
    float* mm = c < w0 ? mm0 + c : mm1 + (c - w0);
    float* mv = c < w0 ? mv0 + c : mv1 + (c - w0);
    *mm = *mm * momentum + mean * rest;
    *mv = *mv * momentum + var * rest;
  }
}

struct FmBwd {
  const float *xs, *P, *hg, *g, *z, *a, *stats, *out, *dout;
  const float* G;                                // the gradient buffer: dbeta / dgamma of the stage's layer are read
  float *dxs, *dx[2];
  float *wd, *wdl, *wq, *wpart, *wdg, *wdh, *slots;
  int64_t B;
  int training, stage;
};

// floats of a tile's slot at a stage:
//   L          dc_1 [o] | dc_2 [o] | dgamma_0, dbeta_0 [2 w_0] | dgamma_1, dbeta_1 [2 w_1]            (layer L - 1)
//   L-1 .. 1   db_0 [w_0] | db_1 [w_1] (layer l) | dgamma_0, dbeta_0 | dgamma_1, dbeta_1              (layer l - 1)
//   0          db_0 | db_1 (layer 0) | dbo_0 [D] | dbh_0 [Hg_0] | dbo_1 [D] | dbh_1 [Hg_1]
__host__ __device__ inline int fm_slot_floats(const FmDims& d, int stage) {
  if (stage == d.L) return 2 * d.o + 2 * d.Wl(d.L - 1);
  if (stage > 0) return d.Wl(stage) + 2 * d.Wl(stage - 1);
  return d.Wl(0) + 2 * d.D + d.HG();
}

__global__ __launch_bounds__(FM_NTHR) void finalmlp_bwd_kernel(FmDims d, FmOff po, FmBwd f) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = d.D, L = d.L, Z = d.Z(), HG = d.HG(), o = d.o, We = mb_even(d.wmax()), stage = f.stage;
  float* A0 = lds;
  float* A1 = A0 + We * MB_LD;
  float* R = A1 + We * MB_LD;
  float* R1 = R + We * MB_LD;
  float* H = R + fm_rrows(d, 1) * MB_LD;
  float* dls = H + fm_hrows(d) * MB_LD;
  float* ps = dls + o * MB_LD;
  const int64_t r0 = (int64_t)blockIdx.x * MB_T, B = f.B;
  const float* __restrict__ P = f.P;
  const int b = tid & (MB_T - 1), g = tid >> 5;
  float* __restrict__ slot = f.slots + (int64_t)blockIdx.x * fm_slot_floats(d, stage);
  const float invB = 1.f / (float)B;
  float *dy0, *dy1, *xh0, *xh1, *bslot;
  int lp;                                        // the layer whose dy this stage produces

  if (stage == L) {
    lp = L - 1;
    const int d1 = d.w[0][lp], d2 = d.w[1][lp], n = d.n, h1 = d.hd(0), h2 = d.hd(1);
    float *a1s = R, *a2s = R1;
    Tile::rows_in(a1s, f.a, r0, B, Z, d.zoff(0, lp), d1, tid);
    Tile::rows_in(a2s, f.a, r0, B, Z, d.zoff(1, lp), d2, tid);
    Tile::rows_in(dls, f.dout, r0, B, o, 0, o, tid);
    Tile::rows_in(ps, f.out, r0, B, o, 0, o, tid);
    __syncthreads();
    if (g < o) {
      const float pv = ps[g * MB_LD + b];
      dls[g * MB_LD + b] = dls[g * MB_LD + b] * (pv * (1.f - pv));
    }
    __syncthreads();
    Tile::rows_out(f.wdl, dls, r0, B, o, 0, o, tid);
    Tile::col_sums(slot, dls, o, tid);
    Tile::col_sums(slot + o, dls, o, tid);
    const int qn = d2 * o;                       // q[b, y o + oo] = a2[b, y] dl[b, oo]: the right operand of dW_12
    for (int i = tid; i < MB_T * qn; i += FM_NTHR) {
      const int row = i / qn, c = i - row * qn, y = c / o, oo = c - y * o;
      if (r0 + row < B) f.wq[(r0 + row) * qn + c] = a2s[y * MB_LD + row] * dls[oo * MB_LD + row];
    }
    for (int k = g; k < d1; k += FM_G) {         // dm_0
      const int h = k / h1;
      float acc = 0.f;
      for (int oo = 0; oo < o; ++oo) {
        const float* W = P + po.W12 + ((int64_t)k * h2) * o + oo;
        float t = 0.f;
        for (int y = 0; y < h2; ++y) t = fmaf(W[y * o], a2s[(h * h2 + y) * MB_LD + b], t);
        acc = fmaf(dls[oo * MB_LD + b], t + P[po.W1 + k * o + oo], acc);
      }
      A0[k * MB_LD + b] = acc;
    }
    for (int k = g; k < d2; k += FM_G) {         // dm_1
      const int h = k / h2, y = k - h * h2;
      float acc = 0.f;
      for (int oo = 0; oo < o; ++oo) {
        const float* W = P + po.W12 + ((int64_t)(h * h1) * h2 + y) * o + oo;
        float t = 0.f;
        for (int x = 0; x < h1; ++x) t = fmaf(W[(int64_t)x * h2 * o], a1s[(h * h1 + x) * MB_LD + b], t);
        acc = fmaf(dls[oo * MB_LD + b], t + P[po.W2 + k * o + oo], acc);
      }
      A1[k * MB_LD + b] = acc;
    }
    __syncthreads();                             // and every read of a1s, a2s lies before it
    dy0 = A0, dy1 = A1, xh0 = R, xh1 = R1;
    bslot = slot + 2 * o;
  } else {
    const int l = stage;
#pragma unroll
    for (int s = 0; s < 2; ++s) {                // dz^l out of dy^l, in place in the workspace and into LDS
      float* As = s ? A1 : A0;
      const int w = d.w[s][l], zo = d.zoff(s, l);
      for (int i = tid; i < MB_T * w; i += FM_NTHR) {
        const int row = i / w, c = i - row * w;
        float v = 0.f;
        if (r0 + row < B) {
          const int64_t at = (r0 + row) * Z + zo + c;
          const float rstd = f.stats[Z + zo + c];
          const float k = P[po.gamma[s][l] + c] * rstd;
          if (f.training) {
            const float xh = (f.z[at] - f.stats[zo + c]) * rstd;
            v = k * (f.wd[at] - f.G[po.beta[s][l] + c] * invB - xh * (f.G[po.gamma[s][l] + c] * invB));
          } else {
            v = k * f.wd[at];
          }
          f.wd[at] = v;
        }
        As[c * MB_LD + row] = v;
      }
      fm_pad(As, w, tid);
    }
    __syncthreads();
    {                                            // db^l: identically zero behind a batch statistic
      const int w0 = d.w[0][l], w1 = d.w[1][l];
      if (f.training) {
        for (int c = tid; c < w0 + w1; c += FM_NTHR) slot[c] = 0.f;
      } else {
        Tile::col_sums(slot, A0, w0, tid);
        Tile::col_sums(slot + w0, A1, w1, tid);
      }
    }
    if (l == 0) {                                // through the gates
      float* __restrict__ sl = slot + d.Wl(0);
#pragma unroll 1
      for (int s = 0; s < 2; ++s) {
        const float* As = s ? A1 : A0;
        const int Dx = s ? d.Dx[1] : d.Dx[0], Hg = s ? d.Hg[1] : d.Hg[0], w0 = s ? d.w[1][0] : d.w[0][0];
        const int hoff = s ? d.Hg[0] : 0;
        const float* __restrict__ W0 = P + (s ? po.W[1][0] : po.W[0][0]);
        const float* __restrict__ Wo = P + (s ? po.Wo[1] : po.Wo[0]);
        const float* __restrict__ Wh = P + (s ? po.Wh[1] : po.Wh[0]);
        const float* __restrict__ shg = f.hg + hoff;
        float* __restrict__ wdh = f.wdh + hoff;
        fm_product<true>(As, w0, W0, w0, D, wave, lo, hi,                       // dpart = dz^0 W^0^T
                         [=](int col, int row, float v) { R[col * MB_LD + row] = v; });
        __syncthreads();
        for (int i = tid; i < MB_T * D; i += FM_NTHR) {
          const int row = i / D, c = i - row * D;
          float dgp = 0.f;
          if (r0 + row < B) {
            const int64_t at = (r0 + row) * 2 * D + s * D + c;
            const float xv = f.xs[(r0 + row) * D + c], gv = f.g[at], dp = R[c * MB_LD + row];
            // dxs = dpart_0 g_0 + dpart_1 g_1: the second gate adds to what this thread wrote for the first
            float* dq = f.dxs + (r0 + row) * D + c;
            *dq = s ? *dq + dp * gv : dp * gv;
            dgp = (dp * xv) * (gv * (1.f - 0.5f * gv));                         // g = 2 sigmoid: g' = g (1 - g / 2)
            f.wdg[at] = dgp;
            f.wpart[at] = gv * xv;
          }
          R[c * MB_LD + row] = dgp;
        }
        fm_pad(R, D, tid);
        __syncthreads();
        Tile::col_sums(sl, R, D, tid);
        fm_product1<true>(R, D, Wo, D, Hg, wave, lo, hi, [=](int col, int row, float v) {
          float m = 0.f;
          if (r0 + row < B) {
            m = shg[(r0 + row) * HG + col] > 0.f ? v : 0.f;
            wdh[(r0 + row) * HG + col] = m;
          }
          H[col * MB_LD + row] = m;
        });
        fm_pad(H, Hg, tid);
        __syncthreads();
        Tile::col_sums(sl + D, H, Hg, tid);
        float* __restrict__ dxp = s ? f.dx[1] : f.dx[0];
        fm_product<true>(H, Hg, Wh, Hg, Dx, wave, lo, hi, [=](int col, int row, float v) {
          if (r0 + row < B) dxp[(r0 + row) * Dx + col] = v;
        });
        __syncthreads();                         // R and H are rewritten by the next gate
        sl += D + Hg;
      }
      return;
    }
    lp = l - 1;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {                // da^{l-1} = dz^l W^l^T
      const float* As = s ? A1 : A0;
      float* out = s ? R1 : R;
      const int w = d.w[s][l];
      fm_product1<true>(As, w, P + po.W[s][l], w, d.w[s][lp], wave, lo, hi,
                        [=](int col, int row, float v) { out[col * MB_LD + row] = v; });
    }
    __syncthreads();                             // and every read of dz lies before it
    dy0 = R, dy1 = R1, xh0 = A0, xh1 = A1;
    bslot = slot + d.Wl(l);
  }

  // dy^{lp} = da (.) [a^{lp} > 0] to the workspace, its sums and its sums against xhat^{lp} to the slot
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float* dys = s ? dy1 : dy0;
    float* xhs = s ? xh1 : xh0;
    const int w = d.w[s][lp], zo = d.zoff(s, lp);
    for (int i = tid; i < MB_T * w; i += FM_NTHR) {
      const int row = i / w, c = i - row * w;
      float v = 0.f, xh = 0.f;
      if (r0 + row < B) {
        const int64_t at = (r0 + row) * Z + zo + c;
        v = f.a[at] > 0.f ? dys[c * MB_LD + row] : 0.f;
        xh = (f.z[at] - f.stats[zo + c]) * f.stats[Z + zo + c];
        f.wd[at] = v;
      }
      dys[c * MB_LD + row] = v;
      xhs[c * MB_LD + row] = xh;
    }
  }
  __syncthreads();
  const int w0 = d.w[0][lp], w1 = d.w[1][lp];
  Tile::col_sums(bslot, dy0, w0, tid, xh0);
  Tile::col_sums(bslot + w0, dy0, w0, tid);
  Tile::col_sums(bslot + 2 * w0, dy1, w1, tid, xh1);
  Tile::col_sums(bslot + 2 * w0 + w1, dy1, w1, tid);
}

// The small weight gradients in one launch (small_dw_kernel, tile_ops.h): matrix 0 is dW_1 = m_0^T dl, matrix 1 dW_2 =
// m_1^T dl, matrix 2 + h is dW_12[h] = m_0h^T q_h with q[b, y o + oo] = m_1[b, y] dl[b, oo]; laid out in that order.
struct FmSmall {
  static constexpr int MAXK = FM_MAXW;
  const float *a, *dl, *q;
  int Z, a0, a1, d1, d2, h1, h2, o;
  __device__ SmallMat mat(int m) const {
    if (m == 0) return {a, Z, a0, d1, dl, o, 0, o, 0, o};
    if (m == 1) return {a, Z, a1, d2, dl, o, 0, o, d1 * o, o};
    m -= 2;
    return {a, Z, a0 + m * h1, h1, q, d2 * o, m * h2 * o, h2 * o, (d1 + d2) * o + m * h1 * h2 * o, h2 * o};
  }
};

static int fm_shape(int64_t B, int D, int D1, int D2, int Hg1, int Hg2, int L, const int* w1, const int* w2, int n,
                    int o, FmDims* out) {
  if (B < 0 || D < 1 || D1 < 1 || D2 < 1 || Hg1 < 1 || Hg2 < 1 || L < 1 || n < 1 || o < 1 || !w1 || !w2) return REC_E_ARG;
  if (L > FM_MAXL) return REC_E_UNSUPPORTED;
  FmDims d{};
  d.D = D, d.Dx[0] = D1, d.Dx[1] = D2, d.Hg[0] = Hg1, d.Hg[1] = Hg2, d.L = L, d.n = n, d.o = o;
  for (int l = 0; l < L; ++l) {
    if (w1[l] < 1 || w2[l] < 1) return REC_E_ARG;
    d.w[0][l] = w1[l], d.w[1][l] = w2[l];
  }
  if (w1[L - 1] % n || w2[L - 1] % n) return REC_E_ARG;
  if (D > FM_MAXD || D1 > FM_MAXD || D2 > FM_MAXD || Hg1 > FM_MAXW || Hg2 > FM_MAXW || d.wmax() > FM_MAXW ||
      o > FM_MAXOUT || (int64_t)d.hd(1) * o > FM_MAXW || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;
  *out = d;
  return REC_OK;
}

static int fm_small_floats(const FmDims& d) {
  const int d1 = d.w[0][d.L - 1], d2 = d.w[1][d.L - 1];
  return (d1 + d2) * d.o + d1 * d.hd(1) * d.o;
}

struct FmWs {
  size_t tstat, wd, wdl, wq, wpart, wdg, wdh, slots, part, gemm, total;      // offsets in floats
};
static FmWs fm_ws(int64_t B, const FmDims& d) {
  FmWs w{};
  const size_t b = (size_t)B, tiles = (size_t)ceil_div64(B, MB_T);
  WsCarve c;
  int wl = 0, sl = 0;
  for (int l = 0; l < d.L; ++l) wl = fm_max(wl, d.Wl(l));
  for (int st = 0; st <= d.L; ++st) sl = fm_max(sl, fm_slot_floats(d, st));
  w.tstat = c.take(tiles * wl * 3);
  w.wd = c.take(b * d.Z());
  w.wdl = c.take(b * d.o);
  w.wq = c.take(b * d.w[1][d.L - 1] * d.o);
  w.wpart = c.take(b * 2 * d.D);
  w.wdg = c.take(b * 2 * d.D);
  w.wdh = c.take(b * d.HG());
  w.slots = c.take(tiles * (size_t)sl);
  w.part = c.take((size_t)mb_small_split(B) * fm_small_floats(d));
  size_t gm = 0;
  for (int s = 0; s < 2; ++s) {
    gm = gm > mb_dw_gemm_floats(B, d.Dx[s], d.Hg[s]) ? gm : mb_dw_gemm_floats(B, d.Dx[s], d.Hg[s]);
    gm = gm > mb_dw_gemm_floats(B, d.Hg[s], d.D) ? gm : mb_dw_gemm_floats(B, d.Hg[s], d.D);
    for (int l = 0; l < d.L; ++l) {
      const size_t q = mb_dw_gemm_floats(B, l ? d.w[s][l - 1] : d.D, d.w[s][l]);
      gm = gm > q ? gm : q;
    }
  }
  w.gemm = c.take(gm);
  w.total = c.at;
  return w;
}

// dW [M, N] = A^T G over the batch, A and G column blocks of wider buffers
static int fm_dw(int M, int N, int64_t B, const float* A, int64_t lda, const float* G, int64_t ldg, float* dW,
                 float* gws, void* stream) {
  return rec_gemm_f32(1, 0, M, N, B, A, lda, G, ldg, dW, N, REC_EPI_NONE, nullptr, nullptr, 0, nullptr, 0,
                      mb_split(B, M, N), gws, nullptr, stream);
}

}  // namespace

extern "C" size_t rec_finalmlp_scratch_bytes(int64_t B, int D, int D1, int D2, int Hg1, int Hg2, int L,
                                               const int* widths1_host, const int* widths2_host, int n, int o) {
  FmDims d;
  if (fm_shape(B, D, D1, D2, Hg1, Hg2, L, widths1_host, widths2_host, n, o, &d) != REC_OK) return 0;
  return sizeof(float) * (fm_ws(B, d).total + 4);
}

extern "C" int rec_finalmlp_fwd_f32(const float* xs, const float* x1, const float* x2, const float* params,
                                    float* const* moving_mean_host, float* const* moving_var_host, int64_t B, int D, int D1,
                                    int D2, int Hg1, int Hg2, int L, const int* widths1_host, const int* widths2_host, int n,
                                    int o, int training, double eps, double momentum, float* out, float* hg, float* g,
                                    float* z, float* a, float* stats, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  FmDims d;
  if (int rc = fm_shape(B, D, D1, D2, Hg1, Hg2, L, widths1_host, widths2_host, n, o, &d)) return rc;
  if ((training != 0 && training != 1) || !(eps > 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!xs || !x1 || !x2 || !params || !moving_mean_host || !moving_var_host || !out) return REC_E_ARG;
  for (int i = 0; i < 2 * L; ++i)
    if (!moving_mean_host[i] || !moving_var_host[i]) return REC_E_ARG;
  const bool save = hg || g || z || a || stats;
  if (save && !(hg && g && z && a && stats)) return REC_E_ARG;                   // all of them or none
  if (training && !save) return REC_E_ARG;                                      // z carries the chain between launches
  const FmWs w = fm_ws(B, d);
  if (training && (!workspace || workspace_bytes < sizeof(float) * w.total)) return workspace ? REC_E_WORKSPACE : REC_E_ARG;
  const FmOff po = fm_off(d);
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, MB_T);
  if (hipError_t err = rec_allow_lds<finalmlp_fwd_kernel>(FM_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * fm_lds_floats(d, 0);
  FmFwd f{};
  f.xs = xs, f.x[0] = x1, f.x[1] = x2, f.P = params;
  for (int s = 0; s < 2; ++s)
    for (int l = 0; l < L; ++l) f.mm[s][l] = moving_mean_host[s * L + l], f.mv[s][l] = moving_var_host[s * L + l];
  f.out = out, f.hg = hg, f.g = g, f.z = z, f.a = a, f.stats = stats;
  f.tstat = training ? static_cast<float*>(workspace) + w.tstat : nullptr;
  f.B = B, f.training = training, f.eps = (float)eps;
  for (int start = -1; start < (training ? L : 0); ++start) {
    f.start = start;
    hipLaunchKernelGGL(finalmlp_fwd_kernel, dim3(tiles), dim3(FM_NTHR), lds, st, d, po, f);
    REC_LAUNCH_CHECK();
    if (training && start + 1 < L) {
      const int l = start + 1;
      // 1 - momentum is rounded to fp32 once, from the double: 1.f - 0.99f would be 9.5e-7 off 0.01, relatively
      hipLaunchKernelGGL(finalmlp_merge_kernel, dim3(d.Wl(l)), dim3(64), 0, st, f.tstat, tiles, d.Wl(l), d.w[0][l],
                         (float)eps, (float)momentum, (float)(1.0 - momentum), moving_mean_host[l], moving_var_host[l],
                         moving_mean_host[L + l], moving_var_host[L + l], stats, d.zoff(0, l), d.Z());
      REC_LAUNCH_CHECK();
    }
  }
  return REC_OK;
}

extern "C" int rec_finalmlp_bwd_f32(const float* xs, const float* x1, const float* x2, const float* params,
                                    const float* hg, const float* g, const float* z, const float* a, const float* stats,
                                    const float* out, const float* dout, int64_t B, int D, int D1, int D2, int Hg1,
                                    int Hg2, int L, const int* widths1_host, const int* widths2_host, int n, int o, int training,
                                    float* dxs, float* dx1, float* dx2, float* dparams, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  FmDims d;
  if (int rc = fm_shape(B, D, D1, D2, Hg1, Hg2, L, widths1_host, widths2_host, n, o, &d)) return rc;
  if (training != 0 && training != 1) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!xs || !x1 || !x2 || !params || !hg || !g || !z || !a || !stats || !out || !dout || !dxs || !dx1 || !dx2 ||
      !dparams || !workspace)
    return REC_E_ARG;
  const FmWs w = fm_ws(B, d);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  const FmOff po = fm_off(d);
  float* base = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, MB_T), Z = d.Z(), HG = d.HG();
  if (hipError_t err = rec_allow_lds<finalmlp_bwd_kernel>(FM_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * fm_lds_floats(d, 1);
  FmBwd f{};
  f.xs = xs, f.P = params, f.hg = hg, f.g = g, f.z = z, f.a = a, f.stats = stats, f.out = out, f.dout = dout;
  f.G = dparams, f.dxs = dxs, f.dx[0] = dx1, f.dx[1] = dx2;
  f.wd = base + w.wd, f.wdl = base + w.wdl, f.wq = base + w.wq, f.wpart = base + w.wpart, f.wdg = base + w.wdg;
  f.wdh = base + w.wdh, f.slots = base + w.slots;
  f.B = B, f.training = training;
  float* G = dparams;
  for (int stage = L; stage >= 0; --stage) {
    f.stage = stage;
    hipLaunchKernelGGL(finalmlp_bwd_kernel, dim3(tiles), dim3(FM_NTHR), lds, st, d, po, f);
    REC_LAUNCH_CHECK();
    const int ns = fm_slot_floats(d, stage);
    int rc;
    if (stage == L) {
      const int l = L - 1;
      rc = rec_slot_sum(REC_SLOTS_WAVE, ns, tiles, f.slots,
                        {{G + po.c1, G + po.c2, G + po.gamma[0][l], G + po.gamma[1][l]},
                         {o, o, 2 * d.w[0][l], 2 * d.w[1][l]}},
                        st);
    } else if (stage > 0) {
      const int l = stage;
      rc = rec_slot_sum(REC_SLOTS_WAVE, ns, tiles, f.slots,
                        {{G + po.b[0][l], G + po.b[1][l], G + po.gamma[0][l - 1], G + po.gamma[1][l - 1]},
                         {d.w[0][l], d.w[1][l], 2 * d.w[0][l - 1], 2 * d.w[1][l - 1]}},
                        st);
    } else {
      rc = rec_slot_sum(REC_SLOTS_WAVE, ns, tiles, f.slots,
                        {{G + po.b[0][0], G + po.b[1][0], G + po.bo[0], G + po.bh[0], G + po.bo[1], G + po.bh[1]},
                         {d.w[0][0], d.w[1][0], D, Hg1, D, Hg2}},
                        st);
    }
    if (rc) return rc;
  }
  const int lp = L - 1, d1 = d.w[0][lp], d2 = d.w[1][lp], h1 = d.hd(0), h2 = d.hd(1);
  const int S = mb_small_split(B), wtot = fm_small_floats(d);
  int big = fm_max(d1, d2) * o;
  big = fm_max(big, h1 * h2 * o);
  if (int rc = small_dw_launch(FmSmall{a, f.wdl, f.wq, Z, d.zoff(0, lp), d.zoff(1, lp), d1, d2, h1, h2, o}, 2 + n, big,
                               wtot, B, base + w.part, st))
    return rc;
  if (int rc = rec_slot_sum(REC_SLOTS_SERIAL, wtot, S, base + w.part,
                            {{G + po.W1, G + po.W2, G + po.W12}, {d1 * o, d2 * o, d1 * h2 * o}}, st))
    return rc;
  float* gws = base + w.gemm;
  const float* xg[2] = {x1, x2};
  for (int s = 0; s < 2; ++s) {
    const int hoff = s ? Hg1 : 0, Hg = d.Hg[s];
    if (int rc = fm_dw(d.Dx[s], Hg, B, xg[s], d.Dx[s], f.wdh + hoff, HG, G + po.Wh[s], gws, stream)) return rc;
    if (int rc = fm_dw(Hg, D, B, hg + hoff, HG, f.wdg + s * D, 2 * D, G + po.Wo[s], gws, stream)) return rc;
    for (int l = 0; l < L; ++l) {
      const float* A = l ? a + d.zoff(s, l - 1) : f.wpart + s * D;
      if (int rc = fm_dw(l ? d.w[s][l - 1] : D, d.w[s][l], B, A, l ? Z : 2 * D, f.wd + d.zoff(s, l), Z,
                         G + po.W[s][l], gws, stream))
        return rc;
    }
  }
  return REC_OK;
}
