// AutoInt attention (TransformerAttentionLayer / AutoIntLayer, 3.DCN/CustomLayers.py:1012-1139) on gfx950.  Per example
// X [F,E], H heads of width d = E/H (head h owns the columns [h d, (h+1) d)):
//   Q = X Wq   K = X Wk   V = X Wv                 S[h,b,i,j] = scale * Q_h[b,i,:] . K_h[b,j,:]
//   P[h,b,i,j] = exp(S[h,b,i,j]) / sum_b' exp(S[h,b',i,j])      -- softmax over the BATCH axis, as the reference's
//                                                                  tf.nn.softmax(axis=1) on (H, B, F, F)
//   O[b,i,h d + c] = sum_j P[h,b,i,j] V[b,j,h d + c]    Z = O (+ X | + X Wres)    Y = relu(Z)
// The continuous fields of AutoIntLayer's first layer (cemb[c,:] * x_cont[b,c], fields Fc .. F-1) are assembled in the
// LDS load; x holds the Fc categorical fields only.
//
// Every (h,i,j) couples the whole batch, so each direction is two passes over the examples:
//   autoint_fwd_stats_kernel  persistent grid; each workgroup keeps an online (max, sum exp) of every (h,i,j) over
//                             its tiles in a workspace slot of its own
//   autoint_ml_reduce_kernel  merges the slots in slot order (one wave per (h,i,j), fixed butterfly): M, 1/L
//   autoint_fwd_out_kernel    recomputes Q, K, V from X (F E floats per example, cheaper to re-read than H F F scores)
//                             and writes Y (and O when asked for)
//   autoint_bwd_stats_kernel  c[h,i,j] = sum_b P dP, dP = dZ_h V_h^T, dZ = dY (Y > 0), per slot, then a slot-order sum
//   autoint_bwd_main_kernel   dS = scale P (dP - c); dQ_i = sum_j dS K_j, dK_j = sum_i dS Q_i, dV_j = sum_i P dZ_i;
//                             dX = dQ Wq^T + dK Wk^T + dV Wv^T + residual path; dW = X^T dQ, ... into a slot per
//                             workgroup, summed in slot order
// The products run on the VALU, not on v_mfma_f32_16x16x4_f32: at the shapes this layer is used with (E = 8 or 16,
// head width 4 or 8, F = 13 .. 29) a 16-wide tile would be mostly padding, and the whole layer is ~10-100 kflop per
// example against F E 4 bytes of X; the launches are bound by latency and LDS, not by the fp32 rate.
// Scores and dP are recomputed with one fixed fma order in every kernel (fp contraction is off in this file), so M is
// exactly the max of the scores the later passes see: at B = 1, P == 1 and dS == 0 exactly.  No float atomics:
// gradients are bit-identical run to run.  No host synchronisation: every launch can be captured in a graph.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AI_NT = 256;
constexpr int AI_MAXF = REC_AUTOINT_MAX_F, AI_MAXE = REC_AUTOINT_MAX_E;
constexpr int AI_MAXG = 512;                   // workgroups (= workspace slots) of the persistent kernels
constexpr int AI_TBMAX = 32;                   // examples per tile
constexpr int AI_LDS_SOFT = 16384;             // floats of LDS a tile aims for (64 KiB: two workgroups per CU)
constexpr size_t AI_LDS_MAX = REC_LDS_CU_BYTES;   // one example of the backward needs <= 128 KiB
enum { AI_RES_NONE = REC_AUTOINT_RES_NONE, AI_RES_ADD = REC_AUTOINT_RES_ADD, AI_RES_LEARNED = REC_AUTOINT_RES_LEARNED };
static_assert(AI_RES_NONE < AI_RES_ADD && AI_RES_ADD < AI_RES_LEARNED && AI_RES_LEARNED - AI_RES_NONE == 2,
              "ai_shape takes the residual kinds as a range");

struct AiShape {
  int64_t B;
  int F, E, H, d, C, Fc, res, HFF, nmat, nWE;  // nmat: weight matrices with a gradient (3, or 4 with Wres)
  float scale;
};

struct AiCfg {
  int tb[4];        // examples per tile: fwd stats, fwd out, bwd stats, bwd main
  int grid[4];
  size_t lds[4];
};

__device__ __forceinline__ float ai_dot(const float* __restrict__ a, const float* __restrict__ b, int d) {
  float acc = 0.f;
  for (int c = 0; c < d; ++c) acc = fmaf(a[c], b[c], acc);
  return acc;
}

// X tile [nb, F, E] into LDS: categorical rows from x [B, Fc, E], continuous rows cemb[c, :] * x_cont[b, c]
__device__ __forceinline__ void ai_load_x(const AiShape& s, const float* __restrict__ x, const float* __restrict__ xc,
                                          const float* __restrict__ ce, int64_t b0, int nb, float* __restrict__ Xs) {
  const int FE = s.F * s.E;
  for (int t = threadIdx.x; t < nb * FE; t += AI_NT) {
    const int b = t / FE, r = t - b * FE, f = r / s.E, e = r - f * s.E;
    Xs[t] = f < s.Fc ? x[((b0 + b) * s.Fc + f) * s.E + e] : ce[(f - s.Fc) * s.E + e] * xc[(b0 + b) * s.C + (f - s.Fc)];
  }
}

// out[b,f,e] = sum_k Xs[b,f,k] W[k,e], in one fma order (every kernel recomputes the same bits)
__device__ __forceinline__ void ai_project(const AiShape& s, const float* __restrict__ Xs, const float* __restrict__ W,
                                           int nb, float* __restrict__ out) {
  const int E = s.E;
  for (int t = threadIdx.x; t < nb * s.F * E; t += AI_NT) {
    const int e = t % E;
    const float* xr = Xs + (t - e);
    float acc = 0.f;
    for (int k = 0; k < E; ++k) acc = fmaf(xr[k], W[k * E + e], acc);
    out[t] = acc;
  }
}

__device__ __forceinline__ void ml_merge(float& m, float& l, float m2, float l2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  l = l * expf(m - mn) + l2 * expf(m2 - mn);
  m = mn;
}

// ------------------------------------------------------------------------------------------------------------------
// forward pass 1: slot [2][HFF] of workgroup g = (max, sum exp) of S[h,:,i,j] over its tiles g, g + grid, ...
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AI_NT) void autoint_fwd_stats_kernel(AiShape s, int TB, const float* __restrict__ x,
                                                                  const float* __restrict__ xc,
                                                                  const float* __restrict__ ce,
                                                                  const float* __restrict__ Wq,
                                                                  const float* __restrict__ Wk, float* __restrict__ ml) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E, FE = F * E, d = s.d;
  float* Xs = lds;
  float* Qs = Xs + TB * FE;
  float* Ks = Qs + TB * FE;
  float* __restrict__ slot = ml + (int64_t)blockIdx.x * 2 * s.HFF;
  const int64_t ntiles = (s.B + TB - 1) / TB;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const bool first = tl == (int64_t)blockIdx.x;
    const int64_t b0 = tl * TB;
    const int nb = (int)min((int64_t)TB, s.B - b0);
    ai_load_x(s, x, xc, ce, b0, nb, Xs);
    __syncthreads();
    ai_project(s, Xs, Wq, nb, Qs);
    ai_project(s, Xs, Wk, nb, Ks);
    __syncthreads();
    for (int t = threadIdx.x; t < s.HFF; t += AI_NT) {
      const int h = t / (F * F), r = t - h * F * F, i = r / F, j = r - i * F;
      const float* qi = Qs + i * E + h * d;
      const float* kj = Ks + j * E + h * d;
      float mt = -INFINITY;
      for (int b = 0; b < nb; ++b) mt = fmaxf(mt, ai_dot(qi + b * FE, kj + b * FE, d) * s.scale);
      float lt = 0.f;
      for (int b = 0; b < nb; ++b) lt += expf(ai_dot(qi + b * FE, kj + b * FE, d) * s.scale - mt);
      if (first) {
        slot[t] = mt;
        slot[s.HFF + t] = lt;
      } else {
        float m = slot[t], l = slot[s.HFF + t];
        ml_merge(m, l, mt, lt);
        slot[t] = m;
        slot[s.HFF + t] = l;
      }
    }
    __syncthreads();                                           // the next tile rewrites the LDS
  }
}

// stats [2][HFF] = (M, 1/L): one wave per (h,i,j); lane l merges the slots l, l + 64, ... in order, then a fixed
// butterfly (merge(a, b) and merge(b, a) give the same bits)
__global__ __launch_bounds__(256) void autoint_ml_reduce_kernel(int HFF, int nslot, const float* __restrict__ ml,
                                                                float* __restrict__ stats) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= HFF) return;
  float m = -INFINITY, l = 0.f;
  for (int sl = lane; sl < nslot; sl += 64) ml_merge(m, l, ml[(int64_t)sl * 2 * HFF + t], ml[(int64_t)sl * 2 * HFF + HFF + t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
    ml_merge(m, l, m2, l2);
  }
  if (lane == 0) {
    stats[t] = m;
    stats[HFF + t] = 1.f / l;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// forward pass 2: grid = ceil(B / TB); one thread per (example, head, query field) of the tile; DC >= d
// ------------------------------------------------------------------------------------------------------------------
template <int DC>
__global__ __launch_bounds__(AI_NT) void autoint_fwd_out_kernel(AiShape s, int TB, const float* __restrict__ x,
                                                                const float* __restrict__ xc,
                                                                const float* __restrict__ ce,
                                                                const float* __restrict__ Wq,
                                                                const float* __restrict__ Wk,
                                                                const float* __restrict__ Wv,
                                                                const float* __restrict__ Wr,
                                                                const float* __restrict__ stats, float* __restrict__ y,
                                                                float* __restrict__ o) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E, FE = F * E, d = s.d, H = s.H;
  float* Xs = lds;
  float* Qs = Xs + TB * FE;
  float* Ks = Qs + TB * FE;
  float* Vs = Ks + TB * FE;
  const int64_t b0 = (int64_t)blockIdx.x * TB;
  const int nb = (int)min((int64_t)TB, s.B - b0);
  ai_load_x(s, x, xc, ce, b0, nb, Xs);
  __syncthreads();
  ai_project(s, Xs, Wq, nb, Qs);
  ai_project(s, Xs, Wk, nb, Ks);
  ai_project(s, Xs, Wv, nb, Vs);
  __syncthreads();
  for (int t = threadIdx.x; t < nb * H * F; t += AI_NT) {
    const int b = t / (H * F), r = t - b * H * F, h = r / F, i = r - h * F, hd = h * d;
    const float* qr = Qs + (b * F + i) * E + hd;
    float q[DC], acc[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      q[c] = c < d ? qr[c] : 0.f;
      acc[c] = 0.f;
    }
    const float* Mr = stats + (h * F + i) * F;
    const float* Lr = Mr + s.HFF;
    for (int j = 0; j < F; ++j) {
      const float* kj = Ks + (b * F + j) * E + hd;
      const float* vj = Vs + (b * F + j) * E + hd;
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < DC; ++c)
        if (c < d) a = fmaf(q[c], kj[c], a);
      const float p = expf(a * s.scale - Mr[j]) * Lr[j];
#pragma unroll
      for (int c = 0; c < DC; ++c)
        if (c < d) acc[c] = fmaf(p, vj[c], acc[c]);
    }
    const float* xr = Xs + (b * F + i) * E;
    const int64_t grow = ((b0 + b) * F + i) * E + hd;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      if (c >= d) continue;
      float z = acc[c];
      if (o) o[grow + c] = z;
      if (s.res == AI_RES_ADD) {
        z += xr[hd + c];
      } else if (s.res == AI_RES_LEARNED) {
        float rr = 0.f;
        for (int k = 0; k < E; ++k) rr = fmaf(xr[k], Wr[k * E + hd + c], rr);
        z += rr;
      }
      y[grow + c] = fmaxf(z, 0.f);
    }
  }
}

// dZ tile = dY where Y > 0 (the ReLU mask z > 0, read back from Y = relu(z))
__device__ __forceinline__ void ai_load_dz(const AiShape& s, const float* __restrict__ y, const float* __restrict__ dy,
                                           int64_t b0, int nb, float* __restrict__ Ds) {
  const int FE = s.F * s.E;
  const float* yr = y + b0 * FE;
  const float* gr = dy + b0 * FE;
  for (int t = threadIdx.x; t < nb * FE; t += AI_NT) Ds[t] = yr[t] > 0.f ? gr[t] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// backward pass 1: slot [HFF] of workgroup g = sum over its tiles of P dP
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AI_NT) void autoint_bwd_stats_kernel(AiShape s, int TB, const float* __restrict__ x,
                                                                  const float* __restrict__ xc,
                                                                  const float* __restrict__ ce,
                                                                  const float* __restrict__ Wq,
                                                                  const float* __restrict__ Wk,
                                                                  const float* __restrict__ Wv,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ dy,
                                                                  const float* __restrict__ stats,
                                                                  float* __restrict__ cs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E, FE = F * E, d = s.d;
  float* Xs = lds;
  float* Qs = Xs + TB * FE;
  float* Ks = Qs + TB * FE;
  float* Vs = Ks + TB * FE;
  float* Ds = Vs + TB * FE;
  float* __restrict__ slot = cs + (int64_t)blockIdx.x * s.HFF;
  const int64_t ntiles = (s.B + TB - 1) / TB;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const bool first = tl == (int64_t)blockIdx.x;
    const int64_t b0 = tl * TB;
    const int nb = (int)min((int64_t)TB, s.B - b0);
    ai_load_x(s, x, xc, ce, b0, nb, Xs);
    ai_load_dz(s, y, dy, b0, nb, Ds);
    __syncthreads();
    ai_project(s, Xs, Wq, nb, Qs);
    ai_project(s, Xs, Wk, nb, Ks);
    ai_project(s, Xs, Wv, nb, Vs);
    __syncthreads();
    for (int t = threadIdx.x; t < s.HFF; t += AI_NT) {
      const int h = t / (F * F), r = t - h * F * F, i = r / F, j = r - i * F;
      const float M = stats[t], iL = stats[s.HFF + t];
      const int oi = i * E + h * d, oj = j * E + h * d;
      float acc = 0.f;
      for (int b = 0; b < nb; ++b) {
        const float p = expf(ai_dot(Qs + b * FE + oi, Ks + b * FE + oj, d) * s.scale - M) * iL;
        acc = fmaf(p, ai_dot(Ds + b * FE + oi, Vs + b * FE + oj, d), acc);
      }
      slot[t] = first ? acc : slot[t] + acc;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward pass 2: persistent grid; LDS X | Q | K | V | dZ | dQ | dK | dV, each [TB, F, E]
// slot of workgroup g [nWE] = dWq | dWk | dWv | dWres (AI_RES_LEARNED) | dcemb [C, E]
// ------------------------------------------------------------------------------------------------------------------
template <int DC>
__global__ __launch_bounds__(AI_NT) void autoint_bwd_main_kernel(AiShape s, int TB, const float* __restrict__ x,
                                                                 const float* __restrict__ xc,
                                                                 const float* __restrict__ ce,
                                                                 const float* __restrict__ Wq,
                                                                 const float* __restrict__ Wk,
                                                                 const float* __restrict__ Wv,
                                                                 const float* __restrict__ Wr,
                                                                 const float* __restrict__ y,
                                                                 const float* __restrict__ dy,
                                                                 const float* __restrict__ stats,
                                                                 const float* __restrict__ cvec,
                                                                 float* __restrict__ dx, float* __restrict__ dws) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E, FE = F * E, d = s.d, H = s.H, EE = E * E;
  float* Xs = lds;
  float* Qs = Xs + TB * FE;
  float* Ks = Qs + TB * FE;
  float* Vs = Ks + TB * FE;
  float* Ds = Vs + TB * FE;
  float* GQ = Ds + TB * FE;
  float* GK = GQ + TB * FE;
  float* GV = GK + TB * FE;
  float* __restrict__ slot = dws + (int64_t)blockIdx.x * s.nWE;
  const int64_t ntiles = (s.B + TB - 1) / TB;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const bool first = tl == (int64_t)blockIdx.x;
    const int64_t b0 = tl * TB;
    const int nb = (int)min((int64_t)TB, s.B - b0);
    ai_load_x(s, x, xc, ce, b0, nb, Xs);
    ai_load_dz(s, y, dy, b0, nb, Ds);
    __syncthreads();
    ai_project(s, Xs, Wq, nb, Qs);
    ai_project(s, Xs, Wk, nb, Ks);
    ai_project(s, Xs, Wv, nb, Vs);
    __syncthreads();

    for (int t = threadIdx.x; t < nb * H * F; t += AI_NT) {
      const int b = t / (H * F), r = t - b * H * F, h = r / F, f = r - h * F, hd = h * d;
      const int bo = b * FE;
      const float* Mh = stats + h * F * F;
      const float* Lh = Mh + s.HFF;
      const float* ch = cvec + h * F * F;
      {  // row f as the query: dQ_f = sum_j dS[f,j] K_j
        float q[DC], dz[DC], acc[DC];
#pragma unroll
        for (int c = 0; c < DC; ++c) {
          q[c] = c < d ? Qs[bo + f * E + hd + c] : 0.f;
          dz[c] = c < d ? Ds[bo + f * E + hd + c] : 0.f;
          acc[c] = 0.f;
        }
        for (int j = 0; j < F; ++j) {
          const float* kj = Ks + bo + j * E + hd;
          const float* vj = Vs + bo + j * E + hd;
          float a = 0.f, dp = 0.f;
#pragma unroll
          for (int c = 0; c < DC; ++c)
            if (c < d) a = fmaf(q[c], kj[c], a);
#pragma unroll
          for (int c = 0; c < DC; ++c)
            if (c < d) dp = fmaf(dz[c], vj[c], dp);
          const int ij = f * F + j;
          const float p = expf(a * s.scale - Mh[ij]) * Lh[ij];
          const float ds = p * (dp - ch[ij]) * s.scale;
#pragma unroll
          for (int c = 0; c < DC; ++c)
            if (c < d) acc[c] = fmaf(ds, kj[c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < DC; ++c)
          if (c < d) GQ[bo + f * E + hd + c] = acc[c];
      }
      {  // row f as the key / value: dK_f = sum_i dS[i,f] Q_i, dV_f = sum_i P[i,f] dZ_i
        float k[DC], v[DC], ak[DC], av[DC];
#pragma unroll
        for (int c = 0; c < DC; ++c) {
          k[c] = c < d ? Ks[bo + f * E + hd + c] : 0.f;
          v[c] = c < d ? Vs[bo + f * E + hd + c] : 0.f;
          ak[c] = 0.f;
          av[c] = 0.f;
        }
        for (int i = 0; i < F; ++i) {
          const float* qi = Qs + bo + i * E + hd;
          const float* di = Ds + bo + i * E + hd;
          float a = 0.f, dp = 0.f;
#pragma unroll
          for (int c = 0; c < DC; ++c)
            if (c < d) a = fmaf(qi[c], k[c], a);
#pragma unroll
          for (int c = 0; c < DC; ++c)
            if (c < d) dp = fmaf(di[c], v[c], dp);
          const int ij = i * F + f;
          const float p = expf(a * s.scale - Mh[ij]) * Lh[ij];
          const float ds = p * (dp - ch[ij]) * s.scale;
#pragma unroll
          for (int c = 0; c < DC; ++c)
            if (c < d) {
              ak[c] = fmaf(ds, qi[c], ak[c]);
              av[c] = fmaf(p, di[c], av[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < DC; ++c)
          if (c < d) {
            GK[bo + f * E + hd + c] = ak[c];
            GV[bo + f * E + hd + c] = av[c];
          }
      }
    }
    __syncthreads();

    // dX = dQ Wq^T + dK Wk^T + dV Wv^T + (dZ | dZ Wres^T); categorical rows to dx, continuous rows into Qs (free now)
    for (int t = threadIdx.x; t < nb * FE; t += AI_NT) {
      const int b = t / FE, rr = t - b * FE, f = rr / E, k = rr - f * E;
      const float* gq = GQ + (t - k);
      const float* gk = GK + (t - k);
      const float* gv = GV + (t - k);
      float acc = 0.f;
      for (int e = 0; e < E; ++e) {
        acc = fmaf(gq[e], Wq[k * E + e], acc);
        acc = fmaf(gk[e], Wk[k * E + e], acc);
        acc = fmaf(gv[e], Wv[k * E + e], acc);
      }
      if (s.res == AI_RES_ADD) {
        acc += Ds[t];
      } else if (s.res == AI_RES_LEARNED) {
        const float* dz = Ds + (t - k);
        for (int e = 0; e < E; ++e) acc = fmaf(dz[e], Wr[k * E + e], acc);
      }
      if (f < s.Fc)
        dx[((b0 + b) * s.Fc + f) * E + k] = acc;
      else
        Qs[t] = acc;
    }
    __syncthreads();

    // this tile's weight gradients, added to the workgroup's slot
    for (int t = threadIdx.x; t < s.nWE; t += AI_NT) {
      float acc = 0.f;
      if (t < s.nmat * EE) {
        const int m = t / EE, r2 = t - m * EE, k = r2 / E, e = r2 - k * E;
        const float* G = m == 0 ? GQ : (m == 1 ? GK : (m == 2 ? GV : Ds));
        for (int b = 0; b < nb; ++b)
          for (int f = 0; f < F; ++f) acc = fmaf(Xs[b * FE + f * E + k], G[b * FE + f * E + e], acc);
      } else {
        const int r2 = t - s.nmat * EE, c = r2 / E, e = r2 - c * E;
        for (int b = 0; b < nb; ++b) acc = fmaf(xc[(b0 + b) * s.C + c], Qs[b * FE + (s.Fc + c) * E + e], acc);
      }
      slot[t] = first ? acc : slot[t] + acc;
    }
    __syncthreads();                                           // the next tile rewrites the LDS
  }
}

// 0 ok (B == 0 included), REC_E_ARG, REC_E_UNSUPPORTED
static int ai_shape(int64_t B, int F, int E, int H, int C, int res, int scaling, AiShape* s) {
  if (B < 0 || F < 0 || E < 0 || H < 0 || C < 0 || res < AI_RES_NONE || res > AI_RES_LEARNED || scaling < 0 ||
      scaling > 1)
    return REC_E_ARG;
  if (F < 1 || F > AI_MAXF || E < 1 || E > AI_MAXE || H < 1 || H > E || E % H != 0 || C >= F) return REC_E_UNSUPPORTED;
  if (B > 0x7fffffffLL || B > ((int64_t)1 << 40) / ((int64_t)F * E)) return REC_E_UNSUPPORTED;
  *s = AiShape{};
  s->B = B;
  s->F = F;
  s->E = E;
  s->H = H;
  s->d = E / H;
  s->C = C;
  s->Fc = F - C;
  s->res = res;
  s->HFF = H * F * F;
  s->nmat = res == AI_RES_LEARNED ? 4 : 3;
  s->nWE = s->nmat * E * E + C * E;
  s->scale = scaling ? (float)(1.0 / sqrt((double)s->d)) : 1.f;
  return REC_OK;
}

static AiCfg ai_cfg(const AiShape& s) {
  AiCfg k{};
  const int per[4] = {3, 4, 5, 8};                       // [TB, F, E] arrays in LDS
  const int FE = s.F * s.E;
  for (int q = 0; q < 4; ++q) {
    int tb = AI_LDS_SOFT / (per[q] * FE);
    tb = tb < 1 ? 1 : (tb > AI_TBMAX ? AI_TBMAX : tb);
    const int64_t ntiles = (s.B + tb - 1) / tb;
    k.tb[q] = tb;
    k.grid[q] = (int)(q == 1 ? ntiles : (ntiles < AI_MAXG ? ntiles : AI_MAXG));
    if (k.grid[q] < 1) k.grid[q] = 1;
    k.lds[q] = (size_t)tb * per[q] * FE * sizeof(float);
  }
  return k;
}

static size_t ai_align(size_t n) { return rec_align_up(n * sizeof(float), 256); }

// forward: ml slots [grid0][2][HFF]; backward: c slots [grid2][HFF] | c [HFF] | dW slots [grid3][nWE]
static size_t ai_ws_bytes(const AiShape& s, const AiCfg& k) {
  const size_t fwd = ai_align((size_t)k.grid[0] * 2 * s.HFF);
  const size_t bwd = ai_align((size_t)k.grid[2] * s.HFF) + ai_align((size_t)s.HFF) + ai_align((size_t)k.grid[3] * s.nWE);
  return fwd > bwd ? fwd : bwd;
}

template <int DC>
static int ai_fwd_out(const AiShape& s, const AiCfg& k, const float* x, const float* xc, const float* ce,
                      const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* stats, float* y,
                      float* o, hipStream_t st) {
  if (hipError_t e = rec_allow_lds<autoint_fwd_out_kernel<DC>>(AI_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(autoint_fwd_out_kernel<DC>, dim3(k.grid[1]), dim3(AI_NT), k.lds[1], st, s, k.tb[1], x, xc, ce, Wq,
                     Wk, Wv, Wr, stats, y, o);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

template <int DC>
static int ai_bwd_main(const AiShape& s, const AiCfg& k, const float* x, const float* xc, const float* ce,
                       const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* y,
                       const float* dy, const float* stats, const float* cvec, float* dx, float* dws, hipStream_t st) {
  if (hipError_t e = rec_allow_lds<autoint_bwd_main_kernel<DC>>(AI_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(autoint_bwd_main_kernel<DC>, dim3(k.grid[3]), dim3(AI_NT), k.lds[3], st, s, k.tb[3], x, xc, ce,
                     Wq, Wk, Wv, Wr, y, dy, stats, cvec, dx, dws);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

}  // namespace

extern "C" size_t rec_autoint_workspace_bytes(int64_t B, int F, int E, int H, int C, int res) {
  AiShape s;
  if (ai_shape(B, F, E, H, C, res, 0, &s) != REC_OK) return 0;
  return ai_ws_bytes(s, ai_cfg(s));
}

extern "C" int rec_autoint_fwd_f32(const float* x, const float* x_cont, const float* cemb, const float* Wq,
                                   const float* Wk, const float* Wv, const float* Wres, int64_t B, int F, int E, int H,
                                   int C, int res, int scaling, float* y, float* o, float* stats, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  AiShape s;
  const int rc = ai_shape(B, F, E, H, C, res, scaling, &s);
  if (rc != REC_OK || B == 0) return rc;
  if (!x || (C > 0 && (!x_cont || !cemb)) || !Wq || !Wk || !Wv || (res == AI_RES_LEARNED && !Wres) || !y || !stats ||
      !workspace)
    return REC_E_ARG;
  const AiCfg k = ai_cfg(s);
  if (workspace_bytes < ai_ws_bytes(s, k)) return REC_E_WORKSPACE;
  float* ml = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  if (hipError_t e = rec_allow_lds<autoint_fwd_stats_kernel>(AI_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(autoint_fwd_stats_kernel, dim3(k.grid[0]), dim3(AI_NT), k.lds[0], st, s, k.tb[0], x, x_cont, cemb,
                     Wq, Wk, ml);
  REC_LAUNCH_CHECK();
  hipLaunchKernelGGL(autoint_ml_reduce_kernel, dim3((s.HFF + 3) / 4), dim3(256), 0, st, s.HFF, k.grid[0], ml, stats);
  REC_LAUNCH_CHECK();
  switch (s.d) {
    case 1: return ai_fwd_out<1>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, stats, y, o, st);
    case 2: return ai_fwd_out<2>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, stats, y, o, st);
    case 3: case 4: return ai_fwd_out<4>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, stats, y, o, st);
    case 5: case 6: case 7: case 8: return ai_fwd_out<8>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, stats, y, o, st);
    default:
      if (s.d <= 16) return ai_fwd_out<16>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, stats, y, o, st);
      if (s.d <= 32) return ai_fwd_out<32>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, stats, y, o, st);
      return ai_fwd_out<64>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, stats, y, o, st);
  }
}

extern "C" int rec_autoint_bwd_f32(const float* x, const float* x_cont, const float* cemb, const float* Wq,
                                   const float* Wk, const float* Wv, const float* Wres, const float* y, const float* dy,
                                   const float* stats, int64_t B, int F, int E, int H, int C, int res, int scaling,
                                   float* dx, float* dWq, float* dWk, float* dWv, float* dWres, float* dcemb,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  AiShape s;
  const int rc = ai_shape(B, F, E, H, C, res, scaling, &s);
  if (rc != REC_OK || B == 0) return rc;
  if (!x || (C > 0 && (!x_cont || !cemb || !dcemb)) || !Wq || !Wk || !Wv ||
      (res == AI_RES_LEARNED && (!Wres || !dWres)) || !y || !dy || !stats || !dx || !dWq || !dWk || !dWv || !workspace)
    return REC_E_ARG;
  const AiCfg k = ai_cfg(s);
  if (workspace_bytes < ai_ws_bytes(s, k)) return REC_E_WORKSPACE;
  float* cs = static_cast<float*>(workspace);
  float* cvec = reinterpret_cast<float*>(reinterpret_cast<char*>(cs) + ai_align((size_t)k.grid[2] * s.HFF));
  float* dws = reinterpret_cast<float*>(reinterpret_cast<char*>(cvec) + ai_align((size_t)s.HFF));
  hipStream_t st = as_stream(stream);
  if (hipError_t e = rec_allow_lds<autoint_bwd_stats_kernel>(AI_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(autoint_bwd_stats_kernel, dim3(k.grid[2]), dim3(AI_NT), k.lds[2], st, s, k.tb[2], x, x_cont, cemb,
                     Wq, Wk, Wv, y, dy, stats, cs);
  REC_LAUNCH_CHECK();
  int r = rec_slot_sum(REC_SLOTS_WAVE, s.HFF, k.grid[2], cs, {{cvec}, {s.HFF}}, st);
  if (r != REC_OK) return r;
  switch (s.d) {
    case 1: r = ai_bwd_main<1>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, y, dy, stats, cvec, dx, dws, st); break;
    case 2: r = ai_bwd_main<2>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, y, dy, stats, cvec, dx, dws, st); break;
    case 3: case 4: r = ai_bwd_main<4>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, y, dy, stats, cvec, dx, dws, st); break;
    case 5: case 6: case 7: case 8:
      r = ai_bwd_main<8>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, y, dy, stats, cvec, dx, dws, st);
      break;
    default:
      if (s.d <= 16)
        r = ai_bwd_main<16>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, y, dy, stats, cvec, dx, dws, st);
      else if (s.d <= 32)
        r = ai_bwd_main<32>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, y, dy, stats, cvec, dx, dws, st);
      else
        r = ai_bwd_main<64>(s, k, x, x_cont, cemb, Wq, Wk, Wv, Wres, y, dy, stats, cvec, dx, dws, st);
      break;
  }
  if (r != REC_OK) return r;
  const int EE = E * E;
  return rec_slot_sum(REC_SLOTS_WAVE, s.nWE, k.grid[3], dws,
                      {{dWq, dWk, dWv, res == AI_RES_LEARNED ? dWres : dcemb, dcemb},
                       {EE, EE, EE, res == AI_RES_LEARNED ? EE : C * E, res == AI_RES_LEARNED ? C * E : 0}}, st);
}
