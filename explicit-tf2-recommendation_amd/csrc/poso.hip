// POSO-MLP (PosoForMLPLayer, 10.POSO/CustomLayers.py:92-119; the task towers of PEPNetLayer, :371-462) on gfx950: T
// stacked MLPs of L chained layers whose every layer is scaled by a GateNU of a second input,
//   gate_ti = 2 sigmoid(relu(g Wg1_ti + bg1_ti) Wg2_ti + bg2_ti)        a_ti = act_i(C_ti ((a_t,i-1 W_ti + b_ti) (.) gate_ti))
// with a_t,-1 = x.  x [B, Dm] and g [B, Dg] have row strides of their own (both may point into one buffer).
// Packed weights (sumU = sum U_i, H_i = m U_i, NG = T m sumU, K_0 = Dm, K_i = U_{i-1}); (t, i) runs task-major:
//   Wg1 [Dg, NG], bg1 [NG]   the first gate layers of all tasks and layers side by side: ONE matrix, so its gradient is
//                            one product g^T dZ; the columns of (t, i) start at m (t sumU + U_0 + .. + U_{i-1})
//   Wg2  the [H_i, U_i] of every (t, i) one after the other, bg2 [T, sumU]
//   W    the [K_i, U_i] of every (t, i) one after the other, b [T, sumU], C [T, L]
// Forward, one launch.  A workgroup of 4 waves owns 32 examples (mfma_tile.h); the g tile stays k-major in LDS for the
// whole kernel.  Per (t, i): the column group of g Wg1 on v_mfma_f32_32x32x2_f32 (<= 512 columns: the 4 x 4 x 32
// accumulator columns of mb_mma) -> relu -> LDS; the gate's second layer and the dense product are both [32, U_i <= 128]
// products, one 32-column block per wave, and land in the SAME accumulator layout: the gate multiply, C and the
// activation happen in registers, the activation goes k-major to LDS as the next layer's operand.  The x tile shares
// the LDS of the gate hidden (it is read again per task, from L2).  NG is walked by column group, never whole: at the
// limits it is 2048 columns.
// Training saves h (gate hidden), gate, d (the dense output) and a; inference writes out alone, the same bits.
// Backward, one launch for the per-example chain: the layers of a task in reverse, the gradient of a layer's input
// staying in registers (the layout again matches); dx adds up over the tasks in place (one owner per element, tasks in
// order) and dg = dZ Wg1^T is ONE product over all NG columns at the end, its operand read back from the workspace
// copy of dZ that the weight gradient needs anyway.  The tile's column sums (bias gradients, dC) go to the tile's slot; the entry point adds the slots
// (rec_slot_sum), runs all dW and dWg2 as one small_dw launch (matrices cut into row blocks of 128) whose batch slices a
// second slot sum adds in order, and enqueues dWg1 = g^T dZ on rec_gemm_f32 (split-K, slices added in order).
// No float atomics and no value with two writers: bit-identical results run to run; no host synchronisation.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

namespace {

constexpr int PO_MAXT = REC_MASKNET_MAX_R, PO_MAXL = REC_MASKNET_MAX_R, PO_MAXU = REC_MASKNET_MAX_O;
constexpr int PO_MAXH = REC_MASKNET_MAX_P, PO_MAXD = REC_MASKNET_MAX_D;
constexpr int PO_NTHR = 256;
constexpr int PO_MB = 128;                       // rows of a block of a small weight gradient
constexpr size_t PO_LDS_CAP = REC_POSO_LDS_CAP;

static_assert(PO_MAXH <= 128 * MB_NJ && PO_MAXD <= 128 * MB_NJ && PO_MAXU <= 128, "accumulator blocks per wave");
static_assert(PO_LDS_CAP <= REC_LDS_CU_BYTES, "LDS of a CU");

struct PoDims {
  int Dm, Dg, T, L, m;
  int U0, U1, U2, U3, A0, A1, A2, A3;            // members and selects, not arrays: a kernel argument indexed by a
                                                 // variable would be copied to scratch
  __host__ __device__ int U(int i) const { return i == 0 ? U0 : (i == 1 ? U1 : (i == 2 ? U2 : U3)); }
  __host__ __device__ int act(int i) const { return i == 0 ? A0 : (i == 1 ? A1 : (i == 2 ? A2 : A3)); }
  __host__ __device__ int K(int i) const { return i ? U(i - 1) : Dm; }
  __host__ __device__ int preU(int i) const {
    int s = 0;
    for (int j = 0; j < i; ++j) s += U(j);
    return s;
  }
  __host__ __device__ int preW(int i) const {    // floats of W before layer i of a task
    int s = 0;
    for (int j = 0; j < i; ++j) s += K(j) * U(j);
    return s;
  }
  __host__ __device__ int preW2(int i) const {
    int s = 0;
    for (int j = 0; j < i; ++j) s += m * U(j) * U(j);
    return s;
  }
  __host__ __device__ int sumU() const { return preU(L); }
  __host__ __device__ int NG() const { return T * m * sumU(); }
  __host__ __device__ int Umax() const {
    int s = 0;
    for (int j = 0; j < L; ++j) s = U(j) > s ? U(j) : s;
    return s;
  }
};

__host__ __device__ inline int po_max(int a, int b) { return a > b ? a : b; }
// rows of LDS ([.][33] floats each):
//   forward   gs [even(Dg)] | buf [max(even(m Umax), even(Dm))] | a0 [even(Umax)] | a1 [even(Umax)] (L > 1)
//   backward  dds [even(Umax)] | dps [even(Umax)] | dcs [Umax] | tmp [4] | dzs [even(m Umax)]
__host__ __device__ inline size_t po_lds_floats(const PoDims& d, int bwd) {
  const int Ue = mb_even(d.Umax()), He = mb_even(d.m * d.Umax());
  const int rows = bwd ? 3 * Ue + 4 + He : mb_even(d.Dg) + po_max(He, mb_even(d.Dm)) + (d.L > 1 ? 2 : 1) * Ue;
  return (size_t)rows * MB_LD;
}
static_assert(sizeof(float) * (3 * PO_MAXU + 4 + PO_MAXH) * MB_LD <= PO_LDS_CAP, "the backward of the largest shape fits");

// the row after an operand of odd K is zero: mb_mma reads it
__device__ __forceinline__ void po_pad(float* buf, int K, int tid) {
  if ((K & 1) && tid < MB_T) buf[K * MB_LD + tid] = 0.f;
}

__device__ __forceinline__ float po_act(float z, int act) {
  return act == REC_ACT_RELU ? fmaxf(z, 0.f) : (act == REC_ACT_SIGMOID ? sigmoid_acc(z) : z);
}
// act'(z) from a = act(z); relu'(0) = 0
__device__ __forceinline__ float po_dact(float a, int act) {
  return act == REC_ACT_RELU ? (a > 0.f ? 1.f : 0.f) : (act == REC_ACT_SIGMOID ? a * (1.f - a) : 1.f);
}

__global__ __launch_bounds__(PO_NTHR) void poso_fwd_kernel(
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ g, int64_t ldg,
    const float* __restrict__ Wg1, const float* __restrict__ bg1, const float* __restrict__ Wg2,
    const float* __restrict__ bg2, const float* __restrict__ W, const float* __restrict__ bw,
    const float* __restrict__ Cs, int64_t B, PoDims d, float* __restrict__ out, float* __restrict__ sh,
    float* __restrict__ sgate, float* __restrict__ sd, float* __restrict__ sa) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Dm = d.Dm, Dg = d.Dg, T = d.T, L = d.L, m = d.m;
  const int sumU = d.sumU(), NG = d.NG(), TU = T * sumU, UL = d.U(L - 1);
  const int Dge = mb_even(Dg), Dme = mb_even(Dm), Ue = mb_even(d.Umax());
  const int wtask = d.preW(L), w2task = d.preW2(L);
  float* gs = lds;                               // [even(Dg)][33]
  float* buf = gs + Dge * MB_LD;                 // the gate hidden of (t, i), then the x tile of layer 0
  float* a0 = buf + po_max(mb_even(m * d.Umax()), Dme) * MB_LD;
  float* a1 = a0 + Ue * MB_LD;
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;

  for (int i = tid; i < MB_T * Dge; i += PO_NTHR) {
    const int row = i / Dge, k = i - row * Dge;
    gs[k * MB_LD + row] = (k < Dg && r0 + row < B) ? g[(r0 + row) * ldg + k] : 0.f;
  }
  __syncthreads();

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
#pragma unroll 1
    for (int i = 0; i < L; ++i) {
      const int U = d.U(i), H = m * U, K = d.K(i);
      const int uoff = t * sumU + d.preU(i), goff = m * uoff;
      {
        f32x16 acc[MB_NJ];
#pragma unroll
        for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
        mb_mma<false>(acc, gs, Dg, Wg1 + goff, NG, 0, H, wave, lo, hi);
#pragma unroll
        for (int j = 0; j < MB_NJ; ++j) {
          const int col = (wave + 4 * j) * 32 + lo;
          if ((wave + 4 * j) * 32 < H && col < H) {
            const float bc = bg1[goff + col];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = mb_row(r, hi);
              const float hv = fmaxf(acc[j][r] + bc, 0.f);
              buf[col * MB_LD + row] = hv;
              if (sh && r0 + row < B) sh[(r0 + row) * NG + goff + col] = hv;
            }
          }
        }
        po_pad(buf, H, tid);
      }
      __syncthreads();
      const bool own = wave * 32 < U;            // uniform over the wave
      f32x16 ga, da;
      mb_zero(ga);
      mb_zero(da);
      if (own) mb_mma1<false>(ga, buf, H, Wg2 + (int64_t)t * w2task + d.preW2(i), U, 0, U, wave * 32, lo, hi);
      const float* in = (i - 1) & 1 ? a1 : a0;
      if (i == 0) {
        __syncthreads();                         // every read of the gate hidden lies before it
        for (int q = tid; q < MB_T * Dme; q += PO_NTHR) {
          const int row = q / Dme, k = q - row * Dme;
          buf[k * MB_LD + row] = (k < Dm && r0 + row < B) ? x[(r0 + row) * ldx + k] : 0.f;
        }
        __syncthreads();
        in = buf;
      }
      if (own) mb_mma1<false>(da, in, K, W + (int64_t)t * wtask + d.preW(i), U, 0, U, wave * 32, lo, hi);
      float* ao = i & 1 ? a1 : a0;
      const int col = wave * 32 + lo;
      if (own && col < U) {
        const float bgc = bg2[uoff + col], bc = bw[uoff + col], Cv = Cs[t * L + i];
        const int act = d.act(i);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mb_row(r, hi);
          const float gate = 2.f * sigmoid_acc(ga[r] + bgc);
          const float dv = da[r] + bc;
          const float av = po_act(Cv * (dv * gate), act);
          if (i + 1 < L) ao[col * MB_LD + row] = av;
          if (r0 + row < B) {
            const int64_t at = (r0 + row) * TU + uoff + col;
            if (sa) {
              sgate[at] = gate;
              sd[at] = dv;
              sa[at] = av;
            }
            if (i == L - 1) out[((r0 + row) * T + t) * UL + col] = av;
          }
        }
      }
      if (i + 1 < L) po_pad(ao, U, tid);
      __syncthreads();                           // buf and the other activation buffer may be rewritten
    }
  }
}

// slot of a tile: dbg1 [NG] | dbg2 [T sumU] | db [T sumU] | dC [T L]
__host__ __device__ inline int po_slot_floats(const PoDims& d) { return d.NG() + 2 * d.T * d.sumU() + d.T * d.L; }

using Tile = TileOps<MB_T, MB_LD, PO_NTHR>;

__global__ __launch_bounds__(PO_NTHR) void poso_bwd_kernel(
    const float* __restrict__ Wg1, const float* __restrict__ Wg2, const float* __restrict__ W,
    const float* __restrict__ Cs, const float* __restrict__ sh, const float* __restrict__ sgate,
    const float* __restrict__ sd, const float* __restrict__ sa, const float* __restrict__ dout, int64_t B, PoDims d,
    float* __restrict__ dx, float* __restrict__ dg, float* ws_dz, float* __restrict__ ws_dd,
    float* __restrict__ ws_dp, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Dm = d.Dm, Dg = d.Dg, T = d.T, L = d.L, m = d.m;
  const int sumU = d.sumU(), NG = d.NG(), TU = T * sumU, UL = d.U(L - 1);
  const int Ue = mb_even(d.Umax());
  const int wtask = d.preW(L), w2task = d.preW2(L);
  float* dds = lds;                              // [even(Umax)]: the gradient of the dense output
  float* dps = dds + Ue * MB_LD;                 // [even(Umax)]: the gradient before the gate's sigmoid
  float* dcs = dps + Ue * MB_LD;                 // [Umax]: the terms of dC
  float* tmp = dcs + d.Umax() * MB_LD;           // their column sums
  float* dzs = tmp + 4 * MB_LD;                  // [even(m Umax)]: the gradient before the gate's relu
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;
  float* __restrict__ slot_g1 = slots + (int64_t)blockIdx.x * po_slot_floats(d);
  float* __restrict__ slot_g2 = slot_g1 + NG;
  float* __restrict__ slot_b = slot_g2 + TU;
  float* __restrict__ slot_C = slot_b + TU;

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    f32x16 dA;
    mb_zero(dA);
#pragma unroll 1
    for (int i = L - 1; i >= 0; --i) {
      const int U = d.U(i), H = m * U, K = d.K(i);
      const int uoff = t * sumU + d.preU(i), goff = m * uoff;
      const bool own = wave * 32 < U;
      const int col = wave * 32 + lo;
      if (own && col < U) {
        const float Cv = Cs[t * L + i];
        const int act = d.act(i);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mb_row(r, hi);
          float dd = 0.f, dp = 0.f, dc = 0.f;
          if (r0 + row < B) {
            const int64_t at = (r0 + row) * TU + uoff + col;
            const float av = sa[at], gt = sgate[at], dv = sd[at];
            const float da = i == L - 1 ? dout[((r0 + row) * T + t) * UL + col] : dA[r];
            const float dz = da * po_dact(av, act);
            dc = dz * (dv * gt);
            dd = dz * (Cv * gt);
            dp = (dz * (Cv * dv)) * (gt * (1.f - 0.5f * gt));
            ws_dd[at] = dd;
            ws_dp[at] = dp;
          }
          dds[col * MB_LD + row] = dd;
          dps[col * MB_LD + row] = dp;
          dcs[col * MB_LD + row] = dc;
        }
      }
      po_pad(dds, U, tid);
      po_pad(dps, U, tid);
      __syncthreads();
      Tile::col_sums(slot_b + uoff, dds, U, tid);
      Tile::col_sums(slot_g2 + uoff, dps, U, tid);
      Tile::col_sums(tmp, dcs, U, tid);
      {
        f32x16 acc[MB_NJ];
#pragma unroll
        for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
        mb_mma<true>(acc, dps, U, Wg2 + (int64_t)t * w2task + d.preW2(i), U, 0, H, wave, lo, hi);
#pragma unroll
        for (int j = 0; j < MB_NJ; ++j) {
          const int ch = (wave + 4 * j) * 32 + lo;
          if ((wave + 4 * j) * 32 < H && ch < H) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = mb_row(r, hi);
              float v = 0.f;
              if (r0 + row < B) {
                const int64_t at = (r0 + row) * NG + goff + ch;
                v = sh[at] > 0.f ? acc[j][r] : 0.f;
                ws_dz[at] = v;
              }
              dzs[ch * MB_LD + row] = v;
            }
          }
        }
        po_pad(dzs, H, tid);
      }
      __syncthreads();
      Tile::col_sums(slot_g1 + goff, dzs, H, tid);
      if (tid == 0) {
        float s = 0.f;
        for (int c = 0; c < U; ++c) s += tmp[c];
        slot_C[t * L + i] = s;
      }
      if (i > 0) {
        mb_zero(dA);
        if (wave * 32 < K) mb_mma1<true>(dA, dds, U, W + (int64_t)t * wtask + d.preW(i), U, 0, K, wave * 32, lo, hi);
      } else {
        // dx += dd_t0 W_t0^T, the tasks in order: through dx itself (every element has one owner), which spares the
        // 64 accumulator registers a sum kept across the tasks would hold next to dgacc
        f32x16 acc[MB_NJ];
#pragma unroll
        for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
        mb_mma<true>(acc, dds, U, W + (int64_t)t * wtask, U, 0, Dm, wave, lo, hi);
#pragma unroll
        for (int j = 0; j < MB_NJ; ++j) {
          const int cx = (wave + 4 * j) * 32 + lo;
          if ((wave + 4 * j) * 32 < Dm && cx < Dm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = mb_row(r, hi);
              if (r0 + row < B) {
                float* p = dx + (r0 + row) * Dm + cx;
                *p = t == 0 ? acc[j][r] : *p + acc[j][r];
              }
            }
          }
        }
      }
      __syncthreads();                           // the operands are rewritten by the next layer
    }
  }
  // dg = dZ Wg1^T over all NG columns at once: the tile's dZ is read back from the workspace (its own writes, behind
  // the barrier above) in chunks as wide as the whole LDS, so no accumulator lives across the layers
  f32x16 dgacc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(dgacc[j]);
  const int CH = (int)(po_lds_floats(d, 1) / MB_LD) & ~1;
#pragma unroll 1
  for (int c0 = 0; c0 < NG; c0 += CH) {
    const int kc = NG - c0 < CH ? NG - c0 : CH;
    Tile::rows_in(lds, ws_dz, r0, B, NG, c0, kc, tid);
    po_pad(lds, kc, tid);
    __syncthreads();
    mb_mma<true>(dgacc, lds, kc, Wg1 + c0, NG, 0, Dg, wave, lo, hi);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int col = (wave + 4 * j) * 32 + lo;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mb_row(r, hi);
      if (r0 + row < B && (wave + 4 * j) * 32 < Dg && col < Dg) dg[(r0 + row) * Dg + col] = dgacc[j][r];
    }
  }
}

// The small weight gradients, all of them in one launch (small_dw_kernel, tile_ops.h): per (t, i) the row blocks of
// dW_ti = a_t,i-1^T dd_ti (x for i = 0) and then those of dWg2_ti = h_ti^T dp_ti, PO_MB rows each; the outputs lie as
// the packed gradients do, dW first, dWg2 after it.
__host__ __device__ inline int po_blocks(int rows) { return (rows + PO_MB - 1) / PO_MB; }
struct PoSmall {
  static constexpr int MAXK = PO_MB;
  PoDims d;
  const float* x;
  int ldx;
  const float *sh, *sa, *dd, *dp;
  __device__ SmallMat mat(int q) const {
    const int sumU = d.sumU(), TU = d.T * sumU, NG = d.NG(), wtask = d.preW(d.L), w2task = d.preW2(d.L);
    for (int t = 0; t < d.T; ++t)
      for (int i = 0; i < d.L; ++i) {
        const int U = d.U(i), K = d.K(i), H = d.m * U, uoff = t * sumU + d.preU(i);
        const int nk = po_blocks(K), nh = po_blocks(H);
        if (q < nk) {
          const int r = q * PO_MB, M = K - r < PO_MB ? K - r : PO_MB;
          if (i == 0) return {x, ldx, r, M, dd, TU, uoff, U, t * wtask + r * U, U};
          return {sa, TU, uoff - d.U(i - 1) + r, M, dd, TU, uoff, U, t * wtask + d.preW(i) + r * U, U};
        }
        q -= nk;
        if (q < nh) {
          const int r = q * PO_MB, M = H - r < PO_MB ? H - r : PO_MB;
          return {sh, NG, d.m * uoff + r, M, dp, TU, uoff, U, d.T * wtask + t * w2task + d.preW2(i) + r * U, U};
        }
        q -= nh;
      }
    return {x, ldx, 0, 0, dd, TU, 0, 0, 0, 1};    // never reached: q < mats
  }
};

static int po_dims(PoDims& d, int64_t B, int Dm, int64_t ldx, int Dg, int64_t ldg, int T, int L, const int* units,
                   const int* acts, int m) {
  if (B < 0 || Dm < 1 || Dg < 1 || T < 1 || L < 1 || m < 1 || !units || !acts) return REC_E_ARG;
  if (ldx < Dm || ldg < Dg) return REC_E_ARG;
  if (T > PO_MAXT || L > PO_MAXL || Dm > PO_MAXD || Dg > PO_MAXD || B >= ((int64_t)1 << 31) ||
      ldx >= ((int64_t)1 << 31) || ldg >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;
  int u[PO_MAXL] = {0, 0, 0, 0}, ac[PO_MAXL] = {0, 0, 0, 0};
  for (int i = 0; i < L; ++i) {
    if (units[i] < 1) return REC_E_ARG;
    if (acts[i] != REC_ACT_NONE && acts[i] != REC_ACT_RELU && acts[i] != REC_ACT_SIGMOID) return REC_E_UNSUPPORTED;
    if (units[i] > PO_MAXU || (int64_t)m * units[i] > PO_MAXH) return REC_E_UNSUPPORTED;
    u[i] = units[i];
    ac[i] = acts[i];
  }
  d = PoDims{Dm, Dg, T, L, m, u[0], u[1], u[2], u[3], ac[0], ac[1], ac[2], ac[3]};
  if (sizeof(float) * po_lds_floats(d, 0) > PO_LDS_CAP) return REC_E_UNSUPPORTED;
  return REC_OK;
}

static int po_small_floats(const PoDims& d) { return d.T * (d.preW(d.L) + d.preW2(d.L)); }

struct PoWs {
  size_t dz, dd, dp, slots, part, gemm, total;   // offsets in floats
};
static PoWs po_ws(int64_t B, const PoDims& d) {
  PoWs w{};
  const size_t b = (size_t)B, tiles = (size_t)ceil_div64(B, MB_T);
  WsCarve c;
  w.dz = c.take(b * d.NG());
  w.dd = c.take(b * d.T * d.sumU());
  w.dp = c.take(b * d.T * d.sumU());
  w.slots = c.take(tiles * (size_t)po_slot_floats(d));
  w.part = c.take((size_t)mb_small_split(B) * po_small_floats(d));
  w.gemm = c.take(mb_dw_gemm_floats(B, d.Dg, d.NG()));
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" size_t rec_poso_mlp_scratch_bytes(int64_t B, int Dm, int Dg, int T, int L, const int* units_host,
                                               int gate_hidden_multiple) {
  PoDims d;
  const int acts[PO_MAXL] = {REC_ACT_NONE, REC_ACT_NONE, REC_ACT_NONE, REC_ACT_NONE};
  if (po_dims(d, B, Dm, Dm, Dg, Dg, T, L, units_host, acts, gate_hidden_multiple) != REC_OK) return 0;
  return sizeof(float) * (po_ws(B, d).total + 4);
}

extern "C" int rec_poso_mlp_fwd_f32(const float* x, int64_t ldx, const float* g, int64_t ldg, const float* Wg1,
                                    const float* bg1, const float* Wg2, const float* bg2, const float* W,
                                    const float* b, const float* C, int64_t B, int Dm, int Dg, int T, int L,
                                    const int* units_host, const int* acts_host, int gate_hidden_multiple, float* out,
                                    float* h, float* gate, float* d_out, float* a, void* stream) {
  PoDims d;
  if (int rc = po_dims(d, B, Dm, ldx, Dg, ldg, T, L, units_host, acts_host, gate_hidden_multiple)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !g || !Wg1 || !bg1 || !Wg2 || !bg2 || !W || !b || !C || !out) return REC_E_ARG;
  const bool save = h || gate || d_out || a;
  if (save && !(h && gate && d_out && a)) return REC_E_ARG;                      // all of them or none
  if (hipError_t err = rec_allow_lds<poso_fwd_kernel>(PO_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * po_lds_floats(d, 0);
  hipLaunchKernelGGL(poso_fwd_kernel, dim3((unsigned)ceil_div64(B, MB_T)), dim3(PO_NTHR), lds, as_stream(stream), x, ldx,
                     g, ldg, Wg1, bg1, Wg2, bg2, W, b, C, B, d, out, h, gate, d_out, a);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_poso_mlp_bwd_f32(const float* x, int64_t ldx, const float* g, int64_t ldg, const float* Wg1,
                                    const float* Wg2, const float* W, const float* C, const float* h, const float* gate,
                                    const float* d_out, const float* a, const float* dout, int64_t B, int Dm, int Dg,
                                    int T, int L, const int* units_host, const int* acts_host, int gate_hidden_multiple,
                                    float* dx, float* dg, float* dWg1, float* dbg1, float* dWg2, float* dbg2, float* dW,
                                    float* db, float* dC, void* workspace, size_t workspace_bytes, void* stream) {
  PoDims d;
  if (int rc = po_dims(d, B, Dm, ldx, Dg, ldg, T, L, units_host, acts_host, gate_hidden_multiple)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !g || !Wg1 || !Wg2 || !W || !C || !h || !gate || !d_out || !a || !dout || !dx || !dg || !dWg1 || !dbg1 ||
      !dWg2 || !dbg2 || !dW || !db || !dC || !workspace)
    return REC_E_ARG;
  const PoWs w = po_ws(B, d);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  float *dz = base + w.dz, *dd = base + w.dd, *dp = base + w.dp, *slots = base + w.slots, *part = base + w.part,
        *gws = base + w.gemm;
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, MB_T), NG = d.NG(), TU = T * d.sumU();
  if (hipError_t err = rec_allow_lds<poso_bwd_kernel>(PO_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * po_lds_floats(d, 1);
  hipLaunchKernelGGL(poso_bwd_kernel, dim3(tiles), dim3(PO_NTHR), lds, st, Wg1, Wg2, W, C, h, gate, d_out, a, dout, B,
                     d, dx, dg, dz, dd, dp, slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, po_slot_floats(d), tiles, slots, {{dbg1, dbg2, db, dC}, {NG, TU, TU, T * L}},
                            st))
    return rc;
  int mats = 0, big = 1;
  for (int i = 0; i < L; ++i) {
    mats += po_blocks(d.K(i)) + po_blocks(d.m * d.U(i));
    const int rows = po_max(d.K(i), d.m * d.U(i));
    big = po_max(big, (rows < PO_MB ? rows : PO_MB) * d.U(i));
  }
  const int S = mb_small_split(B), wtot = po_small_floats(d), wW = T * d.preW(L);
  if (int rc = small_dw_launch(PoSmall{d, x, (int)ldx, h, a, dd, dp}, T * mats, big, wtot, B, part, st)) return rc;
  if (int rc = rec_slot_sum(REC_SLOTS_SERIAL, wtot, S, part, {{dW, dWg2}, {wW, wtot - wW}}, st)) return rc;
  return rec_gemm_f32(1, 0, Dg, NG, B, g, ldg, dz, NG, dWg1, NG, REC_EPI_NONE, nullptr, nullptr, 0, nullptr, 0,
                      mb_split(B, Dg, NG), gws, nullptr, stream);               // dWg1 = g^T dZ
}
