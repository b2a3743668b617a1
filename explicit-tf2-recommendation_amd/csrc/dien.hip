// DIEN (DIENLayer, DienGRU, CustomGRUCell and DienActivationLayer, 5.DIN/CustomLayers.py:292-517) on gfx950, fp32: the
// masked Keras GRU of the interest extractor fused with the series / negative lookups and the auxiliary loss, and the
// attention scores fused with the AGRU / AUGRU of the interest evolution.  All three recurrences are ONE cell with the
// gate blocks [z | r | h] (AGRU: [r | h]), H = D columns each, Wx [H, ng H] on the input, Uh [H, ng H] on the state:
//   pre = x_t Wx + bx            rec = h Uh + bh
//   z = sigmoid(pre_z + rec_z)   r = sigmoid(pre_r + rec_r)   hh = tanh(pre_h + r (.) rec_h)
//   GRU    h' = z h + (1 - z) hh                      (tf.keras.layers.GRU, reset_after=True: bx = bias[0], bh = bias[1])
//   AUGRU  h' = (1 - a z) h + a z hh                  (z is the cell's u, bh = 0)
//   AGRU   h' = (1 - a) h + a hh                      (no z block)
// and h' = h where valid[b,t] = (mask id != padding_index) is false: the state is carried, holes anywhere.
//
// A workgroup of 4 waves owns 32 examples and walks t inside the launch.  h and x_t are k-major LDS operands [k][33] of
// v_mfma_f32_32x32x2_f32, the weights its B operand from global memory (L2-resident: 3 H^2 floats each); the two
// products of a step land in LDS as [column][33] and the gates are one pass over (example, column).  The input
// projection stays inside the loop: hoisting it would write and read back B T ng H floats.
// Forward: every h_t goes to hs [B,T,H] (the GRU's output; the evolution's saved states), the final state to hfin.
// Scores (evolution only), before the loop: product[b,t] = x[b,t] . q[b], e = sel ? exp(product) : 0 with sel = padded
// (mask_valid = 0, the reference) or valid (1), a = e / sum e, NaN -> 0; written to scores [B,T] and kept in LDS.
// Auxiliary loss (extractor with negatives), t >= 1: p = sigmoid(x_{t-1} . h_t), n = sigmoid(x_{t-1} . neg_t),
// valid[b,t] (ce(p, 1) + ce(n, 0)) with ce(x, l) = max(x, 0) - x l + log1p(exp(-|x|)); a row's terms are added over t,
// the rows of a tile in order, the tiles of a workgroup in order into its slot, rec_slot_sum adds the slots.
// Backward: one launch walks t downwards with dh in LDS, recomputes the gates from hs[t-1] and x_t, and per step writes
//   the row gradient dx[b,t] = dpre Wx^T (+ the auxiliary terms of step t+1, + dproduct q in the evolution),
//   dpre [ng H] and dcand (.) r [H] of the step into the workspace G [B T, (ng + 1) H], h_{t-1} and (table mode) x_t
//   beside it, and adds dh_{t-1} = dh (.) carry + drec Uh^T.
// The bias gradients are column sums a thread keeps in registers over the workgroup's tiles (slots, rec_slot_sum);
// dWx = X^T dpre and dUh = Hprev^T drec are rec_gemm_f32 over K = B T (split-K, slices added in order).  The evolution's
// epilogue turns da [T] into dproduct = a (.) (da - sum a da) (rows whose scores were NaN -> 0 have a = 0: zero), dq
// and the second share of dx.  No float atomics, no scratch memory; every launch only enqueues.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

#include "tile_ops.h"

namespace {

constexpr int DN_NTHR = 256, DN_LD = MB_LD;
constexpr int DN_MAXSLOTS = 2048;                 // workgroups of a launch at the most: each owns a slot
constexpr size_t DN_LDS_CAP = REC_TILE_LDS_CAP;
enum { DN_GRU = REC_DIEN_GRU, DN_AUGRU = REC_DIEN_AUGRU, DN_AGRU = REC_DIEN_AGRU };
static_assert(DN_GRU < DN_AUGRU && DN_AUGRU < DN_AGRU && DN_AGRU - DN_GRU == 2, "dn_check takes the modes as a range");

struct DnArgs {
  const float* embed;        // table mode: x_t = concat_r embed[series[b,t,r]]; NULL: dense mode, x [B,T,H]
  int64_t ld, V;
  int E, C;
  const int64_t* series;     // [B,T,C] (table mode)
  const int64_t* neg;        // [B,T,C] or NULL: no auxiliary loss
  const float* x;            // [B,T,H] (dense mode)
  const int64_t* mask_ids;   // valid[b,t] = mask_ids[(b T + t) mask_stride] != pad
  int64_t mask_stride, pad;
  const float *Wx, *Uh, *bx, *bh;   // [H, ng H], [H, ng H], [ng H], [ng H] or NULL (zeros)
  const float* q;            // [B,H] (evolution)
  int64_t B;
  int T, H, ng, mask_valid;
  int64_t per;               // tiles of a workgroup
};

// floats of LDS, the same both ways: the extractor holds x_t, x_{t-1}, h, dh and the (ng + 1) gate blocks, the
// evolution x_t, h, dh, the gate blocks and a, da [T] per example
__host__ __device__ inline size_t dn_lds_floats(int mode, int T, int H) {
  const int He = mb_even(H), ng = mode == DN_AGRU ? 2 : 3;
  const size_t ops = (size_t)(mode == DN_GRU ? 4 : 3) * He + (size_t)(ng + 1) * He;
  return DN_LD * (ops + (mode == DN_GRU ? 0 : 2 * (size_t)T)) + 128;
}

struct DnLds {
  float *xT, *xpT, *hT, *dhT, *G, *S, *dS, *gsp, *gsn, *lrow;
  int* valid;
};
__device__ __forceinline__ DnLds dn_carve(float* lds, int mode, int T, int H) {
  const int He = mb_even(H), ng = mode == DN_AGRU ? 2 : 3;
  DnLds f;
  f.xT = lds;
  f.hT = f.xT + He * DN_LD;
  f.dhT = f.hT + He * DN_LD;
  f.G = f.dhT + He * DN_LD;
  float* p = f.G + (ng + 1) * He * DN_LD;
  if (mode == DN_GRU) {
    f.xpT = p;
    p += He * DN_LD;
    f.S = f.dS = nullptr;
  } else {
    f.xpT = nullptr;
    f.S = p;
    f.dS = p + T * DN_LD;
    p += 2 * T * DN_LD;
  }
  f.gsp = p;
  f.gsn = p + 32;
  f.lrow = p + 64;
  f.valid = reinterpret_cast<int*>(p + 96);
  return f;
}

__device__ __forceinline__ float dn_ce(float x, float label) {
  return (fmaxf(x, 0.f) - x * label) + log1pf(expf(-fabsf(x)));
}

// x rows of step t of the tile into a k-major operand: looked up (ids [B,T,C]) or dense (src [B,T,H])
__device__ __forceinline__ void dn_rows_in(const DnArgs& a, const int64_t* __restrict__ ids,
                                           const float* __restrict__ src, int64_t r0, int t, float* dst, int tid,
                                           bool& bad) {
  const int H = a.H;
  for (int i = tid; i < MB_T * H; i += DN_NTHR) {
    const int row = i / H, d = i - row * H;
    const int64_t b = r0 + row;
    float v = 0.f;
    if (b < a.B) {
      if (ids) {
        const int r = d / a.E, e = d - r * a.E;
        const int64_t id = ids[(b * a.T + t) * a.C + r];
        const bool ok = id >= 0 && id < a.V;
        const float tv = a.embed[(ok ? id : 0) * a.ld + e];
        v = ok ? tv : 0.f;
        bad |= !ok;
      } else {
        v = src[(b * a.T + t) * H + d];
      }
    }
    dst[d * DN_LD + row] = v;
  }
}

__device__ __forceinline__ void dn_valid_in(const DnArgs& a, int64_t r0, int t, int* valid, int tid) {
  if (tid < MB_T) {
    const int64_t b = r0 + tid;
    valid[tid] = (b < a.B && a.mask_ids[(b * a.T + t) * a.mask_stride] != a.pad) ? 1 : 0;
  }
}

// the two products of a step into the gate blocks G: blocks 0 .. ng-1 = x Wx (+ h Uh on all but the last), block ng =
// h Uh of the candidate
__device__ __forceinline__ void dn_products(const DnArgs& a, const float* xT, const float* hT, float* G, int wave,
                                            int lo, int hi) {
  const int H = a.H, ng = a.ng, N = ng * H, He = mb_even(H);
  f32x16 accA[MB_NJ], accB[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    mb_zero(accA[j]);
    mb_zero(accB[j]);
  }
  mb_mma<false>(accA, xT, H, a.Wx, N, 0, N, wave, lo, hi);
  mb_mma<false>(accA, hT, H, a.Uh, N, 0, N - H, wave, lo, hi);
  mb_mma<false>(accB, hT, H, a.Uh + (N - H), N, 0, H, wave, lo, hi);
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int c = (wave + 4 * j) * 32 + lo;
    if (c < N) {
      const int g = c / H, cc = c - g * H;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) G[(g * He + cc) * DN_LD + mb_row(rr, hi)] = accA[j][rr];
    }
    if (c < H) {
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) G[(ng * He + c) * DN_LD + mb_row(rr, hi)] = accB[j][rr];
    }
  }
}

struct DnGates {
  float z, r, rec, hh;
};
// the gates of element (row, c) out of the gate blocks
__device__ __forceinline__ DnGates dn_gates(const DnArgs& a, const float* G, int row, int c) {
  const int H = a.H, ng = a.ng, He = mb_even(H);
  const int rb = ng - 2, hb = ng - 1;
  DnGates g;
  g.z = 0.f;
  if (ng == 3) g.z = sigmoid_acc(G[c * DN_LD + row] + ((a.bx ? a.bx[c] : 0.f) + (a.bh ? a.bh[c] : 0.f)));
  g.r = sigmoid_acc(G[(rb * He + c) * DN_LD + row] +
                    ((a.bx ? a.bx[rb * H + c] : 0.f) + (a.bh ? a.bh[rb * H + c] : 0.f)));
  g.rec = G[(ng * He + c) * DN_LD + row] + (a.bh ? a.bh[hb * H + c] : 0.f);
  g.hh = tanhf((G[(hb * He + c) * DN_LD + row] + (a.bx ? a.bx[hb * H + c] : 0.f)) + g.r * g.rec);
  return g;
}

// s_p[row] = xp . h and s_n[row] = xp . n over the columns, 8 threads a row: every thread of the row gets both
__device__ __forceinline__ void dn_aux_dots(const float* xp, const float* h, const float* n, int H, int tid, float& sp,
                                            float& sn) {
  const int row = tid >> 3, part = tid & 7;
  float p = 0.f, q = 0.f;
  for (int c = part; c < H; c += 8) {
    const float xv = xp[c * DN_LD + row];
    p = fmaf(xv, h[c * DN_LD + row], p);
    q = fmaf(xv, n[c * DN_LD + row], q);
  }
  sp = group_sum<8>(p);
  sn = group_sum<8>(q);
}

// the scores of the tile into S [T][33] and scores [B,T]; xT is used for q
__device__ __forceinline__ void dn_scores(const DnArgs& a, const DnLds& f, int64_t r0, float* __restrict__ scores,
                                          int tid) {
  const int H = a.H, T = a.T;
  for (int i = tid; i < MB_T * H; i += DN_NTHR) {
    const int row = i / H, c = i - row * H;
    f.xT[c * DN_LD + row] = r0 + row < a.B ? a.q[(r0 + row) * H + c] : 0.f;
  }
  __syncthreads();
  const int grp = tid >> 5, lo = tid & 31;
  for (int p = grp; p < MB_T * T; p += DN_NTHR / 32) {
    const int row = p / T, t = p - row * T;
    const int64_t b = r0 + row;
    float acc = 0.f;
    if (b < a.B)
      for (int c = lo; c < H; c += 32) acc = fmaf(a.x[(b * T + t) * H + c], f.xT[c * DN_LD + row], acc);
    acc = group_sum<32>(acc);
    if (lo == 0) f.S[t * DN_LD + row] = acc;
  }
  __syncthreads();
  if (tid < MB_T) {
    const int64_t b = r0 + tid;
    float sum = 0.f;
    for (int t = 0; t < T; ++t) {
      float e = 0.f;
      if (b < a.B) {
        const bool v = a.mask_ids[(b * T + t) * a.mask_stride] != a.pad;
        if (a.mask_valid ? v : !v) e = expf(f.S[t * DN_LD + tid]);
      }
      f.S[t * DN_LD + tid] = e;
      sum += e;
    }
    for (int t = 0; t < T; ++t) {
      float s = f.S[t * DN_LD + tid] / sum;
      if (s != s) s = 0.f;                                       // tf.where(is_nan(scores), 0, scores)
      f.S[t * DN_LD + tid] = s;
      if (b < a.B) scores[b * T + t] = s;
    }
  }
  __syncthreads();
}

template <int MODE>
__global__ __launch_bounds__(DN_NTHR) void dien_fwd_kernel(DnArgs a, float* __restrict__ hs, float* __restrict__ hfin,
                                                           float* __restrict__ scores, float* __restrict__ aux_slots,
                                                           int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, T = a.T;
  const DnLds f = dn_carve(lds, MODE, T, H);
  const size_t nlds = dn_lds_floats(MODE, T, H);
  for (size_t i = tid; i < nlds; i += DN_NTHR) lds[i] = 0.f;      // the pad rows of the operands stay zero
  __syncthreads();
  const bool has_aux = MODE == DN_GRU && a.neg != nullptr;
  const int64_t tiles = (a.B + MB_T - 1) / MB_T;
  const int64_t t0 = (int64_t)blockIdx.x * a.per, t1 = t0 + a.per < tiles ? t0 + a.per : tiles;
  bool bad = false;
  float wg_loss = 0.f;                                           // thread 0: the workgroup's auxiliary sum
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t r0 = tile * MB_T;
    if (MODE != DN_GRU) dn_scores(a, f, r0, scores, tid);
    for (int i = tid; i < MB_T * H; i += DN_NTHR) {
      const int row = i / H, c = i - row * H;
      f.hT[c * DN_LD + row] = 0.f;
    }
    float loss = 0.f;                                            // threads 8 row: the row's auxiliary terms
    float* xT = f.xT;
    float* xpT = f.xpT;
    for (int t = 0; t < T; ++t) {
      dn_rows_in(a, a.embed ? a.series : nullptr, a.x, r0, t, xT, tid, bad);
      dn_valid_in(a, r0, t, f.valid, tid);
      __syncthreads();
      dn_products(a, xT, f.hT, f.G, wave, lo, hi);
      __syncthreads();
      for (int i = tid; i < MB_T * H; i += DN_NTHR) {
        const int row = i / H, c = i - row * H;
        const DnGates g = dn_gates(a, f.G, row, c);
        const float h = f.hT[c * DN_LD + row];
        float hn = h;
        if (f.valid[row]) {
          if (MODE == DN_GRU) {
            hn = g.z * h + (1.f - g.z) * g.hh;
          } else {
            const float av = f.S[t * DN_LD + row], w = MODE == DN_AUGRU ? av * g.z : av;
            hn = (1.f - w) * h + w * g.hh;
          }
        }
        f.hT[c * DN_LD + row] = hn;
        if (hs && r0 + row < a.B) hs[((r0 + row) * T + t) * H + c] = hn;
      }
      __syncthreads();
      if (has_aux) {
        if (t >= 1) {
          dn_rows_in(a, a.neg, nullptr, r0, t, f.G, tid, bad);   // the gate blocks are free: neg_t into block 0
          __syncthreads();
          float sp, sn;
          dn_aux_dots(xpT, f.hT, f.G, H, tid, sp, sn);
          if (f.valid[tid >> 3]) loss += dn_ce(sigmoid_acc(sp), 1.f) + dn_ce(sigmoid_acc(sn), 0.f);
          __syncthreads();
        }
        float* sw = xT;
        xT = xpT;
        xpT = sw;
      }
    }
    if (hfin)
      for (int i = tid; i < MB_T * H; i += DN_NTHR) {
        const int row = i / H, c = i - row * H;
        if (r0 + row < a.B) hfin[(r0 + row) * H + c] = f.hT[c * DN_LD + row];
      }
    if (has_aux) {
      if ((tid & 7) == 0) f.lrow[tid >> 3] = loss;
      __syncthreads();
      if (tid == 0)
        for (int r = 0; r < MB_T; ++r) wg_loss += f.lrow[r];
    }
    __syncthreads();                                             // the next tile rewrites all of it
  }
  if (has_aux && tid == 0) aux_slots[blockIdx.x] = wg_loss;
  if (bad && oob) *oob = 1;
}

template <int MODE>
__global__ __launch_bounds__(DN_NTHR) void dien_bwd_kernel(DnArgs a, const float* __restrict__ hs,
                                                           const float* __restrict__ scores,
                                                           const float* __restrict__ dhs,
                                                           const float* __restrict__ dhfin,
                                                           const float* __restrict__ gaux, float* dx,
                                                           float* __restrict__ dneg, float* __restrict__ dq,
                                                           float* __restrict__ Gws, float* __restrict__ hprev,
                                                           float* __restrict__ xs, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, T = a.T, ng = a.ng, N = ng * H, He = mb_even(H), GW = (ng + 1) * H;
  const DnLds f = dn_carve(lds, MODE, T, H);
  const size_t nlds = dn_lds_floats(MODE, T, H);
  for (size_t i = tid; i < nlds; i += DN_NTHR) lds[i] = 0.f;
  __syncthreads();
  const bool has_aux = MODE == DN_GRU && a.neg != nullptr;
  const float ga = (has_aux && gaux) ? gaux[0] : 0.f;
  const int64_t tiles = (a.B + MB_T - 1) / MB_T;
  const int64_t t0 = (int64_t)blockIdx.x * a.per, t1 = t0 + a.per < tiles ? t0 + a.per : tiles;
  bool bad = false;
  float dbs[3] = {0.f, 0.f, 0.f};                                // bias-gradient columns tid, tid + 256, tid + 512
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t r0 = tile * MB_T;
    for (int i = tid; i < MB_T * H; i += DN_NTHR) {
      const int row = i / H, c = i - row * H;
      f.dhT[c * DN_LD + row] = (dhfin && r0 + row < a.B) ? dhfin[(r0 + row) * H + c] : 0.f;
    }
    if (MODE != DN_GRU)
      for (int i = tid; i < MB_T * T; i += DN_NTHR) {
        const int row = i / T, t = i - row * T;
        f.S[t * DN_LD + row] = r0 + row < a.B ? scores[(r0 + row) * T + t] : 0.f;
      }
    float* xT = f.xT;
    float* xpT = f.xpT;
    for (int t = T - 1; t >= 0; --t) {
      // ---- loads: x_t, h_{t-1}, the mask, the upstream of h_t; with the loss x_{t-1}, neg_t and h_t as well
      if (!has_aux || t == T - 1) dn_rows_in(a, a.embed ? a.series : nullptr, a.x, r0, t, xT, tid, bad);
      dn_valid_in(a, r0, t, f.valid, tid);
      for (int i = tid; i < MB_T * H; i += DN_NTHR) {
        const int row = i / H, c = i - row * H;
        const int64_t b = r0 + row;
        const bool in = b < a.B;
        f.hT[c * DN_LD + row] = (in && t > 0) ? hs[(b * T + t - 1) * H + c] : 0.f;
        if (dhs && in) f.dhT[c * DN_LD + row] = f.dhT[c * DN_LD + row] + dhs[(b * T + t) * H + c];
        if (has_aux && t >= 1) f.G[(He + c) * DN_LD + row] = in ? hs[(b * T + t) * H + c] : 0.f;
      }
      if (has_aux && t >= 1) {
        dn_rows_in(a, a.series, nullptr, r0, t - 1, xpT, tid, bad);
        dn_rows_in(a, a.neg, nullptr, r0, t, f.G, tid, bad);
      }
      __syncthreads();
      // ---- the loss of step t: into dh_t, neg_t's rows and the share of x_{t-1}'s rows
      if (has_aux) {
        if (t >= 1) {
          float sp, sn;
          dn_aux_dots(xpT, f.G + He * DN_LD, f.G, H, tid, sp, sn);
          if ((tid & 7) == 0) {
            const int row = tid >> 3;
            const float g = f.valid[row] ? ga : 0.f;
            const float p = sigmoid_acc(sp), n = sigmoid_acc(sn);
            f.gsp[row] = g * ((sigmoid_acc(p) - 1.f) * (p * (1.f - p)));
            f.gsn[row] = g * (sigmoid_acc(n) * (n * (1.f - n)));
          }
          __syncthreads();
          for (int i = tid; i < MB_T * H; i += DN_NTHR) {
            const int row = i / H, c = i - row * H;
            const int64_t b = r0 + row;
            const float xp = xpT[c * DN_LD + row], gp = f.gsp[row], gn = f.gsn[row];
            f.dhT[c * DN_LD + row] = f.dhT[c * DN_LD + row] + gp * xp;
            if (b < a.B) {
              dneg[(b * T + t) * H + c] = gn * xp;
              dx[(b * T + t - 1) * H + c] = gp * f.G[(He + c) * DN_LD + row] + gn * f.G[c * DN_LD + row];
            }
          }
          __syncthreads();
        } else {
          for (int i = tid; i < MB_T * H; i += DN_NTHR) {
            const int row = i / H, c = i - row * H;
            if (r0 + row < a.B) dneg[((r0 + row) * T) * H + c] = 0.f;
          }
        }
      }
      // ---- the gates again, then their gradients into the gate blocks
      dn_products(a, xT, f.hT, f.G, wave, lo, hi);
      __syncthreads();
      for (int i = tid; i < MB_T * H; i += DN_NTHR) {
        const int row = i / H, c = i - row * H;
        const int64_t b = r0 + row;
        const DnGates g = dn_gates(a, f.G, row, c);
        const float h = f.hT[c * DN_LD + row], dh = f.dhT[c * DN_LD + row];
        float dz = 0.f, dr = 0.f, dc = 0.f, dcr = 0.f, dhold = dh, dap = 0.f;
        if (f.valid[row]) {
          float dhh, dgz = 0.f;
          if (MODE == DN_GRU) {
            dhh = dh * (1.f - g.z);
            dgz = dh * (h - g.hh);
            dhold = dh * g.z;
          } else {
            const float av = f.S[t * DN_LD + row], w = MODE == DN_AUGRU ? av * g.z : av;
            const float dw = dh * (g.hh - h);
            dhh = dh * w;
            dhold = dh * (1.f - w);
            if (MODE == DN_AUGRU) {
              dgz = dw * av;
              dap = dw * g.z;
            } else {
              dap = dw;
            }
          }
          dz = dgz * (g.z * (1.f - g.z));
          dc = dhh * (1.f - g.hh * g.hh);
          dr = (dc * g.rec) * (g.r * (1.f - g.r));
          dcr = dc * g.r;
        }
        const float xv = xT[c * DN_LD + row];
        if (ng == 3) f.G[c * DN_LD + row] = dz;
        f.G[((ng - 2) * He + c) * DN_LD + row] = dr;
        f.G[((ng - 1) * He + c) * DN_LD + row] = dc;
        f.G[(ng * He + c) * DN_LD + row] = dcr;
        f.dhT[c * DN_LD + row] = dhold;
        if (MODE != DN_GRU) xT[c * DN_LD + row] = dap;           // x_t is done with: its buffer takes da's terms
        if (b < a.B) {
          float* gw = Gws + (b * T + t) * GW;
          if (ng == 3) gw[c] = dz;
          gw[(ng - 2) * H + c] = dr;
          gw[(ng - 1) * H + c] = dc;
          gw[ng * H + c] = dcr;
          hprev[(b * T + t) * H + c] = h;
          if (xs) xs[(b * T + t) * H + c] = xv;
        }
      }
      __syncthreads();
      // ---- dh_{t-1} += drec Uh^T, dx_t = dpre Wx^T, the bias columns, da[t]
      {
        const int n0 = wave * 32;
        if (n0 < H) {                                            // uniform over the wave
          f32x16 accX, accH;
          mb_zero(accX);
          mb_zero(accH);
          for (int g = 0; g < ng; ++g) {
            mb_mma1<true>(accX, f.G + g * He * DN_LD, H, a.Wx, N, g * H, H, n0, lo, hi);
            const float* Ah = f.G + (g < ng - 1 ? g : ng) * He * DN_LD;
            mb_mma1<true>(accH, Ah, H, a.Uh, N, g * H, H, n0, lo, hi);
          }
          const int c = n0 + lo;
          if (c < H) {
            const bool add = has_aux && t < T - 1;               // step t + 1 left the loss's share there
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
              const int row = mb_row(rr, hi);
              const int64_t b = r0 + row;
              f.dhT[c * DN_LD + row] = f.dhT[c * DN_LD + row] + accH[rr];
              if (b < a.B) {
                float* at = dx + (b * T + t) * H + c;
                *at = add ? *at + accX[rr] : accX[rr];
              }
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int col = tid + k * DN_NTHR;
          if (col < 2 * N) {
            const int j = col < N ? col / H : (col - N) / H;
            const int cc = col < N ? col - j * H : col - N - j * H;
            const int blk = (col >= N && j == ng - 1) ? ng : j;
            const float* src = f.G + (blk * He + cc) * DN_LD;
            float s = 0.f;
            for (int r = 0; r < MB_T; ++r) s += src[r];
            dbs[k] += s;
          }
        }
        if (MODE != DN_GRU && tid < MB_T) {
          float s = 0.f;
          for (int c = 0; c < H; ++c) s += xT[c * DN_LD + tid];
          f.dS[t * DN_LD + tid] = s;
        }
      }
      __syncthreads();
      if (has_aux) {
        float* sw = xT;
        xT = xpT;
        xpT = sw;
      }
    }
    if (MODE != DN_GRU) {
      // ---- the scores back: dproduct = a (.) (da - sum a da), dq = sum_t dproduct x_t, dx_t += dproduct q
      if (tid < MB_T) {
        float dot = 0.f;
        for (int t = 0; t < T; ++t) dot = fmaf(f.S[t * DN_LD + tid], f.dS[t * DN_LD + tid], dot);
        for (int t = 0; t < T; ++t) f.dS[t * DN_LD + tid] = f.S[t * DN_LD + tid] * (f.dS[t * DN_LD + tid] - dot);
      }
      __syncthreads();
      for (int i = tid; i < MB_T * H; i += DN_NTHR) {
        const int row = i / H, c = i - row * H;
        const int64_t b = r0 + row;
        if (b < a.B) {
          const float qv = a.q[b * H + c];
          float acc = 0.f;
          for (int t = 0; t < T; ++t) {
            const float dp = f.dS[t * DN_LD + row];
            acc = fmaf(dp, a.x[(b * T + t) * H + c], acc);
            dx[(b * T + t) * H + c] = dx[(b * T + t) * H + c] + dp * qv;
          }
          dq[b * H + c] = acc;
        }
      }
    }
    __syncthreads();                                             // the next tile rewrites all of it
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int col = tid + k * DN_NTHR;
    if (col < 2 * N) slots[(int64_t)blockIdx.x * 2 * N + col] = dbs[k];
  }
}

static int dn_ng(int mode) { return mode == DN_AGRU ? 2 : 3; }

static int dn_check(int mode, int64_t B, int T, int H) {
  if (mode < DN_GRU || mode > DN_AGRU || B < 0 || T < 1 || H < 1) return REC_E_ARG;
  if (H > REC_DIN_WIDE_D || B >= ((int64_t)1 << 31) || T > (int)(DN_LDS_CAP / sizeof(float)) ||
      sizeof(float) * dn_lds_floats(mode, T, H) > DN_LDS_CAP)
    return REC_E_UNSUPPORTED;
  return REC_OK;
}

static int64_t dn_slots(int64_t B, int64_t* per) {
  const int64_t tiles = ceil_div64(B > 0 ? B : 1, MB_T);
  *per = ceil_div64(tiles, DN_MAXSLOTS);
  return ceil_div64(tiles, *per);
}

// the backward's scratch, in floats: G [B T, (ng + 1) H], h_{t-1} and x_t [B T, H] each, the slots of the bias columns
// and the split-K partials of the two weight-gradient products
struct DnScratch {
  size_t G, hprev, xs, slots, dbh, gemm, total;
};
static DnScratch dn_scratch(int mode, int64_t B, int T, int H) {
  const int ng = dn_ng(mode);
  int64_t per = 1;
  const int64_t nslot = dn_slots(B, &per);
  const size_t BT = (size_t)B * T;
  WsCarve c;
  DnScratch s;
  s.G = c.take(BT * (ng + 1) * H);
  s.hprev = c.take(BT * H);
  s.xs = c.take(BT * H);
  s.slots = c.take((size_t)nslot * 2 * ng * H);
  s.dbh = c.take((size_t)ng * H);                                // where a cell without a state bias drops that half
  s.gemm = c.take((size_t)16 * H * ng * H);                      // mb_split gives at most 16 slices of [H, ng H]
  s.total = c.at + 4;
  return s;
}

template <int MODE>
static int dn_launch_fwd(const DnArgs& a, int64_t nslot, float* hs, float* hfin, float* scores, float* aux_slots,
                         int* oob, hipStream_t st) {
  const size_t lds = sizeof(float) * dn_lds_floats(MODE, a.T, a.H);
  if (hipError_t err = rec_allow_lds<dien_fwd_kernel<MODE>>(DN_LDS_CAP)) return (int)err;
  hipLaunchKernelGGL(dien_fwd_kernel<MODE>, dim3((unsigned)nslot), dim3(DN_NTHR), lds, st, a, hs, hfin, scores,
                     aux_slots, oob);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

template <int MODE>
static int dn_launch_bwd(const DnArgs& a, int64_t nslot, const float* hs, const float* scores, const float* dhs,
                         const float* dhfin, const float* gaux, float* dx, float* dneg, float* dq, float* Gws,
                         float* hprev, float* xs, float* slots, hipStream_t st) {
  const size_t lds = sizeof(float) * dn_lds_floats(MODE, a.T, a.H);
  if (hipError_t err = rec_allow_lds<dien_bwd_kernel<MODE>>(DN_LDS_CAP)) return (int)err;
  hipLaunchKernelGGL(dien_bwd_kernel<MODE>, dim3((unsigned)nslot), dim3(DN_NTHR), lds, st, a, hs, scores, dhs, dhfin,
                     gaux, dx, dneg, dq, Gws, hprev, xs, slots);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

// what follows the recurrence launch of a backward: the bias columns, dWx = X^T dpre, dUh = Hprev^T drec
static int dn_weight_grads(int mode, int64_t B, int T, int H, const float* X, float* ws, const DnScratch& s,
                           int64_t nslot, float* dWx, float* dUh, float* dbx, float* dbh, hipStream_t st) {
  const int ng = dn_ng(mode), N = ng * H, GW = (ng + 1) * H;
  const int64_t BT = B * T;
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, 2 * N, (int)nslot, ws + s.slots, {{dbx, dbh}, {N, N}}, st)) return rc;
  const auto gemm = [&](const float* A, const float* G, int n, float* C) {
    return rec_gemm_f32(1, 0, H, n, BT, A, H, G, GW, C, N, REC_EPI_NONE, nullptr, nullptr, 0, nullptr, 0,
                        mb_split(BT, H, n), ws + s.gemm, nullptr, st);
  };
  if (int rc = gemm(X, ws + s.G, N, dWx)) return rc;
  if (int rc = gemm(ws + s.hprev, ws + s.G, N - H, dUh)) return rc;
  return gemm(ws + s.hprev, ws + s.G + N, H, dUh + (N - H));
}

}  // namespace

extern "C" size_t rec_dien_gru_lds_bytes(int T, int H) {
  return dn_check(DN_GRU, 0, T, H) == REC_OK ? sizeof(float) * dn_lds_floats(DN_GRU, T, H) : 0;
}
extern "C" size_t rec_dien_augru_lds_bytes(int T, int H, int mode) {
  if (mode != DN_AUGRU && mode != DN_AGRU) return 0;
  return dn_check(mode, 0, T, H) == REC_OK ? sizeof(float) * dn_lds_floats(mode, T, H) : 0;
}
extern "C" size_t rec_dien_gru_scratch_bytes(int64_t B, int T, int H, int backward) {
  if (dn_check(DN_GRU, B, T, H) != REC_OK || (backward != 0 && backward != 1)) return 0;
  int64_t per = 1;
  return sizeof(float) * (backward ? dn_scratch(DN_GRU, B, T, H).total : (size_t)dn_slots(B, &per) + 4);
}
extern "C" size_t rec_dien_augru_scratch_bytes(int64_t B, int T, int H, int mode) {
  if ((mode != DN_AUGRU && mode != DN_AGRU) || dn_check(mode, B, T, H) != REC_OK) return 0;
  return sizeof(float) * dn_scratch(mode, B, T, H).total;
}

extern "C" int rec_dien_gru_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                    const int64_t* negatives, const float* x, const int64_t* mask_ids, int64_t B,
                                    int T, int H, const float* kernel, const float* recurrent_kernel,
                                    const float* bias, int64_t padding_index, float* gru_output, float* h_final,
                                    float* aux, int* oob_flag, void* scratch, size_t scratch_bytes, void* stream) {
  if (E < 1 || C < 1) return REC_E_ARG;
  if (int rc = dn_check(DN_GRU, B, T, H)) return rc;
  if (!kernel || !recurrent_kernel || !bias || (!gru_output && !h_final)) return REC_E_ARG;
  if (embed ? (ld < E || V < 1 || !series || (int64_t)E * C != H || x || mask_ids) : (!x || !mask_ids || negatives))
    return REC_E_ARG;
  if (negatives && (!aux || !scratch)) return REC_E_ARG;
  int64_t per = 1;
  const int64_t nslot = dn_slots(B, &per);
  if (negatives && scratch_bytes < sizeof(float) * (size_t)nslot) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;
  hipStream_t st = as_stream(stream);
  const DnArgs a{embed, ld, V, E, C, series, negatives, x, embed ? series : mask_ids, embed ? C : 1, padding_index,
                 kernel, recurrent_kernel, bias, bias + 3 * H, nullptr, B, T, H, 3, 0, per};
  float* slots = static_cast<float*>(scratch);
  if (int rc = dn_launch_fwd<DN_GRU>(a, nslot, gru_output, h_final, nullptr, slots, oob_flag, st)) return rc;
  if (!negatives) return REC_OK;
  return rec_slot_sum(REC_SLOTS_WAVE, 1, (int)nslot, slots, {{aux}, {1}}, st);
}

extern "C" int rec_dien_gru_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                    const int64_t* negatives, const float* x, const int64_t* mask_ids, int64_t B,
                                    int T, int H, const float* kernel, const float* recurrent_kernel,
                                    const float* bias, int64_t padding_index, const float* gru_output,
                                    const float* dgru_output, const float* dh_final, const float* gaux, float* dx,
                                    float* dneg, float* dkernel, float* drecurrent_kernel, float* dbias,
                                    void* scratch, size_t scratch_bytes, void* stream) {
  if (E < 1 || C < 1) return REC_E_ARG;
  if (int rc = dn_check(DN_GRU, B, T, H)) return rc;
  if (!kernel || !recurrent_kernel || !bias || !gru_output || !dx || !dkernel || !drecurrent_kernel || !dbias ||
      !scratch)
    return REC_E_ARG;
  if (embed ? (ld < E || V < 1 || !series || (int64_t)E * C != H || x || mask_ids) : (!x || !mask_ids || negatives))
    return REC_E_ARG;
  if (negatives && !dneg) return REC_E_ARG;
  const DnScratch s = dn_scratch(DN_GRU, B, T, H);
  if (scratch_bytes < sizeof(float) * s.total) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;
  int64_t per = 1;
  const int64_t nslot = dn_slots(B, &per);
  hipStream_t st = as_stream(stream);
  float* ws = static_cast<float*>(scratch);
  const DnArgs a{embed, ld, V, E, C, series, negatives, x, embed ? series : mask_ids, embed ? C : 1, padding_index,
                 kernel, recurrent_kernel, bias, bias + 3 * H, nullptr, B, T, H, 3, 0, per};
  if (int rc = dn_launch_bwd<DN_GRU>(a, nslot, gru_output, nullptr, dgru_output, dh_final, gaux, dx, dneg, nullptr,
                                     ws + s.G, ws + s.hprev, embed ? ws + s.xs : nullptr, ws + s.slots, st))
    return rc;
  return dn_weight_grads(DN_GRU, B, T, H, embed ? ws + s.xs : x, ws, s, nslot, dkernel, drecurrent_kernel, dbias,
                         dbias + 3 * H, st);
}

extern "C" int rec_dien_augru_fwd_f32(const float* gru_output, const float* q, const int64_t* mask_ids,
                                      int64_t mask_stride, int64_t B, int T, int H, int mode, const float* Wx,
                                      const float* Uh, const float* bx, int64_t padding_index, int mask_valid,
                                      float* scores, float* states, float* h_final, void* stream) {
  if (mode != DN_AUGRU && mode != DN_AGRU) return REC_E_ARG;
  if (int rc = dn_check(mode, B, T, H)) return rc;
  if (!gru_output || !q || !mask_ids || mask_stride < 1 || !Wx || !Uh || !bx || !scores || !h_final ||
      (mask_valid != 0 && mask_valid != 1))
    return REC_E_ARG;
  if (B == 0) return REC_OK;
  int64_t per = 1;
  const int64_t nslot = dn_slots(B, &per);
  const DnArgs a{nullptr, 0, 0, 1, 1, nullptr, nullptr, gru_output, mask_ids, mask_stride, padding_index, Wx, Uh, bx,
                 nullptr, q, B, T, H, dn_ng(mode), mask_valid, per};
  hipStream_t st = as_stream(stream);
  return mode == DN_AUGRU ? dn_launch_fwd<DN_AUGRU>(a, nslot, states, h_final, scores, nullptr, nullptr, st)
                          : dn_launch_fwd<DN_AGRU>(a, nslot, states, h_final, scores, nullptr, nullptr, st);
}

extern "C" int rec_dien_augru_bwd_f32(const float* gru_output, const float* q, const int64_t* mask_ids,
                                      int64_t mask_stride, int64_t B, int T, int H, int mode, const float* Wx,
                                      const float* Uh, const float* bx, int64_t padding_index, int mask_valid,
                                      const float* scores, const float* states, const float* dh_final,
                                      float* dgru_output, float* dq, float* dWx, float* dUh, float* dbx,
                                      void* scratch, size_t scratch_bytes, void* stream) {
  if (mode != DN_AUGRU && mode != DN_AGRU) return REC_E_ARG;
  if (int rc = dn_check(mode, B, T, H)) return rc;
  if (!gru_output || !q || !mask_ids || mask_stride < 1 || !Wx || !Uh || !bx || !scores || !states || !dh_final ||
      !dgru_output || !dq || !dWx || !dUh || !dbx || !scratch || (mask_valid != 0 && mask_valid != 1))
    return REC_E_ARG;
  const DnScratch s = dn_scratch(mode, B, T, H);
  if (scratch_bytes < sizeof(float) * s.total) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;
  int64_t per = 1;
  const int64_t nslot = dn_slots(B, &per);
  hipStream_t st = as_stream(stream);
  float* ws = static_cast<float*>(scratch);
  const DnArgs a{nullptr, 0, 0, 1, 1, nullptr, nullptr, gru_output, mask_ids, mask_stride, padding_index, Wx, Uh, bx,
                 nullptr, q, B, T, H, dn_ng(mode), mask_valid, per};
  const int rc = mode == DN_AUGRU
                     ? dn_launch_bwd<DN_AUGRU>(a, nslot, states, scores, nullptr, dh_final, nullptr, dgru_output,
                                               nullptr, dq, ws + s.G, ws + s.hprev, nullptr, ws + s.slots, st)
                     : dn_launch_bwd<DN_AGRU>(a, nslot, states, scores, nullptr, dh_final, nullptr, dgru_output,
                                              nullptr, dq, ws + s.G, ws + s.hprev, nullptr, ws + s.slots, st);
  if (rc) return rc;
  // the cell has no bias on the state: that half of the bias columns goes to the scratch
  return dn_weight_grads(mode, B, T, H, gru_output, ws, s, nslot, dWx, dUh, dbx, ws + s.dbh, st);
}
