// What the multi-interest kernels share (mind.hip, comirec.hip): the limits and the launch cap, wave-level helpers, the
// series / item gather into LDS, the lambda-operand MFMA block, one routing row both ways (the forward rounds: masked
// softmax over the positions, weighted sum + squash, logit update; the backward of a round: the squash and the softmax),
// the three products around an example held in LDS (x S, du S^T and x^T du with its per-workgroup slot), the frame of the
// one-wave-per-example item kernels (LDS carve, load, scores, log-sum-exp loss and its gradient) and the host side: the
// head of the series arguments, the item arguments, the shape checks, the 4/2/1 wave ladder and the launches.
#pragma once
#include <float.h>
#include <math.h>
#include "common.h"
#include "mfma_tile.h"

namespace {

// the widths and the capsules are DIN's and AFM's limits; the rounds and the launch cap are the header's own
constexpr int MI_MAXD = REC_DIN_MAX_D, MI_MAXK = REC_AFM_MAX_A, MI_MAXR = REC_CAPSULE_MAX_R;
constexpr int MI_NTHR = 256;
constexpr size_t MI_LDS_CAP = REC_TILE_LDS_CAP;
static_assert(MI_LDS_CAP <= REC_LDS_CU_BYTES, "the launch cap fits the LDS of a CU");

__host__ __device__ inline int mi_odd(int n) { return n | 1; }

// floats of LDS of one example of the item kernels (label-aware attention, hard attention): m [K][Dc | 1],
// x [Ns][Dc | 1], two [K][Ns] and two [Ns]
__host__ __device__ inline size_t la_lds_floats(int Ns, int Dc, int K) {
  return ((size_t)K + Ns) * mi_odd(Dc) + 2 * (size_t)K * Ns + 2 * (size_t)Ns;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// what one lane of a wave wrote to LDS is read by another lane of the SAME wave after it
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum_i a[i] b[i sb] over i < n, in that order; the operands of 8 terms are requested together so that the LDS latency is
// paid once per 8, not once per term (a is read at the same address by every lane: a broadcast)
__device__ __forceinline__ float mi_dot(const float* a, const float* b, int sb, int n) {
  float acc = 0.f;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float x[8], y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = a[i + j];
      y[j] = b[(i + j) * sb];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(x[j], y[j], acc);
  }
  for (; i < n; ++i) acc = fmaf(a[i], b[i * sb], acc);
  return acc;
}
// two sums over the same b: r1 = sum a1[i] b[i sb], r2 = sum a2[i] b[i sb]
__device__ __forceinline__ void mi_dot2(const float* a1, const float* a2, const float* b, int sb, int n, float& r1,
                                        float& r2) {
  float s1 = 0.f, s2 = 0.f;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float x[8], z[8], y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = a1[i + j];
      z[j] = a2[i + j];
      y[j] = b[(i + j) * sb];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1 = fmaf(x[j], y[j], s1);
      s2 = fmaf(z[j], y[j], s2);
    }
  }
  for (; i < n; ++i) {
    const float y = b[i * sb];
    s1 = fmaf(a1[i], y, s1);
    s2 = fmaf(a2[i], y, s2);
  }
  r1 = s1;
  r2 = s2;
}

// one 32 x 32 block of acc += A Bm over k < Kd: fa(k) is A[row lo][k], fb(k) is Bm[k][column lo], both already masked.
// The operands of U k-steps are requested together (an operand may come from global memory: one latency per U steps).
template <class FA, class FB>
__device__ __forceinline__ void mi_mma(f32x16& acc, int Kd, int hi, FA fa, FB fb) {
  constexpr int U = 8;
  for (int k = 0; k < Kd; k += 2 * U) {
    float av[U], bv[U];
#pragma unroll
    for (int s = 0; s < U; ++s) {
      const int kk = k + 2 * s + hi;
      const bool kok = kk < Kd;
      const int kc = kok ? kk : Kd - 1;
      const float x = fa(kc), y = fb(kc);
      av[s] = kok ? x : 0.f;
      bv[s] = kok ? y : 0.f;
    }
#pragma unroll
    for (int s = 0; s < U; ++s)
      if (k + 2 * s < Kd) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);   // uniform
  }
}

// rows x (C E) looked-up values of ids [rows][C] into xs [rows][stride], by NT threads (this one is tid): the ids of U
// elements are requested together, then their values, with no branch between them (an id outside [0, V) reads row 0 and
// keeps a zero); valid != NULL: valid[row] = ids[row][0] != pad, taken from the id the element (row, 0) has read anyway
template <int NT>
__device__ __forceinline__ void mi_gather(const float* __restrict__ embed, int64_t ld, int64_t V,
                                          const int64_t* __restrict__ ids, int rows, int C, int E, float* xs, int stride,
                                          int tid, bool& bad, int64_t pad = 0, int* valid = nullptr) {
  constexpr int U = 4;
  const int D = C * E, n = rows * D;
  for (int i0 = tid; i0 < n; i0 += NT * U) {
    int64_t id[U];
    int at[U], e[U], row[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int i = i0 + j * NT, ic = i < n ? i : n - 1;
      const int t = ic / D, d = ic - t * D, r = d / E;
      e[j] = d - r * E;
      at[j] = t * stride + d;
      row[j] = d == 0 ? t : -1;
      id[j] = ids[(int64_t)t * C + r];
    }
    float v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const bool ok = id[j] >= 0 && id[j] < V;
      const float x = embed[(ok ? id[j] : 0) * ld + e[j]];
      v[j] = ok ? x : 0.f;
      bad |= !ok;
    }
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (i0 + j * NT < n) {
        xs[at[j]] = v[j];
        if (valid && row[j] >= 0) valid[row[j]] = id[j] != pad;
      }
  }
}

// ---- one routing row, by one wave: nothing but wave-level ordering ---------------------------------------------------
// Wk[t] = softmax_t(part[t] ? Lk[t] : -FLT_MAX)
__device__ __forceinline__ void caps_softmax_row(const float* Lk, const int* part, float* Wk, int T, int lane) {
  float m = -FLT_MAX;
  for (int t = lane; t < T; t += 64) m = fmaxf(m, part[t] ? Lk[t] : -FLT_MAX);
  m = wave_max(m);
  float sum = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float ex = expf((part[t] ? Lk[t] : -FLT_MAX) - m);
    Wk[t] = ex;
    sum += ex;
  }
  sum = group_sum<64>(sum);
  for (int t = lane; t < T; t += 64) Wk[t] = Wk[t] / sum;
  wave_sync();
}
// ck = squash(Wk u) with u [T][Dcp]; orow (may be NULL): the row of out it also goes to
__device__ __forceinline__ void caps_squash_row(const float* Wk, const float* u, int Dcp, int T, int Dc, float* ck,
                                                float* __restrict__ orow, int lane) {
  float n2 = 0.f;
  for (int d = lane; d < Dc; d += 64) {                        // s = W u
    const float acc = mi_dot(Wk, u + d, Dcp, T);
    ck[d] = acc;
    n2 = fmaf(acc, acc, n2);
  }
  n2 = group_sum<64>(n2);
  const float f = sqrtf(n2) / (1.f + n2);
  for (int d = lane; d < Dc; d += 64) {
    const float cv = ck[d] * f;
    ck[d] = cv;
    if (orow) orow[d] = cv;
  }
  wave_sync();
}
// Lk += ck u^T
__device__ __forceinline__ void caps_logit_update(float* Lk, const float* ck, const float* u, int Dcp, int T, int Dc,
                                                  int lane) {
  for (int t = lane; t < T; t += 64) {
    Lk[t] = Lk[t] + mi_dot(ck, u + t * Dcp, 1, Dc);
  }
  wave_sync();
}

// the R rounds of one row: the weights of round r go to W0 + r wstep with KEEP (the backward), to W0 otherwise; orow (may
// be NULL): the row of out that c of the last round also goes to
template <bool KEEP>
__device__ __forceinline__ void caps_route_rounds(float* Lk, const int* part, float* W0, int wstep, const float* u, int Dcp,
                                                  int T, int Dc, int R, float* ck, float* __restrict__ orow, int lane) {
  for (int r = 0; r < R; ++r) {
    float* Wk = KEEP ? W0 + (size_t)r * wstep : W0;
    caps_softmax_row(Lk, part, Wk, T, lane);
    caps_squash_row(Wk, u, Dcp, T, Dc, ck, r == R - 1 ? orow : nullptr, lane);
    if (r < R - 1) caps_logit_update(Lk, ck, u, Dcp, T, Dc, lane);         // L += c u^T
  }
}
// A round, back.  Neither step ends in an ordering of its own: the callers differ there.
// s = Wk u, dc = grow (the last round: the row of gout) or dLk u  ->  dsk = squash'(s) dc, ck = squash(s)
__device__ __forceinline__ void caps_squash_bwd_row(const float* Wk, const float* dLk, const float* u, int Dcp, int T,
                                                    int Dc, const float* __restrict__ grow, float* dsk, float* ck,
                                                    int lane) {
  float n2 = 0.f, sd = 0.f;
  for (int d = lane; d < Dc; d += 64) {
    float acc = 0.f, dc = 0.f;
    if (grow) {
      dc = grow[d];
      acc = mi_dot(Wk, u + d, Dcp, T);
    } else {
      mi_dot2(Wk, dLk, u + d, Dcp, T, acc, dc);
    }
    ck[d] = acc;
    dsk[d] = dc;
    n2 = fmaf(acc, acc, n2);
    sd = fmaf(acc, dc, sd);
  }
  n2 = group_sum<64>(n2);
  sd = group_sum<64>(sd);
  const float n = sqrtf(n2), den = 1.f + n2, f = n / den;
  const float g = n > 0.f ? (1.f - n2) / (den * den * n) * sd : 0.f;       // f'(n) / n (s . dc)
  for (int d = lane; d < Dc; d += 64) {
    const float sv = ck[d];
    dsk[d] = fmaf(sv, g, f * dsk[d]);
    ck[d] = sv * f;
  }
}
// dWk = dsk u^T, dLk += part ? Wk (dWk - sum_t dWk Wk) : 0
__device__ __forceinline__ void caps_softmax_bwd_row(const float* dsk, const float* u, int Dcp, int T, int Dc,
                                                     const float* Wk, const int* part, float* dWk, float* dLk, int lane) {
  float dot = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float acc = mi_dot(dsk, u + t * Dcp, 1, Dc);
    dWk[t] = acc;
    dot = fmaf(acc, Wk[t], dot);
  }
  dot = group_sum<64>(dot);
  for (int t = lane; t < T; t += 64)
    if (part[t]) dLk[t] = dLk[t] + Wk[t] * (dWk[t] - dot);
}

// ---- the products around one example in LDS, by a workgroup of 4 waves ------------------------------------------------
// u [T][Dcp] = act(xs [T][Dp] S [D, Dc]) on v_mfma_f32_32x32x2_f32, one (32 rows, 32 columns) block per wave and step, S
// read from global memory (every workgroup reads the same few KiB); act is tanh or nothing
template <bool TANH>
__device__ __forceinline__ void caps_project(const float* xs, int Dp, const float* __restrict__ S, int T, int D, int Dc,
                                             float* u, int Dcp, int wave, int lo, int hi) {
  const int ncb = (Dc + 31) / 32, ntile = (T + 31) / 32;
  for (int task = wave; task < ntile * ncb; task += 4) {
    const int tile = task / ncb, cb = task - tile * ncb;
    const int t = tile * 32 + lo, n = cb * 32 + lo;
    const bool tok = t < T, nok = n < Dc;
    const float* xr = xs + (tok ? t : T - 1) * Dp;
    const float* __restrict__ Sc = S + (nok ? n : Dc - 1);
    f32x16 acc;
    mb_zero(acc);
    mi_mma(acc, D, hi, [&](int k) { return tok ? xr[k] : 0.f; },
           [&](int k) { const float v = Sc[(int64_t)k * Dc]; return nok ? v : 0.f; });
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = tile * 32 + mb_row(r, hi);
      if (row < T && nok) u[row * Dcp + n] = TANH ? tanhf(acc[r]) : acc[r];
    }
  }
}
// gk [T][D] (global, the example's rows of gkeys) = du [T][Dcp] S^T
__device__ __forceinline__ void caps_keys_grad(const float* du, int Dcp, const float* __restrict__ S, int T, int D, int Dc,
                                               float* __restrict__ gk, int wave, int lo, int hi) {
  const int ndb = (D + 31) / 32, ntile = (T + 31) / 32;
  for (int task = wave; task < ntile * ndb; task += 4) {
    const int tile = task / ndb, db = task - tile * ndb;
    const int t = tile * 32 + lo, n = db * 32 + lo;
    const bool tok = t < T, nok = n < D;
    const float* dr = du + (tok ? t : T - 1) * Dcp;
    const float* __restrict__ Sr = S + (int64_t)(nok ? n : D - 1) * Dc;
    f32x16 acc;
    mb_zero(acc);
    mi_mma(acc, Dc, hi, [&](int k) { return tok ? dr[k] : 0.f; },
           [&](int k) { const float v = Sr[k]; return nok ? v : 0.f; });
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int row = tile * 32 + mb_row(rr, hi);
      if (row < T && nok) gk[(int64_t)row * D + n] = acc[rr];
    }
  }
}
// sacc += xs^T du over T rows: the NB 32 x 32 blocks (block blk0 + w, blk0 + w + 4, ...) of the [D, Dc] weight gradient
// this wave keeps in registers
template <int NB>
__device__ __forceinline__ void caps_weight_grad(f32x16 (&sacc)[NB], const float* xs, int Dp, const float* du, int Dcp,
                                                 int T, int D, int Dc, int wave, int lo, int hi, int blk0 = 0) {
  const int ncb = (Dc + 31) / 32, ndb = (D + 31) / 32;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int blk = blk0 + wave + 4 * j;
    if (blk < ndb * ncb) {
      const int db = blk / ncb, cb = blk - db * ncb;
      const int m = db * 32 + lo, n = cb * 32 + lo;
      const bool mok = m < D, nok = n < Dc;
      const float* xc = xs + (mok ? m : D - 1);
      const float* dcn = du + (nok ? n : Dc - 1);
      mi_mma(sacc[j], T, hi, [&](int k) { const float v = xc[k * Dp]; return mok ? v : 0.f; },
             [&](int k) { const float v = dcn[k * Dcp]; return nok ? v : 0.f; });
    }
  }
}
// the blocks into the workgroup's slot [D][Dc]; add: onto what the slot holds
template <int NB>
__device__ __forceinline__ void caps_weight_store(const f32x16 (&sacc)[NB], float* __restrict__ slot, int D, int Dc,
                                                  int wave, int lo, int hi, int blk0 = 0, bool add = false) {
  const int ncb = (Dc + 31) / 32, ndb = (D + 31) / 32;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int blk = blk0 + wave + 4 * j;
    if (blk < ndb * ncb) {
      const int db = blk / ncb, cb = blk - db * ncb, n = cb * 32 + lo;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int m = db * 32 + mb_row(rr, hi);
        if (m < D && n < Dc) slot[m * Dc + n] = add ? slot[m * Dc + n] + sacc[j][rr] : sacc[j][rr];
      }
    }
  }
}

// ---- the item kernels: one wave per example, blockDim.x / 64 examples per workgroup, no workgroup-level barrier -----
struct ItemArgs {
  const float* embed;
  int64_t ld, V;
  const int64_t* items;
  int64_t B;
  const float* m;
  const int32_t* kv;                                             // NULL for the hard attention
  int Ns, C, E, Dc, K;
};
// the LDS of the wave's example (la_lds_floats): m [K][Dcp], x [Ns][Dcp], the scores [K][Ns], a second [K][Ns], two [Ns]
struct ItemLds {
  float *ms, *xs, *sc, *w, *o, *go;
};
__device__ __forceinline__ ItemLds la_carve(float* lds, int wave, int Ns, int Dc, int K) {
  ItemLds f;
  f.ms = lds + (size_t)wave * la_lds_floats(Ns, Dc, K);
  f.xs = f.ms + K * mi_odd(Dc);
  f.sc = f.xs + Ns * mi_odd(Dc);
  f.w = f.sc + K * Ns;
  f.o = f.w + K * Ns;
  f.go = f.o + Ns;
  return f;
}
// m of example b and its looked-up items into LDS; the caller orders
__device__ __forceinline__ void la_load(const ItemArgs& a, int64_t b, const ItemLds& f, int lane, bool& bad) {
  const int Dc = a.Dc, Dcp = mi_odd(Dc);
  for (int i = lane; i < a.K * Dc; i += 64) {
    const int k = i / Dc, d = i - k * Dc;
    f.ms[k * Dcp + d] = a.m[b * a.K * Dc + i];
  }
  mi_gather<64>(a.embed, a.ld, a.V, a.items + b * a.Ns * a.C, a.Ns, a.C, a.E, f.xs, Dcp, lane, bad);
}
// sc[k][s] = m_k . x_s
__device__ __forceinline__ void la_scores(const ItemLds& f, int Ns, int Dc, int K, int lane) {
  const int Dcp = mi_odd(Dc);
  for (int i = lane; i < K * Ns; i += 64) {
    const int k = i / Ns, s = i - k * Ns;
    float acc = 0.f;
    for (int d = 0; d < Dc; ++d) acc = fmaf(f.ms[k * Dcp + d], f.xs[s * Dcp + d], acc);
    f.sc[i] = acc;
  }
  wave_sync();
}
// logsumexp_s o[s]; the loss is that minus o[0]
__device__ __forceinline__ float la_logsumexp(const float* o, int Ns, int lane) {
  float mx = -FLT_MAX;
  for (int s = lane; s < Ns; s += 64) mx = fmaxf(mx, o[s]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int s = lane; s < Ns; s += 64) sum += expf(o[s] - mx);
  sum = group_sum<64>(sum);
  return mx + logf(sum);
}
// go[s] = grow[s] + gl (softmax_s(o)[s] - [s == 0]); grow (may be NULL): the example's row of the gradient of o
__device__ __forceinline__ void la_loss_grad(const ItemLds& f, float lse, float gl, const float* __restrict__ grow, int Ns,
                                             int lane) {
  for (int s = lane; s < Ns; s += 64) {
    const float g = grow ? grow[s] : 0.f;
    f.go[s] = fmaf(gl, expf(f.o[s] - lse) - (s == 0 ? 1.f : 0.f), g);
  }
  wave_sync();
}

// ---- the host side ---------------------------------------------------------------------------------------------------
// what every series kernel is given first: the table, the ids [B, T, C] and the sizes (D = E C)
struct CapsSeries {
  const float* embed;
  int64_t ld, V;
  const int64_t* series;
  int64_t B, padding_index;
  int T, C, E, D, Dc, K;
};
static inline int caps_fits(size_t lds_bytes) { return lds_bytes <= MI_LDS_CAP ? REC_OK : REC_E_UNSUPPORTED; }
// the sizes of a series family (R = 1 where it has no rounds); its LDS fit is the family's own
static inline int caps_series_shape(int64_t B, int T, int E, int C, int Dc, int K, int R) {
  if (B < 0 || T < 1 || E < 1 || C < 1 || Dc < 1 || K < 1 || R < 1) return REC_E_ARG;
  if ((int64_t)E * C > MI_MAXD || Dc > MI_MAXD || K > MI_MAXK || R > MI_MAXR || B >= ((int64_t)1 << 31) ||
      T > (int)(MI_LDS_CAP / sizeof(float)))
    return REC_E_UNSUPPORTED;
  return REC_OK;
}
// waves of a workgroup when each holds `one` bytes of LDS: 4, 2 or 1, as many as fit; 0: not even one
static inline int caps_waves(size_t one) {
  return 4 * one <= MI_LDS_CAP ? 4 : (2 * one <= MI_LDS_CAP ? 2 : (one <= MI_LDS_CAP ? 1 : 0));
}
// one launch of a kernel whose dynamic LDS may go up to the cap
template <auto Kernel, class... Args>
static int caps_launch(dim3 grid, int nthr, size_t lds, hipStream_t st, Args... args) {
  if (hipError_t err = rec_allow_lds<Kernel>(MI_LDS_CAP)) return (int)err;
  hipLaunchKernelGGL(Kernel, grid, dim3(nthr), lds, st, args...);
  REC_LAUNCH_CHECK();
  return REC_OK;
}
// workgroups of a persistent forward: one example at a time each
static inline int caps_fwd_grid(int64_t B) { return B < 65536 ? (int)B : 65536; }

// 32 x 32 blocks of the weight gradient per wave: 1, 4 or 16
static inline int caps_weight_nb(int D, int Dc) {
  const int nblk = ((D + 31) / 32) * ((Dc + 31) / 32), nb = (nblk + 3) / 4;
  return nb <= 1 ? 1 : (nb <= 4 ? 4 : 16);
}
// f(std::integral_constant<int, NB>) for that NB: the one spelling of the 1 / 4 / 16 template dispatch
template <class Fn>
static inline int caps_launch_nb(int nb, Fn&& f) {
  return nb == 1   ? f(std::integral_constant<int, 1>{})
         : nb == 4 ? f(std::integral_constant<int, 4>{})
                   : f(std::integral_constant<int, 16>{});
}
// as many workgroups as the chip holds at once: 4, 2 or 1 per CU by the registers of the instantiation (1, 4 or 16 blocks
// of the weight gradient per wave), 256 CUs; `most` workgroups at 4 per CU
static inline int caps_grid(int64_t B, int D, int Dc, int most) {
  const int nb = caps_weight_nb(D, Dc);
  const int cap = nb == 1 ? most : (nb == 4 ? most / 2 : most / 4);
  return B < cap ? (int)B : cap;
}

// the item kernels: examples of a workgroup, LDS of a launch, shape check and launch
static inline int la_waves(int Ns, int Dc, int K) { return caps_waves(sizeof(float) * la_lds_floats(Ns, Dc, K)); }
static inline size_t la_lds_bytes(int Ns, int Dc, int K) {
  return sizeof(float) * la_waves(Ns, Dc, K) * la_lds_floats(Ns, Dc, K);
}
static inline int la_shape(int64_t B, int Ns, int E, int C, int K) {
  if (B < 0 || Ns < 1 || E < 1 || C < 1 || K < 1) return REC_E_ARG;
  if ((int64_t)E * C > MI_MAXD || K > MI_MAXK || B >= ((int64_t)1 << 31) || Ns > (int)(MI_LDS_CAP / sizeof(float)))
    return REC_E_UNSUPPORTED;
  return caps_fits(sizeof(float) * la_lds_floats(Ns, E * C, K));
}
template <auto Kernel, class... Args>
static int la_launch(const ItemArgs& a, void* stream, Args... args) {
  const int wpb = la_waves(a.Ns, a.Dc, a.K);
  return caps_launch<Kernel>(dim3((unsigned)ceil_div64(a.B, wpb)), 64 * wpb, la_lds_bytes(a.Ns, a.Dc, a.K),
                             as_stream(stream), a, args...);
}

}  // namespace
