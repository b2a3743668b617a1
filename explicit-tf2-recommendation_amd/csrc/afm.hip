// Attentional Factorization Machine (InteractionLayer / AttentionLayer / AttentionalFactorizationMachine,
// 3.DCN/CustomLayers.py:825-885) on gfx950, fused with the embedding lookup.  Per example, ids X[b, 0..F-1]:
//   e_f = table[X[b,f]]          p_k = e_i * e_j   for the P = F(F-1)/2 pairs i < j, i outer, j inner
//   pre_k = p_k Wa + ba [A]      s_k = relu(pre_k) . hv + bh       a = softmax over k of s       o = sum_k a_k p_k [E]
// Everything after the gather depends on one example's F rows only, so each direction is ONE kernel and the [B,P,E]
// tensor of the reference never exists:
//   emb_afm_fwd_kernel   a group of LPE (16 or 64) lanes per example.  ids -> LDS, rows -> LDS (row stride E + 4 floats
//                        when E % 4 == 0: 16 lanes reading 16 different rows as float4 hit 16 different bank groups),
//                        lane q scores the pairs q, q + LPE, ...; max and sum by a butterfly inside the group; then the
//                        lanes own output dims and add exp(s_k - m) p_k over the pairs.  Writes o, (m, l) per example
//                        and, when asked, the gathered rows.
//   emb_afm_bwd_kernel   persistent grid.  Rows again (gathered again, or read from the saved rows), do and o -> LDS.
//                        With c = do . o:  ds_k = a_k (do . p_k - c), dpre_k = ds_k hv (pre_k > 0), kept in LDS with
//                        a_k; then one thread per (field, dim) adds dp_k * e_other over the F-1 pairs of its field
//                        (dp_k = a_k do + Wa dpre_k) and writes the IndexedSlices values; then dWa = sum_k p_k (x)
//                        dpre_k with one thread per (element, share of the pairs).  The parameter gradients stay in
//                        registers over the tiles of a workgroup and go to a slot of its own;
//   and rec_slot_sum adds the slots in its wave order.
// Wa, ba, hv are read with wave-uniform addresses straight from global memory (scalar loads).  No float atomics:
// gradients are bit-identical run to run.  Scores are computed by ONE routine with explicit fmas (fp contraction is off
// in this file), so the backward sees exactly the forward's s_k: at F = 2, a == 1, o == p_0 and dWa == dba == dhv == 0
// exactly.  No host synchronisation: both directions can be captured in a graph.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AFM_NT = 256;
constexpr int AFM_MAXF = REC_AFM_MAX_F, AFM_MAXE = REC_AFM_MAX_E, AFM_MAXA = REC_AFM_MAX_A;
constexpr int AFM_MAXG = 1024;                  // workgroups (= workspace slots) of the backward
constexpr int AFM_WPT = 16;                     // dWa elements per thread: E A <= 1024 over >= 64 threads
constexpr size_t AFM_LDS_SOFT = 64 * 1024;      // what a workgroup aims for
constexpr size_t AFM_LDS_MAX = REC_LDS_CU_BYTES;

struct AfmShape {
  int64_t B, V, ld;
  int F, E, A, P, RS, LPE, EP, vec;             // RS: LDS row stride; EP lanes of a group over the output dims
};

struct AfmCfg {
  int epw[2], nthr[2], grid[2];                 // forward, backward
  size_t lds[2];
};

__host__ __device__ inline int afm_r4(int n) { return (n + 3) & ~3; }
// floats of LDS per example: rows | forward: s [P]; backward: (a, dpre) [P, A+1] | do [E] | o [E]
__host__ __device__ inline int afm_ex_floats(const AfmShape& s, int bwd) {
  return afm_r4(s.F * s.RS) + (bwd ? afm_r4(s.P * (s.A + 1)) + 2 * afm_r4(s.E) : afm_r4(s.P));
}
// floats of the backward's reduction buffer: per-wave (dba, dhv, dbh), then the shares of dWa (<= one per thread)
__host__ __device__ inline int afm_red_floats(const AfmShape& s, int nthr) {
  const int a = (nthr / 64) * (2 * s.A + 1);
  return afm_r4(a > nthr ? a : nthr);
}

__device__ __forceinline__ void afm_pair_at(int k, int F, int& i, int& j) {          // k < P
  i = 0;
  while (k >= F - 1 - i) {
    k -= F - 1 - i;
    ++i;
  }
  j = i + 1 + k;
}
__device__ __forceinline__ void afm_pair_step(int step, int F, int& i, int& j) {
  j += step;
  while (j >= F && i < F) {
    j = j - F + i + 2;
    ++i;
  }
}

// pre[a] = (e_i * e_j) . Wa[:, a] + ba[a]; returns d . (e_i * e_j) when d is given.  One fma order for both kernels.
template <bool VEC, int AC>
__device__ __forceinline__ float afm_pair_pre(const float* __restrict__ ei, const float* __restrict__ ej,
                                              const float* __restrict__ d, int E, int A, const float* __restrict__ Wa,
                                              const float* __restrict__ ba, float (&pre)[AC]) {
#pragma unroll
  for (int a = 0; a < AC; ++a) pre[a] = 0.f;
  float g = 0.f;
  if (VEC) {
    for (int e = 0; e < E; e += 4) {
      const float4 x = *reinterpret_cast<const float4*>(ei + e), y = *reinterpret_cast<const float4*>(ej + e);
      const float p0 = x.x * y.x, p1 = x.y * y.y, p2 = x.z * y.z, p3 = x.w * y.w;
      if (d) {
        const float4 dv = *reinterpret_cast<const float4*>(d + e);
        g = fmaf(dv.x, p0, g);
        g = fmaf(dv.y, p1, g);
        g = fmaf(dv.z, p2, g);
        g = fmaf(dv.w, p3, g);
      }
      const float* w = Wa + e * A;
#pragma unroll
      for (int a = 0; a < AC; ++a)
        if (AC <= 4 || a < A) {
          pre[a] = fmaf(p0, w[a], pre[a]);
          pre[a] = fmaf(p1, w[A + a], pre[a]);
          pre[a] = fmaf(p2, w[2 * A + a], pre[a]);
          pre[a] = fmaf(p3, w[3 * A + a], pre[a]);
        }
    }
  } else {
    for (int e = 0; e < E; ++e) {
      const float p = ei[e] * ej[e];
      if (d) g = fmaf(d[e], p, g);
      const float* w = Wa + e * A;
#pragma unroll
      for (int a = 0; a < AC; ++a)
        if (AC <= 4 || a < A) pre[a] = fmaf(p, w[a], pre[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < AC; ++a)
    if (AC <= 4 || a < A) pre[a] += ba[a];
  return g;
}

// d . o in the order afm_pair_pre adds d . p: equal bits when o == p (F = 2)
template <bool VEC>
__device__ __forceinline__ float afm_dot(const float* __restrict__ d, const float* __restrict__ o, int E) {
  float g = 0.f;
  for (int e = 0; e < E; ++e) g = fmaf(d[e], o[e], g);
  return g;
}

template <int AC>
__device__ __forceinline__ float afm_score(const float (&pre)[AC], int A, const float* __restrict__ hv, float bh) {
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < AC; ++a)
    if (AC <= 4 || a < A) s = fmaf(fmaxf(pre[a], 0.f), hv[a], s);
  return s + bh;
}

// ids of a tile as 32-bit row numbers in LDS (-1: out of range); true when one was out of range
__device__ __forceinline__ bool afm_load_ids(const AfmShape& s, const int64_t* __restrict__ X, int64_t b0, int n_ex,
                                             int* __restrict__ ids) {
  bool bad = false;
  for (int t = threadIdx.x; t < n_ex * s.F; t += blockDim.x) {
    const int64_t id = X[b0 * s.F + t];
    const bool ok = (uint64_t)id < (uint64_t)s.V;
    bad |= !ok;
    ids[t] = ok ? (int)id : -1;
  }
  return bad;
}

// rows of a tile -> LDS (example stride exF, row stride RS): from src [B,F,E] when given, else gathered from the table
// by the ids in LDS (an out-of-range id reads as a zero row); copied to rows_out [B,F,E] when given
__device__ __forceinline__ void afm_load_rows(const AfmShape& s, int gvec, const float* __restrict__ table,
                                              const float* __restrict__ src, const int* __restrict__ ids, int64_t b0,
                                              int n_ex, int exF, float* __restrict__ lds, float* __restrict__ rows_out) {
  const int F = s.F, E = s.E;
  if (gvec) {
    const int E4 = E >> 2;
    for (int t = threadIdx.x; t < n_ex * F * E4; t += blockDim.x) {
      const int r = t / E4, c = t - r * E4, ex = r / F, f = r - ex * F;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src) {
        v = reinterpret_cast<const float4*>(src)[(b0 * F + r) * E4 + c];
      } else {
        const int id = ids[r];
        if (id >= 0) v = *reinterpret_cast<const float4*>(table + (int64_t)id * s.ld + 4 * c);
      }
      *reinterpret_cast<float4*>(lds + ex * exF + f * s.RS + 4 * c) = v;
      if (rows_out) reinterpret_cast<float4*>(rows_out)[(b0 * F + r) * E4 + c] = v;
    }
  } else {
    for (int t = threadIdx.x; t < n_ex * F * E; t += blockDim.x) {
      const int r = t / E, c = t - r * E, ex = r / F, f = r - ex * F;
      float v = 0.f;
      if (src) {
        v = src[(b0 * F + r) * E + c];
      } else {
        const int id = ids[r];
        if (id >= 0) v = table[(int64_t)id * s.ld + c];
      }
      lds[ex * exF + f * s.RS + c] = v;
      if (rows_out) rows_out[(b0 * F + r) * E + c] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// forward: grid = ceil(B / EPW), block = EPW * LPE threads
// ------------------------------------------------------------------------------------------------------------------
template <bool VEC, int AC>
__global__ __launch_bounds__(AFM_NT) void emb_afm_fwd_kernel(AfmShape s, int EPW, int gvec,
                                                             const float* __restrict__ table,
                                                             const int64_t* __restrict__ X,
                                                             const float* __restrict__ Wa, const float* __restrict__ ba,
                                                             const float* __restrict__ hv, const float* __restrict__ bh,
                                                             float* __restrict__ o, float* __restrict__ stats,
                                                             float* __restrict__ rows_out, int* oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E, A = s.A, P = s.P, RS = s.RS, LPE = s.LPE;
  const int exF = afm_ex_floats(s, 0);
  int* ids = reinterpret_cast<int*>(lds + EPW * exF);
  const int64_t b0 = (int64_t)blockIdx.x * EPW;
  const int n_ex = (int)min((int64_t)EPW, s.B - b0);
  if (afm_load_ids(s, X, b0, n_ex, ids) && oob) *oob = 1;
  __syncthreads();
  afm_load_rows(s, gvec, table, nullptr, ids, b0, n_ex, exF, lds, rows_out);
  __syncthreads();

  const int ex = threadIdx.x / LPE, q = threadIdx.x - ex * LPE;
  const bool valid = ex < n_ex;
  const float* R = lds + ex * exF;
  float* S = lds + ex * exF + afm_r4(F * RS);
  const float bhv = bh[0];
  float m = -INFINITY;
  if (valid && q < P) {
    int i, j;
    afm_pair_at(q, F, i, j);
    for (int k = q; k < P; k += LPE) {
      float pre[AC];
      afm_pair_pre<VEC, AC>(R + i * RS, R + j * RS, nullptr, E, A, Wa, ba, pre);
      const float sc = afm_score<AC>(pre, A, hv, bhv);
      S[k] = sc;
      m = fmaxf(m, sc);
      afm_pair_step(LPE, F, i, j);
    }
  }
  for (int w = LPE >> 1; w > 0; w >>= 1) m = fmaxf(m, __shfl_xor(m, w, 64));
  float l = 0.f;
  if (valid)
    for (int k = q; k < P; k += LPE) {
      const float w = expf(S[k] - m);
      S[k] = w;
      l += w;
    }
  for (int w = LPE >> 1; w > 0; w >>= 1) l += __shfl_xor(l, w, 64);
  __syncthreads();                                             // the weights of every lane of the group

  const int EP = s.EP, nsub = LPE / EP, sub = q / EP, c = q - sub * EP;
  for (int e0 = 0; e0 < E; e0 += EP) {
    const int e = e0 + c;
    float acc = 0.f;
    if (valid && e < E && sub < P) {
      int i, j;
      afm_pair_at(sub, F, i, j);
      for (int k = sub; k < P; k += nsub) {
        acc = fmaf(S[k], R[i * RS + e] * R[j * RS + e], acc);
        afm_pair_step(nsub, F, i, j);
      }
    }
    for (int w = EP; w < LPE; w <<= 1) acc += __shfl_xor(acc, w, 64);
    if (valid && e < E && sub == 0) o[(b0 + ex) * E + e] = acc / l;
  }
  if (valid && q == 0) {
    stats[2 * (b0 + ex)] = m;
    stats[2 * (b0 + ex) + 1] = l;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward: persistent grid, block = EPW * LPE threads (a multiple of 64); slot of workgroup g [E A + 2 A + 1] =
// dWa | dba | dhv | dbh
// ------------------------------------------------------------------------------------------------------------------
template <bool VEC, int AC>
__global__ __launch_bounds__(AFM_NT) void emb_afm_bwd_kernel(AfmShape s, int EPW, int gvec,
                                                             const float* __restrict__ table,
                                                             const int64_t* __restrict__ X,
                                                             const float* __restrict__ Wa, const float* __restrict__ ba,
                                                             const float* __restrict__ hv, const float* __restrict__ bh,
                                                             const float* __restrict__ o,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ rows_in,
                                                             const float* __restrict__ dout, float* __restrict__ vals,
                                                             float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E, A = s.A, P = s.P, RS = s.RS, LPE = s.LPE, A1 = A + 1, EA = E * A;
  const int nthr = blockDim.x;
  const int exF = afm_ex_floats(s, 1);
  const int offQ = afm_r4(F * RS), offD = offQ + afm_r4(P * A1), offO = offD + afm_r4(E);
  float* red = lds + EPW * exF;
  int* ids = reinterpret_cast<int*>(red + afm_red_floats(s, nthr));
  const int ex = threadIdx.x / LPE, q = threadIdx.x - ex * LPE;
  const float bhv = bh[0];
  // dWa: thread = (element ea, share of the pairs); EA >= nthr: one share, up to AFM_WPT elements per thread
  const int EAs = EA >= nthr ? nthr : EA, nparts = EA >= nthr ? 1 : nthr / EA;
  const int part = threadIdx.x / EAs, ea0 = threadIdx.x - part * EAs;
  float accW[AFM_WPT], dhv[AC], dba[AC], dbh = 0.f;
#pragma unroll
  for (int u = 0; u < AFM_WPT; ++u) accW[u] = 0.f;
#pragma unroll
  for (int a = 0; a < AC; ++a) dhv[a] = dba[a] = 0.f;

  const int64_t ntiles = (s.B + EPW - 1) / EPW;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t b0 = tl * EPW;
    const int n_ex = (int)min((int64_t)EPW, s.B - b0);
    if (!rows_in) {
      afm_load_ids(s, X, b0, n_ex, ids);
      __syncthreads();
    }
    afm_load_rows(s, gvec, table, rows_in, ids, b0, n_ex, exF, lds, nullptr);
    for (int t = threadIdx.x; t < n_ex * E; t += nthr) {
      const int x = t / E, e = t - x * E;
      lds[x * exF + offD + e] = dout[(b0 + x) * E + e];
      lds[x * exF + offO + e] = o[(b0 + x) * E + e];
    }
    __syncthreads();

    const bool valid = ex < n_ex;
    if (valid && q < P) {                                      // the pairs q, q + LPE, ... of example ex
      const float* R = lds + ex * exF;
      float* Q = lds + ex * exF + offQ;
      const float* D = lds + ex * exF + offD;
      const float mx = stats[2 * (b0 + ex)], lx = stats[2 * (b0 + ex) + 1];
      const float cdo = afm_dot<VEC>(D, lds + ex * exF + offO, E);
      int i, j;
      afm_pair_at(q, F, i, j);
      for (int k = q; k < P; k += LPE) {
        float pre[AC];
        const float g = afm_pair_pre<VEC, AC>(R + i * RS, R + j * RS, D, E, A, Wa, ba, pre);
        const float ak = expf(afm_score<AC>(pre, A, hv, bhv) - mx) / lx;
        const float ds = ak * (g - cdo);
        Q[k * A1] = ak;
        dbh += ds;
#pragma unroll
        for (int a = 0; a < AC; ++a)
          if (AC <= 4 || a < A) {
            const float dp = pre[a] > 0.f ? ds * hv[a] : 0.f;
            dhv[a] = fmaf(ds, fmaxf(pre[a], 0.f), dhv[a]);
            dba[a] += dp;
            Q[k * A1 + 1 + a] = dp;
          }
        afm_pair_step(LPE, F, i, j);
      }
    }
    __syncthreads();

    // vals[b, f, e] = sum_{j != f} dp_k[e] e_j[e],  dp_k[e] = a_k do[e] + sum_a Wa[e, a] dpre_k[a],  k = pair(f, j)
    for (int t = threadIdx.x; t < n_ex * F * E; t += nthr) {
      const int x = t / (F * E), r = t - x * F * E, f = r / E, e = r - f * E;
      const float* R = lds + x * exF;
      const float* Q = R + offQ;
      const float dv = R[offD + e];
      float wa[AC];
#pragma unroll
      for (int a = 0; a < AC; ++a) wa[a] = (AC <= 4 || a < A) ? Wa[e * A + a] : 0.f;
      float acc = 0.f;
      for (int j = 0; j < F; ++j) {
        if (j == f) continue;
        const int lo = j < f ? j : f, hi = j < f ? f : j;
        const float* qk = Q + (lo * (2 * F - lo - 1) / 2 + hi - lo - 1) * A1;
        float dp = qk[0] * dv;
#pragma unroll
        for (int a = 0; a < AC; ++a)
          if (AC <= 4 || a < A) dp = fmaf(wa[a], qk[1 + a], dp);
        acc = fmaf(dp, R[j * RS + e], acc);
      }
      vals[(b0 + x) * F * E + r] = acc;
    }

    // dWa[e, a] += sum over the tile's pairs of p_k[e] dpre_k[a]; the share `part` takes the (example, i) units
    // part, part + nparts, ...
    if (part < nparts) {
#pragma unroll
      for (int u = 0; u < AFM_WPT; ++u) {
        const int ea = ea0 + u * EAs;
        if (ea >= EA) break;
        const int e = ea / A, a = ea - e * A;
        float acc = 0.f;
        for (int unit = part; unit < n_ex * (F - 1); unit += nparts) {
          const int x = unit / (F - 1), i = unit - x * (F - 1);
          const float* R = lds + x * exF;
          const float* qk = R + offQ + (i * (2 * F - i - 1) / 2) * A1 + 1 + a;
          const float xi = R[i * RS + e];
          for (int j = i + 1; j < F; ++j, qk += A1) acc = fmaf(xi * R[j * RS + e], qk[0], acc);
        }
        accW[u] += acc;
      }
    }
    __syncthreads();                                           // the next tile rewrites the LDS
  }

  // the workgroup's slot: (dba, dhv, dbh) summed over the lanes of a wave, then over the waves in order; the shares of
  // dWa in order
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * (EA + 2 * A + 1);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = nthr >> 6, NS = 2 * A + 1;
#pragma unroll
  for (int a = 0; a < AC; ++a)
    if (AC <= 4 || a < A) {
      const float x = group_sum<64>(dba[a]), y = group_sum<64>(dhv[a]);
      if (lane == 0) {
        red[wv * NS + a] = x;
        red[wv * NS + A + a] = y;
      }
    }
  dbh = group_sum<64>(dbh);
  if (lane == 0) red[wv * NS + 2 * A] = dbh;
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    float acc = 0.f;
    for (int w = 0; w < nw; ++w) acc += red[w * NS + threadIdx.x];
    slot[EA + threadIdx.x] = acc;
  }
  __syncthreads();
  if (nparts == 1) {
    // part == 0 only: with E A < nthr < 2 E A the threads beyond E A hold no share (part == 1, accW == 0) but their ea0
    // wraps onto the elements 0 .. nthr - E A - 1, whose sums they would overwrite with zeros in whichever order the
    // waves arrive
#pragma unroll
    for (int u = 0; u < AFM_WPT; ++u) {
      const int ea = ea0 + u * EAs;
      if (part == 0 && ea < EA) slot[ea] = accW[u];
    }
  } else {
    if (part < nparts) red[part * EA + ea0] = accW[0];
    __syncthreads();
    if ((int)threadIdx.x < EA) {
      float acc = 0.f;
      for (int p = 0; p < nparts; ++p) acc += red[p * EA + threadIdx.x];
      slot[threadIdx.x] = acc;
    }
  }
}

// 0 ok (B == 0 included), REC_E_ARG, REC_E_UNSUPPORTED
static int afm_shape(int64_t B, int F, int E, int A, int64_t V, int64_t ld, AfmShape* s) {
  if (B < 0 || F < 0 || E < 0 || A < 0 || V <= 0 || ld < E) return REC_E_ARG;
  if (F < 2 || F > AFM_MAXF || E < 1 || E > AFM_MAXE || A < 1 || A > AFM_MAXA) return REC_E_UNSUPPORTED;
  if (B > 0x7fffffffLL || V >= ((int64_t)1 << 31)) return REC_E_UNSUPPORTED;
  *s = AfmShape{};
  s->B = B;
  s->V = V;
  s->ld = ld;
  s->F = F;
  s->E = E;
  s->A = A;
  s->P = F * (F - 1) / 2;
  s->vec = E % 4 == 0;
  s->RS = s->vec ? E + 4 : (E | 1);
  s->LPE = s->P <= 64 ? 16 : 64;
  int ep = 1;
  while (ep < E && ep < s->LPE) ep *= 2;
  s->EP = ep;
  return REC_OK;
}

static AfmCfg afm_cfg(const AfmShape& s) {
  AfmCfg k{};
  for (int d = 0; d < 2; ++d) {
    const int min_epw = 64 / s.LPE;                            // whole waves
    int epw = AFM_NT / s.LPE;
    size_t bytes;
    for (;;) {
      const int nthr = epw * s.LPE;
      bytes = ((size_t)epw * afm_ex_floats(s, d) + (d ? afm_red_floats(s, nthr) : 0) + (size_t)epw * s.F) * 4;
      if (bytes <= AFM_LDS_SOFT || epw <= min_epw) break;
      epw >>= 1;
    }
    const int64_t ntiles = (s.B + epw - 1) / epw;
    k.epw[d] = epw;
    k.nthr[d] = epw * s.LPE;
    k.lds[d] = bytes;
    k.grid[d] = (int)(d == 0 ? ntiles : (ntiles < AFM_MAXG ? ntiles : AFM_MAXG));
    if (k.grid[d] < 1) k.grid[d] = 1;
  }
  return k;
}

static size_t afm_ws_bytes(const AfmShape& s, const AfmCfg& k) {
  return rec_align_up((size_t)k.grid[1] * (s.E * s.A + 2 * s.A + 1) * sizeof(float), 256);
}

struct AfmFwdArgs {
  const float* table; const int64_t* X; const float *Wa, *ba, *hv, *bh;
  float *o, *stats, *rows; int* oob;
};
struct AfmBwdArgs {
  const float* table; const int64_t* X; const float *Wa, *ba, *hv, *bh, *o, *stats, *rows, *dout;
  float *vals, *slots;
};

template <bool VEC, int AC>
static int afm_fwd_launch(const AfmShape& s, const AfmCfg& k, int gvec, const AfmFwdArgs& a, hipStream_t st) {
  if (hipError_t e = rec_allow_lds<emb_afm_fwd_kernel<VEC, AC>>(AFM_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL((emb_afm_fwd_kernel<VEC, AC>), dim3(k.grid[0]), dim3(k.nthr[0]), k.lds[0], st, s, k.epw[0], gvec,
                     a.table, a.X, a.Wa, a.ba, a.hv, a.bh, a.o, a.stats, a.rows, a.oob);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

template <bool VEC, int AC>
static int afm_bwd_launch(const AfmShape& s, const AfmCfg& k, int gvec, const AfmBwdArgs& a, hipStream_t st) {
  if (hipError_t e = rec_allow_lds<emb_afm_bwd_kernel<VEC, AC>>(AFM_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL((emb_afm_bwd_kernel<VEC, AC>), dim3(k.grid[1]), dim3(k.nthr[1]), k.lds[1], st, s, k.epw[1], gvec,
                     a.table, a.X, a.Wa, a.ba, a.hv, a.bh, a.o, a.stats, a.rows, a.dout, a.vals, a.slots);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

#define AFM_DISPATCH(FN, ...)                                                                                        \
  do {                                                                                                               \
    if (s.vec) {                                                                                                     \
      switch (s.A) {                                                                                                 \
        case 1: return FN<true, 1>(__VA_ARGS__);                                                                     \
        case 2: return FN<true, 2>(__VA_ARGS__);                                                                     \
        case 3: return FN<true, 3>(__VA_ARGS__);                                                                     \
        case 4: return FN<true, 4>(__VA_ARGS__);                                                                     \
        default: return s.A <= 8 ? FN<true, 8>(__VA_ARGS__) : FN<true, 16>(__VA_ARGS__);                             \
      }                                                                                                              \
    }                                                                                                                \
    switch (s.A) {                                                                                                   \
      case 1: return FN<false, 1>(__VA_ARGS__);                                                                      \
      case 2: return FN<false, 2>(__VA_ARGS__);                                                                      \
      case 3: return FN<false, 3>(__VA_ARGS__);                                                                      \
      case 4: return FN<false, 4>(__VA_ARGS__);                                                                      \
      default: return s.A <= 8 ? FN<false, 8>(__VA_ARGS__) : FN<false, 16>(__VA_ARGS__);                             \
    }                                                                                                                \
  } while (0)

static int afm_fwd_dispatch(const AfmShape& s, const AfmCfg& k, int gvec, const AfmFwdArgs& a, hipStream_t st) {
  AFM_DISPATCH(afm_fwd_launch, s, k, gvec, a, st);
}
static int afm_bwd_dispatch(const AfmShape& s, const AfmCfg& k, int gvec, const AfmBwdArgs& a, hipStream_t st) {
  AFM_DISPATCH(afm_bwd_launch, s, k, gvec, a, st);
}

}  // namespace

extern "C" size_t rec_afm_workspace_bytes(int64_t B, int F, int E, int A) {
  AfmShape s;
  if (afm_shape(B, F, E, A, 1, E, &s) != REC_OK) return 0;
  const AfmCfg k = afm_cfg(s);
  if (k.lds[0] > AFM_LDS_MAX || k.lds[1] > AFM_LDS_MAX) return 0;
  return afm_ws_bytes(s, k);
}

extern "C" int rec_emb_afm_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F,
                                   int A, const float* Wa, const float* ba, const float* hv, const float* bh, float* o,
                                   float* stats, float* rows, int* oob_flag, void* stream) {
  AfmShape s;
  const int rc = afm_shape(B, F, E, A, V, ld, &s);
  if (rc != REC_OK || B == 0) return rc;
  if (!table || !X || !Wa || !ba || !hv || !bh || !o || !stats) return REC_E_ARG;
  const AfmCfg k = afm_cfg(s);
  if (k.lds[0] > AFM_LDS_MAX) return REC_E_UNSUPPORTED;
  const int gvec = s.vec && ld % 4 == 0 && rec_is_aligned16(table) && (!rows || rec_is_aligned16(rows));
  const AfmFwdArgs a{table, X, Wa, ba, hv, bh, o, stats, rows, oob_flag};
  return afm_fwd_dispatch(s, k, gvec, a, as_stream(stream));
}

extern "C" int rec_emb_afm_bwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F,
                                   int A, const float* Wa, const float* ba, const float* hv, const float* bh,
                                   const float* o, const float* stats, const float* rows, const float* dout,
                                   float* vals, float* dWa, float* dba, float* dhv, float* dbh, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  AfmShape s;
  const int rc = afm_shape(B, F, E, A, V, ld, &s);
  if (rc != REC_OK || B == 0) return rc;
  if ((!rows && (!table || !X)) || !Wa || !ba || !hv || !bh || !o || !stats || !dout || !vals || !dWa || !dba || !dhv ||
      !dbh || !workspace)
    return REC_E_ARG;
  const AfmCfg k = afm_cfg(s);
  if (k.lds[1] > AFM_LDS_MAX) return REC_E_UNSUPPORTED;
  if (workspace_bytes < afm_ws_bytes(s, k)) return REC_E_WORKSPACE;
  const int gvec = s.vec && (rows ? rec_is_aligned16(rows) : (ld % 4 == 0 && rec_is_aligned16(table)));
  hipStream_t st = as_stream(stream);
  const AfmBwdArgs a{table, X, Wa, ba, hv, bh, o, stats, rows, dout, vals, static_cast<float*>(workspace)};
  const int r = afm_bwd_dispatch(s, k, gvec, a, st);
  if (r != REC_OK) return r;
  return rec_slot_sum(REC_SLOTS_WAVE, E * A + 2 * A + 1, k.grid[1], a.slots,
                      {{dWa, dba, dhv, dbh}, {E * A, A, A, 1}}, st);
}
