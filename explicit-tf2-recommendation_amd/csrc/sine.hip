// SINE (SINELayer, 6.MIND/CustomLayers.py:966-1176) on gfx950, fp32: the sparse-interest extractor with its per-example
// top-K of L concepts, and the auxiliary loss of the concept pool.  The extractor gathers from the table itself; the
// formulas (a)-(g) are the header's.
//
// Forward: one launch, one example per workgroup at a time over a persistent grid.  The rows are gathered into LDS once;
// the 3 + K products [T, D] x [D, D] (X W1, X W3, the K products X Wk1[idx_k] and Xh W3) run on v_mfma_f32_32x32x2_f32
// through caps_project with the weight read from global memory; everything between them is wave-level work out of LDS.
// The top-K is K rounds of an arg-max by one wave over sim [L] in LDS; a candidate loses to an equal one with a lower
// index, so chosen is tf.math.top_k's: descending, lower index first.  Nothing but out and chosen leaves the kernel.
//
// Backward: per slab of the batch one example-major launch and one concept-major launch, then one slot sum.
//   example  the forward again with chosen as the forward wrote it (never re-selected), then (g) ... (a) in reverse; the
//            K + 2 projections whose activations the forward overwrote are computed again.  dX is kept in LDS over all
//            its uses and written once.  dW1 and dW3 stay in register blocks over the workgroup's examples, dW2 and dW4 in
//            LDS; the four go to the workgroup's slot (the first slab writes, later slabs add).  What is indexed by the
//            concept -- x^T dpre_k [D, D], the row of dWk2 and the row of dpool of every pair (b, k) -- goes to the
//            scratch, pair-major.  Where dW1 has more than sixteen 32 x 32 blocks the grid has a second dimension of
//            block groups: a group repeats the example and keeps its own blocks; group 0 writes everything else.
//   concept  workgroup (l, 256 elements): the pairs of the slab with chosen == l are listed in ascending (b, k) order
//            (ballot + prefix, no atomics), then one thread owns one element of dWk1[l] | dWk2[l] | dpool[l] and adds the
//            listed contributions in that order.  The first slab writes (zero where nobody chose l), later slabs add.
// One launch handles one slab, so the order of every sum is fixed: no float atomics, bit-identical run to run.
//
// aux: 0.5 sum_{i != j} M_ij^2 with M = Cc Cc^T, Cc = pool - mean_l(pool).  Forward: one workgroup, a thread per pair.
// Backward: workgroup i writes gloss 2 sum_{j != i} M_ij Cc_j, then one workgroup subtracts the column means.
#include "capsule.h"

namespace {

constexpr int SN_MAX_L = REC_SINE_MAX_L;        // concepts of the pool, at the most
constexpr int SN_AUX_MAX_D = REC_SINE_AUX_MAX_D;  // width of a pool row of the aux kernels
static_assert(sizeof(float) * (2 * SN_AUX_MAX_D + SN_MAX_L) <= 64 * 1024,
              "mean, ci and M of the aux backward are static LDS: 64 KiB at the most");
constexpr int SN_GRID = 1024;                   // workgroups (= slots) of the example-major backward, at the most
constexpr int SN_SLAB_MAX = 2048;               // examples of a slab, at the most: the concept-major list holds as many
constexpr int64_t SN_SLAB_BYTES = 64 << 20;     // and bytes of its pair-major scratch (never fewer than one example)
constexpr int SN_SMALL = 128;                   // floats of the K-sized vectors and scalars of an example

struct SnArgs : CapsSeries {
  const float *pool, *W1, *W2, *Wk1, *Wk2, *W3, *W4;
  int L;
  float tau, eps;
};

// floats of LDS of one example, both directions:
//   xs, dX and two activation buffers [T][D | 1], P, A, dP and dA [K][T], sim [L], Cu, Cn, Z, dZ and dCu [K][D | 1],
//   six [T], eight [D | 1] and SN_SMALL for what has K entries
__host__ __device__ inline size_t sn_lds_floats(int T, int D, int L, int K) {
  return 4 * (size_t)T * mi_odd(D) + 4 * (size_t)K * T + L + 5 * (size_t)K * mi_odd(D) + 6 * (size_t)T +
         8 * (size_t)mi_odd(D) + SN_SMALL;
}
static int sn_check(int64_t B, int T, int E, int C, int L, int K) {
  if (L < 1) return REC_E_ARG;
  if (int rc = caps_series_shape(B, T, E, C, 1, K, 1)) return rc;
  if (L > SN_MAX_L || K > L) return REC_E_UNSUPPORTED;
  return caps_fits(sizeof(float) * sn_lds_floats(T, E * C, L, K));
}

struct SnLds {
  float *xs, *dx, *ha, *hb;                               // [T][Dp]
  float *P, *A, *dP, *dA;                                 // [K][T]
  float* sim;                                             // [L]
  float *Cu, *Cn, *Z, *dZ, *dCu;                          // [K][Dp]
  float *a, *b, *rsY, *t1, *t2;                           // [T]
  int* valid;                                             // [T]
  float *w2, *w4, *z, *dz, *cap, *dcap, *dw2, *dw4;       // [Dp]
  int* idx;                                               // [16]
  float *g, *e, *rsC, *rsZ, *kv, *dl, *sc;                // [16] each, sc: scalars
};
__device__ __forceinline__ SnLds sn_carve(float* p, int T, int D, int L, int K) {
  const int Dp = mi_odd(D);
  SnLds f;
  auto take = [&](size_t n) { float* q = p; p += n; return q; };
  f.xs = take(T * Dp), f.dx = take(T * Dp), f.ha = take(T * Dp), f.hb = take(T * Dp);
  f.P = take(K * T), f.A = take(K * T), f.dP = take(K * T), f.dA = take(K * T);
  f.sim = take(L);
  f.Cu = take(K * Dp), f.Cn = take(K * Dp), f.Z = take(K * Dp), f.dZ = take(K * Dp), f.dCu = take(K * Dp);
  f.a = take(T), f.b = take(T), f.rsY = take(T), f.t1 = take(T), f.t2 = take(T);
  f.valid = reinterpret_cast<int*>(take(T));
  f.w2 = take(Dp), f.w4 = take(Dp), f.z = take(Dp), f.dz = take(Dp), f.cap = take(Dp), f.dcap = take(Dp);
  f.dw2 = take(Dp), f.dw4 = take(Dp);
  f.idx = reinterpret_cast<int*>(take(16));
  f.g = take(16), f.e = take(16), f.rsC = take(16), f.rsZ = take(16), f.kv = take(16), f.dl = take(16), f.sc = take(16);
  return f;
}

// ---- rows, by one wave ---------------------------------------------------------------------------------------------
// y = (r - mean) / sqrt(var + eps) over D entries (y may be r); -> 1 / sqrt(var + eps)
__device__ __forceinline__ float sn_ln_row(const float* r, float* y, int D, float eps, int lane) {
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += r[d];
  const float mean = group_sum<64>(s) / (float)D;
  float v = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float c = r[d] - mean;
    v = fmaf(c, c, v);
  }
  const float rs = 1.f / sqrtf(group_sum<64>(v) / (float)D + eps);
  for (int d = lane; d < D; d += 64) y[d] = (r[d] - mean) * rs;
  wave_sync();
  return rs;
}
// dy <- rs (dy - mean(dy) - y mean(dy y))
__device__ __forceinline__ void sn_ln_bwd_row(const float* y, float rs, float* dy, int D, int lane) {
  float s1 = 0.f, s2 = 0.f;
  for (int d = lane; d < D; d += 64) {
    s1 += dy[d];
    s2 = fmaf(dy[d], y[d], s2);
  }
  const float m1 = group_sum<64>(s1) / (float)D, m2 = group_sum<64>(s2) / (float)D;
  for (int d = lane; d < D; d += 64) dy[d] = rs * (dy[d] - m1 - y[d] * m2);
  wave_sync();
}
// v <- softmax(v) over n entries
__device__ __forceinline__ void sn_softmax_row(float* v, int n, int lane) {
  float m = -FLT_MAX;
  for (int t = lane; t < n; t += 64) m = fmaxf(m, v[t]);
  m = wave_max(m);
  float sum = 0.f;
  for (int t = lane; t < n; t += 64) {
    const float ex = expf(v[t] - m);
    v[t] = ex;
    sum += ex;
  }
  sum = group_sum<64>(sum);
  for (int t = lane; t < n; t += 64) v[t] = v[t] / sum;
  wave_sync();
}
// g <- w (g - sum_t w g): a softmax over n entries, back
__device__ __forceinline__ void sn_softmax_bwd_row(const float* w, float* g, int n, int lane) {
  float dot = 0.f;
  for (int t = lane; t < n; t += 64) dot = fmaf(w[t], g[t], dot);
  dot = group_sum<64>(dot);
  for (int t = lane; t < n; t += 64) g[t] = w[t] * (g[t] - dot);
  wave_sync();
}
// z . pool[l], in index order: the forward (every l) and the backward (the chosen ones) add alike
__device__ __forceinline__ float sn_sim(const float* z, const float* __restrict__ row, int D) {
  float acc = 0.f;
  for (int d = 0; d < D; ++d) acc = fmaf(z[d], row[d], acc);
  return acc;
}

// dx [T][Dp] (LDS) (+)= du [T][Dcp] S^T: caps_keys_grad with the rows kept in LDS, where the K + 3 products meet
template <bool ADD>
__device__ __forceinline__ void sn_keys_grad(const float* du, int Dcp, const float* __restrict__ S, int T, int D, int Dc,
                                             float* dx, int Dp, int wave, int lo, int hi) {
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
      if (row < T && nok) dx[row * Dp + n] = ADD ? dx[row * Dp + n] + acc[rr] : acc[rr];
    }
  }
}

// (a)-(g) of example b.  BWD: the concepts are chosen[b] (clamped into the pool), otherwise they are selected here and
// written to chosen[b].  Leaves in LDS: xs, valid, a, z, idx, g, Cu, Cn, rsC, rsY, P, A, Z, rsZ, Xh in hb, tanh(Xh W3) in
// ha, b, cap, sc[0] = its 1 / sqrt(var + eps), e.  out (may be NULL): the row of user_interest.
template <bool BWD>
__device__ __forceinline__ void sn_forward(const SnArgs& a, int64_t b, const SnLds& f, int32_t* __restrict__ chosen,
                                           float* __restrict__ out, int tid, bool& bad) {
  const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, K = a.K, L = a.L, Dp = mi_odd(D);
  mi_gather<MI_NTHR>(a.embed, a.ld, a.V, a.series + b * T * a.C, T, a.C, a.E, f.xs, Dp, tid, bad, a.padding_index,
                     f.valid);
  __syncthreads();
  // (a) the masked attention over the series and its pooled row z
  caps_project<true>(f.xs, Dp, a.W1, T, D, D, f.ha, Dp, wave, lo, hi);
  __syncthreads();
  for (int t = tid; t < T; t += MI_NTHR) f.a[t] = mi_dot(f.w2, f.ha + t * Dp, 1, D) + (f.valid[t] ? 0.f : -1e9f);
  __syncthreads();
  if (wave == 0) sn_softmax_row(f.a, T, lane);
  __syncthreads();
  for (int d = tid; d < D; d += MI_NTHR) f.z[d] = mi_dot(f.a, f.xs + d, Dp, T);
  __syncthreads();
  // (b) the K concepts and their gates
  if (!BWD) {
    for (int l = tid; l < L; l += MI_NTHR) f.sim[l] = sn_sim(f.z, a.pool + (int64_t)l * D, D);
    __syncthreads();
    if (wave == 0)
      for (int k = 0; k < K; ++k) {
        float bv = 0.f;
        int bi = -1;
        for (int l = lane; l < L; l += 64) {                     // ascending l: strictly greater, the lower index stays
          bool taken = false;
          for (int j = 0; j < k; ++j) taken |= f.idx[j] == l;
          const float v = f.sim[l];
          if (!taken && (bi < 0 || v > bv)) {
            bv = v;
            bi = l;
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
          }
        }
        if (lane == 0) {
          f.idx[k] = bi;
          f.kv[k] = bv;
          chosen[b * K + k] = bi;
        }
        wave_sync();
      }
  } else {
    if (tid < K) {
      const int c = chosen[b * K + tid];
      const int l = c < 0 ? 0 : (c < L ? c : L - 1);             // whatever it holds, stay inside the pool
      f.idx[tid] = l;
      f.kv[tid] = sn_sim(f.z, a.pool + (int64_t)l * D, D);
    }
  }
  __syncthreads();
  if (tid < K) f.g[tid] = sigmoid_acc(f.kv[tid]);
  __syncthreads();
  for (int i = tid; i < K * D; i += MI_NTHR) {
    const int k = i / D, d = i - k * D;
    f.Cu[k * Dp + d] = f.g[k] * a.pool[(int64_t)f.idx[k] * D + d];
  }
  __syncthreads();
  // (c) P = softmax_k(LN(X W3) . LN(Cu))
  for (int k = wave; k < K; k += 4) {
    const float rs = sn_ln_row(f.Cu + k * Dp, f.Cn + k * Dp, D, a.eps, lane);
    if (lane == 0) f.rsC[k] = rs;
  }
  caps_project<false>(f.xs, Dp, a.W3, T, D, D, f.ha, Dp, wave, lo, hi);
  __syncthreads();
  for (int t = wave; t < T; t += 4) {
    const float rs = sn_ln_row(f.ha + t * Dp, f.ha + t * Dp, D, a.eps, lane);
    if (lane == 0) f.rsY[t] = rs;
  }
  __syncthreads();
  for (int i = tid; i < K * T; i += MI_NTHR) {
    const int k = i / T, t = i - k * T;
    f.P[i] = mi_dot(f.Cn + k * Dp, f.ha + t * Dp, 1, D);
  }
  __syncthreads();
  for (int t = tid; t < T; t += MI_NTHR) {
    float m = -FLT_MAX, sum = 0.f;
    for (int k = 0; k < K; ++k) m = fmaxf(m, f.P[k * T + t]);
    for (int k = 0; k < K; ++k) {
      const float ex = expf(f.P[k * T + t] - m);
      f.P[k * T + t] = ex;
      sum += ex;
    }
    for (int k = 0; k < K; ++k) f.P[k * T + t] = f.P[k * T + t] / sum;
  }
  // (d) A[k] = softmax_t(tanh(X Wk1[idx_k]) . Wk2[idx_k]), no mask
  for (int k = 0; k < K; ++k) {
    const int l = f.idx[k];
    caps_project<true>(f.xs, Dp, a.Wk1 + (int64_t)l * D * D, T, D, D, f.ha, Dp, wave, lo, hi);
    __syncthreads();
    const float* __restrict__ wk2 = a.Wk2 + (int64_t)l * D;
    for (int t = tid; t < T; t += MI_NTHR) {
      float acc = 0.f;
      for (int d = 0; d < D; ++d) acc = fmaf(f.ha[t * Dp + d], wk2[d], acc);
      f.A[k * T + t] = acc;
    }
    __syncthreads();                                             // the next k overwrites ha
  }
  for (int k = wave; k < K; k += 4) sn_softmax_row(f.A + k * T, T, lane);
  __syncthreads();
  // (e) Z_k = LN(sum_t P[t,k] A[k,t] x_t)
  for (int i = tid; i < K * T; i += MI_NTHR) f.dA[i] = f.P[i] * f.A[i];
  __syncthreads();
  for (int i = tid; i < K * D; i += MI_NTHR) {
    const int k = i / D, d = i - k * D;
    f.Z[k * Dp + d] = mi_dot(f.dA + k * T, f.xs + d, Dp, T);
  }
  // (f) Xh = P Cu, b = softmax_t(tanh(Xh W3) . W4), cap = LN(sum_t b_t Xh_t)
  for (int i = tid; i < T * D; i += MI_NTHR) {
    const int t = i / D, d = i - t * D;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(f.P[k * T + t], f.Cu[k * Dp + d], acc);
    f.hb[t * Dp + d] = acc;
  }
  __syncthreads();
  for (int k = wave; k < K; k += 4) {
    const float rs = sn_ln_row(f.Z + k * Dp, f.Z + k * Dp, D, a.eps, lane);
    if (lane == 0) f.rsZ[k] = rs;
  }
  caps_project<true>(f.hb, Dp, a.W3, T, D, D, f.ha, Dp, wave, lo, hi);
  __syncthreads();
  for (int t = tid; t < T; t += MI_NTHR) f.b[t] = mi_dot(f.w4, f.ha + t * Dp, 1, D);
  __syncthreads();
  if (wave == 0) sn_softmax_row(f.b, T, lane);
  __syncthreads();
  for (int d = tid; d < D; d += MI_NTHR) f.cap[d] = mi_dot(f.b, f.hb + d, Dp, T);
  __syncthreads();
  // (g) e = softmax_k(cap . Z_k / tau)
  if (wave == 0) {
    const float rs = sn_ln_row(f.cap, f.cap, D, a.eps, lane);
    if (lane == 0) f.sc[0] = rs;
    if (lane < K) f.kv[lane] = mi_dot(f.cap, f.Z + lane * Dp, 1, D) / a.tau;
    wave_sync();
    if (lane < K) {
      float m = -FLT_MAX, sum = 0.f;
      for (int k = 0; k < K; ++k) m = fmaxf(m, f.kv[k]);
      for (int k = 0; k < K; ++k) sum += expf(f.kv[k] - m);
      f.e[lane] = expf(f.kv[lane] - m) / sum;
    }
  }
  __syncthreads();
  if (out)
    for (int d = tid; d < D; d += MI_NTHR) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(f.e[k], f.Z[k * Dp + d], acc);
      out[b * D + d] = acc;
    }
}

__device__ __forceinline__ void sn_load_vectors(const SnArgs& a, const SnLds& f, int tid) {
  for (int d = tid; d < a.D; d += MI_NTHR) {
    f.w2[d] = a.W2[d];
    f.w4[d] = a.W4[d];
  }
}

__global__ __launch_bounds__(MI_NTHR) void sine_fwd_kernel(SnArgs a, float* __restrict__ out, int32_t* __restrict__ chosen,
                                                           int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const SnLds f = sn_carve(lds, a.T, a.D, a.L, a.K);
  bool bad = false;
  sn_load_vectors(a, f, threadIdx.x);
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();                                             // the previous example has been read
    sn_forward<false>(a, b, f, chosen, out, threadIdx.x, bad);
  }
  if (bad && oob) *oob = 1;
}

// The examples [s0, s0 + ns) of a slab.  NB: 32 x 32 blocks of dW1 (and of dW3, and of one x^T dpre_k) per wave; grid
// (workgroups, block groups).  slots [gridDim.x][D D | D | D D | D]: dW1, dW2, dW3, dW4 of the workgroup.  pairs
// [ns K][D D | D | D]: x^T dpre_k, the row of dWk2 and the row of dpool of pair (b - s0, k).
template <int NB>
__global__ __launch_bounds__(MI_NTHR) void sine_bwd_kernel(SnArgs a, int64_t s0, int ns, const int32_t* __restrict__ chosen,
                                                           const float* __restrict__ gout, float* __restrict__ gkeys,
                                                           float* __restrict__ slots, float* __restrict__ pairs,
                                                           int first) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, K = a.K, Dp = mi_odd(D);
  const int blk0 = blockIdx.y * 4 * NB;
  const bool lead = blockIdx.y == 0;                             // the group that writes what is not a block of [D, D]
  const SnLds f = sn_carve(lds, T, D, a.L, K);
  const size_t pair_floats = (size_t)D * D + 2 * (size_t)D;
  f32x16 acc1[NB], acc3[NB], acck[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    mb_zero(acc1[j]);
    mb_zero(acc3[j]);
  }
  bool bad = false;
  sn_load_vectors(a, f, tid);
  for (int d = tid; d < D; d += MI_NTHR) f.dw2[d] = f.dw4[d] = 0.f;

  for (int64_t b = s0 + blockIdx.x; b < s0 + ns; b += gridDim.x) {
    __syncthreads();                                             // the previous example has been read
    sn_forward<true>(a, b, f, const_cast<int32_t*>(chosen), nullptr, tid, bad);
    float* __restrict__ pair0 = pairs + (size_t)(b - s0) * K * pair_floats;
    float* go = f.dz;                                            // the row of gout, until (b) needs dz
    // (g), back
    for (int d = tid; d < D; d += MI_NTHR) go[d] = gout[b * D + d];
    __syncthreads();
    if (tid < K) f.kv[tid] = mi_dot(go, f.Z + tid * Dp, 1, D);
    __syncthreads();
    if (tid < K) {
      float dot = 0.f;
      for (int k = 0; k < K; ++k) dot = fmaf(f.e[k], f.kv[k], dot);
      f.dl[tid] = f.e[tid] * (f.kv[tid] - dot) / a.tau;
    }
    __syncthreads();
    for (int d = tid; d < D; d += MI_NTHR) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(f.dl[k], f.Z[k * Dp + d], acc);
      f.dcap[d] = acc;
    }
    for (int i = tid; i < K * D; i += MI_NTHR) {
      const int k = i / D, d = i - k * D;
      f.dZ[k * Dp + d] = fmaf(f.e[k], go[d], f.dl[k] * f.cap[d]);
    }
    __syncthreads();
    // (f), back: the LayerNorms of cap and of Z, the attention b, tanh(Xh W3)
    if (wave == 0) sn_ln_bwd_row(f.cap, f.sc[0], f.dcap, D, lane);
    for (int k = wave; k < K; k += 4) sn_ln_bwd_row(f.Z + k * Dp, f.rsZ[k], f.dZ + k * Dp, D, lane);
    __syncthreads();
    for (int t = tid; t < T; t += MI_NTHR) f.t1[t] = mi_dot(f.dcap, f.hb + t * Dp, 1, D);
    __syncthreads();
    if (wave == 0) sn_softmax_bwd_row(f.b, f.t1, T, lane);
    __syncthreads();
    for (int d = tid; d < D; d += MI_NTHR) f.dw4[d] = f.dw4[d] + mi_dot(f.t1, f.ha + d, Dp, T);
    __syncthreads();
    for (int i = tid; i < T * D; i += MI_NTHR) {
      const int t = i / D, d = i - t * D;
      const float h = f.ha[t * Dp + d];
      f.ha[t * Dp + d] = f.t1[t] * f.w4[d] * (1.f - h * h);
    }
    __syncthreads();
    caps_weight_grad<NB>(acc3, f.hb, Dp, f.ha, Dp, T, D, D, wave, lo, hi, blk0);     // dW3 += Xh^T dpre
    __syncthreads();
    sn_keys_grad<false>(f.ha, Dp, a.W3, T, D, D, f.hb, Dp, wave, lo, hi);            // dXh = dpre W3^T ...
    __syncthreads();
    for (int i = tid; i < T * D; i += MI_NTHR) {
      const int t = i / D, d = i - t * D;
      f.hb[t * Dp + d] = fmaf(f.b[t], f.dcap[d], f.hb[t * Dp + d]);                 // ... + b_t dcap
    }
    __syncthreads();
    for (int i = tid; i < K * T; i += MI_NTHR) {
      const int k = i / T, t = i - k * T;
      f.dP[i] = mi_dot(f.Cu + k * Dp, f.hb + t * Dp, 1, D);
    }
    for (int i = tid; i < K * D; i += MI_NTHR) {
      const int k = i / D, d = i - k * D;
      f.dCu[k * Dp + d] = mi_dot(f.P + k * T, f.hb + d, Dp, T);
    }
    // (e), back: dZ holds the gradient of the sums before their LayerNorm
    for (int i = tid; i < K * T; i += MI_NTHR) {
      const int k = i / T, t = i - k * T;
      const float dw = mi_dot(f.dZ + k * Dp, f.xs + t * Dp, 1, D);
      f.dP[i] = fmaf(f.A[i], dw, f.dP[i]);
      f.dA[i] = f.P[i] * dw;
    }
    for (int i = tid; i < T * D; i += MI_NTHR) {
      const int t = i / D, d = i - t * D;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(f.P[k * T + t] * f.A[k * T + t], f.dZ[k * Dp + d], acc);
      f.dx[t * Dp + d] = acc;
    }
    __syncthreads();
    // (d), back: dA <- dq, then concept by concept
    for (int k = wave; k < K; k += 4) sn_softmax_bwd_row(f.A + k * T, f.dA + k * T, T, lane);
    __syncthreads();
    for (int k = 0; k < K; ++k) {
      const int l = f.idx[k];
      const float* __restrict__ wk1 = a.Wk1 + (int64_t)l * D * D;
      const float* __restrict__ wk2 = a.Wk2 + (int64_t)l * D;
      float* __restrict__ pr = pair0 + (size_t)k * pair_floats;
      caps_project<true>(f.xs, Dp, wk1, T, D, D, f.ha, Dp, wave, lo, hi);
      __syncthreads();
      if (lead)
        for (int d = tid; d < D; d += MI_NTHR) pr[(size_t)D * D + d] = mi_dot(f.dA + k * T, f.ha + d, Dp, T);
      __syncthreads();
      for (int i = tid; i < T * D; i += MI_NTHR) {
        const int t = i / D, d = i - t * D;
        const float h = f.ha[t * Dp + d];
        f.ha[t * Dp + d] = f.dA[k * T + t] * wk2[d] * (1.f - h * h);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NB; ++j) mb_zero(acck[j]);
      caps_weight_grad<NB>(acck, f.xs, Dp, f.ha, Dp, T, D, D, wave, lo, hi, blk0);   // x^T dpre_k of this pair
      caps_weight_store<NB>(acck, pr, D, D, wave, lo, hi, blk0);
      sn_keys_grad<true>(f.ha, Dp, wk1, T, D, D, f.dx, Dp, wave, lo, hi);            // dX += dpre_k Wk1[l]^T
      __syncthreads();
    }
    // (c), back: dP <- dS, LN(X W3) again
    for (int t = tid; t < T; t += MI_NTHR) {
      float dot = 0.f;
      for (int k = 0; k < K; ++k) dot = fmaf(f.P[k * T + t], f.dP[k * T + t], dot);
      for (int k = 0; k < K; ++k) f.dP[k * T + t] = f.P[k * T + t] * (f.dP[k * T + t] - dot);
    }
    caps_project<false>(f.xs, Dp, a.W3, T, D, D, f.ha, Dp, wave, lo, hi);
    __syncthreads();
    for (int t = wave; t < T; t += 4) sn_ln_row(f.ha + t * Dp, f.ha + t * Dp, D, a.eps, lane);
    __syncthreads();
    for (int i = tid; i < K * D; i += MI_NTHR) {                 // dCn, into dZ
      const int k = i / D, d = i - k * D;
      f.dZ[k * Dp + d] = mi_dot(f.dP + k * T, f.ha + d, Dp, T);
    }
    for (int i = tid; i < T * D; i += MI_NTHR) {                 // dYn, into hb
      const int t = i / D, d = i - t * D;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(f.dP[k * T + t], f.Cn[k * Dp + d], acc);
      f.hb[t * Dp + d] = acc;
    }
    __syncthreads();
    for (int t = wave; t < T; t += 4) sn_ln_bwd_row(f.ha + t * Dp, f.rsY[t], f.hb + t * Dp, D, lane);
    for (int k = wave; k < K; k += 4) {
      sn_ln_bwd_row(f.Cn + k * Dp, f.rsC[k], f.dZ + k * Dp, D, lane);
      for (int d = lane; d < D; d += 64) f.dCu[k * Dp + d] = f.dCu[k * Dp + d] + f.dZ[k * Dp + d];
    }
    __syncthreads();
    caps_weight_grad<NB>(acc3, f.xs, Dp, f.hb, Dp, T, D, D, wave, lo, hi, blk0);     // dW3 += X^T dY
    sn_keys_grad<true>(f.hb, Dp, a.W3, T, D, D, f.dx, Dp, wave, lo, hi);             // dX += dY W3^T
    // (b), back: the gates, the pool rows and z
    for (int k = wave; k < K; k += 4) {
      const float* __restrict__ row = a.pool + (int64_t)f.idx[k] * D;
      float v = 0.f;
      for (int d = lane; d < D; d += 64) v = fmaf(f.dCu[k * Dp + d], row[d], v);
      v = group_sum<64>(v);
      if (lane == 0) f.kv[k] = v * f.g[k] * (1.f - f.g[k]);       // dsim_k
    }
    __syncthreads();
    if (lead)
      for (int i = tid; i < K * D; i += MI_NTHR) {
        const int k = i / D, d = i - k * D;
        pair0[(size_t)k * pair_floats + (size_t)D * D + D + d] = fmaf(f.g[k], f.dCu[k * Dp + d], f.kv[k] * f.z[d]);
      }
    for (int d = tid; d < D; d += MI_NTHR) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(f.kv[k], a.pool[(int64_t)f.idx[k] * D + d], acc);
      f.dz[d] = acc;
    }
    // (a), back
    caps_project<true>(f.xs, Dp, a.W1, T, D, D, f.ha, Dp, wave, lo, hi);
    __syncthreads();
    for (int t = tid; t < T; t += MI_NTHR) f.t1[t] = mi_dot(f.dz, f.xs + t * Dp, 1, D);
    __syncthreads();
    if (wave == 0) sn_softmax_bwd_row(f.a, f.t1, T, lane);
    __syncthreads();
    for (int d = tid; d < D; d += MI_NTHR) f.dw2[d] = f.dw2[d] + mi_dot(f.t1, f.ha + d, Dp, T);
    __syncthreads();
    for (int i = tid; i < T * D; i += MI_NTHR) {
      const int t = i / D, d = i - t * D;
      const float h = f.ha[t * Dp + d];
      f.ha[t * Dp + d] = f.t1[t] * f.w2[d] * (1.f - h * h);
      f.dx[t * Dp + d] = fmaf(f.a[t], f.dz[d], f.dx[t * Dp + d]);
    }
    __syncthreads();
    caps_weight_grad<NB>(acc1, f.xs, Dp, f.ha, Dp, T, D, D, wave, lo, hi, blk0);     // dW1 += X^T dpre
    sn_keys_grad<true>(f.ha, Dp, a.W1, T, D, D, f.dx, Dp, wave, lo, hi);             // dX += dpre W1^T
    __syncthreads();
    if (lead)
      for (int i = tid; i < T * D; i += MI_NTHR) {
        const int t = i / D, d = i - t * D;
        gkeys[b * T * D + i] = f.dx[t * Dp + d];
      }
  }

  float* __restrict__ slot = slots + (size_t)blockIdx.x * (2 * (size_t)D * D + 2 * (size_t)D);
  caps_weight_store<NB>(acc1, slot, D, D, wave, lo, hi, blk0, !first);
  caps_weight_store<NB>(acc3, slot + (size_t)D * D + D, D, D, wave, lo, hi, blk0, !first);
  if (lead)
    for (int d = tid; d < D; d += MI_NTHR) {
      float* q2 = slot + (size_t)D * D + d;
      float* q4 = slot + 2 * (size_t)D * D + D + d;
      *q2 = first ? f.dw2[d] : *q2 + f.dw2[d];
      *q4 = first ? f.dw4[d] : *q4 + f.dw4[d];
    }
}

// Workgroup (l, y): element y 256 + tid of dWk1[l] | dWk2[l] | dpool[l] (+)= the sum over the pairs of the slab with
// chosen == l, in ascending pair order.  chosen: the slab's [np]; pairs [np][D D | D | D].
__global__ __launch_bounds__(MI_NTHR) void sine_concept_kernel(const int32_t* __restrict__ chosen, int np, int L, int D,
                                                               const float* __restrict__ pairs, float* __restrict__ dWk1,
                                                               float* __restrict__ dWk2, float* __restrict__ dpool,
                                                               int first) {
  __shared__ int list[SN_SLAB_MAX];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = blockIdx.x;
  int n = 0;
  for (int base = 0; base < np; base += MI_NTHR) {
    const int i = base + tid;
    bool hit = false;
    if (i < np) {
      const int c = chosen[i];
      hit = (c < 0 ? 0 : (c < L ? c : L - 1)) == l;              // clamped as the example-major kernel reads it
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int at = n;
    for (int w = 0; w < wave; ++w) at += wcnt[w];
    at += __popcll(m & ((1ull << lane) - 1ull));
    if (hit && at < SN_SLAB_MAX) list[at] = i;                   // an example lists a concept once: at most ns <= the cap
    n += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  if (n > SN_SLAB_MAX) n = SN_SLAB_MAX;
  const int DD = D * D, per = DD + 2 * D;
  const int el = blockIdx.y * MI_NTHR + tid;
  if (el >= per) return;
  float acc = 0.f;
  for (int j = 0; j < n; ++j) acc += pairs[(size_t)list[j] * per + el];
  float* __restrict__ q = el < DD ? dWk1 + (size_t)l * DD + el
                                  : (el < DD + D ? dWk2 + (size_t)l * D + (el - DD) : dpool + (size_t)l * D + (el - DD - D));
  *q = first ? acc : *q + acc;
}

// ---- aux ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void aux_mean(const float* __restrict__ pool, int L, int D, float* mean, int tid) {
  for (int d = tid; d < D; d += MI_NTHR) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += pool[(size_t)l * D + d];
    mean[d] = s / (float)L;
  }
  __syncthreads();
}

__global__ __launch_bounds__(MI_NTHR) void sine_aux_fwd_kernel(const float* __restrict__ pool, int L, int D,
                                                               float* __restrict__ loss) {
  __shared__ float mean[SN_AUX_MAX_D];
  __shared__ float part[MI_NTHR];
  const int tid = threadIdx.x;
  aux_mean(pool, L, D, mean, tid);
  float acc = 0.f;
  for (int p = tid; p < L * L; p += MI_NTHR) {
    const int i = p / L, j = p - i * L;
    if (i == j) continue;
    const float* __restrict__ ri = pool + (size_t)i * D;
    const float* __restrict__ rj = pool + (size_t)j * D;
    float m = 0.f;
    for (int d = 0; d < D; ++d) m = fmaf(ri[d] - mean[d], rj[d] - mean[d], m);
    acc = fmaf(m, m, acc);
  }
  part[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int i = 0; i < MI_NTHR; ++i) s += part[i];
    loss[0] = 0.5f * s;
  }
}

// row i of dpool = gloss 2 sum_{j != i} M_ij Cc_j, before the centring
__global__ __launch_bounds__(MI_NTHR) void sine_aux_bwd_kernel(const float* __restrict__ pool, int L, int D,
                                                               const float* __restrict__ gloss, float* __restrict__ dpool) {
  __shared__ float mean[SN_AUX_MAX_D];
  __shared__ float ci[SN_AUX_MAX_D];
  __shared__ float M[SN_MAX_L];
  const int tid = threadIdx.x, i = blockIdx.x;
  aux_mean(pool, L, D, mean, tid);
  for (int d = tid; d < D; d += MI_NTHR) ci[d] = pool[(size_t)i * D + d] - mean[d];
  __syncthreads();
  for (int j = tid; j < L; j += MI_NTHR) {
    const float* __restrict__ rj = pool + (size_t)j * D;
    float m = 0.f;
    for (int d = 0; d < D; ++d) m = fmaf(ci[d], rj[d] - mean[d], m);
    M[j] = j == i ? 0.f : m;
  }
  __syncthreads();
  const float g2 = 2.f * gloss[0];
  for (int d = tid; d < D; d += MI_NTHR) {
    float acc = 0.f;
    for (int j = 0; j < L; ++j) acc = fmaf(M[j], pool[(size_t)j * D + d] - mean[d], acc);
    dpool[(size_t)i * D + d] = g2 * acc;
  }
}
// dpool <- dpool - mean_l(dpool): the centring, back
__global__ __launch_bounds__(MI_NTHR) void sine_aux_centre_kernel(int L, int D, float* __restrict__ dpool) {
  for (int d = threadIdx.x; d < D; d += MI_NTHR) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += dpool[(size_t)l * D + d];
    const float m = s / (float)L;
    for (int l = 0; l < L; ++l) dpool[(size_t)l * D + d] = dpool[(size_t)l * D + d] - m;
  }
}

// ---- the host side -------------------------------------------------------------------------------------------------------
// 32 x 32 blocks of a [D, D] gradient per wave (1 or 4) and the block groups that cover it
static int sn_nb(int D) { return ((D + 31) / 32) * ((D + 31) / 32) <= 4 ? 1 : 4; }
static int sn_groups(int D) {
  const int nblk = ((D + 31) / 32) * ((D + 31) / 32), per = 4 * sn_nb(D);
  return (nblk + per - 1) / per;
}
// examples of a slab, workgroups of its launch, floats of the pair-major scratch and of the slots
struct SnPlan {
  int slab, grid;
  size_t pair_floats, slot_floats;
};
static SnPlan sn_plan(int64_t B, int D, int K) {
  const int64_t one = (int64_t)K * ((int64_t)D * D + 2 * D);
  int64_t n = SN_SLAB_BYTES / (int64_t)sizeof(float) / one;
  n = n < 1 ? 1 : (n > SN_SLAB_MAX ? SN_SLAB_MAX : n);
  if (B < n) n = B;
  const int cap = sn_nb(D) == 1 ? SN_GRID : SN_GRID / 4;
  const int grid = n < cap ? (int)n : cap;
  return {(int)n, grid, (size_t)(n * one), (size_t)grid * (2 * (size_t)D * D + 2 * (size_t)D)};
}
static int sn_common(int64_t B, int T, int E, int C, int L, int K, float tau, float ln_eps) {
  if (!(tau > 0.f) || !(ln_eps > 0.f)) return REC_E_ARG;           // with the sizes below 1: the same code
  return sn_check(B, T, E, C, L, K);
}

}  // namespace

extern "C" size_t rec_sine_lds_bytes(int T, int E, int C, int L, int K) {
  return sn_check(0, T, E, C, L, K) == REC_OK ? sizeof(float) * sn_lds_floats(T, E * C, L, K) : 0;
}

extern "C" size_t rec_sine_scratch_bytes(int64_t B, int T, int E, int C, int L, int K) {
  if (sn_check(B, T, E, C, L, K) != REC_OK) return 0;
  const SnPlan p = sn_plan(B, E * C, K);
  return sizeof(float) * (p.pair_floats + p.slot_floats + 4);
}

extern "C" int rec_sine_interest_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                         int64_t B, int T, const float* pool, const float* W1, const float* W2,
                                         const float* Wk1, const float* Wk2, const float* W3, const float* W4, int L, int K,
                                         float tau, float ln_eps, int64_t padding_index, float* out, int32_t* chosen,
                                         int* oob_flag, void* stream) {
  if (int rc = sn_common(B, T, E, C, L, K, tau, ln_eps)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !pool || !W1 || !W2 || !Wk1 || !Wk2 || !W3 || !W4 || !out || !chosen)
    return REC_E_ARG;
  if (B == 0) return REC_OK;
  const int D = E * C;
  const SnArgs a{{embed, ld, V, series, B, padding_index, T, C, E, D, D, K}, pool, W1, W2, Wk1, Wk2, W3, W4, L, tau, ln_eps};
  return caps_launch<sine_fwd_kernel>(dim3(caps_fwd_grid(B)), MI_NTHR, sizeof(float) * sn_lds_floats(T, D, L, K),
                                      as_stream(stream), a, out, chosen, oob_flag);
}

extern "C" int rec_sine_interest_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                         int64_t B, int T, const float* pool, const float* W1, const float* W2,
                                         const float* Wk1, const float* Wk2, const float* W3, const float* W4, int L, int K,
                                         float tau, float ln_eps, int64_t padding_index, const int32_t* chosen,
                                         const float* gout, float* gkeys, float* dpool, float* dW1, float* dW2, float* dWk1,
                                         float* dWk2, float* dW3, float* dW4, void* scratch, size_t scratch_bytes,
                                         void* stream) {
  if (int rc = sn_common(B, T, E, C, L, K, tau, ln_eps)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !pool || !W1 || !W2 || !Wk1 || !Wk2 || !W3 || !W4 || !chosen || !gout ||
      !gkeys || !dpool || !dW1 || !dW2 || !dWk1 || !dWk2 || !dW3 || !dW4 || !scratch)
    return REC_E_ARG;
  const int D = E * C;
  const SnPlan p = sn_plan(B, D, K);
  if (scratch_bytes < sizeof(float) * (p.pair_floats + p.slot_floats)) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;                                     // nothing is launched and nothing written
  hipStream_t st = as_stream(stream);
  const SnArgs a{{embed, ld, V, series, B, padding_index, T, C, E, D, D, K}, pool, W1, W2, Wk1, Wk2, W3, W4, L, tau, ln_eps};
  const size_t lds = sizeof(float) * sn_lds_floats(T, D, L, K);
  float* pairs = static_cast<float*>(scratch);
  float* slots = pairs + p.pair_floats;
  const int per = D * D + 2 * D;
  for (int64_t s0 = 0; s0 < B; s0 += p.slab) {
    const int ns = (int)(B - s0 < p.slab ? B - s0 : p.slab), first = s0 == 0;
    const dim3 grid(ns < p.grid ? ns : p.grid, sn_groups(D));
    const int rc = sn_nb(D) == 1 ? caps_launch<sine_bwd_kernel<1>>(grid, MI_NTHR, lds, st, a, s0, ns, chosen, gout, gkeys,
                                                                   slots, pairs, first)
                                 : caps_launch<sine_bwd_kernel<4>>(grid, MI_NTHR, lds, st, a, s0, ns, chosen, gout, gkeys,
                                                                   slots, pairs, first);
    if (rc) return rc;
    hipLaunchKernelGGL(sine_concept_kernel, dim3(L, (per + MI_NTHR - 1) / MI_NTHR), dim3(MI_NTHR), 0, st, chosen + s0 * K,
                       ns * K, L, D, pairs, dWk1, dWk2, dpool, first);
    REC_LAUNCH_CHECK();
  }
  return rec_slot_sum(REC_SLOTS_WAVE, 2 * D * D + 2 * D, p.grid, slots, {{dW1, dW2, dW3, dW4}, {D * D, D, D * D, D}}, st);
}

extern "C" int rec_sine_aux_fwd_f32(const float* pool, int L, int D, float* loss, void* stream) {
  if (L < 1 || D < 1) return REC_E_ARG;
  if (L > SN_MAX_L || D > SN_AUX_MAX_D) return REC_E_UNSUPPORTED;
  if (!pool || !loss) return REC_E_ARG;
  hipLaunchKernelGGL(sine_aux_fwd_kernel, dim3(1), dim3(MI_NTHR), 0, as_stream(stream), pool, L, D, loss);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_sine_aux_bwd_f32(const float* pool, int L, int D, const float* gloss, float* dpool, void* stream) {
  if (L < 1 || D < 1) return REC_E_ARG;
  if (L > SN_MAX_L || D > SN_AUX_MAX_D) return REC_E_UNSUPPORTED;
  if (!pool || !gloss || !dpool) return REC_E_ARG;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(sine_aux_bwd_kernel, dim3(L), dim3(MI_NTHR), 0, st, pool, L, D, gloss, dpool);
  REC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sine_aux_centre_kernel, dim3(1), dim3(MI_NTHR), 0, st, L, D, dpool);
  REC_LAUNCH_CHECK();
  return REC_OK;
}
