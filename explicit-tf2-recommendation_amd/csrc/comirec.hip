// ComiRec (ComiRecDynamicRoutingLayer, ComiRecSelfAttentiveLayer and ComiRecLayer.manually_negative_sampled_call,
// 6.MIND/CustomLayers.py:528-810) on gfx950, fp32: dynamic routing with unshared weights, the self-attentive extractor,
// and hard attention with the sampled-softmax loss.  All three gather from the table themselves; a position t of example
// b takes part iff (series[b,t,0] == padding_index) == (keep_padding != 0).
//
// (a) Dynamic routing.  W [K, T, D, Dc] has one matrix per capsule and position, so the projection u[b,k,t,:] =
// x[b,t,:] W[k,t] is K T small GEMMs whose long side is the batch.  The batch is cut into slabs (at most 2048 examples and
// at most 64 MiB of u) and a slab goes through, forward:
//   project   workgroup (32-example tile, t): the tile's rows of position t gathered k-major into LDS ([D][33]), then for
//             every k the [32, D] x [D, Dc] product on v_mfma_f32_32x32x2_f32 with W[k,t] read from global memory, once
//             per tile; u goes to the workspace [slab, K, T, Dc].
//   route     one WAVE owns a row (b, k): routing is independent per capsule, so the wave loads its u [T, Dc] into LDS
//             and runs the R rounds with nothing but wave-level ordering (the row steps of capsule.h).
// and backward: project again, then
//   route     the rounds again keeping the weights of every round, then from the last round to the first ds_r, c_r and
//             the logit gradient dL_r that enters the round (zero for the last); du[t,:] = sum_r C_r[t] ds_r +
//             dL_r[t] c_r is formed once at the end and written over u.
//   keys      workgroup (tile, t): for every k the tile of du k-major into LDS ([Dc][33]) and acc += du W[k,t]^T, W read
//             once per tile; gkeys[b,t,:] is written once, after the last k.
//   weight    workgroup ((k,t), batch slice, block group): x_t and du tiles example-major in LDS, x_t^T du on the MFMA
//             into register blocks over the tiles of the slice; the partial goes to slot [slice][k,t] (the first slab
//             writes, later slabs add: one workgroup per element and launch, so the order is fixed).
// and after the last slab rec_slot_sum adds the slices in serial order into dW.  The number of slices is mb_split's.
//
// (b) Self-attentive extractor: one example per workgroup as the MIND routing, h = tanh((x + pos) W1) on the MFMA into
// LDS, a wave per head k for the scores h W2[k], the masked softmax and the weighted sum of h.  Backward: recompute, then
//   dA[k,t] = gout_k . h_t   dsc = part ? A (dA - sum_t A dA) : 0   dh_t = sum_k A[k,t] gout_k + dsc[k,t] W2[k]
//   dW2[k] += sum_t dsc[k,t] h_t (kept in LDS over the workgroup's examples)   dz = dh (1 - h^2)
//   gkeys[b] = dz W1^T   dW1 += (x + pos)^T dz (in registers over the workgroup's examples)
// dW1 | dW2 go to the workgroup's slot of a capped grid and rec_slot_sum adds them in wave order.
//
// (c) Hard attention + loss: one wave per example as the MIND attention.  p[k,s] = m_k . x_s, chosen[s] the smallest k
// that attains the maximum, inner[s] that maximum, loss = logsumexp_s(inner) - inner[0].  The backward reads chosen,
// never recomputes the argmax, and recomputes inner from the chosen capsule:
//   g[s] = ginner[s] + gloss (softmax_s(inner)[s] - [s == 0])
//   gm_k = sum_{s: chosen[s] == k} (g[s] x_s + gsel[s])   gitems_s = g[s] m_chosen[s]
// No family uses a float atomic or scratch; every launch only enqueues.
#include "capsule.h"

namespace {

constexpr int CR_GRID = 1024;                   // workgroups (= partials) of the self-attentive backward, at the most
constexpr int CR_SLAB_MAX = 2048;               // examples of a slab of the dynamic routing, at the most
constexpr int64_t CR_SLAB_BYTES = 64 << 20;     // and bytes of its u [slab, K, T, Dc] (never fewer than 32 examples)

// ---- (a) dynamic routing -------------------------------------------------------------------------------------------
struct DrArgs : CapsSeries {
  const float *W, *B0;
  int keep, R;
};

// floats of LDS of one row (b, k) of the routing backward, which is what both directions are held to:
//   u [T][Dc | 1], C and dL of every round [2 R][T], L / dL, dW and part [3][T], ds and c of every round [2 R][Dc | 1]
__host__ __device__ inline size_t dr_row_floats(int T, int Dc, int R) {
  return (size_t)T * mi_odd(Dc) + (size_t)(2 * R + 3) * T + 2 * (size_t)R * mi_odd(Dc);
}
// rows (= waves) of a workgroup: 4, 2 or 1, as many as fit; 0: not even one
static int dr_waves(int T, int Dc, int R) { return caps_waves(sizeof(float) * dr_row_floats(T, Dc, R)); }
static int dr_check(int64_t B, int T, int E, int C, int Dc, int K, int R) {
  const int rc = caps_series_shape(B, T, E, C, Dc, K, R);
  return rc ? rc : caps_fits(sizeof(float) * dr_row_floats(T, Dc, R));
}
// examples of a slab, slices of the weight gradient, floats of u and of the slots
struct DrPlan {
  int slab, slices;
  size_t u_floats, slot_floats;
};
static DrPlan dr_plan(int64_t B, int T, int D, int Dc, int K) {
  const int64_t row = (int64_t)K * T * Dc;
  int64_t n = CR_SLAB_BYTES / (int64_t)sizeof(float) / row / MB_T * MB_T;
  n = n < MB_T ? MB_T : (n > CR_SLAB_MAX ? CR_SLAB_MAX : n);
  if (B < n) n = B;
  const int s = mb_split(n, D, Dc);
  return {(int)n, s, (size_t)(n * row), (size_t)s * row * D};
}
// 32 x 32 blocks of dW[k,t] per wave (1 or 4) and the block groups that cover it
static int dr_weight_nb(int D, int Dc) { return ((D + 31) / 32) * ((Dc + 31) / 32) <= 4 ? 1 : 4; }
static int dr_weight_groups(int D, int Dc) {
  const int nblk = ((D + 31) / 32) * ((Dc + 31) / 32), per = 4 * dr_weight_nb(D, Dc);
  return (nblk + per - 1) / per;
}

// x[e][d] = row d of position t of example b0 + e for e < 32, at xs[e se + d sd]; examples from bend on are zero rows.
// As mi_gather: ids first, then values, no branch between them.
__device__ __forceinline__ void cr_gather_tile(const DrArgs& a, int64_t b0, int64_t bend, int t, float* xs, int se, int sd,
                                               int tid, bool& bad) {
  constexpr int U = 4;
  const int D = a.D, E = a.E, n = MB_T * D;
  for (int i0 = tid; i0 < n; i0 += MI_NTHR * U) {
    int64_t id[U];
    int at[U], ec[U];
    bool live[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int i = i0 + j * MI_NTHR, ic = i < n ? i : n - 1;
      const int e = ic / D, d = ic - e * D, r = d / E;
      ec[j] = d - r * E;
      at[j] = e * se + d * sd;
      live[j] = b0 + e < bend;
      id[j] = live[j] ? a.series[((b0 + e) * a.T + t) * a.C + r] : 0;
    }
    float v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const bool ok = id[j] >= 0 && id[j] < a.V;
      const float x = a.embed[(ok ? id[j] : 0) * a.ld + ec[j]];
      v[j] = (ok && live[j]) ? x : 0.f;
      bad |= !ok;
    }
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (i0 + j * MI_NTHR < n) xs[at[j]] = v[j];
  }
}

// u[b - s0, k, t, :] = x[b, t, :] W[k, t] for the examples [s0, s0 + ns) of a slab; grid (tiles, T)
__global__ __launch_bounds__(MI_NTHR) void comirec_dr_project_kernel(DrArgs a, int64_t s0, int ns, float* __restrict__ u,
                                                                     int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, Dc = a.Dc, K = a.K, t = blockIdx.y;
  const int64_t b0 = s0 + (int64_t)blockIdx.x * MB_T, bend = s0 + ns;
  float* xs = lds;                                               // [even(D)][33]
  bool bad = false;
  if ((D & 1) && tid < MB_LD) xs[D * MB_LD + tid] = 0.f;
  cr_gather_tile(a, b0, bend, t, xs, 1, MB_LD, tid, bad);
  __syncthreads();
  const int ncb = (Dc + 31) / 32;
  for (int task = wave; task < K * ncb; task += 4) {
    const int k = task / ncb, cb = task - k * ncb, n = cb * 32 + lo;
    f32x16 acc;
    mb_zero(acc);
    mb_mma1<false>(acc, xs, D, a.W + ((int64_t)k * T + t) * D * Dc, Dc, 0, Dc, cb * 32, lo, hi);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t b = b0 + mb_row(r, hi);
      if (b < bend && n < Dc) u[(((b - s0) * K + k) * T + t) * Dc + n] = acc[r];
    }
  }
  if (bad && oob) *oob = 1;
}

// One wave per row (b, k) of the slab; blockDim.x / 64 rows per workgroup and no workgroup-level barrier: a wave past the
// rows leaves.  ws [ns, K, T, Dc]: u coming in; BWD: du going out.
template <bool BWD>
__global__ __launch_bounds__(MI_NTHR) void comirec_dr_route_kernel(DrArgs a, int64_t s0, int ns, float* __restrict__ ws,
                                                                   const float* __restrict__ gout,
                                                                   float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = a.T, Dc = a.Dc, K = a.K, R = a.R, Dcp = mi_odd(Dc);
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (row >= (int64_t)ns * K) return;
  const int k = (int)(row % K);
  const int64_t b = s0 + row / K;
  float* u = lds + (size_t)wave * dr_row_floats(T, Dc, R);       // [T][Dcp]
  float* Call = u + T * Dcp;                                     // [R][T]: the weights of every round
  float* dLall = Call + R * T;                                   // [R][T]: the logit gradient that enters round r
  float* L = dLall + R * T;                                      // [T]: L going forward, dL coming back
  float* dW = L + T;                                             // [T]
  int* part = reinterpret_cast<int*>(dW + T);                    // [T]
  float* dsall = reinterpret_cast<float*>(part + T);             // [R][Dcp]
  float* call = dsall + R * Dcp;                                 // [R][Dcp]: c of every round (forward: row 0 alone)
  float* __restrict__ g = ws + (size_t)row * T * Dc;

  for (int i = lane; i < T * Dc; i += 64) {
    const int t = i / Dc, d = i - t * Dc;
    u[t * Dcp + d] = g[i];
  }
  for (int t = lane; t < T; t += 64) {
    part[t] = (a.series[(b * T + t) * a.C] == a.padding_index) == (a.keep != 0);
    L[t] = a.B0[k * T + t];
  }
  wave_sync();
  caps_route_rounds<BWD>(L, part, Call, T, u, Dcp, T, Dc, R, call, BWD ? nullptr : out + (b * K + k) * Dc, lane);
  if (!BWD) return;

  float* dL = L;
  for (int t = lane; t < T; t += 64) dL[t] = 0.f;
  wave_sync();
  for (int r = R - 1; r >= 0; --r) {
    const bool last = r == R - 1;
    const float* Wk = Call + r * T;
    float *dsr = dsall + r * Dcp, *cr = call + r * Dcp;
    caps_squash_bwd_row(Wk, dL, u, Dcp, T, Dc, last ? gout + (b * K + k) * Dc : nullptr, dsr, cr, lane);   // s, dc
    for (int t = lane; t < T; t += 64) dLall[r * T + t] = dL[t];
    wave_sync();
    caps_softmax_bwd_row(dsr, u, Dcp, T, Dc, Wk, part, dW, dL, lane);      // dW = ds u^T and the softmax, back
    wave_sync();
  }
  for (int i = lane; i < T * Dc; i += 64) {                      // du = sum_r C_r^T ds_r + dL_r^T c_r
    const int t = i / Dc, d = i - t * Dc;
    float acc = 0.f;
    for (int r = 0; r < R; ++r) {
      acc = fmaf(Call[r * T + t], dsall[r * Dcp + d], acc);
      if (r < R - 1) acc = fmaf(dLall[r * T + t], call[r * Dcp + d], acc);
    }
    g[i] = acc;
  }
}

// gkeys[b, t, :] = sum_k du[b - s0, k, t, :] W[k, t]^T; grid (tiles, T)
__global__ __launch_bounds__(MI_NTHR) void comirec_dr_keys_kernel(DrArgs a, int64_t s0, int ns, const float* __restrict__ du,
                                                                  float* __restrict__ gkeys) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, Dc = a.Dc, K = a.K, t = blockIdx.y;
  const int64_t b0 = s0 + (int64_t)blockIdx.x * MB_T, bend = s0 + ns;
  float* dus = lds;                                              // [even(Dc)][33]
  if ((Dc & 1) && tid < MB_LD) dus[Dc * MB_LD + tid] = 0.f;
  f32x16 acc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
  for (int k = 0; k < K; ++k) {
    __syncthreads();                                             // the previous k has been read
    for (int i = tid; i < MB_T * Dc; i += MI_NTHR) {
      const int e = i / Dc, c = i - e * Dc;
      const int64_t b = b0 + e;
      dus[c * MB_LD + e] = b < bend ? du[(((b - s0) * K + k) * T + t) * Dc + c] : 0.f;
    }
    __syncthreads();
    mb_mma<true>(acc, dus, Dc, a.W + ((int64_t)k * T + t) * D * Dc, Dc, 0, D, wave, lo, hi);
  }
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int n = (wave + 4 * j) * 32 + lo;
    if ((wave + 4 * j) * 32 < D) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t b = b0 + mb_row(r, hi);
        if (b < bend && n < D) gkeys[(b * T + t) * D + n] = acc[j][r];
      }
    }
  }
}

// slot[slice][k, t] (+)= x_t^T du[:, k, t, :] over the tiles of the slice; grid (K T, slices, block groups)
template <int NB>
__global__ __launch_bounds__(MI_NTHR) void comirec_dr_weight_kernel(DrArgs a, int64_t s0, int ns,
                                                                    const float* __restrict__ du,
                                                                    float* __restrict__ slots, int first) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, Dc = a.Dc, K = a.K, Dp = mi_odd(D), Dcp = mi_odd(Dc);
  const int kt = blockIdx.x, k = kt / T, t = kt - k * T, blk0 = blockIdx.z * 4 * NB;
  const int ntile = (ns + MB_T - 1) / MB_T, per = (ntile + gridDim.y - 1) / gridDim.y;
  const int tile0 = blockIdx.y * per, tile1 = tile0 + per < ntile ? tile0 + per : ntile;
  const int64_t bend = s0 + ns;
  float* xs = lds;                                               // [32][Dp]
  float* dut = xs + MB_T * Dp;                                   // [32][Dcp]
  f32x16 sacc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) mb_zero(sacc[j]);
  bool bad = false;
  for (int tile = tile0; tile < tile1; ++tile) {
    const int64_t b0 = s0 + (int64_t)tile * MB_T;
    cr_gather_tile(a, b0, bend, t, xs, Dp, 1, tid, bad);
    for (int i = tid; i < MB_T * Dc; i += MI_NTHR) {
      const int e = i / Dc, c = i - e * Dc;
      const int64_t b = b0 + e;
      dut[e * Dcp + c] = b < bend ? du[(((b - s0) * K + k) * T + t) * Dc + c] : 0.f;
    }
    __syncthreads();
    caps_weight_grad<NB>(sacc, xs, Dp, dut, Dcp, MB_T, D, Dc, wave, lo, hi, blk0);
    __syncthreads();                                             // the next tile overwrites both
  }
  caps_weight_store<NB>(sacc, slots + ((int64_t)blockIdx.y * K * T + kt) * D * Dc, D, Dc, wave, lo, hi, blk0, !first);
}

template <int NB>
static int dr_launch_weight(const DrArgs& a, int64_t s0, int ns, int slices, const float* du, float* slots, int first,
                            hipStream_t st) {
  const size_t lds = sizeof(float) * MB_T * (mi_odd(a.D) + mi_odd(a.Dc));
  if (hipError_t err = rec_allow_lds<comirec_dr_weight_kernel<NB>>(sizeof(float) * MB_T * 2 * mi_odd(MI_MAXD)))
    return (int)err;
  hipLaunchKernelGGL(comirec_dr_weight_kernel<NB>, dim3(a.K * a.T, slices, dr_weight_groups(a.D, a.Dc)), dim3(MI_NTHR),
                     lds, st, a, s0, ns, du, slots, first);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

static int dr_project(const DrArgs& a, int64_t s0, int ns, float* u, int* oob, hipStream_t st) {
  const size_t lds = sizeof(float) * mb_even(a.D) * MB_LD;
  hipLaunchKernelGGL(comirec_dr_project_kernel, dim3((ns + MB_T - 1) / MB_T, a.T), dim3(MI_NTHR), lds, st, a, s0, ns, u,
                     oob);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

template <bool BWD>
static int dr_route(const DrArgs& a, int64_t s0, int ns, float* ws, const float* gout, float* out, hipStream_t st) {
  const int wpb = dr_waves(a.T, a.Dc, a.R);
  return caps_launch<comirec_dr_route_kernel<BWD>>(dim3((unsigned)ceil_div64((int64_t)ns * a.K, wpb)), 64 * wpb,
                                                   sizeof(float) * wpb * dr_row_floats(a.T, a.Dc, a.R), st, a, s0, ns, ws,
                                                   gout, out);
}

// ---- (b) self-attentive extractor ------------------------------------------------------------------------------------
struct SaArgs : CapsSeries {
  const float *W1, *W2, *pos;
  int keep;
};

// floats of LDS of the backward, which is what both directions are held to:
//   xs [T][D | 1], h and dz [T][Dc | 1], A and the scores / dsc [K][T], W2, gout and dW2 [K][Dc | 1], part [T]
__host__ __device__ inline size_t sa_lds_floats(int T, int D, int Dc, int K) {
  return (size_t)T * mi_odd(D) + 2 * (size_t)T * mi_odd(Dc) + 2 * (size_t)K * T + 3 * (size_t)K * mi_odd(Dc) + T;
}
// and of the forward: xs, h, A, the scores, W2, part
__host__ __device__ inline size_t sa_fwd_lds_floats(int T, int D, int Dc, int K) {
  return (size_t)T * mi_odd(D) + (size_t)T * mi_odd(Dc) + 2 * (size_t)K * T + (size_t)K * mi_odd(Dc) + T;
}
static int sa_check(int64_t B, int T, int E, int C, int Dc, int K) {
  const int rc = caps_series_shape(B, T, E, C, Dc, K, 1);
  return rc ? rc : caps_fits(sizeof(float) * sa_lds_floats(T, E * C, Dc, K));
}

__device__ __forceinline__ void sa_load_w2(const SaArgs& a, float* w2s, int tid) {
  const int Dc = a.Dc, Dcp = mi_odd(Dc);
  for (int i = tid; i < a.K * Dc; i += MI_NTHR) {
    const int k = i / Dc, d = i - k * Dc;
    w2s[k * Dcp + d] = a.W2[i];
  }
}

// The rows of example b (+ pos) into xs, part, h = tanh(xs W1), the scores into L and the weights into A.  out (may be
// NULL): the weighted sums of h.  w2s holds W2 already.  Ends with every wave done with its own rows only.
__device__ __forceinline__ void sa_forward(const SaArgs& a, int64_t b, float* xs, float* h, float* A, float* L,
                                           const float* w2s, int* part, float* __restrict__ out, int tid, bool& bad) {
  const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, Dc = a.Dc, K = a.K, Dp = mi_odd(D), Dcp = mi_odd(Dc);
  mi_gather<MI_NTHR>(a.embed, a.ld, a.V, a.series + b * T * a.C, T, a.C, a.E, xs, Dp, tid, bad, a.padding_index, part);
  __syncthreads();
  for (int t = tid; t < T; t += MI_NTHR) part[t] = (part[t] != 0) != (a.keep != 0);      // (id == pad) == keep
  if (a.pos)
    for (int i = tid; i < T * D; i += MI_NTHR) {
      const int t = i / D, d = i - t * D;
      xs[t * Dp + d] = xs[t * Dp + d] + a.pos[i];
    }
  __syncthreads();
  caps_project<true>(xs, Dp, a.W1, T, D, Dc, h, Dcp, wave, lo, hi);
  __syncthreads();
  for (int k = wave; k < K; k += 4) {
    float *Lk = L + k * T, *Ak = A + k * T;
    for (int t = lane; t < T; t += 64) Lk[t] = mi_dot(w2s + k * Dcp, h + t * Dcp, 1, Dc);
    wave_sync();
    caps_softmax_row(Lk, part, Ak, T, lane);
    if (out)
      for (int d = lane; d < Dc; d += 64) out[(b * K + k) * Dc + d] = mi_dot(Ak, h + d, Dcp, T);
  }
}

__global__ __launch_bounds__(MI_NTHR) void comirec_sa_fwd_kernel(SaArgs a, float* __restrict__ out, int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = a.T, K = a.K, Dp = mi_odd(a.D), Dcp = mi_odd(a.Dc);
  float* xs = lds;
  float* h = xs + T * Dp;
  float* A = h + T * Dcp;
  float* L = A + K * T;
  float* w2s = L + K * T;
  int* part = reinterpret_cast<int*>(w2s + K * Dcp);
  bool bad = false;
  sa_load_w2(a, w2s, threadIdx.x);
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    sa_forward(a, b, xs, h, A, L, w2s, part, out, threadIdx.x, bad);
    __syncthreads();                                             // the next example overwrites all of it
  }
  if (bad && oob) *oob = 1;
}

// NB: 32 x 32 blocks of dW1 per wave (block w, w + 4, ...): 1, 4 or 16
template <int NB>
__global__ __launch_bounds__(MI_NTHR, NB == 1 ? 4 : 1) void comirec_sa_bwd_kernel(SaArgs a, const float* __restrict__ gout,
                                                                                 float* __restrict__ gkeys,
                                                                                 float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, Dc = a.Dc, K = a.K, Dp = mi_odd(D), Dcp = mi_odd(Dc);
  float* xs = lds;
  float* h = xs + T * Dp;
  float* dz = h + T * Dcp;
  float* A = dz + T * Dcp;                                       // [K][T]
  float* L = A + K * T;                                          // [K][T]: the scores, then dA, then dsc
  float* w2s = L + K * T;                                        // [K][Dcp]
  float* gs = w2s + K * Dcp;                                     // [K][Dcp]: gout of the example
  float* dw2 = gs + K * Dcp;                                     // [K][Dcp]: over the workgroup's examples
  int* part = reinterpret_cast<int*>(dw2 + K * Dcp);
  f32x16 sacc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) mb_zero(sacc[j]);
  bool bad = false;
  sa_load_w2(a, w2s, tid);
  for (int i = tid; i < K * Dcp; i += MI_NTHR) dw2[i] = 0.f;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    for (int i = tid; i < K * Dc; i += MI_NTHR) {
      const int k = i / Dc, d = i - k * Dc;
      gs[k * Dcp + d] = gout[b * K * Dc + i];
    }
    sa_forward(a, b, xs, h, A, L, w2s, part, nullptr, tid, bad);
    for (int k = wave; k < K; k += 4) {                          // the softmax, back: the row's wave goes on
      float *Lk = L + k * T, *Ak = A + k * T;
      float dot = 0.f;
      for (int t = lane; t < T; t += 64) {
        const float dA = mi_dot(gs + k * Dcp, h + t * Dcp, 1, Dc);
        Lk[t] = dA;
        dot = fmaf(dA, Ak[t], dot);
      }
      dot = group_sum<64>(dot);
      for (int t = lane; t < T; t += 64) Lk[t] = part[t] ? Ak[t] * (Lk[t] - dot) : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < T * Dc; i += MI_NTHR) {                // dz = (A^T gout + dsc^T W2) (1 - h^2)
      const int t = i / Dc, d = i - t * Dc;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) {
        acc = fmaf(A[k * T + t], gs[k * Dcp + d], acc);
        acc = fmaf(L[k * T + t], w2s[k * Dcp + d], acc);
      }
      const float hv = h[t * Dcp + d];
      dz[t * Dcp + d] = acc * (1.f - hv * hv);
    }
    for (int i = tid; i < K * Dc; i += MI_NTHR) {                // dW2 += dsc h: an element stays with its thread
      const int k = i / Dc, d = i - k * Dc;
      dw2[k * Dcp + d] = dw2[k * Dcp + d] + mi_dot(L + k * T, h + d, Dcp, T);
    }
    __syncthreads();
    caps_keys_grad(dz, Dcp, a.W1, T, D, Dc, gkeys + b * T * D, wave, lo, hi);      // gkeys[b] = dz W1^T
    caps_weight_grad<NB>(sacc, xs, Dp, dz, Dcp, T, D, Dc, wave, lo, hi);           // dW1 += (x + pos)^T dz
    __syncthreads();                                             // the next example overwrites all of it
  }

  float* __restrict__ slot = slots + (int64_t)blockIdx.x * (D + K) * Dc;
  caps_weight_store<NB>(sacc, slot, D, Dc, wave, lo, hi);
  for (int i = tid; i < K * Dc; i += MI_NTHR) {
    const int k = i / Dc, d = i - k * Dc;
    slot[D * Dc + i] = dw2[k * Dcp + d];
  }
}

// ---- (c) hard attention + loss ---------------------------------------------------------------------------------------
// One wave per example.  A wave past the batch leaves: there is no workgroup-level barrier.  The LDS of an example is
// the label-aware attention's: m, x, p [K][Ns], chosen [Ns] (of the second [K][Ns]), inner and g [Ns].
template <bool BWD>
__global__ __launch_bounds__(MI_NTHR) void comirec_select_kernel(ItemArgs a, int32_t* __restrict__ chosen,
                                                                 float* __restrict__ inner, float* __restrict__ loss,
                                                                 const float* __restrict__ ginner,
                                                                 const float* __restrict__ gloss,
                                                                 const float* __restrict__ gsel, float* __restrict__ gm,
                                                                 float* __restrict__ gitems, int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Ns = a.Ns, Dc = a.Dc, K = a.K, Dcp = mi_odd(Dc);
  const int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= a.B) return;
  const ItemLds f = la_carve(lds, wave, Ns, Dc, K);
  float *ms = f.ms, *xs = f.xs, *p = f.sc, *o = f.o, *go = f.go;
  int* ch = reinterpret_cast<int*>(f.w);                         // [Ns]
  bool bad = false;

  la_load(a, b, f, lane, bad);
  if (BWD)
    for (int s = lane; s < Ns; s += 64) {
      const int c = chosen[b * Ns + s];
      ch[s] = c < 0 ? 0 : (c < K ? c : K - 1);                   // whatever it holds, stay inside m
    }
  wave_sync();
  if (!BWD) {
    la_scores(f, Ns, Dc, K, lane);
    for (int s = lane; s < Ns; s += 64) {
      int best = 0;
      float bv = p[s];
      for (int k = 1; k < K; ++k) {
        const float v = p[k * Ns + s];
        if (v > bv) {                                            // strictly: the smallest k of a tie stays
          bv = v;
          best = k;
        }
      }
      o[s] = bv;
      chosen[b * Ns + s] = best;
      inner[b * Ns + s] = bv;
    }
  } else {
    for (int s = lane; s < Ns; s += 64) {
      const float* mk = ms + ch[s] * Dcp;
      float acc = 0.f;
      for (int d = 0; d < Dc; ++d) acc = fmaf(mk[d], xs[s * Dcp + d], acc);
      o[s] = acc;
    }
  }
  wave_sync();
  const float lse = la_logsumexp(o, Ns, lane);
  if (!BWD) {
    if (lane == 0) loss[b] = lse - o[0];
    if (bad && oob) *oob = 1;
    return;
  }
  la_loss_grad(f, lse, gloss ? gloss[b] : 0.f, ginner ? ginner + b * Ns : nullptr, Ns, lane);
  for (int i = lane; i < K * Dc; i += 64) {
    const int k = i / Dc, d = i - k * Dc;
    float acc = 0.f;
    for (int s = 0; s < Ns; ++s)
      if (ch[s] == k) {
        acc = fmaf(go[s], xs[s * Dcp + d], acc);
        if (gsel) acc += gsel[(b * Ns + s) * Dc + d];
      }
    gm[b * K * Dc + i] = acc;
  }
  for (int i = lane; i < Ns * Dc; i += 64) {
    const int s = i / Dc, d = i - s * Dc;
    gitems[b * Ns * Dc + i] = go[s] * ms[ch[s] * Dcp + d];
  }
}

}  // namespace

extern "C" size_t rec_comirec_dr_workspace_bytes(int64_t B, int T, int E, int C, int Dc, int K, int R) {
  if (dr_check(B, T, E, C, Dc, K, R) != REC_OK) return 0;
  const DrPlan p = dr_plan(B, T, E * C, Dc, K);
  return sizeof(float) * (p.u_floats + p.slot_floats + 4);
}

extern "C" int rec_comirec_dr_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                      int64_t B, int T, const float* W, const float* B0, int Dc, int K, int R,
                                      int64_t padding_index, int keep_padding, float* out, int* oob_flag, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (int rc = dr_check(B, T, E, C, Dc, K, R)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !W || !B0 || !out || !workspace) return REC_E_ARG;
  const int D = E * C;
  const DrPlan p = dr_plan(B, T, D, Dc, K);
  if (workspace_bytes < sizeof(float) * p.u_floats) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;
  hipStream_t st = as_stream(stream);
  const DrArgs a{{embed, ld, V, series, B, padding_index, T, C, E, D, Dc, K}, W, B0, keep_padding, R};
  float* u = static_cast<float*>(workspace);
  for (int64_t s0 = 0; s0 < B; s0 += p.slab) {
    const int ns = (int)(B - s0 < p.slab ? B - s0 : p.slab);
    if (int rc = dr_project(a, s0, ns, u, oob_flag, st)) return rc;
    if (int rc = dr_route<false>(a, s0, ns, u, nullptr, out, st)) return rc;
  }
  return REC_OK;
}

extern "C" int rec_comirec_dr_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                      int64_t B, int T, const float* W, const float* B0, int Dc, int K, int R,
                                      int64_t padding_index, int keep_padding, const float* gout, float* gkeys, float* dW,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = dr_check(B, T, E, C, Dc, K, R)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !W || !B0 || !gout || !gkeys || !dW || !workspace) return REC_E_ARG;
  const int D = E * C;
  const DrPlan p = dr_plan(B, T, D, Dc, K);
  if (workspace_bytes < sizeof(float) * (p.u_floats + p.slot_floats)) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;                                     // nothing is launched and nothing written
  hipStream_t st = as_stream(stream);
  const DrArgs a{{embed, ld, V, series, B, padding_index, T, C, E, D, Dc, K}, W, B0, keep_padding, R};
  float* u = static_cast<float*>(workspace);
  float* slots = u + p.u_floats;
  for (int64_t s0 = 0; s0 < B; s0 += p.slab) {
    const int ns = (int)(B - s0 < p.slab ? B - s0 : p.slab);
    if (int rc = dr_project(a, s0, ns, u, nullptr, st)) return rc;
    if (int rc = dr_route<true>(a, s0, ns, u, gout, nullptr, st)) return rc;
    hipLaunchKernelGGL(comirec_dr_keys_kernel, dim3((ns + MB_T - 1) / MB_T, T), dim3(MI_NTHR),
                       sizeof(float) * mb_even(Dc) * MB_LD, st, a, s0, ns, u, gkeys);
    REC_LAUNCH_CHECK();
    const int rc = dr_weight_nb(D, Dc) == 1 ? dr_launch_weight<1>(a, s0, ns, p.slices, u, slots, s0 == 0, st)
                                            : dr_launch_weight<4>(a, s0, ns, p.slices, u, slots, s0 == 0, st);
    if (rc) return rc;
  }
  const int64_t n = (int64_t)K * T * D * Dc;                     // below 2^31: T (Dc | 1) <= 38400 by the LDS fit
  return rec_slot_sum(REC_SLOTS_SERIAL, (int)n, p.slices, slots, {{dW}, {(int)n}}, st);
}

extern "C" size_t rec_comirec_sa_workspace_bytes(int64_t B, int T, int E, int C, int Dc, int K) {
  if (sa_check(B, T, E, C, Dc, K) != REC_OK) return 0;
  return sizeof(float) * ((size_t)caps_grid(B, E * C, Dc, CR_GRID) * (E * C + K) * Dc + 4);
}

extern "C" int rec_comirec_sa_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                      int64_t B, int T, const float* W1, const float* W2, const float* pos, int Dc, int K,
                                      int64_t padding_index, int keep_padding, float* out, int* oob_flag, void* stream) {
  if (int rc = sa_check(B, T, E, C, Dc, K)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !W1 || !W2 || !out) return REC_E_ARG;
  if (B == 0) return REC_OK;
  const SaArgs a{{embed, ld, V, series, B, padding_index, T, C, E, E * C, Dc, K}, W1, W2, pos, keep_padding};
  return caps_launch<comirec_sa_fwd_kernel>(dim3(caps_fwd_grid(B)), MI_NTHR,
                                            sizeof(float) * sa_fwd_lds_floats(T, E * C, Dc, K), as_stream(stream), a, out,
                                            oob_flag);
}

extern "C" int rec_comirec_sa_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                      int64_t B, int T, const float* W1, const float* W2, const float* pos, int Dc, int K,
                                      int64_t padding_index, int keep_padding, const float* gout, float* gkeys,
                                      float* dW1, float* dW2, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = sa_check(B, T, E, C, Dc, K)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !W1 || !W2 || !gout || !gkeys || !dW1 || !dW2 || !workspace)
    return REC_E_ARG;
  const int D = E * C, grid = caps_grid(B, D, Dc, CR_GRID);
  if (workspace_bytes < sizeof(float) * (size_t)grid * (D + K) * Dc) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;                                     // nothing is launched and nothing written
  hipStream_t st = as_stream(stream);
  const SaArgs a{{embed, ld, V, series, B, padding_index, T, C, E, D, Dc, K}, W1, W2, pos, keep_padding};
  const size_t lds = sizeof(float) * sa_lds_floats(T, D, Dc, K);
  float* slots = static_cast<float*>(workspace);
  const int rc = caps_launch_nb(caps_weight_nb(D, Dc), [&](auto nb) {
    return caps_launch<comirec_sa_bwd_kernel<nb.value>>(dim3(grid), MI_NTHR, lds, st, a, gout, gkeys, slots);
  });
  if (rc) return rc;
  return rec_slot_sum(REC_SLOTS_WAVE, (D + K) * Dc, grid, slots, {{dW1, dW2}, {D * Dc, K * Dc}}, st);
}

extern "C" size_t rec_comirec_select_lds_bytes(int Ns, int E, int C, int K) {
  return la_shape(0, Ns, E, C, K) == REC_OK ? la_lds_bytes(Ns, E * C, K) : 0;
}

extern "C" int rec_comirec_select_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items,
                                          int64_t B, int Ns, const float* m, int K, int32_t* chosen, float* inner,
                                          float* loss, int* oob_flag, void* stream) {
  if (int rc = la_shape(B, Ns, E, C, K)) return rc;
  if (ld < E || V <= 0 || !embed || !items || !m || !chosen || !inner || !loss) return REC_E_ARG;
  if (B == 0) return REC_OK;
  return la_launch<comirec_select_kernel<false>>({embed, ld, V, items, B, m, nullptr, Ns, C, E, E * C, K}, stream, chosen,
                                                 inner, loss, nullptr, nullptr, nullptr, nullptr, nullptr, oob_flag);
}

extern "C" int rec_comirec_select_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items,
                                          int64_t B, int Ns, const float* m, int K, const int32_t* chosen,
                                          const float* ginner, const float* gloss, const float* gsel, float* gm,
                                          float* gitems, void* stream) {
  if (int rc = la_shape(B, Ns, E, C, K)) return rc;
  if (ld < E || V <= 0 || !embed || !items || !m || !chosen || (!ginner && !gloss) || !gm || !gitems) return REC_E_ARG;
  if (B == 0) return REC_OK;
  return la_launch<comirec_select_kernel<true>>({embed, ld, V, items, B, m, nullptr, Ns, C, E, E * C, K}, stream,
                                                const_cast<int32_t*>(chosen), nullptr, nullptr, ginner, gloss, gsel, gm,
                                                gitems, nullptr);
}
