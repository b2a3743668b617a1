// MIND (MultiInterestExtractorLayer, LabelAwareAttention and MINDLayer.call, 6.MIND/CustomLayers.py:62-158, 263-285) on
// gfx950, fp32: the capsule routing and the label-aware attention with its sampled-softmax loss.
//
// Capsule routing, per example b (series int64 [B, T, C] as rec_din_attn_*; D = E C):
//   x_t = concat_r embed[series[b,t,r]]  [T, D]     valid_t = series[b,t,0] != padding_index     u = x S  [T, Dc]
//   L = B0 [K, T];  R times:  W = softmax_t(valid_t ? L : -FLT_MAX),  c = squash(W u),  (but the last)  L += c u^T
//   out[b] = c  [K, Dc]
// squash(s) = s n / (1 + n^2) with n = |s|: the reference's n^2 / ((1 + n^2) n) is 0/0 at n = 0, this form gives 0 there
// and the backward gives a zero gradient there, which is the limit.  An example with no valid position has every logit
// at -FLT_MAX and so the uniform weights 1 / T over ALL positions, padded ones included; nothing becomes NaN.
// Forward, one launch.  A workgroup of 4 waves holds ONE example at a time: its rows are gathered once into LDS
// ([T][D | 1]: the odd stride serves the row-per-lane reads of x S and the column-per-lane reads of x^T du alike),
// u = x S runs on v_mfma_f32_32x32x2_f32, one (32 rows, 32 columns) block per wave and step, S read from global memory
// (every workgroup reads the same few KiB), and lands in LDS ([T][Dc | 1]).  A capsule row k depends on no other row,
// so wave k & 3 owns it through all R rounds with nothing but wave-level ordering: the softmax with lanes over t, W u
// with lanes over the capsule dims (the weight is a broadcast read), the squash with one wave sum, c u^T with lanes
// over t.  K <= 16 rows of T <= ~100 and Dc <= 256 are VALU work; an MFMA tile would be padding.  u, L, W and c never
// leave LDS; the forward saves nothing but out.
// Backward.  It gathers the rows and runs the rounds again, keeping the weights W of every round in LDS; then, from the
// last round to the first (dL is the gradient of the logits that leave round r, zero after the last):
//   s = W_r u   dc = last ? gout : dL u   ds = squash'(s) dc   c = squash(s)          (the row's wave)
//   du += W_r^T ds + dL^T c                                                            (all threads, over (t, dim))
//   dW = ds u^T   dL += valid_t ? W_r (dW - sum_t dW W_r) : 0                          (the row's wave)
// with no stop_gradient anywhere; B0 gets nothing.  gkeys[b] = du S^T and dS += x^T du run on the MFMA again.  dS stays in
// the accumulators of the workgroup over all its examples (the grid is capped, so the number of partials does not grow
// with B), goes to the workgroup's slot and the slots are added by rec_slot_sum in wave order.
//
// Label-aware attention + sampled-softmax loss, per example b (items int64 [B, Ns, C]; Dc = E C):
//   x_s = concat_r embed[items[b,s,r]]   sc[k,s] = m_k . x_s   w[:,s] = softmax_k(k < kv ? sc[k,s] : -FLT_MAX)
//   out[s] = sum_k w[k,s] sc[k,s]   loss = logsumexp_s(out) - out[0]
// One wave owns an example (its m, its rows and the K Ns scores in LDS); a workgroup has 4, 2 or 1 waves, as many as
// fit the launch cap.  The backward recomputes the forward from the ids and m and returns gm and gitems in one launch:
//   g[s] = gout[s] + gloss (softmax_s(out)[s] - [s == 0])
//   dsc[k,s] = g[s] (w[k,s] + (k < kv ? w[k,s] (sc[k,s] - out[s]) : 0))     a masked capsule's score is a constant inside
//   the softmax and keeps the direct term alone, zero unless every capsule is masked
//   gm_k = sum_s dsc[k,s] x_s   gitems_s = sum_k dsc[k,s] m_k
// Neither family uses a float atomic or scratch; every launch only enqueues.  An id outside [0, V) reads as a zero row and
// sets the flag.
#include "capsule.h"

namespace {

constexpr int MI_GRID = 1024;                   // workgroups (= dS partials) of the routing backward, at the most

// floats of LDS of the routing backward, which is what both directions are held to:
//   xs [T][D | 1], u and du [T][Dc | 1], W of every round [R][K][T], dL and dW [K][T], ds and c [K][Dc | 1], valid [T]
__host__ __device__ inline size_t rt_lds_floats(int T, int D, int Dc, int K, int R) {
  return (size_t)T * mi_odd(D) + 2 * (size_t)T * mi_odd(Dc) + (size_t)(R + 2) * K * T + 2 * (size_t)K * mi_odd(Dc) + T;
}
// and of the forward: xs, u, W [K][T], L [K][T], c [K][Dc | 1], valid [T]
__host__ __device__ inline size_t rt_fwd_lds_floats(int T, int D, int Dc, int K) {
  return (size_t)T * mi_odd(D) + (size_t)T * mi_odd(Dc) + 2 * (size_t)K * T + (size_t)K * mi_odd(Dc) + T;
}

struct RtArgs : CapsSeries {
  const float *S, *B0;
  int R;
};

// The rows of example b into xs, valid, L <- B0, u = x S, and the R rounds.  KEEP: W of round r goes to Wall[r] (the
// backward), otherwise every round uses Wall[0].  out (may be NULL): c of the last round.  Ends with every wave done
// with its own rows only: the caller synchronises.
template <bool KEEP>
__device__ __forceinline__ void rt_forward(const RtArgs& a, int64_t b, float* xs, float* u, float* Wall, float* L,
                                           float* c, int* valid, float* __restrict__ out, int tid, bool& bad) {
  const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, C = a.C, E = a.E, D = a.D, Dc = a.Dc, K = a.K, R = a.R, Dp = mi_odd(D), Dcp = mi_odd(Dc);
  const int64_t* __restrict__ ids = a.series + b * T * C;
  const float l0 = tid < K * T ? a.B0[tid] : 0.f;                // in flight beside the rows
  mi_gather<MI_NTHR>(a.embed, a.ld, a.V, ids, T, C, E, xs, Dp, tid, bad, a.padding_index, valid);
  if (tid < K * T) L[tid] = l0;
  for (int i = tid + MI_NTHR; i < K * T; i += MI_NTHR) L[i] = a.B0[i];
  __syncthreads();

  caps_project<false>(xs, Dp, a.S, T, D, Dc, u, Dcp, wave, lo, hi);        // u = x S
  __syncthreads();

  for (int k = wave; k < K; k += 4)                              // a row needs no other row
    caps_route_rounds<KEEP>(L + k * T, valid, Wall + k * T, K * T, u, Dcp, T, Dc, R, c + k * Dcp,
                            out ? out + ((int64_t)b * K + k) * Dc : nullptr, lane);
}

__global__ __launch_bounds__(MI_NTHR) void mind_routing_fwd_kernel(RtArgs a, float* __restrict__ out,
                                                                   int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = a.T, K = a.K, Dp = mi_odd(a.D), Dcp = mi_odd(a.Dc);
  float* xs = lds;
  float* u = xs + T * Dp;
  float* W = u + T * Dcp;
  float* L = W + K * T;
  float* c = L + K * T;
  int* valid = reinterpret_cast<int*>(c + K * Dcp);
  bool bad = false;
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    rt_forward<false>(a, b, xs, u, W, L, c, valid, out, threadIdx.x, bad);
    __syncthreads();                                             // the next example overwrites all of it
  }
  if (bad && oob) *oob = 1;
}

// NB: 32 x 32 blocks of dS per wave (block w, w + 4, ...): 1, 4 or 16
template <int NB>
__global__ __launch_bounds__(MI_NTHR, NB == 1 ? 4 : 1) void mind_routing_bwd_kernel(RtArgs a, const float* __restrict__ gout,
                                                                   float* __restrict__ gkeys,
                                                                   float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, Dc = a.Dc, K = a.K, R = a.R, Dp = mi_odd(D), Dcp = mi_odd(Dc);
  float* xs = lds;
  float* u = xs + T * Dp;
  float* du = u + T * Dcp;
  float* Wall = du + T * Dcp;                                    // [R][K][T]
  float* dL = Wall + (size_t)R * K * T;                          // [K][T]: L going forward, dL coming back
  float* dW = dL + K * T;                                        // [K][T]
  float* ds = dW + K * T;                                        // [K][Dcp]
  float* c = ds + K * Dcp;                                       // [K][Dcp]: s, then c
  int* valid = reinterpret_cast<int*>(c + K * Dcp);
  f32x16 sacc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) mb_zero(sacc[j]);
  bool bad = false;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    rt_forward<true>(a, b, xs, u, Wall, dL, c, valid, nullptr, tid, bad);
    __syncthreads();
    for (int i = tid; i < K * T; i += MI_NTHR) dL[i] = 0.f;
    __syncthreads();

    for (int r = R - 1; r >= 0; --r) {
      const bool last = r == R - 1;
      const float* Wr = Wall + (size_t)r * K * T;
      for (int k = wave; k < K; k += 4)                          // s, dc -> ds, c of the row
        caps_squash_bwd_row(Wr + k * T, dL + k * T, u, Dcp, T, Dc, last ? gout + ((int64_t)b * K + k) * Dc : nullptr,
                            ds + k * Dcp, c + k * Dcp, lane);
      __syncthreads();
      for (int i = tid; i < T * Dc; i += MI_NTHR) {              // du += W_r^T ds + dL^T c
        const int t = i / Dc, d = i - t * Dc;
        float acc = last ? 0.f : du[t * Dcp + d];
        for (int k = 0; k < K; ++k) {
          acc = fmaf(Wr[k * T + t], ds[k * Dcp + d], acc);
          if (!last) acc = fmaf(dL[k * T + t], c[k * Dcp + d], acc);
        }
        du[t * Dcp + d] = acc;
      }
      __syncthreads();
      for (int k = wave; k < K; k += 4)                          // dW = ds u^T and the softmax, back
        caps_softmax_bwd_row(ds + k * Dcp, u, Dcp, T, Dc, Wr + k * T, valid, dW + k * T, dL + k * T, lane);
      __syncthreads();
    }

    caps_keys_grad(du, Dcp, a.S, T, D, Dc, gkeys + b * T * D, wave, lo, hi);       // gkeys[b] = du S^T
    caps_weight_grad<NB>(sacc, xs, Dp, du, Dcp, T, D, Dc, wave, lo, hi);           // dS += x^T du
    __syncthreads();                                             // the next example overwrites all of it
  }

  caps_weight_store<NB>(sacc, slots + (int64_t)blockIdx.x * D * Dc, D, Dc, wave, lo, hi);
}

// One wave per example.  A wave past the batch leaves: there is no workgroup-level barrier.
template <bool BWD>
__global__ __launch_bounds__(MI_NTHR) void mind_laa_kernel(ItemArgs a, float* __restrict__ out, float* __restrict__ loss,
                                                           const float* __restrict__ gout,
                                                           const float* __restrict__ gloss, float* __restrict__ gm,
                                                           float* __restrict__ gitems, int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Ns = a.Ns, Dc = a.Dc, K = a.K, Dcp = mi_odd(Dc);
  const int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= a.B) return;
  const ItemLds f = la_carve(lds, wave, Ns, Dc, K);
  float *ms = f.ms, *xs = f.xs, *sc = f.sc, *w = f.w, *o = f.o;  // sc: the scores, then dsc
  const int kv = a.kv[b];
  bool bad = false;

  la_load(a, b, f, lane, bad);
  wave_sync();
  la_scores(f, Ns, Dc, K, lane);
  for (int sI = lane; sI < Ns; sI += 64) {
    float mx = -FLT_MAX;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, k < kv ? sc[k * Ns + sI] : -FLT_MAX);
    float sum = 0.f;
    for (int k = 0; k < K; ++k) {
      const float ex = expf((k < kv ? sc[k * Ns + sI] : -FLT_MAX) - mx);
      w[k * Ns + sI] = ex;
      sum += ex;
    }
    float ov = 0.f;
    for (int k = 0; k < K; ++k) {
      const float wv = w[k * Ns + sI] / sum;
      w[k * Ns + sI] = wv;
      ov = fmaf(wv, sc[k * Ns + sI], ov);
    }
    o[sI] = ov;
    if (!BWD) out[b * Ns + sI] = ov;
  }
  wave_sync();
  const float lse = la_logsumexp(o, Ns, lane);
  if (!BWD) {
    if (lane == 0) loss[b] = lse - o[0];
    if (bad && oob) *oob = 1;
    return;
  }
  la_loss_grad(f, lse, gloss ? gloss[b] : 0.f, gout ? gout + b * Ns : nullptr, Ns, lane);
  for (int i = lane; i < K * Ns; i += 64) {
    const int k = i / Ns, sI = i - k * Ns;
    const float wv = w[i];
    sc[i] = f.go[sI] * (k < kv ? fmaf(wv, sc[i] - o[sI], wv) : wv);
  }
  wave_sync();
  for (int i = lane; i < K * Dc; i += 64) {
    const int k = i / Dc, d = i - k * Dc;
    float acc = 0.f;
    for (int sI = 0; sI < Ns; ++sI) acc = fmaf(sc[k * Ns + sI], xs[sI * Dcp + d], acc);
    gm[((int64_t)b * K + k) * Dc + d] = acc;
  }
  for (int i = lane; i < Ns * Dc; i += 64) {
    const int sI = i / Dc, d = i - sI * Dc;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(sc[k * Ns + sI], ms[k * Dcp + d], acc);
    gitems[((int64_t)b * Ns + sI) * Dc + d] = acc;
  }
}

// the sizes and the LDS fit of the routing
static int rt_check(int64_t B, int T, int E, int C, int Dc, int K, int R) {
  const int rc = caps_series_shape(B, T, E, C, Dc, K, R);
  return rc ? rc : caps_fits(sizeof(float) * rt_lds_floats(T, E * C, Dc, K, R));
}
static int rt_grid(int64_t B, int D, int Dc) { return caps_grid(B, D, Dc, MI_GRID); }

}  // namespace

extern "C" size_t rec_mind_routing_workspace_bytes(int64_t B, int T, int E, int C, int Dc, int K, int R) {
  if (rt_check(B, T, E, C, Dc, K, R) != REC_OK) return 0;
  return sizeof(float) * ((size_t)rt_grid(B, E * C, Dc) * E * C * Dc + 4);
}

extern "C" int rec_mind_routing_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                        int64_t B, int T, const float* S, const float* B0, int Dc, int K, int R,
                                        int64_t padding_index, float* out, int* oob_flag, void* stream) {
  if (int rc = rt_check(B, T, E, C, Dc, K, R)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !S || !B0 || !out) return REC_E_ARG;
  if (B == 0) return REC_OK;
  const RtArgs a{{embed, ld, V, series, B, padding_index, T, C, E, E * C, Dc, K}, S, B0, R};
  return caps_launch<mind_routing_fwd_kernel>(dim3(caps_fwd_grid(B)), MI_NTHR,
                                              sizeof(float) * rt_fwd_lds_floats(T, E * C, Dc, K), as_stream(stream), a, out,
                                              oob_flag);
}

extern "C" int rec_mind_routing_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                        int64_t B, int T, const float* S, const float* B0, int Dc, int K, int R,
                                        int64_t padding_index, const float* gout, float* gkeys, float* dS,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = rt_check(B, T, E, C, Dc, K, R)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !S || !B0 || !gout || !gkeys || !dS || !workspace) return REC_E_ARG;
  const int D = E * C, grid = rt_grid(B, D, Dc);
  if (workspace_bytes < sizeof(float) * (size_t)grid * D * Dc) return REC_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  if (B == 0) return REC_OK;                                     // nothing is launched and nothing written
  const RtArgs a{{embed, ld, V, series, B, padding_index, T, C, E, D, Dc, K}, S, B0, R};
  const size_t lds = sizeof(float) * rt_lds_floats(T, D, Dc, K, R);
  float* slots = static_cast<float*>(workspace);
  const int rc = caps_launch_nb(caps_weight_nb(D, Dc), [&](auto nb) {
    return caps_launch<mind_routing_bwd_kernel<nb.value>>(dim3(grid), MI_NTHR, lds, st, a, gout, gkeys, slots);
  });
  if (rc) return rc;
  return rec_slot_sum(REC_SLOTS_WAVE, D * Dc, grid, slots, {{dS}, {D * Dc}}, st);
}

extern "C" size_t rec_mind_laa_lds_bytes(int Ns, int E, int C, int K) {
  return la_shape(0, Ns, E, C, K) == REC_OK ? la_lds_bytes(Ns, E * C, K) : 0;
}

extern "C" int rec_mind_laa_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items,
                                    int64_t B, int Ns, const float* m, const int32_t* kv, int K, float* out,
                                    float* loss, int* oob_flag, void* stream) {
  if (int rc = la_shape(B, Ns, E, C, K)) return rc;
  if (ld < E || V <= 0 || !embed || !items || !m || !kv || !out || !loss) return REC_E_ARG;
  if (B == 0) return REC_OK;
  return la_launch<mind_laa_kernel<false>>({embed, ld, V, items, B, m, kv, Ns, C, E, E * C, K}, stream, out, loss, nullptr,
                                           nullptr, nullptr, nullptr, oob_flag);
}

extern "C" int rec_mind_laa_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* items,
                                    int64_t B, int Ns, const float* m, const int32_t* kv, int K, const float* gout,
                                    const float* gloss, float* gm, float* gitems, void* stream) {
  if (int rc = la_shape(B, Ns, E, C, K)) return rc;
  if (ld < E || V <= 0 || !embed || !items || !m || !kv || (!gout && !gloss) || !gm || !gitems) return REC_E_ARG;
  if (B == 0) return REC_OK;
  return la_launch<mind_laa_kernel<true>>({embed, ld, V, items, B, m, kv, Ns, C, E, E * C, K}, stream, nullptr, nullptr,
                                          gout, gloss, gm, gitems, nullptr);
}
