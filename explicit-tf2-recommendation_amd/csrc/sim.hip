// SIM (SIMLayer / ESULayer, 7.SIM/CustomLayers.py:130-282) on gfx950, fp32: the soft search and the one-query
// multi-head attention of the exact search unit.
//
// Search (rec_sim_search_*): the body of ip_attn_kernel (interactions.hip) -- one workgroup per example, its 4 waves
// share the time axis, lane l owns dims l, l + 64, ..., a step's score is group_sum<64> of the lane products, so it
// depends on the values of the key and of q only and equal items tie bit for bit -- plus, in the same launch:
//   forward   rank[t] = <q, k_t> for a valid step, -inf for a padded one, kept in LDS; K rounds of a one-wave arg-max
//             over rank (a candidate loses to an equal one with a lower index: tf.argsort(DESCENDING)[:K]); the K chosen
//             rows are gathered again (L2-hot; a padded position's row too) into sel, with sel_valid and chosen.
//   backward  gkeys[b,t,:] = scores_t gpooled + valid <gpooled, k_t> q  (+ gsel[b,j,:] where chosen[b,j] == t).
//
// ESU attention (rec_esu_attn_*): Keras 2.x MultiHeadAttention (value_dim = key_dim, no dropout) with ONE query over K
// dense keys.  TensorFlow cannot be imported next to this project, so this text is the definition:
//   Q_h  = (q Wq_h + bq_h) / sqrt(dk)          K_jh = x_j Wk_h + bk_h          V_jh = x_j Wv_h + bv_h
//   l_hj = <Q_h, K_jh>      a_hj = float32(l_hj + (1 - mask_j) * (-1e9))       p_h = softmax_j(a_h)
//   out  = sum_h (sum_j p_hj V_jh) Wo_h + bo
// The mask is additive in fp32, not a `where`: a row with every position masked gets a_hj = -1e9 exactly (|l| < 32) and
// so the uniform p = 1/K; the backward is the plain softmax Jacobian dl_hj = p_hj (g_hj - <p_h, g_h>) for every j.
// With one query the key and value projections collapse and the kernels use the collapsed form:
//   u_h = Wk_h Q_h [D]    l_hj = <x_j, u_h> + <bk_h, Q_h>    s_h = sum_j p_hj x_j [D]    ctx_h = s_h Wv_h + bv_h
// A workgroup of 4 waves owns 32 examples.  Every projection runs on v_mfma_f32_32x32x2_f32 through the tile helpers of
// mfma_tile.h: the A operand is staged k-major in ONE LDS buffer, the weights (295 KB at the defaults, more than the LDS)
// stream from L2, the products leave the accumulators for the workspace, from where the next stage reads them back.
// Backward: the forward's stages again (Q, u, s, ctx), then the chain in reverse; per-tile column sums give the bias
// gradients (slot sum, wave order), and ONE small_dw launch over 5 H matrices of at most 64 x 64 gives dWq, dWk, dWv, dWo
// and dbk (at most 16 batch slices, added in slice order).  No float atomics: bit-identical results run to run.
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------------------------
constexpr int SS_MAX_K = REC_SEARCH_MAX_K;
constexpr int SS_MAX_D = REC_SEARCH_MAX_D;
constexpr size_t SS_LDS_CAP = REC_SEARCH_LDS_CAP;
static_assert(sizeof(float) * (4 * SS_MAX_D + SS_MAX_K) < SS_LDS_CAP,
              "four waves' partial rows of the widest key and the SS_MAX_K chosen positions leave LDS for the steps");

__host__ __device__ inline size_t ss_lds_bytes(int T, int C, int D) {
  return (size_t)T * C * 4 + (size_t)4 * D * 4 + (size_t)T * 4 + SS_MAX_K * 4;
}

// The copy of ip_attn_kernel's body is kept on purpose, and a fix to one (the ids[t * C] validity test, say) goes into
// both.  Hoisted into one __forceinline__ template over a hooks struct the two kernels kept their registers, occupancy
// and bits, but the compiler ordered the address arithmetic of the unrolled steps differently and the backward kernels
// ran 2.5 % (ip_attn, config G) and 3 - 4 % (this one, T = 100 and 1000) slower on the MI355X, twice in a row.
template <int NPL, bool BWD>
__global__ __launch_bounds__(256) void sim_search_kernel(
    const float* __restrict__ embed, int64_t ld, int64_t V, int E, int C, const int64_t* __restrict__ series, int64_t B,
    int T, const float* __restrict__ q, int64_t ld_q, int64_t padding_index, int K, float* __restrict__ scores,
    float* __restrict__ pooled, int64_t ld_p, int* __restrict__ chosen, float* __restrict__ sel,
    int* __restrict__ sel_valid, const float* __restrict__ gpooled, int64_t ld_gp, const float* __restrict__ gsel,
    float* __restrict__ gkeys, float* __restrict__ gq, int* oob) {
  constexpr int TB = 8;
  extern __shared__ int ss_ids[];                          // [T*C]; -1 = out of range, -2 = padded step
  const int D = C * E;
  float* partial = reinterpret_cast<float*>(ss_ids + T * C);          // [4 waves][D]
  float* rank = partial + 4 * D;                           // forward: [T] ranked values
  int* pos = reinterpret_cast<int*>(rank);                 // backward: [T] j with chosen[b,j] == t, or -1
  int* ch = reinterpret_cast<int*>(rank + T);              // [SS_MAX_K] chosen positions
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = blockIdx.x;
  bool bad = false;
  for (int i = threadIdx.x; i < T * C; i += 256) {
    int t = i / C;
    int64_t id = series[(b * T) * C + i];
    int64_t id0 = series[(b * T + t) * C];
    bool ok = (uint64_t)id < (uint64_t)V;
    bool pad = id0 == padding_index;
    bad |= !ok;
    ss_ids[i] = pad ? -2 : (ok ? (int)id : -1);
  }
  if (!BWD && bad && oob) *oob = 1;
  if (BWD) {
    for (int t = threadIdx.x; t < T; t += 256) pos[t] = -1;
    __syncthreads();
    if (threadIdx.x < K) {
      int t = chosen[b * K + threadIdx.x];
      if (t >= 0 && t < T) pos[t] = threadIdx.x;
    }
  }
  __syncthreads();
  int rr[NPL], ee[NPL];
  float qv[NPL], gp[NPL], acc[NPL];
#pragma unroll
  for (int a = 0; a < NPL; ++a) {
    int d = lane + 64 * a;
    bool in = d < D;
    rr[a] = in ? d / E : 0;
    ee[a] = in ? d - rr[a] * E : 0;
    qv[a] = in ? q[b * ld_q + d] : 0.f;
    gp[a] = (BWD && in) ? gpooled[b * ld_gp + d] : 0.f;
    acc[a] = 0.f;
  }
  // the 4 waves take the chunks of TB steps round-robin, as ip_attn_kernel does
  for (int t0 = wave * TB; t0 < T; t0 += 4 * TB) {
    float k[TB][NPL];
    bool valid[TB];
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      int t = t0 + u;
      valid[u] = t < T && ss_ids[t * C] != -2;            // wave-uniform
#pragma unroll
      for (int a = 0; a < NPL; ++a) {
        k[u][a] = 0.f;
        if (valid[u] && lane + 64 * a < D) {
          int id = ss_ids[t * C + rr[a]];
          if (id >= 0) k[u][a] = embed[(int64_t)id * ld + ee[a]];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      int t = t0 + u;
      if (t >= T) break;
      float dot = 0.f;
      if (valid[u]) {
        float part = 0.f;
#pragma unroll
        for (int a = 0; a < NPL; ++a) part += (BWD ? gp[a] : qv[a]) * k[u][a];
        dot = group_sum<64>(part);
      }
      if (!BWD) {
        if (lane == 0) {
          scores[b * T + t] = dot;
          rank[t] = (valid[u] && dot == dot) ? dot : -INFINITY;     // a NaN score ranks with the padded steps
        }
#pragma unroll
        for (int a = 0; a < NPL; ++a) acc[a] += dot * k[u][a];
      } else {
        float s = valid[u] ? scores[b * T + t] : 0.f;
        const int j = pos[t];
#pragma unroll
        for (int a = 0; a < NPL; ++a) {
          acc[a] += dot * k[u][a];
          if (lane + 64 * a < D) {
            float g = s * gp[a] + dot * qv[a];
            if (gsel && j >= 0) g += gsel[(b * K + j) * D + lane + 64 * a];
            gkeys[(b * T + t) * D + lane + 64 * a] = g;
          }
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NPL; ++a)
    if (lane + 64 * a < D) partial[wave * D + lane + 64 * a] = acc[a];
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {
    float v = (partial[d] + partial[D + d]) + (partial[2 * D + d] + partial[3 * D + d]);
    if (!BWD) pooled[b * ld_p + d] = v;
    else gq[b * D + d] = v;
  }
  if (BWD) return;
  // K rounds of an arg-max by wave 0: greater value first, on equal values the lower index (K <= T: never runs dry)
  // (the butterfly leaves the same winner in every lane, so each lane keeps the list of taken positions in registers)
  if (wave == 0) {
    int took[SS_MAX_K];
#pragma unroll
    for (int i = 0; i < SS_MAX_K; ++i) took[i] = -1;
    for (int j = 0; j < K; ++j) {
      float bv = -INFINITY;
      int bt = INT32_MAX;
      for (int t = lane; t < T; t += 64) {
        bool taken = false;
#pragma unroll
        for (int i = 0; i < SS_MAX_K; ++i) taken |= took[i] == t;
        const float v = rank[t];
        if (!taken && (v > bv || (v == bv && t < bt))) { bv = v; bt = t; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int ot = __shfl_xor(bt, o, 64);
        if (ov > bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; }
      }
      if (bt >= T) bt = T - 1;                             // unreachable with K <= T; keeps every later index in range
#pragma unroll
      for (int i = 0; i < SS_MAX_K; ++i)
        if (i == j) took[i] = bt;
      if (lane == 0) ch[j] = bt;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * D; i += 256) {
    const int j = i / D, d = i - j * D;
    const int t = ch[j];
    const int64_t id = series[(b * T + t) * C + d / E];
    sel[(b * K + j) * D + d] = (uint64_t)id < (uint64_t)V ? embed[id * ld + d % E] : 0.f;
  }
  if (threadIdx.x < K) {
    const int t = ch[threadIdx.x];
    chosen[b * K + threadIdx.x] = t;
    sel_valid[b * K + threadIdx.x] = ss_ids[t * C] != -2 ? 1 : 0;
  }
}

int ss_check(int64_t ld, int64_t V, int E, int C, int64_t B, int T, int64_t ld_q, int K) {
  if (V <= 0 || E <= 0 || C <= 0 || B < 0 || T <= 0 || K <= 0) return REC_E_ARG;
  if (V > INT32_MAX || B > INT32_MAX || (int64_t)C * E > SS_MAX_D || K > SS_MAX_K ||
      ss_lds_bytes(T, C, C * E) > SS_LDS_CAP)
    return REC_E_UNSUPPORTED;
  if (ld < E || ld_q < (int64_t)C * E || K > T) return REC_E_ARG;
  return REC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// ESU attention
// ------------------------------------------------------------------------------------------------------------------
constexpr int ES_MAX_D = REC_ESU_MAX_D, ES_MAX_DK = REC_ESU_MAX_D, ES_MAX_H = REC_ESU_MAX_H;
constexpr int ES_MAX_K = REC_SEARCH_MAX_K;               // the keys are the positions a search selected
constexpr int ES_NTHR = 256;
constexpr size_t ES_LDS_CAP = REC_TILE_LDS_CAP;
using EsOps = TileOps<MB_T, MB_LD, ES_NTHR>;

struct EsDims {
  int K, D, H, dk;
  __host__ __device__ int HK() const { return H * dk; }
  __host__ __device__ int HD() const { return H * D; }
  __host__ __device__ int rowsA() const {                 // rows of the A operand buffer: the widest operand, made even
    int m = HK() > HD() ? HK() : HD();
    return mb_even(m > D ? m : D) + 2;
  }
  __host__ __device__ size_t lds_floats() const { return (size_t)MB_LD * (rowsA() + 2 * H * K + H); }
  __host__ __device__ int slot_floats() const { return D + 2 * HK(); }                  // dbo | dbv | dbq
  __host__ __device__ int small_floats() const { return 4 * D * HK() + HK(); }          // dWq | dWk | dWv | dWo | dbk
};

bool es_supported(const EsDims& d) {
  return d.D <= ES_MAX_D && d.dk <= ES_MAX_DK && d.H <= ES_MAX_H && d.K <= ES_MAX_K && !(d.D & 1) && !(d.dk & 1) &&
         sizeof(float) * d.lds_floats() <= ES_LDS_CAP;
}

struct EsWs {
  size_t Q, u, ctx, s, gctx, gs, gu, gQ, gc0, slots, part, total;
};
EsWs es_ws(int64_t B, const EsDims& d, bool bwd) {
  WsCarve c;
  EsWs w{};
  w.Q = c.take((size_t)B * d.HK());
  w.u = c.take((size_t)B * d.HD());
  w.ctx = c.take((size_t)B * d.HK());
  if (bwd) {
    w.s = c.take((size_t)B * d.HD());
    w.gctx = c.take((size_t)B * d.HK());
    w.gs = c.take((size_t)B * d.HD());
    w.gu = c.take((size_t)B * d.HD());
    w.gQ = c.take((size_t)B * d.HK());
    w.gc0 = c.take((size_t)B * d.H);
    w.slots = c.take((size_t)ceil_div64(B, MB_T) * d.slot_floats());
    w.part = c.take((size_t)mb_small_split(B) * d.small_floats());
  }
  w.total = c.at;
  return w;
}

struct EsWeights {
  const float *Wq, *bq, *Wk, *bk, *Wv, *bv, *Wo, *bo;
};

// what a tile's threads share: ids of the lane inside the MFMA tile and the tile's first example
struct EsTile {
  int tid, wave, lo, hi;
  int64_t r0, B;
};

// the accumulator of one 32 x 32 block: f(row, value) for the rows of the batch, when the lane's column exists
template <class Fn>
__device__ __forceinline__ void es_acc_out(const f32x16& acc, const EsTile& t, bool nok, Fn&& f) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mb_row(r, t.hi);
    if (nok && t.r0 + row < t.B) f(row, acc[r]);
  }
}

// dst[b, n] = (A . W + bias) * scale for the N <= 512 columns of W [Kd, N]; A: the tile's rows of src [B, ld_src]
template <bool TRANS>
__device__ __forceinline__ void es_wide(float* As, const EsTile& t, const float* __restrict__ src, int64_t ld_src,
                                        int Kd, const float* __restrict__ W, int64_t ldw, int N,
                                        const float* __restrict__ bias, float scale, float* __restrict__ dst,
                                        int64_t ld_dst, float* __restrict__ colsum) {
  EsOps::rows_in(As, src, t.r0, t.B, (int)ld_src, 0, Kd, t.tid);
  if (t.tid < MB_LD) As[Kd * MB_LD + t.tid] = 0.f;         // Kd is even: the row after the operand is never multiplied
  __syncthreads();
  if (colsum) EsOps::col_sums(colsum, As, Kd, t.tid);
  f32x16 acc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
  mb_mma<TRANS>(acc, As, Kd, W, ldw, 0, N, t.wave, t.lo, t.hi);
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int n = (t.wave + 4 * j) * 32 + t.lo;
    if ((t.wave + 4 * j) * 32 < N) {
      const bool nok = n < N;
      const float bn = (bias && nok) ? bias[n] : 0.f;
      es_acc_out(acc[j], t, nok, [&](int row, float v) { dst[(t.r0 + row) * ld_dst + n] = (v + bn) * scale; });
    }
  }
  __syncthreads();
}

// per head h: dst[b, h No + n] = A_h . Bm_h for n < No, A_h = As rows [h Kd, (h + 1) Kd) (already staged),
// Bm_h(k, n) = TRANS ? W[n ldw + h Kd + k] : W[k ldw + h No + n]; f(h, n, row, value) stores
template <bool TRANS, class Fn>
__device__ __forceinline__ void es_heads(const float* As, const EsTile& t, int H, int Kd, int No,
                                         const float* __restrict__ W, int64_t ldw, Fn&& f) {
  const int nb = (No + 31) / 32;
  for (int tk = t.wave; tk < H * nb; tk += 4) {
    const int h = tk / nb, n0 = (tk - h * nb) * 32;
    f32x16 acc;
    mb_zero(acc);
    mb_mma1<TRANS>(acc, As + h * Kd * MB_LD, Kd, TRANS ? W + h * Kd : W + h * No, ldw, 0, No, n0, t.lo, t.hi);
    const int n = n0 + t.lo;
    es_acc_out(acc, t, n < No, [&](int row, float v) { f(h, n, row, v); });
  }
}

// stage the tile's rows of src [B, ld] (n columns) as an A operand
__device__ __forceinline__ void es_stage(float* As, const EsTile& t, const float* __restrict__ src, int ld, int n) {
  EsOps::rows_in(As, src, t.r0, t.B, ld, 0, n, t.tid);
  __syncthreads();
}

// s_h = sum_j p_hj x_j into the A operand (and the workspace): element (b, h, d), d fastest
__device__ __forceinline__ void es_mix(float* As, const EsTile& t, const EsDims& d, const float* w,
                                       const float* __restrict__ x, float* __restrict__ dst) {
  const int HD = d.HD();
  for (int i = t.tid; i < MB_T * HD; i += ES_NTHR) {
    const int row = i / HD, hd = i - row * HD, h = hd / d.D, dd = hd - h * d.D;
    float v = 0.f;
    if (t.r0 + row < t.B) {
      const float* xb = x + (t.r0 + row) * d.K * d.D + dd;
      for (int j = 0; j < d.K; ++j) v += w[(h * d.K + j) * MB_LD + row] * xb[j * d.D];
      if (dst) dst[(t.r0 + row) * HD + hd] = v;
    }
    As[hd * MB_LD + row] = v;
  }
  __syncthreads();
}

// the forward's stages up to ctx; leaves Q, u, ctx in the workspace, p in ps (and probs), s in the workspace when given
__device__ __forceinline__ void es_forward(float* As, float* ps, float* c0s, const EsTile& t, const EsDims& d,
                                           const float* __restrict__ q, int64_t ld_q, const float* __restrict__ x,
                                           const int* __restrict__ mask, const EsWeights& w, float scale,
                                           float* __restrict__ Q, float* __restrict__ u, float* __restrict__ s,
                                           float* __restrict__ ctx, float* __restrict__ probs) {
  const int K = d.K, D = d.D, H = d.H, dk = d.dk, HK = d.HK(), HD = d.HD();
  es_wide<false>(As, t, q, ld_q, D, w.Wq, HK, HK, w.bq, scale, Q, HK, nullptr);
  es_stage(As, t, Q, HK, HK);
  for (int i = t.tid; i < MB_T * H; i += ES_NTHR) {        // c0 = <bk_h, Q_h>
    const int row = i / H, h = i - row * H;
    float v = 0.f;
    for (int c = 0; c < dk; ++c) v += w.bk[h * dk + c] * As[(h * dk + c) * MB_LD + row];
    c0s[h * MB_LD + row] = v;
  }
  es_heads<true>(As, t, H, dk, D, w.Wk, HK,
                 [&](int h, int n, int row, float v) { u[(t.r0 + row) * HD + h * D + n] = v; });
  __syncthreads();
  for (int i = t.tid; i < MB_T * H * K; i += ES_NTHR) {    // a_hj = l_hj + (1 - mask_j) * (-1e9)
    const int row = i / (H * K), hj = i - row * (H * K), h = hj / K, j = hj - h * K;
    float a = 0.f;
    if (t.r0 + row < t.B) {
      const float* xb = x + ((t.r0 + row) * K + j) * D;
      const float* ub = u + (t.r0 + row) * HD + h * D;
      float l = 0.f;
      for (int dd = 0; dd < D; ++dd) l += xb[dd] * ub[dd];
      l += c0s[h * MB_LD + row];
      const float m = mask[(t.r0 + row) * K + j] != 0 ? 1.f : 0.f;
      a = l + (1.f - m) * (-1e9f);
    }
    ps[hj * MB_LD + row] = a;
  }
  __syncthreads();
  for (int i = t.tid; i < MB_T * H; i += ES_NTHR) {
    const int row = i / H, h = i - row * H;
    float* p = ps + h * K * MB_LD + row;
    EsOps::softmax(p, p, K);
    if (probs && t.r0 + row < t.B)
      for (int j = 0; j < K; ++j) probs[((t.r0 + row) * H + h) * K + j] = p[j * MB_LD];
  }
  __syncthreads();
  es_mix(As, t, d, ps, x, s);
  es_heads<false>(As, t, H, D, dk, w.Wv, HK, [&](int h, int n, int row, float v) {
    ctx[(t.r0 + row) * HK + h * dk + n] = v + w.bv[h * dk + n];
  });
  __syncthreads();
}

__device__ __forceinline__ EsTile es_tile(int64_t B) {
  const int tid = threadIdx.x, lane = tid & 63;
  return {tid, tid >> 6, lane & 31, lane >> 5, (int64_t)blockIdx.x * MB_T, B};
}

__global__ __launch_bounds__(ES_NTHR) void esu_attn_fwd_kernel(const float* __restrict__ q, int64_t ld_q,
                                                               const float* __restrict__ x,
                                                               const int* __restrict__ mask, int64_t B, EsDims d,
                                                               EsWeights w, float scale, float* __restrict__ out,
                                                               float* __restrict__ probs, float* __restrict__ Q,
                                                               float* __restrict__ u, float* __restrict__ ctx) {
  extern __shared__ float es_lds[];
  float* As = es_lds;
  float* ps = As + d.rowsA() * MB_LD;
  float* c0s = ps + 2 * d.H * d.K * MB_LD;
  const EsTile t = es_tile(B);
  es_forward(As, ps, c0s, t, d, q, ld_q, x, mask, w, scale, Q, u, nullptr, ctx, probs);
  es_wide<false>(As, t, ctx, d.HK(), d.HK(), w.Wo, d.D, d.D, w.bo, 1.f, out, d.D, nullptr);
}

__global__ __launch_bounds__(ES_NTHR) void esu_attn_bwd_kernel(
    const float* __restrict__ q, int64_t ld_q, const float* __restrict__ x, const int* __restrict__ mask, int64_t B,
    EsDims d, EsWeights w, float scale, const float* __restrict__ gout, int64_t ld_go, float* __restrict__ gq,
    float* __restrict__ gx, float* __restrict__ Q, float* __restrict__ u, float* __restrict__ s,
    float* __restrict__ ctx, float* __restrict__ gctx, float* __restrict__ gs, float* __restrict__ gu,
    float* __restrict__ gQ, float* __restrict__ gc0, float* __restrict__ slots) {
  extern __shared__ float es_lds[];
  const int K = d.K, D = d.D, H = d.H, dk = d.dk, HK = d.HK(), HD = d.HD();
  float* As = es_lds;
  float* ps = As + d.rowsA() * MB_LD;
  float* gl = ps + H * K * MB_LD;
  float* c0s = gl + H * K * MB_LD;
  const EsTile t = es_tile(B);
  float* slot = slots + (int64_t)blockIdx.x * d.slot_floats();       // dbo [D] | dbv [HK] | dbq [HK]
  es_forward(As, ps, c0s, t, d, q, ld_q, x, mask, w, scale, Q, u, s, ctx, nullptr);
  // gctx = gout Wo^T; dbo = column sums of gout
  es_wide<true>(As, t, gout, ld_go, D, w.Wo, D, HK, nullptr, 1.f, gctx, HK, slot);
  // gs_h = gctx_h Wv_h^T; dbv = column sums of gctx
  es_stage(As, t, gctx, HK, HK);
  EsOps::col_sums(slot + D, As, HK, t.tid);
  es_heads<true>(As, t, H, dk, D, w.Wv, HK,
                 [&](int h, int n, int row, float v) { gs[(t.r0 + row) * HD + h * D + n] = v; });
  __syncthreads();
  // g_hj = <gs_h, x_j>, then the softmax Jacobian at p in place: dl_hj = p_hj (g_hj - <p_h, g_h>)
  for (int i = t.tid; i < MB_T * H * K; i += ES_NTHR) {
    const int row = i / (H * K), hj = i - row * (H * K), h = hj / K, j = hj - h * K;
    float g = 0.f;
    if (t.r0 + row < t.B) {
      const float* xb = x + ((t.r0 + row) * K + j) * D;
      const float* gb = gs + (t.r0 + row) * HD + h * D;
      for (int dd = 0; dd < D; ++dd) g += xb[dd] * gb[dd];
    }
    gl[hj * MB_LD + row] = g;
  }
  __syncthreads();
  for (int i = t.tid; i < MB_T * H; i += ES_NTHR) {
    const int row = i / H, h = i - row * H;
    float* g = gl + h * K * MB_LD + row;
    EsOps::softmax_bwd(ps + h * K * MB_LD + row, g, K);
    float c = 0.f;
    for (int j = 0; j < K; ++j) c += g[j * MB_LD];
    c0s[h * MB_LD + row] = c;                              // the gradient of <bk_h, Q_h>: zero in exact arithmetic
    if (t.r0 + row < t.B) gc0[(t.r0 + row) * H + h] = c;
  }
  __syncthreads();
  // gx_j = sum_h (p_hj gs_h + dl_hj u_h)
  for (int i = t.tid; i < MB_T * K * D; i += ES_NTHR) {
    const int row = i / (K * D), jd = i - row * (K * D), j = jd / D, dd = jd - j * D;
    if (t.r0 + row < t.B) {
      const float* gb = gs + (t.r0 + row) * HD + dd;
      const float* ub = u + (t.r0 + row) * HD + dd;
      float v = 0.f;
      for (int h = 0; h < H; ++h)
        v += ps[(h * K + j) * MB_LD + row] * gb[h * D] + gl[(h * K + j) * MB_LD + row] * ub[h * D];
      gx[(t.r0 + row) * K * D + jd] = v;
    }
  }
  // gu_h = sum_j dl_hj x_j;  gQ_h = (gu_h Wk_h + gc0_h bk_h) / sqrt(dk), the gradient of the raw projection
  es_mix(As, t, d, gl, x, gu);
  es_heads<false>(As, t, H, D, dk, w.Wk, HK, [&](int h, int n, int row, float v) {
    gQ[(t.r0 + row) * HK + h * dk + n] = (v + c0s[h * MB_LD + row] * w.bk[h * dk + n]) * scale;
  });
  __syncthreads();
  // gq = gQ Wq^T; dbq = column sums of gQ
  es_wide<true>(As, t, gQ, HK, HK, w.Wq, HK, D, nullptr, 1.f, gq, D, slot + D + HK);
}

// The 5 H small weight gradients in one launch: per head h, in the order of the packed partials
//   dWq[:, h, :] = q^T gQ_h    dWk[:, h, :] = gu_h^T Q_h    dWv[:, h, :] = s_h^T gctx_h    dWo[h] = ctx_h^T gout
//   dbk[h] = gc0_h^T Q_h
struct EsSmall {
  static constexpr int MAXK = ES_MAX_D > ES_MAX_DK ? ES_MAX_D : ES_MAX_DK;
  EsDims d;
  const float *q, *gout, *Q, *s, *ctx, *gctx, *gu, *gQ, *gc0;
  int ld_q, ld_go;
  __device__ SmallMat mat(int m) const {
    const int D = d.D, H = d.H, dk = d.dk, HK = d.HK(), HD = d.HD(), W = D * HK;
    const int h = m % H;
    switch (m / H) {
      case 0: return {q, ld_q, 0, D, gQ, HK, h * dk, dk, h * dk, HK};
      case 1: return {gu, HD, h * D, D, Q, HK, h * dk, dk, W + h * dk, HK};
      case 2: return {s, HD, h * D, D, gctx, HK, h * dk, dk, 2 * W + h * dk, HK};
      case 3: return {ctx, HK, h * dk, dk, gout, ld_go, 0, D, 3 * W + h * dk * D, D};
      default: return {gc0, H, h, 1, Q, HK, h * dk, dk, 4 * W + h * dk, dk};
    }
  }
};

int es_check(int64_t B, const EsDims& d) {
  if (B < 0 || d.K < 1 || d.D < 1 || d.H < 1 || d.dk < 1) return REC_E_ARG;
  if (B > INT32_MAX || !es_supported(d)) return REC_E_UNSUPPORTED;
  return REC_OK;
}

}  // namespace

extern "C" size_t rec_sim_search_lds_bytes(int T, int C, int E, int K) {
  if (ss_check(E, 1, E, C, 0, T, (int64_t)C * E, K) != REC_OK) return 0;
  return ss_lds_bytes(T, C, C * E);
}

extern "C" int rec_sim_search_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                      int64_t B, int T, const float* q, int64_t ld_q, int64_t padding_index, int K,
                                      float* scores, float* pooled, int64_t ld_pooled, int* chosen, float* sel,
                                      int* sel_valid, int* oob_flag, void* stream) {
  if (int rc = ss_check(ld, V, E, C, B, T, ld_q, K)) return rc;
  const int D = C * E;
  if (ld_pooled < D) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!embed || !series || !q || !scores || !pooled || !chosen || !sel || !sel_valid) return REC_E_ARG;
  const size_t lds = ss_lds_bytes(T, C, D);
  return rec_dispatch_1to4((D + 63) / 64, [&](auto npl) {
    hipLaunchKernelGGL((sim_search_kernel<decltype(npl)::value, false>), dim3((unsigned)B), dim3(256), lds,
                       as_stream(stream), embed, ld, V, E, C, series, B, T, q, ld_q, padding_index, K, scores, pooled,
                       ld_pooled, chosen, sel, sel_valid, nullptr, 0, nullptr, nullptr, nullptr, oob_flag);
    REC_LAUNCH_CHECK();
    return (int)REC_OK;
  });
}

extern "C" int rec_sim_search_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                      int64_t B, int T, const float* q, int64_t ld_q, int64_t padding_index, int K,
                                      const float* scores, const float* gpooled, int64_t ld_gpooled, const int* chosen,
                                      const float* gsel, float* gkeys, float* gq, void* stream) {
  if (int rc = ss_check(ld, V, E, C, B, T, ld_q, K)) return rc;
  const int D = C * E;
  if (ld_gpooled < D) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!embed || !series || !q || !scores || !gpooled || !chosen || !gkeys || !gq) return REC_E_ARG;
  const size_t lds = ss_lds_bytes(T, C, D);
  return rec_dispatch_1to4((D + 63) / 64, [&](auto npl) {
    hipLaunchKernelGGL((sim_search_kernel<decltype(npl)::value, true>), dim3((unsigned)B), dim3(256), lds,
                       as_stream(stream), embed, ld, V, E, C, series, B, T, q, ld_q, padding_index, K,
                       const_cast<float*>(scores), nullptr, 0, const_cast<int*>(chosen), nullptr, nullptr, gpooled,
                       ld_gpooled, gsel, gkeys, gq, nullptr);
    REC_LAUNCH_CHECK();
    return (int)REC_OK;
  });
}

extern "C" size_t rec_esu_attn_lds_bytes(int K, int D, int H, int dk) {
  const EsDims d{K, D, H, dk};
  return es_check(0, d) == REC_OK ? sizeof(float) * d.lds_floats() : 0;
}

extern "C" size_t rec_esu_attn_scratch_bytes(int64_t B, int K, int D, int H, int dk) {
  const EsDims d{K, D, H, dk};
  if (es_check(B, d) != REC_OK) return 0;
  return sizeof(float) * es_ws(B > 0 ? B : 1, d, true).total;
}

extern "C" int rec_esu_attn_fwd_f32(const float* q, int64_t ld_q, const float* x, const int* mask, int64_t B, int K,
                                    int D, int H, int dk, const float* Wq, const float* bq, const float* Wk,
                                    const float* bk, const float* Wv, const float* bv, const float* Wo, const float* bo,
                                    float* out, float* probs, void* workspace, size_t workspace_bytes, void* stream) {
  const EsDims d{K, D, H, dk};
  if (int rc = es_check(B, d)) return rc;
  if (ld_q < D) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!q || !x || !mask || !Wq || !bq || !Wk || !bk || !Wv || !bv || !Wo || !bo || !out || !workspace)
    return REC_E_ARG;
  const EsWs w = es_ws(B, d, false);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  if (hipError_t err = rec_allow_lds<esu_attn_fwd_kernel>(ES_LDS_CAP)) return (int)err;
  const float scale = (float)(1.0 / sqrt((double)dk));
  hipLaunchKernelGGL(esu_attn_fwd_kernel, dim3((unsigned)ceil_div64(B, MB_T)), dim3(ES_NTHR),
                     sizeof(float) * d.lds_floats(), as_stream(stream), q, ld_q, x, mask, B, d,
                     EsWeights{Wq, bq, Wk, bk, Wv, bv, Wo, bo}, scale, out, probs, base + w.Q, base + w.u, base + w.ctx);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_esu_attn_bwd_f32(const float* q, int64_t ld_q, const float* x, const int* mask, int64_t B, int K,
                                    int D, int H, int dk, const float* Wq, const float* bq, const float* Wk,
                                    const float* bk, const float* Wv, const float* bv, const float* Wo,
                                    const float* gout, int64_t ld_gout, float* gq, float* gx, float* dWq, float* dbq,
                                    float* dWk, float* dbk, float* dWv, float* dbv, float* dWo, float* dbo,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const EsDims d{K, D, H, dk};
  if (int rc = es_check(B, d)) return rc;
  if (ld_q < D || ld_gout < D) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!q || !x || !mask || !Wq || !bq || !Wk || !bk || !Wv || !bv || !Wo || !gout || !gq || !gx || !dWq || !dbq ||
      !dWk || !dbk || !dWv || !dbv || !dWo || !dbo || !workspace)
    return REC_E_ARG;
  const EsWs w = es_ws(B, d, true);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  if (hipError_t err = rec_allow_lds<esu_attn_bwd_kernel>(ES_LDS_CAP)) return (int)err;
  const float scale = (float)(1.0 / sqrt((double)dk));
  const int tiles = (int)ceil_div64(B, MB_T), HK = d.HK(), Wn = D * HK;
  hipLaunchKernelGGL(esu_attn_bwd_kernel, dim3((unsigned)tiles), dim3(ES_NTHR), sizeof(float) * d.lds_floats(), st, q,
                     ld_q, x, mask, B, d, EsWeights{Wq, bq, Wk, bk, Wv, bv, Wo, nullptr}, scale, gout, ld_gout, gq, gx,
                     base + w.Q, base + w.u, base + w.s, base + w.ctx, base + w.gctx, base + w.gs, base + w.gu,
                     base + w.gQ, base + w.gc0, base + w.slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, d.slot_floats(), tiles, base + w.slots, {{dbo, dbv, dbq}, {D, HK, HK}}, st))
    return rc;
  const EsSmall fam{d,          q,          gout,       base + w.Q,  base + w.s,   base + w.ctx, base + w.gctx,
                    base + w.gu, base + w.gQ, base + w.gc0, (int)ld_q, (int)ld_gout};
  if (int rc = small_dw_launch(fam, 5 * H, D * dk, d.small_floats(), B, base + w.part, st)) return rc;
  return rec_slot_sum(REC_SLOTS_SERIAL, d.small_floats(), mb_small_split(B), base + w.part,
                      {{dWq, dWk, dWv, dWo, dbk}, {Wn, Wn, Wn, Wn, HK}}, st);
}
