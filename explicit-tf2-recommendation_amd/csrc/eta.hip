// ETA (ETALayer, 7.SIM/CustomLayers.py:518-626) on gfx950: the SimHash search of the long behaviour series, one launch.
//
// TensorFlow cannot be imported next to this project, so this text is the definition.  D = E C.
//   key        k_t = concat_c embed[series[b,t,c]]; valid[b,t] = series[b,t,0] != padding_index (the first column alone);
//              an id outside [0, V) reads a zero row and sets *oob_flag
//   code       c(x)_j = sign(sum_d x_d Hm[d,j]) in {-1, 0, +1}, as tf.sign gives it in fp32: a zero projection gives 0, a
//              NaN projection gives NaN, which equals nothing (not even another NaN)
//   score      score[b,t] = #{ j < m : c(k_t)_j == c(q_b)_j }, an integer in [0, m], for every step, padded ones too
//   rank       score for a valid step, -inf for a padded one (the reference adds mask * (-inf), which is NaN for every
//              VALID step; the intent is kept, as the SIM search does)
//   chosen     argsort(rank, DESCENDING)[:, :K], on equal ranks the lower index first; it also orders the padded steps
//              when fewer than K are valid
//   sel        the K chosen keys [B,K,D] (a padded position's row too), sel_valid = valid[b, chosen], sel_ids the ids of
//              the chosen steps as given
// There is no backward kernel: Hm is frozen and sign has no gradient, so the only gradient is the one that arrives
// through sel, and that is the ordinary sparse row gradient over sel_ids.
//
// Layout.  One workgroup per example, min(256, T rounded up to 64) threads.  Hm is staged once in LDS as [D][MC], MC = 16
// or 32 columns, the columns past m zero.  A LANE OWNS A WHOLE STEP: it walks the step's C rows in the order of d, reads
// Hm wave-uniformly (an LDS broadcast) and keeps the MC projections in registers, acc_j = acc_j + x_d Hm[d,j] with the
// product rounded before the sum (fp contract off).  So a projection depends on the values of its row and of Hm only --
// never on t, the lane, T or the table's stride -- and steps with the same ids get the same codes bit for bit.  The
// three instantiations by row access (16 floats in flight as four 16-byte loads, one 16-byte load, one float) run the
// same operations in the same order (et_project of csrc/simhash.h, which csrc/sdim.hip shares).  The query's code is
// computed in every wave, lane j owning column j, with the same operations, and leaves the wave as three ballots.
// The three code planes of a step (positive, negative, NaN) are three
// 32-bit words; equality is one popcount.  The rank is packed with the position as (rank + 1) << 24 | (T - 1 - t) (0 in
// the upper part for a padded step), kept in LDS [T]; K rounds of an integer arg-max by wave 0 give chosen (the taken
// entry is overwritten by -1), then the K rows are gathered again (cache-hot).  No float atomics, no scratch.
//
// Limits, the header's: m <= REC_ETA_MAX_M, K <= REC_SEARCH_MAX_K, D <= REC_SEARCH_MAX_D, V and B < 2^31, and
// 4 (D MC + T + REC_SEARCH_MAX_K) <= REC_SEARCH_LDS_CAP bytes of LDS (T = 2048 at C = 3, E = 16 takes 11 KB; T = 15000
// fits at D = 48).
#include "simhash.h"

#pragma clang fp contract(off)

namespace {

constexpr int ET_MAX_M = REC_ETA_MAX_M, ET_MAX_K = REC_SEARCH_MAX_K, ET_MAX_D = REC_SEARCH_MAX_D;
constexpr int ET_TSHIFT = 24;                              // rank + 1 <= 33 above, T - 1 - t < 2^24 below
constexpr size_t ET_LDS_CAP = REC_SEARCH_LDS_CAP;
static_assert(ET_MAX_M <= 32 && ((int64_t)(ET_MAX_M + 1) << ET_TSHIFT) <= INT32_MAX,
              "a code plane is one 32-bit word, and the packed rank a positive int");
static_assert(sizeof(float) * (ET_MAX_D * 32 + ET_MAX_K) < ET_LDS_CAP,
              "the widest key's projection in 32 columns and the ET_MAX_K chosen positions leave LDS for the steps");

__host__ __device__ inline size_t et_lds_bytes(int T, int D, int m) {
  return sizeof(float) * ((size_t)D * et_mc(m) + (size_t)T + ET_MAX_K);
}

template <int MC, int CH>
__global__ __launch_bounds__(256) void eta_search_kernel(
    const float* __restrict__ embed, int64_t ld, int64_t V, int E, int C, const int64_t* __restrict__ series, int T,
    const float* __restrict__ q, int64_t ld_q, const float* __restrict__ Hm, int m, int64_t padding_index, int K,
    int* __restrict__ scores, int* __restrict__ chosen, float* __restrict__ sel, int* __restrict__ sel_valid,
    int64_t* __restrict__ sel_ids, int* oob) {
  extern __shared__ __attribute__((aligned(16))) float et_lds[];
  const int D = C * E;
  float* Hs = et_lds;                                      // [D][MC], columns >= m zero
  int* rank = reinterpret_cast<int*>(Hs + D * MC);         // [T] (rank + 1) << ET_TSHIFT | (T - 1 - t); -1 = taken
  int* ch = rank + T;                                      // [ET_MAX_K] chosen positions
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int64_t b = blockIdx.x;
  for (int i = tid; i < D * MC; i += nthr) {
    const int d = i / MC, j = i - d * MC;
    Hs[i] = j < m ? Hm[d * m + j] : 0.f;
  }
  // the query's code: lane j owns column j, d in the order the keys use
  const uint32_t mmask = m >= 32 ? 0xffffffffu : (1u << m) - 1u;
  float pq = 0.f;
  if (lane < m) {
    const float* qb = q + b * ld_q;
    for (int d = 0; d < D; ++d) pq = pq + qb[d] * Hm[d * m + lane];
  }
  const uint32_t qp = (uint32_t)__ballot(pq > 0.f) & mmask;
  const uint32_t qn = (uint32_t)__ballot(pq < 0.f) & mmask;
  const uint32_t qx = (uint32_t)__ballot(pq != pq) & mmask;
  __syncthreads();

  bool bad = false;
  for (int t = tid; t < T; t += nthr) {
    const int64_t* idp = series + (b * T + t) * C;
    const bool pad = idp[0] == padding_index;
    float acc[MC];
#pragma unroll
    for (int j = 0; j < MC; ++j) acc[j] = 0.f;
    et_project<MC, CH>(acc, bad, embed, ld, V, E, C, idp, Hs);
    uint32_t kp = 0, kn = 0, kx = 0;
#pragma unroll
    for (int j = 0; j < MC; ++j) {
      kp |= (acc[j] > 0.f ? 1u : 0u) << j;
      kn |= (acc[j] < 0.f ? 1u : 0u) << j;
      kx |= (acc[j] != acc[j] ? 1u : 0u) << j;
    }
    const int s = __popc(~(kp ^ qp) & ~(kn ^ qn) & ~(kx | qx) & mmask);
    if (scores) scores[b * T + t] = s;
    rank[t] = ((pad ? 0 : s + 1) << ET_TSHIFT) | (T - 1 - t);
  }
  if (bad && oob) *oob = 1;
  __syncthreads();

  // K rounds of an integer arg-max by wave 0 (K <= T: never runs dry).  The greater word is the greater rank and, on
  // equal ranks, the lower index; the lane that owns the winner marks it taken, and it is the lane that reads it again.
  if (tid < 64) {
    for (int j = 0; j < K; ++j) {
      int best = -1;
      for (int t = lane; t < T; t += 64) best = max(best, rank[t]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
      int bt = best >= 0 ? T - 1 - (best & ((1 << ET_TSHIFT) - 1)) : T - 1;     // best < 0 is unreachable with K <= T
      if ((bt & 63) == lane) rank[bt] = -1;
      if (lane == 0) ch[j] = bt;
    }
  }
  __syncthreads();
  for (int i = tid; i < K * D; i += nthr) {
    const int j = i / D, d = i - j * D, c = d / E;
    const int64_t id = series[(b * T + ch[j]) * C + c];
    sel[(b * K + j) * D + d] = (uint64_t)id < (uint64_t)V ? embed[id * ld + (d - c * E)] : 0.f;
  }
  for (int i = tid; i < K * C; i += nthr) {
    const int j = i / C, c = i - j * C;
    sel_ids[(b * K + j) * C + c] = series[(b * T + ch[j]) * C + c];
  }
  if (tid < K) {
    const int t = ch[tid];
    chosen[b * K + tid] = t;
    sel_valid[b * K + tid] = series[(b * T + t) * C] != padding_index ? 1 : 0;
  }
}

int et_check(int64_t ld, int64_t V, int E, int C, int64_t B, int T, int64_t ld_q, int m, int K) {
  if (V <= 0 || E <= 0 || C <= 0 || B < 0 || T <= 0 || m <= 0 || K <= 0) return REC_E_ARG;
  if (V > INT32_MAX || B > INT32_MAX || (int64_t)C * E > ET_MAX_D || m > ET_MAX_M || K > ET_MAX_K ||
      T >= (1 << ET_TSHIFT) || et_lds_bytes(T, C * E, m) > ET_LDS_CAP)
    return REC_E_UNSUPPORTED;
  if (ld < E || ld_q < (int64_t)C * E || K > T) return REC_E_ARG;
  return REC_OK;
}

template <int MC, int CH>
int et_launch(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B, int T,
              const float* q, int64_t ld_q, const float* Hm, int m, int64_t padding_index, int K, int* scores,
              int* chosen, float* sel, int* sel_valid, int64_t* sel_ids, int* oob_flag, void* stream) {
  if (hipError_t err = rec_allow_lds<eta_search_kernel<MC, CH>>(ET_LDS_CAP)) return (int)err;
  const int nthr = T >= 256 ? 256 : (T + 63) / 64 * 64;
  hipLaunchKernelGGL((eta_search_kernel<MC, CH>), dim3((unsigned)B), dim3(nthr), et_lds_bytes(T, C * E, m),
                     as_stream(stream), embed, ld, V, E, C, series, T, q, ld_q, Hm, m, padding_index, K, scores, chosen,
                     sel, sel_valid, sel_ids, oob_flag);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

}  // namespace

extern "C" size_t rec_eta_search_lds_bytes(int T, int C, int E, int m, int K) {
  if (et_check(E, 1, E, C, 0, T, (int64_t)C * E, m, K) != REC_OK) return 0;
  return et_lds_bytes(T, C * E, m);
}

extern "C" int rec_eta_search_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                      int64_t B, int T, const float* q, int64_t ld_q, const float* Hm, int m,
                                      int64_t padding_index, int K, int* scores, int* chosen, float* sel,
                                      int* sel_valid, int64_t* sel_ids, int* oob_flag, void* stream) {
  if (int rc = et_check(ld, V, E, C, B, T, ld_q, m, K)) return rc;
  if (B == 0) return REC_OK;
  if (!embed || !series || !q || !Hm || !chosen || !sel || !sel_valid || !sel_ids) return REC_E_ARG;
  // 16-byte loads where every row starts on a 16-byte boundary; the order of the operations is the same in all three
  const bool vec = E % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(embed) % 16 == 0;
#define ET_GO(MC, CH)                                                                                              \
  return et_launch<MC, CH>(embed, ld, V, E, C, series, B, T, q, ld_q, Hm, m, padding_index, K, scores, chosen, sel, \
                           sel_valid, sel_ids, oob_flag, stream)
  if (m <= 16) {
    if (vec && E % 16 == 0) ET_GO(16, 16);
    if (vec) ET_GO(16, 4);
    ET_GO(16, 1);
  }
  if (vec && E % 16 == 0) ET_GO(32, 16);
  if (vec) ET_GO(32, 4);
  ET_GO(32, 1);
#undef ET_GO
}
