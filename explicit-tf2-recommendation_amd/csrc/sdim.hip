// SDIM (SDIMLayer.generate_longterm_interest, once=True, 8.DMR/CustomLayers.py:816-841) on gfx950: the hash-bucket
// interest of the long behaviour series, one launch each way.
//
// TensorFlow cannot be imported next to this project, so this text is the definition.  D = E C; Hm is [D, G, m], frozen,
// row-major the [D, G m] of csrc/eta.hip.
//   key        k_l = concat_c embed[series[b,l,c]]; pad[b,l] = series[b,l,0] == padding_index (the first column alone);
//              an id outside [0, V) reads a zero row and sets *oob_flag
//   code       bit j of a row x's code is sum_d x_d Hm[d,j] > 0 (tf.where(sign == 1, 1, 0): a zero and a NaN projection
//              give 0).  The projection is et_project of csrc/simhash.h, the one csrc/eta.hip runs: d in order, the
//              product rounded before the sum, dependent on the values of the row and of Hm only, so equal ids give
//              equal codes bit for bit.  Group g's code is bits [g m, (g+1) m).
//   match      match[s,l,g] = code_g(k_l) == code_g(q[b,s,:])
//   flags      mode REC_SDIM_MODE_REFERENCE (0; the text as written: its mask is ids == padding_index, so it KEEPS the
//              padded rows and counts every step): w_l = pad[b,l], n_l = 1.  mode REC_SDIM_MODE_VALID (1; the paper's
//              intent): w_l = n_l = !pad[b,l].
//   sum        Sum[s,g,d] = sum_{l: match} float(w_l) k_l[d], added in INCREASING l from 0.f, each product and each sum
//              rounded to fp32; cnt[s,g] = sum_{l: match} n_l, an integer
//   mean       mean[s,g,d] = Sum / float(cnt), replaced by 0 where that is not finite (the empty bucket's 0 / 0 and a
//              non-finite sum: tf.where(is_finite))
//   out        out[b,s,d] = (mean[s,0,d] + mean[s,1,d] + ... in increasing g) / float(G)
// Backward.  sign and one_hot carry no gradient, so q and Hm receive none.  The series receives, WRITTEN and never added
// to -- the IndexedSlices values of the one series lookup --
//   gkeys[b,l,d] = sum over s, then over g, from 0.f, of match[s,l,g] ((gout[b,s,d] / float(G)) / float(cnt[s,g]))
// for a step with w_l = 1 and +0 for a step with w_l = 0 (the product with the sum is not formed: in mode 1 a padded step
// may match a bucket with cnt = 0).  A step with w_l = 1 that matches has n_l = 1 in both modes, so cnt >= 1 there.  For an
// element whose bucket sum was not finite the reference's gradient is zero; here that element's gradient is UNDEFINED
// (the forward saves no mask of them).  The backward reads the forward's codes [B,T], qcodes [B,S] and cnt [B,S,G] and
// neither embed nor Hm.
//
// Layout.  One workgroup of 256 threads per example.  Forward: Hm is staged in LDS as [D][MC], MC = 16 or 32 columns; a
// LANE OWNS A WHOLE STEP for the projections (an LDS broadcast per row of Hm), packs the signs into one word, LDS [T],
// and the wave's ballot of pad goes to a bit map; wave w computes the codes of candidates w, w + 4, ..: lane j owns
// column j and the code leaves the wave as one ballot.  Then, MC / G candidates at a time, A WAVE OWNS A BUCKET (s,g): it
// compacts the matching steps, in the order of l, into a list of its own in LDS (ballots and popcounts, which also
// give cnt) and walks that list with lane = d: every lane reads the same row (one coalesced request, cache-hot), eight
// steps' ids and then their floats in flight, added in the order of the list.  The means land in the LDS that held Hm,
// and thread (s,d) adds them in the order of g.  (A thread per (s,g,d) walking the codes themselves would pay one
// dependent id-then-row round trip per matching step; the list makes the loads independent.)  Backward: the candidates'
// gout / G, float(cnt) and codes are staged in LDS; a thread owns a step and four (or one) of its columns, walks s,
// then g, and stores 16 bytes.  No float atomics, no scratch: bit-identical from run to run.
//
// Limits, the header's: G m <= REC_SDIM_MAX_BITS, S <= REC_SDIM_MAX_S, D <= REC_SEARCH_MAX_D, V and B < 2^31, and
// 4 (D MC + T + 2 ceil(T / 64) + REC_SDIM_MAX_S + 2 (T + T mod 2)) <= REC_SEARCH_LDS_CAP bytes of LDS (T = 2048 at
// C = 3, E = 16, G = 4, m = 3 takes 27 KB; T = 5000 fits at D = 48).  T < 65536 is checked too (the lists' 16-bit
// entries); the LDS rule is the stricter one, as the static_assert below holds it to be.
#include "simhash.h"

#pragma clang fp contract(off)

namespace {

constexpr int SD_MAX_BITS = REC_SDIM_MAX_BITS, SD_MAX_S = REC_SDIM_MAX_S, SD_MAX_D = REC_SEARCH_MAX_D;
constexpr int SD_THREADS = 256, SD_WAVES = SD_THREADS / 64;
constexpr int SD_FLIGHT = 8;                               // steps whose rows a lane has in flight during the walk
constexpr size_t SD_LDS_CAP = REC_SEARCH_LDS_CAP;
static_assert(SD_MAX_BITS <= 32, "the codes of all groups are packed into one 32-bit word");
static_assert(SD_LDS_CAP / sizeof(float) < (1 << 16),
              "a series whose codes [T] fit the launch cap has T < 65536: a step fits a 16-bit list entry");
static_assert(sizeof(float) * (SD_MAX_D * 32 + SD_MAX_S) < SD_LDS_CAP,
              "the widest key's projection in 32 columns and the SD_MAX_S candidates' codes leave LDS for the steps");

__host__ __device__ inline size_t sd_lds_bytes(int T, int D, int G, int m) {
  const size_t Tp = ((size_t)T + 1) & ~(size_t)1;          // a wave's list: Tp 16-bit entries
  return sizeof(float) * ((size_t)D * et_mc(G * m) + (size_t)T + 2 * (((size_t)T + 63) / 64) + SD_MAX_S +
                          SD_WAVES * Tp / 2);
}

__device__ __forceinline__ bool sd_pad(const uint32_t* padw, int l) { return (padw[l >> 5] >> (l & 31)) & 1u; }

template <int MC, int CH>
__global__ __launch_bounds__(SD_THREADS) void sdim_interest_fwd_kernel(
    const float* __restrict__ embed, int64_t ld, int64_t V, int E, int C, const int64_t* __restrict__ series, int T,
    const float* __restrict__ q, int64_t ld_q, int S, const float* __restrict__ Hm, int G, int m, int64_t padding_index,
    int mode, float* __restrict__ out, int* __restrict__ codes, int* __restrict__ qcodes, int* __restrict__ cnt,
    int* oob) {
  extern __shared__ __attribute__((aligned(16))) float sd_lds[];
  const int D = C * E, GM = G * m, NW = (T + 63) / 64, Tp = (T + 1) & ~1;
  float* Hs = sd_lds;                                               // [D][MC], columns >= G m zero; later the means
  uint32_t* code = reinterpret_cast<uint32_t*>(Hs + D * MC);        // [T] the steps' packed codes
  uint32_t* padw = code + T;                                        // [2 NW] bit l: pad[b,l]
  uint32_t* qc = padw + 2 * NW;                                     // [SD_MAX_S] the candidates' packed codes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint16_t* list = reinterpret_cast<uint16_t*>(qc + SD_MAX_S) + wave * Tp;     // [Tp] this wave's matching steps
  const int64_t b = blockIdx.x;
  for (int i = tid; i < D * MC; i += SD_THREADS) {
    const int d = i / MC, j = i - d * MC;
    Hs[i] = j < GM ? Hm[d * GM + j] : 0.f;
  }
  __syncthreads();

  // the candidates' codes: lane j owns column j, d in the order the keys use
  const uint32_t allmask = GM >= 32 ? 0xffffffffu : (1u << GM) - 1u;
  for (int s = wave; s < S; s += SD_WAVES) {
    float pq = 0.f;
    if (lane < GM) {
      const float* qs = q + (b * S + s) * ld_q;
      for (int d = 0; d < D; ++d) pq = pq + qs[d] * Hs[d * MC + lane];
    }
    const uint32_t c = (uint32_t)__ballot(pq > 0.f) & allmask;
    if (lane == 0) {
      qc[s] = c;
      qcodes[b * S + s] = (int)c;
    }
  }
  // the steps' codes: a lane owns a step
  bool bad = false;
  for (int base = 0; base < T; base += SD_THREADS) {
    const int t = base + tid;
    bool pad = false;
    if (t < T) {
      const int64_t* idp = series + (b * T + t) * C;
      pad = idp[0] == padding_index;
      float acc[MC];
#pragma unroll
      for (int j = 0; j < MC; ++j) acc[j] = 0.f;
      et_project<MC, CH>(acc, bad, embed, ld, V, E, C, idp, Hs);
      uint32_t kc = 0;
#pragma unroll
      for (int j = 0; j < MC; ++j) kc |= (acc[j] > 0.f ? 1u : 0u) << j;
      code[t] = kc;
      codes[b * T + t] = (int)kc;
    }
    const uint64_t pb = __ballot(pad);
    const int wi = (base >> 6) + wave;                              // this wave's steps are 64 wi .. 64 wi + 63
    if (lane == 0 && wi < NW) {
      padw[2 * wi] = (uint32_t)pb;
      padw[2 * wi + 1] = (uint32_t)(pb >> 32);
    }
  }
  if (bad && oob) *oob = 1;
  __syncthreads();                                                  // Hs is free from here on

  // MC / G >= 1 candidates at a time: their G D means fit where Hm was.  Every wave runs every trip of the loops
  // (the barriers), with or without a bucket of its own.
  const uint32_t gmask = m >= 32 ? 0xffffffffu : (1u << m) - 1u;
  const int SB = MC / G, GD = G * D;
  const int64_t* ser = series + b * T * C;
  for (int s0 = 0; s0 < S; s0 += SB) {
    const int ns = min(SB, S - s0), np = ns * G;
    for (int p0 = 0; p0 < np; p0 += SD_WAVES) {
      const int p = p0 + wave, sl = p / G, g = p - sl * G, s = s0 + sl;
      const bool own = p < np;
      int n = 0, counted = 0;
      if (own) {                                                    // the bucket's steps, in the order of l
        const uint32_t qx = qc[s];
        const int sh = g * m;
        for (int base = 0; base < T; base += 64) {
          const int l = base + lane;
          const bool hit = l < T && (((code[l] ^ qx) >> sh) & gmask) == 0u;
          const uint64_t hits = __ballot(hit);
          if (hit) list[n + __popcll(hits & ((1ull << lane) - 1ull))] = (uint16_t)l;
          counted += __popcll(__ballot(hit && (mode == REC_SDIM_MODE_REFERENCE || !sd_pad(padw, l))));
          n += __popcll(hits);
        }
        if (lane == 0) cnt[(b * S + s) * G + g] = counted;
      }
      __syncthreads();                                              // the list is written
      if (own) {
        const float fc = (float)counted;
        for (int d = lane; d < D; d += 64) {
          const int c = d / E, e = d - c * E;
          float acc = 0.f;
          for (int i0 = 0; i0 < n; i0 += SD_FLIGHT) {
            int64_t id[SD_FLIGHT];
            float x[SD_FLIGHT], w[SD_FLIGHT];
#pragma unroll
            for (int u = 0; u < SD_FLIGHT; ++u) {
              const int l = list[min(i0 + u, n - 1)];               // past the end: the last step again, not added
              id[u] = ser[(int64_t)l * C + c];
              w[u] = sd_pad(padw, l) == (mode == REC_SDIM_MODE_REFERENCE) ? 1.f : 0.f;
            }
#pragma unroll
            for (int u = 0; u < SD_FLIGHT; ++u) x[u] = (uint64_t)id[u] < (uint64_t)V ? embed[id[u] * ld + e] : 0.f;
#pragma unroll
            for (int u = 0; u < SD_FLIGHT; ++u)
              if (i0 + u < n) acc = acc + w[u] * x[u];
          }
          const float mean = acc / fc;
          Hs[sl * GD + g * D + d] = __builtin_isfinite(mean) ? mean : 0.f;
        }
      }
      __syncthreads();                                              // the list is read (and, at the end, the means written)
    }
    for (int i = tid; i < ns * D; i += SD_THREADS) {
      const int sl = i / D, d = i - sl * D;
      float a = Hs[sl * GD + d];
      for (int g = 1; g < G; ++g) a = a + Hs[sl * GD + g * D + d];
      out[(b * S + s0 + sl) * D + d] = a / (float)G;
    }
    __syncthreads();
  }
}

// VW columns of a step per thread: 4 (one 16-byte store) or 1
template <int VW>
__global__ __launch_bounds__(SD_THREADS) void sdim_interest_bwd_kernel(
    const int64_t* __restrict__ series, int C, int T, int D, int G, int m, int S, int64_t padding_index, int mode,
    const int* __restrict__ codes, const int* __restrict__ qcodes, const int* __restrict__ cnt,
    const float* __restrict__ gout, int64_t ld_gout, float* __restrict__ gkeys) {
  extern __shared__ __attribute__((aligned(16))) float sd_lds[];
  float* gd = sd_lds;                                               // [S][D] gout / float(G)
  float* cf = gd + S * D;                                           // [S][G] float(cnt)
  uint32_t* qc = reinterpret_cast<uint32_t*>(cf + S * G);           // [S]
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  for (int i = tid; i < S * D; i += SD_THREADS) {
    const int s = i / D, d = i - s * D;
    gd[i] = gout[(b * S + s) * ld_gout + d] / (float)G;
  }
  for (int i = tid; i < S * G; i += SD_THREADS) cf[i] = (float)cnt[b * S * G + i];
  if (tid < S) qc[tid] = (uint32_t)qcodes[b * S + tid];
  __syncthreads();
  const uint32_t gmask = m >= 32 ? 0xffffffffu : (1u << m) - 1u;
  const int DV = D / VW, per = SD_THREADS / DV;                     // DV <= 256 threads cover a step, `per` steps a trip
  const int ls = tid / DV, d0 = (tid - ls * DV) * VW;
  if (ls >= per) return;
  for (int l = ls; l < T; l += per) {
    const bool pad = series[(b * T + l) * C] == padding_index;
    float acc[VW];
#pragma unroll
    for (int v = 0; v < VW; ++v) acc[v] = 0.f;
    if (pad == (mode == REC_SDIM_MODE_REFERENCE)) {
      const uint32_t kc = (uint32_t)codes[b * T + l];
      for (int s = 0; s < S; ++s) {
        const uint32_t x = kc ^ qc[s];
        for (int g = 0; g < G; ++g)
          if (((x >> (g * m)) & gmask) == 0u) {
            const float f = cf[s * G + g];
#pragma unroll
            for (int v = 0; v < VW; ++v) acc[v] = acc[v] + gd[s * D + d0 + v] / f;
          }
      }
    }
    float* dst = gkeys + (b * T + l) * D + d0;
    if constexpr (VW == 4) {
      *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      dst[0] = acc[0];
    }
  }
}

// the sizes alone, in the documented order; ld, ld_q / ld_gout: pass the least valid value where there is none
int sd_check(int64_t ld, int64_t V, int E, int C, int64_t B, int T, int64_t ld_q, int G, int m, int S, int mode) {
  if (V <= 0 || E <= 0 || C <= 0 || B < 0 || T <= 0 || G <= 0 || m <= 0 || S <= 0) return REC_E_ARG;
  if (V > INT32_MAX || B > INT32_MAX || (int64_t)C * E > SD_MAX_D || (int64_t)G * m > SD_MAX_BITS || S > SD_MAX_S ||
      T >= (1 << 16) || sd_lds_bytes(T, C * E, G, m) > SD_LDS_CAP)
    return REC_E_UNSUPPORTED;
  if (ld < E || ld_q < (int64_t)C * E || (mode != REC_SDIM_MODE_REFERENCE && mode != REC_SDIM_MODE_VALID))
    return REC_E_ARG;
  return REC_OK;
}

template <int MC, int CH>
int sd_launch(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B, int T,
              const float* q, int64_t ld_q, int S, const float* Hm, int G, int m, int64_t padding_index, int mode,
              float* out, int* codes, int* qcodes, int* cnt, int* oob_flag, void* stream) {
  if (hipError_t err = rec_allow_lds<sdim_interest_fwd_kernel<MC, CH>>(SD_LDS_CAP)) return (int)err;
  hipLaunchKernelGGL((sdim_interest_fwd_kernel<MC, CH>), dim3((unsigned)B), dim3(SD_THREADS),
                     sd_lds_bytes(T, C * E, G, m), as_stream(stream), embed, ld, V, E, C, series, T, q, ld_q, S, Hm, G,
                     m, padding_index, mode, out, codes, qcodes, cnt, oob_flag);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

}  // namespace

extern "C" size_t rec_sdim_lds_bytes(int T, int C, int E, int G, int m, int S) {
  if (sd_check(E, 1, E, C, 0, T, (int64_t)C * E, G, m, S, 0) != REC_OK) return 0;
  return sd_lds_bytes(T, C * E, G, m);
}

extern "C" int rec_sdim_interest_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series,
                                         int64_t B, int T, const float* q, int64_t ld_q, int S, const float* Hm, int G,
                                         int m, int64_t padding_index, int mode, float* out, int* codes, int* qcodes,
                                         int* cnt, int* oob_flag, void* stream) {
  if (int rc = sd_check(ld, V, E, C, B, T, ld_q, G, m, S, mode)) return rc;
  if (B == 0) return REC_OK;
  if (!embed || !series || !q || !Hm || !out || !codes || !qcodes || !cnt) return REC_E_ARG;
  // 16-byte loads where every row starts on a 16-byte boundary; the order of the operations is the same in all three
  const bool vec = E % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(embed) % 16 == 0;
#define SD_GO(MC, CH)                                                                                               \
  return sd_launch<MC, CH>(embed, ld, V, E, C, series, B, T, q, ld_q, S, Hm, G, m, padding_index, mode, out, codes, \
                           qcodes, cnt, oob_flag, stream)
  if (G * m <= 16) {
    if (vec && E % 16 == 0) SD_GO(16, 16);
    if (vec) SD_GO(16, 4);
    SD_GO(16, 1);
  }
  if (vec && E % 16 == 0) SD_GO(32, 16);
  if (vec) SD_GO(32, 4);
  SD_GO(32, 1);
#undef SD_GO
}

extern "C" int rec_sdim_interest_bwd_f32(const int64_t* series, int E, int C, int64_t B, int T, int G, int m, int S,
                                         int64_t padding_index, int mode, const int* codes, const int* qcodes,
                                         const int* cnt, const float* gout, int64_t ld_gout, float* gkeys,
                                         void* stream) {
  if (int rc = sd_check(E, 1, E, C, B, T, ld_gout, G, m, S, mode)) return rc;
  if (B == 0) return REC_OK;
  if (!series || !codes || !qcodes || !cnt || !gout || !gkeys) return REC_E_ARG;
  const int D = C * E;
  const size_t lds = sizeof(float) * ((size_t)S * D + (size_t)S * G + S);
  // 16-byte stores where every step's row starts on a 16-byte boundary; the operations are the same in both
  if (D % 4 == 0 && rec_is_aligned16(gkeys))
    hipLaunchKernelGGL(sdim_interest_bwd_kernel<4>, dim3((unsigned)B), dim3(SD_THREADS), lds, as_stream(stream), series,
                       C, T, D, G, m, S, padding_index, mode, codes, qcodes, cnt, gout, ld_gout, gkeys);
  else
    hipLaunchKernelGGL(sdim_interest_bwd_kernel<1>, dim3((unsigned)B), dim3(SD_THREADS), lds, as_stream(stream), series,
                       C, T, D, G, m, S, padding_index, mode, codes, qcodes, cnt, gout, ld_gout, gkeys);
  REC_LAUNCH_CHECK();
  return REC_OK;
}
