// ContextNet (ContextualEmbeddingLayer / NonLinearFeedforwardLayer / ContextNetBlockLayer / ContextNetLayer,
// 11.FiBiNet++/CustomLayers.py:412-531) on gfx950.
//
// Input stage, fused with the lookup.  X int64 [B, F], F = Fc + Fk with the Fk key columns LAST, values [B, Fk]:
//   x[b,f,:] = table[X[b,f]]  (f < Fc)      x[b,Fc+j,:] = table[X[b,Fc+j]] * values[b,j]
// 16 adjacent lanes share a row.  The backward scales the key fields' gradient rows by their value and writes them in the
// order of X.  It is MaskNet's input stage without the LayerNorm.
//
// Block, one launch each way.  x [B, F, E], D = F E, H = R D:
//   h = relu(flat(x) Wa + ba)   m = h Wb + bb   u = x (.) m
//   pointwise: a_f = relu(u_f W1_f)   r_f = a_f W2_f + u_f        single: r_f = u_f W1_f        y_f = LayerNorm_f(r_f)
// The front half is the mask block's (mfma_tile.h): a workgroup of 4 waves owns 32 examples, h is produced in chunks of
// 128 columns on v_mfma_f32_32x32x2_f32 and consumed at once into the m accumulators; it goes to HBM only when the
// caller asks for it.  u replaces the x tile in LDS ([D][33], k-major).  The per-field products are about 3 % of a
// block's flops and run on the VALU out of LDS: thread t owns example t & 31 and the columns t / 32, t / 32 + 8, ... of a
// pass; the 32 lanes of a half wave read 32 consecutive banks of the tile and ONE weight (a broadcast load).  A pass
// covers whole fields of at most 128 columns, so a lives in the h chunk's LDS and r overwrites u in place (a thread reads
// the u of other columns only before the barrier that follows a).  The LayerNorm takes its statistics per (example,
// field) out of LDS, and y, xhat, a leave LDS in rows of consecutive columns.  Training saves h, m, xhat, rstd and (in
// pointwise mode) a; u is recomputed.
// The backward runs the per-example chain of a tile in one launch: LayerNorm backward per field in place, da = (dr W2^T)
// (.) [a > 0], du = dr + da W1^T (single: du = dr W1^T), dm = du (.) x, the direct part du (.) m kept in LDS, dh = (dm
// Wb^T) (.) [h > 0] in chunks consumed at once into dx += dh Wa^T.  It writes dr, da, u, dm and dh to the workspace and
// the column sums of its tile (dgamma, dbeta, dbb, dba) to the tile's slot; the entry point then adds the slots
// (rec_slot_sum), runs the F (2 F) per-field weight gradients dW1_f = u_f^T da_f, dW2_f = a_f^T dr_f as ONE launch over
// (field, matrix, batch slice) whose at most 16 slices are added in order, and enqueues dWa = x^T dh, dWb = h^T dm on
// rec_gemm_f32 (split-K, slices added in order).  No float atomics and no value with two writers: bit-identical results
// run to run; no host synchronisation.
// Contraction is off in this file as in masknet.hip: a LayerNorm over ONE element (E = 1) must return exactly zero
// gradients, which g gamma - mean(g gamma) only does when both are the same rounded product.
// Shared with the other tile kernels, in tile_ops.h: the row pass out of an LDS operand (TileOps), the batch slices of
// the per-field weight-gradient launch, the workspace carving and the split-K weight-gradient GEMM; the MFMA tile itself
// is mfma_tile.h.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

namespace {

// the limits are MaskNet's: the header gains no constant for this family
constexpr int CN_MAXF = REC_MASKNET_MAX_F, CN_MAXE = REC_MASKNET_MAX_E, CN_MAXD = REC_MASKNET_MAX_D;
constexpr int CN_MAXR = REC_MASKNET_MAX_R;
constexpr float CN_EPS = 1e-3f;                  // tf.keras.layers.LayerNormalization()
constexpr int CN_NTHR = 256;
constexpr int CN_G = CN_NTHR / MB_T;             // column groups of the per-field stages
constexpr int CN_IN_GRID = 4096;
constexpr int CN_DW_ROWS = 32;                   // examples of one step of the per-field weight gradients

static_assert(CN_MAXD <= 128 * MB_NJ, "accumulator blocks per wave");
static_assert(2 * CN_MAXF <= MB_HC, "the LayerNorm statistics of a tile live in the h chunk");
static_assert(CN_MAXE <= MB_HC, "a pass of the per-field stages holds at least one field");

// ------------------------------------------------------------------------------------------------------------------
// input stage
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CN_NTHR) void emb_contextnet_in_fwd_kernel(const float* __restrict__ table, int64_t V, int E,
                                                                        int64_t ld, const int64_t* __restrict__ X,
                                                                        const float* __restrict__ values, int64_t rows,
                                                                        int F, int Fk, float* __restrict__ x, int* oob) {
  const int l = threadIdx.x & 15, Fc = F - Fk;
  bool bad = false;
  for (int64_t r = (int64_t)blockIdx.x * (CN_NTHR / 16) + (threadIdx.x >> 4); r < rows;
       r += (int64_t)gridDim.x * (CN_NTHR / 16)) {
    const int64_t b = r / F;
    const int f = (int)(r - b * F);
    const int64_t id = X[r];
    const bool ok = (uint64_t)id < (uint64_t)V;
    bad |= !ok;
    const bool cont = f >= Fc;
    const float scale = cont ? values[b * Fk + (f - Fc)] : 1.f;
    for (int e = l; e < E; e += 16) {
      float t = ok ? table[id * ld + e] : 0.f;
      if (cont) t *= scale;
      x[r * E + e] = t;
    }
  }
  if (bad && oob) *oob = 1;
}

__global__ __launch_bounds__(CN_NTHR) void emb_contextnet_in_bwd_kernel(const float* __restrict__ values,
                                                                        const float* __restrict__ dx, int64_t rows, int F,
                                                                        int Fk, int E, float* __restrict__ vals) {
  const int l = threadIdx.x & 15, Fc = F - Fk;
  for (int64_t r = (int64_t)blockIdx.x * (CN_NTHR / 16) + (threadIdx.x >> 4); r < rows;
       r += (int64_t)gridDim.x * (CN_NTHR / 16)) {
    const int64_t b = r / F;
    const int f = (int)(r - b * F);
    const bool cont = f >= Fc;
    const float scale = cont ? values[b * Fk + (f - Fc)] : 1.f;
    for (int e = l; e < E; e += 16) {
      const float g = dx[r * E + e];
      vals[r * E + e] = cont ? g * scale : g;
    }
  }
}

static int cn_in_shape(int64_t B, int F, int Fk, int E) {
  if (B < 0 || F < 1 || E < 1 || Fk < 0 || Fk > F) return REC_E_ARG;
  if (F > CN_MAXF || E > CN_MAXE || (int64_t)F * E > CN_MAXD || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;                    // the family has one set of limits, the blocks' F E among them
  return REC_OK;
}
static int cn_in_grid(int64_t rows) {
  const int64_t g = ceil_div64(rows, CN_NTHR / 16);
  return (int)(g < CN_IN_GRID ? g : CN_IN_GRID);
}

// ------------------------------------------------------------------------------------------------------------------
// block
// ------------------------------------------------------------------------------------------------------------------
// sum_e src(f E + e, b) W_f(e, j) for a k-major LDS operand whose row 0 is column col0 of the tile;
// W_f(e, j) = TRANS ? W[f][j][e] : W[f][e][j]
template <bool TRANS>
__device__ __forceinline__ float cn_dot(const float* src, int col0, const float* __restrict__ W, int f, int j, int E,
                                        int b) {
  const float* s = src + (f * E - col0) * MB_LD + b;
  const float* w = W + (int64_t)f * E * E + (TRANS ? j * E : j);
  const int ws = TRANS ? 1 : E;
  float acc = 0.f;
  for (int e = 0; e < E; ++e) acc = fmaf(s[e * MB_LD], w[e * ws], acc);
  return acc;
}

using Tile = TileOps<MB_T, MB_LD, CN_NTHR>;

// floats of LDS: forward  xs / us [even(D)][33] | hs [128][33]
//                backward two tiles [even(D)][33] | chunk [128][33]
__host__ __device__ inline size_t cn_lds_floats(int D, int bwd) {
  return (size_t)((bwd ? 2 : 1) * mb_even(D) + MB_HC) * MB_LD;
}
constexpr size_t CN_LDS_CAP = REC_POSO_LDS_CAP;
static_assert(sizeof(float) * (2 * CN_MAXD + MB_HC) * MB_LD <= CN_LDS_CAP && CN_LDS_CAP <= REC_LDS_CU_BYTES,
              "the backward of the largest block fits the LDS of a CU");

__global__ __launch_bounds__(CN_NTHR) void contextnet_block_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ Wa, const float* __restrict__ ba,
    const float* __restrict__ Wb, const float* __restrict__ bb, const float* __restrict__ W1,
    const float* __restrict__ W2, const float* __restrict__ gamma, const float* __restrict__ beta, int64_t B, int F,
    int E, int H, int pointwise, float* __restrict__ y, float* __restrict__ save_h, float* __restrict__ save_m,
    float* __restrict__ save_xhat, float* __restrict__ save_rstd, float* __restrict__ save_a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = F * E, De = mb_even(D);
  float* xs = lds;                               // [De][33]: the x tile, then u, then r
  float* hs = xs + De * MB_LD;                   // [128][33]: a chunk of h, then of a, then the LayerNorm statistics
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;

  for (int i = tid; i < MB_T * De; i += CN_NTHR) {
    const int m = i / De, k = i - m * De;
    xs[k * MB_LD + m] = (k < D && r0 + m < B) ? x[(r0 + m) * D + k] : 0.f;
  }
  __syncthreads();

  f32x16 macc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(macc[j]);

  for (int c0 = 0; c0 < H; c0 += MB_HC) {
    const int col = c0 + 32 * wave + lo;
    f32x16 hacc;
    mb_zero(hacc);
    if (c0 + 32 * wave < H) mb_mma1<false>(hacc, xs, D, Wa, H, 0, H, c0 + 32 * wave, lo, hi);
    const float bc = col < H ? ba[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mb_row(r, hi);
      const float hv = col < H ? fmaxf(hacc[r] + bc, 0.f) : 0.f;
      hs[(32 * wave + lo) * MB_LD + row] = hv;
      if (save_h && col < H && r0 + row < B) save_h[(r0 + row) * H + col] = hv;
    }
    __syncthreads();
    const int kc = H - c0 < MB_HC ? H - c0 : MB_HC;
    mb_mma<false>(macc, hs, kc, Wb, D, c0, D, wave, lo, hi);
    __syncthreads();                                          // hs is rewritten by the next chunk
  }

  // m = acc + bb, u = x (.) m in place (every operand read of the x tile lies before the last barrier)
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int n = (wave + 4 * j) * 32 + lo;
    if ((wave + 4 * j) * 32 < D) {
      const float bc = n < D ? bb[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mb_row(r, hi);
        const bool in = n < D && r0 + row < B;
        const float mv = macc[j][r] + bc;
        if (in && save_m) save_m[(r0 + row) * D + n] = mv;
        if (n < De) xs[n * MB_LD + row] = in ? xs[n * MB_LD + row] * mv : 0.f;
      }
    }
  }
  __syncthreads();

  // per-field feed-forward, passes of whole fields within 128 columns
  const int b = tid & (MB_T - 1), g = tid >> 5;
  const int fpp = MB_HC / E;
  for (int f0 = 0; f0 < F; f0 += fpp) {
    const int c0 = f0 * E, nc = (F - f0 < fpp ? F - f0 : fpp) * E;
    if (pointwise) {
      for (int c = g; c < nc; c += CN_G) {
        const int f = (c0 + c) / E, j = c0 + c - f * E;
        hs[c * MB_LD + b] = fmaxf(cn_dot<false>(xs, 0, W1, f, j, E, b), 0.f);
      }
      __syncthreads();
      for (int c = g; c < nc; c += CN_G) {                    // r over u: a column's u is read by its owner alone now
        const int f = (c0 + c) / E, j = c0 + c - f * E;
        xs[(c0 + c) * MB_LD + b] = cn_dot<false>(hs, c0, W2, f, j, E, b) + xs[(c0 + c) * MB_LD + b];
      }
      if (save_a) Tile::rows_out(save_a, hs, r0, B, D, c0, nc, tid);
      __syncthreads();                                        // hs is rewritten by the next pass
    } else {
      for (int c = g; c < nc; c += CN_G) {
        const int f = (c0 + c) / E, j = c0 + c - f * E;
        hs[c * MB_LD + b] = cn_dot<false>(xs, 0, W1, f, j, E, b);
      }
      __syncthreads();
      for (int c = g; c < nc; c += CN_G) xs[(c0 + c) * MB_LD + b] = hs[c * MB_LD + b];
      __syncthreads();
    }
  }

  // LayerNorm per (example, field): statistics to hs [2][F][33], then rows of consecutive columns
  const float inv_e = 1.f / (float)E;
  for (int f = g; f < F; f += CN_G) {
    const float* rr = xs + f * E * MB_LD + b;
    float s = 0.f;
    for (int e = 0; e < E; ++e) s += rr[e * MB_LD];
    const float mean = s * inv_e;
    float q = 0.f;
    for (int e = 0; e < E; ++e) {
      const float d = rr[e * MB_LD] - mean;
      q = fmaf(d, d, q);
    }
    const float rstd = 1.f / sqrtf(q * inv_e + CN_EPS);
    hs[f * MB_LD + b] = mean;
    hs[(F + f) * MB_LD + b] = rstd;
    if (save_rstd && r0 + b < B) save_rstd[(r0 + b) * F + f] = rstd;
  }
  __syncthreads();
  for (int i = tid; i < MB_T * D; i += CN_NTHR) {
    const int row = i / D, n = i - row * D, f = n / E;
    if (r0 + row < B) {
      const float xh = (xs[n * MB_LD + row] - hs[f * MB_LD + row]) * hs[(F + f) * MB_LD + row];
      y[(r0 + row) * D + n] = fmaf(xh, gamma[n], beta[n]);
      if (save_xhat) save_xhat[(r0 + row) * D + n] = xh;
    }
  }
}

// slot of a tile: dgamma [D] | dbeta [D] | dbb [D] | dba [H]
__global__ __launch_bounds__(CN_NTHR) void contextnet_block_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ Wa, const float* __restrict__ Wb,
    const float* __restrict__ W1, const float* __restrict__ W2, const float* __restrict__ gamma,
    const float* __restrict__ h, const float* __restrict__ m, const float* __restrict__ xhat,
    const float* __restrict__ rstd, const float* __restrict__ a, const float* __restrict__ dy, int64_t B, int F, int E,
    int H, int pointwise, float* __restrict__ dx, float* __restrict__ ws_dr, float* __restrict__ ws_da,
    float* __restrict__ ws_u, float* __restrict__ ws_dm, float* __restrict__ ws_dh, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = F * E, De = mb_even(D);
  float* ga = lds;                               // [De][33]: dy, then dr, then du, then dm
  float* gb = ga + De * MB_LD;                   // [De][33]: xhat, then a, then the direct part du (.) m
  float* cs = gb + De * MB_LD;                   // [128][33]: a chunk of da (single: of du), then of dh
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * (3 * D + H);
  const int b = tid & (MB_T - 1), g = tid >> 5;

  for (int i = tid; i < MB_T * De; i += CN_NTHR) {
    const int row = i / De, k = i - row * De;
    const bool in = k < D && r0 + row < B;
    ga[k * MB_LD + row] = in ? dy[(r0 + row) * D + k] : 0.f;
    gb[k * MB_LD + row] = in ? xhat[(r0 + row) * D + k] : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < D; c += CN_NTHR) {                    // column sums of the tile, rows in order
    float sg = 0.f, sb = 0.f;
    for (int r = 0; r < MB_T; ++r) {
      const float gv = ga[c * MB_LD + r];
      sg += gv * gb[c * MB_LD + r];
      sb += gv;
    }
    slot[c] = sg;
    slot[D + c] = sb;
  }
  __syncthreads();

  {                                                           // LayerNorm backward per (example, field), in place
    const float inv_e = 1.f / (float)E;
    for (int f = g; f < F; f += CN_G) {
      const float rs = r0 + b < B ? rstd[(r0 + b) * F + f] : 0.f;
      float* gr = ga + f * E * MB_LD + b;
      const float* xr = gb + f * E * MB_LD + b;
      float s1 = 0.f, s2 = 0.f;
      for (int e = 0; e < E; ++e) {
        const float dxh = gr[e * MB_LD] * gamma[f * E + e];
        s1 += dxh;
        s2 = fmaf(dxh, xr[e * MB_LD], s2);
      }
      s1 *= inv_e;
      s2 *= inv_e;
      for (int e = 0; e < E; ++e) {
        const float dxh = gr[e * MB_LD] * gamma[f * E + e];
        gr[e * MB_LD] = rs * (dxh - s1 - xr[e * MB_LD] * s2);
      }
    }
  }
  __syncthreads();
  if (pointwise) {
    for (int i = tid; i < MB_T * De; i += CN_NTHR) {
      const int row = i / De, k = i - row * De;
      gb[k * MB_LD + row] = (k < D && r0 + row < B) ? a[(r0 + row) * D + k] : 0.f;
    }
    __syncthreads();
  }

  const int fpp = MB_HC / E;
  for (int f0 = 0; f0 < F; f0 += fpp) {
    const int c0 = f0 * E, nc = (F - f0 < fpp ? F - f0 : fpp) * E;
    Tile::rows_out(ws_dr, ga + c0 * MB_LD, r0, B, D, c0, nc, tid);
    if (pointwise) {
      for (int c = g; c < nc; c += CN_G) {                    // da = (dr W2^T) (.) [a > 0]
        const int f = (c0 + c) / E, e = c0 + c - f * E;
        const float t = cn_dot<true>(ga, 0, W2, f, e, E, b);
        cs[c * MB_LD + b] = gb[(c0 + c) * MB_LD + b] > 0.f ? t : 0.f;
      }
      __syncthreads();
      for (int c = g; c < nc; c += CN_G) {                    // du = dr + da W1^T over dr: read by its owner alone now
        const int f = (c0 + c) / E, e = c0 + c - f * E;
        ga[(c0 + c) * MB_LD + b] = ga[(c0 + c) * MB_LD + b] + cn_dot<true>(cs, c0, W1, f, e, E, b);
      }
      Tile::rows_out(ws_da, cs, r0, B, D, c0, nc, tid);
      __syncthreads();
    } else {
      for (int c = g; c < nc; c += CN_G) {                    // du = dr W1^T
        const int f = (c0 + c) / E, e = c0 + c - f * E;
        cs[c * MB_LD + b] = cn_dot<true>(ga, 0, W1, f, e, E, b);
      }
      __syncthreads();                                        // every read of this pass's dr lies before it
      for (int c = g; c < nc; c += CN_G) ga[(c0 + c) * MB_LD + b] = cs[c * MB_LD + b];
      __syncthreads();
    }
  }

  for (int i = tid; i < MB_T * De; i += CN_NTHR) {            // dm = du (.) x over du, the direct part du (.) m
    const int row = i / De, k = i - row * De;
    const float du = ga[k * MB_LD + row];
    float dmv = 0.f, dd = 0.f;
    if (k < D && r0 + row < B) {
      const int64_t at = (r0 + row) * D + k;
      const float xv = x[at], mv = m[at];
      dmv = du * xv;
      dd = du * mv;
      ws_dm[at] = dmv;
      ws_u[at] = xv * mv;
    }
    ga[k * MB_LD + row] = dmv;
    gb[k * MB_LD + row] = dd;
  }
  __syncthreads();
  for (int c = tid; c < D; c += CN_NTHR) {
    float s = 0.f;
    for (int r = 0; r < MB_T; ++r) s += ga[c * MB_LD + r];
    slot[2 * D + c] = s;
  }

  f32x16 xacc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(xacc[j]);
  for (int c0 = 0; c0 < H; c0 += MB_HC) {
    const int col = c0 + 32 * wave + lo;
    f32x16 hacc;
    mb_zero(hacc);
    if (c0 + 32 * wave < H) mb_mma1<true>(hacc, ga, D, Wb, D, 0, H, c0 + 32 * wave, lo, hi);   // dm Wb^T
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mb_row(r, hi);
      float dhp = 0.f;
      if (col < H && r0 + row < B) {
        const int64_t at = (r0 + row) * H + col;
        dhp = h[at] > 0.f ? hacc[r] : 0.f;
        ws_dh[at] = dhp;
      }
      cs[(32 * wave + lo) * MB_LD + row] = dhp;
    }
    __syncthreads();
    if (tid < MB_HC && c0 + tid < H) {
      float s = 0.f;
      for (int r = 0; r < MB_T; ++r) s += cs[tid * MB_LD + r];
      slot[3 * D + c0 + tid] = s;
    }
    const int kc = H - c0 < MB_HC ? H - c0 : MB_HC;
    mb_mma<true>(xacc, cs, kc, Wa, H, c0, D, wave, lo, hi);    // dx += dh Wa^T
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int n = (wave + 4 * j) * 32 + lo;
    if ((wave + 4 * j) * 32 < D && n < D) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mb_row(r, hi);
        if (r0 + row < B) dx[(r0 + row) * D + n] = xacc[j][r] + gb[n * MB_LD + row];
      }
    }
  }
}

// Per-field weight gradients, all of them in one launch: workgroup (f and a block of 256 outputs, q, s) adds the examples
// of batch slice s, in order, into part[s][q][f] [E][E] = A_q[:, f]^T G_q[:, f], one output per thread; the slices are
// added by rec_slot_sum in slice order.  It is small_dw_kernel (tile_ops.h) with M = N = E and stays a kernel of its own:
// through the shared kernel it took 240 us against 170 at the default shape, most likely because it stages A and G in
// ONE loop with both loads in flight together where the shared kernel waits for each in turn.
__global__ __launch_bounds__(CN_NTHR) void contextnet_field_dw_kernel(const float* __restrict__ A0,
                                                                      const float* __restrict__ G0,
                                                                      const float* __restrict__ A1,
                                                                      const float* __restrict__ G1, int64_t B, int F,
                                                                      int E, int nblk, int64_t per,
                                                                      float* __restrict__ part) {
  __shared__ float as[CN_DW_ROWS * CN_MAXE], gs[CN_DW_ROWS * CN_MAXE];
  const int tid = threadIdx.x, f = blockIdx.x / nblk, q = blockIdx.y, D = F * E, EE = E * E;
  const int o = (blockIdx.x - f * nblk) * CN_NTHR + tid;
  const bool own = o < EE;
  const int oe = own ? o / E : 0, oj = own ? o - oe * E : 0;
  const float* __restrict__ Am = q ? A1 : A0;
  const float* __restrict__ Gm = q ? G1 : G0;
  const int64_t b0 = (int64_t)blockIdx.z * per, b1 = b0 + per < B ? b0 + per : B;
  float acc = 0.f;
  for (int64_t bb = b0; bb < b1; bb += CN_DW_ROWS) {
    for (int i = tid; i < CN_DW_ROWS * E; i += CN_NTHR) {
      const int r = i / E, e = i - r * E;
      const bool in = bb + r < b1;
      as[i] = in ? Am[(bb + r) * D + f * E + e] : 0.f;
      gs[i] = in ? Gm[(bb + r) * D + f * E + e] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < CN_DW_ROWS; ++r) acc = fmaf(as[r * E + oe], gs[r * E + oj], acc);
    __syncthreads();
  }
  if (own) part[(((int64_t)blockIdx.z * gridDim.y + q) * F + f) * EE + o] = acc;
}

static int cn_shape(int64_t B, int F, int E, int R, int pointwise) {
  if (B < 0 || F < 1 || E < 1 || R < 1 || (pointwise != 0 && pointwise != 1)) return REC_E_ARG;
  if (F > CN_MAXF || E > CN_MAXE || (int64_t)F * E > CN_MAXD || R > CN_MAXR || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;
  return REC_OK;
}

struct CnWs {
  size_t dr, da, u, dm, dh, slots, part, gemm, total;          // offsets in floats
};
static CnWs cn_ws(int64_t B, int F, int E, int H, int pointwise) {
  CnWs w{};
  const size_t b = (size_t)B, tiles = (size_t)ceil_div64(B, MB_T), D = (size_t)F * E;
  WsCarve c;
  w.dr = c.take(b * D);
  w.da = c.take(pointwise ? b * D : 0);
  w.u = c.take(b * D);
  w.dm = c.take(b * D);
  w.dh = c.take(b * H);
  w.slots = c.take(tiles * (3 * D + (size_t)H));
  w.part = c.take((size_t)mb_small_split(B) * (pointwise ? 2 : 1) * D * E);
  const size_t g1 = mb_dw_gemm_floats(B, (int)D, H), g2 = mb_dw_gemm_floats(B, H, (int)D);
  w.gemm = c.take(g1 > g2 ? g1 : g2);
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" int rec_emb_contextnet_in_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X,
                                             const float* values, int64_t B, int F, int Fk, float* x, int* oob_flag,
                                             void* stream) {
  if (int rc = cn_in_shape(B, F, Fk, E)) return rc;
  if (V <= 0 || ld < E) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!table || !X || !x || (Fk > 0 && !values)) return REC_E_ARG;
  const int64_t rows = B * F;
  hipLaunchKernelGGL(emb_contextnet_in_fwd_kernel, dim3(cn_in_grid(rows)), dim3(CN_NTHR), 0, as_stream(stream), table, V,
                     E, ld, X, values, rows, F, Fk, x, oob_flag);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_emb_contextnet_in_bwd_f32(const float* values, const float* dx, int64_t B, int F, int Fk, int E,
                                             float* vals, void* stream) {
  if (int rc = cn_in_shape(B, F, Fk, E)) return rc;
  if (B == 0) return REC_OK;
  if (!dx || !vals || (Fk > 0 && !values)) return REC_E_ARG;
  const int64_t rows = B * F;
  hipLaunchKernelGGL(emb_contextnet_in_bwd_kernel, dim3(cn_in_grid(rows)), dim3(CN_NTHR), 0, as_stream(stream), values,
                     dx, rows, F, Fk, E, vals);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" size_t rec_contextnet_block_workspace_bytes(int64_t B, int F, int E, int R, int pointwise) {
  if (cn_shape(B, F, E, R, pointwise) != REC_OK) return 0;
  return sizeof(float) * (cn_ws(B, F, E, R * F * E, pointwise).total + 4);
}

extern "C" int rec_contextnet_block_fwd_f32(const float* x, const float* Wa, const float* ba, const float* Wb,
                                            const float* bb, const float* W1, const float* W2, const float* gamma,
                                            const float* beta, int64_t B, int F, int E, int R, int pointwise, float* y,
                                            float* h, float* m, float* xhat, float* rstd, float* a, void* stream) {
  if (int rc = cn_shape(B, F, E, R, pointwise)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !Wa || !ba || !Wb || !bb || !W1 || (pointwise && !W2) || !gamma || !beta || !y) return REC_E_ARG;
  const bool save = h || m || xhat || rstd || a;
  if (save && !(h && m && xhat && rstd && (a || !pointwise))) return REC_E_ARG;   // all of them or none
  if (hipError_t e = rec_allow_lds<contextnet_block_fwd_kernel>(CN_LDS_CAP)) return (int)e;
  const int D = F * E;
  const size_t lds = sizeof(float) * cn_lds_floats(D, 0);
  hipLaunchKernelGGL(contextnet_block_fwd_kernel, dim3((unsigned)ceil_div64(B, MB_T)), dim3(CN_NTHR), lds,
                     as_stream(stream), x, Wa, ba, Wb, bb, W1, W2, gamma, beta, B, F, E, R * D, pointwise, y, h, m, xhat,
                     rstd, pointwise ? a : nullptr);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_contextnet_block_bwd_f32(const float* x, const float* Wa, const float* Wb, const float* W1,
                                            const float* W2, const float* gamma, const float* h, const float* m,
                                            const float* xhat, const float* rstd, const float* a, const float* dy,
                                            int64_t B, int F, int E, int R, int pointwise, float* dx, float* dWa,
                                            float* dba, float* dWb, float* dbb, float* dW1, float* dW2, float* dgamma,
                                            float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = cn_shape(B, F, E, R, pointwise)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !Wa || !Wb || !W1 || !gamma || !h || !m || !xhat || !rstd || !dy || !dx || !dWa || !dba || !dWb || !dbb ||
      !dW1 || !dgamma || !dbeta || !workspace || (pointwise && (!W2 || !a || !dW2)))
    return REC_E_ARG;
  const int D = F * E, H = R * D;
  const CnWs w = cn_ws(B, F, E, H, pointwise);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  float *dr = base + w.dr, *da = base + w.da, *u = base + w.u, *dm = base + w.dm, *dh = base + w.dh,
        *slots = base + w.slots, *part = base + w.part, *gws = base + w.gemm;
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, MB_T);
  if (hipError_t e = rec_allow_lds<contextnet_block_bwd_kernel>(CN_LDS_CAP)) return (int)e;
  const size_t lds = sizeof(float) * cn_lds_floats(D, 1);
  hipLaunchKernelGGL(contextnet_block_bwd_kernel, dim3(tiles), dim3(CN_NTHR), lds, st, x, Wa, Wb, W1, W2, gamma, h, m,
                     xhat, rstd, a, dy, B, F, E, H, pointwise, dx, dr, da, u, dm, dh, slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, 3 * D + H, tiles, slots, {{dgamma, dbeta, dbb, dba}, {D, D, D, H}}, st))
    return rc;
  // pointwise: dW1_f = u_f^T da_f, dW2_f = a_f^T dr_f; single: dW1_f = u_f^T dr_f
  const int S = mb_small_split(B), nq = pointwise ? 2 : 1;
  const int64_t per = ceil_div64(ceil_div64(B, S), CN_DW_ROWS) * CN_DW_ROWS;
  const int nblk = (E * E + CN_NTHR - 1) / CN_NTHR;
  hipLaunchKernelGGL(contextnet_field_dw_kernel, dim3(F * nblk, nq, S), dim3(CN_NTHR), 0, st, u, pointwise ? da : dr, a,
                     dr, B, F, E, nblk, per, part);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_SERIAL, nq * D * E, S, part, {{dW1, dW2}, {D * E, pointwise ? D * E : 0}}, st))
    return rc;
  if (int rc = mb_dw_gemm(D, H, B, x, dh, dWa, gws, stream)) return rc;        // dWa = x^T dh
  return mb_dw_gemm(H, D, B, h, dm, dWb, gws, stream);                           // dWb = h^T dm
}
