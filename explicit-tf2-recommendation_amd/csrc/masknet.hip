// MaskNet (LayerNormInputFeaturesEmbeddingLayer / MaskBlockLayer, 11.FiBiNet++/CustomLayers.py:245-337) on gfx950.
//
// Input stage, fused with the lookup.  X int64 [B, F], F = Fc + Fk with the Fk key columns LAST, values [B, Fk]:
//   r[b,f,:] = table[X[b,f]]  (f < Fc)      r[b,Fc+j,:] = table[X[b,Fc+j]] * values[b,j]
//   x_emb = r      x_norm[b,f,:] = (r - mean) * rstd * gamma_f + beta_f      biased variance, epsilon 1e-3, over E
// One workgroup takes one example at a time; 16 adjacent lanes share a row (lane l owns e = l, l + 16, ...), thread t owns
// the rows t / 16, t / 16 + 16, ...  The backward uses the same ownership, so a thread adds the examples of its
// workgroup into ITS (f, e) accumulators of dgamma / dbeta in example order; the workgroups' slots are added by
// rec_slot_sum.  stats [B, F, 2] = (mean, rstd).
//
// Mask block, one launch each way.  x_emb [B, D], v [B, P], H = R P:
//   h = relu(x_emb W1 + b1)   m = h W2 + b2   u = v (.) m   z = u W3 + b3   y = relu(LayerNorm(z))
// A workgroup of 4 waves owns a tile of 32 examples.  Every product runs on v_mfma_f32_32x32x2_f32 (fp32 in, fp32
// accumulate: the instruction of gemm.hip): the A operand is the tile, k-major in LDS ([k][33]: reads and writes of a
// 32-lane half fall on 32 different banks), the B operand is read from the weight in global memory (L2-resident, 128
// bytes per half wave).  h is produced in chunks of 128 columns, one 32-column block per wave, written k-major to LDS
// and consumed at once into the m accumulators (up to 4 blocks of 32 columns per wave): it never goes to HBM unless the
// caller asks for it.  Sizes that are no multiple of a tile are padded with zeros in LDS and by guarded operand reads,
// the epilogues are masked.  Training saves h, m, xhat and rstd; u is recomputed.
// The backward runs the per-example chain in one launch -- LayerNorm and relu backward, du = dz W3^T, dv = du (.) m,
// dm = du (.) v, dh = (dm W2^T) (.) [h > 0] in chunks, dx_emb (+)= dh W1^T -- writes dz, dm, u and dh to the workspace
// and the column sums of its tile (dgamma, dbeta, db3, db2, db1) to the tile's slot; the entry point then adds the slots
// (rec_slot_sum) and enqueues dW1 = x_emb^T dh, dW2 = h^T dm, dW3 = u^T dz on rec_gemm_f32 (split-K, slices added in
// order).  No float atomics and no value with two writers: bit-identical results run to run; no host synchronisation.
// Contraction is off in this file: the LayerNorm backward forms g gamma twice, for the sums and for the result, and a
// LayerNorm over ONE element (E = 1, O = 1) must return exactly zero, which g gamma - mean(g gamma) only does when both
// are the same rounded product.  Where a fused multiply-add is wanted it is written fmaf.
// Shared with the other tile kernels: the MFMA tile is mfma_tile.h; the workspace carving and the split-K
// weight-gradient GEMM are tile_ops.h.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

namespace {

constexpr int MN_MAXF = REC_MASKNET_MAX_F, MN_MAXE = REC_MASKNET_MAX_E;
constexpr int MN_MAXD = REC_MASKNET_MAX_D, MN_MAXP = REC_MASKNET_MAX_P, MN_MAXO = REC_MASKNET_MAX_O;
constexpr int MN_MAXR = REC_MASKNET_MAX_R;
constexpr float MN_EPS = 1e-3f;                  // tf.keras.layers.LayerNormalization()

constexpr int MN_NTHR = 256;
constexpr int MN_RI = (MN_MAXF + 15) / 16, MN_EJ = (MN_MAXE + 15) / 16;   // rows / columns a thread owns
constexpr int MN_FWD_GRID = 4096, MN_BWD_GRID = 512;

static_assert(MN_MAXF <= 64 && MN_MAXE <= 64, "a thread owns at most 4 x 4 elements of an example");

// ------------------------------------------------------------------------------------------------------------------
// input stage
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MN_NTHR) void emb_masknet_ln_fwd_kernel(const float* __restrict__ table, int64_t V, int E,
                                                                     int64_t ld, const int64_t* __restrict__ X,
                                                                     const float* __restrict__ values, int64_t B, int F,
                                                                     int Fk, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta,
                                                                     float* __restrict__ x_emb, float* __restrict__ x_norm,
                                                                     float* __restrict__ stats, int* oob) {
  const int tid = threadIdx.x, fr = tid >> 4, l = tid & 15, Fc = F - Fk;
  const float inv_e = 1.f / (float)E;
  bool bad = false;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
#pragma unroll
    for (int i = 0; i < MN_RI; ++i) {
      const int f = fr + 16 * i;
      if (16 * i >= F) break;                                  // uniform over the workgroup
      const bool row = f < F;
      const int64_t id = row ? X[b * F + f] : 0;
      const bool ok = row && (uint64_t)id < (uint64_t)V;
      bad |= row && !ok;
      const bool cont = row && f >= Fc;
      const float scale = cont ? values[b * Fk + (f - Fc)] : 1.f;
      float x[MN_EJ], s = 0.f;
#pragma unroll
      for (int j = 0; j < MN_EJ; ++j) {
        const int e = l + 16 * j;
        float t = (ok && e < E) ? table[id * ld + e] : 0.f;
        if (cont) t *= scale;
        x[j] = t;
        s += t;
      }
      const float mean = group_sum<16>(s) * inv_e;
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < MN_EJ; ++j) {
        const float d = (l + 16 * j < E) ? x[j] - mean : 0.f;
        q = fmaf(d, d, q);
      }
      const float rstd = 1.f / sqrtf(group_sum<16>(q) * inv_e + MN_EPS);
      if (!row) continue;
      const int64_t at = (b * F + f) * E;
#pragma unroll
      for (int j = 0; j < MN_EJ; ++j) {
        const int e = l + 16 * j;
        if (e < E) {
          x_emb[at + e] = x[j];
          x_norm[at + e] = fmaf((x[j] - mean) * rstd, gamma[f * E + e], beta[f * E + e]);
        }
      }
      if (l == 0) {
        stats[(b * F + f) * 2] = mean;
        stats[(b * F + f) * 2 + 1] = rstd;
      }
    }
  }
  if (bad && oob) *oob = 1;
}

// slot of workgroup w: [2][F E] = (dgamma, dbeta) partials
__global__ __launch_bounds__(MN_NTHR) void emb_masknet_ln_bwd_kernel(const float* __restrict__ x_emb,
                                                                     const float* __restrict__ stats,
                                                                     const float* __restrict__ values,
                                                                     const float* __restrict__ gamma,
                                                                     const float* __restrict__ dx_norm,
                                                                     const float* __restrict__ dx_emb, int64_t B, int F,
                                                                     int Fk, int E, float* __restrict__ vals,
                                                                     float* __restrict__ slots) {
  const int tid = threadIdx.x, fr = tid >> 4, l = tid & 15, Fc = F - Fk;
  const float inv_e = 1.f / (float)E;
  float ag[MN_RI][MN_EJ], ab[MN_RI][MN_EJ];
#pragma unroll
  for (int i = 0; i < MN_RI; ++i)
#pragma unroll
    for (int j = 0; j < MN_EJ; ++j) ag[i][j] = ab[i][j] = 0.f;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
#pragma unroll
    for (int i = 0; i < MN_RI; ++i) {
      const int f = fr + 16 * i;
      if (16 * i >= F) break;
      const bool row = f < F;
      const int64_t at = row ? (b * F + f) * E : 0;
      const float mean = row ? stats[(b * F + f) * 2] : 0.f, rstd = row ? stats[(b * F + f) * 2 + 1] : 0.f;
      float xh[MN_EJ], dxh[MN_EJ], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int j = 0; j < MN_EJ; ++j) {
        const int e = l + 16 * j;
        const bool in = row && e < E;
        const float dy = in ? dx_norm[at + e] : 0.f;
        xh[j] = in ? (x_emb[at + e] - mean) * rstd : 0.f;
        dxh[j] = in ? dy * gamma[f * E + e] : 0.f;
        ag[i][j] = fmaf(dy, xh[j], ag[i][j]);
        ab[i][j] += dy;
        s1 += dxh[j];
        s2 = fmaf(dxh[j], xh[j], s2);
      }
      s1 = group_sum<16>(s1) * inv_e;
      s2 = group_sum<16>(s2) * inv_e;
      if (!row) continue;
      const bool cont = f >= Fc;
      const float scale = cont ? values[b * Fk + (f - Fc)] : 1.f;
#pragma unroll
      for (int j = 0; j < MN_EJ; ++j) {
        const int e = l + 16 * j;
        if (e < E) {
          float g = rstd * (dxh[j] - s1 - xh[j] * s2);
          if (dx_emb) g += dx_emb[at + e];
          vals[at + e] = cont ? g * scale : g;
        }
      }
    }
  }
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * 2 * F * E;
#pragma unroll
  for (int i = 0; i < MN_RI; ++i)
#pragma unroll
    for (int j = 0; j < MN_EJ; ++j) {
      const int f = fr + 16 * i, e = l + 16 * j;
      if (f < F && e < E) {
        slot[f * E + e] = ag[i][j];
        slot[F * E + f * E + e] = ab[i][j];
      }
    }
}

static int mn_ln_shape(int64_t B, int F, int Fk, int E) {
  if (B < 0 || F < 1 || E < 1 || Fk < 0 || Fk > F) return REC_E_ARG;
  if (F > MN_MAXF || E > MN_MAXE || B >= ((int64_t)1 << 31)) return REC_E_UNSUPPORTED;
  return REC_OK;
}
static int mn_ln_bwd_grid(int64_t B) { return (int)(B < MN_BWD_GRID ? (B < 1 ? 1 : B) : MN_BWD_GRID); }

// ------------------------------------------------------------------------------------------------------------------
// mask block
// ------------------------------------------------------------------------------------------------------------------
static_assert(MN_MAXD <= 128 * MB_NJ && MN_MAXP <= 128 * MB_NJ && MN_MAXO <= 128, "accumulator blocks per wave");


// floats of LDS: forward  xs / us [even(max(D,P))][33] | hs [128][33] | zs [32][O + 1]
//                backward dzs [even(O)][33] | ra [max(2 even(O), even(P))][33] (g, g xhat, then dm) | dhs [128][33]
__host__ __device__ inline size_t mb_lds_floats(int D, int P, int O, int bwd) {
  const int DP = mb_even(D > P ? D : P), Oe = mb_even(O), Pe = mb_even(P);
  return bwd ? (size_t)(Oe + (2 * Oe > Pe ? 2 * Oe : Pe) + MB_HC) * MB_LD
             : (size_t)(DP + MB_HC) * MB_LD + (size_t)MB_T * (O + 1);
}
constexpr size_t MB_LDS_CAP = 144 * 1024;

__global__ __launch_bounds__(MN_NTHR) void mask_block_fwd_kernel(
    const float* __restrict__ x_emb, const float* __restrict__ v, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const float* __restrict__ W3, const float* __restrict__ b3, const float* __restrict__ gamma,
    const float* __restrict__ beta, int64_t B, int D, int P, int O, int H, float* __restrict__ y,
    float* __restrict__ save_h, float* __restrict__ save_m, float* __restrict__ save_xhat,
    float* __restrict__ save_rstd) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int De = mb_even(D), Pe = mb_even(P), DP = De > Pe ? De : Pe;
  float* xs = lds;                               // [DP][33]: the x_emb tile, later u
  float* hs = xs + DP * MB_LD;                   // [128][33]
  float* zs = hs + MB_HC * MB_LD;                // [32][O + 1]
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;

  for (int i = tid; i < MB_T * De; i += MN_NTHR) {
    const int m = i / De, k = i - m * De;
    xs[k * MB_LD + m] = (k < D && r0 + m < B) ? x_emb[(r0 + m) * D + k] : 0.f;
  }
  __syncthreads();

  f32x16 macc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(macc[j]);

  for (int c0 = 0; c0 < H; c0 += MB_HC) {
    const int col = c0 + 32 * wave + lo;
    f32x16 hacc;
    mb_zero(hacc);
    if (c0 + 32 * wave < H) mb_mma1<false>(hacc, xs, D, W1, H, 0, H, c0 + 32 * wave, lo, hi);
    const float bc = col < H ? b1[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mb_row(r, hi);
      const float hv = col < H ? fmaxf(hacc[r] + bc, 0.f) : 0.f;
      hs[(32 * wave + lo) * MB_LD + row] = hv;
      if (save_h && col < H && r0 + row < B) save_h[(r0 + row) * H + col] = hv;
    }
    __syncthreads();
    const int kc = H - c0 < MB_HC ? H - c0 : MB_HC;
    mb_mma<false>(macc, hs, kc, W2, P, c0, P, wave, lo, hi);
    __syncthreads();                                          // hs is rewritten by the next chunk
  }

  // m = acc + b2, u = v (.) m -> xs (every read of the x_emb tile lies before the last barrier)
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int n = (wave + 4 * j) * 32 + lo;
    if ((wave + 4 * j) * 32 < P) {
      const float bc = n < P ? b2[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mb_row(r, hi);
        const bool in = n < P && r0 + row < B;
        const float mv = macc[j][r] + bc;
        float u = 0.f;
        if (in) {
          u = v[(r0 + row) * P + n] * mv;
          if (save_m) save_m[(r0 + row) * P + n] = mv;
        }
        if (n < Pe) xs[n * MB_LD + row] = u;
      }
    }
  }
  __syncthreads();

  if (32 * wave < O) {
    f32x16 zacc;
    mb_zero(zacc);
    mb_mma1<false>(zacc, xs, P, W3, O, 0, O, 32 * wave, lo, hi);
    const int col = 32 * wave + lo;
    if (col < O) {
      const float bc = b3[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) zs[mb_row(r, hi) * (O + 1) + col] = zacc[r] + bc;
    }
  }
  __syncthreads();

  {                                                           // LayerNorm + relu: 8 adjacent lanes per example
    const int row = tid >> 3, sub = tid & 7;
    const float* zr = zs + row * (O + 1);
    const float inv_o = 1.f / (float)O;
    float s = 0.f;
    for (int c = sub; c < O; c += 8) s += zr[c];
    const float mean = group_sum<8>(s) * inv_o;
    float q = 0.f;
    for (int c = sub; c < O; c += 8) {
      const float d = zr[c] - mean;
      q = fmaf(d, d, q);
    }
    const float rstd = 1.f / sqrtf(group_sum<8>(q) * inv_o + MN_EPS);
    if (r0 + row < B) {
      for (int c = sub; c < O; c += 8) {
        const float xh = (zr[c] - mean) * rstd;
        y[(r0 + row) * O + c] = fmaxf(fmaf(xh, gamma[c], beta[c]), 0.f);
        if (save_xhat) save_xhat[(r0 + row) * O + c] = xh;
      }
      if (save_rstd && sub == 0) save_rstd[r0 + row] = rstd;
    }
  }
}

// slot of a tile: dgamma [O] | dbeta [O] | db3 [O] | db2 [P] | db1 [H]
__global__ __launch_bounds__(MN_NTHR) void mask_block_bwd_kernel(
    const float* __restrict__ v, const float* __restrict__ W1, const float* __restrict__ W2,
    const float* __restrict__ W3, const float* __restrict__ gamma, const float* __restrict__ y,
    const float* __restrict__ h, const float* __restrict__ m, const float* __restrict__ xhat,
    const float* __restrict__ rstd, const float* __restrict__ dy, int64_t B, int D, int P, int O, int H,
    float* __restrict__ dv, float* __restrict__ dx_emb, int accumulate, float* __restrict__ ws_dz,
    float* __restrict__ ws_dm, float* __restrict__ ws_u, float* __restrict__ ws_dh, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Oe = mb_even(O), Pe = mb_even(P);
  float* dzs = lds;                                            // [Oe][33]
  float* ra = dzs + Oe * MB_LD;                                // gs [Oe][33] | gxs [Oe][33], then dms [Pe][33]
  float* gs = ra;
  float* gxs = ra + Oe * MB_LD;
  float* dms = ra;
  float* dhs = ra + (2 * Oe > Pe ? 2 * Oe : Pe) * MB_LD;       // [128][33]
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * (3 * O + P + H);

  {                                                           // relu and LayerNorm backward: 8 adjacent lanes per example
    const int row = tid >> 3, sub = tid & 7;
    const bool in = r0 + row < B;
    const int64_t at = in ? (r0 + row) * O : 0;
    const float inv_o = 1.f / (float)O, rs = in ? rstd[r0 + row] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    for (int c = sub; c < Oe; c += 8) {
      float g = 0.f, xh = 0.f;
      if (in && c < O) {
        g = y[at + c] > 0.f ? dy[at + c] : 0.f;
        xh = xhat[at + c];
      }
      const float dxh = c < O ? g * gamma[c] : 0.f;
      gs[c * MB_LD + row] = g;
      gxs[c * MB_LD + row] = g * xh;
      s1 += dxh;
      s2 = fmaf(dxh, xh, s2);
    }
    s1 = group_sum<8>(s1) * inv_o;
    s2 = group_sum<8>(s2) * inv_o;
    for (int c = sub; c < Oe; c += 8) {
      float dz = 0.f;
      if (in && c < O) {
        const float g = gs[c * MB_LD + row], xh = xhat[at + c];
        dz = rs * (g * gamma[c] - s1 - xh * s2);
        ws_dz[at + c] = dz;
      }
      dzs[c * MB_LD + row] = dz;
    }
  }
  __syncthreads();
  for (int c = tid; c < O; c += MN_NTHR) {                    // column sums of the tile, rows in order
    float a = 0.f, b = 0.f, d = 0.f;
    for (int r = 0; r < MB_T; ++r) {
      a += gxs[c * MB_LD + r];
      b += gs[c * MB_LD + r];
      d += dzs[c * MB_LD + r];
    }
    slot[c] = a;
    slot[O + c] = b;
    slot[2 * O + c] = d;
  }
  __syncthreads();                                            // ra becomes dms

  {
    f32x16 acc[MB_NJ];
#pragma unroll
    for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
    mb_mma<true>(acc, dzs, O, W3, O, 0, P, wave, lo, hi);      // du = dz W3^T
#pragma unroll
    for (int j = 0; j < MB_NJ; ++j) {
      const int n = (wave + 4 * j) * 32 + lo;
      if ((wave + 4 * j) * 32 < P) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mb_row(r, hi);
          float dmv = 0.f;
          if (n < P && r0 + row < B) {
            const int64_t at = (r0 + row) * P + n;
            const float du = acc[j][r], vv = v[at], mm = m[at];
            dmv = du * vv;
            dv[at] = du * mm;
            ws_dm[at] = dmv;
            ws_u[at] = vv * mm;
          }
          if (n < Pe) dms[n * MB_LD + row] = dmv;
        }
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < P; c += MN_NTHR) {
    float a = 0.f;
    for (int r = 0; r < MB_T; ++r) a += dms[c * MB_LD + r];
    slot[3 * O + c] = a;
  }

  f32x16 xacc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(xacc[j]);
  for (int c0 = 0; c0 < H; c0 += MB_HC) {
    const int col = c0 + 32 * wave + lo;
    f32x16 hacc;
    mb_zero(hacc);
    if (c0 + 32 * wave < H) mb_mma1<true>(hacc, dms, P, W2, P, 0, H, c0 + 32 * wave, lo, hi);   // dm W2^T
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mb_row(r, hi);
      float dhp = 0.f;
      if (col < H && r0 + row < B) {
        const int64_t at = (r0 + row) * H + col;
        dhp = h[at] > 0.f ? hacc[r] : 0.f;
        ws_dh[at] = dhp;
      }
      dhs[(32 * wave + lo) * MB_LD + row] = dhp;
    }
    __syncthreads();
    if (tid < MB_HC && c0 + tid < H) {
      float a = 0.f;
      for (int r = 0; r < MB_T; ++r) a += dhs[tid * MB_LD + r];
      slot[3 * O + P + c0 + tid] = a;
    }
    const int kc = H - c0 < MB_HC ? H - c0 : MB_HC;
    mb_mma<true>(xacc, dhs, kc, W1, H, c0, D, wave, lo, hi);   // dx_emb += dh W1^T
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int n = (wave + 4 * j) * 32 + lo;
    if ((wave + 4 * j) * 32 < D && n < D) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mb_row(r, hi);
        if (r0 + row < B) {
          const int64_t at = (r0 + row) * D + n;
          dx_emb[at] = accumulate ? dx_emb[at] + xacc[j][r] : xacc[j][r];
        }
      }
    }
  }
}

static int mb_shape(int64_t B, int D, int P, int O, int R) {
  if (B < 0 || D < 1 || P < 1 || O < 1 || R < 1) return REC_E_ARG;
  if (D > MN_MAXD || P > MN_MAXP || O > MN_MAXO || R > MN_MAXR || B >= ((int64_t)1 << 31)) return REC_E_UNSUPPORTED;
  return REC_OK;
}

struct MbWs {
  size_t dz, dm, u, dh, slots, gemm, total;                    // offsets in floats
};
static MbWs mb_ws(int64_t B, int D, int P, int O, int H) {
  MbWs w{};
  const size_t b = (size_t)B, tiles = (size_t)ceil_div64(B, MB_T);
  WsCarve c;
  w.dz = c.take(b * O);
  w.dm = c.take(b * P);
  w.u = c.take(b * P);
  w.dh = c.take(b * H);
  w.slots = c.take(tiles * (size_t)(3 * O + P + H));
  const size_t g = mb_dw_gemm_floats(B, D, H), g2 = mb_dw_gemm_floats(B, H, P), g3 = mb_dw_gemm_floats(B, P, O);
  w.gemm = c.take(g > g2 ? (g > g3 ? g : g3) : (g2 > g3 ? g2 : g3));
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" size_t rec_masknet_ln_workspace_bytes(int64_t B, int F, int E) {
  if (mn_ln_shape(B, F, 0, E) != REC_OK) return 0;
  return sizeof(float) * (size_t)mn_ln_bwd_grid(B) * 2 * F * E;
}

extern "C" int rec_emb_masknet_ln_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X,
                                          const float* values, int64_t B, int F, int Fk, const float* gamma,
                                          const float* beta, float* x_emb, float* x_norm, float* stats, int* oob_flag,
                                          void* stream) {
  if (int rc = mn_ln_shape(B, F, Fk, E)) return rc;
  if (V <= 0 || ld < E) return REC_E_ARG;
  if (B == 0) return REC_OK;
  if (!table || !X || !gamma || !beta || !x_emb || !x_norm || !stats || (Fk > 0 && !values)) return REC_E_ARG;
  const int grid = (int)(B < MN_FWD_GRID ? B : MN_FWD_GRID);
  hipLaunchKernelGGL(emb_masknet_ln_fwd_kernel, dim3(grid), dim3(MN_NTHR), 0, as_stream(stream), table, V, E, ld, X,
                     values, B, F, Fk, gamma, beta, x_emb, x_norm, stats, oob_flag);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_emb_masknet_ln_bwd_f32(const float* x_emb, const float* stats, const float* values,
                                          const float* gamma, const float* dx_norm, const float* dx_emb, int64_t B, int F,
                                          int Fk, int E, float* vals, float* dgamma, float* dbeta, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  if (int rc = mn_ln_shape(B, F, Fk, E)) return rc;
  if (B == 0) return REC_OK;
  if (!x_emb || !stats || !gamma || !dx_norm || !vals || !dgamma || !dbeta || !workspace || (Fk > 0 && !values))
    return REC_E_ARG;
  const int grid = mn_ln_bwd_grid(B);
  if (workspace_bytes < sizeof(float) * (size_t)grid * 2 * F * E) return REC_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  float* slots = static_cast<float*>(workspace);
  hipLaunchKernelGGL(emb_masknet_ln_bwd_kernel, dim3(grid), dim3(MN_NTHR), 0, st, x_emb, stats, values, gamma, dx_norm,
                     dx_emb, B, F, Fk, E, vals, slots);
  REC_LAUNCH_CHECK();
  return rec_slot_sum(REC_SLOTS_WAVE, 2 * F * E, grid, slots, {{dgamma, dbeta}, {F * E, F * E}}, st);
}

extern "C" size_t rec_masknet_block_workspace_bytes(int64_t B, int D, int P, int O, int R) {
  if (mb_shape(B, D, P, O, R) != REC_OK) return 0;
  return sizeof(float) * (mb_ws(B, D, P, O, R * P).total + 4);
}

extern "C" int rec_mask_block_fwd_f32(const float* x_emb, const float* v, const float* W1, const float* b1,
                                      const float* W2, const float* b2, const float* W3, const float* b3,
                                      const float* gamma, const float* beta, int64_t B, int D, int P, int O, int R,
                                      float* y, float* h, float* m, float* xhat, float* rstd, void* stream) {
  if (int rc = mb_shape(B, D, P, O, R)) return rc;
  if (B == 0) return REC_OK;
  if (!x_emb || !v || !W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !gamma || !beta || !y) return REC_E_ARG;
  const bool save = h || m || xhat || rstd;
  if (save && !(h && m && xhat && rstd)) return REC_E_ARG;     // the save buffers come together or not at all
  if (hipError_t e = rec_allow_lds<mask_block_fwd_kernel>(MB_LDS_CAP)) return (int)e;
  const size_t lds = sizeof(float) * mb_lds_floats(D, P, O, 0);
  hipLaunchKernelGGL(mask_block_fwd_kernel, dim3((unsigned)ceil_div64(B, MB_T)), dim3(MN_NTHR), lds, as_stream(stream),
                     x_emb, v, W1, b1, W2, b2, W3, b3, gamma, beta, B, D, P, O, R * P, y, h, m, xhat, rstd);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_mask_block_bwd_f32(const float* x_emb, const float* v, const float* W1, const float* W2,
                                      const float* W3, const float* gamma, const float* y, const float* h, const float* m,
                                      const float* xhat, const float* rstd, const float* dy, int64_t B, int D, int P,
                                      int O, int R, float* dv, float* dx_emb, int accumulate, float* dW1, float* db1,
                                      float* dW2, float* db2, float* dW3, float* db3, float* dgamma, float* dbeta,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = mb_shape(B, D, P, O, R)) return rc;
  if (B == 0) return REC_OK;
  if (!x_emb || !v || !W1 || !W2 || !W3 || !gamma || !y || !h || !m || !xhat || !rstd || !dy || !dv || !dx_emb || !dW1 ||
      !db1 || !dW2 || !db2 || !dW3 || !db3 || !dgamma || !dbeta || !workspace)
    return REC_E_ARG;
  const int H = R * P;
  const MbWs w = mb_ws(B, D, P, O, H);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  float *dz = base + w.dz, *dm = base + w.dm, *u = base + w.u, *dh = base + w.dh, *slots = base + w.slots,
        *gws = base + w.gemm;
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, MB_T);
  if (hipError_t e = rec_allow_lds<mask_block_bwd_kernel>(MB_LDS_CAP)) return (int)e;
  const size_t lds = sizeof(float) * mb_lds_floats(D, P, O, 1);
  hipLaunchKernelGGL(mask_block_bwd_kernel, dim3(tiles), dim3(MN_NTHR), lds, st, v, W1, W2, W3, gamma, y, h, m, xhat,
                     rstd, dy, B, D, P, O, H, dv, dx_emb, accumulate, dz, dm, u, dh, slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, 3 * O + P + H, tiles, slots,
                            {{dgamma, dbeta, db3, db2, db1}, {O, O, O, P, H}}, st))
    return rc;
  if (int rc = mb_dw_gemm(D, H, B, x_emb, dh, dW1, gws, stream)) return rc;     // dW1 = x_emb^T dh
  if (int rc = mb_dw_gemm(H, P, B, h, dm, dW2, gws, stream)) return rc;         // dW2 = h^T dm
  return mb_dw_gemm(P, O, B, u, dz, dW3, gws, stream);                           // dW3 = u^T dz
}
