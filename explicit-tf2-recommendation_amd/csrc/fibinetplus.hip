// FiBiNet++ (NormInputFeaturesEmbeddingLayer / SENetPlusLayer / BilinearInteractionPlusLayer / FiBiNetPlusLayer,
// 11.FiBiNet++/CustomLayers.py:78-242) on gfx950.
//
// Input stage, fused with the lookup.  X int64 [B, F], F = Fc + Fk with the Fk key columns LAST, values [B, Fk]:
//   categorical rows  table[X[b,f]]               -> ONE BatchNorm over the B Fc rows, per channel e (gamma, beta [E])
//   key rows          table[X[b,Fc+j]] values[b,j] -> LayerNorm_j over E (gamma, beta [Fk, E])
// 16 adjacent lanes share a row.  The gather kernel finishes the key rows at once (the LayerNorm statistics are a 16-lane
// butterfly) and leaves the categorical rows raw in x.  In training mode the channel statistics follow in two passes over
// those just-written rows: column sums of a batch slice per workgroup into slots (a slot row is [Fc][E], so ONE
// rec_slot_sum over S Fc slots of E floats folds the slices and the fields), first of x, then of (x - mean)^2 -- the
// variance is never formed from raw second moments -- and an elementwise kernel normalises in place, saves xhat and the
// channels' rstd and moves the moving averages (on the device: the call stays graph-capturable).  Eval mode is the one
// gather kernel, on the moving statistics.  The backward takes the column sums of g and g xhat the same way (categorical
// columns fold to [E], key columns stay [Fk, E]) and one row kernel applies the BatchNorm backward (training: the full
// one across the B Fc rows; eval: g gamma rstd) or the LayerNorm backward times the value.
//
// Body, one launch each way.  x [B, F, E], D = F E, P = F (F - 1) / 2 pairs in itertools.combinations order:
//   p[pair] = x_i W x_j^T   q = LN(p Wr + br)                                                   (bilinear+)
//   s = [group means | group maxima] per field   h = relu(LN(s S0 + b0))   A = relu(LN(h S1 + b1))   v = x (.) A   (SENet+)
//   out = [q | v]
// A workgroup of 256 threads owns 16 examples; every operand of the tile lives in LDS k-major ([column][17]: the 16
// lanes of an example group read 16 consecutive banks).  Thread t owns example t & 15 and the columns t / 16, t / 16 + 16,
// ... of whatever vector is being produced; it reads the operand vector of its example out of LDS and ONE weight per
// step (the 16 lanes of a group load the same address).  None of the products is wide: at the default shape the largest
// is the 78 pair forms of 16 x 16, then 17 x 208; they run on the VALU as ContextNet's per-field stage does, and the
// weights are read through the caches rather than staged (DESIGN.md 3.6 has the figures and what that costs).  For
// E = 16 and a 16-byte aligned W a pair form takes x_j into registers and a row of W as four float4 loads, with the
// additions in the order of the plain loop: the same bits.
// The LayerNorm statistics of an example are the sums of its 16 column groups' partials, added in group order through
// LDS, so every thread of the example holds the same bits.  Three regions are reused down the chain (forward: x |
// max(2 G F, D, O) | max(P, mid)); at the limits (D = 512, 2 G F = 1024, mid = 512) that is 2048 columns = 136 KB.
// The backward runs the per-example chain of a tile in one launch and recomputes h and A from the saved xhat: it writes
// dz1, dz0, dzq and dp to the workspace and the column sums of its tile to the tile's two slots; the entry point adds the
// slots (rec_slot_sum), runs ALL bilinear weight gradients as one launch over (matrix, block of outputs, batch slice)
// whose at most 16 slices are added in order, and enqueues dWr = p^T dzq, dS0 = s^T dz0, dS1 = h^T dz1 on rec_gemm_f32
// (split-K, slices added in order).  The gradient of a group maximum goes to the first arg-max element.
// No float atomics and no value with two writers: bit-identical results run to run; no host synchronisation.
// Contraction is off in this file as in masknet.hip: a norm over ONE element must return exactly beta and exactly zero
// gradients, which x - mean and g gamma - mean(g gamma) only do when both sides are the same rounded value.
// Shared with the other tile kernels, in tile_ops.h: the row / column passes over an LDS operand (TileOps, here on the
// 16-example tile), the batch slices of the weight-gradient launch, the workspace carving and the split-K weight-gradient
// GEMM.  The bilinear weight gradients sum over field pairs inside the accumulation and keep a kernel of their own.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

namespace {

// the limits are FiBiNet's and MaskNet's: the header gains no constant for this family
constexpr int FP_MAXF = REC_FIBINET_MAX_F, FP_MAXE = REC_FIBINET_MAX_E, FP_MAXD = REC_MASKNET_MAX_D;
constexpr int FP_MAXO = REC_MASKNET_MAX_O, FP_MAXMID = REC_MASKNET_MAX_P;
constexpr int FP_MAXP = FP_MAXF * (FP_MAXF - 1) / 2;
// the bilinear type is FiBiNet's code
enum { FP_ALL = REC_FIBINET_TYPE_ALL, FP_EACH = REC_FIBINET_TYPE_EACH, FP_INTERACTION = REC_FIBINET_TYPE_INTERACTION };
static_assert(FP_ALL < FP_EACH && FP_EACH < FP_INTERACTION && FP_INTERACTION - FP_ALL == 2,
              "the shape check takes the types as a range");
constexpr float FP_EPS = 1e-3f;                  // Keras' default epsilon of both normalisations
constexpr float FP_MOMENTUM = 0.99f;             // tf.keras.layers.BatchNormalization()
constexpr int FP_NTHR = 256;
constexpr int FP_T = 16;                         // examples of a tile
constexpr int FP_LD = 17;                        // row stride of a k-major LDS operand [k][16 examples]
constexpr int FP_G = FP_NTHR / FP_T;             // column groups
constexpr int FP_IN_GRID = 4096;
constexpr int FP_IN_SLICES = 1024;               // batch slices of the channel statistics
constexpr int FP_DW_ROWS = 32;                   // examples of one step of the bilinear weight gradients

// ------------------------------------------------------------------------------------------------------------------
// input stage
// ------------------------------------------------------------------------------------------------------------------
// training: the categorical rows leave raw (normalised by fp_in_apply_kernel); eval: normalised on the moving statistics
__global__ __launch_bounds__(FP_NTHR) void fp_in_gather_kernel(
    const float* __restrict__ table, int64_t V, int E, int64_t ld, const int64_t* __restrict__ X,
    const float* __restrict__ values, const float* __restrict__ gamma_bn, const float* __restrict__ beta_bn,
    const float* __restrict__ gamma_ln, const float* __restrict__ beta_ln, const float* __restrict__ moving_mean,
    const float* __restrict__ moving_var, int64_t rows, int F, int Fk, int training, float* __restrict__ x,
    float* __restrict__ xhat, float* __restrict__ rstd_bn, float* __restrict__ rstd_ln, int* oob) {
  const int l = threadIdx.x & 15, Fc = F - Fk;
  const float inv_e = 1.f / (float)E;
  bool bad = false;
  if (!training && rstd_bn && blockIdx.x == 0 && (int)threadIdx.x < E && Fc > 0)
    rstd_bn[threadIdx.x] = 1.f / sqrtf(moving_var[threadIdx.x] + FP_EPS);
  for (int64_t r = (int64_t)blockIdx.x * (FP_NTHR / 16) + (threadIdx.x >> 4); r < rows;
       r += (int64_t)gridDim.x * (FP_NTHR / 16)) {
    const int64_t b = r / F;
    const int f = (int)(r - b * F);
    const int64_t id = X[r];
    const bool ok = (uint64_t)id < (uint64_t)V;
    bad |= !ok;
    if (f < Fc) {
      for (int e = l; e < E; e += 16) {
        const float t = ok ? table[id * ld + e] : 0.f;
        if (training) {
          x[r * E + e] = t;
        } else {
          const float xh = (t - moving_mean[e]) * (1.f / sqrtf(moving_var[e] + FP_EPS));
          x[r * E + e] = xh * gamma_bn[e] + beta_bn[e];
          if (xhat) xhat[r * E + e] = xh;
        }
      }
    } else {
      const int j = f - Fc;
      const float scale = values[b * Fk + j];
      float t[4], s = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = l + 16 * k;
        t[k] = (e < E && ok) ? table[id * ld + e] * scale : 0.f;
        s += t[k];
      }
      const float mean = group_sum<16>(s) * inv_e;
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = (l + 16 * k < E) ? t[k] - mean : 0.f;
        q = fmaf(d, d, q);
      }
      const float rs = 1.f / sqrtf(group_sum<16>(q) * inv_e + FP_EPS);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = l + 16 * k;
        if (e < E) {
          const float xh = (t[k] - mean) * rs;
          x[r * E + e] = xh * gamma_ln[j * E + e] + beta_ln[j * E + e];
          if (xhat) xhat[r * E + e] = xh;
        }
      }
      if (rstd_ln && l == 0) rstd_ln[b * Fk + j] = rs;
    }
  }
  if (bad && oob) *oob = 1;
}

// column sums of batch slice blockIdx.x over the ncol = Fc E categorical columns of a [B, ld]:
// SQ == 0: sum a      SQ == 1: sum (a - sum[e] / n)^2      -> slots[slice][ncol]
template <int SQ>
__global__ __launch_bounds__(FP_NTHR) void fp_in_colsum_kernel(const float* __restrict__ a,
                                                               const float* __restrict__ sum, int64_t B, int ld,
                                                               int ncol, int E, int64_t per, float n,
                                                               float* __restrict__ slots) {
  const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < B ? b0 + per : B;
  for (int c = threadIdx.x; c < ncol; c += FP_NTHR) {
    const float mean = SQ ? sum[c % E] / n : 0.f;
    float acc = 0.f;
    for (int64_t b = b0; b < b1; ++b) {
      const float v = a[b * ld + c];
      if (SQ) {
        const float d = v - mean;
        acc = fmaf(d, d, acc);
      } else {
        acc += v;
      }
    }
    slots[(int64_t)blockIdx.x * ncol + c] = acc;
  }
}

__global__ __launch_bounds__(FP_NTHR) void fp_in_apply_kernel(const float* __restrict__ sum, const float* __restrict__ m2,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int64_t B, int F, int Fc,
                                                              int E, float n, float* __restrict__ moving_mean,
                                                              float* __restrict__ moving_var, float* __restrict__ x,
                                                              float* __restrict__ xhat, float* __restrict__ rstd_bn) {
  const int64_t t = (int64_t)blockIdx.x * FP_NTHR + threadIdx.x;
  if (t < E) {
    const float mean = sum[t] / n, var = m2[t] / n;
    if (rstd_bn) rstd_bn[t] = 1.f / sqrtf(var + FP_EPS);
    moving_mean[t] = moving_mean[t] * FP_MOMENTUM + mean * (1.f - FP_MOMENTUM);
    moving_var[t] = moving_var[t] * FP_MOMENTUM + var * (1.f - FP_MOMENTUM);
  }
  const int ce = Fc * E;
  if (t >= B * ce) return;
  const int64_t b = t / ce;
  const int c = (int)(t - b * ce), e = c % E;
  const int64_t at = b * F * E + c;
  const float mean = sum[e] / n, rs = 1.f / sqrtf(m2[e] / n + FP_EPS);
  const float xh = (x[at] - mean) * rs;
  x[at] = xh * gamma[e] + beta[e];
  if (xhat) xhat[at] = xh;
}

// backward column sums of a batch slice: sum g and sum g xhat.  Categorical columns: slot_c[(slice Fc + f)][2][E];
// key columns: slot_k[slice][2][Fk E]
__global__ __launch_bounds__(FP_NTHR) void fp_in_bwd_colsum_kernel(const float* __restrict__ g,
                                                                   const float* __restrict__ xhat, int64_t B, int F,
                                                                   int Fc, int E, int64_t per,
                                                                   float* __restrict__ slot_c,
                                                                   float* __restrict__ slot_k) {
  const int D = F * E, ce = Fc * E, ke = D - ce;
  const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < B ? b0 + per : B;
  for (int c = threadIdx.x; c < D; c += FP_NTHR) {
    float sg = 0.f, sx = 0.f;
    for (int64_t b = b0; b < b1; ++b) {
      const float gv = g[b * D + c];
      sg += gv;
      sx += gv * xhat[b * D + c];
    }
    if (c < ce) {
      const int f = c / E, e = c - f * E;
      float* o = slot_c + ((int64_t)blockIdx.x * Fc + f) * 2 * E;
      o[e] = sg;
      o[E + e] = sx;
    } else {
      float* o = slot_k + (int64_t)blockIdx.x * 2 * ke;
      o[c - ce] = sg;
      o[ke + c - ce] = sx;
    }
  }
}

__global__ __launch_bounds__(FP_NTHR) void fp_in_bwd_apply_kernel(
    const float* __restrict__ g, const float* __restrict__ values, const float* __restrict__ xhat,
    const float* __restrict__ rstd_bn, const float* __restrict__ rstd_ln, const float* __restrict__ gamma_bn,
    const float* __restrict__ gamma_ln, const float* __restrict__ sum_g, const float* __restrict__ sum_gx,
    int64_t rows, int F, int Fk, int E, int training, float n, float* __restrict__ vals) {
  const int l = threadIdx.x & 15, Fc = F - Fk;
  const float inv_e = 1.f / (float)E;
  for (int64_t r = (int64_t)blockIdx.x * (FP_NTHR / 16) + (threadIdx.x >> 4); r < rows;
       r += (int64_t)gridDim.x * (FP_NTHR / 16)) {
    const int64_t b = r / F;
    const int f = (int)(r - b * F);
    if (f < Fc) {
      for (int e = l; e < E; e += 16) {
        const float k = gamma_bn[e] * rstd_bn[e], gv = g[r * E + e];
        vals[r * E + e] = training ? k * (gv - sum_g[e] / n - xhat[r * E + e] * (sum_gx[e] / n)) : k * gv;
      }
    } else {
      const int j = f - Fc;
      float dxh[4], xh[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = l + 16 * k;
        dxh[k] = e < E ? g[r * E + e] * gamma_ln[j * E + e] : 0.f;
        xh[k] = e < E ? xhat[r * E + e] : 0.f;
        s1 += dxh[k];
        s2 = fmaf(dxh[k], xh[k], s2);
      }
      s1 = group_sum<16>(s1) * inv_e;
      s2 = group_sum<16>(s2) * inv_e;
      const float k2 = rstd_ln[b * Fk + j] * values[b * Fk + j];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = l + 16 * k;
        if (e < E) vals[r * E + e] = k2 * (dxh[k] - s1 - xh[k] * s2);
      }
    }
  }
}

static int fp_in_shape(int64_t B, int F, int Fk, int E) {
  if (B < 0 || F < 0 || E < 0 || Fk < 0) return REC_E_ARG;
  if (F < 1 || F > FP_MAXF || E < 1 || E > FP_MAXE || (int64_t)F * E > FP_MAXD || Fk > F || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;                    // one field is an input stage; the body needs a pair
  return REC_OK;
}
static int fp_in_grid(int64_t rows) {
  const int64_t g = ceil_div64(rows, FP_NTHR / 16);
  return (int)(g < FP_IN_GRID ? g : FP_IN_GRID);
}
static int fp_in_slices(int64_t B) {
  const int64_t s = ceil_div64(B, 32);
  return (int)(s < 1 ? 1 : (s > FP_IN_SLICES ? FP_IN_SLICES : s));
}
// floats: sum [E] | m2 [E] | slots [S][max(Fc E, 2 Fc E + 2 Fk E)]
static size_t fp_in_ws_floats(int64_t B, int F, int E) {
  return 2 * (size_t)E + (size_t)fp_in_slices(B) * 2 * F * E;
}

// ------------------------------------------------------------------------------------------------------------------
// body
// ------------------------------------------------------------------------------------------------------------------
struct FpDims {
  int F, E, G, mid, O, type;
  int vec;                                       // E == 16 and W 16-byte aligned: rows of W as four float4 loads
};
__host__ __device__ inline int fp_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline int fp_pairs(int F) { return F * (F - 1) / 2; }
// columns of the LDS regions
__host__ __device__ inline int fp_r1(const FpDims& d) { return fp_max(fp_max(2 * d.G * d.F, d.F * d.E), d.O); }
__host__ __device__ inline int fp_r2(const FpDims& d) { return fp_max(fp_pairs(d.F), d.mid); }
__host__ __device__ inline int fp_ra(const FpDims& d) { return fp_max(d.F * d.E, d.O); }
__host__ __device__ inline int fp_rb(const FpDims& d) { return fp_max(fp_max(d.F * d.E, d.mid), fp_max(d.O, fp_pairs(d.F))); }
// bytes of dynamic LDS: regions | scratch [16][16] | pair table [P]
__host__ __device__ inline size_t fp_lds_bytes(const FpDims& d, int bwd) {
  const int cols = bwd ? d.F * d.E + fp_ra(d) + fp_rb(d) + d.mid : d.F * d.E + fp_r1(d) + fp_r2(d);
  return sizeof(float) * ((size_t)cols * FP_LD + FP_G * FP_T) + sizeof(int) * (size_t)fp_pairs(d.F);
}
constexpr size_t FP_LDS_CAP = 144 * 1024;
static_assert(sizeof(float) * ((size_t)(FP_MAXD + 2 * FP_MAXD + FP_MAXMID) * FP_LD + FP_G * FP_T) + sizeof(int) * FP_MAXP <=
                      FP_LDS_CAP && sizeof(float) * ((size_t)(3 * FP_MAXD + FP_MAXMID) * FP_LD + FP_G * FP_T) +
                      sizeof(int) * FP_MAXP <= FP_LDS_CAP && FP_LDS_CAP <= REC_LDS_CU_BYTES,
              "both kernels fit the LDS of a CU at the limits (2 G F <= 2 D, P <= 496, O <= 128)");
static_assert(FP_MAXP <= FP_MAXD && FP_MAXO <= FP_MAXD, "the regions of the largest shape");

// pair t of itertools.combinations(range(F), 2) as i | j << 8
__device__ __forceinline__ void fp_pair_table(int* pij, int F, int P, int tid) {
  for (int t = tid; t < P; t += FP_NTHR) {
    int i = 0, rem = t;
    while (rem >= F - 1 - i) {
      rem -= F - 1 - i;
      ++i;
    }
    pij[t] = i | ((i + 1 + rem) << 8);
  }
}
__device__ __forceinline__ int fp_pair_index(int i, int j, int F) { return i * (2 * F - i - 1) / 2 + j - i - 1; }
__device__ __forceinline__ int fp_weight_of(int type, int i, int t) {
  return type == FP_ALL ? 0 : (type == FP_EACH ? i : t);
}

// the sum over the 16 column groups of an example, groups added in order: every thread of the example gets the same bits
__device__ __forceinline__ float fp_rowsum(float v, float* sc, int b, int g) {
  sc[g * FP_T + b] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < FP_G; ++k) s += sc[k * FP_T + b];
  __syncthreads();
  return s;
}

// sum_k src[k][b] W[k ldw + c]
__device__ __forceinline__ float fp_dot(const float* src, int K, const float* __restrict__ W, int ldw, int c, int b) {
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(src[k * FP_LD + b], W[(int64_t)k * ldw + c], acc);
  return acc;
}
// sum_k src[k][b] W[c ldw + k]
__device__ __forceinline__ float fp_dot_t(const float* src, int K, const float* __restrict__ W, int ldw, int c, int b) {
  const float* w = W + (int64_t)c * ldw;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(src[k * FP_LD + b], w[k], acc);
  return acc;
}

// sum_k w[k] v[k] for one 16-float row of W (16-byte aligned): the additions in the order of the plain loop
__device__ __forceinline__ float fp_row16(const float* __restrict__ w, const float (&v)[16]) {
  const float4* w4 = reinterpret_cast<const float4*>(w);
  const float4 a = w4[0], b = w4[1], c = w4[2], d = w4[3];
  float u = fmaf(a.x, v[0], 0.f);
  u = fmaf(a.y, v[1], u);  u = fmaf(a.z, v[2], u);  u = fmaf(a.w, v[3], u);
  u = fmaf(b.x, v[4], u);  u = fmaf(b.y, v[5], u);  u = fmaf(b.z, v[6], u);  u = fmaf(b.w, v[7], u);
  u = fmaf(c.x, v[8], u);  u = fmaf(c.y, v[9], u);  u = fmaf(c.z, v[10], u); u = fmaf(c.w, v[11], u);
  u = fmaf(d.x, v[12], u); u = fmaf(d.y, v[13], u); u = fmaf(d.z, v[14], u); u = fmaf(d.w, v[15], u);
  return u;
}

// LayerNorm of R [n][17] over n per example, in place -> xhat; returns rstd.  Ends on a barrier.
__device__ __forceinline__ float fp_ln(float* R, int n, float* sc, int b, int g) {
  float s = 0.f;
  for (int c = g; c < n; c += FP_G) s += R[c * FP_LD + b];
  const float mean = fp_rowsum(s, sc, b, g) / (float)n;
  float q = 0.f;
  for (int c = g; c < n; c += FP_G) {
    const float d = R[c * FP_LD + b] - mean;
    q = fmaf(d, d, q);
  }
  const float rs = 1.f / sqrtf(fp_rowsum(q, sc, b, g) / (float)n + FP_EPS);
  for (int c = g; c < n; c += FP_G) R[c * FP_LD + b] = (R[c * FP_LD + b] - mean) * rs;
  __syncthreads();
  return rs;
}

// LayerNorm backward of Gd [n][17] (the gradient of the output) with XH = xhat, in place -> the gradient of the input.
// Ends on a barrier.
__device__ __forceinline__ void fp_ln_bwd(float* Gd, const float* XH, const float* __restrict__ gamma, int n, float rs,
                                          float* sc, int b, int g) {
  float s1 = 0.f, s2 = 0.f;
  for (int c = g; c < n; c += FP_G) {
    const float dxh = Gd[c * FP_LD + b] * gamma[c];
    s1 += dxh;
    s2 = fmaf(dxh, XH[c * FP_LD + b], s2);
  }
  s1 = fp_rowsum(s1, sc, b, g) / (float)n;
  s2 = fp_rowsum(s2, sc, b, g) / (float)n;
  for (int c = g; c < n; c += FP_G) {
    const float dxh = Gd[c * FP_LD + b] * gamma[c];
    Gd[c * FP_LD + b] = rs * (dxh - s1 - XH[c * FP_LD + b] * s2);
  }
  __syncthreads();
}

using Tile = TileOps<FP_T, FP_LD, FP_NTHR>;

struct FpFwdArgs {
  const float *x, *W, *Wr, *br, *gq, *bq, *S0, *b0, *g0, *be0, *S1, *b1, *g1, *be1;
  float *out, *p, *xhatq, *s, *xhat0, *h, *xhat1, *rstd;
};

__global__ __launch_bounds__(FP_NTHR) void fibinetplus_block_fwd_kernel(FpFwdArgs a, int64_t B, FpDims d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, b = tid & (FP_T - 1), g = tid >> 4;
  const int F = d.F, E = d.E, G = d.G, mid = d.mid, O = d.O, D = F * E, P = fp_pairs(F), S2 = 2 * G * F, w = E / G;
  float* xs = lds;                               // [D]: the x tile
  float* r1 = xs + D * FP_LD;                    // [max(2GF, D, O)]: z_q, then s, then z_1
  float* r2 = r1 + fp_r1(d) * FP_LD;             // [max(P, mid)]: p, then z_0 / h
  float* sc = r2 + fp_r2(d) * FP_LD;             // [16][16]
  int* pij = reinterpret_cast<int*>(sc + FP_G * FP_T);
  const int64_t r0 = (int64_t)blockIdx.x * FP_T;
  const int ldo = O + D;
  const bool mine = r0 + b < B;

  fp_pair_table(pij, F, P, tid);
  Tile::rows_in(xs, a.x, r0, B, D, 0, D, tid);
  __syncthreads();

  // bilinear+: one scalar per pair
  for (int t = g; t < P; t += FP_G) {
    const int i = pij[t] & 255, j = pij[t] >> 8;
    const float* Wm = a.W + (int64_t)fp_weight_of(d.type, i, t) * E * E;
    const float *xi = xs + i * E * FP_LD + b, *xj = xs + j * E * FP_LD + b;
    float acc = 0.f;
    if (d.vec) {                                              // x_j in registers, W by rows of four float4
      float xr[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) xr[k] = xj[k * FP_LD];
#pragma unroll 4
      for (int e = 0; e < 16; ++e) acc = fmaf(xi[e * FP_LD], fp_row16(Wm + e * 16, xr), acc);
    } else {
      for (int e = 0; e < E; ++e) {
        float u = 0.f;
        for (int k = 0; k < E; ++k) u = fmaf(Wm[e * E + k], xj[k * FP_LD], u);
        acc = fmaf(xi[e * FP_LD], u, acc);
      }
    }
    r2[t * FP_LD + b] = acc;
  }
  __syncthreads();
  if (a.p) Tile::rows_out(a.p, r2, r0, B, P, 0, P, tid);
  for (int o = g; o < O; o += FP_G) r1[o * FP_LD + b] = fp_dot(r2, P, a.Wr, O, o, b) + a.br[o];
  __syncthreads();
  {
    const float rs = fp_ln(r1, O, sc, b, g);
    if (a.rstd && mine && g == 0) a.rstd[(r0 + b) * 3] = rs;
  }
  for (int i = tid; i < FP_T * O; i += FP_NTHR) {
    const int row = i / O, o = i - row * O;
    if (r0 + row < B) {
      const float xh = r1[o * FP_LD + row];
      a.out[(r0 + row) * ldo + o] = xh * a.gq[o] + a.bq[o];
      if (a.xhatq) a.xhatq[(r0 + row) * O + o] = xh;
    }
  }
  __syncthreads();

  // SENet+: group means and maxima of every field
  const float inv_w = 1.f / (float)w;
  for (int idx = g; idx < F * G; idx += FP_G) {
    const int f = idx / G, gg = idx - f * G;
    const float* xr = xs + (f * E + gg * w) * FP_LD + b;
    float s = 0.f, m = xr[0];
    for (int e = 0; e < w; ++e) {
      const float v = xr[e * FP_LD];
      s += v;
      m = fmaxf(m, v);
    }
    r1[(f * 2 * G + gg) * FP_LD + b] = s * inv_w;
    r1[(f * 2 * G + G + gg) * FP_LD + b] = m;
  }
  __syncthreads();
  if (a.s) Tile::rows_out(a.s, r1, r0, B, S2, 0, S2, tid);
  for (int m = g; m < mid; m += FP_G) r2[m * FP_LD + b] = fp_dot(r1, S2, a.S0, mid, m, b) + a.b0[m];
  __syncthreads();
  {
    const float rs = fp_ln(r2, mid, sc, b, g);
    if (a.rstd && mine && g == 0) a.rstd[(r0 + b) * 3 + 1] = rs;
  }
  if (a.xhat0) Tile::rows_out(a.xhat0, r2, r0, B, mid, 0, mid, tid);
  __syncthreads();
  for (int m = g; m < mid; m += FP_G) r2[m * FP_LD + b] = fmaxf(r2[m * FP_LD + b] * a.g0[m] + a.be0[m], 0.f);
  __syncthreads();
  if (a.h) Tile::rows_out(a.h, r2, r0, B, mid, 0, mid, tid);
  for (int c = g; c < D; c += FP_G) r1[c * FP_LD + b] = fp_dot(r2, mid, a.S1, D, c, b) + a.b1[c];
  __syncthreads();
  {
    const float rs = fp_ln(r1, D, sc, b, g);
    if (a.rstd && mine && g == 0) a.rstd[(r0 + b) * 3 + 2] = rs;
  }
  for (int i = tid; i < FP_T * D; i += FP_NTHR) {
    const int row = i / D, c = i - row * D;
    if (r0 + row < B) {
      const float xh = r1[c * FP_LD + row];
      a.out[(r0 + row) * ldo + O + c] = xs[c * FP_LD + row] * fmaxf(xh * a.g1[c] + a.be1[c], 0.f);
      if (a.xhat1) a.xhat1[(r0 + row) * D + c] = xh;
    }
  }
}

struct FpBwdArgs {
  const float *x, *W, *Wr, *gq, *S0, *g0, *be0, *S1, *g1, *be1, *xhatq, *xhat0, *xhat1, *rstd, *dout;
  float *dx, *ws_dz1, *ws_dz0, *ws_dzq, *ws_dp, *slot_a, *slot_b;
};

// slot_a of a tile: dgq [O] | dbq [O] | dbr [O] | dg0 [mid] | dbe0 [mid] | db0 [mid]; slot_b: dg1 [D] | dbe1 [D] | db1 [D]
__global__ __launch_bounds__(FP_NTHR) void fibinetplus_block_bwd_kernel(FpBwdArgs a, int64_t B, FpDims d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, b = tid & (FP_T - 1), g = tid >> 4;
  const int F = d.F, E = d.E, G = d.G, mid = d.mid, O = d.O, D = F * E, P = fp_pairs(F), w = E / G;
  float* xs = lds;                               // [D]: the x tile
  float* ra = xs + D * FP_LD;                    // [max(D, O)]: dv -> dy1 -> dz1, dq -> dzq, then the dx tile
  float* rb = ra + fp_ra(d) * FP_LD;             // [max(D, mid, O, P)]: xhat1, xhat0, xhatq, then dp
  float* rc = rb + fp_rb(d) * FP_LD;             // [mid]: dy0 -> dz0
  float* sc = rc + mid * FP_LD;
  int* pij = reinterpret_cast<int*>(sc + FP_G * FP_T);
  const int64_t r0 = (int64_t)blockIdx.x * FP_T;
  const int ldo = O + D;
  const bool mine = r0 + b < B;
  float* __restrict__ sa = a.slot_a + (int64_t)blockIdx.x * 3 * (O + mid);
  float* __restrict__ sb = a.slot_b + (int64_t)blockIdx.x * 3 * D;
  const float rsq = mine ? a.rstd[(r0 + b) * 3] : 0.f, rs0 = mine ? a.rstd[(r0 + b) * 3 + 1] : 0.f,
              rs1 = mine ? a.rstd[(r0 + b) * 3 + 2] : 0.f;

  fp_pair_table(pij, F, P, tid);
  Tile::rows_in(xs, a.x, r0, B, D, 0, D, tid);
  Tile::rows_in(ra, a.dout + O, r0, B, ldo, 0, D, tid);
  Tile::rows_in(rb, a.xhat1, r0, B, D, 0, D, tid);
  __syncthreads();

  // v = x (.) A, A = relu(xhat1 g1 + be1): dy1 = dv x [A > 0]
  for (int c = g; c < D; c += FP_G) {
    const float pre = rb[c * FP_LD + b] * a.g1[c] + a.be1[c];
    ra[c * FP_LD + b] = pre > 0.f ? ra[c * FP_LD + b] * xs[c * FP_LD + b] : 0.f;
  }
  __syncthreads();
  Tile::col_sums(sb, ra, D, tid, rb);
  Tile::col_sums(sb + D, ra, D, tid);
  fp_ln_bwd(ra, rb, a.g1, D, rs1, sc, b, g);
  Tile::rows_out(a.ws_dz1, ra, r0, B, D, 0, D, tid);
  Tile::col_sums(sb + 2 * D, ra, D, tid);
  __syncthreads();                                             // rb (xhat1) is rewritten

  // h = relu(xhat0 g0 + be0): dy0 = (dz1 S1^T) [h > 0]
  Tile::rows_in(rb, a.xhat0, r0, B, mid, 0, mid, tid);
  __syncthreads();
  for (int m = g; m < mid; m += FP_G) {
    const float pre = rb[m * FP_LD + b] * a.g0[m] + a.be0[m];
    const float dh = fp_dot_t(ra, D, a.S1, D, m, b);
    rc[m * FP_LD + b] = pre > 0.f ? dh : 0.f;
  }
  __syncthreads();
  Tile::col_sums(sa + 3 * O, rc, mid, tid, rb);
  Tile::col_sums(sa + 3 * O + mid, rc, mid, tid);
  fp_ln_bwd(rc, rb, a.g0, mid, rs0, sc, b, g);
  Tile::rows_out(a.ws_dz0, rc, r0, B, mid, 0, mid, tid);
  Tile::col_sums(sa + 3 * O + 2 * mid, rc, mid, tid);
  __syncthreads();                                             // ra (dz1) and rb (xhat0) are rewritten

  // q = LN(p Wr + br): dzq, dp = dzq Wr^T
  Tile::rows_in(ra, a.dout, r0, B, ldo, 0, O, tid);
  Tile::rows_in(rb, a.xhatq, r0, B, O, 0, O, tid);
  __syncthreads();
  Tile::col_sums(sa, ra, O, tid, rb);
  Tile::col_sums(sa + O, ra, O, tid);
  fp_ln_bwd(ra, rb, a.gq, O, rsq, sc, b, g);
  Tile::rows_out(a.ws_dzq, ra, r0, B, O, 0, O, tid);
  Tile::col_sums(sa + 2 * O, ra, O, tid);
  for (int t = g; t < P; t += FP_G) rb[t * FP_LD + b] = fp_dot_t(ra, O, a.Wr, O, t, b);
  __syncthreads();
  Tile::rows_out(a.ws_dp, rb, r0, B, P, 0, P, tid);

  // dx: the direct part dv (.) A in rows, then every thread adds the squeeze and the bilinear parts of its columns
  for (int i = tid; i < FP_T * D; i += FP_NTHR) {
    const int row = i / D, c = i - row * D;
    float v = 0.f;
    if (r0 + row < B)
      v = a.dout[(r0 + row) * ldo + O + c] * fmaxf(a.xhat1[(r0 + row) * D + c] * a.g1[c] + a.be1[c], 0.f);
    ra[c * FP_LD + row] = v;
  }
  __syncthreads();
  const float inv_w = 1.f / (float)w;
  for (int c = g; c < D; c += FP_G) {
    const int f = c / E, e = c - f * E, gg = e / w;
    float val = ra[c * FP_LD + b];
    // s: the mean's share and, at the first arg-max of the group, the maximum's
    const float dsm = fp_dot_t(rc, mid, a.S0, mid, f * 2 * G + gg, b);
    const float dsx = fp_dot_t(rc, mid, a.S0, mid, f * 2 * G + G + gg, b);
    const float* xg = xs + (f * E + gg * w) * FP_LD + b;
    int arg = 0;
    float m = xg[0];
    for (int k = 1; k < w; ++k) {
      const float v = xg[k * FP_LD];
      if (v > m) {
        m = v;
        arg = k;
      }
    }
    val += dsm * inv_w;
    if (e - gg * w == arg) val += dsx;
    // p_ij = x_i W x_j^T: field f as the left operand (j > f) and as the right one (i < f)
    for (int j = f + 1; j < F; ++j) {
      const int t = fp_pair_index(f, j, F);
      const float* Wm = a.W + (int64_t)fp_weight_of(d.type, f, t) * E * E + e * E;
      const float* xj = xs + j * E * FP_LD + b;
      float u = 0.f;
      if (d.vec) {
        float xr[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) xr[k] = xj[k * FP_LD];
        u = fp_row16(Wm, xr);
      } else {
        for (int k = 0; k < E; ++k) u = fmaf(Wm[k], xj[k * FP_LD], u);
      }
      val = fmaf(rb[t * FP_LD + b], u, val);
    }
    for (int i = 0; i < f; ++i) {
      const int t = fp_pair_index(i, f, F);
      const float* Wm = a.W + (int64_t)fp_weight_of(d.type, i, t) * E * E + e;
      const float* xi = xs + i * E * FP_LD + b;
      float u = 0.f;
      for (int k = 0; k < E; ++k) u = fmaf(Wm[k * E], xi[k * FP_LD], u);
      val = fmaf(rb[t * FP_LD + b], u, val);
    }
    ra[c * FP_LD + b] = val;
  }
  __syncthreads();
  Tile::rows_out(a.dx, ra, r0, B, D, 0, D, tid);
}

// Bilinear weight gradients, all of them in one launch: workgroup (matrix wi and a block of 256 outputs, slice s) adds,
// over the pairs (i, j) that use matrix wi and the examples of batch slice s, in order, dp[b, pair] x_i[b]^T x_j[b]
// into part[s][wi] [E][E], one output per thread; the slices are added by rec_slot_sum in slice order.
__global__ __launch_bounds__(FP_NTHR) void fibinetplus_dw_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ dp, int64_t B, int F, int E,
                                                                 int type, int nW, int nblk, int64_t per,
                                                                 float* __restrict__ part) {
  __shared__ float us[FP_DW_ROWS * FP_MAXE], vs[FP_DW_ROWS * FP_MAXE];
  const int tid = threadIdx.x, wi = blockIdx.x / nblk, D = F * E, EE = E * E, P = fp_pairs(F);
  const int o = (blockIdx.x - wi * nblk) * FP_NTHR + tid;
  const bool own = o < EE;
  const int oe = own ? o / E : 0, oj = own ? o - oe * E : 0;
  const int64_t b0 = (int64_t)blockIdx.y * per, b1 = b0 + per < B ? b0 + per : B;
  int i0 = 0, i1 = F - 1, jf = -1;               // 'all': every pair
  if (type == FP_EACH) {
    i0 = wi;
    i1 = wi + 1;
  } else if (type == FP_INTERACTION) {
    int i = 0, rem = wi;
    while (rem >= F - 1 - i) {
      rem -= F - 1 - i;
      ++i;
    }
    i0 = i;
    i1 = i + 1;
    jf = i + 1 + rem;
  }
  float acc = 0.f;
  for (int i = i0; i < i1; ++i) {
    const int ja = jf >= 0 ? jf : i + 1, jb = jf >= 0 ? jf + 1 : F;
    for (int j = ja; j < jb; ++j) {
      const int t = fp_pair_index(i, j, F);
      for (int64_t bb = b0; bb < b1; bb += FP_DW_ROWS) {
        for (int q = tid; q < FP_DW_ROWS * E; q += FP_NTHR) {
          const int r = q / E, e = q - r * E;
          const bool in = bb + r < b1;
          us[q] = in ? dp[(bb + r) * P + t] * x[(bb + r) * D + i * E + e] : 0.f;
          vs[q] = in ? x[(bb + r) * D + j * E + e] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < FP_DW_ROWS; ++r) acc = fmaf(us[r * E + oe], vs[r * E + oj], acc);
        __syncthreads();
      }
    }
  }
  if (own) part[((int64_t)blockIdx.y * nW + wi) * EE + o] = acc;
}

static int fp_shape(int64_t B, const FpDims& d) {
  if (B < 0 || d.F < 0 || d.E < 0 || d.G < 0 || d.mid < 0 || d.O < 0) return REC_E_ARG;
  if (d.F < 2 || d.F > FP_MAXF || d.E < 1 || d.E > FP_MAXE || (int64_t)d.F * d.E > FP_MAXD || d.O < 1 ||
      d.O > FP_MAXO || d.mid < 1 || d.mid > FP_MAXMID || d.G < 1 || d.type < FP_ALL ||
      d.type > FP_INTERACTION || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;
  if (d.E % d.G) return REC_E_ARG;
  return REC_OK;
}
static int fp_num_weights(const FpDims& d) {
  return d.type == FP_ALL ? 1 : (d.type == FP_EACH ? d.F - 1 : fp_pairs(d.F));
}

struct FpWs {
  size_t dz1, dz0, dzq, dp, slot_a, slot_b, part, gemm, total;   // offsets in floats
};
static FpWs fp_ws(int64_t B, const FpDims& d) {
  FpWs w{};
  const size_t b = (size_t)B, tiles = (size_t)ceil_div64(B, FP_T), D = (size_t)d.F * d.E, P = (size_t)fp_pairs(d.F);
  const size_t mid = (size_t)d.mid, O = (size_t)d.O, S2 = (size_t)2 * d.G * d.F;
  WsCarve c;
  w.dz1 = c.take(b * D);
  w.dz0 = c.take(b * mid);
  w.dzq = c.take(b * O);
  w.dp = c.take(b * P);
  w.slot_a = c.take(tiles * 3 * (O + mid));
  w.slot_b = c.take(tiles * 3 * D);
  w.part = c.take((size_t)mb_small_split(B) * fp_num_weights(d) * d.E * d.E);
  const size_t g1 = mb_dw_gemm_floats(B, (int)P, d.O), g2 = mb_dw_gemm_floats(B, (int)S2, d.mid),
               g3 = mb_dw_gemm_floats(B, d.mid, (int)D);
  w.gemm = c.take(g1 > g2 ? (g1 > g3 ? g1 : g3) : (g2 > g3 ? g2 : g3));
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" size_t rec_emb_fibinetplus_in_workspace_bytes(int64_t B, int F, int Fk, int E) {
  if (fp_in_shape(B, F, Fk, E) != REC_OK) return 0;
  return sizeof(float) * (fp_in_ws_floats(B, F, E) + 4);
}

extern "C" int rec_emb_fibinetplus_in_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X,
                                              const float* values, const float* gamma_bn, const float* beta_bn,
                                              const float* gamma_ln, const float* beta_ln, int64_t B, int F, int Fk,
                                              int training, float* moving_mean, float* moving_var, float* x,
                                              float* xhat, float* rstd_bn, float* rstd_ln, int* oob_flag,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = fp_in_shape(B, F, Fk, E)) return rc;
  if (V <= 0 || ld < E) return REC_E_ARG;
  if (B == 0) return REC_OK;
  const int Fc = F - Fk;
  if (!table || !X || !x || !workspace || (Fk > 0 && (!values || !gamma_ln || !beta_ln)) ||
      (Fc > 0 && (!gamma_bn || !beta_bn || !moving_mean || !moving_var)))
    return REC_E_ARG;
  const bool save = xhat || rstd_bn || rstd_ln;
  if (save && !(xhat && (rstd_bn || Fc == 0) && (rstd_ln || Fk == 0))) return REC_E_ARG;   // all of them or none
  if (workspace_bytes < sizeof(float) * fp_in_ws_floats(B, F, E)) return REC_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  const int64_t rows = B * F;
  const bool batch_stats = training != 0 && Fc > 0;
  hipLaunchKernelGGL(fp_in_gather_kernel, dim3(fp_in_grid(rows)), dim3(FP_NTHR), 0, st, table, V, E, ld, X, values,
                     gamma_bn, beta_bn, gamma_ln, beta_ln, moving_mean, moving_var, rows, F, Fk, batch_stats ? 1 : 0, x,
                     xhat, rstd_bn, rstd_ln, oob_flag);
  REC_LAUNCH_CHECK();
  if (!batch_stats) return REC_OK;
  float* sum = static_cast<float*>(workspace);
  float *m2 = sum + E, *slots = m2 + E;
  const int S = fp_in_slices(B), ce = Fc * E;
  const int64_t per = ceil_div64(B, S);
  const float n = (float)(B * Fc);
  hipLaunchKernelGGL(fp_in_colsum_kernel<0>, dim3(S), dim3(FP_NTHR), 0, st, x, sum, B, F * E, ce, E, per, n, slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, E, S * Fc, slots, {{sum}, {E}}, st)) return rc;
  hipLaunchKernelGGL(fp_in_colsum_kernel<1>, dim3(S), dim3(FP_NTHR), 0, st, x, sum, B, F * E, ce, E, per, n, slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, E, S * Fc, slots, {{m2}, {E}}, st)) return rc;
  const int64_t elems = B * ce > E ? B * ce : E;
  hipLaunchKernelGGL(fp_in_apply_kernel, dim3((unsigned)ceil_div64(elems, FP_NTHR)), dim3(FP_NTHR), 0, st, sum, m2,
                     gamma_bn, beta_bn, B, F, Fc, E, n, moving_mean, moving_var, x, xhat, rstd_bn);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_emb_fibinetplus_in_bwd_f32(const float* dx, const float* values, const float* xhat,
                                              const float* rstd_bn, const float* rstd_ln, const float* gamma_bn,
                                              const float* gamma_ln, int64_t B, int F, int Fk, int E, int training,
                                              float* vals, float* dgamma_bn, float* dbeta_bn, float* dgamma_ln,
                                              float* dbeta_ln, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = fp_in_shape(B, F, Fk, E)) return rc;
  if (B == 0) return REC_OK;
  const int Fc = F - Fk;
  if (!dx || !xhat || !vals || !workspace || (Fk > 0 && (!values || !rstd_ln || !gamma_ln || !dgamma_ln || !dbeta_ln)) ||
      (Fc > 0 && (!rstd_bn || !gamma_bn || !dgamma_bn || !dbeta_bn)))
    return REC_E_ARG;
  if (workspace_bytes < sizeof(float) * fp_in_ws_floats(B, F, E)) return REC_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  const int S = fp_in_slices(B), ce = Fc * E, ke = Fk * E;
  const int64_t per = ceil_div64(B, S), rows = B * F;
  float* slot_c = static_cast<float*>(workspace) + 2 * E;
  float* slot_k = slot_c + (size_t)S * 2 * ce;
  hipLaunchKernelGGL(fp_in_bwd_colsum_kernel, dim3(S), dim3(FP_NTHR), 0, st, dx, xhat, B, F, Fc, E, per, slot_c, slot_k);
  REC_LAUNCH_CHECK();
  if (Fc > 0)
    if (int rc = rec_slot_sum(REC_SLOTS_WAVE, 2 * E, S * Fc, slot_c, {{dbeta_bn, dgamma_bn}, {E, E}}, st)) return rc;
  if (Fk > 0)
    if (int rc = rec_slot_sum(REC_SLOTS_WAVE, 2 * ke, S, slot_k, {{dbeta_ln, dgamma_ln}, {ke, ke}}, st)) return rc;
  hipLaunchKernelGGL(fp_in_bwd_apply_kernel, dim3(fp_in_grid(rows)), dim3(FP_NTHR), 0, st, dx, values, xhat, rstd_bn,
                     rstd_ln, gamma_bn, gamma_ln, dbeta_bn, dgamma_bn, rows, F, Fk, E, training != 0 ? 1 : 0,
                     (float)(B * Fc), vals);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" size_t rec_fibinetplus_block_workspace_bytes(int64_t B, int F, int E, int G, int mid, int O, int type) {
  const FpDims d{F, E, G, mid, O, type, 0};
  if (fp_shape(B, d) != REC_OK) return 0;
  return sizeof(float) * (fp_ws(B, d).total + 4);
}

extern "C" int rec_fibinetplus_block_fwd_f32(const float* x, const float* W, const float* Wr, const float* br,
                                             const float* gamma_q, const float* beta_q, const float* S0,
                                             const float* b0, const float* gamma0, const float* beta0, const float* S1,
                                             const float* b1, const float* gamma1, const float* beta1, int64_t B, int F,
                                             int E, int G, int mid, int O, int type, float* out, float* p, float* xhat_q,
                                             float* s, float* xhat0, float* h, float* xhat1, float* rstd, void* stream) {
  const FpDims d{F, E, G, mid, O, type, E == 16 && rec_is_aligned16(W)};
  if (int rc = fp_shape(B, d)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !W || !Wr || !br || !gamma_q || !beta_q || !S0 || !b0 || !gamma0 || !beta0 || !S1 || !b1 || !gamma1 ||
      !beta1 || !out)
    return REC_E_ARG;
  const bool save = p || xhat_q || s || xhat0 || h || xhat1 || rstd;
  if (save && !(p && xhat_q && s && xhat0 && h && xhat1 && rstd)) return REC_E_ARG;   // all of them or none
  if (hipError_t e = rec_allow_lds<fibinetplus_block_fwd_kernel>(FP_LDS_CAP)) return (int)e;
  const FpFwdArgs a{x, W, Wr, br, gamma_q, beta_q, S0, b0, gamma0, beta0, S1, b1, gamma1, beta1,
                    out, p, xhat_q, s, xhat0, h, xhat1, rstd};
  hipLaunchKernelGGL(fibinetplus_block_fwd_kernel, dim3((unsigned)ceil_div64(B, FP_T)), dim3(FP_NTHR),
                     fp_lds_bytes(d, 0), as_stream(stream), a, B, d);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_fibinetplus_block_bwd_f32(const float* x, const float* W, const float* Wr, const float* gamma_q,
                                             const float* S0, const float* gamma0, const float* beta0, const float* S1,
                                             const float* gamma1, const float* beta1, const float* p,
                                             const float* xhat_q, const float* s, const float* xhat0, const float* h,
                                             const float* xhat1, const float* rstd, const float* dout, int64_t B, int F,
                                             int E, int G, int mid, int O, int type, float* dx, float* dW, float* dWr,
                                             float* dbr, float* dgamma_q, float* dbeta_q, float* dS0, float* db0,
                                             float* dgamma0, float* dbeta0, float* dS1, float* db1, float* dgamma1,
                                             float* dbeta1, void* workspace, size_t workspace_bytes, void* stream) {
  const FpDims d{F, E, G, mid, O, type, E == 16 && rec_is_aligned16(W)};
  if (int rc = fp_shape(B, d)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !W || !Wr || !gamma_q || !S0 || !gamma0 || !beta0 || !S1 || !gamma1 || !beta1 || !p || !xhat_q || !s ||
      !xhat0 || !h || !xhat1 || !rstd || !dout || !dx || !dW || !dWr || !dbr || !dgamma_q || !dbeta_q || !dS0 || !db0 ||
      !dgamma0 || !dbeta0 || !dS1 || !db1 || !dgamma1 || !dbeta1 || !workspace)
    return REC_E_ARG;
  const FpWs w = fp_ws(B, d);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  float *dz1 = base + w.dz1, *dz0 = base + w.dz0, *dzq = base + w.dzq, *dp = base + w.dp, *slot_a = base + w.slot_a,
        *slot_b = base + w.slot_b, *part = base + w.part, *gws = base + w.gemm;
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, FP_T), D = F * E, P = fp_pairs(F), S2 = 2 * G * F;
  if (hipError_t e = rec_allow_lds<fibinetplus_block_bwd_kernel>(FP_LDS_CAP)) return (int)e;
  const FpBwdArgs a{x, W, Wr, gamma_q, S0, gamma0, beta0, S1, gamma1, beta1, xhat_q, xhat0, xhat1, rstd, dout,
                    dx, dz1, dz0, dzq, dp, slot_a, slot_b};
  hipLaunchKernelGGL(fibinetplus_block_bwd_kernel, dim3(tiles), dim3(FP_NTHR), fp_lds_bytes(d, 1), st, a, B, d);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, 3 * (O + mid), tiles, slot_a,
                            {{dgamma_q, dbeta_q, dbr, dgamma0, dbeta0, db0}, {O, O, O, mid, mid, mid}}, st))
    return rc;
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, 3 * D, tiles, slot_b, {{dgamma1, dbeta1, db1}, {D, D, D}}, st)) return rc;
  const int S = mb_small_split(B), nW = fp_num_weights(d);
  const int64_t per = ceil_div64(ceil_div64(B, S), FP_DW_ROWS) * FP_DW_ROWS;
  const int nblk = (E * E + FP_NTHR - 1) / FP_NTHR;
  hipLaunchKernelGGL(fibinetplus_dw_kernel, dim3(nW * nblk, S), dim3(FP_NTHR), 0, st, x, dp, B, F, E, type, nW, nblk,
                     per, part);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_SERIAL, nW * E * E, S, part, {{dW}, {nW * E * E}}, st)) return rc;
  if (int rc = mb_dw_gemm(P, O, B, p, dzq, dWr, gws, stream)) return rc;         // dWr = p^T dzq
  if (int rc = mb_dw_gemm(S2, mid, B, s, dz0, dS0, gws, stream)) return rc;      // dS0 = s^T dz0
  return mb_dw_gemm(mid, D, B, h, dz1, dS1, gws, stream);                        // dS1 = h^T dz1
}
