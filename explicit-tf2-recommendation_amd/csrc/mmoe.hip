// MMOE / ESMM (MMOELayer / ESMMLayer, 4.MMOE/CustomLayers.py:107-245) on gfx950: n expert MLPs and T gate MLPs over one
// input, the gate-weighted expert outputs flattened into T towers.
//
// x [B, D]; N1 = (n + T) H1.  Packed weights:
//   W1 [D, N1], b1 [N1]        first layer of all experts and gates: column block i < n is expert i, block n + t gate t
//   We2 [n, H1, O], be2 [n, O]      Wg2 [T, H1, n], bg2 [T, n]
//   Wt1 [T, n O, H2], bt1 [T, H2]   Wt2 [T, H2, O2], bt2 [T, O2]   Wt3 [T, O2], bt3 [T]
//   h = relu(x W1 + b1)   e_i = relu(h_i We2[i] + be2[i])   z_t = relu(h_{n+t} Wg2[t] + bg2[t])
//   g_t = softmax(z_t), once (MMOE) or twice (ESMM)          u_t[i O + o] = e_i[o] g_t[i]   (flattened, not summed)
//   a1_t = relu(u_t Wt1[t] + bt1[t])   a2_t = relu(a1_t Wt2[t] + bt2[t])   p_t = sigmoid(a2_t Wt3[t] + bt3[t])
//   out[:, t] = p_t;  ctcvr: out[:, 1] = p_0 p_1
// Forward, one launch.  A workgroup of 4 waves owns 32 examples (mfma_tile.h): x is staged k-major in LDS and x W1 runs on
// v_mfma_f32_32x32x2_f32, N1 <= 512 being exactly the 4 x 4 x 32 accumulator columns of mb_mma.  h stays in LDS
// ([N1][33]); everything after it runs on the VALU out of LDS: thread t owns example t & 31 and the columns t / 32,
// t / 32 + 8, ... of a stage, so the 32 lanes of a half wave read 32 consecutive banks of an operand and ONE weight (a
// broadcast load).  These products have K <= 128 and at most 128 columns per task, about 12 % of the forward's flops at
// the default shape; an MFMA tile would be mostly padding (O = 8, n = 3 columns) and the gate multiply, the softmax and
// the relu masks sit between them.
// Training saves h, e, z, g (the gate after the last softmax), a1, a2 and p; inference writes out alone, the same bits.
// Backward.  One launch runs the per-example chain of a tile back from dout to dZ1 (the gradient before the first relu)
// and dx = dZ1 W1^T (MFMA).  Every stage computes its unmasked gradient into LDS; a second pass with rows of consecutive
// columns applies the relu mask from the saved activation and writes the workspace copy that the weight gradients read.
// The first softmax of a double one is recomputed from z by the forward's own code.  The tile's column sums (the bias
// gradients) go to the tile's slot; the entry point adds the slots (rec_slot_sum), runs ALL small weight gradients
// (dWe2, dWg2, dWt1, dWt2, dWt3) as one launch over (matrix, block of 256 outputs, batch slice) whose at most 16 slices
// a second slot sum adds in order, and enqueues dW1 = x^T dZ1 on rec_gemm_f32 (split-K, slices added in order).
// No float atomics and no value with two writers: bit-identical results run to run; no host synchronisation.
// Contraction is off: a softmax over ONE expert must return exactly zero gradients, which g (dg - dg g) only does when
// both terms are the same rounded product.
// Shared with the other tile kernels, in tile_ops.h: the row / column / softmax passes over an LDS operand (TileOps), the
// small weight-gradient kernel and its launch (this file supplies the matrices: MmSmall), the workspace carving and the
// split-K weight-gradient GEMM; the MFMA tile itself is mfma_tile.h.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

namespace {

// the limits are MaskNet's: the header gains no constant for this family
constexpr int MM_MAXD = REC_MASKNET_MAX_D, MM_MAXN1 = REC_MASKNET_MAX_P, MM_MAXO = REC_MASKNET_MAX_O;
constexpr int MM_MAXT = REC_MASKNET_MAX_R;
constexpr int MM_NTHR = 256;
constexpr int MM_G = MM_NTHR / MB_T;             // column groups of the VALU stages

static_assert(MM_MAXN1 <= 128 * MB_NJ && MM_MAXD <= 128 * MB_NJ, "accumulator blocks per wave");
static_assert(MM_MAXT <= MM_G - 1, "one thread per (example, task), and one more");

struct MmDims {
  int D, n, T, H1, O, H2, O2;
  __host__ __device__ int N1() const { return (n + T) * H1; }
  __host__ __device__ int nO() const { return n * O; }
  __host__ __device__ int Tn() const { return T * n; }
};

// rows of LDS ([.][33] floats each):
//   forward   hs [even(N1)] | max(xs [even(D)], es [nO] zs [Tn] gs [Tn] a1s [H2] a2s [O2] ps [T])
//   backward  des [nO] dzs [Tn] | max(dZ1 [even(N1)], es [nO] gs [Tn] g1s [Tn] dus [nO] d1s [H2] d2s [O2] dls [T] ps [T])
__host__ __device__ inline int mm_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline size_t mm_lds_floats(const MmDims& d, int bwd) {
  const int N1e = mb_even(d.N1());
  const int rows = bwd ? d.nO() + d.Tn() + mm_max(N1e, 2 * d.nO() + 2 * d.Tn() + d.H2 + d.O2 + 2 * d.T)
                       : N1e + mm_max(mb_even(d.D), d.nO() + 2 * d.Tn() + d.H2 + d.O2 + d.T);
  return (size_t)rows * MB_LD;
}
constexpr size_t MM_LDS_CAP = REC_POSO_LDS_CAP;
// n O, T n, H2, O2 <= MM_MAXO
static_assert(sizeof(float) * (MM_MAXN1 + 5 * MM_MAXO + MM_MAXT) * MB_LD <= MM_LDS_CAP &&
                  sizeof(float) * (2 * MM_MAXO + 6 * MM_MAXO + 2 * MM_MAXT) * MB_LD <= MM_LDS_CAP &&
                  MM_LDS_CAP <= REC_LDS_CU_BYTES,
              "both directions of the largest shape fit the LDS of a CU");

using Tile = TileOps<MB_T, MB_LD, MM_NTHR>;

__global__ __launch_bounds__(MM_NTHR) void mmoe_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ We2, const float* __restrict__ be2, const float* __restrict__ Wg2,
    const float* __restrict__ bg2, const float* __restrict__ Wt1, const float* __restrict__ bt1,
    const float* __restrict__ Wt2, const float* __restrict__ bt2, const float* __restrict__ Wt3,
    const float* __restrict__ bt3, int64_t B, MmDims d, int passes, int ctcvr, float* __restrict__ out,
    float* __restrict__ sh, float* __restrict__ se, float* __restrict__ sz, float* __restrict__ sg,
    float* __restrict__ sa1, float* __restrict__ sa2, float* __restrict__ sp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = d.D, n = d.n, T = d.T, H1 = d.H1, O = d.O, H2 = d.H2, O2 = d.O2;
  const int N1 = d.N1(), nO = d.nO(), Tn = d.Tn(), De = mb_even(D);
  float* hs = lds;                               // [even(N1)][33]
  float* xs = hs + mb_even(N1) * MB_LD;          // [De][33]: the x tile; the small operands once h is there
  float* es = xs;                                // [nO]   es and zs are one operand of nO + Tn columns
  float* zs = es + nO * MB_LD;                   // [Tn]
  float* gs = zs + Tn * MB_LD;                   // [Tn]
  float* a1s = gs + Tn * MB_LD;                  // [H2]
  float* a2s = a1s + H2 * MB_LD;                 // [O2]
  float* ps = a2s + O2 * MB_LD;                  // [T]
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;
  const int b = tid & (MB_T - 1), g = tid >> 5;

  for (int i = tid; i < MB_T * De; i += MM_NTHR) {
    const int m = i / De, k = i - m * De;
    xs[k * MB_LD + m] = (k < D && r0 + m < B) ? x[(r0 + m) * D + k] : 0.f;
  }
  __syncthreads();

  {
    f32x16 acc[MB_NJ];
#pragma unroll
    for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
    mb_mma<false>(acc, xs, D, W1, N1, 0, N1, wave, lo, hi);
#pragma unroll
    for (int j = 0; j < MB_NJ; ++j) {
      const int col = (wave + 4 * j) * 32 + lo;
      if ((wave + 4 * j) * 32 < N1 && col < N1) {
        const float bc = b1[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mb_row(r, hi);
          const float hv = fmaxf(acc[j][r] + bc, 0.f);
          hs[col * MB_LD + row] = hv;
          if (sh && r0 + row < B) sh[(r0 + row) * N1 + col] = hv;
        }
      }
    }
  }
  __syncthreads();                               // every read of the x tile lies before it: es .. ps may be written

  for (int c = g; c < nO + Tn; c += MM_G) {      // second layer of the experts and of the gates
    const float* W;
    const float* hp;
    int ldw;
    float bias;
    if (c < nO) {
      const int i = c / O, o = c - i * O;
      W = We2 + (int64_t)i * H1 * O + o;
      ldw = O;
      bias = be2[c];
      hp = hs + i * H1 * MB_LD + b;
    } else {
      const int cc = c - nO, t = cc / n, j = cc - t * n;
      W = Wg2 + (int64_t)t * H1 * n + j;
      ldw = n;
      bias = bg2[cc];
      hp = hs + (n + t) * H1 * MB_LD + b;
    }
    float acc = 0.f;
    for (int k = 0; k < H1; ++k) acc = fmaf(hp[k * MB_LD], W[k * ldw], acc);
    es[c * MB_LD + b] = fmaxf(acc + bias, 0.f);
  }
  __syncthreads();
  if (se) {
    Tile::rows_out(se, es, r0, B, nO, 0, nO, tid);
    Tile::rows_out(sz, zs, r0, B, Tn, 0, Tn, tid);
  }
  if (g < T) {
    Tile::softmax(zs + g * n * MB_LD + b, gs + g * n * MB_LD + b, n);
    if (passes == 2) Tile::softmax(gs + g * n * MB_LD + b, gs + g * n * MB_LD + b, n);
  }
  __syncthreads();
  if (sg) Tile::rows_out(sg, gs, r0, B, Tn, 0, Tn, tid);

  for (int t = 0; t < T; ++t) {                  // the towers, one task at a time
    for (int c = g; c < H2; c += MM_G) {
      const float* W = Wt1 + (int64_t)t * nO * H2 + c;
      float acc = 0.f;
      for (int i = 0; i < n; ++i) {
        const float gv = gs[(t * n + i) * MB_LD + b];
        for (int o = 0; o < O; ++o) {
          const int k = i * O + o;
          acc = fmaf(es[k * MB_LD + b] * gv, W[(int64_t)k * H2], acc);
        }
      }
      a1s[c * MB_LD + b] = fmaxf(acc + bt1[t * H2 + c], 0.f);
    }
    __syncthreads();
    for (int c = g; c < O2; c += MM_G) {
      const float* W = Wt2 + (int64_t)t * H2 * O2 + c;
      float acc = 0.f;
      for (int k = 0; k < H2; ++k) acc = fmaf(a1s[k * MB_LD + b], W[k * O2], acc);
      a2s[c * MB_LD + b] = fmaxf(acc + bt2[t * O2 + c], 0.f);
    }
    if (sa1) Tile::rows_out(sa1, a1s, r0, B, T * H2, t * H2, H2, tid);
    __syncthreads();
    if (g == 0) {
      float acc = 0.f;
      for (int k = 0; k < O2; ++k) acc = fmaf(a2s[k * MB_LD + b], Wt3[t * O2 + k], acc);
      ps[t * MB_LD + b] = sigmoid_acc(acc + bt3[t]);
    }
    if (sa2) Tile::rows_out(sa2, a2s, r0, B, T * O2, t * O2, O2, tid);
    __syncthreads();                             // a1s and a2s are rewritten by the next task
  }
  for (int i = tid; i < MB_T * T; i += MM_NTHR) {
    const int row = i / T, t = i - row * T;
    if (r0 + row < B) {
      const float pv = ps[t * MB_LD + row];
      out[(r0 + row) * T + t] = (ctcvr && t == 1) ? ps[row] * pv : pv;
      if (sp) sp[(r0 + row) * T + t] = pv;
    }
  }
}

// slot of a tile: db1 [N1] | dbe2 [nO] | dbg2 [Tn] | dbt1 [T H2] | dbt2 [T O2] | dbt3 [T]
__host__ __device__ inline int mm_slot_floats(const MmDims& d) {
  return d.N1() + d.nO() + d.Tn() + d.T * d.H2 + d.T * d.O2 + d.T;
}

__global__ __launch_bounds__(MM_NTHR) void mmoe_bwd_kernel(
    const float* __restrict__ W1, const float* __restrict__ We2, const float* __restrict__ Wg2,
    const float* __restrict__ Wt1, const float* __restrict__ Wt2, const float* __restrict__ Wt3,
    const float* __restrict__ h, const float* __restrict__ e, const float* __restrict__ z,
    const float* __restrict__ gt, const float* __restrict__ a1, const float* __restrict__ a2,
    const float* __restrict__ p, const float* __restrict__ dout, int64_t B, MmDims d, int passes, int ctcvr,
    float* __restrict__ dx, float* __restrict__ ws_dz1, float* __restrict__ ws_dze, float* __restrict__ ws_dzz,
    float* __restrict__ ws_d1, float* __restrict__ ws_d2, float* __restrict__ ws_dl, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = d.D, n = d.n, T = d.T, H1 = d.H1, O = d.O, H2 = d.H2, O2 = d.O2;
  const int N1 = d.N1(), nO = d.nO(), Tn = d.Tn(), N1e = mb_even(N1);
  float* des = lds;                              // [nO]: de summed over the tasks, then the masked dze
  float* dzs = des + nO * MB_LD;                 // [Tn]: dg, then dz, then the masked dzz
  float* zt = dzs + Tn * MB_LD;                  // [N1e]: dZ1 at the end; before it the operands below
  float* es = zt;                                // [nO]
  float* gs = es + nO * MB_LD;                   // [Tn]
  float* g1s = gs + Tn * MB_LD;                  // [Tn]: the first softmax of a double one
  float* dus = g1s + Tn * MB_LD;                 // [nO]
  float* d1s = dus + nO * MB_LD;                 // [H2]
  float* d2s = d1s + H2 * MB_LD;                 // [O2]
  float* dls = d2s + O2 * MB_LD;                 // [T]: dout, then the gradient of the logits
  float* ps = dls + T * MB_LD;                   // [T]
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;
  const int b = tid & (MB_T - 1), g = tid >> 5;
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * mm_slot_floats(d);
  float* __restrict__ slot_e = slot + N1;
  float* __restrict__ slot_g = slot_e + nO;
  float* __restrict__ slot_1 = slot_g + Tn;
  float* __restrict__ slot_2 = slot_1 + T * H2;
  float* __restrict__ slot_l = slot_2 + T * O2;

  Tile::rows_in(es, e, r0, B, nO, 0, nO, tid);
  Tile::rows_in(gs, gt, r0, B, Tn, 0, Tn, tid);
  if (passes == 2) Tile::rows_in(g1s, z, r0, B, Tn, 0, Tn, tid);
  Tile::rows_in(ps, p, r0, B, T, 0, T, tid);
  Tile::rows_in(dls, dout, r0, B, T, 0, T, tid);
  for (int c = g; c < nO; c += MM_G) des[c * MB_LD + b] = 0.f;     // by the thread that adds to it below
  __syncthreads();

  if (g == 0) {                                  // dout -> dp (the ctcvr product) -> the gradient of the logits
    const float d0 = dls[b], d1 = T > 1 ? dls[MB_LD + b] : 0.f;
    const float p0 = ps[b], p1 = T > 1 ? ps[MB_LD + b] : 0.f;
    for (int t = 0; t < T; ++t) {
      float dp = dls[t * MB_LD + b];
      if (ctcvr) dp = t == 0 ? d0 + d1 * p1 : d1 * p0;
      const float pv = ps[t * MB_LD + b];
      dls[t * MB_LD + b] = dp * (pv * (1.f - pv));
    }
  } else if (passes == 2 && g - 1 < T) {         // the first softmax again, by the other threads of the example
    Tile::softmax(g1s + (g - 1) * n * MB_LD + b, g1s + (g - 1) * n * MB_LD + b, n);
  }
  __syncthreads();
  Tile::rows_out(ws_dl, dls, r0, B, T, 0, T, tid);
  Tile::col_sums(slot_l, dls, T, tid);

  for (int t = 0; t < T; ++t) {
    for (int c = g; c < O2; c += MM_G) d2s[c * MB_LD + b] = dls[t * MB_LD + b] * Wt3[t * O2 + c];
    __syncthreads();
    Tile::mask_out(d2s, a2, ws_d2, r0, B, T * O2, t * O2, O2, tid);
    __syncthreads();
    Tile::col_sums(slot_2 + t * O2, d2s, O2, tid);
    for (int c = g; c < H2; c += MM_G) {         // da2 Wt2^T
      const float* W = Wt2 + ((int64_t)t * H2 + c) * O2;
      float acc = 0.f;
      for (int k = 0; k < O2; ++k) acc = fmaf(d2s[k * MB_LD + b], W[k], acc);
      d1s[c * MB_LD + b] = acc;
    }
    __syncthreads();
    Tile::mask_out(d1s, a1, ws_d1, r0, B, T * H2, t * H2, H2, tid);
    __syncthreads();
    Tile::col_sums(slot_1 + t * H2, d1s, H2, tid);
    for (int k = g; k < nO; k += MM_G) {         // du = da1 Wt1^T; de += du g
      const float* W = Wt1 + ((int64_t)t * nO + k) * H2;
      float acc = 0.f;
      for (int c = 0; c < H2; ++c) acc = fmaf(d1s[c * MB_LD + b], W[c], acc);
      dus[k * MB_LD + b] = acc;
      des[k * MB_LD + b] = des[k * MB_LD + b] + acc * gs[(t * n + k / O) * MB_LD + b];
    }
    __syncthreads();
    for (int i = g; i < n; i += MM_G) {          // dg_t[i] = sum_o du[i, o] e[i, o]
      float acc = 0.f;
      for (int o = 0; o < O; ++o) acc = fmaf(dus[(i * O + o) * MB_LD + b], es[(i * O + o) * MB_LD + b], acc);
      dzs[(t * n + i) * MB_LD + b] = acc;
    }
    __syncthreads();                             // dus, d1s and d2s are rewritten by the next task
  }

  if (g < T) {
    Tile::softmax_bwd(gs + g * n * MB_LD + b, dzs + g * n * MB_LD + b, n);
    if (passes == 2) Tile::softmax_bwd(g1s + g * n * MB_LD + b, dzs + g * n * MB_LD + b, n);
  }
  __syncthreads();
  Tile::mask_out(dzs, z, ws_dzz, r0, B, Tn, 0, Tn, tid);
  Tile::mask_out(des, e, ws_dze, r0, B, nO, 0, nO, tid);
  __syncthreads();                               // and every read of es .. ps lies before it: zt may be written
  Tile::col_sums(slot_e, des, nO, tid);
  Tile::col_sums(slot_g, dzs, Tn, tid);

  for (int c = g; c < N1e; c += MM_G) {          // dh = dze We2^T | dzz Wg2^T
    float acc = 0.f;
    if (c < N1) {
      const int blk = c / H1, k = c - blk * H1;
      if (blk < n) {
        const float* W = We2 + ((int64_t)blk * H1 + k) * O;
        for (int o = 0; o < O; ++o) acc = fmaf(des[(blk * O + o) * MB_LD + b], W[o], acc);
      } else {
        const int t = blk - n;
        const float* W = Wg2 + ((int64_t)t * H1 + k) * n;
        for (int j = 0; j < n; ++j) acc = fmaf(dzs[(t * n + j) * MB_LD + b], W[j], acc);
      }
    }
    zt[c * MB_LD + b] = acc;
  }
  __syncthreads();
  Tile::mask_out(zt, h, ws_dz1, r0, B, N1, 0, N1, tid);
  __syncthreads();
  Tile::col_sums(slot, zt, N1, tid);

  f32x16 xacc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(xacc[j]);
  mb_mma<true>(xacc, zt, N1, W1, N1, 0, D, wave, lo, hi);      // dx = dZ1 W1^T
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int col = (wave + 4 * j) * 32 + lo;
    if ((wave + 4 * j) * 32 < D && col < D) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mb_row(r, hi);
        if (r0 + row < B) dx[(r0 + row) * D + col] = xacc[j][r];
      }
    }
  }
}

// The small weight gradients, all of them in one launch (small_dw_kernel, tile_ops.h).  Matrix q of the n + 4 T is
// A_q^T G_q over the batch with
//   q < n          dWe2[i]  = h_i^T dze_i            then  dWg2[t] = h_{n+t}^T dzz_t,   dWt1[t] = u_t^T da1_t (u_t = e (.) g_t
//   recomputed: the row scale),   dWt2[t]  = a1_t^T da2_t           and   dWt3[t] = a2_t^T dl_t,
// laid out one after the other in that order (the order of the packed gradients).
struct MmSmall {
  static constexpr int MAXK = MM_MAXO;
  MmDims d;
  const float *h, *e, *gt, *a1, *a2, *dze, *dzz, *d1, *d2, *dl;
  __device__ SmallMat mat(int q) const {
    const int n = d.n, T = d.T, H1 = d.H1, O = d.O, H2 = d.H2, O2 = d.O2, N1 = d.N1(), nO = d.nO(), Tn = d.Tn();
    const int oG = n * H1 * O, o1 = oG + T * H1 * n, o2 = o1 + T * nO * H2, o3 = o2 + T * H2 * O2;
    if (q < n) return {h, N1, q * H1, H1, dze, nO, q * O, O, q * H1 * O, O};
    if ((q -= n) < T) return {h, N1, (n + q) * H1, H1, dzz, Tn, q * n, n, oG + q * H1 * n, n};
    if ((q -= T) < T) return {e, nO, 0, nO, d1, T * H2, q * H2, H2, o1 + q * nO * H2, H2, gt, Tn, q * n, O};
    if ((q -= T) < T) return {a1, T * H2, q * H2, H2, d2, T * O2, q * O2, O2, o2 + q * H2 * O2, O2};
    q -= T;
    return {a2, T * O2, q * O2, O2, dl, T, q, 1, o3 + q * O2, 1};
  }
};

static int mm_shape(int64_t B, int D, int n, int T, int H1, int O, int H2, int O2, int passes, int ctcvr) {
  if (B < 0 || D < 1 || n < 1 || T < 1 || H1 < 1 || O < 1 || H2 < 1 || O2 < 1) return REC_E_ARG;
  if ((passes != 1 && passes != 2) || (ctcvr != 0 && ctcvr != 1) || (ctcvr && T != 2)) return REC_E_ARG;
  if (D > MM_MAXD || T > MM_MAXT || H1 > MM_MAXO || H2 > MM_MAXO || O2 > MM_MAXO || (int64_t)n * O > MM_MAXO ||
      (int64_t)n * T > MM_MAXO || ((int64_t)n + T) * H1 > MM_MAXN1 || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;
  return REC_OK;
}

static int mm_small_floats(const MmDims& d) {
  return d.n * d.H1 * d.O + d.T * d.H1 * d.n + d.T * d.nO() * d.H2 + d.T * d.H2 * d.O2 + d.T * d.O2;
}

struct MmWs {
  size_t dz1, dze, dzz, d1, d2, dl, slots, part, gemm, total;  // offsets in floats
};
static MmWs mm_ws(int64_t B, const MmDims& d) {
  MmWs w{};
  const size_t b = (size_t)B, tiles = (size_t)ceil_div64(B, MB_T);
  WsCarve c;
  w.dz1 = c.take(b * d.N1());
  w.dze = c.take(b * d.nO());
  w.dzz = c.take(b * d.Tn());
  w.d1 = c.take(b * d.T * d.H2);
  w.d2 = c.take(b * d.T * d.O2);
  w.dl = c.take(b * d.T);
  w.slots = c.take(tiles * (size_t)mm_slot_floats(d));
  w.part = c.take((size_t)mb_small_split(B) * mm_small_floats(d));
  w.gemm = c.take(mb_dw_gemm_floats(B, d.D, d.N1()));
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" size_t rec_mmoe_workspace_bytes(int64_t B, int D, int n, int T, int H1, int O, int H2, int O2) {
  if (mm_shape(B, D, n, T, H1, O, H2, O2, 1, 0) != REC_OK) return 0;
  return sizeof(float) * (mm_ws(B, MmDims{D, n, T, H1, O, H2, O2}).total + 4);
}

extern "C" int rec_mmoe_fwd_f32(const float* x, const float* W1, const float* b1, const float* We2, const float* be2,
                                const float* Wg2, const float* bg2, const float* Wt1, const float* bt1,
                                const float* Wt2, const float* bt2, const float* Wt3, const float* bt3, int64_t B, int D,
                                int n, int T, int H1, int O, int H2, int O2, int gate_softmax_passes, int ctcvr,
                                float* out, float* h, float* e, float* z, float* g, float* a1, float* a2, float* p,
                                void* stream) {
  if (int rc = mm_shape(B, D, n, T, H1, O, H2, O2, gate_softmax_passes, ctcvr)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !W1 || !b1 || !We2 || !be2 || !Wg2 || !bg2 || !Wt1 || !bt1 || !Wt2 || !bt2 || !Wt3 || !bt3 || !out)
    return REC_E_ARG;
  const bool save = h || e || z || g || a1 || a2 || p;
  if (save && !(h && e && z && g && a1 && a2 && p)) return REC_E_ARG;            // all of them or none
  const MmDims d{D, n, T, H1, O, H2, O2};
  if (hipError_t err = rec_allow_lds<mmoe_fwd_kernel>(MM_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * mm_lds_floats(d, 0);
  hipLaunchKernelGGL(mmoe_fwd_kernel, dim3((unsigned)ceil_div64(B, MB_T)), dim3(MM_NTHR), lds, as_stream(stream), x, W1,
                     b1, We2, be2, Wg2, bg2, Wt1, bt1, Wt2, bt2, Wt3, bt3, B, d, gate_softmax_passes, ctcvr, out, h, e,
                     z, g, a1, a2, p);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_mmoe_bwd_f32(const float* x, const float* W1, const float* We2, const float* Wg2, const float* Wt1,
                                const float* Wt2, const float* Wt3, const float* h, const float* e, const float* z,
                                const float* g, const float* a1, const float* a2, const float* p, const float* dout,
                                int64_t B, int D, int n, int T, int H1, int O, int H2, int O2, int gate_softmax_passes,
                                int ctcvr, float* dx, float* dW1, float* db1, float* dWe2, float* dbe2, float* dWg2,
                                float* dbg2, float* dWt1, float* dbt1, float* dWt2, float* dbt2, float* dWt3,
                                float* dbt3, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = mm_shape(B, D, n, T, H1, O, H2, O2, gate_softmax_passes, ctcvr)) return rc;
  if (B == 0) return REC_OK;
  if (!x || !W1 || !We2 || !Wg2 || !Wt1 || !Wt2 || !Wt3 || !h || !e || !z || !g || !a1 || !a2 || !p || !dout || !dx ||
      !dW1 || !db1 || !dWe2 || !dbe2 || !dWg2 || !dbg2 || !dWt1 || !dbt1 || !dWt2 || !dbt2 || !dWt3 || !dbt3 ||
      !workspace)
    return REC_E_ARG;
  const MmDims d{D, n, T, H1, O, H2, O2};
  const MmWs w = mm_ws(B, d);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  float *dz1 = base + w.dz1, *dze = base + w.dze, *dzz = base + w.dzz, *d1 = base + w.d1, *d2 = base + w.d2,
        *dl = base + w.dl, *slots = base + w.slots, *part = base + w.part, *gws = base + w.gemm;
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, MB_T), N1 = d.N1(), nO = d.nO(), Tn = d.Tn();
  if (hipError_t err = rec_allow_lds<mmoe_bwd_kernel>(MM_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * mm_lds_floats(d, 1);
  hipLaunchKernelGGL(mmoe_bwd_kernel, dim3(tiles), dim3(MM_NTHR), lds, st, W1, We2, Wg2, Wt1, Wt2, Wt3, h, e, z, g, a1,
                     a2, p, dout, B, d, gate_softmax_passes, ctcvr, dx, dz1, dze, dzz, d1, d2, dl, slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, mm_slot_floats(d), tiles, slots,
                            {{db1, dbe2, dbg2, dbt1, dbt2, dbt3}, {N1, nO, Tn, T * H2, T * O2, T}}, st))
    return rc;
  const int S = mb_small_split(B), wtot = mm_small_floats(d);
  int big = H1 * (O > n ? O : n);
  if (nO * H2 > big) big = nO * H2;
  if (H2 * O2 > big) big = H2 * O2;
  if (int rc = small_dw_launch(MmSmall{d, h, e, g, a1, a2, dze, dzz, d1, d2, dl}, n + 4 * T, big, wtot, B, part, st))
    return rc;
  if (int rc = rec_slot_sum(REC_SLOTS_SERIAL, wtot, S, part,
                            {{dWe2, dWg2, dWt1, dWt2, dWt3}, {n * H1 * O, T * H1 * n, T * nO * H2, T * H2 * O2, T * O2}},
                            st))
    return rc;
  return mb_dw_gemm(D, N1, B, x, dz1, dW1, gws, stream);        // dW1 = x^T dZ1
}
