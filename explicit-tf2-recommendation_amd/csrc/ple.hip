// PLE (PLELayer, 4.MMOE/CustomLayers.py:248-384) on gfx950: one CGC level (customized gate control, one stage of PLE)
// per launch each way.
//
// xin [B, Gin, Din], Gin = 1 (level 0: every MLP reads the same row) or T + 1 (every MLP reads its group's row: tasks
// 0 .. T-1, then the shared branch).  ne = T S + Sh experts, ns = S + Sh, Gout = last ? T : T + 1 gates, M = ne + Gout
// first layers, N1 = M H1, GW = T ns + (last ? 0 : ne) gate columns.  Packed weights:
//   W1 [Din, N1], b1 [N1]     column block m < ne is expert m's first layer, block ne + g gate g's
//   We2 [ne, H1, O], be2 [ne, O]      Wg2 [Gout, H1, Og], bg2 [Gout, Og]
//   Wg3s [T, Og, ns]   Wg3h [Og, ne] (not last)   Wtw [T, O], btw [T] (last)
// group(m): expert m < T S reads group m / S, a shared expert group T, gate g group g.
//   h_m = relu(in_group(m) W1_m + b1_m)    e_i = relu(h_i We2[i] + be2[i])    q_g = relu(h_{ne+g} Wg2[g] + bg2[g])
//   g_t = softmax(softmax(q_t Wg3s[t]))    y_t = sum_{j<S} g_t[j] e_{tS+j} + sum_{k<Sh} g_t[S+k] e_{TS+k}      (a SUM)
//   g_T = softmax(q_T Wg3h), once          y_T = sum_i g_T[i] e_i                                         (not last)
//   out[:, t] = sigmoid(y_t . Wtw[t] + btw[t])                                                                (last)
// Forward, one launch.  A workgroup of 4 waves owns 32 examples (mfma_tile.h); the input tile of every group sits k-major
// in LDS and the first layers run on v_mfma_f32_32x32x2_f32, one (MLP, 32-column block) per wave at a time, the A
// operand being the tile of the MLP's group.  N1 is 1024 at the default level 0 and 1920 at the limits, so the first
// layer runs in CHUNKS of whole MLPs (at most 512 / H1, fewer where LDS is short) and the second layers of a chunk are
// finished before the next chunk overwrites h: LDS holds one h chunk, e, q, the gates and y, never the whole h.  The
// narrow stages (e, q, the gate logits, the softmax, the mixture, the towers) run on the VALU out of LDS: thread t owns
// example t & 31 and the columns t / 32, t / 32 + 8, ...
// Grouped levels (K = Din = 8 at the defaults) keep the MFMA for the first layer: K is even, so no k step is padding, and
// a block of H1 = 64 columns is two full 32-column tiles.  Their dxin has N = Din = 8 columns per group, a quarter of a
// tile, and runs on the VALU; their dW1 is a few KB and joins the batched small weight gradients.
// Training saves h, e, q and g (the gates after their last softmax); inference writes y (and out) alone, the same bits.
// Backward, one launch for the per-example chain: gate logits are not saved, the first softmax of a task gate is
// recomputed from q by the forward's own device functions.  de has ONE owner per column across every gate that reads
// the expert; dh, the relu mask, the workspace copy dZ1 and dxin go chunk by chunk like the forward.  dh = dze We2^T |
// dzq Wg2^T has K = O | Og and N = H1, the shape of a grouped first layer, and runs on the MFMA when both K are even
// (an odd K has no zero row behind it in LDS: the VALU).  Bias gradients go
// through per-tile slots and rec_slot_sum; every small weight gradient (dWe2, dWg2, dWg3s, dWg3h, dWtw and, for a grouped
// level, dW1) is one launch over (matrix, block of 256 outputs, batch slice) whose at most 16 slices a second slot sum
// adds in order; with Gin = 1, dW1 = xin^T dZ1 goes to rec_gemm_f32 (split-K, slices added in order).
// No float atomics and no value with two writers: bit-identical results run to run; no host synchronisation.
// Contraction is off: a softmax over one column must return exactly zero gradients, which g (dg - dg g) only does when
// both terms are the same rounded product.
// Shared with the other tile kernels, in tile_ops.h: the row / column / softmax passes over an LDS operand (TileOps), the
// small weight-gradient kernel and its launch (this file supplies the matrices: PlSmall), the workspace carving and the
// split-K weight-gradient GEMM; the MFMA tile itself is mfma_tile.h.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)
#include "tile_ops.h"

namespace {

// the limits are MaskNet's: the header gains no constant for this family
constexpr int PL_MAXD = REC_MASKNET_MAX_D, PL_MAXO = REC_MASKNET_MAX_O, PL_MAXT = REC_MASKNET_MAX_R;
constexpr int PL_MAXCH = 128 * MB_NJ;            // columns of an h chunk at most: the accumulator columns of mb_mma
constexpr int PL_NTHR = 256;
constexpr int PL_G = PL_NTHR / MB_T;             // column groups of the VALU stages
constexpr size_t PL_LDS_CAP = REC_POSO_LDS_CAP;
constexpr int PL_LDS_ROWS = (int)(PL_LDS_CAP / (sizeof(float) * MB_LD));

static_assert(PL_MAXD <= 128 * MB_NJ, "accumulator blocks per wave of dxin");
static_assert(PL_MAXT + 1 <= PL_G, "one thread per (example, gate)");

struct PlDims {
  int Din, Gin, T, S, Sh, H1, O, Og, last;
  __host__ __device__ int ne() const { return T * S + Sh; }
  __host__ __device__ int ns() const { return S + Sh; }
  __host__ __device__ int Gout() const { return last ? T : T + 1; }
  __host__ __device__ int M() const { return ne() + Gout(); }
  __host__ __device__ int N1() const { return M() * H1; }
  __host__ __device__ int neO() const { return ne() * O; }
  __host__ __device__ int GQ() const { return Gout() * Og; }
  __host__ __device__ int GO() const { return Gout() * O; }
  __host__ __device__ int Tns() const { return T * ns(); }
  __host__ __device__ int GW() const { return Tns() + (last ? 0 : ne()); }
  __host__ __device__ int XD() const { return Gin * Din; }
  // the input group that first layer m reads
  __host__ __device__ int grp(int m) const { return m < T * S ? m / S : (m < ne() ? T : m - ne()); }
};

// rows of LDS ([.][33] floats each) next to the h chunk:
//   forward   xs [Gin even(Din)] es [neO] qs [GQ] gs [GW] ys [GO]
//   backward  es [neO] gs [GW] g1s [T ns] qs = dqs [GQ] dys [GO] des [neO] dgs [GW] dls [T] dxs [Gin Din, grouped only]
__host__ __device__ inline int pl_fixed_rows(const PlDims& d, int bwd) {
  return bwd ? 2 * d.neO() + 2 * d.GW() + d.Tns() + d.GQ() + d.GO() + d.T + (d.Gin > 1 ? d.XD() : 0)
             : d.Gin * mb_even(d.Din) + d.neO() + d.GQ() + d.GW() + d.GO();
}
// first layers of one chunk: whole MLPs, at most PL_MAXCH columns, and what LDS leaves
__host__ __device__ inline int pl_chunk(const PlDims& d, int bwd) {
  int c = PL_MAXCH / d.H1;
  const int fit = (PL_LDS_ROWS - pl_fixed_rows(d, bwd) - 1) / d.H1;
  if (c > fit) c = fit;
  if (c > d.M()) c = d.M();
  return c;
}
__host__ __device__ inline size_t pl_lds_floats(const PlDims& d, int bwd) {
  return (size_t)(pl_fixed_rows(d, bwd) + mb_even(pl_chunk(d, bwd) * d.H1)) * MB_LD;
}
// the largest shape of each direction leaves a chunk of one MLP: Gin even(Din) <= MAXD + 5 is not reached together
// with the other terms (a grouped level has Gin Din <= MAXO), so the forward's worst case is Gin = 1
static_assert(PL_MAXD + 4 * PL_MAXO + PL_MAXO + 1 <= PL_LDS_ROWS, "forward at the limits");
static_assert(8 * PL_MAXO + PL_MAXT + PL_MAXO + 1 <= PL_LDS_ROWS, "backward at the limits");
static_assert(PL_LDS_CAP <= REC_LDS_CU_BYTES, "the LDS of a CU");

using Tile = TileOps<MB_T, MB_LD, PL_NTHR>;

// acc + sum_k a[k][example] w[k ldw], k ascending.  The weights of eight steps are requested together: a workgroup is one
// wave per SIMD, so nothing else hides the latency of a weight load, and one wait per step was a third of the forward.
__device__ __forceinline__ float pl_dot(const float* a, const float* __restrict__ w, int ldw, int K, float acc) {
  int k = 0;
  for (; k + 8 <= K; k += 8) {
    float wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) wv[u] = w[(k + u) * ldw];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fmaf(a[(k + u) * MB_LD], wv[u], acc);
  }
  for (; k < K; ++k) acc = fmaf(a[k * MB_LD], w[k * ldw], acc);
  return acc;
}
// The gate logits q Wg3 of the first ncols gate columns (task gates first, then the shared gate) for example b: both
// directions call this, so the backward's recomputed logits have the forward's bits.
__device__ __forceinline__ void pl_logits(const PlDims& d, const float* qs, const float* __restrict__ Wg3s,
                                          const float* __restrict__ Wg3h, float* dst, int ncols, int b, int g) {
  const int ns = d.ns(), Tns = d.Tns(), ne = d.ne(), Og = d.Og;
  for (int c = g; c < ncols; c += PL_G) {
    const float* qp;
    const float* W;
    int ldw;
    if (c < Tns) {
      const int t = c / ns, j = c - t * ns;
      qp = qs + t * Og * MB_LD + b;
      W = Wg3s + (int64_t)t * Og * ns + j;
      ldw = ns;
    } else {
      qp = qs + d.T * Og * MB_LD + b;
      W = Wg3h + (c - Tns);
      ldw = ne;
    }
    dst[c * MB_LD + b] = pl_dot(qp, W, ldw, Og, 0.f);
  }
}

__global__ __launch_bounds__(PL_NTHR) void ple_cgc_fwd_kernel(
    const float* __restrict__ xin, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ We2, const float* __restrict__ be2, const float* __restrict__ Wg2,
    const float* __restrict__ bg2, const float* __restrict__ Wg3s, const float* __restrict__ Wg3h,
    const float* __restrict__ Wtw, const float* __restrict__ btw, int64_t B, PlDims d, int cm, float* __restrict__ y,
    float* __restrict__ out, float* __restrict__ sh, float* __restrict__ se, float* __restrict__ sq,
    float* __restrict__ sg) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Din = d.Din, Gin = d.Gin, T = d.T, S = d.S, Sh = d.Sh, H1 = d.H1, O = d.O, Og = d.Og;
  const int ne = d.ne(), ns = d.ns(), Gout = d.Gout(), M = d.M(), N1 = d.N1(), neO = d.neO(), GQ = d.GQ(), GW = d.GW();
  const int GO = d.GO(), Tns = d.Tns(), De = mb_even(Din), XD = d.XD();
  float* xs = lds;                               // [Gin][De][33]: the input tile of every group
  float* es = xs + Gin * De * MB_LD;             // [neO]
  float* qs = es + neO * MB_LD;                  // [GQ]
  float* gs = qs + GQ * MB_LD;                   // [GW]: logits, then the gates
  float* ys = gs + GW * MB_LD;                   // [GO]
  float* hs = ys + GO * MB_LD;                   // [even(cm H1)]: one chunk of h
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;
  const int b = tid & (MB_T - 1), g = tid >> 5;

  for (int i = tid; i < MB_T * Gin * De; i += PL_NTHR) {
    const int m = i / (Gin * De), rem = i - m * (Gin * De), gi = rem / De, k = rem - gi * De;
    xs[(gi * De + k) * MB_LD + m] = (k < Din && r0 + m < B) ? xin[(r0 + m) * XD + gi * Din + k] : 0.f;
  }
  __syncthreads();

  const int nblk = (H1 + 31) / 32, wmax = O > Og ? O : Og;
  for (int m0 = 0; m0 < M; m0 += cm) {
    const int mc = M - m0 < cm ? M - m0 : cm;
    if (Gin == 1) {                              // one A operand: the chunk is mc H1 <= 512 consecutive columns of W1
      f32x16 acc[MB_NJ];
#pragma unroll
      for (int j = 0; j < MB_NJ; ++j) mb_zero(acc[j]);
      const int nc = mc * H1, c0 = m0 * H1;
      mb_mma<false>(acc, xs, Din, W1 + c0, N1, 0, nc, wave, lo, hi);
#pragma unroll
      for (int j = 0; j < MB_NJ; ++j) {
        const int col = (wave + 4 * j) * 32 + lo;
        if ((wave + 4 * j) * 32 < nc && col < nc) {
          const float bc = b1[c0 + col];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = mb_row(r, hi);
            const float hv = fmaxf(acc[j][r] + bc, 0.f);
            hs[col * MB_LD + row] = hv;
            if (sh && r0 + row < B) sh[(r0 + row) * N1 + c0 + col] = hv;
          }
        }
      }
    } else {                                     // a block's A operand is the tile of its MLP's group
      for (int job = wave; job < mc * nblk; job += 4) {          // uniform over the wave
        const int mm = job / nblk, blk = job - mm * nblk, m = m0 + mm;
        f32x16 acc;
        mb_zero(acc);
        mb_mma1<false>(acc, xs + d.grp(m) * De * MB_LD, Din, W1 + m * H1, N1, 0, H1, blk * 32, lo, hi);
        const int col = blk * 32 + lo;
        if (col < H1) {
          const float bc = b1[m * H1 + col];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = mb_row(r, hi);
            const float hv = fmaxf(acc[r] + bc, 0.f);
            hs[(mm * H1 + col) * MB_LD + row] = hv;
            if (sh && r0 + row < B) sh[(r0 + row) * N1 + m * H1 + col] = hv;
          }
        }
      }
    }
    __syncthreads();
    for (int c = g; c < mc * wmax; c += PL_G) {                  // second layers of the chunk's experts and gates
      const int mm = c / wmax, o = c - mm * wmax, m = m0 + mm;
      const float* hp = hs + mm * H1 * MB_LD + b;
      const float* W;
      float* dstp;
      int ldw;
      float bias;
      if (m < ne) {
        if (o >= O) continue;
        W = We2 + (int64_t)m * H1 * O + o;
        ldw = O;
        bias = be2[m * O + o];
        dstp = es + (m * O + o) * MB_LD + b;
      } else {
        if (o >= Og) continue;
        W = Wg2 + (int64_t)(m - ne) * H1 * Og + o;
        ldw = Og;
        bias = bg2[(m - ne) * Og + o];
        dstp = qs + ((m - ne) * Og + o) * MB_LD + b;
      }
      *dstp = fmaxf(pl_dot(hp, W, ldw, H1, 0.f) + bias, 0.f);
    }
    __syncthreads();                             // the next chunk overwrites hs
  }
  if (se) {
    Tile::rows_out(se, es, r0, B, neO, 0, neO, tid);
    Tile::rows_out(sq, qs, r0, B, GQ, 0, GQ, tid);
  }
  pl_logits(d, qs, Wg3s, Wg3h, gs, GW, b, g);
  __syncthreads();
  if (g < T) {
    Tile::softmax(gs + g * ns * MB_LD + b, gs + g * ns * MB_LD + b, ns);
    Tile::softmax(gs + g * ns * MB_LD + b, gs + g * ns * MB_LD + b, ns);
  } else if (g == T && !d.last) {
    Tile::softmax(gs + Tns * MB_LD + b, gs + Tns * MB_LD + b, ne);
  }
  __syncthreads();
  if (sg) Tile::rows_out(sg, gs, r0, B, GW, 0, GW, tid);

  for (int c = g; c < GO; c += PL_G) {           // the mixture: a gated SUM over the experts a gate reads
    const int gi = c / O, o = c - gi * O;
    float acc = 0.f;
    if (gi < T) {
      const float* gp = gs + gi * ns * MB_LD + b;
      for (int j = 0; j < S; ++j) acc = fmaf(gp[j * MB_LD], es[((gi * S + j) * O + o) * MB_LD + b], acc);
      for (int k = 0; k < Sh; ++k) acc = fmaf(gp[(S + k) * MB_LD], es[((T * S + k) * O + o) * MB_LD + b], acc);
    } else {
      const float* gp = gs + Tns * MB_LD + b;
      for (int i = 0; i < ne; ++i) acc = fmaf(gp[i * MB_LD], es[(i * O + o) * MB_LD + b], acc);
    }
    ys[c * MB_LD + b] = acc;
  }
  __syncthreads();
  Tile::rows_out(y, ys, r0, B, GO, 0, GO, tid);
  if (d.last && g < T && r0 + b < B) {           // the towers: one sigmoid unit per task
    float acc = 0.f;
    for (int o = 0; o < O; ++o) acc = fmaf(ys[(g * O + o) * MB_LD + b], Wtw[g * O + o], acc);
    out[(r0 + b) * T + g] = sigmoid_acc(acc + btw[g]);
  }
}

// slot of a tile: db1 [N1] | dbe2 [neO] | dbg2 [GQ] | dbtw [T] (last)
__host__ __device__ inline int pl_slot_floats(const PlDims& d) { return d.N1() + d.neO() + d.GQ() + (d.last ? d.T : 0); }

__global__ __launch_bounds__(PL_NTHR) void ple_cgc_bwd_kernel(
    const float* __restrict__ W1, const float* __restrict__ We2, const float* __restrict__ Wg2,
    const float* __restrict__ Wg3s, const float* __restrict__ Wg3h, const float* __restrict__ Wtw,
    const float* __restrict__ h, const float* __restrict__ e, const float* __restrict__ q,
    const float* __restrict__ gt, const float* __restrict__ p, const float* __restrict__ dy,
    const float* __restrict__ dout, int64_t B, PlDims d, int cm, float* __restrict__ dxin,
    float* __restrict__ ws_dz1, float* __restrict__ ws_dze, float* __restrict__ ws_dzq, float* __restrict__ ws_dlg,
    float* __restrict__ ws_dl, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Din = d.Din, Gin = d.Gin, T = d.T, S = d.S, Sh = d.Sh, H1 = d.H1, O = d.O, Og = d.Og, last = d.last;
  const int ne = d.ne(), ns = d.ns(), M = d.M(), N1 = d.N1(), neO = d.neO(), GQ = d.GQ(), GW = d.GW();
  const int GO = d.GO(), Tns = d.Tns(), XD = d.XD();
  float* es = lds;                               // [neO]
  float* gs = es + neO * MB_LD;                  // [GW]: the gates after their last softmax
  float* g1s = gs + GW * MB_LD;                  // [T ns]: the first softmax of the task gates
  float* qs = g1s + Tns * MB_LD;                 // [GQ]: q, and after the logits dq
  float* dys = qs + GQ * MB_LD;                  // [GO]
  float* des = dys + GO * MB_LD;                 // [neO]
  float* dgs = des + neO * MB_LD;                // [GW]: dg, then the gradient of the logits
  float* dls = dgs + GW * MB_LD;                 // [T]: the gradient of the tower logits
  float* dxs = dls + T * MB_LD;                  // [Gin Din] of a grouped level
  float* zt = dxs + (Gin > 1 ? XD : 0) * MB_LD;  // [even(cm H1)]: one chunk of dh, then of dZ1
  const int64_t r0 = (int64_t)blockIdx.x * MB_T;
  const int b = tid & (MB_T - 1), g = tid >> 5;
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * pl_slot_floats(d);
  float* __restrict__ slot_e = slot + N1;
  float* __restrict__ slot_g = slot_e + neO;
  float* __restrict__ slot_l = slot_g + GQ;

  Tile::rows_in(es, e, r0, B, neO, 0, neO, tid);
  Tile::rows_in(gs, gt, r0, B, GW, 0, GW, tid);
  Tile::rows_in(qs, q, r0, B, GQ, 0, GQ, tid);
  Tile::rows_in(dys, dy, r0, B, GO, 0, GO, tid);
  if (last) {
    for (int i = tid; i < MB_T * T; i += PL_NTHR) {
      const int row = i / T, t = i - row * T;
      float v = 0.f;
      if (r0 + row < B) {
        const float pv = p[(r0 + row) * T + t];
        v = dout[(r0 + row) * T + t] * (pv * (1.f - pv));
        ws_dl[(r0 + row) * T + t] = v;
      }
      dls[t * MB_LD + row] = v;
    }
  }
  if (Gin > 1)
    for (int c = g; c < XD; c += PL_G) dxs[c * MB_LD + b] = 0.f;    // by the thread that adds to it below
  __syncthreads();

  pl_logits(d, qs, Wg3s, Wg3h, g1s, Tns, b, g);  // the task gates' logits again
  if (last) {
    Tile::col_sums(slot_l, dls, T, tid);
    for (int c = g; c < GO; c += PL_G)           // dy of the towers
      dys[c * MB_LD + b] = dys[c * MB_LD + b] + dls[(c / O) * MB_LD + b] * Wtw[c];
  }
  __syncthreads();
  if (g < T) Tile::softmax(g1s + g * ns * MB_LD + b, g1s + g * ns * MB_LD + b, ns);

  for (int c = g; c < GW; c += PL_G) {           // dg[i] = dy . e_i
    int gi, ei;
    if (c < Tns) {
      gi = c / ns;
      const int j = c - gi * ns;
      ei = j < S ? gi * S + j : T * S + (j - S);
    } else {
      gi = T;
      ei = c - Tns;
    }
    float acc = 0.f;
    for (int o = 0; o < O; ++o) acc = fmaf(dys[(gi * O + o) * MB_LD + b], es[(ei * O + o) * MB_LD + b], acc);
    dgs[c * MB_LD + b] = acc;
  }
  for (int c = g; c < neO; c += PL_G) {          // de_i = sum over the gates that read expert i of g[i] dy: one owner
    const int i = c / O, o = c - i * O;
    float acc = 0.f;
    if (i < T * S) {
      const int t = i / S, j = i - t * S;
      acc = gs[(t * ns + j) * MB_LD + b] * dys[(t * O + o) * MB_LD + b];
    } else {
      const int k = i - T * S;
      for (int t = 0; t < T; ++t) acc = fmaf(gs[(t * ns + S + k) * MB_LD + b], dys[(t * O + o) * MB_LD + b], acc);
    }
    if (!last) acc = fmaf(gs[(Tns + i) * MB_LD + b], dys[(T * O + o) * MB_LD + b], acc);
    des[c * MB_LD + b] = acc;
  }
  __syncthreads();

  if (g < T) {                                   // through both softmax passes of a task gate, one of the shared gate
    Tile::softmax_bwd(gs + g * ns * MB_LD + b, dgs + g * ns * MB_LD + b, ns);
    Tile::softmax_bwd(g1s + g * ns * MB_LD + b, dgs + g * ns * MB_LD + b, ns);
  } else if (g == T && !last) {
    Tile::softmax_bwd(gs + Tns * MB_LD + b, dgs + Tns * MB_LD + b, ne);
  }
  __syncthreads();                               // and every read of q lies before it: qs becomes dq
  Tile::rows_out(ws_dlg, dgs, r0, B, GW, 0, GW, tid);
  for (int c = g; c < GQ; c += PL_G) {           // dq = dlogits Wg3^T
    const int gi = c / Og, k = c - gi * Og;
    qs[c * MB_LD + b] = gi < T ? pl_dot(dgs + gi * ns * MB_LD + b, Wg3s + ((int64_t)gi * Og + k) * ns, 1, ns, 0.f)
                               : pl_dot(dgs + Tns * MB_LD + b, Wg3h + (int64_t)k * ne, 1, ne, 0.f);
  }
  __syncthreads();
  Tile::mask_out(qs, q, ws_dzq, r0, B, GQ, 0, GQ, tid);
  Tile::mask_out(des, e, ws_dze, r0, B, neO, 0, neO, tid);
  __syncthreads();
  Tile::col_sums(slot_e, des, neO, tid);
  Tile::col_sums(slot_g, qs, GQ, tid);

  f32x16 xacc[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) mb_zero(xacc[j]);
  const int nblk = (H1 + 31) / 32;
  const bool dh_mma = !(O & 1) && !(Og & 1);
  for (int m0 = 0; m0 < M; m0 += cm) {
    const int mc = M - m0 < cm ? M - m0 : cm, nc = mc * H1;
    if (dh_mma) {                                // dh = dze We2^T | dzq Wg2^T, K = O | Og, one (MLP, block) per wave
      if ((nc & 1) && g == 0) zt[nc * MB_LD + b] = 0.f;
      for (int job = wave; job < mc * nblk; job += 4) {          // uniform over the wave
        const int mm = job / nblk, blk = job - mm * nblk, m = m0 + mm;
        f32x16 acc;
        mb_zero(acc);
        if (m < ne)
          mb_mma1<true>(acc, des + m * O * MB_LD, O, We2 + (int64_t)m * H1 * O, O, 0, H1, blk * 32, lo, hi);
        else
          mb_mma1<true>(acc, qs + (m - ne) * Og * MB_LD, Og, Wg2 + (int64_t)(m - ne) * H1 * Og, Og, 0, H1, blk * 32, lo,
                        hi);
        const int col = blk * 32 + lo;
        if (col < H1) {                          // the relu mask and the workspace copy straight from the accumulator
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = mb_row(r, hi);
            float v = 0.f;
            if (r0 + row < B) {
              const int64_t at = (r0 + row) * N1 + m * H1 + col;
              v = h[at] > 0.f ? acc[r] : 0.f;
              ws_dz1[at] = v;
            }
            zt[(mm * H1 + col) * MB_LD + row] = v;
          }
        }
      }
      __syncthreads();
    } else {                                     // an odd K has no zero row behind it in LDS: the VALU
      for (int c = g; c < mb_even(nc); c += PL_G) {
        float acc = 0.f;
        if (c < nc) {
          const int mm = c / H1, k = c - mm * H1, m = m0 + mm;
          acc = m < ne ? pl_dot(des + m * O * MB_LD + b, We2 + ((int64_t)m * H1 + k) * O, 1, O, 0.f)
                       : pl_dot(qs + (m - ne) * Og * MB_LD + b, Wg2 + ((int64_t)(m - ne) * H1 + k) * Og, 1, Og, 0.f);
        }
        zt[c * MB_LD + b] = acc;
      }
      __syncthreads();
      Tile::mask_out(zt, h, ws_dz1, r0, B, N1, m0 * H1, nc, tid);
      __syncthreads();
    }
    Tile::col_sums(slot + m0 * H1, zt, nc, tid);
    if (Gin == 1) {                              // dxin += dZ1 W1^T over the chunk's columns
      mb_mma<true>(xacc, zt, nc, W1, N1, m0 * H1, Din, wave, lo, hi);
    } else {                                     // each group's dxin sums its own MLPs' blocks only
      for (int c = g; c < XD; c += PL_G) {
        const int gi = c / Din, k = c - gi * Din;
        float acc = 0.f;
        for (int mm = 0; mm < mc; ++mm) {
          if (d.grp(m0 + mm) != gi) continue;
          acc = pl_dot(zt + mm * H1 * MB_LD + b, W1 + (int64_t)k * N1 + (m0 + mm) * H1, 1, H1, acc);
        }
        dxs[c * MB_LD + b] = dxs[c * MB_LD + b] + acc;
      }
    }
    __syncthreads();                             // the next chunk overwrites zt
  }
  if (Gin == 1) {
#pragma unroll
    for (int j = 0; j < MB_NJ; ++j) {
      const int col = (wave + 4 * j) * 32 + lo;
      if ((wave + 4 * j) * 32 < Din && col < Din) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mb_row(r, hi);
          if (r0 + row < B) dxin[(r0 + row) * Din + col] = xacc[j][r];
        }
      }
    }
  } else {
    Tile::rows_out(dxin, dxs, r0, B, XD, 0, XD, tid);
  }
}

// The small weight gradients, all of them in one launch (small_dw_kernel, tile_ops.h).  Every matrix is A^T G over the
// batch:
//   dWe2[i] = h_i^T dze_i   dWg2[g] = h_{ne+g}^T dzq_g   dWg3s[t] = q_t^T dlg_t   dWg3h = q_T^T dlg_T (not last)
//   dWtw[t] = y_t^T dl_t (last)   and for a grouped level dW1 block m = xin_group(m)^T dZ1_m, written in place in the
//   [Din, N1] layout of dW1,
// laid out one after the other in that order.
struct PlSmall {
  static constexpr int MAXK = PL_MAXO;
  PlDims d;
  const float *xin, *h, *q, *y, *dz1, *dze, *dzq, *dlg, *dl;
  __device__ SmallMat mat(int mq) const {
    const int T = d.T, H1 = d.H1, O = d.O, Og = d.Og, ne = d.ne(), ns = d.ns(), Gout = d.Gout(), N1 = d.N1();
    const int neO = d.neO(), GQ = d.GQ(), GW = d.GW(), GO = d.GO(), Tns = d.Tns();
    const int oG = ne * H1 * O, oS = oG + Gout * H1 * Og, oH = oS + T * Og * ns, oT = oH + (d.last ? 0 : Og * ne);
    const int oW = oT + (d.last ? T * O : 0);
    const int nH = d.last ? 0 : 1, nT = d.last ? T : 0;          // shared-gate and tower matrices
    if (mq < ne) return {h, N1, mq * H1, H1, dze, neO, mq * O, O, mq * H1 * O, O};
    if ((mq -= ne) < Gout) return {h, N1, (ne + mq) * H1, H1, dzq, GQ, mq * Og, Og, oG + mq * H1 * Og, Og};
    if ((mq -= Gout) < T) return {q, GQ, mq * Og, Og, dlg, GW, mq * ns, ns, oS + mq * Og * ns, ns};
    if ((mq -= T) < nH) return {q, GQ, T * Og, Og, dlg, GW, Tns, ne, oH, ne};
    if ((mq -= nH) < nT) return {y, GO, mq * O, O, dl, T, mq, 1, oT + mq * O, 1};
    mq -= nT;                                    // a first layer of a grouped level
    return {xin, d.XD(), d.grp(mq) * d.Din, d.Din, dz1, N1, mq * H1, H1, oW + mq * H1, N1};
  }
};

static int pl_shape(int64_t B, int Din, int Gin, int T, int S, int Sh, int H1, int O, int Og, int last) {
  if (B < 0 || Din < 1 || T < 1 || S < 1 || Sh < 1 || H1 < 1 || O < 1 || Og < 1) return REC_E_ARG;
  if ((last != 0 && last != 1) || (Gin != 1 && Gin != T + 1)) return REC_E_ARG;
  const int64_t ne = (int64_t)T * S + Sh, gw = (int64_t)T * ((int64_t)S + Sh) + (last ? 0 : ne);
  if (Din > PL_MAXD || T > PL_MAXT || H1 > PL_MAXO || ne * O > PL_MAXO || ((int64_t)T + 1) * Og > PL_MAXO ||
      gw > PL_MAXO || (Gin > 1 && (int64_t)Gin * Din > PL_MAXO) || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;
  return REC_OK;
}

static int pl_small_floats(const PlDims& d) {
  return d.ne() * d.H1 * d.O + d.Gout() * d.H1 * d.Og + d.T * d.Og * d.ns() + (d.last ? d.T * d.O : d.Og * d.ne()) +
         (d.Gin > 1 ? d.Din * d.N1() : 0);
}

struct PlWs {
  size_t dz1, dze, dzq, dlg, dl, slots, part, gemm, total;       // offsets in floats
};
static PlWs pl_ws(int64_t B, const PlDims& d) {
  PlWs w{};
  const size_t b = (size_t)B, tiles = (size_t)ceil_div64(B, MB_T);
  WsCarve c;
  w.dz1 = c.take(b * d.N1());
  w.dze = c.take(b * d.neO());
  w.dzq = c.take(b * d.GQ());
  w.dlg = c.take(b * d.GW());
  w.dl = c.take(b * d.T);
  w.slots = c.take(tiles * (size_t)pl_slot_floats(d));
  w.part = c.take((size_t)mb_small_split(B) * pl_small_floats(d));
  w.gemm = c.take(d.Gin == 1 ? mb_dw_gemm_floats(B, d.Din, d.N1()) : 0);
  w.total = c.at;
  return w;
}

}  // namespace

extern "C" size_t rec_ple_cgc_workspace_bytes(int64_t B, int Din, int Gin, int T, int S, int Sh, int H1, int O, int Og,
                                              int last) {
  if (pl_shape(B, Din, Gin, T, S, Sh, H1, O, Og, last) != REC_OK) return 0;
  return sizeof(float) * (pl_ws(B, PlDims{Din, Gin, T, S, Sh, H1, O, Og, last}).total + 4);
}

extern "C" int rec_ple_cgc_fwd_f32(const float* xin, const float* W1, const float* b1, const float* We2,
                                   const float* be2, const float* Wg2, const float* bg2, const float* Wg3s,
                                   const float* Wg3h, const float* Wtw, const float* btw, int64_t B, int Din, int Gin,
                                   int T, int S, int Sh, int H1, int O, int Og, int last, float* y, float* out, float* h,
                                   float* e, float* q, float* g, void* stream) {
  if (int rc = pl_shape(B, Din, Gin, T, S, Sh, H1, O, Og, last)) return rc;
  if (B == 0) return REC_OK;
  if (!xin || !W1 || !b1 || !We2 || !be2 || !Wg2 || !bg2 || !Wg3s || !y) return REC_E_ARG;
  if (last ? (Wg3h || !Wtw || !btw || !out) : (!Wg3h || Wtw || btw || out)) return REC_E_ARG;
  const bool save = h || e || q || g;
  if (save && !(h && e && q && g)) return REC_E_ARG;             // all of them or none
  const PlDims d{Din, Gin, T, S, Sh, H1, O, Og, last};
  if (hipError_t err = rec_allow_lds<ple_cgc_fwd_kernel>(PL_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * pl_lds_floats(d, 0);
  hipLaunchKernelGGL(ple_cgc_fwd_kernel, dim3((unsigned)ceil_div64(B, MB_T)), dim3(PL_NTHR), lds, as_stream(stream), xin,
                     W1, b1, We2, be2, Wg2, bg2, Wg3s, Wg3h, Wtw, btw, B, d, pl_chunk(d, 0), y, out, h, e, q, g);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_ple_cgc_bwd_f32(const float* xin, const float* W1, const float* We2, const float* Wg2,
                                   const float* Wg3s, const float* Wg3h, const float* Wtw, const float* h,
                                   const float* e, const float* q, const float* g, const float* y, const float* out,
                                   const float* dy, const float* dout, int64_t B, int Din, int Gin, int T, int S, int Sh,
                                   int H1, int O, int Og, int last, float* dxin, float* dW1, float* db1, float* dWe2,
                                   float* dbe2, float* dWg2, float* dbg2, float* dWg3s, float* dWg3h, float* dWtw,
                                   float* dbtw, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = pl_shape(B, Din, Gin, T, S, Sh, H1, O, Og, last)) return rc;
  if (B == 0) return REC_OK;
  if (!xin || !W1 || !We2 || !Wg2 || !Wg3s || !h || !e || !q || !g || !y || !dxin || !dW1 || !db1 || !dWe2 || !dbe2 ||
      !dWg2 || !dbg2 || !dWg3s || !workspace)
    return REC_E_ARG;
  if (last ? (Wg3h || dWg3h || !Wtw || !out || !dout || !dWtw || !dbtw)
           : (!Wg3h || !dWg3h || Wtw || out || dout || dWtw || dbtw || !dy))
    return REC_E_ARG;
  const PlDims d{Din, Gin, T, S, Sh, H1, O, Og, last};
  const PlWs w = pl_ws(B, d);
  if (workspace_bytes < sizeof(float) * w.total) return REC_E_WORKSPACE;
  float* base = static_cast<float*>(workspace);
  float *dz1 = base + w.dz1, *dze = base + w.dze, *dzq = base + w.dzq, *dlg = base + w.dlg, *dl = base + w.dl,
        *slots = base + w.slots, *part = base + w.part, *gws = base + w.gemm;
  hipStream_t st = as_stream(stream);
  const int tiles = (int)ceil_div64(B, MB_T), ne = d.ne(), ns = d.ns(), Gout = d.Gout(), N1 = d.N1();
  if (hipError_t err = rec_allow_lds<ple_cgc_bwd_kernel>(PL_LDS_CAP)) return (int)err;
  const size_t lds = sizeof(float) * pl_lds_floats(d, 1);
  hipLaunchKernelGGL(ple_cgc_bwd_kernel, dim3(tiles), dim3(PL_NTHR), lds, st, W1, We2, Wg2, Wg3s, Wg3h, Wtw, h, e, q, g,
                     out, dy, dout, B, d, pl_chunk(d, 1), dxin, dz1, dze, dzq, dlg, dl, slots);
  REC_LAUNCH_CHECK();
  if (int rc = rec_slot_sum(REC_SLOTS_WAVE, pl_slot_floats(d), tiles, slots,
                            {{db1, dbe2, dbg2, dbtw}, {N1, d.neO(), d.GQ(), last ? T : 0}}, st))
    return rc;
  const int Sl = mb_small_split(B), wtot = pl_small_floats(d);
  int big = H1 * (O > Og ? O : Og);
  if (Og * (ne > ns ? ne : ns) > big) big = Og * (ne > ns ? ne : ns);
  if (Gin > 1 && Din * H1 > big) big = Din * H1;
  const int mats = ne + Gout + T + (last ? T : 1) + (Gin > 1 ? d.M() : 0);
  if (int rc = small_dw_launch(PlSmall{d, xin, h, q, y, dz1, dze, dzq, dlg, dl}, mats, big, wtot, B, part, st)) return rc;
  if (int rc = rec_slot_sum(REC_SLOTS_SERIAL, wtot, Sl, part,
                            {{dWe2, dWg2, dWg3s, dWg3h, dWtw, dW1},
                             {ne * H1 * O, Gout * H1 * Og, T * Og * ns, last ? 0 : Og * ne, last ? T * O : 0,
                              Gin > 1 ? Din * N1 : 0}},
                            st))
    return rc;
  if (Gin > 1) return REC_OK;
  return mb_dw_gemm(Din, N1, B, xin, dz1, dW1, gws, stream);   // dW1 = xin^T dZ1
}
