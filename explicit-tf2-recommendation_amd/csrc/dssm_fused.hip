// Fused DSSM two-tower train step (2.FM/CustomLayers.py:208-239 under 2.FM/ModelManager.py:171-177): two launches.
//
// Main launch: a workgroup owns M consecutive examples (M = 32, or 16 when the tile's rows would not fit the LDS) and, for
// both towers, gathers the rows ids -> [F, E] of each example (64-bit row offsets), runs the tower MLP
// F*E -> 64 (relu) -> 32 (relu) -> 8 (linear) on fp32 MFMA (v_mfma_f32_16x16x4_f32), the score (1 - cos)/2 with
// tf.nn.l2_normalize's x * rsqrt(max(sum x^2, 1e-12)), the Keras BCE on probabilities and the whole backward.  It writes
// the per-lookup gradient rows of both tables (dX = dH1 . W0^T, one [F*E] row per example) and, per workgroup, its
// contributions to the twelve dense gradients and its sum of per-example loss terms into the workspace.
//
// Post launch: the fixed-order reduction of those per-workgroup partials (loss = their sum / B) side by side with the
// segment sums of both towers' gradient rows over a rec_dedup_plan_i64 of each tower's flat [B*F] ids -- and, optionally,
// the touched-rows Adam update of each unique row (rec_adam_rows_f32's arithmetic: common.h adam_touch) with the step
// size read from device memory.
//
// No float atomics: every sum has a fixed order, so two runs on the same inputs are bit-identical.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int H1 = 64, H2 = 32, DO = 8;     // mlp_dims [64, 32], final_dim 8
constexpr int LH1 = H1 + 4, LH2 = H2 + 4;   // LDS row strides (odd multiples of 4 floats: no bank conflicts on columns)
constexpr int MAXF = 8;
constexpr int NT = 256;                     // threads of a main-launch workgroup (4 waves)
constexpr size_t LDS_LIMIT = REC_LDS_CU_BYTES;

// floats of one tower's dense partials in a workgroup block: dW0 [K0,64], db0 [64], dW1 [64,32], db1 [32], dWf [32,8], dbf [8]
__host__ __device__ inline int64_t tower_partials(int K0) { return (int64_t)K0 * H1 + H1 + H1 * H2 + H2 + H2 * DO + DO; }
__host__ __device__ inline int64_t block_floats(int K0u, int K0i) {
  return (tower_partials(K0u) + tower_partials(K0i) + 1 + 3) & ~int64_t(3);
}
// LDS floats of the main launch at tile M: X of both towers, H1 / H2 / O of both towers, dO of both towers, dH1 / dH2
// (shared by the towers' backward passes, which run one after the other), the per-example loss terms
// (X rows are padded to a multiple of 16 columns: the dK0 and dX blocks are 16 wide)
__host__ __device__ inline int pad16(int K0) { return (K0 + 15) & ~15; }
inline size_t lds_floats(int M, int K0u, int K0i) {
  return (size_t)M * ((pad16(K0u) + 4) + (pad16(K0i) + 4) + 2 * (LH1 + LH2 + DO) + 2 * DO + LH1 + LH2 + 1);
}
inline int tile_rows(int K0u, int K0i) { return lds_floats(32, K0u, K0i) * 4 <= LDS_LIMIT ? 32 : 16; }

struct Tower {
  const float* table;
  int64_t ld, V;
  const int64_t* ids;     // [B, F] row-major
  int F;
  const float *K0, *b0, *K1, *b1, *Kf, *bf;
  float* vals;            // [B, F*E] per-lookup gradient rows
  float* emb;             // [B, 8] or null
};

struct MainArgs {
  Tower t[2];
  int64_t B;
  const float* label;
  float* score;
  int* oob;
  float* ws;
  int64_t blk;            // floats per workgroup block of ws
  int64_t* step_dev;
  const float* lr_tab;
  int64_t n_tab;
  float* lr_t_dev;
};

// One 16x16 block of C = A[16,K] . B[K,16] on v_mfma_f32_16x16x4_f32 (lane l: A[l&15][k+(l>>4)], B[k+(l>>4)][l&15]; C: row
// 4*(l>>4)+q, column l&15).  Eight k-steps are loaded before they are multiplied, so that operands read from global
// memory (the weights: L2-resident) overlap their latency.  K is a multiple of 4.
template <class FA, class FB>
__device__ __forceinline__ f32x4 mma16(FA a, FB b, int K, int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int r = lane & 15, kk = lane >> 4;
  int k = 0;
  for (; k + 32 <= K; k += 32) {
    float av[8], bv[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      av[s] = a(r, k + 4 * s + kk);
      bv[s] = b(k + 4 * s + kk, r);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  }
  for (; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a(r, k + kk), b(k + kk, r), acc, 0, 0, 0);
  return acc;
}

template <int E, int M>
__global__ __launch_bounds__(NT) void dssm_main_kernel(MainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int C4 = E / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * M;
  const int nrow = (int)((a.B - b0) < M ? (a.B - b0) : M);    // valid examples of the tile
  if (a.step_dev && blockIdx.x == 0 && tid == 0) {
    // the optimizer's device-side step counter (the launches behind this one on the stream see the new step)
    const int64_t s = *a.step_dev + 1;
    *a.step_dev = s;
    *a.lr_t_dev = a.lr_tab[(s < a.n_tab ? s : a.n_tab) - 1];
  }
  const int K0[2] = {a.t[0].F * E, a.t[1].F * E};
  const int LX[2] = {pad16(K0[0]) + 4, pad16(K0[1]) + 4};
  float* X[2];
  X[0] = lds;
  X[1] = X[0] + M * LX[0];
  float* sH1[2];
  float* sH2[2];
  float* sO[2];
  float* sdO[2];
  sH1[0] = X[1] + M * LX[1];
  sH1[1] = sH1[0] + M * LH1;
  sH2[0] = sH1[1] + M * LH1;
  sH2[1] = sH2[0] + M * LH2;
  sO[0] = sH2[1] + M * LH2;
  sO[1] = sO[0] + M * DO;
  sdO[0] = sO[1] + M * DO;
  sdO[1] = sdO[0] + M * DO;
  float* dH1 = sdO[1] + M * DO;
  float* dH2 = dH1 + M * LH1;
  float* lossv = dH2 + M * LH2;

  // ---- gather: rows of both towers (zero rows for the tail of the tile and for ids outside [0, V))
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const Tower& T = a.t[t];
    const int F = T.F, n4 = M * F * C4;
#pragma unroll 4
    for (int idx = tid; idx < n4; idx += NT) {
      const int bf = idx / C4, c = idx - bf * C4;
      const int b = bf / F, f = bf - b * F;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b < nrow) {
        const int64_t id = T.ids[(b0 + b) * F + f];
        if ((uint64_t)id < (uint64_t)T.V)
          v = reinterpret_cast<const float4*>(T.table + id * T.ld)[c];
        else if (c == 0)
          atomicOr(a.oob, 1);
      }
      *reinterpret_cast<float4*>(X[t] + b * LX[t] + f * E + 4 * c) = v;
    }
  }
  __syncthreads();

  // ---- forward of both towers
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const Tower& T = a.t[t];
    const float* x = X[t];
    const int lx = LX[t];
    const float* W0 = T.K0;
    for (int blk = wave; blk < (M / 16) * (H1 / 16); blk += 4) {     // H1 = relu(X . K0 + b0)
      const int mi = blk / (H1 / 16), nj = blk % (H1 / 16);
      f32x4 acc = mma16([&](int i, int k) { return x[(mi * 16 + i) * lx + k]; },
                        [&](int k, int j) { return W0[k * H1 + nj * 16 + j]; }, K0[t], lane);
      const int col = nj * 16 + (lane & 15);
      const float bias = T.b0[col];
#pragma unroll
      for (int q = 0; q < 4; ++q) sH1[t][(mi * 16 + 4 * (lane >> 4) + q) * LH1 + col] = fmaxf(acc[q] + bias, 0.f);
    }
    __syncthreads();
    const float* h1 = sH1[t];
    for (int blk = wave; blk < (M / 16) * (H2 / 16); blk += 4) {     // H2 = relu(H1 . K1 + b1)
      const int mi = blk / (H2 / 16), nj = blk % (H2 / 16);
      f32x4 acc = mma16([&](int i, int k) { return h1[(mi * 16 + i) * LH1 + k]; },
                        [&](int k, int j) { return T.K1[k * H2 + nj * 16 + j]; }, H1, lane);
      const int col = nj * 16 + (lane & 15);
      const float bias = T.b1[col];
#pragma unroll
      for (int q = 0; q < 4; ++q) sH2[t][(mi * 16 + 4 * (lane >> 4) + q) * LH2 + col] = fmaxf(acc[q] + bias, 0.f);
    }
    __syncthreads();
    for (int idx = tid; idx < M * DO; idx += NT) {                    // O = H2 . Kf + bf
      const int b = idx / DO, c = idx % DO;
      float s = T.bf[c];
      for (int k = 0; k < H2; ++k) s = fmaf(sH2[t][b * LH2 + k], T.Kf[k * DO + c], s);
      sO[t][b * DO + c] = s;
    }
  }
  __syncthreads();

  // ---- score, loss term and the gradient at both towers' outputs (one thread per example)
  if (tid < M) {
    const int b = tid;
    const float* u = sO[0] + b * DO;
    const float* v = sO[1] + b * DO;
    float su = 0.f, sv = 0.f;
#pragma unroll
    for (int c = 0; c < DO; ++c) {
      su = fmaf(u[c], u[c], su);
      sv = fmaf(v[c], v[c], sv);
    }
    const float ru = rsqrtf(fmaxf(su, 1e-12f)), rv = rsqrtf(fmaxf(sv, 1e-12f));
    float un[DO], vn[DO], cs = 0.f;
#pragma unroll
    for (int c = 0; c < DO; ++c) {
      un[c] = u[c] * ru;
      vn[c] = v[c] * rv;
      cs = fmaf(un[c], vn[c], cs);
    }
    const float p = (1.f - cs) * 0.5f;
    float term = 0.f, dp = 0.f;
    if (b < nrow) {
      const float y = a.label[b0 + b];
      const float eps = 1e-7f;
      const float pc = fminf(fmaxf(p, eps), 1.f - eps);
      term = -(y * logf(pc + eps) + (1.f - y) * logf(1.f - pc + eps));
      if (p >= eps && p <= 1.f - eps) dp = (-(y / (pc + eps)) + (1.f - y) / (1.f - pc + eps)) / (float)a.B;
      if (a.score) a.score[b0 + b] = p;
      if (a.t[0].emb) for (int c = 0; c < DO; ++c) a.t[0].emb[(b0 + b) * DO + c] = u[c];
      if (a.t[1].emb) for (int c = 0; c < DO; ++c) a.t[1].emb[(b0 + b) * DO + c] = v[c];
    }
    lossv[b] = term;
    const float dcs = -0.5f * dp;
    // d un = dcs * vn, d vn = dcs * un; through x * rsqrt(max(sum x^2, 1e-12)): dx = r (dn - n (n . dn)) (the second
    // term only where the clamp is inactive)
    float pu = 0.f, pv = 0.f;
#pragma unroll
    for (int c = 0; c < DO; ++c) {
      pu = fmaf(un[c], dcs * vn[c], pu);
      pv = fmaf(vn[c], dcs * un[c], pv);
    }
    if (su < 1e-12f) pu = 0.f;
    if (sv < 1e-12f) pv = 0.f;
#pragma unroll
    for (int c = 0; c < DO; ++c) {
      sdO[0][b * DO + c] = ru * (dcs * vn[c] - un[c] * pu);
      sdO[1][b * DO + c] = rv * (dcs * un[c] - vn[c] * pv);
    }
  }
  __syncthreads();
  float* part = a.ws + (int64_t)blockIdx.x * a.blk;
  if (tid == 0) {
    float s = 0.f;
    for (int b = 0; b < M; ++b) s += lossv[b];
    part[tower_partials(K0[0]) + tower_partials(K0[1])] = s;
  }

  // ---- backward of each tower
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const Tower& T = a.t[t];
    const float* x = X[t];
    const int lx = LX[t], k0 = K0[t];
    const float* h1 = sH1[t];
    const float* h2 = sH2[t];
    const float* dO = sdO[t];
    float* pW0 = part;
    float* pb0 = pW0 + (int64_t)k0 * H1;
    float* pW1 = pb0 + H1;
    float* pb1 = pW1 + H1 * H2;
    float* pWf = pb1 + H2;
    float* pbf = pWf + H2 * DO;
    {                                                                  // dKf = H2^T dO, dbf = colsum dO
      const int k = tid / DO, c = tid % DO;                            // NT = H2 * DO
      float s = 0.f;
      for (int b = 0; b < M; ++b) s = fmaf(h2[b * LH2 + k], dO[b * DO + c], s);
      pWf[k * DO + c] = s;
      if (tid < DO) {
        float sb = 0.f;
        for (int b = 0; b < M; ++b) sb += dO[b * DO + tid];
        pbf[tid] = sb;
      }
    }
    for (int idx = tid; idx < M * H2; idx += NT) {                     // dH2 = (dO . Kf^T) * [H2 > 0]
      const int b = idx / H2, k = idx % H2;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < DO; ++c) s = fmaf(dO[b * DO + c], T.Kf[k * DO + c], s);
      dH2[b * LH2 + k] = h2[b * LH2 + k] > 0.f ? s : 0.f;
    }
    __syncthreads();
    for (int blk = wave; blk < (H1 / 16) * (H2 / 16); blk += 4) {    // dK1 = H1^T dH2
      const int mi = blk / (H2 / 16), nj = blk % (H2 / 16);
      f32x4 acc = mma16([&](int i, int k) { return h1[k * LH1 + mi * 16 + i]; },
                        [&](int k, int j) { return dH2[k * LH2 + nj * 16 + j]; }, M, lane);
      const int col = nj * 16 + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; ++q) pW1[(mi * 16 + 4 * (lane >> 4) + q) * H2 + col] = acc[q];
    }
    if (tid < H2) {
      float s = 0.f;
      for (int b = 0; b < M; ++b) s += dH2[b * LH2 + tid];
      pb1[tid] = s;
    }
    for (int blk = wave; blk < (M / 16) * (H1 / 16); blk += 4) {     // dH1 = (dH2 . K1^T) * [H1 > 0]
      const int mi = blk / (H1 / 16), nj = blk % (H1 / 16);
      f32x4 acc = mma16([&](int i, int k) { return dH2[(mi * 16 + i) * LH2 + k]; },
                        [&](int k, int j) { return T.K1[(nj * 16 + j) * H2 + k]; }, H2, lane);
      const int col = nj * 16 + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = mi * 16 + 4 * (lane >> 4) + q;
        dH1[row * LH1 + col] = h1[row * LH1 + col] > 0.f ? acc[q] : 0.f;
      }
    }
    __syncthreads();
    for (int blk = wave; blk < (pad16(k0) / 16) * (H1 / 16); blk += 4) {   // dK0 = X^T dH1
      const int mi = blk / (H1 / 16), nj = blk % (H1 / 16);
      f32x4 acc = mma16([&](int i, int k) { return x[k * lx + mi * 16 + i]; },
                        [&](int k, int j) { return dH1[k * LH1 + nj * 16 + j]; }, M, lane);
      const int col = nj * 16 + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = mi * 16 + 4 * (lane >> 4) + q;
        if (row < k0) pW0[(int64_t)row * H1 + col] = acc[q];
      }
    }
    if (tid < H1) {
      float s = 0.f;
      for (int b = 0; b < M; ++b) s += dH1[b * LH1 + tid];
      pb0[tid] = s;
    }
    const float* W0 = T.K0;
    for (int blk = wave; blk < (M / 16) * (pad16(k0) / 16); blk += 4) {   // dX = dH1 . K0^T -> per-lookup rows
      const int nb = pad16(k0) / 16;
      const int mi = blk / nb, nj = blk % nb;
      f32x4 acc = mma16([&](int i, int k) { return dH1[(mi * 16 + i) * LH1 + k]; },
                        [&](int k, int j) { return nj * 16 + j < k0 ? W0[(nj * 16 + j) * H1 + k] : 0.f; }, H1, lane);
      const int col = nj * 16 + (lane & 15);
      const int f = col / E;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = mi * 16 + 4 * (lane >> 4) + q;
        if (row < nrow && col < k0) {
          const int64_t id = T.ids[(b0 + row) * T.F + f];
          T.vals[(b0 + row) * k0 + col] = (uint64_t)id < (uint64_t)T.V ? acc[q] : 0.f;
        }
      }
    }
    __syncthreads();                                                   // dH1 / dH2 are reused by the next tower
    part += tower_partials(k0);
  }
}

// ---- post launch
struct SegTower {
  const float* vals;      // [n, E]
  const int32_t* perm;
  const int32_t* seg;
  const int64_t* uniq;
  const int64_t* n_uniq;
  float* rows;            // [n, E]
  int64_t n;
  float *table, *m, *v;   // optional touched-rows Adam
  int64_t ld, V;
};

struct PostArgs {
  const float* ws;
  int64_t blk, nwg, ndense, B;
  int K0[2];
  float* grads[12];
  float* loss;
  SegTower s[2];
  int64_t seg_blocks0;    // workgroups of tower 0's segment sums (4 unique slots each)
  int64_t dense_blocks;
  const float* lr_t_dev;
  float b1, b2, eps;
};

constexpr int DGRP = 8, DEL = 32;     // dense reduction: 32 elements x 8 fixed-stride groups of workgroups per block

template <int E>
__global__ __launch_bounds__(256) void dssm_post_kernel(PostArgs a) {
  __shared__ float4 red[256];
  const int tid = threadIdx.x;
  int64_t bid = blockIdx.x;
  if (bid < a.dense_blocks) {
    const int g = tid / DEL, e = tid % DEL;
    const int64_t idx = bid * DEL + e;
    float s = 0.f;
    if (idx < a.ndense)
      for (int64_t w = g; w < a.nwg; w += DGRP) s += a.ws[w * a.blk + idx];
    reinterpret_cast<float*>(red)[tid] = s;
    __syncthreads();
    if (tid < DEL && idx < a.ndense) {
      float tot = 0.f;
      for (int q = 0; q < DGRP; ++q) tot += reinterpret_cast<float*>(red)[q * DEL + tid];
      int64_t o = idx;
      int t = 0;
      const int64_t p0 = tower_partials(a.K0[0]);
      if (o >= p0) {
        o -= p0;
        t = 1;
        if (o >= tower_partials(a.K0[1])) {
          *a.loss = tot / (float)a.B;
          return;
        }
      }
      const int64_t sizes[6] = {(int64_t)a.K0[t] * H1, H1, H1 * H2, H2, H2 * DO, DO};
      int j = 0;
      while (o >= sizes[j]) o -= sizes[j++];
      a.grads[6 * t + j][o] = tot;
    }
    return;
  }
  bid -= a.dense_blocks;
  const int t = bid < a.seg_blocks0 ? 0 : 1;
  if (t) bid -= a.seg_blocks0;
  const SegTower& S = a.s[t];
  constexpr int C4 = E / 4, G = 64 / C4;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane / C4, c = lane % C4;
  const int64_t u = bid * 4 + wave;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (u < S.n) {
    const int lo = S.seg[u], hi = S.seg[u + 1];
    const float4* vals = reinterpret_cast<const float4*>(S.vals);
    for (int s = lo + g; s < hi; s += G) {                            // group g: positions lo+g, lo+g+G, ... in order
      const float4 x = vals[(int64_t)S.perm[s] * C4 + c];
      acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (u < S.n && g == 0) {
    float4 tot = red[wave * 64 + c];
    for (int q = 1; q < G; ++q) {                                      // groups combined in a fixed order
      const float4 x = red[wave * 64 + q * C4 + c];
      tot.x += x.x; tot.y += x.y; tot.z += x.z; tot.w += x.w;
    }
    reinterpret_cast<float4*>(S.rows)[u * C4 + c] = tot;
    if (a.lr_t_dev && u < *S.n_uniq) {
      const int64_t id = S.uniq[u];
      if ((uint64_t)id < (uint64_t)S.V) {
        const float lr_t = *a.lr_t_dev;
        float4* xp = reinterpret_cast<float4*>(S.table + id * S.ld) + c;
        float4* mp = reinterpret_cast<float4*>(S.m + id * E) + c;
        float4* vp = reinterpret_cast<float4*>(S.v + id * E) + c;
        float4 x = *xp, m = *mp, v = *vp;
        adam_touch(x.x, m.x, v.x, tot.x, lr_t, a.b1, a.b2, a.eps);
        adam_touch(x.y, m.y, v.y, tot.y, lr_t, a.b1, a.b2, a.eps);
        adam_touch(x.z, m.z, v.z, tot.z, lr_t, a.b1, a.b2, a.eps);
        adam_touch(x.w, m.w, v.w, tot.w, lr_t, a.b1, a.b2, a.eps);
        *xp = x; *mp = m; *vp = v;
      }
    }
  }
}

inline bool supported_e(int E) { return E == 8 || E == 16 || E == 32 || E == 64; }

}  // namespace

extern "C" size_t rec_dssm_fused_workspace_bytes(int64_t B, int E, int F_u, int F_i) {
  if (B < 1 || !supported_e(E) || F_u < 1 || F_u > MAXF || F_i < 1 || F_i > MAXF) return 0;
  const int K0u = F_u * E, K0i = F_i * E;
  const int64_t nwg = ceil_div64(B, tile_rows(K0u, K0i));
  return sizeof(float) * (size_t)(nwg * block_floats(K0u, K0i));
}

extern "C" int rec_dssm_fused_main_f32(const float* u_table, int64_t u_ld, int64_t u_V, const int64_t* u_ids, int F_u,
                                       const float* i_table, int64_t i_ld, int64_t i_V, const int64_t* i_ids, int F_i,
                                       int E, int h1, int h2, int d_out, int64_t B, const float* const* weights,
                                       const float* label, float* u_vals, float* i_vals, float* user_emb,
                                       float* item_emb, float* score, int* oob_flag, void* workspace,
                                       size_t workspace_bytes, int64_t* step_dev, const float* lr_table,
                                       int64_t n_table, float* lr_t_dev, void* stream) {
  if (!u_table || !i_table || !u_ids || !i_ids || !weights || !label || !u_vals || !i_vals || !oob_flag || !workspace ||
      B < 1 || u_V < 1 || i_V < 1)
    return REC_E_ARG;
  if (!supported_e(E) || F_u < 1 || F_u > MAXF || F_i < 1 || F_i > MAXF || h1 != H1 || h2 != H2 || d_out != DO)
    return REC_E_UNSUPPORTED;
  if (u_ld < E || i_ld < E || (u_ld & 3) || (i_ld & 3) || !rec_is_aligned16(u_table) || !rec_is_aligned16(i_table) ||
      !rec_is_aligned16(workspace))
    return REC_E_ARG;
  for (int j = 0; j < 12; ++j)
    if (!weights[j]) return REC_E_ARG;
  if (step_dev && (!lr_table || n_table < 1 || !lr_t_dev)) return REC_E_ARG;
  if (workspace_bytes < rec_dssm_fused_workspace_bytes(B, E, F_u, F_i)) return REC_E_WORKSPACE;
  const int K0u = F_u * E, K0i = F_i * E;
  const int M = tile_rows(K0u, K0i);
  MainArgs a;
  a.t[0] = Tower{u_table, u_ld, u_V, u_ids, F_u, weights[0], weights[1], weights[2], weights[3], weights[4], weights[5],
                 u_vals, user_emb};
  a.t[1] = Tower{i_table, i_ld, i_V, i_ids, F_i, weights[6], weights[7], weights[8], weights[9], weights[10],
                 weights[11], i_vals, item_emb};
  a.B = B;
  a.label = label;
  a.score = score;
  a.oob = oob_flag;
  a.ws = (float*)workspace;
  a.blk = block_floats(K0u, K0i);
  a.step_dev = step_dev;
  a.lr_tab = lr_table;
  a.n_tab = n_table;
  a.lr_t_dev = lr_t_dev;
  const size_t lds = 4 * lds_floats(M, K0u, K0i);
  const unsigned nwg = (unsigned)ceil_div64(B, M);
  hipStream_t st = as_stream(stream);
#define DSSM_MAIN(EE, MM)                                                                                           \
  do {                                                                                                              \
    if (hipError_t e = rec_allow_lds<dssm_main_kernel<EE, MM>>(LDS_LIMIT)) return (int)e;                          \
    hipLaunchKernelGGL((dssm_main_kernel<EE, MM>), dim3(nwg), dim3(NT), lds, st, a);                                \
  } while (0)
#define DSSM_MAIN_E(EE) \
  do {                  \
    if (M == 32) DSSM_MAIN(EE, 32); else DSSM_MAIN(EE, 16); \
  } while (0)
  switch (E) {
    case 8: DSSM_MAIN_E(8); break;
    case 16: DSSM_MAIN_E(16); break;
    case 32: DSSM_MAIN_E(32); break;
    default: DSSM_MAIN_E(64); break;
  }
#undef DSSM_MAIN_E
#undef DSSM_MAIN
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_dssm_fused_post_f32(int64_t B, int E, int F_u, int F_i, const void* workspace,
                                       size_t workspace_bytes, float* const* grads, float* loss, const float* u_vals,
                                       const int32_t* u_perm, const int32_t* u_seg, const int64_t* u_uniq,
                                       const int64_t* u_n_uniq, float* u_rows, const float* i_vals,
                                       const int32_t* i_perm, const int32_t* i_seg, const int64_t* i_uniq,
                                       const int64_t* i_n_uniq, float* i_rows, float* const* adam, int64_t u_ld,
                                       int64_t u_V, int64_t i_ld, int64_t i_V, const float* lr_t_dev, float b1,
                                       float b2, float eps, void* stream) {
  if (!workspace || !grads || !loss || !u_vals || !u_perm || !u_seg || !u_uniq || !u_n_uniq || !u_rows || !i_vals ||
      !i_perm || !i_seg || !i_uniq || !i_n_uniq || !i_rows || B < 1)
    return REC_E_ARG;
  if (!supported_e(E) || F_u < 1 || F_u > MAXF || F_i < 1 || F_i > MAXF) return REC_E_UNSUPPORTED;
  for (int j = 0; j < 12; ++j)
    if (!grads[j]) return REC_E_ARG;
  if (!rec_is_aligned16(u_vals) || !rec_is_aligned16(i_vals) || !rec_is_aligned16(u_rows) || !rec_is_aligned16(i_rows))
    return REC_E_ARG;
  if (adam) {
    if (!lr_t_dev || u_V < 1 || i_V < 1 || u_ld < E || i_ld < E || (u_ld & 3) || (i_ld & 3)) return REC_E_ARG;
    for (int j = 0; j < 6; ++j)
      if (!adam[j] || !rec_is_aligned16(adam[j])) return REC_E_ARG;
  }
  if (workspace_bytes < rec_dssm_fused_workspace_bytes(B, E, F_u, F_i)) return REC_E_WORKSPACE;
  const int K0u = F_u * E, K0i = F_i * E;
  PostArgs a;
  a.ws = (const float*)workspace;
  a.blk = block_floats(K0u, K0i);
  a.nwg = ceil_div64(B, tile_rows(K0u, K0i));
  a.ndense = tower_partials(K0u) + tower_partials(K0i) + 1;
  a.B = B;
  a.K0[0] = K0u;
  a.K0[1] = K0i;
  for (int j = 0; j < 12; ++j) a.grads[j] = grads[j];
  a.loss = loss;
  a.s[0] = SegTower{u_vals, u_perm, u_seg, u_uniq, u_n_uniq, u_rows, B * F_u, adam ? adam[0] : nullptr,
                    adam ? adam[1] : nullptr, adam ? adam[2] : nullptr, u_ld, u_V};
  a.s[1] = SegTower{i_vals, i_perm, i_seg, i_uniq, i_n_uniq, i_rows, B * F_i, adam ? adam[3] : nullptr,
                    adam ? adam[4] : nullptr, adam ? adam[5] : nullptr, i_ld, i_V};
  a.dense_blocks = ceil_div64(a.ndense, DEL);
  a.seg_blocks0 = ceil_div64(B * F_u, 4);
  a.lr_t_dev = adam ? lr_t_dev : nullptr;
  a.b1 = b1;
  a.b2 = b2;
  a.eps = eps;
  const unsigned grid = (unsigned)(a.dense_blocks + a.seg_blocks0 + ceil_div64(B * F_i, 4));
  hipStream_t st = as_stream(stream);
  switch (E) {
    case 8: hipLaunchKernelGGL(dssm_post_kernel<8>, dim3(grid), dim3(256), 0, st, a); break;
    case 16: hipLaunchKernelGGL(dssm_post_kernel<16>, dim3(grid), dim3(256), 0, st, a); break;
    case 32: hipLaunchKernelGGL(dssm_post_kernel<32>, dim3(grid), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(dssm_post_kernel<64>, dim3(grid), dim3(256), 0, st, a); break;
  }
  REC_LAUNCH_CHECK();
  return REC_OK;
}
