// What the tile kernels of masknet.hip, contextnet.hip, fibinetplus.hip, mmoe.hip and ple.hip share around the MFMA tile
// of mfma_tile.h: the row / column passes over a k-major LDS operand, the batched small weight-gradient launch, and the
// host plumbing of a backward entry point (workspace carving, batch slices, the split-K weight-gradient GEMM).  Include it
// after the file's `#pragma clang fp contract(off)`: the loops and the order of their additions define result bits.
#pragma once
#include "mfma_tile.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// device: passes over k-major LDS operands [column][LD] of a tile of ROWS examples, by a workgroup of NTHR threads
// ------------------------------------------------------------------------------------------------------------------
template <int ROWS, int LD, int NTHR>
struct TileOps {
  // rows of consecutive columns out of an operand: dst[(r0 + row) ld + c0 + c] = src[c][row], c < nc
  static __device__ __forceinline__ void rows_out(float* __restrict__ dst, const float* src, int64_t r0, int64_t B,
                                                  int ld, int c0, int nc, int tid) {
    for (int i = tid; i < ROWS * nc; i += NTHR) {
      const int row = i / nc, c = i - row * nc;
      if (r0 + row < B) dst[(r0 + row) * ld + c0 + c] = src[c * LD + row];
    }
  }
  // and into one; rows past the batch read as zero, and so does all of it when src is NULL
  static __device__ __forceinline__ void rows_in(float* dst, const float* __restrict__ src, int64_t r0, int64_t B,
                                                 int ld, int c0, int nc, int tid) {
    for (int i = tid; i < ROWS * nc; i += NTHR) {
      const int row = i / nc, c = i - row * nc;
      dst[c * LD + row] = (src && r0 + row < B) ? src[(r0 + row) * ld + c0 + c] : 0.f;
    }
  }
  // buf <- buf (.) [act > 0] in place, and its copy to the workspace; rows past the batch become zero
  static __device__ __forceinline__ void mask_out(float* buf, const float* __restrict__ act, float* __restrict__ ws,
                                                  int64_t r0, int64_t B, int ld, int c0, int nc, int tid) {
    for (int i = tid; i < ROWS * nc; i += NTHR) {
      const int row = i / nc, c = i - row * nc;
      float v = 0.f;
      if (r0 + row < B) {
        const int64_t at = (r0 + row) * ld + c0 + c;
        v = act[at] > 0.f ? buf[c * LD + row] : 0.f;
        ws[at] = v;
      }
      buf[c * LD + row] = v;
    }
  }
  // column sums of the tile, rows in order: out[c] = sum_row a[c][row] (* b[c][row] when b is given)
  static __device__ __forceinline__ void col_sums(float* __restrict__ out, const float* a, int nc, int tid,
                                                  const float* b = nullptr) {
    for (int c = tid; c < nc; c += NTHR) {
      float s = 0.f;
      for (int r = 0; r < ROWS; ++r) s += b ? a[c * LD + r] * b[c * LD + r] : a[c * LD + r];
      out[c] = s;
    }
  }
  // softmax over n elements of stride LD (one example's entries of n columns); dst may be src
  static __device__ __forceinline__ void softmax(const float* src, float* dst, int n) {
    float m = src[0];
    for (int i = 1; i < n; ++i) m = fmaxf(m, src[i * LD]);
    float s = 0.f;
    for (int i = 0; i < n; ++i) {
      const float ex = expf(src[i * LD] - m);
      dst[i * LD] = ex;
      s += ex;
    }
    for (int i = 0; i < n; ++i) dst[i * LD] = dst[i * LD] / s;
  }
  // dz over dg in place: dz = g (.) (dg - sum(dg (.) g))
  static __device__ __forceinline__ void softmax_bwd(const float* gp, float* dp, int n) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += dp[i * LD] * gp[i * LD];
    for (int i = 0; i < n; ++i) dp[i * LD] = gp[i * LD] * (dp[i * LD] - s);
  }
};

// ------------------------------------------------------------------------------------------------------------------
// the small weight gradients of a backward, all of them in one launch
// ------------------------------------------------------------------------------------------------------------------
constexpr int DW_NTHR = 256;
constexpr int DW_ROWS = 32;                      // examples of one step

// One matrix [M, N] = A^T G over the batch: A(b, m) = A[b lda + a0 + m] (times scale[b lds + s0 + m / sdiv] when scale is
// given), G(b, c) = G[b ldg + g0 + c]; output (m, c) goes to element off + m ldo + c of a slice's partials.
struct SmallMat {
  const float* A;
  int lda, a0, M;
  const float* G;
  int ldg, g0, N, off, ldo;
  const float* scale = nullptr;
  int lds = 0, s0 = 0, sdiv = 1;
};

// slices of the small weight gradients over the batch: at most 16, at least 256 examples each
static inline int mb_small_split(int64_t B) {
  const int64_t s = B / 256;
  return s < 1 ? 1 : (s > 16 ? 16 : (int)s);
}

// Family: a struct passed by value with the dims and pointers of one layer family, `__device__ SmallMat mat(int q) const`
// for matrix q of the launch and `static constexpr int MAXK` >= every M and N.  Workgroup (q and a block of 256 outputs,
// s) adds the examples of batch slice s, in order, into part[s], one output per thread; rec_slot_sum adds the slices in
// slice order.
template <class Family>
__global__ __launch_bounds__(DW_NTHR) void small_dw_kernel(Family f, int64_t B, int maxblk, int64_t per, int wtot,
                                                           float* __restrict__ part) {
  __shared__ float as[DW_ROWS * Family::MAXK], gsh[DW_ROWS * Family::MAXK];
  const int tid = threadIdx.x, blk = blockIdx.x % maxblk;
  const SmallMat t = f.mat(blockIdx.x / maxblk);
  const int M = t.M, N = t.N;
  if (blk * DW_NTHR >= M * N) return;            // uniform over the workgroup
  const int o = blk * DW_NTHR + tid;
  const bool own = o < M * N;
  const int om = own ? o / N : 0, on = own ? o - om * N : 0;
  const int64_t b0 = (int64_t)blockIdx.y * per, b1 = b0 + per < B ? b0 + per : B;
  float acc = 0.f;
  for (int64_t bb = b0; bb < b1; bb += DW_ROWS) {
    for (int i = tid; i < DW_ROWS * M; i += DW_NTHR) {
      const int r = i / M, m = i - r * M;
      float v = 0.f;
      if (bb + r < b1) {
        v = t.A[(bb + r) * t.lda + t.a0 + m];
        if (t.scale) v = v * t.scale[(bb + r) * t.lds + t.s0 + m / t.sdiv];
      }
      as[i] = v;
    }
    for (int i = tid; i < DW_ROWS * N; i += DW_NTHR) {
      const int r = i / N, c = i - r * N;
      gsh[i] = bb + r < b1 ? t.G[(bb + r) * t.ldg + t.g0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < DW_ROWS; ++r) acc = fmaf(as[r * M + om], gsh[r * N + on], acc);
    __syncthreads();
  }
  if (own) part[(int64_t)blockIdx.y * wtot + t.off + om * t.ldo + on] = acc;
}

// launches it for the `mats` matrices of f, the largest of them `big` = M N outputs, into part [mb_small_split(B)][wtot]
template <class Family>
static int small_dw_launch(const Family& f, int mats, int big, int wtot, int64_t B, float* part, hipStream_t st) {
  const int S = mb_small_split(B), maxblk = (big + DW_NTHR - 1) / DW_NTHR;
  const int64_t per = ceil_div64(ceil_div64(B, S), DW_ROWS) * DW_ROWS;
  hipLaunchKernelGGL(small_dw_kernel<Family>, dim3(mats * maxblk, S), dim3(DW_NTHR), 0, st, f, B, maxblk, per, wtot,
                     part);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// host: workspace carving and the split-K weight-gradient GEMM
// ------------------------------------------------------------------------------------------------------------------
// consecutive regions of a float workspace, each rounded up to 4 floats: take() returns the region's offset
struct WsCarve {
  size_t at = 0;
  size_t take(size_t floats) {
    const size_t p = at;
    at += (floats + 3) & ~(size_t)3;
    return p;
  }
};

// dW [M, N] = A^T G with A [B, M] and G [B, N]: transA, K = B, split over the batch (slices added in order) through the
// partials gws, which hold mb_dw_gemm_floats(B, M, N) floats
static inline size_t mb_dw_gemm_floats(int64_t B, int M, int N) { return (size_t)mb_split(B, M, N) * M * N; }
static inline int mb_dw_gemm(int M, int N, int64_t B, const float* A, const float* G, float* dW, float* gws,
                             void* stream) {
  return rec_gemm_f32(1, 0, M, N, B, A, M, G, N, dW, N, REC_EPI_NONE, nullptr, nullptr, 0, nullptr, 0,
                      mb_split(B, M, N), gws, nullptr, stream);
}

}  // namespace
