// The 32-example tile of the MFMA block kernels (masknet.hip, contextnet.hip): a workgroup of 4 waves owns 32 examples,
// the A operand of v_mfma_f32_32x32x2_f32 is the tile, k-major in LDS ([k][33]: reads and writes of a 32-lane half fall
// on 32 different banks), the B operand is read from the weight in global memory with clamped, masked reads; and the
// split-K choice of the weight-gradient GEMMs that follow such a kernel.  Include it after the file's `#pragma clang fp
// contract(off)`.
#pragma once
#include "common.h"

namespace {

constexpr int MB_T = 32;          // examples of a tile
constexpr int MB_LD = 33;         // row stride of a k-major LDS operand [k][32 examples]
constexpr int MB_HC = 128;        // hidden columns of a chunk: one 32-column block per wave
constexpr int MB_NJ = 4;          // 32-column blocks of an accumulator row per wave: block w, w + 4, ... (512 columns)
typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline int mb_even(int n) { return (n + 1) & ~1; }

// row of accumulator register r in a 32x32 MFMA tile; the column is lane & 31
__device__ __forceinline__ int mb_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ void mb_zero(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// acc[j] += As . Bm for the column blocks nb = wave + 4 j of Bm [K, N].  As: LDS [>= even(K)][MB_LD], zero beyond K.
// Bm(k, n) = TRANS ? W[n * ldw + k0 + k] : W[(k0 + k) * ldw + n]: reads are clamped into the matrix and masked.
template <bool TRANS>
__device__ __forceinline__ void mb_mma(f32x16 (&acc)[MB_NJ], const float* As, int K, const float* __restrict__ W,
                                       int64_t ldw, int k0, int N, int wave, int lo, int hi) {
  constexpr int U = 4;                                         // k steps whose operands are requested together
  int nc[MB_NJ];
  bool nok[MB_NJ];
#pragma unroll
  for (int j = 0; j < MB_NJ; ++j) {
    const int n = (wave + 4 * j) * 32 + lo;
    nok[j] = n < N;
    nc[j] = nok[j] ? n : N - 1;
  }
  const int Ke = mb_even(K);
  for (int k = 0; k < Ke; k += 2 * U) {
    float a[U], w[U][MB_NJ];
#pragma unroll
    for (int s = 0; s < U; ++s) {
      const int kk = k + 2 * s + hi;
      const bool kok = kk < K;
      const int kc = k0 + (kok ? kk : K - 1);
      const float av = As[(kk < Ke ? kk : Ke - 1) * MB_LD + lo];
      a[s] = kk < Ke ? av : 0.f;
#pragma unroll
      for (int j = 0; j < MB_NJ; ++j) {
        w[s][j] = 0.f;
        if ((wave + 4 * j) * 32 < N) {                         // uniform over the wave
          const float t = TRANS ? W[(int64_t)nc[j] * ldw + kc] : W[(int64_t)kc * ldw + nc[j]];
          w[s][j] = (kok && nok[j]) ? t : 0.f;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < U; ++s)
#pragma unroll
      for (int j = 0; j < MB_NJ; ++j)
        if ((wave + 4 * j) * 32 < N) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], w[s][j], acc[j], 0, 0, 0);
  }
}

// the same for ONE block: columns n0 + lo of Bm
template <bool TRANS>
__device__ __forceinline__ void mb_mma1(f32x16& acc, const float* As, int K, const float* __restrict__ W, int64_t ldw,
                                        int k0, int N, int n0, int lo, int hi) {
  constexpr int U = 8;
  const int n = n0 + lo;
  const bool nok = n < N;
  const int nc = nok ? n : N - 1;
  const int Ke = mb_even(K);
  for (int k = 0; k < Ke; k += 2 * U) {
    float a[U], w[U];
#pragma unroll
    for (int s = 0; s < U; ++s) {
      const int kk = k + 2 * s + hi;
      const bool kok = kk < K;
      const int kc = k0 + (kok ? kk : K - 1);
      const float av = As[(kk < Ke ? kk : Ke - 1) * MB_LD + lo];
      a[s] = kk < Ke ? av : 0.f;
      const float t = TRANS ? W[(int64_t)nc * ldw + kc] : W[(int64_t)kc * ldw + nc];
      w[s] = (kok && nok) ? t : 0.f;
    }
#pragma unroll
    for (int s = 0; s < U; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], w[s], acc, 0, 0, 0);
  }
}

// slices of the weight-gradient product [M, N] = A^T B over K = batch: enough to fill the chip, at most 16, so the
// partials stay a small multiple of the weight whatever the batch
static int mb_split(int64_t K, int M, int N) {
  const int t = (M > 64 && N > 64) ? 128 : 64;
  const int64_t tiles = (int64_t)((M + t - 1) / t) * ((N + t - 1) / t);
  int64_t s = 512 / tiles;
  if (s > K / 256) s = K / 256;
  if (s > 16) s = 16;
  return s < 1 ? 1 : (int)s;
}

}  // namespace
