// The SimHash projection that csrc/eta.hip and csrc/sdim.hip share: one copy, so that both compute a step's projections
// with the same operations in the same order.  The product is rounded before the sum: clang fixes the contraction state
// where a template is DEFINED, not where it is instantiated, so the pragma stands here, ahead of the definitions (and
// holds for the rest of the file that includes this one).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

// the projection is staged in LDS as [D][MC], MC = 16 or 32 columns, the columns past the hash bits zero
__host__ __device__ inline int et_mc(int m) { return m <= 16 ? 16 : 32; }

// acc_j += x Hm[d, j] for the MC columns of row d (hs: that row in LDS, the same address in every lane)
template <int MC>
__device__ __forceinline__ void et_row(float (&acc)[MC], float x, const float* hs) {
#pragma unroll
  for (int j = 0; j < MC; ++j) acc[j] = acc[j] + x * hs[j];
}

// acc_j += sum_d k_d Hs[d, j] of the step whose C ids start at idp, k = concat_c embed[idp[c]], d in order; the caller
// zeroes acc.  CH floats of a row are in flight: 16 (four 16-byte loads), 4 (one) or 1 (a scalar load); the three run the
// same operations in the same order.  An id outside [0, V) reads as a zero row and sets `bad`.
template <int MC, int CH>
__device__ __forceinline__ void et_project(float (&acc)[MC], bool& bad, const float* __restrict__ embed, int64_t ld,
                                           int64_t V, int E, int C, const int64_t* __restrict__ idp, const float* Hs) {
  for (int c = 0; c < C; ++c) {
    const int64_t id = idp[c];
    const bool ok = (uint64_t)id < (uint64_t)V;
    bad |= !ok;
    const float* row = embed + (ok ? id : 0) * ld;
    const float* hs = Hs + c * E * MC;
    for (int e = 0; e < E; e += CH) {
      if constexpr (CH == 1) {
        et_row<MC>(acc, ok ? row[e] : 0.f, hs + e * MC);
      } else {
        float4 x[CH / 4];
#pragma unroll
        for (int u = 0; u < CH / 4; ++u) x[u] = *reinterpret_cast<const float4*>(row + e + 4 * u);
#pragma unroll
        for (int u = 0; u < CH / 4; ++u) {
          et_row<MC>(acc, ok ? x[u].x : 0.f, hs + (e + 4 * u) * MC);
          et_row<MC>(acc, ok ? x[u].y : 0.f, hs + (e + 4 * u + 1) * MC);
          et_row<MC>(acc, ok ? x[u].z : 0.f, hs + (e + 4 * u + 2) * MC);
          et_row<MC>(acc, ok ? x[u].w : 0.f, hs + (e + 4 * u + 3) * MC);
        }
      }
    }
  }
}
