// What ccpm.hip and fgcnn.hip both mean by a field-conv stack: ids X[b, 0..F-1] -> x_0[h, e, 0] = table[X[b,h]][e], then
// L layers of a (kw_j, 1) convolution along the field axis with C_j channels, each followed by a pooling over h that
// leaves H_j rows.  The weights are one flat array K_1 | b_1 | K_2 | b_2 | ... (K_j [kw_j, 1, C_{j-1}, C_j]), and nothing
// mixes values across e, so the unit of work is the COLUMN (b, e) with the states x_0 | x_1 | ... | x_L.
// Shared here: the limits, the shape with its weight and state offsets, the argument checks, the column geometry and the
// sizes of the launch.  Not shared: the pooling rule (each file checks its own and names H_j), the conv loops and the
// backward walks (fgcnn.hip says why).
// FieldConvShape is the kernels' first argument as it stands, and its field order is the kernel-argument layout
// fgcnn.hip's kernels have always had.  Do not reorder it or move PW[] / span out: where the forward's conv loop starts
// depends on it, and 4 bytes cost 9 to 15 % (profiles/r07_field_conv_split_shape_bench.jsonl).
#pragma once
#include <limits.h>
#include "common.h"

constexpr int FC_MAXL = REC_FIELD_CONV_MAX_L, FC_MAXF = REC_FIELD_CONV_MAX_F, FC_MAXE = REC_FIELD_CONV_MAX_E;
constexpr int FC_MAXC = REC_FIELD_CONV_MAX_C, FC_MAXKW = REC_FIELD_CONV_MAX_KW;
constexpr int FC_MAXG_BWD = REC_FIELD_CONV_BWD_GRID;   // workgroups (= workspace slots) of a backward
constexpr size_t FC_LDS_SOFT = 64 * 1024;        // what a workgroup aims for
constexpr size_t FC_LDS_MAX = REC_LDS_CU_BYTES;

struct FieldConvShape {
  int64_t B, V, ld, ncol;                        // ncol = B E columns
  int F, E, L, NW;                               // NW: all weights, K_1 | b_1 | K_2 | b_2 | ...
  int C[FC_MAXL + 1], H[FC_MAXL + 1];            // channels and height of state j (C[0] = 1, H[0] = F)
  int KW[FC_MAXL];
  int PW[FC_MAXL];                               // pooling width: set and read by fgcnn.hip only, 0 in ccpm.hip (k_j is H[j])
  int woff[FC_MAXL], boff[FC_MAXL];
  int soff[FC_MAXL + 2];                         // state j starts at soff[j] (floats per column); soff[L+1] = all states
  int span;                                      // set by the file: ccpm.hip the largest state, fgcnn.hip the column stride
};

__host__ __device__ inline int fc_r4(int n) { return (n + 3) & ~3; }

// column index -> (b, e); columns past the last one are not valid
struct FcCol {
  int64_t b;
  int e;
  bool valid;
};
__device__ __forceinline__ FcCol fc_col(const FieldConvShape& s, int64_t col) {
  FcCol k;
  k.valid = col < s.ncol;
  k.b = col / s.E;
  k.e = (int)(col - k.b * s.E);
  return k;
}

// The checks that come before the layers, and the stack without layers.  `pool` is the pooling argument of every layer
// (k_j or pw_j) and pool_min its smallest value that is still an argument.  0, REC_E_ARG or REC_E_UNSUPPORTED
static inline int fc_begin(FieldConvShape* s, int64_t B, int F, int E, int L, const int* filters, const int* kernel_width,
                           const int* pool, int pool_min, int64_t V, int64_t ld) {
  if (B < 0 || F < 0 || E < 0 || L < 0 || V <= 0 || ld < E || !filters || !kernel_width || !pool) return REC_E_ARG;
  for (int j = 0; j < L && j < FC_MAXL; ++j)
    if (filters[j] < 0 || kernel_width[j] < 0 || pool[j] < pool_min) return REC_E_ARG;
  if (F < 1 || F > FC_MAXF || E < 1 || E > FC_MAXE || L < 1 || L > FC_MAXL) return REC_E_UNSUPPORTED;
  if (B > 0x7fffffffLL || V >= ((int64_t)1 << 31)) return REC_E_UNSUPPORTED;
  *s = FieldConvShape{B, V, ld, B * E, F, E, L};
  s->C[0] = 1;
  s->H[0] = F;
  s->soff[1] = F;
  return REC_OK;
}

// Appends layer j (in order, after the caller's own pooling check): c channels, kernel width kw, Hout rows left by its
// pooling.  0 or REC_E_UNSUPPORTED
static inline int fc_layer(FieldConvShape* s, int j, int c, int kw, int Hout) {
  if (c < 1 || c > FC_MAXC || kw < 1 || kw > FC_MAXKW) return REC_E_UNSUPPORTED;
  s->C[j + 1] = c;
  s->H[j + 1] = Hout;
  s->KW[j] = kw;
  s->woff[j] = s->NW;
  s->boff[j] = s->woff[j] + kw * s->C[j] * c;
  s->NW = s->boff[j] + c;
  s->soff[j + 2] = s->soff[j + 1] + Hout * c;
  return REC_OK;
}

// workgroups for tiles of `per` columns, at most cap and at least one
static inline int fc_grid(const FieldConvShape& s, int per, int64_t cap = INT_MAX) {
  const int64_t ntiles = (s.ncol + per - 1) / per;
  return (int)(ntiles < 1 ? 1 : ntiles < cap ? ntiles : cap);
}

// the backward's workspace: a slot of NW floats per workgroup
static inline size_t fc_ws_bytes(const FieldConvShape& s, int grid) {
  return rec_align_up((size_t)grid * s.NW * sizeof(float), 256);
}
