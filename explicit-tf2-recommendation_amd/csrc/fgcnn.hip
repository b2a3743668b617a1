// Feature Generation by CNN (FGCNNBaseLayer / FGCNNLayer, 3.DCN/CustomLayers.py:728-822) on gfx950, fused with the
// embedding lookup.  Per example, ids X[b, 0..F-1], x_0[h, e, 0] = table[X[b,h]][e] (NHWC with H = fields, W = E,
// C = 1), and for the layers j = 1..L (C_j = filters, kw_j = kernel_width, pw_j = pooling_width, H_0 = F):
//   y[h, e, co] = tanh(b[co] + sum_t sum_ci K[t, 0, ci, co] x_{j-1}[h - pad + t, e, ci])      pad = (kw - 1) / 2, zeros
//                 outside [0, H_{j-1}): TF's SAME padding, the extra row at the END
//   x_j[r, e, co] = max over q < pw_j of y[r pw_j + q, e, co]                                  H_j = H_{j-1} / pw_j; the
//                 trailing H_{j-1} mod pw_j rows are dropped; on equal values the LOWER h takes the gradient
//   p_j[b, (r E + e) C_j + c] = x_j[r, e, c]                                                   (Flatten of [H_j, E, C_j])
// Every p_j leaves the kernel (a Dense layer recombines each one on the GEMM kernels), and so do the gathered rows,
// which the MLP consumes beside them.
// The kernel is (kw, 1) and the pooling runs over h only, so nothing mixes values across e: each (example, e) COLUMN is
// an independent problem.  tanh is monotone, so the pooling runs on the PRE-activations and one tanh is taken per pooled
// value; selection and tie rule are made on the pre-activation in both directions.
// A column is worked on by G adjacent lanes (G a power of two, 16 unless the state needs more): a workgroup of 256
// threads holds 256 / G columns, the state of a column is one contiguous LDS array (x_0 | x_1 | ... | x_L), and the
// weights sit in LDS once per workgroup.  Both kernels are persistent over tiles of 256 / G columns.
//   emb_fgcnn_fwd_kernel  gathers the rows of a tile, then per layer lane g of a column computes the pooled outputs
//                         (r, co) = g, g + G, ... : adjacent lanes read adjacent weights and broadcast the inputs.
//   emb_fgcnn_bwd_kernel  recomputes the stack from the saved rows with the SAME routine, keeping the selected row of
//                         every pooled value (one byte each), then walks back with g(x_j) = dp_j + (what layer j + 1
//                         sends down): dpre = g (1 - x_j^2) at the selected rows; dx is a GATHER, lane g of a column
//                         owns the inputs (hin, ci) = g, g + G, ... and sums over (t, co) in that order; dK and db are
//                         owned per WEIGHT, thread w of the workgroup adds the columns of the tile in order into its own
//                         LDS accumulator, which lives across the workgroup's tiles and ends in the workgroup's slot;
//   and rec_slot_sum adds the slots in its wave order.  No float atomics and no value with two writers: bit-identical
// gradients run to run; no host synchronisation: both directions can be captured in a graph.
// Every position of a column is computed by one fma order (contraction is off in this file; a tap outside the column is
// skipped, for every position alike), so equal inputs give bit-equal pre-activations and the tie rule is observable;
// tanhf is the accurate one.  The conv loop is not shared with ccpm.hip: there a thread walks a column with a stride of
// blockDim floats and wave-uniform weights from global memory, here a lane group walks a contiguous column with the
// weights in LDS and pools inside the loop; one routine for both would change what either compiles to.
#include <math.h>
#include "field_conv.h"

#pragma clang fp contract(off)

namespace {

constexpr int FG_MAXPW = REC_FGCNN_MAX_PW;
constexpr int FG_NTHR = 256, FG_MING = 16;
constexpr int FG_MAXG_FWD = 2048;                // workgroups of the forward

// In the FieldConvShape of this file PW[j-1] = pw_j, H[j] = H[j-1] / pw_j, and span = S, the stride of a column:
// soff[L+1] rounded up to an odd multiple of 4.

struct FgPtrs {
  float* p[FC_MAXL];
};

struct FgCfg {
  int G[2], grid[2];                             // forward, backward; G == 0: the state does not fit
  size_t lds[2];
};

// floats of LDS of a workgroup.  forward: weights | cols x states; backward: weights | their gradients | cols x
// (states | gradients | selected rows, one byte each)
__host__ __device__ inline size_t fg_lds_floats(const FieldConvShape& s, int G, int bwd) {
  const size_t cols = FG_NTHR / G;
  return bwd ? 2 * (size_t)fc_r4(s.NW) + cols * (2 * (size_t)s.span + s.span / 4)
             : (size_t)fc_r4(s.NW) + cols * s.span;
}

// One conv + max-pool + tanh layer of one column, by the G lanes of its group: lane g computes the pooled values
// i = (r, co) = g, g + G, ...  W / bias and xin [Hin, Cin] / xout [Hout, Cout] are LDS arrays; sel, when given, receives
// the selected row of every pooled value.  The forward and the backward's recomputation both call this, so both select
// the same rows.  `>` keeps the lower row on equal pre-activations.
__device__ __forceinline__ void fg_conv_pool(const float* W, const float* bias, int Hin, int Cin, int Cout, int kw, int pw,
                                             int Hout, const float* xin, float* xout, unsigned char* sel, int g, int G) {
  const int pad = (kw - 1) >> 1, n = Hout * Cout;
  for (int i = g; i < n; i += G) {
    const int r = i / Cout, co = i - r * Cout;
    const float bc = bias[co];
    float best = 0.f;
    int at = 0;
    for (int q = 0; q < pw; ++q) {
      const int h = r * pw + q;
      float pre = bc;
      for (int t = 0; t < kw; ++t) {
        const int hin = h - pad + t;
        if (hin < 0 || hin >= Hin) continue;
        const float* w = W + (t * Cin) * Cout + co;
        const float* x = xin + hin * Cin;
        for (int ci = 0; ci < Cin; ++ci) pre = fmaf(w[ci * Cout], x[ci], pre);
      }
      if (q == 0 || pre > best) {
        best = pre;
        at = h;
      }
    }
    xout[i] = tanhf(best);
    if (sel) sel[i] = (unsigned char)at;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// forward: persistent over tiles of 256 / G columns
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FG_NTHR) void emb_fgcnn_fwd_kernel(FieldConvShape s, int G, const float* __restrict__ table,
                                                                const int64_t* __restrict__ X,
                                                                const float* __restrict__ par,
                                                                float* __restrict__ rows_out, FgPtrs pooled, int* oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, cols = FG_NTHR / G, L = s.L, S = s.span;
  float* wl = lds;                                             // [NW]
  float* xs = wl + fc_r4(s.NW);                                // [cols][S]
  for (int t = tid; t < s.NW; t += FG_NTHR) wl[t] = par[t];
  const int myc = tid / G, g = tid - myc * G;
  float* mx = xs + myc * S;
  bool bad = false;

  const int64_t ntiles = (s.ncol + cols - 1) / cols;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    __syncthreads();                                           // the weights; the previous tile's readers
    for (int i = tid; i < s.F * cols; i += FG_NTHR) {          // gather: [h][c], the lanes along e
      const int h = i / cols, c = i - h * cols;
      const FcCol k = fc_col(s, tl * cols + c);                // column slot c of tile tl
      float v = 0.f;
      if (k.valid) {
        const int64_t id = X[k.b * s.F + h];
        if ((uint64_t)id < (uint64_t)s.V)
          v = table[id * s.ld + k.e];
        else
          bad = true;
        rows_out[(k.b * s.F + h) * s.E + k.e] = v;
      }
      xs[c * S + h] = v;
    }
    __syncthreads();
    for (int j = 0; j < L; ++j) {
      fg_conv_pool(wl + s.woff[j], wl + s.boff[j], s.H[j], s.C[j], s.C[j + 1], s.KW[j], s.PW[j], s.H[j + 1],
                   mx + s.soff[j], mx + s.soff[j + 1], nullptr, g, G);
      __syncthreads();
    }
    for (int j = 1; j <= L; ++j) {                             // p_j: [r][c][ch], runs of cols C_j floats
      const int Cj = s.C[j], per = cols * Cj, n = s.H[j] * per;
      float* __restrict__ out = pooled.p[j - 1];
      for (int i = tid; i < n; i += FG_NTHR) {
        const int r = i / per, rem = i - r * per, c = rem / Cj, ch = rem - c * Cj;
        const FcCol k = fc_col(s, tl * cols + c);
        if (k.valid) out[k.b * ((int64_t)s.H[j] * s.E * Cj) + (r * s.E + k.e) * Cj + ch] = xs[c * S + s.soff[j] + r * Cj + ch];
      }
    }
  }
  if (bad && oob) *oob = 1;
}

// ------------------------------------------------------------------------------------------------------------------
// backward: persistent over tiles of 256 / G columns; slot of workgroup w [NW] in the layout of the weights
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FG_NTHR) void emb_fgcnn_bwd_kernel(FieldConvShape s, int G, const float* __restrict__ par,
                                                                const float* __restrict__ rows, FgPtrs dpooled,
                                                                const float* __restrict__ ddirect,
                                                                float* __restrict__ vals, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, cols = FG_NTHR / G, L = s.L, S = s.span;
  float* wl = lds;                                             // [NW]
  float* wacc = wl + fc_r4(s.NW);                              // [NW]: element w has ONE writer, thread w mod 256
  float* xs = wacc + fc_r4(s.NW);                              // [cols][S] states
  float* gs = xs + cols * S;                                   // [cols][S] their gradients
  unsigned char* sl = reinterpret_cast<unsigned char*>(gs + cols * S);   // [cols][S] selected rows
  for (int t = tid; t < s.NW; t += FG_NTHR) {
    wl[t] = par[t];
    wacc[t] = 0.f;
  }
  const int myc = tid / G, g = tid - myc * G;
  float* mx = xs + myc * S;
  float* mg = gs + myc * S;
  unsigned char* ms = sl + myc * S;

  const int64_t ntiles = (s.ncol + cols - 1) / cols;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    __syncthreads();
    for (int i = tid; i < s.F * cols; i += FG_NTHR) {
      const int h = i / cols, c = i - h * cols;
      const FcCol k = fc_col(s, tl * cols + c);
      xs[c * S + h] = k.valid ? rows[(k.b * s.F + h) * s.E + k.e] : 0.f;
    }
    for (int j = 1; j <= L; ++j) {                             // g(x_j) starts as dp_j
      const int Cj = s.C[j], per = cols * Cj, n = s.H[j] * per;
      const float* __restrict__ d = dpooled.p[j - 1];
      for (int i = tid; i < n; i += FG_NTHR) {
        const int r = i / per, rem = i - r * per, c = rem / Cj, ch = rem - c * Cj;
        const FcCol k = fc_col(s, tl * cols + c);
        gs[c * S + s.soff[j] + r * Cj + ch] =
            k.valid ? d[k.b * ((int64_t)s.H[j] * s.E * Cj) + (r * s.E + k.e) * Cj + ch] : 0.f;
      }
    }
    __syncthreads();
    for (int j = 0; j < L; ++j) {
      fg_conv_pool(wl + s.woff[j], wl + s.boff[j], s.H[j], s.C[j], s.C[j + 1], s.KW[j], s.PW[j], s.H[j + 1],
                   mx + s.soff[j], mx + s.soff[j + 1], ms + s.soff[j + 1], g, G);
      __syncthreads();
    }
    for (int j = L; j >= 1; --j) {
      const int Hin = s.H[j - 1], Cin = s.C[j - 1], Cout = s.C[j], kw = s.KW[j - 1], pw = s.PW[j - 1], Ho = s.H[j];
      const int pad = (kw - 1) >> 1, so = s.soff[j], si = s.soff[j - 1];
      const float* W = wl + s.woff[j - 1];
      for (int i = g; i < Ho * Cout; i += G) {                 // through the tanh, in place: dpre at the selected rows
        const float yv = mx[so + i];
        mg[so + i] = mg[so + i] * fmaf(-yv, yv, 1.f);
      }
      __syncthreads();
      for (int i = g; i < Hin * Cin; i += G) {                 // dx: input (hin, ci) gathers over (t, co)
        const int hin = i / Cin, ci = i - hin * Cin;
        float acc = 0.f;
        for (int t = 0; t < kw; ++t) {
          const int h = hin + pad - t;
          if (h < 0 || h >= Ho * pw) continue;                 // outside the column, or a dropped trailing row
          const int r = h / pw;
          const float* w = W + (t * Cin + ci) * Cout;
          for (int co = 0; co < Cout; ++co)
            if ((int)ms[so + r * Cout + co] == h) acc = fmaf(mg[so + r * Cout + co], w[co], acc);
        }
        if (j > 1)
          mg[si + i] += acc;                                   // dp_{j-1} + what this layer sends down
        else
          mg[i] = acc;
      }
      const int nk = kw * Cin * Cout;
      for (int w = tid; w < nk; w += FG_NTHR) {                // dK: thread owns weight (t, ci, co)
        const int t = w / (Cin * Cout), rem = w - t * (Cin * Cout), ci = rem / Cout, co = rem - ci * Cout;
        float acc = wacc[s.woff[j - 1] + w];
        for (int c = 0; c < cols; ++c) {
          const float* cg = gs + c * S + so + co;
          const float* cx = xs + c * S + si + ci;
          const unsigned char* cs = sl + c * S + so + co;
          for (int r = 0; r < Ho; ++r) {
            const int hin = (int)cs[r * Cout] - pad + t;
            if (hin >= 0 && hin < Hin) acc = fmaf(cg[r * Cout], cx[hin * Cin], acc);
          }
        }
        wacc[s.woff[j - 1] + w] = acc;
      }
      for (int co = tid; co < Cout; co += FG_NTHR) {           // db
        float acc = wacc[s.boff[j - 1] + co];
        for (int c = 0; c < cols; ++c) {
          const float* cg = gs + c * S + so + co;
          for (int r = 0; r < Ho; ++r) acc += cg[r * Cout];
        }
        wacc[s.boff[j - 1] + co] = acc;
      }
      __syncthreads();
    }
    for (int i = tid; i < s.F * cols; i += FG_NTHR) {
      const int h = i / cols, c = i - h * cols;
      const FcCol k = fc_col(s, tl * cols + c);
      if (k.valid) {
        const int64_t at = (k.b * s.F + h) * s.E + k.e;
        vals[at] = ddirect ? ddirect[at] + gs[c * S + h] : gs[c * S + h];
      }
    }
  }
  __syncthreads();
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * s.NW;
  for (int t = tid; t < s.NW; t += FG_NTHR) slot[t] = wacc[t];
}

// 0 ok (B == 0 included), REC_E_ARG, REC_E_UNSUPPORTED
static int fg_shape(int64_t B, int F, int E, int L, const int* filters, const int* kernel_width, const int* pooling_width,
                    int64_t V, int64_t ld, FieldConvShape* s) {
  if (int rc = fc_begin(s, B, F, E, L, filters, kernel_width, pooling_width, 1, V, ld)) return rc;
  for (int j = 0; j < L; ++j) {
    const int pw = pooling_width[j];
    if (s->H[j] / pw < 1) return REC_E_ARG;                    // a pooling wider than what it pools: nothing is left
    if (pw > FG_MAXPW) return REC_E_UNSUPPORTED;
    if (int rc = fc_layer(s, j, filters[j], kernel_width[j], s->H[j] / pw)) return rc;
    s->PW[j] = pw;
  }
  s->span = fc_r4(s->soff[L + 1]);
  if (!(s->span & 4)) s->span += 4;                            // an odd number of 16-byte units: columns spread over banks
  return REC_OK;
}

// G[d] == 0: the state of one column does not fit the LDS of a CU
static FgCfg fg_cfg(const FieldConvShape& s) {
  FgCfg k{};
  for (int d = 0; d < 2; ++d) {
    int G = FG_MING;
    size_t bytes;
    for (;;) {
      bytes = fg_lds_floats(s, G, d) * 4;
      if (bytes <= FC_LDS_SOFT || G == 64) break;
      G <<= 1;
    }
    if (bytes > FC_LDS_MAX) continue;
    k.G[d] = G;
    k.lds[d] = bytes;
    k.grid[d] = fc_grid(s, FG_NTHR / G, d ? FC_MAXG_BWD : FG_MAXG_FWD);
  }
  return k;
}

}  // namespace

extern "C" size_t rec_fgcnn_workspace_bytes(int64_t B, int F, int E, int L, const int* filters, const int* kernel_width,
                                            const int* pooling_width) {
  FieldConvShape s;
  if (fg_shape(B, F, E, L, filters, kernel_width, pooling_width, 1, E, &s) != REC_OK) return 0;
  const FgCfg k = fg_cfg(s);
  if (!k.G[0] || !k.G[1]) return 0;
  return fc_ws_bytes(s, k.grid[1]);
}

extern "C" int rec_emb_fgcnn_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F,
                                     int L, const int* filters, const int* kernel_width, const int* pooling_width,
                                     const float* params, float* rows, float* const* pooled, int* oob_flag,
                                     void* stream) {
  FieldConvShape s;
  const int rc = fg_shape(B, F, E, L, filters, kernel_width, pooling_width, V, ld, &s);
  if (rc != REC_OK) return rc;
  const FgCfg k = fg_cfg(s);
  if (!k.G[0] || !k.G[1]) return REC_E_UNSUPPORTED;
  if (B == 0) return REC_OK;
  if (!table || !X || !params || !rows || !pooled) return REC_E_ARG;
  FgPtrs pp{};
  for (int j = 0; j < L; ++j) {
    if (!pooled[j]) return REC_E_ARG;
    pp.p[j] = pooled[j];
  }
  if (hipError_t e = rec_allow_lds<emb_fgcnn_fwd_kernel>(FC_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(emb_fgcnn_fwd_kernel, dim3(k.grid[0]), dim3(FG_NTHR), k.lds[0], as_stream(stream), s, k.G[0], table,
                     X, params, rows, pp, oob_flag);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_emb_fgcnn_bwd_f32(int E, int64_t B, int F, int L, const int* filters, const int* kernel_width,
                                     const int* pooling_width, const float* params, const float* rows,
                                     const float* const* dpooled, const float* drows_direct, float* vals, float* dparams,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  FieldConvShape s;
  const int rc = fg_shape(B, F, E, L, filters, kernel_width, pooling_width, 1, E, &s);
  if (rc != REC_OK) return rc;
  const FgCfg k = fg_cfg(s);
  if (!k.G[0] || !k.G[1]) return REC_E_UNSUPPORTED;
  if (B == 0) return REC_OK;
  if (!params || !rows || !dpooled || !vals || !dparams || !workspace) return REC_E_ARG;
  FgPtrs pp{};
  for (int j = 0; j < L; ++j) {
    if (!dpooled[j]) return REC_E_ARG;
    pp.p[j] = const_cast<float*>(dpooled[j]);
  }
  if (workspace_bytes < fc_ws_bytes(s, k.grid[1])) return REC_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  float* slots = static_cast<float*>(workspace);
  if (hipError_t e = rec_allow_lds<emb_fgcnn_bwd_kernel>(FC_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(emb_fgcnn_bwd_kernel, dim3(k.grid[1]), dim3(FG_NTHR), k.lds[1], st, s, k.G[1], params, rows, pp,
                     drows_direct, vals, slots);
  REC_LAUNCH_CHECK();
  return rec_slot_sum(REC_SLOTS_WAVE, s.NW, k.grid[1], slots, {{dparams}, {s.NW}}, st);
}
