// Convolutional Click Prediction Model (KMaxPool / CCPMBaseLayer / CCPMLayer, 3.DCN/CustomLayers.py:621-725) on gfx950,
// fused with the embedding lookup.  Per example, ids X[b, 0..F-1], x_0[h, e, 0] = table[X[b,h]][e] (NHWC with H = fields,
// W = E, C = 1), and for the layers j = 1..L (C_j = filters, kw_j = kernel_width, k_j = pool_k, H_0 = F, H_j = k_j):
//   y[h, e, co] = tanh(b[co] + sum_t sum_ci K[t, 0, ci, co] x_{j-1}[h - pad + t, e, ci])      pad = (kw - 1) / 2, zeros
//                 outside [0, H_{j-1}): TF's SAME padding, the extra row at the END
//   x_j[r, e, co] = the r-th largest of y[., e, co] over h (values in descending order; on equal values the lower h first)
//   out[b, (r E + e) C_L + c] = x_L[r, e, c]                                                   (Flatten of [k_L, E, C_L])
// The kernel is (kw, 1) and the pooling runs over h only, so nothing mixes values across e: each (example, e) COLUMN is
// an independent problem on at most F values, and each direction is one kernel in which a thread owns a column:
//   emb_ccpm_fwd_kernel  thread = column (b, e), columns in order over the lanes: the 16 lanes of an example read one
//                        64-byte row together at E = 16.  The column state lives in LDS as [index][thread] (stride
//                        blockDim: no bank conflicts, nothing is shared between threads).  Per layer and output channel
//                        the unpooled column y[0..H) exists once, in a scratch of F floats; k selection passes move its
//                        largest values into the next state.  Only out (and, when asked, the gathered rows) leave.
//   emb_ccpm_bwd_kernel  persistent grid.  Recomputes the forward of its columns from the rows (gathered again, or the
//                        saved ones) with the SAME routine, keeping every state and the selected positions (one byte
//                        each), then walks back: dpre = dy (1 - y^2) at the selected positions only, dx through the
//                        taps into the previous state's gradient, and per weight the column's sum, added over the wave
//                        by the xor butterfly and kept per wave in LDS over the workgroup's tiles.  At the end the waves
//                        are added in order into the workgroup's slot;
//   and rec_slot_sum adds the slots in its wave order.  No float atomics: bit-identical gradients run to run; no host
// synchronisation: both directions can be captured in a graph.
// Every position of a column is computed by one fma order (contraction is off in this file; a tap outside the column is
// skipped, for every position alike), so equal inputs give bit-equal outputs and the tie rule is observable; tanhf is
// the accurate one.  The conv weights are read with wave-uniform addresses straight from global memory.
#include <math.h>
#include "field_conv.h"

#pragma clang fp contract(off)

namespace {

// In the FieldConvShape of this file H[j] = k_j, and span is the largest state: the size of each of the forward's two
// ping-pong buffers.

struct CcpmCfg {
  int nthr[2], grid[2];                          // forward, backward
  size_t lds[2];
};

// floats of LDS per column.  forward: two states (ping-pong) | y [F]; backward: every state | its gradient | y [F] |
// the selected positions, one byte each
__host__ __device__ inline int ccpm_col_floats(const FieldConvShape& s, int bwd) {
  const int all = s.soff[s.L + 1];
  return bwd ? 2 * all + s.F + fc_r4(all) / 4 : 2 * s.span + s.F;
}

// One conv + tanh + k-max-pool layer of one column.  xin [Hin, Cin] and xout [k, Cout] are LDS arrays of stride `st`
// floats; y [Hin] is the scratch; sel (stride `st` bytes), when given, receives the selected position of every output.
// The forward and the backward's recomputation both call this, so both select the same positions.
__device__ __forceinline__ void ccpm_conv_pool(const float* __restrict__ Kw, const float* __restrict__ bias, int Hin,
                                               int Cin, int Cout, int kw, int k, int st, const float* xin, float* xout,
                                               float* y, unsigned char* sel) {
  const int pad = (kw - 1) >> 1;
  for (int co = 0; co < Cout; ++co) {
    const float bc = bias[co];
    for (int h = 0; h < Hin; ++h) {
      float pre = bc;
      for (int t = 0; t < kw; ++t) {
        const int hin = h - pad + t;
        if (hin < 0 || hin >= Hin) continue;
        const float* w = Kw + (t * Cin) * Cout + co;
        const float* x = xin + (hin * Cin) * st;
        for (int ci = 0; ci < Cin; ++ci) pre = fmaf(w[ci * Cout], x[ci * st], pre);
      }
      y[h * st] = tanhf(pre);
    }
    // the k largest in descending order; `>` keeps the lower position on equal values.  tanh is within [-1, 1]: -2
    // marks a taken position, -3 starts below everything
    for (int r = 0; r < k; ++r) {
      float best = -3.f;
      int at = 0;
      for (int h = 0; h < Hin; ++h) {
        const float v = y[h * st];
        if (v > best) {
          best = v;
          at = h;
        }
      }
      y[at * st] = -2.f;
      xout[(r * Cout + co) * st] = best;
      if (sel) sel[(r * Cout + co) * st] = (unsigned char)at;
    }
  }
}

// the rows of column (b, e) -> x [F] (stride st); true when an id was out of range (it reads as a zero row)
__device__ __forceinline__ bool ccpm_load_col(const FieldConvShape& s, const float* __restrict__ table,
                                              const int64_t* __restrict__ X, const float* __restrict__ rows_in, bool valid,
                                              int64_t b, int e, int st, float* x, float* __restrict__ rows_out) {
  bool bad = false;
  for (int h = 0; h < s.F; ++h) {
    float v = 0.f;
    if (valid) {
      if (rows_in) {
        v = rows_in[(b * s.F + h) * s.E + e];
      } else {
        const int64_t id = X[b * s.F + h];
        if ((uint64_t)id < (uint64_t)s.V)
          v = table[id * s.ld + e];
        else
          bad = true;
      }
      if (rows_out) rows_out[(b * s.F + h) * s.E + e] = v;
    }
    x[h * st] = v;
  }
  return bad;
}

// ------------------------------------------------------------------------------------------------------------------
// forward: grid = ceil(B E / blockDim)
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emb_ccpm_fwd_kernel(FieldConvShape s, const float* __restrict__ table,
                                                           const int64_t* __restrict__ X,
                                                           const float* __restrict__ par, float* __restrict__ out,
                                                           float* __restrict__ rows_out, int* oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int st = blockDim.x;
  float* cur = lds + threadIdx.x;
  float* nxt = cur + s.span * st;
  float* y = nxt + s.span * st;
  const int64_t col = (int64_t)blockIdx.x * st + threadIdx.x;
  const auto [b, e, valid] = fc_col(s, col);
  if (ccpm_load_col(s, table, X, nullptr, valid, b, e, st, cur, rows_out) && oob) *oob = 1;
  for (int j = 0; j < s.L; ++j) {
    ccpm_conv_pool(par + s.woff[j], par + s.boff[j], s.H[j], s.C[j], s.C[j + 1], s.KW[j], s.H[j + 1], st, cur, nxt, y,
                   nullptr);
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (!valid) return;
  const int CL = s.C[s.L], kL = s.H[s.L];
  float* o = out + b * ((int64_t)kL * s.E * CL);
  for (int r = 0; r < kL; ++r)
    for (int c = 0; c < CL; ++c) o[(r * s.E + e) * CL + c] = cur[(r * CL + c) * st];
}

// ------------------------------------------------------------------------------------------------------------------
// backward: persistent grid, blockDim a multiple of 64; slot of workgroup g [NW] in the layout of the weights
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emb_ccpm_bwd_kernel(FieldConvShape s, const float* __restrict__ table,
                                                           const int64_t* __restrict__ X,
                                                           const float* __restrict__ par,
                                                           const float* __restrict__ rows_in,
                                                           const float* __restrict__ dout, float* __restrict__ vals,
                                                           float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int st = blockDim.x, L = s.L, all = s.soff[L + 1];
  float* xs = lds + threadIdx.x;                                // states, [all] per column
  float* gs = xs + all * st;                                    // their gradients
  float* y = gs + all * st;
  unsigned char* sel = reinterpret_cast<unsigned char*>(lds + (2 * all + s.F) * st) + threadIdx.x;
  float* wacc = lds + ccpm_col_floats(s, 1) * st;               // [waves][NW]
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = st >> 6;
  for (int t = threadIdx.x; t < nw * s.NW; t += st) wacc[t] = 0.f;
  float* mine = wacc + wv * s.NW;                               // only lane 0 of the wave touches it until the end
  __syncthreads();

  const int64_t ntiles = (s.ncol + st - 1) / st;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t col = tl * st + threadIdx.x;
    const auto [b, e, valid] = fc_col(s, col);
    ccpm_load_col(s, table, X, rows_in, valid, b, e, st, xs, nullptr);
    for (int j = 0; j < L; ++j)
      ccpm_conv_pool(par + s.woff[j], par + s.boff[j], s.H[j], s.C[j], s.C[j + 1], s.KW[j], s.H[j + 1], st,
                     xs + s.soff[j] * st, xs + s.soff[j + 1] * st, y, sel + s.soff[j + 1] * st);
    for (int i = 0; i < s.soff[L]; ++i) gs[i * st] = 0.f;
    {
      const int CL = s.C[L], kL = s.H[L];
      const float* d = dout + b * ((int64_t)kL * s.E * CL);
      float* g = gs + s.soff[L] * st;
      for (int r = 0; r < kL; ++r)
        for (int c = 0; c < CL; ++c) g[(r * CL + c) * st] = valid ? d[(r * s.E + e) * CL + c] : 0.f;
    }
    for (int j = L; j >= 1; --j) {
      const int Hin = s.H[j - 1], Cin = s.C[j - 1], Cout = s.C[j], kw = s.KW[j - 1], k = s.H[j], pad = (kw - 1) >> 1;
      const float* Kw = par + s.woff[j - 1];
      const float* xin = xs + s.soff[j - 1] * st;
      const float* xo = xs + s.soff[j] * st;
      float* g = gs + s.soff[j] * st;
      float* gin = gs + s.soff[j - 1] * st;
      const unsigned char* sl = sel + s.soff[j] * st;
      for (int i = 0; i < k * Cout; ++i) {                      // through the tanh, in place
        const float yv = xo[i * st];
        g[i * st] = g[i * st] * fmaf(-yv, yv, 1.f);
      }
      for (int r = 0; r < k; ++r)                               // dx: to the taps of the selected positions only
        for (int co = 0; co < Cout; ++co) {
          const float d = g[(r * Cout + co) * st];
          const int h0 = (int)sl[(r * Cout + co) * st] - pad;
          for (int t = 0; t < kw; ++t) {
            const int hin = h0 + t;
            if (hin < 0 || hin >= Hin) continue;
            const float* w = Kw + (t * Cin) * Cout + co;
            float* gi = gin + (hin * Cin) * st;
            for (int ci = 0; ci < Cin; ++ci) gi[ci * st] = fmaf(d, w[ci * Cout], gi[ci * st]);
          }
        }
      for (int co = 0; co < Cout; ++co) {                       // db and dK: the column's sum, then the wave's
        float acc = 0.f;
        for (int r = 0; r < k; ++r) acc += g[(r * Cout + co) * st];
        acc = group_sum<64>(acc);
        if (lane == 0) mine[s.boff[j - 1] + co] += acc;
        for (int t = 0; t < kw; ++t)
          for (int ci = 0; ci < Cin; ++ci) {
            acc = 0.f;
            for (int r = 0; r < k; ++r) {
              const int hin = (int)sl[(r * Cout + co) * st] - pad + t;
              if (hin >= 0 && hin < Hin) acc = fmaf(g[(r * Cout + co) * st], xin[(hin * Cin + ci) * st], acc);
            }
            acc = group_sum<64>(acc);
            if (lane == 0) mine[s.woff[j - 1] + (t * Cin + ci) * Cout + co] += acc;
          }
      }
    }
    if (valid)
      for (int h = 0; h < s.F; ++h) vals[(b * s.F + h) * s.E + e] = gs[h * st];
  }
  __syncthreads();
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * s.NW;
  for (int t = threadIdx.x; t < s.NW; t += st) {
    float acc = 0.f;
    for (int w = 0; w < nw; ++w) acc += wacc[w * s.NW + t];
    slot[t] = acc;
  }
}

// 0 ok (B == 0 included), REC_E_ARG, REC_E_UNSUPPORTED
static int ccpm_shape(int64_t B, int F, int E, int L, const int* filters, const int* kernel_width, const int* pool_k,
                      int64_t V, int64_t ld, FieldConvShape* s) {
  if (int rc = fc_begin(s, B, F, E, L, filters, kernel_width, pool_k, 0, V, ld)) return rc;
  s->span = F;
  for (int j = 0; j < L; ++j) {
    const int k = pool_k[j];
    if (k > s->H[j]) return REC_E_ARG;                         // top_k over fewer values than k: the reference raises
    if (k < 1) return REC_E_UNSUPPORTED;
    if (int rc = fc_layer(s, j, filters[j], kernel_width[j], k)) return rc;
    if (k * filters[j] > s->span) s->span = k * filters[j];
  }
  return REC_OK;
}

// nthr[d] == 0: the column state does not fit the LDS of a CU
static CcpmCfg ccpm_cfg(const FieldConvShape& s) {
  CcpmCfg k{};
  for (int d = 0; d < 2; ++d) {
    int nthr = 256;
    size_t bytes;
    for (;;) {
      bytes = ((size_t)ccpm_col_floats(s, d) * nthr + (d ? (size_t)(nthr / 64) * s.NW : 0)) * 4;
      if (bytes <= FC_LDS_SOFT || nthr == 64) break;
      nthr >>= 1;
    }
    if (bytes > FC_LDS_MAX) continue;
    k.nthr[d] = nthr;
    k.lds[d] = bytes;
    k.grid[d] = d ? fc_grid(s, nthr, FC_MAXG_BWD) : fc_grid(s, nthr);
  }
  return k;
}

}  // namespace

extern "C" size_t rec_ccpm_workspace_bytes(int64_t B, int F, int E, int L, const int* filters, const int* kernel_width,
                                           const int* pool_k) {
  FieldConvShape s;
  if (ccpm_shape(B, F, E, L, filters, kernel_width, pool_k, 1, E, &s) != REC_OK) return 0;
  const CcpmCfg k = ccpm_cfg(s);
  if (!k.nthr[0] || !k.nthr[1]) return 0;
  return fc_ws_bytes(s, k.grid[1]);
}

extern "C" int rec_emb_ccpm_fwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F,
                                    int L, const int* filters, const int* kernel_width, const int* pool_k,
                                    const float* params, float* out, float* rows, int* oob_flag, void* stream) {
  FieldConvShape s;
  const int rc = ccpm_shape(B, F, E, L, filters, kernel_width, pool_k, V, ld, &s);
  if (rc != REC_OK) return rc;
  const CcpmCfg k = ccpm_cfg(s);
  if (!k.nthr[0] || !k.nthr[1]) return REC_E_UNSUPPORTED;
  if (B == 0) return REC_OK;
  if (!table || !X || !params || !out) return REC_E_ARG;
  if (hipError_t e = rec_allow_lds<emb_ccpm_fwd_kernel>(FC_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(emb_ccpm_fwd_kernel, dim3(k.grid[0]), dim3(k.nthr[0]), k.lds[0], as_stream(stream), s, table, X,
                     params, out, rows, oob_flag);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_emb_ccpm_bwd_f32(const float* table, int64_t V, int E, int64_t ld, const int64_t* X, int64_t B, int F,
                                    int L, const int* filters, const int* kernel_width, const int* pool_k,
                                    const float* params, const float* rows, const float* dout, float* vals,
                                    float* dparams, void* workspace, size_t workspace_bytes, void* stream) {
  FieldConvShape s;
  const int rc = ccpm_shape(B, F, E, L, filters, kernel_width, pool_k, V, ld, &s);
  if (rc != REC_OK) return rc;
  const CcpmCfg k = ccpm_cfg(s);
  if (!k.nthr[0] || !k.nthr[1]) return REC_E_UNSUPPORTED;
  if (B == 0) return REC_OK;
  if ((!rows && (!table || !X)) || !params || !dout || !vals || !dparams || !workspace) return REC_E_ARG;
  if (workspace_bytes < fc_ws_bytes(s, k.grid[1])) return REC_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  float* slots = static_cast<float*>(workspace);
  if (hipError_t e = rec_allow_lds<emb_ccpm_bwd_kernel>(FC_LDS_MAX)) return (int)e;
  hipLaunchKernelGGL(emb_ccpm_bwd_kernel, dim3(k.grid[1]), dim3(k.nthr[1]), k.lds[1], st, s, table, X, params, rows,
                     dout, vals, slots);
  REC_LAUNCH_CHECK();
  return rec_slot_sum(REC_SLOTS_WAVE, s.NW, k.grid[1], slots, {{dparams}, {s.NW}}, st);
}
