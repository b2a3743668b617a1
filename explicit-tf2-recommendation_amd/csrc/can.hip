// CAN co-action (CoActionUnit, 7.SIM/CustomLayers.py:285-378) for gfx950: both lookups, the powers of the feed rows and
// the per-example micro-MLP in one launch each way; formulas, layouts, limits and return codes: include/mi355rec.h.
//
// One workgroup of 256 threads owns an example through all orders.  Its LDS holds the raw feed rows [T][E], the order's
// induction row with every W_l padded to an odd row stride (the forward walks a W row, the backward a W column: both
// are conflict-free), the activations [T][w|1] and, backward, two dz buffers and the running gfeed.  The first 1024
// floats of the next order's row are prefetched into registers across the barriers (which wait for LDS only).  The
// products are f32 FMA chains out of LDS (v_pk_fma_f32): a [T,16]x[16,16] product has a different W per example, T
// rows and widths from 1 to 64 that need not be square; an MFMA tile over positions would pad T to 16 or 32 rows per
// (example, order, layer) and re-lay the fragments between layers, at the same f32 peak.  The forward
// gives a thread four positions of one output column (five LDS reads per four FMAs); dW_l[i][j] is one thread's
// register sum over the positions, written straight into gind: each gind row is written once and nothing is added
// anywhere, so results are bit-identical run to run.
#include "common.h"

namespace {

constexpr int CAN_NTHR = 256;
constexpr int CAN_MAX_W = REC_AFM_MAX_E;            // the widest layer: 64
constexpr int CAN_MAX_L = REC_CAN_MAX_L;            // layers, and orders
constexpr size_t CAN_LDS_CAP = REC_TILE_LDS_CAP;
constexpr int CAN_GRID = 2048;                      // workgroups of a launch: beyond it a workgroup takes another example
constexpr int CAN_TP = 4;                           // positions per thread of a forward layer
constexpr int CAN_RED = 256;                        // floats of the pooled sum's partials
constexpr int CAN_U = 4;                            // global loads a thread keeps in flight

__host__ __device__ constexpr int can_odd(int x) { return x | 1; }

// n / d for 0 <= n with n d < 2^32 in one v_mul_hi_u32: mg = floor(2^32 / d) + 1, or 0 for d = 1.  (An index of this
// kernel is below T wmax <= 38400 and d <= 64; a runtime division is some forty instructions, and the kernel is bound
// by its instruction count.)
static unsigned can_magic(int d) { return d == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)d + 1); }
__device__ __forceinline__ int can_div(int n, unsigned mg) { return mg ? (int)__umulhi((unsigned)n, mg) : n; }

struct CanShape {
  int La, O, n, P, Pa, Eo;                          // Pa: the floats of a row the applied layers cover
  int w[CAN_MAX_L + 1];                             // widths 0..n
  int off[CAN_MAX_L];                               // W_l in a row of the table (B_l follows it)
  int voff[CAN_MAX_L];                              // W_l in the padded LDS copy
  unsigned mg[CAN_MAX_L + 1];                       // can_div's multiplier of every width
  // LDS offsets in floats
  int xf, gf, v, act[CAN_MAX_L + 1], d0, d1, red, flag, total;
};

// REC_OK and the filled shape, or the error of the sizes alone.  bwd: the backward's layout (every activation kept).
int can_shape(int64_t B, int T, int E, int n_layers, const int* coefs, int order, bool bwd, CanShape& s) {
  if (B < 0 || T < 1 || E < 1 || n_layers < 1 || order < 1 || !coefs) return REC_E_ARG;
  for (int l = 0; l < n_layers && l < CAN_MAX_L; ++l)
    if (coefs[l] < 1) return REC_E_ARG;
  if (n_layers > CAN_MAX_L || order > CAN_MAX_L || B >= (int64_t(1) << 31) || E > CAN_MAX_W) return REC_E_UNSUPPORTED;
  s.n = n_layers;
  s.O = order;
  s.La = n_layers < order ? n_layers : order;
  s.w[0] = E;
  for (int l = 0; l < n_layers; ++l) {
    if (coefs[l] > CAN_MAX_W / E) return REC_E_UNSUPPORTED;
    s.w[l + 1] = E * coefs[l];
  }
  int P = 0, Pv = 0, wmax = E, wsum = can_odd(E);
  for (int l = 0; l < n_layers; ++l) {
    s.off[l] = P;
    P += s.w[l] * s.w[l + 1] + s.w[l + 1];
    if (l < s.La) {
      s.Pa = P;
      s.voff[l] = Pv;
      Pv += s.w[l] * can_odd(s.w[l + 1]) + s.w[l + 1];
      wmax = s.w[l + 1] > wmax ? s.w[l + 1] : wmax;
      wsum += can_odd(s.w[l + 1]);
    }
  }
  for (int l = 0; l <= n_layers; ++l) s.mg[l] = can_magic(s.w[l]);
  s.P = P;
  s.Eo = s.w[s.La];
  // the limit is the backward's working set, whichever direction asks
  const int64_t need = 2 * (int64_t)T * E + Pv + (int64_t)T * wsum + 2 * (int64_t)T * can_odd(wmax) + T + CAN_RED;
  if (4 * need > (int64_t)CAN_LDS_CAP) return REC_E_UNSUPPORTED;
  int at = 0;
  s.xf = at; at += T * E;
  s.gf = at; at += bwd ? T * E : 0;
  s.v = at; at += Pv;
  const int buf = T * can_odd(wmax);
  if (bwd) {
    for (int l = 0; l <= s.La; ++l) { s.act[l] = at; at += T * can_odd(s.w[l]); }
  } else {                                          // forward: the activations ping-pong between the two dz buffers
    for (int l = 0; l <= s.La; ++l) s.act[l] = at + (l & 1) * buf;
  }
  s.d0 = at; at += buf;
  s.d1 = at; at += buf;
  s.red = at; at += CAN_RED;
  s.flag = at; at += T;
  s.total = at;
  return REC_OK;
}

struct CanArgs {
  const float* feed;
  int64_t ld_f, Vf;
  const float* ind[CAN_MAX_L];
  int64_t ld_i, Vi;
  const int64_t* iid;
  const int64_t* fid;
  int64_t B, pad;
  int T, E, act;
  CanShape s;
};
static_assert(sizeof(CanArgs) + 7 * sizeof(void*) <= 4096,
              "CanArgs is passed by value: its arrays of CAN_MAX_L entries fit the 4 KiB of kernel arguments");

__device__ __forceinline__ float can_act(int act, float z) {
  switch (act) {
    case REC_ACT_RELU: return z > 0.f ? z : 0.f;
    case REC_ACT_SIGMOID: return sigmoid_acc(z);
    case REC_ACT_TANH: return tanhf(z);
    default: return z;
  }
}
// the derivative from the activation's OUTPUT y
__device__ __forceinline__ float can_dact(int act, float y) {
  switch (act) {
    case REC_ACT_RELU: return y > 0.f ? 1.f : 0.f;
    case REC_ACT_SIGMOID: return y * (1.f - y);
    case REC_ACT_TANH: return fmaf(-y, y, 1.f);
    default: return 1.f;
  }
}

// Workgroup barrier for LDS hand-overs only: the wave's LDS operations are drained, its global loads are not (a
// __syncthreads() waits vmcnt(0) and would end the prefetch of the next induction row at the first barrier it meets).
// Nothing the kernel stores to global memory is read back inside it.
__device__ __forceinline__ void can_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// floats [from, n) of a global row (zeros if !ok) -> put(index, value), CAN_U loads per thread in flight
template <class Put>
__device__ __forceinline__ void can_copy(const float* __restrict__ src, bool ok, int from, int n, int tid, Put put) {
  for (int base = from; base < n; base += CAN_U * CAN_NTHR) {
    float r[CAN_U];
#pragma unroll
    for (int u = 0; u < CAN_U; ++u) {
      const int i = base + u * CAN_NTHR + tid;
      r[u] = ok && i < n ? src[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < CAN_U; ++u) {
      const int i = base + u * CAN_NTHR + tid;
      if (i < n) put(i, r[u]);
    }
  }
}

// x_out [T][ldn] = act(x_in [T][ldi] W + Bv); W [w_in][ldo] in LDS.  A thread: CAN_TP positions of one column.
__device__ __forceinline__ void can_layer(const float* __restrict__ xin, int ldi, float* __restrict__ xout, int ldn,
                                          const float* __restrict__ W, int ldo, const float* __restrict__ Bv, int T,
                                          int w_in, int w_out, unsigned mg_out, int act, int tid) {
  const int ntg = (T + CAN_TP - 1) / CAN_TP;
  for (int it = tid; it < ntg * w_out; it += CAN_NTHR) {
    const int tg = can_div(it, mg_out), j = it - tg * w_out, t0 = tg * CAN_TP;
    const float bj = Bv[j];
    float acc[CAN_TP];
    const float* xr[CAN_TP];
#pragma unroll
    for (int q = 0; q < CAN_TP; ++q) {
      acc[q] = bj;
      xr[q] = xin + (t0 + q < T ? t0 + q : T - 1) * ldi;       // past the end: a row that exists, its result is dropped
    }
#pragma unroll 4
    for (int i = 0; i < w_in; ++i) {
      const float w = W[i * ldo + j];
#pragma unroll
      for (int q = 0; q < CAN_TP; ++q) acc[q] = fmaf(xr[q][i], w, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < CAN_TP; ++q)
      if (t0 + q < T) xout[(t0 + q) * ldn + j] = can_act(act, acc[q]);
  }
}

template <bool BWD>
__global__ __launch_bounds__(CAN_NTHR) void can_kernel(CanArgs a, float* __restrict__ out, float* __restrict__ pool,
                                                       const float* __restrict__ gout, const float* __restrict__ gpool,
                                                       float* __restrict__ gfeed, float* __restrict__ gind,
                                                       int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const CanShape& s = a.s;
  const int T = a.T, E = a.E, La = s.La, Eo = s.Eo, ldE = can_odd(Eo);
  const unsigned mgE = s.mg[0], mgO = s.mg[La];
  float* xf = lds + s.xf;
  float* gf = lds + s.gf;
  float* v = lds + s.v;
  float* red = lds + s.red;
  int* flag = reinterpret_cast<int*>(lds + s.flag);
  bool bad = false;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    can_barrier();                                               // the previous example has left the LDS
    const int64_t iid = a.iid[b];
    const bool iok = iid >= 0 && iid < a.Vi;
    if (!iok) bad = true;
    // the first CAN_U * 256 floats of the row of the order to come: in flight while the feed rows are gathered and,
    // later, while the layers of the order before run
    float pre[CAN_U];
    auto prefetch = [&](int o) {
      const float* row = a.ind[o - 1] + (iok ? iid : 0) * a.ld_i;
#pragma unroll
      for (int u = 0; u < CAN_U; ++u) {
        const int i = u * CAN_NTHR + tid;
        pre[u] = iok && i < s.Pa ? row[i] : 0.f;
      }
    };
    prefetch(1);
    for (int base = 0; base < T * E; base += CAN_U * CAN_NTHR) {  // ids first, then the rows: two latencies per batch
      int64_t id[CAN_U];
      float r[CAN_U];
#pragma unroll
      for (int u = 0; u < CAN_U; ++u) {
        const int i = base + u * CAN_NTHR + tid;
        id[u] = i < T * E ? a.fid[b * T + can_div(i, mgE)] : 0;
      }
#pragma unroll
      for (int u = 0; u < CAN_U; ++u) {
        const int i = base + u * CAN_NTHR + tid;
        const bool ok = id[u] >= 0 && id[u] < a.Vf;
        r[u] = ok && i < T * E ? a.feed[id[u] * a.ld_f + (i - can_div(i, mgE) * E)] : 0.f;
        if (!ok) bad = true;
      }
#pragma unroll
      for (int u = 0; u < CAN_U; ++u) {
        const int i = base + u * CAN_NTHR + tid;
        if (i < T * E) {
          xf[i] = r[u];
          if (BWD) gf[i] = 0.f;
          const int t = can_div(i, mgE);
          if (i == t * E) flag[t] = id[u] == a.pad;
        }
      }
    }
    float poolacc = 0.f;
    // a float of the row -> its place in the padded copy
    auto put_v = [&](int i, float val) {
      for (int l = 0; l < La; ++l) {                             // l stays uniform: the shape is read through scalars
        const int k = i - s.off[l], w_in = s.w[l], w_out = s.w[l + 1], ldo = can_odd(w_out), nW = w_in * w_out;
        float* vl = v + s.voff[l];
        if (k >= 0 && k < nW) {
          const int r = can_div(k, s.mg[l + 1]), c = k - r * w_out;
          vl[r * ldo + c] = val;
        } else if (k >= nW && k < nW + w_out) {
          vl[w_in * ldo + (k - nW)] = val;
        }
      }
    };

    for (int o = 1; o <= s.O; ++o) {
      const int64_t ob = (int64_t)(o - 1) * a.B + b;
      can_barrier();                                             // xf is there; v and the buffers of the last order are free
#pragma unroll
      for (int u = 0; u < CAN_U; ++u) {
        const int i = u * CAN_NTHR + tid;
        if (i < s.Pa) put_v(i, pre[u]);
      }
      can_copy(a.ind[o - 1] + (iok ? iid : 0) * a.ld_i, iok, CAN_U * CAN_NTHR, s.Pa, tid, put_v);
      if (o < s.O) prefetch(o + 1);
      {
        float* x0 = lds + s.act[0];
        const int ld0 = can_odd(E);
        for (int i = tid; i < T * E; i += CAN_NTHR) {
          const int t = can_div(i, mgE), e = i - t * E;
          const float x = xf[i];
          float p = x;
          for (int k = 1; k < o; ++k) p *= x;
          x0[t * ld0 + e] = p;
        }
      }
      can_barrier();
      for (int l = 0; l < La; ++l) {
        const int w_in = s.w[l], w_out = s.w[l + 1], ldo = can_odd(w_out);
        const float* vl = v + s.voff[l];
        can_layer(lds + s.act[l], can_odd(w_in), lds + s.act[l + 1], ldo, vl, ldo, vl + w_in * ldo, T, w_in, w_out,
                  s.mg[l + 1], a.act, tid);
        can_barrier();
      }
      const float* xL = lds + s.act[La];

      if (!BWD) {
        if (out) {
          float* dst = out + ob * T * Eo;
          for (int i = tid; i < T * Eo; i += CAN_NTHR) {
            const int t = can_div(i, mgO), j = i - t * Eo;
            dst[i] = flag[t] ? 0.f : xL[t * ldE + j];
          }
        } else {
          const int npo = can_div(CAN_NTHR, mgO), np = npo < 16 ? npo : 16;
          const int part = can_div(tid, mgO), j = tid - part * Eo;
          if (part < np) {
            float sum = 0.f;
            for (int t = part; t < T; t += np) sum += flag[t] ? 0.f : xL[t * ldE + j];
            red[part * Eo + j] = sum;
          }
          can_barrier();
          if (tid < Eo)
            for (int p = 0; p < np; ++p) poolacc += red[p * Eo + tid];
        }
        continue;
      }

      // ---- backward of this order: dz of the last layer, then layer by layer down to the feed rows
      float* dcur = lds + s.d0;
      float* dnext = lds + s.d1;
      {
        const float* g = gout ? gout + ob * T * Eo : gpool + b * Eo;
        for (int i = tid; i < T * Eo; i += CAN_NTHR) {
          const int t = can_div(i, mgO), j = i - t * Eo;
          const float gv = flag[t] ? 0.f : (gout ? g[i] : g[j]);
          dcur[t * ldE + j] = gv * can_dact(a.act, xL[t * ldE + j]);
        }
      }
      can_barrier();
      float* grow = gind + ob * s.P;
      for (int l = La - 1; l >= 0; --l) {
        const int w_in = s.w[l], w_out = s.w[l + 1], ldo = can_odd(w_out), ldi = can_odd(w_in), nW = w_in * w_out;
        const float* vl = v + s.voff[l];
        const float* xl = lds + s.act[l];
        // dW_l, dB_l: one thread, one element, the positions in order
        for (int it = tid; it < nW + w_out; it += CAN_NTHR) {
          float acc = 0.f;
          if (it < nW) {
            const int i = can_div(it, s.mg[l + 1]), j = it - i * w_out;
#pragma unroll 4
            for (int t = 0; t < T; ++t) acc = fmaf(xl[t * ldi + i], dcur[t * ldo + j], acc);
          } else {
            const int j = it - nW;
#pragma unroll 4
            for (int t = 0; t < T; ++t) acc += dcur[t * ldo + j];
          }
          grow[s.off[l] + it] = acc;
        }
        // dx_l = dz_l W_l^T
        for (int it = tid; it < T * w_in; it += CAN_NTHR) {
          const int t = can_div(it, s.mg[l]), i = it - t * w_in;
          float acc = 0.f;
#pragma unroll 4
          for (int j = 0; j < w_out; ++j) acc = fmaf(dcur[t * ldo + j], vl[i * ldo + j], acc);
          if (l > 0) {
            dnext[t * ldi + i] = acc * can_dact(a.act, xl[t * ldi + i]);
          } else {                                               // through the power: o x^(o-1), x^0 = 1
            const float x = xf[it];
            float p = (float)o;
            for (int k = 1; k < o; ++k) p *= x;
            gf[it] = fmaf(acc, p, gf[it]);                       // this thread owns gf[it] in every order
          }
        }
        can_barrier();
        float* tmp = dcur;
        dcur = dnext;
        dnext = tmp;
      }
      for (int i = s.Pa + tid; i < s.P; i += CAN_NTHR) grow[i] = 0.f;      // the layers the reference drops
    }

    if (!BWD) {
      if (pool && tid < Eo) pool[b * Eo + tid] = poolacc;
    } else {
      for (int i = tid; i < T * E; i += CAN_NTHR) gfeed[b * T * E + i] = gf[i];
    }
  }
  if (!BWD && bad && oob) *oob = 1;
}

template <bool BWD>
int can_launch(const CanArgs& a, float* out, float* pool, const float* gout, const float* gpool, float* gfeed,
               float* gind, int* oob, hipStream_t st) {
  if (hipError_t err = rec_allow_lds<can_kernel<BWD>>(CAN_LDS_CAP)) return (int)err;
  const int grid = a.B < CAN_GRID ? (int)a.B : CAN_GRID;
  hipLaunchKernelGGL(can_kernel<BWD>, dim3(grid), dim3(CAN_NTHR), sizeof(float) * (size_t)a.s.total, st, a, out, pool,
                     gout, gpool, gfeed, gind, oob);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

int can_args(CanArgs& a, bool bwd, const float* feed, int64_t ld_f, int64_t Vf, int E, const float* const* ind,
             int shared, int64_t ld_i, int64_t Vi, int n_layers, const int* coefs, int order, int act,
             const int64_t* iid, const int64_t* fid, int64_t B, int T, int64_t padding_index) {
  if (int rc = can_shape(B, T, E, n_layers, coefs, order, bwd, a.s)) return rc;
  if (ld_f < E || ld_i < a.s.P || Vf < 1 || Vi < 1 || !feed || !ind || !iid || !fid) return REC_E_ARG;
  if (act != REC_ACT_NONE && act != REC_ACT_RELU && act != REC_ACT_SIGMOID && act != REC_ACT_TANH) return REC_E_ARG;
  for (int o = 0; o < CAN_MAX_L; ++o) {
    a.ind[o] = o < order ? ind[shared ? 0 : o] : nullptr;
    if (o < order && !a.ind[o]) return REC_E_ARG;
  }
  a.feed = feed; a.ld_f = ld_f; a.Vf = Vf;
  a.ld_i = ld_i; a.Vi = Vi;
  a.iid = iid; a.fid = fid;
  a.B = B; a.pad = padding_index;
  a.T = T; a.E = E; a.act = act;
  return REC_OK;
}

}  // namespace

extern "C" size_t rec_can_lds_bytes(int T, int E, int n_layers, const int* coefs_host, int order) {
  CanShape s;
  if (can_shape(0, T, E, n_layers, coefs_host, order, true, s) != REC_OK) return 0;
  return sizeof(float) * (size_t)s.total;
}

extern "C" int rec_can_fwd_f32(const float* feed, int64_t ld_f, int64_t Vf, int E, const float* const* ind_host,
                               int shared, int64_t ld_i, int64_t Vi, int n_layers, const int* coefs_host, int order,
                               int act, const int64_t* iid, const int64_t* fid, int64_t B, int T, int64_t padding_index,
                               float* out, float* pool, int* oob_flag, void* stream) {
  CanArgs a;
  if (int rc = can_args(a, false, feed, ld_f, Vf, E, ind_host, shared, ld_i, Vi, n_layers, coefs_host, order, act, iid,
                        fid, B, T, padding_index))
    return rc;
  if (!out == !pool) return REC_E_ARG;
  if (B == 0) return REC_OK;
  return can_launch<false>(a, out, pool, nullptr, nullptr, nullptr, nullptr, oob_flag, as_stream(stream));
}

extern "C" int rec_can_bwd_f32(const float* feed, int64_t ld_f, int64_t Vf, int E, const float* const* ind_host,
                               int shared, int64_t ld_i, int64_t Vi, int n_layers, const int* coefs_host, int order,
                               int act, const int64_t* iid, const int64_t* fid, int64_t B, int T, int64_t padding_index,
                               const float* gout, const float* gpool, float* gfeed, float* gind, void* stream) {
  CanArgs a;
  if (int rc = can_args(a, true, feed, ld_f, Vf, E, ind_host, shared, ld_i, Vi, n_layers, coefs_host, order, act, iid,
                        fid, B, T, padding_index))
    return rc;
  if (!gout == !gpool || !gfeed || !gind) return REC_E_ARG;
  if (B == 0) return REC_OK;                                     // nothing is launched and nothing written
  return can_launch<true>(a, nullptr, nullptr, gout, gpool, gfeed, gind, nullptr, as_stream(stream));
}
