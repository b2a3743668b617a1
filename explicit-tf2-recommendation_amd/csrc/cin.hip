// Compressed Interaction Network of xDeepFM (CINLayer, 3.DCN/CustomLayers.py:377-417) on the fp32 matrix cores.
//
// Per example, X0 [F,E], H_0 = F, H_{k+1} = cin_size[k], W_k [F*H_k, H_{k+1}] (row m*H_k + n):
//   X^{k+1}[h,e] = sum_{m,n} W_k[m*H_k + n, h] * X0[m,e] * X^k[n,e]          cin_part = concat_k sum_e X^{k+1}[:,e]
// Every layer is a GEMM over the rows (b,e): A_k[(b,e), m*H_k + n] = X0[m,e] * X^k[n,e] (K = F*H_k), B = W_k.  A is
// formed on the fly from X0 and X^k held in LDS (it is never written anywhere), W_k is read from L2, and the products run
// on v_mfma_f32_16x16x4_f32 (lane l: A[l&15][k + (l>>4)], B[k + (l>>4)][l&15]; C: row 4*(l>>4) + q, column l&15).
//
// Forward (cin_fwd_kernel): one workgroup owns TB whole examples (rows b*E + e) across all layers, so the sum over e
// stays inside it.  States X^1..X^L are written [B, sum H, E] for the backward.
// Backward (cin_bwd_kernel): rows are independent here (g is given per example), so a workgroup owns a tile of RP rows
// and walks the layers down: with G^{k+1} = g_k (broadcast over e) + dX^{k+1},
//   S = G^{k+1} W_k^T                      (MFMA, K = H_{k+1}; S never leaves registers)
//   dX^k[n] = sum_m X0[m] S[m*H_k + n]     dX0[m] += sum_n X^k[n] S[m*H_k + n]      (VALU on the MFMA result)
//   dW_k   += A_k^T G^{k+1}                (MFMA, K = the tile's rows)
// Each workgroup adds its tiles' dW into a slot of its own in the workspace (a fixed order of tiles), and
// rec_slot_sum adds the slots in slot order (serial): no float atomics, bit-identical gradients run to run.
#include "common.h"

namespace {

constexpr int CIN_NT = 256;                       // 4 waves
constexpr int CIN_MAXF = REC_CIN_MAX_F, CIN_MAXE = REC_CIN_MAX_E, CIN_MAXL = REC_CIN_MAX_L, CIN_MAXH = REC_CIN_MAX_H;
constexpr size_t CIN_LDS_BUDGET = REC_LDS_CU_BYTES;
constexpr size_t CIN_WS_CAP = (size_t)512 << 20;  // bytes of dW slots the backward may ask for

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct CinShape {
  int64_t B;
  int F, E, L;
  int H[CIN_MAXL + 1];      // H[0] = F
  int off[CIN_MAXL];        // column of layer k's output in [sum H]
  int SH;                   // sum of H[1..L]
  int64_t woff[CIN_MAXL];   // float offset of W_k in one dW slot
  int64_t wsum;             // floats of one dW slot
  const float* W[CIN_MAXL];
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int odd_stride(int n) { return n | 1; }

// ------------------------------------------------------------------------------------------------------------------
// forward: grid = ceil(B / TB), LDS x0s [RP][sX] | buf0 [RP][sH] | buf1 [RP][sH]; wave w owns row tiles
// [w*RT, w*RT + RT) of 16 rows for w < ng.
// ------------------------------------------------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(CIN_NT) void cin_fwd_kernel(CinShape s, const float* __restrict__ x0, int TB, int RP, int ng,
                                                          float* __restrict__ states, float* __restrict__ cin) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E;
  int hmax = 1;
  for (int k = 1; k <= s.L; ++k) hmax = max(hmax, s.H[k]);
  const int sX = odd_stride(F), sH = odd_stride(hmax);
  float* x0s = lds;
  float* buf[2] = {x0s + (size_t)RP * sX, x0s + (size_t)RP * sX + (size_t)RP * sH};
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * TB;
  const int nb = (int)min((int64_t)TB, s.B - b0);   // valid examples of the tile
  const int R = nb * E;                               // valid rows

  for (int i = tid; i < RP * F; i += CIN_NT) {        // e fastest: coalesced reads of x0 [B,F,E]
    const int r = i % RP, m = i / RP;
    float v = 0.f;
    if (r < R) v = x0[(b0 + r / E) * F * E + (int64_t)m * E + r % E];
    x0s[r * sX + m] = v;
  }
  __syncthreads();

  const int c = lane & 15, kk = lane >> 4;
  for (int k = 0; k < s.L; ++k) {
    const int Hin = s.H[k], Hout = s.H[k + 1];
    const float* xin = k == 0 ? x0s : buf[(k - 1) & 1];
    const int sI = k == 0 ? sX : sH;
    float* xout = buf[k & 1];
    const float* __restrict__ W = s.W[k];
    const int nkn = (Hin + 3) >> 2, nsteps = F * nkn;
    const int ntile = (Hout + 15) >> 4;
    if (wave < ng) {
      for (int hc = 0; hc < ntile; hc += 4) {
        const int nh = min(4, ntile - hc);
        f32x4 acc[RT][4];
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
        // B fragments of step st: W[(m*Hin + n) * Hout + h], n = 4*(st % nkn) + kk, h = 16*(hc+u) + c
        auto loadw = [&](int st, float* bw) {
          const int m = st / nkn, n = ((st - m * nkn) << 2) + kk;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int h = ((hc + u) << 4) + c;
            bw[u] = (u < nh && n < Hin && h < Hout) ? W[((int64_t)m * Hin + n) * Hout + h] : 0.f;
          }
        };
        float bw[4], bn[4];
        loadw(0, bw);
        for (int st = 0; st < nsteps; ++st) {
          if (st + 1 < nsteps) loadw(st + 1, bn);     // next step's weights in flight under this step's products
          const int m = st / nkn, n = ((st - m * nkn) << 2) + kk;
          float a[RT];
#pragma unroll
          for (int t = 0; t < RT; ++t) {
            const int r = ((wave * RT + t) << 4) + c;
            a[t] = n < Hin ? x0s[r * sX + m] * xin[r * sI + n] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (u < nh)
#pragma unroll
              for (int t = 0; t < RT; ++t) acc[t][u] = mfma4(a[t], bw[u], acc[t][u]);
#pragma unroll
          for (int u = 0; u < 4; ++u) bw[u] = bn[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int h = ((hc + u) << 4) + c;
          if (u < nh && h < Hout)
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
              for (int q = 0; q < 4; ++q) xout[(((wave * RT + t) << 4) + 4 * kk + q) * sH + h] = acc[t][u][q];
        }
      }
    }
    __syncthreads();
    // states [B, SH, E] (e fastest: coalesced) and cin_part [B, SH] = sum over e in order
    const int off = s.off[k];
    for (int i = tid; i < nb * Hout * E; i += CIN_NT) {
      const int e = i % E, h = (i / E) % Hout, bl = i / (E * Hout);
      states[((b0 + bl) * s.SH + off + h) * E + e] = xout[(bl * E + e) * sH + h];
    }
    for (int i = tid; i < nb * Hout; i += CIN_NT) {
      const int h = i % Hout, bl = i / Hout;
      float sum = 0.f;
      for (int e = 0; e < E; ++e) sum += xout[(bl * E + e) * sH + h];
      cin[(b0 + bl) * s.SH + off + h] = sum;
    }
    // the next layer writes the other buffer and reads this one: the barrier above orders it
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward: a persistent grid of G workgroups; workgroup w takes row tiles w, w + G, ... of RP rows (rows = b*E + e,
// b < B).  LDS x0s | dx0s [RP][sX], xk | gn | gc [RP][sK].
// ------------------------------------------------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(CIN_NT) void cin_bwd_kernel(CinShape s, const float* __restrict__ x0,
                                                          const float* __restrict__ states, const float* __restrict__ g,
                                                          int RP, int ng, float* __restrict__ dx0,
                                                          float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int F = s.F, E = s.E;
  int hmax = F;
  for (int k = 1; k <= s.L; ++k) hmax = max(hmax, s.H[k]);
  const int sX = odd_stride(F), sK = odd_stride(hmax);
  float* x0s = lds;
  float* dx0s = x0s + (size_t)RP * sX;
  float* xk = dx0s + (size_t)RP * sX;
  float* gbuf[2] = {xk + (size_t)RP * sK, xk + 2 * (size_t)RP * sK};
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, kk = lane >> 4;
  const int64_t M = s.B * E;
  const int64_t ntiles = (M + RP - 1) / RP;
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * s.wsum;

  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const bool first = tl == (int64_t)blockIdx.x;     // the slot's first tile stores, later tiles add
    const int64_t g0 = tl * RP;
    const int R = (int)min((int64_t)RP, M - g0);
    for (int i = tid; i < RP * F; i += CIN_NT) {
      const int r = i % RP, m = i / RP;
      float v = 0.f;
      if (r < R) {
        const int64_t gr = g0 + r;
        v = x0[(gr / E) * F * E + (int64_t)m * E + gr % E];
      }
      x0s[r * sX + m] = v;
      dx0s[r * sX + m] = 0.f;
    }
    {
      const int Hl = s.H[s.L], off = s.off[s.L - 1];
      float* gn = gbuf[(s.L - 1) & 1];
      for (int i = tid; i < RP * Hl; i += CIN_NT) {
        const int r = i % RP, h = i / RP;
        gn[r * sK + h] = r < R ? g[((g0 + r) / E) * s.SH + off + h] : 0.f;
      }
    }
    for (int k = s.L - 1; k >= 0; --k) {
      const int Hin = s.H[k], Hout = s.H[k + 1];
      const float* gn = gbuf[k & 1];
      float* gc = gbuf[(k + 1) & 1];
      const float* xin = x0s;
      int sI = sX;
      if (k > 0) {                                    // X^k from the saved states
        const int off = s.off[k - 1];
        for (int i = tid; i < RP * Hin; i += CIN_NT) {
          const int r = i % RP, n = i / RP;
          float v = 0.f;
          if (r < R) {
            const int64_t gr = g0 + r;
            v = states[((gr / E) * s.SH + off + n) * E + gr % E];
          }
          xk[r * sK + n] = v;
        }
        xin = xk;
        sI = sK;
      }
      __syncthreads();
      const float* __restrict__ W = s.W[k];
      const int nkh = (Hout + 3) >> 2;
      // ---- S = G W^T, contracted at once into dX^k (registers) and dX0 (LDS, this wave's rows only)
      if (wave < ng) {
        for (int nt = 0; nt < Hin; nt += 16) {
          const int n = nt + c;
          f32x4 dxk[RT];
#pragma unroll
          for (int t = 0; t < RT; ++t) dxk[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          const int nsteps = F * nkh;
          auto loadw = [&](int st) {
            const int m = st / nkh, h = ((st - m * nkh) << 2) + kk;
            return (n < Hin && h < Hout) ? W[((int64_t)m * Hin + n) * Hout + h] : 0.f;
          };
          float bw = loadw(0);
          f32x4 sa[RT];
#pragma unroll
          for (int t = 0; t < RT; ++t) sa[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int st = 0; st < nsteps; ++st) {
            const float bn = st + 1 < nsteps ? loadw(st + 1) : 0.f;
            const int m = st / nkh, h0 = (st - m * nkh) << 2;
            const int h = h0 + kk;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
              const int r = ((wave * RT + t) << 4) + c;
              const float a = h < Hout ? gn[r * sK + h] : 0.f;
              sa[t] = mfma4(a, bw, sa[t]);
            }
            bw = bn;
            if (h0 + 4 >= Hout) {                     // S[rows, m*Hin + nt .. +16) complete
#pragma unroll
              for (int t = 0; t < RT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const int r = ((wave * RT + t) << 4) + 4 * kk + q;
                  const float sv = sa[t][q];
                  dxk[t][q] += x0s[r * sX + m] * sv;
                  float p = n < Hin ? xin[r * sI + n] * sv : 0.f;
                  p = row16_allsum(p);
                  if (c == 0) dx0s[r * sX + m] += p;
                }
                sa[t] = f32x4{0.f, 0.f, 0.f, 0.f};
              }
            }
          }
          if (n < Hin) {
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int r = ((wave * RT + t) << 4) + 4 * kk + q;
                if (k > 0) {
                  gc[r * sK + n] = dxk[t][q] + (r < R ? g[((g0 + r) / E) * s.SH + s.off[k - 1] + n] : 0.f);
                } else {
                  dx0s[r * sX + n] += dxk[t][q];      // X^0 = X0: the second factor's share
                }
              }
          }
        }
      }
      // ---- dW_k[(m, n), h] += sum_r X0[r,m] X^k[r,n] G[r,h]: tasks (m, 16 n) x (up to 64 h), K = the RP rows
      {
        const int nnt = (Hin + 15) >> 4, nhc = (Hout + 63) >> 6;
        const int ntask = F * nnt * nhc;
        for (int task = wave; task < ntask; task += CIN_NT / 64) {
          const int m = task / (nnt * nhc), rem = task - m * nnt * nhc;
          const int nt = (rem / nhc) << 4, hb = (rem % nhc) << 6;
          const int nh = min(4, (Hout - hb + 15) >> 4);
          const int n = nt + c;
          f32x4 acc[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int r0 = 0; r0 < RP; r0 += 4) {
            const int r = r0 + kk;
            const float a = n < Hin ? x0s[r * sX + m] * xin[r * sI + n] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (u < nh) {
                const int h = hb + (u << 4) + c;
                const float b = h < Hout ? gn[r * sK + h] : 0.f;
                acc[u] = mfma4(a, b, acc[u]);
              }
            }
          }
          float* __restrict__ dst = slot + s.woff[k];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int h = hb + (u << 4) + c;
            if (u < nh && h < Hout)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int nn = nt + 4 * kk + q;
                if (nn < Hin) {
                  float* p = dst + ((int64_t)m * Hin + nn) * Hout + h;
                  *p = first ? acc[u][q] : *p + acc[u][q];
                }
              }
          }
        }
      }
      __syncthreads();                                // gc complete, xk / gn free for the next layer
    }
    for (int i = tid; i < RP * F; i += CIN_NT) {
      const int r = i % RP, m = i / RP;
      if (r < R) {
        const int64_t gr = g0 + r;
        dx0[(gr / E) * F * E + (int64_t)m * E + gr % E] = dx0s[r * sX + m];
      }
    }
    __syncthreads();
  }
}

struct CinCfg {
  int RT, ng, RP;
  size_t lds;
};

// the largest row tile 16*RT*ng (RT <= 4 row tiles of 16 per wave, ng <= 4 waves) whose LDS fits, at least min_rows rows
static bool cin_pick(int floats_per_row, int min_rows, CinCfg* cfg) {
  for (int rows = 256; rows >= 16; rows -= 16) {
    if (rows < min_rows) break;
    const size_t lds = (size_t)rows * floats_per_row * sizeof(float);
    if (lds > CIN_LDS_BUDGET) continue;
    int ng = 4, RT = 0;
    while (ng > 0 && (rows % (16 * ng) != 0 || rows / (16 * ng) > 4)) --ng;
    if (ng == 0) continue;
    RT = rows / (16 * ng);
    cfg->RT = RT;
    cfg->ng = ng;
    cfg->RP = rows;
    cfg->lds = lds;
    return true;
  }
  return false;
}

// 0 ok, REC_E_ARG, REC_E_UNSUPPORTED; fills the shape (without weight pointers)
static int cin_shape(int64_t B, int F, int E, int L, const int* H_host, CinShape* s) {
  if (B < 1 || F < 1 || E < 1 || L < 1 || !H_host) return REC_E_ARG;
  for (int k = 0; k < L && k < CIN_MAXL; ++k)
    if (H_host[k] < 1) return REC_E_ARG;
  if (F > CIN_MAXF || E > CIN_MAXE || L > CIN_MAXL) return REC_E_UNSUPPORTED;
  for (int k = 0; k < L; ++k)
    if (H_host[k] > CIN_MAXH) return REC_E_UNSUPPORTED;
  if (B > ((int64_t)1 << 40) / 64) return REC_E_UNSUPPORTED;
  *s = CinShape{};
  s->B = B;
  s->F = F;
  s->E = E;
  s->L = L;
  s->H[0] = F;
  int off = 0;
  int64_t woff = 0;
  for (int k = 0; k < L; ++k) {
    s->H[k + 1] = H_host[k];
    s->off[k] = off;
    off += H_host[k];
    s->woff[k] = woff;
    woff += (int64_t)F * s->H[k] * s->H[k + 1];
  }
  s->SH = off;
  s->wsum = woff;
  return REC_OK;
}

static int cin_hmax(const CinShape& s, bool with_f) {
  int h = with_f ? s.F : 1;
  for (int k = 1; k <= s.L; ++k) h = h > s.H[k] ? h : s.H[k];
  return h;
}

static bool cin_bwd_cfg(const CinShape& s, CinCfg* cfg, int* grid) {
  const int sX = s.F | 1, sK = cin_hmax(s, true) | 1;
  if (!cin_pick(2 * sX + 3 * sK, 16, cfg)) return false;
  const int64_t ntiles = (s.B * s.E + cfg->RP - 1) / cfg->RP;
  int64_t gmax = (int64_t)(CIN_WS_CAP / ((size_t)s.wsum * sizeof(float)));
  if (gmax < 1) gmax = 1;
  if (gmax > 256) gmax = 256;
  *grid = (int)(ntiles < gmax ? ntiles : gmax);
  return true;
}

template <int RT>
static int cin_launch_fwd(const CinShape& s, const CinCfg& cfg, int TB, const float* x0, float* states, float* cin,
                          hipStream_t st) {
  if (hipError_t e = rec_allow_lds<cin_fwd_kernel<RT>>(CIN_LDS_BUDGET)) return (int)e;
  const int64_t grid = (s.B + TB - 1) / TB;
  hipLaunchKernelGGL(cin_fwd_kernel<RT>, dim3((unsigned)grid), dim3(CIN_NT), cfg.lds, st, s, x0, TB, cfg.RP, cfg.ng,
                     states, cin);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

template <int RT>
static int cin_launch_bwd(const CinShape& s, const CinCfg& cfg, int grid, const float* x0, const float* states,
                          const float* g, float* dx0, float* slots, hipStream_t st) {
  if (hipError_t e = rec_allow_lds<cin_bwd_kernel<RT>>(CIN_LDS_BUDGET)) return (int)e;
  hipLaunchKernelGGL(cin_bwd_kernel<RT>, dim3(grid), dim3(CIN_NT), cfg.lds, st, s, x0, states, g, cfg.RP, cfg.ng, dx0,
                     slots);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

}  // namespace

extern "C" size_t rec_cin_workspace_bytes(int64_t B, int F, int E, int L, const int* H_host) {
  CinShape s;
  if (cin_shape(B, F, E, L, H_host, &s) != REC_OK) return 0;
  CinCfg cfg;
  int grid;
  if (!cin_bwd_cfg(s, &cfg, &grid)) return 0;
  return (size_t)grid * (size_t)s.wsum * sizeof(float);
}

extern "C" int rec_cin_fwd_f32(const float* x0, int64_t B, int F, int E, int L, const int* H_host,
                               const float* const* W_host, float* states, float* cin_part, void* stream) {
  CinShape s;
  const int rc = cin_shape(B, F, E, L, H_host, &s);
  if (rc != REC_OK) return rc;
  if (!x0 || !W_host || !states || !cin_part) return REC_E_ARG;
  for (int k = 0; k < L; ++k) {
    if (!W_host[k]) return REC_E_ARG;
    s.W[k] = W_host[k];
  }
  CinCfg cfg;
  // whole examples per workgroup: at least E rows
  if (!cin_pick((F | 1) + 2 * (cin_hmax(s, false) | 1), E, &cfg)) return REC_E_UNSUPPORTED;
  const int TB = cfg.RP / E;
  hipStream_t st = as_stream(stream);
  return rec_dispatch_1to4(cfg.RT,
                           [&](auto rt) { return cin_launch_fwd<rt.value>(s, cfg, TB, x0, states, cin_part, st); });
}

extern "C" int rec_cin_bwd_f32(const float* x0, const float* states, const float* g, int64_t B, int F, int E, int L,
                               const int* H_host, const float* const* W_host, float* dx0, float* const* dW_host,
                               void* workspace, size_t workspace_bytes, void* stream) {
  CinShape s;
  const int rc = cin_shape(B, F, E, L, H_host, &s);
  if (rc != REC_OK) return rc;
  if (!x0 || !states || !g || !W_host || !dx0 || !dW_host || !workspace) return REC_E_ARG;
  SlotDst dw{};                                      // layer k's dW is segment k of a slot
  for (int k = 0; k < L; ++k) {
    if (!W_host[k] || !dW_host[k]) return REC_E_ARG;
    s.W[k] = W_host[k];
    dw.p[k] = dW_host[k];
    dw.len[k] = F * s.H[k] * s.H[k + 1];
  }
  CinCfg cfg;
  int grid;
  if (!cin_bwd_cfg(s, &cfg, &grid)) return REC_E_UNSUPPORTED;
  if (workspace_bytes < (size_t)grid * (size_t)s.wsum * sizeof(float)) return REC_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  float* slots = static_cast<float*>(workspace);
  const int r = rec_dispatch_1to4(
      cfg.RT, [&](auto rt) { return cin_launch_bwd<rt.value>(s, cfg, grid, x0, states, g, dx0, slots, st); });
  if (r != REC_OK) return r;
  return rec_slot_sum(REC_SLOTS_SERIAL, (int)s.wsum, grid, slots, dw, st);   // wsum <= 8 * 64 * 256 * 256: fits int
}
