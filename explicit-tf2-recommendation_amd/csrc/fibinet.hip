// FiBiNet interaction (FiBiNetLayer, SENetLayer, BilinearInteractionLayer; 3.DCN/CustomLayers.py:888-1011) on the
// fp32 matrix cores.  Per example, v = x_emb [F,E], P = F(F-1)/2 pairs (i<j) in itertools.combinations order:
//   SENet   Z_f = mean_e v_f     H1 = relu(Z S0)  [mid]     A = relu(H1 S1)  [F]      (no bias)
//   pairs   p_ij = (v_i W_ij) (.) v_j          W_ij = W[0] ('all'), W[i] ('each'), W[pair] ('interaction')
//   SENet pairs: ((A_i v_i) W_ij) (.) (A_j v_j) = A_i A_j p_ij   -- the second bilinear pass is one scale per element
//   dnn_in [B, 2PE + C] = [raw pairs | SENet pairs | x_cont], element (s, pair, e) at column (s P + pair) E + e.
// An "item" is one left product q = v_i W: one pair for 'interaction', one field i (reused for every j > i) otherwise.
// q runs on v_mfma_f32_16x16x4_f32 over a tile of 16 examples (lane l: A[l&15][k + (l>>4)], B[k + (l>>4)][l&15];
// D: row 4*(l>>4) + q, column l&15), E padded to a multiple of 4 by zero operands, 16-column tiles of e.
//
// Forward (fibinet_fwd_kernel): one workgroup per 16 examples; SENet by the whole workgroup, then the 4 waves take
// items round robin.  Each D register stores 16 consecutive floats of one row (4 rows per store instruction).
// Backward, with gp = g_raw + A_i A_j g_senet and u = v_j (.) gp:
//   fibinet_bwd_x_kernel  one wave per tile of 16 examples (a persistent grid): dv_j += q (.) gp and
//                         dv_i += u W^T (MFMA; u transposed through the wave's LDS), dA_i += A_j <g_senet, p_ij>,
//                         dA_j += A_i <g_senet, p_ij>, then back through both ReLUs: dv_f += dZ_f / E and the wave's
//                         dS0 / dS1 partial into a workspace slot of its own.  dx rows belong to one wave and every
//                         element to one lane, so the read-modify-writes of dx need no atomics.
//   fibinet_bwd_w_kernel  one workgroup per (item, chunk of examples): dW_item += v_i^T (sum_j u) with K over the
//                         chunk's examples (MFMA, accumulated in registers), the 4 waves summed in wave order into a slot.
//   rec_slot_sum adds the dW slots in chunk order (serial) and the dS slots in its wave order.
// No float atomics: bit-identical results run to run.
#include "common.h"

namespace {

constexpr int FB_NT = 256;                       // 4 waves
constexpr int FB_MAXF = REC_FIBINET_MAX_F, FB_MAXE = REC_FIBINET_MAX_E, FB_MAXC = REC_FIBINET_MAX_C;
enum { FB_ALL = REC_FIBINET_TYPE_ALL, FB_EACH = REC_FIBINET_TYPE_EACH, FB_INTERACTION = REC_FIBINET_TYPE_INTERACTION };
static_assert(FB_ALL < FB_EACH && FB_EACH < FB_INTERACTION && FB_INTERACTION - FB_ALL == 2,
              "fb_shape takes the types as a range");
constexpr int FB_MAXX_BLOCKS = 1024;             // persistent grid of the dx kernel: at most 4096 dS slots
constexpr int FB_TARGET_W_BLOCKS = 2048;         // workgroups of the dW kernel (items x chunks)
constexpr int FB_MAX_CHUNKS = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct FbShape {
  int64_t B, D;       // D = 2 P E + C, the row length of dnn_in
  int F, E, C, mid, type, P, nW, nitem;
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// LDS written by some lanes of a wave and read by others of the same wave
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int pair_index(int F, int i, int j) { return i * F - i * (i + 1) / 2 + (j - i - 1); }

// item -> left field i, weight w, right fields [j0, j1)
__device__ __forceinline__ void item_of(const FbShape& s, int it, int& i, int& w, int& j0, int& j1) {
  if (s.type == FB_INTERACTION) {
    int p = it;
    i = 0;
    while (p >= s.F - 1 - i) {
      p -= s.F - 1 - i;
      ++i;
    }
    w = it;
    j0 = i + 1 + p;
    j1 = j0 + 1;
  } else {
    i = it;
    w = s.type == FB_EACH ? it : 0;
    j0 = it + 1;
    j1 = s.F;
  }
}

// q[u] = v_i W over the rows b0 .. b0+15 (rows >= nb read as 0): D layout, row 4*kk + r, column 16u + c
template <int NTC>
__device__ __forceinline__ void left_product(const FbShape& s, const float* __restrict__ x, int64_t b0, int nb, int i,
                                             const float* __restrict__ Ww, int c, int kk, f32x4 (&q)[NTC]) {
  const int E = s.E, ns = (E + 3) >> 2;
#pragma unroll
  for (int u = 0; u < NTC; ++u) q[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* xr = x + ((b0 + c) * s.F + i) * E;
  for (int st = 0; st < ns; ++st) {
    const int k = 4 * st + kk;
    const float a = (c < nb && k < E) ? xr[k] : 0.f;
#pragma unroll
    for (int u = 0; u < NTC; ++u) {
      const int col = 16 * u + c;
      const float b = (k < E && col < E) ? Ww[k * E + col] : 0.f;
      q[u] = mfma4(a, b, q[u]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// forward: grid = ceil(B/16)
// ------------------------------------------------------------------------------------------------------------------
template <int NTC>
__global__ __launch_bounds__(FB_NT) void fibinet_fwd_kernel(FbShape s, const float* __restrict__ x,
                                                             const float* __restrict__ xc, const float* __restrict__ S0,
                                                             const float* __restrict__ S1, const float* __restrict__ W,
                                                             float* __restrict__ dnn, float* __restrict__ Aout,
                                                             float* __restrict__ H1out) {
  __shared__ float zs[16 * FB_MAXF], hs[16 * FB_MAXF], as[16 * FB_MAXF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kk = lane >> 4;
  const int F = s.F, E = s.E, mid = s.mid, C = s.C, P = s.P;
  const int64_t b0 = (int64_t)blockIdx.x * 16;
  const int nb = (int)min((int64_t)16, s.B - b0);

  for (int t = tid; t < 16 * F; t += FB_NT) {
    const int r = t / F, f = t - r * F;
    float z = 0.f;
    if (r < nb) {
      const float* p = x + ((b0 + r) * F + f) * E;
      for (int e = 0; e < E; ++e) z += p[e];
      z /= (float)E;
    }
    zs[t] = z;
  }
  __syncthreads();
  for (int t = tid; t < 16 * mid; t += FB_NT) {
    const int r = t / mid, m = t - r * mid;
    float h = 0.f;
    for (int f = 0; f < F; ++f) h += zs[r * F + f] * S0[f * mid + m];
    h = h > 0.f ? h : 0.f;
    hs[t] = h;
    if (r < nb) H1out[(b0 + r) * mid + m] = h;
  }
  __syncthreads();
  for (int t = tid; t < 16 * F; t += FB_NT) {
    const int r = t / F, f = t - r * F;
    float a = 0.f;
    for (int m = 0; m < mid; ++m) a += hs[r * mid + m] * S1[m * F + f];
    a = a > 0.f ? a : 0.f;
    as[t] = a;
    if (r < nb) Aout[(b0 + r) * F + f] = a;
  }
  const int64_t cbase = 2LL * P * E;
  for (int t = tid; t < nb * C; t += FB_NT) {
    const int r = t / C, k = t - r * C;
    dnn[(b0 + r) * s.D + cbase + k] = xc[(b0 + r) * C + k];
  }
  __syncthreads();

  for (int it = wave; it < s.nitem; it += FB_NT / 64) {
    int i, w, j0, j1;
    item_of(s, it, i, w, j0, j1);
    f32x4 q[NTC];
    left_product<NTC>(s, x, b0, nb, i, W + (int64_t)w * E * E, c, kk, q);
    for (int j = j0; j < j1; ++j) {
      const int pr = pair_index(F, i, j);
#pragma unroll
      for (int u = 0; u < NTC; ++u) {
        const int e = 16 * u + c;
        if (e >= E) continue;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int r = 4 * kk + qq;
          if (r < nb) {
            const float p = q[u][qq] * x[((b0 + r) * F + j) * E + e];
            float* row = dnn + (b0 + r) * s.D;
            row[(int64_t)pr * E + e] = p;
            row[(int64_t)(P + pr) * E + e] = (as[r * F + i] * as[r * F + j]) * p;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward, dx / dA / dS: wave gw of the grid takes the 16-example tiles gw, gw + 4*grid, ...
// LDS per wave: as | da | zs | hs | t2 | ub   (16F, 16F, 16F, 16mid, 16mid, 16*sU floats)
// ------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int fb_ustride(int E) { return E | 1; }
__host__ __device__ inline int fb_wave_floats(int F, int mid, int E) { return 48 * F + 32 * mid + 16 * fb_ustride(E); }

template <int NTC>
__global__ __launch_bounds__(FB_NT) void fibinet_bwd_x_kernel(FbShape s, const float* __restrict__ x,
                                                               const float* __restrict__ g,
                                                               const float* __restrict__ Asv,
                                                               const float* __restrict__ H1sv,
                                                               const float* __restrict__ S0,
                                                               const float* __restrict__ S1,
                                                               const float* __restrict__ W, float* __restrict__ dx,
                                                               float* __restrict__ dsl) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kk = lane >> 4;
  const int F = s.F, E = s.E, mid = s.mid, P = s.P, sU = fb_ustride(E), ns = (E + 3) >> 2;
  float* as = lds + (size_t)wave * fb_wave_floats(F, mid, E);
  float* da = as + 16 * F;
  float* zs = da + 16 * F;
  float* hs = zs + 16 * F;
  float* t2 = hs + 16 * mid;
  float* ub = t2 + 16 * mid;
  const int nsf = 2 * F * mid;
  const int64_t gw = (int64_t)blockIdx.x * (FB_NT / 64) + wave, nwg = (int64_t)gridDim.x * (FB_NT / 64);
  float* __restrict__ slot = dsl + gw * nsf;
  const int64_t ntiles = (s.B + 15) / 16;
  const float invE = 1.f / (float)E;

  for (int64_t tl = gw; tl < ntiles; tl += nwg) {
    const bool first = tl == gw;
    const int64_t b0 = tl * 16;
    const int nb = (int)min((int64_t)16, s.B - b0);
    for (int t = lane; t < 16 * F; t += 64) {
      const int r = t / F, f = t - r * F;
      as[t] = r < nb ? Asv[(b0 + r) * F + f] : 0.f;
      da[t] = 0.f;
    }
    for (int t = lane; t < 16 * mid; t += 64) {
      const int r = t / mid, m = t - r * mid;
      hs[t] = r < nb ? H1sv[(b0 + r) * mid + m] : 0.f;
    }
    // dx rows of the tile start at 0; element (r, f, e) is always touched by lane (c = e % 16, kk = r / 4)
    for (int f = 0; f < F; ++f)
#pragma unroll
      for (int u = 0; u < NTC; ++u) {
        const int e = 16 * u + c;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int r = 4 * kk + qq;
          if (e < E && r < nb) dx[((b0 + r) * F + f) * E + e] = 0.f;
        }
      }
    wave_sync();

    for (int it = 0; it < s.nitem; ++it) {
      int i, w, j0, j1;
      item_of(s, it, i, w, j0, j1);
      const float* __restrict__ Ww = W + (int64_t)w * E * E;
      f32x4 q[NTC], us[NTC];
      left_product<NTC>(s, x, b0, nb, i, Ww, c, kk, q);
#pragma unroll
      for (int u = 0; u < NTC; ++u) us[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = j0; j < j1; ++j) {
        const int pr = pair_index(F, i, j);
        float sp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NTC; ++u) {
          const int e = 16 * u + c;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int r = 4 * kk + qq;
            const bool ok = e < E && r < nb;
            const float* grow = g + (b0 + r) * s.D;
            const float vj = ok ? x[((b0 + r) * F + j) * E + e] : 0.f;
            const float gr = ok ? grow[(int64_t)pr * E + e] : 0.f;
            const float gs = ok ? grow[(int64_t)(P + pr) * E + e] : 0.f;
            const float aa = as[r * F + i] * as[r * F + j];
            const float gp = gr + aa * gs;
            if (ok) dx[((b0 + r) * F + j) * E + e] += q[u][qq] * gp;
            sp[qq] += gs * (q[u][qq] * vj);
            us[u][qq] += vj * gp;
          }
        }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const float sr = row16_allsum(sp[qq]);
          const int r = 4 * kk + qq;
          if (c == 0) {
            da[r * F + i] += as[r * F + j] * sr;
            da[r * F + j] += as[r * F + i] * sr;
          }
        }
        if (s.type != FB_INTERACTION && j + 1 < j1) continue;   // 'all' / 'each': u summed over j, one u W^T per item
        // dv_i += u W^T: u to LDS in D layout, back as the A operand (row c, k = e)
#pragma unroll
        for (int u = 0; u < NTC; ++u) {
          const int e = 16 * u + c;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq)
            if (e < E) ub[(4 * kk + qq) * sU + e] = us[u][qq];
          us[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        wave_sync();
        f32x4 o[NTC];
#pragma unroll
        for (int u = 0; u < NTC; ++u) o[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int st = 0; st < ns; ++st) {
          const int k = 4 * st + kk;
          const float a = k < E ? ub[c * sU + k] : 0.f;
#pragma unroll
          for (int u = 0; u < NTC; ++u) {
            const int col = 16 * u + c;
            const float b = (k < E && col < E) ? Ww[col * E + k] : 0.f;
            o[u] = mfma4(a, b, o[u]);
          }
        }
        wave_sync();                                 // ub is rewritten by the next pair
#pragma unroll
        for (int u = 0; u < NTC; ++u) {
          const int e = 16 * u + c;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int r = 4 * kk + qq;
            if (e < E && r < nb) dx[((b0 + r) * F + i) * E + e] += o[u][qq];
          }
        }
      }
    }

    // SENet backward: dP2 = dA (A > 0); dP1 = (dP2 S1^T)(H1 > 0); dZ = dP1 S0^T; dv_f += dZ_f / E
    wave_sync();
    for (int t = lane; t < 16 * F; t += 64) {
      const int r = t / F, f = t - r * F;
      float z = 0.f;
      if (r < nb) {
        const float* p = x + ((b0 + r) * F + f) * E;
        for (int e = 0; e < E; ++e) z += p[e];
        z /= (float)E;
      }
      zs[t] = z;
      da[t] = as[t] > 0.f ? da[t] : 0.f;
    }
    wave_sync();
    for (int t = lane; t < 16 * mid; t += 64) {
      const int r = t / mid, m = t - r * mid;
      float h = 0.f;
      for (int f = 0; f < F; ++f) h += da[r * F + f] * S1[m * F + f];
      t2[t] = hs[t] > 0.f ? h : 0.f;
    }
    wave_sync();
    for (int t = lane; t < F * mid; t += 64) {
      const int f = t / mid, m = t - f * mid;
      float d0 = 0.f, d1 = 0.f;
      for (int r = 0; r < 16; ++r) {
        d0 += zs[r * F + f] * t2[r * mid + m];
        d1 += hs[r * mid + m] * da[r * F + f];
      }
      float* p0 = slot + t;                                   // dS0 [F, mid]
      float* p1 = slot + F * mid + m * F + f;                  // dS1 [mid, F]
      *p0 = first ? d0 : *p0 + d0;
      *p1 = first ? d1 : *p1 + d1;
    }
    for (int t = lane; t < 16 * F; t += 64) {                 // dZ / E into as (A is not read again in this tile)
      const int r = t / F, f = t - r * F;
      float z = 0.f;
      for (int m = 0; m < mid; ++m) z += t2[r * mid + m] * S0[f * mid + m];
      as[t] = z * invE;
    }
    wave_sync();
    for (int f = 0; f < F; ++f)
#pragma unroll
      for (int u = 0; u < NTC; ++u) {
        const int e = 16 * u + c;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const int r = 4 * kk + qq;
          if (e < E && r < nb) dx[((b0 + r) * F + f) * E + e] += as[r * F + f];
        }
      }
    wave_sync();                                              // the next tile rewrites as / da / zs / hs
  }
}

// ------------------------------------------------------------------------------------------------------------------
// backward, dW: workgroup (item it, chunk ch) over the tiles [ch*tpc, min(ntiles, ch*tpc + tpc)); LDS red [E*E]
// ------------------------------------------------------------------------------------------------------------------
template <int NTC>
__global__ __launch_bounds__(FB_NT) void fibinet_bwd_w_kernel(FbShape s, const float* __restrict__ x,
                                                               const float* __restrict__ g,
                                                               const float* __restrict__ Asv, int64_t tpc,
                                                               float* __restrict__ wsl) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kk = lane >> 4;
  const int F = s.F, E = s.E, P = s.P;
  const int it = (int)(blockIdx.x % s.nitem);
  const int64_t ch = blockIdx.x / s.nitem;
  int i, w, j0, j1;
  item_of(s, it, i, w, j0, j1);
  const int64_t ntiles = (s.B + 15) / 16;
  const int64_t t0 = ch * tpc, t1 = min(ntiles, t0 + tpc);
  f32x4 acc[NTC][NTC];
#pragma unroll
  for (int a = 0; a < NTC; ++a)
#pragma unroll
    for (int u = 0; u < NTC; ++u) acc[a][u] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t tl = t0 + wave; tl < t1; tl += FB_NT / 64) {
    const int64_t b0 = tl * 16;
    const int nb = (int)min((int64_t)16, s.B - b0);
    f32x4 us[NTC];
#pragma unroll
    for (int u = 0; u < NTC; ++u) us[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ai[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int r = 4 * kk + qq;
      ai[qq] = r < nb ? Asv[(b0 + r) * F + i] : 0.f;
    }
    for (int j = j0; j < j1; ++j) {
      const int pr = pair_index(F, i, j);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int r = 4 * kk + qq;
        const float aa = r < nb ? ai[qq] * Asv[(b0 + r) * F + j] : 0.f;
        const float* grow = g + (b0 + r) * s.D;
#pragma unroll
        for (int u = 0; u < NTC; ++u) {
          const int e = 16 * u + c;
          const bool ok = e < E && r < nb;
          const float vj = ok ? x[((b0 + r) * F + j) * E + e] : 0.f;
          const float gr = ok ? grow[(int64_t)pr * E + e] : 0.f;
          const float gs = ok ? grow[(int64_t)(P + pr) * E + e] : 0.f;
          us[u][qq] += vj * (gr + aa * gs);
        }
      }
    }
    // dW[e'][e] += sum_r v_i[r][e'] u[r][e]; k-step qq takes the rows 4*kk + qq (u straight from its D registers)
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int r = 4 * kk + qq;
#pragma unroll
      for (int a = 0; a < NTC; ++a) {
        const int ep = 16 * a + c;
        const float av = (r < nb && ep < E) ? x[((b0 + r) * F + i) * E + ep] : 0.f;
#pragma unroll
        for (int u = 0; u < NTC; ++u) acc[a][u] = mfma4(av, us[u][qq], acc[a][u]);
      }
    }
  }
  // the 4 waves' partials summed in wave order
  for (int wv = 0; wv < FB_NT / 64; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int a = 0; a < NTC; ++a)
#pragma unroll
        for (int u = 0; u < NTC; ++u)
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int ep = 16 * a + 4 * kk + qq, e = 16 * u + c;
            if (ep < E && e < E) red[ep * E + e] = wv == 0 ? acc[a][u][qq] : red[ep * E + e] + acc[a][u][qq];
          }
    }
    __syncthreads();
  }
  float* __restrict__ dst = wsl + ((int64_t)ch * s.nitem + it) * E * E;
  for (int t = tid; t < E * E; t += FB_NT) dst[t] = red[t];
}

// 0 ok (B == 0 included), REC_E_ARG, REC_E_UNSUPPORTED
static int fb_shape(int64_t B, int F, int E, int C, int mid, int type, FbShape* s) {
  if (B < 0 || F < 0 || E < 0 || C < 0 || mid < 0 || type < FB_ALL || type > FB_INTERACTION) return REC_E_ARG;
  if (F < 2 || F > FB_MAXF || E < 1 || E > FB_MAXE || C > FB_MAXC || mid < 1 || mid > F) return REC_E_UNSUPPORTED;
  if (B > ((int64_t)1 << 40) / 64) return REC_E_UNSUPPORTED;
  *s = FbShape{};
  s->B = B;
  s->F = F;
  s->E = E;
  s->C = C;
  s->mid = mid;
  s->type = type;
  s->P = F * (F - 1) / 2;
  s->nW = type == FB_ALL ? 1 : (type == FB_EACH ? F - 1 : s->P);
  s->nitem = type == FB_INTERACTION ? s->P : F - 1;
  s->D = 2LL * s->P * E + C;
  return REC_OK;
}

struct FbBwdCfg {
  int xgrid;            // workgroups of the dx kernel
  int64_t nslot;        // dS slots written (waves that own at least one tile)
  int64_t tpc, nchunk;  // tiles per chunk and chunks of the dW kernel
  size_t wsl_floats, dsl_floats;
};

static FbBwdCfg fb_bwd_cfg(const FbShape& s) {
  FbBwdCfg k{};
  const int64_t ntiles = (s.B + 15) / 16;
  int64_t xg = (ntiles + 3) / 4;
  k.xgrid = (int)(xg < FB_MAXX_BLOCKS ? (xg < 1 ? 1 : xg) : FB_MAXX_BLOCKS);
  k.nslot = ntiles < 4LL * k.xgrid ? ntiles : 4LL * k.xgrid;
  int64_t want = (FB_TARGET_W_BLOCKS + s.nitem - 1) / s.nitem;
  if (want > FB_MAX_CHUNKS) want = FB_MAX_CHUNKS;
  if (want > ntiles) want = ntiles;
  if (want < 1) want = 1;
  k.tpc = (ntiles + want - 1) / want;
  if (k.tpc < 1) k.tpc = 1;
  k.nchunk = (ntiles + k.tpc - 1) / k.tpc;
  if (k.nchunk < 1) k.nchunk = 1;
  k.wsl_floats = (size_t)k.nchunk * s.nitem * s.E * s.E;
  k.dsl_floats = (size_t)4 * k.xgrid * 2 * s.F * s.mid;
  return k;
}

static size_t fb_ws_bytes(const FbBwdCfg& k) {
  return rec_align_up(k.wsl_floats * sizeof(float), 256) + k.dsl_floats * sizeof(float);
}

template <int NTC>
static int fb_fwd(const FbShape& s, const float* x, const float* xc, const float* S0, const float* S1, const float* W,
                  float* dnn, float* A, float* H1, hipStream_t st) {
  hipLaunchKernelGGL(fibinet_fwd_kernel<NTC>, dim3((unsigned)((s.B + 15) / 16)), dim3(FB_NT), 0, st, s, x, xc, S0, S1,
                     W, dnn, A, H1);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

template <int NTC>
static int fb_bwd(const FbShape& s, const FbBwdCfg& k, const float* x, const float* g, const float* A, const float* H1,
                  const float* S0, const float* S1, const float* W, float* dx, float* wsl, float* dsl, hipStream_t st) {
  const size_t xlds = (size_t)4 * fb_wave_floats(s.F, s.mid, s.E) * sizeof(float);
  hipLaunchKernelGGL(fibinet_bwd_x_kernel<NTC>, dim3(k.xgrid), dim3(FB_NT), xlds, st, s, x, g, A, H1, S0, S1, W, dx,
                     dsl);
  REC_LAUNCH_CHECK();
  hipLaunchKernelGGL(fibinet_bwd_w_kernel<NTC>, dim3((unsigned)(k.nchunk * s.nitem)), dim3(FB_NT),
                     (size_t)s.E * s.E * sizeof(float), st, s, x, g, A, k.tpc, wsl);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

}  // namespace

extern "C" size_t rec_fibinet_workspace_bytes(int64_t B, int F, int E, int mid, int type) {
  FbShape s;
  if (fb_shape(B, F, E, 0, mid, type, &s) != REC_OK) return 0;
  return fb_ws_bytes(fb_bwd_cfg(s));
}

extern "C" int rec_fibinet_fwd_f32(const float* x_emb, const float* x_cont, const float* S0, const float* S1,
                                   const float* W, int64_t B, int F, int E, int C, int mid, int type, float* dnn_in,
                                   float* A, float* H1, void* stream) {
  FbShape s;
  const int rc = fb_shape(B, F, E, C, mid, type, &s);
  if (rc != REC_OK || B == 0) return rc;
  if (!x_emb || (C > 0 && !x_cont) || !S0 || !S1 || !W || !dnn_in || !A || !H1) return REC_E_ARG;
  hipStream_t st = as_stream(stream);
  return rec_dispatch_1to4((E + 15) / 16,
                           [&](auto ntc) { return fb_fwd<ntc.value>(s, x_emb, x_cont, S0, S1, W, dnn_in, A, H1, st); });
}

extern "C" int rec_fibinet_bwd_f32(const float* x_emb, const float* g, const float* A, const float* H1,
                                   const float* S0, const float* S1, const float* W, int64_t B, int F, int E, int C,
                                   int mid, int type, float* dx_emb, float* dW, float* dS0, float* dS1,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  FbShape s;
  const int rc = fb_shape(B, F, E, C, mid, type, &s);
  if (rc != REC_OK || B == 0) return rc;
  if (!x_emb || !g || !A || !H1 || !S0 || !S1 || !W || !dx_emb || !dW || !dS0 || !dS1 || !workspace) return REC_E_ARG;
  const FbBwdCfg k = fb_bwd_cfg(s);
  if (workspace_bytes < fb_ws_bytes(k)) return REC_E_WORKSPACE;
  float* wsl = static_cast<float*>(workspace);
  float* dsl =
      reinterpret_cast<float*>(static_cast<char*>(workspace) + rec_align_up(k.wsl_floats * sizeof(float), 256));
  hipStream_t st = as_stream(stream);
  int r = rec_dispatch_1to4((E + 15) / 16, [&](auto ntc) {
    return fb_bwd<ntc.value>(s, k, x_emb, g, A, H1, S0, S1, W, dx_emb, wsl, dsl, st);
  });
  if (r != REC_OK) return r;
  // dW: the chunks in chunk order, a slot holding the chunk's nitem = nW matrices; 'all' has one W, which takes every
  // (chunk, item) in that order
  const int nw = s.nW * E * E, nws = (int)(type == FB_ALL ? k.nchunk * s.nitem : k.nchunk);
  r = rec_slot_sum(REC_SLOTS_SERIAL, nw, nws, wsl, {{dW}, {nw}}, st);
  if (r != REC_OK) return r;
  return rec_slot_sum(REC_SLOTS_WAVE, 2 * F * mid, (int)k.nslot, dsl, {{dS0, dS1}, {F * mid, F * mid}}, st);
}
