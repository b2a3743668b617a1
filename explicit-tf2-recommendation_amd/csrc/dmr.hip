// DMR (DMRI2INetworkLayer, DMRU2INetworkLayer and compute_auxiliary_loss, 8.DMR/CustomLayers.py:203-316) on gfx950, fp32:
// both attention units over the looked-up behaviour series and the auxiliary match loss over the sampled negatives, one
// launch each way.  The batch-independent P = pos [Wp_i2i | Wp_u2i] [T, 2H] and the batch GEMM q = xi Wc [B, H] come in
// as operands (rec_gemm_f32 makes them); We = [We_i2i | We_u2i] [D, 2H] and z = [z_i2i ; z_u2i] [2, H].
//
// One example per workgroup of 4 waves, a capped persistent grid, as the ComiRec self-attentive extractor:
//   gather   the T C series rows into xs [T][D|1] (valid[t] = series[b,t,0] != pad, from the id read anyway), the Nn C
//            negative rows into xn [Nn][D|1]: each row is read once for both units and for the loss
//   project  h [T][2H|1] = xs We on v_mfma_f32_32x32x2_f32, then h = tanh(([q |0] + h) + P)
//   scores   s[u,t] = z_u . h[t, uH:(u+1)H]; wave u: the masked softmax A[u], score_sum, n = sum valid (n = 0: A = 0)
//   pool     i2i = A0 xs, u = A1 xs, lv = A1[last] xs[last], ov = sum_{t<last} A1[t] xs[t]           (last = n - 1)
//   loss     nrm(v) = v / sqrt(max(sum v^2, 1e-12)), cos = sum nrm(p) nrm(q); pos = (1 - cos(lv, ov)) / 2,
//            neg_j = (1 - cos(xneg_j, ov)) / 2, aux = softplus(-pos) + sum_j softplus(neg_j)         (n = 0: aux = 0)
// Backward: the forward again, then with gi | gss = g_i2i, gu | gin = g_u2i, ga = g_aux
//   dcp = ga (1 - sigmoid(pos)) / 2   dc_j = -ga sigmoid(neg_j) / 2                  (the cosine enters negated, halved)
//   d cos(p,q) / dp = rp (nrm(q) - cos nrm(p)) where sum p^2 >= 1e-12, rp nrm(q) with rp = 1e6 below (the clamp is a
//   constant there, as in TF)      dlv, dov (the negatives add into dov), gneg_j from it
//   gav_t = gu + gin xi + [t == last] dlv + [t < last] dov       dA0[t] = gi . x_t    dA1[t] = gav_t . x_t
//   ds_u[t] = valid ? A_u[t] (dA_u[t] - sum A_u dA_u) + [u == 0] gss : 0
//   dz_u += sum_t ds_u[t] h[t, u]    dh = ds_u z_u (1 - h^2) (over h)    gq = sum_t dh[t, :H]    dP += dh
//   gkeys[t] = dh[t] We^T + A0[t] gi + A1[t] gav_t    dWe += xs^T dh    gitem = gin u
// dWe stays in registers over the workgroup's examples where its 32 x 32 blocks fit 8 per wave (else a block group at a
// time is added to the slot per example), dz in LDS, dP in the workgroup's own slot (one thread owns an element: the
// order is fixed); rec_slot_sum adds the slots [dWe | dP | dz] in wave order.  No float atomics, no scratch memory;
// every launch only enqueues.
#include "capsule.h"

namespace {

constexpr int DM_GRID = 1024;                   // workgroups (= slots) of the backward, at the most
constexpr float DM_EPS = 1e-12f;                // tf.math.l2_normalize's epsilon

struct DmArgs : CapsSeries {                    // Dc = 2 H, K = 1
  const int64_t* neg;
  const float *xi, *q, *P, *We, *z;
  int H, Nn;
};

// floats of LDS of one example, the same both ways (include/mi355rec.h):
//   xs [T][D|1], h [T][2H|1], xn [Nn][D|1], 8 vectors [D|1] (xi, gi, gb, u, lv, ov, dlv, dov), s, A and ds [2][T] each,
//   valid [T], z and dz [2H] each, q [H], three [Nn] (sum of squares, cosine, dc) and 16 scalars
__host__ __device__ inline size_t dm_lds_floats(int T, int D, int H, int Nn) {
  return (size_t)T * (mi_odd(D) + mi_odd(2 * H) + 7) + (size_t)Nn * (mi_odd(D) + 3) + 8 * (size_t)mi_odd(D) +
         5 * (size_t)H + 16;
}

static int dm_check(int64_t B, int T, int E, int C, int H, int Nn) {
  if (B < 0 || T < 1 || E < 1 || C < 1 || H < 1 || Nn < 1) return REC_E_ARG;
  if ((int64_t)E * C > MI_MAXD || H > MI_MAXD || B >= ((int64_t)1 << 31) || T > (int)(MI_LDS_CAP / sizeof(float)) ||
      Nn > (int)(MI_LDS_CAP / sizeof(float)))
    return REC_E_UNSUPPORTED;
  return caps_fits(sizeof(float) * dm_lds_floats(T, E * C, H, Nn));
}
// floats of a workgroup's slot: dWe [D, 2H], dP [T, 2H], dz [2H]
__host__ __device__ inline size_t dm_slot_floats(int T, int D, int H) { return ((size_t)D + T + 1) * 2 * H; }

struct DmLds {
  float *xs, *h, *xn, *xi, *gi, *gb, *u, *lv, *ov, *dlv, *dov, *s, *A, *ds, *zs, *dzs, *qs, *sn, *cn, *dcn, *sc;
  int* valid;
};
enum { DM_SS, DM_N, DM_INNER, DM_SL, DM_SO, DM_CP };           // the scalars of sc

__device__ __forceinline__ DmLds dm_carve(float* lds, int T, int D, int H, int Nn) {
  const int Dp = mi_odd(D), Hp = mi_odd(2 * H);
  DmLds f;
  f.xs = lds;
  f.h = f.xs + (size_t)T * Dp;
  f.xn = f.h + (size_t)T * Hp;
  f.xi = f.xn + (size_t)Nn * Dp;
  f.gi = f.xi + Dp;
  f.gb = f.gi + Dp;
  f.u = f.gb + Dp;
  f.lv = f.u + Dp;
  f.ov = f.lv + Dp;
  f.dlv = f.ov + Dp;
  f.dov = f.dlv + Dp;
  f.s = f.dov + Dp;
  f.A = f.s + 2 * T;
  f.ds = f.A + 2 * T;
  f.valid = reinterpret_cast<int*>(f.ds + 2 * T);
  f.zs = reinterpret_cast<float*>(f.valid + T);
  f.dzs = f.zs + 2 * H;
  f.qs = f.dzs + 2 * H;
  f.sn = f.qs + H;
  f.cn = f.sn + Nn;
  f.dcn = f.cn + Nn;
  f.sc = f.dcn + Nn;
  return f;
}

__device__ __forceinline__ float dm_rs(float s) { return 1.f / sqrtf(fmaxf(s, DM_EPS)); }
__device__ __forceinline__ float dm_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
// sum_d (a[d] ra) (b[d] rb) by one wave, every lane gets it
__device__ __forceinline__ float dm_wdot(const float* a, float ra, const float* b, float rb, int n, int lane) {
  float s = 0.f;
  for (int d = lane; d < n; d += 64) s = fmaf(a[d] * ra, b[d] * rb, s);
  return group_sum<64>(s);
}

// Example b into LDS and, where given, its outputs.  Ends behind a barrier: every thread may read all of it.
__device__ __forceinline__ void dm_forward(const DmArgs& a, int64_t b, const DmLds& f, float* __restrict__ i2i,
                                           float* __restrict__ u2i, float* __restrict__ aux, int tid, bool& bad) {
  const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, H = a.H, H2 = 2 * H, Nn = a.Nn, Dp = mi_odd(D), Hp = mi_odd(H2);
  mi_gather<MI_NTHR>(a.embed, a.ld, a.V, a.series + b * T * a.C, T, a.C, a.E, f.xs, Dp, tid, bad, a.padding_index,
                     f.valid);
  mi_gather<MI_NTHR>(a.embed, a.ld, a.V, a.neg + b * Nn * a.C, Nn, a.C, a.E, f.xn, Dp, tid, bad);
  for (int d = tid; d < D; d += MI_NTHR) f.xi[d] = a.xi[b * D + d];
  for (int c = tid; c < H; c += MI_NTHR) f.qs[c] = a.q[b * H + c];
  __syncthreads();
  caps_project<false>(f.xs, Dp, a.We, T, D, H2, f.h, Hp, wave, lo, hi);
  __syncthreads();
  for (int i = tid; i < T * H2; i += MI_NTHR) {
    const int t = i / H2, c = i - t * H2;
    const float xw = f.h[t * Hp + c], pre = c < H ? f.qs[c] + xw : xw;
    f.h[t * Hp + c] = tanhf(pre + a.P[i]);
  }
  __syncthreads();
  for (int i = tid; i < 2 * T; i += MI_NTHR) {
    const int u = i / T, t = i - u * T;
    f.s[i] = mi_dot(f.zs + u * H, f.h + t * Hp + u * H, 1, H);
  }
  __syncthreads();
  if (wave < 2) {                                                // uniform over the wave
    const float* su = f.s + wave * T;
    float* Au = f.A + wave * T;
    float cnt = 0.f, ss = 0.f;
    for (int t = lane; t < T; t += 64) {
      cnt += f.valid[t] ? 1.f : 0.f;
      ss += f.valid[t] ? su[t] : 0.f;
    }
    cnt = group_sum<64>(cnt);
    ss = group_sum<64>(ss);
    caps_softmax_row(su, f.valid, Au, T, lane);
    if (cnt == 0.f)
      for (int t = lane; t < T; t += 64) Au[t] = 0.f;
    if (wave == 0 && lane == 0) {
      f.sc[DM_SS] = ss;
      f.sc[DM_N] = cnt;
      if (i2i) i2i[b * (D + 1) + D] = ss;
    }
  }
  __syncthreads();
  const int last = (int)f.sc[DM_N] - 1;
  for (int i = tid; i < 2 * D; i += MI_NTHR) {
    if (i < D) {
      const int d = i;
      const float o0 = mi_dot(f.A, f.xs + d, Dp, T);
      const float uv = mi_dot(f.A + T, f.xs + d, Dp, T);
      f.u[d] = uv;
      if (i2i) i2i[b * (D + 1) + d] = o0;
      if (u2i) u2i[b * (D + 1) + d] = uv;
    } else {
      const int d = i - D;
      f.lv[d] = last >= 0 ? f.A[T + last] * f.xs[last * Dp + d] : 0.f;
      f.ov[d] = last > 0 ? mi_dot(f.A + T, f.xs + d, Dp, last) : 0.f;
    }
  }
  __syncthreads();
  const float so = dm_wdot(f.ov, 1.f, f.ov, 1.f, D, lane), ro = dm_rs(so);
  if (wave == 0) {
    const float inner = dm_wdot(f.u, 1.f, f.xi, 1.f, D, lane);
    const float sl = dm_wdot(f.lv, 1.f, f.lv, 1.f, D, lane);
    const float cp = dm_wdot(f.lv, dm_rs(sl), f.ov, ro, D, lane);
    if (lane == 0) {
      f.sc[DM_INNER] = inner;
      f.sc[DM_SL] = sl;
      f.sc[DM_SO] = so;
      f.sc[DM_CP] = cp;
      if (u2i) u2i[b * (D + 1) + D] = inner;
    }
  }
  for (int j = wave; j < Nn; j += 4) {
    const float* xj = f.xn + j * Dp;
    const float sn = dm_wdot(xj, 1.f, xj, 1.f, D, lane);
    const float cn = dm_wdot(xj, dm_rs(sn), f.ov, ro, D, lane);
    if (lane == 0) {
      f.sn[j] = sn;
      f.cn[j] = cn;
    }
  }
  __syncthreads();
  if (aux && wave == 0) {
    float acc = 0.f;
    for (int j = lane; j < Nn; j += 64) acc += dm_softplus((1.f - f.cn[j]) * 0.5f);
    acc = group_sum<64>(acc);
    if (lane == 0) aux[b] = last >= 0 ? dm_softplus(-(1.f - f.sc[DM_CP]) * 0.5f) + acc : 0.f;
  }
}

__device__ __forceinline__ void dm_load_z(const DmArgs& a, const DmLds& f, int tid) {
  for (int i = tid; i < 2 * a.H; i += MI_NTHR) f.zs[i] = a.z[i];
}

__global__ __launch_bounds__(MI_NTHR) void dmr_fwd_kernel(DmArgs a, float* __restrict__ i2i, float* __restrict__ u2i,
                                                          float* __restrict__ aux, int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DmLds f = dm_carve(lds, a.T, a.D, a.H, a.Nn);
  bool bad = false;
  dm_load_z(a, f, threadIdx.x);
  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    dm_forward(a, b, f, i2i, u2i, aux, threadIdx.x, bad);
    __syncthreads();                                             // the next example overwrites all of it
  }
  if (bad && oob) *oob = 1;
}

// d cos(p, q) / dp[d] over the factor the caller multiplies in: rp (qh - c ph), or rp qh where the clamp holds sum p^2
__device__ __forceinline__ float dm_dcos(float sp, float rp, float ph, float qh, float c) {
  return rp * (sp >= DM_EPS ? qh - c * ph : qh);
}

// NB: 32 x 32 blocks of dWe per wave (block w, w + 4, ...): 1, 2, 4 or 8
template <int NB>
__global__ __launch_bounds__(MI_NTHR, NB <= 2 ? 2 : 1) void dmr_bwd_kernel(
    DmArgs a, const float* __restrict__ g_i2i, const float* __restrict__ g_u2i, const float* __restrict__ g_aux,
    float* __restrict__ gkeys, float* __restrict__ gneg, float* __restrict__ gitem, float* __restrict__ gq,
    float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, H = a.H, H2 = 2 * H, Nn = a.Nn, Dp = mi_odd(D), Hp = mi_odd(H2);
  const DmLds f = dm_carve(lds, T, D, H, Nn);
  const int nblk = ((D + 31) / 32) * ((H2 + 31) / 32);
  const bool held = nblk <= 4 * NB;                              // dWe stays in registers over the examples
  float* __restrict__ slotW = slots + (int64_t)blockIdx.x * dm_slot_floats(T, D, H);
  float* __restrict__ slotP = slotW + (size_t)D * H2;
  f32x16 sacc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) mb_zero(sacc[j]);
  bool bad = false;
  dm_load_z(a, f, tid);
  for (int i = tid; i < H2; i += MI_NTHR) f.dzs[i] = 0.f;

  for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
    const bool first = b == blockIdx.x;
    dm_forward(a, b, f, nullptr, nullptr, nullptr, tid, bad);
    const int last = (int)f.sc[DM_N] - 1;
    const float gss = g_i2i ? g_i2i[b * (D + 1) + D] : 0.f, gin = g_u2i ? g_u2i[b * (D + 1) + D] : 0.f;
    const float ga = (g_aux && last >= 0) ? g_aux[b] : 0.f;
    const float sl = f.sc[DM_SL], so = f.sc[DM_SO], cp = f.sc[DM_CP], rl = dm_rs(sl), ro = dm_rs(so);
    const float dcp = ga * (1.f - sigmoid_acc((1.f - cp) * 0.5f)) * 0.5f;
    for (int j = tid; j < Nn; j += MI_NTHR) f.dcn[j] = -ga * sigmoid_acc((1.f - f.cn[j]) * 0.5f) * 0.5f;
    __syncthreads();
    for (int d = tid; d < D; d += MI_NTHR) {
      const float lh = f.lv[d] * rl, oh = f.ov[d] * ro;
      f.gi[d] = g_i2i ? g_i2i[b * (D + 1) + d] : 0.f;
      f.gb[d] = (g_u2i ? g_u2i[b * (D + 1) + d] : 0.f) + gin * f.xi[d];
      f.dlv[d] = dcp * dm_dcos(sl, rl, lh, oh, cp);
      float dv = dcp * dm_dcos(so, ro, oh, lh, cp);
      for (int j = 0; j < Nn; ++j) {
        const float rn = dm_rs(f.sn[j]), nh = f.xn[j * Dp + d] * rn;
        dv = fmaf(f.dcn[j], dm_dcos(so, ro, oh, nh, f.cn[j]), dv);
        gneg[(b * Nn + j) * D + d] = f.dcn[j] * dm_dcos(f.sn[j], rn, nh, oh, f.cn[j]);
      }
      f.dov[d] = dv;
      gitem[b * D + d] = gin * f.u[d];
    }
    __syncthreads();
    for (int i = tid; i < 2 * T; i += MI_NTHR) {                 // dA
      const int u = i / T, t = i - u * T;
      const float* xr = f.xs + t * Dp;
      float acc = 0.f;
      if (u == 0) {
        acc = mi_dot(f.gi, xr, 1, D);
      } else {
        const float wl = t == last ? 1.f : 0.f, wo = t < last ? 1.f : 0.f;
        for (int d = 0; d < D; ++d) acc = fmaf(f.gb[d] + wl * f.dlv[d] + wo * f.dov[d], xr[d], acc);
      }
      f.ds[i] = acc;
    }
    __syncthreads();
    if (wave < 2) {                                              // the softmax, back
      const float* Au = f.A + wave * T;
      float* dsu = f.ds + wave * T;
      float dot = 0.f;
      for (int t = lane; t < T; t += 64) dot = fmaf(dsu[t], Au[t], dot);
      dot = group_sum<64>(dot);
      for (int t = lane; t < T; t += 64)
        dsu[t] = f.valid[t] ? Au[t] * (dsu[t] - dot) + (wave == 0 ? gss : 0.f) : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < H2; i += MI_NTHR)                      // dz += ds h: an element stays with its thread
      f.dzs[i] = f.dzs[i] + mi_dot(f.ds + (i / H) * T, f.h + i, Hp, T);
    __syncthreads();
    for (int i = tid; i < T * H2; i += MI_NTHR) {                // dh over h, and into the slot's dP
      const int t = i / H2, c = i - t * H2;
      const float hv = f.h[t * Hp + c];
      const float dh = f.ds[(c / H) * T + t] * f.zs[c] * (1.f - hv * hv);
      f.h[t * Hp + c] = dh;
      slotP[i] = first ? dh : slotP[i] + dh;
    }
    __syncthreads();
    for (int c = tid; c < H; c += MI_NTHR) {
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc += f.h[t * Hp + c];
      gq[b * H + c] = acc;
    }
    {                                                            // gkeys[b] = dh We^T + A0 gi + A1 gav
      const int ndb = (D + 31) / 32, ntile = (T + 31) / 32;
      float* __restrict__ gk = gkeys + b * T * D;
      for (int task = wave; task < ntile * ndb; task += 4) {
        const int tile = task / ndb, db = task - tile * ndb;
        const int t = tile * 32 + lo, n = db * 32 + lo;
        const bool tok = t < T, nok = n < D;
        const float* dr = f.h + (tok ? t : T - 1) * Hp;
        const float* __restrict__ Wr = a.We + (int64_t)(nok ? n : D - 1) * H2;
        f32x16 acc;
        mb_zero(acc);
        mi_mma(acc, H2, hi, [&](int k) { return tok ? dr[k] : 0.f; },
               [&](int k) { const float v = Wr[k]; return nok ? v : 0.f; });
        if (nok) {
          const float gi = f.gi[n], gb = f.gb[n], dl = f.dlv[n], dv = f.dov[n];
#pragma unroll
          for (int rr = 0; rr < 16; ++rr) {
            const int row = tile * 32 + mb_row(rr, hi);
            if (row < T) {
              const float gav = gb + (row == last ? dl : 0.f) + (row < last ? dv : 0.f);
              gk[(int64_t)row * D + n] = acc[rr] + f.A[row] * gi + f.A[T + row] * gav;
            }
          }
        }
      }
    }
    if (held) {
      caps_weight_grad<NB>(sacc, f.xs, Dp, f.h, Hp, T, D, H2, wave, lo, hi);
    } else {
      for (int blk0 = 0; blk0 < nblk; blk0 += 4 * NB) {
#pragma unroll
        for (int j = 0; j < NB; ++j) mb_zero(sacc[j]);
        caps_weight_grad<NB>(sacc, f.xs, Dp, f.h, Hp, T, D, H2, wave, lo, hi, blk0);
        caps_weight_store<NB>(sacc, slotW, D, H2, wave, lo, hi, blk0, !first);
      }
    }
    __syncthreads();                                             // the next example overwrites all of it
  }
  if (held) caps_weight_store<NB>(sacc, slotW, D, H2, wave, lo, hi);
  for (int i = tid; i < H2; i += MI_NTHR) slotP[(size_t)T * H2 + i] = f.dzs[i];
}

// blocks of dWe per wave: 1, 2, 4 or 8 (16 would spill beside what the backward keeps live), and the workgroups the
// chip holds at once by the registers of that instantiation
static int dm_nb(int D, int H) {
  const int nblk = ((D + 31) / 32) * ((2 * H + 31) / 32);
  return nblk <= 4 ? 1 : (nblk <= 8 ? 2 : (nblk <= 16 ? 4 : 8));
}
static int dm_grid(int64_t B, int D, int H) {
  const int nb = dm_nb(D, H), cap = nb <= 2 ? DM_GRID : (nb == 4 ? DM_GRID / 2 : DM_GRID / 4);
  return B < cap ? (int)B : cap;
}

static DmArgs dm_args(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B, int T,
                      const int64_t* neg, int Nn, const float* xi, const float* q, const float* P, const float* We,
                      const float* z, int H, int64_t pad) {
  return DmArgs{{embed, ld, V, series, B, pad, T, C, E, E * C, 2 * H, 1}, neg, xi, q, P, We, z, H, Nn};
}

}  // namespace

extern "C" size_t rec_dmr_lds_bytes(int T, int E, int C, int H, int Nn) {
  return dm_check(0, T, E, C, H, Nn) == REC_OK ? sizeof(float) * dm_lds_floats(T, E * C, H, Nn) : 0;
}

extern "C" size_t rec_dmr_scratch_bytes(int64_t B, int T, int E, int C, int H, int Nn) {
  if (dm_check(B, T, E, C, H, Nn) != REC_OK) return 0;
  return sizeof(float) * ((size_t)dm_grid(B, E * C, H) * dm_slot_floats(T, E * C, H) + 4);
}

extern "C" int rec_dmr_fwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                               int T, const int64_t* negatives, int Nn, const float* xi, const float* q, const float* P,
                               const float* We, const float* z, int H, int64_t padding_index, float* i2i, float* u2i,
                               float* aux, int* oob_flag, void* stream) {
  if (int rc = dm_check(B, T, E, C, H, Nn)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !negatives || !xi || !q || !P || !We || !z || !i2i || !u2i || !aux)
    return REC_E_ARG;
  if (B == 0) return REC_OK;
  const DmArgs a = dm_args(embed, ld, V, E, C, series, B, T, negatives, Nn, xi, q, P, We, z, H, padding_index);
  return caps_launch<dmr_fwd_kernel>(dim3(caps_fwd_grid(B)), MI_NTHR, sizeof(float) * dm_lds_floats(T, E * C, H, Nn),
                                     as_stream(stream), a, i2i, u2i, aux, oob_flag);
}

extern "C" int rec_dmr_bwd_f32(const float* embed, int64_t ld, int64_t V, int E, int C, const int64_t* series, int64_t B,
                               int T, const int64_t* negatives, int Nn, const float* xi, const float* q, const float* P,
                               const float* We, const float* z, int H, int64_t padding_index, const float* g_i2i,
                               const float* g_u2i, const float* g_aux, float* gkeys, float* gneg, float* gitem,
                               float* gq, float* dP, float* dWe, float* dz, void* scratch, size_t scratch_bytes,
                               void* stream) {
  if (int rc = dm_check(B, T, E, C, H, Nn)) return rc;
  if (ld < E || V <= 0 || !embed || !series || !negatives || !xi || !q || !P || !We || !z || !gkeys || !gneg ||
      !gitem || !gq || !dP || !dWe || !dz || !scratch)
    return REC_E_ARG;
  const int D = E * C, grid = dm_grid(B, D, H);
  const size_t slot = dm_slot_floats(T, D, H);
  if (scratch_bytes < sizeof(float) * (size_t)grid * slot) return REC_E_WORKSPACE;
  if (B == 0) return REC_OK;                                     // nothing is launched and nothing written
  hipStream_t st = as_stream(stream);
  const DmArgs a = dm_args(embed, ld, V, E, C, series, B, T, negatives, Nn, xi, q, P, We, z, H, padding_index);
  const size_t lds = sizeof(float) * dm_lds_floats(T, D, H, Nn);
  float* slots = static_cast<float*>(scratch);
  const auto launch = [&](auto nb) {
    return caps_launch<dmr_bwd_kernel<nb.value>>(dim3(grid), MI_NTHR, lds, st, a, g_i2i, g_u2i, g_aux, gkeys, gneg,
                                                 gitem, gq, slots);
  };
  const int nb = dm_nb(D, H);
  const int rc = nb == 1   ? launch(std::integral_constant<int, 1>{})
                 : nb == 2 ? launch(std::integral_constant<int, 2>{})
                 : nb == 4 ? launch(std::integral_constant<int, 4>{})
                           : launch(std::integral_constant<int, 8>{});
  if (rc) return rc;
  // below 2^31: T (2H|1) and (D|1) are bounded by the LDS fit and the limits
  return rec_slot_sum(REC_SLOTS_WAVE, (int)slot, grid, slots, {{dWe, dP, dz}, {D * 2 * H, T * 2 * H, 2 * H}}, st);
}
