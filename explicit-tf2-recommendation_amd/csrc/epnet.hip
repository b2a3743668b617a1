// EPNet lookup (the embedding stage of PEPNetLayer, 10.POSO/CustomLayers.py:415-457) on gfx950: the rows of F main ids and
// P personalisation ids out of ONE table, the main rows rescaled by F GateNUs of the personalisation rows, written as
// one buffer u [B, (F + P) E]:
//   pp = rows of ids[:, F:] flattened [P E]      gate_f = 2 sigmoid(relu(pp A_f + a_f) Bm_f + bm_f)  [E]
//   u[:, f E + e] = gate_f[e] table[ids[:, f]][e]            u[:, F E + k] = pp[k]
// so u is the towers' gate input and its leading F E columns their main input: nothing is concatenated afterwards.
// Gather-bound (F + P rows of E floats per example against ~770 flops per row at the default shape), so the mapping
// follows the rows: E adjacent lanes read one row (one 32-byte sector at E = 8), a workgroup of 256 threads owns 32
// examples, thread (example, field) runs the field's two tiny layers out of LDS -- the 32 lanes of a half wave share the
// field, so a weight is one broadcast read and an operand of [column][33] is read on 32 different banks.  The gate
// weights of the fields of a pass (all F of them at the default shape: ~15 KiB) are staged in LDS once per workgroup;
// shapes whose weights and operands pass 96 KiB walk the fields in several passes.
// Backward: the gates are recomputed from the ids (nothing but the ids is saved: the recompute is the forward's own
// arithmetic, the save would be F (Hg + E) floats per example written and read back).  Row gradients go to drows
// [B, F + P, E] for the de-duplicated sparse path; the weight gradients of a tile are summed over its examples in order
// and added into the workgroup's slot, whose owner walks its tiles in order; rec_slot_sum adds the slots.  No float
// atomics: bit-identical results run to run.
#include <math.h>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EP_NTHR = 256, EP_T = 32, EP_LD = 33;
constexpr int EP_MAXSLOTS = 256;                 // workgroups of a backward: each owns a slot of all weight gradients
constexpr size_t EP_LDS_BUDGET = 96 * 1024;

struct EpDims {
  int F, P, E, Hg;
  __host__ __device__ int PE() const { return P * E; }
  __host__ __device__ int WF() const { return PE() * Hg + Hg + Hg * E + E; }   // weights of one field
};

// fields of a pass and whether their weights are staged in LDS.  Rows of LDS ([.][33]): forward pps [PE] | hs [FC Hg];
// backward pps [PE] | dpps [PE] | hs [FC Hg] | dzs [FC Hg] | dps [FC E]; then FC WF floats of weights.
struct EpPlan {
  int FC, wlds;
  size_t lds;
};
static EpPlan ep_plan(const EpDims& d, int bwd) {
  const size_t fixed = sizeof(float) * EP_LD * (bwd ? 2 : 1) * d.PE();
  const size_t per_op = sizeof(float) * EP_LD * (bwd ? 2 * d.Hg + d.E : d.Hg), per_w = sizeof(float) * d.WF();
  EpPlan p{0, 1, 0};
  size_t fc = (EP_LDS_BUDGET - fixed) / (per_op + per_w);
  if (fc < 1) {
    p.wlds = 0;
    fc = (EP_LDS_BUDGET - fixed) / per_op;
  }
  const int passes = (int)((d.F + fc - 1) / fc);
  p.FC = (d.F + passes - 1) / passes;
  p.lds = fixed + p.FC * (per_op + (p.wlds ? per_w : 0));
  return p;
}

__device__ __forceinline__ int64_t ep_id(const int64_t* __restrict__ ids, int64_t at, int64_t V, int* oob) {
  int64_t id = ids[at];
  if (id < 0 || id >= V) {
    if (oob) *oob = 1;
    id = 0;
  }
  return id;
}

// the weights of fields f0 .. f0 + fc - 1, field-major: A_f [PE, Hg] | a_f [Hg] | Bm_f [Hg, E] | bm_f [E]
__device__ __forceinline__ void ep_stage(float* w, const float* __restrict__ A, const float* __restrict__ a,
                                         const float* __restrict__ Bm, const float* __restrict__ bm, const EpDims& d,
                                         int f0, int fc, int tid) {
  const int PEH = d.PE() * d.Hg, Hg = d.Hg, HE = d.Hg * d.E, E = d.E, WF = d.WF();
  for (int i = tid; i < fc * WF; i += EP_NTHR) {
    const int fl = i / WF, f = f0 + fl;
    int r = i - fl * WF;
    float v;
    if (r < PEH) v = A[(int64_t)f * PEH + r];
    else if ((r -= PEH) < Hg) v = a[f * Hg + r];
    else if ((r -= Hg) < HE) v = Bm[(int64_t)f * HE + r];
    else v = bm[f * E + (r - HE)];
    w[i] = v;
  }
}

struct EpW {
  const float *A, *a, *Bm, *bm;
};
template <bool WLDS>
__device__ __forceinline__ EpW ep_weights(const float* w, const float* __restrict__ A, const float* __restrict__ a,
                                          const float* __restrict__ Bm, const float* __restrict__ bm, const EpDims& d,
                                          int f, int fl) {
  const int PEH = d.PE() * d.Hg, HE = d.Hg * d.E;
  if (WLDS) {
    const float* p = w + fl * d.WF();
    return {p, p + PEH, p + PEH + d.Hg, p + PEH + d.Hg + HE};
  }
  return {A + (int64_t)f * PEH, a + f * d.Hg, Bm + (int64_t)f * HE, bm + f * d.E};
}

// the pp rows of a tile, k-major; the forward also writes them to u
__device__ __forceinline__ void ep_load_pp(float* pps, const float* __restrict__ table, int64_t V, int64_t ldt,
                                           const int64_t* __restrict__ ids, int64_t r0, int64_t B, const EpDims& d,
                                           float* __restrict__ u, int* oob, int tid) {
  const int PE = d.PE(), E = d.E, FP = d.F + d.P;
  for (int i = tid; i < EP_T * PE; i += EP_NTHR) {
    const int ex = i / PE, k = i - ex * PE, p = k / E, e = k - p * E;
    float v = 0.f;
    if (r0 + ex < B) {
      const int64_t id = ep_id(ids, (r0 + ex) * FP + d.F + p, V, oob);
      v = table[id * ldt + e];
      if (u) u[(r0 + ex) * FP * E + d.F * E + k] = v;
    }
    pps[k * EP_LD + ex] = v;
  }
}

// h_f = relu(pp A_f + a_f) of one (example, field) into hs[(fl Hg + j)][ex]
__device__ __forceinline__ void ep_hidden(const float* pps, float* hs, const EpW& w, const EpDims& d, int fl, int ex) {
  const int PE = d.PE(), Hg = d.Hg;
  for (int j = 0; j < Hg; ++j) {
    float acc = 0.f;
    for (int k = 0; k < PE; ++k) acc = fmaf(pps[k * EP_LD + ex], w.A[k * Hg + j], acc);
    hs[(fl * Hg + j) * EP_LD + ex] = fmaxf(acc + w.a[j], 0.f);
  }
}
__device__ __forceinline__ float ep_gate(const float* hs, const EpW& w, const EpDims& d, int fl, int ex, int e) {
  float acc = 0.f;
  for (int j = 0; j < d.Hg; ++j) acc = fmaf(hs[(fl * d.Hg + j) * EP_LD + ex], w.Bm[j * d.E + e], acc);
  return 2.f * sigmoid_acc(acc + w.bm[e]);
}

template <bool WLDS>
__global__ __launch_bounds__(EP_NTHR) void epnet_fwd_kernel(
    const float* __restrict__ table, int64_t V, int64_t ldt, const int64_t* __restrict__ ids,
    const float* __restrict__ A, const float* __restrict__ a, const float* __restrict__ Bm,
    const float* __restrict__ bm, int64_t B, EpDims d, int FC, float* __restrict__ u, int* __restrict__ oob) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, F = d.F, E = d.E, FP = d.F + d.P;
  float* pps = lds;
  float* hs = pps + d.PE() * EP_LD;
  float* wl = hs + FC * d.Hg * EP_LD;
  const int64_t tiles = (B + EP_T - 1) / EP_T;
  const bool one_pass = FC >= F;
  bool staged = false;
  for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const int64_t r0 = tl * EP_T;
    ep_load_pp(pps, table, V, ldt, ids, r0, B, d, u, oob, tid);
    for (int f0 = 0; f0 < F; f0 += FC) {
      const int fc = F - f0 < FC ? F - f0 : FC;
      if (WLDS && !(one_pass && staged)) {
        ep_stage(wl, A, a, Bm, bm, d, f0, fc, tid);
        staged = true;
      }
      __syncthreads();
      for (int it = tid; it < fc * EP_T; it += EP_NTHR) {
        const int ex = it & (EP_T - 1), fl = it >> 5, f = f0 + fl;
        const EpW w = ep_weights<WLDS>(wl, A, a, Bm, bm, d, f, fl);
        ep_hidden(pps, hs, w, d, fl, ex);
        if (r0 + ex < B) {
          const int64_t id = ep_id(ids, (r0 + ex) * FP + f, V, oob);
          const float* __restrict__ row = table + id * ldt;
          float* __restrict__ dst = u + ((r0 + ex) * FP + f) * E;
          for (int e = 0; e < E; ++e) dst[e] = ep_gate(hs, w, d, fl, ex, e) * row[e];
        }
      }
      __syncthreads();                           // the weights and pps are rewritten by the next pass / tile
    }
  }
}

template <bool WLDS>
__global__ __launch_bounds__(EP_NTHR) void epnet_bwd_kernel(
    const float* __restrict__ table, int64_t V, int64_t ldt, const int64_t* __restrict__ ids,
    const float* __restrict__ A, const float* __restrict__ a, const float* __restrict__ Bm,
    const float* __restrict__ bm, const float* __restrict__ du, int64_t B, EpDims d, int FC, int64_t per,
    float* __restrict__ drows, float* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, F = d.F, E = d.E, Hg = d.Hg, PE = d.PE(), FP = d.F + d.P, WF = d.WF();
  const int PEH = PE * Hg, HE = Hg * E;
  float* pps = lds;
  float* dpps = pps + PE * EP_LD;
  float* hs = dpps + PE * EP_LD;
  float* dzs = hs + FC * Hg * EP_LD;
  float* dps = dzs + FC * Hg * EP_LD;
  float* wl = dps + FC * E * EP_LD;
  float* __restrict__ slot = slots + (int64_t)blockIdx.x * F * WF;   // dA [F PE Hg] | da [F Hg] | dBm [F Hg E] | dbm [F E]
  const int64_t tiles = (B + EP_T - 1) / EP_T;
  const int64_t t0 = (int64_t)blockIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
  const bool one_pass = FC >= F;
  bool staged = false;
  for (int64_t tl = t0; tl < t1; ++tl) {
    const int64_t r0 = tl * EP_T;
    const bool first = tl == t0;
    ep_load_pp(pps, table, V, ldt, ids, r0, B, d, nullptr, nullptr, tid);
    for (int i = tid; i < EP_T * PE; i += EP_NTHR) dpps[(i >> 5) * EP_LD + (i & 31)] = 0.f;
    for (int f0 = 0; f0 < F; f0 += FC) {
      const int fc = F - f0 < FC ? F - f0 : FC;
      if (WLDS && !(one_pass && staged)) {
        ep_stage(wl, A, a, Bm, bm, d, f0, fc, tid);
        staged = true;
      }
      __syncthreads();
      for (int it = tid; it < fc * EP_T; it += EP_NTHR) {
        const int ex = it & (EP_T - 1), fl = it >> 5, f = f0 + fl;
        const EpW w = ep_weights<WLDS>(wl, A, a, Bm, bm, d, f, fl);
        ep_hidden(pps, hs, w, d, fl, ex);
        if (r0 + ex < B) {
          const int64_t id = ep_id(ids, (r0 + ex) * FP + f, V, nullptr);
          const float* __restrict__ row = table + id * ldt;
          const float* __restrict__ duc = du + ((r0 + ex) * FP + f) * E;
          float* __restrict__ dr = drows + ((r0 + ex) * FP + f) * E;
          for (int e = 0; e < E; ++e) {
            const float gt = ep_gate(hs, w, d, fl, ex, e), dv = duc[e];
            dr[e] = dv * gt;
            dps[(fl * E + e) * EP_LD + ex] = (dv * row[e]) * (gt * (1.f - 0.5f * gt));
          }
        } else {
          for (int e = 0; e < E; ++e) dps[(fl * E + e) * EP_LD + ex] = 0.f;
        }
        for (int j = 0; j < Hg; ++j) {
          float acc = 0.f;
          for (int e = 0; e < E; ++e) acc = fmaf(dps[(fl * E + e) * EP_LD + ex], w.Bm[j * E + e], acc);
          dzs[(fl * Hg + j) * EP_LD + ex] = hs[(fl * Hg + j) * EP_LD + ex] > 0.f ? acc : 0.f;
        }
      }
      __syncthreads();
      for (int o = tid; o < fc * WF; o += EP_NTHR) {       // the tile's weight gradients, examples in order
        const int fl = o / WF, f = f0 + fl;
        int r = o - fl * WF, at;
        const float *p, *q = nullptr;
        if (r < PEH) {
          p = pps + (r / Hg) * EP_LD;
          q = dzs + (fl * Hg + r % Hg) * EP_LD;
          at = f * PEH + r;
        } else if ((r -= PEH) < Hg) {
          p = dzs + (fl * Hg + r) * EP_LD;
          at = F * PEH + f * Hg + r;
        } else if ((r -= Hg) < HE) {
          p = hs + (fl * Hg + r / E) * EP_LD;
          q = dps + (fl * E + r % E) * EP_LD;
          at = F * (PEH + Hg) + f * HE + r;
        } else {
          r -= HE;
          p = dps + (fl * E + r) * EP_LD;
          at = F * (PEH + Hg + HE) + f * E + r;
        }
        float s = 0.f;
        for (int ex = 0; ex < EP_T; ++ex) s += q ? p[ex] * q[ex] : p[ex];
        slot[at] = first ? s : slot[at] + s;
      }
      for (int i = tid; i < EP_T * PE; i += EP_NTHR) {     // dpp += dz_f A_f^T over the fields of the pass
        const int ex = i & 31, k = i >> 5;
        float acc = dpps[k * EP_LD + ex];
        for (int fl = 0; fl < fc; ++fl) {
          const EpW w = ep_weights<WLDS>(wl, A, a, Bm, bm, d, f0 + fl, fl);
          for (int j = 0; j < Hg; ++j) acc = fmaf(dzs[(fl * Hg + j) * EP_LD + ex], w.A[k * Hg + j], acc);
        }
        dpps[k * EP_LD + ex] = acc;
      }
      __syncthreads();
    }
    for (int i = tid; i < EP_T * PE; i += EP_NTHR) {
      const int ex = i / PE, k = i - ex * PE;
      if (r0 + ex < B) drows[((r0 + ex) * FP + F) * E + k] = du[(r0 + ex) * FP * E + F * E + k] + dpps[k * EP_LD + ex];
    }
    __syncthreads();                             // pps and dpps are rewritten by the next tile
  }
}

static int ep_shape(int64_t B, int64_t V, int64_t ldt, int F, int P, int E, int Hg) {
  if (B < 0 || V < 1 || F < 1 || P < 1 || E < 1 || Hg < 1 || ldt < E) return REC_E_ARG;
  if (F > REC_MASKNET_MAX_F || E > REC_MASKNET_MAX_E || Hg > REC_MASKNET_MAX_E || (int64_t)P * E > REC_MASKNET_MAX_O ||
      ((int64_t)F + P) * E > REC_MASKNET_MAX_D || B >= ((int64_t)1 << 31))
    return REC_E_UNSUPPORTED;
  return REC_OK;
}

static int64_t ep_slots(int64_t B, int64_t* per) {
  const int64_t tiles = ceil_div64(B, EP_T);
  *per = ceil_div64(tiles, EP_MAXSLOTS);
  return ceil_div64(tiles, *per);
}

}  // namespace

extern "C" size_t rec_epnet_lookup_scratch_bytes(int64_t B, int F, int P, int E, int Hg) {
  if (ep_shape(B, 1, E, F, P, E, Hg) != REC_OK) return 0;
  int64_t per = 1;
  const int64_t nslot = B > 0 ? ep_slots(B, &per) : 1;
  return sizeof(float) * ((size_t)nslot * F * EpDims{F, P, E, Hg}.WF() + 4);
}

extern "C" int rec_epnet_lookup_fwd_f32(const float* table, int64_t V, int64_t ld, const int64_t* ids, const float* A,
                                        const float* a, const float* Bm, const float* bm, int64_t B, int F, int P, int E,
                                        int Hg, float* u, int* oob_flag, void* stream) {
  if (int rc = ep_shape(B, V, ld, F, P, E, Hg)) return rc;
  if (B == 0) return REC_OK;
  if (!table || !ids || !A || !a || !Bm || !bm || !u) return REC_E_ARG;
  const EpDims d{F, P, E, Hg};
  const EpPlan p = ep_plan(d, 0);
  const int64_t tiles = ceil_div64(B, EP_T);
  const dim3 grid((unsigned)(tiles < 2048 ? tiles : 2048));
  if (p.wlds) {
    if (hipError_t err = rec_allow_lds<epnet_fwd_kernel<true>>(EP_LDS_BUDGET)) return (int)err;
    hipLaunchKernelGGL(epnet_fwd_kernel<true>, grid, dim3(EP_NTHR), p.lds, as_stream(stream), table, V, ld, ids, A, a,
                       Bm, bm, B, d, p.FC, u, oob_flag);
  } else {
    if (hipError_t err = rec_allow_lds<epnet_fwd_kernel<false>>(EP_LDS_BUDGET)) return (int)err;
    hipLaunchKernelGGL(epnet_fwd_kernel<false>, grid, dim3(EP_NTHR), p.lds, as_stream(stream), table, V, ld, ids, A, a,
                       Bm, bm, B, d, p.FC, u, oob_flag);
  }
  REC_LAUNCH_CHECK();
  return REC_OK;
}

extern "C" int rec_epnet_lookup_bwd_f32(const float* table, int64_t V, int64_t ld, const int64_t* ids, const float* A,
                                        const float* a, const float* Bm, const float* bm, const float* du, int64_t B,
                                        int F, int P, int E, int Hg, float* drows, float* dA, float* da, float* dBm,
                                        float* dbm, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = ep_shape(B, V, ld, F, P, E, Hg)) return rc;
  if (B == 0) return REC_OK;
  if (!table || !ids || !A || !a || !Bm || !bm || !du || !drows || !dA || !da || !dBm || !dbm || !workspace)
    return REC_E_ARG;
  const EpDims d{F, P, E, Hg};
  const EpPlan p = ep_plan(d, 1);
  int64_t per = 1;
  const int64_t nslot = ep_slots(B, &per);
  const int n = F * d.WF();
  if (workspace_bytes < sizeof(float) * (size_t)nslot * n) return REC_E_WORKSPACE;
  float* slots = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  if (p.wlds) {
    if (hipError_t err = rec_allow_lds<epnet_bwd_kernel<true>>(EP_LDS_BUDGET)) return (int)err;
    hipLaunchKernelGGL(epnet_bwd_kernel<true>, dim3((unsigned)nslot), dim3(EP_NTHR), p.lds, st, table, V, ld, ids, A, a,
                       Bm, bm, du, B, d, p.FC, per, drows, slots);
  } else {
    if (hipError_t err = rec_allow_lds<epnet_bwd_kernel<false>>(EP_LDS_BUDGET)) return (int)err;
    hipLaunchKernelGGL(epnet_bwd_kernel<false>, dim3((unsigned)nslot), dim3(EP_NTHR), p.lds, st, table, V, ld, ids, A,
                       a, Bm, bm, du, B, d, p.FC, per, drows, slots);
  }
  REC_LAUNCH_CHECK();
  const int PEH = d.PE() * Hg;
  return rec_slot_sum(REC_SLOTS_WAVE, n, (int)nslot, slots, {{dA, da, dBm, dbm}, {F * PEH, F * Hg, F * Hg * E, F * E}},
                      st);
}
