// Post launch of the fused DeepFM train step (2.FM/CustomLayers.py:279-308 under 2.FM/ModelManager.py:171-177): what
// is left after the main kernel of deepfm_fused3.hip has written gz, the IndexedSlices value rows and the per-workgroup
// partials of the dense gradients into the workspace of deepfm_fused.h.  ONE launch, two jobs side by side:
//
//   reduction      the fixed-order sum of the per-workgroup partials (dK0, the SMALL block: dK1, biases, loss) over the
//                  ~210 workgroups of a step
//   segment sums   the de-duplicated gradient of both tables over the plan of colsort.hip.  Direct mode
//                  (deepfm_post_direct_kernel: the plan existed before the main kernel, which wrote the value row of
//                  every run's head straight to the run's slot) finishes runs of more than one lookup, unique ids,
//                  first-order rows and the zero-padded tail, optionally with the lazy (touched-rows) Adam update of
//                  every finished row.  deepfm_post_kernel: the plain form, every run summed here (the row-sharded step).
//
// Also here: the exact lazy evaluation of Keras' Adam sweep (adam_keras_catchup_kernel: the steps a row skipped are
// replayed before a batch reads it; the flush brings every row up to date).
//
// ONE entry point, rec_deepfm_fused_post_f32: slot_map, direct and the lazy-Adam group are independent options and reach
// the kernels as the ColSegArgs fields they are.  (ColSegArgs::lr_t is filled by the kernel from lr_t_dev; `packed` is
// slot_map != null.)
//
// Everything is deterministic (no float atomics): per-workgroup partials + fixed-order reductions, stable sort keys.
#include "deepfm_fused.h"
#include <math.h>

namespace {

constexpr int LD = 32;        // fused row stride (floats)

// fixed-order sum of the per-workgroup partials.  1024 threads = 16 slices x 64 lanes; lane owns 4 consecutive
// outputs (float4), slice q adds workgroups q, q+16, q+32, ... (independent 16-B loads), then the 16 slices are
// added in slice order through LDS.
struct ReduceArgs {
  const float* dK0part; const float* small; int nwg; int D; int64_t B;
  float* dK0; float* dK1; float* db0; float* db1; float* dK2; float* db2; float* dbias; float* loss;
};

// 1024 threads = 64 slices x 16 lanes; a lane owns 4 consecutive outputs (float4), slice q adds the partials of
// workgroups q, q+64, q+128, ... (all of them in flight before the first add), then the 64 slices meet in LDS and are
// added in a fixed two-level order.  16 float4 columns per workgroup -> 208 + 5 workgroups at F = 26: with 64 columns
// per workgroup (round 1) only 54 CUs shared the 13.6 MB of partials, 256 KB each, and the reduction took ~10 us.
constexpr int RC = 16;         // float4 columns per reduce workgroup
constexpr int RS = 64;         // slices
__host__ __device__ inline int reduce_blocks(int D) {
  return (int)(((int64_t)D * U1 / 4 + RC - 1) / RC) + (SMALL / 4 + RC - 1) / RC;
}

__device__ __forceinline__ void reduce_body(const ReduceArgs& r, int bidx) {
  const float* __restrict__ dK0part = r.dK0part;
  const float* __restrict__ small = r.small;
  const int nwg = r.nwg, D = r.D;
  const int64_t B = r.B;
  float* __restrict__ dK0 = r.dK0; float* __restrict__ dK1 = r.dK1; float* __restrict__ db0 = r.db0;
  float* __restrict__ db1 = r.db1; float* __restrict__ dK2 = r.dK2; float* __restrict__ db2 = r.db2;
  float* __restrict__ dbias = r.dbias; float* __restrict__ loss = r.loss;
  __shared__ float4 red[RS][RC];
  __shared__ float4 red2[8][RC];
  const int lane = threadIdx.x & (RC - 1), q = threadIdx.x / RC;
  const int64_t n0 = (int64_t)D * U1;                  // multiple of 4
  const int nb0 = (int)((n0 / 4 + RC - 1) / RC);       // blocks that cover dK0
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t e4 = 0;
  const bool is_small = bidx >= nb0;
  const float* src;
  int64_t stride;
  bool in = false;
  if (!is_small) {
    e4 = (int64_t)bidx * RC + lane;                    // float4 index into dK0
    in = e4 * 4 < n0;
    src = dK0part + e4 * 4;
    stride = n0;
  } else {
    e4 = (int64_t)(bidx - nb0) * RC + lane;            // float4 index into the SMALL block
    in = e4 * 4 < SMALL;
    src = small + e4 * 4;
    stride = SMALL;
  }
  if (in) {
    int w = q;
    for (; w + 3 * RS < nwg; w += 4 * RS) {
      float4 x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const float4*>(src + (int64_t)(w + RS * j) * stride);
#pragma unroll
      for (int j = 0; j < 4; ++j) { acc.x += x[j].x; acc.y += x[j].y; acc.z += x[j].z; acc.w += x[j].w; }
    }
    for (; w < nwg; w += RS) {
      float4 x = *reinterpret_cast<const float4*>(src + (int64_t)w * stride);
      acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
    }
  }
  red[q][lane] = acc;
  __syncthreads();
  if (q < 8) {                                         // slices 8q .. 8q+7, in order
    float4 s = red[8 * q][lane];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      float4 x = red[8 * q + k][lane];
      s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
    }
    red2[q][lane] = s;
  }
  __syncthreads();
  if (q != 0) return;
  float4 s = red2[0][lane];
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    float4 x = red2[k][lane];
    s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
  }
  if (!is_small) {
    if (e4 * 4 < n0) *reinterpret_cast<float4*>(dK0 + e4 * 4) = s;
    return;
  }
  if (e4 * 4 >= SMALL) return;
  float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int k = (int)(e4 * 4) + i;
    if (k < SM_DB0) dK1[k - SM_DK1] = sv[i];
    else if (k < SM_DB1) db0[k - SM_DB0] = sv[i];
    else if (k < SM_DK2) db1[k - SM_DB1] = sv[i];
    else if (k < SM_DB2) dK2[k - SM_DK2] = sv[i];
    else if (k == SM_DB2) { db2[0] = sv[i]; dbias[0] = sv[i]; }
    else if (k == SM_LOSS) loss[0] = sv[i] / (float)B;
  }
}

// ------------------------------------------------------------------------------------------------
// segment sums of both tables + global compaction.  One lane group (4 lanes x float4) per (column, local run).
// Long runs: the first 16 rows per group directly; what is left of a long run is summed by the whole wave.
// ------------------------------------------------------------------------------------------------
struct ColSegArgs {
  const float4* vals; const float* gz; const int32_t* perm; const int64_t* col_uid; const int32_t* col_seg;
  const int32_t* col_nu; int64_t B; int F; int64_t* uniq_ids; float4* g_embed; float* g_w; int64_t* n_uniq; int packed;
  // lazy (touched-rows) Adam applied to a row the moment its gradient is final (direct-mode post launch only; table ==
  // null: off).  table: fused rows [V, 32] = [embed 16 | w | pad]; m_e, v_e [V,16]; m_w, v_w [V]
  float* table; float* m_e; float* v_e; float* m_w; float* v_w; int64_t V; float lr_t, b1, b2, eps;
  // fixed-capacity exchange layout (sharded step): slot of every unique id (index = its rank in the batch's ascending
  // list) inside the [owners x capacity] send buffer; null = the compact list itself
  const int32_t* slot_map;
  // bias-corrected step size of the lazy Adam read from device memory (advanced by the main kernel's launch): the train
  // step then holds no per-step host scalar and can be replayed from a hipGraph; null = lr_t above
  const float* lr_t_dev;
  // row strides (floats) of m_e / v_e and of m_w / v_w: 16 and 1 for dense state arrays; 32 and 32 when the state is
  // packed beside the rows ([m 16 | v 16] in one 128-byte row, m_w / v_w in the padding of the table row) so that a
  // touched row costs two line requests instead of five or six
  int64_t ldm, ldw;
  // exact lazy evaluation of Keras' dense sweep (rec_adam_keras_catchup_f32): last[row] = the step whose update the row
  // holds; a touched row holds step *step_dev afterwards.  null: plain touched-rows Adam
  int32_t* last; const int64_t* step_dev;
};

// m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2 ; var <- var - lr_t m / (sqrt(v) + eps)   (rec_adam_rows_f32's formula:
// adam_touch of common.h, rounding pinned, the same bits in every kernel)
__device__ __forceinline__ void adam_chunk(const ColSegArgs& k, int64_t id, int c, const float4& g) {
  float4* vp = reinterpret_cast<float4*>(k.table + id * LD) + c;
  float4* mp = reinterpret_cast<float4*>(k.m_e + id * k.ldm) + c;
  float4* qp = reinterpret_cast<float4*>(k.v_e + id * k.ldm) + c;
  float4 x = *vp, m = *mp, v = *qp;
  adam_touch(x.x, m.x, v.x, g.x, k.lr_t, k.b1, k.b2, k.eps);
  adam_touch(x.y, m.y, v.y, g.y, k.lr_t, k.b1, k.b2, k.eps);
  adam_touch(x.z, m.z, v.z, g.z, k.lr_t, k.b1, k.b2, k.eps);
  adam_touch(x.w, m.w, v.w, g.w, k.lr_t, k.b1, k.b2, k.eps);
  *vp = x; *mp = m; *qp = v;
}
__device__ __forceinline__ void adam_w(const ColSegArgs& k, int64_t id, float g) {
  float x = k.table[id * LD + E16], m = k.m_w[id * k.ldw], v = k.v_w[id * k.ldw];
  adam_touch(x, m, v, g, k.lr_t, k.b1, k.b2, k.eps);
  k.table[id * LD + E16] = x; k.m_w[id * k.ldw] = m; k.v_w[id * k.ldw] = v;
}

__device__ __forceinline__ void colseg_body(const ColSegArgs& k, int bidx) {
  const float4* __restrict__ vals = k.vals;
  const float* __restrict__ gz = k.gz;
  const int32_t* __restrict__ perm = k.perm;
  const int64_t* __restrict__ col_uid = k.col_uid;
  const int32_t* __restrict__ col_seg = k.col_seg;
  const int32_t* __restrict__ col_nu = k.col_nu;
  const int64_t B = k.B;
  const int F = k.F;
  int64_t* __restrict__ uniq_ids = k.uniq_ids;
  float4* __restrict__ g_embed = k.g_embed;
  float* __restrict__ g_w = k.g_w;
  int64_t* __restrict__ n_uniq = k.n_uniq;
  const int packed = k.packed;
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = tid & 3;                       // float4 chunk of the 16-float row
  const int64_t grp = ((int64_t)bidx * blockDim.x + tid) >> 2;     // (f, u_local) = (grp / B, grp % B)
  const int f = (int)(grp / B);
  int u = (int)(grp - (int64_t)f * B);
  if ((B & 63) == 0) {
    // Long runs (a hot id) are worked off by a wave one after the other.  When hot ids are neighbours (the synthetic
    // Zipf draws make the smallest ids of a field the frequent ones) they would all fall to the same wave: deal the
    // runs out so that a wave (16 lane groups) takes four consecutive runs from each quarter of the column -- the
    // first 64 runs then go to 16 different waves, a workgroup still writes 4 KB pieces.  Measured (B=8192, F=26):
    // Zipf(1.05) 113 -> 101 us/step, uniform unchanged.  (Summing a long run with the whole workgroup instead:
    // Zipf 89 us but uniform +5 us -- not taken.)
    const int w = u >> 4, g = u & 15;
    u = (g >> 2) * (int)(B >> 2) + 4 * w + (g & 3);
  }
  const bool in_range = f < F;
  __shared__ int nu_s[REC_MAX_COLS];
  if (tid < F) nu_s[tid] = col_nu[tid];
  __syncthreads();
  int64_t before = 0, total = 0;               // unique ids in earlier columns / in all columns
  for (int q = 0; q < F; ++q) {
    int nq = nu_s[q];
    if (q < f) before += nq;
    total += nq;
  }
  const int nu = in_range ? nu_s[f] : 0;
  const bool live = in_range && u < nu;
  int s0 = 0, s1 = 0;
  if (live) {
    s0 = col_seg[(int64_t)f * (B + 1) + u];
    s1 = col_seg[(int64_t)f * (B + 1) + u + 1];
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float accw = 0.f;
  const int32_t* pf = perm + (int64_t)f * B;
  int s_end = s1 < s0 + 16 ? s1 : s0 + 16;
  for (int s = s0; s < s_end; ++s) {
    int64_t b = pf[s];
    float4 x = vals[(b * F + f) * 4 + c];
    acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
    accw += gz[b];
  }
  // long runs, one at a time, by all 16 lane groups of the wave (wave-uniform loop)
  unsigned long long longm = __ballot(live && (s1 - s0) > 16 && c == 0);
  while (longm) {
    int src = __ffsll((long long)longm) - 1;   // lane (c == 0) of the group that owns the run
    longm &= longm - 1;
    int rs0 = __shfl(s0, src, 64) + 16, rs1 = __shfl(s1, src, 64);
    int rf = __shfl(f, src, 64);
    const int32_t* rp = perm + (int64_t)rf * B;
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f);
    float pw = 0.f;
#pragma unroll 4
    for (int s = rs0 + (lane >> 2); s < rs1; s += 16) {    // independent loads: several iterations in flight
      int64_t b = rp[s];
      float4 x = vals[(b * F + rf) * 4 + c];
      pa.x += x.x; pa.y += x.y; pa.z += x.z; pa.w += x.w;
      pw += gz[b];
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {         // fixed butterfly over the 16 groups (same chunk lanes)
      pa.x += __shfl_xor(pa.x, o, 64); pa.y += __shfl_xor(pa.y, o, 64);
      pa.z += __shfl_xor(pa.z, o, 64); pa.w += __shfl_xor(pa.w, o, 64);
      pw += __shfl_xor(pw, o, 64);
    }
    if ((lane & ~3) == src) {
      acc.x += pa.x; acc.y += pa.y; acc.z += pa.z; acc.w += pa.w;
      accw += pw;
    }
  }
  if (!in_range) return;
  int64_t dst;
  int64_t idv;
  if (live) {
    dst = before + u;
    idv = col_uid[(int64_t)f * B + u];
    if (k.slot_map) dst = k.slot_map[dst];
  } else {
    if (k.slot_map) return;                      // the unused slots of a send buffer are never read by the owner
    // padded tail: slot = total + rank among the non-live groups; id = the smallest id of column 0
    dst = total + ((int64_t)f * B - before) + (u - nu);
    idv = col_uid[0];
    acc = make_float4(0.f, 0.f, 0.f, 0.f);
    accw = 0.f;
  }
  if (packed) {                                  // rows of 20 floats: [embed 16 | w | 0 0 0] (one exchange buffer)
    g_embed[dst * 5 + c] = acc;
    if (c == 0) g_embed[dst * 5 + 4] = make_float4(accw, 0.f, 0.f, 0.f);
  } else {
    g_embed[dst * 4 + c] = acc;
    if (c == 0) g_w[dst] = accw;
  }
  if (c == 0 && uniq_ids) uniq_ids[dst] = idv;
  if (grp == 0 && c == 0 && n_uniq) *n_uniq = total;
}


// ---- direct mode: what is left for the launch after the fused kernel.  ONE LANE per run (slot) of the plan:
//   a run of one lookup (almost all of them with uniform ids): g_w = gz of that lookup, uniq_ids = its id -- coalesced
//     stores, the value row is already in place;
//   a pair: the lane adds the second member's value row to the head's row itself;
//   a run of 3..FIX_SHORT lookups: four lanes (one 16-byte chunk each), 16 runs of the wave at a time, members in order;
//   a run of up to FIX_HUGE: the whole wave adds it, 16 members x 4 float4 chunks per round, fixed butterfly over the rows;
//   longer ones (Zipf heads): the whole workgroup, partial rows of its 16 waves added in wave order;
//   slots beyond the column's runs: the zero-padded tail.
constexpr int FIX_T = 1024, FIX_HUGE = 128, FIX_SHORT = 17, FIX_SKEW = 256;
// slot t of a column (thread order) -> run u, twice.
// fix_deal: the mapping of the FAST path (ids, single lookups, pairs, the padded tail -- nearly everything, and all of it
// coalesced stores): a wave takes 4 consecutive runs from each sixteenth of the column, so that plan words arrive and ids
// leave as 16-byte pieces, and a workgroup owns whole lines of uniq_ids / g_w.  (Interleaving the waves of different
// workgroups here cost 2.3 us with uniform ids: every line of the outputs was then written in pieces by four CUs.)
// fix_spread: the mapping under which the runs of MORE THAN TWO members are looked at a second time and summed: lane l of
// the column's wave w takes run l * (B / 64) + w -- the hot ids of a field, neighbours at the head of the column with
// the synthetic Zipf draws, fall to different waves (a wave adds its long runs one after the other).  Read-only plan
// words, scattered row stores either way.
__device__ __forceinline__ int fix_deal(int t, int64_t B) {
  if ((B & 63) != 0) return t;
  return ((t & 63) >> 2) * (int)(B >> 4) + 4 * (t >> 6) + (t & 3);
}
__device__ __forceinline__ int fix_spread(int t, int64_t B) {
  if ((B & 63) != 0) return t;
  return (t & 63) * (int)(B >> 6) + (t >> 6);
}
// lanes 4g .. 4g+3 get the lane index of the g-th set bit of mask (-1: fewer than g+1 bits).  mask is wave-uniform: the
// scan runs on the scalar unit
__device__ __forceinline__ int fix_group_src(unsigned long long mask, int lane) {
  int src = -1;
  const int g = lane >> 2;
  for (int i = 0; i < 16 && mask; ++i) {
    const int sl = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    if (g == i) src = sl;
  }
  return src;
}
__device__ __forceinline__ void fixup_body(const ColSegArgs& k_in, int bidx) {
  ColSegArgs k = k_in;
  if (k.lr_t_dev) k.lr_t = *k.lr_t_dev;
  const float4* __restrict__ vals = k.vals;
  const float* __restrict__ gz = k.gz;
  const int64_t B = k.B;
  const int F = k.F;
  float4* __restrict__ g_embed = k.g_embed;
  const int tid = threadIdx.x, lane = tid & 63;
  const int per_col = (int)((B + FIX_T - 1) / FIX_T);           // workgroups per column
  const int f = bidx / per_col;
  const int t = (bidx - f * per_col) * FIX_T + tid;             // slot of the column before the deal
  const int u = fix_deal(t, B);
  __shared__ int nu_s[REC_MAX_COLS];
  // runs of more than FIX_HUGE members (Zipf heads: the hottest id of a column holds ~10 % of its lookups) are left to
  // the WHOLE workgroup: at most B / FIX_HUGE <= 128 of them exist in a column
  __shared__ int huge_n, huge_s0[128], huge_s1[128], huge_u[128];
  __shared__ float huge_gz[128];
  __shared__ float4 hpart[FIX_T / 64][4];
  __shared__ float hw_s[FIX_T / 64];
  if (tid < F) nu_s[tid] = k.col_nu[tid];
  if (tid == 0) huge_n = 0;
  __syncthreads();
  int64_t before = 0, total = 0;
  for (int q = 0; q < F; ++q) {
    const int nq = nu_s[q];
    if (q < f) before += nq;
    total += nq;
  }
  const int nu = nu_s[f];
  const bool in_col = t < B;
  const bool live = in_col && u < nu;
  const int32_t* pf = k.perm + (int64_t)f * B;
  int s0 = 0, s1 = 0;
  if (live) {
    s0 = k.col_seg[(int64_t)f * (B + 1) + u];
    s1 = k.col_seg[(int64_t)f * (B + 1) + u + 1];
  }
  const int len = s1 - s0;
  const int64_t dst = before + u;
  const bool adam = k.table != nullptr;
  float accw = 0.f;                                             // gz of the run's head
  if (live) {
    accw = gz[pf[s0]];
    const int64_t id = k.col_uid[(int64_t)f * B + u];
    if (len == 2) {                                             // a pair (nearly every multi-member run of a uniform batch):
      const int64_t b2 = pf[s0 + 1];                            // this lane alone, two dependent round trips
      const float4* r2 = vals + (b2 * F + f) * 4;
      float4 a0 = g_embed[dst * 4], a1 = g_embed[dst * 4 + 1], a2 = g_embed[dst * 4 + 2], a3 = g_embed[dst * 4 + 3];
      const float4 x0 = r2[0], x1 = r2[1], x2 = r2[2], x3 = r2[3];
      a0.x += x0.x; a0.y += x0.y; a0.z += x0.z; a0.w += x0.w;
      a1.x += x1.x; a1.y += x1.y; a1.z += x1.z; a1.w += x1.w;
      a2.x += x2.x; a2.y += x2.y; a2.z += x2.z; a2.w += x2.w;
      a3.x += x3.x; a3.y += x3.y; a3.z += x3.z; a3.w += x3.w;
      g_embed[dst * 4] = a0; g_embed[dst * 4 + 1] = a1; g_embed[dst * 4 + 2] = a2; g_embed[dst * 4 + 3] = a3;
      k.g_w[dst] = accw + gz[b2];
    }
    if (len == 1) k.g_w[dst] = accw;
    k.uniq_ids[dst] = id;
  } else if (in_col) {
    // padded tail: slot = total + rank among the column's unused slots; id = the smallest id of column 0, zero rows
    const int64_t d2 = total + ((int64_t)f * B - before) + (u - nu);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    g_embed[d2 * 4] = z; g_embed[d2 * 4 + 1] = z; g_embed[d2 * 4 + 2] = z; g_embed[d2 * 4 + 3] = z;
    k.g_w[d2] = 0.f;
    k.uniq_ids[d2] = k.col_uid[0];
  }
  // ---- runs of more than two members: the second look (fix_spread) -- for a column with more than FIX_SKEW lookups
  // beyond the first of their runs; a column without (uniform ids: ~90 pairs) has next to nothing to balance, and the
  // second look costs 1.3 us of scattered plan-word loads: its few longer runs are added where the fast path found them
  const bool skew = B - nu > FIX_SKEW;                           // uniform over the workgroup
  const int ub = skew ? fix_spread(t, B) : u;
  int s0b = s0, s1b = s1;
  if (skew) {
    s0b = 0; s1b = 0;
    if (in_col && ub < nu) {
      s0b = k.col_seg[(int64_t)f * (B + 1) + ub];
      s1b = k.col_seg[(int64_t)f * (B + 1) + ub + 1];
    }
  }
  const int lenb = s1b - s0b;
  float accwb = 0.f;                                            // gz of the run's head
  if (lenb > 2) accwb = skew ? gz[pf[s0b]] : accw;
  // (without skew the few runs of more than two members all take the whole-wave path below: no list, no barrier)
  if (skew && lenb > FIX_HUGE) {                                 // (which entry a run gets does not matter: every run is
    const int i = atomicAdd(&huge_n, 1);                         // summed on its own, in a fixed order)
    if (i < 128) { huge_s0[i] = s0b; huge_s1[i] = s1b; huge_u[i] = ub; huge_gz[i] = accwb; }
  }
  const int r = lane >> 2, c = lane & 3;
  // runs of 3..FIX_SHORT members: FOUR lanes per run (one 16-byte chunk of the row each), 16 runs per round; head + member
  // 2 + member 3 ... in member order, four members' loads in flight at a time.  (One lane per run walking its members
  // paid two dependent round trips per member: up to 14 in a row for a run of 8 -- with Zipf ids every wave has a few.)
  {
    unsigned long long shortm = __ballot(skew && lenb > 2 && lenb <= FIX_SHORT);
#ifdef ABL_NOSHORT
    shortm = 0;
#endif
    while (shortm) {                                            // wave-uniform
      const int src = fix_group_src(shortm, lane);
      const bool has = src >= 0;
      const int sl = has ? src : 0;
      const int gs0 = __shfl(s0b, sl, 64), gs1_ = __shfl(s1b, sl, 64), gu = __shfl(ub, sl, 64);
      float wsum = __shfl(accwb, sl, 64);
      const int gs1 = has ? gs1_ : 0;                            // (the shuffles themselves need every lane)
      const int64_t gdst = before + gu;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has) acc = g_embed[gdst * 4 + c];
      for (int sp = gs0 + 1; __any(sp < gs1); sp += 4) {
        if (sp < gs1) {
          int e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) e[j] = pf[sp + j < gs1 ? sp + j : gs1 - 1];
          float4 xm[4];
          float gm[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            xm[j] = vals[((int64_t)e[j] * F + f) * 4 + c];
            gm[j] = gz[e[j]];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (sp + j < gs1) {
              acc.x += xm[j].x; acc.y += xm[j].y; acc.z += xm[j].z; acc.w += xm[j].w;
              wsum += gm[j];
            }
          }
        }
      }
      if (has) {
        g_embed[gdst * 4 + c] = acc;
        if (c == 0) k.g_w[gdst] = wsum;
      }
      for (int i = 0; i < 16 && shortm; ++i) shortm &= shortm - 1;
    }
  }
  // long runs, one at a time, by the whole wave: lane = (member slot r of 16, chunk c of 4)
  unsigned long long longm = __ballot(skew ? (lenb > FIX_SHORT && lenb <= FIX_HUGE) : lenb > 2);
#ifdef ABL_NOLONG
  longm = 0;
#endif
  while (longm) {
    const int src = __ffsll((long long)longm) - 1;
    longm &= longm - 1;
    const int rs0 = __shfl(s0b, src, 64), rs1 = __shfl(s1b, src, 64);
    const int ru = __shfl(ub, src, 64);
    const float rgz = __shfl(accwb, src, 64);
    const int64_t rdst = before + ru;
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f);
    float pw = 0.f;
#pragma unroll 4
    for (int s = rs0 + 1 + r; s < rs1; s += 16) {              // independent loads: several rounds in flight
      const int64_t b = pf[s];
      const float4 x = vals[(b * F + f) * 4 + c];
      pa.x += x.x; pa.y += x.y; pa.z += x.z; pa.w += x.w;
      pw += gz[b];
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {                         // fixed butterfly over the 16 member slots
      pa.x += __shfl_xor(pa.x, o, 64); pa.y += __shfl_xor(pa.y, o, 64);
      pa.z += __shfl_xor(pa.z, o, 64); pa.w += __shfl_xor(pa.w, o, 64);
      pw += __shfl_xor(pw, o, 64);
    }
    if (r == 0) {
      float4 h = g_embed[rdst * 4 + c];
      h.x += pa.x; h.y += pa.y; h.z += pa.z; h.w += pa.w;
      g_embed[rdst * 4 + c] = h;
      const float wsum = rgz + pw;
      if (c == 0) k.g_w[rdst] = wsum;
    }
  }
  // huge runs, up to 16 at a time, by the whole workgroup: with n of them in a round, 16 / n waves share a run (wave of run
  // h, sub-index sw: member slots 16 sw + r, stride 16 * waves-per-run, four members per lane in flight); the waves'
  // partial rows meet in LDS and the run's first wave adds them in wave order.  (One wave walking the 848 members of a
  // Zipf head 64 at a time was a 13-round dependent chain; the whole workgroup taking the huge runs one after the other
  // still paid ~5 round trips per run: 16 us of the 34-us launch with Zipf ids.)
  if (skew) __syncthreads();                                     // (uniform over the workgroup)
#ifdef ABL_NOHUGE
  const int n_huge = 0;
#else
  const int n_huge = skew ? (huge_n < 128 ? huge_n : 128) : 0;
#endif
  const int wv = tid >> 6;
  constexpr int NWV_F = FIX_T / 64;
  // more than one round: the list goes into ascending run order first.  The round a run falls in fixes how many waves
  // add it (16 / nr) and so the order of its additions; taken in the order the atomics above landed, a run's sum changed
  // in its last bits from one launch to the next.  (One round: every run gets the same 16 / nr waves wherever it sits.)
  if (n_huge > NWV_F) {                                          // (uniform over the workgroup)
    int hs0 = 0, hs1 = 0, hu = 0, rk = 0;
    float hg = 0.f;
    if (tid < n_huge) {
      hs0 = huge_s0[tid]; hs1 = huge_s1[tid]; hu = huge_u[tid]; hg = huge_gz[tid];
      for (int j = 0; j < n_huge; ++j) rk += huge_u[j] < hu ? 1 : 0;   // runs are distinct: ranks 0 .. n_huge-1
    }
    __syncthreads();
    if (tid < n_huge) { huge_s0[rk] = hs0; huge_s1[rk] = hs1; huge_u[rk] = hu; huge_gz[rk] = hg; }
    __syncthreads();
  }
  for (int h0 = 0; h0 < n_huge; h0 += NWV_F) {
    const int nr = n_huge - h0 < NWV_F ? n_huge - h0 : NWV_F;    // runs of this round
    const int wpr = NWV_F / nr;                                  // waves per run
    const int hl = wv / wpr, sw = wv - hl * wpr;
    const bool mine = hl < nr;
    const int h = h0 + (mine ? hl : 0);
    const int rs0 = huge_s0[h], rs1 = mine ? huge_s1[h] : 0;
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f);
    float pw = 0.f;
    const int stride = 16 * wpr;
    // four members per lane and round in flight (eight cost 25 more registers: at 81 the launch dropped to one workgroup
    // per CU and the uniform step lost 0.7 us)
    for (int base = rs0 + 1 + 16 * sw + r; base < rs1; base += 4 * stride) {
      int bm[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sidx = base + j * stride;
        bm[j] = pf[sidx < rs1 ? sidx : rs1 - 1];
      }
      float4 xm[4];
      float gm[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xm[j] = vals[((int64_t)bm[j] * F + f) * 4 + c];
        gm[j] = gz[bm[j]];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (base + j * stride < rs1) {
          pa.x += xm[j].x; pa.y += xm[j].y; pa.z += xm[j].z; pa.w += xm[j].w;
          pw += gm[j];
        }
      }
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {
      pa.x += __shfl_xor(pa.x, o, 64); pa.y += __shfl_xor(pa.y, o, 64);
      pa.z += __shfl_xor(pa.z, o, 64); pa.w += __shfl_xor(pa.w, o, 64);
      pw += __shfl_xor(pw, o, 64);
    }
    float4 hsum = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t rdst = before + huge_u[h];
    const bool fin = mine && sw == 0 && r == 0;                  // the run's first wave, one lane per chunk
    if (fin) hsum = g_embed[rdst * 4 + c];                       // (in flight across the barrier)
    if (r == 0) {
      hpart[wv][c] = pa;
      if (c == 0) hw_s[wv] = pw;
    }
    __syncthreads();
    if (fin) {
      float wsum = huge_gz[h];
      for (int q = 0; q < wpr; ++q) {
        const float4 x = hpart[wv + q][c];
        hsum.x += x.x; hsum.y += x.y; hsum.z += x.z; hsum.w += x.w;
        wsum += hw_s[wv + q];
      }
      g_embed[rdst * 4 + c] = hsum;
      if (c == 0) k.g_w[rdst] = wsum;
    }
    __syncthreads();
  }
  if (bidx == 0 && tid == 0) *k.n_uniq = total;
  // The optimizer, once every row sum of this workgroup's slots is final: 8 lanes per row -- lanes 0..3 one 16-byte
  // chunk of the embedding row and of its moments, lane 4 the first-order weight -- so that a wave instruction covers 8
  // rows with one line request each.  (Applied by the lane that owns the run, 16 bytes at a time, every instruction
  // touched 64 different rows: 2.5 M line requests per launch for 0.4 M distinct lines, 75 us.)
  if (adam) {                                                   // uniform over the launch
    __syncthreads();
    const int piece = tid & 7, rr = tid >> 3;
    const int step_now = k.last ? (int32_t)*k.step_dev : 0;
    // a row is updated by the workgroup that made its sum final: runs of up to two members under the fast mapping, longer
    // ones under the spread mapping (another workgroup may still be adding those of this one's fast slots)
    const bool skew_a = B - nu > FIX_SKEW;
#pragma unroll 1
    for (int p = 0; p < (skew_a ? 2 : 1) * (FIX_T / 128); ++p) {
      const bool spread = p >= FIX_T / 128;
      const int tl = (bidx - f * per_col) * FIX_T + (spread ? p - FIX_T / 128 : p) * 128 + rr;
      const int uu = spread ? fix_spread(tl, B) : fix_deal(tl, B);
      if (tl < B && uu < nu && piece < 5) {
        const int ln = k.col_seg[(int64_t)f * (B + 1) + uu + 1] - k.col_seg[(int64_t)f * (B + 1) + uu];
        if (!skew_a || (ln > 2) == spread) {
          const int64_t d2 = before + uu;
          const int64_t id = k.col_uid[(int64_t)f * B + uu];
          if ((uint64_t)id < (uint64_t)k.V) {
            if (piece < 4) {
              adam_chunk(k, id, piece, g_embed[d2 * 4 + piece]);
            } else {
              adam_w(k, id, k.g_w[d2]);
              if (k.last) k.last[id] = step_now;
            }
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(1024, 8) void deepfm_post_direct_kernel(ReduceArgs r, ColSegArgs k, int nb_reduce) {
  if ((int)blockIdx.x < nb_reduce) reduce_body(r, (int)blockIdx.x);
  else fixup_body(k, (int)blockIdx.x - nb_reduce);
}

// reduction of the workgroup partials and the segment sums only depend on the fused kernel, not on each other: one
// launch, the first nb_reduce workgroups (1024 threads) reduce, the others sum segments -- they run side by side
__global__ __launch_bounds__(1024) void deepfm_post_kernel(ReduceArgs r, ColSegArgs k, int nb_reduce) {
  if ((int)blockIdx.x < nb_reduce) reduce_body(r, (int)blockIdx.x);
  else colseg_body(k, (int)blockIdx.x - nb_reduce);
}


// ---- Keras Adam, evaluated lazily AND exactly.  Keras' sparse apply is a dense sweep: every row of the table decays its
// moments and moves every step (2.FM/ModelManager.py:178-179 on IndexedSlices gradients).  The update of an untouched row
// at step j depends on nothing but the row and lr_j, so a row may skip the sweeps and REPLAY them later: last[row] = the
// step the row holds, and before a batch reads its rows this kernel applies the steps last+1 .. *step_dev they missed,
// element by element with the sweep's own arithmetic (adam_decay) -- the same bits the sweep would have left.  The rows
// of a batch then receive the touched update of the current step in the post launch, which also sets last.
struct CatchArgs {
  const int64_t* col_uid; const int32_t* col_nu; int64_t B; int F;   // plan of the batch; null col_uid: all rows [0, V)
  float* table; int64_t V; float* m_e; float* v_e; int64_t ldm; float* m_w; float* v_w; int64_t ldw;
  const int32_t* last; const int64_t* step_dev; const float* lr_tab; int64_t n_tab; float b1, b2, eps;
};
// A workgroup (256 threads) takes CATCH_R = 64 consecutive slots (unique ids of the plan, or table rows for the flush),
// FOUR lanes per row: lane q owns elements 4q .. 4q+3 of the row (lane 0 also the first-order weight) -- four or five
// independent chains per lane, 512 rows in flight per CU.  The kernel is a chain of latencies, not arithmetic (at 1M rows
// the arithmetic is ~25 us of the chip, the first form -- 16 lanes per row, 128 rows in flight per CU, a global load of
// lr_t in every replayed step, three dependent round trips before the first of them -- took 78 us):
//   trip 1   plan word of the slot (col_nu of its column beside it)
//   trip 2   last[id] AND the row's x / m / v pieces (their addresses only need the id)
//   LDS      the rows change hands: how many steps each one replays is known now, and the rows are handed out again in
//            DESCENDING order of that count -- a wave of 16 rows runs as long as its longest row, and with the pending
//            counts of a batch spread geometrically (mean ~47 at 213k of 10M rows per step) unsorted waves ran twice the
//            mean
//   replay   lr_t of the last CATCH_LR steps comes from LDS (older ones from the table in memory)
constexpr int CATCH_R = 64, CATCH_T = 256, CATCH_LR = 1024;
__global__ __launch_bounds__(CATCH_T) void adam_keras_catchup_kernel(CatchArgs a) {
  __shared__ float4 x_s[CATCH_R][4], m_s[CATCH_R][4], v_s[CATCH_R][4];
  __shared__ float xw_s[CATCH_R], mw_s[CATCH_R], vw_s[CATCH_R];
  __shared__ int64_t id_s[CATCH_R];
  __shared__ int k_s[CATCH_R];
  __shared__ unsigned char ord[CATCH_R];
  __shared__ float lr_s[CATCH_LR];
  const int tid = threadIdx.x, r = tid >> 2, q = tid & 3;
  const int64_t nslot = a.col_uid ? a.B * a.F : a.V;
  const int64_t j1 = *a.step_dev;
#pragma unroll
  for (int i = tid; i < CATCH_LR; i += CATCH_T) {          // lr_s[i] = lr_t of step j1 - i
    const int64_t j = j1 - i;
    lr_s[i] = j >= 1 ? a.lr_tab[(j < a.n_tab ? j : a.n_tab) - 1] : 0.f;
  }
  const int64_t slot = (int64_t)blockIdx.x * CATCH_R + r;
  int64_t id = -1;
  if (a.col_uid) {
    const int64_t sc = slot < nslot ? slot : nslot - 1;    // unconditional loads, judged afterwards
    const int f = (int)(sc / a.B);
    const int64_t u = sc - (int64_t)f * a.B;
    const int nu = a.col_nu[f];
    const int64_t cand = a.col_uid[sc];
    if (slot < nslot && u < nu) id = cand;
  } else if (slot < nslot) {
    id = slot;
  }
  const bool ok = (uint64_t)id < (uint64_t)a.V;
  const int64_t idc = ok ? id : 0;
  const int j0 = a.last[idc];
  float4 x4 = *reinterpret_cast<const float4*>(a.table + idc * LD + 4 * q);
  float4 m4 = *reinterpret_cast<const float4*>(a.m_e + idc * a.ldm + 4 * q);
  float4 v4 = *reinterpret_cast<const float4*>(a.v_e + idc * a.ldm + 4 * q);
  x_s[r][q] = x4; m_s[r][q] = m4; v_s[r][q] = v4;
  if (q == 0) {
    xw_s[r] = a.table[idc * LD + E16];
    mw_s[r] = a.m_w[idc * a.ldw];
    vw_s[r] = a.v_w[idc * a.ldw];
    id_s[r] = id;
    k_s[r] = (ok && j1 > j0) ? (int)(j1 - j0) : 0;
  }
  __syncthreads();
  if (tid < CATCH_R) {
    const int k = k_s[tid];
    int rank = 0;
#pragma unroll 8
    for (int c = 0; c < CATCH_R; ++c) rank += (k_s[c] > k || (k_s[c] == k && c < tid)) ? 1 : 0;
    ord[rank] = (unsigned char)tid;
  }
  __syncthreads();
  const int rr = ord[r];                                   // the row this lane group replays
  const int k = k_s[rr];
  if (k <= 0) return;
  const int64_t rid = id_s[rr];
  x4 = x_s[rr][q]; m4 = m_s[rr][q]; v4 = v_s[rr][q];
  float xw = 0.f, mw = 0.f, vw = 0.f;
  if (q == 0) { xw = xw_s[rr]; mw = mw_s[rr]; vw = vw_s[rr]; }
  // (a row that was never touched -- m = v = 0 -- stays put: x - lr*0/(0+eps) = x; skipping it is only cheaper)
  const bool any_e = m4.x != 0.f || v4.x != 0.f || m4.y != 0.f || v4.y != 0.f || m4.z != 0.f || v4.z != 0.f ||
                     m4.w != 0.f || v4.w != 0.f;
  const bool any_w = q == 0 && (mw != 0.f || vw != 0.f);
  if (!any_e && !any_w) return;
  for (int i = k - 1; i >= 0; --i) {                       // step j1 - i
    float lr;
    if (i < CATCH_LR) {
      lr = lr_s[i];
    } else {
      const int64_t j = j1 - i;
      lr = a.lr_tab[(j < a.n_tab ? j : a.n_tab) - 1];
    }
    adam_decay(x4.x, m4.x, v4.x, lr, a.b1, a.b2, a.eps);
    adam_decay(x4.y, m4.y, v4.y, lr, a.b1, a.b2, a.eps);
    adam_decay(x4.z, m4.z, v4.z, lr, a.b1, a.b2, a.eps);
    adam_decay(x4.w, m4.w, v4.w, lr, a.b1, a.b2, a.eps);
    if (q == 0) adam_decay(xw, mw, vw, lr, a.b1, a.b2, a.eps);
  }
  if (any_e) {
    *reinterpret_cast<float4*>(a.table + rid * LD + 4 * q) = x4;
    *reinterpret_cast<float4*>(a.m_e + rid * a.ldm + 4 * q) = m4;
    *reinterpret_cast<float4*>(a.v_e + rid * a.ldm + 4 * q) = v4;
  }
  if (any_w) {
    a.table[rid * LD + E16] = xw;
    a.m_w[rid * a.ldw] = mw;
    a.v_w[rid * a.ldw] = vw;
  }
}
__global__ __launch_bounds__(256) void fill_last_kernel(int32_t* __restrict__ last, int64_t V,
                                                        const int64_t* __restrict__ step_dev) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < V) last[t] = (int32_t)*step_dev;
}

}  // namespace

extern "C" size_t rec_deepfm_fused_workspace_bytes(int64_t B, int F) {
  if (B <= 0 || F <= 0) return 0;
  return fused_workspace(B, F).bytes() + 256;
}

// The one entry point of the post launch.  Three independent options:
//   slot_map   (sharded step) packed rows [embed 16 | w | 0 0 0] go to the slots rec_colsort_shard_map_fixed_i64 gave the
//              batch's unique ids inside g_embed_rows [owners * capacity, 20]; unused slots are not written
//   direct     the plan (rec_colsort_plan_dest_i64) existed BEFORE the main kernel ran, which wrote the value row of every
//              run's first member straight into g_embed_rows; this launch finishes runs with more members, fills uniq_ids /
//              g_w_rows / n_uniq and the padded tail
//   adam       (direct only) the lazy (touched-rows) Adam update of both tables (rec_adam_rows_f32's arithmetic) applied to
//              every row the moment its gradient is final: no second pass over g_embed_rows / g_w_rows, no extra launch.
//              The step size is read from device memory (lr_t_dev, advanced by the main launch on the same stream): no
//              per-step host scalar, so a whole train step replays from a hipGraph.  last / step_dev (optional): the exact
//              lazy evaluation of Keras' sweep
extern "C" int rec_deepfm_fused_post_f32(int F, int64_t B, const float* gz, const float* vals, float* const* grads,
                                         float* loss, void* workspace, const int32_t* perm, const int64_t* col_uid,
                                         const int32_t* col_seg, const int32_t* col_nu, int64_t* uniq_ids,
                                         float* g_embed_rows, float* g_w_rows, int64_t* n_uniq, const int32_t* slot_map,
                                         int direct, const rec_deepfm_lazy_adam* adam, void* stream) {
  if (adam) {
    if (!adam->table || !adam->m_e || !adam->v_e || !adam->m_w || !adam->v_w || !adam->lr_t_dev || adam->V <= 0 ||
        adam->ld_state < E16 || (adam->ld_state & 3) != 0 || adam->ld_wstate < 1)
      return REC_E_ARG;
    if (adam->ld != LD || !rec_is_aligned16(adam->table) || !rec_is_aligned16(adam->m_e) || !rec_is_aligned16(adam->v_e))
      return REC_E_UNSUPPORTED;
    if (adam->last && !adam->step_dev) return REC_E_ARG;
  }
  if (B <= 0 || F <= 0 || F > 28) return REC_E_ARG;
  if (!gz || !vals || !grads || !loss || !workspace || !perm || !col_uid || !col_seg || !col_nu || !g_embed_rows)
    return REC_E_ARG;
  for (int i = 0; i < 7; ++i)
    if (!grads[i]) return REC_E_ARG;
  if (slot_map ? (uniq_ids || g_w_rows || n_uniq) : (!uniq_ids || !g_w_rows || !n_uniq)) return REC_E_ARG;
  if ((slot_map && direct) || (adam && !direct)) return REC_E_UNSUPPORTED;
  if (!rec_is_aligned16(vals) || !rec_is_aligned16(g_embed_rows))
    return REC_E_UNSUPPORTED;
  const FusedWorkspace ws = fused_workspace(B, F);
  int D = F * E16;
  unsigned nb = (unsigned)reduce_blocks(D);
  ReduceArgs r{ws.dK0part(workspace), ws.small(workspace), ws.nwg, D, B,
               grads[0], grads[2], grads[1], grads[3], grads[4], grads[5], grads[6], loss};   // dK0 dK1 db0 db1 dK2 db2 dbias
  ColSegArgs k{};                                        // (lr_t stays 0: the step size comes from lr_t_dev)
  k.vals = (const float4*)vals; k.gz = gz; k.perm = perm; k.col_uid = col_uid; k.col_seg = col_seg; k.col_nu = col_nu;
  k.B = B; k.F = F; k.uniq_ids = uniq_ids; k.g_embed = (float4*)g_embed_rows; k.g_w = g_w_rows; k.n_uniq = n_uniq;
  k.packed = slot_map ? 1 : 0; k.slot_map = slot_map;
  if (adam) {
    k.table = adam->table; k.m_e = adam->m_e; k.v_e = adam->v_e; k.m_w = adam->m_w; k.v_w = adam->v_w; k.V = adam->V;
    k.b1 = adam->b1; k.b2 = adam->b2; k.eps = adam->eps; k.lr_t_dev = adam->lr_t_dev;
    k.ldm = adam->ld_state; k.ldw = adam->ld_wstate; k.last = adam->last; k.step_dev = adam->step_dev;
  }
  if (direct) {
    unsigned nbf = (unsigned)F * (unsigned)ceil_div64(B, FIX_T);
    hipLaunchKernelGGL(deepfm_post_direct_kernel, dim3(nb + nbf), dim3(1024), 0, as_stream(stream), r, k, (int)nb);
  } else {
    unsigned nbs = (unsigned)ceil_div64(B * F * 4, 1024);
    hipLaunchKernelGGL(deepfm_post_kernel, dim3(nb + nbs), dim3(1024), 0, as_stream(stream), r, k, (int)nb);
  }
  REC_LAUNCH_CHECK();
  return REC_OK;
}

static int catchup_args_ok(const float* table, int64_t ld, int64_t V, const float* m_e, const float* v_e, int64_t ld_state,
                           const float* m_w, const float* v_w, int64_t ld_wstate, const int32_t* last,
                           const int64_t* step_dev, const float* lr_table, int64_t n_table) {
  if (!table || !m_e || !v_e || !m_w || !v_w || !last || !step_dev || !lr_table || V <= 0 || n_table <= 0 ||
      ld_state < E16 || ld_wstate < 1)
    return REC_E_ARG;
  if (ld != LD) return REC_E_UNSUPPORTED;
  // the rows' x / m / v travel as 16-byte pieces
  if ((ld_state & 3) != 0 || !rec_is_aligned16(table) || !rec_is_aligned16(m_e) || !rec_is_aligned16(v_e))
    return REC_E_UNSUPPORTED;
  return REC_OK;
}

extern "C" int rec_adam_keras_catchup_f32(const int64_t* col_uid, const int32_t* col_nu, int64_t B, int F, float* table,
                                          int64_t ld, int64_t V, float* m_e, float* v_e, int64_t ld_state, float* m_w,
                                          float* v_w, int64_t ld_wstate, const int32_t* last, const int64_t* step_dev,
                                          const float* lr_table, int64_t n_table, float b1, float b2, float eps,
                                          void* stream) {
  if (!col_uid || !col_nu || B <= 0 || F <= 0) return REC_E_ARG;
  int rc = catchup_args_ok(table, ld, V, m_e, v_e, ld_state, m_w, v_w, ld_wstate, last, step_dev, lr_table, n_table);
  if (rc != REC_OK) return rc;
  CatchArgs a{col_uid, col_nu, B, F, table, V, m_e, v_e, ld_state, m_w, v_w, ld_wstate, last, step_dev, lr_table, n_table,
              b1, b2, eps};
  hipLaunchKernelGGL(adam_keras_catchup_kernel, dim3((unsigned)ceil_div64(B * F, CATCH_R)), dim3(CATCH_T), 0,
                     as_stream(stream), a);
  REC_LAUNCH_CHECK();
  return REC_OK;
}

// every row of the table up to date (before the parameters are read from outside: evaluation, checkpoint), last = step
extern "C" int rec_adam_keras_flush_f32(float* table, int64_t ld, int64_t V, float* m_e, float* v_e, int64_t ld_state,
                                        float* m_w, float* v_w, int64_t ld_wstate, int32_t* last, const int64_t* step_dev,
                                        const float* lr_table, int64_t n_table, float b1, float b2, float eps,
                                        void* stream) {
  int rc = catchup_args_ok(table, ld, V, m_e, v_e, ld_state, m_w, v_w, ld_wstate, last, step_dev, lr_table, n_table);
  if (rc != REC_OK) return rc;
  CatchArgs a{nullptr, nullptr, 0, 0, table, V, m_e, v_e, ld_state, m_w, v_w, ld_wstate, last, step_dev, lr_table,
              n_table, b1, b2, eps};
  hipLaunchKernelGGL(adam_keras_catchup_kernel, dim3((unsigned)ceil_div64(V, CATCH_R)), dim3(CATCH_T), 0,
                     as_stream(stream), a);
  REC_LAUNCH_CHECK();
  hipLaunchKernelGGL(fill_last_kernel, dim3((unsigned)ceil_div64(V, 256)), dim3(256), 0, as_stream(stream), last, V,
                     step_dev);
  REC_LAUNCH_CHECK();
  return REC_OK;
}