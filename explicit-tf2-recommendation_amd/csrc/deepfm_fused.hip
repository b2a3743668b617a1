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

// Phase stamps of the direct-mode post launch (diagnostic builds, -DREC_POST_STAMPS; scripts/exp/post_stamps.py reads
// them): lane 0 of every wave writes the wall clock (100 MHz) at the phases of its job, 8 words per wave; the reduce
// workgroups come first in the buffer, then the fix-up workgroups, wherever they sit in the grid (PSTAMP_WG).  PSTAMP_WAIT
// makes "landed" mean what it says: the wave waits for its outstanding loads before it stamps.  Off: all are nothing.
#ifdef REC_POST_STAMPS
#define PSTAMP_WG(wg_) const int pstamp_wg = (wg_)
#define PSTAMP(A, k_)                                                                                          \
  do {                                                                                                         \
    if ((threadIdx.x & 63) == 0)                                                                               \
      (A).stamps[((int64_t)pstamp_wg * 16 + (threadIdx.x >> 6)) * 8 + (k_)] = wall_clock64();                  \
  } while (0)
#ifdef REC_POST_STAMPS_NOWAIT                            // (stamps where the waves are anyway: no wait added)
#define PSTAMP_WAIT() do {} while (0)
#else
#define PSTAMP_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#endif
#else
#define PSTAMP_WG(wg_) do {} while (0)
#define PSTAMP(A, k_) do {} while (0)
#define PSTAMP_WAIT() do {} while (0)
#endif

// fixed-order sum of the per-workgroup partials.  1024 threads = 16 slices x 64 lanes; lane owns 4 consecutive
// outputs (float4), slice q adds workgroups q, q+16, q+32, ... (independent 16-B loads), then the 16 slices are
// added in slice order through LDS.
struct ReduceArgs {
  const float* dK0part; const float* small; int nwg; int D; int64_t B;
  float* dK0; float* dK1; float* db0; float* db1; float* dK2; float* db2; float* dbias; float* loss;
#ifdef REC_POST_STAMPS
  unsigned long long* stamps;
#endif
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
  PSTAMP_WG(bidx);
  PSTAMP(r, 0);
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
  PSTAMP_WAIT();
  PSTAMP(r, 1);                                        // partials landed (and added)
  red[q][lane] = acc;
  __syncthreads();
  PSTAMP(r, 2);
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
    PSTAMP(r, 3);
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
  PSTAMP(r, 3);
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
#ifdef REC_POST_STAMPS
  unsigned long long* stamps;
#endif
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


// ---- direct mode: what is left for the launch after the fused kernel.  One lane per run (slot) of the plan
// (fixup_body), or four consecutive runs per lane where B is a multiple of 1024 and no lazy Adam rides along
// (fixq_body, further down); in both:
//   a run of one lookup (almost all of them with uniform ids): g_w = gz of that lookup, uniq_ids = its id -- coalesced
//     stores, the value row is already in place;
//   a pair: the lane adds the second member's value row to the head's row itself;
//   a run of 3..FIX_SHORT lookups: four lanes (one 16-byte chunk each), 16 runs of the wave at a time, members in order;
//   a run of up to FIX_HUGE: the whole wave adds it, 16 members x 4 float4 chunks per round, fixed butterfly over the rows;
//   longer ones (Zipf heads): the whole workgroup, partial rows of its 16 waves added in wave order;
//   slots beyond the column's runs: the zero-padded tail.
constexpr int FIX_T = 1024, FIX_HUGE = 128, FIX_SHORT = 17, FIX_SKEW = 256;
// slot t of a column (thread order) -> run u, twice.
// fix_deal: the mapping of fixup_body's FAST path (ids, single lookups, pairs, the padded tail -- nearly everything, and
// all of it coalesced stores): a wave takes 4 consecutive runs from each sixteenth of the column, so that plan words arrive and ids
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
// what the paths for runs of more than two members keep in LDS.  Runs of more than FIX_HUGE members (Zipf heads: the
// hottest id of a column holds ~10 % of its lookups) are left to the WHOLE workgroup: at most B / FIX_HUGE <= 128 of them
// exist in a column
struct FixShared {
  int huge_n, huge_s0[128], huge_s1[128], huge_u[128];
  float huge_gz[128];
  float4 hpart[FIX_T / 64][4];
  float hw_s[FIX_T / 64];
};

// The runs of `longm` (one bit per owning lane: members s0b+1 .. s1b-1 of perm, slot ub, gz of the head accwb), one at a
// time, by the whole wave: lane = (member slot r of 16, chunk c of 4).  IX: the integer the offsets are formed in.
// HEADGZ: the wave reads gz of the run's head itself, beside the members (accwb is not used).  The head's row is asked
// for before the members: it is only needed after the butterfly, and asked for there it was a round trip of its own
template <typename IX, bool HEADGZ = false>
__device__ __forceinline__ void fix_wave_runs(const ColSegArgs& k, const int32_t* __restrict__ pf, int f, IX before,
                                              unsigned long long longm, int s0b, int s1b, int ub, float accwb) {
  const float4* __restrict__ vals = k.vals;
  const float* __restrict__ gz = k.gz;
  float4* __restrict__ g_embed = k.g_embed;
  const int F = k.F;
  const int lane = threadIdx.x & 63, r = lane >> 2, c = lane & 3;
#ifdef ABL_NOLONG
  longm = 0;
#endif
  while (longm) {
    const int src = __ffsll((long long)longm) - 1;
    longm &= longm - 1;
    const int rs0 = __shfl(s0b, src, 64), rs1 = __shfl(s1b, src, 64);
    const int ru = __shfl(ub, src, 64);
    float rgz = __shfl(accwb, src, 64);
    const IX rdst = before + ru;
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r == 0) h = g_embed[rdst * 4 + c];
    if (HEADGZ) rgz = gz[pf[rs0]];
    float4 pa = make_float4(0.f, 0.f, 0.f, 0.f);
    float pw = 0.f;
#pragma unroll 4
    for (int s = rs0 + 1 + r; s < rs1; s += 16) {              // independent loads: several rounds in flight
      const IX b = pf[s];
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
      h.x += pa.x; h.y += pa.y; h.z += pa.z; h.w += pa.w;
      g_embed[rdst * 4 + c] = h;
      const float wsum = rgz + pw;
      if (c == 0) k.g_w[rdst] = wsum;
    }
  }
}

// ---- runs of more than two members of a SKEWED column (more than FIX_SKEW lookups beyond the first of their runs): the
// second look, under fix_spread.  Slot t of the column (this workgroup's 1024, one per thread; sh.huge_n was zeroed
// before a barrier).  (A column without skew -- uniform ids: ~90 pairs -- has next to nothing to balance, and the second
// look costs 1.3 us of scattered plan-word loads: its few longer runs are added where the fast path found them.)
template <typename IX>
__device__ __forceinline__ void fix_skew_runs(const ColSegArgs& k, FixShared& sh, const int32_t* __restrict__ pf, int f,
                                              IX before, int nu, bool in_col, int t) {
  const float4* __restrict__ vals = k.vals;
  const float* __restrict__ gz = k.gz;
  float4* __restrict__ g_embed = k.g_embed;
  const int64_t B = k.B;
  const int F = k.F;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ub = fix_spread(t, B);
  int s0b = 0, s1b = 0;
  if (in_col && ub < nu) {
    s0b = k.col_seg[(IX)f * (IX)(B + 1) + ub];
    s1b = k.col_seg[(IX)f * (IX)(B + 1) + ub + 1];
  }
  const int lenb = s1b - s0b;
  float accwb = 0.f;                                            // gz of the run's head
  if (lenb > 2) accwb = gz[pf[s0b]];
  if (lenb > FIX_HUGE) {                                         // (which entry a run gets does not matter: every run is
    const int i = atomicAdd(&sh.huge_n, 1);                      // summed on its own, in a fixed order)
    if (i < 128) { sh.huge_s0[i] = s0b; sh.huge_s1[i] = s1b; sh.huge_u[i] = ub; sh.huge_gz[i] = accwb; }
  }
  const int r = lane >> 2, c = lane & 3;
  // runs of 3..FIX_SHORT members: FOUR lanes per run (one 16-byte chunk of the row each), 16 runs per round; head + member
  // 2 + member 3 ... in member order, four members' loads in flight at a time.  (One lane per run walking its members
  // paid two dependent round trips per member: up to 14 in a row for a run of 8 -- with Zipf ids every wave has a few.)
  {
    unsigned long long shortm = __ballot(lenb > 2 && lenb <= FIX_SHORT);
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
      const IX gdst = before + gu;
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
            xm[j] = vals[((IX)e[j] * F + f) * 4 + c];
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
  fix_wave_runs<IX>(k, pf, f, before, __ballot(lenb > FIX_SHORT && lenb <= FIX_HUGE), s0b, s1b, ub, accwb);
  // huge runs, up to 16 at a time, by the whole workgroup: with n of them in a round, 16 / n waves share a run (wave of run
  // h, sub-index sw: member slots 16 sw + r, stride 16 * waves-per-run, four members per lane in flight); the waves'
  // partial rows meet in LDS and the run's first wave adds them in wave order.  (One wave walking the 848 members of a
  // Zipf head 64 at a time was a 13-round dependent chain; the whole workgroup taking the huge runs one after the other
  // still paid ~5 round trips per run: 16 us of the 34-us launch with Zipf ids.)
  __syncthreads();
#ifdef ABL_NOHUGE
  const int n_huge = 0;
#else
  const int n_huge = sh.huge_n < 128 ? sh.huge_n : 128;
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
      hs0 = sh.huge_s0[tid]; hs1 = sh.huge_s1[tid]; hu = sh.huge_u[tid]; hg = sh.huge_gz[tid];
      for (int j = 0; j < n_huge; ++j) rk += sh.huge_u[j] < hu ? 1 : 0;   // runs are distinct: ranks 0 .. n_huge-1
    }
    __syncthreads();
    if (tid < n_huge) { sh.huge_s0[rk] = hs0; sh.huge_s1[rk] = hs1; sh.huge_u[rk] = hu; sh.huge_gz[rk] = hg; }
    __syncthreads();
  }
  for (int h0 = 0; h0 < n_huge; h0 += NWV_F) {
    const int nr = n_huge - h0 < NWV_F ? n_huge - h0 : NWV_F;    // runs of this round
    const int wpr = NWV_F / nr;                                  // waves per run
    const int hl = wv / wpr, sw = wv - hl * wpr;
    const bool mine = hl < nr;
    const int h = h0 + (mine ? hl : 0);
    const int rs0 = sh.huge_s0[h], rs1 = mine ? sh.huge_s1[h] : 0;
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
        xm[j] = vals[((IX)bm[j] * F + f) * 4 + c];
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
    const IX rdst = before + sh.huge_u[h];
    const bool fin = mine && sw == 0 && r == 0;                  // the run's first wave, one lane per chunk
    if (fin) hsum = g_embed[rdst * 4 + c];                       // (in flight across the barrier)
    if (r == 0) {
      sh.hpart[wv][c] = pa;
      if (c == 0) sh.hw_s[wv] = pw;
    }
    __syncthreads();
    if (fin) {
      float wsum = sh.huge_gz[h];
      for (int q = 0; q < wpr; ++q) {
        const float4 x = sh.hpart[wv + q][c];
        hsum.x += x.x; hsum.y += x.y; hsum.z += x.z; hsum.w += x.w;
        wsum += sh.hw_s[wv + q];
      }
      g_embed[rdst * 4 + c] = hsum;
      if (c == 0) k.g_w[rdst] = wsum;
    }
    __syncthreads();
  }
}

// The one-run-per-lane body: every B that is no multiple of 1024, and every launch with the lazy Adam.
__device__ __forceinline__ void fixup_body(const ColSegArgs& k_in, int bidx) {
  ColSegArgs k = k_in;
  if (k.lr_t_dev) k.lr_t = *k.lr_t_dev;
  const float4* __restrict__ vals = k.vals;
  const float* __restrict__ gz = k.gz;
  const int64_t B = k.B;
  const int F = k.F;
  float4* __restrict__ g_embed = k.g_embed;
  const int tid = threadIdx.x;
  const int per_col = (int)((B + FIX_T - 1) / FIX_T);           // workgroups per column
  PSTAMP_WG((int)gridDim.x - F * per_col + bidx);
  PSTAMP(k, 0);
  const int f = bidx / per_col;
  const int t = (bidx - f * per_col) * FIX_T + tid;             // slot of the column before the deal
  const int u = fix_deal(t, B);
  __shared__ int nu_s[REC_MAX_COLS];
  __shared__ FixShared sh;
  if (tid < F) nu_s[tid] = k.col_nu[tid];
  if (tid == 0) sh.huge_n = 0;
  __syncthreads();
  PSTAMP(k, 1);
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
    PSTAMP_WAIT();
    PSTAMP(k, 2);
    const int hb = pf[s0];
    PSTAMP_WAIT();
    PSTAMP(k, 3);
    accw = gz[hb];
    const int64_t id = k.col_uid[(int64_t)f * B + u];
    PSTAMP_WAIT();
    PSTAMP(k, 4);
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
  PSTAMP(k, 5);
  // ---- runs of more than two members: a skewed column looks at them a second time (fix_skew_runs); the few of a column
  // without skew all take the whole-wave path where the fast path found them: no list, no barrier
  const bool skew = B - nu > FIX_SKEW;                           // uniform over the workgroup
  if (skew) fix_skew_runs<int64_t>(k, sh, pf, f, before, nu, in_col, t);
  else fix_wave_runs<int64_t>(k, pf, f, before, __ballot(len > 2), s0, s1, u, accw);
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
  PSTAMP(k, 6);
}

// ---- the body for B % 1024 == 0 without the lazy Adam: FOUR CONSECUTIVE RUNS PER LANE.  A workgroup still owns 1024
// consecutive slots of one column (whole lines of uniq_ids / g_w / g_embed), but its fast path is the work of waves
// 0..3 only: lane L of wave w owns runs u0 = 1024 wg + 256 w + 4 L .. u0 + 3, so the plan words arrive as one 16-byte and
// one 4-byte piece of col_seg and two 16-byte pieces of col_uid, four perm and four gz gathers are in flight per lane,
// and the ids and first-order rows leave as 16-byte pieces.  Every plan word is asked for BEFORE col_nu is waited for
// (u0 + 4 <= B: the addresses need no clamp), and before / total come from one col_nu[lane] load and a wave scan: no LDS
// and no barrier ahead of the plan loads.  Waves 4..7 read the col_seg words of waves 0..3 a second time and add the
// few runs of more than two members of a column without skew BESIDE the fast path (behind it, in the same wave, they
// were three more round trips at the very end of the launch, profiles/r09_post_stamps.txt); waves 8..15 of such a
// column leave at once.  In a skewed column all 16 waves take the second look of fix_skew_runs, as in
// the other body: every run of more than two members is summed by the same code in the same order of additions,
// whichever wave does it.  32-bit offsets (the entry point checks the sizes).
constexpr int FIXQ_WV = FIX_T / 256;                             // waves of a workgroup on the fast path
typedef int32_t fixq_seg4 __attribute__((ext_vector_type(4), aligned(4)));   // col_seg + f (B + 1) + u0: 4-byte aligned
typedef long long fixq_id2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void fixq_body(const ColSegArgs& k, int bidx) {
  const float4* __restrict__ vals = k.vals;
  const float* __restrict__ gz = k.gz;
  float4* __restrict__ g_embed = k.g_embed;
  const int B = (int)k.B, F = k.F;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);       // (scalar: the branches on it are wave-uniform)
  const int per_col = B >> 10;                                   // workgroups per column
  PSTAMP_WG((int)gridDim.x - F * per_col + bidx);
  PSTAMP(k, 0);
  const int f = bidx / per_col;
  const int wgc = bidx - f * per_col;
  const bool fast = wv < FIXQ_WV;                                // wave-uniform
  const bool helper = !fast && wv < 2 * FIXQ_WV;                 // the long runs of wave wv - 4's slots
  const int u0 = wgc * FIX_T + (fast || helper ? 256 * (wv & (FIXQ_WV - 1)) + 4 * lane : 0);
  __shared__ FixShared sh;
  const int nu_l = k.col_nu[lane < F ? lane : 0];
  fixq_seg4 sg4 = {0, 0, 0, 0};
  int sg4e = 0;
  fixq_id2 id01 = {0, 0}, id23 = {0, 0};
  int64_t id_pad = 0;
  if (fast || helper) {
    const int32_t* segp = k.col_seg + (f * (B + 1) + u0);
    sg4 = *reinterpret_cast<const fixq_seg4*>(segp);
    sg4e = segp[4];
  }
  if (fast) {
    const fixq_id2* idp = reinterpret_cast<const fixq_id2*>(k.col_uid + (f * B + u0));
    id01 = idp[0];
    id23 = idp[1];
    id_pad = k.col_uid[0];
  }
  // runs per column: lane c holds col_nu[c]; the prefix over the columns is a wave scan
  int incl = lane < F ? nu_l : 0;
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
    const int x = __shfl_up(incl, o, 64);
    if (lane >= o) incl += x;
  }
  // (read as scalars: everything that only depends on them is wave-uniform)
  const int before = __builtin_amdgcn_readlane(incl - (lane < F ? nu_l : 0), f);   // unique ids in earlier columns
  const int total = __builtin_amdgcn_readlane(incl, F - 1);                         // ... in all columns
  const int nu = __builtin_amdgcn_readlane(nu_l, f);
  PSTAMP(k, 1);
  const bool skew = B - nu > FIX_SKEW;                           // uniform over the workgroup
  const int32_t* pf = k.perm + f * B;
  if (fast) {
    const int nl = nu - u0;                                      // runs u0 + j with j < nl are live
    const int sg[5] = {sg4.x, sg4.y, sg4.z, sg4.w, sg4e};
    PSTAMP_WAIT();
    PSTAMP(k, 2);
    // ids and the padded tail first: they need nothing but the plan words, and their registers are free afterwards
    {
    const int dst = before + u0;
    if (nl >= 4) {
      if ((dst & 1) == 0) {                                      // (wave-uniform: u0 is a multiple of 4)
        fixq_id2* op = reinterpret_cast<fixq_id2*>(k.uniq_ids + dst);
        op[0] = id01;
        op[1] = id23;
      } else {
        k.uniq_ids[dst] = id01.x; k.uniq_ids[dst + 1] = id01.y; k.uniq_ids[dst + 2] = id23.x; k.uniq_ids[dst + 3] = id23.y;
      }
    } else {
      // the column's last live runs and / or its share of the padded tail: slot = total + rank among the column's
      // unused slots; id = the smallest id of column 0, zero rows
      const int64_t idv[4] = {id01.x, id01.y, id23.x, id23.y};
      const int d2 = total + (f * B - before) + (u0 - nu);       // slot of u0 if it were unused
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (nl <= 0 && (d2 & 3) == 0) {                            // (total, before, nu: wave-uniform)
#pragma unroll
        for (int i = 0; i < 16; ++i) g_embed[d2 * 4 + i] = z;
        *reinterpret_cast<float4*>(k.g_w + d2) = z;
        const fixq_id2 p2 = {id_pad, id_pad};
        fixq_id2* op = reinterpret_cast<fixq_id2*>(k.uniq_ids + d2);
        op[0] = p2;
        op[1] = p2;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < nl) {
            k.uniq_ids[dst + j] = idv[j];
          } else {
            g_embed[(d2 + j) * 4] = z; g_embed[(d2 + j) * 4 + 1] = z; g_embed[(d2 + j) * 4 + 2] = z;
            g_embed[(d2 + j) * 4 + 3] = z;
            k.g_w[d2 + j] = 0.f;
            k.uniq_ids[d2 + j] = id_pad;
          }
        }
      }
    }
    }
    int ln[4], hb[4], hb2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ln[j] = j < nl ? sg[j + 1] - sg[j] : 0;
    // head of every run, and the member behind it (the head again for a run of one): a pair's second member is then
    // one round trip away, not two
#pragma unroll
    for (int j = 0; j < 4; ++j) hb[j] = pf[j < nl ? sg[j] : 0];
#pragma unroll
    for (int j = 0; j < 4; ++j) hb2[j] = pf[j < nl ? sg[j] + (ln[j] > 1 ? 1 : 0) : 0];
    PSTAMP_WAIT();
    PSTAMP(k, 3);
    float gw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gw[j] = gz[hb[j]];
    // (keeps the second members' loads up here: sunk into the pair branch they would be a round trip of their own)
    asm volatile("" : "+v"(hb2[0]), "+v"(hb2[1]), "+v"(hb2[2]), "+v"(hb2[3]));
    PSTAMP_WAIT();
    PSTAMP(k, 4);
    const int dst = before + u0;
    // pairs (nearly every multi-member run of a uniform batch): the owning lane, head row + second member.  A lane takes
    // its pairs one after the other, the lanes of a wave theirs at the same time: a wave (2.7 pairs on average with
    // uniform ids) is one round trip behind its slowest lane, not one per position of the quadruple that holds a pair
    // (taken position by position the launch measured 8.9 us, so 7.8)
    const bool anylong = ln[0] > 2 || ln[1] > 2 || ln[2] > 2 || ln[3] > 2;
    unsigned pm = (ln[0] == 2 ? 1u : 0u) | (ln[1] == 2 ? 2u : 0u) | (ln[2] == 2 ? 4u : 0u) | (ln[3] == 2 ? 8u : 0u);
    while (pm) {
      const int j = __ffs((int)pm) - 1;
      pm &= pm - 1;
      const int b2 = j == 0 ? hb2[0] : j == 1 ? hb2[1] : j == 2 ? hb2[2] : hb2[3];
      const float4* r2 = vals + (b2 * F + f) * 4;
      float4* hr = g_embed + (dst + j) * 4;
      float4 a0 = hr[0], a1 = hr[1], a2 = hr[2], a3 = hr[3];
      const float4 x0 = r2[0], x1 = r2[1], x2 = r2[2], x3 = r2[3];
      const float g2 = gz[b2];
      a0.x += x0.x; a0.y += x0.y; a0.z += x0.z; a0.w += x0.w;
      a1.x += x1.x; a1.y += x1.y; a1.z += x1.z; a1.w += x1.w;
      a2.x += x2.x; a2.y += x2.y; a2.z += x2.z; a2.w += x2.w;
      a3.x += x3.x; a3.y += x3.y; a3.z += x3.z; a3.w += x3.w;
      hr[0] = a0; hr[1] = a1; hr[2] = a2; hr[3] = a3;
#pragma unroll
      for (int i = 0; i < 4; ++i) gw[i] = i == j ? gw[i] + g2 : gw[i];
    }
    // first-order rows of the runs of one and two members (a longer run's is written by whoever sums the run -- in a
    // skewed column another workgroup: a quadruple that holds one leaves its g_w element by element)
    if (nl >= 4 && !anylong && (dst & 3) == 0) {
      *reinterpret_cast<float4*>(k.g_w + dst) = make_float4(gw[0], gw[1], gw[2], gw[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ln[j] == 1 || ln[j] == 2) k.g_w[dst + j] = gw[j];
    }
    PSTAMP(k, 5);
  }
  // a column without skew: its few runs of more than two members
  if (helper && !skew) {
    const int nl = nu - u0;
    const int sg[5] = {sg4.x, sg4.y, sg4.z, sg4.w, sg4e};
    PSTAMP_WAIT();
    PSTAMP(k, 2);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      fix_wave_runs<int, true>(k, pf, f, before, __ballot(j < nl && sg[j + 1] - sg[j] > 2), sg[j], sg[j + 1], u0 + j, 0.f);
  }
  if (bidx == 0 && tid == 0) *k.n_uniq = total;
  if (skew) {
    if (tid == 0) sh.huge_n = 0;
    __syncthreads();
    fix_skew_runs<int>(k, sh, pf, f, before, nu, true, wgc * FIX_T + tid);
  }
  PSTAMP(k, 6);
}

// QUADS: the fix-up workgroups come FIRST in the grid.  Their job is a chain of dependent round trips (col_nu, plan
// words, perm, rows of the pairs), the reduction a 2.5-us flood of independent loads that ends at 4 us either way: with
// the plan words asked for ahead of the flood the launch measured 7.5 us against 7.8 (profiles/r09_post_stamps.txt)
template <bool QUADS>
__global__ __launch_bounds__(1024, 8) void deepfm_post_direct_kernel(ReduceArgs r, ColSegArgs k, int nb_reduce) {
  if (QUADS) {
    const int nbf = (int)gridDim.x - nb_reduce;
    if ((int)blockIdx.x < nbf) fixq_body(k, (int)blockIdx.x);
    else reduce_body(r, (int)blockIdx.x - nbf);
    return;
  }
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

#ifdef REC_POST_STAMPS
static unsigned long long* g_post_stamps = nullptr;
constexpr size_t POST_STAMP_WGS = 4096;
// stamps of the last direct-mode launch: [workgroup][wave 16][8] wall-clock words (a wave leaves the words of phases
// it did not reach as an earlier launch left them)
extern "C" int rec_debug_post_stamps(unsigned long long* host_out, int n_wg) {
  if (!g_post_stamps || n_wg < 0 || (size_t)n_wg > POST_STAMP_WGS) return REC_E_ARG;
  return (int)hipMemcpy(host_out, g_post_stamps, sizeof(unsigned long long) * 8 * 16 * (size_t)n_wg, hipMemcpyDeviceToHost);
}
#endif

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
  if (B > (((int64_t)1 << 31) - 1) / ((int64_t)F * E16)) return REC_E_UNSUPPORTED;   // 32-bit offsets into the row arrays
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
#ifdef REC_POST_STAMPS
    if (nb + nbf > POST_STAMP_WGS) return REC_E_UNSUPPORTED;
    if (!g_post_stamps &&
        (hipMalloc(&g_post_stamps, sizeof(unsigned long long) * 8 * 16 * POST_STAMP_WGS) != hipSuccess ||
         hipMemset(g_post_stamps, 0, sizeof(unsigned long long) * 8 * 16 * POST_STAMP_WGS) != hipSuccess))
      return REC_E_ARG;
    r.stamps = g_post_stamps;
    k.stamps = g_post_stamps;
#endif
    // four runs per lane (fixq_body) where a workgroup's 1024 slots are whole quadruples and the 16-byte pieces of the
    // plan and of the outputs are aligned; the lazy Adam stays with the one-run-per-lane body
    bool quads = !adam && (B % FIX_T) == 0 && rec_is_aligned16(col_uid) && rec_is_aligned16(uniq_ids) &&
                 rec_is_aligned16(g_w_rows);
#ifdef REC_POST_NO_QUADS
    quads = false;                                       // (diagnostic builds: the one-run-per-lane body everywhere)
#endif
    if (quads)
      hipLaunchKernelGGL(deepfm_post_direct_kernel<true>, dim3(nb + nbf), dim3(1024), 0, as_stream(stream), r, k, (int)nb);
    else
      hipLaunchKernelGGL(deepfm_post_direct_kernel<false>, dim3(nb + nbf), dim3(1024), 0, as_stream(stream), r, k, (int)nb);
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