// De-duplication plan of the fused DeepFM steps (the fused step and the row-sharded step): the DataGenerator contract
// (2.FM/DataGenerator.py:76-88) gives every feature column its own contiguous id range, so duplicates only occur inside a
// column.  One 1024-thread workgroup sorts a column (B <= 16384 ids) in LDS as 32-bit (key << PB | position) words and
// finds the runs.  The plan depends on ids only: the engine sorts upcoming batches ahead, up to 256 columns per launch.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// per-column sort of the de-duplication plan (the DataGenerator contract gives every feature column its own contiguous
// id range, so duplicates only occur inside a column): 32-bit words (key << pos_bits | example), key = id - col_lo.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t PADW = 0xFFFFFFFFu;

struct ColSortArgs {
  int64_t B; int F; int64_t V; int key_bits; int pos_bits;
  int32_t* perm;        // [F][B]  sorted position -> example
  int64_t* col_uid;     // [F][B]  unique ids of the column, ascending (first col_nu[f] valid)
  int32_t* col_seg;     // [F][B+1] run starts in the column's sorted order (tail = B)
  int32_t* col_nu;      // [F]
  int* bad;
  int32_t* dloc;        // [F][B] or null: run index of lookup (f, example) inside its column, sign bit = not the run's head
};

// ------------------------------------------------------------------------------------------------
// ONE kernel: one 1024-thread workgroup per column sorts the column's <= 16384 words in LDS (stable LSD radix sort on
// the key bits, 7 bits per pass, in place: every key is in a register between the barrier that ends the reads and the
// one that starts the writes) and goes straight on to the run heads.  (Round 1 ran a chunk-sort / rank-merge / heads
// chain of three latency-bound launches on ~200 CUs: 65 us for the plans of four batches against 42 us here on
// 4 x F workgroups of 37 KB of LDS.)
//   ranking: element e = wave*64*KPT + round*64 + lane, so (wave, round, lane) order is array order; lanes of equal
//   digit are matched by 7 ballots, the lowest lane of a group bumps the wave's 16-bit counter of the digit (LDS
//   operations of one wave complete in program order); a key's new place = digit base + counts of earlier waves + its
//   rank in the wave.
// ------------------------------------------------------------------------------------------------
constexpr int OW_T = 1024, OW_W = OW_T / 64, OW_BINS = 128, OW_DB = 7;

#ifdef REC_SORT_STAMPS
__device__ unsigned long long g_sort_stamps[256 * 16];
#define SSTAMP(k) do { if (threadIdx.x == 0) g_sort_stamps[blockIdx.x * 16 + (k)] = wall_clock64(); } while (0)
#else
#define SSTAMP(k) do {} while (0)
#endif

// up to 256 columns per launch (8 batches of 26..32 columns: ONE launch per 8 upcoming batches -- every sort launch holds
// its CUs for the duration of a latency-bound kernel, and a fused kernel that finds CUs taken runs a second round)
constexpr int SORT_MAX_COLS = 256;
struct SortCols {
  const int64_t* p[SORT_MAX_COLS];
};

template <int KPT>
__global__ __launch_bounds__(OW_T, 4) void colsort_onewg_kernel(SortCols cols, const int64_t* __restrict__ col_lo, ColSortArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t owl[];
  constexpr int NW = OW_T * KPT;                       // padded word count
  uint32_t* words = owl;                               // [NW]
  unsigned short* cnt = reinterpret_cast<unsigned short*>(owl + NW);      // [OW_W][OW_BINS]
  uint32_t* dbase = owl + NW + OW_W * OW_BINS / 2;     // [OW_BINS]
  uint32_t* wtot = dbase + OW_BINS;                    // [OW_W] scratch of the block scans
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.x;
  const int64_t B = a.B;
  const int64_t lo = col_lo[f];
  const int pb = a.pos_bits;
  const uint32_t pmask = (1u << pb) - 1u;
  // ---- load: word = (id - lo) << pos_bits | example; pad words sort last
  SSTAMP(0);
  bool bad = false;
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int e = r * OW_T + tid;
    uint32_t w = PADW;
    if (e < B) {
      const int64_t id = cols.p[f][e];
      int64_t key = id - lo;
      if (key < 0 || key >= (int64_t(1) << a.key_bits) || (uint64_t)id >= (uint64_t)a.V) {
        bad = true;
        key = key < 0 ? 0 : (int64_t(1) << a.key_bits) - 1;
      }
      w = ((uint32_t)key << pb) | (uint32_t)e;
    }
    words[e] = w;
  }
  if (bad && a.bad) *a.bad = 1;
  SSTAMP(1);
  const unsigned long long lt = (1ull << lane) - 1ull;
  int pass_ = 0;
  // ---- radix passes over the key bits
  for (int shift = pb; shift < pb + a.key_bits; shift += OW_DB) {
    reinterpret_cast<uint32_t*>(cnt)[tid] = 0;         // OW_W*OW_BINS/2 = 1024 words
    __syncthreads();
    uint32_t w[KPT];
    unsigned short loc[KPT];
#pragma unroll
    for (int r = 0; r < KPT; ++r) w[r] = words[wave * (64 * KPT) + r * 64 + lane];
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const uint32_t d = (w[r] >> shift) & (OW_BINS - 1);
      unsigned long long m = ~0ull;
#pragma unroll
      for (int b = 0; b < OW_DB; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        m &= bit ? bal : ~bal;
      }
      const unsigned short old = cnt[wave * OW_BINS + d];
      if ((m & lt) == 0) cnt[wave * OW_BINS + d] = (unsigned short)(old + __popcll(m));
      loc[r] = (unsigned short)(old + __popcll(m & lt));
    }
    __syncthreads();                                   // every word is in a register: the array may be overwritten
    if (tid < OW_BINS) {                               // per digit: counts -> exclusive prefix over the waves, total
      uint32_t run = 0;
#pragma unroll
      for (int q = 0; q < OW_W; ++q) {
        const uint32_t c = cnt[q * OW_BINS + tid];
        cnt[q * OW_BINS + tid] = (unsigned short)run;
        run += c;
      }
      // exclusive scan of the 128 totals (two waves)
      uint32_t incl = run;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (lane == 63) wtot[wave] = incl;
      dbase[tid] = incl - run;                         // within the wave; wave 1 adds wave 0's total below
    }
    __syncthreads();
    if (tid >= 64 && tid < OW_BINS) dbase[tid] += wtot[0];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const uint32_t d = (w[r] >> shift) & (OW_BINS - 1);
      words[dbase[d] + cnt[wave * OW_BINS + d] + loc[r]] = w[r];
    }
    __syncthreads();
    SSTAMP(2 + pass_);
    ++pass_;
  }
  // ---- run heads: thread t owns the KPT consecutive sorted positions from t*KPT
  const int s0 = tid * KPT;
  uint32_t v[KPT];
  bool hd[KPT];
  int heads = 0;
  uint32_t prev = s0 > 0 ? words[s0 - 1] : PADW;
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int sp = s0 + r;
    v[r] = words[sp];
    const uint32_t pk = (r == 0 ? prev : v[r - 1]) >> pb;
    hd[r] = sp < B && (sp == 0 || (v[r] >> pb) != pk);
    heads += hd[r] ? 1 : 0;
  }
  int incl = heads;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wtot[wave] = (uint32_t)incl;
  __syncthreads();
  int woff = 0, all = 0;
  for (int q = 0; q < OW_W; ++q) {
    const int c = (int)wtot[q];
    if (q < wave) woff += c;
    all += c;
  }
  int rank = woff + incl - heads;
  // Outputs go through LDS and leave coalesced.  (Stored straight from the registers -- a lane owns 8 consecutive sorted
  // positions -- every wave instruction wrote 64 scattered 4- or 8-byte pieces: ~32 such instructions per wave on one
  // address path, and the last wave finished 12 us after the first, 36 us into a kernel whose sort is done at 19.)
  //   st_uq [rank]    key of the run (aliases `words`: every thread holds its words in registers behind the barrier above)
  //   st_sg [rank]    first sorted position of the run         (16 bit: B <= 16384)
  //   st_dl [example] run index | 0x8000 unless head of its run (16 bit)
  uint32_t* st_uq = words;
  unsigned short* st_sg = reinterpret_cast<unsigned short*>(wtot + OW_W);
  unsigned short* st_dl = st_sg + NW;
  int32_t* permf = a.perm + (int64_t)f * B;
  if ((B & 7) == 0 && KPT == 8) {
    // the thread's 8 consecutive perm entries as two 16-byte stores: a wave writes 2 KB of contiguous memory
    if (s0 < B) {
      int4 p0 = make_int4((int)(v[0] & pmask), (int)(v[1] & pmask), (int)(v[2] & pmask), (int)(v[3] & pmask));
      int4 p1 = make_int4((int)(v[4 % KPT] & pmask), (int)(v[5 % KPT] & pmask), (int)(v[6 % KPT] & pmask), (int)(v[7 % KPT] & pmask));
      *reinterpret_cast<int4*>(permf + s0) = p0;
      *reinterpret_cast<int4*>(permf + s0 + 4) = p1;
    }
  } else {
#pragma unroll
    for (int r = 0; r < KPT; ++r)
      if (s0 + r < B) permf[s0 + r] = (int32_t)(v[r] & pmask);
  }
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int sp = s0 + r;
    if (sp < B) {
      if (hd[r]) {
        st_uq[rank] = v[r] >> pb;
        st_sg[rank] = (unsigned short)sp;
        ++rank;
      }
      st_dl[v[r] & pmask] = (unsigned short)(hd[r] ? (rank - 1) : ((rank - 1) | 0x8000));
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int i = r * OW_T + tid;
    if (i < B) {
      if (a.dloc) {
        const uint32_t d = st_dl[i];
        a.dloc[(int64_t)f * B + i] = (int32_t)((d & 0x7FFFu) | ((d & 0x8000u) << 16));
      }
      if (i < all) {
        a.col_uid[(int64_t)f * B + i] = lo + (int64_t)st_uq[i];
        a.col_seg[(int64_t)f * (B + 1) + i] = (int32_t)st_sg[i];
      } else {
        a.col_seg[(int64_t)f * (B + 1) + i] = (int32_t)B;           // tail [all .. B] = B
      }
    }
  }
  if (tid == 0) a.col_seg[(int64_t)f * (B + 1) + B] = (int32_t)B;
  if (tid == 0) a.col_nu[f] = all;
  SSTAMP(8);
#ifdef REC_SORT_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  SSTAMP(9);
  if (threadIdx.x == 1023) g_sort_stamps[blockIdx.x * 16 + 10] = wall_clock64();
  if (threadIdx.x == 512) g_sort_stamps[blockIdx.x * 16 + 11] = wall_clock64();
#endif
}
}  // namespace

#ifdef REC_SORT_STAMPS
extern "C" int rec_debug_sort_stamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_sort_stamps), sizeof(unsigned long long) * 256 * 16);
}
#endif
extern "C" size_t rec_colsort_workspace_bytes(int64_t B, int F) {
  if (B <= 0 || F <= 0) return 0;
  return 256;      // the sort runs in LDS; the argument is kept for callers written against the three-kernel version
}

static int colsort_plan(const int64_t* const* cols_host, int F, int64_t B, int64_t V, const int64_t* col_lo,
                        int64_t max_key, int32_t* perm, int64_t* col_uid, int32_t* col_seg, int32_t* col_nu,
                        int32_t* dloc, int* bad_flag, void* workspace, void* stream) {
  if (!cols_host || !col_lo || !perm || !col_uid || !col_seg || !col_nu || !workspace || F <= 0 || B <= 0 || V <= 0 ||
      max_key < 0)
    return REC_E_ARG;
  if (F > SORT_MAX_COLS || B > 16384) return REC_E_UNSUPPORTED;
  int pos_bits = 1, key_bits = 1;
  while ((int64_t(1) << pos_bits) < B) ++pos_bits;
  while ((int64_t(1) << key_bits) <= max_key) ++key_bits;
  if (key_bits + pos_bits > 32) return REC_E_UNSUPPORTED;
  // the pad word 0xFFFFFFFF must be larger than every real (key, position) word
  if ((((uint64_t)max_key << pos_bits) | (uint64_t)(B - 1)) >= 0xFFFFFFFFull) return REC_E_UNSUPPORTED;
  SortCols cp;
  for (int f = 0; f < F; ++f) {
    if (!cols_host[f]) return REC_E_ARG;
    cp.p[f] = cols_host[f];
  }
  ColSortArgs a{B, F, V, key_bits, pos_bits, perm, col_uid, col_seg, col_nu, bad_flag, dloc};
  hipStream_t st = as_stream(stream);
  // one workgroup per column (LDS radix sort + run heads in one launch); columns longer than 16 x 1024 do not occur
  // (B <= 16384)
  {
    const int kpt = B <= 8192 ? 8 : 16;
    // words + counters + the 16-bit staging arrays of the outputs (st_sg, st_dl)
    const size_t lds = sizeof(uint32_t) * ((size_t)OW_T * kpt + OW_W * OW_BINS / 2 + OW_BINS + OW_W) +
                       2 * sizeof(unsigned short) * (size_t)OW_T * kpt;
    hipError_t e;
    if (kpt == 8) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(colsort_onewg_kernel<8>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(colsort_onewg_kernel<8>, dim3(F), dim3(OW_T), lds, st, cp, col_lo, a);
    } else {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(colsort_onewg_kernel<16>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(colsort_onewg_kernel<16>, dim3(F), dim3(OW_T), lds, st, cp, col_lo, a);
    }
    REC_LAUNCH_CHECK();
    return REC_OK;
  }
}

extern "C" int rec_colsort_plan_i64(const int64_t* const* cols_host, int F, int64_t B, int64_t V, const int64_t* col_lo,
                                    int64_t max_key, int32_t* perm, int64_t* col_uid, int32_t* col_seg, int32_t* col_nu,
                                    int* bad_flag, void* workspace, void* stream) {
  return colsort_plan(cols_host, F, B, V, col_lo, max_key, perm, col_uid, col_seg, col_nu, nullptr, bad_flag, workspace,
                      stream);
}

extern "C" int rec_colsort_plan_dest_i64(const int64_t* const* cols_host, int F, int64_t B, int64_t V,
                                         const int64_t* col_lo, int64_t max_key, int32_t* perm, int64_t* col_uid,
                                         int32_t* col_seg, int32_t* col_nu, int32_t* dloc, int* bad_flag, void* workspace,
                                         void* stream) {
  if (!dloc) return REC_E_ARG;
  return colsort_plan(cols_host, F, B, V, col_lo, max_key, perm, col_uid, col_seg, col_nu, dloc, bad_flag, workspace,
                      stream);
}