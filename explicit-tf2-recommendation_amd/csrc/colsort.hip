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
  int64_t B; int F; int64_t V; int key_bits; int pos_bits; int passes; int digit_bits;
  int32_t* perm;        // [F][B]  sorted position -> example
  int64_t* col_uid;     // [F][B]  unique ids of the column, ascending (first col_nu[f] valid)
  int32_t* col_seg;     // [F][B+1] run starts in the column's sorted order (tail = B)
  int32_t* col_nu;      // [F]
  int* bad;
  int64_t max_key;      // largest key of the launch (the widest field's dim - 1)
  int bm_words;         // bitmap path: 32-bit words that cover keys 0 .. max_key; 0 = the launch does not take it
  int32_t* dloc;        // [F][B] or null: run index of lookup (f, example) inside its column, sign bit = not the run's head
};

// ------------------------------------------------------------------------------------------------
// ONE kernel: one 1024-thread workgroup per column sorts the column's <= 16384 words in LDS and goes straight on to the
// run heads.  Columns without a hot bucket take the bitmap path (no sort at all: CS_BM_WORDS below) when the launch's key
// range fits it, else the bucket path below; the others a stable LSD radix sort on the key
// bits in as few passes of at most 10 bits as cover the key (19-bit keys: 10 + 9), in place: every key is in a register
// between the barrier that ends the reads and the one that starts the writes.  (Round 1 ran a chunk-sort / rank-merge /
// heads chain of three latency-bound launches.)
//   ranking: element e = wave*64*KPT + round*64 + lane, so (wave, round, lane) order is array order; lanes of equal
//   digit are matched by one ballot per digit bit, the lowest lane of a group adds the group's size to the wave's 32-bit
//   counter of the digit with an LDS atomic that returns the old count, and the group reads that count from its lowest
//   lane.  A wave's LDS operations complete in program order, so the KPT atomics of a pass go out back to back and are
//   waited for once.  A key's new place = digit base + counts of earlier waves + its rank in the wave.
//   (Round 3 ran 3 passes of 7 bits, each round of a pass a dependent read-modify-write of a 16-bit counter: 5.7 us per
//   pass at B = 8192.)
// ------------------------------------------------------------------------------------------------
constexpr int CS_T = 1024, CS_W = CS_T / 64, CS_DB = 10, CS_BINS = 1 << CS_DB;
// bucket path: 2^13 buckets of the top word bits (8 per thread), taken when no bucket holds more than CS_BIG words and
// no round of 64 words has more than CS_PROBE in lane 0's bucket
constexpr int CS_BKB = 13, CS_NBK = 1 << CS_BKB, CS_BIG = 32, CS_PROBE = 16;
static_assert(CS_BINS == CS_T, "the count scan gives every thread one digit");
// bitmap path (8 words per thread only: B <= 8192): a launch whose keys 0 .. max_key fit CS_BM_WORDS 32-bit words ranks
// a column without sorting it.  One bit per distinct key; the popcount prefix over the words is the ascending rank of
// every distinct id.  A lookup whose word holds no duplicated id has its sorted position from two prefixes and one
// popcount; the lookups of the other words ("slow") go to a list, every such word to a segment of its own.
//   LDS, inside the other paths' arrays (32-bit word offsets; `wtot` behind them is shared):
//     bm   [CS_BM_WORDS]          the bitmap                                            4 bytes per word
//     xc   [CS_BM_WORDS] 16 bit   lookups - distinct keys of the word; after the scan the lookups beyond the distinct
//                                 keys in all earlier words, or 0x8000 | index of the word's record   2 bytes per word
//     pu   [CS_BM_WORDS / 2] 16 bit  distinct keys before the PAIR of words (one 8-byte read gives a lookup its pair of
//                                 the bitmap: the odd word adds the even word's popcount)             1 byte per word
//     list [CS_BM_CAP]            sort words of the slow lookups, one segment per slow word
//     rec  [CS_BM_CAP / 2] x 2    per slow word: (extras before | segment start << 16, append cursor -> segment end)
//   7 bytes per word + 8 per list entry inside the 98 KB the kernel has at 8 words per thread: 13 x 1024 words =
//   425,984 keys (the headline's widest field: 384,625 keys = 12,020 words).  The widest legal key at B = 8192
//   (2^19 - 2: 16,384 words) would need 112 KB and stays on the bucket path, as does B > 8192 (16 words per thread, keys
//   of at most 18 bits: a uniform column there has more than a thousand slow lookups, see CS_BM_CAP).
// CS_BM_CAP: a word's segment is scanned by each of its members, so the work does not grow with the list, only the LDS
// does (8 bytes per entry).  512 = the largest power of two that leaves the bitmap its 13 K words; uniform headline
// columns have 229 slow lookups on average and 329 at most in 2000 draws.  The stamps put the bitmap's own work (set,
// scan: ~6 us) in front of the test, which a column over the cap pays before it starts the bucket path.
constexpr int CS_BM_WORDS = 13 * CS_T, CS_BM_CAP = 512, CS_BM_PPT = 7;
constexpr int CS_BM_XC = CS_BM_WORDS, CS_BM_PU = CS_BM_XC + CS_BM_WORDS / 2, CS_BM_LIST = CS_BM_PU + CS_BM_WORDS / 4,
              CS_BM_REC = CS_BM_LIST + CS_BM_CAP, CS_BM_WTOT = CS_BM_REC + CS_BM_CAP, CS_BM_END = CS_BM_WTOT + CS_W;
static_assert(CS_BM_PPT * CS_T * 2 >= CS_BM_WORDS && CS_BM_WORDS % 8 == 0, "the scan covers the bitmap, 16-byte zeroing");
static_assert(CS_BM_END <= CS_T * 8 + CS_W * CS_BINS, "the bitmap path fits the LDS of the other paths at 8 words per thread");
static_assert(CS_BM_REC % 2 == 0 && CS_BM_XC % 4 == 0, "8-byte records, 16-byte zeroing of xc");
// its output staging: 32-bit keys [8192], 16-bit run starts [8192], 16-bit perm [8192] -- below the list and the records
static_assert(CS_T * 8 * 2 <= CS_BM_PU, "the staging leaves pu, list and records alone");

#ifdef REC_SORT_STAMPS
__device__ unsigned long long g_sort_stamps[256 * 16];
#define SSTAMP(k) do { if (threadIdx.x == 0) g_sort_stamps[blockIdx.x * 16 + (k)] = wall_clock64(); } while (0)
#define SSTAMP_END() do { SSTAMP(8); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); SSTAMP(9); \
    if (threadIdx.x == 1023) g_sort_stamps[blockIdx.x * 16 + 10] = wall_clock64(); \
    if (threadIdx.x == 512) g_sort_stamps[blockIdx.x * 16 + 11] = wall_clock64(); } while (0)
#else
#define SSTAMP(k) do {} while (0)
#define SSTAMP_END() do {} while (0)
#endif

// up to 256 columns per launch (8 batches of 26..32 columns: ONE launch per 8 upcoming batches -- every sort launch holds
// its CUs for the duration of a latency-bound kernel, and a fused kernel that finds CUs taken runs a second round)
constexpr int SORT_MAX_COLS = 256;
struct SortCols {
  const int64_t* p[SORT_MAX_COLS];
};

// radix passes of key_bits-bit keys: as few passes of at most CS_DB bits as cover the key, the bits spread evenly over
// them (the last pass takes what is left)
static inline void colsort_digits(int key_bits, int* passes, int* digit_bits) {
  const int p = (key_bits + CS_DB - 1) / CS_DB;
  *passes = p;
  *digit_bits = (key_bits + p - 1) / p;
}

template <int KPT>
__global__ __launch_bounds__(CS_T, 4) void colsort_kernel(SortCols cols, const int64_t* __restrict__ col_lo, ColSortArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sml[];
  constexpr int NW = CS_T * KPT;                       // padded word count
  uint32_t* words = sml;                               // [NW]
  uint32_t* cnt = sml + NW;                            // [CS_W][CS_BINS] per-wave digit counts, then scatter bases
  uint32_t* wtot = cnt + CS_W * CS_BINS;               // [CS_W] scratch of the block scans
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.x;
  const int64_t B = a.B;
  const int64_t lo = col_lo[f];
  const int pb = a.pos_bits;
  const uint32_t pmask = (1u << pb) - 1u;
  uint32_t* wcnt = cnt + wave * CS_BINS;
  const unsigned long long lt = (1ull << lane) - 1ull;
  // ---- load straight into the ranking layout (e = wave*64*KPT + round*64 + lane): word = (id - lo) << pos_bits | example; pad words sort last
  SSTAMP(0);
  uint32_t w[KPT];
  bool bad = false;
  const int nw = KPT == 8 ? a.bm_words : 0;            // bitmap words of the launch (0: no bitmap path)
  int hot = 0;
  const int64_t* col = cols.p[f];
  int64_t id[KPT];
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int e = wave * (64 * KPT) + r * 64 + lane;
    id[r] = e < B ? col[e] : lo;
  }
  // bitmap and per-word counts are cleared while the ids are in flight (words and counts are read in pairs: both
  // arrays in 16-byte pieces, past an odd last word)
  uint32_t* bm = sml;
  uint32_t* xc32 = sml + CS_BM_XC;
  for (int i = tid; i < (nw + 3) / 4; i += CS_T) reinterpret_cast<uint4*>(bm)[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int i = tid; i < (nw + 7) / 8; i += CS_T) reinterpret_cast<uint4*>(xc32)[i] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int e = wave * (64 * KPT) + r * 64 + lane;
    w[r] = PADW;
    if (e < B) {
      int64_t key = id[r] - lo;
      if (key < 0 || key >= (int64_t(1) << a.key_bits) || (uint64_t)id[r] >= (uint64_t)a.V) {
        bad = true;
        key = key < 0 ? 0 : (int64_t(1) << a.key_bits) - 1;
      }
      // a key beyond the launch's largest (a clamped id, an id of a neighbouring field) has no bit: radix passes
      if (nw && key > a.max_key) hot = 1;
      w[r] = ((uint32_t)key << pb) | (uint32_t)e;
    }
  }
  if (bad && a.bad) *a.bad = 1;
  SSTAMP(1);
  // ---- bucket path: the words are unique, so ANY sort of the full word gives the one sorted order, stable or not.
  // Count the words per bucket of their top CS_BKB bits (LDS atomics), scan, scatter every word to a slot of its
  // bucket (atomic cursor: order inside a bucket arbitrary), then rank each word inside its bucket by counting the
  // smaller words there.  Linear in the bucket size, so a column with a bucket of more than CS_BIG words (hot ids,
  // narrow fields) takes the radix passes below instead.  Counts, then bucket starts, then (after the scatter) bucket
  // ends live in the counter array: bucket b = [end of b - 1, end of b).
  const int wbits = a.key_bits + pb;
  const int bsh = wbits > CS_BKB ? wbits - CS_BKB : 0;
  uint32_t* bk = cnt;                                  // [CS_NBK]
  static_assert(CS_NBK == 8 * CS_T && CS_NBK <= CS_W * CS_BINS, "8 buckets per thread, inside the counters");
  if (!nw) {
#pragma unroll
    for (int i = 0; i < 2; ++i) reinterpret_cast<uint4*>(bk)[i * CS_T + tid] = make_uint4(0u, 0u, 0u, 0u);
  }
  // probe: more than CS_PROBE words of a round share lane 0's bucket -> a hot bucket.  Such a column takes the radix
  // passes without counting (64 lanes adding to one LDS address serialise: Zipf heads cost 1.3 us more counting)
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const bool real = wave * (64 * KPT) + r * 64 + lane < B;
    const uint32_t b0 = __shfl(w[r] >> bsh, 0, 64);
    hot |= __popcll(__ballot(real && (w[r] >> bsh) == b0)) > CS_PROBE;
  }
  bool fast = !__syncthreads_or(hot);                 // (uniform over the workgroup, as every test below)
  if (KPT == 8 && nw && fast) {
    // ---- bitmap path.  Set the bits; a lookup that finds its bit set is one more than the distinct keys of its word
    // (the total per word does not depend on the order of arrival).  Here and below every loop issues its LDS
    // operations back to back and uses the results in a loop of its own: a wave's LDS operations complete in order, so
    // the 8 of a loop are waited for once.
    uint32_t was[KPT];
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const uint32_t key = w[r] >> pb, bit = 1u << (key & 31u);
      was[r] = 0u;
      if (wave * (64 * KPT) + r * 64 + lane < B) was[r] = atomicOr(&bm[key >> 5], bit) & bit;
    }
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const uint32_t wd = w[r] >> (pb + 5);
      if (was[r]) atomicAdd(&xc32[wd >> 1], (wd & 1u) ? 0x10000u : 1u);
    }
    __syncthreads();
    SSTAMP(12);
    // scan: thread tid owns the pairs of words CS_BM_PPT tid ...  A = distinct keys | extras << 16 and
    // S = slow words | slow lookups << 16 (a slow word: one with extras; all of its lookups are slow); no field passes
    // B <= 8192
    const int npairs = (nw + 1) >> 1;
    const uint2* bm2 = reinterpret_cast<const uint2*>(bm);
    uint2 bw[CS_BM_PPT];
    uint32_t xw[CS_BM_PPT];
#pragma unroll
    for (int i = 0; i < CS_BM_PPT; ++i) {
      const int p = min(tid * CS_BM_PPT + i, npairs - 1);
      bw[i] = bm2[p];
      xw[i] = xc32[p];
    }
    uint32_t accA = 0, accS = 0;
#pragma unroll
    for (int i = 0; i < CS_BM_PPT; ++i) {
      if (tid * CS_BM_PPT + i >= npairs) {
        bw[i] = make_uint2(0u, 0u);
        xw[i] = 0u;
      }
      const uint32_t x0 = xw[i] & 0xFFFFu, x1 = xw[i] >> 16;
      const uint32_t c0 = (uint32_t)__popc(bw[i].x), c1 = (uint32_t)__popc(bw[i].y);
      accA += c0 + c1 + ((x0 + x1) << 16);
      accS += (x0 ? 1u + ((c0 + x0) << 16) : 0u) + (x1 ? 1u + ((c1 + x1) << 16) : 0u);
    }
    uint32_t inA = accA, inS = accS;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t tA = __shfl_up(inA, o, 64), tS = __shfl_up(inS, o, 64);
      if (lane >= o) {
        inA += tA;
        inS += tS;
      }
    }
    uint32_t* wtotS = sml + CS_BM_WTOT;
    if (lane == 63) {
      wtot[wave] = inA;
      wtotS[wave] = inS;
    }
    __syncthreads();
    uint32_t A = inA - accA, S = inS - accS, allA = 0, allS = 0;
#pragma unroll
    for (int q = 0; q < CS_W; ++q) {
      const uint32_t tA = wtot[q], tS = wtotS[q];
      if (q < wave) {
        A += tA;
        S += tS;
      }
      allA += tA;
      allS += tS;
    }
    const uint32_t nslow = allS >> 16;                   // (uniform: every thread sums the same totals)
    if (nslow <= (uint32_t)CS_BM_CAP) {
      const int all = (int)(allA & 0xFFFFu);
      unsigned short* pu = reinterpret_cast<unsigned short*>(sml + CS_BM_PU);
      uint32_t* list = sml + CS_BM_LIST;
      uint2* rec = reinterpret_cast<uint2*>(sml + CS_BM_REC);
      // the prefixes take the places of the counts
#pragma unroll
      for (int i = 0; i < CS_BM_PPT; ++i) {
        const int p = tid * CS_BM_PPT + i;
        if (p < npairs) {
          const uint32_t xs[2] = {xw[i] & 0xFFFFu, xw[i] >> 16};
          const uint32_t cs[2] = {(uint32_t)__popc(bw[i].x), (uint32_t)__popc(bw[i].y)};
          uint32_t o[2];
          pu[p] = (unsigned short)(A & 0xFFFFu);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            o[h] = A >> 16;                              // extras before this word (< 8192)
            if (xs[h]) {
              o[h] = 0x8000u | (S & 0xFFFFu);
              rec[S & 0xFFFFu] = make_uint2((A >> 16) | (S & 0xFFFF0000u), S >> 16);
              S += 1u + ((cs[h] + xs[h]) << 16);
            }
            A += cs[h] + (xs[h] << 16);
          }
          xc32[p] = o[0] | (o[1] << 16);
        }
      }
      __syncthreads();
      SSTAMP(13);
      // rank: run = distinct keys below the lookup's; a fast lookup is its run's head at run + the extras before its
      // word.  A slow lookup only appends its sort word to its word's segment of the list (order arbitrary).
      const unsigned short* xc16 = reinterpret_cast<const unsigned short*>(xc32);
      uint32_t xv[KPT], run[KPT], pos[KPT];
#pragma unroll
      for (int c0 = 0; c0 < KPT; c0 += 4) {              // (4 rounds at a time, as the radix passes take 8: registers)
        uint32_t b0[4], b1[4];                           // the pair of bitmap words (two scalars: no indexed struct)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = c0 + q;
          const bool real = wave * (64 * KPT) + r * 64 + lane < B;
          const uint32_t wd = real ? w[r] >> (pb + 5) : 0u;
          const uint2 t = bm2[wd >> 1];
          b0[q] = t.x;
          b1[q] = t.y;
          xv[r] = real ? (uint32_t)xc16[wd] : 0u;
          run[r] = pu[wd >> 1];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = c0 + q;
          pos[r] = 0u;
          if (xv[r] & 0x8000u) pos[r] = atomicAdd(&rec[xv[r] & 0x7FFFu].y, 1u);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = c0 + q;
          if (xv[r] & 0x8000u) {
            list[pos[r]] = w[r];
          } else {
            const uint32_t key = w[r] >> pb, wd = key >> 5, below = (1u << (key & 31u)) - 1u;
            const uint32_t odd = 0u - (wd & 1u);          // all ones for the pair's second word
            run[r] += (uint32_t)__popc(b0[q] & odd) + (uint32_t)__popc(((b1[q] & odd) | (b0[q] & ~odd)) & below);
            pos[r] = run[r] + xv[r];
          }
        }
      }
      __syncthreads();                                   // the segments are complete
      // slow lookups, one per thread from the list: sorted position = keys and extras before its word + the smaller sort
      // words of its segment; head iff none of those has its key.  Both are counts over a complete segment: the order
      // of the appends does not show.
      uint32_t s_w = 0, s_pos = 0, s_run = 0;
      bool s_hd = false;
      if ((uint32_t)tid < nslow) {
        s_w = list[tid];
        const uint32_t key = s_w >> pb, wd = key >> 5, below = (1u << (key & 31u)) - 1u;
        const uint2 b = bm2[wd >> 1];
        const uint32_t odd = 0u - (wd & 1u), bx = b.x, by = b.y;
        const uint32_t base = pu[wd >> 1] + (uint32_t)__popc(bx & odd);
        const uint2 t = rec[xc16[wd] & 0x7FFFu];
        const uint32_t sb = t.x >> 16, end = min(t.y, (uint32_t)CS_BM_CAP);   // (the segment; never past the list)
        uint32_t v[4], c = 0, same = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = list[min(sb + q, (uint32_t)CS_BM_CAP - 1u)];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool lt = sb + q < end && v[q] < s_w;
          c += lt ? 1u : 0u;
          same += (lt && (v[q] >> pb) == key) ? 1u : 0u;
        }
        for (uint32_t j = sb + 4; j < end; ++j) {
          const uint32_t u = list[j];
          c += u < s_w ? 1u : 0u;
          same += (u < s_w && (u >> pb) == key) ? 1u : 0u;
        }
        s_run = base + (uint32_t)__popc(((by & odd) | (bx & ~odd)) & below);
        s_pos = base + (t.x & 0xFFFFu) + c;
        s_hd = same == 0u;
      }
      __syncthreads();                                   // bitmap, xc and pu are dead: the staging takes their place
      uint32_t* st_uq = sml;
      unsigned short* st_sg = reinterpret_cast<unsigned short*>(sml + NW);
      unsigned short* st_pm = st_sg + NW;
      int32_t* permf = a.perm + (int64_t)f * B;
#pragma unroll
      for (int r = 0; r < KPT; ++r) {
        const int e = wave * (64 * KPT) + r * 64 + lane;
        if (e < B && !(xv[r] & 0x8000u)) {
          st_pm[pos[r]] = (unsigned short)e;
          st_uq[run[r]] = w[r] >> pb;
          st_sg[run[r]] = (unsigned short)pos[r];
          if (a.dloc) a.dloc[(int64_t)f * B + e] = (int32_t)run[r];
        }
      }
      if ((uint32_t)tid < nslow) {
        const uint32_t e = s_w & pmask;
        st_pm[s_pos] = (unsigned short)e;
        if (s_hd) {
          st_uq[s_run] = s_w >> pb;
          st_sg[s_run] = (unsigned short)s_pos;
        }
        if (a.dloc) a.dloc[(int64_t)f * B + e] = (int32_t)(s_run | (s_hd ? 0u : 0x80000000u));
      }
      __syncthreads();
      SSTAMP(14);
      if ((B & 7) == 0) {
        if (tid * 8 < B) {
          const uint4 q = reinterpret_cast<const uint4*>(st_pm)[tid];
          *reinterpret_cast<int4*>(permf + tid * 8) = make_int4((int)(q.x & 0xFFFFu), (int)(q.x >> 16), (int)(q.y & 0xFFFFu), (int)(q.y >> 16));
          *reinterpret_cast<int4*>(permf + tid * 8 + 4) = make_int4((int)(q.z & 0xFFFFu), (int)(q.z >> 16), (int)(q.w & 0xFFFFu), (int)(q.w >> 16));
        }
      } else {
#pragma unroll
        for (int r = 0; r < KPT; ++r)
          if (r * CS_T + tid < B) permf[r * CS_T + tid] = (int32_t)st_pm[r * CS_T + tid];
      }
#pragma unroll
      for (int r = 0; r < KPT; ++r) {
        const int i = r * CS_T + tid;
        if (i < B) {
          if (i < all) {
            a.col_uid[(int64_t)f * B + i] = lo + (int64_t)st_uq[i];
            a.col_seg[(int64_t)f * (B + 1) + i] = (int32_t)st_sg[i];
          } else {
            a.col_seg[(int64_t)f * (B + 1) + i] = (int32_t)B;
          }
        }
      }
      if (tid == 0) a.col_seg[(int64_t)f * (B + 1) + B] = (int32_t)B;
      if (tid == 0) a.col_nu[f] = all;
      SSTAMP_END();
      return;
    }
    // more slow lookups than the list holds: the bucket path from its start (every thread is past its reads of the
    // bitmap: the barrier of the scan)
#pragma unroll
    for (int i = 0; i < 2; ++i) reinterpret_cast<uint4*>(bk)[i * CS_T + tid] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
  }
  if (fast) {
#pragma unroll
    for (int r = 0; r < KPT; ++r)
      if (wave * (64 * KPT) + r * 64 + lane < B) atomicAdd(&bk[w[r] >> bsh], 1u);
    __syncthreads();
    // thread tid: buckets 8 tid .. 8 tid + 7 -> exclusive starts (block scan), largest count
    const uint4 q0 = reinterpret_cast<const uint4*>(bk)[2 * tid], q1 = reinterpret_cast<const uint4*>(bk)[2 * tid + 1];
    uint32_t c[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t run = 0, mx = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      run += c[q];
      mx = max(mx, c[q]);
    }
    uint32_t incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t base = incl - run;
#pragma unroll
    for (int q = 0; q < CS_W; ++q)
      if (q < wave) base += wtot[q];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t n = c[q];
      c[q] = base;
      base += n;
    }
    reinterpret_cast<uint4*>(bk)[2 * tid] = make_uint4(c[0], c[1], c[2], c[3]);
    reinterpret_cast<uint4*>(bk)[2 * tid + 1] = make_uint4(c[4], c[5], c[6], c[7]);
    fast = !__syncthreads_or(mx > (uint32_t)CS_BIG);  // (also the barrier before the scatter)
  }
  SSTAMP(2);
  if (fast) {
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const int e = wave * (64 * KPT) + r * 64 + lane;
      if (e < B) words[atomicAdd(&bk[w[r] >> bsh], 1u)] = w[r];
      else words[e] = PADW;                            // pads keep their places at the end
    }
    __syncthreads();
    SSTAMP(3);
    uint32_t dst[KPT];
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const int e = wave * (64 * KPT) + r * 64 + lane;
      dst[r] = (uint32_t)e;
      if (e < B) {
        const uint32_t b = w[r] >> bsh;
        const uint32_t end = bk[b];
        uint32_t j = b > 0 ? bk[b - 1] : 0u, rk = j;
        for (; j < end; ++j) rk += words[j] < w[r] ? 1u : 0u;
        dst[r] = rk;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < KPT; ++r) words[dst[r]] = w[r];
    __syncthreads();
    SSTAMP(4);
  }
  // ---- radix passes over the key bits (columns the bucket path does not take)
  for (int pass = 0; pass < (fast ? 0 : a.passes); ++pass) {
    const int shift = pb + pass * a.digit_bits;
    const int nb = min(a.digit_bits, a.key_bits - pass * a.digit_bits);    // digit bits of this pass
    const uint32_t dmask = (1u << nb) - 1u;
    if (pass > 0) {
#pragma unroll
      for (int r = 0; r < KPT; ++r) w[r] = words[wave * (64 * KPT) + r * 64 + lane];
    }
    // the wave's own counters (no other wave touches them before the barrier below)
#pragma unroll
    for (int i = 0; i < CS_BINS / 256; ++i) reinterpret_cast<uint4*>(wcnt)[i * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    // rank in the wave, 8 rounds at a time (KPT = 16 would not fit 128 VGPRs in one go)
    uint32_t below[KPT];
#pragma unroll
    for (int c0 = 0; c0 < KPT; c0 += 8) {
      // peers: lanes of the same round whose digit equals this lane's, one ballot per digit bit (rounds interleaved)
      unsigned long long m[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) m[r] = ~0ull;
      for (int b = 0; b < nb; ++b) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          // s = the bit as 0 / ~0 (one bit-field extract); a lane keeps the lanes whose ballot bit equals its own:
          // m &= ~(bal ^ s) -- 6 VALU instructions per round and bit (extract, compare, xor and and-not per half)
          const uint32_t s = (uint32_t)__builtin_amdgcn_sbfe((int)w[c0 + r], shift + b, 1);
          const unsigned long long bal = __ballot(s != 0u);
          m[r] &= ~(bal ^ (((unsigned long long)s << 32) | s));
        }
      }
      uint32_t old[8];
      int lead[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        lead[r] = __ffsll((long long)m[r]) - 1;        // lowest lane of the group
        below[c0 + r] = (uint32_t)__popcll(m[r] & lt);
        old[r] = 0u;
        if (below[c0 + r] == 0u) old[r] = atomicAdd(&wcnt[(w[c0 + r] >> shift) & dmask], (uint32_t)__popcll(m[r]));
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) below[c0 + r] += (uint32_t)__shfl((int)old[r], lead[r], 64);
    }
    __syncthreads();                                   // every word is in a register, every count is in
    {
      // digit tid: counts of the 16 waves -> exclusive prefix over the waves; block scan of the digit totals
      uint32_t c[CS_W];
      uint32_t run = 0;
#pragma unroll
      for (int q = 0; q < CS_W; ++q) {
        c[q] = cnt[q * CS_BINS + tid];
        run += c[q];
      }
      uint32_t incl = run;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (lane == 63) wtot[wave] = incl;
      __syncthreads();
      uint32_t base = incl - run;
#pragma unroll
      for (int q = 0; q < CS_W; ++q)
        if (q < wave) base += wtot[q];
#pragma unroll
      for (int q = 0; q < CS_W; ++q) {
        cnt[q * CS_BINS + tid] = base;                 // first place of (wave q, digit tid)
        base += c[q];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < KPT; ++r) words[wcnt[(w[r] >> shift) & dmask] + below[r]] = w[r];
    __syncthreads();
    SSTAMP(2 + pass);
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
  for (int q = 0; q < CS_W; ++q) {
    const int c = (int)wtot[q];
    if (q < wave) woff += c;
    all += c;
  }
  int rank = woff + incl - heads;
  SSTAMP(7);
  // Outputs go through LDS and leave coalesced.  (Stored straight from the registers -- a lane owns 8 consecutive sorted
  // positions -- every wave instruction wrote 64 scattered 4- or 8-byte pieces: ~32 such instructions per wave on one
  // address path.)
  //   st_uq [rank]    key of the run (aliases `words`: every thread holds its words in registers behind the barrier above)
  //   st_sg [rank]    first sorted position of the run (16 bit: B <= 16384; aliases the counters, dead since the last pass)
  //   st_dl [example] run index | 0x8000 unless head of its run (16 bit)
  static_assert(2 * sizeof(unsigned short) * NW <= sizeof(uint32_t) * CS_W * CS_BINS, "the staging fits the counters");
  uint32_t* st_uq = words;
  unsigned short* st_sg = reinterpret_cast<unsigned short*>(cnt);
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
    const int i = r * CS_T + tid;
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
  SSTAMP_END();
}

// key and position bits of the sort words: REC_OK, or the status the plan calls return
static int colsort_widths(int64_t B, int64_t max_key, int* key_bits, int* pos_bits) {
  if (B <= 0 || max_key < 0) return REC_E_ARG;
  if (B > 16384) return REC_E_UNSUPPORTED;
  int pbits = 1, kbits = 1;
  while ((int64_t(1) << pbits) < B) ++pbits;
  while ((int64_t(1) << kbits) <= max_key) ++kbits;
  if (kbits + pbits > 32) return REC_E_UNSUPPORTED;
  // the pad word 0xFFFFFFFF must be larger than every real (key, position) word
  if ((((uint64_t)max_key << pbits) | (uint64_t)(B - 1)) >= 0xFFFFFFFFull) return REC_E_UNSUPPORTED;
  *key_bits = kbits;
  *pos_bits = pbits;
  return REC_OK;
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

// bitmap words of a launch: ceil((max_key + 1) / 32) when the bitmap path takes it, else 0
static inline int colsort_bitmap_words(int64_t B, int64_t max_key) {
  const int64_t nw = (max_key + 32) / 32;
  return B <= 8192 && nw <= CS_BM_WORDS ? (int)nw : 0;
}

extern "C" int rec_colsort_bitmap_limits(int64_t B, int64_t max_key, int* words, int* slow_cap) {
  if (!words || !slow_cap) return REC_E_ARG;
  int key_bits = 0, pos_bits = 0;
  const int rc = colsort_widths(B, max_key, &key_bits, &pos_bits);
  if (rc != REC_OK) return rc;
  *words = colsort_bitmap_words(B, max_key);
  *slow_cap = CS_BM_CAP;
  return REC_OK;
}

extern "C" int rec_colsort_digits(int64_t B, int64_t max_key, int* passes, int* digit_bits) {
  if (!passes || !digit_bits) return REC_E_ARG;
  int key_bits = 0, pos_bits = 0;
  const int rc = colsort_widths(B, max_key, &key_bits, &pos_bits);
  if (rc != REC_OK) return rc;
  colsort_digits(key_bits, passes, digit_bits);
  return REC_OK;
}

static int colsort_plan(const int64_t* const* cols_host, int F, int64_t B, int64_t V, const int64_t* col_lo,
                        int64_t max_key, int32_t* perm, int64_t* col_uid, int32_t* col_seg, int32_t* col_nu,
                        int32_t* dloc, int* bad_flag, void* workspace, void* stream) {
  if (!cols_host || !col_lo || !perm || !col_uid || !col_seg || !col_nu || !workspace || F <= 0 || B <= 0 || V <= 0 ||
      max_key < 0)
    return REC_E_ARG;
  if (F > SORT_MAX_COLS) return REC_E_UNSUPPORTED;
  int key_bits = 0, pos_bits = 0;
  const int rc = colsort_widths(B, max_key, &key_bits, &pos_bits);
  if (rc != REC_OK) return rc;
  int passes = 0, digit_bits = 0;
  colsort_digits(key_bits, &passes, &digit_bits);
  SortCols cp;
  for (int f = 0; f < F; ++f) {
    if (!cols_host[f]) return REC_E_ARG;
    cp.p[f] = cols_host[f];
  }
  ColSortArgs a{B, F, V, key_bits, pos_bits, passes, digit_bits, perm, col_uid, col_seg, col_nu, bad_flag, max_key,
                colsort_bitmap_words(B, max_key), dloc};
  hipStream_t st = as_stream(stream);
  // one workgroup per column (LDS radix sort + run heads in one launch); B <= 16384 = 16 x 1024
  const int kpt = B <= 8192 ? 8 : 16;
  // words + per-wave counters (the 16-bit staging arrays of the outputs reuse them) + block-scan scratch
  const size_t lds = sizeof(uint32_t) * ((size_t)CS_T * kpt + CS_W * CS_BINS + CS_W);   // one size per kpt
  const hipError_t e = kpt == 8 ? rec_allow_lds<colsort_kernel<8>>(lds) : rec_allow_lds<colsort_kernel<16>>(lds);
  if (e != hipSuccess) return (int)e;
  if (kpt == 8)
    hipLaunchKernelGGL(colsort_kernel<8>, dim3(F), dim3(CS_T), lds, st, cp, col_lo, a);
  else
    hipLaunchKernelGGL(colsort_kernel<16>, dim3(F), dim3(CS_T), lds, st, cp, col_lo, a);
  REC_LAUNCH_CHECK();
  return REC_OK;
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
