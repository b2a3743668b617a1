// Shared helpers for the gfx950 kernels of libmi355rec.so.  Wave = 64 lanes (CDNA4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "mi355rec.h"

#define REC_WAVE 64

#define REC_LAUNCH_CHECK()                      \
  do {                                          \
    hipError_t e_ = hipGetLastError();          \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// wave-level sum over a power-of-two group of `width` adjacent lanes (xor butterfly: every lane gets the sum)
template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
// accurate form used where parity at 1e-6 matters (logits can be large)
__device__ __forceinline__ float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// Sum over the 16 lanes of a DPP row (lanes 16k .. 16k+15), result in every lane, by four v_add_f32 with DPP operands
// (quad_perm xor 1, quad_perm xor 2, row_half_mirror, row_mirror) instead of four ds_bpermute round trips.  After the
// two quad steps every lane of a quad holds the quad's sum, so the mirror steps pair lanes that hold the SAME partial
// on each side: all 16 lanes end with bit-identical sums (a + b == b + a).
template <int CTRL>
__device__ __forceinline__ float dpp_mov_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_allsum(float v) {
  v += dpp_mov_f32<0xB1>(v);     // quad_perm [1,0,3,2]
  v += dpp_mov_f32<0x4E>(v);     // quad_perm [2,3,0,1]
  v += dpp_mov_f32<0x141>(v);    // row_half_mirror: lane i <-> 7 - i inside each half row
  v += dpp_mov_f32<0x140>(v);    // row_mirror: lane i <-> 15 - i
  return v;
}


// Keras Adam on one element with the operation sequence pinned: every multiply-add is an EXPLICIT fma (the compiler may
// fuse `a*b + c` or not, differently in every kernel; an explicit fma it can only keep) and what is left offers nothing to
// fuse.  Every kernel that applies a step -- the dense sweep, the touched-row kernels, the update inside the fused post
// launch, the catch-up of lazily evaluated rows -- therefore produces the same bits:
//   touched   m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2 ; x <- x - lr_t m / (sqrt(v) + eps)
//   untouched m <- b1 m            ; v <- b2 v              ; x <- x - lr_t m / (sqrt(v) + eps)   (Keras' dense sweep)
// The quotient: hardware square root and reciprocal (v_sqrt_f32, v_rcp_f32: 1 ulp each) and ONE pinned fma, not the
// correctly rounded sqrtf() and `/` (35 instruction slots per element and step against 14 -- and the lazily evaluated Adam
// replays ~47 steps per row it touches at 10M rows: that kernel is arithmetic-bound).  m and v are unaffected; the step
// lr_t m / (sqrt(v) + eps) is off by <= ~3 ulp of ITSELF, i.e. far below one ulp of x: x equals the correctly rounded
// evaluation in most steps and differs by one ulp of x in the rest (tests/test_gpu_adam_classes.py holds every kernel
// class to ulp(x) + 6 ulp of the step against an fp64 reference; measured: never past the half ulp of x's own rounding).
// -DREC_ADAM_IEEE restores the correctly rounded form in every kernel at once.
__device__ __forceinline__ float adam_step_x(float x, float m, float v, float lr_t, float eps) {
  const float num = lr_t * m;                        // a product that feeds a division: nothing to fuse
#ifdef REC_ADAM_IEEE
  const float den = sqrtf(v) + eps;
  return x - num / den;
#else
  const float den = __builtin_amdgcn_sqrtf(v) + eps;
  return __builtin_fmaf(-num, __builtin_amdgcn_rcpf(den), x);
#endif
}
__device__ __forceinline__ void adam_touch(float& x, float& m, float& v, float g, float lr_t, float b1, float b2,
                                           float eps) {
  m = __builtin_fmaf(g, 1.f - b1, m * b1);
  v = __builtin_fmaf(g * g, 1.f - b2, v * b2);
  x = adam_step_x(x, m, v, lr_t, eps);
}
// dense parameters (Keras' dense apply): m <- m + (g - m)(1 - b1) ; v <- v + (g^2 - v)(1 - b2)
__device__ __forceinline__ void adam_dense_elem(float& x, float& m, float& v, float g, float lr_t, float b1, float b2,
                                                float eps) {
  m = __builtin_fmaf(g - m, 1.f - b1, m);
  v = __builtin_fmaf(__builtin_fmaf(g, g, -v), 1.f - b2, v);
  x = adam_step_x(x, m, v, lr_t, eps);
}
__device__ __forceinline__ void adam_decay(float& x, float& m, float& v, float lr_t, float b1, float b2, float eps) {
  m = m * b1;
  v = v * b2;
  x = adam_step_x(x, m, v, lr_t, eps);
}

// ------------------------------------------------------------------------------------------------------------------
// host-side launch support: the one copy of what every kernel file needs around a launch
// ------------------------------------------------------------------------------------------------------------------
constexpr size_t REC_LDS_CU_BYTES = 160 * 1024;   // LDS of one CU (gfx950)

// `a` is a power of two
static inline size_t rec_align_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }
static inline bool rec_is_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Lets Kernel be launched with up to cap_bytes of dynamic LDS; nothing to do up to 64 KiB.  cap_bytes is the most its
// launcher can ever ask for (minus the kernel's static LDS), not the size of one launch: the attribute is set once per
// kernel and process -- never again on the launch path or inside a graph capture -- and every later call returns what
// that first call returned.  It bounds the launch size only; occupancy follows the size given at launch.  The once-flag
// is per kernel VALUE (two instantiations of one template share a type).  One process drives one device everywhere
// here, so once per process is once per device.
template <auto Kernel>
static hipError_t rec_allow_lds(size_t cap_bytes) {
  if (cap_bytes <= 64 * 1024) return hipSuccess;
  static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap_bytes);
  return e;
}

// f(std::integral_constant<int, c>) for c = clamp(n, 1, 4): the one spelling of a 1..4 template dispatch
template <class Fn>
static inline int rec_dispatch_1to4(int n, Fn&& f) {
  switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// Deterministic sums of per-workgroup partials (slot_sum.hip): out[t] = sum_s slots[s * n + t] for t < n, where element
// t lands in one of up to 8 destination segments of lengths len[0], len[1], ... (their sum is n).  Two orders of
// addition, and a caller keeps the one its results were defined with:
//   wave    one wave per element: lane l adds slots l, l + 64, ... in order, then the xor butterfly of group_sum<64>
//   serial  one thread per element: slots 0, 1, ..., nslot - 1 in order
struct SlotDst {
  float* p[8];
  int len[8];
};
enum RecSlotOrder { REC_SLOTS_WAVE, REC_SLOTS_SERIAL };

// call as rec_slot_sum(order, n, nslot, slots, {{p0, p1, ...}, {len0, len1, ...}}, stream); REC_OK or an error code
__attribute__((visibility("hidden"))) int rec_slot_sum(RecSlotOrder order, int n, int nslot, const float* slots,
                                                       const SlotDst& dst, hipStream_t st);
