// The two slot-sum kernels behind rec_slot_sum (common.h): every layer that leaves per-workgroup partials in workspace
// slots adds them here, in one of two fixed orders.  No float atomics: bit-identical sums run to run.
#include "common.h"

namespace {

__device__ __forceinline__ void slot_store(const SlotDst& dst, int t, float v) {
  int seg = 0;
  while (t >= dst.len[seg]) t -= dst.len[seg++];
  dst.p[seg][t] = v;
}

__global__ __launch_bounds__(256) void slot_sum_wave_kernel(int n, int nslot, const float* __restrict__ slots,
                                                            SlotDst dst) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= n) return;
  float acc = 0.f;
  for (int s = lane; s < nslot; s += 64) acc += slots[(int64_t)s * n + t];
  acc = group_sum<64>(acc);
  if (lane == 0) slot_store(dst, t, acc);
}

__global__ __launch_bounds__(256) void slot_sum_serial_kernel(int n, int nslot, const float* __restrict__ slots,
                                                              SlotDst dst) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  float acc = 0.f;
  for (int s = 0; s < nslot; ++s) acc += slots[(int64_t)s * n + t];
  slot_store(dst, t, acc);
}

}  // namespace

int rec_slot_sum(RecSlotOrder order, int n, int nslot, const float* slots, const SlotDst& dst, hipStream_t st) {
  int64_t total = 0;
  for (int q = 0; q < 8; ++q) {
    if (dst.len[q] < 0) return REC_E_ARG;
    total += dst.len[q];
  }
  if (n < 1 || nslot < 0 || total != n) return REC_E_ARG;               // the kernels walk the segments unchecked
  if (order == REC_SLOTS_WAVE)
    hipLaunchKernelGGL(slot_sum_wave_kernel, dim3((n + 3) / 4), dim3(256), 0, st, n, nslot, slots, dst);
  else
    hipLaunchKernelGGL(slot_sum_serial_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, nslot, slots, dst);
  REC_LAUNCH_CHECK();
  return REC_OK;
}
