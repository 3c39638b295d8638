// wave_times.h — the hooks of the per-wave timeline build that the kernels
// call, and the gate of the event counters (fsdf_kernel_stats). Only
// sdf_kernels.hip includes it (through its other headers).
#pragma once
#include "fsdf_internal.h"

namespace fsdf {
// The timeline build (-DFSDF_WAVE_TIMES=1, tools/wave_times.py): a
// per-wave timeline with per-phase 100 MHz clocks and event counts; every hook
// below compiles to nothing in the product library.
#if FSDF_WAVE_TIMES
// per wave-iteration, packed 16-bit fields:
//   ev[0]: hull evaluations | screen rejections << 16 | slow evaluations << 32 | walk steps << 48
//   ev[1]: seed evaluations | needing lanes << 16 | wave candidates << 32 | full fp64 scans << 48
//   ph[0]: 10-ns units in hull staging | screen | fast path | closest-feature search
//   ph[1]: culling | RBF | segmented reduction + stores | descent walk (within the search)
//   ev[2]: lane-evaluations through the closest-feature search | those whose
//          hull won the lane | lanes spared the search by the h_max bound |
//          10-ns units in the candidate need tests of phase C
constexpr int kWtWaves = kPassBlock / 64;
__shared__ unsigned long long fsdf_wave_ev[kWtWaves][3];
__shared__ bool fsdf_wt_slow[64 * kWtWaves];  // per lane: the last hull_sdf ran its search
__shared__ unsigned long long fsdf_wave_ph[kWtWaves][2];
//   ph2[0]: 10-ns units in walk certificates | walk closest points | vertex-
//           region lane-certificates | fan iterations (max over lanes, per step)
//   ph2[1]: 10-ns units in the screen loop | screen fix-up | edge-region
//           lane-certificates | interior-region lane-certificates
__shared__ unsigned long long fsdf_wave_ph2[kWtWaves][2];
#endif
__device__ __forceinline__ uint64_t wt_now() {
#if FSDF_WAVE_TIMES
  return __builtin_amdgcn_s_memrealtime();
#else
  return 0;
#endif
}
// adds the time since t0 to phase field f (0..7); returns now
__device__ __forceinline__ uint64_t wt_add(int f, uint64_t t0) {
#if FSDF_WAVE_TIMES
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  if ((threadIdx.x & 63) == 0) fsdf_wave_ph[threadIdx.x >> 6][f >> 2] += (t1 - t0) << (16 * (f & 3));
  return t1;
#else
  return t0;
#endif
}
// sub-phase clocks / counts (ph2 fields 0..7)
__device__ __forceinline__ uint64_t wt_add2(int f, uint64_t t0) {
#if FSDF_WAVE_TIMES
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  if ((threadIdx.x & 63) == 0) fsdf_wave_ph2[threadIdx.x >> 6][f >> 2] += (t1 - t0) << (16 * (f & 3));
  return t1;
#else
  return t0;
#endif
}
__device__ __forceinline__ void wt_count2(int f, uint64_t v) {
#if FSDF_WAVE_TIMES
  if ((threadIdx.x & 63) == 0) fsdf_wave_ph2[threadIdx.x >> 6][f >> 2] += v << (16 * (f & 3));
#endif
}
// adds v to event field f (0..7) of this wave-iteration
__device__ __forceinline__ void wt_count(int f, uint64_t v) {
#if FSDF_WAVE_TIMES
  if ((threadIdx.x & 63) == 0) fsdf_wave_ev[threadIdx.x >> 6][f >> 2] += v << (16 * (f & 3));
#endif
}
// the event counters (fsdf_kernel_stats) are off in the timeline build: their
// contended atomics would dominate the timed windows
__device__ __forceinline__ bool count_events(const unsigned long long* stats) {
  return !FSDF_WAVE_TIMES && stats != nullptr;
}

}  // namespace fsdf
