// moments.hip — the per-surface second moments of the residual on the device
// (include/flashsdf.h "second-order solver"): M_k = Σ_{p: k*(p)=k} w_p w_pᵀ,
// w_p = (∇d*, p × ∇d*), from the per-point k* and ∇d* a pass wrote in resident
// order. A launch of its own after the pass (the pass kernels are not
// touched), then the pass's tile reduce over the workgroups' partials.
//
// Every workgroup owns a fixed, contiguous run of 64-point chunks (moments_run:
// a function of n alone), each of its waves a contiguous share of the run and
// an [S][21] fp64 table of its own in LDS — as many waves (4, 2 or 1) as have
// room for their tables (moments_waves: a function of S alone). Per chunk each
// lane forms w and adds its 21 products to sums it carries while its k* stays
// the same; when a lane's k* changes (and at the end) the wave sums across
// lanes: per distinct k* of the wave (a ballot loop) a masked DPP wave sum of
// each entry, entry e ending in lane e, and lanes 0..20 add them to row k of
// the wave's table. No wave waits for another until the end, where the waves' tables are summed in wave order into
// the workgroup's partial. No floating-point atomics: the summation order is a
// function of (n, S, the resident order, k*) alone, so results are
// bit-identical from run to run.
// (sdf_device_math.h is shared with sdf_kernels.hip for wave_sum only.)

#include <hip/hip_runtime.h>

#include <algorithm>

#include "fsdf_internal.h"
#include "sdf_device_math.h"

namespace fsdf {

static_assert(kMomentsMinChunks % (kMomentsBlock / 64) == 0, "a run is whole rounds of one chunk per wave");

int64_t moments_run(int64_t n) {
  const int64_t nc = (n + 63) / 64, waves = kMomentsBlock / 64;
  const int64_t run = std::max<int64_t>(kMomentsMinChunks, (nc + kMomentsMaxGroups - 1) / kMomentsMaxGroups);
  return (run + waves - 1) / waves * waves;
}

int moments_groups(int64_t n) {
  const int64_t nc = (n + 63) / 64, run = moments_run(n);
  return (int)((nc + run - 1) / run);
}

int moments_waves(int S) {
  const size_t table = (size_t)std::max(S, 1) * kMomentsLen * sizeof(double);
  for (int w = kMomentsBlock / 64; w >= 1; w /= 2)
    if (w * table <= (size_t)kMomentsMaxLds) return w;
  return 0;
}

bool moments_fit(int S) { return S >= 1 && moments_waves(S) >= 1; }

size_t moments_partials_len(int64_t n, int S) {
  // (whole 8-entry line tiles: reduce_tiles_kernel's layout)
  return (size_t)((kMomentsLen * S + 7) & ~7) * (size_t)std::max(moments_groups(n), 1);
}

extern __shared__ __attribute__((aligned(16))) double moments_tab[];  // [waves][S][21]

// blockDim.x / 64 waves; run is a multiple of them
template <typename T>
__global__ __launch_bounds__(kMomentsBlock) void moments_kernel(const T* __restrict__ pts,
                                                                const int32_t* __restrict__ kstar,
                                                                const double* __restrict__ grad, int64_t n, int S,
                                                                int run, double* __restrict__ partials,
                                                                const int* __restrict__ skip) {
  if (skip && *skip) return;  // (uniform: a finished device LM frame)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const int len = kMomentsLen * S;
  for (int t = tid; t < waves * len; t += blockDim.x) moments_tab[t] = 0.0;
  __syncthreads();
  double* tab = moments_tab + wave * len;  // this wave's own
  const int share = run / waves;
  const int64_t c0 = (int64_t)blockIdx.x * run + (int64_t)wave * share;
  // Each lane carries the sums of its own points from chunk to chunk while its
  // k* stays the same (ck: the surface they belong to, -1: none yet); the wave
  // sums across lanes only when a lane's k* changes, and at the end of its
  // share. In a regrouped cloud that is once per surface instead of once per
  // chunk.
  int ck = -1;
  double acc[kMomentsLen];
#pragma unroll
  for (int e = 0; e < kMomentsLen; ++e) acc[e] = 0.0;
  // the carried sums into the table: per distinct surface of the wave (that of
  // its first lane still to be summed) a masked wave sum of each entry, entry e
  // ending in lane e (rem is wave-uniform: the sums run with the whole wave active)
  auto flush = [&]() {
    unsigned long long rem = __ballot(ck >= 0);
    while (rem != 0) {
      const int kk = __builtin_amdgcn_readlane(ck, __ffsll((long long)rem) - 1);
      const bool in = ck == kk;
      rem &= ~__ballot(in);
      double mine = 0.0;
#pragma unroll
      for (int e = 0; e < kMomentsLen; ++e) {
        const double s = wave_sum(in ? acc[e] : 0.0);
        mine = lane == e ? s : mine;
      }
      if (lane < kMomentsLen) tab[kMomentsLen * kk + lane] += mine;
    }
    ck = -1;
#pragma unroll
    for (int e = 0; e < kMomentsLen; ++e) acc[e] = 0.0;
  };
  for (int r = 0; r < share; ++r) {
    // a lane beyond n, or whose k* is not a surface of the scene, contributes nothing
    const int64_t i = (c0 + r) * 64 + lane;
    int k = -1;
    if (i < n) {
      k = kstar[i];
      if (k < 0 || k >= S) k = -1;
    }
    if (__ballot(k >= 0 && ck >= 0 && k != ck) != 0) flush();
    if (k >= 0) {
      const double px = (double)pts[3 * i], py = (double)pts[3 * i + 1], pz = (double)pts[3 * i + 2];
      double w[6];
      w[0] = grad[3 * i];
      w[1] = grad[3 * i + 1];
      w[2] = grad[3 * i + 2];
      w[3] = py * w[2] - pz * w[1];
      w[4] = pz * w[0] - px * w[2];
      w[5] = px * w[1] - py * w[0];
      int e = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b, ++e) acc[e] += w[a] * w[b];
      ck = k;
    }
  }
  flush();
  __syncthreads();
  // the waves' tables in wave order: this workgroup's partial, in the line tiles
  // reduce_tiles_kernel reads (pass_kernels.h pidx: entry t of block b at [t / 8][b][t % 8])
  for (int t = tid; t < len; t += blockDim.x) {
    double s = moments_tab[t];
    for (int w = 1; w < waves; ++w) s += moments_tab[w * len + t];
    partials[((int64_t)(t >> 3) * gridDim.x + blockIdx.x) * 8 + (t & 7)] = s;
  }
}

hipError_t launch_moments(int precision, const void* d_pts, const int32_t* d_kstar, const double* d_grad, int64_t n,
                          int S, double* d_partials, double* d_moments, hipStream_t s, const int* skip) {
  if (n <= 0 || !moments_fit(S) || !d_pts || !d_kstar || !d_grad || !d_partials || !d_moments)
    return hipErrorInvalidValue;
  const int groups = moments_groups(n), run = (int)moments_run(n), block = 64 * moments_waves(S);
  const size_t lds = (size_t)moments_waves(S) * S * kMomentsLen * sizeof(double);
  if (precision == 64)
    hipLaunchKernelGGL(moments_kernel<double>, dim3(groups), dim3(block), lds, s, (const double*)d_pts,
                       d_kstar, d_grad, n, S, run, d_partials, skip);
  else
    hipLaunchKernelGGL(moments_kernel<float>, dim3(groups), dim3(block), lds, s, (const float*)d_pts, d_kstar,
                       d_grad, n, S, run, d_partials, skip);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the partials in workgroup order (the pass's tile reduce: fixed order)
  return launch_reduce(d_partials, groups, kMomentsLen * S, d_moments, s, nullptr, nullptr, nullptr, skip);
}

}  // namespace fsdf
