// robust.hip — the per-surface sums of a robust point loss on the device
// (include/flashsdf.h "robust point losses"; the loss itself: robust_impl.h).
// Per surface k over the resident points with k*(p) = k, with w = w(d*),
// v = (∇d*, p × ∇d*): the IRLS moments Σ w v vᵀ (21 entries), the wrench
// Σ 2 w d* v (6), Σ ρ(d*) and Σ w — one row of kRobustLen = 29 doubles
// (MOMENTS = false: the last 8 alone, for callers that need no Hessian). From
// the per-point k*, d* and ∇d* a pass wrote in resident order: a launch of its
// own after the pass (the pass kernels are not touched), then the pass's tile
// reduce over the workgroups' partials.
//
// The design is moments_kernel's (moments.hip): every workgroup owns a fixed,
// contiguous run of 64-point chunks (robust_run: a function of n alone), each of
// its waves a contiguous share of the run and an [S][len] fp64 table of its own
// in LDS — as many waves (4, 2 or 1) as have room for their [S][29] tables
// (robust_waves: a function of S alone, the same for both variants, so their
// common entries are summed in the same order: the same bits). Lanes carry
// their sums from chunk to chunk while their k* stays the same; when a lane's
// k* changes (and at the end) a ballot loop over the wave's distinct k* sums
// each entry with a masked DPP wave sum, entry e ending in lane e, and lanes
// 0..len-1 add them to row k of the wave's table (consecutive doubles: no bank
// conflict). The waves' tables are summed in wave order into the workgroup's
// partial. No floating-point atomics: the summation order is a function of
// (n, S, the resident order, k*) alone, so results are bit-identical from run
// to run.
//
// WEIGHTED (fsdf_set_point_weights): a confidence a_i >= 0 per resident point,
// conf[i] in resident order (fp64 also in fp32 contexts). One product
// aw = a · w stands wherever w does (the moments, wrench_scale(aw, d), Σw), and
// a · ρ in the cost. A point of weight 0 stays in the sums as zero terms: the
// summation order is the unweighted kernel's, a function of the layout alone.
//
// ONE_SIDED (fsdf_set_free_split): caller points [n_surface, n) are free-space
// samples, penalised only where the model covers them (d* < 0). Resident point
// i is one iff (perm ? perm[i] : i) >= n_surface — the cloud's resident→caller
// permutation, read here (4 B per point): nothing is gathered, nothing goes
// stale across a regroup. The gate (robust_impl.h one_sided_factor) replaces a
// by 0.0 for a sample outside the model and the WEIGHTED arithmetic follows, so
// the bits are those of the weighted kernel given weights a · gate; table, run
// and wave layout are unchanged.
//
// skip (the device solver loops, fsdf_set_robust_loops): a device flag a frame's
// step kernel raises when the frame is done; robust_kernel, the tile reduce and
// robust_assemble_kernel — the rows into the accumulator [1 + 6S] and the
// moments [S][21] the step kernels read, robust_rows_finish's arithmetic on the
// device — then return at once. skip == nullptr is the launch without it.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "fsdf_internal.h"
#include "robust_impl.h"
#include "sdf_device_math.h"

namespace fsdf {

static_assert(kRobustMinChunks % (kRobustBlock / 64) == 0, "a run is whole rounds of one chunk per wave");
static_assert(kRobustLen == kMomentsLen + kRobustTail, "a row: the moments, then the wrench, the cost and the weight");

int64_t robust_run(int64_t n) {
  const int64_t nc = (n + 63) / 64, waves = kRobustBlock / 64;
  const int64_t run = std::max<int64_t>(kRobustMinChunks, (nc + kRobustMaxGroups - 1) / kRobustMaxGroups);
  return (run + waves - 1) / waves * waves;
}

int robust_groups(int64_t n) {
  const int64_t nc = (n + 63) / 64, run = robust_run(n);
  return (int)((nc + run - 1) / run);
}

int robust_waves(int S) {
  const size_t table = (size_t)std::max(S, 1) * kRobustLen * sizeof(double);
  for (int w = kRobustBlock / 64; w >= 1; w /= 2)
    if (w * table <= (size_t)kRobustMaxLds) return w;
  return 0;
}

bool robust_fit(int S) { return S >= 1 && robust_waves(S) >= 1; }

size_t robust_partials_len(int64_t n, int S) {
  // (whole 8-entry line tiles: reduce_tiles_kernel's layout)
  return (size_t)((kRobustLen * S + 7) & ~7) * (size_t)std::max(robust_groups(n), 1);
}

extern __shared__ __attribute__((aligned(16))) double robust_tab[];  // [waves][S][LEN]

// blockDim.x / 64 waves; run is a multiple of them (the statements: robust_body.inc, shared with batch.hip)
template <typename T, bool MOMENTS, bool WEIGHTED, bool ONE_SIDED>
__global__ __launch_bounds__(kRobustBlock) void robust_kernel(const T* __restrict__ pts,
                                                              const int32_t* __restrict__ kstar,
                                                              const double* __restrict__ dstar,
                                                              const double* __restrict__ grad, int64_t n, int S,
                                                              int run, int kind, double scale,
                                                              double* __restrict__ partials,
                                                              const double* __restrict__ conf,
                                                              const int32_t* __restrict__ perm, int64_t n_surface,
                                                              const int* __restrict__ skip) {
  // (uniform: a finished device frame — one address for every thread of the launch, written only by
  // a step kernel of an earlier launch on the same stream, so every wave of every workgroup reads
  // the same value and leaves, or stays, as a whole: no barrier below is reached by a part of one)
  if (skip && *skip) return;
#include "robust_body.inc"
}

hipError_t launch_robust(int precision, bool moments, const void* d_pts, const int32_t* d_kstar, const double* d_d,
                         const double* d_grad, const double* d_conf, const int32_t* d_perm, int64_t n_surface,
                         int64_t n, int S, int kind, double scale, double* d_partials, double* d_rows,
                         hipStream_t s, const int* skip) {
  if (n <= 0 || !robust_fit(S) || !robust::valid(kind, scale) || !d_pts || !d_kstar || !d_d || !d_grad ||
      !d_partials || !d_rows)
    return hipErrorInvalidValue;
  const int groups = robust_groups(n), run = (int)robust_run(n), waves = robust_waves(S), block = 64 * waves;
  const int len = moments ? kRobustLen : kRobustTail;
  const size_t lds = (size_t)waves * S * len * sizeof(double);
#define FSDF_ROBUST_LAUNCH(T, M, W, O)                                                                         \
  hipLaunchKernelGGL((robust_kernel<T, M, W, O>), dim3(groups), dim3(block), lds, s, (const T*)d_pts, d_kstar, \
                     d_d, d_grad, n, S, run, kind, scale, d_partials, d_conf, d_perm, n_surface, skip)
#define FSDF_ROBUST_LAUNCH_M(T, W, O)              \
  do {                                             \
    if (moments) FSDF_ROBUST_LAUNCH(T, true, W, O); \
    else FSDF_ROBUST_LAUNCH(T, false, W, O);        \
  } while (0)
#define FSDF_ROBUST_LAUNCH_W(T, O)                 \
  do {                                             \
    if (d_conf) FSDF_ROBUST_LAUNCH_M(T, true, O);  \
    else FSDF_ROBUST_LAUNCH_M(T, false, O);        \
  } while (0)
  // (d_conf null: the unweighted instantiations, which never read it; n_surface < 0: no split — the
  // instantiations that read neither the permutation nor d* for a gate)
  if (precision == 64) {
    if (n_surface >= 0) FSDF_ROBUST_LAUNCH_W(double, true);
    else FSDF_ROBUST_LAUNCH_W(double, false);
  } else {
    if (n_surface >= 0) FSDF_ROBUST_LAUNCH_W(float, true);
    else FSDF_ROBUST_LAUNCH_W(float, false);
  }
#undef FSDF_ROBUST_LAUNCH_W
#undef FSDF_ROBUST_LAUNCH_M
#undef FSDF_ROBUST_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the partials in workgroup order (the pass's tile reduce: fixed order)
  return launch_reduce(d_partials, groups, len * S, d_rows, s, nullptr, nullptr, nullptr, skip);
}

// The accumulator in fsdf_eval's layout and — MOMENTS — the [S][21] moments from
// the reduced rows, on the device: robust_rows_finish's (pass.hip) arithmetic.
// One thread per entry copied — surface k's 6 wrench entries to accum[1 + 6k ..],
// its 21 moments to moments[21k ..]; a surface that is no hull gets 0.0 in their
// place — over as many workgroups as the S · (6 [+ 21]) entries need, so any S
// is served. accum[0] = Σρ is summed by thread 0 of workgroup 0 alone, serially
// over the surfaces in ascending order from 0.0: the host's order is what the
// bits are (at most 256 additions: the library's surface limit; tiles of
// kRobustAssembleBlock serve any S).
template <bool MOMENTS>
__global__ __launch_bounds__(kRobustAssembleBlock) void robust_assemble_kernel(const double* __restrict__ rows,
                                                                               const int32_t* __restrict__ surface_kind,
                                                                               int S, double* __restrict__ accum,
                                                                               double* __restrict__ moments,
                                                                               const int* __restrict__ skip) {
  // (uniform: a finished device frame; the flag is written only by a step kernel of an earlier
  // launch on the same stream, as robust_kernel's)
  if (skip && *skip) return;
  constexpr int LEN = MOMENTS ? kRobustLen : kRobustTail;
  constexpr int M0 = LEN - kRobustTail;  // the wrench's first entry; Σρ at M0 + 6
  constexpr int PER = 6 + (MOMENTS ? kMomentsLen : 0);  // entries copied per surface
  const int t = blockIdx.x * kRobustAssembleBlock + threadIdx.x;
  if (t < S * PER) {
    const int k = t / PER, e = t - k * PER;
    const bool hull = surface_kind[k] == 0;  // (FSDF_SURFACE_HULL)
    const double* r = rows + (size_t)LEN * k;
    if (e < 6)
      accum[1 + 6 * k + e] = hull ? r[M0 + e] : 0.0;
    else if (MOMENTS)
      moments[kMomentsLen * k + (e - 6)] = hull ? r[e - 6] : 0.0;
  }
  // Σρ, workgroup 0 (block-uniform: its barriers are reached by the whole workgroup): the
  // surfaces' Σρ come into LDS a tile of one per thread at a time — the loads side by side, not
  // one round trip to memory per surface (13 µs at S = 64 that way) — and thread 0 adds each
  // tile serially: ascending k from 0.0, the host's order
  if (blockIdx.x == 0) {
    __shared__ double rho[kRobustAssembleBlock];
    double cost = 0.0;
    for (int base = 0; base < S; base += kRobustAssembleBlock) {
      const int k = base + (int)threadIdx.x;
      if (k < S) rho[threadIdx.x] = rows[(size_t)LEN * k + M0 + 6];
      __syncthreads();
      if (threadIdx.x == 0) {
        const int m = S - base < kRobustAssembleBlock ? S - base : kRobustAssembleBlock;
        for (int j = 0; j < m; ++j) cost += rho[j];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) accum[0] = cost;
  }
}

hipError_t launch_robust_assemble(bool moments, const double* d_rows, const int32_t* d_surface_kind, int S,
                                  double* d_accum, double* d_moments, hipStream_t s, const int* skip) {
  if (S < 1 || !d_rows || !d_surface_kind || !d_accum || (moments && !d_moments)) return hipErrorInvalidValue;
  const int per = 6 + (moments ? kMomentsLen : 0);
  const int groups = (S * per + kRobustAssembleBlock - 1) / kRobustAssembleBlock;
  if (moments)
    hipLaunchKernelGGL(robust_assemble_kernel<true>, dim3(groups), dim3(kRobustAssembleBlock), 0, s, d_rows,
                       d_surface_kind, S, d_accum, d_moments, skip);
  else
    hipLaunchKernelGGL(robust_assemble_kernel<false>, dim3(groups), dim3(kRobustAssembleBlock), 0, s, d_rows,
                       d_surface_kind, S, d_accum, d_moments, skip);
  return hipGetLastError();
}

}  // namespace fsdf
