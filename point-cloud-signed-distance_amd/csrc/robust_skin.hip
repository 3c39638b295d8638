// robust_skin.hip — the RBF skins' blocks of the accumulator under a robust
// objective (include/flashsdf.h "robust objectives on skins"; the loss:
// robust_impl.h). The pass's block of skin r is Σ 2 s j(p) over the points with
// k*(p) = r's surface, j the point's row of ∂s/∂(w, a, b, c) (rbf_sdf.h
// rbf_adjoint). Under Σ a ρ(d*) the factor 2s of a point becomes
//   t = 2 (aw d*),  aw = a · w(d*),  w = ρ′ / 2d
// — robust::wrench_scale, formed in fp64 from the pass's d* exactly as
// robust_kernel forms it (the weights, the one-sided gate included), then
// rounded to the context's T, where it takes the place of two_s in
// rbf_adjoint's arithmetic (rbf_adjoint<T, true>). The pass's d* of a skin lane
// IS the s rbf_skin_from_field gives for the same rows (scene_eval.h: `best`
// is that s, widened), so with a ≡ 1 under SQUARE a lane's summands are the
// pass's, bit for bit: only the order of summation differs.
//
// A launch of its own after the pass (the pass kernels are not touched), in
// robust_kernel's shape: workgroup g owns the chunks [g · run, (g + 1) · run),
// run = robust_run(n); each of its four waves a contiguous share of the run,
// a table of rbf_acc (<= kMaxRbfAccum) doubles of its own in LDS and a staging
// area for the centre rows. A chunk with no skin lane is skipped by a ballot,
// a skin none of the chunk's lanes is nearest to likewise. Per centre the
// wave's lanes are summed by wave_sum and lane 0 adds to the table (as the
// pass does); the waves' tables are summed in wave order into the workgroup's
// partial in the line-tile layout, and launch_reduce sums the partials in
// workgroup order. No floating-point atomics: the launch geometry is a
// function of n and the model alone, the summation order of (n, the resident
// order, k*) — the same bits from run to run.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "fsdf_internal.h"
#include "rbf_sdf.h"
#include "robust_impl.h"

namespace fsdf {

constexpr int kRobustSkinStage = 64;  // centre rows staged per wave at a time (rbf_field's cap)

size_t robust_skin_partials_len(int64_t n, int rbf_acc) {
  // (whole 8-entry line tiles: reduce_tiles_kernel's layout)
  return (size_t)((std::max(rbf_acc, 1) + 7) & ~7) * (size_t)std::max(robust_groups(n), 1);
}

extern __shared__ __attribute__((aligned(32))) double robust_skin_lds[];  // [waves][acc_len] | T [waves][stage][4]

// kRobustBlock threads; run is a multiple of its four waves
template <typename T, bool WEIGHTED, bool ONE_SIDED>
__global__ __launch_bounds__(kRobustBlock) void robust_skin_kernel(
    const T* __restrict__ pts, const int32_t* __restrict__ kstar, const double* __restrict__ dstar,
    const T* __restrict__ rows, const int32_t* __restrict__ surface_kind, const int32_t* __restrict__ rbf_surface,
    const int32_t* __restrict__ rbf_row_off, const int32_t* __restrict__ rbf_acc_off, int S, int R, int acc_len,
    int64_t n, int run, int kind, double scale, double* __restrict__ partials, const double* __restrict__ conf,
    const int32_t* __restrict__ perm, int64_t n_surface) {
  constexpr bool FACTOR = WEIGHTED || ONE_SIDED;  // a point's terms carry a factor a
  constexpr int waves = kRobustBlock / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int t = tid; t < waves * acc_len; t += kRobustBlock) robust_skin_lds[t] = 0.0;
  __syncthreads();
  double* tab = robust_skin_lds + wave * acc_len;  // this wave's own
  T* stage = (T*)(robust_skin_lds + waves * acc_len) + wave * 4 * kRobustSkinStage;
  const int share = run / waves;
  const int64_t c0 = (int64_t)blockIdx.x * run + (int64_t)wave * share;
  for (int r = 0; r < share; ++r) {
    // a lane beyond n, or whose k* is no skin of the scene, contributes nothing
    const int64_t i = (c0 + r) * 64 + lane;
    int k = -1;
    if (i < n) {
      k = kstar[i];
      if (k < 0 || k >= S || surface_kind[k] == 0) k = -1;
    }
    if (__ballot(k >= 0) == 0) continue;  // (wave-uniform: no skin lane in this chunk)
    T px = (T)0, py = (T)0, pz = (T)0;
    double t64 = 0.0;
    if (k >= 0) {
      px = pts[3 * i];
      py = pts[3 * i + 1];
      pz = pts[3 * i + 2];
      const double d = dstar[i];
      double a = WEIGHTED ? conf[i] : 1.0;
      if (ONE_SIDED) a = robust::one_sided_factor(robust::free_sample(perm ? (int64_t)perm[i] : i, n_surface), d, a);
      const double w = FACTOR ? a * robust::weight(kind, scale, d) : robust::weight(kind, scale, d);  // aw
      t64 = robust::wrench_scale(w, d);
    }
    const T t = (T)t64;
    for (int rr = 0; rr < R; ++rr) {
      const bool sel = k == rbf_surface[rr];
      if (__ballot(sel) == 0) continue;  // (wave-uniform: the sums below run with the whole wave active)
      const int r0 = rbf_row_off[rr];
      rbf_adjoint<T, true>(px, py, pz, rows + 4 * r0, rbf_row_off[rr + 1] - r0 - 1, stage, kRobustSkinStage, sel,
                           tab + rbf_acc_off[rr], t);
    }
  }
  __syncthreads();
  // the waves' tables in wave order: this workgroup's partial, in the line tiles
  // reduce_tiles_kernel reads (pass_kernels.h pidx: entry t of block b at [t / 8][b][t % 8])
  for (int t = tid; t < acc_len; t += kRobustBlock) {
    double s = robust_skin_lds[t];
    for (int w = 1; w < waves; ++w) s += robust_skin_lds[w * acc_len + t];
    partials[((int64_t)(t >> 3) * gridDim.x + blockIdx.x) * 8 + (t & 7)] = s;
  }
}

hipError_t launch_robust_skin(int precision, const void* d_pts, const int32_t* d_kstar, const double* d_d,
                              const void* d_rows, const LocalModel& lm, const double* d_conf, const int32_t* d_perm,
                              int64_t n_surface, int64_t n, int kind, double scale, double* d_partials,
                              double* d_blocks, hipStream_t s) {
  if (n <= 0 || lm.R < 1 || lm.rbf_acc < 1 || lm.rbf_acc > kMaxRbfAccum || !robust::valid(kind, scale) || !d_pts ||
      !d_kstar || !d_d || !d_rows || !d_partials || !d_blocks || !lm.surface_kind || !lm.rbf_surface ||
      !lm.rbf_row_off || !lm.rbf_acc_off)
    return hipErrorInvalidValue;
  const int groups = robust_groups(n), run = (int)robust_run(n), waves = kRobustBlock / 64;
  const size_t elt = precision == 64 ? sizeof(double) : sizeof(float);
  const size_t lds = (size_t)waves * lm.rbf_acc * sizeof(double) + (size_t)waves * 4 * kRobustSkinStage * elt;
#define FSDF_RSKIN_LAUNCH(T, W, O)                                                                              \
  hipLaunchKernelGGL((robust_skin_kernel<T, W, O>), dim3(groups), dim3(kRobustBlock), lds, s, (const T*)d_pts,  \
                     d_kstar, d_d, (const T*)d_rows, lm.surface_kind, lm.rbf_surface, lm.rbf_row_off,           \
                     lm.rbf_acc_off, lm.S, lm.R, lm.rbf_acc, n, run, kind, scale, d_partials, d_conf, d_perm,   \
                     n_surface)
#define FSDF_RSKIN_LAUNCH_W(T, O)             \
  do {                                        \
    if (d_conf) FSDF_RSKIN_LAUNCH(T, true, O); \
    else FSDF_RSKIN_LAUNCH(T, false, O);       \
  } while (0)
  // (d_conf null: the unweighted instantiations, which never read it; n_surface < 0: no split — the
  // instantiations that read neither the permutation nor d* for a gate)
  if (precision == 64) {
    if (n_surface >= 0) FSDF_RSKIN_LAUNCH_W(double, true);
    else FSDF_RSKIN_LAUNCH_W(double, false);
  } else {
    if (n_surface >= 0) FSDF_RSKIN_LAUNCH_W(float, true);
    else FSDF_RSKIN_LAUNCH_W(float, false);
  }
#undef FSDF_RSKIN_LAUNCH_W
#undef FSDF_RSKIN_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the partials in workgroup order (the pass's tile reduce: fixed order)
  return launch_reduce(d_partials, groups, lm.rbf_acc, d_blocks, s);
}

}  // namespace fsdf
