// skin_moments.hip — the second moments of the residual of RBF skins on the
// device (include/flashsdf.h "Gauss-Newton for RBF skins"): per skin r of n
// centres, m = 4n + 4,
//   M_r = Σ_{p: k*(p) = r} j(p) j(p)ᵀ,   j = (∂s/∂w [n], ∂s/∂a, ∂s/∂b [3], ∂s/∂c [n][3])
// — rbf_adjoint's summands (rbf_sdf.h) without the factor 2s, so the pass's
// accumulator block is Σ 2 s j. A launch of its own after the pass (the pass
// kernels are not touched), reading the resident points, the pass's k* in
// resident order and the context's current RBF rows; fp64 throughout (an fp32
// context's points and rows are widened).
//
// A symmetric rank-N update in fp64: the fp64 matrix unit's work. A unit is
// one 64x64 block pair (bi <= bj) of one skin's matrix; workgroup (unit, g)
// owns the chunks [g · run, (g + 1) · run) of the cloud (fsdf_internal.h
// skin_moments_run). Per round of four 64-point chunks every wave evaluates
// the field of one chunk's points as rbf_field / rbf_skin_from_field do (lane =
// point; a chunk with no point of the skin is skipped by a ballot) and leaves
// (p, 1/|∇f|, ∂s/∂∇f) in LDS; then per half chunk the workgroup forms the 32
// rows' columns of its two blocks in LDS (rows of points with k* != r or beyond
// N are zero, as are columns beyond m; inside the kernel the columns are ordered
// (w_i, c_i) per centre, then (a, b), so a centre's terms are formed once for its
// four columns — the finish launch writes the block order) and every wave adds Jᵀ J of its 16x64
// strip with v_mfma_f64_16x16x4_f64: lane l supplies J[4t + (l>>4)][16 w + (l&15)]
// as A and J[4t + (l>>4)][16 tj + (l&15)] as B; the result lies col = l & 15,
// row = (l>>4) + 4·reg (the f64 map, not the f32 one).
// No floating-point atomics: a workgroup writes its block as one partial, the
// finish launch sums a unit's partials in workgroup order, takes the upper
// triangle of the diagonal blocks and mirrors every block — for a given cloud
// layout M_r is bit-identical from run to run, and exactly symmetric.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "fsdf_internal.h"
#include "rbf_sdf.h"
#include "robust_impl.h"

namespace fsdf {

static_assert(kSkinMinChunks % (kSkinBlock / 64) == 0, "a run is whole rounds of one chunk per wave");
static_assert(kSkinMaxCentres + 4 <= 128 && 4 * kSkinMaxCentres + 4 <= kMaxRbfAccum, "the largest skin served");

constexpr int kSkinLd = kSkinTile + 4;   // row stride of a block's columns in LDS (doubles)
constexpr int kSkinPartial = kSkinTile * kSkinTile;

bool skin_moments_plan(int S, const int32_t* kind, const int32_t* n_centers, SkinPlan* out) {
  SkinPlan P;
  int rows = 0;
  for (int k = 0; k < S; ++k) {
    if (kind[k] != 1) continue;  // FSDF_SURFACE_RBF
    const int n = n_centers[k];
    if (n < 1 || n > kSkinMaxCentres || P.R >= kSkinMaxUnits) return false;
    const int m = 4 * n + 4, nbk = (m + kSkinTile - 1) / kSkinTile;
    if (P.U + nbk * (nbk + 1) / 2 > kSkinMaxUnits) return false;
    P.unit0[P.R] = P.U;
    P.U += nbk * (nbk + 1) / 2;
    P.n[P.R] = n;
    P.row_off[P.R] = rows;
    P.surf[P.R] = k;
    P.mom_off[P.R] = P.total;
    rows += n + 1;
    P.total += m * m;
    ++P.R;
  }
  if (P.R == 0) return false;
  *out = P;
  return true;
}

int64_t skin_moments_run(int64_t n, int U) {
  const int64_t nc = (n + 63) / 64, waves = kSkinBlock / 64;
  const int64_t cap = std::max<int64_t>(1, kSkinMaxPartials / std::max(U, 1));
  const int64_t run = std::max<int64_t>(kSkinMinChunks, (nc + cap - 1) / cap);
  return (run + waves - 1) / waves * waves;
}

int skin_moments_groups(int64_t n, int U) {
  const int64_t nc = (n + 63) / 64, run = skin_moments_run(n, U);
  return (int)std::max<int64_t>(1, (nc + run - 1) / run);
}

size_t skin_moments_partials_len(int64_t n, int U) {
  return (size_t)std::max(U, 1) * (size_t)skin_moments_groups(n, U) * kSkinPartial;
}

typedef double skin_v4d __attribute__((ext_vector_type(4)));

// a unit index within one skin -> its block pair (bi <= bj), nbk blocks a side
__device__ __forceinline__ void skin_unit_pair(int u, int nbk, int& bi, int& bj) {
  bi = 0;
  while (u >= nbk - bi) {
    u -= nbk - bi;
    ++bi;
  }
  bj = bi + u;
}

// FACTOR (skin_moments_factor_kernel): what a point's factor aw = a · w(d*) of a robust
// objective is formed from — the pass's d* in resident order, the loss, the weights in
// resident order (null: none), the resident→caller permutation (null: the caller's
// order) and n_surface (< 0: no split), as robust_kernel reads them
struct SkinFactor {
  const double* dstar = nullptr;
  const double* conf = nullptr;
  const int32_t* perm = nullptr;
  int64_t n_surface = -1;
  int kind = 0;
  double scale = 0.0;
};

// the body of both kernels. FACTOR = false: Σ j jᵀ. FACTOR: Σ aw j jᵀ — aw is formed in fp64
// where the point's field is, travels in the selection slot pd[7] of its staged record
// (aw = 0: the point contributes nothing, as a point of another surface) and scales the
// A operand of the rank update
template <typename T, bool MFMA, bool FACTOR>
__device__ __forceinline__ void skin_moments_body(const T* __restrict__ pts, const int32_t* __restrict__ kstar,
                                                  const T* __restrict__ rows_g, int64_t N, int n, int surf,
                                                  int groups, int run, double* __restrict__ partials,
                                                  const SkinFactor& fac) {
  __shared__ __attribute__((aligned(32))) double s_rows[4 * (kSkinMaxCentres + 1)];  // the skin's rows, widened
  __shared__ __attribute__((aligned(16))) double s_pd[4][64][8];  // per chunk and point: p, 1/|∇f|, ∂s/∂∇f, selected
  __shared__ __attribute__((aligned(32))) double s_J[2][32][kSkinLd];  // a half chunk's columns of blocks bi, bj
  __shared__ int s_any[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = (int)blockIdx.x / groups, g = (int)blockIdx.x % groups;
  const int m = 4 * n + 4;
  int bi, bj;
  skin_unit_pair(u, (m + kSkinTile - 1) / kSkinTile, bi, bj);
  for (int t = tid; t < 4 * (n + 1); t += kSkinBlock) s_rows[t] = (double)rows_g[t];
  __syncthreads();
  const int nblk = bi == bj ? 1 : 2;
  const double(*JA)[kSkinLd] = s_J[0];
  const double(*JB)[kSkinLd] = s_J[nblk - 1];
  skin_v4d acc[4];
  double facc[16];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = skin_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < 16; ++t) facc[t] = 0.0;
  const int64_t nc = (N + 63) / 64;
  const int64_t c_begin = (int64_t)g * run, c_end = c_begin + run < nc ? c_begin + run : nc;
  for (int64_t c0 = c_begin; c0 < c_end; c0 += 4) {
    {  // the field at this wave's chunk (lane = point)
      const int64_t c = c0 + wave, i = c * 64 + lane;
      bool sel = false;
      if (c < c_end && i < N) sel = kstar[i] == surf;
      const bool any = __ballot(sel) != 0;
      if (lane == 0) s_any[wave] = any;
      if (any) {
        double px = 0.0, py = 0.0, pz = 0.0;
        if (sel) {
          px = (double)pts[3 * i];
          py = (double)pts[3 * i + 1];
          pz = (double)pts[3 * i + 2];
        }
        typedef Row4<double>::type R4;
        const R4 poly = *(const R4*)(s_rows + 4 * n);
        RbfField<double> F;
        F.f = mfma_(poly[1], px, mfma_(poly[2], py, mfma_(poly[3], pz, poly[0])));
        F.gx = poly[1]; F.gy = poly[2]; F.gz = poly[3];
        F.hxx = F.hyy = F.hzz = F.hxy = F.hxz = F.hyz = 0.0;
        for (int k = 0; k < n; ++k) {  // (rbf_field's centre loop over the widened rows)
          const R4 cw = *(const R4*)(s_rows + 4 * k);
          const double dx = px - cw[0], dy = py - cw[1], dz = pz - cw[2];
          const double r2 = mfma_(dx, dx, mfma_(dy, dy, dz * dz));
          const double rho = tsqrt(r2);
          const double wr = cw[3] * rho;
          F.f = mfma_(wr, r2, F.f);
          const double t3 = 3.0 * wr;
          F.gx = mfma_(t3, dx, F.gx); F.gy = mfma_(t3, dy, F.gy); F.gz = mfma_(t3, dz, F.gz);
        }
        // (s = f/|∇f| needs no Hessian: ∂s/∂f = 1/|∇f|, ∂s/∂∇f = −f ∇f/|∇f|³)
        double s, sgx, sgy, sgz, cc, invG;
        rbf_skin_from_field(F, s, sgx, sgy, sgz, cc, invG);
        double* pd = s_pd[wave][lane];
        pd[0] = px; pd[1] = py; pd[2] = pz; pd[3] = invG;
        pd[4] = -cc * F.gx; pd[5] = -cc * F.gy; pd[6] = -cc * F.gz;
        double aw = sel ? 1.0 : 0.0;
        if (FACTOR && sel) {
          const double d = fac.dstar[i];
          double a = fac.conf ? fac.conf[i] : 1.0;
          if (fac.n_surface >= 0)
            a = robust::one_sided_factor(robust::free_sample(fac.perm ? (int64_t)fac.perm[i] : i, fac.n_surface), d, a);
          aw = a * robust::weight(fac.kind, fac.scale, d);
        }
        pd[7] = aw;
      }
    }
    __syncthreads();
    for (int ch = 0; ch < 4; ++ch) {
      if (!s_any[ch]) continue;  // (uniform over the workgroup)
      for (int h = 0; h < 2; ++h) {
        {  // 32 rows x 8 columns per thread group of 32: the half chunk's columns of the two blocks,
           // in the kernel's own column order — (w_i, c_i) per centre, then (a, b) — so a centre's
           // distance, e and k1 are formed once for its four columns
          const int p = tid & 31, cg = tid >> 5;
          const double* pd = s_pd[ch][32 * h + p];
          const double px = pd[0], py = pd[1], pz = pd[2], dsdf = pd[3], ux = pd[4], uy = pd[5], uz = pd[6];
          const bool sel = pd[7] != 0.0;
          typedef Row4<double>::type R4;
          for (int blk = 0; blk < nblk; ++blk) {
#pragma unroll
            for (int q4 = 0; q4 < 2; ++q4) {
              const int col = 8 * cg + 4 * q4, i = (kSkinTile * (blk ? bj : bi) + col) >> 2;
              R4 v = {0.0, 0.0, 0.0, 0.0};
              if (sel && i == n) {  // ∂s/∂a, ∂s/∂b
                v[0] = dsdf;
                v[1] = mfma_(dsdf, px, ux);
                v[2] = mfma_(dsdf, py, uy);
                v[3] = mfma_(dsdf, pz, uz);
              } else if (sel && i < n) {  // ∂s/∂w_i, ∂s/∂c_i (coefficients fixed): rbf_adjoint's terms
                const R4 cw = *(const R4*)(s_rows + 4 * i);
                const double dx = px - cw[0], dy = py - cw[1], dz = pz - cw[2];
                const double r2 = mfma_(dx, dx, mfma_(dy, dy, dz * dz));
                const double rho = tsqrt(r2);
                const double e = mfma_(dx, ux, mfma_(dy, uy, dz * uz));
                const double k1 = mfma_(3.0 * rho, dsdf, r2 > 0.0 ? (3.0 * e) / rho : 0.0);
                const double k2 = 3.0 * rho, sc = -cw[3];
                v[0] = mfma_(dsdf * r2, rho, 3.0 * rho * e);
                v[1] = sc * mfma_(k1, dx, k2 * ux);
                v[2] = sc * mfma_(k1, dy, k2 * uy);
                v[3] = sc * mfma_(k1, dz, k2 * uz);
              }
              *(R4*)&s_J[blk][p][col] = v;
            }
          }
        }
        __syncthreads();
        if (MFMA) {
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const int row = 4 * t + (lane >> 4);
            const double a = FACTOR ? JA[row][16 * wave + (lane & 15)] * s_pd[ch][32 * h + row][7]
                                    : JA[row][16 * wave + (lane & 15)];
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
              acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, JB[row][16 * tj + (lane & 15)], acc[tj], 0, 0, 0);
          }
        } else {  // (A/B: thread t owns row t >> 2 of the block, 16 columns)
          const int i = tid >> 2, j0 = 16 * (tid & 3);
          for (int p = 0; p < 32; ++p) {
            const double a = FACTOR ? JA[p][i] * s_pd[ch][32 * h + p][7] : JA[p][i];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) facc[jj] = mfma_(a, JB[p][j0 + jj], facc[jj]);
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();  // (a round whose chunks were all skipped: s_any is rewritten next)
  }
  double* out = partials + (int64_t)blockIdx.x * kSkinPartial;
  if (MFMA) {
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        out[(16 * wave + (lane >> 4) + 4 * reg) * kSkinTile + 16 * tj + (lane & 15)] = acc[tj][reg];
  } else {
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) out[(tid >> 2) * kSkinTile + 16 * (tid & 3) + jj] = facc[jj];
  }
}

template <typename T, bool MFMA>
__global__ __launch_bounds__(kSkinBlock) void skin_moments_kernel(const T* __restrict__ pts,
                                                                  const int32_t* __restrict__ kstar,
                                                                  const T* __restrict__ rows_g, int64_t N, int n,
                                                                  int surf, int groups, int run,
                                                                  double* __restrict__ partials,
                                                                  const int* __restrict__ skip) {
  if (skip && *skip) return;  // (uniform: a finished device LM frame)
  skin_moments_body<T, MFMA, false>(pts, kstar, rows_g, N, n, surf, groups, run, partials, SkinFactor());
}

template <typename T, bool MFMA>
__global__ __launch_bounds__(kSkinBlock) void skin_moments_factor_kernel(const T* __restrict__ pts,
                                                                         const int32_t* __restrict__ kstar,
                                                                         const T* __restrict__ rows_g, int64_t N,
                                                                         int n, int surf, int groups, int run,
                                                                         double* __restrict__ partials,
                                                                         SkinFactor fac) {
  skin_moments_body<T, MFMA, true>(pts, kstar, rows_g, N, n, surf, groups, run, partials, fac);
}

// the kernel's column q — (w_i, c_i) per centre i = q >> 2, then (a, b) — in the block's order
__device__ __forceinline__ int skin_block_column(int q, int n) {
  const int i = q >> 2, t = q & 3;
  return i < n ? (t == 0 ? i : n + 4 + 3 * i + t - 1) : n + t;
}

// a unit's partials in workgroup order, the block and its mirror image into M_r
__global__ __launch_bounds__(256) void skin_moments_finish_kernel(const double* __restrict__ partials, int n,
                                                                   int groups, double* __restrict__ M,
                                                                   const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int u = (int)blockIdx.x >> 4, e = (((int)blockIdx.x & 15) << 8) + (int)threadIdx.x;
  const int m = 4 * n + 4;
  int bi, bj;
  skin_unit_pair(u, (m + kSkinTile - 1) / kSkinTile, bi, bj);
  const int row = e >> 6, col = e & 63, gi = kSkinTile * bi + row, gj = kSkinTile * bj + col;
  if (gi >= m || gj >= m || (bi == bj && row > col)) return;
  const double* p = partials + (int64_t)u * groups * kSkinPartial + e;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += p[(int64_t)g * kSkinPartial];
  const int oi = skin_block_column(gi, n), oj = skin_block_column(gj, n);
  M[(int64_t)oi * m + oj] = s;
  M[(int64_t)oj * m + oi] = s;
}

// one pair of launches per skin: its units' workgroups, then the finish
static hipError_t launch_skin_moments_impl(int precision, const void* d_pts, const int32_t* d_kstar,
                                           const void* d_rows, int64_t n, const SkinPlan& plan, double* d_partials,
                                           double* d_moments, hipStream_t s, const int* skip,
                                           const SkinFactor* fac) {
  if (n <= 0 || plan.U < 1 || plan.U > kSkinMaxUnits || plan.R < 1 || !d_pts || !d_kstar || !d_rows || !d_partials ||
      !d_moments)
    return hipErrorInvalidValue;
  const int groups = skin_moments_groups(n, plan.U), run = (int)skin_moments_run(n, plan.U);
  constexpr bool kMfma = !FSDF_SKIN_MOMENTS_FMA;
  for (int r = 0; r < plan.R; ++r) {
    const int units = (r + 1 < plan.R ? plan.unit0[r + 1] : plan.U) - plan.unit0[r];
    double* part = d_partials + (size_t)plan.unit0[r] * groups * kSkinPartial;
    if (fac && precision == 64)
      hipLaunchKernelGGL((skin_moments_factor_kernel<double, kMfma>), dim3(units * groups), dim3(kSkinBlock), 0, s,
                         (const double*)d_pts, d_kstar, (const double*)d_rows + 4 * (size_t)plan.row_off[r], n,
                         plan.n[r], plan.surf[r], groups, run, part, *fac);
    else if (fac)
      hipLaunchKernelGGL((skin_moments_factor_kernel<float, kMfma>), dim3(units * groups), dim3(kSkinBlock), 0, s,
                         (const float*)d_pts, d_kstar, (const float*)d_rows + 4 * (size_t)plan.row_off[r], n,
                         plan.n[r], plan.surf[r], groups, run, part, *fac);
    else if (precision == 64)
      hipLaunchKernelGGL((skin_moments_kernel<double, kMfma>), dim3(units * groups), dim3(kSkinBlock), 0, s,
                         (const double*)d_pts, d_kstar, (const double*)d_rows + 4 * (size_t)plan.row_off[r], n,
                         plan.n[r], plan.surf[r], groups, run, part, skip);
    else
      hipLaunchKernelGGL((skin_moments_kernel<float, kMfma>), dim3(units * groups), dim3(kSkinBlock), 0, s,
                         (const float*)d_pts, d_kstar, (const float*)d_rows + 4 * (size_t)plan.row_off[r], n,
                         plan.n[r], plan.surf[r], groups, run, part, skip);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(skin_moments_finish_kernel, dim3(units * 16), dim3(256), 0, s, part, plan.n[r], groups,
                       d_moments + plan.mom_off[r], skip);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_skin_moments(int precision, const void* d_pts, const int32_t* d_kstar, const void* d_rows, int64_t n,
                               const SkinPlan& plan, double* d_partials, double* d_moments, hipStream_t s,
                               const int* skip) {
  return launch_skin_moments_impl(precision, d_pts, d_kstar, d_rows, n, plan, d_partials, d_moments, s, skip, nullptr);
}

// Σ aw j jᵀ: the factor of resident point i from d_d[i] (the pass's d* in resident order), the
// loss, d_conf (null: no weights), d_perm and n_surface (< 0: no split), as launch_robust's
hipError_t launch_skin_moments_weighted(int precision, const void* d_pts, const int32_t* d_kstar, const double* d_d,
                                        const void* d_rows, const double* d_conf, const int32_t* d_perm,
                                        int64_t n_surface, int kind, double scale, int64_t n, const SkinPlan& plan,
                                        double* d_partials, double* d_moments, hipStream_t s) {
  if (!d_d || !robust::valid(kind, scale)) return hipErrorInvalidValue;
  SkinFactor fac;
  fac.dstar = d_d;
  fac.conf = d_conf;
  fac.perm = d_perm;
  fac.n_surface = n_surface;
  fac.kind = kind;
  fac.scale = scale;
  return launch_skin_moments_impl(precision, d_pts, d_kstar, d_rows, n, plan, d_partials, d_moments, s, nullptr, &fac);
}

}  // namespace fsdf
