// depth.hip — depth-frame ingest (include/flashsdf.h "depth frames"): a depth
// image over the sensor's resident pixel directions becomes the fp64 cloud of
// its valid pixels, in row-major pixel order, with each point's pixel index.
//
// Three launches on one stream, no atomics, and no workgroup waits on another
// inside a launch — the output order is a function of the image alone:
//   depth_count_kernel<T>    counts[block] = valid pixels of the block's 256
//   depth_scan_kernel        counts -> exclusive prefix in place, total to a slot
//   depth_scatter_kernel<T>  recomputes validity; a lane's slot = the block's
//                            offset + the preceding waves' counts + the valid
//                            lanes below it in its wave; writes xyz and pix
// Per pixel, in this order and uncontracted (-ffp-contract=off):
//   s = scale · (double)depth            (exact widening for f64, f32, u16)
//   valid iff s finite, s > 0, near <= s <= far
//   c = (s u_x, s u_y, s u_z)
//   p_j = ((R_j0 c_x + R_j1 c_y) + R_j2 c_z) + t_j
// flash/depthsensors.py depth_points restates it operation for operation.
//
// Free-space samples (fsdf_set_free_space; include/flashsdf.h "free space"): the
// same three launches with a second predicate and a second total —
//   depth_count_free_kernel<T>    counts[0][block] valid, counts[1][block] sending pixels
//   depth_scan_kernel             one workgroup per row of counts, each its own total
//   depth_scatter_free_kernel<T>  the valid pixels' points as above, then J samples per
//                                 sending pixel, j-major: sample j of the r-th sending pixel
//                                 (row-major rank) at n_surface + (j − 1) · m + r
// A pixel sends iff it lies on the stride grid (row % stride == 0 and
// col % stride == 0), has a free length L — s − gap when valid; miss_range when
// that is > 0 and the pixel is a miss: not valid and not too near,
// !(s > 0 && s < near) — and L − (double)(J − 1) · spacing > 0. Sample j sits at
// range t = L − (double)(j − 1) · spacing: c = (t u_x, t u_y, t u_z), then p as
// above. flash/depthsensors.py free_space_points restates it.
//
// depth_scan_kernel also serves voxel.hip's head-flag counts (launch_block_scan).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flashsdf.h"
#include "fsdf_internal.h"

namespace fsdf {

constexpr int kDepthBlock = 256;   // one pixel per lane, four waves
constexpr int kScanBlock = 1024;   // the scan's tile: one count per lane, sixteen waves

template <typename T>
__device__ __forceinline__ bool depth_valid(T raw, const DepthRange& r, double& s) {
  s = r.scale * (double)raw;
  return __builtin_isfinite(s) && s > 0.0 && s >= r.near && s <= r.far;  // (a NaN fails every comparison)
}

template <typename T>
__global__ __launch_bounds__(kDepthBlock) void depth_count_kernel(const T* __restrict__ depth, int32_t npix,
                                                                  DepthRange r, int32_t* __restrict__ counts) {
  __shared__ int32_t wave_count[kDepthBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kDepthBlock + threadIdx.x;
  double s;
  const bool v = i < npix && depth_valid(depth[i], r, s);
  const unsigned long long m = __ballot(v);
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

// the free length L of a pixel that sends samples; false: it sends none
template <typename T>
__device__ __forceinline__ bool depth_sends(T raw, int64_t i, const DepthRange& r, const DepthFree& F, double& s,
                                            bool& valid, double& L) {
  valid = depth_valid(raw, r, s);
  const int64_t row = i / F.cols, col = i - row * F.cols;
  if (row % F.stride != 0 || col % F.stride != 0) return false;
  if (valid) L = s - F.gap;
  else if (F.miss_range > 0.0 && !(s > 0.0 && s < r.near)) L = F.miss_range;  // (a miss: NaN, <= 0, beyond far, +inf)
  else return false;
  return L - (double)(F.samples - 1) * F.spacing > 0.0;
}

template <typename T>
__global__ __launch_bounds__(kDepthBlock) void depth_count_free_kernel(const T* __restrict__ depth, int32_t npix,
                                                                       DepthRange r, DepthFree F,
                                                                       int32_t* __restrict__ counts) {
  __shared__ int32_t wave_count[2][kDepthBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kDepthBlock + threadIdx.x;
  double s = 0.0, L = 0.0;
  bool v = false;
  const bool send = i < npix && depth_sends(depth[i], i, r, F, s, v, L);
  const unsigned long long mv = __ballot(v), ms = __ballot(send);
  if ((threadIdx.x & 63) == 0) {
    wave_count[0][threadIdx.x >> 6] = __popcll(mv);
    wave_count[1][threadIdx.x >> 6] = __popcll(ms);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int32_t* wc = wave_count[threadIdx.x];
    counts[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
  }
}

// One workgroup per row of counts (gridDim.x rows of nblocks each, a total per
// row): tiles of kScanBlock counts with a running carry. A row's counts sum to
// < 2^31 (the image has fewer pixels): int32 throughout.
__global__ __launch_bounds__(kScanBlock) void depth_scan_kernel(int32_t* __restrict__ counts, int32_t nblocks,
                                                                int64_t* __restrict__ total_out) {
  __shared__ int32_t wave_total[kScanBlock / 64];
  counts += (int64_t)blockIdx.x * nblocks;
  total_out += blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t carry = 0;
  for (int32_t base = 0; base < nblocks; base += kScanBlock) {
    const int32_t i = base + (int32_t)threadIdx.x;
    const int32_t v = i < nblocks ? counts[i] : 0;
    int32_t x = v;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wave_total[w] = x;
    __syncthreads();
    int32_t before = 0, tile = 0;
#pragma unroll
    for (int k = 0; k < kScanBlock / 64; ++k) {
      const int32_t t = wave_total[k];
      if (k < w) before += t;
      tile += t;
    }
    if (i < nblocks) counts[i] = carry + before + (x - v);
    carry += tile;
    __syncthreads();  // (the next tile rewrites wave_total)
  }
  if (threadIdx.x == 0) *total_out = carry;
}

template <typename T>
__global__ __launch_bounds__(kDepthBlock) void depth_scatter_kernel(const T* __restrict__ depth,
                                                                    const double* __restrict__ u, int32_t npix,
                                                                    DepthRange r, DepthPose P,
                                                                    const int32_t* __restrict__ offsets,
                                                                    double* __restrict__ xyz,
                                                                    int32_t* __restrict__ pix) {
  __shared__ int32_t wave_count[kDepthBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kDepthBlock + threadIdx.x;
  const int w = threadIdx.x >> 6;
  double s = 0.0;
  const bool v = i < npix && depth_valid(depth[i], r, s);
  const unsigned long long m = __ballot(v);
  if ((threadIdx.x & 63) == 0) wave_count[w] = __popcll(m);
  __syncthreads();
  if (!v) return;
  int64_t slot = offsets[blockIdx.x];
  for (int k = 0; k < w; ++k) slot += wave_count[k];
  // the valid lanes below this one in its wave
  slot += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  const double cx = s * u[3 * i + 0], cy = s * u[3 * i + 1], cz = s * u[3 * i + 2];
  xyz[3 * slot + 0] = ((P.R[0] * cx + P.R[1] * cy) + P.R[2] * cz) + P.t[0];
  xyz[3 * slot + 1] = ((P.R[3] * cx + P.R[4] * cy) + P.R[5] * cz) + P.t[1];
  xyz[3 * slot + 2] = ((P.R[6] * cx + P.R[7] * cy) + P.R[8] * cz) + P.t[2];
  pix[slot] = (int32_t)i;
}

template <typename T>
__global__ __launch_bounds__(kDepthBlock) void depth_scatter_free_kernel(const T* __restrict__ depth,
                                                                         const double* __restrict__ u, int32_t npix,
                                                                         DepthRange r, DepthPose P, DepthFree F,
                                                                         int64_t n_surface, int64_t m,
                                                                         const int32_t* __restrict__ offsets,
                                                                         double* __restrict__ xyz,
                                                                         int32_t* __restrict__ pix) {
  __shared__ int32_t wave_count[2][kDepthBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kDepthBlock + threadIdx.x;
  const int w = threadIdx.x >> 6;
  double s = 0.0, L = 0.0;
  bool v = false;
  const bool send = i < npix && depth_sends(depth[i], i, r, F, s, v, L);
  const unsigned long long mv = __ballot(v), ms = __ballot(send);
  if ((threadIdx.x & 63) == 0) {
    wave_count[0][w] = __popcll(mv);
    wave_count[1][w] = __popcll(ms);
  }
  __syncthreads();
  if (!v && !send) return;
  const double ux = u[3 * i + 0], uy = u[3 * i + 1], uz = u[3 * i + 2];
  auto put = [&](int64_t slot, double t) {
    const double cx = t * ux, cy = t * uy, cz = t * uz;
    xyz[3 * slot + 0] = ((P.R[0] * cx + P.R[1] * cy) + P.R[2] * cz) + P.t[0];
    xyz[3 * slot + 1] = ((P.R[3] * cx + P.R[4] * cy) + P.R[5] * cz) + P.t[1];
    xyz[3 * slot + 2] = ((P.R[6] * cx + P.R[7] * cy) + P.R[8] * cz) + P.t[2];
    pix[slot] = (int32_t)i;
  };
  if (v) {
    int64_t slot = offsets[blockIdx.x];
    for (int k = 0; k < w; ++k) slot += wave_count[0][k];
    slot += __builtin_amdgcn_mbcnt_hi((uint32_t)(mv >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mv, 0u));
    if (slot < n_surface) put(slot, s);
  }
  if (send) {
    // this pixel's rank among the sending pixels, row-major
    int64_t rank = offsets[(int64_t)gridDim.x + blockIdx.x];
    for (int k = 0; k < w; ++k) rank += wave_count[1][k];
    rank += __builtin_amdgcn_mbcnt_hi((uint32_t)(ms >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ms, 0u));
    if (rank < m)
      for (int j = 0; j < F.samples; ++j) put(n_surface + (int64_t)j * m + rank, L - (double)j * F.spacing);
  }
}

static inline int depth_blocks(int64_t npix) { return (int)((npix + kDepthBlock - 1) / kDepthBlock); }

template <typename T>
static hipError_t count_scan(const void* d_depth, int64_t npix, const DepthRange& r, const DepthFree* F,
                             int32_t* d_counts, int64_t* d_total, hipStream_t s) {
  const int nb = depth_blocks(npix);
  if (F)
    hipLaunchKernelGGL(depth_count_free_kernel<T>, dim3((unsigned)nb), dim3(kDepthBlock), 0, s, (const T*)d_depth,
                       (int32_t)npix, r, *F, d_counts);
  else
    hipLaunchKernelGGL(depth_count_kernel<T>, dim3((unsigned)nb), dim3(kDepthBlock), 0, s, (const T*)d_depth,
                       (int32_t)npix, r, d_counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(depth_scan_kernel, dim3(F ? 2 : 1), dim3(kScanBlock), 0, s, d_counts, (int32_t)nb, d_total);
  return hipGetLastError();
}

hipError_t launch_block_scan(int32_t* d_counts, int rows, int32_t nblocks, int64_t* d_total, hipStream_t s) {
  if (!d_counts || !d_total || rows < 1 || nblocks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(depth_scan_kernel, dim3((unsigned)rows), dim3(kScanBlock), 0, s, d_counts, nblocks, d_total);
  return hipGetLastError();
}

static bool depth_free_ok(const DepthFree* F) {
  return !F || (F->samples >= 1 && F->samples <= 16 && F->stride >= 1 && F->cols >= 1);
}

static bool depth_args_ok(int format, const void* d_depth, int64_t npix) {
  return d_depth && npix >= 1 && npix <= INT32_MAX &&
         (format == FSDF_DEPTH_F64 || format == FSDF_DEPTH_F32 || format == FSDF_DEPTH_U16);
}

size_t depth_format_bytes(int format) {
  return format == FSDF_DEPTH_F64 ? sizeof(double) : format == FSDF_DEPTH_F32 ? sizeof(float) : sizeof(uint16_t);
}

hipError_t launch_depth_count(int format, const void* d_depth, int64_t npix, const DepthRange& r,
                              const DepthFree* free, int32_t* d_counts, int64_t* d_total, hipStream_t s) {
  if (!depth_args_ok(format, d_depth, npix) || !depth_free_ok(free) || !d_counts || !d_total)
    return hipErrorInvalidValue;
  if (format == FSDF_DEPTH_F64) return count_scan<double>(d_depth, npix, r, free, d_counts, d_total, s);
  if (format == FSDF_DEPTH_F32) return count_scan<float>(d_depth, npix, r, free, d_counts, d_total, s);
  return count_scan<uint16_t>(d_depth, npix, r, free, d_counts, d_total, s);
}

template <typename T>
static hipError_t scatter(const void* d_depth, const double* d_u, int64_t npix, const DepthRange& r,
                          const DepthPose& P, const DepthFree* F, int64_t n_surface, int64_t m,
                          const int32_t* d_offsets, double* d_xyz, int32_t* d_pix, hipStream_t s) {
  if (F)
    hipLaunchKernelGGL(depth_scatter_free_kernel<T>, dim3((unsigned)depth_blocks(npix)), dim3(kDepthBlock), 0, s,
                       (const T*)d_depth, d_u, (int32_t)npix, r, P, *F, n_surface, m, d_offsets, d_xyz, d_pix);
  else
    hipLaunchKernelGGL(depth_scatter_kernel<T>, dim3((unsigned)depth_blocks(npix)), dim3(kDepthBlock), 0, s,
                       (const T*)d_depth, d_u, (int32_t)npix, r, P, d_offsets, d_xyz, d_pix);
  return hipGetLastError();
}

hipError_t launch_depth_scatter(int format, const void* d_depth, const double* d_u, int64_t npix, const DepthRange& r,
                                const DepthPose& P, const DepthFree* free, int64_t n_surface, int64_t m,
                                const int32_t* d_offsets, double* d_xyz, int32_t* d_pix, hipStream_t s) {
  if (!depth_args_ok(format, d_depth, npix) || !depth_free_ok(free) || n_surface < 0 || m < 0 || !d_u ||
      !d_offsets || !d_xyz || !d_pix)
    return hipErrorInvalidValue;
#define FSDF_DEPTH_SCATTER(T) scatter<T>(d_depth, d_u, npix, r, P, free, n_surface, m, d_offsets, d_xyz, d_pix, s)
  if (format == FSDF_DEPTH_F64) return FSDF_DEPTH_SCATTER(double);
  if (format == FSDF_DEPTH_F32) return FSDF_DEPTH_SCATTER(float);
  return FSDF_DEPTH_SCATTER(uint16_t);
#undef FSDF_DEPTH_SCATTER
}

}  // namespace fsdf
