// voxel.hip — voxel-grid downsampling of a cloud on the device
// (include/flashsdf.h "voxel grid"): n fp64 points become the m centroids of
// the occupied cells of a world-anchored grid, each with its cell's population,
// in ascending cell-key order. The centroids then take the path of
// fsdf_set_points_device and the populations that of
// fsdf_set_point_weights_device (FSDF_VOXEL_COUNT).
//
// The stage, on one stream, with no atomics and no workgroup waiting on another
// — the output is a function of the input array alone:
//   voxel_key_kernel      key[i] (63 bits, all ones: dropped), idx[i] = i
//   rocprim radix sort    (u64 key, i32 idx) pairs, bits 0..64, stable
//   voxel_count_kernel    counts[0][block] segment heads, counts[1][block] dropped keys
//   block scan            depth.hip's, one workgroup per row; totals {m, dropped}
//     — the one read-back that sizes the outputs —
//   voxel_scatter_kernel  recomputes the head flags; a position's voxel = the
//                         heads at or before it − 1: start[voxel] = position of a
//                         head, voxel_of_point[idx[position]] for every position
//   voxel_fold_kernel     one lane per voxel: the left fold of its segment
//   voxel_finish_kernel   the weights (double)count (then 1.0 per free-space
//                         sample) and a depth frame's pixel list
// Per point and axis, fp64 in every context precision and uncontracted
// (-ffp-contract=off; the division is the device's correctly rounded one):
//   q = floor((x − o) / h), clamped to [−2^20, 2^20 − 1], as int32
//   key = (cz + 2^20) << 42 | (cy + 2^20) << 21 | (cx + 2^20)
// A point with a non-finite coordinate takes the all-ones key: it sorts last,
// belongs to no voxel and is counted. Centroid: acc = p_first; acc = acc + p_next
// over the segment in sorted order (ascending input index within a voxel: the
// sort is stable), then acc / (double)count, per coordinate.
// flash/depthdata.py voxel_downsample restates it operation for operation.
//
// The fold is one lane per voxel and linear in the largest cell's population: on
// camera data a segment is a few to a few dozen points; a cloud that falls into
// one cell folds on one lane (4,097 points: tests/test_gpu_voxel.py). That is
// the price of a summation order that does not depend on the launch geometry.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "ctx.h"

namespace fsdf {

constexpr int kVoxelBlock = 256;  // one point (sorted position, voxel) per lane, four waves
constexpr uint64_t kVoxelDropped = ~(uint64_t)0;
constexpr int32_t kVoxelBias = 1 << 20;

__device__ __forceinline__ uint64_t voxel_axis(double x, double o, double h) {
  double q = floor((x - o) / h);
  q = q < -1048576.0 ? -1048576.0 : (q > 1048575.0 ? 1048575.0 : q);
  return (uint64_t)((int32_t)q + kVoxelBias);
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_key_kernel(const double* __restrict__ xyz, int64_t n, VoxelGrid g,
                                                                uint64_t* __restrict__ keys,
                                                                int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  if (i >= n) return;
  const double x = xyz[3 * i + 0], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  uint64_t key = kVoxelDropped;
  if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))
    key = (voxel_axis(z, g.origin[2], g.size) << 42) | (voxel_axis(y, g.origin[1], g.size) << 21) |
          voxel_axis(x, g.origin[0], g.size);
  keys[i] = key;
  idx[i] = (int32_t)i;
}

// sorted position i starts a voxel's segment
__device__ __forceinline__ bool voxel_head(const uint64_t* __restrict__ keys, int64_t i, uint64_t k) {
  return k != kVoxelDropped && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_count_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                                                  int32_t* __restrict__ counts) {
  __shared__ int32_t wave_count[2][kVoxelBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  const uint64_t k = i < n ? keys[i] : 0;
  const bool head = i < n && voxel_head(keys, i, k), drop = i < n && k == kVoxelDropped;
  const unsigned long long mh = __ballot(head), md = __ballot(drop);
  if ((threadIdx.x & 63) == 0) {
    wave_count[0][threadIdx.x >> 6] = __popcll(mh);
    wave_count[1][threadIdx.x >> 6] = __popcll(md);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int32_t* wc = wave_count[threadIdx.x];
    counts[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
  }
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_scatter_kernel(const uint64_t* __restrict__ keys,
                                                                    const int32_t* __restrict__ idx, int64_t n,
                                                                    int64_t m, const int32_t* __restrict__ offsets,
                                                                    int32_t* __restrict__ start,
                                                                    int32_t* __restrict__ voxel_of_point) {
  __shared__ int32_t wave_count[kVoxelBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  const int w = threadIdx.x >> 6;
  const uint64_t k = i < n ? keys[i] : 0;
  const bool head = i < n && voxel_head(keys, i, k);
  const unsigned long long mh = __ballot(head);
  if ((threadIdx.x & 63) == 0) wave_count[w] = __popcll(mh);
  __syncthreads();
  if (i >= n) return;
  // the heads before this position, then this position's voxel
  int64_t v = offsets[blockIdx.x];
  for (int j = 0; j < w; ++j) v += wave_count[j];
  v += __builtin_amdgcn_mbcnt_hi((uint32_t)(mh >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mh, 0u));
  if (!head) v -= 1;
  const bool kept = k != kVoxelDropped && v >= 0 && v < m;
  if (head && kept) start[v] = (int32_t)i;
  const int64_t p = idx[i];
  if (p >= 0 && p < n) voxel_of_point[p] = kept ? (int32_t)v : -1;
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_fold_kernel(const double* __restrict__ xyz,
                                                                 const uint64_t* __restrict__ keys,
                                                                 const int32_t* __restrict__ idx,
                                                                 const int32_t* __restrict__ start, int64_t n,
                                                                 int64_t n_kept, int64_t m, double* __restrict__ out,
                                                                 int32_t* __restrict__ count,
                                                                 int32_t* __restrict__ cell,
                                                                 int32_t* __restrict__ first) {
  const int64_t v = (int64_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  if (v >= m) return;
  const int64_t s = start[v], e = v + 1 < m ? (int64_t)start[v + 1] : n_kept;
  if (s < 0 || s >= e || e > n_kept || n_kept > n) return;  // (never: the segments partition [0, n_kept))
  int64_t p = idx[s];
  if (p < 0 || p >= n) return;
  first[v] = (int32_t)p;
  double ax = xyz[3 * p + 0], ay = xyz[3 * p + 1], az = xyz[3 * p + 2];
  for (int64_t j = s + 1; j < e; ++j) {
    p = idx[j];
    if (p < 0 || p >= n) return;
    ax = ax + xyz[3 * p + 0];
    ay = ay + xyz[3 * p + 1];
    az = az + xyz[3 * p + 2];
  }
  const double c = (double)(e - s);
  out[3 * v + 0] = ax / c;
  out[3 * v + 1] = ay / c;
  out[3 * v + 2] = az / c;
  count[v] = (int32_t)(e - s);
  const uint64_t k = keys[s];
  cell[3 * v + 0] = (int32_t)(k & 0x1fffff) - kVoxelBias;
  cell[3 * v + 1] = (int32_t)((k >> 21) & 0x1fffff) - kVoxelBias;
  cell[3 * v + 2] = (int32_t)((k >> 42) & 0x1fffff) - kVoxelBias;
}

// caller point i of the downsampled cloud: a voxel (i < m) or one of the
// `tail` points that follow the input's first n_in (a depth frame's free-space
// samples). weights[i] = (double)count or 1.0; pix_out[i] = the pixel of the
// voxel's first point or the sample's own (pix_in null: no pixel list)
__global__ __launch_bounds__(kVoxelBlock) void voxel_finish_kernel(const int32_t* __restrict__ count,
                                                                   const int32_t* __restrict__ first, int64_t m,
                                                                   int64_t n_in, int64_t tail,
                                                                   const int32_t* __restrict__ pix_in,
                                                                   double* __restrict__ weights,
                                                                   int32_t* __restrict__ pix_out) {
  const int64_t i = (int64_t)blockIdx.x * kVoxelBlock + threadIdx.x;
  if (i >= m + tail) return;
  weights[i] = i < m ? (double)count[i] : 1.0;
  if (!pix_in) return;
  int64_t src = i < m ? (int64_t)first[i] : n_in + (i - m);
  if (src < 0 || src >= n_in + tail) src = 0;
  pix_out[i] = pix_in[src];
}

static inline unsigned voxel_blocks(int64_t n) { return (unsigned)((n + kVoxelBlock - 1) / kVoxelBlock); }

}  // namespace fsdf

// The stage over d_xyz [n][3] (device, fp64; read until the stream has run the
// fold): c->voxel.{xyz, count, cell, first} [m], of_point [n], vox_m, vox_n_in,
// vox_dropped. One synchronisation, for {m, dropped}. The caller has
// synchronised the stream since the lists' last reader was queued.
int voxel_downsample(fsdf_ctx* c, const double* d_xyz, int64_t n, const char* who) {
  using namespace fsdf;
  VoxelBuffers& V = c->voxel;
  c->voxel_cloud = false;  // (the lists are overwritten from here on)
  c->vox_m = c->vox_dropped = 0;
  c->vox_n_in = n;
  if (n > INT32_MAX) return fail(c, FSDF_ERR_ARG, "%s: a voxel grid downsamples < 2^31 points (n=%lld)", who, (long long)n);
  if (n <= 0) return FSDF_OK;
  const VoxelGrid g = {c->vox_size, {c->vox_origin[0], c->vox_origin[1], c->vox_origin[2]}};
  const unsigned nb = voxel_blocks(n);
  HIPCHECK(c, V.k0.reserve((size_t)n));
  HIPCHECK(c, V.k1.reserve((size_t)n));
  HIPCHECK(c, V.i0.reserve((size_t)n));
  HIPCHECK(c, V.i1.reserve((size_t)n));
  HIPCHECK(c, V.counts.reserve((size_t)2 * nb));
  HIPCHECK(c, V.total.reserve(2));
  HIPCHECK(c, V.h_total.reserve(2));
  HIPCHECK(c, V.of_point.reserve((size_t)n));
  hipStream_t st = c->stream;
  hipLaunchKernelGGL(voxel_key_kernel, dim3(nb), dim3(kVoxelBlock), 0, st, d_xyz, n, g, V.k0.get(), V.i0.get());
  HIPCHECK(c, hipGetLastError());
  {
    rocprim::double_buffer<uint64_t> keys(V.k0.get(), V.k1.get());
    rocprim::double_buffer<int32_t> vals(V.i0.get(), V.i1.get());
    size_t need = 0;
    HIPCHECK(c, rocprim::radix_sort_pairs(nullptr, need, keys, vals, (size_t)n, 0, 64, st));
    HIPCHECK(c, V.tmp.reserve(need));
    HIPCHECK(c, rocprim::radix_sort_pairs(V.tmp.get(), need, keys, vals, (size_t)n, 0, 64, st));
    // (the sorted pairs are k0 / i0 from here on)
    if (keys.current() != V.k0.get()) V.k0.swap(V.k1);
    if (vals.current() != V.i0.get()) V.i0.swap(V.i1);
  }
  hipLaunchKernelGGL(voxel_count_kernel, dim3(nb), dim3(kVoxelBlock), 0, st, V.k0.get(), n, V.counts.get());
  HIPCHECK(c, hipGetLastError());
  HIPCHECK(c, launch_block_scan(V.counts.get(), 2, (int32_t)nb, V.total.get(), st));
  HIPCHECK(c, hipMemcpyAsync(V.h_total.get(), V.total.get(), 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHECK(c, hipStreamSynchronize(st));
  const int64_t m = V.h_total.get()[0], dropped = V.h_total.get()[1];
  if (m < 0 || dropped < 0 || m + dropped > n || (m == 0) != (dropped == n))
    return fail(c, FSDF_ERR_HIP, "%s: %lld voxels and %lld dropped points of %lld", who, (long long)m,
                (long long)dropped, (long long)n);
  const size_t cap = (size_t)std::max<int64_t>(m, 1);
  HIPCHECK(c, V.start.reserve(cap));
  HIPCHECK(c, V.xyz.reserve(cap * 3));
  HIPCHECK(c, V.count.reserve(cap));
  HIPCHECK(c, V.cell.reserve(cap * 3));
  HIPCHECK(c, V.first.reserve(cap));
  hipLaunchKernelGGL(voxel_scatter_kernel, dim3(nb), dim3(kVoxelBlock), 0, st, V.k0.get(), V.i0.get(), n, m,
                     V.counts.get(), V.start.get(), V.of_point.get());
  HIPCHECK(c, hipGetLastError());
  if (m > 0) {
    hipLaunchKernelGGL(voxel_fold_kernel, dim3(voxel_blocks(m)), dim3(kVoxelBlock), 0, st, d_xyz, V.k0.get(),
                       V.i0.get(), V.start.get(), n, n - dropped, m, V.xyz.get(), V.count.get(), V.cell.get(),
                       V.first.get());
    HIPCHECK(c, hipGetLastError());
  }
  c->vox_m = m;
  c->vox_dropped = dropped;
  return FSDF_OK;
}

// After voxel_downsample: c->voxel.weights [vox_m + tail] = the counts as
// doubles, then 1.0 per tail point; with d_pix_in (a depth frame's pixel list
// [vox_n_in + tail]) also c->voxel.pix [vox_m + tail].
int voxel_finish(fsdf_ctx* c, int64_t tail, const int32_t* d_pix_in) {
  using namespace fsdf;
  VoxelBuffers& V = c->voxel;
  const int64_t n2 = c->vox_m + tail;
  const size_t cap = (size_t)std::max<int64_t>(n2, 1);
  HIPCHECK(c, V.weights.reserve(cap));
  if (d_pix_in) HIPCHECK(c, V.pix.reserve(cap));
  if (n2 <= 0) return FSDF_OK;
  hipLaunchKernelGGL(voxel_finish_kernel, dim3(voxel_blocks(n2)), dim3(kVoxelBlock), 0, c->stream, V.count.get(),
                     V.first.get(), c->vox_m, c->vox_n_in, tail, d_pix_in, V.weights.get(),
                     d_pix_in ? V.pix.get() : nullptr);
  HIPCHECK(c, hipGetLastError());
  return FSDF_OK;
}

// The counts become the resident cloud's weights (FSDF_VOXEL_COUNT): the path of
// fsdf_set_point_weights_device. An empty cloud takes none.
int voxel_set_weights(fsdf_ctx* c) {
  if (c->vox_weights != FSDF_VOXEL_COUNT || c->n <= 0) return FSDF_OK;
  return fsdf_set_point_weights_device(c, c->voxel.weights.get(), c->n);
}

static int set_voxel_grid_impl(fsdf_ctx* c, double size, const double* origin, int32_t weights) {
  if (!c) return FSDF_ERR_ARG;
  if (size == 0.0) {  // off (origin and weights ignored)
    c->vox_size = 0.0;
    return FSDF_OK;
  }
  if (!(size > 0.0 && size <= 1.79769313486231570815e308))  // (a NaN fails the first test)
    return fail(c, FSDF_ERR_ARG, "set_voxel_grid: cell size %g (finite and > 0, or 0 for off); the earlier grid stays",
                size);
  if (origin)
    for (int j = 0; j < 3; ++j)
      if (!std::isfinite(origin[j]))
        return fail(c, FSDF_ERR_ARG, "set_voxel_grid: origin entry %d is %g; the earlier grid stays", j, origin[j]);
  if (weights != FSDF_VOXEL_UNIT && weights != FSDF_VOXEL_COUNT)
    return fail(c, FSDF_ERR_ARG, "set_voxel_grid: unknown weights mode %d; the earlier grid stays", weights);
  c->vox_size = size;
  for (int j = 0; j < 3; ++j) c->vox_origin[j] = origin ? origin[j] : 0.0;
  c->vox_weights = weights;
  return FSDF_OK;
}

extern "C" int fsdf_set_voxel_grid(fsdf_ctx* c, double size, const double* origin, int32_t weights) {
  return set_voxel_grid_impl(c, size, origin, weights);
}

extern "C" int fsdf_set_voxel_grid_ref(fsdf_ctx* c, const double* size, const double* origin, int32_t weights) {
  return set_voxel_grid_impl(c, size ? *size : 0.0, origin, weights);
}

extern "C" int fsdf_get_voxel_grid(const fsdf_ctx* c, double* size_out, double* origin_out, int32_t* weights_out) {
  if (!c) return FSDF_ERR_ARG;
  if (size_out) *size_out = c->vox_size;
  if (origin_out)
    for (int j = 0; j < 3; ++j) origin_out[j] = c->vox_origin[j];
  if (weights_out) *weights_out = c->vox_weights;
  return FSDF_OK;
}

static int set_points_voxel_impl(fsdf_ctx* c, const double* src, int64_t n, bool device_src, const char* who) {
  if (!c) return FSDF_ERR_ARG;
  if (!(c->vox_size > 0.0)) return fail(c, FSDF_ERR_STATE, "%s: no voxel grid (fsdf_set_voxel_grid first)", who);
  if (n < 0 || (n > 0 && !src)) return fail(c, FSDF_ERR_ARG, "%s: bad buffer (n=%lld)", who, (long long)n);
  HIPCHECK(c, hipSetDevice(c->device));
  // the previous frame's work may still read the staging buffer and the lists a reserve frees
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  const double* d_src = src;
  if (!device_src && n > 0) {
    HIPCHECK(c, c->staging.reserve((size_t)n * 3));
    HIPCHECK(c, hipMemcpyAsync(c->staging.get(), src, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice,
                               c->stream));
    d_src = c->staging.get();
  }
  int rc = voxel_downsample(c, d_src, n, who);
  if (rc) return rc;
  rc = voxel_finish(c, 0, nullptr);
  if (rc) return rc;
  // (synchronous: the fold has read the caller's array when this returns)
  rc = fsdf_set_points_device(c, c->voxel.xyz.get(), c->vox_m);
  if (rc) return rc;
  c->voxel_cloud = true;
  return voxel_set_weights(c);
}

extern "C" int fsdf_set_points_voxel(fsdf_ctx* c, const double* xyz, int64_t n) {
  return set_points_voxel_impl(c, xyz, n, false, "set_points_voxel");
}

extern "C" int fsdf_set_points_voxel_device(fsdf_ctx* c, const double* d_xyz, int64_t n) {
  return set_points_voxel_impl(c, d_xyz, n, true, "set_points_voxel_device");
}

extern "C" int fsdf_get_voxels(fsdf_ctx* c, double* xyz_out, int32_t* count_out, int32_t* cell_out, int64_t* m_out,
                               int64_t* n_in_out, int64_t* dropped_out) {
  if (!c) return FSDF_ERR_ARG;
  if (!c->voxel_cloud)
    return fail(c, FSDF_ERR_STATE,
                "get_voxels: the resident cloud did not come through a voxel grid (fsdf_set_voxel_grid, then "
                "fsdf_set_points_voxel or a depth frame)");
  if (m_out) *m_out = c->vox_m;
  if (n_in_out) *n_in_out = c->vox_n_in;
  if (dropped_out) *dropped_out = c->vox_dropped;
  const size_t m = (size_t)c->vox_m;
  if (m == 0 || (!xyz_out && !count_out && !cell_out)) return FSDF_OK;
  HIPCHECK(c, hipSetDevice(c->device));
  if (xyz_out)
    HIPCHECK(c, hipMemcpyAsync(xyz_out, c->voxel.xyz.get(), m * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (count_out)
    HIPCHECK(c, hipMemcpyAsync(count_out, c->voxel.count.get(), m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (cell_out)
    HIPCHECK(c, hipMemcpyAsync(cell_out, c->voxel.cell.get(), m * 3 * sizeof(int32_t), hipMemcpyDeviceToHost,
                               c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}

extern "C" int fsdf_get_voxel_of_point(fsdf_ctx* c, int32_t* out, int64_t* n_in_out) {
  if (!c) return FSDF_ERR_ARG;
  if (!c->voxel_cloud)
    return fail(c, FSDF_ERR_STATE,
                "get_voxel_of_point: the resident cloud did not come through a voxel grid (fsdf_set_voxel_grid, then "
                "fsdf_set_points_voxel or a depth frame)");
  if (n_in_out) *n_in_out = c->vox_n_in;
  if (!out || c->vox_n_in == 0) return FSDF_OK;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipMemcpyAsync(out, c->voxel.of_point.get(), (size_t)c->vox_n_in * sizeof(int32_t),
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}
