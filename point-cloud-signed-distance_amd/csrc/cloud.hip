// cloud.hip — the resident cloud of a context: ingest (host, device, ranges,
// keyed shards, depth frames over a resident sensor), the seeds carried from
// one cloud to the next, the next frame's prefetch, and the regroup by nearest
// surface.

#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ctx.h"

// Convert/copy AoS f64 points already on the device into a resident buffer of
// the context precision, growing it when needed.
int adopt_points_device(fsdf_ctx* c, const double* d_src, int64_t n, fsdf::DevBuf<unsigned char>& dst) {
  HIPCHECK(c, dst.reserve((size_t)std::max<int64_t>(n, 1) * 3 * point_bytes(c)));
  if (n == 0) return FSDF_OK;
  if (c->precision == 64) {
    HIPCHECK(c, hipMemcpyAsync(dst.get(), d_src, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  } else {
    HIPCHECK(c, fsdf::launch_to_f32(d_src, (float*)dst.get(), n * 3, c->stream));
  }
  return FSDF_OK;
}

static int finish_resident(fsdf_ctx* c, int64_t n, bool ranged, bool spheres_done = false);

// Seeds for a new cloud's first pass from the last pass over the previous one
// (fsdf_set_points / fsdf_set_points_prefetched of sorting hull-only contexts):
// before the cloud is replaced its points write their k* into a coarse voxel
// grid (carry_seeds_out), after it the new points read theirs into the seed
// buffer (finish_resident). The grid's box is the first cloud's box grown by
// a quarter of its extent each way, fixed for the context. Seeds only order
// the search — the pass's bits do not depend on them (tests/test_gpu_tracking.py).
static bool seeds_apply(const fsdf_ctx* c) {
  return c->sort_points && c->lm.R == 0 && c->lm.S <= 64 && c->lm.K > 0;
}

static int ensure_vox_box(fsdf_ctx* c, const double* d_src, int64_t n) {
  if (c->vox_ok || n <= 0 || !seeds_apply(c)) return FSDF_OK;
  double* d_box = nullptr;
  hipError_t e = fsdf::cloud_box(d_src, n, c->sort, c->stream, &d_box);
  if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "set_points (seed box): %s", hipGetErrorString(e));
  double box[6];
  HIPCHECK(c, hipMemcpyAsync(box, d_box, sizeof box, hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (once per context)
  for (int j = 0; j < 3; ++j) {
    const double ext = std::max(box[3 + j] - box[j], 1e-3);
    if (!std::isfinite(ext)) return FSDF_OK;  // (no seeds)
    c->vox.lo[j] = box[j] - 0.25 * ext;
    c->vox.inv[j] = fsdf::kVoxDim / (1.5 * ext);
  }
  HIPCHECK(c, c->vox_grid.reserve((size_t)fsdf::kVoxDim * fsdf::kVoxDim * fsdf::kVoxDim));
  c->vox_ok = true;
  return FSDF_OK;
}

static int carry_seeds_out(fsdf_ctx* c) {
  c->seed_pending = false;
  if (!c->vox_ok || !seeds_apply(c) || c->n <= 0 || !c->prior_pass || c->prior.capacity() < (size_t)c->n || c->ranged)
    return FSDF_OK;
  uint8_t* grid = c->vox_grid.get();
  HIPCHECK(c, hipMemsetAsync(grid, 0xFF, (size_t)fsdf::kVoxDim * fsdf::kVoxDim * fsdf::kVoxDim, c->stream));
  hipError_t e = fsdf::vox_scatter(c->precision, c->cur.pts.get(), c->n, c->prior.get(), c->vox, grid, c->stream);
  if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "set_points (seeds): %s", hipGetErrorString(e));
  c->seed_pending = true;
  return FSDF_OK;
}

// [begin, end): the resident cloud is that range of the whole cloud's order
// (the Hilbert order of all n points with sort_points, else the caller's);
// the permutation then holds the points' indices in the whole cloud
// (fsdf_set_points_range). begin = 0, end = n: the whole cloud.
static int set_points_impl(fsdf_ctx* c, const double* src, int64_t n, bool device_src, int64_t begin, int64_t end,
                           bool range_call = false) {
  if (!c) return FSDF_ERR_ARG;
  if (n < 0 || (n > 0 && !src)) return fail(c, FSDF_ERR_ARG, "set_points: bad buffer (n=%lld)", (long long)n);
  if (begin < 0 || end < begin || end > n)
    return fail(c, FSDF_ERR_ARG, "set_points_range: bad range [%lld, %lld) of %lld points", (long long)begin,
                (long long)end, (long long)n);
  if ((c->sort_points || begin > 0 || end < n) && n > INT32_MAX)
    return fail(c, FSDF_ERR_ARG, "set_points: sorted or ranged clouds support < 2^31 points (n=%lld)", (long long)n);
  const bool ranged = begin > 0 || end < n;
  HIPCHECK(c, hipSetDevice(c->device));
  // the previous frame's work may still read the staging buffer / the cloud
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  int rc0 = ranged ? FSDF_OK : carry_seeds_out(c);  // (the previous cloud, still resident)
  if (rc0) return rc0;
  c->n = 0;
  c->conf_set = c->conf_stale = false;  // (weights belong to the cloud that leaves)
  c->free_split = -1;                    // (and so does the split of its free-space samples)
  c->depth_cloud = false;                // (and so do a depth frame's pixel indices)
  c->voxel_cloud = false;                // (and a voxel cloud's lists)
  const double* d_src = src;
  if (!device_src && n > 0) {
    HIPCHECK(c, c->staging.reserve((size_t)n * 3));
    HIPCHECK(c, hipMemcpyAsync(c->staging.get(), src, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice,
                               c->stream));
    d_src = c->staging.get();
  }
  const int64_t nr = end - begin;  // resident points
  const size_t tsz = point_bytes(c);
  auto ensure_res = [&]() -> int {
    HIPCHECK(c, c->cur.pts.reserve((size_t)std::max<int64_t>(nr, 1) * 3 * tsz));
    HIPCHECK(c, c->cur.perm.reserve((size_t)std::max<int64_t>(nr, 1)));
    return FSDF_OK;
  };
  if (c->sort_points && n > 0) {
    // spatially coherent resident order + permutation back to caller order
    int rc = ensure_res();
    if (rc) return rc;
    if (!ranged) {
      rc = ensure_vox_box(c, d_src, n);
      if (rc) return rc;
    }
    if (!ranged) {
      hipError_t e = fsdf::sort_points_spatial(d_src, n, c->precision, c->cur.pts.get(), c->cur.perm.get(), c->sort,
                                               c->stream);
      if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "set_points (sort): %s", hipGetErrorString(e));
    } else {
      // the whole cloud sorted into scratch, then the range kept
      HIPCHECK(c, c->range_pts.reserve((size_t)n * 3 * tsz));
      HIPCHECK(c, c->range_perm.reserve((size_t)n));
      hipError_t e = fsdf::sort_points_spatial(d_src, n, c->precision, c->range_pts.get(), c->range_perm.get(),
                                               c->sort, c->stream);
      if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "set_points_range (sort): %s", hipGetErrorString(e));
      if (nr > 0) {
        HIPCHECK(c, hipMemcpyAsync(c->cur.pts.get(), c->range_pts.get() + (size_t)begin * 3 * tsz,
                                   (size_t)nr * 3 * tsz, hipMemcpyDeviceToDevice, c->stream));
        HIPCHECK(c, hipMemcpyAsync(c->cur.perm.get(), c->range_perm.get() + begin, (size_t)nr * sizeof(int32_t),
                                   hipMemcpyDeviceToDevice, c->stream));
      }
    }
  } else if (ranged) {
    // a slice of the caller's order; the permutation names the slice's indices
    int rc = ensure_res();
    if (rc) return rc;
    rc = adopt_points_device(c, d_src + 3 * begin, nr, c->cur.pts);
    if (rc) return rc;
    std::vector<int32_t> idx((size_t)std::max<int64_t>(nr, 0));
    for (int64_t i = 0; i < nr; ++i) idx[(size_t)i] = (int32_t)(begin + i);
    if (nr > 0)
      HIPCHECK(c, hipMemcpyAsync(c->cur.perm.get(), idx.data(), (size_t)nr * sizeof(int32_t), hipMemcpyHostToDevice,
                                 c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (idx is a host temporary)
  } else {
    c->cur.perm.reset();  // (no permutation: the resident order is the caller's)
    int rc = adopt_points_device(c, d_src, n, c->cur.pts);
    if (rc) return rc;
  }
  return finish_resident(c, nr, ranged || range_call);
}

// the per-cloud state of a new resident cloud of n points (cur.pts / cur.perm
// written, stream-ordered): chunk spheres (unless spheres_done: a prefetched
// cloud's came with it), seed buffer, plan and regroup state
static int finish_resident(fsdf_ctx* c, int64_t n, bool ranged, bool spheres_done) {
  if (n > 0 && !spheres_done) {  // per-chunk bounding spheres of the resident order (pose-independent)
    // (padded to whole 4-chunk pass workgroups: every wave of a hull-partitioned
    // pass reads its chunk's row, also past the cloud's end)
    const int64_t nc = ((n + 63) / 64 + 3) & ~(int64_t)3;
    if (c->cur.chunk_ws.capacity() < (size_t)nc * 4) HIPCHECK(c, hipStreamSynchronize(c->stream));
    HIPCHECK(c, c->cur.chunk_ws.reserve((size_t)nc * 4));
    HIPCHECK(c, fsdf::launch_chunk_spheres(c->precision, c->cur.pts.get(), n, nc, c->cur.chunk_ws.get(),
                                           c->stream));
  }
  if (n > 0) {
    // (the previous frame's passes are done: synchronised above; the seed scatter may still read it)
    if (c->prior.capacity() < (size_t)n) HIPCHECK(c, hipStreamSynchronize(c->stream));
    HIPCHECK(c, c->prior.reserve((size_t)n));
  }
  // a new cloud: its first pass seeds from the previous cloud's voxels, else from the bounds;
  // gathered seeds are readable (prior_ok) but no pass's k* (prior_pass): 0xFF where no voxel was hit
  c->prior_ok = c->prior_pass = false;
  if (c->seed_pending && n > 0 && !ranged) {
    hipError_t e = fsdf::vox_gather(c->precision, c->cur.pts.get(), n, c->vox, c->vox_grid.get(), c->prior.get(),
                                    c->stream);
    if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "set_points (seeds): %s", hipGetErrorString(e));
    c->prior_ok = true;
  }
  c->seed_pending = false;
  c->conf_set = c->conf_stale = false;  // (a new cloud: no weights until fsdf_set_point_weights)
  c->free_split = -1;                    // (and no free-space samples until fsdf_set_free_split)
  c->regrouped = false;
  c->regroup_pending = true;  // (the auto regroup follows the new cloud's first iteration pass)
  c->last_pass_shape = 0;
  // the caller may reuse its buffer once this returns
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  c->n = n;
  // (a range call keeps resident-order outputs even when its range is the
  // whole cloud: the caller indexes them through the permutation)
  c->ranged = ranged;
  c->plan_nc = -1;  // a new cloud: its first planned pass runs the default shape and measures
  // and its first one-wave pass runs the previous cloud's Hilbert-layout
  // order and rebuilds it from its own costs (left to age, a stale order cost
  // the next passes 0.094 -> 0.111 ms, tools/seed_probe.py)
  c->order_age[0] = kOrderEvery;
  return FSDF_OK;
}

// ---- exchanged spatial shards (O(N/W) ingest per rank) ------------------------
extern "C" int fsdf_cloud_box_device(fsdf_ctx* c, const double* d_xyz, int64_t n, double* box_out) {
  if (!c) return FSDF_ERR_ARG;
  if (n < 0 || (n > 0 && !d_xyz) || !box_out) return fail(c, FSDF_ERR_ARG, "cloud_box_device: bad arguments");
  HIPCHECK(c, hipSetDevice(c->device));
  if (n == 0) {
    for (int j = 0; j < 3; ++j) {
      box_out[j] = HUGE_VAL;
      box_out[3 + j] = -HUGE_VAL;
    }
    return FSDF_OK;
  }
  double* d_box = nullptr;
  hipError_t e = fsdf::cloud_box(d_xyz, n, c->sort, c->stream, &d_box);
  if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "cloud_box_device: %s", hipGetErrorString(e));
  HIPCHECK(c, hipMemcpyAsync(box_out, d_box, 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}

extern "C" int fsdf_curve_keys_device(fsdf_ctx* c, const double* d_xyz, int64_t n, const double* box,
                                      uint32_t* d_keys) {
  if (!c) return FSDF_ERR_ARG;
  if (n < 0 || (n > 0 && (!d_xyz || !d_keys)) || !box) return fail(c, FSDF_ERR_ARG, "curve_keys_device: bad arguments");
  for (int j = 0; j < 6; ++j)
    if (!std::isfinite(box[j])) return fail(c, FSDF_ERR_ARG, "curve_keys_device: box not finite");
  HIPCHECK(c, hipSetDevice(c->device));
  if (n == 0) return FSDF_OK;
  double* d_box = nullptr;  // (the scratch's box slot, filled from the host)
  hipError_t e = fsdf::cloud_box(d_xyz, 0, c->sort, c->stream, &d_box);
  if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "curve_keys_device: %s", hipGetErrorString(e));
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (an earlier sort may still read the slot)
  HIPCHECK(c, hipMemcpy(d_box, box, 6 * sizeof(double), hipMemcpyHostToDevice));
  e = fsdf::curve_keys(d_xyz, n, d_box, d_keys, c->stream);
  if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "curve_keys_device: %s", hipGetErrorString(e));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}

extern "C" int fsdf_set_points_keyed_device(fsdf_ctx* c, const double* d_xyz, const uint32_t* d_keys,
                                            const int64_t* d_index, int64_t n) {
  if (!c) return FSDF_ERR_ARG;
  if (n < 0 || (n > 0 && (!d_xyz || !d_keys || !d_index)))
    return fail(c, FSDF_ERR_ARG, "set_points_keyed_device: bad arguments");
  if (n > INT32_MAX) return fail(c, FSDF_ERR_ARG, "set_points_keyed_device: < 2^31 points per shard");
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  c->n = 0;
  c->conf_set = c->conf_stale = false;  // (weights belong to the cloud that leaves)
  c->free_split = -1;                    // (and so does the split of its free-space samples)
  c->depth_cloud = false;                // (and so do a depth frame's pixel indices)
  c->voxel_cloud = false;                // (and a voxel cloud's lists)
  HIPCHECK(c, c->cur.pts.reserve((size_t)std::max<int64_t>(n, 1) * 3 * point_bytes(c)));
  HIPCHECK(c, c->cur.perm.reserve((size_t)std::max<int64_t>(n, 1)));
  if (n > 0) {
    hipError_t e = fsdf::sort_points_keyed(d_xyz, d_keys, d_index, n, c->precision, c->cur.pts.get(),
                                           c->cur.perm.get(), c->sort, c->stream);
    if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "set_points_keyed_device (sort): %s", hipGetErrorString(e));
  }
  return finish_resident(c, n, true);
}

extern "C" int fsdf_set_points(fsdf_ctx* c, const double* xyz, int64_t n) {
  return set_points_impl(c, xyz, n, false, 0, n);
}

extern "C" int fsdf_set_points_device(fsdf_ctx* c, const double* d_xyz, int64_t n) {
  return set_points_impl(c, d_xyz, n, true, 0, n);
}

// ---- depth frames (include/flashsdf.h "depth frames"; kernels: depth.hip) ------
// The sensor: one direction per pixel, computed here once and kept on the device.
extern "C" int fsdf_set_sensor(fsdf_ctx* c, const double* rays, int32_t rows, int32_t cols, int32_t depth_kind) {
  if (!c) return FSDF_ERR_ARG;
  if (!rays) {  // clear
    c->sensor_rows = c->sensor_cols = 0;
    return FSDF_OK;
  }
  if (depth_kind != FSDF_DEPTH_RANGE && depth_kind != FSDF_DEPTH_Z)
    return fail(c, FSDF_ERR_ARG, "set_sensor: unknown depth kind %d; the earlier sensor stays", depth_kind);
  if (rows < 1 || cols < 1 || (int64_t)rows * cols > INT32_MAX)
    return fail(c, FSDF_ERR_ARG, "set_sensor: %d x %d pixels (rows, cols >= 1, rows * cols < 2^31); the earlier sensor stays",
                rows, cols);
  const int64_t npix = (int64_t)rows * cols;
  std::vector<double> u((size_t)npix * 3);
  for (int64_t i = 0; i < npix; ++i) {
    const double x = rays[3 * i], y = rays[3 * i + 1], z = rays[3 * i + 2];
    bool ok = std::isfinite(x) && std::isfinite(y) && std::isfinite(z);
    if (ok && depth_kind == FSDF_DEPTH_RANGE) {
      const double nrm = sqrt((x * x + y * y) + z * z);
      ok = std::isfinite(nrm) && nrm > 0.0;
      if (ok) {
        u[3 * i] = x / nrm;
        u[3 * i + 1] = y / nrm;
        u[3 * i + 2] = z / nrm;
      }
    } else if (ok) {
      ok = z > 0.0;
      if (ok) {
        u[3 * i] = x / z;
        u[3 * i + 1] = y / z;
        u[3 * i + 2] = 1.0;
      }
    }
    if (!ok)
      return fail(c, FSDF_ERR_ARG,
                  "set_sensor: ray %lld is (%g, %g, %g) (rays are finite and not zero, z > 0 for FSDF_DEPTH_Z); the "
                  "earlier sensor stays", (long long)i, x, y, z);
  }
  HIPCHECK(c, hipSetDevice(c->device));
  // (a depth frame still queued may read the table a growing reserve frees)
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  c->sensor_rows = c->sensor_cols = 0;
  HIPCHECK(c, c->sensor_u.reserve(u.size()));
  HIPCHECK(c, hipMemcpyAsync(c->sensor_u.get(), u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (u is a host temporary)
  c->sensor_rows = rows;
  c->sensor_cols = cols;
  c->sensor_kind = depth_kind;
  return FSDF_OK;
}

extern "C" int fsdf_get_sensor(const fsdf_ctx* c, int32_t* rows_out, int32_t* cols_out, int32_t* kind_out) {
  if (!c) return FSDF_ERR_ARG;
  if (rows_out) *rows_out = c->sensor_rows;
  if (cols_out) *cols_out = c->sensor_cols;
  if (kind_out) *kind_out = c->sensor_kind;
  return FSDF_OK;
}

// A frame under a voxel grid (fsdf_set_voxel_grid; voxel.hip): `staging` holds
// the frame's n_surface observed points, then `tail` free-space samples, and
// depth_pix their pixels. The observed points become their m voxel centroids —
// one more sizing synchronisation, for m —, the samples follow unchanged
// (c->voxel.cloud), a voxel's pixel is its first point's, the split is m, and
// under FSDF_VOXEL_COUNT the weights are the counts, then 1.0 per sample.
static int set_depth_voxel(fsdf_ctx* c, int64_t n_surface, int64_t tail, const char* who) {
  int rc = voxel_downsample(c, c->staging.get(), n_surface, who);
  if (rc) return rc;
  rc = voxel_finish(c, tail, c->depth_pix.get());
  if (rc) return rc;
  const int64_t m = c->vox_m, n = m + tail;
  HIPCHECK(c, c->voxel.cloud.reserve((size_t)std::max<int64_t>(n, 1) * 3));
  if (m > 0)
    HIPCHECK(c, hipMemcpyAsync(c->voxel.cloud.get(), c->voxel.xyz.get(), (size_t)m * 3 * sizeof(double),
                               hipMemcpyDeviceToDevice, c->stream));
  if (tail > 0)
    HIPCHECK(c, hipMemcpyAsync(c->voxel.cloud.get() + 3 * m, c->staging.get() + 3 * n_surface,
                               (size_t)tail * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  c->depth_pix.swap(c->voxel.pix);  // (stream-ordered: the finish kernel read the old list)
  rc = set_points_impl(c, c->voxel.cloud.get(), n, true, 0, n);
  if (rc) return rc;
  c->depth_cloud = true;
  c->voxel_cloud = true;
  c->free_split = m < n ? m : -1;
  return voxel_set_weights(c);
}

// A frame: count and scan, the 8-byte total back (the one synchronisation that
// sizes the cloud), the scatter into `staging`, and from there the frame is
// fsdf_set_points_device of that array.
static int set_depth_impl(fsdf_ctx* c, const void* depth, int format, bool device_src, const double* pose,
                          const double* range, const char* who) {
  if (!c) return FSDF_ERR_ARG;
  if (format != FSDF_DEPTH_F64 && format != FSDF_DEPTH_F32 && format != FSDF_DEPTH_U16)
    return fail(c, FSDF_ERR_ARG, "%s: unknown depth format %d", who, format);
  if (c->sensor_rows < 1) return fail(c, FSDF_ERR_STATE, "%s: no sensor (fsdf_set_sensor first)", who);
  if (!depth) return fail(c, FSDF_ERR_ARG, "%s: null depth image", who);
  fsdf::DepthPose P = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}};
  if (pose) {
    for (int j = 0; j < 12; ++j)
      if (!std::isfinite(pose[j])) return fail(c, FSDF_ERR_ARG, "%s: pose entry %d is %g; the resident cloud stays", who, j, pose[j]);
    for (int j = 0; j < 9; ++j) P.R[j] = pose[j];
    for (int j = 0; j < 3; ++j) P.t[j] = pose[9 + j];
  }
  fsdf::DepthRange r = {0.0, HUGE_VAL, 1.0};
  if (range) {
    r.near = range[0];
    r.far = range[1];
    r.scale = range[2];
    if (std::isnan(r.near) || std::isnan(r.far) || r.near > r.far)
      return fail(c, FSDF_ERR_ARG, "%s: range [%g, %g] (near <= far, neither a NaN); the resident cloud stays", who,
                  r.near, r.far);
    if (!(std::isfinite(r.scale) && r.scale > 0.0))
      return fail(c, FSDF_ERR_ARG, "%s: scale %g (finite and > 0); the resident cloud stays", who, r.scale);
  }
  const int64_t npix = (int64_t)c->sensor_rows * c->sensor_cols;
  const size_t nblocks = (size_t)((npix + 255) / 256);
  // free-space samples (fsdf_set_free_space): a second predicate and a second total in the same launches
  const int J = c->free_samples;
  const fsdf::DepthFree F = {J, c->free_stride, c->sensor_cols, c->free_gap, c->free_spacing, c->free_miss};
  const fsdf::DepthFree* Fp = J > 0 ? &F : nullptr;
  HIPCHECK(c, hipSetDevice(c->device));
  // the previous frame's work may still read the staging buffer and the buffers a reserve frees
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  HIPCHECK(c, c->depth_counts.reserve(2 * nblocks));
  HIPCHECK(c, c->depth_total.reserve(2));
  HIPCHECK(c, c->h_depth_total.reserve(2));
  const void* d_depth = depth;
  if (!device_src) {
    const size_t bytes = (size_t)npix * fsdf::depth_format_bytes(format);
    HIPCHECK(c, c->depth_raw.reserve(bytes));
    HIPCHECK(c, hipMemcpyAsync(c->depth_raw.get(), depth, bytes, hipMemcpyHostToDevice, c->stream));
    d_depth = c->depth_raw.get();
  }
  hipError_t e = fsdf::launch_depth_count(format, d_depth, npix, r, Fp, c->depth_counts.get(), c->depth_total.get(),
                                          c->stream);
  if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "%s (count): %s", who, hipGetErrorString(e));
  // (both totals in the one read-back that sizes the cloud)
  HIPCHECK(c, hipMemcpyAsync(c->h_depth_total.get(), c->depth_total.get(), (Fp ? 2 : 1) * sizeof(int64_t),
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  const int64_t n_surface = c->h_depth_total.get()[0], m = Fp ? c->h_depth_total.get()[1] : 0;
  if (n_surface < 0 || n_surface > npix)
    return fail(c, FSDF_ERR_HIP, "%s: %lld valid pixels of %lld", who, (long long)n_surface, (long long)npix);
  if (m < 0 || m > npix)
    return fail(c, FSDF_ERR_HIP, "%s: %lld pixels of %lld send free-space samples", who, (long long)m, (long long)npix);
  const int64_t n = n_surface + (int64_t)J * m;
  if (n > INT32_MAX)
    return fail(c, FSDF_ERR_ARG,
                "%s: %lld points and %d x %lld free-space samples (fsdf_set_free_space) exceed 2^31 - 1 points; the "
                "resident cloud stays", who, (long long)n_surface, J, (long long)m);
  // (the resident cloud's pixel list is overwritten from here on: whatever
  // happens next, it no longer names a depth frame's pixels)
  c->depth_cloud = false;
  HIPCHECK(c, c->staging.reserve((size_t)std::max<int64_t>(n, 1) * 3));
  HIPCHECK(c, c->depth_pix.reserve((size_t)std::max<int64_t>(n, 1)));
  if (n > 0) {
    e = fsdf::launch_depth_scatter(format, d_depth, c->sensor_u.get(), npix, r, P, Fp, n_surface, m,
                                   c->depth_counts.get(), c->staging.get(), c->depth_pix.get(), c->stream);
    if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "%s (scatter): %s", who, hipGetErrorString(e));
  }
  if (c->vox_size > 0.0) return set_depth_voxel(c, n_surface, n - n_surface, who);
  const int rc = set_points_impl(c, c->staging.get(), n, true, 0, n);
  if (rc) return rc;
  c->depth_cloud = true;
  c->free_split = n_surface < n ? n_surface : -1;  // (the samples follow the observed points; none: no split)
  return FSDF_OK;
}

// ---- free space (include/flashsdf.h "free space") --------------------------------
extern "C" int fsdf_set_free_split(fsdf_ctx* c, int64_t n_surface) {
  if (!c) return FSDF_ERR_ARG;
  if (n_surface < 0 || n_surface == c->n) {  // clear: every point is a surface observation again
    c->free_split = -1;
    return FSDF_OK;
  }
  if (c->ranged)
    return fail(c, FSDF_ERR_STATE, "set_free_split: a split serves a whole resident cloud (not a ranged or keyed one)");
  if (n_surface > c->n)
    return fail(c, FSDF_ERR_ARG, "set_free_split: n_surface %lld of a resident cloud of %lld points; the earlier split stays",
                (long long)n_surface, (long long)c->n);
  c->free_split = n_surface;
  return FSDF_OK;
}

extern "C" int fsdf_get_free_split(const fsdf_ctx* c, int64_t* n_surface_out, int32_t* set_out) {
  if (!c) return FSDF_ERR_ARG;
  if (n_surface_out) *n_surface_out = c->free_split >= 0 ? c->free_split : c->n;
  if (set_out) *set_out = c->free_split >= 0 ? 1 : 0;
  return FSDF_OK;
}

extern "C" int fsdf_set_free_space(fsdf_ctx* c, int32_t samples, int32_t stride, const double* lengths) {
  if (!c) return FSDF_ERR_ARG;
  if (samples == 0) {  // off (stride and lengths ignored)
    c->free_samples = 0;
    return FSDF_OK;
  }
  if (samples < 0 || samples > 16)
    return fail(c, FSDF_ERR_ARG, "set_free_space: %d samples per pixel (0 to 16); the earlier setting stays", samples);
  if (stride < 1) return fail(c, FSDF_ERR_ARG, "set_free_space: stride %d (>= 1); the earlier setting stays", stride);
  if (!lengths) return fail(c, FSDF_ERR_ARG, "set_free_space: null lengths; the earlier setting stays");
  const double gap = lengths[0], spacing = lengths[1], miss = lengths[2];
  const double big = 1.79769313486231570815e308;
  if (!(gap >= 0.0 && gap <= big) || !(spacing >= 0.0 && spacing <= big) || !(miss >= 0.0 && miss <= big) ||
      (samples > 1 && !(spacing > 0.0)))  // (a NaN fails the first test of each)
    return fail(c, FSDF_ERR_ARG,
                "set_free_space: gap %g, spacing %g, miss_range %g (finite and >= 0, spacing > 0 with more than one "
                "sample); the earlier setting stays", gap, spacing, miss);
  c->free_samples = samples;
  c->free_stride = stride;
  c->free_gap = gap;
  c->free_spacing = spacing;
  c->free_miss = miss;
  return FSDF_OK;
}

extern "C" int fsdf_get_free_space(const fsdf_ctx* c, int32_t* samples_out, int32_t* stride_out, double* lengths_out) {
  if (!c) return FSDF_ERR_ARG;
  if (samples_out) *samples_out = c->free_samples;
  if (stride_out) *stride_out = c->free_stride;
  if (lengths_out) {
    lengths_out[0] = c->free_gap;
    lengths_out[1] = c->free_spacing;
    lengths_out[2] = c->free_miss;
  }
  return FSDF_OK;
}

extern "C" int fsdf_set_depth_f64(fsdf_ctx* c, const double* depth, const double* pose, const double* range) {
  return set_depth_impl(c, depth, FSDF_DEPTH_F64, false, pose, range, "set_depth_f64");
}

extern "C" int fsdf_set_depth_f32(fsdf_ctx* c, const float* depth, const double* pose, const double* range) {
  return set_depth_impl(c, depth, FSDF_DEPTH_F32, false, pose, range, "set_depth_f32");
}

extern "C" int fsdf_set_depth_u16(fsdf_ctx* c, const uint16_t* depth, const double* pose, const double* range) {
  return set_depth_impl(c, depth, FSDF_DEPTH_U16, false, pose, range, "set_depth_u16");
}

extern "C" int fsdf_set_depth_device(fsdf_ctx* c, const void* d_depth, int32_t format, const double* pose,
                                     const double* range) {
  return set_depth_impl(c, d_depth, format, true, pose, range, "set_depth_device");
}

extern "C" int fsdf_get_depth_pixels(fsdf_ctx* c, int32_t* pixels_out, int64_t* n_out) {
  if (!c) return FSDF_ERR_ARG;
  if (!c->depth_cloud)
    return fail(c, FSDF_ERR_STATE, "get_depth_pixels: the resident cloud did not come from a depth frame");
  if (n_out) *n_out = c->n;
  if (!pixels_out || c->n == 0) return FSDF_OK;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipMemcpyAsync(pixels_out, c->depth_pix.get(), (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}

// The next frame's cloud ahead of time: its host-to-device copy runs on a
// stream of the context's own while the current frame's passes run on the
// context stream (the copy engine beside the compute units), and
// fsdf_set_points_prefetched then makes it resident from the device copy —
// the per-frame ingest loses its host-link transfer (25 MB at 2^20 points).
// The copy overlaps only from page-locked host memory; the caller keeps xyz
// unchanged until fsdf_set_points_prefetched returns. A second prefetch
// replaces a pending one. fsdf_prefetch_points only records the cloud;
// prefetch_issue enqueues the copy and sort on the copy stream, from the next
// pass's launch (run_pass) or from fsdf_set_points_prefetched when no pass
// came between.
int prefetch_issue(fsdf_ctx* c) {
  c->prefetch_deferred = false;
  const double* xyz = c->prefetch_src;
  const int64_t n = c->prefetch_n;
  HIPCHECK(c, hipSetDevice(c->device));
  // (an earlier prefetch's copy may still write the buffer; a consumed one's
  // sort has finished: fsdf_set_points_prefetched returns after it)
  HIPCHECK(c, hipStreamSynchronize(c->copy_stream));
  if (n > 0) {
    HIPCHECK(c, c->prefetch.reserve((size_t)n * 3));
    HIPCHECK(c, hipMemcpyAsync(c->prefetch.get(), xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice,
                               c->copy_stream));
  }
  // the next resident cloud, Hilbert-sorted on the copy stream as well (its own
  // buffers and sort scratch: the current frame's cloud is untouched), so the
  // next frame's set_points_prefetched only swaps buffers
  c->prefetch_sorted = false;
  if (n > 0 && c->sort_points && n <= INT32_MAX) {
    const int64_t nc = ((n + 63) / 64 + 3) & ~(int64_t)3;  // (finish_resident's padding)
    ResidentCloud& nx = c->next;
    HIPCHECK(c, nx.pts.reserve((size_t)n * 3 * point_bytes(c)));
    HIPCHECK(c, nx.perm.reserve((size_t)n));
    HIPCHECK(c, nx.chunk_ws.reserve((size_t)nc * 4));
    hipError_t e = fsdf::sort_points_spatial(c->prefetch.get(), n, c->precision, nx.pts.get(), nx.perm.get(),
                                             c->sort_next, c->copy_stream);
    if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "prefetch_points (sort): %s", hipGetErrorString(e));
    HIPCHECK(c, fsdf::launch_chunk_spheres(c->precision, nx.pts.get(), n, nc, nx.chunk_ws.get(), c->copy_stream));
    c->prefetch_sorted = true;
  }
  HIPCHECK(c, hipEventRecord(c->ev_prefetch, c->copy_stream));
  return FSDF_OK;
}

extern "C" int fsdf_prefetch_points(fsdf_ctx* c, const double* xyz, int64_t n) {
  if (!c) return FSDF_ERR_ARG;
  if (n < 0 || (n > 0 && !xyz)) return fail(c, FSDF_ERR_ARG, "prefetch_points: bad buffer (n=%lld)", (long long)n);
  c->prefetch_src = xyz;
  c->prefetch_n = n;
  c->prefetch_deferred = true;
  c->prefetch_rc = FSDF_OK;
  return FSDF_OK;
}

extern "C" int fsdf_set_points_prefetched(fsdf_ctx* c) {
  if (!c) return FSDF_ERR_ARG;
  if (c->prefetch_n < 0) return fail(c, FSDF_ERR_STATE, "set_points_prefetched: no prefetch pending");
  const int64_t n = c->prefetch_n;
  int rc = c->prefetch_deferred ? prefetch_issue(c) : c->prefetch_rc;
  c->prefetch_n = -1;
  c->prefetch_rc = FSDF_OK;
  if (rc) return rc;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamWaitEvent(c->stream, c->ev_prefetch, 0));  // (the copy, and the sort when done there)
  if (!c->prefetch_sorted) return set_points_impl(c, c->prefetch.get(), n, true, 0, n);
  // the sorted next cloud becomes resident: the current frame's work is done
  // (synchronised), its buffers become the next prefetch's
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  rc = ensure_vox_box(c, c->prefetch.get(), n);  // (a first cloud: the seed box)
  if (rc) return rc;
  rc = carry_seeds_out(c);  // (the previous cloud, still resident)
  if (rc) return rc;
  c->n = 0;
  c->conf_set = c->conf_stale = false;  // (weights belong to the cloud that leaves)
  c->free_split = -1;                    // (and so does the split of its free-space samples)
  c->depth_cloud = false;                // (and so do a depth frame's pixel indices)
  c->voxel_cloud = false;                // (and a voxel cloud's lists)
  std::swap(c->cur, c->next);
  return finish_resident(c, n, false, true);
}

extern "C" int fsdf_set_points_range(fsdf_ctx* c, const double* xyz, int64_t n, int64_t begin, int64_t end) {
  return set_points_impl(c, xyz, n, false, begin, end, true);
}

extern "C" int fsdf_set_points_range_device(fsdf_ctx* c, const double* d_xyz, int64_t n, int64_t begin,
                                            int64_t end) {
  return set_points_impl(c, d_xyz, n, true, begin, end, true);
}

// Regroup the resident cloud by each point's nearest surface in the last pass
// (a stable device sort on PassOutputs::prior_out's bytes: the Hilbert order
// kept within each group), so that a chunk's points share their surface and
// the seeded passes evaluate fewer hulls per chunk. Per-point results do not
// change; sums change in rounding only (other chunks). Stream-ordered after
// the passes already queued.
extern "C" int fsdf_regroup_points(fsdf_ctx* c) {
  if (!c) return FSDF_ERR_ARG;
  if (c->n == 0) return FSDF_OK;
  if (!c->cur.perm.get())
    return fail(c, FSDF_ERR_STATE, "regroup_points: needs a sorted (sort_points) or ranged resident cloud");
  if (!c->prior_pass || c->prior.capacity() < (size_t)c->n)
    return fail(c, FSDF_ERR_STATE, "regroup_points: run a pass over the resident cloud first (hull-only scenes)");
  HIPCHECK(c, hipSetDevice(c->device));
  hipError_t e =
      fsdf::regroup_points(c->cur.pts, c->n, c->precision, c->cur.perm.get(), c->prior.get(), c->sort, c->stream);
  if (e != hipSuccess) return fail(c, FSDF_ERR_HIP, "regroup_points: %s", hipGetErrorString(e));
  const int64_t nc = ((c->n + 63) / 64 + 3) & ~(int64_t)3;
  HIPCHECK(c, fsdf::launch_chunk_spheres(c->precision, c->cur.pts.get(), c->n, nc, c->cur.chunk_ws.get(), c->stream));
  c->plan_nc = -1;  // other chunks: the next planned pass measures anew
  // the one-wave grid's heaviest-first block order: the next pass runs the
  // regrouped layout's order (the previous frame's) and rebuilds it from its
  // own costs — unordered, that pass took 163 us, with the Hilbert layout's
  // order 177, with the previous regrouped one 122 (M64 2^20, profiles/r06/regroup_order/)
  c->order_age[1] = kOrderEvery;
  c->regrouped = true;
  c->regroup_pending = false;
  c->conf_stale = c->conf_set;  // (another layout: the weights are regathered before the next robust launch)
  return FSDF_OK;
}

// The auto rule (FSDF_REGROUP_AUTO): regroup where the pass is bound by its
// summed work — the last resident pass ran one wave per chunk (the grid above
// the planned window) — and not where the planned pass or a hull-partitioned
// tier is bound by its heaviest chunk, which grouping makes heavier (2^17 step
// 0.0612 -> 0.0677 ms and worse). Needs a pass over the
// cloud (its k* are the groups) and a sorted or ranged cloud.
static bool regroup_wanted(const fsdf_ctx* c) {
  return c->n > 0 && c->cur.perm.get() && c->prior_pass && !c->regrouped && c->last_pass_shape == 1;
}

extern "C" int fsdf_regroup_auto(fsdf_ctx* c, int32_t* applied_out) {
  if (!c) return FSDF_ERR_ARG;
  if (applied_out) *applied_out = 0;
  if (!regroup_wanted(c)) return FSDF_OK;
  const int rc = fsdf_regroup_points(c);
  if (rc) return rc;
  if (applied_out) *applied_out = 1;
  return FSDF_OK;
}

extern "C" int fsdf_set_regroup(fsdf_ctx* c, int32_t mode) {
  if (!c) return FSDF_ERR_ARG;
  if (mode != FSDF_REGROUP_OFF && mode != FSDF_REGROUP_AUTO)
    return fail(c, FSDF_ERR_ARG, "set_regroup: unknown mode %d", mode);
  c->regroup_mode = mode;
  return FSDF_OK;
}
