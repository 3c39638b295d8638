// point_weights.hip — per-point confidence weights of the resident cloud
// (include/flashsdf.h "per-point confidence weights"): the side array a_i >= 0
// that the robust reduction (robust.hip, WEIGHTED) multiplies into every
// point's terms, and its life cycle next to the cloud.
//
// The context keeps the weights twice: conf_src in the caller's order (the
// order of the array the cloud was set from) and conf_res in resident order,
// res[i] = src[perm[i]] through the cloud's permutation (gather_f64_kernel). A
// cloud with no permutation reads conf_src directly. Whatever changes the
// layout of the resident cloud (fsdf_regroup_points, the auto regroup) only
// marks conf_res stale; point_weights_resident regathers it on the context
// stream ahead of the next robust launch — at most one gather per layout
// change. Whatever makes another cloud resident clears the weights
// (cloud.hip): a stale array never weighs a new frame.

#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "ctx.h"

namespace fsdf {

constexpr int kGatherBlock = 256;

__global__ __launch_bounds__(kGatherBlock) void gather_f64_kernel(const double* __restrict__ src,
                                                                  const int32_t* __restrict__ perm, int64_t n,
                                                                  double* __restrict__ res) {
  const int64_t i = (int64_t)blockIdx.x * kGatherBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t j = perm[i];
  res[i] = j >= 0 && j < n ? src[j] : 0.0;
}

hipError_t launch_gather_f64(const double* d_src, const int32_t* d_perm, int64_t n, double* d_res, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!d_src || !d_perm || !d_res) return hipErrorInvalidValue;
  const int64_t groups = (n + kGatherBlock - 1) / kGatherBlock;
  if (groups > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather_f64_kernel, dim3((unsigned)groups), dim3(kGatherBlock), 0, s, d_src, d_perm, n, d_res);
  return hipGetLastError();
}

}  // namespace fsdf

// The weights in resident order for a launch on the context stream: null when
// none are set. Both buffers were reserved when the weights were set (for this
// cloud's n): no reserve here, the pointers are read and used at once.
int point_weights_resident(fsdf_ctx* c, const double** d_conf_out) {
  *d_conf_out = nullptr;
  if (!c->conf_set) return FSDF_OK;
  const int32_t* d_perm = c->cur.perm.get();
  if (!d_perm) {  // (the resident order is the caller's)
    *d_conf_out = c->conf_src.get();
    return FSDF_OK;
  }
  if (c->conf_stale) {
    HIPCHECK(c, fsdf::launch_gather_f64(c->conf_src.get(), d_perm, c->n, c->conf_res.get(), c->stream));
    c->conf_stale = false;
  }
  *d_conf_out = c->conf_res.get();
  return FSDF_OK;
}

static int set_point_weights_impl(fsdf_ctx* c, const double* w, int64_t n, bool device_src, const char* who) {
  if (!c) return FSDF_ERR_ARG;
  if (!w) {  // clear: every point counts 1 again, on the unweighted code path
    c->conf_set = false;
    c->conf_stale = false;
    return FSDF_OK;
  }
  if (c->ranged)
    return fail(c, FSDF_ERR_STATE, "%s: weights serve a whole resident cloud (not a ranged or keyed one)", who);
  if (n != c->n)
    return fail(c, FSDF_ERR_ARG, "%s: %lld weights for a resident cloud of %lld points", who, (long long)n,
                (long long)c->n);
  if (!device_src)
    for (int64_t i = 0; i < n; ++i)
      if (!(w[i] >= 0.0) || !(w[i] <= 1.79769313486231570815e308))  // (a NaN fails the first test)
        return fail(c, FSDF_ERR_ARG, "%s: weight %lld is %g (weights are finite and >= 0); the earlier weights stay",
                    who, (long long)i, w[i]);
  HIPCHECK(c, hipSetDevice(c->device));
  const size_t cap = (size_t)std::max<int64_t>(n, 1);
  const bool perm = c->cur.perm.get() != nullptr;
  // (a robust launch still queued may read the buffers a growing reserve frees)
  if (c->conf_src.capacity() < cap || (perm && c->conf_res.capacity() < cap)) HIPCHECK(c, hipStreamSynchronize(c->stream));
  HIPCHECK(c, c->conf_src.reserve(cap));
  if (perm) HIPCHECK(c, c->conf_res.reserve(cap));
  if (n > 0)
    HIPCHECK(c, hipMemcpyAsync(c->conf_src.get(), w, (size_t)n * sizeof(double),
                               device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  c->conf_set = true;
  c->conf_stale = perm;
  // a host array: the caller may reuse it once this returns
  if (!device_src) HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}

extern "C" int fsdf_set_point_weights(fsdf_ctx* c, const double* weights, int64_t n) {
  return set_point_weights_impl(c, weights, n, false, "set_point_weights");
}

extern "C" int fsdf_set_point_weights_device(fsdf_ctx* c, const double* d_weights, int64_t n) {
  return set_point_weights_impl(c, d_weights, n, true, "set_point_weights_device");
}

extern "C" int fsdf_get_point_weights(fsdf_ctx* c, double* out, int32_t* set_out) {
  if (!c) return FSDF_ERR_ARG;
  if (set_out) *set_out = c->conf_set ? 1 : 0;
  if (!c->conf_set || !out || c->n == 0) return FSDF_OK;
  HIPCHECK(c, hipSetDevice(c->device));
  const double* d_conf = nullptr;
  const int rc = point_weights_resident(c, &d_conf);
  if (rc) return rc;
  HIPCHECK(c, hipMemcpyAsync(out, d_conf, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}
