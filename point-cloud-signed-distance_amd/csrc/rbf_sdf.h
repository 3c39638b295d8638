// rbf_sdf.h — RBF interpolating skins in the pass kernels: the field, the
// skin's signed distance, the adjoint sums of the lanes nearest to a skin.
// sdf_kernels.hip includes it (through scene_eval.h), skin_moments.hip for
// the field's types and rbf_skin_from_field, and robust_skin.hip for
// rbf_adjoint with a robust factor in place of 2s.
#pragma once
#include "sdf_device_math.h"

namespace fsdf {
// Row-chunked per-wave LDS staging (RBF centre rows). Must be called with
// every lane of the wave active (wave-uniform control flow).
template <typename T>
__device__ __forceinline__ void stage_rows(T* __restrict__ lds, const T* __restrict__ src, int rows) {
  typedef typename Row4<T>::type R;
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // prior reads of this stage precede the overwrite
  for (int r = lane; r < rows; r += 64) *(R*)(lds + 4 * r) = *(const R*)(src + 4 * r);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------
// RBF interpolating skin (src/Flash.jl:207-213; SpatialFields XCubed + affine):
//   f(x) = Σ w_i |x-c_i|^3 + a + b·x,   s = f/|∇f|,
//   ∇s = ∇f/|∇f| − f (H ∇f)/|∇f|^3      (H = Hessian of f).
// Centre rows are LDS-staged per wave (call with the whole wave active).
// ---------------------------------------------------------------------------
template <typename T>
struct RbfField {
  T f, gx, gy, gz, hxx, hyy, hzz, hxy, hxz, hyz;
};

template <typename T>
__device__ __forceinline__ void rbf_field(T px, T py, T pz, const T* __restrict__ rows, int nc,
                                          T* __restrict__ lw, int cap, RbfField<T>& F) {
  typedef typename Row4<T>::type R4;
  const R4 poly = *(const R4*)(rows + 4 * nc);
  F.f = mfma_(poly[1], px, mfma_(poly[2], py, mfma_(poly[3], pz, poly[0])));
  F.gx = poly[1]; F.gy = poly[2]; F.gz = poly[3];
  F.hxx = F.hyy = F.hzz = F.hxy = F.hxz = F.hyz = (T)0;
  for (int c0 = 0; c0 < nc; c0 += cap) {
    const int cn = min(cap, nc - c0);
    stage_rows(lw, rows + 4 * c0, cn);
    for (int i = 0; i < cn; ++i) {
      const R4 c = *(const R4*)(lw + 4 * i);
      const T dx = px - c[0], dy = py - c[1], dz = pz - c[2];
      const T r2 = mfma_(dx, dx, mfma_(dy, dy, dz * dz));
      const T r = tsqrt(r2);
      const T wr = c[3] * r;
      F.f = mfma_(wr, r2, F.f);
      const T t3 = (T)3 * wr;
      F.gx = mfma_(t3, dx, F.gx); F.gy = mfma_(t3, dy, F.gy); F.gz = mfma_(t3, dz, F.gz);
      const T hq = r2 > (T)0 ? ((T)3 * c[3]) / r : (T)0;
      F.hxx = mfma_(hq * dx, dx, F.hxx + t3);
      F.hyy = mfma_(hq * dy, dy, F.hyy + t3);
      F.hzz = mfma_(hq * dz, dz, F.hzz + t3);
      F.hxy = mfma_(hq * dx, dy, F.hxy);
      F.hxz = mfma_(hq * dx, dz, F.hxz);
      F.hyz = mfma_(hq * dy, dz, F.hyz);
    }
  }
}

// s and ∇s from the field; also returns c = f/|∇f|^3 and 1/|∇f| for the adjoint.
template <typename T>
__device__ __forceinline__ void rbf_skin_from_field(const RbfField<T>& F, T& s, T& gx, T& gy, T& gz, T& c,
                                                    T& invG) {
  const T G2 = mfma_(F.gx, F.gx, mfma_(F.gy, F.gy, F.gz * F.gz));
  const T G = tsqrt(G2);
  s = F.f / G;
  invG = (T)1 / G;
  c = F.f / (G2 * G);
  const T hgx = mfma_(F.hxx, F.gx, mfma_(F.hxy, F.gy, F.hxz * F.gz));
  const T hgy = mfma_(F.hxy, F.gx, mfma_(F.hyy, F.gy, F.hyz * F.gz));
  const T hgz = mfma_(F.hxz, F.gx, mfma_(F.hyz, F.gy, F.hzz * F.gz));
  gx = mfma_(-c, hgx, F.gx * invG);
  gy = mfma_(-c, hgy, F.gy * invG);
  gz = mfma_(-c, hgz, F.gz * invG);
}

// Adjoint contributions of the lanes whose nearest surface is RBF skin r
// (sel): per centre λ_w_i = Σ 2s ∂s/∂w_i and E_i = Σ 2s ∂s/∂c_i (coefficients
// fixed), then λ_a, λ_b — wave-summed, added by lane 0 into acc (LDS):
//   acc[0..n) = λ_w, acc[n] = λ_a, acc[n+1..n+4) = λ_b, acc[n+4+3i..] = E_i.
// SCALED (robust_skin.hip): the lane's `scale` stands where 2s does — the
// robust factor 2 (aw d*) of a weighted or robust objective; the pass's own
// instantiation (SCALED = false) never reads it.
template <typename T, bool SCALED = false>
__device__ __forceinline__ void rbf_adjoint(T px, T py, T pz, const T* __restrict__ rows, int nc,
                                            T* __restrict__ lw, int cap, bool sel, double* __restrict__ acc,
                                            T scale = (T)0) {
  typedef typename Row4<T>::type R4;
  RbfField<T> F;
  rbf_field(px, py, pz, rows, nc, lw, cap, F);
  T s, sgx, sgy, sgz, c, invG;
  rbf_skin_from_field(F, s, sgx, sgy, sgz, c, invG);
  const T two_s = SCALED ? scale : (T)2 * s;
  const T dsdf = invG;
  const T ux = -c * F.gx, uy = -c * F.gy, uz = -c * F.gz;  // ∂s/∂∇f
  const int lane = threadIdx.x & 63;
  for (int c0 = 0; c0 < nc; c0 += cap) {
    const int cn = min(cap, nc - c0);
    stage_rows(lw, rows + 4 * c0, cn);
    for (int i = 0; i < cn; ++i) {
      const R4 cw = *(const R4*)(lw + 4 * i);
      const T dx = px - cw[0], dy = py - cw[1], dz = pz - cw[2];
      const T r2 = mfma_(dx, dx, mfma_(dy, dy, dz * dz));
      const T r = tsqrt(r2);
      const T e = mfma_(dx, ux, mfma_(dy, uy, dz * uz));
      const T lam = two_s * mfma_(dsdf * r2, r, (T)3 * r * e);
      const T k1 = mfma_((T)3 * r, dsdf, r2 > (T)0 ? ((T)3 * e) / r : (T)0);
      const T k2 = (T)3 * r;
      const T sc = -two_s * cw[3];
      double v[4] = {(double)lam, (double)(sc * mfma_(k1, dx, k2 * ux)), (double)(sc * mfma_(k1, dy, k2 * uy)),
                     (double)(sc * mfma_(k1, dz, k2 * uz))};
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = wave_sum(sel ? v[j] : 0.0);
      if (lane == 0) {
        acc[c0 + i] += v[0];
        double* E = acc + nc + 4 + 3 * (c0 + i);
        E[0] += v[1]; E[1] += v[2]; E[2] += v[3];
      }
    }
  }
  double w[4] = {(double)(two_s * dsdf), (double)(two_s * mfma_(dsdf, px, ux)),
                 (double)(two_s * mfma_(dsdf, py, uy)), (double)(two_s * mfma_(dsdf, pz, uz))};
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = wave_sum(sel ? w[j] : 0.0);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[nc + j] += w[j];
  }
}

}  // namespace fsdf
