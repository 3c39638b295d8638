// hull_sdf.h — one posed hull in the pass kernels: the model as the kernels
// see it, the LDS hull table with its culling bounds, the hull's LDS stage, the
// fp32 plane screen, the certified closest-feature walk, hull_sdf. Only
// sdf_kernels.hip includes it (through scene_eval.h).
#pragma once
#include "fsdf_internal.h"
#include "pose_impl.h"  // (I4)
#include "sdf_device_math.h"
#include "wave_times.h"

namespace fsdf {
// Posed model as the pass kernel sees it (device pointers, world frame).
template <typename T>
struct PassModel {
  int K;  // hulls
  int S;  // surfaces (hulls + RBF skins), the k* index space
  int R;  // RBF skins
  int stage_bytes;  // LDS stage per wave (bytes, multiple of 16)
  int planes64;     // f64 contexts: the fp64 planes are staged too (LocalModel::planes64)
  const int32_t* __restrict__ hull_surface;  // [K] surface index of hull h
  const int32_t* __restrict__ surface_kind;  // [S] FSDF_SURFACE_*
  const int32_t* __restrict__ rbf_surface;   // [R] surface index of RBF skin r
  const int32_t* __restrict__ rbf_row_off;   // [R+1] rows (n centres + 1 poly row)
  const int32_t* __restrict__ rbf_acc_off;   // [R+1] offsets in the RBF accumulator block
  const T* __restrict__ rbf_rows;            // [rows][4] (c, w) ... (a, b)
  const I4* __restrict__ face_rows;          // [F] packed local vertex / neighbour indices
  const T* __restrict__ planes;
  const T* __restrict__ verts;
  const I4* __restrict__ hull_rows;          // posed hull table, [K+1] HullRow (PosedModel::hull_rows)
  const float* __restrict__ screen;          // fp32 screening pairs (f64 contexts)
  const I4* __restrict__ image;              // per-hull stage images (planes64; PosedModel::image_w)
};

// Per-workgroup LDS hull table (HullRow: pose_impl.h), a copy of the posed
// table made once in the kernel prologue: the per-lane culling loops and every
// hull evaluation read it at LDS latency instead of a global round trip.

// Lower bound of hull k's signed distance at x from its oriented box (the hull
// lies inside the box): with u_i = |a_i·(x − c)| − e_i, outside the box
// d_k(x) >= |max(u, 0)| (distance to the box); inside, the hull's inner ball
// around x fits in the box, so d_k(x) >= max_i u_i. 1-Lipschitz in x. f32
// rounding (~1e-6 of |x|_1 + |c|_1 + the bound, |c|_1 <= |c_k|_1 + 3 r_k) is
// inside the culling margins. Returns max_i u_i and s = |max(u, 0)|^2: the
// bound is sqrt(s) when max_i u_i > 0, else max_i u_i.
__device__ __forceinline__ float box_bound(const HullRow& h, float x, float y, float z, float& s) {
  const F4 c = h.box[0];
  const float qx = x - c[0], qy = y - c[1], qz = z - c[2];
  float mx = -__builtin_huge_valf();
  s = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const F4 a = h.box[1 + i];
    const float u = fabsf(__builtin_fmaf(a[0], qx, __builtin_fmaf(a[1], qy, a[2] * qz))) - a[3];
    mx = fmaxf(mx, u);
    const float pu = fmaxf(u, 0.0f);
    s = __builtin_fmaf(pu, pu, s);
  }
  return mx;
}
// box lower bound <= t
__device__ __forceinline__ bool box_within(const HullRow& h, float x, float y, float z, float t) {
  float s;
  const float mx = box_bound(h, x, y, z, s);
  // (bitwise & throughout: short-circuit && on lane values becomes exec-mask
  // branches; every operand here is cheap and already loaded)
  return ((mx <= 0.0f) & (mx <= t)) | ((mx > 0.0f) & (t >= 0.0f) & (s <= t * t));
}
__device__ __forceinline__ float box_lower(const HullRow& h, float x, float y, float z) {
  float s;
  const float mx = box_bound(h, x, y, z, s);
  return mx <= 0.0f ? mx : __builtin_sqrtf(s);
}

// Lane need test of hull k at threshold tb = min(ub, best) + margin: hull k is
// needed unless |p-c_k| - r_k > tb (tested without a sqrt: |p-c_k|^2 <=
// (tb + r_k)^2) or its box bound exceeds tb.
__device__ __forceinline__ bool needs_at(const HullRow& h, float x, float y, float z, float tb) {
  const F4 sp = h.sphere;
  const float dx = x - sp[0], dy = y - sp[1], dz = z - sp[2];
  const float dist2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
  const float t = tb + sp[3];
  return (t >= 0.0f) & (dist2 <= t * t) & box_within(h, x, y, z, tb);
}

// Bounding sphere of the wave's points (f32, wave-uniform): every valid lane's
// point p satisfies |p - c| <= r up to f32 rounding (covered by the margins).
struct WaveSphere {
  float x, y, z, r;
};

// copy the posed table (whole workgroup: its (K+1) x 6 16-byte chunks; ends
// with a barrier) and return the culling-margin scale smax = max_k |c_k|_1 +
// 2 r_k, which the pose left in the sentinel row (wave-uniform)
template <typename T>
__device__ __forceinline__ float load_hull_table(const PassModel<T>& m, HullRow* __restrict__ ht) {
  I4* dst = (I4*)ht;
  const int nchunks = (m.K + 1) * (int)(sizeof(HullRow) / sizeof(I4));
  for (int c = threadIdx.x; c < nchunks; c += (int)blockDim.x) dst[c] = m.hull_rows[c];
  __syncthreads();
  return ht[m.K].box[0][3];  // (one LDS read per lane, the same address)
}

// One bulk copy of everything hull k's evaluation reads — plane rows, vertex
// rows, packed face rows — into this wave's LDS stage: every 16-byte chunk of
// the hull is loaded before any is stored, so the wave pays ONE global-memory
// latency per hull evaluation; all later reads (broadcast plane reads, per-lane
// triangle / neighbour / certificate reads) are LDS. Whole wave active.
constexpr int kPlaneBatch = FSDF_PLANE_BATCH;  // plane rows per LDS batch (power of 2, >= 2)
constexpr int kWalkSteps = 24;  // descent-walk cap before the exhaustive stage C

// Consecutive regions of 16-byte chunks: n0 from s0, n1 from s1, n2 from s2,
// n3 from s3.
__device__ __forceinline__ void stage_hull(void* __restrict__ lw, const I4* __restrict__ s0, int n0,
                                           const I4* __restrict__ s1, int n1, const I4* __restrict__ s2, int n2,
                                           const I4* __restrict__ s3 = nullptr, int n3 = 0) {
  const int P = n0, Q = P + n1, N3 = Q + n2, N = N3 + n3;
  const int lane = threadIdx.x & 63;
  I4* dst = (I4*)lw;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  for (int c0 = 0; c0 < N; c0 += 8 * 64) {
    I4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = min(c0 + 64 * j + lane, N - 1);
      const I4* src = c < P ? s0 + c : (c < Q ? s1 + (c - P) : (c < N3 ? s2 + (c - Q) : s3 + (c - N3)));
      v[j] = *src;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // lanes past the end hold chunk N-1 (clamped load) and store it there
      // again: same bits, and no exec-mask branch per store
      dst[min(c0 + 64 * j + lane, N - 1)] = v[j];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One contiguous region (a hull's stage image, PosedModel::image_w): the same
// one-latency bulk copy with no region selects.
__device__ __forceinline__ void stage_image(void* __restrict__ lw, const I4* __restrict__ src, int N) {
  const int lane = threadIdx.x & 63;
  I4* dst = (I4*)lw;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  for (int c0 = 0; c0 < N; c0 += 8 * 64) {
    I4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[min(c0 + 64 * j + lane, N - 1)];
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[min(c0 + 64 * j + lane, N - 1)] = v[j];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// packed face row: (i0 | i1<<16, i2 | n0<<16, n1 | n2<<16, 0) with i_j the
// hull-local vertex indices and n_e the hull-local face across edge e (i_e -> i_e+1)
// Decoded with one variable 64-bit shift, no selects: with a lane-divergent j
// the compiler turns a select chain into a switch, i.e. an exec-mask branch
// tree (~25 scalar instructions and 6 branches per decode in the fan walk).
__device__ __forceinline__ int fr_vert(const I4& r, int j) {
  const uint64_t w = ((uint64_t)(uint32_t)r[1] << 32) | (uint32_t)r[0];
  return (int)((w >> (16 * j)) & 0xffff);
}
__device__ __forceinline__ int fr_nbr(const I4& r, int e) {
  const uint64_t w = ((uint64_t)(uint32_t)r[2] << 32) | (uint32_t)r[1];
  return (int)((w >> (16 * e + 16)) & 0xffff);
}

// Local optimality certificate of q = the closest point of triangle f (in
// Voronoi region reg) to p: q is the closest point of the convex hull iff
// w = p − q lies in the hull's normal cone at q (exact characterisation):
//   edge u→v of f, shared with face g:  m_f·w <= 0 and m_g·w <= 0 (m the
//     in-plane inward edge normals; m·w is the edge value of p since q is on
//     the edge line);
//   vertex v:  w·(u − v) <= 0 for every neighbour u of v — the fan of faces
//     around v is walked through the packed neighbour rows (<= 32 steps).
// When the test fails it names the faces holding strictly closer points (a
// descent step): across the edge, g; at a vertex whose edge v→u is violated,
// the face g of that edge in the fan and the face across it (n1, n2; -1 =
// none; the current face f is never repeated). An interior point is
// certified iff p is above f's plane; a fan longer than 32 gives no
// certificate and no step. Tolerances accept rounding-level violations (a
// false certificate moves the answer by O(tol^2)). oracle/flash_oracle.c:
// cert_step mirrors every operation.
template <typename T, typename LP>
__device__ __forceinline__ bool cert_step(T px, T py, T pz, int f, int reg, const LP& lp,
                                          const typename Row4<T>::type* __restrict__ lv,
                                          const I4* __restrict__ lf, T scale, int& n1, int& n2,
                                          int* __restrict__ fan_it = nullptr) {
  typedef typename Row4<T>::type R;
  n1 = -1;
  n2 = -1;
  // interior of triangle f: q is p's projection on f's plane, optimal iff p is
  // on the outer side (the plane supports the hull)
  if (reg == 6) return plane_h<T>(lp[f], px, py, pz) > (T)0;
  const I4 fr = lf[f];
  if (reg >= 3) {
    const int e = reg - 3;
    const R U = lv[fr_vert(fr, e)], W = lv[fr_vert(fr, e + 1 - 3 * (e == 2))];
    const int g = fr_nbr(fr, e);
    const T sf = edge_value<T>(lp[f], U, W, px, py, pz);
    const T sg = edge_value<T>(lp[g], W, U, px, py, pz);
    // |m| = |W − U|: the tolerance is a lateral offset of eps (|p|_1 + scale)
    const T tol = cert_eps<T>() * (((fabs(px) + fabs(py)) + fabs(pz)) + scale) *
                  ((fabs(W[0] - U[0]) + fabs(W[1] - U[1])) + fabs(W[2] - U[2]));
    if (sf <= tol && sg <= tol) return true;
    if (sg > tol && g != f) n1 = g;
    return false;
  }
  const int v = fr_vert(fr, reg);
  const R V = lv[v];
  const T wx = px - V[0], wy = py - V[1], wz = pz - V[2];
  const T tol = cert_eps<T>() * ((fabs(wx) + fabs(wy)) + fabs(wz)) * scale;
  int g = f, j = reg;
  I4 r = fr;
  for (int it = 0; it < 32; ++it) {
    if (fan_it) *fan_it = it + 1;
    const int g2 = fr_nbr(r, j);  // across edge v -> u
    const R Un = lv[fr_vert(r, j + 1 - 3 * (j == 2))];
    const T dot = mfma_(wx, Un[0] - V[0], mfma_(wy, Un[1] - V[1], wz * (Un[2] - V[2])));
    if (dot > tol) {
      n1 = g != f ? g : g2;
      n2 = g != f && g2 != f ? g2 : -1;
      return false;
    }
    if (g2 == f) return true;
    r = lf[g2];
    j = 2 - (fr_vert(r, 1) == v) - 2 * (fr_vert(r, 0) == v);  // (the row's vertices are distinct)
    g = g2;
  }
  return false;
}

// ---------------------------------------------------------------------------
// fp32-screened plane max (f64 contexts): the exact first-index argmax of the
// fp64 plane values h_f = n_f·p − d_f, from an fp32 pass over all faces plus
// an fp64 pass over ONE batch of 8.
//   Screen: h'_f = n'·q − d'' in packed fp32 (v_pk_fma_f32: two faces per
//   instruction, plane pairs staged in LDS and read with ds_read_b128),
//   q = fl32(p − c),
//   c the hull's sphere centre, with |h'_f − h_f| <= E = 16u (|q|_1 + r)
//   (u = 2^-24; |n_i| <= 1 and |d − n·c| <= r). Per batch of 8 faces the
//   maximum b; b1 = best batch maximum, b2 = best over the other batches.
//   If b2 < b1 − 2E, every face g outside the best batch has
//   h_g <= b2 + E < b1 − E <= max h over the batch: the exact maximum lies in
//   the best batch only, and its first-index argmax over the batch's 8 faces
//   (fp64, the same plane_h arithmetic) IS the first-index argmax over all
//   faces — bit for bit the full fp64 scan (the oracle's). Lanes without that
//   margin (near-ties across batches) return false and take the full scan.
// Returns true iff the result is final for every lane that needs it.
// ---------------------------------------------------------------------------
template <typename T>
constexpr bool kStagePairs = sizeof(T) == 8;  // (see hull_sdf; fsdf_set_surfaces sizes the stage to match)
constexpr int kScreenIlp = FSDF_SCREEN_ILP;  // independent 8-face batches per loop iteration
typedef float F2v __attribute__((ext_vector_type(2)));

template <typename T, typename LP>
__device__ __forceinline__ bool screen_plane_max(T px, T py, T pz, int k, int f0, int nf, const PassModel<T>& m,
                                                 const HullRow* __restrict__ ht, const void* __restrict__ lw,
                                                 const LP& lp, bool active,
                                                 T bound, T& hA, int& iA, bool& rejected) {
  const F4 sp = ht[k].sphere;
  const float qx = (float)(px - (T)sp[0]), qy = (float)(py - (T)sp[1]), qz = (float)(pz - (T)sp[2]);
  // 2E, plus an absolute term for the fp64 rounding of h_f itself (~1e-15 |p|)
  const float E2 = 32.0f * 5.9604645e-8f * (((fabsf(qx) + fabsf(qy)) + fabsf(qz)) + sp[3]) * 1.0001f +
                   1e-12f * (1.0f + fabsf((float)px) + fabsf((float)py) + fabsf((float)pz) + sp[3]);
  const F2v qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
  const F4* ls = (const F4*)lw;  // staged pairs: two 16-byte chunks each
  const int np = (nf + 1) >> 1;
  float b1 = -__builtin_huge_valf(), b2 = -__builtin_huge_valf();
  int ib = 0;
  // maximum of the 8 faces in pairs i..i+3 (tail: indices clamped to the last pair)
  auto batch_max = [&](int i, bool tail) -> float {
    F4 c[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = tail ? min(i + q, np - 1) : i + q;
      c[2 * q] = ls[2 * j];
      c[2 * q + 1] = ls[2 * j + 1];
    }
    float hm[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const F4 u = c[2 * q], w = c[2 * q + 1];
      const F2v nx = {u[0], u[1]}, ny = {u[2], u[3]}, nz = {w[0], w[1]}, nd = {w[2], w[3]};
      const F2v h = __builtin_elementwise_fma(nx, qx2, __builtin_elementwise_fma(ny, qy2, __builtin_elementwise_fma(nz, qz2, nd)));
      hm[q] = fmaxf(h[0], h[1]);
    }
    return fmaxf(fmaxf(hm[0], hm[1]), fmaxf(hm[2], hm[3]));
  };
  auto update = [&](float mb, int i) {
    b2 = fmaxf(b2, fminf(b1, mb));
    if (mb > b1) { b1 = mb; ib = i; }
  };
  // Early rejection: h_max >= b1 − E, so once b1 − E exceeds a lane's best
  // distance the hull can neither win nor tie for it (d >= h_max). When that
  // holds for every lane that needs the hull, the scan stops (d = +inf).
  const float bf = (float)bound;
  const float thr = bf + E2 + 2.5e-7f * fabsf(bf);
  const uint64_t tw_screen = wt_now();
  rejected = false;
  int i0 = 0;
  // the first 16 faces get a rejection test of their own: a hull that cannot
  // win is usually exposed by its first planes (3 % faster than waiting for
  // the first 32-face round)
  if (np >= 8) {
    const float a = batch_max(0, false), b = batch_max(4, false);
    update(a, 0);
    update(b, 4);
    i0 = 8;
    if (!__any(active && !(b1 > thr))) { rejected = true; return true; }
  }
  // kScreenIlp independent batches per iteration; rejection tested once per round
  for (; i0 + 4 * kScreenIlp <= np; i0 += 4 * kScreenIlp) {
    float mx[kScreenIlp];
#pragma unroll
    for (int u = 0; u < kScreenIlp; ++u) mx[u] = batch_max(i0 + 4 * u, false);
#pragma unroll
    for (int u = 0; u < kScreenIlp; ++u) update(mx[u], i0 + 4 * u);
    if (!__any(active && !(b1 > thr))) { rejected = true; return true; }
  }
  for (; i0 < np; i0 += 4) update(batch_max(i0, i0 + 4 > np), i0);
  if (!__any(active && !(b1 > thr))) { rejected = true; return true; }
  // exact fp64 first-index argmax over the best batch's faces
  const uint64_t tw_fix = wt_add2(4, tw_screen);
  const int fb = 2 * ib;
  hA = -tinf<T>();
  iA = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int f = min(fb + q, nf - 1);
    const T h = plane_h<T>(lp[f], px, py, pz);
    if (h > hA) { hA = h; iA = f; }
  }
  const bool safe = b2 < b1 - E2;
  wt_add2(5, tw_fix);
  return !__any(active && !safe);
}

// ---------------------------------------------------------------------------
// Exact signed distance of p to posed hull k, with its unit gradient.
//   inside / on the surface: max_f h_f, gradient n_{f*} (first max face; f64
//     contexts find it with the fp32 screen above);
//   outside: if the projection on f* lies in triangle f*, d = h_{f*};
//     otherwise the closest point on triangle f* and a descent walk certified
//     by the hull's normal cone at the closest feature (cert_step); a stalled
//     walk falls back to the exhaustive scan of the visible faces.
// `active`: this lane's result is used (gates the wave-uniform slow branches).
// `bound`: the lane's best distance so far (only a result below it matters).
// `lw`: this wave's LDS stage (m.stage_bytes). Whole wave active.
// ---------------------------------------------------------------------------
template <typename T, bool P64 = false>
__device__ __forceinline__ void hull_sdf(T px, T py, T pz, int k, const PassModel<T>& m,
                                         const HullRow* __restrict__ ht, bool active, T bound,
                                         T& d, T& gx, T& gy, T& gz, T* __restrict__ lw,
                                         unsigned long long* __restrict__ stats) {
  typedef typename Row4<T>::type R;
  const int f0 = __builtin_amdgcn_readfirstlane(ht[k].f0);
  const int nf = __builtin_amdgcn_readfirstlane(ht[k + 1].f0) - f0;
  const int v0 = __builtin_amdgcn_readfirstlane(ht[k].v0);
  const int nv = __builtin_amdgcn_readfirstlane(ht[k + 1].v0) - v0;
  uint64_t tw = wt_now();
#if FSDF_WAVE_TIMES
  fsdf_wt_slow[threadIdx.x] = false;
#endif
  // Stage layout: f64 contexts stage the fp32 screening pairs (16 B per face)
  // and read the fp64 planes — needed per lane only for the batch fix-up, the
  // max face and the certificates — from global memory (L1/L2); f32 contexts
  // stage the planes themselves. Then vertex rows and packed face rows.
  constexpr int cpr = (int)sizeof(T) / 4;  // 16-byte chunks per row of 4 T
  const int np2 = kStagePairs<T> ? 2 * ((nf + 1) >> 1) : nf * cpr;  // chunks of region 0
  const I4* src0 = kStagePairs<T> ? (const I4*)(m.screen + 4 * (f0 + k)) : (const I4*)(m.planes + 4 * f0);
  // f64 contexts also stage the fp64 planes (after the pairs) in the
  // one-chunk-per-wave pass (P64: pass_kernel ALIAS, LocalModel::planes64)
  constexpr bool kP64 = kStagePairs<T> && P64;
  const int npl = kP64 ? nf * cpr : 0;
  // (P64: the hull's stage image, whose pair region is nf + 1 chunks)
  const int npr = kP64 ? nf + 1 : np2;
  if constexpr (kP64) {
    stage_image(lw, m.image + (4 * f0 + k + 2 * v0), npr + npl + nv * cpr + nf);
  } else {
    stage_hull(lw, src0, np2, (const I4*)(m.planes + 4 * f0), npl, (const I4*)(m.verts + 4 * v0), nv * cpr,
               m.face_rows + f0, nf);
  }
  tw = wt_add(0, tw);
  const R* lp = kP64 ? (const R*)((const I4*)lw + npr) : (kStagePairs<T> ? (const R*)(m.planes + 4 * f0) : (const R*)lw);
  const R* lv = (const R*)((const I4*)lw + npr + npl);
  const I4* lf = (const I4*)(lv + nv);
  const T scale = (T)ht[k].hscale;
  auto uplane = [&](int f) -> R { return lp[f]; };
  // two independent running maxima (even / odd faces) shorten the serial
  // compare chain; merged with the first-index rule, identical to one chain
  // Batches of kPlaneBatch rows, all of a batch's LDS reads issued before the
  // first is consumed. The loop keeps only the exact maximum (a v_max tree per
  // batch) and the first batch that strictly raised it; the first face of that
  // batch equal to the maximum is then found by re-evaluating the batch (same
  // operations, same bits) — the first-index argmax over all faces. Missing
  // rows of the last batch repeat the last face (same value, never first).
  T hA = -tinf<T>();
  int iA = 0;
  bool screened = false;
  if constexpr (sizeof(T) == 8) {
    bool rejected = false;
    screened = screen_plane_max(px, py, pz, k, f0, nf, m, ht, lw, lp, active, bound, hA, iA, rejected);
    if (count_events(stats) && lane_id() == 0) {
      if (rejected) atomicAdd(stats + 20, 1ull);
      else if (!screened) atomicAdd(stats + 19, 1ull);
    }
    if (rejected) wt_count(1, 1);
    else if (!screened) wt_count(7, 1);
    if (rejected) {  // cannot win nor tie for any lane that needs it
      d = tinf<T>();
      gx = gy = gz = (T)0;
      wt_add(1, tw);
      return;
    }
  }
  if (!screened) {
  hA = -tinf<T>();
  int ib = 0;
  auto batch = [&](int i, bool tail) {
    R c[kPlaneBatch];
#pragma unroll
    for (int q = 0; q < kPlaneBatch; ++q) c[q] = uplane(tail ? min(i + q, nf - 1) : i + q);
    T h[kPlaneBatch];
#pragma unroll
    for (int q = 0; q < kPlaneBatch; ++q) h[q] = plane_h<T>(c[q], px, py, pz);
#pragma unroll
    for (int w = 1; w < kPlaneBatch; w *= 2)
#pragma unroll
      for (int q = 0; q + w < kPlaneBatch; q += 2 * w) h[q] = __builtin_fmax(h[q], h[q + w]);
    if (h[0] > hA) { hA = h[0]; ib = i; }
  };
  int i0 = 0;
  for (; i0 + kPlaneBatch <= nf; i0 += kPlaneBatch) batch(i0, false);  // one base address, immediate offsets
  if (i0 < nf) batch(i0, true);
  // faces before batch ib are all < hA, so the window may start earlier
  const int fb = nf >= kPlaneBatch ? min(ib, nf - kPlaneBatch) : ib;
  iA = min(fb + kPlaneBatch - 1, nf - 1);
#pragma unroll
  for (int q = kPlaneBatch - 1; q >= 0; --q) {
    const int f = nf >= kPlaneBatch ? fb + q : min(fb + q, nf - 1);
    if (plane_h<T>(lp[f], px, py, pz) == hA) iA = f;
  }
  }
  tw = wt_add(1, tw);
  if (count_events(stats) && lane_id() == 0) {
    atomicAdd(stats + 9, (unsigned long long)nf);
  }
  const T hmax = hA;
  const int fs = iA;  // hull-local
  const R ns = lp[fs];
  d = hmax;
  gx = ns[0]; gy = ns[1]; gz = ns[2];
  bool slow = false;
  T s0 = (T)0, s1 = (T)0, s2 = (T)0;
  if (hmax > (T)0) {
    // Fast path: the projection of p on the max-violated face lies inside that
    // triangle => it is the closest point and the distance equals hmax.
    const I4 fr = lf[fs];
    const R a = lv[fr_vert(fr, 0)], b = lv[fr_vert(fr, 1)], c = lv[fr_vert(fr, 2)];
    s0 = edge_value<T>(ns, a, b, px, py, pz);
    s1 = edge_value<T>(ns, b, c, px, py, pz);
    s2 = edge_value<T>(ns, c, a, px, py, pz);
    slow = !(s0 >= (T)0 && s1 >= (T)0 && s2 >= (T)0);
  }
  // hmax is a lower bound of the distance: when it exceeds the lane's best so
  // far by more than the rounding of either value, hull k cannot win (nor tie)
  // and its exact distance is not needed — d stays hmax (> bound).
  const T lb_margin = (T)16 * cert_eps<T>() * (scale + ((fabs(px) + fabs(py)) + fabs(pz)));
#if FSDF_WAVE_TIMES
  wt_count(10, __builtin_popcountll(__ballot(slow && active && (hmax - lb_margin > bound))));
#endif
  slow = slow && active && !(hmax - lb_margin > bound);
  const uint64_t slow_mask = __ballot(slow);
#if FSDF_WAVE_TIMES
  wt_count(8, __builtin_popcountll(slow_mask));
  fsdf_wt_slow[threadIdx.x] = slow;
#endif
  tw = wt_add(2, tw);
  if (!slow_mask) return;
  wt_count(2, 1);
  if (count_events(stats) && (threadIdx.x & 63) == 0) {
    atomicAdd(stats + 2, 1ull);
    atomicAdd(stats + 4, (unsigned long long)__builtin_popcountll(slow_mask));
  }
  // stage A: closest point on triangle f*, certified by the normal cone at
  // its Voronoi feature
  const I4 frs = lf[fs];
  T qx, qy, qz;
  int rA;
  closest_on_triangle<T>(px, py, pz, lv[fr_vert(frs, 0)], lv[fr_vert(frs, 1)], lv[fr_vert(frs, 2)], qx, qy, qz, rA);
  T ex = px - qx, ey = py - qy, ez = pz - qz;
  T best2 = mfma_(ex, ex, mfma_(ey, ey, ez * ez));
  // stage B: descent walk — certify the current point; on failure move to the
  // face(s) the certificate names (each accepted step strictly lowers the
  // distance, so the walk cannot cycle); lanes that stall or exceed the step
  // cap keep `todo` for the exhaustive stage C.
  bool todo = slow;
  int cf = fs, cr = rA;
  bool walking = todo;
  const uint64_t tw_walk = wt_now();
  for (int step = 0; step < kWalkSteps && __any(walking); ++step) {
    if (count_events(stats) && lane_id() == 0) atomicAdd(stats + 21, 1ull);
    wt_count(3, 1);
#if FSDF_WAVE_TIMES
    const uint64_t tw_c = wt_now();
    int fan_it = 0;
    wt_count2(2, __builtin_popcountll(__ballot(walking && cr <= 2)));
    wt_count2(6, __builtin_popcountll(__ballot(walking && cr >= 3 && cr <= 5)));
    wt_count2(7, __builtin_popcountll(__ballot(walking && cr == 6)));
    int* fan_p = &fan_it;
#else
    int* fan_p = nullptr;
#endif
    int n1 = -1, n2 = -1;
    const bool certified = walking && cert_step<T>(px, py, pz, cf, cr, lp, lv, lf, scale, n1, n2, fan_p);
#if FSDF_WAVE_TIMES
    {
      int fm = fan_it;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) fm = max(fm, __shfl_xor(fm, off, 64));
      wt_count2(3, fm);
    }
    const uint64_t tw_s = wt_add2(0, tw_c);
#endif
    if (walking) {
      if (certified) {
        todo = false;
        walking = false;
      } else {
        bool moved = false;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int g = t == 0 ? n1 : n2;
          if (g >= 0) {
            const I4 gr = lf[g];
            T cx, cy, cz;
            int rg;
            closest_on_triangle<T>(px, py, pz, lv[fr_vert(gr, 0)], lv[fr_vert(gr, 1)], lv[fr_vert(gr, 2)], cx, cy, cz,
                                   rg);
            const T dx = px - cx, dy = py - cy, dz = pz - cz;
            const T d2 = mfma_(dx, dx, mfma_(dy, dy, dz * dz));
            if (d2 < best2) { best2 = d2; qx = cx; qy = cy; qz = cz; cf = g; cr = rg; moved = true; }
          }
        }
        walking = moved;
      }
    }
#if FSDF_WAVE_TIMES
    wt_add2(1, tw_s);
#endif
  }
  wt_add(7, tw_walk);  // (the descent walk: certificates and steps)
  if (__any(todo)) {
    if (count_events(stats) && (threadIdx.x & 63) == 0) atomicAdd(stats + 6, 1ull);
    const uint64_t scan_mask = __ballot(todo);
    if (scan_mask) {
      // stage C: exhaustive scan of the visible faces (the closest boundary
      // point of a convex polytope lies on one of them); a face whose plane
      // distance already exceeds the best distance cannot improve it.
      if (count_events(stats) && (threadIdx.x & 63) == 0) atomicAdd(stats + 7, (unsigned long long)__builtin_popcountll(scan_mask));
      // starts from the stage-B point (strict < keeps it on ties): with b2
      // already near the optimum, the plane-distance test h^2 < b2 leaves only
      // the few faces around the closest feature for closest_on_triangle
      T b2 = best2;
      T bx = qx, by = qy, bz = qz;
      // Per chunk of 64 faces: a wave-uniform pass marks, per lane, the faces
      // that pass the test against the stage-B distance (broadcast plane rows,
      // no branches); then each lane walks its own marks in index order,
      // re-testing against its current b2 — the oracle's sequential scan,
      // without running closest_on_triangle for faces no lane needs.
      for (int c0 = 0; c0 < nf; c0 += 64) {
        const int cn = min(64, nf - c0);
        uint64_t mark = 0;
        for (int j = 0; j < cn; ++j) {
          const T h = plane_h<T>(uplane(c0 + j), px, py, pz);
          if (h > (T)0 && h * h < b2) mark |= 1ull << j;
        }
        if (!todo) mark = 0;
        while (mark) {
          const int ff = c0 + __builtin_ctzll(mark);
          mark &= mark - 1;
          const T h = plane_h<T>(lp[ff], px, py, pz);
          if (h * h < b2) {
            const I4 gr = lf[ff];
            T cx, cy, cz;
            int rg;
            closest_on_triangle<T>(px, py, pz, lv[fr_vert(gr, 0)], lv[fr_vert(gr, 1)], lv[fr_vert(gr, 2)], cx, cy,
                                   cz, rg);
            const T dx = px - cx, dy = py - cy, dz = pz - cz;
            const T d2 = mfma_(dx, dx, mfma_(dy, dy, dz * dz));
            if (d2 < b2) { b2 = d2; bx = cx; by = cy; bz = cz; }
          }
        }
      }
      if (todo) { best2 = b2; qx = bx; qy = by; qz = bz; }
    }
  }
  wt_add(3, tw);
  if (slow) {
    if (best2 > (T)0) {
      d = tsqrt(best2);
      const T inv = (T)1 / d;
      gx = (px - qx) * inv; gy = (py - qy) * inv; gz = (pz - qz) * inv;
    } else {
      // p on the boundary (a vertex/edge): d = 0, subgradient = face normal
      d = (T)0;
    }
  }
}

}  // namespace fsdf
