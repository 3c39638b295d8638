// sdf_device_math.h — device arithmetic the kernels share: fma / sqrt /
// infinity by precision, the triangle and plane primitives, the DPP wave
// reductions. Only sdf_kernels.hip includes it (through its other headers).
#pragma once
#include <hip/hip_runtime.h>

namespace fsdf {
template <typename T> __device__ __forceinline__ T mfma_(T a, T b, T c);
template <> __device__ __forceinline__ double mfma_(double a, double b, double c) {
  return __builtin_fma(a, b, c);
}
template <> __device__ __forceinline__ float mfma_(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}
template <typename T> __device__ __forceinline__ T tsqrt(T a);
template <> __device__ __forceinline__ double tsqrt(double a) { return __builtin_sqrt(a); }
template <> __device__ __forceinline__ float tsqrt(float a) { return __builtin_sqrtf(a); }
template <typename T> __device__ __forceinline__ T tinf();
template <> __device__ __forceinline__ double tinf() { return __builtin_huge_val(); }
template <> __device__ __forceinline__ float tinf() { return __builtin_huge_valf(); }

// ---------------------------------------------------------------------------
// Closest point on triangle (a, b, c) to p — Voronoi-region walk.
// ---------------------------------------------------------------------------
template <typename T> struct Row4 { typedef T __attribute__((ext_vector_type(4))) type; };
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// reg: the Voronoi region of the result — 0, 1, 2 vertex a, b, c; 3, 4, 5 the
// edge a→b, b→c, c→a (face edges 0, 1, 2); 6 the interior.
// Branch-free: every region test is evaluated, the first that holds (the
// classic early-return order) selects the region, and the region's one
// division (edge parameter, or the interior's 1/(va+vb+vc)) runs once — a
// wave whose lanes sit in different regions no longer executes every
// region's division in turn. Each region's result is the same expression as
// in the early-return form (oracle/flash_oracle.c), so the bits are too.
template <typename T>
__device__ __forceinline__ void closest_on_triangle(T px, T py, T pz, const typename Row4<T>::type& A,
                                                    const typename Row4<T>::type& B,
                                                    const typename Row4<T>::type& C, T& qx, T& qy, T& qz,
                                                    int& reg) {
  const T ax = A[0], ay = A[1], az = A[2];
  const T bx = B[0], by = B[1], bz = B[2];
  const T cx = C[0], cy = C[1], cz = C[2];
  const T abx = bx - ax, aby = by - ay, abz = bz - az;
  const T acx = cx - ax, acy = cy - ay, acz = cz - az;
  const T apx = px - ax, apy = py - ay, apz = pz - az;
  const T d1 = mfma_(abx, apx, mfma_(aby, apy, abz * apz));
  const T d2 = mfma_(acx, apx, mfma_(acy, apy, acz * apz));
  const T bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const T d3 = mfma_(abx, bpx, mfma_(aby, bpy, abz * bpz));
  const T d4 = mfma_(acx, bpx, mfma_(acy, bpy, acz * bpz));
  const T vc = mfma_(d1, d4, -(d3 * d2));
  const T cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const T d5 = mfma_(abx, cpx, mfma_(aby, cpy, abz * cpz));
  const T d6 = mfma_(acx, cpx, mfma_(acy, cpy, acz * cpz));
  const T vb = mfma_(d5, d2, -(d1 * d6));
  const T va = mfma_(d3, d6, -(d5 * d4));
  const T e43 = d4 - d3, e56 = d5 - d6;
  const bool c0 = d1 <= (T)0 && d2 <= (T)0;
  const bool c1 = d3 >= (T)0 && d4 <= d3;
  const bool c3 = vc <= (T)0 && d1 >= (T)0 && d3 <= (T)0;
  const bool c2 = d6 >= (T)0 && d5 <= d6;
  const bool c5 = vb <= (T)0 && d2 >= (T)0 && d6 <= (T)0;
  const bool c4 = va <= (T)0 && e43 >= (T)0 && e56 >= (T)0;
  reg = c0 ? 0 : (c1 ? 1 : (c3 ? 3 : (c2 ? 2 : (c5 ? 5 : (c4 ? 4 : 6)))));
  // the region's quotient: edge a→b t = d1/(d1−d3), c→a t = d2/(d2−d6),
  // b→c t = e43/(e43+e56), interior inv = 1/(va+vb+vc); vertices none
  T num = (T)1, den = (va + vb) + vc;
  if (reg == 3) { num = d1; den = d1 - d3; }
  if (reg == 5) { num = d2; den = d2 - d6; }
  if (reg == 4) { num = e43; den = e43 + e56; }
  if (reg <= 2) { num = (T)0; den = (T)1; }
  const T t = num / den;
  // q = fma(s1, D1, base) (+ the interior's second term)
  const bool edge_bc = reg == 4, edge_ca = reg == 5, inner = reg == 6;
  const T bsx = edge_bc ? bx : ax, bsy = edge_bc ? by : ay, bsz = edge_bc ? bz : az;
  const T dx1 = edge_bc ? cx - bx : (edge_ca ? acx : abx);
  const T dy1 = edge_bc ? cy - by : (edge_ca ? acy : aby);
  const T dz1 = edge_bc ? cz - bz : (edge_ca ? acz : abz);
  const T s1 = inner ? vb * t : t;
  const T q1x = mfma_(s1, dx1, bsx), q1y = mfma_(s1, dy1, bsy), q1z = mfma_(s1, dz1, bsz);
  const T w_ = vc * t;
  qx = inner ? mfma_(w_, acx, q1x) : q1x;
  qy = inner ? mfma_(w_, acy, q1y) : q1y;
  qz = inner ? mfma_(w_, acz, q1z) : q1z;
  if (reg <= 2) {
    qx = reg == 0 ? ax : (reg == 1 ? bx : cx);
    qy = reg == 0 ? ay : (reg == 1 ? by : cy);
    qz = reg == 0 ? az : (reg == 1 ? bz : cz);
  }
}

// Inward edge-plane value of edge u -> w of a face with unit normal n:
//   m = n x (w - u),  s = m·p − m·u   (s >= 0 on the triangle's side).
// Same operation order as oracle/flash_oracle.c (its pose step precomputes m, m·u).
template <typename T>
__device__ __forceinline__ T edge_value(const typename Row4<T>::type& n, const typename Row4<T>::type& u,
                                        const typename Row4<T>::type& w, T px, T py, T pz) {
  const T e0 = w[0] - u[0], e1 = w[1] - u[1], e2 = w[2] - u[2];
  const T m0 = mfma_(n[1], e2, -(n[2] * e1));
  const T m1 = mfma_(n[2], e0, -(n[0] * e2));
  const T m2 = mfma_(n[0], e1, -(n[1] * e0));
  const T o = mfma_(m0, u[0], mfma_(m1, u[1], m2 * u[2]));
  return mfma_(m0, px, mfma_(m1, py, mfma_(m2, pz, -o)));
}

template <typename T>
__device__ __forceinline__ T plane_h(const typename Row4<T>::type& pl, T px, T py, T pz) {
  return mfma_(pl[0], px, mfma_(pl[1], py, mfma_(pl[2], pz, -pl[3])));
}

template <typename T> __device__ __forceinline__ T cert_eps();
template <> __device__ __forceinline__ double cert_eps() { return 1e-13; }
template <> __device__ __forceinline__ float cert_eps() { return 4e-6f; }

// Wave-wide f64 sum in the VALU (DPP, no LDS round trips): inclusive scan
// within each 16-lane row (row_shr 1, 2, 4, 8), then row_bcast 15 / 31 carry
// the row totals; lane 63 holds the sum, returned to every lane. Fixed order
// (deterministic). Whole wave active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_shifted(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
  return __hiloint2double(hi, lo);
}
// Wave-wide f32 min / max in the VALU (DPP scan, identity fill), result to
// every lane. Whole wave active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_shifted_f(float v, float identity) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK,
                                                    0xf, false));
}
template <bool MAX>
__device__ __forceinline__ float wave_minmax(float v) {
  const float id = MAX ? -__builtin_huge_valf() : __builtin_huge_valf();
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); };
  v = op(v, dpp_shifted_f<0x111, 0xf>(v, id));
  v = op(v, dpp_shifted_f<0x112, 0xf>(v, id));
  v = op(v, dpp_shifted_f<0x114, 0xf>(v, id));
  v = op(v, dpp_shifted_f<0x118, 0xf>(v, id));
  v = op(v, dpp_shifted_f<0x142, 0xa>(v, id));
  v = op(v, dpp_shifted_f<0x143, 0xc>(v, id));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_shifted<0x111, 0xf>(v);  // row_shr:1
  v += dpp_shifted<0x112, 0xf>(v);  // row_shr:2
  v += dpp_shifted<0x114, 0xf>(v);  // row_shr:4
  v += dpp_shifted<0x118, 0xf>(v);  // row_shr:8
  v += dpp_shifted<0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
  v += dpp_shifted<0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                          __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// The wave totals of N <= 8 doubles at once, each with wave_sum's addition
// tree at lane 63 — pairs (2i, 2i+1), quads, eights, rows of 16, then
// (row 3 + row 2) + (row 1 + row 0); IEEE addition commutes, so the tree's
// shape alone fixes the bits — in about a quarter of the adds. A scan keeps 64
// prefixes per value where one total is wanted; here a level that halves the
// lanes a value needs lets two values share a register: lanes whose level bit
// is clear keep a's partial sums, the others b's (packed_level). Pairs and
// quads pack 8 values into 2 registers (quad_perm), eights and rows run on
// those two (row_shr 4, 8: lanes 12..15 of each row hold four row totals),
// v_permlane16_swap lays the two registers' odd and even rows side by side for
// ONE add of both row pairs, v_permlane32_swap does the same for the halves.
// Returns the packed totals: value j's is in lane packed_sum_lane(j) (and the
// same lane + 32). Whole wave active.
template <int CTRL>
__device__ __forceinline__ double packed_level(double a, double b, bool hi) {
  const double x = hi ? b : a, y = hi ? a : b;
  return x + dpp_shifted<CTRL, 0xf>(y);
}
template <int CTRL>
__device__ __forceinline__ double plain_level(double a) { return a + dpp_shifted<CTRL, 0xf>(a); }
// a + b after the swap: rows (SWAP32: halves) (0, 1) of a and b side by side
template <bool SWAP32>
__device__ __forceinline__ double swapped_sum(double a, double b) {
  unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
  unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
  if constexpr (SWAP32) {
    const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    alo = lo[0]; blo = lo[1]; ahi = hi[0]; bhi = hi[1];
  } else {
    const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    alo = lo[0]; blo = lo[1]; ahi = hi[0]; bhi = hi[1];
  }
  return __hiloint2double((int)ahi, (int)alo) + __hiloint2double((int)bhi, (int)blo);
}
__device__ __forceinline__ constexpr int packed_sum_lane(int j) { return 12 + (j & 3) + 16 * (j >> 2); }
template <int N>
__device__ __forceinline__ double wave_sum_packed(const double (&v)[N]) {
  static_assert(N >= 1 && N <= 8, "two packed registers: at most 8 values");
  int lane = lane_id();
  asm volatile("" : "+v"(lane));  // (the level masks are made here, not carried by the caller's loop)
  const bool b0 = lane & 1, b1 = lane & 2;
  constexpr int NR = (N + 1) / 2, NS = (NR + 1) / 2;
  double r[NR], s[NS];
#pragma unroll
  for (int a = 0; a < NR; ++a)  // pairs: quad_perm [1, 0, 3, 2]
    r[a] = 2 * a + 1 < N ? packed_level<0xB1>(v[2 * a], v[2 * a + 1 < N ? 2 * a + 1 : 0], b0) : plain_level<0xB1>(v[2 * a]);
#pragma unroll
  for (int b = 0; b < NS; ++b)  // quads: quad_perm [2, 3, 0, 1]
    s[b] = 2 * b + 1 < NR ? packed_level<0x4E>(r[2 * b], r[2 * b + 1 < NR ? 2 * b + 1 : 0], b1) : plain_level<0x4E>(r[2 * b]);
#pragma unroll
  for (int b = 0; b < NS; ++b) {
    s[b] = plain_level<0x114>(s[b]);  // eights: row_shr:4
    s[b] = plain_level<0x118>(s[b]);  // rows: row_shr:8
  }
  // rows of s[0] | s[1]: (0 1 2 3 | 0' 1' 2' 3') -> (0 0' 2 2' | 1 1' 3 3'), summed:
  // row 0 + row 1 and row 2 + row 3 of s[0] in rows 0, 2, of s[1] in rows 1, 3
  const double t = swapped_sum<false>(s[0], s[NS - 1]);
  return swapped_sum<true>(t, t);  // (lower half, lower half) + (upper half, upper half)
}

}  // namespace fsdf
