// solver_rbf.h — the RBF skins' half of the device solver step (solver.hip's
// EXT kernels): the weight solve after the FK and its adjoint before the chain
// rule, the host loop's arithmetic (rbf_impl.h) by the workgroup.
#pragma once
#include "rbf_impl.h"
#include "solver_common.h"

namespace fsdf {

namespace {

// ---- RBF skins: the weight solve and its adjoint (rbf_impl.h) ------------------
// The last step's R | centres | u | LU (the state slot the step reads) into
// L.R and L.cen | L.u | L.lu (contiguous), and the row permutation: every
// thread's loads before its first store, as stage(). (8 doubles per thread:
// 64 KB, more than a carve that fits holds; solver_fits checks it, and that
// the row maps of all skins together, rm ints, are one load per thread.)
constexpr int kRbfPer = 8;

template <int NT>
__device__ void stage_rbf(const SolverTree& T, const SolverState& st, const Lds& L, int slot) {
  const int tid = threadIdx.x, nR = 9 * T.nb, tot = nR + 3 * T.rc + T.rm + T.rlu;
  const double* src = st.rbf + (size_t)slot * tot;
  double v[kRbfPer];
#pragma unroll
  for (int u = 0; u < kRbfPer; ++u) {
    const int i = tid + u * NT;
    v[u] = i < tot ? src[i] : 0.0;
  }
  const int pr = tid < T.rm ? st.prow[(size_t)slot * T.rm + tid] : 0;  // (rm <= NT: solver_fits)
#pragma unroll
  for (int u = 0; u < kRbfPer; ++u) {
    const int i = tid + u * NT;
    if (i < nR) L.R[i] = v[u];
    else if (i < tot) L.cen[i - nR] = v[u];
  }
  if (tid < T.rm) L.prow[tid] = pr;
}

// the LU's row map, rows 0..63 in `lo` and 64..127 in `hi` of the wave's lanes (i uniform)
__device__ __forceinline__ int prow_get(int lo, int hi, int i) {
  return i < 64 ? __builtin_amdgcn_readlane(lo, i) : __builtin_amdgcn_readlane(hi, i - 64);
}

// v moved across the lanes of each row of 16 by a DPP control (both halves)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// the wave's largest v (no NaN among them; all 64 lanes active): rotations by
// 1, 2, 4, 8 within each row of 16 lanes (row_ror), then the four rows' maxima
// from their first lanes. A maximum is exact in any order.
__device__ __forceinline__ double wave_max_f64(double v) {
  v = fmax(v, dpp_f64<0x121>(v));
  v = fmax(v, dpp_f64<0x122>(v));
  v = fmax(v, dpp_f64<0x124>(v));
  v = fmax(v, dpp_f64<0x128>(v));
  return fmax(fmax(readlane_f64(v, 0), readlane_f64(v, 16)), fmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// PA = LU of the m x m system A (LDS, m <= 128) by the workgroup: the host's
// lu_factor (rbf_impl.h) with the rows left where they are and the row map
// swapped instead (logical row i = stored row prow[i]; lane i of every wave
// holds prow[i] and prow[i + 64], the same in every wave). Step k: a barrier,
// then every working wave finds the pivot — lane i reads a_ik of its rows,
// the wave's maximum |.|, the first lane that holds it: the first index of the
// largest |.| under the host's strict > (rbf::lu_pivot), a NaN below row k
// never taken and a NaN in row k, a zero or an infinite maximum singular —
// and row i > k is eliminated by one wave, a lane per column right of k.
// Column k is read by every wave's pivot search, so no wave writes it in step
// k: the multipliers l_ik (from the a_ik the pivot search read, the host's
// product) wait in wave 0's registers and go into column k after the next
// step's barrier, when column k is no longer read by any step. With that, one
// barrier per step orders every LDS access: step k writes columns > k of rows
// > k (each entry by one lane) and column k - 1, and reads column k, the pivot
// row (not written) and the entries its own lane writes. Eliminations of a
// step are independent of each other: the host's bits.
// A singular / non-finite column sets *sing and goes on with p = k (in
// bounds; the frame fails). Ends with prow (LDS) written, no barrier after.
template <int NT>
__device__ void rbf_factor(int m, double* A, int32_t* prow, int* sing) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int W = m - 1 < NT / 64 ? (m > 1 ? m - 1 : 1) : NT / 64;  // (a wave per row below the first pivot)
  const bool two = m > 64;
  const int j0 = lane, j1 = lane + 64;  // (this lane's rows in the pivot search, its columns in the elimination)
  const bool in0 = j0 < m, in1 = j1 < m;
  int plo = lane, phi = lane + 64;
  double l0 = 0.0, l1 = 0.0;  // (wave 0: the last step's multipliers of this lane's rows, and where they go)
  int at0 = -1, at1 = -1;
  for (int k = 0; k < m; ++k) {
    __syncthreads();
    if (wave >= W) continue;
    if (wave == 0) {  // (column k - 1: read by no step from here on)
      if (at0 >= 0) A[at0] = l0;
      if (at1 >= 0) A[at1] = l1;
    }
    const int e0 = plo * m + k, e1 = phi * m + k;  // (before the swap: the stored rows this lane read)
    const bool r0 = in0 && j0 >= k, r1 = two && in1 && j1 >= k;
    const double s0 = r0 ? A[e0] : 0.0, s1 = r1 ? A[e1] : 0.0;
    double v0 = r0 ? fabs(s0) : -1.0, v1 = r1 ? fabs(s1) : -1.0;
    const bool n0 = v0 != v0, n1 = v1 != v1;
    const bool nan_k = __builtin_amdgcn_ballot_w64((n0 && j0 == k) || (n1 && j1 == k)) != 0;
    if (n0) v0 = -1.0;
    if (n1) v1 = -1.0;
    const double best = wave_max_f64(fmax(v0, v1));
    const uint64_t b0 = __builtin_amdgcn_ballot_w64(v0 == best);
    int p = b0 ? __builtin_ctzll(b0) : 64 + __builtin_ctzll(__builtin_amdgcn_ballot_w64(v1 == best) | (1ull << 63));
    if (nan_k || !(best > 0.0) || !isfinite(best)) {
      *sing = 1;  // (every writer writes the same value)
      p = k;
    }
    if (p != k) {
      const int a = prow_get(plo, phi, k), b = prow_get(plo, phi, p);
      if (lane == (k & 63)) {
        if (k < 64) plo = b;
        else phi = b;
      }
      if (lane == (p & 63)) {
        if (p < 64) plo = a;
        else phi = a;
      }
    }
    const double* Ak = A + prow_get(plo, phi, k) * m;
    const bool c0 = in0 && j0 > k, c1 = two && in1 && j1 > k;  // (columns right of the pivot)
    const double ak0 = c0 ? Ak[j0] : 0.0, ak1 = c1 ? Ak[j1] : 0.0;
    const double inv = 1.0 / Ak[k];
    if (wave == 0) {  // (every row the search read but the pivot's, the lane that read row p included)
      l0 = rbf::lu_multiplier(s0, inv);
      l1 = rbf::lu_multiplier(s1, inv);
      at0 = r0 && j0 != p ? e0 : -1;
      at1 = r1 && j1 != p ? e1 : -1;
    }
    for (int i = k + 1 + wave; i < m; i += W) {
      double* Ai = A + prow_get(plo, phi, i) * m;
      const double aik = Ai[k], a0 = c0 ? Ai[j0] : 0.0, a1 = c1 ? Ai[j1] : 0.0;
      const double l = rbf::lu_multiplier(aik, inv);
      if (c0) Ai[j0] = rbf::lu_eliminate(a0, l, ak0);
      if (c1) Ai[j1] = rbf::lu_eliminate(a1, l, ak1);
    }
  }
  // (the last step has no row below its pivot: nothing waits)
  __syncthreads();
  if (wave == 0) {
    if (in0) prow[j0] = plo;
    if (in1) prow[j1] = phi;
  }
}

// One wave solves A x = b from the factors: lane i (and i + 64) owns row i.
// rhs(r): entry r of the system's right-hand side (row i's is rhs(prow[i]):
// the host's swaps of b); stored: the factors lie in stored rows (this step's,
// rbf_factor) or in pivoted order (the staged ones). Forward: s_i -= l_ij b_j
// for j ascending, b_j from lane j once it is final — every row's terms in the
// host's order. Backward: row i's products u_ij b_j in the lanes j > i, then
// subtracted from b_i in ascending j (the host's order starts at j = i + 1,
// the last b to become known: the sum cannot start earlier), read straight
// from the lanes. x into out [m] (LDS); *sing = 1 if an entry is not finite.
template <class Rhs>
__device__ void rbf_wave_solve(int m, const double* lu, const int32_t* prow, bool stored, Rhs rhs, double* out,
                               int* sing) {
  const int lane = threadIdx.x & 63, i0 = lane, i1 = lane + 64;
  const bool a0 = i0 < m, a1 = i1 < m;
  const int r0 = a0 ? prow[i0] : 0, r1 = a1 ? prow[i1] : 0;
  double s0 = a0 ? rhs(r0) : 0.0, s1 = a1 ? rhs(r1) : 0.0;
  const double* row0 = lu + (stored ? r0 : (a0 ? i0 : 0)) * m;
  const double* row1 = lu + (stored ? r1 : (a1 ? i1 : 0)) * m;
  // (the next column's factors load while this one's terms are subtracted)
  const bool two = m > 64;
  double n0 = row0[0], n1 = two ? row1[0] : 0.0;
  for (int j = 0; j < m - 1; ++j) {
    const double l0 = n0, l1 = n1;
    if (j + 2 < m) {
      n0 = row0[j + 1];
      if (two) n1 = row1[j + 1];
    }
    const double bj = j < 64 ? readlane_f64(s0, j) : readlane_f64(s1, j - 64);
    if (a0 && i0 > j) s0 = rbf::subst_term(s0, l0, bj);
    if (a1 && i1 > j) s1 = rbf::subst_term(s1, l1, bj);
  }
  for (int i = m - 1; i >= 0; --i) {
    const int ri = stored ? prow_get(r0, r1, i) : i;
    const double* rowi = lu + ri * m;
    const double p0 = a0 && i0 > i ? rowi[i0] * s0 : 0.0;  // (subst_term's product; its subtraction below)
    const double p1 = a1 && i1 > i ? rowi[i1] * s1 : 0.0;
    const double dii = rowi[i];
    double s = i < 64 ? readlane_f64(s0, i) : readlane_f64(s1, i - 64);
    const int e0 = m < 64 ? m : 64;
    for (int j = i + 1; j < e0; ++j) s = s - readlane_f64(p0, j);
    for (int j = i + 1 > 64 ? i + 1 : 64; j < m; ++j) s = s - readlane_f64(p1, j - 64);
    s = s / dii;
    if (lane == (i & 63)) {
      if (i < 64) s0 = s;
      else s1 = s;
    }
  }
  if (a0) out[i0] = s0;
  if (a1) out[i1] = s1;
  if (sing && ((a0 && !isfinite(s0)) || (a1 && !isfinite(s1)))) *sing = 1;
}

// After the step's FK (L.R, L.t, L.x): the centres c_j = R_b (p_j + δ_j) + t_b
// (iterate.hip iteration_prepare's expression), every skin's fill, LU and weight
// solve: L.cen, L.lu (stored rows), L.prow, L.u. Ends with a barrier.
template <int NT>
__device__ void rbf_prepare(const SolverTree& T, const Lds& L, int* sing) {
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int e = tid; e < 3 * T.rc; e += NT) {
    const int j = e / 3, i = e - 3 * j, b = L.rbody[j], dr = L.rdrow[j];
    double p0 = L.rlocal[3 * j], p1 = L.rlocal[3 * j + 1], p2 = L.rlocal[3 * j + 2];
    if (dr >= 0) {
      const double* dl = L.x + T.nq + 3 * dr;
      p0 += dl[0];
      p1 += dl[1];
      p2 += dl[2];
    }
    const double pi = i == 0 ? p0 : (i == 1 ? p1 : p2);
    L.cen[e] = b < 0 ? pi
                     : (L.R[9 * b + 3 * i] * p0 + L.R[9 * b + 3 * i + 1] * p1 + L.R[9 * b + 3 * i + 2] * p2) +
                           L.t[3 * b + i];
  }
  __syncthreads();
  for (int r = 0; r < T.R; ++r) {
    const int n = L.rn[r], m = n + 4;
    double* A = L.lu + L.rluoff[r];
    const double* c = L.cen + 3 * L.rcoff[r];
    for (int e = tid; e < m * m; e += NT) A[e] = rbf::matrix_entry(n, c, e / m, e % m);
  }
  for (int r = 0; r < T.R; ++r)  // (each begins with a barrier)
    rbf_factor<NT>(L.rn[r] + 4, L.lu + L.rluoff[r], L.prow + L.rcoff[r] + 4 * r, sing);
  __syncthreads();
  for (int r = wave; r < T.R; r += NT / 64) {
    const int n = L.rn[r], mo = L.rcoff[r] + 4 * r;
    const double* val = L.rvalues + L.rcoff[r];
    rbf_wave_solve(n + 4, L.lu + L.rluoff[r], L.prow + mo, true,
                   [&](int i) { return rbf::rhs_entry(n, val, i); }, L.u + mo, sing);
  }
  __syncthreads();
}

// Before the chain rule: the adjoint of the last weight solve from the pass's
// RBF accumulator block (iterate.hip iteration_finish): per skin μ = M⁻¹λ (a
// wave), the pair factors 3 |c_j - c_i| (into the LU's place, done with), G_j
// (a thread per (centre, component), i ascending), then the body wrenches in
// centre order, skins in surface order (a thread per (body, component)) into
// L.bw, ∂c/∂δ = Rᵀ G (+ the regularizer's 2 weight δ: the host adds it last)
// into L.g, and Σ δ² in index order into *reg. Ends with a barrier.
template <int NT>
__device__ void rbf_adjoint(const SolverTree& T, const SolverState& st, const Lds& L, double* reg) {
  const int tid = threadIdx.x, wave = tid >> 6, nb = T.nb, R = T.R, rc = T.rc;
  const double* block = L.acc + 1 + 6 * T.S;
  for (int r = wave; r < R; r += NT / 64) {
    const int mo = L.rcoff[r] + 4 * r;
    const double* lam = block + 4 * L.rcoff[r] + 4 * r;
    rbf_wave_solve(L.rn[r] + 4, L.lu + L.rluoff[r], L.prow + mo, false, [&](int i) { return lam[i]; }, L.mu + mo,
                   nullptr);
  }
  __syncthreads();
  for (int r = 0; r < R; ++r) {
    const int n = L.rn[r];
    double* r3 = L.lu + L.rluoff[r];
    const double* c = L.cen + 3 * L.rcoff[r];
    for (int e = tid; e < n * n; e += NT) r3[e] = rbf::adjoint_r3(c, e / n, e % n);
  }
  __syncthreads();
  for (int e = tid; e < 3 * rc; e += NT) {
    const int jj = e / 3, c = e - 3 * jj;
    int r = 0;
    while (jj >= L.rcoff[r + 1]) ++r;
    const int n = L.rn[r], co = L.rcoff[r], mo = co + 4 * r, j = jj - co;
    const double* E = block + 4 * co + 4 * r + (n + 4);
    L.G[e] = rbf::adjoint_entry(n, L.cen + 3 * co, L.u + mo, L.mu + mo, E, j, c, L.lu + L.rluoff[r] + j * n);
  }
  __syncthreads();
  const int nd3 = 3 * T.n_deform;
  for (int e = tid; e < 6 * nb + nd3; e += NT) {
    if (e < 6 * nb) {
      const int b = e / 6, q = e - 6 * b;
      double w = 0.0;
      for (int jj = 0; jj < rc; ++jj) {
        if (L.rbody[jj] != b) continue;
        const double* G = L.G + 3 * jj;
        const double* cj = L.cen + 3 * jj;
        const double v = q < 3   ? G[q]
                         : q == 3 ? cj[1] * G[2] - cj[2] * G[1]
                         : q == 4 ? cj[2] * G[0] - cj[0] * G[2]
                                  : cj[0] * G[1] - cj[1] * G[0];
        w -= v;
      }
      L.bw[e] = w;
    } else {
      const int k = e - 6 * nb, row = k / 3, i = k - 3 * row;
      double gd = 0.0;
      for (int jj = 0; jj < rc; ++jj) {
        if (L.rdrow[jj] != row) continue;
        const double* G = L.G + 3 * jj;
        const int b = L.rbody[jj];
        gd += b < 0 ? G[i] : (L.R[9 * b + i] * G[0] + L.R[9 * b + 3 + i] * G[1] + L.R[9 * b + 6 + i] * G[2]);
      }
      const double dl = L.x[T.nq + k];
      gd += 2.0 * st.weight * dl;
      L.g[T.nq + k] = gd;
    }
  }
  if (tid == NT - 1) {
    double s = 0.0;
    for (int i = 0; i < nd3; ++i) s += L.x[T.nq + i] * L.x[T.nq + i];
    *reg = s;
  }
  __syncthreads();
}

}  // namespace

}  // namespace fsdf
