// solver.hip — estimate_state's solver iteration on the device: after a
// residual pass and its reduce, one launch turns
// the accumulator into the next configuration, the next surface poses and the
// next pass's posed model, so a whole frame of iterations is enqueued with no
// host round trip (fsdf_descend, iterate.hip descend_device; the default for
// rigid scenes, fsdf_set_solver).
//
// Per iteration, the arithmetic of the host loop (iterate.hip fsdf_descend around
// fsdf_value_and_gradient) in the same order, from kin_impl.h:
//   chain rule  surface wrenches -> body sums (surfaces in index order) ->
//               subtree sums (children in descending index, as the host's
//               reverse topological loop adds them) -> per joint ∂c/∂q
//               (src/gradientdescent.jl:28-39 through ForwardDiff in the
//               reference; src/tracking.jl:16-21 divides by N)
//   NaiveSolver g = (∂c/∂x / N) ./ divisors, stop at |g| < tolerance, else
//               x += clamp(-rate g, ±max_step) (flash/tracking.py; the
//               un-vendored SimpleGradientDescent.jl, src/tracking.jl:12-15)
//   FK          joint motions in parallel, then each body's chain from the
//               root composed in registers (each product as the host's level
//               order computes it), surface poses
// so x, f and the iteration count equal the host loop's bit for bit. Every
// workgroup of the launch runs the whole step on the same inputs (the same
// values) and then poses its 1,024 of the model's pose items (pose_impl.h);
// workgroup 0 alone writes the state, double-buffered by iteration parity.
//
// Scenes with RBF skins or deformations (fsdf_set_solver 3 / 4; the EXT
// kernels) add the host loop's halves around the pass, from rbf_impl.h:
//   before the chain rule  per skin μ = M⁻¹λ from the pass's RBF accumulator
//               block with the LU of the solve that produced the pass's rows,
//               G_j (sum over i ascending), body wrenches in centre order,
//               ∂c/∂δ = Rᵀ G + 2 weight δ, cost + weight Σδ² (iterate.hip
//               iteration_finish); x, g, the divisors are [nq + 3 n_deform]
//   after the FK  centres c_j = R_b (p_j + δ_j) + t_b, the fill, PA = LU, the
//               weight solve, the next pass's RBF rows in the context
//               precision (iterate.hip iteration_prepare); centres, u, LU and
//               the row permutation go to the state slot for the next step
// A singular / non-finite system ends the frame with error 3.
//
// The pass / reduce / step launches of later iterations read `flags[0]`
// (SolverState::flags) and return at once after convergence; the remaining
// iterations of the frame cost their (empty) launches only.
//
// fsdf_descend_lm's device loop (fsdf_set_lm_solver) is at the end of this
// file: lm_step_kernel and lm_pose_kernel.
#include <hip/hip_runtime.h>

#include "fsdf_internal.h"
#include "gn_impl.h"
#include "kin_impl.h"
#include "pose_impl.h"
#include "rbf_impl.h"

namespace fsdf {

namespace {

// kSolverBlock: the unit the staging capacities are counted in (kBlobPer /
// kDynPer per thread of a 256-thread group); kStepThreads: the kernels'
// width. 16 waves run the step's per-(body, component) loops in one round
// (6 (nb - 1) = 384 for M64) and publish the 12 S pose entries in one round:
// the M64 step 15.8 -> 12.6 us against 4 waves (profiles/r06/solver_nt/)
constexpr int kSolverBlock = 256;
constexpr int kStepThreads = 1024;

#if FSDF_SOLVER_TIMES
__device__ unsigned long long g_solver_times[64];
#define STAMP(i) \
  if (threadIdx.x == 0 && blockIdx.x == 0 && it0 == 5) g_solver_times[i] = wall_clock64()
#else
#define STAMP(i)
#endif

// The step's LDS: the tree blob (doubles [nd], ints [ni], padded to 16 B) |
// the accumulator [1+6S] | Rb [9nb] | tb [3nb] (the last FK's joint frames:
// read by the chain rule, then overwritten by this step's FK) | x [nx] |
// div [nx] | sub [6nb] | LR [9nb] | Lt [3nb] | R [9nb] | t [3nb] | g [nx] |
// P [12S] (the surface poses the pose items read).
// Every array the level loops touch is here: a level costs LDS latency and a
// barrier, not a global-memory round trip.
// RBF / deformable scenes (EXT kernels) append: cen [3 rc] | u [rm] | lu [rlu]
// (the last solve's centres, weights and LU factors, staged for the adjoint,
// then this step's) | mu [rm] | G [3 rc] | bw [6 nb] (the RBF chain's body
// wrenches) | prow [rm] ints (the LU's row permutation); the accumulator is
// [1 + 6S + racc] and R is staged too (the last FK's, for ∂c/∂δ).
struct Lds {
  const double *axis, *AR, *At, *BR, *Bt, *FR, *Ft;
  double *acc, *Rb, *tb, *sub, *LR, *Lt, *R, *t, *x, *g, *div, *P;
  const int32_t *parent, *kind, *qoff, *plist, *poff, *hord, *hoff, *coff, *clist, *soff, *slist, *sbody;
  const int32_t *chlist, *choff;
  const double *rlocal, *rvalues;
  const int32_t *rn, *rcoff, *rluoff, *rbody, *rdrow;
  double *cen, *u, *lu, *mu, *G, *bw;
  int32_t* prow;
};

// the doubles after the blob: acc | Rb | tb | x | div | sub | LR | Lt | R | t | g | P (the surface poses)
__host__ __device__ inline size_t work_doubles(int nb, int nx, int S) {
  return 1 + 18 * (size_t)S + 42 * (size_t)nb + 3 * (size_t)nx;
}
// and of an RBF / deformable scene: the accumulator's RBF block (after the
// 1 + 6S, so counted here) and the arrays above
__host__ __device__ inline size_t ext_doubles(int nb, int rc, int rm, int rlu, int racc) {
  return (size_t)racc + 6 * (size_t)rc + 2 * (size_t)rm + (size_t)rlu + 6 * (size_t)nb + ((size_t)rm + 1) / 2;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// The tree blob, the accumulator (optional), Rb / tb and x (+ divisors) into
// LDS: every thread issues all of its loads before its first store, so the
// staging costs one memory latency (the blob is ~23 KB for M64: 6 16-B chunks
// per thread). A copy loop that stores each load before the next one waits a
// full memory round trip (~1-2 us) per element per thread — measured 28 us per
// step that way.
constexpr int kBlobPer = 12;  // 16-B blob chunks per thread: blobs up to 48 KB
constexpr int kDynPer = 8;    // dynamic doubles per thread (accum, Rb|tb, x, div): up to 2,048

template <int NT, bool EXT>
__device__ Lds stage(const SolverTree& T, const SolverState& st, double* lds, const double* accum, int slot) {
  // (per-thread load counts for NT threads: the same totals as kBlobPer / kDynPer at kSolverBlock)
  constexpr int BP = (kBlobPer * kSolverBlock + NT - 1) / NT, DP = (kDynPer * kSolverBlock + NT - 1) / NT;
  const int tid = threadIdx.x, nb = T.nb, nx = T.nx, S = T.S;
  typedef double D2 __attribute__((ext_vector_type(2)));
  // loads: blob chunks, then the dynamic doubles (a flat index over accum | Rb tb | x | div)
  const D2* blob = (const D2*)T.blob;
  D2 bv[BP];
#pragma unroll
  for (int u = 0; u < BP; ++u) {
    const int i = tid + u * NT;
    bv[u] = i < T.chunks16 ? blob[i] : D2{0.0, 0.0};
  }
  const int nacc = 1 + 6 * S + (EXT ? T.racc : 0);  // (EXT: the RBF block follows the surface wrenches)
  const int na = accum ? nacc : 0, nr = accum ? 12 * nb : 0, nd_ = st.div ? nx : 0;
  const int ndyn = na + nr + nx + nd_;
  double dv[DP];
#pragma unroll
  for (int u = 0; u < DP; ++u) {
    const int i = tid + u * NT;
    double v = 0.0;
    if (i < na) v = accum[i];
    else if (i < na + nr) v = st.Rb[(size_t)slot * 12 * nb + (i - na)];  // (Rb | tb adjacent in a slot)
    else if (i < na + nr + nx) v = st.x[(size_t)slot * nx + (i - na - nr)];
    else if (i < ndyn) v = st.div[i - na - nr - nx];
    dv[u] = v;
  }
  Lds L;
  double* d = lds;
  D2* l2 = (D2*)lds;
#pragma unroll
  for (int u = 0; u < BP; ++u) {
    const int i = tid + u * NT;
    if (i < T.chunks16) l2[i] = bv[u];
  }
  L.axis = d + T.axis;
  L.AR = d + T.AR;
  L.At = d + T.At;
  L.BR = d + T.BR;
  L.Bt = d + T.Bt;
  L.FR = d + T.frame_R;
  L.Ft = d + T.frame_t;
  const int32_t* iv = (const int32_t*)(d + T.nd);
  L.parent = iv + T.parent;
  L.kind = iv + T.kind;
  L.qoff = iv + T.qoff;
  L.plist = iv + T.path_list;
  L.poff = iv + T.path_off;
  L.hord = iv + T.height_order;
  L.hoff = iv + T.height_off;
  L.coff = iv + T.child_off;
  L.clist = iv + T.child_list;
  L.soff = iv + T.surf_off;
  L.slist = iv + T.surf_list;
  L.sbody = iv + T.surface_body;
  L.chlist = iv + T.chain_list;
  L.choff = iv + T.chain_off;
  d += 2 * T.chunks16;  // (the blob, padded to 16 B)
  L.acc = d;
  d += nacc;
  L.Rb = d;
  d += 9 * nb;
  L.tb = d;
  d += 3 * nb;
  L.x = d;
  d += nx;
  L.div = st.div ? d : nullptr;
  d += nx;
  L.sub = d;
  d += 6 * nb;
  L.LR = d;
  d += 9 * nb;
  L.Lt = d;
  d += 3 * nb;
  L.R = d;
  d += 9 * nb;
  L.t = d;
  d += 3 * nb;
  L.g = d;
  d += nx;
  L.P = d;
  if (EXT) {
    const double* bd = lds;
    const int32_t* bi = (const int32_t*)(bd + T.nd);
    L.rlocal = bd + T.rbf_local;
    L.rvalues = bd + T.rbf_values;
    L.rn = bi + T.rbf_n;
    L.rcoff = bi + T.rbf_coff;
    L.rluoff = bi + T.rbf_luoff;
    L.rbody = bi + T.rbf_body;
    L.rdrow = bi + T.rbf_drow;
    d += 12 * S;
    L.cen = d;
    d += 3 * T.rc;
    L.u = d;
    d += T.rm;
    L.lu = d;
    d += T.rlu;
    L.mu = d;
    d += T.rm;
    L.G = d;
    d += 3 * T.rc;
    L.bw = d;
    d += 6 * nb;
    L.prow = (int32_t*)d;
  }
  // the dynamic doubles land at acc (accum | Rb tb | x | div are contiguous
  // there too; without an accumulator x lands at L.x)
#pragma unroll
  for (int u = 0; u < DP; ++u) {
    const int i = tid + u * NT;
    if (i < na + nr) L.acc[i] = dv[u];
    else if (i < ndyn) L.x[i - na - nr] = dv[u];
  }
  for (int i = tid; i < nx; i += NT) L.g[i] = 0.0;
  return L;
}

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

// FK of L.x into L.R, t, Rb, tb (LDS; *bad |= 1 for a zero quaternion /
// unknown joint). Global memory is not touched: a workgroup barrier after a
// global store waits for the store to complete (its release fence), so every
// store of the step is issued after the last barrier (publish()).
template <int NT>
__device__ void fk(const SolverTree& T, const Lds& L, int* bad, int it0 = -1) {
  (void)it0;  // (FSDF_SOLVER_TIMES: the iteration whose phases are clocked)
  const int tid = threadIdx.x, nb = T.nb;
  for (int b = 1 + tid; b < nb; b += NT) {
    const int k = L.kind[b];
    if (!kin::joint_local(k, L.axis + 3 * b, L.AR + 9 * b, L.At + 3 * b, L.BR + 9 * b, L.Bt + 3 * b,
                          L.x + (k ? L.qoff[b] : 0), L.LR + 9 * b, L.Lt + 3 * b))
      atomicOr(bad, 1);
  }
  if (tid == 0) {  // the root: identity (one thread: no per-lane choice of the destination array)
    for (int i = 0; i < 9; ++i) {
      const double v = (i % 4 == 0) ? 1.0 : 0.0;
      L.R[i] = v;
      L.Rb[i] = v;
    }
    for (int i = 0; i < 3; ++i) {
      L.t[i] = 0.0;
      L.tb[i] = 0.0;
    }
  }
  __syncthreads();
  STAMP(5);
  // one thread per body composes its chain from the root in registers (every
  // ancestor's product as the host's level order computes it: the same bits,
  // no barrier per level); the ancestors' R, t only, and the joint frame
  // Rb, tb = R_parent · joint_to_parent for b itself
  for (int b = 1 + tid; b < nb; b += NT) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, v[12], w[12], Rp[9], tp[3];
    const int q0 = L.poff[b], q1 = L.poff[b + 1];
    // the next ancestor's joint motion is loaded while this one composes
    double nLR[9], nLt[3];
    int an = L.plist[q0];
    kin::load(L.LR + 9 * an, nLR, 9);
    kin::load(L.Lt + 3 * an, nLt, 3);
    for (int q = q0; q < q1; ++q) {
      const int a = an;
      double LR[9], Lt[3];
#pragma unroll
      for (int e = 0; e < 9; ++e) LR[e] = nLR[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) Lt[e] = nLt[e];
      if (q + 1 < q1) {
        an = L.plist[q + 1];
        kin::load(L.LR + 9 * an, nLR, 9);
        kin::load(L.Lt + 3 * an, nLt, 3);
      }
      (void)a;
#pragma unroll
      for (int e = 0; e < 9; ++e) Rp[e] = R[e];  // (the parent's frame, for b's joint frame below)
#pragma unroll
      for (int e = 0; e < 3; ++e) tp[e] = t[e];
#pragma unroll
      for (int e = 0; e < 12; ++e) v[e] = kin::compose_entry(e, R, t, LR, Lt, nullptr, nullptr);
#pragma unroll
      for (int e = 0; e < 9; ++e) R[e] = v[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) t[e] = v[9 + e];
    }
    // b's joint frame Tb_b = T_parent · joint_to_parent, after the walk (not a
    // branch on the last level inside it: lanes of different depths would run
    // that branch at every level between them)
    {
      double AR[9], At[3];
      kin::load(L.AR + 9 * b, AR, 9);
      kin::load(L.At + 3 * b, At, 3);
#pragma unroll
      for (int e = 0; e < 12; ++e) w[e] = kin::compose_entry(12 + e, Rp, tp, nullptr, nullptr, AR, At);
    }
    kin::store(L.R + 9 * b, v, 9);
    kin::store(L.t + 3 * b, v + 9, 3);
    kin::store(L.Rb + 9 * b, w, 9);
    kin::store(L.tb + 3 * b, w + 9, 3);
  }
  __syncthreads();
}

// The end of a step (and of the init): the surface poses into LDS (a
// non-finite entry marks the frame failed, error 2), then — the next pass's
// pose, in this launch instead of a pose kernel of its own — every work item
// of the model's pose from them (pose_impl.h: world planes, screening pairs,
// stage images, vertices, spheres and scales into the posed model the pass
// reads), the joint frames for the next chain rule, x and — thread 0 — f, the
// iteration count and the done / error flags. Every global store is issued
// after the last barrier (a barrier's release fence would wait for them).
// pose = false: the last iteration (no pass follows) publishes x and the flags only.
// EXT with skins: the next pass's RBF rows too (centre, w_j per centre, then
// a, b; the context precision: (float) of the f64 rows, as launch_to_f32), and
// what the next step's adjoint needs (SolverState::rbf, prow); sing: a
// singular weight solve (error 3, as the host fails before it poses).
template <typename TP, int NT, bool EXT>
__device__ void publish(const SolverTree& T, const SolverState& st, const Lds& L, bool pose, int bad, double f,
                        int it, int done, const LocalModel& lm, const PosedModel& pm, int sing = 0) {
  const int tid = threadIdx.x, nb = T.nb, wg = blockIdx.x;
  const int slot = it & 1;  // (the state the next step reads: x, Rb, tb of iteration it)
  __shared__ int nonfinite;
  if (pose) {
    if (tid == 0) nonfinite = 0;
    __syncthreads();
    for (int i = tid; i < 12 * T.S; i += NT) {
      const int k = i / 12, q = i % 12, b = L.sbody[k];
      const double v = b < 0 ? ((q % 4 == 0 && q < 9) ? 1.0 : 0.0)
                             : kin::surface_pose_entry(q, L.R + 9 * b, L.t + 3 * b, L.FR + 9 * k, L.Ft + 3 * k);
      L.P[i] = v;
      if (!isfinite(v)) nonfinite = 1;  // (every writer writes the same value)
    }
    __syncthreads();
    // this workgroup's NT consecutive work items of the pose (whole waves: the
    // total is a multiple of 64, as NT)
    const int item = wg * NT + tid;
    if (item < pose_items(lm))
      pose_item<TP>(lm, L.P, (TP*)pm.planes_w, pm.spheres_w, (TP*)pm.verts_w, (TP*)pm.hscale_w,
                    sizeof(TP) == 8 ? pm.screen_w : nullptr, sizeof(TP) == 8 ? (I4*)pm.image_w : nullptr, item);
  }
  if (wg != 0) return;  // (the state: workgroup 0; every workgroup computed the same values)
  if (pose) {
    double* Rb = st.Rb + (size_t)slot * 12 * nb;
    for (int i = tid; i < 9 * nb; i += NT) Rb[i] = L.Rb[i];
    for (int i = tid; i < 3 * nb; i += NT) Rb[9 * nb + i] = L.tb[i];
  }
  if (EXT && pose && T.R > 0) {
    TP* rows = (TP*)pm.rbf_rows;
    const int nR = 9 * nb;
    double* dst = st.rbf + (size_t)slot * (nR + 3 * T.rc + T.rm + T.rlu);
    for (int i = tid; i < nR; i += NT) dst[i] = L.R[i];
    dst += nR;
    for (int i = tid; i < 3 * T.rc + T.rm; i += NT) dst[i] = L.cen[i];  // (cen | u adjacent)
    dst += 3 * T.rc + T.rm;
    for (int r = 0; r < T.R; ++r) {
      const int n = L.rn[r], m = n + 4, co = L.rcoff[r], mo = co + 4 * r;
      const double *c = L.cen + 3 * co, *u = L.u + mo, *A = L.lu + L.rluoff[r];
      const int32_t* pr = L.prow + mo;
      for (int e = tid; e < 4 * (n + 1); e += NT) {
        const int j = e >> 2, q = e & 3;
        const double v = j < n ? (q < 3 ? c[3 * j + q] : u[j]) : u[n + q];
        rows[4 * (size_t)(co + r) + e] = (TP)v;
      }
      // the factors in pivoted order, as the host's in-place swaps leave them
      for (int e = tid; e < m * m; e += NT) dst[L.rluoff[r] + e] = A[pr[e / m] * m + e % m];
      for (int i = tid; i < m; i += NT) st.prow[(size_t)slot * T.rm + mo + i] = pr[i];
    }
  }
  if (it > 0)  // (the init's x is slot 0's own, which its workgroups are reading)
    for (int i = tid; i < T.nx; i += NT) st.x[(size_t)slot * T.nx + i] = L.x[i];
  if (tid == 0) {
    *st.f = f;
    st.flags[1] = it;
    if (EXT && sing && !bad) {
      st.flags[2] = 3;
      st.flags[0] = 1;
    } else if (pose && nonfinite) {
      st.flags[2] = 2;
      st.flags[0] = 1;
    } else if (bad || done) {
      st.flags[2] = bad ? 1 : 0;
      st.flags[0] = 1;
    }
  }
}

// The chain rule's subtree wrenches: per body its surfaces' accumulator rows in
// index order (from the RBF chain's body wrench with skins), then the subtree
// sums, children in descending index — fsdf_config_gradient's additions in its
// order — into L.sub [nb][6]. Ends with a barrier.
template <int NT>
__device__ void subtree_wrenches(const SolverTree& T, const Lds& L, bool skins) {
  const int tid = threadIdx.x, nb = T.nb;
  if (T.chains) {
    // chains (every non-root body has <= 1 child): body b's subtree sum along
    // its chain, deepest first — sub[a] = own[a] + sub[child], own[a] the body's
    // surfaces summed in index order from 0.0: fsdf_config_gradient's additions
    // in its order, no level barriers. First every own[a] (one thread per (a,
    // component); into L.LR, free until the FK), then one thread per (b,
    // component) walks its chain, the next four own[] loads issued before
    // their additions (a chain level costs an addition, not a chain of
    // dependent LDS loads)
    double* own = L.LR;
    for (int i = tid; i < 6 * (nb - 1); i += NT) {
      const int a = 1 + i / 6, j = i % 6;
      double o = skins ? L.bw[6 * a + j] : 0.0;  // (fsdf_config_gradient starts from the RBF chain's body wrench)
      for (int u = L.soff[a]; u < L.soff[a + 1]; ++u) o += L.acc[1 + 6 * L.slist[u] + j];
      own[6 * a + j] = o;
    }
    __syncthreads();
    for (int i = tid; i < 6 * (nb - 1); i += NT) {
      const int b = 1 + i / 6, j = i % 6;
      const int q0 = L.choff[b];
      int q = L.choff[b + 1] - 1;
      double s = own[6 * L.chlist[q] + j];
      for (--q; q >= q0; q -= 4) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = q - k >= q0 ? own[6 * L.chlist[q - k] + j] : 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (q - k >= q0) s = v[k] + s;
      }
      L.sub[6 * b + j] = s;
    }
    __syncthreads();
  } else {
    // body wrenches: each body's surfaces in index order (fsdf_config_gradient)
    for (int i = tid; i < 6 * nb; i += NT) {
      const int b = i / 6, j = i - 6 * b;
      double s = skins ? L.bw[i] : 0.0;
      for (int q = L.soff[b]; q < L.soff[b + 1]; ++q) s += L.acc[1 + 6 * L.slist[q] + j];
      L.sub[i] = s;
    }
    __syncthreads();
    // subtree sums: parents by height, each adding its children in descending
    // index; a narrow tree (<= 10 parents per height) in one wave, its levels
    // ordered by wave-local fences instead of workgroup barriers
    if (T.narrow) {
      if (tid < 64) {
        for (int h = 0; h < T.H; ++h) {
          const int a = L.hoff[h], e = L.hoff[h + 1];
          if (tid < 6 * (e - a)) {
            const int p = L.hord[a + tid / 6], j = tid % 6;
            double s = L.sub[6 * p + j];
            for (int q = L.coff[p]; q < L.coff[p + 1]; ++q) s += L.sub[6 * L.clist[q] + j];
            L.sub[6 * p + j] = s;
          }
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      }
      __syncthreads();
    } else {
      for (int h = 0; h < T.H; ++h) {
        const int a = L.hoff[h], e = L.hoff[h + 1];
        for (int i = tid; i < 6 * (e - a); i += NT) {
          const int p = L.hord[a + i / 6], j = i % 6;
          double s = L.sub[6 * p + j];
          for (int q = L.coff[p]; q < L.coff[p + 1]; ++q) s += L.sub[6 * L.clist[q] + j];
          L.sub[6 * p + j] = s;
        }
        __syncthreads();
      }
    }
  }
}

template <typename TP, bool EXT>
__global__ __launch_bounds__(kStepThreads) void solver_init_kernel(SolverTree T, SolverState st, LocalModel lm,
                                                                   PosedModel pm) {
  extern __shared__ double lds[];
  __shared__ int bad, sing;
  const int tid = threadIdx.x;
  if (tid == 0) {
    bad = 0;
    sing = 0;
  }
  const Lds L = stage<kStepThreads, EXT>(T, st, lds, nullptr, 0);  // (x0 in slot 0)
  __syncthreads();
  fk<kStepThreads>(T, L, &bad);  // (ends with a barrier; the host zeroed the flags before this launch)
  if (EXT && T.R > 0) rbf_prepare<kStepThreads>(T, L, &sing);  // (ends with a barrier)
  publish<TP, kStepThreads, EXT>(T, st, L, true, bad, 0.0, 0, 0, lm, pm, EXT ? sing : 0);
}

// One step over NT threads (solver_step_kernel: kStepThreads). (A launch
// that also did the pass's final reduce — its last workgroup running the step
// — measured no faster: the hand-off between workgroups costs what the launch
// saves; branch archive/fused-reduce-step)
template <typename TP, int NT, bool EXT>
__device__ void step_body(const SolverTree& T, const SolverState& st, const double* __restrict__ accum,
                          double* __restrict__ lds, const LocalModel& lm, const PosedModel& pm, int it_before) {
  // (the frame's done flag loads with the stage's loads — thread 0's, into LDS:
  // workgroup 0 of this launch may set the flag at its end, so two threads'
  // own loads could disagree; after the stage's barrier the whole workgroup
  // branches on the one value. A workgroup that reads it set returns — no
  // pass follows a converged step)
  __shared__ int bad, verdict, s_done, sing;
  __shared__ double s_f, s_reg;
  const int tid = threadIdx.x, nb = T.nb, nx = T.nx;
  if (tid == 0) s_done = __builtin_nontemporal_load(st.flags);
#if FSDF_SOLVER_TIMES
  const int it0 = it_before;
#endif
  STAMP(0);
  if (tid == 0) {
    bad = 0;
    if (EXT) sing = 0;
  }
  const Lds L = stage<NT, EXT>(T, st, lds, accum, it_before & 1);
  if (EXT && T.R > 0) stage_rbf<NT>(T, st, L, it_before & 1);
  __syncthreads();
  if (s_done) return;  // converged (or failed): the frame's remaining steps are no-ops (workgroup-uniform)
  STAMP(1);
  const bool skins = EXT && T.R > 0;
  if (EXT) rbf_adjoint<NT>(T, st, L, &s_reg);  // (ends with a barrier)
  subtree_wrenches<NT>(T, L, skins);  // (ends with a barrier)
  STAMP(2);
  for (int b = 1 + tid; b < nb; b += NT) {
    const int k = L.kind[b];
    if (k && !kin::joint_gradient(k, L.axis + 3 * b, L.Rb + 9 * b, L.tb + 3 * b, L.x + L.qoff[b], L.sub + 6 * b,
                                  L.g + L.qoff[b]))
      atomicOr(&bad, 1);
  }
  __syncthreads();
  for (int i = tid; i < nx; i += NT) {
    double gi = L.g[i] / st.n_points;
    if (L.div) gi = gi / L.div[i];
    L.g[i] = gi;
  }
  __syncthreads();
  STAMP(3);
  // |g|^2 in index order, as the host sums it: wave 0 squares in parallel, lane
  // 0 adds the squares in order, read straight from the lanes (readlane: no
  // LDS round trip per term)
  double nrm2 = 0.0;
  if (nx <= 64) {
    if (tid < 64) {
      const double gi = tid < nx ? L.g[tid] : 0.0;
      const double sq = gi * gi;
      for (int i = 0; i < nx; ++i) nrm2 += readlane_f64(sq, i);
    }
  } else if (tid == 0) {
    for (int i = 0; i < nx; ++i) nrm2 += L.g[i] * L.g[i];
  }
  const int it = it_before + 1;
  if (tid == 0) {
    const double cost = L.acc[0] + st.weight * (EXT ? s_reg : 0.0);  // (rigid: the regularizer's sum is 0.0)
    s_f = cost / st.n_points;
    verdict = bad ? 3 : (sqrt(nrm2) < st.tol ? 1 : (it >= st.limit ? 2 : 0));
  }
  __syncthreads();
  const int v = verdict;
  const double f = s_f;
  if (v == 3 || v == 1) {  // failed / converged: x stays
    publish<TP, NT, EXT>(T, st, L, false, v == 3, f, it, 1, lm, pm);
    return;
  }
  for (int i = tid; i < nx; i += NT) L.x[i] = L.x[i] + kin::clipped_step(st.rate, L.g[i], st.max_step);
  if (v == 2) {  // the last iteration: no pass follows
    __syncthreads();
    publish<TP, NT, EXT>(T, st, L, false, 0, f, it, 1, lm, pm);
    return;
  }
  __syncthreads();
  STAMP(4);
#if FSDF_SOLVER_TIMES
  fk<NT>(T, L, &bad, it0);  // (ends with a barrier)
#else
  fk<NT>(T, L, &bad);  // (ends with a barrier)
#endif
  STAMP(6);
  if (skins) rbf_prepare<NT>(T, L, &sing);  // (ends with a barrier)
  publish<TP, NT, EXT>(T, st, L, true, bad, f, it, 0, lm, pm, EXT ? sing : 0);
  STAMP(9);
}

template <typename TP, bool EXT>
__global__ __launch_bounds__(kStepThreads) void solver_step_kernel(SolverTree T, SolverState st,
                                                                   const double* __restrict__ accum, LocalModel lm,
                                                                   PosedModel pm, int it_before) {
  extern __shared__ double lds[];
  step_body<TP, kStepThreads, EXT>(T, st, accum, lds, lm, pm, it_before);
}

// ---- the device Levenberg-Marquardt loop (fsdf_descend_lm, fsdf_set_lm_solver) ----
// After every evaluation (pass, reduce, moments, their reduce) one single-
// workgroup launch, lm_step_kernel, does what fsdf_lm_minimize does between two
// calls of its objective, in the host's order and with gn_impl.h's arithmetic:
//   objective   the chain rule of step_body; f_t = c / N, g / N (+ the prior of
//               fsdf_set_lm_prior, iterate.hip lm_objective's operations)
//   verdict     the first evaluation is accepted, a later one when f_t < f; on
//               acceptance the Gauss-Newton matrix at the trial (per-body
//               moments in surface order, subtree sums by height with the
//               children in descending index, u = C_b s_j, one thread per
//               matrix entry), H = (2 A) / N (+ prior), and x, f, g, H kept as
//               the accepted state in global memory; lambda / 10 (>= 1e-12),
//               or x 10 and the end beyond 1e12 on rejection
//   end         the evaluation count, then |g|_2 of the accepted point summed
//               in index order
//   step        fsdf_lm_step in wave 0, a matrix row per lane: left-looking
//               Cholesky (every L_ij subtracts L_ik L_jk for k ascending), the
//               forward solve column by column, the back-substitution's
//               products in the lanes and added in ascending k (readlane); a
//               degenerate factorisation raises lambda and factors again
//   next trial  x + step into the other slot
// and a second launch, lm_pose_kernel (solver_init_kernel's work on that slot:
// FK, the joint frames, the posed model), prepares the next pass. The solve in
// a launch of one workgroup keeps the matrix, the factor and the subtree
// moments out of the many-workgroup pose launch, whose carve (the tree blob in
// LDS) fills most of 64 KB at M64; here the tree is read from global memory
// (L2) and the carve is acc | Rb tb | x | own | sub | g | xa | pe | C [nb][36] |
// rows [nq][6] | u [nq][6] | L [nq][nq | 1] | the coordinates' bodies | the parents: 60 KB at
// M64 (65 bodies, 48 coordinates, 64 surfaces).
constexpr int kLmThreads = 1024;
constexpr int kLmMaxRaises = 400;  // tenfold raises from the smallest positive double pass 1e12 in 336

__host__ __device__ inline int lm_ld(int nq) { return nq | 1; }  // (odd row stride: the lanes' rows in different banks)
__host__ __device__ inline size_t lm_work_doubles(int nb, int nq, int S) {
  return (1 + 6 * (size_t)S) + 60 * (size_t)nb + 16 * (size_t)nq + (size_t)nq * lm_ld(nq) + ((size_t)nq + (size_t)nb + 1) / 2;
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// fsdf_lm_step by one wave, lane i owning row i (n <= 64): A [n][ld] in LDS
// holds H (its lower triangle is read) and becomes the factor; hd = this
// lane's H_ii, g its gradient entry. false: a degenerate factorisation or a
// solve that is not finite. *step = this lane's clamped step entry.
__device__ bool lm_wave_step(int n, int ld, double* A, double hd, double g, double lambda, double floor_d,
                             double max_step, double* step, int it0 = -1) {
  (void)it0;  // (FSDF_SOLVER_TIMES: the evaluation whose phases are clocked)
  const int lane = threadIdx.x & 63;
  const bool in = lane < n;
  double* row = A + (in ? lane : 0) * ld;
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    if (in && lane >= j) {
      s = lane == j ? gn::damped_diagonal(hd, lambda, floor_d) : row[j];
      const double* rj = A + j * ld;
      // (eight terms' loads before their subtractions: the chain then waits for one LDS latency
      // per eight terms, not per term — the order of the subtractions is unchanged)
      int k = 0;
      for (; k + 8 <= j; k += 8) {
        double a[8], b[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          a[v] = row[k + v];
          b[v] = rj[k + v];
        }
#pragma unroll
        for (int v = 0; v < 8; ++v) s = gn::minus_product(s, a[v], b[v]);
      }
      for (; k < j; ++k) s = gn::minus_product(s, row[k], rj[k]);
    }
    const double p = readlane_f64(s, j);
    if (gn::bad_pivot(p)) return false;
    const double ljj = sqrt(p);
    if (in && lane >= j) row[j] = lane == j ? ljj : s / ljj;
    wave_lds_fence();
  }
  STAMP(6);
  double y = in ? g : 0.0;
  for (int k = 0; k < n; ++k) {  // L y = g, column by column: every row's terms in ascending k
    const double lkk = A[k * ld + k];
    if (lane == k) y = y / lkk;
    const double yk = readlane_f64(y, k);
    if (in && lane > k) y = gn::minus_product(y, row[k], yk);
  }
  STAMP(7);
  for (int i = n - 1; i >= 0; --i) {  // Lᵀ z = y: the products in the lanes k > i, subtracted in ascending k
    const double p = in && lane > i ? row[i] * y : 0.0;
    double s = readlane_f64(y, i);
    for (int k = i + 1; k < n; ++k) s = s - readlane_f64(p, k);
    s = s / A[i * ld + i];
    if (lane == i) y = s;
  }
  STAMP(8);
  if (__builtin_amdgcn_ballot_w64(in && !isfinite(y)) != 0) return false;
  *step = gn::clamped_step(y, max_step);
  return true;
}

__global__ __launch_bounds__(kLmThreads) void lm_step_kernel(SolverTree T, LmState ls,
                                                             const double* __restrict__ accum,
                                                             const double* __restrict__ moments, int it_before) {
  extern __shared__ double lds[];
  constexpr int NT = kLmThreads;
  // (bad: the chain rule's failures, read by every thread before the matrix phase; bad_rows: that phase's own)
  __shared__ int s_done, bad, bad_rows, s_accept, s_end;
  __shared__ double s_f, s_lam;
  const int tid = threadIdx.x, nb = T.nb, nq = T.nq, S = T.S, ld = lm_ld(nq);
#if FSDF_SOLVER_TIMES
  const int it0 = it_before;  // (phases, 10 ns: 1 staged, 2 chain rule, 3 verdict, 4 matrix, 5 end checks,
                              // 6 factor, 7 forward solve, 8 back-substitution, 9 end)
#else
  const int it0 = -1;
#endif
  STAMP(0);
  if (tid == 0) {
    s_done = __builtin_nontemporal_load(ls.flags);
    bad = 0;
    bad_rows = 0;
  }
  // the tree from global memory; the work arrays in LDS
  const double* bd = (const double*)T.blob;
  const int32_t* bi = (const int32_t*)(bd + T.nd);
  Lds L = {};
  L.axis = bd + T.axis;
  L.parent = bi + T.parent;
  L.kind = bi + T.kind;
  L.qoff = bi + T.qoff;
  L.hord = bi + T.height_order;
  L.hoff = bi + T.height_off;
  L.coff = bi + T.child_off;
  L.clist = bi + T.child_list;
  L.soff = bi + T.surf_off;
  L.slist = bi + T.surf_list;
  L.chlist = bi + T.chain_list;
  L.choff = bi + T.chain_off;
  double* d = lds;
  const int na = 1 + 6 * S, nr = 12 * nb;
  L.acc = d;
  d += na;
  L.Rb = d;
  d += 9 * nb;
  L.tb = d;
  d += 3 * nb;
  L.x = d;
  d += nq;
  L.LR = d;  // (subtree_wrenches' own [nb][6])
  d += 6 * nb;
  L.sub = d;
  d += 6 * nb;
  L.g = d;
  d += nq;
  double* xa = d;  // the accepted x
  d += nq;
  double* pe = d;  // the prior's terms mu_i e_i^2
  d += nq;
  double* C = d;  // [nb][36] subtree moments
  d += 36 * nb;
  double* rows = d;  // [nq][6] motion rows
  d += 6 * nq;
  double* u = d;  // [nq][6] C_b s_j
  d += 6 * nq;
  double* A = d;  // [nq][ld] H, then its factor
  d += nq * ld;
  int32_t* cbody = (int32_t*)d;  // [nq] the body whose joint owns the coordinate (-1: none)
  int32_t* par = cbody + nq;     // [nb] the tree's parents (the matrix entries' ancestor walks)
  // stage: every thread's loads before its first store (stage()); na <= NT, nr <= 2 NT, nq <= 64 (lm_solver_fits)
  const int slot = it_before & 1;
  const double* rsrc = ls.Rb + (size_t)slot * nr;
  const bool mine = tid < nq, later = it_before > 0;
  const double a0 = tid < na ? accum[tid] : 0.0;
  const double r0 = tid < nr ? rsrc[tid] : 0.0, r1 = tid + NT < nr ? rsrc[tid + NT] : 0.0;
  const double x0 = mine ? ls.x[(size_t)slot * nq + tid] : 0.0;
  const double xa0 = mine && later ? ls.xa[tid] : 0.0, ga0 = mine && later ? ls.g[tid] : 0.0;
  const double mu0 = mine && ls.mu ? ls.mu[tid] : 0.0, xr0 = mine && ls.mu ? ls.x_ref[tid] : 0.0;
  double h_old[(64 * 64 + NT - 1) / NT];  // (a rejected trial: the accepted H into the factor's place)
#pragma unroll
  for (int v = 0; v < (64 * 64 + NT - 1) / NT; ++v) {
    const int i = tid + v * NT;
    h_old[v] = later && i < nq * nq ? ls.H[i] : 0.0;
  }
  if (tid < na) L.acc[tid] = a0;
  if (tid < nr) L.Rb[tid] = r0;  // (Rb | tb adjacent, as in a slot)
  if (tid + NT < nr) L.Rb[tid + NT] = r1;
  if (mine) {
    L.x[tid] = x0;
    L.g[tid] = 0.0;
    cbody[tid] = -1;
    const double e = x0 - xr0;
    pe[tid] = mu0 * (e * e);
  }
  for (int i = tid; i < 6 * nq; i += NT) rows[i] = 0.0;
  for (int i = tid; i < nb; i += NT) par[i] = L.parent[i];
  __syncthreads();
  if (s_done) return;  // the frame has ended: its remaining launches are no-ops (workgroup-uniform)
  STAMP(1);
  // the chain rule (step_body's)
  subtree_wrenches<NT>(T, L, false);  // (ends with a barrier)
  for (int b = 1 + tid; b < nb; b += NT) {
    const int k = L.kind[b];
    if (k && !kin::joint_gradient(k, L.axis + 3 * b, L.Rb + 9 * b, L.tb + 3 * b, L.x + L.qoff[b], L.sub + 6 * b,
                                  L.g + L.qoff[b]))
      atomicOr(&bad, 1);
  }
  __syncthreads();
  STAMP(2);
  // the wrapped objective at the trial (iterate.hip lm_objective) and the verdict
  if (mine) {
    double gi = L.g[tid] / ls.n_points;
    if (ls.mu) gi = gi + (2.0 * mu0) * (x0 - xr0);
    L.g[tid] = gi;
  }
  if (tid == 0) {
    const double cost = L.acc[0] + ls.weight * 0.0;  // (iteration_finish: the regularizer's sum is 0.0)
    double ft = cost / ls.n_points;
    if (ls.mu) {
      double r = 0.0;
      for (int i = 0; i < nq; ++i) r += pe[i];
      ft = ft + r;
    }
    const double f = later ? *ls.f : ft;
    double lam = *ls.lam;
    const bool accept = !later || ft < f;
    int end = 0;
    if (accept) {
      if (later) lam = 1e-12 > lam / 10.0 ? 1e-12 : lam / 10.0;
    } else {
      lam *= 10.0;
      if (lam > 1e12) end = 1;
    }
    s_f = accept ? ft : f;
    s_lam = lam;
    s_accept = accept;
    s_end = end;
  }
  __syncthreads();
  STAMP(3);
  const int count = it_before + 1;
  const bool accept = s_accept != 0, last = count >= ls.limit;
  if (accept && !last && !bad) {
    // the Gauss-Newton matrix at the trial (fsdf_gauss_newton_matrix): per-body
    // moments, surfaces in index order; the motion rows
    for (int i = tid; i < 36 * (nb - 1); i += NT) {
      const int b = 1 + i / 36, e = i % 36, t = gn::tri_index(e / 6, e % 6);
      double s = 0.0;
      for (int q = L.soff[b]; q < L.soff[b + 1]; ++q) s += moments[kMomentsLen * L.slist[q] + t];
      C[36 * b + e] = s;
    }
    for (int b = 1 + tid; b < nb; b += NT) {
      const int k = L.kind[b], w = gn::joint_width(k), q0 = L.qoff[b];
      if (!w) continue;
      if (!gn::joint_rows(k, L.axis + 3 * b, L.Rb + 9 * b, L.tb + 3 * b, L.x + q0, rows + 6 * q0))
        atomicOr(&bad_rows, 1);
      for (int e = 0; e < w; ++e) cbody[q0 + e] = b;
    }
    __syncthreads();
    // subtree sums: parents by height, children in descending index
    for (int h = 0; h < T.H; ++h) {
      const int a = L.hoff[h], e = L.hoff[h + 1];
      for (int i = tid; i < 36 * (e - a); i += NT) {
        const int p = L.hord[a + i / 36], j = i % 36;
        double s = C[36 * p + j];
        for (int q = L.coff[p]; q < L.coff[p + 1]; ++q) s += C[36 * L.clist[q] + j];
        C[36 * p + j] = s;
      }
      __syncthreads();
    }
    for (int i = tid; i < 6 * nq; i += NT) {
      const int c = i / 6, b = cbody[c];
      u[i] = b > 0 ? gn::moment_row(C + 36 * b, rows + 6 * c, i % 6) : 0.0;
    }
    __syncthreads();
    // one entry per thread: coordinate i against j when i's body is j's, or
    // an ancestor of it (a parent's index is below its child's)
    for (int i = tid; i < nq * nq; i += NT) {
      const int r = i / nq, c = i % nq, br = cbody[r], bc = cbody[c];
      double a = 0.0;
      if (br > 0 && bc > 0) {
        if (br == bc) {
          a = gn::row_dot(rows + 6 * (r < c ? r : c), u + 6 * (r < c ? c : r));
        } else {
          const int deep = br > bc ? br : bc, top = br > bc ? bc : br;
          int t = deep;
          while (t > top) t = par[t];
          if (t == top) a = gn::row_dot(rows + 6 * (br > bc ? c : r), u + 6 * (br > bc ? r : c));
        }
      }
      double h = (2.0 * a) / ls.n_points;
      if (ls.mu && r == c) h = h + 2.0 * ls.mu[r];
      ls.H[i] = h;
      A[r * ld + c] = h;
    }
  } else if (!accept) {
#pragma unroll
    for (int v = 0; v < (64 * 64 + NT - 1) / NT; ++v) {
      const int i = tid + v * NT;
      if (i < nq * nq) A[(i / nq) * ld + i % nq] = h_old[v];
    }
  }
  if (mine) {  // (the accepted point, for the step)
    xa[tid] = accept ? x0 : xa0;
    if (!accept) L.g[tid] = ga0;
  }
  __syncthreads();
  if (bad || bad_rows) {  // (the evaluation failed: not counted, the accepted state as it was — the host's)
    if (tid == 0) {
      ls.flags[2] = 1;
      ls.flags[0] = 1;
    }
    return;
  }
  if (tid >= 64) return;
  STAMP(4);
  if (mine && accept) {
    ls.xa[tid] = x0;
    ls.g[tid] = L.g[tid];
  }
  // wave 0: the end conditions in fsdf_lm_minimize's order, then the damped step
  const int lane = tid;
  const double gi = mine ? L.g[lane] : 0.0;
  double lam = s_lam, step = 0.0;
  int done = s_end || last;
  if (!done) {
    const double sq = gi * gi;
    double nrm2 = 0.0;
    for (int i = 0; i < nq; ++i) nrm2 += readlane_f64(sq, i);
    if (sqrt(nrm2) < ls.tol) done = 1;
  }
  if (!done) {
    const double hd = mine ? A[lane * ld + lane] : 0.0;
    double hmax = 0.0;
    for (int i = 0; i < nq; ++i) hmax = gn::diag_max(hmax, readlane_f64(hd, i));
    const double floor_d = 1e-12 * hmax;
    STAMP(5);
    for (int raises = 0;; ++raises) {  // (bounded: lambda grows tenfold every turn)
      if (raises > 0) {  // the factor's place holds a failed factorisation: H again
        for (int i = lane; i < nq * nq; i += 64) A[(i / nq) * ld + i % nq] = ls.H[i];
        wave_lds_fence();
      }
      if (lm_wave_step(nq, ld, A, hd, gi, lam, floor_d, ls.max_step, &step, it0)) break;
      lam *= 10.0;
      if (lam > 1e12 || raises >= kLmMaxRaises) {
        done = 1;
        break;
      }
    }
  }
  if (!done && mine) ls.x[(size_t)(count & 1) * nq + lane] = xa[lane] + step;
  if (lane == 0) {
    *ls.lam = lam;
    if (accept) *ls.f = s_f;
    ls.flags[1] = count;
    if (done) ls.flags[0] = 1;
  }
  STAMP(9);
}

// solver_init_kernel's work for a later trial of the LM frame: FK of the x in
// `slot`, the surface poses, this workgroup's pose items, and — workgroup 0 —
// the joint frames into the slot and the error flags (publish()'s, without the
// NaiveSolver's x, f and count).
template <typename TP>
__global__ __launch_bounds__(kStepThreads) void lm_pose_kernel(SolverTree T, SolverState st, LocalModel lm,
                                                               PosedModel pm, int slot) {
  extern __shared__ double lds[];
  constexpr int NT = kStepThreads;
  __shared__ int bad, s_done, nonfinite;
  const int tid = threadIdx.x, nb = T.nb;
  if (tid == 0) {
    s_done = __builtin_nontemporal_load(st.flags);
    bad = 0;
    nonfinite = 0;
  }
  const Lds L = stage<NT, false>(T, st, lds, nullptr, slot);
  __syncthreads();
  if (s_done) return;
  fk<NT>(T, L, &bad);  // (ends with a barrier)
  for (int i = tid; i < 12 * T.S; i += NT) {
    const int k = i / 12, q = i % 12, b = L.sbody[k];
    const double v = b < 0 ? ((q % 4 == 0 && q < 9) ? 1.0 : 0.0)
                           : kin::surface_pose_entry(q, L.R + 9 * b, L.t + 3 * b, L.FR + 9 * k, L.Ft + 3 * k);
    L.P[i] = v;
    if (!isfinite(v)) nonfinite = 1;  // (every writer writes the same value)
  }
  __syncthreads();
  const int item = blockIdx.x * NT + tid;
  if (item < pose_items(lm))
    pose_item<TP>(lm, L.P, (TP*)pm.planes_w, pm.spheres_w, (TP*)pm.verts_w, (TP*)pm.hscale_w,
                  sizeof(TP) == 8 ? pm.screen_w : nullptr, sizeof(TP) == 8 ? (I4*)pm.image_w : nullptr, item);
  if (blockIdx.x != 0) return;
  double* Rb = st.Rb + (size_t)slot * 12 * nb;
  for (int i = tid; i < 9 * nb; i += NT) Rb[i] = L.Rb[i];
  for (int i = tid; i < 3 * nb; i += NT) Rb[9 * nb + i] = L.tb[i];
  if (tid == 0 && (bad || nonfinite)) {
    st.flags[2] = nonfinite ? 2 : 1;
    st.flags[0] = 1;
  }
}

bool extended(const SolverTree& T) { return T.R > 0 || T.n_deform > 0; }

size_t solver_lds_bytes(const SolverTree& T) {
  return (size_t)T.chunks16 * 16 +
         (work_doubles(T.nb, T.nx, T.S) + (extended(T) ? ext_doubles(T.nb, T.rc, T.rm, T.rlu, T.racc) : 0)) *
             sizeof(double);
}

// the most static __shared__ any of the solver kernels declares (the flags and
// sums of step_body / publish), which the 64 KB of a workgroup also hold
size_t solver_static_lds() {
  static size_t cached = 0;
  static bool known = false;
  if (!known) {
    const void* fns[] = {(const void*)solver_init_kernel<double, false>, (const void*)solver_init_kernel<float, false>,
                         (const void*)solver_init_kernel<double, true>,  (const void*)solver_init_kernel<float, true>,
                         (const void*)solver_step_kernel<double, false>, (const void*)solver_step_kernel<float, false>,
                         (const void*)solver_step_kernel<double, true>,  (const void*)solver_step_kernel<float, true>};
    size_t most = 0;
    for (const void* f : fns) {
      hipFuncAttributes a;
      // (a failed query: an allowance above what the kernels declare today)
      const size_t b = hipFuncGetAttributes(&a, f) == hipSuccess ? a.sharedSizeBytes : 256;
      most = b > most ? b : most;
    }
    cached = most;
    known = true;
  }
  return cached;
}

}  // namespace

// the blob (nd doubles + ni ints) within kBlobPer chunks per thread, the
// dynamic loads (the accumulator with its RBF block, Rb | tb, x, divisors)
// within kDynPer, every skin's system within the two rows per lane of the
// solves, the skins' state within stage_rbf's loads, and the whole carve — the LU and work arrays of the skins included —
// with the kernels' static __shared__ within 64 KB of LDS
bool solver_fits(int nb, int nx, int S, int ni, int nd, int n_deform, int R, const int32_t* rbf_n) {
  size_t rc = 0, rm = 0, rlu = 0, racc = 0;
  for (int r = 0; r < R; ++r) {
    const size_t n = (size_t)rbf_n[r], m = n + 4;
    if (m > 128) return false;
    rc += n;
    rm += m;
    rlu += m * m;
    racc += 4 * n + 4;
  }
  const bool ext = R > 0 || n_deform > 0;  // (the EXT kernels' carve)
  const size_t blob = ((size_t)nd * 8 + (size_t)ni * 4 + 15) / 16;
  const size_t dyn = 1 + 6 * (size_t)S + racc + 12 * (size_t)nb + 2 * (size_t)nx;
  const size_t work = work_doubles(nb, nx, S) + (ext ? ext_doubles(nb, (int)rc, (int)rm, (int)rlu, (int)racc) : 0);
  // (stage_rbf: a slot of the weight solve's state in kRbfPer loads per thread, the row map in one)
  const bool stage_rbf_fits =
      9 * (size_t)nb + 3 * rc + rm + rlu <= (size_t)kRbfPer * kStepThreads && rm <= (size_t)kStepThreads;
  return nb >= 1 && blob <= (size_t)kBlobPer * kSolverBlock && dyn <= (size_t)kDynPer * kSolverBlock &&
         stage_rbf_fits && blob * 16 + work * 8 + solver_static_lds() <= 65536;
}

// one workgroup per kStepThreads work items of the pose, each running the whole
// step (the same arithmetic on the same inputs: the same values) and then
// posing its items — the pose in the step's launch, at the latency of one step
static dim3 solver_grid(const LocalModel& lm) {
  const int g = (pose_items(lm) + kStepThreads - 1) / kStepThreads;
  return dim3((unsigned)(g > 0 ? g : 1));
}

hipError_t launch_solver_init(const SolverTree& T, const SolverState& st, const LocalModel& lm,
                              const PosedModel& pm, int precision, hipStream_t s) {
  const dim3 g = solver_grid(lm), b(kStepThreads);
  const size_t lds = solver_lds_bytes(T);
  if (extended(T)) {
    if (precision == 64) hipLaunchKernelGGL((solver_init_kernel<double, true>), g, b, lds, s, T, st, lm, pm);
    else hipLaunchKernelGGL((solver_init_kernel<float, true>), g, b, lds, s, T, st, lm, pm);
  } else {
    if (precision == 64) hipLaunchKernelGGL((solver_init_kernel<double, false>), g, b, lds, s, T, st, lm, pm);
    else hipLaunchKernelGGL((solver_init_kernel<float, false>), g, b, lds, s, T, st, lm, pm);
  }
  return hipGetLastError();
}

void solver_times(unsigned long long* out) {
#if FSDF_SOLVER_TIMES
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_solver_times), 16 * sizeof(unsigned long long));
#else
  for (int i = 0; i < 16; ++i) out[i] = 0;
#endif
}

hipError_t launch_solver_step(const SolverTree& T, const SolverState& st, const double* d_accum,
                              const LocalModel& lm, const PosedModel& pm, int precision, int it_before,
                              hipStream_t s) {
  const dim3 g = solver_grid(lm), b(kStepThreads);
  const size_t lds = solver_lds_bytes(T);
  if (extended(T)) {
    if (precision == 64)
      hipLaunchKernelGGL((solver_step_kernel<double, true>), g, b, lds, s, T, st, d_accum, lm, pm, it_before);
    else hipLaunchKernelGGL((solver_step_kernel<float, true>), g, b, lds, s, T, st, d_accum, lm, pm, it_before);
  } else {
    if (precision == 64)
      hipLaunchKernelGGL((solver_step_kernel<double, false>), g, b, lds, s, T, st, d_accum, lm, pm, it_before);
    else hipLaunchKernelGGL((solver_step_kernel<float, false>), g, b, lds, s, T, st, d_accum, lm, pm, it_before);
  }
  return hipGetLastError();
}

// the LM step's carve with lm_step_kernel's static __shared__ within 64 KB; a
// matrix row per lane of one wave; the staging's loads per thread
bool lm_solver_fits(int nb, int nq, int S) {
  static size_t fixed = 0;
  static bool known = false;
  if (!known) {
    hipFuncAttributes a;
    // (a failed query: an allowance above what the kernel declares today)
    fixed = hipFuncGetAttributes(&a, (const void*)lm_step_kernel) == hipSuccess ? a.sharedSizeBytes : 256;
    known = true;
  }
  return nb >= 1 && nq >= 1 && nq <= 64 && 1 + 6 * (size_t)S <= (size_t)kLmThreads &&
         12 * (size_t)nb <= 2 * (size_t)kLmThreads && lm_work_doubles(nb, nq, S) * 8 + fixed <= 65536;
}

hipError_t launch_lm_step(const SolverTree& T, const LmState& ls, const double* d_accum, const double* d_moments,
                          int it_before, hipStream_t s) {
  hipLaunchKernelGGL(lm_step_kernel, dim3(1), dim3(kLmThreads), lm_work_doubles(T.nb, T.nq, T.S) * sizeof(double), s,
                     T, ls, d_accum, d_moments, it_before);
  return hipGetLastError();
}

hipError_t launch_lm_pose(const SolverTree& T, const LmState& ls, const LocalModel& lm, const PosedModel& pm,
                          int precision, int slot, hipStream_t s) {
  SolverState st;
  st.x = ls.x;
  st.Rb = ls.Rb;
  st.flags = ls.flags;
  const dim3 g = solver_grid(lm), b(kStepThreads);
  const size_t lds = solver_lds_bytes(T);
  if (precision == 64) hipLaunchKernelGGL(lm_pose_kernel<double>, g, b, lds, s, T, st, lm, pm, slot);
  else hipLaunchKernelGGL(lm_pose_kernel<float>, g, b, lds, s, T, st, lm, pm, slot);
  return hipGetLastError();
}

}  // namespace fsdf
