// lm_solver.hip — the device Levenberg-Marquardt loop (fsdf_descend_lm,
// fsdf_set_lm_solver; descend.hip descend_lm_device enqueues it).
// After every evaluation (pass, reduce, moments, their reduce) one single-
// workgroup launch, lm_step_kernel, does what fsdf_lm_minimize does between two
// calls of its objective, in the host's order and with gn_impl.h's arithmetic:
//   objective   the chain rule of the NaiveSolver step (solver_common.h); f_t =
//               c / N, g / N (+ the prior of fsdf_set_lm_prior, descend.hip
//               lm_objective's operations)
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
// and a second launch, lm_pose_kernel (the rigid solver_init_kernel's body on
// that slot, solver_common.h pose_body: FK, the joint frames, the posed
// model), prepares the next pass. The solve in
// a launch of one workgroup keeps the matrix, the factor and the subtree
// moments out of the many-workgroup pose launch, whose carve (the tree blob in
// LDS) fills most of 64 KB at M64; here the tree is read from global memory
// (L2) and the carve is acc | Rb tb | x | own | sub | g | xa | pe | C [nb][36] |
// rows [nq][6] | u [nq][6] | L [nq][nq | 1] | the coordinates' bodies | the parents: 60 KB at
// M64 (65 bodies, 48 coordinates, 64 surfaces).
#include <hip/hip_runtime.h>

#include "gn_impl.h"
#include "solver_common.h"

namespace fsdf {

namespace {

constexpr int kLmThreads = 1024;
constexpr int kLmMaxRaises = 400;  // tenfold raises from the smallest positive double pass 1e12 in 336

__host__ __device__ inline int lm_ld(int nq) { return nq | 1; }  // (odd row stride: the lanes' rows in different banks)

// The step's LDS, walked once: the doubles it takes, and with PTRS the pointers
// from `base`. The staging relies on Rb | tb being contiguous, as in a slot.
struct LmWork {
  double *acc, *Rb, *tb, *x, *own, *sub, *g, *xa, *pe, *C, *rows, *u, *A;
  int32_t *cbody, *par;
};
template <bool PTRS>
__host__ __device__ inline size_t lm_carve(int nb, int nq, int S, double* base, LmWork& W) {
  size_t o = 0;
  auto take = [&](double*& p, size_t count) {
    if constexpr (PTRS) p = base + o;
    o += count;
  };
  double* ints = nullptr;
  take(W.acc, 1 + 6 * (size_t)S);
  take(W.Rb, 9 * (size_t)nb);
  take(W.tb, 3 * (size_t)nb);
  take(W.x, nq);
  take(W.own, 6 * (size_t)nb);  // subtree_wrenches' scratch
  take(W.sub, 6 * (size_t)nb);
  take(W.g, nq);
  take(W.xa, nq);                     // the accepted x
  take(W.pe, nq);                     // the prior's terms mu_i e_i^2
  take(W.C, 36 * (size_t)nb);         // [nb][36] subtree moments
  take(W.rows, 6 * (size_t)nq);       // [nq][6] motion rows
  take(W.u, 6 * (size_t)nq);          // [nq][6] C_b s_j
  take(W.A, (size_t)nq * lm_ld(nq));  // [nq][ld] H, then its factor
  take(ints, ((size_t)nq + (size_t)nb + 1) / 2);
  if constexpr (PTRS) {
    W.cbody = (int32_t*)ints;  // [nq] the body whose joint owns the coordinate (-1: none)
    W.par = W.cbody + nq;      // [nb] the tree's parents (the matrix entries' ancestor walks)
  }
  return o;
}
inline size_t lm_doubles(int nb, int nq, int S) {
  LmWork w;
  return lm_carve<false>(nb, nq, S, nullptr, w);
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
                             double max_step, double* step, int it) {  // (it: the evaluation, for the phase clocks)
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
  STAMP(6, it);
  double y = in ? g : 0.0;
  for (int k = 0; k < n; ++k) {  // L y = g, column by column: every row's terms in ascending k
    const double lkk = A[k * ld + k];
    if (lane == k) y = y / lkk;
    const double yk = readlane_f64(y, k);
    if (in && lane > k) y = gn::minus_product(y, row[k], yk);
  }
  STAMP(7, it);
  for (int i = n - 1; i >= 0; --i) {  // Lᵀ z = y: the products in the lanes k > i, subtracted in ascending k
    const double p = in && lane > i ? row[i] * y : 0.0;
    double s = readlane_f64(y, i);
    for (int k = i + 1; k < n; ++k) s = s - readlane_f64(p, k);
    s = s / A[i * ld + i];
    if (lane == i) y = s;
  }
  STAMP(8, it);
  if (__builtin_amdgcn_ballot_w64(in && !isfinite(y)) != 0) return false;
  *step = gn::clamped_step(y, max_step);
  return true;
}


// ---- the step's phases (lm_step_kernel below is their sequence) ---------------
constexpr int kLmHPer = (64 * 64 + kLmThreads - 1) / kLmThreads;  // H entries per thread (nq <= 64)

// the workgroup's flags and sums (bad: the chain rule's failures, read by every
// thread before the matrix phase; bad_rows: that phase's own)
struct LmShared {
  int done, bad, bad_rows, accept, end;
  double f, lam;
};

// what a thread keeps in registers from the staging on: its coordinate's (tid <
// nq) trial x0, accepted xa0 / ga0, prior weight mu0 and reference xr0, and the
// accepted H's entries tid + v NT (a rejected trial puts them back)
struct LmStaged {
  double x0, xa0, ga0, mu0, xr0;
  double h_old[kLmHPer];
};

// Staging into the carve: every thread's loads before its first store
// (stage()); na <= NT, nr <= 2 NT, nq <= 64 (lm_solver_fits). No barrier.
template <int NT>
__device__ __forceinline__ void lm_stage(const SolverTree& T, const LmState& ls, const TreeView& V, const LmWork& W,
                                         const double* __restrict__ accum, int it_before, LmStaged& r) {
  const int tid = threadIdx.x, nb = T.nb, nq = T.nq;
  const int na = 1 + 6 * T.S, nr = 12 * nb;
  const int slot = it_before & 1;
  const double* rsrc = ls.Rb + (size_t)slot * nr;
  const bool mine = tid < nq, later = it_before > 0;
  const double a0 = tid < na ? accum[tid] : 0.0;
  const double r0 = tid < nr ? rsrc[tid] : 0.0, r1 = tid + NT < nr ? rsrc[tid + NT] : 0.0;
  r.x0 = mine ? ls.x[(size_t)slot * nq + tid] : 0.0;
  r.xa0 = mine && later ? ls.xa[tid] : 0.0;
  r.ga0 = mine && later ? ls.g[tid] : 0.0;
  r.mu0 = mine && ls.mu ? ls.mu[tid] : 0.0;
  r.xr0 = mine && ls.mu ? ls.x_ref[tid] : 0.0;
#pragma unroll
  for (int v = 0; v < kLmHPer; ++v) {
    const int i = tid + v * NT;
    r.h_old[v] = later && i < nq * nq ? ls.H[i] : 0.0;
  }
  if (tid < na) W.acc[tid] = a0;
  if (tid < nr) W.Rb[tid] = r0;  // (Rb | tb adjacent, as in a slot)
  if (tid + NT < nr) W.Rb[tid + NT] = r1;
  if (mine) {
    W.x[tid] = r.x0;
    W.g[tid] = 0.0;
    W.cbody[tid] = -1;
    const double e = r.x0 - r.xr0;
    W.pe[tid] = r.mu0 * (e * e);
  }
  for (int i = tid; i < 6 * nq; i += NT) W.rows[i] = 0.0;
  for (int i = tid; i < nb; i += NT) W.par[i] = V.parent[i];
}

// The wrapped objective at the trial (descend.hip lm_objective) and, thread 0,
// the verdict into sh: accept, the damping after it, the end beyond 1e12, f.
__device__ __forceinline__ void lm_verdict(const SolverTree& T, const LmState& ls, const LmWork& W,
                                           const LmStaged& r, bool later, LmShared& sh) {
  const int tid = threadIdx.x, nq = T.nq;
  if (tid < nq) {
    double gi = W.g[tid] / ls.n_points;
    if (ls.mu) gi = gi + (2.0 * r.mu0) * (r.x0 - r.xr0);
    W.g[tid] = gi;
  }
  if (tid == 0) {
    const double cost = W.acc[0] + ls.weight * 0.0;  // (iteration_finish: the regularizer's sum is 0.0)
    double ft = cost / ls.n_points;
    if (ls.mu) {
      double s = 0.0;
      for (int i = 0; i < nq; ++i) s += W.pe[i];
      ft = ft + s;
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
    sh.f = accept ? ft : f;
    sh.lam = lam;
    sh.accept = accept;
    sh.end = end;
  }
}

// The Gauss-Newton matrix at the trial (fsdf_gauss_newton_matrix): per-body
// moments, surfaces in index order, and the motion rows; the subtree sums by
// height; u; then one entry per thread into ls.H and W.A. Barriers between its
// parts, none after the entries.
template <int NT>
__device__ __forceinline__ void lm_matrix(const SolverTree& T, const LmState& ls, const TreeView& V, const LmWork& W,
                                          const double* __restrict__ moments, LmShared& sh) {
  const int tid = threadIdx.x, nb = T.nb, nq = T.nq, ld = lm_ld(nq);
  for (int i = tid; i < 36 * (nb - 1); i += NT) {
    const int b = 1 + i / 36, e = i % 36, t = gn::tri_index(e / 6, e % 6);
    double s = 0.0;
    for (int q = V.soff[b]; q < V.soff[b + 1]; ++q) s += moments[kMomentsLen * V.slist[q] + t];
    W.C[36 * b + e] = s;
  }
  for (int b = 1 + tid; b < nb; b += NT) {
    const int k = V.kind[b], w = gn::joint_width(k), q0 = V.qoff[b];
    if (!w) continue;
    if (!gn::joint_rows(k, V.axis + 3 * b, W.Rb + 9 * b, W.tb + 3 * b, W.x + q0, W.rows + 6 * q0))
      atomicOr(&sh.bad_rows, 1);
    for (int e = 0; e < w; ++e) W.cbody[q0 + e] = b;
  }
  __syncthreads();
  // subtree sums: parents by height, children in descending index
  for (int h = 0; h < T.H; ++h) {
    const int a = V.hoff[h], e = V.hoff[h + 1];
    for (int i = tid; i < 36 * (e - a); i += NT) {
      const int p = V.hord[a + i / 36], j = i % 36;
      double s = W.C[36 * p + j];
      for (int q = V.coff[p]; q < V.coff[p + 1]; ++q) s += W.C[36 * V.clist[q] + j];
      W.C[36 * p + j] = s;
    }
    __syncthreads();
  }
  for (int i = tid; i < 6 * nq; i += NT) {
    const int c = i / 6, b = W.cbody[c];
    W.u[i] = b > 0 ? gn::moment_row(W.C + 36 * b, W.rows + 6 * c, i % 6) : 0.0;
  }
  __syncthreads();
  // one entry per thread: coordinate i against j when i's body is j's, or
  // an ancestor of it (a parent's index is below its child's)
  for (int i = tid; i < nq * nq; i += NT) {
    const int r = i / nq, c = i % nq, br = W.cbody[r], bc = W.cbody[c];
    double a = 0.0;
    if (br > 0 && bc > 0) {
      if (br == bc) {
        a = gn::row_dot(W.rows + 6 * (r < c ? r : c), W.u + 6 * (r < c ? c : r));
      } else {
        const int deep = br > bc ? br : bc, top = br > bc ? bc : br;
        int t = deep;
        while (t > top) t = W.par[t];
        if (t == top) a = gn::row_dot(W.rows + 6 * (br > bc ? c : r), W.u + 6 * (br > bc ? r : c));
      }
    }
    double h = (2.0 * a) / ls.n_points;
    if (ls.mu && r == c) h = h + 2.0 * ls.mu[r];
    ls.H[i] = h;
    W.A[r * ld + c] = h;
  }
}

// a rejected trial: the accepted H into the factor's place
template <int NT>
__device__ __forceinline__ void lm_restore_H(int nq, double* A, const LmStaged& r) {
  const int tid = threadIdx.x, ld = lm_ld(nq);
#pragma unroll
  for (int v = 0; v < kLmHPer; ++v) {
    const int i = tid + v * NT;
    if (i < nq * nq) A[(i / nq) * ld + i % nq] = r.h_old[v];
  }
}

// Wave 0 after a good evaluation: the accepted x and g kept in global memory,
// the end conditions in fsdf_lm_minimize's order, then the damped step (a
// degenerate factorisation raises the damping and factors H again), the next
// trial into the other slot, and — lane 0 — the damping, f, the count and the
// done flag.
__device__ __forceinline__ void lm_wave0_end(const SolverTree& T, const LmState& ls, const LmWork& W,
                                             const LmStaged& r, const LmShared& sh, int it_before) {
  const int lane = threadIdx.x, nq = T.nq, ld = lm_ld(nq), count = it_before + 1;
  const bool mine = lane < nq, accept = sh.accept != 0, last = count >= ls.limit;
  STAMP(4, it_before);
  if (mine && accept) {
    ls.xa[lane] = r.x0;
    ls.g[lane] = W.g[lane];
  }
  const double gi = mine ? W.g[lane] : 0.0;
  double lam = sh.lam, step = 0.0;
  int done = sh.end || last;
  if (!done) {
    const double sq = gi * gi;
    double nrm2 = 0.0;
    for (int i = 0; i < nq; ++i) nrm2 += readlane_f64(sq, i);
    if (sqrt(nrm2) < ls.tol) done = 1;
  }
  if (!done) {
    const double hd = mine ? W.A[lane * ld + lane] : 0.0;
    double hmax = 0.0;
    for (int i = 0; i < nq; ++i) hmax = gn::diag_max(hmax, readlane_f64(hd, i));
    const double floor_d = 1e-12 * hmax;
    STAMP(5, it_before);
    for (int raises = 0;; ++raises) {  // (bounded: lambda grows tenfold every turn)
      if (raises > 0) {  // the factor's place holds a failed factorisation: H again
        for (int i = lane; i < nq * nq; i += 64) W.A[(i / nq) * ld + i % nq] = ls.H[i];
        wave_lds_fence();
      }
      if (lm_wave_step(nq, ld, W.A, hd, gi, lam, floor_d, ls.max_step, &step, it_before)) break;
      lam *= 10.0;
      if (lam > 1e12 || raises >= kLmMaxRaises) {
        done = 1;
        break;
      }
    }
  }
  if (!done && mine) ls.x[(size_t)(count & 1) * nq + lane] = W.xa[lane] + step;
  if (lane == 0) {
    *ls.lam = lam;
    if (accept) *ls.f = sh.f;
    ls.flags[1] = count;
    if (done) ls.flags[0] = 1;
  }
  STAMP(9, it_before);
}

// (phase clocks, 10 ns: 1 staged, 2 chain rule, 3 verdict, 4 matrix, 5 end checks, 6 factor, 7 forward solve,
// 8 back-substitution, 9 end)
__global__ __launch_bounds__(kLmThreads) void lm_step_kernel(SolverTree T, LmState ls,
                                                             const double* __restrict__ accum,
                                                             const double* __restrict__ moments, int it_before) {
  extern __shared__ double lds[];
  constexpr int NT = kLmThreads;
  __shared__ LmShared sh;
  const int tid = threadIdx.x, nq = T.nq;
  const bool later = it_before > 0;
  STAMP(0, it_before);
  if (tid == 0) {
    sh.done = __builtin_nontemporal_load(ls.flags);
    sh.bad = 0;
    sh.bad_rows = 0;
  }
  // the tree from global memory; the work arrays in LDS
  const TreeView V = tree_view(T, (const double*)T.blob);
  LmWork W;
  lm_carve<true>(T.nb, nq, T.S, lds, W);
  LmStaged r;
  lm_stage<NT>(T, ls, V, W, accum, it_before, r);
  __syncthreads();
  if (sh.done) return;  // the frame has ended: its remaining launches are no-ops (workgroup-uniform)
  STAMP(1, it_before);
  chain_rule<NT>(T, V, W.acc, nullptr, W.own, W.sub, W.Rb, W.tb, W.x, W.g, &sh.bad);  // (ends with a barrier)
  STAMP(2, it_before);
  lm_verdict(T, ls, W, r, later, sh);
  __syncthreads();
  STAMP(3, it_before);
  const bool accept = sh.accept != 0, last = it_before + 1 >= ls.limit;
  if (accept && !last && !sh.bad) lm_matrix<NT>(T, ls, V, W, moments, sh);
  else if (!accept) lm_restore_H<NT>(nq, W.A, r);
  if (tid < nq) {  // (the accepted point, for the step)
    W.xa[tid] = accept ? r.x0 : r.xa0;
    if (!accept) W.g[tid] = r.ga0;
  }
  __syncthreads();
  if (sh.bad || sh.bad_rows) {  // (the evaluation failed: not counted, the accepted state as it was — the host's)
    if (tid == 0) {
      ls.flags[2] = 1;
      ls.flags[0] = 1;
    }
    return;
  }
  if (tid >= 64) return;
  lm_wave0_end(T, ls, W, r, sh, it_before);
}

template <typename TP>
__global__ __launch_bounds__(kStepThreads) void lm_pose_kernel(SolverTree T, SolverState st, LocalModel lm,
                                                               PosedModel pm, int slot) {
  extern __shared__ double lds[];
  pose_body<TP, true>(T, st, lm, pm, slot, lds);
}

}  // namespace

// the LM step's carve with lm_step_kernel's static __shared__ within 64 KB; a
// matrix row per lane of one wave; the staging's loads per thread; and the
// pose kernel's LDS — the blob (nd doubles + ni ints), the rigid step's carve
// and its own static __shared__ — within 64 KB too
bool lm_solver_fits(int nb, int nq, int S, int ni, int nd) {
  static size_t step_fixed = 0, pose_fixed = 0;
  static bool known = false;
  if (!known) {
    step_fixed = static_lds((const void*)lm_step_kernel);
    const size_t p64 = static_lds((const void*)lm_pose_kernel<double>), p32 = static_lds((const void*)lm_pose_kernel<float>);
    pose_fixed = p64 > p32 ? p64 : p32;
    known = true;
  }
  const size_t blob = ((size_t)nd * 8 + (size_t)ni * 4 + 15) / 16;
  const size_t pose = blob * 16 + step_doubles(StepDims{nb, nq, S, false, 0, 0, 0, 0}) * 8 + pose_fixed;
  return nb >= 1 && nq >= 1 && nq <= 64 && 1 + 6 * (size_t)S <= (size_t)kLmThreads &&
         12 * (size_t)nb <= 2 * (size_t)kLmThreads && lm_doubles(nb, nq, S) * 8 + step_fixed <= 65536 && pose <= 65536;
}

void lm_solver_times(unsigned long long* out) { read_solver_times(out); }

hipError_t launch_lm_step(const SolverTree& T, const LmState& ls, const double* d_accum, const double* d_moments,
                          int it_before, hipStream_t s) {
  hipLaunchKernelGGL(lm_step_kernel, dim3(1), dim3(kLmThreads), lm_doubles(T.nb, T.nq, T.S) * sizeof(double), s, T, ls,
                     d_accum, d_moments, it_before);
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
