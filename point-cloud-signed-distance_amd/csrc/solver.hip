// solver.hip — estimate_state's solver iteration on the device: after a
// residual pass and its reduce, one launch turns
// the accumulator into the next configuration, the next surface poses and the
// next pass's posed model, so a whole frame of iterations is enqueued with no
// host round trip (fsdf_descend, descend.hip descend_device; the default for
// rigid scenes, fsdf_set_solver).
//
// Per iteration, the arithmetic of the host loop (descend.hip fsdf_descend around
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
// What this loop shares with fsdf_descend_lm's device loop (lm_solver.hip) —
// the tree view, the LDS carve, the staging, the FK, the chain rule, the end
// of a pose launch — is in solver_common.h; the skins' half in solver_rbf.h.
#include "solver_common.h"
#include "solver_rbf.h"

namespace fsdf {

namespace {

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
    pose_tail<TP, NT>(T, L, lm, pm, &nonfinite);
  }
  if (wg != 0) return;  // (the state: workgroup 0; every workgroup computed the same values)
  if (pose) store_joint_frames<NT>(T, L, st.Rb, slot);
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

template <typename TP, bool EXT>
__global__ __launch_bounds__(kStepThreads) void solver_init_kernel(SolverTree T, SolverState st, LocalModel lm,
                                                                   PosedModel pm) {
  extern __shared__ double lds[];
  if constexpr (!EXT) {
    pose_body<TP, false>(T, st, lm, pm, 0, lds);  // (x0 in slot 0; the host zeroed the flags before this launch)
  } else {
    __shared__ int bad, sing;
    if (threadIdx.x == 0) {
      bad = 0;
      sing = 0;
    }
    const Lds L = stage<kStepThreads, true>(T, st, lds, nullptr, 0);
    __syncthreads();
    fk<kStepThreads>(T, L, &bad, -1);  // (ends with a barrier)
    if (T.R > 0) rbf_prepare<kStepThreads>(T, L, &sing);  // (ends with a barrier)
    publish<TP, kStepThreads, true>(T, st, L, true, bad, 0.0, 0, 0, lm, pm, sing);
  }
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
  const int tid = threadIdx.x, nx = T.nx;
  if (tid == 0) s_done = __builtin_nontemporal_load(st.flags);
  STAMP(0, it_before);
  if (tid == 0) {
    bad = 0;
    if (EXT) sing = 0;
  }
  const Lds L = stage<NT, EXT>(T, st, lds, accum, it_before & 1);
  if (EXT && T.R > 0) stage_rbf<NT>(T, st, L, it_before & 1);
  __syncthreads();
  if (s_done) return;  // converged (or failed): the frame's remaining steps are no-ops (workgroup-uniform)
  STAMP(1, it_before);
  const bool skins = EXT && T.R > 0;
  if (EXT) rbf_adjoint<NT>(T, st, L, &s_reg);  // (ends with a barrier)
  // (own: L.LR, free until the FK; ends with a barrier)
  chain_rule<NT>(T, L, L.acc, skins ? L.bw : nullptr, L.LR, L.sub, L.Rb, L.tb, L.x, L.g, &bad);
  STAMP(2, it_before);
  for (int i = tid; i < nx; i += NT) {
    double gi = L.g[i] / st.n_points;
    if (L.div) gi = gi / L.div[i];
    L.g[i] = gi;
  }
  __syncthreads();
  STAMP(3, it_before);
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
  STAMP(4, it_before);
  fk<NT>(T, L, &bad, it_before);  // (ends with a barrier)
  STAMP(6, it_before);
  if (skins) rbf_prepare<NT>(T, L, &sing);  // (ends with a barrier)
  publish<TP, NT, EXT>(T, st, L, true, bad, f, it, 0, lm, pm, EXT ? sing : 0);
  STAMP(9, it_before);
}

template <typename TP, bool EXT>
__global__ __launch_bounds__(kStepThreads) void solver_step_kernel(SolverTree T, SolverState st,
                                                                   const double* __restrict__ accum, LocalModel lm,
                                                                   PosedModel pm, int it_before) {
  extern __shared__ double lds[];
  step_body<TP, kStepThreads, EXT>(T, st, accum, lds, lm, pm, it_before);
}

// the most static __shared__ any of this loop's kernels declares (the flags and
// sums of step_body / publish / pose_body), which the 64 KB of a workgroup also
// hold (the LM loop's kernels: lm_solver_fits)
size_t solver_static_lds() {
  static size_t cached = 0;
  static bool known = false;
  if (!known) {
    const void* fns[] = {(const void*)solver_init_kernel<double, false>, (const void*)solver_init_kernel<float, false>,
                         (const void*)solver_init_kernel<double, true>,  (const void*)solver_init_kernel<float, true>,
                         (const void*)solver_step_kernel<double, false>, (const void*)solver_step_kernel<float, false>,
                         (const void*)solver_step_kernel<double, true>,  (const void*)solver_step_kernel<float, true>};
    for (const void* f : fns) cached = static_lds(f) > cached ? static_lds(f) : cached;
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
  const size_t work = step_doubles(StepDims{nb, nx, S, ext, (int)rc, (int)rm, (int)rlu, (int)racc});
  // (stage_rbf: a slot of the weight solve's state in kRbfPer loads per thread, the row map in one)
  const bool stage_rbf_fits =
      9 * (size_t)nb + 3 * rc + rm + rlu <= (size_t)kRbfPer * kStepThreads && rm <= (size_t)kStepThreads;
  return nb >= 1 && blob <= (size_t)kBlobPer * kSolverBlock && dyn <= (size_t)kDynPer * kSolverBlock &&
         stage_rbf_fits && blob * 16 + work * 8 + solver_static_lds() <= 65536;
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

void solver_times(unsigned long long* out) { read_solver_times(out); }

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

}  // namespace fsdf
