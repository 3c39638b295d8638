// solver_common.h — what the device solver loops share (solver.hip: the
// NaiveSolver init / step kernels; lm_solver.hip: the Levenberg-Marquardt step
// and pose kernels): the view of the tree blob, the carves of the kernels'
// LDS, the staging, the FK, the chain rule and the end of a pose launch.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fsdf_internal.h"
#include "kin_impl.h"
#include "pose_impl.h"

namespace fsdf {

namespace {

// kSolverBlock: the unit the staging capacities are counted in (kBlobPer /
// kDynPer per thread of a 256-thread group); kStepThreads: the kernels'
// width. 16 waves run the step's per-(body, component) loops in one round
// (6 (nb - 1) = 384 for M64) and publish the 12 S pose entries in one round:
// the M64 step 15.8 -> 12.6 us against 4 waves (profiles/r06/solver_nt/)
constexpr int kSolverBlock = 256;
constexpr int kStepThreads = 1024;

// diagnostic builds (-DFSDF_SOLVER_TIMES=1): workgroup 0's clock at phase i of
// iteration / evaluation 5, one table per translation unit (solver_times,
// lm_solver_times). The default build's STAMP does not evaluate its arguments.
#if FSDF_SOLVER_TIMES
__device__ unsigned long long g_solver_times[64];
#define STAMP(i, it) \
  if (threadIdx.x == 0 && blockIdx.x == 0 && (it) == 5) g_solver_times[i] = wall_clock64()
#else
#define STAMP(i, it)
#endif
inline void read_solver_times(unsigned long long* out) {  // (this translation unit's table: 16 slots)
#if FSDF_SOLVER_TIMES
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_solver_times), 16 * sizeof(unsigned long long));
#else
  for (int i = 0; i < 16; ++i) out[i] = 0;
#endif
}

// what a kernel declares as static __shared__ (a failed query: an allowance above what they declare today)
inline size_t static_lds(const void* kernel) {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, kernel) == hipSuccess ? a.sharedSizeBytes : 256;
}

// The mechanism's arrays in the tree blob (SolverTree: doubles [nd], ints [ni],
// padded to 16 B), the RBF skins' included: pointers from one base, the blob's
// copy in LDS (stage()) or the blob itself in global memory (the LM step).
struct TreeView {
  const double *axis, *AR, *At, *BR, *Bt, *FR, *Ft;
  const int32_t *parent, *kind, *qoff, *plist, *poff, *hord, *hoff, *coff, *clist, *soff, *slist, *sbody;
  const int32_t *chlist, *choff;
  const double *rlocal, *rvalues;
  const int32_t *rn, *rcoff, *rluoff, *rbody, *rdrow;
};

__device__ __forceinline__ TreeView tree_view(const SolverTree& T, const double* base) {
  const int32_t* iv = (const int32_t*)(base + T.nd);
  TreeView V;
  V.axis = base + T.axis;
  V.AR = base + T.AR;
  V.At = base + T.At;
  V.BR = base + T.BR;
  V.Bt = base + T.Bt;
  V.FR = base + T.frame_R;
  V.Ft = base + T.frame_t;
  V.parent = iv + T.parent;
  V.kind = iv + T.kind;
  V.qoff = iv + T.qoff;
  V.plist = iv + T.path_list;
  V.poff = iv + T.path_off;
  V.hord = iv + T.height_order;
  V.hoff = iv + T.height_off;
  V.coff = iv + T.child_off;
  V.clist = iv + T.child_list;
  V.soff = iv + T.surf_off;
  V.slist = iv + T.surf_list;
  V.sbody = iv + T.surface_body;
  V.chlist = iv + T.chain_list;
  V.choff = iv + T.chain_off;
  V.rlocal = base + T.rbf_local;
  V.rvalues = base + T.rbf_values;
  V.rn = iv + T.rbf_n;
  V.rcoff = iv + T.rbf_coff;
  V.rluoff = iv + T.rbf_luoff;
  V.rbody = iv + T.rbf_body;
  V.rdrow = iv + T.rbf_drow;
  return V;
}

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
struct StepWork {
  double *acc, *Rb, *tb, *x, *div, *sub, *LR, *Lt, *R, *t, *g, *P;
  double *cen = nullptr, *u = nullptr, *lu = nullptr, *mu = nullptr, *G = nullptr, *bw = nullptr;
  int32_t* prow = nullptr;
};
struct Lds : TreeView, StepWork {};

// what the step's carve is sized by; ext: the EXT kernels' (R > 0 or n_deform > 0)
struct StepDims {
  int nb, nx, S;
  bool ext;
  int rc, rm, rlu, racc;
};
__host__ __device__ inline bool extended(const SolverTree& T) { return T.R > 0 || T.n_deform > 0; }
__host__ __device__ inline StepDims step_dims(const SolverTree& T, bool ext) {
  return StepDims{T.nb, T.nx, T.S, ext, T.rc, T.rm, T.rlu, T.racc};
}

// The step's work arrays after the blob, walked once: the doubles they take,
// and with PTRS the pointers from `base` (the first double after the blob).
// stage() relies on acc | Rb | tb | x | div being contiguous, stage_rbf() and
// publish() on cen | u | lu.
template <bool PTRS>
__host__ __device__ inline size_t step_carve(const StepDims& n, double* base, StepWork& W) {
  // (the kernels bump a pointer by int counts — a carve that fits is below 8,192 doubles —, the host sums size_t)
  using Count = std::conditional_t<PTRS, int, size_t>;
  const Count nb = n.nb, nx = n.nx, S = n.S, rc = n.rc, rm = n.rm;
  size_t o = 0;
  auto take = [&](double*& p, Count count) {
    if constexpr (PTRS) {
      p = base;
      base += count;
    }
    o += (size_t)count;
  };
  take(W.acc, 1 + 6 * S + (n.ext ? (Count)n.racc : 0));  // (EXT: the RBF block follows the surface wrenches)
  take(W.Rb, 9 * nb);
  take(W.tb, 3 * nb);
  take(W.x, nx);
  take(W.div, nx);
  take(W.sub, 6 * nb);
  take(W.LR, 9 * nb);
  take(W.Lt, 3 * nb);
  take(W.R, 9 * nb);
  take(W.t, 3 * nb);
  take(W.g, nx);
  take(W.P, 12 * S);
  if (n.ext) {
    double* prow = nullptr;
    take(W.cen, 3 * rc);
    take(W.u, rm);
    take(W.lu, (Count)n.rlu);
    take(W.mu, rm);
    take(W.G, 3 * rc);
    take(W.bw, 6 * nb);
    take(prow, (rm + 1) / 2);  // (rm ints)
    if constexpr (PTRS) W.prow = (int32_t*)prow;
  }
  return o;
}
inline size_t step_doubles(const StepDims& n) {
  StepWork w;
  return step_carve<false>(n, nullptr, w);
}

// the dynamic LDS of the init / step / LM pose kernels: the blob, then the carve
inline size_t solver_lds_bytes(const SolverTree& T) {
  return (size_t)T.chunks16 * 16 + step_doubles(step_dims(T, extended(T))) * sizeof(double);
}

// one workgroup per kStepThreads work items of the pose, each running the whole
// step (the same arithmetic on the same inputs: the same values) and then
// posing its items — the pose in the step's launch, at the latency of one step
inline dim3 solver_grid(const LocalModel& lm) {
  const int g = (pose_items(lm) + kStepThreads - 1) / kStepThreads;
  return dim3((unsigned)(g > 0 ? g : 1));
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
  D2* l2 = (D2*)lds;
#pragma unroll
  for (int u = 0; u < BP; ++u) {
    const int i = tid + u * NT;
    if (i < T.chunks16) l2[i] = bv[u];
  }
  static_cast<TreeView&>(L) = tree_view(T, lds);
  step_carve<true>(step_dims(T, EXT), lds + 2 * T.chunks16, L);  // (after the blob, padded to 16 B)
  if (!st.div) L.div = nullptr;
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

// FK of L.x into L.R, t, Rb, tb (LDS; *bad |= 1 for a zero quaternion /
// unknown joint). Global memory is not touched: a workgroup barrier after a
// global store waits for the store to complete (its release fence), so every
// store of the step is issued after the last barrier (publish()).
template <int NT>
__device__ void fk(const SolverTree& T, const Lds& L, int* bad, int it) {  // (it: the iteration, for the phase clocks)
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
  STAMP(5, it);
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

// The chain rule's subtree wrenches: per body its surfaces' accumulator rows in
// index order (from the RBF chain's body wrench with skins), then the subtree
// sums, children in descending index — fsdf_config_gradient's additions in its
// order — into sub [nb][6]. acc: the pass's accumulator; bw: the RBF chain's
// body wrenches [nb][6], or null; own: scratch [nb][6]. Ends with a barrier.
template <int NT>
__device__ void subtree_wrenches(const SolverTree& T, const TreeView& L, const double* acc, const double* bw,
                                 double* own, double* sub) {
  const int tid = threadIdx.x, nb = T.nb;
  if (T.chains) {
    // chains (every non-root body has <= 1 child): body b's subtree sum along
    // its chain, deepest first — sub[a] = own[a] + sub[child], own[a] the body's
    // surfaces summed in index order from 0.0: fsdf_config_gradient's additions
    // in its order, no level barriers. First every own[a] (one thread per (a,
    // component)), then one thread per (b,
    // component) walks its chain, the next four own[] loads issued before
    // their additions (a chain level costs an addition, not a chain of
    // dependent LDS loads)
    for (int i = tid; i < 6 * (nb - 1); i += NT) {
      const int a = 1 + i / 6, j = i % 6;
      double o = bw ? bw[6 * a + j] : 0.0;  // (fsdf_config_gradient starts from the RBF chain's body wrench)
      for (int u = L.soff[a]; u < L.soff[a + 1]; ++u) o += acc[1 + 6 * L.slist[u] + j];
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
      sub[6 * b + j] = s;
    }
    __syncthreads();
  } else {
    // body wrenches: each body's surfaces in index order (fsdf_config_gradient)
    for (int i = tid; i < 6 * nb; i += NT) {
      const int b = i / 6, j = i - 6 * b;
      double s = bw ? bw[i] : 0.0;
      for (int q = L.soff[b]; q < L.soff[b + 1]; ++q) s += acc[1 + 6 * L.slist[q] + j];
      sub[i] = s;
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
            double s = sub[6 * p + j];
            for (int q = L.coff[p]; q < L.coff[p + 1]; ++q) s += sub[6 * L.clist[q] + j];
            sub[6 * p + j] = s;
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
          double s = sub[6 * p + j];
          for (int q = L.coff[p]; q < L.coff[p + 1]; ++q) s += sub[6 * L.clist[q] + j];
          sub[6 * p + j] = s;
        }
        __syncthreads();
      }
    }
  }
}

// The chain rule from the accumulator: the subtree wrenches, then per joint
// ∂c/∂q into g (its entries start from what the caller left there) with the
// joint frames Rb, tb of the FK that posed the pass; *bad |= 1 where
// kin::joint_gradient fails. Ends with a barrier.
template <int NT>
__device__ void chain_rule(const SolverTree& T, const TreeView& V, const double* acc, const double* bw, double* own,
                           double* sub, const double* Rb, const double* tb, const double* x, double* g, int* bad) {
  subtree_wrenches<NT>(T, V, acc, bw, own, sub);  // (ends with a barrier)
  for (int b = 1 + (int)threadIdx.x; b < T.nb; b += NT) {
    const int k = V.kind[b];
    if (k && !kin::joint_gradient(k, V.axis + 3 * b, Rb + 9 * b, tb + 3 * b, x + V.qoff[b], sub + 6 * b, g + V.qoff[b]))
      atomicOr(bad, 1);
  }
  __syncthreads();
}

// The end of a pose launch, after the FK (L.R, L.t): the surface poses into
// L.P (a non-finite entry sets *nonfinite, zeroed before an earlier barrier),
// a barrier, then this workgroup's NT consecutive work items of the model's
// pose from them (pose_impl.h; whole waves: the total is a multiple of 64, as
// NT).
template <typename TP, int NT>
__device__ void pose_tail(const SolverTree& T, const Lds& L, const LocalModel& lm, const PosedModel& pm,
                          int* nonfinite) {
  const int tid = threadIdx.x;
  for (int i = tid; i < 12 * T.S; i += NT) {
    const int k = i / 12, q = i % 12, b = L.sbody[k];
    const double v = b < 0 ? ((q % 4 == 0 && q < 9) ? 1.0 : 0.0)
                           : kin::surface_pose_entry(q, L.R + 9 * b, L.t + 3 * b, L.FR + 9 * k, L.Ft + 3 * k);
    L.P[i] = v;
    if (!isfinite(v)) *nonfinite = 1;  // (every writer writes the same value)
  }
  __syncthreads();
  const int item = blockIdx.x * NT + tid;
  if (item < pose_items(lm))
    pose_item<TP>(lm, L.P, (TP*)pm.planes_w, (HullRow*)pm.hull_rows, (TP*)pm.verts_w,
                  sizeof(TP) == 8 ? pm.screen_w : nullptr, sizeof(TP) == 8 ? (I4*)pm.image_w : nullptr, item);
}

// the FK's joint frames Rb | tb into a slot of the state, for the next chain rule
template <int NT>
__device__ void store_joint_frames(const SolverTree& T, const Lds& L, double* Rb_slots, int slot) {
  const int tid = threadIdx.x, nb = T.nb;
  double* Rb = Rb_slots + (size_t)slot * 12 * nb;
  for (int i = tid; i < 9 * nb; i += NT) Rb[i] = L.Rb[i];
  for (int i = tid; i < 3 * nb; i += NT) Rb[9 * nb + i] = L.tb[i];
}

// A rigid scene's pose launch: FK of the x in `slot`, the surface poses, this
// workgroup's pose items, and — workgroup 0 — the joint frames into the slot
// and the error flags (1 FK, 2 a non-finite pose). The NaiveSolver's init
// (LM = false, slot 0; the host zeroed the flags) also writes f = 0 and the
// count 0; the LM loop's pose of a later trial (LM = true) returns at once
// when the frame's done flag is set and leaves f and the count alone.
template <typename TP, bool LM>
__device__ void pose_body(const SolverTree& T, const SolverState& st, const LocalModel& lm, const PosedModel& pm,
                          int slot, double* lds) {
  constexpr int NT = kStepThreads;
  __shared__ int bad, s_done, nonfinite;
  const int tid = threadIdx.x;
  if (tid == 0) {
    if (LM) s_done = __builtin_nontemporal_load(st.flags);
    bad = 0;
    nonfinite = 0;
  }
  const Lds L = stage<NT, false>(T, st, lds, nullptr, slot);
  __syncthreads();
  if (LM && s_done) return;
  fk<NT>(T, L, &bad, -1);  // (ends with a barrier)
  pose_tail<TP, NT>(T, L, lm, pm, &nonfinite);
  if (blockIdx.x != 0) return;  // (the state: workgroup 0; every workgroup computed the same values)
  store_joint_frames<NT>(T, L, st.Rb, slot);
  if (tid == 0) {
    if (!LM) {
      *st.f = 0.0;
      st.flags[1] = 0;
    }
    if (bad || nonfinite) {
      st.flags[2] = nonfinite ? 2 : 1;
      st.flags[0] = 1;
    }
  }
}

}  // namespace

}  // namespace fsdf
