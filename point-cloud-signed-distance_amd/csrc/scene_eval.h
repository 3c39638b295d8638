// scene_eval.h — the scene's signed distance for a wave's 64 points (culling,
// seeds, the minimum over hulls and RBF skins) and the chunk epilogue: wrench
// sums and per-point outputs. Only sdf_kernels.hip includes it (through
// pass_kernels.h).
#pragma once
#include "fsdf_internal.h"
#include "hull_sdf.h"
#include "rbf_sdf.h"

namespace fsdf {
// scene_eval's best-first seed takes max(sphere, box) lower bounds below this
// many hulls and the sphere bound alone at or above it (round 5 A/B, DESIGN §7:
// sphere-only at M64 = 64 hulls 0.0489 -> 0.0460 ms pass at 2^17, 0.0908 ->
// 0.0899 at 2^20; at C2 = 7 hulls 0.0680 -> 0.0687, so the box stays there)
constexpr int kSeedBoxMaxHulls = 32;

// Bounding sphere (bbox centre, half diagonal) of the wave's valid lanes'
// points (invalid lanes stand in for the first valid one). Whole wave active.
__device__ __forceinline__ WaveSphere wave_sphere(float pxf, float pyf, float pzf, bool valid) {
  const uint64_t vm = __ballot(valid);
  const int src = vm ? __builtin_ctzll(vm) : 0;
  float qx = pxf, qy = pyf, qz = pzf;
  if (!valid) { qx = __shfl(pxf, src, 64); qy = __shfl(pyf, src, 64); qz = __shfl(pzf, src, 64); }
  const float lx = wave_minmax<false>(qx), ly = wave_minmax<false>(qy), lz = wave_minmax<false>(qz);
  const float hx = wave_minmax<true>(qx), hy = wave_minmax<true>(qy), hz = wave_minmax<true>(qz);
  const float ex = hx - lx, ey = hy - ly, ez = hz - lz;
  WaveSphere ws;
  ws.x = 0.5f * (lx + hx); ws.y = 0.5f * (ly + hy); ws.z = 0.5f * (lz + hz);
  ws.r = 0.5f * __builtin_sqrtf(__builtin_fmaf(ex, ex, __builtin_fmaf(ey, ey, ez * ez)));
  return ws;
}

// ---------------------------------------------------------------------------
// Scene signed distance of this lane's point: minimum over all surfaces with
// the first-index tie rule (src/Flash.jl:265-268), its surface index and
// gradient. Wave-cooperative (ballots, LDS staging): call with the whole wave
// active; `valid` marks lanes whose result is used.
// ---------------------------------------------------------------------------
template <typename T, int SLOTS, bool CULL, bool RBF, bool P64 = false, int NSHARE = 1>
__device__ __forceinline__ void scene_eval(T px, T py, T pz, bool valid, const PassModel<T>& m,
                                           const HullRow* __restrict__ ht, float smax, T* __restrict__ lw,
                                           unsigned long long* __restrict__ stats, T& best, int& bk, T& gx, T& gy,
                                           T& gz, const F4* __restrict__ cws = nullptr, uint64_t partmask = ~0ull,
                                           double* shbest = nullptr, int prior = -1) {
  // partmask (hull-partitioned pass, pass_kernel HPART): this wave evaluates
  // only the hulls whose bit (k & 63) is set; culling and the upper bound
  // still use every hull
  const int K = m.K;
  const int lane = threadIdx.x & 63;
  // Phase A (fp32, exact-safe): with c_k inside hull k and r_k its bounding
  // radius, d_k(p) >= |p-c_k| - r_k and d_k(p) >= the oriented-box bound
  // (lower bounds), d_k(p) <= |p-c_k| (upper bound). ub = min_k |p-c_k|; the
  // best-first seed is the hull of least lower bound (a heuristic: any seed
  // is exact).
  float ub2 = __builtin_huge_valf(), lb_min = __builtin_huge_valf();
  int kseed = 0;
  float pxf = 0.f, pyf = 0.f, pzf = 0.f;
  // candidate hulls of the wave (bit k&63 of cand[k>>6]); all hulls without culling
  uint64_t cand[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int left = K - 64 * s;
    cand[s] = left >= 64 ? ~0ull : (left > 0 ? (1ull << left) - 1 : 0ull);
  }
  uint64_t tw = wt_now();
  pxf = (float)px; pyf = (float)py; pzf = (float)pz;
  // the point's nearest surface in the previous pass over this cloud, when
  // known (PassOutputs::prior_in), is its seed: tracking passes move the model
  // little, so it is usually this pass's nearest too, and `best` is tight after
  // the first evaluation (any seed gives the same bits)
  const bool prior_ok = CULL && !RBF && SLOTS == 1 && prior >= 0 && prior < K && ((partmask >> (prior & 63)) & 1);
  // Seed-first path (wave-uniform): every valid lane of the wave has a usable
  // prior (and the chunk its precomputed sphere, as every resident cloud's
  // has). No candidate loop and no wave-level cull here: the seed is the prior,
  // ub = |p - c_prior| (a true upper bound of d*, one table row per lane), every
  // hull stays a candidate until the seeds are evaluated, and ONE wave-level
  // cull then runs against the lanes' tight bests (in the loop below). Every
  // other wave — a cloud's first pass, a lane whose prior is missing or outside
  // the wave's part, the hull-partitioned tiers — runs Phase A as before.
  constexpr bool kSeedFirst = CULL && !RBF && SLOTS == 1;
  bool seed_first = false;
  if constexpr (kSeedFirst) {
    const uint64_t vm = __ballot(valid);
    seed_first = cws != nullptr && vm != 0 && __ballot(prior_ok) == vm;
  }
  // the wave-level cull's test of hull (64 s + lane) against the upper bound
  // `u` of every valid lane's d*: with the wave's points inside the sphere
  // w = (c_w, r_w) and D_k = |c_w - c_k|, every point of the wave has
  // d_k >= D_k - r_w - r_k and d_k >= the box bound at c_w (1-Lipschitz) minus
  // r_w, so a hull one of whose lower bounds exceeds u by the fp32 margin is
  // needed by no lane
  // (its fp32 rounding margin, >= 1e-5 x every magnitude in the test; the
  // seed-first cull below takes the same margin but runs the test through the
  // loop's needs_at site rather than a second inlined copy of the box test,
  // which cost registers at the budget)
  auto wave_margin = [&](float wx, float wy, float wz, float wr, float u) -> float {
    return 1e-5f * (1.0f + fabsf(wx) + fabsf(wy) + fabsf(wz) + smax + 4.0f * wr + 2.0f * fabsf(u));
  };
  auto wave_cull_at = [&](const WaveSphere& w, int s, float Dks, float u) -> uint64_t {
    const float mrgw = wave_margin(w.x, w.y, w.z, w.r, u);
    const int k = 64 * s + lane;
    const HullRow& h = ht[k < K ? k : 0];
    const bool c = (k < K) & (Dks - w.r - h.sphere[3] <= u + mrgw) & box_within(h, w.x, w.y, w.z, u + mrgw + w.r);
    return __ballot(c);
  };
  if (CULL && seed_first) {
    kseed = prior_ok ? prior : 0;
    const F4 sp = ht[kseed].sphere;
    const float dx = pxf - sp[0], dy = pyf - sp[1], dz = pzf - sp[2];
    ub2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
  } else if (CULL) {
    // the wave's bounding sphere (bbox centre, half diagonal) over the valid
    // lanes: precomputed per resident chunk at set_points (pose-independent,
    // the same arithmetic) or computed here
    WaveSphere ws;
    if (cws) {
      const F4 v = *cws;
      ws = WaveSphere{v[0], v[1], v[2], v[3]};
    } else {
      ws = wave_sphere(pxf, pyf, pzf, valid);
    }
    // Wave-level culling, one hull per lane: with the wave's points inside the
    // sphere (c_w, r_w) and D_k = |c_w - c_k|, every point of the wave has
    // d_k >= D_k - r_w - r_k and d_k <= D_k + r_w, so a hull whose lower bound
    // exceeds UB_w = min_k (D_k + r_w) by the fp32 margin is needed by no lane.
    const float cwx = ws.x, cwy = ws.y, cwz = ws.z, rw = ws.r;
    float Dk[SLOTS];
    float ubw = __builtin_huge_valf();
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int k = 64 * s + lane;
      Dk[s] = __builtin_huge_valf();
      if (k < K) {
        const F4 sp = ht[k].sphere;
        const float dx = cwx - sp[0], dy = cwy - sp[1], dz = cwz - sp[2];
        Dk[s] = __builtin_sqrtf(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz)));
        ubw = fminf(ubw, Dk[s] + rw);
      }
    }
    ubw = wave_minmax<false>(ubw);
    // ... and so does one whose box bound at c_w (1-Lipschitz) minus r_w does
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) cand[s] = wave_cull_at(ws, s, Dk[s], ubw);
    if (count_events(stats) && lane == 0) {
      unsigned long long nc = 0;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) nc += __builtin_popcountll(cand[s]);
      atomicAdd(stats + 8, nc);
    }
    // per lane over the candidates: ub = min_k |p-c_k| and the best-first seed
    // (hull-partitioned pass: over this wave's part only — its ub is still an
    // upper bound of d*, and the chunk's waves share their bests anyway)
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      uint64_t cm = cand[s] & partmask;
      while (cm) {
        const int k = 64 * s + __builtin_ctzll(cm);
        cm &= cm - 1;
        const F4 sp = ht[k].sphere;
        const float dx = pxf - sp[0], dy = pyf - sp[1], dz = pzf - sp[2];
        const float dist2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
        ub2 = fminf(ub2, dist2);
        // seed: the least lower bound — sphere, and on scenes of few hulls also
        // box (a heuristic only: every candidate is still searched, so either
        // seed gives the same bits; kSeedBoxMaxHulls)
        float lb = __builtin_sqrtf(dist2) - sp[3];
        if (K < kSeedBoxMaxHulls) lb = fmaxf(lb, box_lower(ht[k], pxf, pyf, pzf));
        if (lb < lb_min) { lb_min = lb; kseed = k; }
      }
    }
  }
  // (a lane's prior, where it has one, replaces the best-first seed)
  if (prior_ok) kseed = prior;
  const float ub = __builtin_sqrtf(ub2);
  tw = wt_add(4, tw);
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) wt_count(6, __builtin_popcountll(cand[s]));
  // one rounding margin per lane, >= 1e-5 x every magnitude in the test below
  const float mrg = 1e-5f * (1.0f + fabsf(pxf) + fabsf(pyf) + fabsf(pzf) + smax + 2.0f * ub);

  best = tinf<T>();
  bk = 0x7fffffff;
  gx = (T)0; gy = (T)0; gz = (T)0;
  if (RBF) {
    // RBF skins first: always needed (no cheap bound), and they tighten `best`
    for (int r = 0; r < m.R; ++r) {
      const int ks = m.rbf_surface[r];
      const int r0 = m.rbf_row_off[r];
      const int nc = m.rbf_row_off[r + 1] - r0 - 1;
      RbfField<T> F;
      rbf_field(px, py, pz, m.rbf_rows + 4 * r0, nc, lw, m.stage_bytes / (4 * (int)sizeof(T)), F);
      T sv, hx, hy, hz, c_, iG;
      rbf_skin_from_field(F, sv, hx, hy, hz, c_, iG);
      if (valid && (sv < best || (sv == best && ks < bk))) { best = sv; bk = ks; gx = hx; gy = hy; gz = hz; }
    }
    wt_add(5, tw);
  }
  // hull k is needed by a lane unless its lower bound exceeds min(ub, best)
  // by more than the fp32 rounding margin
  // hull k is needed by a lane unless |p-c_k| - r_k > min(ub, best) + mrg,
  // tested without a sqrt: |p-c_k|^2 <= (min(ub, best) + mrg + r_k)^2
  // (HPART) the least best distance the chunk's waves have found so far, per
  // lane, one LDS slot kept by ds_min_f64: an upper bound of d* — as exact-safe
  // a pruning bound as this wave's own best (a stale read only bounds less).
  // (One slot read per test: 2.6 % faster at 2^17 than a slot per wave, a
  // cached copy refreshed per evaluation no faster; profiles/r03/experiments)
  // (NSHARE == 0: shared iff shbest is given — the planned pass decides per
  // workgroup at run time)
  auto bound_now = [&]() -> T {
    T b = best;
    if constexpr (NSHARE > 1) {
      const T o = (T)((const volatile double*)shbest)[lane];
      b = o < b ? o : b;
    } else if constexpr (NSHARE == 0) {
      if (shbest) {
        const T o = (T)((const volatile double*)shbest)[lane];
        b = o < b ? o : b;
      }
    }
    return b;
  };
  // evaluations may run out of index order: ties keep the smaller k
#if FSDF_WAVE_TIMES
  uint64_t wt_slowk = 0;  // hulls whose evaluation ran this lane's search
#endif
  auto evaluate = [&](int k, bool need) {
    wt_count(0, 1);
    wt_count(5, __builtin_popcountll(__ballot(need)));
    T dk, hx, hy, hz;
    hull_sdf<T, P64>(px, py, pz, k, m, ht, need, bound_now(), dk, hx, hy, hz, lw, stats);
#if FSDF_WAVE_TIMES
    if (fsdf_wt_slow[threadIdx.x]) wt_slowk |= 1ull << (k & 63);
#endif
    if (count_events(stats)) {
      const uint64_t nm = __ballot(need);
      if (lane == 0) {
        atomicAdd(stats + 1, 1ull);
        atomicAdd(stats + 3, (unsigned long long)__builtin_popcountll(nm));
      }
    }
    const int ks = RBF ? m.hull_surface[k] : k;
    if (need && (dk < best || (dk == best && ks < bk))) { best = dk; bk = ks; gx = hx; gy = hy; gz = hz; }
    if constexpr (NSHARE > 1)  // (one slot per lane: the minimum over the chunk's waves, ds_min_f64)
      __hip_atomic_fetch_min(shbest + lane, (double)best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else if constexpr (NSHARE == 0)
      if (shbest) __hip_atomic_fetch_min(shbest + lane, (double)best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  uint64_t done[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) done[s] = 0;
#if FSDF_WAVE_TIMES
  auto wt_won = [&]() { wt_count(9, __builtin_popcountll(__ballot(valid && ((wt_slowk >> (bk & 63)) & 1)))); };
#endif
  // ONE evaluation site (hull_sdf is large: two inlined copies doubled the
  // kernel's code to ~40 KB): first each lane's seed hull (Phase B, one
  // evaluation per distinct seed in the wave, so that `best` is tight), then
  // the remaining candidates in index order (Phase C).
  uint64_t pend = (CULL && K > 0) ? __ballot(valid && (lb_min < __builtin_huge_valf() || prior_ok)) : 0ull;
  int slot = seed_first ? -2 : -1;  // Phase C slot; -1 while seeds are pending (-2: and the seed-first cull)
  uint64_t cm = 0ull;  // Phase C candidates left in `slot`
  for (;;) {
    // each turn tests ONE hull row per lane with needs_at (one site: the seed
    // and Phase C turns test the turn's hull k at the lane's point against the
    // lane's bound, the seed-first cull turn tests hull `lane` at the chunk's
    // centre against the wave's bound)
    int k = 0, row;
    float qx, qy, qz, tb;
    bool cull_turn = false;
#if FSDF_WAVE_TIMES
    uint64_t tw_need = 0;
#endif
    if (pend) {
      k = __builtin_amdgcn_readfirstlane(__shfl(kseed, __builtin_ctzll(pend), 64));
      pend &= ~__ballot(valid && kseed == k);
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if ((k >> 6) == s) done[s] |= 1ull << (k & 63);
      if (count_events(stats) && lane == 0) atomicAdd(stats + 5, 1ull);
      wt_count(4, 1);
    } else {
      if constexpr (kSeedFirst) cull_turn = slot == -2;
      if (!cull_turn) {
        while (!cm && slot < SLOTS - 1) {
          ++slot;
#pragma unroll
          for (int s = 0; s < SLOTS; ++s)
            if (s == slot) cm = cand[s] & ~done[s] & partmask;
        }
        if (!cm) break;
        k = 64 * slot + __builtin_ctzll(cm);
        cm &= cm - 1;
#if FSDF_WAVE_TIMES
        tw_need = wt_now();
#endif
      }
    }
    if (cull_turn) {
      // seed-first: the one wave-level cull, after the seeds, the existing test
      // (D_k - r_w - r_k and the box bound at c_w minus r_w, in needs_at's
      // sqrt-free form) against bw, the worst valid lane's min(ub, best), with
      // mrgw's margin (+inf while a lane has no finite best: nothing is culled)
      slot = -1;
      // (the chunk's sphere is read here, not before the seeds: four registers
      // live through the evaluations spilled at the budget. The empty asm makes
      // the pointer opaque so the compiler cannot carry an earlier load over; it
      // changes no value. Both this and the barrier below exist for the register
      // budget alone: after a compiler update or a change here, re-check
      // `make asm`'s resource-usage lines of pass_kernel<double, 1, true, false,
      // true, false, 256, 4> and planned_pass_kernel<double, true> — VGPRs <=
      // 128, ScratchSize 0, Occupancy 4 — and drop a barrier that no longer pays)
      uint32_t cwl = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)cws);
      uint32_t cwh = __builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)cws >> 32));
      asm volatile("" : "+s"(cwl), "+s"(cwh));
      const F4 w = *(const F4*)(((uintptr_t)cwh << 32) | cwl);
      const float bw = wave_minmax<true>(valid ? fminf(ub, (float)bound_now()) : -__builtin_huge_valf());
      const float mrgw = wave_margin(w[0], w[1], w[2], w[3], bw);
      row = lane < K ? lane : 0;
      qx = w[0]; qy = w[1]; qz = w[2];
      tb = bw + mrgw + w[3];
    } else {
      // hull k is needed by a lane unless its lower bound exceeds min(ub, best)
      // by more than the fp32 rounding margin
      row = k;
      if constexpr (kSeedFirst) {
        // (the fp32 point converted again per test — three conversions — rather
        // than three more registers live through the evaluations; the empty asm
        // keeps the compiler from hoisting them back — see the note above on
        // what to re-check)
        T tx = px, ty = py, tz = pz;
        asm volatile("" : "+v"(tx), "+v"(ty), "+v"(tz));
        qx = (float)tx; qy = (float)ty; qz = (float)tz;
      } else {
        qx = pxf; qy = pyf; qz = pzf;
      }
      tb = fminf(ub, (float)bound_now()) + mrg;
    }
    bool need = CULL ? needs_at(ht[row], qx, qy, qz, tb) : true;
    if (cull_turn) {
      cand[0] = __ballot(need & (lane < K));
      if (count_events(stats) && lane == 0) {
        atomicAdd(stats + 8, (unsigned long long)__builtin_popcountll(cand[0]));
        atomicAdd(stats + 22, 1ull);
      }
      continue;
    }
    need &= valid;
    // (a seed the earlier seeds' results have ruled out for every lane — its
    // bit is in `done`; bounds only tighten, so Phase C would skip it too —
    // takes no staging and no screen either: 2^17 0.0464 -> 0.0454 ms pass,
    // DESIGN §7)
    const bool any_need = __any(need);
#if FSDF_WAVE_TIMES
    if (tw_need) wt_count(11, wt_now() - tw_need);
#endif
    if (!any_need) continue;
    evaluate(k, need);
  }
#if FSDF_WAVE_TIMES
  wt_won();
#endif
  if (count_events(stats) && lane == 0) atomicAdd(stats + 0, 1ull);
}

// Per-chunk epilogue (pass and merge kernels): this wave's contributions
//   c += d^2;  F_k += 2 d g;  M_k += 2 d (p x g)   (RBF skins: adjoint sums)
// segmented by k* (ballot loop; the group's six sums in one packed wave
// reduction, wave_sum_packed, added into surface k's LDS row by the lanes that
// hold them), then the per-point outputs. acc_row: this lane's row (row `lane`
// of the wave's rows). CHUNK_COST: the chunk's Σ d² rides in the first group's
// reduction as a seventh value and is RETURNED in cost_acc (wave-uniform, the
// bits of wave_sum over the lanes' d²); otherwise cost_acc is the lane's
// running sum. Whole wave active.
template <typename T, int SLOTS, bool RBF, bool CHUNK_COST = false>
__device__ __forceinline__ uint64_t emit_chunk(T px, T py, T pz, bool valid, T best, int bk, T gx, T gy, T gz, int64_t i,
                                           int64_t base, int64_t n, const PassModel<T>& m, const PassOutputs& out,
                                           double* __restrict__ acc_row, double& cost_acc,
                                           double* __restrict__ rbf_wave, T* __restrict__ stage, int stage_cap) {
  const int lane = threadIdx.x & 63;
  // contributions: c += d^2; F_k += 2 d g; M_k += 2 d (p x g)
  double cF[3] = {0.0, 0.0, 0.0}, cM[3] = {0.0, 0.0, 0.0};
  double ccost = 0.0;  // (CHUNK_COST) this lane's d², until the first group has summed it
  if (valid) {
    const double bd = (double)best;
    const double dgx = gx, dgy = gy, dgz = gz;
    const double dpx = px, dpy = py, dpz = pz;
    if constexpr (CHUNK_COST) ccost = __builtin_fma(bd, bd, 0.0);
    else cost_acc = __builtin_fma(bd, bd, cost_acc);
    const double w = 2.0 * bd;
    cF[0] = w * dgx; cF[1] = w * dgy; cF[2] = w * dgz;
    cM[0] = w * __builtin_fma(dpy, dgz, -(dpz * dgy));
    cM[1] = w * __builtin_fma(dpz, dgx, -(dpx * dgz));
    cM[2] = w * __builtin_fma(dpx, dgy, -(dpy * dgx));
  }
  const uint64_t tw = wt_now();
  uint64_t pending = __ballot(valid);
  uint64_t touched = 0;  // surfaces (k & 63) of this chunk's points
  if constexpr (CHUNK_COST) cost_acc = 0.0;
  constexpr int kSums = CHUNK_COST ? 7 : 6;
  while (pending) {
    const int leader = __builtin_ctzll(pending);
    const int kk = __builtin_amdgcn_readfirstlane(__shfl(bk, leader, 64));
    const bool sel = valid && (bk == kk);
    pending &= ~__ballot(sel);
    touched |= 1ull << (kk & 63);
    if (RBF && m.surface_kind[kk] != 0) {
      // RBF skin: adjoint sums instead of a rigid wrench
      int r = 0;
      while (m.rbf_surface[r] != kk) ++r;
      const int r0 = m.rbf_row_off[r];
      rbf_adjoint(px, py, pz, m.rbf_rows + 4 * r0, m.rbf_row_off[r + 1] - r0 - 1, stage, stage_cap, sel,
                  rbf_wave + m.rbf_acc_off[r]);
      continue;
    }
    double v[kSums];
#pragma unroll
    for (int j = 0; j < 3; ++j) { v[j] = sel ? cF[j] : 0.0; v[3 + j] = sel ? cM[j] : 0.0; }
    if constexpr (CHUNK_COST) v[6] = ccost;
    const double u = wave_sum_packed<kSums>(v);
    if constexpr (CHUNK_COST) {
      if (touched == (1ull << (kk & 63)))  // the chunk's first group (wave-uniform)
        cost_acc = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(u), packed_sum_lane(6)),
                                    __builtin_amdgcn_readlane(__double2loint(u), packed_sum_lane(6)));
      ccost = 0.0;
    }
    // the lanes that hold sum pj (packed_sum_lane) add it into row kk, (kk - lane)
    // rows from their own: one add per sum, as before. (The holders' mask and
    // index come from an opaque copy of the lane, so that they are not hoisted
    // and carried through the loop — or, in the grid-stride kernels, through
    // the next scene evaluation: the register budget again, see scene_eval's
    // note and DESIGN §7 "Pass overhead".)
    int l = lane;
    asm volatile("" : "+v"(l));
    const int pj = (l & 3) + ((l >> 2) & 4);
    if (((l & 0x2c) == 0x0c) & (pj < 6)) acc_row[(kk - lane) * 6 + pj] += u;
  }

  {
    // the next pass's seed hint (resident order), stored only where it changed
    // (re-read here rather than carried from the seed load: a register live
    // through scene_eval spills at the budget)
    if (out.prior_out && valid && out.prior_out[i] != (uint8_t)bk) out.prior_out[i] = (uint8_t)bk;
    if (out.perm) {  // caller order: scattered through the sort permutation
      if (valid) {
        const int64_t o = out.perm[i];
        if (out.kstar) out.kstar[o] = bk;
        if (out.d) out.d[o] = (double)best;
        if (out.grad) {
          out.grad[3 * o + 0] = (double)gx;
          out.grad[3 * o + 1] = (double)gy;
          out.grad[3 * o + 2] = (double)gz;
        }
      }
    } else {  // resident order: coalesced
      if (valid) {
        if (out.kstar) out.kstar[i] = bk;
        if (out.d) out.d[i] = (double)best;
      }
      if (out.grad) {
        // the wave's [64][3] gradient block is contiguous: transpose it
        // through this wave's (now free) stage and store whole 16-B chunks —
        // three strided 8-B stores per lane would each write a third of
        // every 64-B granule (3x the bytes at the memory side)
        double* sg = (double*)stage;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        sg[3 * lane + 0] = (double)gx;
        sg[3 * lane + 1] = (double)gy;
        sg[3 * lane + 2] = (double)gz;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int nvalid = (int)(n - base < 64 ? n - base : 64);
        typedef double D2 __attribute__((ext_vector_type(2)));
        D2* dst = (D2*)(out.grad + 3 * base);  // 16-B aligned: base is a multiple of 64
        const D2* src = (const D2*)sg;
        for (int c = lane; 2 * c < 3 * nvalid; c += 64) {
          if (2 * c + 1 < 3 * nvalid) dst[c] = src[c];
          else out.grad[3 * base + 2 * c] = sg[2 * c];  // odd tail (3 * nvalid odd)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // stage reads before the next overwrite
      }
    }
  }
  wt_add(6, tw);
  return touched;
}

}  // namespace fsdf
