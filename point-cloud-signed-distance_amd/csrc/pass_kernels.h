// pass_kernels.h — the kernels that evaluate the scene over a cloud: the
// residual pass (pass_kernel), the planned pass of resident clouds and the
// depth-sensor raycast, with their dynamic LDS and the partials layout. Only
// sdf_kernels.hip includes it.
#pragma once
#include "fsdf_internal.h"
#include "scene_eval.h"

namespace fsdf {
constexpr int kMaxRbfAcc = kMaxRbfAccum;
constexpr int kHpart = 4;  // waves per chunk in the hull-partitioned pass's first tier (the second: 2)
constexpr int kPassWavesPerSimd = FSDF_PASS_WAVES_PER_SIMD;  // occupancy target (VGPR budget 512/w)

// Per-block partial sums in line tiles: entry t of logical block b at
// partials[t / 8][b][t % 8] — a block writes whole 64-B lines and
// reduce_tiles_kernel reads whole lines (entry-major columns
// wrote one 8-B entry per line, block-major rows made the reduce stride).
__device__ __forceinline__ int64_t pidx(int t, int b, int nblocks) {
  return ((int64_t)(t >> 3) * nblocks + b) * 8 + (t & 7);
}

// ---------------------------------------------------------------------------
// Residual pass.
// ---------------------------------------------------------------------------
extern __shared__ __attribute__((aligned(16))) char fsdf_lds[];

// ALIAS (one chunk per wave: n <= grid * 256; hull-only, <= 64 surfaces; f64
// models with LocalModel::planes64): the wave's wrench rows live in its own
// hull stage, which is free once the chunk's scene evaluation is done — 12 KiB
// less LDS per workgroup, spent on staging the fp64 planes with the hull
// (hull_sdf P64) at the same occupancy.
//
// HPART (hull-partitioned, with ALIAS; small clouds, hpart_pass): kHpart
// waves share one 64-point chunk and split its hull evaluations by hull index
// (part j of the chunk evaluates hulls k with k % kHpart == j; culling and the
// upper bound use every hull, each wave prunes with its own best). Any upper
// bound of d* is exact-safe, so each wave's result is the exact first-index
// minimum over its hulls, and the lexicographic (d, k) minimum over the
// chunk's waves is the full scene's — bit for bit. The heaviest chunks'
// serial evaluations are spread over kHpart waves where a one-wave-per-chunk
// grid would leave most wave slots idle.
template <typename T, int SLOTS, bool CULL, bool RBF, bool ALIAS = false, bool HPART = false, int NB = kPassBlock,
          int NPART = kHpart>
// (occupancy target in waves per SIMD, whatever the workgroup size NB; NPART:
// waves per chunk of the hull-partitioned pass, 4 or 2 — hpart_parts)
__global__ __launch_bounds__(NB) __attribute__((
    amdgpu_waves_per_eu((SLOTS == 1 ? kPassWavesPerSimd : (SLOTS == 2 ? 3 : 2)) - (RBF ? 1 : 0)))) void pass_kernel(
    const T* __restrict__ pts, int64_t n, PassModel<T> m, PassOutputs out) {
  if (out.skip && *out.skip) return;  // (uniform: a converged device solver loop)
  static_assert(!ALIAS || (SLOTS == 1 && !RBF), "aliased wrench rows: hull-only, <= 64 surfaces");
  static_assert(!HPART || ALIAS, "the hull-partitioned pass is an aliased pass");
  constexpr int kParts = HPART ? NPART : 1;
  constexpr int kChunkStride = NB / kParts;  // points per logical block
  const int lane = threadIdx.x & 63;
  // The wave index is wave-uniform, and readfirstlane tells the compiler so:
  // the wave's stage and row addresses then stay out of the vector registers,
  // which scene_eval fills to the budget (the bench variant spilled without
  // it once the seed-first path was added). It is a register-budget measure
  // only, checked per variant against the resource-usage remarks of `make
  // asm`: 1 to 15 VGPRs fewer everywhere except the brute-force variants of
  // more than 64 hulls (!CULL, !RBF, SLOTS > 1), which took 2 more and
  // therefore keep the lane value. When this line or scene_eval changes,
  // re-check the VGPRs / ScratchSize / Occupancy lines of every pass_kernel
  // variant (profiles/r09/pass_overhead/resource_usage_head.txt is the record).
  const int wave = (SLOTS == 1 || CULL || RBF) ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)
                                                : (int)(threadIdx.x >> 6);
  // (wave-uniform: readfirstlane keeps the hull mask and the loops scalar)
  const int part = HPART ? __builtin_amdgcn_readfirstlane(wave % kParts) : 0;  // (HPART) this wave's hull residue
  const int cw = HPART ? __builtin_amdgcn_readfirstlane(wave / kParts) : wave;  // the block's chunk this wave works on
  // All LDS is one dynamic region (16-byte aligned carve, see pass_lds_bytes):
  //   red     [4 waves][kRedStride] f64  per-hull wrench sums + cost (not ALIAS)
  //   rbf_acc [4 waves][kMaxRbfAcc] f64  (RBF variants only)
  //   stage   [4 waves][m.stage_bytes]   hull / RBF row stage (ALIAS: after the
  //                                      evaluation, the wave's red rows, then
  //                                      the gradient transpose)
  // per-hull wrench sums: row (s*64 + lane) of this wave's slab is owned by
  // lane `lane` (hull s*64 + lane)
  constexpr int kRedStride = SLOTS * 64 * 6 + 2;
  double* red = (double*)fsdf_lds;
  HullRow* ht = (HullRow*)(fsdf_lds + (ALIAS ? 0 : ((NB / 64) * kRedStride + (RBF ? (NB / 64) * kMaxRbfAcc : 0)) * 8));
  T* stage = (T*)((char*)(ht + m.K + 1) + wave * m.stage_bytes);
  auto red_of = [&](int w) -> double* {
    return ALIAS ? (double*)((char*)(ht + m.K + 1) + w * m.stage_bytes) : red + w * kRedStride;
  };
  double* acc_row = red_of(wave) + lane * 6;
  auto zero_rows = [&]() {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc_row[s * 64 * 6 + j] = 0.0;
  };
  if (!ALIAS) zero_rows();
  double cost_acc = 0.0;
  // RBF adjoint sums of this wave (lane 0 adds)
  double* rbf_acc = red + (NB / 64) * kRedStride;
  double* rbf_wave = rbf_acc + wave * kMaxRbfAcc;
  const int stage_cap = m.stage_bytes / (4 * (int)sizeof(T));
  if (RBF)
    for (int e = lane; e < m.rbf_acc_off[m.R]; e += 64) rbf_wave[e] = 0.0;
  // logical block of this launch slot (cost-ordered schedule, see PassOutputs)
  const int lb = out.order ? __builtin_amdgcn_readfirstlane(out.order[blockIdx.x]) : (int)blockIdx.x;
  // (ALIAS: a wave past the cloud's end never evaluates; its rows are zeroed now)
  if (ALIAS && (int64_t)lb * kChunkStride + cw * 64 >= n) {
    zero_rows();
    if (lane == 0) red_of(wave)[SLOTS * 64 * 6] = 0.0;
  }
  const uint64_t t_block = out.cost ? __builtin_amdgcn_s_memrealtime() : 0;
#if FSDF_WAVE_TIMES
  const uint64_t t_block0 = __builtin_amdgcn_s_memrealtime();
#endif
  const float smax = load_hull_table(m, ht);
  const int64_t stride = (int64_t)gridDim.x * kChunkStride;
  // (HPART: exactly one iteration for every wave, also for a chunk past the
  // cloud's end — its lanes are all invalid — because the combine below holds
  // workgroup barriers)
  const int64_t base0 = (int64_t)lb * kChunkStride + cw * 64;
  for (int64_t base = base0; HPART ? base == base0 : base < n; base += stride) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const int64_t ii = valid ? i : n - 1;
    const T px = pts[3 * ii + 0], py = pts[3 * ii + 1], pz = pts[3 * ii + 2];
#if FSDF_WAVE_TIMES
    const uint64_t w_t0 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0)
      fsdf_wave_ev[wave][0] = fsdf_wave_ev[wave][1] = fsdf_wave_ev[wave][2] = fsdf_wave_ph[wave][0] =
          fsdf_wave_ph[wave][1] = fsdf_wave_ph2[wave][0] = fsdf_wave_ph2[wave][1] = 0;
#endif

    T best, gx, gy, gz;
    int bk;
    const F4* cws = out.chunk_ws ? (const F4*)out.chunk_ws + (base >> 6) : nullptr;
    double* shb = nullptr;
    if constexpr (HPART) {  // the chunk's shared per-lane bests, after the stages
      shb = (double*)((char*)(ht + m.K + 1) + (NB / 64) * m.stage_bytes) + 64 * cw;
      if (part == 0) ((volatile double*)shb)[lane] = __builtin_huge_val();
      __syncthreads();
    }
    // (not in the hull-partitioned tiers: bound by their heaviest chunk's
    // latency, the prior's load in front of it cost 2^16 0.0501 -> 0.0532 ms)
    const int prior = (!HPART && out.prior_in && valid) ? (int)out.prior_in[i] : -1;
    scene_eval<T, SLOTS, CULL, RBF, ALIAS, kParts>(px, py, pz, valid, m, ht, smax, stage, out.stats, best, bk, gx, gy,
                                                   gz, cws,
                                                   HPART ? ((kParts == 4 ? 0x1111111111111111ull
                                                                         : 0x5555555555555555ull)
                                                            << part)
                                                         : ~0ull,
                                                   shb, prior);
    if constexpr (HPART) {
      // the chunk's waves' results meet in their stages; part 0 keeps the
      // lexicographic (d, k) minimum per point
      T* rs = stage;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      rs[4 * lane + 0] = best; rs[4 * lane + 1] = gx; rs[4 * lane + 2] = gy; rs[4 * lane + 3] = gz;
      ((int*)(rs + 256))[lane] = bk;
      __syncthreads();
      if (part == 0) {
#pragma unroll
        for (int w = 1; w < kParts; ++w) {
          const T* ro = (const T*)((char*)(ht + m.K + 1) + (wave + w) * m.stage_bytes);
          const T d2 = ro[4 * lane];
          const int k2 = ((const int*)(ro + 256))[lane];
          if (d2 < best || (d2 == best && k2 < bk)) {
            best = d2; bk = k2; gx = ro[4 * lane + 1]; gy = ro[4 * lane + 2]; gz = ro[4 * lane + 3];
          }
        }
      }
      __syncthreads();
    }
    if (!valid) bk = 0;

    if (ALIAS) {  // the stage is free: this wave's rows go there (once: one chunk per wave)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      zero_rows();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    T* tstage = ALIAS ? (T*)((char*)stage + kRedStride * 8) : stage;  // gradient transpose after the rows
    // (ALIAS: the wave's one chunk; its cost is summed and parked in the
    // wave's row now — a per-lane accumulator live through the whole kernel
    // was spilled to scratch at the register budget)
    double cost_chunk = 0.0;
    if (!HPART || part == 0)  // (HPART: part 0 emits the chunk; the other waves' rows stay zero)
      emit_chunk<T, SLOTS, RBF, ALIAS>(px, py, pz, valid, best, bk, gx, gy, gz, i, base, n, m, out, acc_row,
                                       ALIAS ? cost_chunk : cost_acc, rbf_wave, tstage, stage_cap);
    // (ALIAS: emit_chunk returned the chunk's sum)
    if (ALIAS && lane == 0) red_of(wave)[SLOTS * 64 * 6] = cost_chunk;
#if FSDF_WAVE_TIMES
    // diagnostic: 100 MHz wall clock around each wave-iteration of the first
    // grid pass (stats + 32 + 2 * wave), written by lane 0
    if (out.stats && lane == 0 && (!HPART || part == 0) && base < (int64_t)64 * 4 * kMaxBlocks) {
      const int64_t wv = base / 64;
      out.stats[32 + 2 * wv] = w_t0;
      out.stats[33 + 2 * wv] = __builtin_amdgcn_s_memrealtime();
      out.stats[32 + 8 * kMaxBlocks + 2 * wv] = fsdf_wave_ev[wave][0];
      out.stats[33 + 8 * kMaxBlocks + 2 * wv] = fsdf_wave_ev[wave][1];
      out.stats[32 + 18 * kMaxBlocks + 2 * wv] = fsdf_wave_ph[wave][0];
      out.stats[33 + 18 * kMaxBlocks + 2 * wv] = fsdf_wave_ph[wave][1];
      out.stats[32 + 26 * kMaxBlocks + wv] = fsdf_wave_ev[wave][2];
      if (wv < kMaxBlocks) {
        out.stats[32 + 30 * kMaxBlocks + 2 * wv] = fsdf_wave_ph2[wave][0];
        out.stats[33 + 30 * kMaxBlocks + 2 * wv] = fsdf_wave_ph2[wave][1];
      }
    }
#endif
  }

  // ---- block combine (fixed order) ----
  if (!ALIAS) {
    cost_acc = wave_sum(cost_acc);
    if (lane == 0) red_of(wave)[SLOTS * 64 * 6] = cost_acc;
  }
  __syncthreads();
  const int len6 = 1 + 6 * m.S;
  const int len = len6 + (RBF ? m.rbf_acc_off[m.R] : 0);
  for (int t = threadIdx.x; t < len; t += NB) {
    double s;
    if (t < len6) {
      const int src = (t == 0) ? SLOTS * 64 * 6 : t - 1;
      s = red_of(0)[src];
#pragma unroll
      for (int w = 1; w < NB / 64; ++w) s += red_of(w)[src];
    } else {
      const int src = RBF ? t - len6 : 0;
      s = rbf_acc[src];
#pragma unroll
      for (int w = 1; w < NB / 64; ++w) s += rbf_acc[w * kMaxRbfAcc + src];
    }
    out.partials[pidx(t, lb, gridDim.x)] = s;
  }
  if (out.cost && threadIdx.x == 0) out.cost[lb] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_block);
#if FSDF_WAVE_TIMES
  if (out.stats && threadIdx.x == 0 && lb < kMaxBlocks) {  // diagnostic: block start / end (100 MHz)
    out.stats[32 + 16 * kMaxBlocks + 2 * lb] = t_block0;
    out.stats[33 + 16 * kMaxBlocks + 2 * lb] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

// ---------------------------------------------------------------------------
// Planned pass: resident clouds of hull-only scenes with <= 64 surfaces whose
// fp64 planes are staged (the aliased layout, pass_kernel ALIAS / HPART).
//
// Launch slot b runs plan[b], one of three workgroup shapes — 4 chunks of 64
// points one wave each; 2 chunks over 2 waves each; 1 chunk over all 4 waves
// (hull-partitioned: wave j evaluates the hulls k = j mod parts, bests shared
// through one ds_min_f64 slot per lane, merged by the first-index (d, k) rule,
// exactly as pass_kernel HPART) — chosen per chunk from the chunks' measured
// durations (plan_kernel: the heaviest chunks split over 4 or 2 waves, the
// rest grouped by similar cost, heaviest workgroups first). The pass is bound
// by its heaviest chunks' serial hull evaluations (~100 us at 2^20 points
// against ~70 us of average wave work); a per-chunk split only
// where it pays leaves the rest of the grid one wave per chunk. Without a
// plan (a new cloud's first pass) slot b runs `dparts` waves per chunk in
// index order — the size tiers of hpart_parts.
//
// Every chunk writes its OWN partial row — the chunk's Σ d², and its wrench
// sums (F, M) per nearest surface as up to 4 (k, F, M) entries, or a dense
// [S][6] row when more than 4 surfaces meet in the chunk — so the
// accumulator (reduce_chunks_kernel, one launch) sums the chunk rows in a
// fixed order whatever the plan: bit-identical across plans, schedules and
// passes. No block combine, no
// barrier after the prologue for one-wave chunks.
// ---------------------------------------------------------------------------
constexpr int kPlanChunkMask = (1 << kPlanPartsShift) - 1;

// One chunk's epilogue in the planned pass: the wave's wrench
// rows (lane k owns surface k) in its free stage, the per-point outputs, and
// the chunk's partial row — Σ d², then sparse (k, F, M) entries in ascending k
// or, when more than 4 surfaces meet in the chunk, a dense [S][6] row.
template <typename T>
__device__ __forceinline__ void emit_chunk_row(T px, T py, T pz, bool valid, T best, int bk, T gx, T gy, T gz, int cid,
                                               int64_t n, const PassModel<T>& m, const PassOutputs& out,
                                               const ChunkOutputs& co, T* __restrict__ stage) {
  const int lane = threadIdx.x & 63;
  const int64_t base = (int64_t)cid * 64;
  const int64_t i = base + lane;
  double* acc_row = (double*)stage + lane * 6;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
  for (int j = 0; j < 6; ++j) acc_row[j] = 0.0;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  T* tstage = (T*)((char*)stage + (64 * 6 + 2) * 8);  // gradient transpose after the rows
  double cost_chunk = 0.0;
  const uint64_t touched = emit_chunk<T, 1, false, true>(px, py, pz, valid, best, bk, gx, gy, gz, i, base, n, m, out,
                                                         acc_row, cost_chunk, nullptr, tstage,
                                                         m.stage_bytes / (4 * (int)sizeof(T)));  // (cost_chunk: the chunk's sum)
  const int cnt = __builtin_popcountll(touched);
  if (cnt <= 4) {
    if ((touched >> lane) & 1) {
      const int sl = __builtin_popcountll(touched & ((1ull << lane) - 1));
      double* e = co.ent + ((int64_t)cid * 4 + sl) * 6;
#pragma unroll
      for (int j = 0; j < 6; ++j) e[j] = acc_row[j];
    }
    if (lane == 0) {
      I4 h = I4{-1, -1, -1, -1};
      uint64_t t = touched;
      for (int sl = 0; sl < 4 && t; ++sl) {
        h[sl] = __builtin_ctzll(t);
        t &= t - 1;
      }
      ((I4*)co.hdr)[cid] = h;
      co.csum[cid] = cost_chunk;
    }
  } else {
    if (lane < m.S) {
      double* r = co.dense + ((int64_t)cid * m.S + lane) * 6;  // [nc][S][6]
#pragma unroll
      for (int j = 0; j < 6; ++j) r[j] = acc_row[j];
    }
    if (lane == 0) {
      ((I4*)co.hdr)[cid] = I4{-2, -1, -1, -1};
      co.csum[cid] = cost_chunk;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // row reads before the stage is overwritten
}

template <typename T, bool CULL>
__global__ __launch_bounds__(kPassBlock) __attribute__((amdgpu_waves_per_eu(kPassWavesPerSimd))) void planned_pass_kernel(
    const T* __restrict__ pts, int64_t n, PassModel<T> m, PassOutputs out, ChunkOutputs co) {
  if (out.skip && *out.skip) return;
  const int lane = threadIdx.x & 63;
  // (a lane value here: told wave-uniform as in pass_kernel, the kernel took 8
  // registers fewer and ran 1.3 % slower at 2^17 points)
  const int wave = threadIdx.x >> 6;
  HullRow* ht = (HullRow*)fsdf_lds;
  char* stages = (char*)(ht + m.K + 1);
  T* stage = (T*)(stages + wave * m.stage_bytes);
  double* shb_all = (double*)(stages + 4 * m.stage_bytes);  // [4][64] shared per-lane bests
  uint64_t* t0_lds = (uint64_t*)(shb_all + 4 * 64);         // [4] chunk start times
  // this wave's (waves per chunk, chunk): re-read after the scene evaluation
  // rather than kept live through it (scalar registers are spilled to vector
  // lanes at this kernel's register budget)
  auto slot_of = [&](int& parts_, int& cid_) {
    if (co.plan) {
      const I4 e = ((const I4*)co.plan)[blockIdx.x];
      parts_ = (e[0] >> kPlanPartsShift) & 7;
      const int sl = wave / parts_;
      cid_ = sl == 0 ? (e[0] & kPlanChunkMask) : (sl == 1 ? e[1] : (sl == 2 ? e[2] : e[3]));
    } else {
      parts_ = co.dparts;
      cid_ = (int)blockIdx.x * (4 / parts_) + wave / parts_;
    }
    parts_ = __builtin_amdgcn_readfirstlane(parts_);
    cid_ = __builtin_amdgcn_readfirstlane(cid_);
  };
  int parts, cid;
  slot_of(parts, cid);
  const float smax = load_hull_table(m, ht);  // (the workgroup's one barrier for one-wave chunks)
  bool has = cid >= 0 && (int64_t)cid * 64 < n;
  if (!has && parts == 1) return;  // wave-uniform; no barrier follows for one-wave chunks
  if (lane == 0) t0_lds[wave] = __builtin_amdgcn_s_memrealtime();
  const int part = __builtin_amdgcn_readfirstlane(wave % parts);
  int64_t base = (int64_t)cid * 64;
  const bool valid = has && base + lane < n;
  const int64_t ii = valid ? base + lane : (has ? n - 1 : 0);
  const T px = pts[3 * ii + 0], py = pts[3 * ii + 1], pz = pts[3 * ii + 2];
  double* shb = parts > 1 ? shb_all + 64 * (wave / parts) : nullptr;
  if (parts > 1) {
    if (part == 0) ((volatile double*)shb)[lane] = __builtin_huge_val();
    __syncthreads();
  }
  T best = tinf<T>(), gx = (T)0, gy = (T)0, gz = (T)0;
  int bk = 0x7fffffff;
  if (has) {
    const uint64_t pm = parts == 4 ? (0x1111111111111111ull << part)
                                   : (parts == 2 ? (0x5555555555555555ull << part) : ~0ull);
    const F4* cws = out.chunk_ws ? (const F4*)out.chunk_ws + cid : nullptr;
    const int prior = (out.prior_in && valid) ? (int)out.prior_in[base + lane] : -1;
    scene_eval<T, 1, CULL, false, true, 0>(px, py, pz, valid, m, ht, smax, stage, out.stats, best, bk, gx, gy, gz,
                                           cws, pm, shb, prior);
  }
  if (parts > 1) {
    // the chunk's waves' results meet in their stages; part 0 keeps the
    // lexicographic (d, k) minimum per point (pass_kernel HPART's merge)
    T* rs = stage;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    rs[4 * lane + 0] = best; rs[4 * lane + 1] = gx; rs[4 * lane + 2] = gy; rs[4 * lane + 3] = gz;
    ((int*)(rs + 256))[lane] = bk;
    __syncthreads();
    if (part == 0) {
      for (int w = 1; w < parts; ++w) {
        const T* ro = (const T*)(stages + (wave + w) * m.stage_bytes);
        const T d2 = ro[4 * lane];
        const int k2 = ((const int*)(ro + 256))[lane];
        if (d2 < best || (d2 == best && k2 < bk)) {
          best = d2; bk = k2; gx = ro[4 * lane + 1]; gy = ro[4 * lane + 2]; gz = ro[4 * lane + 3];
        }
      }
    }
    __syncthreads();
  }
  if (!has || part != 0) return;  // (no barrier follows)
  slot_of(parts, cid);
  base = (int64_t)cid * 64;
  if (!valid) bk = 0;
  emit_chunk_row<T>(px, py, pz, valid, best, bk, gx, gy, gz, cid, n, m, out, co, stage);
  if (co.dur && lane == 0) {
    // serial-equivalent duration: a split chunk's wall time scaled by the
    // speed-up its split buys (ChunkOutputs::r4n / r4d, r2n / r2d)
    const uint64_t dt = __builtin_amdgcn_s_memrealtime() - t0_lds[wave];
    const uint64_t est = parts == 4 ? (dt * (uint64_t)co.r4n) / (uint64_t)co.r4d
                                    : (parts == 2 ? (dt * (uint64_t)co.r2n) / (uint64_t)co.r2d : dt);
    co.dur[cid] = (uint32_t)(est < 0xffffffffull ? est : 0xffffffffull);
  }
}

// ---------------------------------------------------------------------------
// Depth-sensor raycast (src/depthsensors.jl:56-97, doRaycast): secant march
// along each ray on the scene SDF from the sensor origin:
//   step = -last/est_grad, clamped to |step| <= 0.4; est_grad starts at -1;
//   stop when |SDF| <= 1e-5 or after 60 steps; depth = NaN when the final
//   |SDF| > 1e-2. One lane per ray; each step is one wave-cooperative
//   scene_eval (lanes that have converged ride along as invalid).
// ---------------------------------------------------------------------------
struct RayOrigin {
  double x, y, z;
};

template <typename T, int SLOTS, bool CULL, bool RBF>
__global__ __launch_bounds__(kBlock, (SLOTS == 1 ? kPassWavesPerSimd : (SLOTS == 2 ? 3 : 2)) - (RBF ? 1 : 0)) void
raycast_kernel(RayOrigin o, const double* __restrict__ rays, int64_t n, PassModel<T> m, double* __restrict__ depth) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  HullRow* ht = (HullRow*)fsdf_lds;  // dynamic LDS: hull table, then 4 wave stages
  T* stage = (T*)((char*)(ht + m.K + 1) + wave * m.stage_bytes);
  const float smax = load_hull_table(m, ht);
  const T EPS = (T)1e-5, SAFE_RATE = (T)0.4;
  const int SAFE_ITER_LIMIT = 60;
  const T ox = (T)o.x, oy = (T)o.y, oz = (T)o.z;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t base = (int64_t)blockIdx.x * kBlock + wave * 64; base < n; base += stride) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const int64_t ii = valid ? i : n - 1;
    const T rx = (T)rays[3 * ii + 0], ry = (T)rays[3 * ii + 1], rz = (T)rays[3 * ii + 2];
    T dist = (T)0, est = (T)-1, last, gx, gy, gz;
    int bk, k = 0;
    scene_eval<T, SLOTS, CULL, RBF>(ox + dist * rx, oy + dist * ry, oz + dist * rz, valid, m, ht, smax, stage, nullptr,
                                    last, bk, gx, gy, gz);
    bool active = valid && fabs(last) > EPS;
    while (__any(active)) {
      T step = (T)0;
      if (active) {
        step = -last / est;
        const T a = fabs(step);
        step = copysign(a < SAFE_RATE ? a : SAFE_RATE, step);
        dist += step;
      }
      T v;
      scene_eval<T, SLOTS, CULL, RBF>(ox + dist * rx, oy + dist * ry, oz + dist * rz, active, m, ht, smax, stage,
                                      nullptr, v, bk, gx, gy, gz);
      if (active) {
        est = (v - last) / step;
        last = v;
        ++k;
        active = fabs(last) > EPS && k < SAFE_ITER_LIMIT;
      }
    }
    if (valid) depth[i] = fabs(last) > (T)1000 * EPS ? __builtin_nan("") : (double)dist;
  }
}

}  // namespace fsdf
