// reduce_kernels.h — what follows a pass on the device: the planned pass's
// chunk-group sums and its plan, the tile reduce into the accumulator, the
// cost-ordered block schedule. Only sdf_kernels.hip includes it.
#pragma once
#include "pass_kernels.h"  // (pidx, fsdf_lds, wave_sum)

namespace fsdf {
// The planned pass's reduction, stage 1: workgroup g sums the chunk rows of
// chunks 16g .. 16g+15 into row g of the line-tiled partials, which
// reduce_tiles_kernel (the unplanned pass's stage 2) then sums. The group's
// rows are expanded in LDS into a dense [16][len] table — zeros, each sparse
// entry scattered to its surface's columns, dense rows copied — and thread t
// sums column t over the 16 chunks in order. The sparse entries and Σ d² are
// one coalesced, unconditional read each (whatever the header says), issued
// before the headers are known: one memory latency per group. Deterministic,
// and it reads only the chunk rows: independent of the plan.
// (Gathering entry columns straight from the chunk rows — a thread per entry,
// a lane per chunk — touches 64 lines per wave load: 17 us at 2^17 points,
// 70 us at 2^20, tag-lookup bound on the few CUs the 49 tiles occupy.)
constexpr int kGroupChunks = 16;
constexpr int kGroupBlock = 512;
static_assert(kGroupChunks * 24 <= kGroupBlock, "one sparse entry per thread");
__global__ __launch_bounds__(kGroupBlock) void chunk_groups_kernel(const I4* __restrict__ hdr,
                                                                   const double* __restrict__ ent,
                                                                   const double* __restrict__ csum,
                                                                   const double* __restrict__ dense, int nc, int S,
                                                                   double* __restrict__ partials, int ngroups,
                                                                   const int* __restrict__ skip) {
  if (skip && *skip) return;
  const int len = 1 + 6 * S;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int c0 = g * kGroupChunks;
  double* tab = (double*)fsdf_lds;                // [kGroupChunks][len]
  I4* sh = (I4*)(tab + kGroupChunks * len);       // [kGroupChunks] headers
  const int ec = tid / 24;                         // this thread's sparse entry: chunk c0 + ec, slot (tid % 24) / 6
  const bool inr = tid < kGroupChunks * 24 && c0 + ec < nc;
  const double v = ent[inr ? (int64_t)c0 * 24 + tid : 0];
  const int hc = c0 + (tid & (kGroupChunks - 1));
  const bool hv = hc < nc;
  const I4 h = hdr[hv ? hc : 0];
  const double cs = csum[hv ? hc : 0];
  for (int i = tid; i < kGroupChunks * len; i += kGroupBlock) tab[i] = 0.0;
  if (tid < kGroupChunks) sh[tid] = hv ? h : I4{-1, -1, -1, -1};
  __syncthreads();
  if (tid < kGroupChunks && hv) tab[tid * len] = cs;
  if (inr) {
    const I4 hh = sh[ec];
    const int sl = (tid % 24) / 6, j = tid % 6;
    const int k = sl == 0 ? hh[0] : (sl == 1 ? hh[1] : (sl == 2 ? hh[2] : hh[3]));
    if (hh[0] != -2 && k >= 0 && k < S) tab[ec * len + 1 + 6 * k + j] = v;
  }
  // dense rows (a chunk that met more than 4 surfaces): entry 1 + i = dense[i]
  for (int c = 0; c < kGroupChunks; ++c) {
    if (sh[c][0] == -2)
      for (int i = tid; i < 6 * S; i += kGroupBlock) tab[c * len + 1 + i] = dense[(int64_t)(c0 + c) * 6 * S + i];
  }
  __syncthreads();
  for (int t = tid; t < len; t += kGroupBlock) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < kGroupChunks; ++c) s += tab[c * len + t];
    partials[pidx(t, g, ngroups)] = s;
  }
}

// The plan for the next passes (one workgroup, kPlanBlock threads): a counting
// sort of the chunks' serial-equivalent durations into kPlanBuckets buckets,
// heaviest first; the first n4 chunks of that order get a workgroup each (4
// waves), the next n2 one per 2 waves (pairs of similar cost), the rest one
// wave each in groups of 4 consecutive (similar cost: little idle inside a
// workgroup). Workgroups are listed in that order — heaviest first, longest-
// processing-time-first list scheduling. `order` is [nc] scratch.
constexpr int kPlanBlock = 1024;
constexpr int kPlanBuckets = 256;
__global__ __launch_bounds__(kPlanBlock) void plan_kernel(const uint32_t* __restrict__ dur, int nc, int n4, int n2,
                                                          int32_t* __restrict__ order, I4* __restrict__ plan) {
  __shared__ unsigned hist[kPlanBuckets];
  __shared__ unsigned wmax[kPlanBlock / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned mx = 0;
  for (int c = t; c < nc; c += kPlanBlock) mx = max(mx, dur[c]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off, 64));
  if (lane == 0) wmax[w] = mx;
  for (int b = t; b < kPlanBuckets; b += kPlanBlock) hist[b] = 0;
  __syncthreads();
  mx = 0;
  for (int j = 0; j < kPlanBlock / 64; ++j) mx = max(mx, wmax[j]);
  const float sc = (float)(kPlanBuckets - 1) / (float)(mx ? mx : 1u);
  auto bucket = [&](int c) { return kPlanBuckets - 1 - min(kPlanBuckets - 1, (int)((float)dur[c] * sc)); };
  for (int c = t; c < nc; c += kPlanBlock) atomicAdd(&hist[bucket(c)], 1u);
  __syncthreads();
  if (t == 0) {  // exclusive scan (256 buckets, once per plan)
    unsigned acc = 0;
    for (int b = 0; b < kPlanBuckets; ++b) {
      const unsigned h = hist[b];
      hist[b] = acc;
      acc += h;
    }
  }
  __syncthreads();
  for (int c = t; c < nc; c += kPlanBlock) order[atomicAdd(&hist[bucket(c)], 1u)] = c;
  __threadfence();
  __syncthreads();
  const int n1 = nc - n4 - n2;
  const int g2 = n2 / 2 + (n2 & 1), g1 = (n1 + 3) / 4;
  for (int b = t; b < n4 + g2 + g1; b += kPlanBlock) {
    I4 e = I4{-1, -1, -1, -1};
    if (b < n4) {
      e[0] = order[b] | (4 << kPlanPartsShift);
    } else if (b < n4 + g2) {
      const int p0 = n4 + 2 * (b - n4);
      e[0] = order[p0] | (2 << kPlanPartsShift);
      if (p0 + 1 < n4 + n2) e[1] = order[p0 + 1];
    } else {
      const int p0 = n4 + n2 + 4 * (b - n4 - g2);
      e[0] = order[p0] | (1 << kPlanPartsShift);
      for (int j = 1; j < 4; ++j)
        if (p0 + j < nc) e[j] = order[p0 + j];
    }
    plan[b] = e;
  }
}

// Schedule for the next pass (one workgroup): the workgroups of a pass hold
// their slot until their slowest wave ends and durations vary ~10x (waves
// whose points span several hulls), so launching the logical blocks in index
// order leaves a tail of late heavy blocks. Counting sort of this pass's
// durations into 64 buckets, heaviest first (list scheduling, longest first).
__device__ void build_order(const uint32_t* __restrict__ cost, int nb, int32_t* __restrict__ order) {
  constexpr int kPer = 16;  // costs per thread and tile (tile = 4,096 blocks)
  __shared__ uint8_t bkt[kMaxBlocks];
  __shared__ unsigned hist[64][kBlock / 64];  // [bucket][wave]: 4x less atomic contention
  __shared__ unsigned wmax[kBlock / 64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  unsigned mx = 0;
  for (int b0 = 0; b0 < nb; b0 += kPer * kBlock) {
    unsigned c[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = b0 + u * kBlock + t;
      c[u] = i < nb ? cost[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) mx = max(mx, c[u]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off, 64));
  if (lane == 0) wmax[w] = mx;
  hist[lane][w] = 0;
  __syncthreads();
  mx = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
  const float sc = 63.0f / (float)(mx ? mx : 1u);
  for (int b0 = 0; b0 < nb; b0 += kPer * kBlock) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = b0 + u * kBlock + t;
      if (i < nb) {
        const int b = 63 - min(63, (int)((float)cost[i] * sc));  // 0 = heaviest
        bkt[i] = (uint8_t)b;
        atomicAdd(&hist[b][w], 1u);
      }
    }
  }
  __syncthreads();
  // exclusive scan over (bucket, wave) in bucket-major order: wave 0, lane = bucket
  if (w == 0) {
    const unsigned h0 = hist[lane][0], h1 = hist[lane][1], h2 = hist[lane][2], h3 = hist[lane][3];
    const unsigned tot = h0 + h1 + h2 + h3;
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned o = (unsigned)__shfl_up((int)inc, off, 64);
      if (lane >= off) inc += o;
    }
    const unsigned ex = inc - tot;
    hist[lane][0] = ex;
    hist[lane][1] = ex + h0;
    hist[lane][2] = ex + h0 + h1;
    hist[lane][3] = ex + h0 + h1 + h2;
  }
  __syncthreads();
  for (int b0 = 0; b0 < nb; b0 += kPer * kBlock) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = b0 + u * kBlock + t;
      if (i < nb) order[atomicAdd(&hist[bkt[i]][w], 1u)] = i;
    }
  }
}

// Line-tiled partials: workgroup x (16 waves) sums
// entries 8x .. 8x+7 over all blocks. The tile is read as a flat array of
// 16-B pairs, fully coalesced: thread i reads pairs i + 1024 j (pair e holds
// entries 2 (e & 3), +1 of block e >> 2), 16 loads in flight, so it always
// sums the same two entries over blocks (i >> 2) + 256 j, in order; then per
// entry pair a masked DPP wave sum and a fixed-order 16-wave combine
// (deterministic). The schedule rebuild is a launch of its own (order_kernel).
// (The statements: reduce_tiles_body.inc, shared with batch.hip; kTileBlock: fsdf_internal.h.)
__global__ __launch_bounds__(kTileBlock) void reduce_tiles_kernel(const double* __restrict__ partials, int nblocks,
                                                                  int len, double* __restrict__ accum,
                                                                  const int* __restrict__ skip) {
  if (skip && *skip) return;
#include "reduce_tiles_body.inc"
}

__global__ __launch_bounds__(kBlock) void order_kernel(const uint32_t* __restrict__ cost, int nblocks,
                                                       int32_t* __restrict__ order) {
  build_order(cost, nblocks, order);
}

}  // namespace fsdf
