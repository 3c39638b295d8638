// reduce_tiles_body.inc — the statements of reduce_tiles_kernel
// (reduce_kernels.h), included textually into that kernel and into
// batch_reduce_tiles_kernel (batch.hip), for robust_body.inc's reason: the same
// tokens, the same instructions, the same sums. The including kernel runs
// kTileBlock threads, includes sdf_device_math.h (wave_sum) and has in scope:
// partials (ONE set of line-tiled partials), nblocks, len, accum — a launch with
// a candidate dimension keeps the tile on blockIdx.x and the candidate on grid.y.
  const int x = blockIdx.x;
  typedef double D2 __attribute__((ext_vector_type(2)));
  const D2* tile = (const D2*)(partials + (int64_t)x * nblocks * 8);
  const int np = 4 * nblocks;  // pairs in the tile
  double s0 = 0.0, s1 = 0.0;
  int e = threadIdx.x;
  // U loads in flight per thread, the last batch predicated (a serial tail
  // loop cost one L2 round trip per pair: 5.5 us at 2^17 points, where a
  // thread has 8 pairs). Same addition order; the missing pairs add +0.0,
  // which leaves a sum that started at +0.0 bit for bit unchanged.
  constexpr int U = 16;
  for (; e < np; e += U * kTileBlock) {
    D2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = e + u * kTileBlock;
      v[u] = i < np ? tile[i] : D2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { s0 += v[u][0]; s1 += v[u][1]; }
  }
  constexpr int W = kTileBlock / 64;
  __shared__ double sh[8][W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & 3;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double w0 = wave_sum(q == r ? s0 : 0.0), w1 = wave_sum(q == r ? s1 : 0.0);
    if (lane == 0) { sh[2 * r][wave] = w0; sh[2 * r + 1][wave] = w1; }
  }
  __syncthreads();
  const int t = 8 * x + (int)threadIdx.x;
  if (threadIdx.x < 8 && t < len) {
    double a[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      a[g] = (sh[threadIdx.x][4 * g] + sh[threadIdx.x][4 * g + 1]) + (sh[threadIdx.x][4 * g + 2] + sh[threadIdx.x][4 * g + 3]);
    accum[t] = (a[0] + a[1]) + (a[2] + a[3]);
  }
