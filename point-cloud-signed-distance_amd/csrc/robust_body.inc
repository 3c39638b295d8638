// robust_body.inc — the statements of robust_kernel (robust.hip), included
// textually into that kernel and into batch_robust_kernel (batch.hip): one
// workgroup's run of 64-point chunks of ONE cloud's per-point k*, d*, ∇d*
// summed into its partial. The including kernel is a template over
// <T, MOMENTS, WEIGHTED, ONE_SIDED>, declares robust_tab (the dynamic LDS,
// [waves][S][LEN] doubles) and has in scope: pts, kstar, dstar, grad, n, S, run,
// kind, scale, partials, conf, perm, n_surface — each pointer the start of its
// own cloud's (candidate's) array. The workgroup is blockIdx.x of gridDim.x:
// a launch with a candidate dimension keeps it on grid.y.
//
// Why an include and not a __device__ function: robust_kernel has to stay the
// ISA it was. A forced-inline function holding these statements commuted the
// operands of several hundred v_mul_f64 / v_add_f64 and moved registers in
// robust_kernel (the same values, another binary); the same tokens compile to
// the same instructions (DESIGN.md §7 "Batched gradients").
  constexpr int LEN = MOMENTS ? kRobustLen : kRobustTail;
  constexpr bool FACTOR = WEIGHTED || ONE_SIDED;  // a point's terms carry a factor a
  constexpr int M0 = LEN - kRobustTail;  // the wrench's first entry; Σρ at M0 + 6, Σw at M0 + 7
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const int len = LEN * S;
  for (int t = tid; t < waves * len; t += blockDim.x) robust_tab[t] = 0.0;
  __syncthreads();
  double* tab = robust_tab + wave * len;  // this wave's own
  const int share = run / waves;
  const int64_t c0 = (int64_t)blockIdx.x * run + (int64_t)wave * share;
  // each lane's sums over its own points while its k* stays the same (ck: the
  // surface they belong to, -1: none yet), as moments_kernel's
  int ck = -1;
  double acc[LEN];
#pragma unroll
  for (int e = 0; e < LEN; ++e) acc[e] = 0.0;
  // the carried sums into the table: per distinct surface of the wave (that of
  // its first lane still to be summed) a masked wave sum of each entry, entry e
  // ending in lane e (rem is wave-uniform: the sums run with the whole wave active)
  auto flush = [&]() {
    unsigned long long rem = __ballot(ck >= 0);
    while (rem != 0) {
      const int kk = __builtin_amdgcn_readlane(ck, __ffsll((long long)rem) - 1);
      const bool in = ck == kk;
      rem &= ~__ballot(in);
      double mine = 0.0;
#pragma unroll
      for (int e = 0; e < LEN; ++e) {
        const double s = wave_sum(in ? acc[e] : 0.0);
        mine = lane == e ? s : mine;
      }
      if (lane < LEN) tab[LEN * kk + lane] += mine;
    }
    ck = -1;
#pragma unroll
    for (int e = 0; e < LEN; ++e) acc[e] = 0.0;
  };
  for (int r = 0; r < share; ++r) {
    // a lane beyond n, or whose k* is not a surface of the scene, contributes nothing
    const int64_t i = (c0 + r) * 64 + lane;
    int k = -1;
    if (i < n) {
      k = kstar[i];
      if (k < 0 || k >= S) k = -1;
    }
    if (__ballot(k >= 0 && ck >= 0 && k != ck) != 0) flush();
    if (k >= 0) {
      const double px = (double)pts[3 * i], py = (double)pts[3 * i + 1], pz = (double)pts[3 * i + 2];
      const double d = dstar[i];
      double v[6];
      v[0] = grad[3 * i];
      v[1] = grad[3 * i + 1];
      v[2] = grad[3 * i + 2];
      v[3] = py * v[2] - pz * v[1];
      v[4] = pz * v[0] - px * v[2];
      v[5] = px * v[1] - py * v[0];
      double a = WEIGHTED ? conf[i] : 1.0;
      if (ONE_SIDED) a = robust::one_sided_factor(robust::free_sample(perm ? (int64_t)perm[i] : i, n_surface), d, a);
      const double w = FACTOR ? a * robust::weight(kind, scale, d) : robust::weight(kind, scale, d);  // aw
      if (MOMENTS) {
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const double wa = w * v[a];
#pragma unroll
          for (int b = a; b < 6; ++b, ++e) acc[e] += wa * v[b];
        }
      }
      const double t = robust::wrench_scale(w, d);
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[M0 + a] += t * v[a];
      acc[M0 + 6] += FACTOR ? a * robust::rho(kind, scale, d) : robust::rho(kind, scale, d);
      acc[M0 + 7] += w;
      ck = k;
    }
  }
  flush();
  __syncthreads();
  // the waves' tables in wave order: this workgroup's partial, in the line tiles
  // reduce_tiles_kernel reads (pass_kernels.h pidx: entry t of block b at [t / 8][b][t % 8])
  for (int t = tid; t < len; t += blockDim.x) {
    double s = robust_tab[t];
    for (int w = 1; w < waves; ++w) s += robust_tab[w * len + t];
    partials[((int64_t)(t >> 3) * gridDim.x + blockIdx.x) * 8 + (t & 7)] = s;
  }
