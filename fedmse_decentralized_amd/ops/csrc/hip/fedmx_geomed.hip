// Geometric-median aggregation (update type geomed; RFA: Pillutla, Kakade,
// Harchaoui 2019): the smoothed Weiszfeld iteration over the selected models.
// A model is down-weighted continuously with its distance from the crowd; no
// share of poisoned clients is assumed and no whole model is thrown away.
//
// k models in selection order, each a row of P fp32 values (the whole row
// counts, padding included), T = iters in 0..64, nu a finite f64 > 0.  All
// arithmetic is IEEE, one rounding per operation, no contraction.
//
//  * block sum of a length-P f64 vector s: zero-extended to nb = ceil(P / 256)
//    blocks of 256; in block b lane l holds s[256 b + l]; eight folds p_l +=
//    p_{l+h}, h = 128 .. 1, give q_b = p_0; the sum is ((+0.0 + q_0) + q_1) +
//    ... + q_{nb-1} in block order.
//  * lane sum of a length-k f64 vector x: zero-extended to a multiple of 256;
//    lane l adds x_l + x_{l+256} + ... in that order from +0.0; then the same
//    eight folds.
//
//  1. d_i(z): per coordinate e = fp32(theta_i[c] - z[c]) (one rounding), s_c =
//     (double)e * (double)e (exact in f64), d_i the block sum of s; d_i(None)
//     has z = 0.  A d_i that is NaN or +inf is stored as +inf: the row is bad
//     for that step.
//  2. step -1: d_i = d_i(None); beta_i = 1.0 for a finite d_i, else 0.0.
//  3. steps t = 0 .. T: B the lane sum of beta.  B == 0 (every row bad): every
//     w_i = 0.0, every output coordinate the fp32 NaN 0x7FC00000, and the rule
//     ends.  Else w_i = beta_i / B; per coordinate acc = +0.0, and for i = 0 ..
//     k-1 in selection order with beta_i != 0: acc = acc + (w_i *
//     (double)theta_i[c]) (product rounded, then sum rounded); z_t[c] =
//     (float)acc.  t == T stops; else d_i = d_i(z_t), r_i = sqrt(d_i), beta_i =
//     1.0 / max(r_i, nu) for a finite d_i, else 0.0.
//  4. out = z_T; weights[k] the w_i that formed z_T; dist[k] the (squared) d_i
//     those weights came from, +inf for a bad row.
//
// sqrt and the divisions are the correctly rounded f64 operations
// (__dsqrt_rn, __ddiv_rn).
//
// One kernel, geomed_step_kernel, launched T + 2 times in stream order (steps
// -1, 0, .., T).  Nothing is handed over inside a launch: no workgroup waits
// for another, no float atomics, no grid barrier, no co-residency needed.
// Workgroup b (256 threads) owns coordinate block b.  A launch for step t
//   1. folds the previous launch's partials part[nb][k] to d_i in block order
//      (every workgroup for itself), forms beta in LDS, B by the lane sum, w;
//      workgroup 0 of the last launch also publishes weights and dist;
//   2. forms its 256 coordinates of z_t over the k rows in order (eight row
//      loads in flight) and writes them to out, which doubles as the current
//      z: a workgroup keeps its own coordinates in registers for part 3;
//   3. unless t == T goes over its slab of the k rows again, eight rows at a
//      time, and forms each row's block partial q_b: the folds for h = 128 and
//      64 go across the four waves through LDS, those for h <= 32 are wave
//      shuffles (p_l + p_{l+h} either way: the same bits), and lane 0 stores
//      part[b][i].
// The step -1 launch does part 3 only, against z = 0.  Successive launches
// read one half of the partials workspace and write the other (a workgroup of
// launch t may still read block b's partials of launch t - 1 while workgroup b
// writes its new ones).  Like every kernel after the election all launches
// are no-ops when no aggregator was elected (state[0] < 0).
#include "fedmx_common.h"

namespace fedmx {

constexpr int GEOMED_MAX_K = 1024;
constexpr int GEOMED_MAX_ITERS = 64;
constexpr int GEOMED_R = 8;   // rows folded per pass of part 3 (and row loads in flight in part 2)

// eight folds p_l += p_{l+h}, h = 128 .. 1, of R values per lane; the results
// are in lane 0 (wave 0).  s_a: R x 128, s_b: R x 64 doubles.  Two barriers;
// back-to-back calls need none between them (s_a is read before the second
// barrier and rewritten after it, s_b is read before the next first barrier).
template <int R>
__device__ __forceinline__ void geomed_fold(double (&v)[R], double* s_a, double* s_b, int tid) {
  const int wave = tid >> 6;
  if (wave >= 2) {
#pragma unroll
    for (int r = 0; r < R; ++r) s_a[r * 128 + tid - 128] = v[r];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = v[r] + s_a[r * 128 + tid];   // h = 128
  }
  if (wave == 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) s_b[r * 64 + tid - 64] = v[r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double p = v[r] + s_b[r * 64 + tid];                          // h = 64
#pragma unroll
      for (int h = 32; h >= 1; h >>= 1) p = p + __shfl_down(p, h, 64);   // lanes >= h hold values never used
      v[r] = p;
    }
  }
}

// mode bit 0: step -1 (part 3 only, z = 0); bit 1: step 0 (beta_i = 1 for a
// finite d_i); bit 2: step T (no part 3; workgroup 0 publishes weights / dist)
__global__ __launch_bounds__(256) void geomed_step_kernel(const float* __restrict__ base,
                                                          const int64_t* __restrict__ rows,
                                                          const int32_t* __restrict__ state, float* __restrict__ out,
                                                          const double* __restrict__ part_in,
                                                          double* __restrict__ part_out,
                                                          double* __restrict__ weights, double* __restrict__ dist,
                                                          int k, int P, int mode, double nu) {
  constexpr int R = GEOMED_R;
  __shared__ int64_t s_row[GEOMED_MAX_K];
  __shared__ double s_w[GEOMED_MAX_K];      // d_i, then beta_i, then w_i
  __shared__ uint8_t s_on[GEOMED_MAX_K];    // beta_i != 0
  __shared__ double s_a[R * 128];
  __shared__ double s_b[R * 64];
  __shared__ double s_B;
  if (state != nullptr && state[0] < 0) return;   // no aggregator this round (uniform)
  const int tid = threadIdx.x, b = blockIdx.x, nb = gridDim.x;
  const int c = b * 256 + tid;
  const bool in = c < P;                          // past P: the zero extension
  const int cc = in ? c : P - 1;
  const bool first = mode & 1, initial = mode & 2, last = mode & 4;
  // the row table may live in mapped host memory: one load per entry
  for (int j = tid; j < k; j += 256) s_row[j] = rows != nullptr ? rows[j] : (int64_t)j;
  float z = 0.f;
  if (!first) {
    // part 1: d_i in block order, beta_i, B, w_i (thread j % 256 owns entry j throughout)
    const bool publish = b == 0 && last;
    double x[1] = {0.0};
    for (int j = tid; j < k; j += 256) {
      double d = 0.0;
#pragma unroll 4
      for (int bb = 0; bb < nb; ++bb) d = d + part_in[(size_t)bb * k + j];
      const bool finite = d < __builtin_huge_val();   // false for NaN and +inf
      if (!finite) d = __builtin_huge_val();
      double beta = 0.0;
      if (finite) {
        if (initial) {
          beta = 1.0;
        } else {
          const double r = __dsqrt_rn(d);
          beta = __ddiv_rn(1.0, r > nu ? r : nu);
        }
      }
      s_w[j] = beta;
      s_on[j] = beta != 0.0 ? 1 : 0;
      x[0] = x[0] + beta;                             // the lane sum's sequential part
      if (publish && dist != nullptr) dist[j] = d;
    }
    geomed_fold<1>(x, s_a, s_b, tid);
    if (tid == 0) s_B = x[0];
    __syncthreads();
    const double B = s_B;
    for (int j = tid; j < k; j += 256) {
      const double w = B == 0.0 ? 0.0 : __ddiv_rn(s_w[j], B);
      s_w[j] = w;
      if (publish && weights != nullptr) weights[j] = w;
    }
    __syncthreads();
    // part 2: this workgroup's coordinates of z_t
    if (B == 0.0) {
      z = __builtin_bit_cast(float, 0x7FC00000u);
    } else {
      double acc = 0.0;
      for (int j0 = 0; j0 < k; j0 += R) {
        float v[R];
#pragma unroll
        for (int u = 0; u < R; ++u) v[u] = base[(size_t)s_row[min(j0 + u, k - 1)] * P + cc];
#pragma unroll
        for (int u = 0; u < R; ++u)
          if (j0 + u < k && s_on[j0 + u]) acc = acc + s_w[j0 + u] * (double)v[u];
      }
      z = (float)acc;
    }
    if (in) out[c] = z;
    if (last) return;
  } else {
    __syncthreads();   // s_row
  }
  // part 3: each row's block partial of d_i(z_t)
  for (int i0 = 0; i0 < k; i0 += R) {
    float th[R];
#pragma unroll
    for (int u = 0; u < R; ++u) th[u] = base[(size_t)s_row[min(i0 + u, k - 1)] * P + cc];
    double s[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const double e = (double)__fsub_rn(th[u], z);
      s[u] = in ? e * e : 0.0;
    }
    geomed_fold<R>(s, s_a, s_b, tid);
    if (tid == 0) {
#pragma unroll
      for (int u = 0; u < R; ++u)
        if (i0 + u < k) part_out[(size_t)b * k + i0 + u] = s[u];
    }
  }
}

}  // namespace fedmx

extern "C" {

int fedmx_geomed_max_k() { return fedmx::GEOMED_MAX_K; }

// out = z_T of the smoothed Weiszfeld iteration over base[rows[j]], j < k (rows
// null: rows 0..k-1).  part: f64[2 * ceil(P / 256) * k] workspace; weights,
// dist: f64[k] or null.  state null or state[0] >= 0, else nothing is written.
int fedmx_geomed_agg(const float* base, const int64_t* rows, const int32_t* state, float* out, int k, int P,
                     int iters, double nu, double* part, double* weights, double* dist, hipStream_t stream) {
  if (k < 1 || k > fedmx::GEOMED_MAX_K || P < 1 || iters < 0 || iters > fedmx::GEOMED_MAX_ITERS || !(nu > 0.0) ||
      !(nu < __builtin_huge_val()) || part == nullptr)
    return -1;
  const int nb = (P + 255) / 256;
  double* half[2] = {part, part + (size_t)nb * k};
  for (int t = -1; t <= iters; ++t) {
    const int mode = (t == -1 ? 1 : 0) | (t == 0 ? 2 : 0) | (t == iters ? 4 : 0);
    hipLaunchKernelGGL(fedmx::geomed_step_kernel, dim3(nb), dim3(256), 0, stream, base, rows, state, out,
                       half[t & 1], half[(t + 1) & 1], weights, dist, k, P, mode, nu);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
