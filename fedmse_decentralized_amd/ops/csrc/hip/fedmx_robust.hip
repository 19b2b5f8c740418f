// Robust aggregation (update types trimmed_mean / median): per-coordinate
// order-statistic selection over the k gathered models.
//
//  * robust_agg_kernel : for every coordinate i, rank the k values
//                          theta_{row_j}[i] under the total order
//                          -inf < ... < -0 < +0 < ... < +inf < NaN (ties by
//                          selection position: a stable argsort), keep the
//                          models with t <= rank < k - t, add the kept values
//                          in selection order (separately rounded fp32 adds,
//                          starting from the first kept value) and divide
//                          (IEEE) by k - 2t.  t = 0 is the plain mean's
//                          sum / k; t = (k - 1) / 2 is the median.
//
// Unlike the four linear rules this is not sum_j w_j * theta_j, so it cannot
// ride elect_wsum_kernel's weighted sum: the device round launches it right
// behind that kernel, over the same row table and election state, and it
// overwrites the aggregate.  Like every kernel after the election it is a
// no-op when no aggregator was elected (state[0] < 0).
//
// A workgroup owns W consecutive coordinates.  The k x W tile is staged in
// LDS as sortable 32-bit keys, [k][W] so lane-consecutive coordinates sit in
// consecutive banks; the k rank computations of a coordinate are spread over
// the workgroup's 256 / W lane groups (each thread ranks up to four models
// per sweep of the tile column, one LDS read serving four compares); a kept
// flag per (model, coordinate) then feeds one in-order sum per coordinate.
// W shrinks with k so that the tile is 32 KiB whatever k is:
// W = 32 / 16 / 8 for k <= 256 / 512 / 1024 (48 KiB of LDS per workgroup
// with the flags and the row table, three workgroups per CU).
#include "fedmx_common.h"

namespace fedmx {

constexpr int ROBUST_MAX_K = 1024;
constexpr uint32_t ROBUST_KEY_NAN = 0xFFFFFFFFu;

// float bits -> key whose unsigned order is the total order above
__device__ __forceinline__ uint32_t robust_key(uint32_t b) {
  uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) key = ROBUST_KEY_NAN;
  return key;
}

// the value back from its key (every NaN comes back as the canonical quiet NaN)
__device__ __forceinline__ float robust_value(uint32_t key) {
  uint32_t b = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  if (key == ROBUST_KEY_NAN) b = 0x7FC00000u;
  return __builtin_bit_cast(float, b);
}

template <int W, int KMAX>
__global__ __launch_bounds__(256) void robust_agg_kernel(const uint32_t* __restrict__ base,
                                                         const int64_t* __restrict__ rows,
                                                         const int32_t* __restrict__ state, float* __restrict__ out,
                                                         int k, int P, int t) {
  static_assert(256 % W == 0 && KMAX * W == 8192, "a 32 KiB key tile whatever the width");
  constexpr int G = 256 / W;   // lane groups: each takes every G-th model
  __shared__ uint32_t s_key[KMAX * W];
  __shared__ uint8_t s_kept[KMAX * W];
  __shared__ int64_t s_rows[KMAX];
  if (state != nullptr && state[0] < 0) return;   // no aggregator this round (uniform)
  const int tid = threadIdx.x;
  const int c = tid % W, g = tid / W;
  const int i = blockIdx.x * W + c;
  const bool live = i < P;
  // the row table may live in mapped host memory: one parallel load
  for (int j = tid; j < k; j += 256) s_rows[j] = rows != nullptr ? rows[j] : (int64_t)j;
  __syncthreads();
  // stage the tile: up to 8 row segments per thread in flight before the first
  // use (unconditional loads: a model or coordinate past the end re-reads the
  // last one, and its key is never stored / never summed)
  constexpr int U = 8;
  const int ic = live ? i : P - 1;
  for (int j0 = g; j0 < k; j0 += G * U) {
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = min(j0 + u * G, k - 1);
      v[u] = base[(size_t)s_rows[j] * P + ic];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * G;
      if (j < k) s_key[j * W + c] = robust_key(v[u]);
    }
  }
  __syncthreads();
  // rank_j = #{l : key_l < key_j or (key_l == key_j and l < j)}; kept iff t <= rank_j < k - t
  constexpr int JU = 4;
  for (int j0 = g; j0 < k; j0 += G * JU) {
    // (as one 64-bit compare of (key, position) pairs: a compare and an add
    // per pair, no lane-mask arithmetic)
    uint64_t mk[JU];
    int rk[JU];
#pragma unroll
    for (int u = 0; u < JU; ++u) {
      mk[u] = ((uint64_t)s_key[min(j0 + u * G, k - 1) * W + c] << 32) | (uint32_t)(j0 + u * G);
      rk[u] = 0;
    }
#pragma unroll 2
    for (int l = 0; l < k; ++l) {
      const uint64_t kl = ((uint64_t)s_key[l * W + c] << 32) | (uint32_t)l;
#pragma unroll
      for (int u = 0; u < JU; ++u) rk[u] += kl < mk[u] ? 1 : 0;
    }
#pragma unroll
    for (int u = 0; u < JU; ++u) {
      const int j = j0 + u * G;
      if (j < k) s_kept[j * W + c] = (rk[u] >= t && rk[u] < k - t) ? 1 : 0;
    }
  }
  __syncthreads();
  if (g != 0 || !live) return;
  // the kept values in selection order, one rounding per add
  float acc = 0.f;
  bool first = true;
  for (int j = 0; j < k; ++j) {
    if (s_kept[j * W + c]) {
      const float v = robust_value(s_key[j * W + c]);
      acc = first ? v : __fadd_rn(acc, v);
      first = false;
    }
  }
  out[i] = __fdiv_rn(acc, (float)(k - 2 * t));
}

}  // namespace fedmx

extern "C" {

int fedmx_robust_max_k() { return fedmx::ROBUST_MAX_K; }

// out[i] = trimmed mean (trim count t per side) over base[rows[j]][i], j < k
// (rows null: rows 0..k-1); state null or state[0] >= 0, else nothing is written
int fedmx_robust_agg(const float* base, const int64_t* rows, const int32_t* state, float* out, int k, int P, int t,
                     hipStream_t stream) {
  if (k < 1 || k > fedmx::ROBUST_MAX_K || P < 1 || t < 0 || 2 * t >= k) return -1;
  const uint32_t* b = reinterpret_cast<const uint32_t*>(base);
  if (k <= 256)
    hipLaunchKernelGGL((fedmx::robust_agg_kernel<32, 256>), dim3((P + 31) / 32), dim3(256), 0, stream, b, rows, state,
                       out, k, P, t);
  else if (k <= 512)
    hipLaunchKernelGGL((fedmx::robust_agg_kernel<16, 512>), dim3((P + 15) / 16), dim3(256), 0, stream, b, rows, state,
                       out, k, P, t);
  else
    hipLaunchKernelGGL((fedmx::robust_agg_kernel<8, 1024>), dim3((P + 7) / 8), dim3(256), 0, stream, b, rows, state,
                       out, k, P, t);
  return (int)hipGetLastError();
}

}  // extern "C"
