// Distance-based robust aggregation (update types krum / multi_krum;
// Blanchard et al. 2017): whole models far from the crowd are discarded.
//
// k models in selection order, each a row of P fp32 values (the whole row
// counts, padding included).  With f models assumed poisoned, q = max(k - f -
// 2, 0) neighbours scored and m models kept (1: krum, k - f: multi_krum):
//
//  * krum_dist_kernel   : d(i, j) for every pair into D[k][k] (f64).  Per
//                           coordinate e = fp32(a - b) (one rounding), s =
//                           (double)e * (double)e (exact in f64); lane l of 256
//                           adds s_l + s_{l+256} + ... sequentially in f64 (the
//                           row zero-extended to a multiple of 256), then the
//                           256 partials fold p_l += p_{l+h}, h = 128 .. 1.
//                           NaN becomes +inf; d(i, j) and d(j, i) are the same
//                           bits; the diagonal is written as 0 and never read.
//  * krum_score_kernel  : model i's k - 1 distances ranked ascending (64-bit
//                           compares of the distance bits: non-negative doubles
//                           and +inf order as unsigned integers; ties by the
//                           smaller j), the q lowest added in order of j in f64.
//  * krum_mean_kernel   : rank_i = #{l : score_l < score_i or (score_l ==
//                           score_i and l < i)}, model i kept iff rank_i < m;
//                           per coordinate the kept rows' values added in
//                           selection order in fp32 (one rounding per add, from
//                           the first kept value), divided (IEEE) by (float)m.
//
// Three launches in stream order, nothing handed over inside a launch: no
// workgroup waits for or reads from another, so no grid needs co-residency.
// Every workgroup of the last kernel derives the selection from the k scores
// for itself (k compares per model, spread over the workgroup); workgroup 0
// also publishes the kept mask and the compacted kept positions.  Like every
// kernel after the election all three are no-ops when no aggregator was
// elected (state[0] < 0).
//
// Distances: a workgroup owns a KRUM_T x KRUM_T tile of pairs.  Lane l loads
// coordinate l + 256c of the tile's 2 * KRUM_T rows once per chunk c (coalesced,
// straight into registers: lane l never needs another lane's coordinate before
// the fold) and feeds KRUM_T^2 f64 accumulators, so every row is read
// ceil(k / KRUM_T) times, not k times.  Only tiles on or above the diagonal
// work; each writes d(i, j) and d(j, i).
#include "fedmx_common.h"

namespace fedmx {

constexpr int KRUM_MAX_K = 1024;
constexpr int KRUM_T = 4;   // pair tile edge: 16 f64 accumulators per lane

__global__ __launch_bounds__(256) void krum_dist_kernel(const float* __restrict__ base,
                                                        const int64_t* __restrict__ rows,
                                                        const int32_t* __restrict__ state, double* __restrict__ D,
                                                        int k, int P) {
  constexpr int T = KRUM_T;
  __shared__ int64_t s_row[2 * T];
  __shared__ double s_p[T * T * 256];
  if (state != nullptr && state[0] < 0) return;   // no aggregator this round (uniform)
  const int I = blockIdx.y, J = blockIdx.x;
  if (I > J) return;                              // d(j, i) comes from tile (I, J)
  const int tid = threadIdx.x;
  // the row table may live in mapped host memory: one load per entry (a row
  // past the end re-reads the last one; its distances are never stored)
  if (tid < 2 * T) {
    const int j = min((tid < T ? I * T : J * T - T) + tid, k - 1);
    s_row[tid] = rows != nullptr ? rows[j] : (int64_t)j;
  }
  __syncthreads();
  const float* ra[T];
  const float* rb[T];
#pragma unroll
  for (int u = 0; u < T; ++u) {
    ra[u] = base + (size_t)s_row[u] * P;
    rb[u] = base + (size_t)s_row[T + u] * P;
  }
  double acc[T][T];
#pragma unroll
  for (int u = 0; u < T; ++u)
#pragma unroll
    for (int v = 0; v < T; ++v) acc[u][v] = 0.0;
  // lane l: coordinates l, l + 256, ... in that order (past P: the zero
  // extension, which adds +0 to a non-negative sum and changes no bit)
#pragma unroll 2
  for (int c = tid; c < P; c += 256) {
    float a[T], b[T];
#pragma unroll
    for (int u = 0; u < T; ++u) {
      a[u] = ra[u][c];
      b[u] = rb[u][c];
    }
#pragma unroll
    for (int u = 0; u < T; ++u)
#pragma unroll
      for (int v = 0; v < T; ++v) {
        const double e = (double)__fsub_rn(a[u], b[v]);
        acc[u][v] = fma(e, e, acc[u][v]);   // e * e is exact in f64: the same bits as multiply, then add
      }
  }
#pragma unroll
  for (int u = 0; u < T; ++u)
#pragma unroll
    for (int v = 0; v < T; ++v) s_p[(u * T + v) * 256 + tid] = acc[u][v];
  __syncthreads();
  // eight folds p_l += p_{l+h} of each pair's 256 partials
  for (int h = 128; h >= 1; h >>= 1) {
    for (int x = tid; x < T * T * h; x += 256) {
      const int pr = x / h, l = x % h;
      s_p[pr * 256 + l] += s_p[pr * 256 + l + h];
    }
    __syncthreads();
  }
  if (tid < T * T) {
    const int i = I * T + tid / T, j = J * T + tid % T;
    if (i < k && j < k) {
      double d = s_p[tid * 256];
      if (d != d) d = __builtin_huge_val();   // NaN -> +inf
      if (i == j) d = 0.0;                    // never read
      D[(size_t)i * k + j] = d;
      if (I != J) D[(size_t)j * k + i] = d;
    }
  }
}

// stable rank by counting: #{l : x_l < x_j or (x_l == x_j and l < j)}
__device__ __forceinline__ int krum_rank(const uint64_t* s_x, int k, int j) {
  const uint64_t mine = s_x[j];
  int r = 0;
#pragma unroll 4
  for (int l = 0; l < k; ++l) {
    const uint64_t x = s_x[l];
    r += (x < mine || (x == mine && l < j)) ? 1 : 0;
  }
  return r;
}

__global__ __launch_bounds__(256) void krum_score_kernel(const uint64_t* __restrict__ D,
                                                         const int32_t* __restrict__ state,
                                                         double* __restrict__ score, int k, int q) {
  __shared__ uint64_t s_d[KRUM_MAX_K];
  __shared__ uint8_t s_keep[KRUM_MAX_K];
  if (state != nullptr && state[0] < 0) return;
  const int tid = threadIdx.x, i = blockIdx.x;
  // d(i, i) takes no part: as the largest key it ranks last, and q <= k - 2
  for (int j = tid; j < k; j += 256) s_d[j] = j == i ? ~0ull : D[(size_t)i * k + j];
  __syncthreads();
  for (int j = tid; j < k; j += 256) s_keep[j] = krum_rank(s_d, k, j) < q ? 1 : 0;
  __syncthreads();
  if (tid != 0) return;
  // the kept distances in order of j, one f64 rounding per add
  double acc = 0.0;
  bool first = true;
  for (int j = 0; j < k; ++j) {
    if (s_keep[j]) {
      const double d = __builtin_bit_cast(double, s_d[j]);
      acc = first ? d : acc + d;
      first = false;
    }
  }
  score[i] = acc;
}

__global__ __launch_bounds__(256) void krum_mean_kernel(const float* __restrict__ base,
                                                        const int64_t* __restrict__ rows,
                                                        const int32_t* __restrict__ state,
                                                        const uint64_t* __restrict__ score, float* __restrict__ out,
                                                        int32_t* __restrict__ kept, int32_t* __restrict__ pos, int k,
                                                        int P, int m) {
  __shared__ uint64_t s_s[KRUM_MAX_K];
  __shared__ int64_t s_krow[KRUM_MAX_K];
  __shared__ uint8_t s_keep[KRUM_MAX_K];
  if (state != nullptr && state[0] < 0) return;
  const int tid = threadIdx.x;
  // the selection, derived by every workgroup for itself from the k scores
  // (sums of non-negative doubles: never NaN, so the bits order as integers)
  for (int j = tid; j < k; j += 256) s_s[j] = score[j];
  __syncthreads();
  for (int j = tid; j < k; j += 256) s_keep[j] = krum_rank(s_s, k, j) < m ? 1 : 0;
  __syncthreads();
  // compact the kept positions (selection order); the row table may live in
  // mapped host memory: one load per kept entry
  for (int j = tid; j < k; j += 256) {
    const int kj = s_keep[j];
    if (kj) {
      int idx = 0;
      for (int l = 0; l < j; ++l) idx += s_keep[l];
      s_krow[idx] = rows != nullptr ? rows[j] : (int64_t)j;
      if (blockIdx.x == 0 && pos != nullptr) pos[idx] = j;
    }
    if (blockIdx.x == 0 && kept != nullptr) kept[j] = kj;
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + tid;
  if (i >= P) return;
  // the kept rows in selection order, one rounding per add, up to 8 loads in flight
  constexpr int U = 8;
  float acc = base[(size_t)s_krow[0] * P + i];
  for (int j0 = 1; j0 < m; j0 += U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = base[(size_t)s_krow[min(j0 + u, m - 1)] * P + i];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (j0 + u < m) acc = __fadd_rn(acc, v[u]);
  }
  out[i] = __fdiv_rn(acc, (float)m);
}

}  // namespace fedmx

extern "C" {

int fedmx_krum_max_k() { return fedmx::KRUM_MAX_K; }
int fedmx_krum_tile() { return fedmx::KRUM_T; }

// out[c] = mean over the m lowest-scored models of base[rows[j]][c], j < k
// (rows null: rows 0..k-1), scores = sums of each model's q = max(k - f - 2, 0)
// smallest distances.  D: f64[k * k], score: f64[k], pos: int32[k] (its first
// m entries are written) workspaces; kept: int32[k] mask or null.  state null
// or state[0] >= 0, else nothing is written.
int fedmx_krum_agg(const float* base, const int64_t* rows, const int32_t* state, float* out, int k, int P, int f,
                   int m, double* D, double* score, int32_t* kept, int32_t* pos, hipStream_t stream) {
  if (k < 1 || k > fedmx::KRUM_MAX_K || P < 1 || f < 0 || m < 1 || m > k || D == nullptr || score == nullptr)
    return -1;
  const int q = k - f - 2 > 0 ? k - f - 2 : 0;
  const int nt = (k + fedmx::KRUM_T - 1) / fedmx::KRUM_T;
  hipLaunchKernelGGL(fedmx::krum_dist_kernel, dim3(nt, nt), dim3(256), 0, stream, base, rows, state, D, k, P);
  hipLaunchKernelGGL(fedmx::krum_score_kernel, dim3(k), dim3(256), 0, stream,
                     reinterpret_cast<const uint64_t*>(D), state, score, k, q);
  hipLaunchKernelGGL(fedmx::krum_mean_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, base, rows, state,
                     reinterpret_cast<const uint64_t*>(score), out, kept, pos, k, P, m);
  return (int)hipGetLastError();
}

}  // extern "C"
