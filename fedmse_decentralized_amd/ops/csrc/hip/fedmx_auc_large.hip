// Exact ROC-AUC on gfx950 for classes of any size (up to 2^26 rows per pair):
// the multi-workgroup path that takes over where auc_kernel (fedmx_eval.hip)
// answers -1 because the smaller class does not fit its one LDS sort.
//
// The rule is auc_kernel's, cut into chunks.  A score is read as there (fp32
// times score_scale in fp32, widened; f64 as is; NaN -> 0, +-inf -> +-DBL_MAX).
// The smaller class (the positives on a tie) is the sort class with m rows, the
// other one the probe class.  The sort class is split into chunks of at most
// chunk_keys values; per chunk and probe value v, less += #{x in chunk: x < v}
// and eq += #{x in chunk: x == v}.  L and E, the sums over all chunks and
// probes, are unsigned 64-bit integers, so neither the split nor the order
// in which workgroups arrive can change them, and
//   auc = (P N - L - E/2) / (P N)   (sort class = positives)
//   auc = (L + E/2) / (P N)         (sort class = negatives)
// divides the same two exact numbers as the host's rank-sum form.
//
// Four launches on one stream, no workgroup waits for another inside one:
//   count     class counts, one integer atomic per workgroup
//   partition cleaned f64 values into the workspace: sort class in [0, m),
//             probe class in [m, n); slots from two integer cursors, one
//             atomic per wave, class and 512-row tile (ballot + popcount)
//   pairs     grid (chunk, slice, pair): sort the chunk in LDS, search the
//             slice of the probe class in it, one 64-bit atomic each for L, E
//   finalize  one lane per pair: the division, and the counters back to zero
//             (a cached plan relaunches with no memset)
#include "fedmx_common.h"
#include <float.h>

namespace fedmx {
namespace aucl {

struct AucLargeDesc {
  const void* score;        // float32 or float64 [n]
  const int32_t* label;     // [n] (non-zero = positive / abnormal)
  double* out;              // [1]
  double* ws;               // [n] workspace: sort class, then probe class
  unsigned long long* ctr;  // [CTR_WORDS], zero before the first launch
  int32_t n;
  int32_t score_is_f64;
  float score_scale;        // multiply float32 scores by this
  int32_t pad;
};
static_assert(sizeof(AucLargeDesc) == 56, "AucLargeDesc layout is shared with Python");

constexpr int CTR_WORDS = 8;  // P, sort cursor, probe cursor, L, E (+3 spare: one 64-byte line per pair)
constexpr int CTR_P = 0, CTR_SORT = 1, CTR_PROBE = 2, CTR_L = 3, CTR_E = 4;
constexpr int ROW_THREADS = 256;
constexpr int ROW_ITERS = 8;                             // rows per lane and tile
constexpr int ROW_TILE = ROW_THREADS * ROW_ITERS;        // rows per workgroup and pass
constexpr int WAVE_TILE = 64 * ROW_ITERS;                // rows per wave and pass (consecutive)
constexpr int MIN_CHUNK = 64, MAX_CHUNK = 8192;
constexpr int SLICE_MIN_ROWS = 1024;                     // a pair takes at most ceil(probe / this) slices
constexpr int MAX_ROWS = 1 << 26;

__device__ __forceinline__ double clean(double v) {
  // numpy.nan_to_num: nan -> 0, +-inf -> +-DBL_MAX
  if (v != v) return 0.0;
  if (v == INFINITY) return DBL_MAX;
  if (v == -INFINITY) return -DBL_MAX;
  return v;
}

__device__ __forceinline__ double load_score(const AucLargeDesc& d, int i) {
  if (d.score_is_f64) return clean(reinterpret_cast<const double*>(d.score)[i]);
  const float f = reinterpret_cast<const float*>(d.score)[i] * d.score_scale;
  return clean((double)f);
}

__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (row blocks, pairs)
__global__ __launch_bounds__(ROW_THREADS) void auc_large_count_kernel(const AucLargeDesc* __restrict__ descs) {
  const AucLargeDesc d = descs[blockIdx.y];
  __shared__ int s_pos;
  const int tid = threadIdx.x;
  if ((long long)blockIdx.x * ROW_TILE >= d.n) return;   // (the whole workgroup: its first tile is past the end)
  if (tid == 0) s_pos = 0;
  __syncthreads();
  int npos = 0;
  for (long long t0 = (long long)blockIdx.x * ROW_TILE; t0 < d.n; t0 += (long long)gridDim.x * ROW_TILE) {
#pragma unroll
    for (int k = 0; k < ROW_ITERS; ++k) {
      const long long i = t0 + k * ROW_THREADS + tid;
      if (i < d.n) npos += (d.label[i] != 0);
    }
  }
  npos = wave_sum_i(npos);
  if ((tid & 63) == 0) atomicAdd(&s_pos, npos);
  __syncthreads();
  if (tid == 0 && s_pos) atomicAdd(&d.ctr[CTR_P], (unsigned long long)s_pos);
}

// grid (row blocks, pairs); every wave takes tiles of 512 consecutive rows
__global__ __launch_bounds__(ROW_THREADS) void auc_large_partition_kernel(const AucLargeDesc* __restrict__ descs) {
  const AucLargeDesc d = descs[blockIdx.y];
  const long long P = (long long)d.ctr[CTR_P];
  const long long N = (long long)d.n - P;
  if (P <= 0 || N <= 0) return;
  const int sort_pos = (P <= N) ? 1 : 0;
  const int m = (int)(sort_pos ? P : N);
  const int np = d.n - m;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long long t0 = (long long)blockIdx.x * ROW_TILE + wave * WAVE_TILE; t0 < d.n;
       t0 += (long long)gridDim.x * ROW_TILE) {
    // first pass: the labels; the wave's class counts give its two slot ranges
    unsigned long long bs[ROW_ITERS], bp[ROW_ITERS];
    int ns = 0, npr = 0;
#pragma unroll
    for (int k = 0; k < ROW_ITERS; ++k) {
      const long long i = t0 + k * 64 + lane;
      const bool live = i < d.n;
      const bool is_sort = live && ((d.label[live ? i : 0] != 0) == (sort_pos != 0));
      bs[k] = __ballot(is_sort);
      bp[k] = __ballot(live && !is_sort);
      ns += __popcll(bs[k]);
      npr += __popcll(bp[k]);
    }
    unsigned long long base_s = 0, base_p = 0;
    if (lane == 0) {
      if (ns) base_s = atomicAdd(&d.ctr[CTR_SORT], (unsigned long long)ns);
      if (npr) base_p = atomicAdd(&d.ctr[CTR_PROBE], (unsigned long long)npr);
    }
    base_s = __shfl(base_s, 0, 64);
    base_p = __shfl(base_p, 0, 64);
    // second pass: the scores, each into its class's next slot
#pragma unroll
    for (int k = 0; k < ROW_ITERS; ++k) {
      const long long i = t0 + k * 64 + lane;
      const bool mine_s = (bs[k] >> lane) & 1ull;
      const bool mine_p = (bp[k] >> lane) & 1ull;
      if (mine_s) {
        const unsigned long long slot = base_s + (unsigned long long)__popcll(bs[k] & below);
        if (slot < (unsigned long long)m) d.ws[slot] = load_score(d, (int)i);
      } else if (mine_p) {
        const unsigned long long slot = base_p + (unsigned long long)__popcll(bp[k] & below);
        if (slot < (unsigned long long)np) d.ws[(unsigned long long)m + slot] = load_score(d, (int)i);
      }
      base_s += (unsigned long long)__popcll(bs[k]);
      base_p += (unsigned long long)__popcll(bp[k]);
    }
  }
}

// grid (chunks, slices, pairs), 1024 threads, dynamic LDS: chunk_keys doubles + 2 u64
__global__ __launch_bounds__(1024) void auc_large_pairs_kernel(const AucLargeDesc* __restrict__ descs,
                                                               int chunk_keys) {
  const AucLargeDesc d = descs[blockIdx.z];
  extern __shared__ __attribute__((aligned(16))) double keys[];  // [chunk_keys], then the two sums
  unsigned long long* s_acc = reinterpret_cast<unsigned long long*>(keys + chunk_keys);
  const long long P = (long long)d.ctr[CTR_P];
  const long long N = (long long)d.n - P;
  if (P <= 0 || N <= 0) return;
  const int m = (int)((P <= N) ? P : N);
  const int np = d.n - m;
  const int nchunks = (m + chunk_keys - 1) / chunk_keys;
  int nslices = (np + SLICE_MIN_ROWS - 1) / SLICE_MIN_ROWS;
  nslices = min(max(nslices, 1), (int)gridDim.y);
  if ((int)blockIdx.x >= nchunks || (int)blockIdx.y >= nslices) return;
  const int tid = threadIdx.x;
  const int k0 = blockIdx.x * chunk_keys;
  const int len = min(chunk_keys, m - k0);   // >= 1
  const int p0 = (int)(((long long)np * blockIdx.y) / nslices);
  const int p1 = (int)(((long long)np * (blockIdx.y + 1)) / nslices);
  int m2 = 1;
  while (m2 < len) m2 <<= 1;                 // <= chunk_keys (a power of two)
  if (tid < 2) s_acc[tid] = 0ull;
  for (int i = tid; i < m2; i += blockDim.x) keys[i] = (i < len) ? d.ws[k0 + i] : INFINITY;
  __syncthreads();
  // bitonic sort ascending (+inf padding stays at the end)
  for (int k = 2; k <= m2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < m2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const double a = keys[i], b = keys[ixj];
          const bool up = ((i & k) == 0);
          if ((a > b) == up) {
            keys[i] = b;
            keys[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  // for each probe value of the slice: #chunk < v and #chunk == v
  const double* probe = d.ws + m;
  unsigned long long less = 0, eq = 0;
  for (int i = p0 + tid; i < p1; i += blockDim.x) {
    const double v = probe[i];
    int lo = 0, hi = len;  // lower_bound
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    const int lb = lo;
    hi = len;  // upper_bound
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] <= v) lo = mid + 1; else hi = mid;
    }
    less += (unsigned long long)lb;
    eq += (unsigned long long)(lo - lb);
  }
  less = wave_sum_u64(less);
  eq = wave_sum_u64(eq);
  if ((tid & 63) == 0) {
    if (less) atomicAdd(&s_acc[0], less);
    if (eq) atomicAdd(&s_acc[1], eq);
  }
  __syncthreads();
  if (tid == 0) {
    if (s_acc[0]) atomicAdd(&d.ctr[CTR_L], s_acc[0]);
    if (s_acc[1]) atomicAdd(&d.ctr[CTR_E], s_acc[1]);
  }
}

// one lane per pair
__global__ __launch_bounds__(64) void auc_large_finalize_kernel(const AucLargeDesc* __restrict__ descs, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AucLargeDesc d = descs[i];
  const long long P = (long long)d.ctr[CTR_P];
  const long long N = (long long)d.n - P;
  double auc = __builtin_nan("");
  if (P > 0 && N > 0) {
    const double L = (double)d.ctr[CTR_L], E = (double)d.ctr[CTR_E];
    const double pairs = (double)P * (double)N;
    // sorted = positives: pairs (neg v, pos) with pos < v count against the AUC
    auc = (P <= N) ? (pairs - L - 0.5 * E) / pairs : (L + 0.5 * E) / pairs;
  }
  d.out[0] = auc;
  for (int k = 0; k < CTR_WORDS; ++k) d.ctr[k] = 0ull;
}

}  // namespace aucl
}  // namespace fedmx

extern "C" {

// n pairs; max_rows: the largest pair's row count; chunks / slices: the pairs
// kernel's grid (workgroups beyond a pair's own counts leave at once)
int fedmx_auc_large(const void* descs, int n, int max_rows, int chunks, int slices, int chunk_keys,
                    hipStream_t stream) {
  using namespace fedmx::aucl;
  if (n <= 0) return 0;
  if (n > 65535 || max_rows < 0 || max_rows > MAX_ROWS || chunks < 0 || slices < 1 || slices > 65535 ||
      chunk_keys < MIN_CHUNK || chunk_keys > MAX_CHUNK || (chunk_keys & (chunk_keys - 1)))
    return (int)hipErrorInvalidValue;
  const AucLargeDesc* d = reinterpret_cast<const AucLargeDesc*>(descs);
  const size_t lds = (size_t)chunk_keys * sizeof(double) + 2 * sizeof(unsigned long long);
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(auc_large_pairs_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       MAX_CHUNK * (int)sizeof(double) + 2 * (int)sizeof(unsigned long long));
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  if (max_rows > 0) {
    const int tiles = (max_rows + ROW_TILE - 1) / ROW_TILE;
    const int gx = tiles < 2048 ? tiles : 2048;
    hipLaunchKernelGGL(auc_large_count_kernel, dim3(gx, n), dim3(ROW_THREADS), 0, stream, d);
    hipLaunchKernelGGL(auc_large_partition_kernel, dim3(gx, n), dim3(ROW_THREADS), 0, stream, d);
    if (chunks > 0)
      hipLaunchKernelGGL(auc_large_pairs_kernel, dim3(chunks, slices, n), dim3(1024), lds, stream, d, chunk_keys);
  }
  hipLaunchKernelGGL(auc_large_finalize_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d, n);
  return (int)hipGetLastError();
}

int fedmx_auc_large_desc_size() { return (int)sizeof(fedmx::aucl::AucLargeDesc); }
int fedmx_auc_large_ctr_words() { return fedmx::aucl::CTR_WORDS; }
int fedmx_auc_large_slice_min_rows() { return fedmx::aucl::SLICE_MIN_ROWS; }
int fedmx_auc_large_max_rows() { return fedmx::aucl::MAX_ROWS; }

}  // extern "C"
