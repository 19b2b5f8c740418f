// Nearest-neighbour latent scorer on gfx950 (README "Latent scorers"; not in
// the reference): the score of a query latent is its Euclidean distance to
// the k-th nearest of its client's training latents, both under the scaler
// that cen_score_kernel fits (fedmx_scaler_fit.h).
//
//   scaled value : t0 = fp32((double)v - mean), t1 = fp32((double)t0 / scale),
//                  for train rows and query rows alike
//   d2(q, x)     : sum over c = 0..Z-1, in that order, of ((double)q_c - (double)x_c)^2
//                  in float64 from 0 (the rows are compared directly: the
//                  |q|^2 + |x|^2 - 2 q.x form cancels on exactly the small
//                  distances this scorer lives on); NaN counts as +inf
//   score        : sqrt of the min(k, n_train)-th smallest d2, duplicates
//                  counted with multiplicity
//
// One descriptor per (train set, query set) pair, grid (n_desc, Y): the query
// rows are split over Y workgroups of 256 threads, each of which refits the
// scaler.  A workgroup walks the train set in tiles of KNN_TILE_ROWS scaled
// rows staged in LDS as [row][ZP] float64 (the fp32-rounded values, widened
// once at staging so the scan's inner loop is a subtract and an FMA per
// column and no conversion).  Every lane reads the same train row, so each
// ds_read_b128 is one address for the whole wave: a broadcast, no bank
// conflict whatever the row stride.  Each thread owns one query row per pass
// and keeps its K smallest d2 in a sorted register list; the common case per
// train row is one compare against the list's last entry.
//
// LDS: KNN_TILE_ROWS * ZP * 8 B = 60 KiB of tile + 768 B of scaler state, so
// two workgroups share a CU's 160 KB (two waves per SIMD, which is what hides
// the LDS latency under the float64 VALU work); __launch_bounds__(256, 2)
// gives the register allocator the matching 256 VGPRs.
#include "fedmx_common.h"
#include "fedmx_scaler_fit.h"

namespace fedmx {

struct KnnDesc {
  const float* train_lat;  // [n_train, train_stride]
  const float* query_lat;  // [n_query, query_stride]
  double* out;             // [n_query]
  int32_t n_train;
  int32_t n_query;
  int32_t latent;
  int32_t k;
  int32_t train_stride;
  int32_t query_stride;
};
static_assert(sizeof(KnnDesc) == 48, "KnnDesc layout is shared with Python");

constexpr int KNN_TILE_ROWS = 480;
constexpr int KNN_MAX_K = 16;
constexpr int KNN_THREADS = 256;

typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double knn_scaled(float v, double mean, double scale) {
  const float t0 = (float)((double)v - mean);
  const float t1 = (float)((double)t0 / scale);
  return (double)t1;
}

// Sorted insert of d2 into best[0..K) (ascending); a NaN fails the compare
// and is never inserted, which is what counting it as +inf means.
template <int K>
__device__ __forceinline__ void knn_insert(double (&best)[K], double d2) {
  if (d2 < best[K - 1]) {
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
      const double lo = best[j - 1];
      best[j] = (d2 < lo) ? lo : ((d2 < best[j]) ? d2 : best[j]);
    }
    best[0] = (d2 < best[0]) ? d2 : best[0];
  }
}

// One tile against this thread's query row; G = ceil(Z / 4) column groups
// (the tile's and the query's columns Z.. hold 0, which adds an exact +0).
template <int K, int G>
__device__ __forceinline__ void knn_scan_tile(const double* __restrict__ s_tile, int rows, const double (&q)[ZP],
                                              double (&best)[K]) {
#pragma unroll 2
  for (int r = 0; r < rows; ++r) {
    const f64x2* x = reinterpret_cast<const f64x2*>(s_tile + r * ZP);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 2 * G; ++c) {
      const f64x2 xv = x[c];
      const double d0 = q[2 * c] - xv.x;
      acc = __builtin_fma(d0, d0, acc);
      const double d1 = q[2 * c + 1] - xv.y;
      acc = __builtin_fma(d1, d1, acc);
    }
    knn_insert<K>(best, acc);
  }
}

template <int K>
__global__ __launch_bounds__(KNN_THREADS, 2) void knn_score_kernel(const KnnDesc* __restrict__ descs) {
  const KnnDesc d = descs[blockIdx.x];
  __shared__ __attribute__((aligned(16))) double s_tile[KNN_TILE_ROWS * ZP];
  __shared__ double s_red[4 * ZP];
  __shared__ double s_mean[ZP];
  __shared__ double s_scale[ZP];
  const int tid = threadIdx.x;
  const int m = d.latent;
  // (uniform over the workgroup: no query rows for it, or nothing to compare with)
  if ((int)blockIdx.y * KNN_THREADS >= d.n_query || d.n_train <= 0) return;
  fit_standard_scaler(d.train_lat, d.n_train, d.train_stride, m, s_red, s_mean, s_scale);
  // staging: thread tid scales column tid & 15 of rows tid >> 4, +16, ...
  const int sc = tid & (ZP - 1);
  const double c_mean = (sc < m) ? s_mean[sc] : 0.0;
  const double c_scale = (sc < m) ? s_scale[sc] : 1.0;
  const int groups = (m + 3) >> 2;
  const int k_eff = min(min(max(d.k, 1), K), d.n_train);
  int staged = -1;
  for (int base = blockIdx.y * KNN_THREADS; base < d.n_query; base += KNN_THREADS * gridDim.y) {
    const int r = base + tid;
    double q[ZP];
#pragma unroll
    for (int c = 0; c < ZP; ++c)
      q[c] = (r < d.n_query && c < m)
                 ? knn_scaled(d.query_lat[(size_t)r * d.query_stride + c], s_mean[c], s_scale[c])
                 : 0.0;
    double best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = INFINITY;
    for (int t0 = 0; t0 < d.n_train; t0 += KNN_TILE_ROWS) {
      const int rows = min(KNN_TILE_ROWS, d.n_train - t0);
      if (staged != t0) {   // (a train set of one tile is staged once for every pass)
        __syncthreads();
        for (int e = tid; e < rows * ZP; e += KNN_THREADS) {
          const int row = t0 + (e >> 4);
          s_tile[e] = (sc < m) ? knn_scaled(d.train_lat[(size_t)row * d.train_stride + sc], c_mean, c_scale) : 0.0;
        }
        __syncthreads();
        staged = t0;
      }
      switch (groups) {
        case 1: knn_scan_tile<K, 1>(s_tile, rows, q, best); break;
        case 2: knn_scan_tile<K, 2>(s_tile, rows, q, best); break;
        case 3: knn_scan_tile<K, 3>(s_tile, rows, q, best); break;
        default: knn_scan_tile<K, 4>(s_tile, rows, q, best); break;
      }
    }
    double sel = best[0];
#pragma unroll
    for (int j = 1; j < K; ++j)
      if (j < k_eff) sel = best[j];
    if (r < d.n_query) d.out[r] = sqrt(sel);
  }
}

template <int K>
static int knn_launch(const KnnDesc* descs, int n, int y, hipStream_t stream) {
  hipLaunchKernelGGL(knn_score_kernel<K>, dim3(n, y), dim3(KNN_THREADS), 0, stream, descs);
  return (int)hipGetLastError();
}

}  // namespace fedmx

extern "C" {

// k: the launch's list capacity, at least every descriptor's k (a descriptor
// with a smaller k is still scored at its own k); y: workgroups per descriptor.
int fedmx_knn_score(const void* descs, int n, int k, int y, hipStream_t stream) {
  if (n <= 0) return 0;
  if (y < 1 || y > 65535) return (int)hipErrorInvalidValue;
  const fedmx::KnnDesc* p = reinterpret_cast<const fedmx::KnnDesc*>(descs);
  switch (k) {
#define FEDMX_KNN_CASE(K) case K: return fedmx::knn_launch<K>(p, n, y, stream);
    FEDMX_KNN_CASE(1) FEDMX_KNN_CASE(2) FEDMX_KNN_CASE(3) FEDMX_KNN_CASE(4)
    FEDMX_KNN_CASE(5) FEDMX_KNN_CASE(6) FEDMX_KNN_CASE(7) FEDMX_KNN_CASE(8)
    FEDMX_KNN_CASE(9) FEDMX_KNN_CASE(10) FEDMX_KNN_CASE(11) FEDMX_KNN_CASE(12)
    FEDMX_KNN_CASE(13) FEDMX_KNN_CASE(14) FEDMX_KNN_CASE(15) FEDMX_KNN_CASE(16)
#undef FEDMX_KNN_CASE
    default: return (int)hipErrorInvalidValue;
  }
}

int fedmx_knn_desc_size() { return (int)sizeof(fedmx::KnnDesc); }
int fedmx_knn_tile_rows() { return fedmx::KNN_TILE_ROWS; }
int fedmx_knn_max_k() { return fedmx::KNN_MAX_K; }

}  // extern "C"
