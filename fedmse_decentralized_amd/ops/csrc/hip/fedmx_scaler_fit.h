// The latent scorers' scaler fit, shared by cen_score_kernel (fedmx_eval.hip)
// and knn_score_kernel (fedmx_knn.hip): sklearn StandardScaler on the train
// latents (float64 accumulation, corrected two-pass variance, near-constant
// features -> scale 1), one 256-thread workgroup per fit.
#pragma once
#include "fedmx_common.h"
#include <float.h>

namespace fedmx {

// All latent dimensions are reduced together: one wave-shuffle + LDS pass per
// statistic (3 block reductions instead of 3 per dimension).
__device__ __forceinline__ void block_sum_vec(double* v, int m, double* s_red /*[4][ZP]*/) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < ZP; ++j) {
    if (j >= m) break;
    double x = v[j];
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane == 0) s_red[wv * ZP + j] = x;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < ZP; ++j)
    if (j < m) v[j] = s_red[j] + s_red[ZP + j] + s_red[2 * ZP + j] + s_red[3 * ZP + j];
  __syncthreads();
}

// Fits the scaler of train_lat[n_train, stride] (m real columns) into
// s_mean[ZP] / s_scale[ZP]; every thread of the 256-thread workgroup calls
// it, and the results are visible to all of them on return.
__device__ __forceinline__ void fit_standard_scaler(const float* __restrict__ train_lat, int n_train, int stride,
                                                    int m, double* s_red /*[4][ZP]*/, double* s_mean,
                                                    double* s_scale) {
  const int tid = threadIdx.x;
  double acc[ZP], acc2[ZP];
  // mean (float64 sums of float32 values)
#pragma unroll
  for (int j = 0; j < ZP; ++j) acc[j] = 0.0;
  for (int r = tid; r < n_train; r += blockDim.x) {
    const float* row = train_lat + (size_t)r * stride;
#pragma unroll
    for (int j = 0; j < ZP; ++j)
      if (j < m) acc[j] += (double)row[j];
  }
  block_sum_vec(acc, m, s_red);
  double mean[ZP];
#pragma unroll
  for (int j = 0; j < ZP; ++j) mean[j] = (j < m) ? acc[j] / n_train : 0.0;
  // corrected two-pass variance: (sum (x-m)^2 - (sum (x-m))^2 / n) / n
#pragma unroll
  for (int j = 0; j < ZP; ++j) {
    acc[j] = 0.0;
    acc2[j] = 0.0;
  }
  for (int r = tid; r < n_train; r += blockDim.x) {
    const float* row = train_lat + (size_t)r * stride;
#pragma unroll
    for (int j = 0; j < ZP; ++j) {
      if (j < m) {
        const double df = (double)row[j] - mean[j];
        acc[j] += df;
        acc2[j] += df * df;
      }
    }
  }
  block_sum_vec(acc, m, s_red);
  block_sum_vec(acc2, m, s_red);
  if (tid == 0) {
    const double n = (double)n_train;
#pragma unroll
    for (int j = 0; j < ZP; ++j) {
      if (j >= m) break;
      const double var = (acc2[j] - acc[j] * acc[j] / n) / n;
      const double eps = DBL_EPSILON;
      const double upper = n * eps * var + (n * mean[j] * eps) * (n * mean[j] * eps);
      s_mean[j] = mean[j];
      s_scale[j] = (var <= upper) ? 1.0 : sqrt(var);
    }
  }
  __syncthreads();
}

}  // namespace fedmx
