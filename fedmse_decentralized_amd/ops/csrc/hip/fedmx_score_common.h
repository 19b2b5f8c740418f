// What score_rows_kernel (fedmx_score.hip) and explain_rows_kernel
// (fedmx_explain.hip) share, so that both standardise a raw value to the same
// bits: the descriptor flag bits, the workgroup geometry and the per-feature
// standardisation.
#pragma once
#include "fedmx_common.h"
#include <float.h>

namespace fedmx {

constexpr int SCORE_RAW_F64 = 1;   // raw rows are float64 (else float32)
constexpr int SCORE_MINMAX = 2;    // feature scaler is minmax (else standard)
constexpr int SCORE_KIND_AE = 4;   // score = mean squared reconstruction error
constexpr int SCORE_KIND_CEN = 8;  // score = scaled latent's distance to the origin
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_WAVES = SCORE_THREADS / 64;
constexpr int SCORE_TILE = 16;     // rows of one wave's tile (the MFMA batch)

__device__ __forceinline__ double score_clean(double v) {
  // numpy.nan_to_num: nan -> 0, +-inf -> +-DBL_MAX
  if (v != v) return 0.0;
  if (v == INFINITY) return DBL_MAX;
  if (v == -INFINITY) return -DBL_MAX;
  return v;
}

// One feature, as IoTDataProcessor.transform(...).astype(float32) computes it.
template <bool MINMAX>
__device__ __forceinline__ float score_standardise(double x, double a, double b) {
#pragma clang fp contract(off)
  if (MINMAX) {
    const double m = x * a;   // rounded on its own: X *= scale_; X += min_
    return (float)(m + b);
  }
  const double s = x - a;     // X -= mean_; X /= scale_
  return (float)(s / b);
}

}  // namespace fedmx
