// Calibrated detection threshold and operating-point metrics on gfx950.
//
// One 1024-thread workgroup per client:
//   select : tau = the j-th smallest (0-based) cleaned calibration value, by an
//            MSD radix select over a 64-bit sortable key (sign set -> ~bits,
//            else bits | 1 << 63): eight passes of 8 bits, each a 256-bin u32
//            LDS histogram of the keys that still share the chosen prefix
//            (integer LDS atomics: the result does not depend on arrival
//            order), a scan by the first wave that finds the bin holding rank
//            j, then the prefix grows by that bin.  The calibration values are
//            re-read from global memory each pass (L2 hits), so there is no
//            bound on n_c.  An optional label array filters the calibration
//            rows while reading (keep label == 0: "TPR at x % FPR" calibrates
//            on the test set's normal rows).
//   count  : one strided pass over the test scores, row i flagged iff
//            s_i > tau (strict); per-lane integer counters, wave shuffles, LDS.
//   write  : one lane stores value, tau, tp, fp, fn, tn, precision, recall,
//            `out_stride` doubles apart (struct-of-arrays [8][C]).
// Scores are read exactly as auc_kernel's load_score reads them (fp32 times
// score_scale in fp32, widened; NaN -> 0, +-inf -> +-DBL_MAX).
#include "fedmx_common.h"
#include <float.h>

namespace fedmx {

struct DetectDesc {
  const void* calib;           // float32 or float64 [n_c]
  const int32_t* calib_label;  // optional [n_c]: only rows with label 0 calibrate
  const void* score;           // float32 or float64 [n]
  const int32_t* label;        // [n] (non-zero = abnormal)
  double* out;                 // row 0 of this client's column
  int32_t n_c;
  int32_t n;
  int32_t j;                   // rank among the (filtered) calibration values; < 0: no threshold
  int32_t calib_is_f64;
  int32_t score_is_f64;
  float score_scale;           // multiply float32 values by this (1/D for AE SSE -> mean)
  int32_t value_is_recall;     // row 0: recall (else F1)
  int32_t out_stride;          // doubles between output rows
};
static_assert(sizeof(DetectDesc) == 72, "DetectDesc layout is shared with Python");

constexpr int DET_THREADS = 1024;
constexpr int DET_WAVES = DET_THREADS / 64;

__device__ __forceinline__ double det_clean(double v) {
  // numpy.nan_to_num: nan -> 0, +-inf -> +-DBL_MAX
  if (v != v) return 0.0;
  if (v == INFINITY) return DBL_MAX;
  if (v == -INFINITY) return -DBL_MAX;
  return v;
}

__device__ __forceinline__ double det_load(const void* p, int is_f64, float scale, int i) {
  if (is_f64) return det_clean(reinterpret_cast<const double*>(p)[i]);
  const float f = reinterpret_cast<const float*>(p)[i] * scale;
  return det_clean((double)f);
}

// order-preserving map of a (non-NaN) double onto unsigned integers
__device__ __forceinline__ unsigned long long det_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double det_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k ^ (1ull << 63)) : ~k;
  return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(DET_THREADS) void detect_kernel(const DetectDesc* __restrict__ descs) {
  const DetectDesc d = descs[blockIdx.x];
  __shared__ unsigned int s_hist[2][256];
  __shared__ unsigned int s_sel[3];  // chosen bin, rank inside it, threshold exists
  __shared__ unsigned int s_cnt[DET_WAVES][3];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;

  // ---- select -----------------------------------------------------------------
  if (tid < 256) s_hist[0][tid] = 0u;
  if (tid == 0) s_sel[2] = 0u;
  __syncthreads();
  unsigned long long prefix = 0ull;  // the key's bits chosen so far (above `shift + 8`)
  unsigned int rank = (unsigned int)(d.j < 0 ? 0 : d.j);
  bool have = d.j >= 0 && d.n_c > 0;  // workgroup-uniform
  if (have) {
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      unsigned int* hist = s_hist[pass & 1];
      for (int i = tid; i < d.n_c; i += DET_THREADS) {
        if (d.calib_label != nullptr && d.calib_label[i] != 0) continue;
        const unsigned long long k = det_key(det_load(d.calib, d.calib_is_f64, d.score_scale, i));
        // pass 0 counts every key; later passes those under the chosen prefix
        if (pass == 0 || ((k ^ prefix) >> (shift + 8)) == 0ull) atomicAdd(&hist[(unsigned int)(k >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (wv == 0) {
        // lane l owns bins 4l .. 4l+3: exclusive prefix sum over the lanes, then
        // the one bin with below <= rank < below + count reports itself
        const unsigned int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2],
                           c3 = hist[4 * lane + 3];
        const unsigned int mine = c0 + c1 + c2 + c3;
        unsigned int incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned int up = __shfl_up(incl, o, 64);
          if (lane >= o) incl += up;
        }
        unsigned int below = incl - mine;
        const unsigned int c[4] = {c0, c1, c2, c3};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (rank >= below && rank < below + c[b]) {
            s_sel[0] = (unsigned int)(4 * lane + b);
            s_sel[1] = rank - below;
            s_sel[2] = 1u;
          }
          below += c[b];
        }
      } else if (wv >= 4 && wv < 8) {
        s_hist[(pass + 1) & 1][tid - 256] = 0u;  // the next pass's histogram
      }
      __syncthreads();
      // (rank beyond the filtered count: no bin reported in pass 0, no threshold)
      have = s_sel[2] != 0u;
      if (!have) break;
      prefix |= (unsigned long long)s_sel[0] << shift;
      rank = s_sel[1];
      // (no barrier here: the next scan rewrites s_sel only behind the next
      // pass's histogram barrier, which every thread reaches after these reads)
    }
  }
  double tau = __builtin_nan("");
  if (have) {
    tau = det_unkey(prefix);
    if (tau == 0.0) tau = 0.0;  // a selected -0.0 is reported as +0.0
  }

  // ---- count ------------------------------------------------------------------
  unsigned int tp = 0, fp = 0, pos = 0;
  for (int i = tid; i < d.n; i += DET_THREADS) {
    const double s = det_load(d.score, d.score_is_f64, d.score_scale, i);
    const bool y = d.label[i] != 0;
    const bool flag = s > tau;  // false for every row when tau is NaN
    pos += y ? 1u : 0u;
    tp += (flag && y) ? 1u : 0u;
    fp += (flag && !y) ? 1u : 0u;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    tp += __shfl_xor(tp, o, 64);
    fp += __shfl_xor(fp, o, 64);
    pos += __shfl_xor(pos, o, 64);
  }
  if (lane == 0) {
    s_cnt[wv][0] = tp;
    s_cnt[wv][1] = fp;
    s_cnt[wv][2] = pos;
  }
  __syncthreads();
  if (tid == 0) {
    long long TP = 0, FP = 0, P = 0;
    for (int w = 0; w < DET_WAVES; ++w) {
      TP += s_cnt[w][0];
      FP += s_cnt[w][1];
      P += s_cnt[w][2];
    }
    const long long N = (long long)d.n - P;
    const long long FN = P - TP, TN = N - FP;
    double precision, recall, f1;
    if (!have || P == 0 || N == 0) {
      precision = recall = f1 = __builtin_nan("");
    } else {
      // one f64 division of exactly represented integers each; 0 for an empty denominator
      precision = (TP + FP) ? (double)TP / (double)(TP + FP) : 0.0;
      recall = (TP + FN) ? (double)TP / (double)(TP + FN) : 0.0;
      f1 = (2 * TP + FP + FN) ? (double)(2 * TP) / (double)(2 * TP + FP + FN) : 0.0;
    }
    const size_t st = (size_t)d.out_stride;
    d.out[0] = d.value_is_recall ? recall : f1;
    d.out[st] = tau;
    d.out[2 * st] = (double)TP;
    d.out[3 * st] = (double)FP;
    d.out[4 * st] = (double)FN;
    d.out[5 * st] = (double)TN;
    d.out[6 * st] = precision;
    d.out[7 * st] = recall;
  }
}

}  // namespace fedmx

extern "C" {

int fedmx_detect(const void* descs, int n, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(fedmx::detect_kernel, dim3(n), dim3(fedmx::DET_THREADS), 0, stream,
                     reinterpret_cast<const fedmx::DetectDesc*>(descs));
  return (int)hipGetLastError();
}

int fedmx_detect_desc_size() { return (int)sizeof(fedmx::DetectDesc); }

}  // extern "C"
