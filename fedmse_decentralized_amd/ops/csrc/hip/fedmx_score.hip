// Deployed-detector scoring on gfx950 (README "Deploying a detector"; not in
// the reference): raw feature rows in, anomaly scores and alarm flags out, in
// one launch.
//
// One descriptor per (detector, block of raw rows).  A 256-thread workgroup
// stages its detector's weights in LDS (stage_params, 40 KB) and then its four
// waves work independently, each on 16-row tiles of the block (wave w takes
// tiles w, w + 4, ...), with no workgroup barrier in the loop:
//   standardise : the tile's raw values (row-major [n, D], float64 or float32,
//                 rows only element-aligned) become fp32 in the wave's LDS
//                 tile [16][DP]; lane l owns columns l and l + 64, whose scaler
//                 constants it keeps in registers for the whole block
//                   standard: fp32(((double)x - mean) / scale)   (IEEE f64 divide)
//                   minmax  : fp32(((double)x * scale) + min)    (no contraction)
//                 and columns D.. hold 0 (pad_features)
//   forward     : fwd_rows_block on that tile (the forward of fwd_rows_kernel:
//                 same bits), per-row SSE and latents to LDS
//   score       : lanes 0..15, one row each
//                   AE  : (double)(sse * score_scale) in fp32, score_scale = fp32(1 / D)
//                   CEN : cen_score_kernel's per-row loop with the descriptor's
//                         stored mean / scale
//                 cleaned (NaN -> 0, +-inf -> +-DBL_MAX), flagged iff
//                 score > threshold (false for a NaN threshold)
//   write       : float64 scores, uint8 flags, optionally the fp32 latents
// A wave counts its alarms in a register; the workgroup adds them to the
// detector's counter with one integer atomic at the end.
//
// LDS: 40,192 B of weights + 4 x (8 KB tile + 64 B SSE + 1 KB latents) + 256 B
// of latent scaler = 76.8 KB, so two workgroups share a CU's 160 KB.
#include "fedmx_forward_common.h"
#include "fedmx_score_common.h"

namespace fedmx {

struct ScoreDesc {
  const float* params;    // [P_PAD] padded parameter vector
  const void* raw;        // [nrows, d_in] raw rows of this block (float64 or float32)
  const double* sc_a;     // [d_in] standard: mean_   minmax: scale_
  const double* sc_b;     // [d_in] standard: scale_  minmax: min_
  const double* z_mean;   // [latent] latent scaler (CEN), else null
  const double* z_scale;  // [latent]
  double* score;          // [nrows], or null (latents only)
  uint8_t* flag;          // [nrows], or null
  float* lat;             // [nrows, latent] latents out, or null
  uint32_t* alarms;       // the detector's alarm counter
  double threshold;
  int32_t nrows;
  int32_t d_in;
  int32_t hidden;
  int32_t latent;
  int32_t flags;          // SCORE_* bits
  float score_scale;      // AE: fp32(1 / d_in)
};
static_assert(sizeof(ScoreDesc) == 112, "ScoreDesc layout is shared with Python");

// (flag bits, SCORE_THREADS / SCORE_WAVES / SCORE_TILE, score_clean and
// score_standardise: fedmx_score_common.h, shared with explain_rows_kernel)

template <bool CP, bool F64, bool MINMAX>
__device__ __forceinline__ void score_block(const ScoreDesc& d, const float* sW1, const float* sW2, const float* sW3,
                                            const float* sW4, float* tile, float* s_sse, float* s_lat,
                                            const double* s_zmean, const double* s_zscale, unsigned int& alarms) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int D = d.d_in;
  const bool want_lat = d.lat != nullptr || (d.flags & SCORE_KIND_CEN);
  const bool want_sse = (d.flags & SCORE_KIND_AE) != 0;
  // scaler constants of this lane's two columns (x 1 / + 0 past D: never used)
  const int c0 = lane, c1 = lane + 64;
  const double a0 = c0 < D ? d.sc_a[c0] : 0.0, b0 = c0 < D ? d.sc_b[c0] : 1.0;
  const double a1 = c1 < D ? d.sc_a[c1] : 0.0, b1 = c1 < D ? d.sc_b[c1] : 1.0;
  const int ntiles = (d.nrows + SCORE_TILE - 1) / SCORE_TILE;
  for (int t = wave; t < ntiles; t += SCORE_WAVES) {
    const int r0 = t * SCORE_TILE;
    const int rows = min(SCORE_TILE, d.nrows - r0);
    // ---- standardise: all of the tile's loads first, then the arithmetic
    double v0[SCORE_TILE], v1[SCORE_TILE];
#pragma unroll
    for (int r = 0; r < SCORE_TILE; ++r) {
      const size_t base = (size_t)(r0 + (r < rows ? r : 0)) * (size_t)D;
      if (F64) {
        const double* p = reinterpret_cast<const double*>(d.raw) + base;
        v0[r] = c0 < D ? p[c0] : 0.0;
        v1[r] = c1 < D ? p[c1] : 0.0;
      } else {
        const float* p = reinterpret_cast<const float*>(d.raw) + base;
        v0[r] = c0 < D ? (double)p[c0] : 0.0;
        v1[r] = c1 < D ? (double)p[c1] : 0.0;
      }
    }
#pragma unroll
    for (int r = 0; r < SCORE_TILE; ++r) {
      tile[r * DP + c0] = c0 < D ? score_standardise<MINMAX>(v0[r], a0, b0) : 0.0f;
      tile[r * DP + c1] = c1 < D ? score_standardise<MINMAX>(v1[r], a1, b1) : 0.0f;
    }
    wave_sync();
    // ---- forward: this wave alone, its one tile
    FwdDesc f;
    f.params = d.params;
    f.x = tile;
    f.sse = nullptr;
    f.lat = want_lat ? s_lat : nullptr;
    f.nrows = rows;
    f.lat_stride = ZP;
    f.d_in = D;
    f.latent = d.latent;
    f.hidden = d.hidden;
    fwd_rows_block<CP, false>(f, sW1, sW2, sW3, sW4, 0, 1, want_sse ? s_sse : nullptr);
    wave_sync();
    // ---- score, clean, compare, write
    if (d.score != nullptr) {
      bool flagged = false;
      if (lane < rows) {
        double s;
        if (want_sse) {
          s = (double)(s_sse[lane] * d.score_scale);
        } else {
          double acc = 0.0;
          for (int j = 0; j < d.latent; ++j) {
            const float t0 = (float)((double)s_lat[lane * ZP + j] - s_zmean[j]);
            const float t1 = (float)((double)t0 / s_zscale[j]);
            const double v = (double)t1;
            acc += v * v;
          }
          s = sqrt(acc);
        }
        s = score_clean(s);
        flagged = s > d.threshold;   // false for every row when the threshold is NaN
        d.score[r0 + lane] = s;
        d.flag[r0 + lane] = flagged ? 1 : 0;
      }
      alarms += (unsigned int)__popcll(__ballot(flagged));
    }
    if (d.lat != nullptr) {
      // lane (row = lane & 15, g = lane >> 4) copies latents g, g + 4, g + 8, g + 12
      const int row = lane & 15, g = lane >> 4;
      if (row < rows) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int z = g + 4 * k;
          if (z < d.latent) d.lat[(size_t)(r0 + row) * d.latent + z] = s_lat[row * ZP + z];
        }
      }
    }
    wave_sync();   // the next tile's writes come after these reads
  }
}

template <bool CP>
__device__ __forceinline__ void score_dispatch(const ScoreDesc& d, const float* sW1, const float* sW2,
                                               const float* sW3, const float* sW4, float* tile, float* s_sse,
                                               float* s_lat, const double* s_zmean, const double* s_zscale,
                                               unsigned int& alarms) {
  const bool f64 = d.flags & SCORE_RAW_F64, mm = d.flags & SCORE_MINMAX;
  if (f64 && !mm) score_block<CP, true, false>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, alarms);
  else if (f64) score_block<CP, true, true>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, alarms);
  else if (!mm) score_block<CP, false, false>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, alarms);
  else score_block<CP, false, true>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, alarms);
}

__global__ __launch_bounds__(SCORE_THREADS, 2) void score_rows_kernel(const ScoreDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) float sW1[HP * S_W1];
  __shared__ __attribute__((aligned(16))) float sW2[ZP * S_W2];
  __shared__ __attribute__((aligned(16))) float sW3[HP * S_W3];
  __shared__ __attribute__((aligned(16))) float sW4[DP * S_W4];
  __shared__ __attribute__((aligned(16))) float s_tile[SCORE_WAVES][SCORE_TILE * DP];
  __shared__ float s_sse[SCORE_WAVES][SCORE_TILE];
  __shared__ float s_lat[SCORE_WAVES][SCORE_TILE * ZP];
  __shared__ double s_zmean[ZP];
  __shared__ double s_zscale[ZP];
  __shared__ unsigned int s_alarms;

  const ScoreDesc d = descs[blockIdx.x];
  if (d.nrows <= 0) return;   // (whole workgroup)
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  FwdDesc shape;
  shape.d_in = d.d_in;
  shape.hidden = d.hidden;
  shape.latent = d.latent;
  const bool compact = fwd_compact_ok(shape);
  if (compact) stage_params<true>(d.params, sW1, sW2, sW3, sW4);
  else stage_params<false>(d.params, sW1, sW2, sW3, sW4);
  if (tid < ZP) {
    const bool cen = (d.flags & SCORE_KIND_CEN) && tid < d.latent;
    s_zmean[tid] = cen ? d.z_mean[tid] : 0.0;
    s_zscale[tid] = cen ? d.z_scale[tid] : 1.0;
  }
  if (tid == 0) s_alarms = 0u;
  __syncthreads();
  unsigned int alarms = 0u;   // wave-uniform
  if (compact)
    score_dispatch<true>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_sse[wave], s_lat[wave], s_zmean, s_zscale, alarms);
  else
    score_dispatch<false>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_sse[wave], s_lat[wave], s_zmean, s_zscale, alarms);
  if ((tid & 63) == 0 && alarms) atomicAdd(&s_alarms, alarms);
  __syncthreads();
  if (tid == 0 && s_alarms) atomicAdd(d.alarms, s_alarms);
}

}  // namespace fedmx

extern "C" {

int fedmx_score_rows(const void* descs, int nblocks, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  hipLaunchKernelGGL(fedmx::score_rows_kernel, dim3(nblocks), dim3(fedmx::SCORE_THREADS), 0, stream,
                     reinterpret_cast<const fedmx::ScoreDesc*>(descs));
  return (int)hipGetLastError();
}

int fedmx_score_desc_size() { return (int)sizeof(fedmx::ScoreDesc); }
int fedmx_score_chunk_rows() { return fedmx::SCORE_WAVES * fedmx::SCORE_TILE; }

}  // extern "C"
