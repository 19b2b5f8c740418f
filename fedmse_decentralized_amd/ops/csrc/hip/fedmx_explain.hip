// Explaining a deployed detector's alarms on gfx950 (README "Explaining an
// alarm"; not in the reference): raw feature rows in, per row the K features
// the model reconstructed worst with their signed residuals, the row's SSE,
// optionally every residual and, for CEN, the squared scaled latents whose sum
// is the score's square.  One launch, beside score_rows_kernel and with its
// structure:
//
// One descriptor per (detector, block of rows to explain).  A 256-thread
// workgroup stages its detector's weights in LDS (stage_params) and then its
// four waves work independently, each on 16-row tiles of the block (wave w
// takes tiles w, w + 4, ...), with no workgroup barrier in the loop:
//   standardise : as score_rows_kernel (score_standardise: same bits); with
//                 `which` the tile's rows are gathered, row i of the block
//                 being raw row which[i] (any order, repeats allowed; the
//                 host checks the range)
//   forward     : fwd_rows_block on that tile with a sink that keeps the 32
//                 residuals df = y - x each lane forms (columns 16u + 4g + r
//                 of row c; lane = 16g + c); the per-row SSE goes straight to
//                 global memory (fwd_rows_kernel's bits), latents to LDS
//   dense       : the residuals of columns < D, stored from the lanes (16-byte
//                 stores when D % 4 == 0, else the rows are only element-aligned)
//   select      : key = fp32(df * df), NaN ranked as +inf, columns >= D as -1;
//                 K rounds in registers: every lane finds its best (key, d) by
//                 unrolled compares (ascending d, strict >: the lowest d of
//                 equal keys), two cross-lane exchanges combine the row's four
//                 lanes under (key descending, d ascending), and the lane that
//                 owns the winner retires it (key -2) and writes idx / resid
//                 slot k of its row; slots past min(K, D) hold -1 / 0
//   latent terms: lanes 0..15, one row each: (double)t1 * (double)t1 with t0 /
//                 t1 as in cen_score_kernel and score_block
//
// LDS: score_rows_kernel's without its SSE and alarm words (76.5 KB), so two
// workgroups share a CU's 160 KB.
#include "fedmx_forward_common.h"
#include "fedmx_score_common.h"

namespace fedmx {

struct ExplainDesc {
  const float* params;     // [P_PAD] padded parameter vector
  const void* raw;         // which == null: [nrows, d_in] raw rows of this block; else the whole raw array
  const double* sc_a;      // [d_in] standard: mean_   minmax: scale_
  const double* sc_b;      // [d_in] standard: scale_  minmax: min_
  const double* z_mean;    // [latent] latent scaler (with latent_terms), else null
  const double* z_scale;   // [latent]
  const int32_t* which;    // [nrows] this block's row indices into raw, or null
  int32_t* idx;            // [nrows, top_k] feature indices, worst first; -1 past min(top_k, d_in)
  float* resid;            // [nrows, top_k] their residuals y - x; 0 past min(top_k, d_in)
  float* sse;              // [nrows]
  float* resid_full;       // [nrows, d_in] every residual, or null
  double* latent_terms;    // [nrows, latent] squared scaled latents (CEN), or null
  int32_t nrows;
  int32_t d_in;
  int32_t hidden;
  int32_t latent;
  int32_t flags;           // SCORE_RAW_F64 | SCORE_MINMAX
  int32_t top_k;           // 1..EXPLAIN_MAX_K
};
static_assert(sizeof(ExplainDesc) == 120, "ExplainDesc layout is shared with Python");

constexpr int EXPLAIN_MAX_K = 16;

// fwd_rows_block's residual sink: the lane's 32 values, index 4u + r.
//
// Only the values of columns < d_in mean anything, and everything below masks
// by `dc < D`.  The forward forms df against its x registers *after* it put
// its layer-1 bias inputs into them: column DP - 1 = 127 in identity order
// (x[7][3] of lane group 3) and columns 116 / 120 / 124 in compact order
// (x[7][0] of lane groups 1..3, fedmx_forward_common.h fwd_xcol), so the
// "residuals" there are not y - x.  Those columns are never features:
// ModelDims caps d_in at DP - 1 (the bias column) and the compact order is
// taken only for d_in <= 115 (fwd_compact_ok).  A change of the padded layout
// or of the compact order's bound must keep every reused column >= d_in; the
// kernel writes nothing for a descriptor whose d_in reaches one
// (EXPLAIN_FIRST_REUSED_*), and ops/_hip.explain_desc raises for it.
constexpr int EXPLAIN_FIRST_REUSED_COMPACT = 116;   // min(fwd_xcol's swapped columns >= 115)
constexpr int EXPLAIN_FIRST_REUSED_IDENTITY = DP - 1;
struct ExplainSink {
  float* df;
  __device__ __forceinline__ void operator()(int u, int r, float v) const { df[4 * u + r] = v; }
};

template <bool CP, bool F64, bool MINMAX>
__device__ __forceinline__ void explain_block(const ExplainDesc& d, const float* sW1, const float* sW2,
                                              const float* sW3, const float* sW4, float* tile, float* s_lat,
                                              const double* s_zmean, const double* s_zscale) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c = lane & 15;   // the lane's row of the tile
  const int g = lane >> 4;   // its lane group: columns 16u + 4g + r
  const int D = d.d_in;
  const int K = d.top_k;
  const int kreal = min(K, D);
  const bool want_terms = d.latent_terms != nullptr;
  // scaler constants of this lane's two columns (x 1 / + 0 past D: never used)
  const int c0 = lane, c1 = lane + 64;
  const double a0 = c0 < D ? d.sc_a[c0] : 0.0, b0 = c0 < D ? d.sc_b[c0] : 1.0;
  const double a1 = c1 < D ? d.sc_a[c1] : 0.0, b1 = c1 < D ? d.sc_b[c1] : 1.0;
  const int ntiles = (d.nrows + SCORE_TILE - 1) / SCORE_TILE;
  for (int t = wave; t < ntiles; t += SCORE_WAVES) {
    const int r0 = t * SCORE_TILE;
    const int rows = min(SCORE_TILE, d.nrows - r0);
    const bool valid = c < rows;
    // ---- standardise: all of the tile's loads first, then the arithmetic
    double v0[SCORE_TILE], v1[SCORE_TILE];
#pragma unroll
    for (int r = 0; r < SCORE_TILE; ++r) {
      const int rb = r0 + (r < rows ? r : 0);
      const size_t base = (d.which != nullptr ? (size_t)d.which[rb] : (size_t)rb) * (size_t)D;
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
    // ---- forward: this wave alone, its one tile; the residuals stay in registers
    float df[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) df[q] = 0.0f;
    FwdDesc f;
    f.params = d.params;
    f.x = tile;
    f.sse = nullptr;
    f.lat = want_terms ? s_lat : nullptr;
    f.nrows = rows;
    f.lat_stride = ZP;
    f.d_in = D;
    f.latent = d.latent;
    f.hidden = d.hidden;
    fwd_rows_block<CP, false>(f, sW1, sW2, sW3, sW4, 0, 1, d.sse + r0, ExplainSink{df});
    const size_t row = (size_t)(r0 + c);
    // ---- dense residuals
    if (d.resid_full != nullptr && valid) {
      float* o = d.resid_full + row * (size_t)D;
      if ((D & 3) == 0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int dc = 16 * u + 4 * g;
          if (dc < D)
            *reinterpret_cast<f32x4*>(o + dc) = f32x4{df[4 * u], df[4 * u + 1], df[4 * u + 2], df[4 * u + 3]};
        }
      } else {
#pragma unroll
        for (int q = 0; q < 32; ++q) {
          const int dc = 16 * (q >> 2) + 4 * g + (q & 3);
          if (dc < D) o[dc] = df[q];
        }
      }
    }
    // ---- ranking keys
    float key[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) {
      const int dc = 16 * (q >> 2) + 4 * g + (q & 3);
      const float e = df[q] * df[q];
      key[q] = dc < D ? (e != e ? INFINITY : e) : -1.0f;
    }
    // ---- top K: one round per slot
    for (int k = 0; k < K; ++k) {
      if (k >= kreal) {   // (wave-uniform) fewer features than slots
        if (g == 0 && valid) {
          d.idx[row * (size_t)K + k] = -1;
          d.resid[row * (size_t)K + k] = 0.0f;
        }
        continue;
      }
      float best = key[0];
      int bq = 0;
#pragma unroll
      for (int q = 1; q < 32; ++q) {
        const bool gt = key[q] > best;
        best = gt ? key[q] : best;
        bq = gt ? q : bq;
      }
      const int bd = 16 * (bq >> 2) + 4 * g + (bq & 3);
      float wk = best;
      int wd = bd;
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const float ok = __shfl_xor(wk, off, 64);
        const int od = __shfl_xor(wd, off, 64);
        const bool take = ok > wk || (ok == wk && od < wd);
        wk = take ? ok : wk;
        wd = take ? od : wd;
      }
      const bool owner = wd == bd;   // (a column belongs to one lane of the row)
      float rv = 0.0f;
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const bool hit = owner && q == bq;
        rv = hit ? df[q] : rv;
        key[q] = hit ? -2.0f : key[q];
      }
      if (owner && valid) {
        d.idx[row * (size_t)K + k] = wd;
        d.resid[row * (size_t)K + k] = rv;
      }
    }
    // ---- CEN: the squared scaled latents
    if (want_terms) {
      wave_sync();
      if (lane < rows) {
        for (int j = 0; j < d.latent; ++j) {
          const float t0 = (float)((double)s_lat[lane * ZP + j] - s_zmean[j]);
          const float t1 = (float)((double)t0 / s_zscale[j]);
          const double v = (double)t1;
          d.latent_terms[(size_t)(r0 + lane) * (size_t)d.latent + j] = v * v;
        }
      }
    }
    wave_sync();   // the next tile's writes come after these reads
  }
}

template <bool CP>
__device__ __forceinline__ void explain_dispatch(const ExplainDesc& d, const float* sW1, const float* sW2,
                                                 const float* sW3, const float* sW4, float* tile, float* s_lat,
                                                 const double* s_zmean, const double* s_zscale) {
  const bool f64 = d.flags & SCORE_RAW_F64, mm = d.flags & SCORE_MINMAX;
  if (f64 && !mm) explain_block<CP, true, false>(d, sW1, sW2, sW3, sW4, tile, s_lat, s_zmean, s_zscale);
  else if (f64) explain_block<CP, true, true>(d, sW1, sW2, sW3, sW4, tile, s_lat, s_zmean, s_zscale);
  else if (!mm) explain_block<CP, false, false>(d, sW1, sW2, sW3, sW4, tile, s_lat, s_zmean, s_zscale);
  else explain_block<CP, false, true>(d, sW1, sW2, sW3, sW4, tile, s_lat, s_zmean, s_zscale);
}

__global__ __launch_bounds__(SCORE_THREADS, 2) void explain_rows_kernel(const ExplainDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) float sW1[HP * S_W1];
  __shared__ __attribute__((aligned(16))) float sW2[ZP * S_W2];
  __shared__ __attribute__((aligned(16))) float sW3[HP * S_W3];
  __shared__ __attribute__((aligned(16))) float sW4[DP * S_W4];
  __shared__ __attribute__((aligned(16))) float s_tile[SCORE_WAVES][SCORE_TILE * DP];
  __shared__ float s_lat[SCORE_WAVES][SCORE_TILE * ZP];
  __shared__ double s_zmean[ZP];
  __shared__ double s_zscale[ZP];

  const ExplainDesc d = descs[blockIdx.x];
  if (d.nrows <= 0) return;   // (whole workgroup)
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  FwdDesc shape;
  shape.d_in = d.d_in;
  shape.hidden = d.hidden;
  shape.latent = d.latent;
  const bool compact = fwd_compact_ok(shape);
  if (d.d_in > (compact ? EXPLAIN_FIRST_REUSED_COMPACT : EXPLAIN_FIRST_REUSED_IDENTITY)) return;   // (see ExplainSink)
  if (compact) stage_params<true>(d.params, sW1, sW2, sW3, sW4);
  else stage_params<false>(d.params, sW1, sW2, sW3, sW4);
  if (tid < ZP) {
    const bool cen = d.latent_terms != nullptr && tid < d.latent;
    s_zmean[tid] = cen ? d.z_mean[tid] : 0.0;
    s_zscale[tid] = cen ? d.z_scale[tid] : 1.0;
  }
  __syncthreads();
  if (compact) explain_dispatch<true>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_lat[wave], s_zmean, s_zscale);
  else explain_dispatch<false>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_lat[wave], s_zmean, s_zscale);
}

}  // namespace fedmx

extern "C" {

int fedmx_explain_rows(const void* descs, int nblocks, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  hipLaunchKernelGGL(fedmx::explain_rows_kernel, dim3(nblocks), dim3(fedmx::SCORE_THREADS), 0, stream,
                     reinterpret_cast<const fedmx::ExplainDesc*>(descs));
  return (int)hipGetLastError();
}

int fedmx_explain_desc_size() { return (int)sizeof(fedmx::ExplainDesc); }
int fedmx_explain_max_k() { return fedmx::EXPLAIN_MAX_K; }

}  // extern "C"
