// Monitoring a deployed detector on gfx950 (README "Monitoring a deployed
// detector"; not in the reference): raw feature rows in, per-feature statistics
// of the standardised values and a histogram of the scores out.  Two launches
// on one stream:
//
// monitor_rows_kernel, beside score_rows_kernel and with its structure.  One
// descriptor per (detector, block of raw rows).  A 256-thread workgroup stages
// its detector's weights in LDS (stage_params) and then its four waves work
// independently, each on 16-row tiles of the block (wave w takes tiles w,
// w + 4, ...: stream (block, w)), with no workgroup barrier in the loop:
//   standardise : as score_rows_kernel (score_standardise: same bits).  Lane l
//                 owns columns l and l + 64; it folds the fp32 value t of every
//                 real row, in row order, into that column's accumulators,
//                 which stay in registers for the whole block:
//                   t NaN or +-inf : bad += 1
//                   otherwise      : cnt += 1; sum += (double)t;
//                                    sq += (double)t * (double)t  (exact product)
//                                    mn = t < mn ? t : mn; mx = t > mx ? t : mx
//                                    out += t < lo || t > hi
//   forward     : fwd_rows_block on that tile (same bits as fwd_rows_kernel)
//   score       : lanes 0..15, one row each, score_rows_kernel's rule; the
//                 cleaned score s is compared with the threshold and binned,
//                 bin = #{i : edge_i < s}, into the workgroup's LDS histogram
//                 (integer atomics); nothing per row is written
//   latents     : written for a latents-only descriptor (kNN: scored after)
// After the loop each wave parks its partials in its own, now free, LDS tile;
// threads 0..127 fold the four waves' in wave order, ((p0 + p1) + p2) + p3,
// and write the block's partial, one per column.  The workgroup adds its
// alarm count and each non-empty bin to the detector's counters with one
// integer atomic each.  No float goes through an atomic.
//
// monitor_fold_kernel: 16 workgroups per detector, eight columns each, walk
// that detector's block partials in block order, T = (+0.0 + S_0) + S_1 + ...,
// one thread per column, and write the totals.  Each workgroup's 1,024 threads
// first bring 128 blocks' partials of its columns into LDS: a walk of one
// block per memory latency takes about 0.7 us per block, and one workgroup
// alone pulls every partial (4.6 KB per block) through a single CU.
//
// Measurement builds (never the library's): -DFEDMX_MONITOR_VARIANT=1 drops the
// per-value statistics from monitor_rows_kernel, =2 only their two float64
// chains (profiles/monitor_rows_kernel.md).
//
// LDS: score_rows_kernel's + 128 B of edges + 64 B of histogram = 77.0 KB, so
// two workgroups share a CU's 160 KB.
#include "fedmx_forward_common.h"
#include "fedmx_score_common.h"

#ifndef FEDMX_MONITOR_VARIANT
#define FEDMX_MONITOR_VARIANT 0
#endif

namespace fedmx {

constexpr int MONITOR_MAX_EDGES = 15;
constexpr int MONITOR_COLS = DP;   // one partial per padded column
constexpr int MONITOR_FOLD_COLS = 8;      // columns one monitor_fold_kernel workgroup folds
constexpr int MONITOR_FOLD_SLOTS = 128;   // block partials it loads before it folds them
constexpr int MONITOR_FOLD_THREADS = MONITOR_FOLD_COLS * MONITOR_FOLD_SLOTS;
constexpr int MONITOR_FOLD_GROUPS = MONITOR_COLS / MONITOR_FOLD_COLS;
static_assert(MONITOR_FOLD_THREADS <= 1024 && MONITOR_COLS % MONITOR_FOLD_COLS == 0, "fold geometry");

// One block's (or, in sum / sq / mn / mx, one detector's) statistics, column-wise.
struct MonitorPartial {
  double sum[MONITOR_COLS];
  double sq[MONITOR_COLS];
  float mn[MONITOR_COLS];
  float mx[MONITOR_COLS];
  uint32_t cnt[MONITOR_COLS];
  uint32_t bad[MONITOR_COLS];
  uint32_t out[MONITOR_COLS];
  uint32_t pad[MONITOR_COLS];
};
static_assert(sizeof(MonitorPartial) == 5120, "MonitorPartial layout is shared with Python");

struct MonitorTotal {
  double sum[MONITOR_COLS];
  double sq[MONITOR_COLS];
  int64_t cnt[MONITOR_COLS];
  int64_t bad[MONITOR_COLS];
  int64_t out[MONITOR_COLS];
  float mn[MONITOR_COLS];
  float mx[MONITOR_COLS];
};
static_assert(sizeof(MonitorTotal) == 6144, "MonitorTotal layout is shared with Python");

struct MonitorDesc {
  const float* params;     // [P_PAD] padded parameter vector
  const void* raw;         // [nrows, d_in] raw rows of this block (float64 or float32)
  const double* sc_a;      // [d_in] standard: mean_   minmax: scale_
  const double* sc_b;      // [d_in] standard: scale_  minmax: min_
  const double* z_mean;    // [latent] latent scaler (CEN), else null
  const double* z_scale;   // [latent]
  const float* lo;         // [d_in] the baseline's band, or null (nothing is out)
  const float* hi;         // [d_in]
  const double* edges;     // [nedges] score edges, non-decreasing
  unsigned long long* hist;  // [nedges + 1] the detector's bin counters, or null (no baseline)
  float* lat;              // [nrows, latent] latents out, or null
  uint32_t* alarms;        // the detector's alarm counter
  MonitorPartial* part;    // this block's partial
  double threshold;
  int32_t nrows;
  int32_t d_in;
  int32_t hidden;
  int32_t latent;
  int32_t flags;           // SCORE_* bits
  float score_scale;       // AE: fp32(1 / d_in)
  int32_t nedges;          // 0..MONITOR_MAX_EDGES
  int32_t pad;
};
static_assert(sizeof(MonitorDesc) == 144, "MonitorDesc layout is shared with Python");

struct MonitorFoldDesc {
  const MonitorPartial* part;   // [nblocks] this detector's block partials, in block order
  MonitorTotal* total;
  int32_t nblocks;
  int32_t pad;
};
static_assert(sizeof(MonitorFoldDesc) == 24, "MonitorFoldDesc layout is shared with Python");

// One column's accumulators (registers).
struct MonitorAcc {
  double sum, sq;
  float mn, mx;
  unsigned int cnt, bad, out;
  __device__ __forceinline__ void init() {
    sum = 0.0;
    sq = 0.0;
    mn = INFINITY;
    mx = -INFINITY;
    cnt = bad = out = 0u;
  }
  __device__ __forceinline__ void add(float t, float lo, float hi) {
#if FEDMX_MONITOR_VARIANT == 1
    return;
#endif
    if (!(fabsf(t) < INFINITY)) {   // NaN, +-inf
      bad += 1u;
      return;
    }
    cnt += 1u;
#if FEDMX_MONITOR_VARIANT != 2
    const double v = (double)t;
    sum = sum + v;
    sq = sq + v * v;
#endif
    mn = t < mn ? t : mn;
    mx = t > mx ? t : mx;
    out += (t < lo || t > hi) ? 1u : 0u;
  }
};

// The parked partials of one wave, laid over its 8 KB tile (4,608 B used).
struct MonitorPark {
  double sum[MONITOR_COLS];
  double sq[MONITOR_COLS];
  float mn[MONITOR_COLS];
  float mx[MONITOR_COLS];
  unsigned int cnt[MONITOR_COLS];
  unsigned int bad[MONITOR_COLS];
  unsigned int out[MONITOR_COLS];
};
static_assert(sizeof(MonitorPark) <= SCORE_TILE * DP * sizeof(float), "a wave's partials fit its tile");

template <bool CP, bool F64, bool MINMAX>
__device__ __forceinline__ void monitor_block(const MonitorDesc& d, const float* sW1, const float* sW2,
                                              const float* sW3, const float* sW4, float* tile, float* s_sse,
                                              float* s_lat, const double* s_zmean, const double* s_zscale,
                                              const double* s_edges, unsigned int* s_hist, unsigned int& alarms) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int D = d.d_in;
  const bool scoring = (d.flags & (SCORE_KIND_AE | SCORE_KIND_CEN)) != 0;
  const bool want_lat = d.lat != nullptr || (d.flags & SCORE_KIND_CEN);
  const bool want_sse = (d.flags & SCORE_KIND_AE) != 0;
  // scaler constants and band of this lane's two columns (past D: never used)
  const int c0 = lane, c1 = lane + 64;
  const double a0 = c0 < D ? d.sc_a[c0] : 0.0, b0 = c0 < D ? d.sc_b[c0] : 1.0;
  const double a1 = c1 < D ? d.sc_a[c1] : 0.0, b1 = c1 < D ? d.sc_b[c1] : 1.0;
  const bool band = d.lo != nullptr;
  const float lo0 = band && c0 < D ? d.lo[c0] : -INFINITY, hi0 = band && c0 < D ? d.hi[c0] : INFINITY;
  const float lo1 = band && c1 < D ? d.lo[c1] : -INFINITY, hi1 = band && c1 < D ? d.hi[c1] : INFINITY;
  MonitorAcc acc0, acc1;
  acc0.init();
  acc1.init();
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
      const float t0 = c0 < D ? score_standardise<MINMAX>(v0[r], a0, b0) : 0.0f;
      const float t1 = c1 < D ? score_standardise<MINMAX>(v1[r], a1, b1) : 0.0f;
      tile[r * DP + c0] = t0;
      tile[r * DP + c1] = t1;
      if (r < rows) {   // (wave-uniform) rows past the block's end repeat row r0: not counted
        if (c0 < D) acc0.add(t0, lo0, hi0);
        if (c1 < D) acc1.add(t1, lo1, hi1);
      }
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
    // ---- score, clean, compare, bin
    if (scoring) {
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
        if (d.hist != nullptr) {
          int bin = 0;
          for (int i = 0; i < d.nedges; ++i) bin += s_edges[i] < s ? 1 : 0;   // a tie: the lower bin
          atomicAdd(&s_hist[bin], 1u);
        }
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
  // ---- park this wave's partials in its own tile (no tile of it is in use any more)
  MonitorPark* park = reinterpret_cast<MonitorPark*>(tile);
  park->sum[c0] = acc0.sum;
  park->sq[c0] = acc0.sq;
  park->mn[c0] = acc0.mn;
  park->mx[c0] = acc0.mx;
  park->cnt[c0] = acc0.cnt;
  park->bad[c0] = acc0.bad;
  park->out[c0] = acc0.out;
  park->sum[c1] = acc1.sum;
  park->sq[c1] = acc1.sq;
  park->mn[c1] = acc1.mn;
  park->mx[c1] = acc1.mx;
  park->cnt[c1] = acc1.cnt;
  park->bad[c1] = acc1.bad;
  park->out[c1] = acc1.out;
}

template <bool CP>
__device__ __forceinline__ void monitor_dispatch(const MonitorDesc& d, const float* sW1, const float* sW2,
                                                 const float* sW3, const float* sW4, float* tile, float* s_sse,
                                                 float* s_lat, const double* s_zmean, const double* s_zscale,
                                                 const double* s_edges, unsigned int* s_hist, unsigned int& alarms) {
  const bool f64 = d.flags & SCORE_RAW_F64, mm = d.flags & SCORE_MINMAX;
  if (f64 && !mm)
    monitor_block<CP, true, false>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, s_edges, s_hist, alarms);
  else if (f64)
    monitor_block<CP, true, true>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, s_edges, s_hist, alarms);
  else if (!mm)
    monitor_block<CP, false, false>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, s_edges, s_hist, alarms);
  else
    monitor_block<CP, false, true>(d, sW1, sW2, sW3, sW4, tile, s_sse, s_lat, s_zmean, s_zscale, s_edges, s_hist, alarms);
}

__global__ __launch_bounds__(SCORE_THREADS, 2) void monitor_rows_kernel(const MonitorDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) float sW1[HP * S_W1];
  __shared__ __attribute__((aligned(16))) float sW2[ZP * S_W2];
  __shared__ __attribute__((aligned(16))) float sW3[HP * S_W3];
  __shared__ __attribute__((aligned(16))) float sW4[DP * S_W4];
  __shared__ __attribute__((aligned(16))) float s_tile[SCORE_WAVES][SCORE_TILE * DP];
  __shared__ float s_sse[SCORE_WAVES][SCORE_TILE];
  __shared__ float s_lat[SCORE_WAVES][SCORE_TILE * ZP];
  __shared__ double s_zmean[ZP];
  __shared__ double s_zscale[ZP];
  __shared__ double s_edges[MONITOR_MAX_EDGES + 1];
  __shared__ unsigned int s_hist[MONITOR_MAX_EDGES + 1];
  __shared__ unsigned int s_alarms;

  const MonitorDesc d = descs[blockIdx.x];
  if (d.nrows <= 0 || d.nedges < 0 || d.nedges > MONITOR_MAX_EDGES) return;   // (whole workgroup)
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
  if (tid >= 64 && tid < 64 + MONITOR_MAX_EDGES + 1) {
    const int i = tid - 64;
    s_edges[i] = (d.hist != nullptr && i < d.nedges) ? d.edges[i] : 0.0;
    s_hist[i] = 0u;
  }
  if (tid == 0) s_alarms = 0u;
  __syncthreads();
  unsigned int alarms = 0u;   // wave-uniform
  if (compact)
    monitor_dispatch<true>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_sse[wave], s_lat[wave], s_zmean, s_zscale, s_edges,
                           s_hist, alarms);
  else
    monitor_dispatch<false>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_sse[wave], s_lat[wave], s_zmean, s_zscale, s_edges,
                            s_hist, alarms);
  if ((tid & 63) == 0 && alarms) atomicAdd(&s_alarms, alarms);
  __syncthreads();
  // ---- the four waves' partials, in wave order; one column per thread
  if (tid < MONITOR_COLS) {
    const MonitorPark* p0 = reinterpret_cast<const MonitorPark*>(s_tile[0]);
    double sum = p0->sum[tid], sq = p0->sq[tid];
    float mn = p0->mn[tid], mx = p0->mx[tid];
    unsigned int cnt = p0->cnt[tid], bad = p0->bad[tid], out = p0->out[tid];
#pragma unroll
    for (int w = 1; w < SCORE_WAVES; ++w) {
      const MonitorPark* p = reinterpret_cast<const MonitorPark*>(s_tile[w]);
      sum = sum + p->sum[tid];
      sq = sq + p->sq[tid];
      mn = p->mn[tid] < mn ? p->mn[tid] : mn;
      mx = p->mx[tid] > mx ? p->mx[tid] : mx;
      cnt += p->cnt[tid];
      bad += p->bad[tid];
      out += p->out[tid];
    }
    MonitorPartial* o = d.part;
    o->sum[tid] = sum;
    o->sq[tid] = sq;
    o->mn[tid] = mn;
    o->mx[tid] = mx;
    o->cnt[tid] = cnt;
    o->bad[tid] = bad;
    o->out[tid] = out;
    o->pad[tid] = 0u;
  }
  if (tid == 128 && s_alarms) atomicAdd(d.alarms, s_alarms);
  if (tid >= 192 && tid <= 192 + d.nedges && d.hist != nullptr) {
    const unsigned int h = s_hist[tid - 192];
    if (h) atomicAdd(d.hist + (tid - 192), (unsigned long long)h);
  }
}

// One workgroup per (detector, group of MONITOR_FOLD_COLS columns).  Thread
// (slot = tid / MONITOR_FOLD_COLS, column = tid % MONITOR_FOLD_COLS) loads block
// b0 + slot's partial of its column into LDS, so MONITOR_FOLD_SLOTS blocks are in
// flight at once and the groups' workgroups pull the partials through 16 CUs;
// then the group's first MONITOR_FOLD_COLS threads fold that batch in block
// order, each its own column: the order of the rule, whatever the batch size.
__global__ __launch_bounds__(MONITOR_FOLD_THREADS) void monitor_fold_kernel(const MonitorFoldDesc* __restrict__ descs) {
  __shared__ double s_sum[MONITOR_FOLD_SLOTS][MONITOR_FOLD_COLS];
  __shared__ double s_sq[MONITOR_FOLD_SLOTS][MONITOR_FOLD_COLS];
  __shared__ float s_mn[MONITOR_FOLD_SLOTS][MONITOR_FOLD_COLS];
  __shared__ float s_mx[MONITOR_FOLD_SLOTS][MONITOR_FOLD_COLS];
  __shared__ uint32_t s_cnt[MONITOR_FOLD_SLOTS][MONITOR_FOLD_COLS];
  __shared__ uint32_t s_bad[MONITOR_FOLD_SLOTS][MONITOR_FOLD_COLS];
  __shared__ uint32_t s_out[MONITOR_FOLD_SLOTS][MONITOR_FOLD_COLS];

  const MonitorFoldDesc d = descs[blockIdx.x];
  const int tid = threadIdx.x;
  const int lc = tid % MONITOR_FOLD_COLS;
  const int slot = tid / MONITOR_FOLD_COLS;
  const int c = (int)blockIdx.y * MONITOR_FOLD_COLS + lc;   // < MONITOR_COLS: the grid's y is MONITOR_FOLD_GROUPS
  double sum = 0.0, sq = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  long long cnt = 0, bad = 0, out = 0;
  for (int b0 = 0; b0 < d.nblocks; b0 += MONITOR_FOLD_SLOTS) {
    const int b = b0 + slot;
    if (b < d.nblocks) {
      const MonitorPartial* p = d.part + b;
      s_sum[slot][lc] = p->sum[c];
      s_sq[slot][lc] = p->sq[c];
      s_mn[slot][lc] = p->mn[c];
      s_mx[slot][lc] = p->mx[c];
      s_cnt[slot][lc] = p->cnt[c];
      s_bad[slot][lc] = p->bad[c];
      s_out[slot][lc] = p->out[c];
    }
    __syncthreads();
    if (tid < MONITOR_FOLD_COLS) {
      const int m = min(MONITOR_FOLD_SLOTS, d.nblocks - b0);
#pragma unroll 8
      for (int k = 0; k < m; ++k) {
        sum = sum + s_sum[k][lc];
        sq = sq + s_sq[k][lc];
        const float pmn = s_mn[k][lc], pmx = s_mx[k][lc];
        mn = pmn < mn ? pmn : mn;
        mx = pmx > mx ? pmx : mx;
        cnt += (long long)s_cnt[k][lc];
        bad += (long long)s_bad[k][lc];
        out += (long long)s_out[k][lc];
      }
    }
    __syncthreads();   // the next batch's writes come after these reads
  }
  if (tid < MONITOR_FOLD_COLS) {
    MonitorTotal* o = d.total;
    o->sum[c] = sum;
    o->sq[c] = sq;
    o->cnt[c] = cnt;
    o->bad[c] = bad;
    o->out[c] = out;
    o->mn[c] = mn;
    o->mx[c] = mx;
  }
}

}  // namespace fedmx

extern "C" {

// monitor_fold_kernel alone over `nfold` descriptors (one per detector with rows).
int fedmx_monitor_fold(const void* fold_descs, int nfold, hipStream_t stream) {
  if (nfold <= 0) return 0;
  hipLaunchKernelGGL(fedmx::monitor_fold_kernel, dim3(nfold, fedmx::MONITOR_FOLD_GROUPS),
                     dim3(fedmx::MONITOR_FOLD_THREADS), 0, stream,
                     reinterpret_cast<const fedmx::MonitorFoldDesc*>(fold_descs));
  return (int)hipGetLastError();
}

// monitor_rows_kernel over `nblocks` descriptors, then monitor_fold_kernel over
// `nfold` (none: the first kernel alone), both on `stream`.
int fedmx_monitor_rows(const void* descs, int nblocks, const void* fold_descs, int nfold, hipStream_t stream) {
  if (nblocks <= 0) return 0;
  hipLaunchKernelGGL(fedmx::monitor_rows_kernel, dim3(nblocks), dim3(fedmx::SCORE_THREADS), 0, stream,
                     reinterpret_cast<const fedmx::MonitorDesc*>(descs));
  const int err = (int)hipGetLastError();
  if (err != 0) return err;
  return fedmx_monitor_fold(fold_descs, nfold, stream);
}

int fedmx_monitor_desc_size() { return (int)sizeof(fedmx::MonitorDesc); }
int fedmx_monitor_fold_desc_size() { return (int)sizeof(fedmx::MonitorFoldDesc); }
int fedmx_monitor_partial_size() { return (int)sizeof(fedmx::MonitorPartial); }
int fedmx_monitor_total_size() { return (int)sizeof(fedmx::MonitorTotal); }
int fedmx_monitor_max_edges() { return fedmx::MONITOR_MAX_EDGES; }

}  // extern "C"
