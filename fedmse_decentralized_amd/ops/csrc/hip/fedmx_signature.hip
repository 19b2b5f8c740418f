// Incident signatures of a deployed detector on gfx950 (README "Incident
// signatures"; not in the reference): raw feature rows, the list of flagged
// rows inside the chosen incidents and each list position's incident in; per
// incident and feature the float64 sums of the squared and of the signed
// residuals over the incident's flagged rows out, in a fixed order.  Two
// launches on one stream:
//
// incident_sig_kernel, beside explain_rows_kernel and with its structure.  One
// descriptor per (item, block of R list positions).  A 256-thread workgroup
// stages its detector's weights in LDS (stage_params) and then its four waves
// work independently, each on 16-position tiles of the block (wave w takes
// tiles w, w + 4, ...: stream (block, w)), with no workgroup barrier in the
// loop:
//   standardise : as explain_rows_kernel with `which` (score_standardise: same
//                 bits): position p of the block is raw row which[p]
//   forward     : fwd_rows_block on that tile with explain_rows_kernel's sink:
//                 the lane keeps its 32 residuals df = y - x (columns 16u + 4g
//                 + r of row c; lane = 16g + c); the per-row SSE lands in a
//                 16-word LDS scratch nobody reads (the forward stops after
//                 layer 2 without a destination)
//   transpose   : the tile is free now; the lanes store their residuals into
//                 it, row c, column 16u + 4g + r
//   reduce      : lane l owns columns l and l + 64 and walks them down the
//                 tile's real rows in order.  Each row's incident seg[p] is
//                 wave-uniform.  Per column the accumulators se, sr (float64)
//                 and bad stay in registers across the stream's tiles:
//                   e = fp32(r * r) NaN or +-inf : bad += 1
//                   otherwise : se = se + (double)e; sr = sr + (double)r
//                 A stream meets its incidents in rising order; when seg
//                 changes, and at the stream's end, the lane stores the
//                 accumulators to the partial slot of (block, incident, wave)
//                 and resets them.
// The pairs (block b, incident j) that hold a position form a staircase (both
// rise along the list), so slot b + j belongs to one pair; the host zeroes the
// nb + s slots, and a stream without a position of j leaves its part of the
// slot at the rule's initial values.  Plain vector stores; no float goes
// through an atomic.
//
// incident_sig_fold_kernel: one workgroup per (item, incident), one thread per
// column: walks the incident's blocks first .. last in order, forms the block
// partial ((p0 + p1) + p2) + p3 over the four streams, adds it to the total
// (from +0.0) and writes err_sum, resid_sum and bad.
//
// The reused bias columns of the forward's x registers (fedmx_explain.hip,
// ExplainSink) hold no residual; as there, they are never features, and the
// kernel writes nothing for a descriptor whose d_in reaches one.
//
// LDS: explain_rows_kernel's without its latents and latent scaler, plus 256 B
// of SSE scratch (71.5 KB), so two workgroups share a CU's 160 KB.
#include "fedmx_forward_common.h"
#include "fedmx_score_common.h"

namespace fedmx {

constexpr int SIG_COLS = DP;   // one accumulator per padded column
constexpr int SIG_FIRST_REUSED_COMPACT = 116;   // fedmx_explain.hip EXPLAIN_FIRST_REUSED_*
constexpr int SIG_FIRST_REUSED_IDENTITY = DP - 1;

// The four streams' sums of one (block, incident) pair, column-wise.
struct SigPartial {
  double se[SCORE_WAVES][SIG_COLS];
  double sr[SCORE_WAVES][SIG_COLS];
  uint32_t bad[SCORE_WAVES][SIG_COLS];
};
static_assert(sizeof(SigPartial) == 10240, "SigPartial layout is shared with Python");

struct SigDesc {
  const float* params;     // [P_PAD] padded parameter vector
  const void* raw;         // the item's whole raw array [n, d_in] (float64 or float32)
  const double* sc_a;      // [d_in] standard: mean_   minmax: scale_
  const double* sc_b;      // [d_in] standard: scale_  minmax: min_
  const int32_t* which;    // [nrows] this block's list entries: row indices into raw
  const int32_t* seg;      // [nrows] their incidents' positions, non-decreasing along the list
  SigPartial* part;        // the item's slot 0; this block writes slots block + seg
  int32_t nrows;
  int32_t d_in;
  int32_t hidden;
  int32_t latent;
  int32_t flags;           // SCORE_RAW_F64 | SCORE_MINMAX
  int32_t block;           // this block's index within the item
  int32_t nslots;          // slots the item owns (blocks + incidents)
  int32_t pad;
};
static_assert(sizeof(SigDesc) == 88, "SigDesc layout is shared with Python");

struct SigFoldDesc {
  const SigPartial* part;  // the item's slot 0
  double* err_sum;         // [d_in] this incident's row of the results
  double* resid_sum;       // [d_in]
  long long* bad;          // [d_in]
  int32_t seg;             // the incident's position j
  int32_t first;           // first block holding one of its list positions
  int32_t last;            // last such block (< first: none; the initial values are the answer)
  int32_t d_in;
};
static_assert(sizeof(SigFoldDesc) == 48, "SigFoldDesc layout is shared with Python");

// fwd_rows_block's residual sink, as explain_rows_kernel's: the lane's 32 values, index 4u + r.
struct SigSink {
  float* df;
  __device__ __forceinline__ void operator()(int u, int r, float v) const { df[4 * u + r] = v; }
};

// One column's accumulators (registers).
struct SigAcc {
  double se, sr;
  unsigned int bad;
  __device__ __forceinline__ void init() {
    se = 0.0;
    sr = 0.0;
    bad = 0u;
  }
  __device__ __forceinline__ void add(float r) {
#pragma clang fp contract(off)
    const float e = r * r;
    if (!(fabsf(e) < INFINITY)) {   // NaN, +-inf: neither sum takes the row
      bad += 1u;
      return;
    }
    se = se + (double)e;
    sr = sr + (double)r;
  }
};

template <bool CP, bool F64, bool MINMAX>
__device__ __forceinline__ void sig_block(const SigDesc& d, const float* sW1, const float* sW2, const float* sW3,
                                          const float* sW4, float* tile, float* s_sse) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c = lane & 15;   // the lane's row of the tile
  const int g = lane >> 4;   // its lane group: columns 16u + 4g + r
  const int D = d.d_in;
  // scaler constants of this lane's two columns (x 1 / + 0 past D: never used)
  const int c0 = lane, c1 = lane + 64;
  const double a0 = c0 < D ? d.sc_a[c0] : 0.0, b0 = c0 < D ? d.sc_b[c0] : 1.0;
  const double a1 = c1 < D ? d.sc_a[c1] : 0.0, b1 = c1 < D ? d.sc_b[c1] : 1.0;
  SigAcc acc0, acc1;
  acc0.init();
  acc1.init();
  int cur = -1;   // (wave-uniform) the incident the accumulators belong to; -1: none yet
  auto flush = [&]() {
    const int slot = d.block + cur;
    if (cur >= 0 && slot < d.nslots) {
      SigPartial* p = d.part + slot;
      p->se[wave][c0] = acc0.se;
      p->sr[wave][c0] = acc0.sr;
      p->bad[wave][c0] = acc0.bad;
      p->se[wave][c1] = acc1.se;
      p->sr[wave][c1] = acc1.sr;
      p->bad[wave][c1] = acc1.bad;
    }
  };
  const int ntiles = (d.nrows + SCORE_TILE - 1) / SCORE_TILE;
  for (int t = wave; t < ntiles; t += SCORE_WAVES) {
    const int r0 = t * SCORE_TILE;
    const int rows = min(SCORE_TILE, d.nrows - r0);
    // ---- standardise: all of the tile's loads first, then the arithmetic
    double v0[SCORE_TILE], v1[SCORE_TILE];
#pragma unroll
    for (int r = 0; r < SCORE_TILE; ++r) {
      const int rb = r0 + (r < rows ? r : 0);
      const size_t base = (size_t)d.which[rb] * (size_t)D;
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
    f.lat = nullptr;
    f.nrows = rows;
    f.lat_stride = ZP;
    f.d_in = D;
    f.latent = d.latent;
    f.hidden = d.hidden;
    fwd_rows_block<CP, false>(f, sW1, sW2, sW3, sW4, 0, 1, s_sse, SigSink{df});
    wave_sync();   // every lane has its x values: the tile is free
    // ---- transpose through the tile: row c, columns 16u + 4g .. + 3
#pragma unroll
    for (int u = 0; u < 8; ++u)
      lds_write4(&tile[c * DP + 16 * u + 4 * g], f32x4{df[4 * u], df[4 * u + 1], df[4 * u + 2], df[4 * u + 3]});
    wave_sync();
    // ---- reduce: this lane's two columns down the real rows, in order
#pragma unroll
    for (int r = 0; r < SCORE_TILE; ++r) {
      if (r < rows) {   // (wave-uniform)
        const int sg = d.seg[r0 + r];
        if (sg != cur) {   // (wave-uniform) the next incident
          flush();
          acc0.init();
          acc1.init();
          cur = sg;
        }
        if (c0 < D) acc0.add(tile[r * DP + c0]);
        if (c1 < D) acc1.add(tile[r * DP + c1]);
      }
    }
    wave_sync();   // the next tile's writes come after these reads
  }
  flush();
}

template <bool CP>
__device__ __forceinline__ void sig_dispatch(const SigDesc& d, const float* sW1, const float* sW2, const float* sW3,
                                             const float* sW4, float* tile, float* s_sse) {
  const bool f64 = d.flags & SCORE_RAW_F64, mm = d.flags & SCORE_MINMAX;
  if (f64 && !mm) sig_block<CP, true, false>(d, sW1, sW2, sW3, sW4, tile, s_sse);
  else if (f64) sig_block<CP, true, true>(d, sW1, sW2, sW3, sW4, tile, s_sse);
  else if (!mm) sig_block<CP, false, false>(d, sW1, sW2, sW3, sW4, tile, s_sse);
  else sig_block<CP, false, true>(d, sW1, sW2, sW3, sW4, tile, s_sse);
}

__global__ __launch_bounds__(SCORE_THREADS, 2) void incident_sig_kernel(const SigDesc* __restrict__ descs) {
  __shared__ __attribute__((aligned(16))) float sW1[HP * S_W1];
  __shared__ __attribute__((aligned(16))) float sW2[ZP * S_W2];
  __shared__ __attribute__((aligned(16))) float sW3[HP * S_W3];
  __shared__ __attribute__((aligned(16))) float sW4[DP * S_W4];
  __shared__ __attribute__((aligned(16))) float s_tile[SCORE_WAVES][SCORE_TILE * DP];
  __shared__ float s_sse[SCORE_WAVES][SCORE_TILE];

  const SigDesc d = descs[blockIdx.x];
  if (d.nrows <= 0 || d.block < 0) return;   // (whole workgroup)
  const int wave = threadIdx.x >> 6;
  FwdDesc shape;
  shape.d_in = d.d_in;
  shape.hidden = d.hidden;
  shape.latent = d.latent;
  const bool compact = fwd_compact_ok(shape);
  if (d.d_in > (compact ? SIG_FIRST_REUSED_COMPACT : SIG_FIRST_REUSED_IDENTITY)) return;   // (see above)
  if (compact) stage_params<true>(d.params, sW1, sW2, sW3, sW4);
  else stage_params<false>(d.params, sW1, sW2, sW3, sW4);
  __syncthreads();
  if (compact) sig_dispatch<true>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_sse[wave]);
  else sig_dispatch<false>(d, sW1, sW2, sW3, sW4, s_tile[wave], s_sse[wave]);
}

__global__ __launch_bounds__(SIG_COLS) void incident_sig_fold_kernel(const SigFoldDesc* __restrict__ descs) {
#pragma clang fp contract(off)
  const SigFoldDesc d = descs[blockIdx.x];
  const int c = threadIdx.x;
  if (c >= d.d_in || c >= SIG_COLS) return;
  double te = 0.0, tr = 0.0;
  long long tb = 0;
#pragma unroll 4
  for (int b = d.first; b <= d.last; ++b) {
    const SigPartial* p = d.part + (b + d.seg);
    double e = p->se[0][c], r = p->sr[0][c];
    long long n = (long long)p->bad[0][c];
#pragma unroll
    for (int w = 1; w < SCORE_WAVES; ++w) {
      e = e + p->se[w][c];
      r = r + p->sr[w][c];
      n += (long long)p->bad[w][c];
    }
    te = te + e;
    tr = tr + r;
    tb += n;
  }
  d.err_sum[c] = te;
  d.resid_sum[c] = tr;
  d.bad[c] = tb;
}

}  // namespace fedmx

extern "C" {

// incident_sig_kernel over `nblocks` descriptors, then incident_sig_fold_kernel
// over `nfold` (one per incident of an item with list positions), both on `stream`.
int fedmx_incident_signatures(const void* descs, int nblocks, const void* fold_descs, int nfold,
                              hipStream_t stream) {
  if (nblocks <= 0 || nfold <= 0) return 0;
  hipLaunchKernelGGL(fedmx::incident_sig_kernel, dim3(nblocks), dim3(fedmx::SCORE_THREADS), 0, stream,
                     reinterpret_cast<const fedmx::SigDesc*>(descs));
  const int err = (int)hipGetLastError();
  if (err != 0) return err;
  hipLaunchKernelGGL(fedmx::incident_sig_fold_kernel, dim3(nfold), dim3(fedmx::SIG_COLS), 0, stream,
                     reinterpret_cast<const fedmx::SigFoldDesc*>(fold_descs));
  return (int)hipGetLastError();
}

int fedmx_sig_desc_size() { return (int)sizeof(fedmx::SigDesc); }
int fedmx_sig_fold_desc_size() { return (int)sizeof(fedmx::SigFoldDesc); }
int fedmx_sig_partial_size() { return (int)sizeof(fedmx::SigPartial); }

}  // extern "C"
