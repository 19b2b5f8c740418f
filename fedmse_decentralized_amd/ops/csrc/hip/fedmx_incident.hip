// Grouping a deployed detector's alarms into incidents on gfx950 (README
// "Incidents"; not in the reference).  Per item: flags[0..n) (uint8, non-zero =
// flagged) and scores[0..n) (float64) in, the incidents of the rule
//   cnt[i] = #{j in [max(0, i-w+1), i] : flags[j] != 0},  hot[i] = cnt[i] >= m,
//   start  = hot and no hot row in [i-h-1, i-1],  end = hot and none in [i+1, i+h+1]
// out: start_k, end_k, alarms_k (flags in [max(0, start_k-w+1), end_k]), the
// peak (smallest row of [start_k, end_k] whose cleaned score none of the range
// exceeds, -0.0 equal to +0.0) and the totals.  Integers and one comparison;
// no float goes through an atomic.
//
// One descriptor per (item, span of INCIDENT_SPAN rows), one 1,024-thread
// workgroup each, and no workgroup waits for another: passes are ordered by
// launch order on one stream.  Every pass starts with the same analysis:
//   the workgroup reads its span's flags plus a halo of ceil64(h+1) + ceil64(w)
//   rows before it and ceil64(h+1) after it as bit words (one ballot per 64
//   rows; rows outside [0, n) read as 0), scans the words' popcounts (wave
//   scans by shuffle, 16 wave sums through LDS), and so has P(r), the flags
//   before row r, for every row of the region.  hot follows for its rows and
//   h+1 rows either side, as bit words again, with their scan H; start and end
//   for its own rows from H, and their scans.
// mark   : writes the span's totals (flags, hot rows, starts, ends).
// scan   : one wave per item turns the totals into exclusive per-span offsets
//          and writes hot_rows and count.
// emit   : a start at own row o is incident k = starts before the span + starts
//          before o in the span: writes start_k and P(start_k-w+1); an end is
//          incident (starts at or before it) - 1: writes end_k and P(end_k+1).
//          Then the peak keys: row i lies inside incident k iff the starts at
//          or before it outnumber the ends before it.  Its key is det_key's
//          (fedmx_detect.hip) order-preserving integer of the cleaned score
//          with both zeros as +0.0.  Rows of one incident are folded by a
//          segmented wave maximum (shuffles), then by 64-bit integer maxima
//          in an LDS table over the incidents of a 4,096-row chunk, and each
//          used table entry goes to key_k with one global 64-bit atomicMax: an
//          incident covering every row costs four global atomics per span.
// peak   : the same walk with ~row for the rows whose key equals key_k, 0
//          for the others: the maximum is the smallest such row.
// finish : one thread per incident: peak_row_k, peak_score_k = the cleaned
//          scores[peak_row_k] (read, not decoded), alarms_k as the difference
//          of the two prefix values, rows_covered and longest by integer atomics.
//
// LDS: 2 x 451 + 2 x 257 bit words with their prefix counts (17.0 KB) and the
// 2,112-entry table (16.9 KB).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fedmx {

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;

constexpr int INCIDENT_SPAN = 16384;        // own rows of one workgroup
constexpr int INCIDENT_MAX_WINDOW = 4096;
constexpr int INCIDENT_MAX_HOLD = 4096;
constexpr int INC_THREADS = 1024;
constexpr int INC_WAVES = INC_THREADS / 64;
constexpr int INC_HALO_AFTER = (INCIDENT_MAX_HOLD + 1 + 63) / 64 * 64;     // 4,160
constexpr int INC_HALO_BEFORE = INC_HALO_AFTER + INCIDENT_MAX_WINDOW;      // 8,256
constexpr int INC_WORDS = (INCIDENT_SPAN + INC_HALO_BEFORE + INC_HALO_AFTER) / 64;   // 450
constexpr int INC_SPAN_WORDS = INCIDENT_SPAN / 64;                          // 256
constexpr int INC_CHUNK = 4096;             // rows whose incidents share one LDS table
constexpr int INC_TABLE = 2112;             // >= INC_CHUNK / 2 + 1: starts lie at least two rows apart
static_assert(INCIDENT_SPAN >= 8192 + 4098, "one halo must suffice");
static_assert(INC_WORDS <= INC_THREADS && INC_SPAN_WORDS <= INC_THREADS, "one thread per word in the scans");
static_assert(INCIDENT_SPAN % INC_CHUNK == 0 && INC_CHUNK % INC_THREADS == 0 && INC_TABLE > INC_CHUNK / 2,
              "chunk geometry");

struct IncidentItem {
  const uint8_t* flags;   // [n]
  const double* scores;   // [n]
  u32* totals;            // [nspans][4]: flags, hot rows, starts, ends (mark)
  u32* offs;              // [nspans][4]: their exclusive prefixes over the spans (scan)
  i64* start;             // [kmax]
  i64* end;               // [kmax]
  i64* pa;                // [kmax]: flags before row start - w + 1
  i64* pb;                // [kmax]: flags before row end + 1; alarms after finish
  u64* key;               // [kmax], zeroed: largest key; peak_score's bits after finish
  u64* enc;               // [kmax], zeroed: largest ~row among the key's rows; peak_row after finish
  u64* summary;           // [4], zeroed: hot_rows, count, rows_covered, longest
  int n, nspans, window, min_alarms, hold, kmax;
};

struct IncidentSpanDesc {
  int item, span;
};

__device__ __forceinline__ double inc_clean(double v) {
  if (v != v) return 0.0;
  if (v > 1.7976931348623157e308) return 1.7976931348623157e308;
  if (v < -1.7976931348623157e308) return -1.7976931348623157e308;
  return v;
}

// det_key (fedmx_detect.hip) of the cleaned score, both zeros as +0.0: never 0
__device__ __forceinline__ u64 inc_key(double v) {
  v = inc_clean(v);
  if (v == 0.0) v = 0.0;
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// bits set below position `rel` of the bit words (`pc`: the words' exclusive popcount scan)
__device__ __forceinline__ u32 inc_before(const u64* bits, const u32* pc, int rel) {
  const int wd = rel >> 6, b = rel & 63;
  return pc[wd] + (u32)__popcll(bits[wd] & ((1ull << b) - 1ull));
}

// pc[0..nw] = exclusive scan of the popcounts of bits[0..nw); every thread of
// the workgroup calls it, with bits[] written and a barrier passed
__device__ __forceinline__ void inc_scan_words(const u64* bits, u32* pc, int nw, u32* wsum) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const u32 v = t < nw ? (u32)__popcll(bits[t]) : 0u;
  u32 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 y = __shfl_up(inc, o);
    if (lane >= o) inc += y;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  u32 base = 0u;
  for (int i = 0; i < wv; ++i) base += wsum[i];
  if (t < nw) pc[t] = base + inc - v;
  if (t == nw - 1) pc[nw] = base + inc;
  __syncthreads();
}

// PHASE 0: mark, 1: emit + peak keys, 2: peak rows
template <int PHASE>
__global__ __launch_bounds__(INC_THREADS) void incident_kernel(const IncidentItem* __restrict__ items,
                                                                const IncidentSpanDesc* __restrict__ spans) {
  __shared__ u64 s_fb[INC_WORDS + 1], s_hb[INC_WORDS + 1], s_sb[INC_SPAN_WORDS + 1], s_eb[INC_SPAN_WORDS + 1];
  __shared__ u32 s_fp[INC_WORDS + 1], s_hp[INC_WORDS + 1], s_sp[INC_SPAN_WORDS + 1], s_ep[INC_SPAN_WORDS + 1];
  __shared__ u32 s_wsum[INC_WAVES];
  const IncidentSpanDesc sd = spans[blockIdx.x];
  const IncidentItem it = items[sd.item];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int w = it.window, m = it.min_alarms, h = it.hold;
  const int ha = (h + 1 + 63) & ~63;            // rows after the span
  const int hb = ha + ((w + 63) & ~63);         // rows before it
  const int nw = (hb + INCIDENT_SPAN + ha) >> 6;
  const i64 n = it.n;
  const i64 s0 = (i64)sd.span * INCIDENT_SPAN;  // first own row
  const i64 r0 = s0 - hb;                       // first row of the region (may lie before row 0)

  // flags -> bit words
  for (int wd = wv; wd < nw; wd += INC_WAVES) {
    const i64 row = r0 + (i64)wd * 64 + lane;
    bool f = false;
    if (row >= 0 && row < n) f = it.flags[row] != 0;
    const u64 b = __ballot(f);
    if (lane == 0) s_fb[wd] = b;
  }
  if (tid == 0) {
    s_fb[nw] = 0ull;
    s_hb[nw] = 0ull;
    s_sb[INC_SPAN_WORDS] = 0ull;
    s_eb[INC_SPAN_WORDS] = 0ull;
  }
  __syncthreads();
  inc_scan_words(s_fb, s_fp, nw, s_wsum);

  // hot rows of [s0 - ha, s0 + SPAN + ha)
  const int hw0 = (hb - ha) >> 6;
  for (int wd = wv; wd < nw; wd += INC_WAVES) {
    u64 b = 0ull;
    if (wd >= hw0) {
      const int rel = wd * 64 + lane;
      const i64 row = r0 + rel;
      bool hot = false;
      if (row >= 0 && row < n)
        hot = (int)(inc_before(s_fb, s_fp, rel + 1) - inc_before(s_fb, s_fp, rel - w + 1)) >= m;
      b = __ballot(hot);
    }
    if (lane == 0) s_hb[wd] = b;
  }
  __syncthreads();
  inc_scan_words(s_hb, s_hp, nw, s_wsum);

  // starts and ends among the own rows
  const int ow0 = hb >> 6;
  for (int wd = wv; wd < INC_SPAN_WORDS; wd += INC_WAVES) {
    const int rel = (ow0 + wd) * 64 + lane;
    const bool hot = (s_hb[ow0 + wd] >> lane) & 1ull;
    bool st = false, en = false;
    if (hot) {
      st = inc_before(s_hb, s_hp, rel) == inc_before(s_hb, s_hp, rel - h - 1);
      en = inc_before(s_hb, s_hp, rel + h + 2) == inc_before(s_hb, s_hp, rel + 1);
    }
    const u64 bs = __ballot(st), be = __ballot(en);
    if (lane == 0) {
      s_sb[wd] = bs;
      s_eb[wd] = be;
    }
  }
  __syncthreads();
  inc_scan_words(s_sb, s_sp, INC_SPAN_WORDS, s_wsum);
  inc_scan_words(s_eb, s_ep, INC_SPAN_WORDS, s_wsum);

  if (PHASE == 0) {
    if (tid == 0) {
      uint4 t;
      t.x = s_fp[ow0 + INC_SPAN_WORDS] - s_fp[ow0];
      t.y = s_hp[ow0 + INC_SPAN_WORDS] - s_hp[ow0];
      t.z = s_sp[INC_SPAN_WORDS];
      t.w = s_ep[INC_SPAN_WORDS];
      reinterpret_cast<uint4*>(it.totals)[sd.span] = t;
    }
    return;
  }

  __shared__ u64 s_tbl[INC_TABLE];
  const uint4 off = reinterpret_cast<const uint4*>(it.offs)[sd.span];
  const i64 flags_off = off.x, start_off = off.z, end_off = off.w;
  const i64 kmax = it.kmax;
  // nothing of an incident in this span: no start in it and none open at its first row
  if (s_sp[INC_SPAN_WORDS] == 0u && start_off <= end_off) return;

  if (PHASE == 1) {
    const i64 f0 = (i64)s_fp[ow0];
    for (int o = tid; o < INCIDENT_SPAN; o += INC_THREADS) {
      const int wd = o >> 6, b = o & 63;
      if ((s_sb[wd] >> b) & 1ull) {
        const i64 k = start_off + inc_before(s_sb, s_sp, o);
        if (k < kmax) {
          it.start[k] = s0 + o;
          it.pa[k] = flags_off + (i64)inc_before(s_fb, s_fp, hb + o - w + 1) - f0;
        }
      }
      if ((s_eb[wd] >> b) & 1ull) {
        const i64 k = start_off + inc_before(s_sb, s_sp, o + 1) - 1;
        if (k >= 0 && k < kmax) {
          it.end[k] = s0 + o;
          it.pb[k] = flags_off + (i64)inc_before(s_fb, s_fp, hb + o + 1) - f0;
        }
      }
    }
  }

  u64* const dst = PHASE == 1 ? it.key : it.enc;
  for (int c = 0; c < INCIDENT_SPAN / INC_CHUNK; ++c) {
    if (s0 + (i64)c * INC_CHUNK >= n) break;
    for (int j = tid; j < INC_TABLE; j += INC_THREADS) s_tbl[j] = 0ull;
    __syncthreads();
    const i64 kb = start_off + inc_before(s_sb, s_sp, c * INC_CHUNK) - 1;   // the incident open at the chunk's first row, if any
    for (int o = c * INC_CHUNK + tid; o < (c + 1) * INC_CHUNK; o += INC_THREADS) {
      const i64 row = s0 + o;
      const i64 sc = start_off + inc_before(s_sb, s_sp, o + 1);   // starts at or before the row
      const i64 ec = end_off + inc_before(s_eb, s_ep, o);         // ends before it
      const bool inside = row < n && sc > ec && sc <= kmax;
      int lid = -1;
      u64 v = 0ull;
      if (inside) {
        lid = (int)(sc - 1 - kb);
        const u64 key = inc_key(it.scores[row]);
        if (PHASE == 1)
          v = key;
        else
          v = key == it.key[sc - 1] ? ~(u64)row : 0ull;
      }
      // the maximum over the lanes of one incident lands in its first lane
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int ol = __shfl_down(lid, d);
        const u64 ov = __shfl_down(v, d);
        if (lane + d < 64 && ol == lid && ov > v) v = ov;
      }
      const int pl = __shfl_up(lid, 1);
      if ((lane == 0 || pl != lid) && lid >= 0 && lid < INC_TABLE && v != 0ull) atomicMax(&s_tbl[lid], v);
    }
    __syncthreads();
    for (int j = tid; j < INC_TABLE; j += INC_THREADS) {
      const u64 v = s_tbl[j];
      const i64 k = kb + j;
      if (v != 0ull && k >= 0 && k < kmax) atomicMax(&dst[k], v);
    }
    __syncthreads();
  }
}

// one wave per item: exclusive prefixes of the span totals, hot_rows and count
__global__ __launch_bounds__(64) void incident_scan_kernel(const IncidentItem* __restrict__ items) {
  const IncidentItem it = items[blockIdx.x];
  const int lane = threadIdx.x;
  const uint4* tot = reinterpret_cast<const uint4*>(it.totals);
  uint4* offs = reinterpret_cast<uint4*>(it.offs);
  u32 c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
  for (int base = 0; base < it.nspans; base += 64) {
    const int j = base + lane;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (j < it.nspans) v = tot[j];
    u32 i0 = v.x, i1 = v.y, i2 = v.z, i3 = v.w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u32 y0 = __shfl_up(i0, o), y1 = __shfl_up(i1, o), y2 = __shfl_up(i2, o), y3 = __shfl_up(i3, o);
      if (lane >= o) {
        i0 += y0;
        i1 += y1;
        i2 += y2;
        i3 += y3;
      }
    }
    if (j < it.nspans) offs[j] = make_uint4(c0 + i0 - v.x, c1 + i1 - v.y, c2 + i2 - v.z, c3 + i3 - v.w);
    c0 += __shfl(i0, 63);
    c1 += __shfl(i1, 63);
    c2 += __shfl(i2, 63);
    c3 += __shfl(i3, 63);
  }
  if (lane == 0) {
    it.summary[0] = c1;
    it.summary[1] = c2;
  }
}

constexpr int INC_FINISH_THREADS = 256;

__global__ __launch_bounds__(INC_FINISH_THREADS) void incident_finish_kernel(const IncidentItem* __restrict__ items) {
  const IncidentItem it = items[blockIdx.y];
  i64 count = (i64)it.summary[1];
  if (count > it.kmax) count = it.kmax;
  if ((i64)blockIdx.x * INC_FINISH_THREADS >= count) return;
  const i64 k = (i64)blockIdx.x * INC_FINISH_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  u64 len = 0ull;
  if (k < count) {
    const u64 row = ~it.enc[k];
    if (row < (u64)it.n) {
      reinterpret_cast<i64*>(it.enc)[k] = (i64)row;
      reinterpret_cast<double*>(it.key)[k] = inc_clean(it.scores[row]);
    }
    it.pb[k] -= it.pa[k];
    len = (u64)(it.end[k] - it.start[k] + 1);
  }
  u64 sum = len, mx = len;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 a = __shfl_down(sum, o), b = __shfl_down(mx, o);
    sum += a;
    mx = b > mx ? b : mx;
  }
  if (lane == 0 && sum != 0ull) {
    atomicAdd(&it.summary[2], sum);
    atomicMax(&it.summary[3], mx);
  }
}

}  // namespace fedmx

extern "C" {

// The five launches over `n_spans` (item, span) descriptors of `n_items` items
// with rows, in order on `stream`.  `phases`: bit 0 mark, 1 scan, 2 emit, 3
// peak, 4 finish (31: all; single passes are for measurements and read what
// the earlier ones left).  `max_kmax`: the largest incident bound of an item.
int fedmx_incidents(const void* items, int n_items, const void* spans, int n_spans, int max_kmax, int phases,
                    hipStream_t stream) {
  using namespace fedmx;
  if (n_items <= 0 || n_spans <= 0) return 0;
  const IncidentItem* it = reinterpret_cast<const IncidentItem*>(items);
  const IncidentSpanDesc* sp = reinterpret_cast<const IncidentSpanDesc*>(spans);
  int err = 0;
  if (phases & 1) {
    hipLaunchKernelGGL(incident_kernel<0>, dim3(n_spans), dim3(INC_THREADS), 0, stream, it, sp);
    if ((err = (int)hipGetLastError()) != 0) return err;
  }
  if (phases & 2) {
    hipLaunchKernelGGL(incident_scan_kernel, dim3(n_items), dim3(64), 0, stream, it);
    if ((err = (int)hipGetLastError()) != 0) return err;
  }
  if (phases & 4) {
    hipLaunchKernelGGL(incident_kernel<1>, dim3(n_spans), dim3(INC_THREADS), 0, stream, it, sp);
    if ((err = (int)hipGetLastError()) != 0) return err;
  }
  if (phases & 8) {
    hipLaunchKernelGGL(incident_kernel<2>, dim3(n_spans), dim3(INC_THREADS), 0, stream, it, sp);
    if ((err = (int)hipGetLastError()) != 0) return err;
  }
  if ((phases & 16) && max_kmax > 0) {
    const int gx = (max_kmax + INC_FINISH_THREADS - 1) / INC_FINISH_THREADS;
    hipLaunchKernelGGL(incident_finish_kernel, dim3(gx, n_items), dim3(INC_FINISH_THREADS), 0, stream, it);
    if ((err = (int)hipGetLastError()) != 0) return err;
  }
  return 0;
}

int fedmx_incident_span_rows() { return fedmx::INCIDENT_SPAN; }
int fedmx_incident_item_size() { return (int)sizeof(fedmx::IncidentItem); }
int fedmx_incident_span_desc_size() { return (int)sizeof(fedmx::IncidentSpanDesc); }

}  // extern "C"
