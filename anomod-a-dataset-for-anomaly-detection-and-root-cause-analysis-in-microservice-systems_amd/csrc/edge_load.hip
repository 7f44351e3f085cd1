// Edge load: per (time window, call-graph edge) the time the edge's calls were
// open inside the window (busy_us) and the calls still open when the window
// opens (carried), of a grouped span set that carries start times.  The
// windowed table (edge_windows.hip) books a call in the window it starts in
// only; this one follows it for as long as it lasts.  Unlike that table's
// `outside`, a span that starts before t0 but reaches into the range is
// clipped, not dropped.
//
// Per span O(1), whatever the number of windows it covers.  With a..b the
// windows the span touches (clipped to [0, T)):
//   busy[a]    += the overlap with window a (the whole duration when a == b)
//   busy[b]    += the overlap with window b                     (a < b)
//   dfull[a+1] += 1, dfull[b] -= 1                              (a + 2 <= b)
//   dcar[f]    += 1, dcar[b+1] -= 1   (f <= b; f = 0 for a start before t0,
//                                      else a + 1; the add at index T skipped)
// and edge_load_scan_kernel takes inclusive prefix sums along w per row:
// busy[w] += full[w] * step, carried[w] = the dcar prefix.  The difference
// tables hold transient negatives as wrapped u64: any order of the atomic
// adds gives the same sums.  full[w] > 0 only when step <= dur < 2^32, so the
// product fits u64.  Nothing ever forms t0 + T * step: every comparison is a
// quotient against T or an offset inside one window.
//
// edge_load_kernel is a persistent stream over span positions in the shape of
// edge_windows_kernel (512 threads, one contiguous range per workgroup, 16-B
// non-temporal loads, 2048 spans per iteration), with two sources of the edge
// row:
//   rows  the set holds complete parent rows (anomod_spans::parent_row): row
//         2 B, svc|flags 4 B, dur 4 B, start 8 B = 18 B/span in one pass
//   keys  any other grouped set: span_edge_keys (the aggregation's own walk)
//         writes edge << 32 | dur by span position, then key 8 B + start 8 B;
//         the row column is not filled from here
// The head partial (window a) goes through a sliding LDS ring of Wt windows x
// E cells, one u64 a cell, anchored and flushed as in edge_windows.hip; a cell
// outside the tile, the tail partial and the four difference adds go to global
// atomics, so correctness never depends on the hit rate (Wt = 0: all global).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

constexpr int kLoadThreads = 512;
constexpr int kLoadPairs = 2;                              // two-span loads per lane per batch
constexpr int kLoadBatch = kLoadThreads * kLoadPairs * 2;  // spans per workgroup iteration
constexpr uint32_t kLoadLdsBudget = 40u * 1024u - 64u;     // four workgroups per CU (+ s_min)
constexpr uint64_t kLoadMaxRange = 1ull << 31;             // spans per workgroup (u32 counters)
constexpr uint32_t kNoWin = 0xFFFFFFFFu;
constexpr uint32_t kLoadSeg = 256;  // windows per scan segment (anomod_edge_load_scan_segment)
constexpr int kScanThreads = 256;
constexpr int kScanChunk = 8;  // windows a scan thread loads before it adds and stores

using u64x2 = unsigned long long __attribute__((ext_vector_type(2)));
using u32x2 = uint32_t __attribute__((ext_vector_type(2)));
using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

enum { kSrcRows = 0, kSrcKeys = 1 };

struct LoadArgs {
  const unsigned long long* keys;  // keys form: [n] edge << 32 | dur
  const uint16_t* rows;            // rows form: [n] parent rows
  const uint32_t* svcfl;           //            [n] svc | flags << 16
  const uint32_t* dur;             //            [n]
  const uint64_t* start;           // [n]
  uint64_t begin, n, per_wg;       // spans [begin, n) lie in traces; per_wg: a multiple of kLoadBatch
  uint64_t t0, step;
  uint32_t T, E, Wt;
  uint32_t S, S0;                  // rows form: the call's S, the S the rows were written with
  unsigned long long* busy;        // [T * E] or NULL
  unsigned long long* dfull;       // [T * E] full-window differences (with busy)
  unsigned long long* dcar;        // [T * E] carried differences, or NULL
  unsigned long long* misc;        // [0] outside, [1] spans that name no edge row
};

extern __shared__ __align__(16) unsigned char load_lds[];

template <int SRC>
__global__ __launch_bounds__(kLoadThreads) void edge_load_kernel(LoadArgs a) {
  const uint32_t E = a.E, Wt = a.Wt, T = a.T;
  const uint32_t cells = Wt * E;
  auto* l_busy = reinterpret_cast<unsigned long long*>(load_lds);
  __shared__ uint32_t s_min[3];
  const uint32_t tid = threadIdx.x;
  for (uint32_t c = tid; c < cells; c += kLoadThreads) l_busy[c] = 0ull;
  if (tid < 3) s_min[tid] = kNoWin;
  __syncthreads();

  // window `w` of the tile [base, base + Wt) lives in slot (slot0 + w - base) mod Wt
  auto flush_slot = [&](uint32_t slot, uint32_t w) {
    for (uint32_t e = tid; e < E; e += kLoadThreads) {
      const uint32_t c = slot * E + e;
      const unsigned long long v = l_busy[c];
      if (!v) continue;
      atomicAdd(a.busy + (uint64_t)w * E + e, v);
      l_busy[c] = 0ull;
    }
  };

  const uint64_t lo = (uint64_t)blockIdx.x * a.per_wg;
  const uint64_t hi = lo + a.per_wg < a.n ? lo + a.per_wg : a.n;
  bool anchored = false;
  uint32_t base = 0, slot0 = 0;
  uint32_t outside = 0, bad = 0;
  uint32_t it = 0;
  for (uint64_t b = lo; b < hi; b += kLoadBatch, ++it) {
    uint64_t st[kLoadPairs * 2];
    uint32_t edge[kLoadPairs * 2], dur[kLoadPairs * 2];
    bool live[kLoadPairs * 2];
    if constexpr (SRC == kSrcRows) {
      uint32_t row[kLoadPairs * 2], sf[kLoadPairs * 2];
      // four consecutive spans a lane: 16 B of svc|flags, 16 B of durations,
      // 8 B of rows and two 16-B loads of start times
      static_assert(kLoadPairs == 2, "the rows form loads four spans a lane");
      const uint64_t i0 = b + (uint64_t)tid * 4;
      if (b + kLoadBatch <= hi) {  // (b is a multiple of kLoadBatch: aligned groups)
        const u64x2 s0 = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.start + i0));
        const u64x2 s1 = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.start + i0 + 2));
        const u32x4 f = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.svcfl + i0));
        const u32x4 d = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.dur + i0));
        const u32x2 r = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(a.rows + i0));
        st[0] = s0.x, st[1] = s0.y, st[2] = s1.x, st[3] = s1.y;
        sf[0] = f.x, sf[1] = f.y, sf[2] = f.z, sf[3] = f.w;
        dur[0] = d.x, dur[1] = d.y, dur[2] = d.z, dur[3] = d.w;
        row[0] = r.x & 0xFFFFu, row[1] = r.x >> 16, row[2] = r.y & 0xFFFFu, row[3] = r.y >> 16;
#pragma unroll
        for (int j = 0; j < 4; ++j) live[j] = i0 + j >= a.begin;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint64_t i = i0 + j;
          live[j] = i < hi && i >= a.begin;
          st[j] = live[j] ? a.start[i] : 0ull;
          sf[j] = live[j] ? a.svcfl[i] : 0u;
          dur[j] = live[j] ? a.dur[i] : 0u;
          row[j] = live[j] ? (uint32_t)a.rows[i] : 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < kLoadPairs * 2; ++j) {
        // root / orphan codes of the aggregation that wrote the rows -> this call's
        const uint32_t p = row[j] >= a.S0 ? row[j] - a.S0 + a.S : row[j];
        const uint32_t svc = sf[j] & 0xFFFFu;
        edge[j] = p < a.S + ANOMOD_ROOT_ROWS && svc < a.S ? p * a.S + svc : kNoWin;
      }
    } else {
      unsigned long long key[kLoadPairs * 2];
      if (b + kLoadBatch <= hi) {
#pragma unroll
        for (int j = 0; j < kLoadPairs; ++j) {
          const uint64_t i = b + ((uint64_t)j * kLoadThreads + tid) * 2;
          const u64x2 k = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.keys + i));
          const u64x2 s = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.start + i));
          key[2 * j] = k.x, key[2 * j + 1] = k.y;
          st[2 * j] = s.x, st[2 * j + 1] = s.y;
          live[2 * j] = i >= a.begin;
          live[2 * j + 1] = i + 1 >= a.begin;
        }
      } else {
#pragma unroll
        for (int j = 0; j < kLoadPairs * 2; ++j) {
          const uint64_t i = b + ((uint64_t)(j >> 1) * kLoadThreads + tid) * 2 + (j & 1);
          live[j] = i < hi && i >= a.begin;
          key[j] = live[j] ? a.keys[i] : 0ull;
          st[j] = live[j] ? a.start[i] : 0ull;
        }
      }
#pragma unroll
      for (int j = 0; j < kLoadPairs * 2; ++j) {
        edge[j] = (uint32_t)(key[j] >> 32);
        dur[j] = (uint32_t)key[j];
      }
    }
    uint32_t wa[kLoadPairs * 2];              // window of the head partial, kNoWin: none
    unsigned long long head[kLoadPairs * 2];  // the head partial
    uint32_t lmin = kNoWin;
#pragma unroll
    for (int j = 0; j < kLoadPairs * 2; ++j) {
      wa[j] = kNoWin;
      head[j] = 0ull;
      if (!live[j]) continue;
      if (edge[j] >= E) {  // never for rows of the aggregation / keys of span_edge_keys
        ++bad;
        continue;
      }
      const uint64_t s = st[j];
      uint64_t e = s + (uint64_t)dur[j];
      if (e < s) e = ~0ull;  // saturating, as in the critical path
      if (e == s || e <= a.t0) {  // (e == s: dur 0, or a start of 2^64 - 1)
        ++outside;
        continue;
      }
      // Everything from here is relative to t0 and to one window: the span
      // covers `len` microseconds from offset `oa` of window `aw` on.
      const bool before = s < a.t0;
      uint64_t aw = 0, oa = 0;
      if (!before) {
        const uint64_t rs = s - a.t0;
        aw = rs / a.step;
        if (aw >= (uint64_t)T) {  // s >= t0 + T * step, without forming it
          ++outside;
          continue;
        }
        oa = rs - aw * a.step;
      }
      const uint64_t len = before ? e - a.t0 : e - s;  // 1 <= len < 2^32
      const uint64_t room = a.step - oa;               // what window aw still holds, >= 1
      const uint32_t w0 = (uint32_t)aw;
      uint32_t w1 = w0;  // the last window touched, clipped to T - 1
      wa[j] = w0;
      lmin = lmin < w0 ? lmin : w0;
      if (len <= room) {
        head[j] = len;
      } else {  // (rare at collector step sizes)
        head[j] = room;
        const uint32_t x = (uint32_t)(len - room);  // past the end of window aw, >= 1
        const uint32_t k = a.step > 0xFFFFFFFFull ? 0u : (x - 1u) / (uint32_t)a.step;
        const uint64_t qe = aw + 1ull + k;  // the window of the span's last microsecond
        const bool clip = qe >= (uint64_t)T;
        w1 = clip ? T - 1u : (uint32_t)qe;
        if (a.busy && w1 > w0) {
          const unsigned long long tail = clip ? a.step : (uint64_t)x - (uint64_t)k * a.step;
          atomicAdd(a.busy + (uint64_t)w1 * E + edge[j], tail);
          if (w1 >= w0 + 2u) {
            atomicAdd(a.dfull + (uint64_t)(w0 + 1u) * E + edge[j], 1ull);
            atomicAdd(a.dfull + (uint64_t)w1 * E + edge[j], ~0ull);
          }
        }
      }
      if (a.dcar) {
        const uint32_t f = before ? 0u : w0 + 1u;
        if (f <= w1) {
          atomicAdd(a.dcar + (uint64_t)f * E + edge[j], 1ull);
          if (w1 + 1u < T) atomicAdd(a.dcar + (uint64_t)(w1 + 1u) * E + edge[j], ~0ull);
        }
      }
    }
    if (!a.busy) continue;  // (uniform) only the carried table was asked for
    if (Wt) {               // (uniform) move the tile's anchor to the batch's smallest window
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)lmin, o);
        lmin = lmin < other ? lmin : other;
      }
      if ((tid & 63u) == 0 && lmin != kNoWin) atomicMin(&s_min[it % 3u], lmin);
      __syncthreads();  // also: the previous batch's LDS atomics have landed
      const uint32_t bmin = s_min[it % 3u];
      if (tid == 0) s_min[(it + 2u) % 3u] = kNoWin;  // read last in batch it - 1
      if (bmin != kNoWin) {
        if (!anchored) {
          anchored = true;
          base = bmin;
        } else if (bmin > base) {
          const uint32_t adv = bmin - base;
          const uint32_t nf = adv < Wt ? adv : Wt;
          for (uint32_t k = 0; k < nf; ++k) {
            const uint32_t s = slot0 + k;
            flush_slot(s >= Wt ? s - Wt : s, base + k);
          }
          slot0 = adv < Wt ? (slot0 + adv >= Wt ? slot0 + adv - Wt : slot0 + adv) : 0u;
          base = bmin;
          __syncthreads();  // slots are clean before anyone reuses them
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kLoadPairs * 2; ++j) {
      if (wa[j] == kNoWin) continue;
      if (anchored && wa[j] >= base && wa[j] - base < Wt) {
        uint32_t s = slot0 + (wa[j] - base);
        s = s >= Wt ? s - Wt : s;
        atomicAdd(&l_busy[s * E + edge[j]], head[j]);
      } else {
        atomicAdd(a.busy + (uint64_t)wa[j] * E + edge[j], head[j]);
      }
    }
  }
  if (Wt && a.busy) {
    __syncthreads();
    if (anchored)
      for (uint32_t k = 0; k < Wt && (uint64_t)base + k < T; ++k) {
        const uint32_t s = slot0 + k;
        flush_slot(s >= Wt ? s - Wt : s, base + k);
      }
  }
  for (int o = 32; o > 0; o >>= 1) {
    outside += (uint32_t)__shfl_xor((int)outside, o);
    bad += (uint32_t)__shfl_xor((int)bad, o);
  }
  if ((tid & 63u) == 0) {
    if (outside) atomicAdd(a.misc, (unsigned long long)outside);
    if (bad) atomicAdd(a.misc + 1, (unsigned long long)bad);
  }
}

// The prefix sums along w and the full * step fold, over the T x E cells.
// Adjacent rows are adjacent in memory, so lanes take rows; T is cut into
// G = ceil(T / kLoadSeg) segments and a thread owns one (segment, row):
//   phase 0  the segment's totals of both difference tables -> tf / tc [G * E]
//   phase 1  one thread per row: exclusive prefix of the totals over the G
//            (<= 256) segments, in place
//   phase 2  every (segment, row) starts from its carried-in prefix and walks
//            its kLoadSeg windows: busy += full * step, dcar becomes carried
// Phases 0 and 2 are bounded by the number of cells per thread-step; a call of
// one segment runs phase 2 alone.  Either table pair may be absent.
struct ScanArgs {
  unsigned long long* busy;   // [T * E] or NULL
  unsigned long long* dfull;  // with busy
  unsigned long long* dcar;   // [T * E] or NULL; carried on return
  unsigned long long* tf;     // [G * E] segment totals (G > 1)
  unsigned long long* tc;
  uint64_t step;
  uint32_t T, E, G;
};

__global__ __launch_bounds__(kScanThreads) void edge_load_scan_kernel(ScanArgs a, int phase) {
  const uint64_t idx = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
  const uint64_t E = a.E;
  if (phase == 1) {
    if (idx >= E) return;
    unsigned long long rf = 0ull, rc = 0ull;
    for (uint32_t g = 0; g < a.G; ++g) {
      const uint64_t c = (uint64_t)g * E + idx;
      if (a.dfull) {
        const unsigned long long v = a.tf[c];
        a.tf[c] = rf;
        rf += v;
      }
      if (a.dcar) {
        const unsigned long long v = a.tc[c];
        a.tc[c] = rc;
        rc += v;
      }
    }
    return;
  }
  if (idx >= (uint64_t)a.G * E) return;
  const uint32_t g = (uint32_t)(idx / E);
  const uint64_t row = idx - (uint64_t)g * E;
  const uint32_t w0 = g * kLoadSeg;
  const uint32_t w1 = a.T - w0 < kLoadSeg ? a.T : w0 + kLoadSeg;
  // kScanChunk windows a round: every load of the round is issued before the
  // first dependent add and the first store (the tables may alias for all the
  // compiler knows), so a thread pays the memory latency once a round
  if (phase == 0) {
    unsigned long long sf = 0ull, sc = 0ull;
    for (uint32_t wb = w0; wb < w1; wb += kScanChunk) {
      unsigned long long vf[kScanChunk], vc[kScanChunk];
#pragma unroll
      for (int k = 0; k < kScanChunk; ++k) {
        const uint32_t w = wb + k < w1 ? wb + k : w1 - 1u;
        const uint64_t c = (uint64_t)w * E + row;
        vf[k] = a.dfull ? a.dfull[c] : 0ull;
        vc[k] = a.dcar ? a.dcar[c] : 0ull;
      }
#pragma unroll
      for (int k = 0; k < kScanChunk; ++k)
        if (wb + k < w1) sf += vf[k], sc += vc[k];
    }
    if (a.dfull) a.tf[idx] = sf;
    if (a.dcar) a.tc[idx] = sc;
    return;
  }
  unsigned long long rf = a.G > 1u && a.dfull ? a.tf[idx] : 0ull;
  unsigned long long rc = a.G > 1u && a.dcar ? a.tc[idx] : 0ull;
  for (uint32_t wb = w0; wb < w1; wb += kScanChunk) {
    unsigned long long vf[kScanChunk], vc[kScanChunk], vb[kScanChunk];
#pragma unroll
    for (int k = 0; k < kScanChunk; ++k) {
      const uint32_t w = wb + k < w1 ? wb + k : w1 - 1u;
      const uint64_t c = (uint64_t)w * E + row;
      vf[k] = a.dfull ? a.dfull[c] : 0ull;
      vb[k] = a.dfull ? a.busy[c] : 0ull;
      vc[k] = a.dcar ? a.dcar[c] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < kScanChunk; ++k) {
      if (wb + k >= w1) break;
      const uint64_t c = (uint64_t)(wb + k) * E + row;
      if (a.dfull) {
        rf += vf[k];
        if (rf) a.busy[c] = vb[k] + rf * a.step;
      }
      if (a.dcar) {
        rc += vc[k];
        if (rc != vc[k]) a.dcar[c] = rc;  // (else the cell already holds it)
      }
    }
  }
}

// Value of a numeric environment cap, "no cap" when unset or not a number;
// ANOMOD_EDGE_LOAD_WGS must be at least 1.
uint64_t load_env_cap(const char* name) {
  const char* e = getenv(name);
  if (!e || !*e) return 0xFFFFFFFFull;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  if (*end) return 0xFFFFFFFFull;
  return !strcmp(name, "ANOMOD_EDGE_LOAD_WGS") && v == 0 ? 1 : (uint64_t)v;
}

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

uint32_t anomod_edge_load_scan_segment(void) { return kLoadSeg; }

int anomod_edge_load_spans(anomod_ctx* ctx, const anomod_spans* spans, anomod_edge_load* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_edge_load_spans: NULL argument");
  const uint32_t S = out->n_services, T = out->n_windows;
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  ANOMOD_REQUIRE(ctx, T >= 1 && T <= 65536, "n_windows=%u outside [1, 65536]", T);
  ANOMOD_REQUIRE(ctx, (uint64_t)T * E <= (1ull << 24), "n_windows * edge rows = %u * %u > 2^24", T,
                 E);
  ANOMOD_REQUIRE(ctx, out->step_us >= 1, "step_us must be at least 1");
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_REQUIRE(ctx, spans->grouped, "span set is not grouped by trace: anomod_spans_group first");
  if (!spans->start_us) {
    set_error(ctx, "span set has no start-time column: anomod_spans_set_start_us first");
    return ANOMOD_ESTATE;
  }
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "span service index %u >= n_services %u", spans->max_svc, S);
  uint64_t in_traces[2];
  if (spans->n_traces && spans->n_spans)
    if (int rc = bind(ctx)) return rc;
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  const uint64_t n = in_traces[1] > in_traces[0] ? in_traces[1] : 0;
  const uint64_t TE = (uint64_t)T * E;
  out->outside = 0;
  if (n == 0) {
    if (out->busy_us) memset(out->busy_us, 0, TE * 8);
    if (out->carried) memset(out->carried, 0, TE * 8);
    return ANOMOD_OK;
  }
  // the rows form: complete parent rows over exactly the spans in traces
  const bool rows = span_rows_ready(spans) && spans->rows_lo == in_traces[0] &&
                    spans->rows_hi == in_traces[1];
  const uint32_t G = (T + kLoadSeg - 1) / kLoadSeg;
  // One workspace in the windowed table's slot: (keys form: keys | the key
  // walk's words |) misc + the requested tables (zeroed together) | the scan's
  // segment totals.
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t b_keys = rows ? 0 : al(n * 8);
  const size_t b_ws = rows ? 0 : al(span_edge_keys_ws_bytes(spans));
  const size_t b_u64 = al(TE * 8), b_tot = G > 1 ? al((size_t)G * E * 8) : 0;
  const size_t b_tab = 256 + (out->busy_us ? 2 * b_u64 : 0) + (out->carried ? b_u64 : 0);
  const size_t b_scan = (out->busy_us ? b_tot : 0) + (out->carried ? b_tot : 0);
  char* w = nullptr;
  if (int rc = ensure_scratch(ctx, kScratchEdgeWindows, b_keys + b_ws + b_tab + b_scan,
                              reinterpret_cast<void**>(&w)))
    return rc;
  LoadArgs a{};
  auto* keys = reinterpret_cast<unsigned long long*>(w);
  auto* ws = reinterpret_cast<unsigned long long*>(w + b_keys);
  char* t = w + b_keys + b_ws;
  a.misc = reinterpret_cast<unsigned long long*>(t);
  t += 256;
  auto take = [&](bool want, size_t bytes) -> unsigned long long* {
    char* p = want ? t : nullptr;
    if (want) t += bytes;
    return reinterpret_cast<unsigned long long*>(p);
  };
  a.busy = take(out->busy_us, b_u64);
  a.dfull = take(out->busy_us, b_u64);
  a.dcar = take(out->carried, b_u64);
  ScanArgs sc{};
  sc.busy = a.busy;
  sc.dfull = a.dfull;
  sc.dcar = a.dcar;
  sc.tf = take(out->busy_us && G > 1, b_tot);
  sc.tc = take(out->carried && G > 1, b_tot);
  sc.step = out->step_us;
  sc.T = T;
  sc.E = E;
  sc.G = G;
  if (rows) {
    a.rows = spans->parent_row;
    a.svcfl = spans->svc_flags;
    a.dur = spans->dur_us;
    a.S0 = spans->rows_S;
  } else {
    a.keys = keys;
  }
  a.start = spans->start_us;
  a.begin = in_traces[0];
  a.n = n;
  a.t0 = out->t0_us;
  a.step = out->step_us;
  a.T = T;
  a.E = E;
  a.S = S;
  a.Wt = out->busy_us ? std::min<uint32_t>(kLoadLdsBudget / (E * 8u), T) : 0u;
  // (tests, A/B: fewer tile windows — 0 = every partial to global atomics — and
  // fewer workgroups, so that small sets give a workgroup several batches)
  a.Wt = std::min<uint32_t>(a.Wt, (uint32_t)load_env_cap("ANOMOD_EDGE_LOAD_TILE"));
  const size_t lds = (size_t)a.Wt * E * 8;
  auto fn = rows ? edge_load_kernel<kSrcRows> : edge_load_kernel<kSrcKeys>;
  int per_cu = 0;
  ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void*>(fn), kLoadThreads, lds));
  // persistent workgroups, one contiguous range of whole batches each
  const uint64_t batches = (n + kLoadBatch - 1) / kLoadBatch;
  uint64_t grid = std::min<uint64_t>((uint64_t)ctx->num_cus * (per_cu > 0 ? per_cu : 1), batches);
  grid = std::min<uint64_t>(grid, load_env_cap("ANOMOD_EDGE_LOAD_WGS"));
  a.per_wg = (batches + grid - 1) / grid * kLoadBatch;
  if (a.per_wg > kLoadMaxRange) a.per_wg = kLoadMaxRange;  // (more workgroups than are resident)
  grid = (n + a.per_wg - 1) / a.per_wg;
  if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests, timing)
    fprintf(stderr, "anomod: edge load kernel edge_load_kernel<%s>, tile %u windows\n",
            rows ? "rows" : "keys", a.Wt);
  if (int rc = stage_begin(ctx, kStageEdgeLoad)) return rc;
  ANOMOD_HIP(ctx, hipMemsetAsync(a.misc, 0, b_tab, ctx->stream));
  if (!rows)
    if (int rc = span_edge_keys(ctx, spans, S, keys, ws)) return rc;
  if (int rc = stage_begin(ctx, kStageEdgeLoadKernel)) return rc;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kLoadThreads), lds, ctx->stream, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeLoadKernel)) return rc;
  if (int rc = stage_begin(ctx, kStageEdgeLoadScan)) return rc;
  const uint64_t seg_threads = (uint64_t)G * E;
  const unsigned seg_grid = (unsigned)((seg_threads + kScanThreads - 1) / kScanThreads);
  if (G > 1) {
    hipLaunchKernelGGL(edge_load_scan_kernel, dim3(seg_grid), dim3(kScanThreads), 0, ctx->stream,
                       sc, 0);
    hipLaunchKernelGGL(edge_load_scan_kernel, dim3((E + kScanThreads - 1) / kScanThreads),
                       dim3(kScanThreads), 0, ctx->stream, sc, 1);
  }
  hipLaunchKernelGGL(edge_load_scan_kernel, dim3(seg_grid), dim3(kScanThreads), 0, ctx->stream, sc,
                     2);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeLoadScan)) return rc;
  if (int rc = stage_end(ctx, kStageEdgeLoad)) return rc;
  unsigned long long misc[2] = {0ull, 0ull};
  ANOMOD_HIP(ctx, hipMemcpyAsync(misc, a.misc, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (out->busy_us)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->busy_us, a.busy, TE * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
  if (out->carried)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->carried, a.dcar, TE * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (misc[1]) {
    set_error(ctx, "edge load: %llu spans carry no edge row (internal error)", misc[1]);
    return ANOMOD_ESTATE;
  }
  out->outside = misc[0];
  return ANOMOD_OK;
}

}  // extern "C"
