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
// edge_load_kernel is the shared edge stream (edge_stream.h) in both of its
// forms: rows (row 2 B, svc|flags 4 B, dur 4 B, start 8 B = 18 B/span in one
// pass) and keys (key 8 B + start 8 B after span_edge_keys).  The head partial
// (window a) goes through the stream's sliding LDS window ring, one u64 a cell;
// a cell outside the tile, the tail partial and the four difference adds go to
// global atomics, so correctness never depends on the hit rate (Wt = 0: all
// global).
#include <algorithm>
#include <cstring>

#include "edge_stream.h"

namespace anomod {
namespace {

constexpr int kLoadThreads = 512;                       // 2048 spans per workgroup iteration
constexpr uint32_t kLoadLdsBudget = 40u * 1024u - 64u;  // four workgroups per CU (+ the ring's minima)
constexpr uint32_t kLoadSeg = 256;  // windows per scan segment (anomod_edge_load_scan_segment)
constexpr int kScanThreads = 256;
constexpr int kScanChunk = 8;  // windows a scan thread loads before it adds and stores

enum { kSrcRows = 0, kSrcKeys = 1 };

struct LoadArgs {
  const unsigned long long* keys;  // keys form: [n] edge << 32 | dur
  const uint16_t* rows;            // rows form: [n] parent rows
  const uint32_t* svcfl;           //            [n] svc | flags << 16
  const uint32_t* dur;             //            [n]
  const uint64_t* start;           // [n]
  uint64_t begin, n, per_wg;       // spans [begin, n) lie in traces; per_wg: a multiple of the batch
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
  using Lanes = stream::Lanes<kLoadThreads, SRC == kSrcRows ? 4 : 2>;
  const uint32_t E = a.E, T = a.T;
  const uint32_t cells = a.Wt * E;
  auto* l_busy = reinterpret_cast<unsigned long long*>(load_lds);
  const uint32_t tid = threadIdx.x;
  stream::WindowRing ring{a.Wt};
  for (uint32_t c = tid; c < cells; c += kLoadThreads) l_busy[c] = 0ull;
  ring.init(tid);
  __syncthreads();

  auto flush_slot = [&](uint32_t slot, uint32_t w) {
    for (uint32_t e = tid; e < E; e += kLoadThreads) {
      const uint32_t c = slot * E + e;
      const unsigned long long v = l_busy[c];
      if (!v) continue;
      atomicAdd(a.busy + (uint64_t)w * E + e, v);
      l_busy[c] = 0ull;
    }
  };

  uint64_t lo, hi;
  stream::wg_range(a.per_wg, a.n, &lo, &hi);
  uint32_t outside = 0, bad = 0;
  uint32_t it = 0;
  for (uint64_t b = lo; b < hi; b += Lanes::kBatch, ++it) {
    Lanes L(b, hi, a.begin, tid);
    uint64_t st[4];
    uint32_t edge[4], dur[4];
    if constexpr (SRC == kSrcRows) {
      uint32_t sf[4];
      stream::load_rows(L, a.rows, a.svcfl, a.dur, a.S, a.S0, edge, dur, sf, a.start, st);
    } else {
      stream::load_keys(L, a.keys, edge, dur, a.start, st);
    }
    uint32_t wa[4];              // window of the head partial, kNone: none
    unsigned long long head[4];  // the head partial
    uint32_t lmin = stream::kNone;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wa[j] = stream::kNone;
      head[j] = 0ull;
      if (!L.live[j]) continue;
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
    ring.advance(it, lmin, tid, flush_slot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (wa[j] == stream::kNone) continue;
      const uint32_t s = ring.slot_of(wa[j]);
      if (s != stream::kNone) {
        atomicAdd(&l_busy[s * E + edge[j]], head[j]);
      } else {
        atomicAdd(a.busy + (uint64_t)wa[j] * E + edge[j], head[j]);
      }
    }
  }
  if (a.busy) ring.finish(T, flush_slot);
  stream::count_add(a.misc, outside, tid);
  stream::count_add(a.misc + 1, bad, tid);
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

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

uint32_t anomod_edge_load_scan_segment(void) { return kLoadSeg; }

int anomod_edge_load_spans(anomod_ctx* ctx, const anomod_spans* spans, anomod_edge_load* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_edge_load_spans: NULL argument");
  const uint32_t S = out->n_services, T = out->n_windows;
  uint32_t E = 0;
  uint64_t in_traces[2], n = 0;
  if (int rc = stream_table_args(ctx, S, T, out->step_us, &E)) return rc;
  if (int rc = stream_set_args(ctx, spans, S, true, ANOMOD_EINVAL, in_traces, &n)) return rc;
  const uint64_t TE = (uint64_t)T * E;
  out->outside = 0;
  if (n == 0) {
    if (out->busy_us) memset(out->busy_us, 0, TE * 8);
    if (out->carried) memset(out->carried, 0, TE * 8);
    return ANOMOD_OK;
  }
  EdgeSource src(spans, in_traces, n);
  const uint32_t G = (T + kLoadSeg - 1) / kLoadSeg;
  // One workspace in the windowed table's slot: (keys form: keys | the key
  // walk's words |) misc + the requested tables (zeroed together) | the scan's
  // segment totals.
  const size_t b_u64 = Carve::al(TE * 8), b_tot = G > 1 ? Carve::al((size_t)G * E * 8) : 0;
  const size_t b_tab = 256 + (out->busy_us ? 2 * b_u64 : 0) + (out->carried ? b_u64 : 0);
  const size_t b_scan = (out->busy_us ? b_tot : 0) + (out->carried ? b_tot : 0);
  char* w = nullptr;
  if (int rc = ensure_scratch(ctx, kScratchEdgeWindows, src.b_keys + src.b_ws + b_tab + b_scan,
                              reinterpret_cast<void**>(&w)))
    return rc;
  Carve cv{w + src.b_keys + src.b_ws};
  LoadArgs a{};
  a.misc = cv.take<unsigned long long>(256);
  a.busy = cv.take<unsigned long long>(b_u64, out->busy_us);
  a.dfull = cv.take<unsigned long long>(b_u64, out->busy_us);
  a.dcar = cv.take<unsigned long long>(b_u64, out->carried);
  ScanArgs sc{};
  sc.busy = a.busy;
  sc.dfull = a.dfull;
  sc.dcar = a.dcar;
  sc.tf = cv.take<unsigned long long>(b_tot, out->busy_us && G > 1);
  sc.tc = cv.take<unsigned long long>(b_tot, out->carried && G > 1);
  sc.step = out->step_us;
  sc.T = T;
  sc.E = E;
  sc.G = G;
  if (src.rows) {
    a.rows = spans->parent_row;
    a.svcfl = spans->svc_flags;
    a.dur = spans->dur_us;
    a.S0 = spans->rows_S;
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
  a.Wt = std::min<uint32_t>(a.Wt, (uint32_t)env_cap("ANOMOD_EDGE_LOAD_TILE"));
  const size_t lds = (size_t)a.Wt * E * 8;
  auto fn = src.rows ? edge_load_kernel<kSrcRows> : edge_load_kernel<kSrcKeys>;
  uint64_t grid = 0;
  if (int rc = stream_geometry(ctx, fn, kLoadThreads, lds, n, "ANOMOD_EDGE_LOAD_WGS", &a.per_wg,
                               &grid))
    return rc;
  if (log_kernel())  // (tests, timing)
    fprintf(stderr, "anomod: edge load kernel edge_load_kernel<%s>, tile %u windows\n",
            src.rows ? "rows" : "keys", a.Wt);
  stream_log("edge_load_kernel", src.rows ? "rows" : "keys", a.Wt, nullptr, grid, a.per_wg);
  if (int rc = stage_begin(ctx, kStageEdgeLoad)) return rc;
  ANOMOD_HIP(ctx, hipMemsetAsync(a.misc, 0, b_tab, ctx->stream));
  if (int rc = src.fill(ctx, spans, S, w)) return rc;
  a.keys = src.keys;
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
  ANOMOD_HIP(ctx, stream_back(ctx, out->busy_us, a.busy, TE * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->carried, a.dcar, TE * 8));
  unsigned long long misc[2];
  if (int rc = stream_finish(ctx, a.misc, 1, "edge load", "row", misc)) return rc;
  out->outside = misc[0];
  return ANOMOD_OK;
}

}  // extern "C"
