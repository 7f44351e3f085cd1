// Windowed edge table: per (time window, call-graph edge) count / errors /
// latency sum / max of a grouped span set that carries start times, plus the
// start-time column itself (set / get / synthetic fill).
//
// Two passes.  Pass 1 is the aggregation kernels' own walk in its key form
// (span_edge_keys, edge_agg.hip): keys[i] = edge row << 32 | dur_us by span
// position, so the edge of a span is by construction the row
// anomod_edge_aggregate_spans counts it in.  Pass 2 (edge_windows_kernel) is
// the keys form of the shared edge stream (edge_stream.h): 20 B read per span
// (key 8, start 8, svc|flags 4), accumulated into cell w * E + edge.  The 16 B
// / span key round trip through HBM is the known cost of not fusing the
// accumulation into the walk.
//
// Pass 2 privatises cells in LDS in the stream's sliding window ring: every
// workgroup owns one contiguous span range, and collector files (and the
// synthetic fill) are close to time-ordered, so a range touches a narrow band
// of windows.  A cell is count | errors << 32 as one u64, sum u64, max u32 =
// 20 B, in three planes.  A workgroup's range holds < 2^32 spans, so the u32
// halves of the packed count | errors word cannot carry into each other.
#include <algorithm>
#include <cstring>

#include "edge_stream.h"

namespace anomod {
namespace {

constexpr int kWinThreads = 512;
constexpr uint32_t kWinLdsBudget = 64u * 1024u - 64u;  // two workgroups per CU (+ the ring's minima)
constexpr uint32_t kCellBytes = 20;
using WinLanes = stream::Lanes<kWinThreads, 2>;  // 2048 spans per workgroup iteration

struct WinArgs {
  const unsigned long long* keys;   // [n] edge << 32 | dur
  const uint64_t* start;            // [n]
  const uint32_t* svcfl;            // [n] svc | flags << 16
  uint64_t begin, n, per_wg;        // spans [begin, n) lie in traces; per_wg: a multiple of the batch
  uint64_t t0, step;
  uint32_t T, E, Wt;
  unsigned long long* count;        // [T * E] each, or NULL
  unsigned long long* errors;
  unsigned long long* sum;
  unsigned int* mx;
  unsigned long long* misc;         // [0] outside, [1] spans whose key names no edge row
};

__device__ inline void cell_global(const WinArgs& a, uint64_t cell, uint32_t cnt, uint32_t err,
                                   unsigned long long sum, uint32_t mx) {
  if (a.count) atomicAdd(a.count + cell, (unsigned long long)cnt);
  if (a.errors && err) atomicAdd(a.errors + cell, (unsigned long long)err);
  if (a.sum && sum) atomicAdd(a.sum + cell, sum);
  if (a.mx && mx) atomicMax(a.mx + cell, mx);
}

extern __shared__ __align__(16) unsigned char win_lds[];

__global__ __launch_bounds__(kWinThreads) void edge_windows_kernel(WinArgs a) {
  const uint32_t E = a.E;
  const uint32_t cells = a.Wt * E;
  auto* l_ce = reinterpret_cast<unsigned long long*>(win_lds);  // count | errors << 32
  auto* l_sum = l_ce + cells;
  auto* l_mx = reinterpret_cast<unsigned int*>(l_sum + cells);
  const uint32_t tid = threadIdx.x;
  stream::WindowRing ring{a.Wt};
  for (uint32_t c = tid; c < cells; c += kWinThreads) {
    l_ce[c] = 0ull;
    l_sum[c] = 0ull;
    l_mx[c] = 0u;
  }
  ring.init(tid);
  __syncthreads();

  auto flush_slot = [&](uint32_t slot, uint32_t w) {
    for (uint32_t e = tid; e < E; e += kWinThreads) {
      const uint32_t c = slot * E + e;
      const unsigned long long ce = l_ce[c];
      if (!ce) continue;
      cell_global(a, (uint64_t)w * E + e, (uint32_t)ce, (uint32_t)(ce >> 32), l_sum[c], l_mx[c]);
      l_ce[c] = 0ull;
      l_sum[c] = 0ull;
      l_mx[c] = 0u;
    }
  };

  uint64_t lo, hi;
  stream::wg_range(a.per_wg, a.n, &lo, &hi);
  uint32_t outside = 0, bad = 0;
  uint32_t it = 0;
  for (uint64_t b = lo; b < hi; b += WinLanes::kBatch, ++it) {
    WinLanes L(b, hi, a.begin, tid);
    uint32_t edge[4], dur[4], sf[4];
    uint64_t st[4];
    stream::load_keys(L, a.keys, edge, dur, a.start, st, a.svcfl, sf);
    uint32_t w[4];
    uint32_t lmin = stream::kNone;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = stream::kNone;
      if (!L.live[j]) continue;
      if (edge[j] >= E) {  // never for keys of span_edge_keys
        ++bad;
        continue;
      }
      w[j] = stream::window_of(st[j], a.t0, a.step, a.T);
      if (w[j] == stream::kNone) {
        ++outside;
        continue;
      }
      lmin = lmin < w[j] ? lmin : w[j];
    }
    ring.advance(it, lmin, tid, flush_slot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (w[j] == stream::kNone) continue;
      const uint32_t err = (sf[j] >> 16) & ANOMOD_FLAG_ERROR;
      const uint32_t s = ring.slot_of(w[j]);
      if (s != stream::kNone) {
        const uint32_t c = s * E + edge[j];
        atomicAdd(&l_ce[c], 1ull | ((unsigned long long)err << 32));
        if (dur[j]) {
          atomicAdd(&l_sum[c], (unsigned long long)dur[j]);
          atomicMax(&l_mx[c], dur[j]);
        }
      } else {
        cell_global(a, (uint64_t)w[j] * E + edge[j], 1u, err, dur[j], dur[j]);
      }
    }
  }
  ring.finish(a.T, flush_slot);
  stream::count_add(a.misc, outside, tid);
  stream::count_add(a.misc + 1, bad, tid);
}

// start[i] = t0 + (t * period) / n_traces + pos * gap.  One wave per 64
// consecutive traces: the lanes hold the 64 trace starts, walk the traces'
// span range 64 spans at a time (coalesced stores) and find each span's
// trace among the 64 by a shuffle binary search.
__global__ __launch_bounds__(256) void fill_start_kernel(const uint64_t* __restrict__ trace_ptr,
                                                         uint64_t n_traces, uint64_t t0,
                                                         uint64_t period, uint64_t gap,
                                                         uint64_t* __restrict__ start) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_groups = (n_traces + 63) / 64;
  for (uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups;
       g += (uint64_t)gridDim.x * 4) {
    const uint64_t tl = g * 64 + lane;
    const uint64_t p = trace_ptr[tl < n_traces ? tl : n_traces];
    const uint64_t te = g * 64 + 64;
    const uint64_t first = trace_ptr[g * 64];                        // wave-uniform
    const uint64_t last = trace_ptr[te < n_traces ? te : n_traces];  // wave-uniform
    for (uint64_t b = first; b < last; b += 64) {
      const uint64_t i = b + lane;
      uint32_t l = 0;  // largest lane whose trace starts at or before span i
      for (uint32_t s = 32; s > 0; s >>= 1) {
        const uint64_t pc = (uint64_t)__shfl((unsigned long long)p, (int)(l + s));
        if (pc <= i) l += s;
      }
      const uint64_t pl = (uint64_t)__shfl((unsigned long long)p, (int)l);
      if (i < last) start[i] = t0 + ((g * 64 + l) * period) / n_traces + (i - pl) * gap;
    }
  }
}

int ensure_start(anomod_ctx* ctx, anomod_spans* s) {
  if (s->start_us) return ANOMOD_OK;
  void* p = nullptr;
  if (dev_malloc(ctx, &p, (s->n_spans ? s->n_spans : 1) * 8) != hipSuccess) {
    set_error(ctx, "hipMalloc failed for the start column of %llu spans",
              (unsigned long long)s->n_spans);
    return ANOMOD_ENOMEM;
  }
  s->start_us = static_cast<uint64_t*>(p);
  ANOMOD_HIP(ctx, hipMemsetAsync(p, 0, (s->n_spans ? s->n_spans : 1) * 8, ctx->stream));
  return ANOMOD_OK;
}

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_spans_set_start_us(anomod_ctx* ctx, anomod_spans* spans, const uint64_t* start_us) {
  ANOMOD_REQUIRE(nullptr, ctx && spans, "anomod_spans_set_start_us: NULL argument");
  ANOMOD_REQUIRE(ctx, start_us || spans->n_spans == 0, "anomod_spans_set_start_us: NULL column");
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  if (int rc = bind(ctx)) return rc;
  if (int rc = ensure_start(ctx, spans)) return rc;
  if (spans->n_spans) {
    ANOMOD_HIP(ctx, hipMemcpyAsync(spans->start_us, start_us, spans->n_spans * 8,
                                   hipMemcpyHostToDevice, ctx->stream));
    ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ANOMOD_OK;
}

int anomod_spans_has_start_us(const anomod_spans* spans, int* has) {
  ANOMOD_REQUIRE(nullptr, spans && has, "anomod_spans_has_start_us: NULL argument");
  *has = spans->start_us ? 1 : 0;
  return ANOMOD_OK;
}

int anomod_spans_get_start_us(anomod_ctx* ctx, const anomod_spans* spans, uint64_t* dst) {
  ANOMOD_REQUIRE(nullptr, ctx && spans, "anomod_spans_get_start_us: NULL argument");
  ANOMOD_REQUIRE(ctx, dst || spans->n_spans == 0, "anomod_spans_get_start_us: NULL destination");
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  if (!spans->start_us) {
    set_error(ctx, "span set has no start-time column");
    return ANOMOD_ESTATE;
  }
  if (int rc = bind(ctx)) return rc;
  if (spans->n_spans) {
    ANOMOD_HIP(ctx, hipMemcpyAsync(dst, spans->start_us, spans->n_spans * 8,
                                   hipMemcpyDeviceToHost, ctx->stream));
    ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ANOMOD_OK;
}

int anomod_spans_fill_start_synthetic(anomod_ctx* ctx, anomod_spans* spans, uint64_t t0_us,
                                      uint64_t period_us, uint64_t gap_us) {
  ANOMOD_REQUIRE(nullptr, ctx && spans, "anomod_spans_fill_start_synthetic: NULL argument");
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_REQUIRE(ctx, spans->grouped, "span set is not grouped by trace: anomod_spans_group first");
  ANOMOD_REQUIRE(ctx, period_us == 0 || spans->n_traces <= ((1ull << 63) - 1) / period_us,
                 "n_traces * period_us = %llu * %llu is not below 2^63",
                 (unsigned long long)spans->n_traces, (unsigned long long)period_us);
  if (int rc = bind(ctx)) return rc;
  if (int rc = ensure_start(ctx, spans)) return rc;
  if (spans->n_spans && spans->n_traces) {
    const uint64_t groups = (spans->n_traces + 63) / 64;
    const uint64_t grid = std::min<uint64_t>((groups + 3) / 4, (uint64_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(fill_start_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream,
                       spans->trace_ptr, spans->n_traces, t0_us, period_us, gap_us,
                       spans->start_us);
    ANOMOD_HIP(ctx, hipGetLastError());
    ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ANOMOD_OK;
}

int anomod_edge_windows_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_edge_windows* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_edge_windows_spans: NULL argument");
  const uint32_t S = out->n_services, T = out->n_windows;
  uint32_t E = 0;
  uint64_t in_traces[2], n = 0;
  if (int rc = stream_table_args(ctx, S, T, out->step_us, &E)) return rc;
  if (int rc = stream_set_args(ctx, spans, S, true, ANOMOD_EINVAL, in_traces, &n)) return rc;
  const uint64_t TE = (uint64_t)T * E;
  out->outside = 0;
  if (n == 0) {
    if (out->count) memset(out->count, 0, TE * 8);
    if (out->errors) memset(out->errors, 0, TE * 8);
    if (out->sum_us) memset(out->sum_us, 0, TE * 8);
    if (out->max_us) memset(out->max_us, 0, TE * 4);
    return ANOMOD_OK;
  }
  // One workspace: keys | the key walk's words | misc + the requested tables
  // (zeroed together).  The ctx's slot: reused by the next call, not freed.
  const size_t b_keys = Carve::al(n * 8), b_ws = Carve::al(span_edge_keys_ws_bytes(spans));
  const size_t b_u64 = Carve::al(TE * 8), b_u32 = Carve::al(TE * 4);
  const size_t b_tab = 256 + (out->count ? b_u64 : 0) + (out->errors ? b_u64 : 0) +
                       (out->sum_us ? b_u64 : 0) + (out->max_us ? b_u32 : 0);
  char* w = nullptr;
  if (int rc = ensure_scratch(ctx, kScratchEdgeWindows, b_keys + b_ws + b_tab,
                              reinterpret_cast<void**>(&w)))
    return rc;
  Carve cv{w};
  auto* keys = cv.take<unsigned long long>(b_keys);
  auto* ws = cv.take<unsigned long long>(b_ws);
  WinArgs a{};
  a.keys = keys;
  a.misc = cv.take<unsigned long long>(256);
  a.count = cv.take<unsigned long long>(b_u64, out->count);
  a.errors = cv.take<unsigned long long>(b_u64, out->errors);
  a.sum = cv.take<unsigned long long>(b_u64, out->sum_us);
  a.mx = cv.take<unsigned int>(b_u32, out->max_us);
  a.start = spans->start_us;
  a.svcfl = spans->svc_flags;
  a.begin = in_traces[0];
  a.n = n;
  a.t0 = out->t0_us;
  a.step = out->step_us;
  a.T = T;
  a.E = E;
  a.Wt = std::min<uint32_t>(kWinLdsBudget / (E * kCellBytes), T);
  // (tests, A/B: fewer tile windows — 0 = every span to global atomics — and
  // fewer workgroups, so that small sets give a workgroup several batches)
  a.Wt = std::min<uint32_t>(a.Wt, (uint32_t)env_cap("ANOMOD_EDGE_WINDOWS_TILE"));
  const size_t lds = (size_t)a.Wt * E * kCellBytes;
  uint64_t grid = 0;
  if (int rc = stream_geometry(ctx, edge_windows_kernel, kWinThreads, lds, n,
                               "ANOMOD_EDGE_WINDOWS_WGS", &a.per_wg, &grid))
    return rc;
  stream_log("edge_windows_kernel", "keys", a.Wt, nullptr, grid, a.per_wg);
  if (int rc = stage_begin(ctx, kStageEdgeWindows)) return rc;
  ANOMOD_HIP(ctx, hipMemsetAsync(a.misc, 0, b_tab, ctx->stream));
  if (int rc = span_edge_keys(ctx, spans, S, keys, ws)) return rc;
  if (int rc = stage_begin(ctx, kStageEdgeWindowKernel)) return rc;
  hipLaunchKernelGGL(edge_windows_kernel, dim3((unsigned)grid), dim3(kWinThreads), lds,
                     ctx->stream, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeWindowKernel)) return rc;
  if (int rc = stage_end(ctx, kStageEdgeWindows)) return rc;
  ANOMOD_HIP(ctx, stream_back(ctx, out->count, a.count, TE * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->errors, a.errors, TE * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->sum_us, a.sum, TE * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->max_us, a.mx, TE * 4));
  unsigned long long misc[2];
  if (int rc = stream_finish(ctx, a.misc, 1, "edge windows", "key", misc)) return rc;
  out->outside = misc[0];
  return ANOMOD_OK;
}

}  // extern "C"
