// Windowed edge table: per (time window, call-graph edge) count / errors /
// latency sum / max of a grouped span set that carries start times, plus the
// start-time column itself (set / get / synthetic fill).
//
// Two passes.  Pass 1 is the aggregation kernels' own walk in its key form
// (span_edge_keys, edge_agg.hip): keys[i] = edge row << 32 | dur_us by span
// position, so the edge of a span is by construction the row
// anomod_edge_aggregate_spans counts it in.  Pass 2 (edge_windows_kernel) is a
// plain stream over span positions: 20 B read per span (key 8, start 8,
// svc|flags 4), accumulated into cell w * E + edge.  The 16 B / span key round
// trip through HBM is the known cost of not fusing the accumulation into the
// walk.
//
// Pass 2 privatises cells in LDS as a sliding tile of Wt consecutive windows:
// every workgroup owns one contiguous span range, and collector files (and the
// synthetic fill) are close to time-ordered, so a range touches a narrow band
// of windows.  The tile is a ring of Wt window slots x E cells (count | errors
// << 32 as one u64, sum u64, max u32 = 20 B a cell) anchored at the smallest
// window of the current batch; when the stream moves past a window its slot is
// flushed to the global table with integer atomics.  A span whose window falls
// outside the tile goes straight to global atomics, so correctness never
// depends on the hit rate; Wt = 0 (a table too wide for one window slot) is
// the all-global kernel.  A workgroup's range holds < 2^32 spans, so the u32
// halves of the packed count | errors word cannot carry into each other.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

constexpr int kWinThreads = 512;
constexpr int kWinPairs = 2;                            // 16-B (two-span) loads per lane per batch
constexpr int kWinBatch = kWinThreads * kWinPairs * 2;  // spans per workgroup iteration
constexpr uint32_t kWinLdsBudget = 64u * 1024u - 64u;   // two workgroups per CU (+ s_min)
constexpr uint32_t kCellBytes = 20;
constexpr uint64_t kMaxRange = 1ull << 31;              // spans per workgroup (u32 LDS counts)
constexpr uint32_t kNoWindow = 0xFFFFFFFFu;

using u64x2 = unsigned long long __attribute__((ext_vector_type(2)));
using u32x2 = uint32_t __attribute__((ext_vector_type(2)));

struct WinArgs {
  const unsigned long long* keys;   // [n] edge << 32 | dur
  const uint64_t* start;            // [n]
  const uint32_t* svcfl;            // [n] svc | flags << 16
  uint64_t begin, n, per_wg;        // spans [begin, n) lie in traces; per_wg: a multiple of kWinBatch
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
  const uint32_t E = a.E, Wt = a.Wt;
  const uint32_t cells = Wt * E;
  auto* l_ce = reinterpret_cast<unsigned long long*>(win_lds);  // count | errors << 32
  auto* l_sum = l_ce + cells;
  auto* l_mx = reinterpret_cast<unsigned int*>(l_sum + cells);
  __shared__ uint32_t s_min[3];
  const uint32_t tid = threadIdx.x;
  for (uint32_t c = tid; c < cells; c += kWinThreads) {
    l_ce[c] = 0ull;
    l_sum[c] = 0ull;
    l_mx[c] = 0u;
  }
  if (tid < 3) s_min[tid] = kNoWindow;
  __syncthreads();

  // window `w` of the tile [base, base + Wt) lives in slot (slot0 + w - base) mod Wt
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

  const uint64_t lo = (uint64_t)blockIdx.x * a.per_wg;
  const uint64_t hi = lo + a.per_wg < a.n ? lo + a.per_wg : a.n;
  bool anchored = false;
  uint32_t base = 0, slot0 = 0;
  uint32_t outside = 0, bad = 0;
  uint32_t it = 0;
  for (uint64_t b = lo; b < hi; b += kWinBatch, ++it) {
    unsigned long long key[kWinPairs * 2];
    uint64_t st[kWinPairs * 2];
    uint32_t sf[kWinPairs * 2];
    bool live[kWinPairs * 2];
    if (b + kWinBatch <= hi) {  // (b is a multiple of kWinBatch: 16-B aligned pairs)
#pragma unroll
      for (int j = 0; j < kWinPairs; ++j) {
        const uint64_t i = b + ((uint64_t)j * kWinThreads + tid) * 2;
        const u64x2 k = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.keys + i));
        const u64x2 s = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.start + i));
        const u32x2 f = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(a.svcfl + i));
        key[2 * j] = k.x, key[2 * j + 1] = k.y;
        st[2 * j] = s.x, st[2 * j + 1] = s.y;
        sf[2 * j] = f.x, sf[2 * j + 1] = f.y;
        live[2 * j] = i >= a.begin;
        live[2 * j + 1] = i + 1 >= a.begin;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kWinPairs * 2; ++j) {
        const uint64_t i = b + ((uint64_t)(j >> 1) * kWinThreads + tid) * 2 + (j & 1);
        live[j] = i < hi && i >= a.begin;
        key[j] = live[j] ? a.keys[i] : 0ull;
        st[j] = live[j] ? a.start[i] : 0ull;
        sf[j] = live[j] ? a.svcfl[i] : 0u;
      }
    }
    uint32_t w[kWinPairs * 2];
    uint32_t lmin = kNoWindow;
#pragma unroll
    for (int j = 0; j < kWinPairs * 2; ++j) {
      w[j] = kNoWindow;
      if (!live[j]) continue;
      if ((uint32_t)(key[j] >> 32) >= E) {  // never for keys of span_edge_keys
        ++bad;
        continue;
      }
      // start < t0 first (unsigned), then w against T: t0 + T * step may pass 2^64
      const uint64_t q = st[j] >= a.t0 ? (st[j] - a.t0) / a.step : (uint64_t)a.T;
      if (q >= (uint64_t)a.T) {
        ++outside;
        continue;
      }
      w[j] = (uint32_t)q;
      lmin = lmin < w[j] ? lmin : w[j];
    }
    if (Wt) {  // (uniform) move the tile's anchor to the batch's smallest window
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)lmin, o);
        lmin = lmin < other ? lmin : other;
      }
      if ((tid & 63u) == 0 && lmin != kNoWindow) atomicMin(&s_min[it % 3u], lmin);
      __syncthreads();  // also: the previous batch's LDS atomics have landed
      const uint32_t bmin = s_min[it % 3u];
      if (tid == 0) s_min[(it + 2u) % 3u] = kNoWindow;  // read last in batch it - 1
      if (bmin != kNoWindow) {
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
    for (int j = 0; j < kWinPairs * 2; ++j) {
      if (w[j] == kNoWindow) continue;
      const uint32_t edge = (uint32_t)(key[j] >> 32), dur = (uint32_t)key[j];
      const uint32_t err = (sf[j] >> 16) & ANOMOD_FLAG_ERROR;
      if (anchored && w[j] >= base && w[j] - base < Wt) {
        uint32_t s = slot0 + (w[j] - base);
        s = s >= Wt ? s - Wt : s;
        const uint32_t c = s * E + edge;
        atomicAdd(&l_ce[c], 1ull | ((unsigned long long)err << 32));
        if (dur) {
          atomicAdd(&l_sum[c], (unsigned long long)dur);
          atomicMax(&l_mx[c], dur);
        }
      } else {
        cell_global(a, (uint64_t)w[j] * E + edge, 1u, err, dur, dur);
      }
    }
  }
  if (Wt) {
    __syncthreads();
    if (anchored)
      for (uint32_t k = 0; k < Wt && (uint64_t)base + k < a.T; ++k) {
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

// Value of a numeric environment cap, "no cap" when unset or not a number;
// ANOMOD_EDGE_WINDOWS_WGS must be at least 1.
uint64_t env_cap(const char* name) {
  const char* e = getenv(name);
  if (!e || !*e) return 0xFFFFFFFFull;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  if (*end) return 0xFFFFFFFFull;
  return !strcmp(name, "ANOMOD_EDGE_WINDOWS_WGS") && v == 0 ? 1 : (uint64_t)v;
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
  // the spans that lie in traces (an upload may leave spans outside every
  // trace: the aggregation counts none of them)
  uint64_t in_traces[2];
  if (spans->n_traces && spans->n_spans)
    if (int rc = bind(ctx)) return rc;
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  const uint64_t n = in_traces[1] > in_traces[0] ? in_traces[1] : 0;
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
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t b_keys = al(n * 8), b_ws = al(span_edge_keys_ws_bytes(spans));
  const size_t b_u64 = al(TE * 8), b_u32 = al(TE * 4);
  const size_t b_tab = 256 + (out->count ? b_u64 : 0) + (out->errors ? b_u64 : 0) +
                       (out->sum_us ? b_u64 : 0) + (out->max_us ? b_u32 : 0);
  char* w = nullptr;
  if (int rc = ensure_scratch(ctx, kScratchEdgeWindows, b_keys + b_ws + b_tab,
                              reinterpret_cast<void**>(&w)))
    return rc;
  WinArgs a{};
  a.keys = reinterpret_cast<unsigned long long*>(w);
  auto* ws = reinterpret_cast<unsigned long long*>(w + b_keys);
  char* t = w + b_keys + b_ws;
  a.misc = reinterpret_cast<unsigned long long*>(t);
  t += 256;
  auto take = [&](bool want, size_t bytes) -> char* {
    char* p = want ? t : nullptr;
    if (want) t += bytes;
    return p;
  };
  a.count = reinterpret_cast<unsigned long long*>(take(out->count, b_u64));
  a.errors = reinterpret_cast<unsigned long long*>(take(out->errors, b_u64));
  a.sum = reinterpret_cast<unsigned long long*>(take(out->sum_us, b_u64));
  a.mx = reinterpret_cast<unsigned int*>(take(out->max_us, b_u32));
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
  int per_cu = 0;
  ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void*>(edge_windows_kernel), kWinThreads,
                      lds));
  // persistent workgroups, one contiguous range of whole batches each
  const uint64_t batches = (n + kWinBatch - 1) / kWinBatch;
  uint64_t grid = std::min<uint64_t>((uint64_t)ctx->num_cus * (per_cu > 0 ? per_cu : 1), batches);
  grid = std::min<uint64_t>(grid, env_cap("ANOMOD_EDGE_WINDOWS_WGS"));
  a.per_wg = (batches + grid - 1) / grid * kWinBatch;
  if (a.per_wg > kMaxRange) a.per_wg = kMaxRange;  // (more workgroups than are resident)
  grid = (n + a.per_wg - 1) / a.per_wg;
  if (int rc = stage_begin(ctx, kStageEdgeWindows)) return rc;
  ANOMOD_HIP(ctx, hipMemsetAsync(a.misc, 0, b_tab, ctx->stream));
  if (int rc = span_edge_keys(ctx, spans, S, const_cast<unsigned long long*>(a.keys), ws))
    return rc;
  if (int rc = stage_begin(ctx, kStageEdgeWindowKernel)) return rc;
  hipLaunchKernelGGL(edge_windows_kernel, dim3((unsigned)grid), dim3(kWinThreads), lds,
                     ctx->stream, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeWindowKernel)) return rc;
  if (int rc = stage_end(ctx, kStageEdgeWindows)) return rc;
  unsigned long long misc[2] = {0ull, 0ull};
  ANOMOD_HIP(ctx, hipMemcpyAsync(misc, a.misc, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (out->count)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->count, a.count, TE * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out->errors)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->errors, a.errors, TE * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
  if (out->sum_us)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->sum_us, a.sum, TE * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (out->max_us)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->max_us, a.mx, TE * 4, hipMemcpyDeviceToHost, ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (misc[1]) {
    set_error(ctx, "edge windows: %llu spans carry no edge key (internal error)", misc[1]);
    return ANOMOD_ESTATE;
  }
  out->outside = misc[0];
  return ANOMOD_OK;
}

}  // extern "C"
