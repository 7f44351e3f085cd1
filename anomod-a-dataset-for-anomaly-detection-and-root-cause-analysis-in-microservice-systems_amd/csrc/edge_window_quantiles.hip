// Per-window edge latency quantiles: for every (time window, call-graph edge)
// cell of a grouped span set that carries start times, the span count and the
// exact nearest-rank order statistics x[int(c * q)] of the cell's sorted
// latencies (the index rule of exact_pick_kernel, edge_agg.hip).
//
// Pass 1 is the aggregation kernels' own walk in its key form (span_edge_keys,
// edge_agg.hip): keys[i] = edge row << 32 | dur_us by span position, so a
// span's row is by construction the one anomod_edge_aggregate_spans counts it
// in.  window_cell_keys_kernel then widens the key in place to
// cell << 32 | dur_us with cell = w * E + row and w the window rule of
// edge_windows_kernel (start < t0 first, then (start - t0) / step against T):
// a stream over span positions, 16 B read (key 8, start 8) and 8 B written
// per span.  A span in no cell — outside [0, T), before trace_ptr[0], or with
// a key that names no row — takes the sentinel cell T * E, which sorts behind
// every real cell.  One radix sort (radix.hip) over bits [0, 32 + bits(T * E))
// orders the spans by (cell, latency); window_cell_bounds_kernel streams the
// sorted keys once (8 B per span) and writes where each cell begins and ends;
// window_pick_kernel reads the picks.  Every value is an integer: results are
// bit-exact for any launch geometry.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "radix.h"
#include "walk.h"

namespace anomod {
namespace {

constexpr int kCellThreads = 256;
constexpr int kCellPairs = 2;                              // 16-B (two-span) loads per lane per batch
constexpr int kCellBatch = kCellThreads * kCellPairs * 2;  // spans per workgroup iteration
constexpr uint32_t kMaxQ = 8;

using u64x2 = unsigned long long __attribute__((ext_vector_type(2)));

struct CellArgs {
  unsigned long long* keys;  // [n] in: edge << 32 | dur; out: cell << 32 | dur
  const uint64_t* start;     // [n]
  uint64_t begin, n, per_wg; // spans [begin, n) lie in traces; per_wg: a multiple of kCellBatch
  uint64_t t0, step;
  uint32_t T, E, TE;
  unsigned long long* misc;  // [0] outside, [1] spans whose key names no edge row
};

// (no __restrict__: keys is read and written, each position by one lane)
__global__ __launch_bounds__(kCellThreads) void window_cell_keys_kernel(CellArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint64_t lo = (uint64_t)blockIdx.x * a.per_wg;
  const uint64_t hi = lo + a.per_wg < a.n ? lo + a.per_wg : a.n;
  const unsigned long long none = (unsigned long long)a.TE << 32;
  uint32_t outside = 0, bad = 0;
  auto widen = [&](unsigned long long key, uint64_t st, bool live) -> unsigned long long {
    const uint32_t dur = (uint32_t)key;
    if (!live) return none;
    if ((uint32_t)(key >> 32) >= a.E) {  // never for keys of span_edge_keys
      ++bad;
      return none | dur;
    }
    // start < t0 first (unsigned), then w against T: t0 + T * step may pass 2^64
    const uint64_t w = st >= a.t0 ? (st - a.t0) / a.step : (uint64_t)a.T;
    if (w >= (uint64_t)a.T) {
      ++outside;
      return none | dur;
    }
    const uint32_t cell = (uint32_t)w * a.E + (uint32_t)(key >> 32);
    return (unsigned long long)cell << 32 | dur;
  };
  for (uint64_t b = lo; b < hi; b += kCellBatch) {
    if (b + kCellBatch <= hi) {  // (b is a multiple of kCellBatch: 16-B aligned pairs)
      u64x2 k[kCellPairs], s[kCellPairs];
#pragma unroll
      for (int j = 0; j < kCellPairs; ++j) {
        const uint64_t i = b + ((uint64_t)j * kCellThreads + tid) * 2;
        k[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.keys + i));
        s[j] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.start + i));
      }
#pragma unroll
      for (int j = 0; j < kCellPairs; ++j) {
        const uint64_t i = b + ((uint64_t)j * kCellThreads + tid) * 2;
        u64x2 o;
        o.x = widen(k[j].x, s[j].x, i >= a.begin);
        o.y = widen(k[j].y, s[j].y, i + 1 >= a.begin);
        *reinterpret_cast<u64x2*>(a.keys + i) = o;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kCellPairs * 2; ++j) {
        const uint64_t i = b + ((uint64_t)(j >> 1) * kCellThreads + tid) * 2 + (j & 1);
        if (i >= hi) continue;
        const bool live = i >= a.begin;
        a.keys[i] = widen(live ? a.keys[i] : 0ull, live ? a.start[i] : 0ull, live);
      }
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

// Where each cell's run of the sorted keys begins and ends.  Position i opens
// its cell and closes that of position i - 1 when the two differ; position 0
// opens its cell, position m - 1 closes its cell.  The tables arrive zeroed,
// so a cell no span fell in reads begin = end = 0; the sentinel cell T * E has
// no entry.  m <= 2^32 - 4097: positions are u32.
struct BoundArgs {
  const unsigned long long* sk;  // [m] sorted cell << 32 | dur
  uint64_t m, per_wg;            // per_wg: a multiple of kCellBatch
  uint32_t TE;
  uint32_t* cbegin;              // [TE]
  uint32_t* cend;                // [TE]
};

__device__ inline void cell_edge(const BoundArgs& a, uint64_t i, uint32_t cur, uint32_t prev,
                                 bool first) {
  if (first || cur != prev) {
    if (!first && prev < a.TE) a.cend[prev] = (uint32_t)i;
    if (cur < a.TE) a.cbegin[cur] = (uint32_t)i;
  }
  if (i + 1 == a.m && cur < a.TE) a.cend[cur] = (uint32_t)a.m;
}

__global__ __launch_bounds__(kCellThreads) void window_cell_bounds_kernel(BoundArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint64_t lo = (uint64_t)blockIdx.x * a.per_wg;
  const uint64_t hi = lo + a.per_wg < a.m ? lo + a.per_wg : a.m;
  for (uint64_t b = lo; b < hi; b += kCellBatch) {
    if (b + kCellBatch <= hi) {  // (b is a multiple of kCellBatch: 16-B aligned pairs)
#pragma unroll
      for (int j = 0; j < kCellPairs; ++j) {
        const uint64_t i = b + ((uint64_t)j * kCellThreads + tid) * 2;
        const u64x2 k = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.sk + i));
        const uint32_t c0 = (uint32_t)(k.x >> 32), c1 = (uint32_t)(k.y >> 32);
        // the cell of position i - 1: the lane below holds it, except at a
        // wave's first lane (the wave, workgroup or range before this one)
        uint32_t prev = (uint32_t)__shfl_up((int)c1, 1);
        if ((tid & 63u) == 0 && i > 0) prev = (uint32_t)(a.sk[i - 1] >> 32);
        cell_edge(a, i, c0, prev, i == 0);
        cell_edge(a, i + 1, c1, c0, false);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kCellPairs * 2; ++j) {
        const uint64_t i = b + ((uint64_t)(j >> 1) * kCellThreads + tid) * 2 + (j & 1);
        if (i >= hi) continue;
        const uint32_t cur = (uint32_t)(a.sk[i] >> 32);
        const uint32_t prev = i > 0 ? (uint32_t)(a.sk[i - 1] >> 32) : 0u;
        cell_edge(a, i, cur, prev, i == 0);
      }
    }
  }
}

// One thread per (cell, pick): consecutive threads store consecutive q_us
// words; the thread of a cell's first pick stores its count.  The index is
// the reference's int(c * q) with q = q_pct / 100 as a double and the product
// truncated (exact_pick_kernel, edge_agg.hip).
struct PickArgs {
  const unsigned long long* sk;
  const uint32_t* cbegin;
  const uint32_t* cend;
  uint32_t TE, nq;
  uint32_t q_pct[kMaxQ];
  unsigned long long* count;  // [TE] or NULL
  uint32_t* q_us;             // [TE * nq]
};

__global__ __launch_bounds__(256) void window_pick_kernel(PickArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= (uint64_t)a.TE * a.nq) return;
  const uint32_t cell = (uint32_t)(t / a.nq), k = (uint32_t)(t % a.nq);
  const uint32_t b = a.cbegin[cell];
  const uint32_t c = a.cend[cell] - b;
  if (k == 0 && a.count) a.count[cell] = c;
  uint32_t q = 0;  // (a select chain: no runtime-indexed array of the argument block)
#pragma unroll
  for (uint32_t j = 0; j < kMaxQ; ++j) q = j == k ? a.q_pct[j] : q;
  a.q_us[t] = c ? (uint32_t)a.sk[(uint64_t)b + (uint64_t)((double)c * ((double)q / 100.0))] : 0u;
}

// Workgroup cap of the two stream kernels (tests: one workgroup over the whole
// set, many small ones); "no cap" when unset or not a number, at least 1.
uint64_t wgs_cap() {
  const char* e = getenv("ANOMOD_EDGE_WINDOW_QUANTILES_WGS");
  if (!e || !*e) return 0xFFFFFFFFull;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  if (*end) return 0xFFFFFFFFull;
  return v == 0 ? 1 : (uint64_t)v;
}

// Persistent workgroups over n positions, one contiguous range of whole
// batches each: *per_wg spans a workgroup, the grid as the return value.
uint64_t stream_grid(const anomod_ctx* ctx, uint64_t n, uint64_t* per_wg) {
  const uint64_t batches = (n + kCellBatch - 1) / kCellBatch;
  uint64_t grid = std::min<uint64_t>((uint64_t)ctx->num_cus * 8, batches);
  grid = std::min<uint64_t>(grid, wgs_cap());
  *per_wg = (batches + grid - 1) / grid * kCellBatch;
  return (n + *per_wg - 1) / *per_wg;
}

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_edge_window_quantiles_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                       anomod_edge_window_quantiles* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out,
                 "anomod_edge_window_quantiles_spans: NULL argument");
  const uint32_t S = out->n_services, T = out->n_windows, nq = out->nq;
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  ANOMOD_REQUIRE(ctx, T >= 1 && T <= 65536, "n_windows=%u outside [1, 65536]", T);
  ANOMOD_REQUIRE(ctx, (uint64_t)T * E <= (1ull << 24), "n_windows * edge rows = %u * %u > 2^24", T,
                 E);
  ANOMOD_REQUIRE(ctx, out->step_us >= 1, "step_us must be at least 1");
  ANOMOD_REQUIRE(ctx, nq >= 1 && nq <= kMaxQ, "nq=%u outside [1, %u]", nq, kMaxQ);
  ANOMOD_REQUIRE(ctx, out->q_pct && out->q_us, "anomod_edge_window_quantiles: NULL q_pct or q_us");
  for (uint32_t k = 0; k < nq; ++k)
    ANOMOD_REQUIRE(ctx, out->q_pct[k] <= 99, "q_pct[%u]=%u outside [0, 99]", k, out->q_pct[k]);
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  if (!spans->grouped) {
    set_error(ctx, "span set is not grouped by trace: anomod_spans_group first");
    return ANOMOD_ESTATE;
  }
  if (!spans->start_us) {
    set_error(ctx, "span set has no start-time column: anomod_spans_set_start_us first");
    return ANOMOD_ESTATE;
  }
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "span service index %u >= n_services %u", spans->max_svc, S);
  // the spans that lie in traces
  uint64_t in_traces[2];
  if (spans->n_traces && spans->n_spans)
    if (int rc = bind(ctx)) return rc;
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  const uint64_t n = in_traces[1] > in_traces[0] ? in_traces[1] : 0;
  const uint64_t m = n ? n - in_traces[0] : 0;  // the spans that are sorted
  // one radix sort over the in-trace spans' keys (u32 tile offsets inside)
  ANOMOD_REQUIRE(ctx, m <= kMaxSortKeys,
                 "edge window quantiles: %llu spans in traces, at most 2^32 - 4097 per call",
                 (unsigned long long)m);
  const uint32_t TE = T * E;
  out->outside = 0;
  if (n == 0) {
    if (out->count) memset(out->count, 0, (size_t)TE * 8);
    memset(out->q_us, 0, (size_t)TE * nq * 4);
    return ANOMOD_OK;
  }
  int cbits = 1;  // the sentinel cell T * E is a key too
  while ((uint64_t)TE >> cbits) ++cbits;
  // The call's workspace (freed when the call returns, after the stream's
  // work): keys (widened in place) | sorted keys | sort temp | the key walk's
  // words | misc + cell begins + cell ends (zeroed together) | count | q_us.
  CallWorkspace wsp{ctx};
  const auto al = CallWorkspace::al;
  const size_t sort_tmp = radix_temp_bytes(m);
  const size_t b_keys = al(n * 8), b_sorted = al(m * 8), b_tmp = al(sort_tmp),
               b_ws = al(span_edge_keys_ws_bytes(spans)), b_u32 = al((size_t)TE * 4),
               b_cnt = out->count ? al((size_t)TE * 8) : 0, b_q = al((size_t)TE * nq * 4);
  const size_t b_zero = 256 + 2 * b_u32;
  const size_t total = b_keys + b_sorted + b_tmp + b_ws + b_zero + b_cnt + b_q;
  if (int rc = wsp.take(&wsp.block, total, "edge-window-quantile")) return rc;
  auto* keys = wsp.carve<unsigned long long>(b_keys);
  auto* sorted = wsp.carve<unsigned long long>(b_sorted);
  void* tmp = wsp.carve(b_tmp);
  auto* walk = wsp.carve<unsigned long long>(b_ws);
  auto* misc_d = wsp.carve<unsigned long long>(256);
  auto* cbegin = wsp.carve<uint32_t>(b_u32);
  auto* cend = wsp.carve<uint32_t>(b_u32);
  auto* d_cnt = out->count ? wsp.carve<unsigned long long>(b_cnt) : nullptr;
  auto* d_q = wsp.carve<uint32_t>(b_q);

  ANOMOD_HIP(ctx, hipMemsetAsync(misc_d, 0, b_zero, ctx->stream));
  if (int rc = span_edge_keys(ctx, spans, S, keys, walk)) return rc;

  CellArgs a{};
  a.keys = keys;
  a.start = spans->start_us;
  a.begin = in_traces[0];
  a.n = n;
  a.t0 = out->t0_us;
  a.step = out->step_us;
  a.T = T;
  a.E = E;
  a.TE = TE;
  a.misc = misc_d;
  uint64_t grid = stream_grid(ctx, n, &a.per_wg);
  hipLaunchKernelGGL(window_cell_keys_kernel, dim3((unsigned)grid), dim3(kCellThreads), 0,
                     ctx->stream, a);
  ANOMOD_HIP(ctx, hipGetLastError());

  int passes = 0;
  ANOMOD_HIP(ctx, radix_sort_u64(reinterpret_cast<const uint64_t*>(keys + in_traces[0]),
                                 reinterpret_cast<uint64_t*>(sorted), m, 0, 32 + cbits, tmp,
                                 sort_tmp, ctx->stream, &passes));
  if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests, timing)
    fprintf(stderr, "anomod: edge window quantiles: %llu keys of %d bits, %d sort passes\n",
            (unsigned long long)m, 32 + cbits, passes);

  BoundArgs ba{};
  ba.sk = sorted;
  ba.m = m;
  ba.TE = TE;
  ba.cbegin = cbegin;
  ba.cend = cend;
  grid = stream_grid(ctx, m, &ba.per_wg);
  hipLaunchKernelGGL(window_cell_bounds_kernel, dim3((unsigned)grid), dim3(kCellThreads), 0,
                     ctx->stream, ba);
  ANOMOD_HIP(ctx, hipGetLastError());

  PickArgs pa{};
  pa.sk = sorted;
  pa.cbegin = cbegin;
  pa.cend = cend;
  pa.TE = TE;
  pa.nq = nq;
  for (uint32_t k = 0; k < nq; ++k) pa.q_pct[k] = out->q_pct[k];
  pa.count = d_cnt;
  pa.q_us = d_q;
  const uint64_t picks = (uint64_t)TE * nq;
  hipLaunchKernelGGL(window_pick_kernel, dim3((unsigned)((picks + 255) / 256)), dim3(256), 0,
                     ctx->stream, pa);
  ANOMOD_HIP(ctx, hipGetLastError());

  unsigned long long misc[2] = {0ull, 0ull};
  ANOMOD_HIP(ctx, hipMemcpyAsync(misc, misc_d, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (out->count)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->count, d_cnt, (size_t)TE * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
  ANOMOD_HIP(ctx, hipMemcpyAsync(out->q_us, d_q, picks * 4, hipMemcpyDeviceToHost, ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (misc[1]) {
    set_error(ctx, "edge window quantiles: %llu spans carry no edge key (internal error)", misc[1]);
    return ANOMOD_ESTATE;
  }
  out->outside = misc[0];
  return ANOMOD_OK;
}

}  // extern "C"
