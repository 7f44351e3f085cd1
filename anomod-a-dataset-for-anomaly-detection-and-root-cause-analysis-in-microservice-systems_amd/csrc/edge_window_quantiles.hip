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
// edge_windows_kernel (window_of, edge_stream.h): the keys form of the shared
// edge stream, 16 B read (key 8, start 8) and 8 B written per span.  A span in no cell — outside [0, T), before trace_ptr[0], or with
// a key that names no row — takes the sentinel cell T * E, which sorts behind
// every real cell.  One radix sort (radix.hip) over bits [0, 32 + bits(T * E))
// orders the spans by (cell, latency); window_cell_bounds_kernel streams the
// sorted keys once (8 B per span) and writes where each cell begins and ends;
// window_pick_kernel reads the picks.  Every value is an integer: results are
// bit-exact for any launch geometry.
#include <algorithm>
#include <cstring>

#include "edge_stream.h"
#include "radix.h"

namespace anomod {
namespace {

constexpr int kCellThreads = 256;
constexpr uint32_t kMaxQ = 8;
using CellLanes = stream::Lanes<kCellThreads, 2>;  // 1024 spans per workgroup iteration

struct CellArgs {
  unsigned long long* keys;  // [n] in: edge << 32 | dur; out: cell << 32 | dur
  const uint64_t* start;     // [n]
  uint64_t begin, n, per_wg; // spans [begin, n) lie in traces; per_wg: a multiple of the batch
  uint64_t t0, step;
  uint32_t T, E, TE;
  unsigned long long* misc;  // [0] outside, [1] spans whose key names no edge row
};

// (no __restrict__: keys is read and written, each position by one lane)
__global__ __launch_bounds__(kCellThreads) void window_cell_keys_kernel(CellArgs a) {
  const uint32_t tid = threadIdx.x;
  uint64_t lo, hi;
  stream::wg_range(a.per_wg, a.n, &lo, &hi);
  const unsigned long long none = (unsigned long long)a.TE << 32;
  uint32_t outside = 0, bad = 0;
  for (uint64_t b = lo; b < hi; b += CellLanes::kBatch) {
    CellLanes L(b, hi, a.begin, tid);
    unsigned long long key[4];
    uint64_t st[4];
    L.load(a.keys, key, a.start, st);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t row = (uint32_t)(key[j] >> 32), dur = (uint32_t)key[j];
      key[j] = none;
      if (!L.live[j]) continue;
      key[j] |= dur;
      if (row >= a.E) {  // never for keys of span_edge_keys
        ++bad;
      } else if (const uint32_t w = stream::window_of(st[j], a.t0, a.step, a.T);
                 w == stream::kNone) {
        ++outside;
      } else {
        key[j] = (unsigned long long)(w * a.E + row) << 32 | dur;
      }
    }
    L.store(a.keys, key);
  }
  stream::count_add(a.misc, outside, tid);
  stream::count_add(a.misc + 1, bad, tid);
}

// Where each cell's run of the sorted keys begins and ends.  Position i opens
// its cell and closes that of position i - 1 when the two differ; position 0
// opens its cell, position m - 1 closes its cell.  The tables arrive zeroed,
// so a cell no span fell in reads begin = end = 0; the sentinel cell T * E has
// no entry.  m <= 2^32 - 4097: positions are u32.
struct BoundArgs {
  const unsigned long long* sk;  // [m] sorted cell << 32 | dur
  uint64_t m, per_wg;            // per_wg: a multiple of the batch
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
  uint64_t lo, hi;
  stream::wg_range(a.per_wg, a.m, &lo, &hi);
  for (uint64_t b = lo; b < hi; b += CellLanes::kBatch) {
    CellLanes L(b, hi, 0, tid);
    unsigned long long k[4];
    L.load(a.sk, k);
    if (L.full) {
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const uint64_t i = L.pos(j);
        const uint32_t c0 = (uint32_t)(k[j] >> 32), c1 = (uint32_t)(k[j + 1] >> 32);
        // the cell of position i - 1: the lane below holds it, except at a
        // wave's first lane (the wave, workgroup or range before this one)
        uint32_t prev = (uint32_t)__shfl_up((int)c1, 1);
        if ((tid & 63u) == 0 && i > 0) prev = (uint32_t)(a.sk[i - 1] >> 32);
        cell_edge(a, i, c0, prev, i == 0);
        cell_edge(a, i + 1, c1, c0, false);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t i = L.pos(j);
        if (!L.live[j]) continue;
        const uint32_t prev = i > 0 ? (uint32_t)(a.sk[i - 1] >> 32) : 0u;
        cell_edge(a, i, (uint32_t)(k[j] >> 32), prev, i == 0);
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

// Geometry of the two stream kernels: eight workgroups a CU, capped by
// ANOMOD_EDGE_WINDOW_QUANTILES_WGS (tests: one workgroup over the whole set,
// many small ones), no range clamp (positions are u64 throughout).
uint64_t cell_grid(const anomod_ctx* ctx, uint64_t n, uint64_t* per_wg) {
  return stream_grid(ctx, n, CellLanes::kBatch, 8, env_cap("ANOMOD_EDGE_WINDOW_QUANTILES_WGS", 1),
                     ~0ull, per_wg);
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
  uint32_t E = 0;
  if (int rc = stream_table_args(ctx, S, T, out->step_us, &E)) return rc;
  ANOMOD_REQUIRE(ctx, nq >= 1 && nq <= kMaxQ, "nq=%u outside [1, %u]", nq, kMaxQ);
  ANOMOD_REQUIRE(ctx, out->q_pct && out->q_us, "anomod_edge_window_quantiles: NULL q_pct or q_us");
  for (uint32_t k = 0; k < nq; ++k)
    ANOMOD_REQUIRE(ctx, out->q_pct[k] <= 99, "q_pct[%u]=%u outside [0, 99]", k, out->q_pct[k]);
  uint64_t in_traces[2], n = 0;
  if (int rc = stream_set_args(ctx, spans, S, true, ANOMOD_ESTATE, in_traces, &n)) return rc;
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
  uint64_t grid = cell_grid(ctx, n, &a.per_wg);
  stream_log("window_cell_keys_kernel", "keys", -1, nullptr, grid, a.per_wg);
  hipLaunchKernelGGL(window_cell_keys_kernel, dim3((unsigned)grid), dim3(kCellThreads), 0,
                     ctx->stream, a);
  ANOMOD_HIP(ctx, hipGetLastError());

  int passes = 0;
  ANOMOD_HIP(ctx, radix_sort_u64(reinterpret_cast<const uint64_t*>(keys + in_traces[0]),
                                 reinterpret_cast<uint64_t*>(sorted), m, 0, 32 + cbits, tmp,
                                 sort_tmp, ctx->stream, &passes));
  if (log_kernel())  // (tests, timing)
    fprintf(stderr, "anomod: edge window quantiles: %llu keys of %d bits, %d sort passes\n",
            (unsigned long long)m, 32 + cbits, passes);

  BoundArgs ba{};
  ba.sk = sorted;
  ba.m = m;
  ba.TE = TE;
  ba.cbegin = cbegin;
  ba.cend = cend;
  grid = cell_grid(ctx, m, &ba.per_wg);
  stream_log("window_cell_bounds_kernel", "keys", -1, nullptr, grid, ba.per_wg);
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

  ANOMOD_HIP(ctx, stream_back(ctx, out->count, d_cnt, (size_t)TE * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->q_us, d_q, picks * 4));
  unsigned long long misc[2];
  if (int rc = stream_finish(ctx, misc_d, 1, "edge window quantiles", "key", misc)) return rc;
  out->outside = misc[0];
  return ANOMOD_OK;
}

}  // extern "C"
