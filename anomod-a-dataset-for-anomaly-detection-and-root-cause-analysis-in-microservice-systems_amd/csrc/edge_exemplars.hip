// Edge exemplars: for every call-graph edge row the K slowest calls of a
// grouped span set (all spans, or those with ANOMOD_FLAG_ERROR), ordered by
// dur_us descending, then span position ascending — the calls behind an edge
// table's tail, to be carried back to their traces.
//
// Every span in traces gets the key
//   dur_us << 32 | (0xFFFFFFFF - (position - trace_ptr[0]))
// unique per span, >= 1 (at most 2^32 - 2 spans a call), and its unsigned order
// is the contract's order.  A row's list is K u64 slots, 0 = empty, and the
// insertion of x is a cascade over the slots i = 0 .. K-1:
//   old = atomicMax(&a[i], x);  if (old < x) x = old;  stop when x == 0
// Slot values only grow, and a value sits at or passes slot i only after it
// found every slot j < i holding something larger; so whatever falls off slot
// K-1 is smaller than all K final values, and the final list is the top K in
// descending order under any interleaving of the atomics.  Two shortcuts, both
// exact for the same reason (a slot never shrinks):
//   - a slot whose plain read already shows a larger value may be passed
//     without the atomic (the atomic would have returned that or more and
//     changed nothing; a stale read only means the atomic is done after all:
//     the global lists do that at every slot), and since a list is descending
//     at every instant the first slot to look at is found by binary search;
//   - whatever a[K-1] held at any time is a lower bound of every final slot,
//     so a span whose key is below a read of it — however stale — is skipped
//     after that one read: in steady state almost every span.
//
// edge_exemplars_kernel is the shared edge stream (edge_stream.h) in both of
// its forms: rows (row 2 B, svc|flags 4 B, dur 4 B = 10 B/span in one pass) and
// keys (key 8 B after span_edge_keys, + svc|flags 4 B when only error spans are
// wanted: the key carries no error bit), and two placements of the lists,
// picked on the host from E * K * 8:
//   lds     workgroup-private lists in LDS; at the end the workgroup pushes
//           each non-empty entry through the same cascade on the global lists
//   global  the cascade runs on the global lists (they stay in L2); the
//           threshold a[K-1] is read through an LDS cache of one u64 per row
//           when E * 8 fits (a stale cached threshold is still a lower bound),
//           else from the global slot
// edge_exemplars_gather_kernel, one thread per (row, slot), decodes the key to
// a position, looks the span's columns up, finds its trace by binary search in
// trace_ptr and writes the output columns.
#include <algorithm>
#include <cstring>

#include "edge_stream.h"

namespace anomod {
namespace {

constexpr int kExThreads = 512;                       // 2048 spans per workgroup iteration
constexpr uint32_t kExLdsBudget = 40u * 1024u - 64u;  // four workgroups per CU
constexpr uint64_t kExMaxSpans = 0xFFFFFFFEull;       // spans in traces per call
constexpr int kGatherThreads = 256;

enum { kSrcRows = 0, kSrcKeys = 1 };
enum { kListsGlobal = 0, kListsGlobalCached = 1, kListsLds = 2 };

struct ExArgs {
  const unsigned long long* keys;  // keys form: [n] edge << 32 | dur
  const uint16_t* rows;            // rows form: [n] parent rows
  const uint32_t* svcfl;           // [n] svc | flags << 16 (rows form; keys form when errors)
  const uint32_t* dur;             // rows form: [n]
  uint64_t begin, n, per_wg;       // spans [begin, n) lie in traces; per_wg: a multiple of the batch
  uint32_t E, K;
  uint32_t S, S0;                  // rows form: the call's S, the S the rows were written with
  uint32_t errors;                 // 1: only spans with ANOMOD_FLAG_ERROR
  uint32_t place;                  // kLists*
  unsigned long long* lists;       // [E * K] zeroed
  unsigned long long* misc;        // [0] spans that name no edge row, [1] gather mismatches
};

extern __shared__ __align__(16) unsigned char ex_lds[];

template <int SCOPE>
__device__ __forceinline__ unsigned long long peek(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// The cascade of the header comment on the K slots at `a`, entered at the first
// slot that may hold less than x.  A list is descending at every instant (what
// reaches slot i + 1 was smaller than slot i's value at that time, and slots
// only grow), so a read of a[m] above x rules out every slot up to m for good,
// and a binary search over reads taken at different times — stale ones
// included: they only show less — never enters too late.  On the global lists
// every slot from there on is read before its atomic: while other inserters
// raise the list, most values in flight are overtaken, and a read-modify-write
// that changes nothing still queues behind the others on the same address
// (without the read the pass took 3 - 6 times as long).  In
// LDS the extra read costs more than the atomics it saves (SN: + 17 %).
template <int SCOPE>
__device__ __forceinline__ void cascade(unsigned long long* a, uint32_t K, unsigned long long x) {
  uint32_t lo = 0, hi = K - 1u;  // (the caller has seen a[K - 1] < x)
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (peek<SCOPE>(a + mid) > x) lo = mid + 1u; else hi = mid;
  }
  for (uint32_t i = lo; i < K; ++i) {
    if (SCOPE == __HIP_MEMORY_SCOPE_AGENT && peek<SCOPE>(a + i) > x) continue;
    const unsigned long long old = __hip_atomic_fetch_max(a + i, x, __ATOMIC_RELAXED, SCOPE);
    if (old < x) {
      x = old;
      if (!x) return;
    }
  }
}

template <int SRC>
__global__ __launch_bounds__(kExThreads) void edge_exemplars_kernel(ExArgs a) {
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP, AG = __HIP_MEMORY_SCOPE_AGENT;
  const uint32_t E = a.E, K = a.K;
  auto* l64 = reinterpret_cast<unsigned long long*>(ex_lds);  // lds: lists; cached: thresholds
  const uint32_t tid = threadIdx.x;
  const uint32_t cells = a.place == kListsLds ? E * K : a.place == kListsGlobalCached ? E : 0u;
  for (uint32_t c = tid; c < cells; c += kExThreads) l64[c] = 0ull;
  __syncthreads();

  using Lanes = stream::Lanes<kExThreads, SRC == kSrcRows ? 4 : 2>;
  uint64_t lo, hi;
  stream::wg_range(a.per_wg, a.n, &lo, &hi);
  uint32_t bad = 0;
  for (uint64_t b = lo; b < hi; b += Lanes::kBatch) {
    Lanes L(b, hi, a.begin, tid);
    uint32_t edge[4], dur[4], sf[4] = {0u, 0u, 0u, 0u};
    if constexpr (SRC == kSrcRows) {
      stream::load_rows(L, a.rows, a.svcfl, a.dur, a.S, a.S0, edge, dur, sf);
    } else if (a.errors) {  // (uniform) the key carries no error bit
      stream::load_keys(L, a.keys, edge, dur, a.svcfl, sf);
    } else {
      stream::load_keys(L, a.keys, edge, dur);
    }
    unsigned long long x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = 0ull;  // 0: nothing to insert
      if (!L.live[j]) continue;
      if (edge[j] >= E) {  // never for rows of the aggregation / keys of span_edge_keys
        ++bad;
        continue;
      }
      if (a.errors && !((sf[j] >> 16) & ANOMOD_FLAG_ERROR)) continue;
      x[j] = (unsigned long long)dur[j] << 32 | (0xFFFFFFFFull - (L.pos(j) - a.begin));
    }
    if (a.place == kListsLds) {  // (uniform)
      // the four thresholds are read before the first cascade (one LDS latency
      // a batch instead of four): a threshold read early is a stale one
      unsigned long long thr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) thr[j] = x[j] ? peek<WG>(l64 + edge[j] * K + K - 1u) : 0ull;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x[j] > thr[j]) cascade<WG>(l64 + edge[j] * K, K, x[j]);
    } else {
      // one span after the other: the same four reads issued together were
      // 1.2 - 1.6 times slower on the global lists (they meet on a few lines)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!x[j]) continue;
        unsigned long long* g = a.lists + edge[j] * K;
        if (a.place == kListsGlobalCached) {
          if (x[j] < peek<WG>(l64 + edge[j])) continue;
          const unsigned long long t = peek<AG>(g + K - 1u);
          if (t) __hip_atomic_fetch_max(l64 + edge[j], t, __ATOMIC_RELAXED, WG);
          if (x[j] < t) continue;
        } else if (x[j] < peek<AG>(g + K - 1u)) {
          continue;
        }
        cascade<AG>(g, K, x[j]);
      }
    }
  }
  if (a.place == kListsLds) {
    __syncthreads();  // every cascade of the workgroup has landed
    for (uint32_t c = tid; c < cells; c += kExThreads) {
      const unsigned long long x = l64[c];
      if (!x) continue;
      unsigned long long* g = a.lists + (c / K) * K;
      if (x > peek<AG>(g + K - 1u)) cascade<AG>(g, K, x);
    }
  }
  stream::count_add(a.misc, bad, tid);
}

struct GatherArgs {
  const unsigned long long* lists;  // [E * K]
  const uint64_t* trace_ptr;        // [n_traces + 1]
  const uint64_t* span_id;
  const uint32_t* svcfl;
  const uint32_t* dur;
  const uint64_t* start;            // or NULL
  uint64_t begin, n, n_traces;
  uint32_t EK, K;
  uint32_t* n_found;                // [E] zeroed
  uint64_t* position;               // [E * K] each
  uint64_t* trace;
  uint64_t* o_span_id;
  uint32_t* o_dur;
  uint16_t* o_flags;
  uint64_t* o_start;
  unsigned long long* misc;
};

__global__ __launch_bounds__(kGatherThreads) void edge_exemplars_gather_kernel(GatherArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * kGatherThreads + threadIdx.x;
  if (c >= a.EK) return;
  const unsigned long long key = a.lists[c];
  uint64_t pos = ~0ull, trace = ~0ull, id = 0ull, start = 0ull;
  uint32_t dur = 0u, flags = 0u;
  if (key) {
    const uint64_t p = a.begin + (0xFFFFFFFFull - (key & 0xFFFFFFFFull));
    const uint32_t d = p < a.n ? a.dur[p] : 0u;
    if (p >= a.n || d != (uint32_t)(key >> 32)) {
      atomicAdd(a.misc + 1, 1ull);  // the key names no span of the set: reported, slot unused
    } else {
      pos = p;
      dur = d;
      flags = a.svcfl[p] >> 16;
      id = a.span_id[p];
      start = a.start ? a.start[p] : 0ull;
      // the last t with trace_ptr[t] <= p (begin <= p < trace_ptr[n_traces]: t < n_traces)
      uint64_t lo = 0, hi = a.n_traces;
      while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.trace_ptr[mid] <= p) lo = mid; else hi = mid;
      }
      trace = lo;
      atomicAdd(a.n_found + c / a.K, 1u);
    }
  }
  a.position[c] = pos;
  a.trace[c] = trace;
  a.o_span_id[c] = id;
  a.o_dur[c] = dur;
  a.o_flags[c] = (uint16_t)flags;
  a.o_start[c] = start;
}

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_edge_exemplars_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                anomod_edge_exemplars* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_edge_exemplars_spans: NULL argument");
  const uint32_t S = out->n_services, K = out->k;
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  ANOMOD_REQUIRE(ctx, K >= 1 && K <= 64, "k=%u outside [1, 64]", K);
  ANOMOD_REQUIRE(ctx, out->which <= 1, "which=%u: 0 (every span) or 1 (error spans)", out->which);
  ANOMOD_REQUIRE(ctx, (uint64_t)E * K <= (1ull << 24), "edge rows * k = %u * %u > 2^24", E, K);
  uint64_t in_traces[2], n = 0;
  if (int rc = stream_set_args(ctx, spans, S, false, ANOMOD_EINVAL, in_traces, &n)) return rc;
  const uint64_t EK = (uint64_t)E * K;
  if (n == 0) {
    if (out->n_found) memset(out->n_found, 0, (size_t)E * 4);
    if (out->position) memset(out->position, 0xFF, EK * 8);
    if (out->trace) memset(out->trace, 0xFF, EK * 8);
    if (out->span_id) memset(out->span_id, 0, EK * 8);
    if (out->dur_us) memset(out->dur_us, 0, EK * 4);
    if (out->flags) memset(out->flags, 0, EK * 2);
    if (out->start_us) memset(out->start_us, 0, EK * 8);
    return ANOMOD_OK;
  }
  ANOMOD_REQUIRE(ctx, in_traces[1] - in_traces[0] <= kExMaxSpans,
                 "edge exemplars: %llu spans in traces, at most 2^32 - 2 = %llu a call",
                 (unsigned long long)(in_traces[1] - in_traces[0]), (unsigned long long)kExMaxSpans);
  EdgeSource src(spans, in_traces, n);
  // One workspace in the windowed table's slot: (keys form: keys | the key
  // walk's words |) misc + the lists + n_found (zeroed together) | the gathered
  // columns.
  const size_t b_u64 = Carve::al(EK * 8), b_u32 = Carve::al(EK * 4), b_u16 = Carve::al(EK * 2),
               b_nf = Carve::al((size_t)E * 4);
  const size_t b_zero = 256 + b_u64 + b_nf;
  const size_t b_cols = 4 * b_u64 + b_u32 + b_u16;
  char* w = nullptr;
  if (int rc = ensure_scratch(ctx, kScratchEdgeWindows, src.b_keys + src.b_ws + b_zero + b_cols,
                              reinterpret_cast<void**>(&w)))
    return rc;
  Carve cv{w + src.b_keys + src.b_ws};
  ExArgs a{};
  a.misc = cv.take<unsigned long long>(256);
  a.lists = cv.take<unsigned long long>(b_u64);
  GatherArgs g{};
  g.n_found = cv.take<uint32_t>(b_nf);
  g.position = cv.take<uint64_t>(b_u64);
  g.trace = cv.take<uint64_t>(b_u64);
  g.o_span_id = cv.take<uint64_t>(b_u64);
  g.o_start = cv.take<uint64_t>(b_u64);
  g.o_dur = cv.take<uint32_t>(b_u32);
  g.o_flags = cv.take<uint16_t>(b_u16);
  g.lists = a.lists;
  g.misc = a.misc;
  g.trace_ptr = spans->trace_ptr;
  g.span_id = spans->span_id;
  g.svcfl = spans->svc_flags;
  g.dur = spans->dur_us;
  g.start = spans->start_us;
  g.begin = in_traces[0];
  g.n = n;
  g.n_traces = spans->n_traces;
  g.EK = (uint32_t)EK;
  g.K = K;
  if (src.rows) {
    a.rows = spans->parent_row;
    a.dur = spans->dur_us;
    a.S0 = spans->rows_S;
  }
  a.svcfl = spans->svc_flags;
  a.begin = in_traces[0];
  a.n = n;
  a.E = E;
  a.K = K;
  a.S = S;
  a.errors = out->which;
  // (tests, A/B: a smaller LDS budget — 0 = the lists in global memory, no
  // threshold cache — and fewer workgroups, so that small sets give a
  // workgroup several batches and several workgroups meet on a list)
  const uint64_t budget = std::min<uint64_t>(kExLdsBudget, env_cap("ANOMOD_EXEMPLARS_LDS"));
  a.place = EK * 8 <= budget ? kListsLds : (uint64_t)E * 8 <= budget ? kListsGlobalCached
                                                                      : kListsGlobal;
  const size_t lds = a.place == kListsLds ? EK * 8 : a.place == kListsGlobalCached ? E * 8u : 0;
  auto fn = src.rows ? edge_exemplars_kernel<kSrcRows> : edge_exemplars_kernel<kSrcKeys>;
  uint64_t grid = 0;
  if (int rc = stream_geometry(ctx, fn, kExThreads, lds, n, "ANOMOD_EXEMPLARS_WGS", &a.per_wg,
                               &grid))
    return rc;
  if (log_kernel())  // (tests, timing)
    fprintf(stderr, "anomod: edge exemplars kernel edge_exemplars_kernel<%s>, lists %s\n",
            src.rows ? "rows" : "keys", a.place == kListsLds ? "lds" : "global");
  stream_log("edge_exemplars_kernel", src.rows ? "rows" : "keys", -1,
             a.place == kListsLds ? "lds" : a.place == kListsGlobalCached ? "cached" : "global",
             grid, a.per_wg);
  if (int rc = stage_begin(ctx, kStageEdgeExemplars)) return rc;
  ANOMOD_HIP(ctx, hipMemsetAsync(a.misc, 0, b_zero, ctx->stream));
  if (int rc = src.fill(ctx, spans, S, w)) return rc;
  a.keys = src.keys;
  if (int rc = stage_begin(ctx, kStageEdgeExemplarsKernel)) return rc;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kExThreads), lds, ctx->stream, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeExemplarsKernel)) return rc;
  hipLaunchKernelGGL(edge_exemplars_gather_kernel,
                     dim3((unsigned)((EK + kGatherThreads - 1) / kGatherThreads)),
                     dim3(kGatherThreads), 0, ctx->stream, g);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeExemplars)) return rc;
  ANOMOD_HIP(ctx, stream_back(ctx, out->n_found, g.n_found, (size_t)E * 4));
  ANOMOD_HIP(ctx, stream_back(ctx, out->position, g.position, EK * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->trace, g.trace, EK * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->span_id, g.o_span_id, EK * 8));
  ANOMOD_HIP(ctx, stream_back(ctx, out->dur_us, g.o_dur, EK * 4));
  ANOMOD_HIP(ctx, stream_back(ctx, out->flags, g.o_flags, EK * 2));
  ANOMOD_HIP(ctx, stream_back(ctx, out->start_us, g.o_start, EK * 8));
  unsigned long long misc[2];
  if (int rc = stream_finish(ctx, a.misc, 0, "edge exemplars", "row", misc)) return rc;
  if (misc[1]) {
    set_error(ctx, "edge exemplars: %llu list entries name no span of the set (internal error)",
              misc[1]);
    return ANOMOD_ESTATE;
  }
  return ANOMOD_OK;
}

}  // extern "C"
