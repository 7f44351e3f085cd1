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
// edge_exemplars_kernel is a persistent stream over span positions in the
// shape of edge_load_kernel (512 threads, one contiguous range per workgroup,
// 16-B non-temporal loads, 2048 spans per iteration), with its two sources:
//   rows  complete parent rows (anomod_spans::parent_row): row 2 B, svc|flags
//         4 B, dur 4 B = 10 B/span in one pass
//   keys  any other grouped set: span_edge_keys writes edge << 32 | dur by
//         span position, then key 8 B (+ svc|flags 4 B when only error spans
//         are wanted: the key carries no error bit)
// and two placements of the lists, picked on the host from E * K * 8:
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
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

constexpr int kExThreads = 512;
constexpr int kExBatch = kExThreads * 4;              // spans per workgroup iteration
constexpr uint32_t kExLdsBudget = 40u * 1024u - 64u;  // four workgroups per CU
constexpr uint64_t kExMaxRange = 1ull << 31;          // spans per workgroup (u32 counter)
constexpr uint64_t kExMaxSpans = 0xFFFFFFFEull;       // spans in traces per call
constexpr uint32_t kNoEdge = 0xFFFFFFFFu;
constexpr int kGatherThreads = 256;

using u64x2 = unsigned long long __attribute__((ext_vector_type(2)));
using u32x2 = uint32_t __attribute__((ext_vector_type(2)));
using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

enum { kSrcRows = 0, kSrcKeys = 1 };
enum { kListsGlobal = 0, kListsGlobalCached = 1, kListsLds = 2 };

struct ExArgs {
  const unsigned long long* keys;  // keys form: [n] edge << 32 | dur
  const uint16_t* rows;            // rows form: [n] parent rows
  const uint32_t* svcfl;           // [n] svc | flags << 16 (rows form; keys form when errors)
  const uint32_t* dur;             // rows form: [n]
  uint64_t begin, n, per_wg;       // spans [begin, n) lie in traces; per_wg: a multiple of kExBatch
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

  const uint64_t lo = (uint64_t)blockIdx.x * a.per_wg;
  const uint64_t hi = lo + a.per_wg < a.n ? lo + a.per_wg : a.n;
  uint32_t bad = 0;
  for (uint64_t b = lo; b < hi; b += kExBatch) {
    uint64_t pos[4];
    uint32_t edge[4], dur[4], sf[4];
    bool live[4];
    if constexpr (SRC == kSrcRows) {
      // four consecutive spans a lane: 16 B of svc|flags, 16 B of durations, 8 B of rows
      uint32_t row[4];
      const uint64_t i0 = b + (uint64_t)tid * 4;
      if (b + kExBatch <= hi) {  // (b is a multiple of kExBatch: aligned groups)
        const u32x4 f = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.svcfl + i0));
        const u32x4 d = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.dur + i0));
        const u32x2 r = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(a.rows + i0));
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
          sf[j] = live[j] ? a.svcfl[i] : 0u;
          dur[j] = live[j] ? a.dur[i] : 0u;
          row[j] = live[j] ? (uint32_t)a.rows[i] : 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pos[j] = i0 + j;
        // root / orphan codes of the aggregation that wrote the rows -> this call's
        const uint32_t p = row[j] >= a.S0 ? row[j] - a.S0 + a.S : row[j];
        const uint32_t svc = sf[j] & 0xFFFFu;
        edge[j] = p < a.S + ANOMOD_ROOT_ROWS && svc < a.S ? p * a.S + svc : kNoEdge;
      }
    } else {
      unsigned long long key[4];
      if (b + kExBatch <= hi) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint64_t i = b + ((uint64_t)j * kExThreads + tid) * 2;
          const u64x2 k = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.keys + i));
          key[2 * j] = k.x, key[2 * j + 1] = k.y;
          sf[2 * j] = sf[2 * j + 1] = 0u;
          if (a.errors) {  // (uniform)
            const u32x2 f = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(a.svcfl + i));
            sf[2 * j] = f.x, sf[2 * j + 1] = f.y;
          }
          live[2 * j] = i >= a.begin;
          live[2 * j + 1] = i + 1 >= a.begin;
          pos[2 * j] = i, pos[2 * j + 1] = i + 1;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint64_t i = b + ((uint64_t)(j >> 1) * kExThreads + tid) * 2 + (j & 1);
          live[j] = i < hi && i >= a.begin;
          key[j] = live[j] ? a.keys[i] : 0ull;
          sf[j] = live[j] && a.errors ? a.svcfl[i] : 0u;
          pos[j] = i;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        edge[j] = (uint32_t)(key[j] >> 32);
        dur[j] = (uint32_t)key[j];
      }
    }
    unsigned long long x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = 0ull;  // 0: nothing to insert
      if (!live[j]) continue;
      if (edge[j] >= E) {  // never for rows of the aggregation / keys of span_edge_keys
        ++bad;
        continue;
      }
      if (a.errors && !((sf[j] >> 16) & ANOMOD_FLAG_ERROR)) continue;
      x[j] = (unsigned long long)dur[j] << 32 | (0xFFFFFFFFull - (pos[j] - a.begin));
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
  for (int o = 32; o > 0; o >>= 1) bad += (uint32_t)__shfl_xor((int)bad, o);
  if ((tid & 63u) == 0 && bad) atomicAdd(a.misc, (unsigned long long)bad);
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

// Value of a numeric environment cap, "no cap" when unset or not a number;
// ANOMOD_EXEMPLARS_WGS must be at least 1.
uint64_t ex_env_cap(const char* name) {
  const char* e = getenv(name);
  if (!e || !*e) return 0xFFFFFFFFull;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  if (*end) return 0xFFFFFFFFull;
  return !strcmp(name, "ANOMOD_EXEMPLARS_WGS") && v == 0 ? 1 : (uint64_t)v;
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
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_REQUIRE(ctx, spans->grouped, "span set is not grouped by trace: anomod_spans_group first");
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "span service index %u >= n_services %u", spans->max_svc, S);
  uint64_t in_traces[2];
  if (spans->n_traces && spans->n_spans)
    if (int rc = bind(ctx)) return rc;
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  const uint64_t n = in_traces[1] > in_traces[0] ? in_traces[1] : 0;
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
  // the rows form: complete parent rows over exactly the spans in traces
  const bool rows = span_rows_ready(spans) && spans->rows_lo == in_traces[0] &&
                    spans->rows_hi == in_traces[1];
  // One workspace in the windowed table's slot: (keys form: keys | the key
  // walk's words |) misc + the lists + n_found (zeroed together) | the gathered
  // columns.
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t b_keys = rows ? 0 : al(n * 8);
  const size_t b_ws = rows ? 0 : al(span_edge_keys_ws_bytes(spans));
  const size_t b_u64 = al(EK * 8), b_u32 = al(EK * 4), b_u16 = al(EK * 2), b_nf = al((size_t)E * 4);
  const size_t b_zero = 256 + b_u64 + b_nf;
  const size_t b_cols = 4 * b_u64 + b_u32 + b_u16;
  char* w = nullptr;
  if (int rc = ensure_scratch(ctx, kScratchEdgeWindows, b_keys + b_ws + b_zero + b_cols,
                              reinterpret_cast<void**>(&w)))
    return rc;
  auto* keys = reinterpret_cast<unsigned long long*>(w);
  auto* ws = reinterpret_cast<unsigned long long*>(w + b_keys);
  char* t = w + b_keys + b_ws;
  auto take = [&](size_t bytes) {
    char* p = t;
    t += bytes;
    return p;
  };
  ExArgs a{};
  a.misc = reinterpret_cast<unsigned long long*>(take(256));
  a.lists = reinterpret_cast<unsigned long long*>(take(b_u64));
  GatherArgs g{};
  g.n_found = reinterpret_cast<uint32_t*>(take(b_nf));
  g.position = reinterpret_cast<uint64_t*>(take(b_u64));
  g.trace = reinterpret_cast<uint64_t*>(take(b_u64));
  g.o_span_id = reinterpret_cast<uint64_t*>(take(b_u64));
  g.o_start = reinterpret_cast<uint64_t*>(take(b_u64));
  g.o_dur = reinterpret_cast<uint32_t*>(take(b_u32));
  g.o_flags = reinterpret_cast<uint16_t*>(take(b_u16));
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
  if (rows) {
    a.rows = spans->parent_row;
    a.dur = spans->dur_us;
    a.S0 = spans->rows_S;
  } else {
    a.keys = keys;
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
  const uint64_t budget = std::min<uint64_t>(kExLdsBudget, ex_env_cap("ANOMOD_EXEMPLARS_LDS"));
  a.place = EK * 8 <= budget ? kListsLds : (uint64_t)E * 8 <= budget ? kListsGlobalCached
                                                                      : kListsGlobal;
  const size_t lds = a.place == kListsLds ? EK * 8 : a.place == kListsGlobalCached ? E * 8u : 0;
  auto fn = rows ? edge_exemplars_kernel<kSrcRows> : edge_exemplars_kernel<kSrcKeys>;
  int per_cu = 0;
  ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void*>(fn), kExThreads, lds));
  // persistent workgroups, one contiguous range of whole batches each
  const uint64_t batches = (n + kExBatch - 1) / kExBatch;
  uint64_t grid = std::min<uint64_t>((uint64_t)ctx->num_cus * (per_cu > 0 ? per_cu : 1), batches);
  grid = std::min<uint64_t>(grid, ex_env_cap("ANOMOD_EXEMPLARS_WGS"));
  a.per_wg = (batches + grid - 1) / grid * kExBatch;
  if (a.per_wg > kExMaxRange) a.per_wg = kExMaxRange;  // (more workgroups than are resident)
  grid = (n + a.per_wg - 1) / a.per_wg;
  if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests, timing)
    fprintf(stderr, "anomod: edge exemplars kernel edge_exemplars_kernel<%s>, lists %s\n",
            rows ? "rows" : "keys", a.place == kListsLds ? "lds" : "global");
  if (int rc = stage_begin(ctx, kStageEdgeExemplars)) return rc;
  ANOMOD_HIP(ctx, hipMemsetAsync(a.misc, 0, b_zero, ctx->stream));
  if (!rows)
    if (int rc = span_edge_keys(ctx, spans, S, keys, ws)) return rc;
  if (int rc = stage_begin(ctx, kStageEdgeExemplarsKernel)) return rc;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kExThreads), lds, ctx->stream, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeExemplarsKernel)) return rc;
  hipLaunchKernelGGL(edge_exemplars_gather_kernel,
                     dim3((unsigned)((EK + kGatherThreads - 1) / kGatherThreads)),
                     dim3(kGatherThreads), 0, ctx->stream, g);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeExemplars)) return rc;
  unsigned long long misc[2] = {0ull, 0ull};
  ANOMOD_HIP(ctx, hipMemcpyAsync(misc, a.misc, 16, hipMemcpyDeviceToHost, ctx->stream));
  auto back = [&](void* dst, const void* src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
  };
  ANOMOD_HIP(ctx, back(out->n_found, g.n_found, (size_t)E * 4));
  ANOMOD_HIP(ctx, back(out->position, g.position, EK * 8));
  ANOMOD_HIP(ctx, back(out->trace, g.trace, EK * 8));
  ANOMOD_HIP(ctx, back(out->span_id, g.o_span_id, EK * 8));
  ANOMOD_HIP(ctx, back(out->dur_us, g.o_dur, EK * 4));
  ANOMOD_HIP(ctx, back(out->flags, g.o_flags, EK * 2));
  ANOMOD_HIP(ctx, back(out->start_us, g.o_start, EK * 8));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (misc[0]) {
    set_error(ctx, "edge exemplars: %llu spans carry no edge row (internal error)", misc[0]);
    return ANOMOD_ESTATE;
  }
  if (misc[1]) {
    set_error(ctx, "edge exemplars: %llu list entries name no span of the set (internal error)",
              misc[1]);
    return ANOMOD_ESTATE;
  }
  return ANOMOD_OK;
}

}  // extern "C"
