// What the span-walk passes (self time, critical path, trace shapes, trace
// spectrum, error origins) share around chunk.h's leaves: the parent-scan dispatch, the
// pipelined walk driver with its share policy, the listing of traces longer
// than a chunk and their windowed parent lookup, the sweep barrier of the
// long-trace kernels, and the host side of a call (trace range, workspace,
// long-trace count, scan choice, grid).  A pass keeps what it computes: its
// column loader, its chunk body and the phases of its long-trace kernel.
// Internal header (not part of the ABI).
#pragma once

#include "chunk.h"

namespace anomod {
namespace {  // internal linkage
namespace chunk {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// ---- parent scan ------------------------------------------------------------
// The scan dispatch of the edge kernels: sets not declared unique scan forward
// for the first match; unique ids scan from both ends, and tables wider than
// kNarrowRows rows (TrainTicket: 48 * 46) and sets holding long traces take
// the split-word form of that scan.
enum Scan { kScanFwd = 0, kScanBidir = 1, kScanSplit = 2 };
constexpr uint32_t kNarrowRows = 512;
constexpr uint32_t kSplitFwd = 12, kSplitBwd = 4;  // edge_agg.hip kWFwd / kWBwd

// First span of [a, b) whose id equals pid (-1: none): the forward scan of
// sets not declared unique, kFwdScan ids per step.
constexpr uint32_t kFwdScan = 10;
static_assert(kFwdScan % 2 == 0 && kFwdScan <= kScanSlack, "scan step");
__device__ __forceinline__ int find_first(const uint64_t* lsid, uint32_t a, uint32_t b,
                                          uint64_t pid) {
  for (uint32_t q0 = a; q0 < b; q0 += kFwdScan) {
    uint64_t v[kFwdScan];
#pragma unroll
    for (uint32_t j = 0; j < kFwdScan; ++j) v[j] = lsid[q0 + j];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFwdScan; ++j) m |= (v[j] == pid ? 1u : 0u) << j;
    const uint32_t hi = (b - q0) < kFwdScan ? (b - q0) : kFwdScan;  // >= 1
    m &= (1u << hi) - 1u;
    if (m) return (int)(q0 + __ffs(m) - 1u);
  }
  return -1;
}

// The parent of span i of the trace [a, b) by the set's scan (-1: none).  The
// ids are staged as u64 (lsid) or, for the split scan, as two u32 planes over
// the same bytes (llo, lhi).
template <int SCAN>
__device__ __forceinline__ int find_parent(const uint64_t* lsid, const uint32_t* llo,
                                           const uint32_t* lhi, uint32_t a, uint32_t b, uint32_t i,
                                           uint64_t pid) {
  if constexpr (SCAN == kScanSplit)
    return find_parent_split<kSplitFwd, kSplitBwd>(llo, lhi, a, b, i, pid);
  else if constexpr (SCAN == kScanBidir)
    return find_parent_bidir<kFwd, kBwd>(lsid, a, b, i, pid);
  else
    return find_first(lsid, a, b, pid);
}

// ---- records, ranks -----------------------------------------------------------
// The edge record edge_aggregate_records takes: (parent row * S + service) <<
// 33 | error << 32 | v, with sf = svc | flags << 16.
__device__ __forceinline__ unsigned long long edge_rec(uint32_t row, uint32_t S, uint32_t sf,
                                                       uint32_t v) {
  return ((unsigned long long)(row * S + (sf & 0xFFFFu)) << 33) |
         ((unsigned long long)((sf >> 16) & ANOMOD_FLAG_ERROR ? 1u : 0u) << 32) | v;
}
// The record of no span: edge_aggregate_records skips it (no real record is
// all ones: a row index stays far below 2^31).
constexpr unsigned long long kSkipRec = ~0ull;

// Index, among the chunk's trace-start flags, of the last flag at or before
// position s (< kStage): trace_in_chunk for a position that is not the lane's.
__device__ __forceinline__ uint32_t rank_at(const uint64_t (&Sm)[kPer], uint32_t s) {
  const uint32_t q = s >> 6, b = s & 63u;
  uint32_t before = 0;
  uint64_t m = Sm[0];
#pragma unroll
  for (int j = 1; j < kPer; ++j) {
    before += q >= (uint32_t)j ? (uint32_t)__popcll(Sm[j - 1]) : 0u;
    m = q >= (uint32_t)j ? Sm[j] : m;
  }
  const uint64_t le = b == 63u ? ~0ull : ((2ull << b) - 1ull);
  return before + (uint32_t)__popcll(m & le) - 1u;
}

// ---- the walk -------------------------------------------------------------------
// Every wave of a grid of WAVES-wave workgroups walks its traces in chunks:
// load(chunk, R) starts the chunk's column loads into a Regs, body(chunk, end,
// t0, R) resolves a chunk of whole traces (end: this lane's trace end relative
// to chunk.base, lanes < chunk.k; t0: the chunk's first trace) and on_long(t,
// n) takes trace t of n > kStage spans, which no body sees.  Software
// pipeline: the bounds of chunk c+2 and the span columns of chunk c+1 are in
// flight while chunk c is resolved.  Share policy: a static share per wave,
// then the last 1 / DYN of the traces in segments of kDynSeg from the global
// counter *ctr (zeroed before the launch).
constexpr uint64_t kDynSeg = 512;

template <int WAVES, uint64_t DYN, typename Regs, typename Load, typename Body, typename OnLong>
__device__ __forceinline__ void walk_traces(const uint64_t* __restrict__ trace_ptr,
                                            uint64_t n_traces, unsigned long long* ctr,
                                            const Load& load, const Body& body,
                                            const OnLong& on_long) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES + wid;
  const uint64_t nw = (uint64_t)gridDim.x * WAVES;
  auto run = [&](const uint64_t t_begin, const uint64_t t_end) __attribute__((always_inline)) {
    uint64_t lo, hi;
    load_bounds(trace_ptr, t_begin, t_end, lane, lo, hi);
    Chunk cur = make_chunk(t_begin, t_end, lane, lo, hi);
    uint32_t end_cur = (uint32_t)(hi - cur.base);
    uint64_t t_cur = t_begin;
    Regs R;
    load(cur, R);
    uint64_t t_next = t_begin + (cur.k ? cur.k : 1u);
    load_bounds(trace_ptr, t_next, t_end, lane, lo, hi);
    while (true) {
      const bool has_next = t_next < t_end;
      const uint64_t t_nxt = t_next;
      Chunk nxt{};
      uint32_t end_nxt = 0;
      Regs Rn;
      if (has_next) {
        nxt = make_chunk(t_next, t_end, lane, lo, hi);
        end_nxt = (uint32_t)(hi - nxt.base);
        load(nxt, Rn);
        t_next += nxt.k ? nxt.k : 1u;
        load_bounds(trace_ptr, t_next, t_end, lane, lo, hi);
      }
      if (cur.k == 0)
        on_long(t_cur, cur.n);
      else
        body(cur, end_cur, t_cur, R);
      if (!has_next) break;
      cur = nxt;
      end_cur = end_nxt;
      t_cur = t_nxt;
      R = Rn;
    }
  };
  const uint64_t n_static = n_traces - n_traces / DYN;
  uint64_t t_begin = uniform64(n_static * gw / nw);
  uint64_t t_end = uniform64(n_static * (gw + 1) / nw);
  while (true) {
    if (t_begin < t_end) run(t_begin, t_end);
    if (n_static == n_traces) break;
    unsigned long long g = 0;
    if (lane == 0) g = atomicAdd(ctr, (unsigned long long)kDynSeg);
    g = __shfl(g, 0);
    t_begin = uniform64(n_static + g);
    if (t_begin >= n_traces) break;
    t_end = uniform64(t_begin + kDynSeg < n_traces ? t_begin + kDynSeg : n_traces);
  }
}

// ---- long traces ------------------------------------------------------------------
// The walk lists trace t of n spans for the pass's long-trace kernel: big[0]
// counts the listed traces, big[1] their spans (the trace's offset into the
// per-span scratch), big[2] is that kernel's ticket; big_list holds (trace,
// scratch offset) pairs.
__device__ __forceinline__ void list_long(unsigned long long* big, unsigned long long* big_list,
                                          uint64_t big_cap, int lane, uint64_t t, uint32_t n) {
  if (lane == 0) {
    const unsigned long long j = atomicAdd(&big[0], 1ull);
    if (j < big_cap) {  // (always: the list is sized to the counted long traces)
      big_list[2 * j] = t;
      big_list[2 * j + 1] = atomicAdd(&big[1], (unsigned long long)n);
    }
  }
}

// The long-trace kernels run one workgroup of kBigThreads per listed trace.
// Parent positions come from an LDS hash table over a window of kBigWin ids
// (id -> first position in the window): a block of kBigThreads * kBigPer
// spans probes the trace's windows in trace order, so the first window holding
// an id gives its first occurrence — ceil(L / block) * ceil(L / kBigWin)
// window builds of kBigWin inserts each, O(L^2 / block) LDS inserts for a
// trace of L spans.
constexpr int kBigThreads = 512;
constexpr int kBigPer = 8;
constexpr uint32_t kBigWin = 2048;
constexpr uint32_t kBigSlots = 2 * kBigWin;  // load <= 1/2
static_assert((kBigSlots & (kBigSlots - 1)) == 0, "power-of-two table");

__device__ __forceinline__ uint32_t big_slot(uint64_t id) {
  return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32) & (kBigSlots - 1u);
}

// bkey[kBigSlots]: 0 = empty (id 0 is never a parent reference); bpos[kBigSlots]:
// first position in the window.  big_parents needs the table clear and leaves
// it clear; a barrier orders the clear before the next insert.
__device__ __forceinline__ void big_clear(unsigned long long* bkey, uint32_t* bpos, int tid) {
  for (uint32_t k = tid; k < kBigSlots; k += kBigThreads) {
    bkey[k] = 0ull;
    bpos[k] = kNone;
  }
}

// For the spans i = b0 + r * kBigThreads + tid, r < kBigPer, of the trace [lo,
// lo + L): pid[r] = the parent reference (0 past the trace) and pp[r] = the
// first position in the trace whose id equals it (kNone: none).  Called by
// the whole workgroup.  L may lie within a window of 2^32: b0 is u64 (b0 +=
// block must not wrap in the caller), the block's spans are tested as offsets
// from b0, and the window loop leaves before its u32 start could wrap.
__device__ __forceinline__ void big_parents(const uint64_t* __restrict__ span_id,
                                            const uint64_t* __restrict__ parent, uint64_t lo,
                                            uint32_t L, uint64_t b0, int tid,
                                            unsigned long long* bkey, uint32_t* bpos,
                                            uint64_t (&pid)[kBigPer], uint32_t (&pp)[kBigPer]) {
  bool need = false;
  const uint32_t left = L - (uint32_t)b0;  // (b0 < L) spans from b0 on
#pragma unroll
  for (int r = 0; r < kBigPer; ++r) {
    const uint32_t o = (uint32_t)r * kBigThreads + tid;
    pid[r] = o < left ? parent[lo + ((uint32_t)b0 + o)] : 0ull;  // (no wrap: b0 + o < L)
    pp[r] = kNone;
    need |= pid[r] != 0ull;
  }
  for (uint32_t w0 = 0; w0 < L; w0 += kBigWin) {
    if (!__syncthreads_or(need)) break;  // also orders the previous clear
    for (uint32_t k = tid; k < kBigWin && (uint64_t)w0 + k < L; k += kBigThreads) {
      const uint64_t id = span_id[lo + w0 + k];
      if (id == 0ull) continue;
      for (uint32_t sl = big_slot(id);; sl = (sl + 1u) & (kBigSlots - 1u)) {
        const unsigned long long prev = atomicCAS(&bkey[sl], 0ull, (unsigned long long)id);
        if (prev == 0ull || prev == id) {
          atomicMin(&bpos[sl], k);  // the first position wins
          break;
        }
      }
    }
    __syncthreads();
    need = false;
#pragma unroll
    for (int r = 0; r < kBigPer; ++r) {
      if (pid[r] == 0ull || pp[r] != kNone) continue;
      for (uint32_t sl = big_slot(pid[r]);; sl = (sl + 1u) & (kBigSlots - 1u)) {
        const unsigned long long key = bkey[sl];
        if (key == pid[r]) {
          pp[r] = w0 + bpos[sl];
          break;
        }
        if (key == 0ull) break;
      }
      need |= pp[r] == kNone;
    }
    __syncthreads();
    big_clear(bkey, bpos, tid);
    if ((uint64_t)w0 + kBigWin >= L) break;  // (w0 += kBigWin must not wrap)
  }
}

// Per-span state of a long trace in global scratch: words another thread may
// have written are written by agent-scope stores and atomics and read by
// agent-scope loads, all served by L2.
template <typename T>
__device__ __forceinline__ T aload(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void astore(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Every store and atomic of the sweep has reached L2 before any thread starts
// the next one: each wave waits for its own vector-memory operations, then the
// workgroup's barrier (which alone waits for LDS only).  The words threads
// share are written by agent-scope stores and atomics and read by agent-scope
// loads, all served by L2, so no cache needs writing back or invalidating: a
// __threadfence() per sweep made the critical-path long-trace kernel 16 times
// slower.
constexpr int kWaitVm0 = 0x0F70;  // s_waitcnt vmcnt(0), expcnt and lgkmcnt at their maxima
__device__ __forceinline__ void wait_stores() { __builtin_amdgcn_s_waitcnt(kWaitVm0); }
__device__ __forceinline__ void sweep_sync() {
  wait_stores();
  __syncthreads();
}

}  // namespace chunk
}  // namespace

// ---- host side of a walk call (span_walk.hip) -------------------------------------
// The spans that lie in traces: in_traces = [trace_ptr[0], trace_ptr[n_traces])
// read back from the device ({0, 0} for a set without traces or spans; an
// upload may leave spans outside every trace).  A range outside the set's
// spans sets the error (`who` prefixes its text), zeroes in_traces and returns
// ANOMOD_EINVAL.
int trace_span_range(anomod_ctx* ctx, const anomod_spans* spans, uint64_t in_traces[2],
                     const char* who = "");

// A call's device workspace, freed when the call returns, after the stream's
// work: a small block of words (counters) and one block the call carves its
// arrays from.
struct CallWorkspace {
  anomod_ctx* ctx;
  void* words = nullptr;
  void* block = nullptr;
  size_t carved = 0;
  ~CallWorkspace();
  CallWorkspace(anomod_ctx* c) : ctx(c) {}
  CallWorkspace(const CallWorkspace&) = delete;
  CallWorkspace& operator=(const CallWorkspace&) = delete;
  // *p (words or block) = `bytes` of device memory; on failure ANOMOD_ENOMEM
  // and "hipMalloc(bytes) for the `what` workspace failed".
  int take(void** p, size_t bytes, const char* what);
  static size_t al(size_t x) { return (x + 255) & ~size_t(255); }
  // the next `bytes` of the block
  template <typename T = char>
  T* carve(size_t bytes) {
    char* p = static_cast<char*>(block) + carved;
    carved += bytes;
    return reinterpret_cast<T*>(p);
  }
};

// nlong = {traces, spans} of the set that outgrow a chunk, counted on the
// device in d_words[0..1] (one small kernel and a host wait; {0, 0} without
// either when the set's longest trace is known to fit a chunk).
int count_long_traces(anomod_ctx* ctx, const anomod_spans* spans, unsigned long long* d_words,
                      unsigned long long nlong[2]);

// *scan = the Scan of the walk kernels for the set and a table of S services:
// span_scan_choice (d_cnt: its two device words) and the split-word rule.
int pick_walk_scan(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S,
                   unsigned long long* d_cnt, int* scan);
const char* scan_name(int scan);
// With ANOMOD_LOG_KERNEL=1 (tests): "anomod: <pass> kernel <kernel><<scan>>, N long traces".
void log_walk_kernel(const char* pass, const char* kernel, int scan, unsigned long long n_long);

// Persistent grid of a walk kernel: what the occupancy allows on every CU.
template <typename Fn>
int walk_grid(anomod_ctx* ctx, Fn fn, int threads, uint64_t* grid, size_t dyn_lds = 0) {
  int per_cu = 0;
  ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void*>(fn), threads, dyn_lds));
  *grid = (uint64_t)ctx->num_cus * (uint64_t)(per_cu > 0 ? per_cu : 1);
  return ANOMOD_OK;
}

}  // namespace anomod
