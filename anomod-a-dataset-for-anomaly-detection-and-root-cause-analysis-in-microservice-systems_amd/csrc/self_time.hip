// Self time (exclusive latency) of a grouped span set, and its edge table.
//
//   par(i)       = the first span of i's trace, in position order, whose
//                  span_id equals i's parent_span_id (the edge table's rule);
//                  none for a root (reference 0), an orphan (no such span) and
//                  a span whose first match is itself
//   child_sum(j) = sum of dur_us[i] over par(i) == j                   (u64)
//   self_us[i]   = dur_us[i] - min(dur_us[i], child_sum(i))            (u32)
//
// Children overlapping in time are summed, not merged.
//
// One chunk walk (chunk.h: persistent waves, <= 256 spans / <= 64 whole
// traces per chunk, buffer loads, the columns of chunk c+1 in flight while
// chunk c is resolved) stages ids and services in the wave's LDS, finds every
// span's parent *position*, adds the span's duration to the parent's u64
// child-sum slot (ds_add_u64; the children of one parent serialise on its
// slot) and, after a wave sync, writes one edge record per span in the form
// edge_aggregate_records takes: (parent row * S + service) << 33 | error << 32
// | self_us.  The table — histogram forms, finalize, the merge over an
// attached communicator — is that call's, unchanged.
//
// Traces longer than a chunk are listed by the walk and resolved by
// self_big_kernel, one workgroup per listed trace.
#include <algorithm>
#include <cstring>

#include "chunk.h"
#include "common.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kSelfWaves = 8;
constexpr int kSelfThreads = kSelfWaves * kWave;
// Tables wider than this many rows (TrainTicket: 48 * 46) and sets holding
// long traces take the split-word scan, as the edge kernels do.
constexpr uint32_t kNarrowRows = 512;
enum Scan { kScanFwd = 0, kScanBidir = 1, kScanSplit = 2 };
constexpr uint32_t kSplitFwd = 12, kSplitBwd = 4;  // edge_agg.hip kWFwd / kWBwd

// Per-wave LDS (every offset a multiple of 16).
constexpr int kSSid = 0;  // u64 span ids [kStage + kScanSlack], or two u32 planes of that length
constexpr int kSSum = kSSid + (kStage + (int)kScanSlack) * 8;  // u64 child sums [kStage]
constexpr int kSSvc = kSSum + kStage * 8;                      // u16 services [kStage]
constexpr int kSFlag = kSSvc + kStage * 2;                     // u8 trace-start flags [kStage]
constexpr int kSBytes = kSFlag + kStage;
static_assert(kSBytes % 16 == 0, "wave staging must stay 16-B aligned");

struct SelfArgs {
  unsigned long long* rec;       // [n_spans] edge records by span position
  uint32_t* self_us;             // [n_spans] or NULL
  unsigned long long* ctr;       // trace-segment counter of the dynamic tail
  unsigned long long* big;       // [0] listed traces, [1] their spans, [2] ticket
  unsigned long long* big_list;  // (trace, child-sum offset) per listed trace
  uint64_t big_cap;              // entries big_list holds
  unsigned long long* csum;      // child sums of the listed traces' spans (zeroed)
  uint32_t S;
};

struct Regs {
  uint64_t sid[kPer], pid[kPer];
  uint32_t dur[kPer], sf[kPer];  // sf = svc | flags << 16
};

__device__ __forceinline__ void load_regs(const uint64_t* __restrict__ span_id,
                                          const uint64_t* __restrict__ parent,
                                          const uint32_t* __restrict__ svcfl,
                                          const uint32_t* __restrict__ dur, const Chunk& c, int lane,
                                          Regs& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by self_big_kernel
  const auto rsid = rsrc(span_id + c.base, n * 8u);
  const auto rpid = rsrc(parent + c.base, n * 8u);
  const auto rsf = rsrc(svcfl + c.base, n * 4u);
  const auto rdur = rsrc(dur + c.base, n * 4u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.sid[r] = bload64(rsid, i * 8u);
    R.pid[r] = bload64(rpid, i * 8u);
    R.sf[r] = bload32(rsf, i * 4u);
    R.dur[r] = bload32(rdur, i * 4u);
  }
}

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

__device__ __forceinline__ unsigned long long make_rec(uint32_t row, uint32_t S, uint32_t sf,
                                                       uint32_t self) {
  return ((unsigned long long)(row * S + (sf & 0xFFFFu)) << 33) |
         ((unsigned long long)((sf >> 16) & ANOMOD_FLAG_ERROR ? 1u : 0u) << 32) | self;
}

template <int SCAN>
__device__ __forceinline__ void self_chunk(unsigned char* wsm, int lane, const Chunk& c,
                                           const Regs& R, const SelfArgs& a) {
  auto* lsid = reinterpret_cast<uint64_t*>(wsm + kSSid);
  auto* llo = reinterpret_cast<uint32_t*>(wsm + kSSid);
  uint32_t* lhi = llo + (kStage + kScanSlack);
  auto* lsum = reinterpret_cast<unsigned long long*>(wsm + kSSum);
  auto* lsvc = reinterpret_cast<uint16_t*>(wsm + kSSvc);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kSFlag);
  // Stage ids / services (lanes past n hold zeros from the buffer loads),
  // clear the child sums, mark trace starts.  Durations stay in registers:
  // a span adds its own to the parent's slot and reads back only its own slot.
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if constexpr (SCAN == kScanSplit) {
      llo[i] = (uint32_t)R.sid[r];
      lhi[i] = (uint32_t)(R.sid[r] >> 32);
    } else {
      lsid[i] = R.sid[r];
    }
    lsvc[i] = (uint16_t)R.sf[r];
    lsum[i] = 0ull;
  }
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);
  uint32_t row[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    uint32_t p = a.S;  // ROOT
    if (i < c.n && R.pid[r] != 0ull) {
      p = a.S + 1u;  // ORPHAN unless found in the trace
      uint32_t ta, tb;
      trace_bounds(Sm, r, lane, c.n, ta, tb);
      int q;
      if constexpr (SCAN == kScanSplit)
        q = find_parent_split<kSplitFwd, kSplitBwd>(llo, lhi, ta, tb, i, R.pid[r]);
      else if constexpr (SCAN == kScanBidir)
        q = find_parent_bidir<kFwd, kBwd>(lsid, ta, tb, i, R.pid[r]);
      else
        q = find_first(lsid, ta, tb, R.pid[r]);
      if (q >= 0) {
        p = lsvc[q];
        // a span is not its own child; its row keeps its own service as parent
        if ((uint32_t)q != i) atomicAdd(&lsum[q], (unsigned long long)R.dur[r]);
      }
    }
    row[r] = p;
  }
  wave_sync();
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if (i >= c.n) continue;
    const unsigned long long cs = lsum[i];
    const uint32_t d = R.dur[r];
    const uint32_t self = d - (cs < (unsigned long long)d ? (uint32_t)cs : d);
    a.rec[c.base + i] = make_rec(row[r], a.S, R.sf[r], self);
    if (a.self_us) a.self_us[c.base + i] = self;
  }
  wave_sync();  // the staging area is free for the next chunk
}

template <int SCAN>
__global__ __launch_bounds__(kSelfThreads) void self_time_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ trace_ptr, uint64_t n_traces, SelfArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kSBytes * kSelfWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  unsigned char* wsm = smem + wid * kSBytes;
  const uint64_t gw = (uint64_t)blockIdx.x * kSelfWaves + wid;
  const uint64_t nw = (uint64_t)gridDim.x * kSelfWaves;
  auto run = [&](const uint64_t t_begin, const uint64_t t_end) __attribute__((always_inline)) {
    // Software pipeline (as the edge kernel): the bounds of chunk c+2 and the
    // span columns of chunk c+1 are in flight while chunk c is resolved.
    uint64_t lo, hi;
    load_bounds(trace_ptr, t_begin, t_end, lane, lo, hi);
    Chunk cur = make_chunk(t_begin, t_end, lane, lo, hi);
    uint64_t t_cur = t_begin;
    Regs R;
    load_regs(span_id, parent, svcfl, dur, cur, lane, R);
    uint64_t t_next = t_begin + (cur.k ? cur.k : 1u);
    load_bounds(trace_ptr, t_next, t_end, lane, lo, hi);
    while (true) {
      const bool has_next = t_next < t_end;
      const uint64_t t_nxt = t_next;
      Chunk nxt{};
      Regs Rn;
      if (has_next) {
        nxt = make_chunk(t_next, t_end, lane, lo, hi);
        load_regs(span_id, parent, svcfl, dur, nxt, lane, Rn);
        t_next += nxt.k ? nxt.k : 1u;
        load_bounds(trace_ptr, t_next, t_end, lane, lo, hi);
      }
      if (cur.k == 0) {  // longer than kStage: listed for self_big_kernel
        if (lane == 0) {
          const unsigned long long j = atomicAdd(&a.big[0], 1ull);
          if (j < a.big_cap) {  // (always: the list is sized to the counted long traces)
            a.big_list[2 * j] = t_cur;
            a.big_list[2 * j + 1] = atomicAdd(&a.big[1], (unsigned long long)cur.n);
          }
        }
      } else {
        self_chunk<SCAN>(wsm, lane, cur, R, a);
      }
      if (!has_next) break;
      cur = nxt;
      t_cur = t_nxt;
      R = Rn;
    }
  };
  // As the edge kernel: a static share per wave, then the last 1 / kDyn of
  // the traces in segments of kDynSeg from a global counter.
  constexpr uint64_t kDyn = 4, kDynSeg = 512;
  const uint64_t n_static = n_traces - n_traces / kDyn;
  uint64_t t_begin = uniform64(n_static * gw / nw);
  uint64_t t_end = uniform64(n_static * (gw + 1) / nw);
  while (true) {
    if (t_begin < t_end) run(t_begin, t_end);
    if (n_static == n_traces) break;
    unsigned long long g = 0;
    if (lane == 0) g = atomicAdd(a.ctr, (unsigned long long)kDynSeg);
    g = __shfl(g, 0);
    t_begin = uniform64(n_static + g);
    if (t_begin >= n_traces) break;
    t_end = uniform64(t_begin + kDynSeg < n_traces ? t_begin + kDynSeg : n_traces);
  }
}

// ---- long traces ----------------------------------------------------------
// Traces and spans of the set that outgrow a chunk: cnt[0] traces, cnt[1]
// spans (sizes the list and the child-sum scratch before the walk).
__global__ __launch_bounds__(256) void self_long_count_kernel(const uint64_t* __restrict__ trace_ptr,
                                                              uint64_t n_traces,
                                                              unsigned long long* __restrict__ cnt) {
  unsigned long long nt = 0, ns = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n_traces;
       t += (uint64_t)gridDim.x * 256) {
    const uint64_t L = trace_ptr[t + 1] - trace_ptr[t];
    if (L > (uint64_t)kStage) {
      nt += 1;
      ns += L;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    nt += __shfl_xor(nt, o);
    ns += __shfl_xor(ns, o);
  }
  if ((threadIdx.x & 63) == 0 && nt) {
    atomicAdd(&cnt[0], nt);
    atomicAdd(&cnt[1], ns);
  }
}

// One workgroup per listed trace.  Parent positions come from an LDS hash
// table over a window of kBigWin ids (id -> first position in the window):
// a block of kBigThreads * kBigPer spans probes the trace's windows in trace
// order, so the first window holding an id gives its first occurrence —
// ceil(L / block) * ceil(L / kBigWin) window builds of kBigWin inserts each,
// O(L^2 / block) LDS inserts for a trace of L spans.  Child sums go to the
// u64 scratch by global atomics, the spans' records hold (row, error,
// dur_us) meanwhile, and a final sweep by the same threads turns dur_us into
// self_us.
constexpr int kBigThreads = 512;
constexpr int kBigPer = 8;
constexpr uint32_t kBigWin = 2048;
constexpr uint32_t kBigSlots = 2 * kBigWin;  // load <= 1/2
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert((kBigSlots & (kBigSlots - 1)) == 0, "power-of-two table");

__device__ __forceinline__ uint32_t big_slot(uint64_t id) {
  return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32) & (kBigSlots - 1u);
}

__global__ __launch_bounds__(kBigThreads) void self_big_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ trace_ptr, SelfArgs a) {
  __shared__ unsigned long long bkey[kBigSlots];  // 0 = empty (id 0 is never a parent reference)
  __shared__ uint32_t bpos[kBigSlots];            // first position in the window
  __shared__ unsigned long long s_j;
  const int tid = threadIdx.x;
  const uint64_t nbig = a.big[0] < a.big_cap ? a.big[0] : a.big_cap;
  const uint32_t S = a.S;
  for (uint32_t k = tid; k < kBigSlots; k += kBigThreads) {
    bkey[k] = 0ull;
    bpos[k] = kNone;
  }
  while (true) {
    __syncthreads();
    if (tid == 0) s_j = atomicAdd(&a.big[2], 1ull);
    __syncthreads();
    const uint64_t j = s_j;
    if (j >= nbig) break;
    const uint64_t t = a.big_list[2 * j];
    unsigned long long* csum = a.csum + a.big_list[2 * j + 1];
    const uint64_t lo = trace_ptr[t];
    const uint32_t L = (uint32_t)(trace_ptr[t + 1] - lo);  // the call takes < 2^32 spans
    for (uint32_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
      uint64_t pid[kBigPer];
      uint32_t pp[kBigPer];  // parent position in the trace (kNone: not found yet)
      bool need = false;
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint32_t i = b0 + (uint32_t)r * kBigThreads + tid;
        pid[r] = i < L ? parent[lo + i] : 0ull;
        pp[r] = kNone;
        need |= pid[r] != 0ull;
      }
      for (uint32_t w0 = 0; w0 < L; w0 += kBigWin) {
        if (!__syncthreads_or(need)) break;  // also orders the previous clear
        for (uint32_t k = tid; k < kBigWin && w0 + k < L; k += kBigThreads) {
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
        for (uint32_t k = tid; k < kBigSlots; k += kBigThreads) {
          bkey[k] = 0ull;
          bpos[k] = kNone;
        }
      }
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint32_t i = b0 + (uint32_t)r * kBigThreads + tid;
        if (i >= L) continue;
        const uint32_t sf = svcfl[lo + i], d = dur[lo + i];
        uint32_t p = S;
        if (pid[r] != 0ull) {
          p = S + 1u;
          if (pp[r] != kNone) {
            p = svcfl[lo + pp[r]] & 0xFFFFu;
            if (pp[r] != i) atomicAdd(&csum[pp[r]], (unsigned long long)d);
          }
        }
        a.rec[lo + i] = make_rec(p, S, sf, d);
      }
    }
    // every child sum of the trace landed (this workgroup made all of them)
    __threadfence();
    __syncthreads();
    for (uint32_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint32_t i = b0 + (uint32_t)r * kBigThreads + tid;
        if (i >= L) continue;
        const unsigned long long x = a.rec[lo + i];  // this thread's own store
        const unsigned long long cs =
            __hip_atomic_load(&csum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t d = (uint32_t)x;
        const uint32_t self = d - (cs < (unsigned long long)d ? (uint32_t)cs : d);
        a.rec[lo + i] = (x & 0xFFFFFFFF00000000ull) | self;
        if (a.self_us) a.self_us[lo + i] = self;
      }
    }
  }
}

using WalkFn = void (*)(const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                        const uint64_t*, uint64_t, SelfArgs);

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_edge_self_time_spans(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S,
                                anomod_edge_table* out, uint32_t* self_us) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_edge_self_time_spans: NULL argument");
  // As anomod_edge_aggregate_spans: what can fail on one rank only feeds the
  // status agreement (the table is merged over an attached communicator).
  int local = ANOMOD_OK;
  ANOMOD_CHECK_LOCAL(ctx, local, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_CHECK_LOCAL(ctx, local, out->n_services == S, "out->n_services=%u != n_services=%u",
                     out->n_services, S);
  ANOMOD_CHECK_LOCAL(ctx, local, out->n_bins == ANOMOD_HIST_BINS,
                     "out->n_bins=%u != ANOMOD_HIST_BINS=%u", out->n_bins,
                     (unsigned)ANOMOD_HIST_BINS);
  ANOMOD_CHECK_LOCAL(ctx, local, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_CHECK_LOCAL(ctx, local, spans->n_spans == 0 || spans->max_svc < S,
                     "span service index %u >= n_services %u", spans->max_svc, S);
  ANOMOD_CHECK_LOCAL(ctx, local, spans->n_spans < max_launch_spans(),
                     "%llu spans: at most 2^32 - 2 per call", (unsigned long long)spans->n_spans);
  if (local == ANOMOD_OK && !spans->grouped) {
    set_error(ctx, "span set is not grouped by trace: anomod_spans_group first");
    local = ANOMOD_ESTATE;
  }
  if (local == ANOMOD_OK) local = bind(ctx);
  if (int rc = comm_agree(ctx, local)) return rc;

  const uint64_t n = spans->n_spans, nt = spans->n_traces;
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  // the spans that lie in traces: [trace_ptr[0], trace_ptr[n_traces]) (an
  // upload may leave spans outside every trace: they are on no edge and their
  // self_us reads 0)
  uint64_t in_traces[2] = {0, 0};
  if (nt && n) {
    ANOMOD_HIP(ctx, hipMemcpyAsync(in_traces, spans->trace_ptr, 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
    ANOMOD_HIP(ctx, hipMemcpyAsync(in_traces + 1, spans->trace_ptr + nt, 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
    ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!(in_traces[0] <= in_traces[1] && in_traces[1] <= n)) {
      set_error(ctx, "trace_ptr range [%llu, %llu) outside the set's %llu spans",
                (unsigned long long)in_traces[0], (unsigned long long)in_traces[1],
                (unsigned long long)n);
      in_traces[0] = in_traces[1] = 0;
      local = ANOMOD_EINVAL;
    }
  }
  const uint64_t n_rec = in_traces[1] - in_traces[0];

  // The call's workspace, freed when it returns (after the stream's work):
  // a block of words (dynamic-tail counter, long-trace counters, order-probe
  // scratch, long-trace count) and a block of records | self_us (when asked
  // for) | long-trace list | child sums of the listed spans.  The long traces
  // are counted first (one small kernel and a host wait, skipped when the
  // set's longest trace is known to fit a chunk), so the list and the child
  // sums are sized to them.
  struct Workspace {
    anomod_ctx* ctx;
    void* words = nullptr;
    void* block = nullptr;
    ~Workspace() {
      if (!words && !block) return;
      (void)hipStreamSynchronize(ctx->stream);
      if (words) (void)hipFree(words);
      if (block) (void)hipFree(block);
    }
  } ws{ctx};
  auto take = [&](void** p, size_t bytes) {
    if (dev_malloc(ctx, p, bytes) == hipSuccess) return ANOMOD_OK;
    (void)hipGetLastError();
    *p = nullptr;
    set_error(ctx, "hipMalloc(%zu) for the self-time workspace failed", bytes);
    return ANOMOD_ENOMEM;
  };
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  unsigned long long nlong[2] = {0ull, 0ull};
  if (local == ANOMOD_OK && n_rec) local = take(&ws.words, 256);
  if (local == ANOMOD_OK && n_rec && spans->max_trace_len > (uint64_t)kStage) {
    auto* cnt = static_cast<unsigned long long*>(ws.words);
    ANOMOD_HIP(ctx, hipMemsetAsync(cnt, 0, 16, ctx->stream));
    hipLaunchKernelGGL(self_long_count_kernel,
                       dim3((unsigned)std::min<uint64_t>((nt + 255) / 256, 4ull * ctx->num_cus)),
                       dim3(256), 0, ctx->stream, spans->trace_ptr, nt, cnt);
    ANOMOD_HIP(ctx, hipGetLastError());
    ANOMOD_HIP(ctx, hipMemcpyAsync(nlong, cnt, 16, hipMemcpyDeviceToHost, ctx->stream));
    ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  const size_t b_rec = al(n * 8), b_self = self_us ? al(n * 4) : 0;
  const size_t b_list = al(nlong[0] * 16), b_csum = al(nlong[1] * 8);
  if (local == ANOMOD_OK && n_rec) local = take(&ws.block, b_rec + b_self + b_list + b_csum);
  if (int rc = comm_agree(ctx, local)) return rc;

  SelfArgs a{};
  if (n_rec) {
    auto* words = static_cast<unsigned long long*>(ws.words);
    char* w = static_cast<char*>(ws.block);
    a.rec = reinterpret_cast<unsigned long long*>(w);
    a.self_us = self_us ? reinterpret_cast<uint32_t*>(w + b_rec) : nullptr;
    a.ctr = words;
    a.big = words + 1;
    a.big_list = reinterpret_cast<unsigned long long*>(w + b_rec + b_self);
    a.big_cap = nlong[0];
    a.csum = reinterpret_cast<unsigned long long*>(w + b_rec + b_self + b_list);
    a.S = S;
    // The scan the edge kernels would use for the set (its order hint is
    // probed when unknown: the value the first aggregation would find).
    bool uni = false;
    if (int rc = span_scan_choice(ctx, spans, words + 4, &uni)) return rc;
    const bool long_set = spans->max_trace_len != ~0ull && spans->max_trace_len > (uint64_t)kStage;
    const int scan = !uni ? kScanFwd : (E > kNarrowRows || long_set) ? kScanSplit : kScanBidir;
    const WalkFn fn = scan == kScanFwd     ? self_time_kernel<kScanFwd>
                      : scan == kScanSplit ? self_time_kernel<kScanSplit>
                                           : self_time_kernel<kScanBidir>;
    int per_cu = 0;
    ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                        &per_cu, reinterpret_cast<const void*>(fn), kSelfThreads, 0));
    const uint64_t grid = (uint64_t)ctx->num_cus * (uint64_t)(per_cu > 0 ? per_cu : 1);
    if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests)
      fprintf(stderr, "anomod: self-time kernel self_time_kernel<%s>, %llu long traces\n",
              scan == kScanFwd ? "forward" : scan == kScanSplit ? "split" : "bidir", nlong[0]);
    ANOMOD_HIP(ctx, hipMemsetAsync(words, 0, 32, ctx->stream));  // ctr + big counters
    if (nlong[1]) ANOMOD_HIP(ctx, hipMemsetAsync(a.csum, 0, nlong[1] * 8, ctx->stream));
    if (a.self_us && n_rec < n) ANOMOD_HIP(ctx, hipMemsetAsync(a.self_us, 0, n * 4, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kSelfThreads), 0, ctx->stream, spans->span_id,
                       spans->parent_span_id, spans->svc_flags, spans->dur_us, spans->trace_ptr, nt,
                       a);
    ANOMOD_HIP(ctx, hipGetLastError());
    if (nlong[0]) {
      hipLaunchKernelGGL(self_big_kernel,
                         dim3((unsigned)std::min<uint64_t>(nlong[0], 2ull * ctx->num_cus)),
                         dim3(kBigThreads), 0, ctx->stream, spans->span_id, spans->parent_span_id,
                         spans->svc_flags, spans->dur_us, spans->trace_ptr, a);
      ANOMOD_HIP(ctx, hipGetLastError());
    }
  }
  // The table of the records.  The self-time distribution is not the
  // durations': the set's histogram-form hint is neither read nor touched
  // (form unknown: the compact form, which has nothing to saturate).
  int8_t form = -1;
  if (int rc = edge_aggregate_records(
          ctx, n_rec ? reinterpret_cast<const uint64_t*>(a.rec + in_traces[0]) : nullptr, n_rec, S,
          &form, out))
    return rc;
  if (self_us && n) {
    if (n_rec) {
      ANOMOD_HIP(ctx, hipMemcpyAsync(self_us, a.self_us, n * 4, hipMemcpyDeviceToHost, ctx->stream));
      ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else {
      memset(self_us, 0, n * 4);
    }
  }
  return ANOMOD_OK;
}

}  // extern "C"
