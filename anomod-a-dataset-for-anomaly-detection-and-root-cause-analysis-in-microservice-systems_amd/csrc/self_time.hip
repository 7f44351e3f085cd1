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
// One chunk walk (walk.h: persistent waves, <= 256 spans / <= 64 whole
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

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kSelfWaves = 8;
constexpr int kSelfThreads = kSelfWaves * kWave;

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
      const int q = find_parent<SCAN>(lsid, llo, lhi, ta, tb, i, R.pid[r]);
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
    a.rec[c.base + i] = edge_rec(row[r], a.S, R.sf[r], self);
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
  unsigned char* wsm = smem + (threadIdx.x / kWave) * kSBytes;
  walk_traces<kSelfWaves, 4, Regs>(
      trace_ptr, n_traces, a.ctr,
      [&](const Chunk& c, Regs& R) __attribute__((always_inline)) {
        load_regs(span_id, parent, svcfl, dur, c, lane, R);
      },
      [&](const Chunk& c, uint32_t, uint64_t, const Regs& R) __attribute__((always_inline)) {
        self_chunk<SCAN>(wsm, lane, c, R, a);
      },
      // longer than kStage: listed for self_big_kernel
      [&](uint64_t t, uint32_t n) __attribute__((always_inline)) {
        list_long(a.big, a.big_list, a.big_cap, lane, t, n);
      });
}

// ---- long traces ----------------------------------------------------------
// One workgroup per listed trace.  Parent positions come from walk.h's
// windowed LDS id table (big_parents).  Child sums go to the u64 scratch by
// global atomics, the spans' records hold (row, error, dur_us) meanwhile, and
// a final sweep by the same threads turns dur_us into self_us.
__global__ __launch_bounds__(kBigThreads) void self_big_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ trace_ptr, SelfArgs a) {
  __shared__ unsigned long long bkey[kBigSlots];
  __shared__ uint32_t bpos[kBigSlots];
  __shared__ unsigned long long s_j;
  const int tid = threadIdx.x;
  const uint64_t nbig = a.big[0] < a.big_cap ? a.big[0] : a.big_cap;
  const uint32_t S = a.S;
  big_clear(bkey, bpos, tid);
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
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
      uint64_t pid[kBigPer];
      uint32_t pp[kBigPer];  // parent position in the trace (kNone: none)
      big_parents(span_id, parent, lo, L, b0, tid, bkey, bpos, pid, pp);
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
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
        a.rec[lo + i] = edge_rec(p, S, sf, d);
      }
    }
    // every child sum of the trace landed (this workgroup made all of them)
    __threadfence();
    __syncthreads();
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
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
  // the spans that lie in traces (an upload may leave spans outside every
  // trace: they are on no edge and their self_us reads 0)
  uint64_t in_traces[2];
  local = trace_span_range(ctx, spans, in_traces);
  if (local != ANOMOD_OK && local != ANOMOD_EINVAL) return local;
  const uint64_t n_rec = in_traces[1] - in_traces[0];

  // The call's workspace: a block of words (dynamic-tail counter, long-trace
  // counters, order-probe scratch, long-trace count) and a block of records |
  // self_us (when asked for) | long-trace list | child sums of the listed
  // spans.  The long traces are counted first, so the list and the child sums
  // are sized to them.
  CallWorkspace ws{ctx};
  const auto al = CallWorkspace::al;
  unsigned long long nlong[2] = {0ull, 0ull};
  if (local == ANOMOD_OK && n_rec) local = ws.take(&ws.words, 256, "self-time");
  auto* words = static_cast<unsigned long long*>(ws.words);
  if (local == ANOMOD_OK && n_rec)
    if (int rc = count_long_traces(ctx, spans, words, nlong)) return rc;
  const size_t b_rec = al(n * 8), b_self = self_us ? al(n * 4) : 0;
  const size_t b_list = al(nlong[0] * 16), b_csum = al(nlong[1] * 8);
  if (local == ANOMOD_OK && n_rec)
    local = ws.take(&ws.block, b_rec + b_self + b_list + b_csum, "self-time");
  if (int rc = comm_agree(ctx, local)) return rc;

  SelfArgs a{};
  if (n_rec) {
    a.rec = ws.carve<unsigned long long>(b_rec);
    a.self_us = self_us ? ws.carve<uint32_t>(b_self) : nullptr;
    a.big_list = ws.carve<unsigned long long>(b_list);
    a.csum = ws.carve<unsigned long long>(b_csum);
    a.ctr = words;
    a.big = words + 1;
    a.big_cap = nlong[0];
    a.S = S;
    int scan = kScanFwd;
    if (int rc = pick_walk_scan(ctx, spans, S, words + 4, &scan)) return rc;
    const WalkFn fn = scan == kScanFwd     ? self_time_kernel<kScanFwd>
                      : scan == kScanSplit ? self_time_kernel<kScanSplit>
                                           : self_time_kernel<kScanBidir>;
    uint64_t grid = 0;
    if (int rc = walk_grid(ctx, fn, kSelfThreads, &grid)) return rc;
    log_walk_kernel("self-time", "self_time_kernel", scan, nlong[0]);
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
