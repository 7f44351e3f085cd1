// Call transit of a grouped span set: the time between two services.  For a
// call whose parent span made no other call (a client / exit span and the
// callee's server / entry span), the request gap from the parent's start to
// the call's start and the response gap from the call's end to the parent's.
//
//   s(i), e(i) = start_us[i], start_us[i] + dur_us[i] (u64, saturating)
//   par(i)     = self time's parent (self_time.hip): the first span of i's
//                trace, in position order, whose span_id equals i's
//                parent_span_id; a root, an orphan and a self-reference have
//                none
//   kids(j)    = the spans i with par(i) = j
//   a call c with p = par(c) is paired iff kids(p) == 1; its row is svc[p] * S
//   + svc[c].  Untimed (a start of 0 on either side): counted, nothing else.
//   Else s(c) >= s(p) gives a request record min(s(c) - s(p), 2^32 - 1), an
//   earlier start an early count; e(c) <= e(p) gives a response record
//   min(e(p) - e(c), 2^32 - 1), a later end a late count.
//
// One chunk walk (walk.h: persistent waves, <= 256 spans / <= 64 whole traces
// per chunk, buffer loads, the columns of chunk c+1 in flight while chunk c is
// resolved) reads 32 B per span (id 8, parent id 8, svc|flags 4, duration 4,
// start 8), stages ids, services, starts and durations in the wave's LDS,
// finds every span's parent *position*, keeps it in a register and adds 1 to
// the parent's u32 kids slot (ds_add).  After a wave sync a span whose
// parent's slot reads 1 takes the parent's start and duration from LDS, and
// every position writes two records in the form edge_aggregate_records takes
// (kSkipRec where nothing is recorded).  The two tables — histogram, finalize,
// the merge over an attached communicator — are that call's, unchanged.
//
// Row counters (untimed, early, late and the two sums of microseconds) are
// privatised per workgroup in a sparse LDS table of (kind * E + row, count,
// microseconds) slots, claimed by ds_cmpst, probed linearly and flushed once
// with u64 global adds; a u32 word that wraps carries 2^32 into the global
// word at once, and an add that finds no slot in kSpProbes steps goes to the
// global words itself.  One skewed host pair makes every call of a row early:
// a global atomic per event would serialise on that row's word (DESIGN.md
// §2.23).  calls and paired are per-lane counts, summed per wave, one global
// add per wave.
//
// Traces longer than a chunk are listed by the walk and resolved by
// call_transit_big_kernel, one workgroup per listed trace.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kTrWaves = 4;
constexpr int kTrThreads = kTrWaves * kWave;

// Per-wave LDS (every offset a multiple of 16).
constexpr int kTSid = 0;  // u64 span ids [kStage + kScanSlack], or two u32 planes of that length
constexpr int kTSt = kTSid + (kStage + (int)kScanSlack) * 8;  // u64 starts [kStage]
constexpr int kTDur = kTSt + kStage * 8;                      // u32 durations [kStage]
constexpr int kTKid = kTDur + kStage * 4;                     // u32 kids [kStage]
constexpr int kTSvc = kTKid + kStage * 4;                     // u16 services [kStage]
constexpr int kTFlag = kTSvc + kStage * 2;                    // u8 trace-start flags [kStage]
constexpr int kTBytes = kTFlag + kStage;
static_assert(kTSt % 16 == 0 && kTDur % 16 == 0 && kTKid % 16 == 0 && kTBytes % 16 == 0,
              "wave staging must stay 16-B aligned");

// The sparse counters: slot key = kind * E + row (< 3 E < 2^32 - 1).
constexpr uint32_t kSpSlots = 512, kSpProbes = 16, kSpEmpty = 0xFFFFFFFFu;
static_assert(kSpSlots == 1u << 9, "row_add takes the top 9 bits of its hash");
enum { kKUntimed, kKEarly, kKLate, kKinds };
constexpr uint32_t kTabs = 5;  // u64 [E] each: untimed | early | late | early_us | late_us
constexpr uint32_t kUsTab = 2;  // the microseconds of kind k (early, late) are table k + kUsTab
static_assert(4 * (kTBytes * kTrWaves + (int)kSpSlots * 12) <= 160 * 1024, "LDS of a CU");

constexpr uint32_t kMaxGap = 0xFFFFFFFFu;
constexpr uint32_t kStCall = ANOMOD_TRANSIT_CALL, kStPaired = ANOMOD_TRANSIT_PAIRED,
                   kStTimed = ANOMOD_TRANSIT_TIMED, kStEarly = ANOMOD_TRANSIT_EARLY,
                   kStLate = ANOMOD_TRANSIT_LATE;

struct TrArgs {
  unsigned long long* req;       // [n_spans] request records by span position (kSkipRec: none)
  unsigned long long* resp;      // [n_spans] response records
  uint32_t* req_us;              // [n_spans] or NULL
  uint32_t* resp_us;             // [n_spans] or NULL
  uint8_t* state;                // [n_spans] or NULL
  unsigned long long* ctr;       // trace-segment counter of the dynamic tail
  unsigned long long* big;       // [0] listed traces, [1] their spans, [2] ticket
  unsigned long long* total;     // [0] calls, [1] paired
  unsigned long long* tab;       // u64 [kTabs][E] (zeroed)
  unsigned long long* big_list;  // (trace, scratch offset) per listed trace
  uint64_t big_cap;              // entries big_list holds
  uint32_t* l_kids;              // [long spans] kids (zeroed)
  uint32_t* l_par;               // [long spans] parent position in the trace (kNone: none)
  uint32_t S, E;
};

// A workgroup's sparse counters.
struct Counters {
  uint32_t* key;  // [kSpSlots] kind * E + row (kSpEmpty: free)
  uint32_t* cnt;  // [kSpSlots] events
  uint32_t* us;   // [kSpSlots] their microseconds
};

// One event of `kind` on `row`, `us` microseconds of it (0 for kUntimed).
__device__ __forceinline__ void row_add(const TrArgs& a, const Counters& C, uint32_t kind,
                                        uint32_t row, uint32_t us) {
  const uint32_t idx = kind * a.E + row;
  uint32_t sl = (idx * 0x9E3779B1u) >> 23 & (kSpSlots - 1u);
#pragma nounroll  // (unrolled, every probe's exec mask is live at once: hundreds of SGPR spills)
  for (uint32_t p = 0; p < kSpProbes; ++p, sl = (sl + 1u) & (kSpSlots - 1u)) {
    const uint32_t seen = atomicCAS(&C.key[sl], kSpEmpty, idx);
    if (seen == kSpEmpty || seen == idx) {
      const uint32_t c0 = atomicAdd(&C.cnt[sl], 1u);
      if (c0 + 1u < c0) atomicAdd(&a.tab[idx], 1ull << 32);
      if (us) {
        const uint32_t u0 = atomicAdd(&C.us[sl], us);
        if (u0 + us < u0) atomicAdd(&a.tab[idx + kUsTab * a.E], 1ull << 32);
      }
      return;
    }
  }
  atomicAdd(&a.tab[idx], 1ull);
  if (us) atomicAdd(&a.tab[idx + kUsTab * a.E], (unsigned long long)us);
}

// The workgroup's counters: cleared (a barrier orders it before the first
// add), and flushed into the global tables (after a barrier).
__device__ __forceinline__ void clear_counters(const Counters& C, int threads) {
  for (uint32_t k = threadIdx.x; k < kSpSlots; k += threads) {
    C.key[k] = kSpEmpty;
    C.cnt[k] = 0u;
    C.us[k] = 0u;
  }
}
__device__ __forceinline__ void flush_counters(const TrArgs& a, const Counters& C, int threads) {
  for (uint32_t k = threadIdx.x; k < kSpSlots; k += threads) {
    const uint32_t idx = C.key[k];
    if (idx == kSpEmpty) continue;
    if (C.cnt[k]) atomicAdd(&a.tab[idx], (unsigned long long)C.cnt[k]);
    if (C.us[k]) atomicAdd(&a.tab[idx + kUsTab * a.E], (unsigned long long)C.us[k]);
  }
}

// This lane's calls and paired calls into the wave's sum, one global add each
// per wave.  (A lane counts spans of one call: < 2^32.)
__device__ __forceinline__ void add_totals(const TrArgs& a, int lane, uint32_t calls,
                                           uint32_t paired) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    calls += __shfl_xor(calls, d);
    paired += __shfl_xor(paired, d);
  }
  if (lane == 0) {
    if (calls) atomicAdd(&a.total[0], (unsigned long long)calls);
    if (paired) atomicAdd(&a.total[1], (unsigned long long)paired);
  }
}

__device__ __forceinline__ uint64_t end_sat(uint64_t s, uint32_t d) {
  const uint64_t e = s + d;
  return e < s ? ~0ull : e;
}
__device__ __forceinline__ uint32_t clamp_gap(uint64_t g) {
  return g < (uint64_t)kMaxGap ? (uint32_t)g : kMaxGap;
}

// What one paired call (cs, cd) of parent (ps, pd) records and counts on `row`
// = parent service * S + service; prow is the parent's service.
struct Transit {
  unsigned long long req, resp;  // records (kSkipRec: none)
  uint32_t req_us, resp_us, state;
};
__device__ __forceinline__ void paired_call(const TrArgs& a, const Counters& C, uint32_t prow,
                                            uint32_t sf, uint64_t ps, uint32_t pd, uint64_t cs,
                                            uint32_t cd, Transit& t) {
  const uint32_t row = prow * a.S + (sf & 0xFFFFu);
  if (cs == 0ull || ps == 0ull) {
    row_add(a, C, kKUntimed, row, 0u);
    return;
  }
  t.state |= kStTimed;
  if (cs >= ps) {
    t.req_us = clamp_gap(cs - ps);
    t.req = edge_rec(prow, a.S, sf, t.req_us);
  } else {
    t.state |= kStEarly;
    row_add(a, C, kKEarly, row, clamp_gap(ps - cs));
  }
  const uint64_t ec = end_sat(cs, cd), ep = end_sat(ps, pd);
  if (ec <= ep) {
    t.resp_us = clamp_gap(ep - ec);
    t.resp = edge_rec(prow, a.S, sf, t.resp_us);
  } else {
    t.state |= kStLate;
    row_add(a, C, kKLate, row, clamp_gap(ec - ep));
  }
}

struct Regs {
  uint64_t sid[kPer], pid[kPer], st[kPer];
  uint32_t dur[kPer], sf[kPer];  // sf = svc | flags << 16
};

__device__ __forceinline__ void load_regs(const uint64_t* __restrict__ span_id,
                                          const uint64_t* __restrict__ parent,
                                          const uint32_t* __restrict__ svcfl,
                                          const uint32_t* __restrict__ dur,
                                          const uint64_t* __restrict__ start_us, const Chunk& c,
                                          int lane, Regs& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by call_transit_big_kernel
  const auto rsid = rsrc(span_id + c.base, n * 8u);
  const auto rpid = rsrc(parent + c.base, n * 8u);
  const auto rst = rsrc(start_us + c.base, n * 8u);
  const auto rsf = rsrc(svcfl + c.base, n * 4u);
  const auto rdur = rsrc(dur + c.base, n * 4u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.sid[r] = bload64(rsid, i * 8u);
    R.pid[r] = bload64(rpid, i * 8u);
    R.st[r] = bload64(rst, i * 8u);
    R.sf[r] = bload32(rsf, i * 4u);
    R.dur[r] = bload32(rdur, i * 4u);
  }
}

template <int SCAN>
__device__ __forceinline__ void transit_chunk(unsigned char* wsm, const Counters& C, int lane,
                                              const Chunk& c, const Regs& R, const TrArgs& a,
                                              uint32_t& calls, uint32_t& paired) {
  auto* lsid = reinterpret_cast<uint64_t*>(wsm + kTSid);
  auto* llo = reinterpret_cast<uint32_t*>(wsm + kTSid);
  uint32_t* lhi = llo + (kStage + kScanSlack);
  auto* lst = reinterpret_cast<uint64_t*>(wsm + kTSt);
  auto* ldur = reinterpret_cast<uint32_t*>(wsm + kTDur);
  auto* lkid = reinterpret_cast<uint32_t*>(wsm + kTKid);
  auto* lsvc = reinterpret_cast<uint16_t*>(wsm + kTSvc);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kTFlag);
  // Stage ids, services, starts and durations (lanes past n hold zeros from
  // the buffer loads), clear the kids.
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
    lst[i] = R.st[r];
    ldur[i] = R.dur[r];
    lkid[i] = 0u;
  }
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);  // (its wave syncs also publish the staging)
  uint32_t par[kPer];  // parent position in the chunk (kNone: none)
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    par[r] = kNone;
    if (i < c.n && R.pid[r] != 0ull) {
      uint32_t ta, tb;
      trace_bounds(Sm, r, lane, c.n, ta, tb);
      const int q = find_parent<SCAN>(lsid, llo, lhi, ta, tb, i, R.pid[r]);
      if (q >= 0 && (uint32_t)q != i) {  // a span is not its own call
        par[r] = (uint32_t)q;
        atomicAdd(&lkid[q], 1u);
      }
    }
  }
  wave_sync();
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if (i >= c.n) continue;
    Transit t{kSkipRec, kSkipRec, 0u, 0u, 0u};
    if (par[r] != kNone) {
      t.state = kStCall;
      ++calls;
      const uint32_t q = par[r];
      if (lkid[q] == 1u) {
        t.state |= kStPaired;
        ++paired;
        paired_call(a, C, lsvc[q], R.sf[r], lst[q], ldur[q], R.st[r], R.dur[r], t);
      }
    }
    a.req[c.base + i] = t.req;
    a.resp[c.base + i] = t.resp;
    if (a.req_us) a.req_us[c.base + i] = t.req_us;
    if (a.resp_us) a.resp_us[c.base + i] = t.resp_us;
    if (a.state) a.state[c.base + i] = (uint8_t)t.state;
  }
  wave_sync();  // the staging area is free for the next chunk
}

template <int SCAN>
__global__ __launch_bounds__(kTrThreads) void call_transit_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ start_us, const uint64_t* __restrict__ trace_ptr,
    uint64_t n_traces, TrArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kTBytes * kTrWaves];
  __shared__ uint32_t sp_key[kSpSlots], sp_cnt[kSpSlots], sp_us[kSpSlots];
  const int lane = threadIdx.x & (kWave - 1);
  unsigned char* wsm = smem + (threadIdx.x / kWave) * kTBytes;
  const Counters C{sp_key, sp_cnt, sp_us};
  clear_counters(C, kTrThreads);
  __syncthreads();
  uint32_t calls = 0u, paired = 0u;
  walk_traces<kTrWaves, 4, Regs>(
      trace_ptr, n_traces, a.ctr,
      [&](const Chunk& c, Regs& R) __attribute__((always_inline)) {
        load_regs(span_id, parent, svcfl, dur, start_us, c, lane, R);
      },
      [&](const Chunk& c, uint32_t, uint64_t, const Regs& R) __attribute__((always_inline)) {
        transit_chunk<SCAN>(wsm, C, lane, c, R, a, calls, paired);
      },
      // longer than kStage: listed for call_transit_big_kernel
      [&](uint64_t t, uint32_t n) __attribute__((always_inline)) {
        list_long(a.big, a.big_list, a.big_cap, lane, t, n);
      });
  add_totals(a, lane, calls, paired);
  __syncthreads();
  flush_counters(a, C, kTrThreads);
}

// ---- long traces ----------------------------------------------------------
// One workgroup per listed trace (tickets).  Parent positions come from
// walk.h's windowed LDS id table (big_parents); a first sweep keeps each
// span's parent position in the u32 scratch (read back by its owner: plain
// stores and loads) and adds 1 to the parent's u32 kids word by an agent-scope
// atomic — a star of 66,000 spans puts more than 2^16 on one word.  After the
// sweep barrier (sweep_sync) a second sweep by the same threads reads the kids
// (agent-scope loads, served by L2) and the parent's columns from global
// memory and writes the records.
__global__ __launch_bounds__(kBigThreads) void call_transit_big_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ start_us, const uint64_t* __restrict__ trace_ptr, TrArgs a) {
  __shared__ unsigned long long bkey[kBigSlots];
  __shared__ uint32_t bpos[kBigSlots];
  __shared__ unsigned long long s_j;
  __shared__ uint32_t sp_key[kSpSlots], sp_cnt[kSpSlots], sp_us[kSpSlots];
  const int tid = threadIdx.x;
  const uint64_t nbig = a.big[0] < a.big_cap ? a.big[0] : a.big_cap;
  const Counters C{sp_key, sp_cnt, sp_us};  // (the loop's first barrier orders the clear)
  clear_counters(C, kBigThreads);
  big_clear(bkey, bpos, tid);
  uint32_t calls = 0u, paired = 0u;
  while (true) {
    __syncthreads();
    if (tid == 0) s_j = atomicAdd(&a.big[2], 1ull);
    __syncthreads();
    const uint64_t j = s_j;
    if (j >= nbig) break;
    const uint64_t t = a.big_list[2 * j];
    const uint64_t off = a.big_list[2 * j + 1];
    const uint64_t lo = trace_ptr[t];
    const uint32_t L = (uint32_t)(trace_ptr[t + 1] - lo);  // the call takes < 2^32 spans
    uint32_t* kids = a.l_kids + off;
    uint32_t* lpar = a.l_par + off;
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
      uint64_t pid[kBigPer];
      uint32_t pp[kBigPer];  // parent position in the trace (kNone: none)
      big_parents(span_id, parent, lo, L, b0, tid, bkey, bpos, pid, pp);
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
        if (i >= L) continue;
        const uint32_t q = pp[r] == (uint32_t)i ? kNone : pp[r];  // a span is not its own call
        lpar[i] = q;
        if (q != kNone)
          __hip_atomic_fetch_add(&kids[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // every kids word of the trace landed (this workgroup made all of them)
    sweep_sync();
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
        if (i >= L) continue;
        const uint32_t q = lpar[i];  // this thread's own store
        Transit tr{kSkipRec, kSkipRec, 0u, 0u, 0u};
        if (q != kNone) {
          tr.state = kStCall;
          ++calls;
          if (aload(&kids[q]) == 1u) {
            tr.state |= kStPaired;
            ++paired;
            paired_call(a, C, svcfl[lo + q] & 0xFFFFu, svcfl[lo + i], start_us[lo + q],
                        dur[lo + q], start_us[lo + i], dur[lo + i], tr);
          }
        }
        a.req[lo + i] = tr.req;
        a.resp[lo + i] = tr.resp;
        if (a.req_us) a.req_us[lo + i] = tr.req_us;
        if (a.resp_us) a.resp_us[lo + i] = tr.resp_us;
        if (a.state) a.state[lo + i] = (uint8_t)tr.state;
      }
    }
  }
  add_totals(a, tid & (kWave - 1), calls, paired);
  __syncthreads();
  flush_counters(a, C, kBigThreads);
}

using WalkFn = void (*)(const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                        const uint64_t*, const uint64_t*, uint64_t, TrArgs);

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_call_transit_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_call_transit* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_call_transit_spans: NULL argument");
  // As anomod_edge_critical_path_spans: what can fail on one rank only feeds
  // the status agreement (the two tables are merged over an attached
  // communicator).
  const uint32_t S = out->n_services;
  anomod_edge_table* tabs[2] = {out->request, out->response};
  int local = ANOMOD_OK;
  ANOMOD_CHECK_LOCAL(ctx, local, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_CHECK_LOCAL(ctx, local, out->request && out->response,
                     "anomod_call_transit_spans: NULL request or response table");
  for (const anomod_edge_table* t : tabs) {
    if (!t) continue;
    ANOMOD_CHECK_LOCAL(ctx, local, t->n_services == S, "table n_services=%u != n_services=%u",
                       t->n_services, S);
    ANOMOD_CHECK_LOCAL(ctx, local, t->n_bins == ANOMOD_HIST_BINS,
                       "table n_bins=%u != ANOMOD_HIST_BINS=%u", t->n_bins,
                       (unsigned)ANOMOD_HIST_BINS);
  }
  ANOMOD_CHECK_LOCAL(ctx, local, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_CHECK_LOCAL(ctx, local, spans->n_spans == 0 || spans->max_svc < S,
                     "span service index %u >= n_services %u", spans->max_svc, S);
  ANOMOD_CHECK_LOCAL(ctx, local, spans->n_spans < max_launch_spans(),
                     "%llu spans: at most 2^32 - 2 per call", (unsigned long long)spans->n_spans);
  if (local == ANOMOD_OK && !spans->grouped) {
    set_error(ctx, "span set is not grouped by trace: anomod_spans_group first");
    local = ANOMOD_ESTATE;
  }
  if (local == ANOMOD_OK && !spans->start_us) {
    set_error(ctx, "span set has no start-time column: anomod_spans_set_start_us first");
    local = ANOMOD_ESTATE;
  }
  if (local == ANOMOD_OK) local = bind(ctx);
  if (int rc = comm_agree(ctx, local)) return rc;

  const uint64_t n = spans->n_spans, nt = spans->n_traces;
  const size_t E = (size_t)(S + ANOMOD_ROOT_ROWS) * S;
  out->calls = 0;
  out->paired = 0;
  // the spans that lie in traces (spans outside every trace are no calls:
  // their columns read 0)
  uint64_t in_traces[2];
  local = trace_span_range(ctx, spans, in_traces);
  if (local != ANOMOD_OK && local != ANOMOD_EINVAL) return local;
  const uint64_t n_in = in_traces[1] - in_traces[0];

  // The call's workspace: a block of words (dynamic-tail counter, long-trace
  // counters, order-probe scratch, the two totals) and a block of the count
  // tables | request records | response records | the per-span columns (when
  // asked for) | long-trace list | the listed spans' kids and parent
  // positions.  The long traces are counted first.
  CallWorkspace ws{ctx};
  const auto al = CallWorkspace::al;
  unsigned long long nlong[2] = {0ull, 0ull};
  if (local == ANOMOD_OK && n_in) local = ws.take(&ws.words, 256, "call-transit");
  auto* words = static_cast<unsigned long long*>(ws.words);
  if (local == ANOMOD_OK && n_in)
    if (int rc = count_long_traces(ctx, spans, words, nlong)) return rc;
  const size_t nl = (size_t)nlong[1];
  const size_t tab_bytes = E * 8 * kTabs, b_tab = al(tab_bytes), b_rec = al(n * 8);
  const size_t b_rq = out->span_req_us ? al(n * 4) : 0, b_rs = out->span_resp_us ? al(n * 4) : 0;
  const size_t b_st = out->span_state ? al(n) : 0;
  const size_t b_list = al(nlong[0] * 16), b_l4 = al(nl * 4);
  if (local == ANOMOD_OK && n_in)
    local = ws.take(&ws.block, b_tab + 2 * b_rec + b_rq + b_rs + b_st + b_list + 2 * b_l4,
                    "call-transit");
  if (int rc = comm_agree(ctx, local)) return rc;

  TrArgs a{};
  if (n_in) {
    a.tab = ws.carve<unsigned long long>(b_tab);
    a.req = ws.carve<unsigned long long>(b_rec);
    a.resp = ws.carve<unsigned long long>(b_rec);
    a.req_us = b_rq ? ws.carve<uint32_t>(b_rq) : nullptr;
    a.resp_us = b_rs ? ws.carve<uint32_t>(b_rs) : nullptr;
    a.state = b_st ? ws.carve<uint8_t>(b_st) : nullptr;
    a.big_list = ws.carve<unsigned long long>(b_list);
    a.l_kids = ws.carve<uint32_t>(b_l4);
    a.l_par = ws.carve<uint32_t>(b_l4);
    a.ctr = words;
    a.big = words + 1;
    a.total = words + 8;
    a.big_cap = nlong[0];
    a.S = S;
    a.E = (uint32_t)E;
    int scan = kScanFwd;
    if (int rc = pick_walk_scan(ctx, spans, S, words + 4, &scan)) return rc;
    const WalkFn fn = scan == kScanFwd     ? call_transit_kernel<kScanFwd>
                      : scan == kScanSplit ? call_transit_kernel<kScanSplit>
                                           : call_transit_kernel<kScanBidir>;
    uint64_t grid = 0;
    if (int rc = walk_grid(ctx, fn, kTrThreads, &grid)) return rc;
    log_walk_kernel("call-transit", "call_transit_kernel", scan, nlong[0]);
    ANOMOD_HIP(ctx, hipMemsetAsync(words, 0, 32, ctx->stream));       // ctr + big counters
    ANOMOD_HIP(ctx, hipMemsetAsync(words + 8, 0, 16, ctx->stream));  // the totals
    ANOMOD_HIP(ctx, hipMemsetAsync(a.tab, 0, tab_bytes, ctx->stream));
    if (nl) ANOMOD_HIP(ctx, hipMemsetAsync(a.l_kids, 0, nl * 4, ctx->stream));
    if (n_in < n) {
      if (a.req_us) ANOMOD_HIP(ctx, hipMemsetAsync(a.req_us, 0, n * 4, ctx->stream));
      if (a.resp_us) ANOMOD_HIP(ctx, hipMemsetAsync(a.resp_us, 0, n * 4, ctx->stream));
      if (a.state) ANOMOD_HIP(ctx, hipMemsetAsync(a.state, 0, n, ctx->stream));
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kTrThreads), 0, ctx->stream, spans->span_id,
                       spans->parent_span_id, spans->svc_flags, spans->dur_us, spans->start_us,
                       spans->trace_ptr, nt, a);
    ANOMOD_HIP(ctx, hipGetLastError());
    if (nlong[0]) {
      hipLaunchKernelGGL(call_transit_big_kernel,
                         dim3((unsigned)std::min<uint64_t>(nlong[0], 2ull * ctx->num_cus)),
                         dim3(kBigThreads), 0, ctx->stream, spans->span_id, spans->parent_span_id,
                         spans->svc_flags, spans->dur_us, spans->start_us, spans->trace_ptr, a);
      ANOMOD_HIP(ctx, hipGetLastError());
    }
  }
  // The two tables of the records (the skipped ones are no records).  The
  // gaps' distribution is not the durations': the set's histogram-form hint is
  // neither read nor touched (form unknown: the compact form, which has
  // nothing to saturate).
  const unsigned long long* recs[2] = {a.req, a.resp};
  for (int k = 0; k < 2; ++k) {
    int8_t form = -1;
    if (int rc = edge_aggregate_records(
            ctx, n_in ? reinterpret_cast<const uint64_t*>(recs[k] + in_traces[0]) : nullptr, n_in,
            S, &form, tabs[k]))
      return rc;
  }
  uint64_t* h_tab[kTabs] = {out->untimed, out->early, out->late, out->early_us, out->late_us};
  if (!n_in) {
    for (uint64_t* p : h_tab)
      if (p) memset(p, 0, E * 8);
    if (out->span_req_us && n) memset(out->span_req_us, 0, n * 4);
    if (out->span_resp_us && n) memset(out->span_resp_us, 0, n * 4);
    if (out->span_state && n) memset(out->span_state, 0, n);
    return ANOMOD_OK;
  }
  std::vector<unsigned long long> h(E * kTabs);
  unsigned long long total[2] = {0ull, 0ull};
  ANOMOD_HIP(ctx, hipMemcpyAsync(h.data(), a.tab, tab_bytes, hipMemcpyDeviceToHost, ctx->stream));
  ANOMOD_HIP(ctx, hipMemcpyAsync(total, a.total, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (a.req_us)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->span_req_us, a.req_us, n * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
  if (a.resp_us)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->span_resp_us, a.resp_us, n * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
  if (a.state)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->span_state, a.state, n, hipMemcpyDeviceToHost,
                                   ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t k = 0; k < kTabs; ++k)
    if (h_tab[k]) memcpy(h_tab[k], h.data() + E * k, E * 8);
  out->calls = total[0];
  out->paired = total[1];
  return ANOMOD_OK;
}

}  // extern "C"
