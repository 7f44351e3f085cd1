// Critical path of a grouped span set with a start column, and its edge table.
//
//   s(i), e(i)  = start_us[i], start_us[i] + dur_us[i] (u64, saturating)
//   par(i)      = self time's parent (self_time.hip): the first span of i's
//                 trace, in position order, whose span_id equals i's
//                 parent_span_id; none for reference 0, for a reference naming
//                 no span of the trace and when the first match is i itself.
//                 A span of a trace without a parent is a head.
//   a(c), b(c)  = max(s(c), s(p)), min(e(c), e(p)) for p = par(c); c is
//                 eligible when a(c) < b(c)
//   selection at p: cur = e(p); repeatedly take, among the eligible children
//                 with b <= cur, the largest b (smallest position among equal
//                 b), select it and set cur = a of it
//   on_path     = the least set holding every head and every selected span
//                 whose parent is on the path
//   cp_us[i]    = dur_us[i] - sum of (b - a) over the selected children of i
//                 for i on the path, else 0
//
// One chunk walk (walk.h: persistent waves, <= 256 spans / <= 64 whole traces
// per chunk, buffer loads, the columns of chunk c+1 in flight while chunk c is
// resolved) finds every span's parent position in the
// wave's LDS, runs the selection of all parents of the chunk in rounds (one
// step of every parent per round: ds_max_u64 on the parent's slot, ds_min on
// the position among the holders of the maximum), then 8 rounds of pointer
// jumping over (ancestor, all selected so far) words, and writes one edge
// record per span by span position for edge_aggregate_records — (parent row *
// S + service) << 33 | error << 32 | cp_us for a span on the path, the skip
// record (all ones) for one off it.  Traces longer than a
// chunk are listed by the walk and resolved by critical_path_big_kernel, one
// workgroup per listed trace, with the per-span state in global scratch.
// Every value is an integer: results are bit-exact for any launch geometry.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kCpWaves = 4;
constexpr int kCpThreads = kCpWaves * kWave;

// Per-wave LDS (every offset a multiple of 16).  Three arrays are reused once
// the parents are found and a / b sit in registers: the ids become the u64
// offer slots, the starts the u64 cursors, the durations the winner positions
// and later the jump words.
constexpr int kCSid = 0;  // u64 ids [kStage + kScanSlack] (or two u32 planes) | u64 best b [kStage]
constexpr int kCStart = kCSid + (kStage + (int)kScanSlack) * 8;  // u64 starts | u64 cursors [kStage]
constexpr int kCDur = kCStart + kStage * 8;   // u32 durations | winner positions | jump words [kStage]
constexpr int kCSum = kCDur + kStage * 4;     // u32 selected-children sums [kStage]
constexpr int kCSvc = kCSum + kStage * 4;     // u16 services [kStage]
constexpr int kCFlag = kCSvc + kStage * 2;    // u8 trace-start flags [kStage]
constexpr int kCBytes = kCFlag + kStage;
static_assert(kCBytes % 16 == 0, "wave staging must stay 16-B aligned");

// span states of the selection
constexpr uint32_t kOut = 0, kCand = 1, kOffer = 2, kSel = 3;
// chunk jump word: ancestor position | kOk (every span up to it selected) | kDone (it is a head)
constexpr uint32_t kPosMask = 0xFFFFu, kOk = 1u << 16, kDone = 1u << 17;
// long-trace jump word: the same over u32 positions
constexpr unsigned long long kOk64 = 1ull << 32, kDone64 = 1ull << 33;

struct CpArgs {
  unsigned long long* rec;       // [n_spans] edge records by span position (kSkipRec: off the path)
  uint32_t* cp_us;               // [n_spans] or NULL
  uint8_t* on_path;              // [n_spans] or NULL
  unsigned long long* ctr;       // trace-segment counter of the dynamic tail
  unsigned long long* big;       // [0] listed traces, [1] their spans, [2] ticket
  unsigned long long* big_list;  // (trace, scratch offset) per listed trace
  uint64_t big_cap;              // entries big_list holds
  // per-span state of the listed traces, [counted long spans] each
  uint32_t* l_ppos;              // parent position in the trace (kNone: none; own position: self-reference)
  unsigned long long* l_a;       // a(c)
  unsigned long long* l_b;       // b(c)
  unsigned long long* l_best;    // largest b offered to the span this round (0: none)
  uint32_t* l_bpos;              // smallest position among the holders of l_best
  unsigned long long* l_cur;     // the span's cursor
  uint32_t* l_sum;               // sum of b - a over its selected children
  uint32_t* l_st;                // selection state
  unsigned long long* l_j[2];    // jump words, two buffers
  uint32_t S;
};

struct Regs {
  uint64_t sid[kPer], pid[kPer], start[kPer];
  uint32_t dur[kPer], sf[kPer];  // sf = svc | flags << 16
};

__device__ __forceinline__ void load_regs(const uint64_t* __restrict__ span_id,
                                          const uint64_t* __restrict__ parent,
                                          const uint32_t* __restrict__ svcfl,
                                          const uint32_t* __restrict__ dur,
                                          const uint64_t* __restrict__ start, const Chunk& c,
                                          int lane, Regs& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by critical_path_big_kernel
  const auto rsid = rsrc(span_id + c.base, n * 8u);
  const auto rpid = rsrc(parent + c.base, n * 8u);
  const auto rsf = rsrc(svcfl + c.base, n * 4u);
  const auto rdur = rsrc(dur + c.base, n * 4u);
  const auto rst = rsrc(start + c.base, n * 8u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.sid[r] = bload64(rsid, i * 8u);
    R.pid[r] = bload64(rpid, i * 8u);
    R.start[r] = bload64(rst, i * 8u);
    R.sf[r] = bload32(rsf, i * 4u);
    R.dur[r] = bload32(rdur, i * 4u);
  }
}

__device__ __forceinline__ uint64_t sat_end(uint64_t s, uint32_t d) {
  const uint64_t e = s + (uint64_t)d;
  return e < s ? ~0ull : e;
}

template <int SCAN>
__device__ __forceinline__ void cp_chunk(unsigned char* wsm, int lane, const Chunk& c,
                                         const Regs& R, const CpArgs& a) {
  auto* lsid = reinterpret_cast<uint64_t*>(wsm + kCSid);
  auto* llo = reinterpret_cast<uint32_t*>(wsm + kCSid);
  uint32_t* lhi = llo + (kStage + kScanSlack);
  auto* lstart = reinterpret_cast<uint64_t*>(wsm + kCStart);
  auto* ldur = reinterpret_cast<uint32_t*>(wsm + kCDur);
  auto* lbest = reinterpret_cast<unsigned long long*>(wsm + kCSid);   // after the parent phase
  auto* lcur = reinterpret_cast<unsigned long long*>(wsm + kCStart);  // "
  auto* lpos = reinterpret_cast<uint32_t*>(wsm + kCDur);              // "
  auto* lj = reinterpret_cast<uint32_t*>(wsm + kCDur);                // after the selection
  auto* lsum = reinterpret_cast<uint32_t*>(wsm + kCSum);
  auto* lsvc = reinterpret_cast<uint16_t*>(wsm + kCSvc);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kCFlag);
  // Stage ids, services, starts and durations (lanes past n hold zeros from
  // the buffer loads) and mark trace starts.
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
    lstart[i] = R.start[r];
    ldur[i] = R.dur[r];
  }
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);
  // Parent position, edge row, and the child's interval clipped to the
  // parent's: a, b stay in registers from here on.
  uint32_t row[kPer], pp[kPer], st[kPer];
  uint64_t av[kPer], bv[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    uint32_t p = a.S;  // ROOT
    int q = -1;
    if (i < c.n && R.pid[r] != 0ull) {
      p = a.S + 1u;  // ORPHAN unless found in the trace
      uint32_t ta, tb;
      trace_bounds(Sm, r, lane, c.n, ta, tb);
      q = find_parent<SCAN>(lsid, llo, lhi, ta, tb, i, R.pid[r]);
      if (q >= 0) p = lsvc[q];  // a self-reference keeps its own service as parent
    }
    row[r] = p;
    const bool has = q >= 0 && (uint32_t)q != i;  // a span is not its own child
    pp[r] = has ? (uint32_t)q : kNone;
    av[r] = bv[r] = 0ull;
    st[r] = kOut;
    if (has) {
      const uint64_t sp = lstart[q], ep = sat_end(sp, ldur[q]);
      const uint64_t s = R.start[r], e = sat_end(s, R.dur[r]);
      av[r] = s > sp ? s : sp;
      bv[r] = e < ep ? e : ep;
      if (av[r] < bv[r]) st[r] = kCand;
    }
  }
  wave_sync();  // ids, starts and durations are dead: their arrays change roles
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    lcur[i] = sat_end(R.start[r], R.dur[r]);
    lbest[i] = 0ull;  // an offer is a b > a >= 0, so 0 is "none"
    lpos[i] = kNone;
    lsum[i] = 0u;
  }
  wave_sync();
  // Selection rounds: every parent of the chunk takes one step per round.  A
  // candidate whose b lies past its parent's cursor never fits again (the
  // cursor only moves down).
  while (true) {
    bool off[kPer], won[kPer];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      off[r] = false;
      if (st[r] == kCand) {
        if (bv[r] <= lcur[pp[r]]) {
          atomicMax(&lbest[pp[r]], (unsigned long long)bv[r]);
          off[r] = true;
        } else {
          st[r] = kOut;
        }
      }
    }
    bool any = false;
#pragma unroll
    for (int r = 0; r < kPer; ++r) any |= off[r];
    if (!__ballot(any)) break;
    wave_sync();
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const uint32_t i = lane + r * kWave;
      off[r] = off[r] && lbest[pp[r]] == bv[r];
      if (off[r]) atomicMin(&lpos[pp[r]], i);
    }
    wave_sync();
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const uint32_t i = lane + r * kWave;
      won[r] = off[r] && lpos[pp[r]] == i;
    }
    wave_sync();
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      if (!won[r]) continue;  // one winner per parent: plain stores
      const uint32_t p = pp[r];
      st[r] = kSel;
      lcur[p] = av[r];
      lsum[p] += (uint32_t)(bv[r] - av[r]);
      lbest[p] = 0ull;
      lpos[p] = kNone;
    }
    wave_sync();
  }
  wave_sync();
  // Pointer jumping: 2^8 hops cover a chunk.  A head points at itself, done.
  uint32_t w[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if (i >= c.n)
      w[r] = i | kDone;  // not a span: done, never on the path
    else if (pp[r] == kNone)
      w[r] = i | kOk | kDone;
    else
      w[r] = pp[r] | (st[r] == kSel ? kOk : 0u);
    lj[i] = w[r];
  }
  wave_sync();
  for (int round = 0; round < 8; ++round) {
    uint32_t nw[kPer];
    bool open = false;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      nw[r] = w[r];
      if (!(w[r] & kDone)) {
        const uint32_t w2 = lj[w[r] & kPosMask];
        nw[r] = (w2 & (kPosMask | kDone)) | (w[r] & w2 & kOk);
        open = true;
      }
    }
    if (!__ballot(open)) break;
    wave_sync();
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      w[r] = nw[r];
      lj[lane + r * kWave] = nw[r];
    }
    wave_sync();
  }
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    const bool on = i < c.n && (w[r] & (kOk | kDone)) == (kOk | kDone);
    const uint32_t cp = on ? R.dur[r] - lsum[i] : 0u;
    if (i >= c.n) continue;
    a.rec[c.base + i] = on ? edge_rec(row[r], a.S, R.sf[r], cp) : kSkipRec;
    if (a.cp_us) a.cp_us[c.base + i] = cp;
    if (a.on_path) a.on_path[c.base + i] = on ? 1 : 0;
  }
  wave_sync();  // the staging area is free for the next chunk
}

// Three waves per SIMD (three workgroups per CU) is what the registers allow:
// declared, so that the forward instantiation keeps to it too.
template <int SCAN>
__global__ __launch_bounds__(kCpThreads, 3) void critical_path_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ start, const uint64_t* __restrict__ trace_ptr, uint64_t n_traces,
    CpArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kCBytes * kCpWaves];
  const int lane = threadIdx.x & (kWave - 1);
  unsigned char* wsm = smem + (threadIdx.x / kWave) * kCBytes;
  walk_traces<kCpWaves, 4, Regs>(
      trace_ptr, n_traces, a.ctr,
      [&](const Chunk& c, Regs& R) __attribute__((always_inline)) {
        load_regs(span_id, parent, svcfl, dur, start, c, lane, R);
      },
      [&](const Chunk& c, uint32_t, uint64_t, const Regs& R) __attribute__((always_inline)) {
        cp_chunk<SCAN>(wsm, lane, c, R, a);
      },
      // longer than kStage: listed for critical_path_big_kernel
      [&](uint64_t t, uint32_t n) __attribute__((always_inline)) {
        list_long(a.big, a.big_list, a.big_cap, lane, t, n);
      });
}

// ---- long traces ----------------------------------------------------------
// One workgroup per listed trace (tickets).  Parent positions come from
// walk.h's windowed LDS id table (big_parents).  The
// per-span state lives in global scratch: a span's words are written by the
// thread that owns the span (position % kBigThreads) or, for the words of a
// parent, by atomics and agent-scope stores of its children; every word
// another thread may have written is read with an agent-scope atomic load,
// and every wave waits for its own stores and atomics before the barrier that
// separates two sweeps (sweep_sync).  The selection runs the
// chunk kernel's rounds — offer b (atomic max), offer the position among the
// holders of the maximum (atomic min), the winner moves the cursor — at three
// sweeps of the trace per round, then ceil(log2 L) pointer-jumping rounds
// between the two jump buffers: O((rounds + log L) * L) global accesses for a
// trace of L spans, rounds = the largest number of selected children of one
// span.
__global__ __launch_bounds__(kBigThreads) void critical_path_big_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ start, const uint64_t* __restrict__ trace_ptr, CpArgs a) {
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
    const uint64_t off = a.big_list[2 * j + 1];
    const uint64_t lo = trace_ptr[t];
    const uint32_t L = (uint32_t)(trace_ptr[t + 1] - lo);  // the call takes < 2^32 spans
    uint32_t* ppos = a.l_ppos + off;
    unsigned long long* sa = a.l_a + off;
    unsigned long long* sb = a.l_b + off;
    unsigned long long* best = a.l_best + off;
    uint32_t* wpos = a.l_bpos + off;
    unsigned long long* cur = a.l_cur + off;
    uint32_t* sum = a.l_sum + off;
    uint32_t* st = a.l_st + off;
    unsigned long long* jA = a.l_j[0] + off;
    unsigned long long* jB = a.l_j[1] + off;
    // ---- parent positions
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
      uint64_t pid[kBigPer];
      uint32_t pp[kBigPer];  // parent position in the trace (kNone: none)
      big_parents(span_id, parent, lo, L, b0, tid, bkey, bpos, pid, pp);
      // The span's interval clipped to its parent's, and the span's own slots.
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
        if (i >= L) continue;
        const uint32_t q = pp[r];
        const uint64_t s = start[lo + i], e = sat_end(s, dur[lo + i]);
        uint64_t av = 0, bv = 0;
        uint32_t state = kOut;
        if (q != kNone && q != (uint32_t)i) {
          const uint64_t sp = start[lo + q], ep = sat_end(sp, dur[lo + q]);
          av = s > sp ? s : sp;
          bv = e < ep ? e : ep;
          if (av < bv) state = kCand;
        }
        ppos[i] = q;
        sa[i] = av;
        sb[i] = bv;
        st[i] = state;
        astore(&cur[i], (unsigned long long)e);
        astore(&best[i], 0ull);
        astore(&wpos[i], kNone);
        astore(&sum[i], 0u);
      }
    }
    sweep_sync();
    // ---- selection rounds
    while (true) {
      bool any = false;
      for (uint64_t i = tid; i < L; i += kBigThreads) {
        if (st[i] != kCand) continue;
        const uint32_t p = ppos[i];
        if (sb[i] <= aload(&cur[p])) {
          atomicMax(&best[p], sb[i]);
          st[i] = kOffer;
          any = true;
        } else {
          st[i] = kOut;  // the cursor only moves down
        }
      }
      wait_stores();
      if (!__syncthreads_or(any)) break;
      for (uint64_t i = tid; i < L; i += kBigThreads) {
        if (st[i] != kOffer) continue;
        const uint32_t p = ppos[i];
        if (aload(&best[p]) == sb[i])
          atomicMin(&wpos[p], (uint32_t)i);
        else
          st[i] = kCand;
      }
      sweep_sync();
      // The winner clears its parent's slots at once: a span that still reads
      // them is not the winner under the old values or the new ones.
      for (uint64_t i = tid; i < L; i += kBigThreads) {
        if (st[i] != kOffer) continue;
        const uint32_t p = ppos[i];
        if (aload(&wpos[p]) == (uint32_t)i) {
          st[i] = kSel;
          astore(&cur[p], sa[i]);
          astore(&sum[p], aload(&sum[p]) + (uint32_t)(sb[i] - sa[i]));
          astore(&best[p], 0ull);
          astore(&wpos[p], kNone);
        } else {
          st[i] = kCand;
        }
      }
      sweep_sync();
    }
    // ---- pointer jumping between the two buffers
    for (uint64_t i = tid; i < L; i += kBigThreads) {
      const uint32_t q = ppos[i];
      const bool has = q != kNone && q != (uint32_t)i;
      astore(&jA[i], has ? (unsigned long long)q | (st[i] == kSel ? kOk64 : 0ull)
                         : (unsigned long long)i | kOk64 | kDone64);
    }
    sweep_sync();
    for (uint64_t hops = 1; hops < L; hops <<= 1) {
      for (uint64_t i = tid; i < L; i += kBigThreads) {
        const unsigned long long w = aload(&jA[i]);
        unsigned long long nw = w;
        if (!(w & kDone64)) {
          const unsigned long long w2 = aload(&jA[(uint32_t)w]);
          nw = (w2 & (0xFFFFFFFFull | kDone64)) | (w & w2 & kOk64);
        }
        astore(&jB[i], nw);
      }
      sweep_sync();
      unsigned long long* x = jA;
      jA = jB;
      jB = x;
    }
    // ---- outputs
    for (uint64_t i = tid; i < L; i += kBigThreads) {
      const unsigned long long w = aload(&jA[i]);
      const bool on = (w & (kOk64 | kDone64)) == (kOk64 | kDone64);
      const uint32_t cp = on ? dur[lo + i] - aload(&sum[i]) : 0u;
      if (a.cp_us) a.cp_us[lo + i] = cp;
      if (a.on_path) a.on_path[lo + i] = on ? 1 : 0;
      const uint32_t q = ppos[i];
      const uint32_t p = parent[lo + i] == 0ull ? S
                         : q == kNone           ? S + 1u
                                                : (svcfl[lo + q] & 0xFFFFu);
      a.rec[lo + i] = on ? edge_rec(p, S, svcfl[lo + i], cp) : kSkipRec;
    }
  }
}

using WalkFn = void (*)(const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                        const uint64_t*, const uint64_t*, uint64_t, CpArgs);

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_edge_critical_path_spans(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S,
                                    anomod_edge_table* out, uint32_t* cp_us, uint8_t* on_path) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_edge_critical_path_spans: NULL argument");
  // As anomod_edge_self_time_spans: what can fail on one rank only feeds the
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
  if (local == ANOMOD_OK && !spans->start_us) {
    set_error(ctx, "span set has no start-time column: anomod_spans_set_start_us first");
    local = ANOMOD_ESTATE;
  }
  if (local == ANOMOD_OK) local = bind(ctx);
  if (int rc = comm_agree(ctx, local)) return rc;

  const uint64_t n = spans->n_spans, nt = spans->n_traces;
  // the spans that lie in traces (spans outside every trace are on no path:
  // their cp_us and on_path read 0)
  uint64_t in_traces[2];
  local = trace_span_range(ctx, spans, in_traces);
  if (local != ANOMOD_OK && local != ANOMOD_EINVAL) return local;
  const uint64_t n_in = in_traces[1] - in_traces[0];

  // The call's workspace: a block of words (dynamic-tail counter, long-trace
  // counters, order-probe scratch) and a block of records | cp_us | on_path
  // (when asked for) | long-trace list | the listed spans' state (64 B per
  // span).  The long traces are counted first.
  CallWorkspace ws{ctx};
  const auto al = CallWorkspace::al;
  unsigned long long nlong[2] = {0ull, 0ull};
  if (local == ANOMOD_OK && n_in) local = ws.take(&ws.words, 256, "critical-path");
  auto* words = static_cast<unsigned long long*>(ws.words);
  if (local == ANOMOD_OK && n_in)
    if (int rc = count_long_traces(ctx, spans, words, nlong)) return rc;
  const size_t nl = (size_t)nlong[1];
  const size_t b_rec = al(n * 8), b_cp = cp_us ? al(n * 4) : 0, b_on = on_path ? al(n) : 0;
  const size_t b_list = al(nlong[0] * 16), b_l8 = al(nl * 8), b_l4 = al(nl * 4);
  if (local == ANOMOD_OK && n_in)
    local = ws.take(&ws.block, b_rec + b_cp + b_on + b_list + 6 * b_l8 + 4 * b_l4,
                    "critical-path");
  if (int rc = comm_agree(ctx, local)) return rc;

  CpArgs a{};
  if (n_in) {
    a.rec = ws.carve<unsigned long long>(b_rec);
    a.cp_us = cp_us ? ws.carve<uint32_t>(b_cp) : nullptr;
    a.on_path = on_path ? ws.carve<uint8_t>(b_on) : nullptr;
    a.big_list = ws.carve<unsigned long long>(b_list);
    a.l_a = ws.carve<unsigned long long>(b_l8);
    a.l_b = ws.carve<unsigned long long>(b_l8);
    a.l_best = ws.carve<unsigned long long>(b_l8);
    a.l_cur = ws.carve<unsigned long long>(b_l8);
    a.l_j[0] = ws.carve<unsigned long long>(b_l8);
    a.l_j[1] = ws.carve<unsigned long long>(b_l8);
    a.l_ppos = ws.carve<uint32_t>(b_l4);
    a.l_bpos = ws.carve<uint32_t>(b_l4);
    a.l_sum = ws.carve<uint32_t>(b_l4);
    a.l_st = ws.carve<uint32_t>(b_l4);
    a.ctr = words;
    a.big = words + 1;
    a.big_cap = nlong[0];
    a.S = S;
    int scan = kScanFwd;
    if (int rc = pick_walk_scan(ctx, spans, S, words + 4, &scan)) return rc;
    const WalkFn fn = scan == kScanFwd     ? critical_path_kernel<kScanFwd>
                      : scan == kScanSplit ? critical_path_kernel<kScanSplit>
                                           : critical_path_kernel<kScanBidir>;
    uint64_t grid = 0;
    if (int rc = walk_grid(ctx, fn, kCpThreads, &grid)) return rc;
    log_walk_kernel("critical-path", "critical_path_kernel", scan, nlong[0]);
    ANOMOD_HIP(ctx, hipMemsetAsync(words, 0, 32, ctx->stream));  // ctr + big counters
    if (a.cp_us && n_in < n) ANOMOD_HIP(ctx, hipMemsetAsync(a.cp_us, 0, n * 4, ctx->stream));
    if (a.on_path && n_in < n) ANOMOD_HIP(ctx, hipMemsetAsync(a.on_path, 0, n, ctx->stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kCpThreads), 0, ctx->stream, spans->span_id,
                       spans->parent_span_id, spans->svc_flags, spans->dur_us, spans->start_us,
                       spans->trace_ptr, nt, a);
    ANOMOD_HIP(ctx, hipGetLastError());
    if (nlong[0]) {
      hipLaunchKernelGGL(critical_path_big_kernel,
                         dim3((unsigned)std::min<uint64_t>(nlong[0], 2ull * ctx->num_cus)),
                         dim3(kBigThreads), 0, ctx->stream, spans->span_id, spans->parent_span_id,
                         spans->svc_flags, spans->dur_us, spans->start_us, spans->trace_ptr, a);
      ANOMOD_HIP(ctx, hipGetLastError());
    }
  }
  // The table of the records (the off-path spans' are skipped).  The
  // distribution is not the durations': the set's histogram-form hint is
  // neither read nor touched (form unknown: the compact form, which has
  // nothing to saturate).
  int8_t form = -1;
  if (int rc = edge_aggregate_records(
          ctx, n_in ? reinterpret_cast<const uint64_t*>(a.rec + in_traces[0]) : nullptr, n_in, S,
          &form, out))
    return rc;
  if (n) {
    if (n_in) {
      if (cp_us)
        ANOMOD_HIP(ctx, hipMemcpyAsync(cp_us, a.cp_us, n * 4, hipMemcpyDeviceToHost, ctx->stream));
      if (on_path)
        ANOMOD_HIP(ctx, hipMemcpyAsync(on_path, a.on_path, n, hipMemcpyDeviceToHost, ctx->stream));
      if (cp_us || on_path) ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } else {
      if (cp_us) memset(cp_us, 0, n * 4);
      if (on_path) memset(on_path, 0, n);
    }
  }
  return ANOMOD_OK;
}

}  // extern "C"
