// Error origins of a grouped span set: where failures start, how far they
// travel up their callers, and whether they reach the trace's entry.
//
//   err(i)     = flags[i] & ANOMOD_FLAG_ERROR
//   par(i)     = self time's parent (self_time.hip): the first span of i's
//                trace, in position order, whose span_id equals i's
//                parent_span_id; a root, an orphan and a self-reference have
//                none and are heads
//   kid_err(j) = error-flagged spans whose parent is j
//   class(i)   = CLEAN / ORIGIN (err, no failing callee) / PROPAGATED (err, a
//                failing callee) / ABSORBER (a failing callee, no err)
//   up(i)      = par(i) when it exists and carries the flag; hops(i) = steps
//                along up until a span without one, top(i)
//   fate(i)    = SURFACED (top is a head) / CONTAINED (top has a parent, which
//                carries no flag) / LOOP (the chain never ends: hops 0)
//
// One chunk walk (walk.h: persistent waves, <= 256 spans / <= 64 whole traces
// per chunk, buffer loads, the columns of chunk c+1 in flight while chunk c is
// resolved) reads 20 B per span (svc|flags 4, id 8, parent id 8).  A chunk
// without an error flag — one wave ballot over the svc|flags registers — is
// done: it touches no LDS and writes nothing.  Otherwise the wave stages ids,
// services and one state word per span; the error-flagged spans find their
// parent positions and OR the child-error bit into their parent's word
// (ds_or; siblings serialise on the word); after a wave sync every span knows
// its class, an absorber finds its own parent (its row needs the service), an
// error-flagged span links to up(i) or is terminal with its fate, and at most
// 8 pointer-jumping rounds (hops += hops(anc); anc = anc(anc); a terminal
// ancestor's fate is adopted — read all, sync, write all, the form of
// trace_shapes_kernel) close every chain a chunk can hold: after round k the
// chains of <= 2^k - 1 hops are closed.  What is still open is LOOP.
//
// Row counters: only error-flagged spans and absorbers count.  With 7 E u32
// words within the dynamic-LDS budget they are privatised per workgroup in
// LDS and flushed once (u64 global adds, atomicMax for hops_max; a u32 LDS sum
// of hops that wraps carries 2^32 into the global word at once), else they go
// to the global table directly: results never depend on which form ran.
//
// Traces longer than a chunk are listed by the walk and resolved by
// error_origins_big_kernel, one workgroup per listed trace.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kOrWaves = 4;
constexpr int kOrThreads = kOrWaves * kWave;
// dynamic LDS of the counters: two workgroups of 15.5 + 64 KiB fit a CU's 160 KiB
constexpr uint32_t kDynLdsBudget = 64u * 1024u;
constexpr uint32_t kTabs = 6;  // u64 tables; hops_max is the seventh (u32)
enum { kTOrigin, kTProp, kTStopped, kTSurfaced, kTAbsorb, kTHops, kTMax };

// Per-wave LDS (every offset a multiple of 16).
constexpr int kOSid = 0;  // u64 span ids [kStage + kScanSlack], or two u32 planes of that length
constexpr int kOWord = kOSid + (kStage + (int)kScanSlack) * 8;  // u32 state words [kStage]
constexpr int kOSvc = kOWord + kStage * 4;                      // u16 services [kStage]
constexpr int kOFlag = kOSvc + kStage * 2;                      // u8 trace-start flags [kStage]
constexpr int kOBytes = kOFlag + kStage;
static_assert(kOBytes % 16 == 0, "wave staging must stay 16-B aligned");
static_assert(2 * (kOBytes * kOrWaves + kDynLdsBudget) <= 160u * 1024u, "LDS of a CU");

// Chunk state word: ancestor position (a terminal span: its own) | hops << 8 |
// kTerm | fate << 25 | kErr | kKid.  An open chain of a reference cycle doubles
// its hops every round: 2^8 after the last one, inside the 16-bit field.
constexpr uint32_t kAncMask = 0xFFu, kHopShift = 8, kHopMask = 0xFFFFu;
constexpr uint32_t kTerm = 1u << 24, kFateShift = 25, kFateMask = 3u << kFateShift;
constexpr uint32_t kErr = 1u << 27, kKid = 1u << 28;
static_assert(kStage <= 256, "the ancestor field holds a chunk position");

// Long-trace jump word: ancestor position in the trace, or the fate of a closed
// chain (positions stay below 2^32 - 2: the call takes at most that many
// spans), | hops << 32.
constexpr uint32_t kBigSurf = 0xFFFFFFFFu, kBigCont = 0xFFFFFFFEu;
constexpr uint32_t kBigKid = 1u;  // child-error bit of the long-trace scratch word

struct OrArgs {
  unsigned long long* ctr;       // trace-segment counter of the dynamic tail
  unsigned long long* big;       // [0] listed traces, [1] their spans, [2] ticket
  unsigned long long* misc;      // [0] error-flagged spans, [1] those of fate LOOP
  unsigned long long* tab;       // u64 [kTabs][E]: origin | propagated | stopped | surfaced |
                                 // absorbers | hops_sum
  uint32_t* hmax;                // u32 [E]
  uint8_t* state;                // [n_spans] or NULL (zeroed: clean chunks write nothing)
  uint32_t* hops;                // [n_spans] or NULL (zeroed)
  unsigned long long* big_list;  // (trace, scratch offset) per listed trace
  uint64_t big_cap;              // entries big_list holds
  uint32_t* l_kid;               // [long spans] child-error bits (zeroed)
  uint32_t* l_row;               // [long spans] edge rows
  unsigned long long* l_w[2];    // [long spans] jump words, two buffers
  uint32_t S, E;
  uint32_t lds;                  // counters privatised in LDS (else global atomics)
};

extern __shared__ __align__(16) unsigned char origins_lds[];

struct Regs {
  uint64_t sid[kPer], pid[kPer];
  uint32_t sf[kPer];  // svc | flags << 16
};

// svc|flags first: the clean-chunk ballot needs nothing else, and the loads
// return in order.
__device__ __forceinline__ void load_regs(const uint64_t* __restrict__ span_id,
                                          const uint64_t* __restrict__ parent,
                                          const uint32_t* __restrict__ svcfl, const Chunk& c,
                                          int lane, Regs& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by error_origins_big_kernel
  const auto rsf = rsrc(svcfl + c.base, n * 4u);
  const auto rsid = rsrc(span_id + c.base, n * 8u);
  const auto rpid = rsrc(parent + c.base, n * 8u);
#pragma unroll
  for (int r = 0; r < kPer; ++r)
    R.sf[r] = bload32(rsf, ((uint32_t)lane + (uint32_t)(r * kWave)) * 4u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.sid[r] = bload64(rsid, i * 8u);
    R.pid[r] = bload64(rpid, i * 8u);
  }
}

__device__ __forceinline__ bool sf_err(uint32_t sf) {
  return ((sf >> 16) & ANOMOD_FLAG_ERROR) != 0u;
}

// What one classified span adds to the tables: cls / fate of include/anomod.h,
// row its edge row.  LDS: u32 adds (a wrapped hops sum carries into the global
// word); global: the u64 table itself.
__device__ __forceinline__ void count_span(const OrArgs& a, uint32_t* lctr, bool lds, uint32_t row,
                                           uint32_t cls, uint32_t fate, uint32_t hops) {
  const uint32_t E = a.E;
  auto add1 = [&](uint32_t t) __attribute__((always_inline)) {
    if (lds) atomicAdd(&lctr[t * E + row], 1u);
    else atomicAdd(&a.tab[(size_t)t * E + row], 1ull);
  };
  if (cls == ANOMOD_ERR_ABSORBER) {
    add1(kTAbsorb);
    return;
  }
  add1(cls == ANOMOD_ERR_ORIGIN ? kTOrigin : kTProp);
  if (hops == 0u && fate == ANOMOD_FATE_CONTAINED) add1(kTStopped);
  if (cls != ANOMOD_ERR_ORIGIN) return;
  if (fate == ANOMOD_FATE_SURFACED) add1(kTSurfaced);
  if (hops == 0u) return;
  if (lds) {
    const uint32_t old = atomicAdd(&lctr[kTHops * E + row], hops);
    if (old + hops < old) atomicAdd(&a.tab[(size_t)kTHops * E + row], 1ull << 32);
    atomicMax(&lctr[kTMax * E + row], hops);
  } else {
    atomicAdd(&a.tab[(size_t)kTHops * E + row], (unsigned long long)hops);
    atomicMax(&a.hmax[row], hops);
  }
}

// n_err / n_loop: the lane's counts of error-flagged spans and of those of
// fate LOOP.
template <int SCAN>
__device__ __forceinline__ void origins_chunk(unsigned char* wsm, uint32_t* lctr, int lane,
                                              const Chunk& c, const Regs& R, const OrArgs& a,
                                              uint32_t& n_err, uint32_t& n_loop) {
  // A chunk without a flag: nothing to classify, nothing to count, and the
  // per-span columns read 0 from the call's memset.  (Lanes past n hold zeros
  // from the buffer loads.)
  bool e[kPer], any = false;
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    e[r] = sf_err(R.sf[r]);
    any |= e[r];
  }
  if (!__ballot(any)) return;

  auto* lsid = reinterpret_cast<uint64_t*>(wsm + kOSid);
  auto* llo = reinterpret_cast<uint32_t*>(wsm + kOSid);
  uint32_t* lhi = llo + (kStage + kScanSlack);
  auto* lw = reinterpret_cast<uint32_t*>(wsm + kOWord);
  auto* lsvc = reinterpret_cast<uint16_t*>(wsm + kOSvc);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kOFlag);
  const uint32_t S = a.S;
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
    lw[i] = e[r] ? kErr : 0u;
  }
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);  // (its wave syncs also publish the staging)
  // Parent position q (-1: none) and parent service of span r of this lane.
  auto parent_of = [&](int r, uint32_t i, uint32_t& prow) __attribute__((always_inline)) -> int {
    prow = S;  // ROOT
    if (R.pid[r] == 0ull) return -1;
    prow = S + 1u;  // ORPHAN unless found in the trace
    uint32_t ta, tb;
    trace_bounds(Sm, r, lane, c.n, ta, tb);
    const int q = find_parent<SCAN>(lsid, llo, lhi, ta, tb, i, R.pid[r]);
    if (q >= 0) prow = lsvc[q];  // (a self-reference keeps its own service as parent)
    return q;
  };
  // The error-flagged spans tell their parents.
  uint32_t prow[kPer];
  int q[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    q[r] = -1;
    prow[r] = S;
    if (!e[r]) continue;  // (e: i < c.n)
    q[r] = parent_of(r, i, prow[r]);
    if (q[r] >= 0 && (uint32_t)q[r] != i) atomicOr(&lw[q[r]], kKid);
  }
  wave_sync();
  // Class; an absorber's row; an error-flagged span's link or fate.
  uint32_t w[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    const uint32_t own = lw[i];
    if (e[r]) {
      const bool has = q[r] >= 0 && (uint32_t)q[r] != i;
      if (has && (lw[q[r]] & kErr))
        w[r] = own | (uint32_t)q[r] | (1u << kHopShift);
      else
        w[r] = own | i | kTerm |
               ((has ? ANOMOD_FATE_CONTAINED : ANOMOD_FATE_SURFACED) << kFateShift);
    } else {
      w[r] = own | i | kTerm;
      if (own & kKid) (void)parent_of(r, i, prow[r]);
    }
  }
  wave_sync();  // every word was read: the links replace them
#pragma unroll
  for (int r = 0; r < kPer; ++r) lw[lane + r * kWave] = w[r];
  wave_sync();
  // Pointer jumping: 2^8 - 1 hops cover a chunk.  Read all, sync, write all.
  for (int round = 0; round < 8; ++round) {
    bool open = false;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      if (!(w[r] & kTerm)) {
        const uint32_t wa = lw[w[r] & kAncMask];
        const uint32_t h = (((w[r] >> kHopShift) & kHopMask) + ((wa >> kHopShift) & kHopMask)) &
                           kHopMask;
        w[r] = (w[r] & (kErr | kKid)) | (wa & (kAncMask | kTerm | kFateMask)) | (h << kHopShift);
        open = true;
      }
    }
    if (!__ballot(open)) break;
    wave_sync();
#pragma unroll
    for (int r = 0; r < kPer; ++r) lw[lane + r * kWave] = w[r];
    wave_sync();
  }
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if (i >= c.n) continue;
    const bool kid = (w[r] & kKid) != 0u, done = (w[r] & kTerm) != 0u;
    const uint32_t cls = e[r] ? (kid ? ANOMOD_ERR_PROPAGATED : ANOMOD_ERR_ORIGIN)
                              : (kid ? ANOMOD_ERR_ABSORBER : ANOMOD_ERR_CLEAN);
    const uint32_t fate = !e[r] ? 0u : done ? (w[r] & kFateMask) >> kFateShift : ANOMOD_FATE_LOOP;
    const uint32_t hops = e[r] && done ? (w[r] >> kHopShift) & kHopMask : 0u;
    if (a.state) a.state[c.base + i] = (uint8_t)(cls | fate << 2);
    if (a.hops) a.hops[c.base + i] = hops;
    if (cls == ANOMOD_ERR_CLEAN) continue;
    n_err += e[r] ? 1u : 0u;
    n_loop += fate == ANOMOD_FATE_LOOP ? 1u : 0u;
    count_span(a, lctr, a.lds != 0u, prow[r] * S + (R.sf[r] & 0xFFFFu), cls, fate, hops);
  }
  wave_sync();  // the staging area is free for the next chunk
}

template <int SCAN>
__global__ __launch_bounds__(kOrThreads, 3) void error_origins_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint64_t* __restrict__ trace_ptr, uint64_t n_traces,
    OrArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kOBytes * kOrWaves];
  const int lane = threadIdx.x & (kWave - 1);
  unsigned char* wsm = smem + (threadIdx.x / kWave) * kOBytes;
  uint32_t* lctr = reinterpret_cast<uint32_t*>(origins_lds);
  const uint32_t n_ctr = (kTabs + 1u) * a.E;
  if (a.lds) {
    for (uint32_t k = threadIdx.x; k < n_ctr; k += kOrThreads) lctr[k] = 0u;
    __syncthreads();
  }
  uint32_t n_err = 0, n_loop = 0;
  walk_traces<kOrWaves, 4, Regs>(
      trace_ptr, n_traces, a.ctr,
      [&](const Chunk& c, Regs& R) __attribute__((always_inline)) {
        load_regs(span_id, parent, svcfl, c, lane, R);
      },
      [&](const Chunk& c, uint32_t, uint64_t, const Regs& R) __attribute__((always_inline)) {
        origins_chunk<SCAN>(wsm, lctr, lane, c, R, a, n_err, n_loop);
      },
      // longer than kStage: listed for error_origins_big_kernel
      [&](uint64_t t, uint32_t n) __attribute__((always_inline)) {
        list_long(a.big, a.big_list, a.big_cap, lane, t, n);
      });
  for (int o = 32; o > 0; o >>= 1) {
    n_err += (uint32_t)__shfl_xor((int)n_err, o);
    n_loop += (uint32_t)__shfl_xor((int)n_loop, o);
  }
  if (lane == 0) {
    if (n_err) atomicAdd(a.misc, (unsigned long long)n_err);
    if (n_loop) atomicAdd(a.misc + 1, (unsigned long long)n_loop);
  }
  if (a.lds) {
    __syncthreads();
    const uint32_t n_sum = kTabs * a.E;
    for (uint32_t k = threadIdx.x; k < n_ctr; k += kOrThreads) {
      const uint32_t v = lctr[k];
      if (!v) continue;
      if (k < n_sum) atomicAdd(&a.tab[k], (unsigned long long)v);
      else atomicMax(&a.hmax[k - n_sum], v);
    }
  }
}

// ---- long traces ----------------------------------------------------------
// One workgroup per listed trace (tickets).  Parent positions come from
// walk.h's windowed LDS id table (big_parents).  Child-error bits go by
// agent-scope atomicOr into the zeroed scratch words; the jump word (ancestor
// position or the fate of a closed chain, hops) lives in global scratch in two
// buffers: a round reads one and writes the other.  A span's words are written
// by the thread that owns the span (position % kBigThreads) with agent-scope
// stores and read by any thread with agent-scope loads, all served by L2;
// every wave waits for its own stores before the barrier that separates two
// rounds (sweep_sync).  ceil(log2 L) rounds, fewer when a round finds no open
// span; what stays open is LOOP.  The edge row of a span stays with its owner
// (plain stores and loads).
__global__ __launch_bounds__(kBigThreads) void error_origins_big_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint64_t* __restrict__ trace_ptr, OrArgs a) {
  __shared__ unsigned long long bkey[kBigSlots];
  __shared__ uint32_t bpos[kBigSlots];
  __shared__ unsigned long long s_j;
  const int tid = threadIdx.x;
  const uint64_t nbig = a.big[0] < a.big_cap ? a.big[0] : a.big_cap;
  const uint32_t S = a.S;
  unsigned long long n_err = 0ull, n_loop = 0ull;
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
    uint32_t* kid = a.l_kid + off;
    uint32_t* lrow = a.l_row + off;
    unsigned long long* wA = a.l_w[0] + off;
    unsigned long long* wB = a.l_w[1] + off;
    // A trace without a flag (one sweep of 4 B per span): nothing to classify,
    // and its per-span columns read 0 from the call's memset.
    bool flagged = false;
    for (uint64_t i = tid; i < L; i += kBigThreads) flagged |= sf_err(svcfl[lo + i]);
    if (!__syncthreads_or(flagged)) continue;
    // ---- parent positions, child-error bits, links
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
      uint64_t pid[kBigPer];
      uint32_t pp[kBigPer];  // parent position in the trace (kNone: none)
      big_parents(span_id, parent, lo, L, b0, tid, bkey, bpos, pid, pp);
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
        if (i >= L) continue;
        const uint32_t sf = svcfl[lo + i];
        const bool has = pp[r] != kNone && pp[r] != (uint32_t)i;
        uint32_t p = S, psf = 0u;
        if (pid[r] != 0ull) {
          p = S + 1u;
          if (pp[r] != kNone) {
            psf = svcfl[lo + pp[r]];
            p = psf & 0xFFFFu;
          }
        }
        lrow[i] = p * S + (sf & 0xFFFFu);
        uint32_t anc = kBigSurf, h = 0u;  // (a span without the flag: never read by another)
        if (sf_err(sf)) {
          if (has)
            __hip_atomic_fetch_or(&kid[pp[r]], kBigKid, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
          if (has && sf_err(psf)) {
            anc = pp[r];
            h = 1u;
          } else {
            anc = has ? kBigCont : kBigSurf;
          }
        }
        astore(&wA[i], (unsigned long long)anc | (unsigned long long)h << 32);
      }
    }
    sweep_sync();
    // ---- pointer jumping between the two buffers
    for (uint64_t reach = 1; reach < L; reach <<= 1) {
      bool open = false;
      for (uint64_t i = tid; i < L; i += kBigThreads) {
        unsigned long long w = aload(&wA[i]);
        const uint32_t anc = (uint32_t)w;
        if (anc < kBigCont) {
          const unsigned long long wa = aload(&wA[anc]);
          w = (wa & 0xFFFFFFFFull) | ((w >> 32) + (wa >> 32)) << 32;
          open = true;
        }
        astore(&wB[i], w);
      }
      wait_stores();
      const bool any = __syncthreads_or(open);
      unsigned long long* x = wA;
      wA = wB;
      wB = x;
      if (!any) break;
    }
    // ---- outputs
    for (uint64_t i = tid; i < L; i += kBigThreads) {
      const unsigned long long w = aload(&wA[i]);
      const bool e = sf_err(svcfl[lo + i]), k = (aload(&kid[i]) & kBigKid) != 0u;
      const uint32_t anc = (uint32_t)w;
      const bool done = anc >= kBigCont;
      const uint32_t cls = e ? (k ? ANOMOD_ERR_PROPAGATED : ANOMOD_ERR_ORIGIN)
                             : (k ? ANOMOD_ERR_ABSORBER : ANOMOD_ERR_CLEAN);
      const uint32_t closed = anc == kBigSurf ? ANOMOD_FATE_SURFACED : ANOMOD_FATE_CONTAINED;
      const uint32_t fate = !e ? 0u : done ? closed : ANOMOD_FATE_LOOP;
      const uint32_t hops = e && done ? (uint32_t)(w >> 32) : 0u;
      if (a.state) a.state[lo + i] = (uint8_t)(cls | fate << 2);
      if (a.hops) a.hops[lo + i] = hops;
      if (cls == ANOMOD_ERR_CLEAN) continue;
      n_err += e ? 1ull : 0ull;
      n_loop += fate == ANOMOD_FATE_LOOP ? 1ull : 0ull;
      count_span(a, nullptr, false, lrow[i], cls, fate, hops);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_err += __shfl_xor(n_err, o);
    n_loop += __shfl_xor(n_loop, o);
  }
  if ((tid & (kWave - 1)) == 0) {
    if (n_err) atomicAdd(a.misc, n_err);
    if (n_loop) atomicAdd(a.misc + 1, n_loop);
  }
}

using WalkFn = void (*)(const uint64_t*, const uint64_t*, const uint32_t*, const uint64_t*,
                        uint64_t, OrArgs);

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_error_origins_spans(anomod_ctx* ctx, const anomod_spans* spans,
                               anomod_error_origins* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_error_origins_spans: NULL argument");
  const uint32_t S = out->n_services;
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "span service index %u >= n_services %u", spans->max_svc, S);
  ANOMOD_REQUIRE(ctx, spans->n_spans < max_launch_spans(), "%llu spans: at most 2^32 - 2 per call",
                 (unsigned long long)spans->n_spans);
  if (!spans->grouped) {
    set_error(ctx, "span set is not grouped by trace: anomod_spans_group first");
    return ANOMOD_ESTATE;
  }
  if (int rc = bind(ctx)) return rc;

  const uint64_t n = spans->n_spans, nt = spans->n_traces;
  const size_t E = (size_t)(S + ANOMOD_ROOT_ROWS) * S;
  uint64_t* h_tab[kTabs] = {out->origin, out->propagated, out->stopped,
                            out->surfaced, out->absorbers, out->hops_sum};
  out->error_spans = 0;
  out->loop_spans = 0;
  // the spans that lie in traces (spans outside every trace are in no class:
  // their columns read 0)
  uint64_t in_traces[2];
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  if (in_traces[1] == in_traces[0]) {  // no span in any trace
    for (uint64_t* p : h_tab)
      if (p) memset(p, 0, E * 8);
    if (out->hops_max) memset(out->hops_max, 0, E * 4);
    if (out->span_state && n) memset(out->span_state, 0, n);
    if (out->span_hops && n) memset(out->span_hops, 0, n * 4);
    return ANOMOD_OK;
  }

  // The call's workspace: a block of words (dynamic-tail counter, long-trace
  // counters, order-probe scratch) and a block of the two scalars and the
  // tables (zeroed together, downloaded in one copy) | the per-span columns
  // (when asked for, zeroed) | the long-trace list | the listed spans'
  // child-error words (zeroed), rows and jump words (24 B per span).  The long
  // traces are counted first.
  CallWorkspace ws{ctx};
  const auto al = CallWorkspace::al;
  unsigned long long nlong[2] = {0ull, 0ull};
  if (int rc = ws.take(&ws.words, 256, "error-origins")) return rc;
  auto* words = static_cast<unsigned long long*>(ws.words);
  if (int rc = count_long_traces(ctx, spans, words, nlong)) return rc;
  const size_t nl = (size_t)nlong[1];
  const size_t tab_bytes = 16 + E * 8 * kTabs + E * 4, b_tab = al(tab_bytes);
  const size_t b_state = out->span_state ? al(n) : 0, b_hops = out->span_hops ? al(n * 4) : 0;
  const size_t b_list = al(nlong[0] * 16), b_l4 = al(nl * 4), b_l8 = al(nl * 8);
  if (int rc = ws.take(&ws.block, b_tab + b_state + b_hops + b_list + 2 * b_l4 + 2 * b_l8,
                       "error-origins"))
    return rc;
  OrArgs a{};
  a.misc = ws.carve<unsigned long long>(b_tab);
  a.tab = a.misc + 2;
  a.hmax = reinterpret_cast<uint32_t*>(a.tab + E * kTabs);
  a.state = out->span_state ? ws.carve<uint8_t>(b_state) : nullptr;
  a.hops = out->span_hops ? ws.carve<uint32_t>(b_hops) : nullptr;
  a.big_list = ws.carve<unsigned long long>(b_list);
  a.l_kid = ws.carve<uint32_t>(b_l4);
  a.l_row = ws.carve<uint32_t>(b_l4);
  a.l_w[0] = ws.carve<unsigned long long>(b_l8);
  a.l_w[1] = ws.carve<unsigned long long>(b_l8);
  a.ctr = words;
  a.big = words + 1;
  a.big_cap = nlong[0];
  a.S = S;
  a.E = (uint32_t)E;
  const size_t lds_ctr = E * 4 * (kTabs + 1);
  a.lds = lds_ctr <= kDynLdsBudget ? 1u : 0u;
  const size_t dyn = a.lds ? lds_ctr : 0;

  int scan = kScanFwd;
  if (int rc = pick_walk_scan(ctx, spans, S, words + 4, &scan)) return rc;
  const WalkFn fn = scan == kScanFwd     ? error_origins_kernel<kScanFwd>
                    : scan == kScanSplit ? error_origins_kernel<kScanSplit>
                                         : error_origins_kernel<kScanBidir>;
  if (kOBytes * kOrWaves + dyn > 64u * 1024u) {  // above the default limit of a workgroup
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    (void)hipGetLastError();
  }
  uint64_t grid = 0;
  if (int rc = walk_grid(ctx, fn, kOrThreads, &grid, dyn)) return rc;
  log_walk_kernel("error-origins", "error_origins_kernel", scan, nlong[0]);
  ANOMOD_HIP(ctx, hipMemsetAsync(words, 0, 64, ctx->stream));  // every counter
  ANOMOD_HIP(ctx, hipMemsetAsync(a.misc, 0, tab_bytes, ctx->stream));
  if (a.state) ANOMOD_HIP(ctx, hipMemsetAsync(a.state, 0, n, ctx->stream));
  if (a.hops) ANOMOD_HIP(ctx, hipMemsetAsync(a.hops, 0, n * 4, ctx->stream));
  if (nl) ANOMOD_HIP(ctx, hipMemsetAsync(a.l_kid, 0, nl * 4, ctx->stream));
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kOrThreads), dyn, ctx->stream, spans->span_id,
                     spans->parent_span_id, spans->svc_flags, spans->trace_ptr, nt, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (nlong[0]) {
    hipLaunchKernelGGL(error_origins_big_kernel,
                       dim3((unsigned)std::min<uint64_t>(nlong[0], 2ull * ctx->num_cus)),
                       dim3(kBigThreads), 0, ctx->stream, spans->span_id, spans->parent_span_id,
                       spans->svc_flags, spans->trace_ptr, a);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  std::vector<unsigned long long> h((tab_bytes + 7) / 8);  // scalars | u64 tables | hops_max
  ANOMOD_HIP(ctx,
             hipMemcpyAsync(h.data(), a.misc, tab_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (a.state)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->span_state, a.state, n, hipMemcpyDeviceToHost, ctx->stream));
  if (a.hops)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->span_hops, a.hops, n * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out->error_spans = h[0];
  out->loop_spans = h[1];
  for (uint32_t k = 0; k < kTabs; ++k)
    if (h_tab[k]) memcpy(h_tab[k], h.data() + 2 + E * k, E * 8);
  if (out->hops_max) memcpy(out->hops_max, h.data() + 2 + E * kTabs, E * 4);
  return ANOMOD_OK;
}

}  // extern "C"
