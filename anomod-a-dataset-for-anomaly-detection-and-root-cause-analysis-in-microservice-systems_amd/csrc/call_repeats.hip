// Call repeats of a grouped span set: how often one parent span called the
// same callee service more than once — retries after a failure, retry storms,
// an N+1 loop over a result set.
//
//   par(i)   = self time's parent (self_time.hip): the first span of i's
//              trace, in position order, whose span_id equals i's
//              parent_span_id; a root, an orphan and a self-reference have
//              none and are heads
//   G(j, c)  = { i : par(i) = j, svc[i] = c }: one parent span's calls to one
//              callee service, n its size, e its error-flagged members; all
//              members share the edge row svc[j] * S + c
//   e_end(m) = start_us[m] + max(dur_us[m], 1); member i is counted in
//              after_error iff start_us[i] != 0 and start_us[i] >= the least
//              e_end over the error-flagged members with a start time (an
//              e_end past 2^64 - 1 lies after every start)
//
// One chunk walk (walk.h: persistent waves, <= 256 spans / <= 64 whole traces
// per chunk, buffer loads, the columns of chunk c+1 in flight while chunk c is
// resolved) reads 20 B per span (svc|flags 4, id 8, parent id 8), 28 B with
// the start column; the duration of an error-flagged member with a start time
// is fetched where it is needed.  Per chunk: (a) every span finds its parent
// and writes a key word (parent position | svc << 8 | has-parent bit); (b) a
// span with a parent finds its group's leader — the first position of its
// trace whose key word equals its own, a forward scan over the u32 keys — and
// adds 1 | err << 16 to the leader's group word (ds_add; the timed form also
// takes the minimum e_end - 1 into the leader's u64 slot, ds_min_u64); (c) the
// leaders classify their group and count, every member reads its group's size
// and, in the timed form, compares its start with the leader's minimum.
//
// Row counters, all privatised per workgroup in LDS and flushed once with u64
// global adds (a u32 sum that wraps carries 2^32 into the global word at once):
// a handful of rows takes most of the counts, and global atomics on a hot word
// serialise.  groups, repeats, repeated and the largest n are what a group
// touches (every group the first, every group of n >= 2 the others: a fifth of
// SocialNetwork's groups): a dense table of 4 E u32 words where that fits the
// dynamic-LDS budget.  The others touch few words of a wide table — retried /
// recovered / exhausted (n >= 2 and a failure), after_error and the size
// histogram from bucket 2 (n >= 4) on: a sparse table of kSpSlots (word index,
// count) pairs, claimed by ds_cmpst and probed linearly; an add that finds no
// slot in kSpProbes steps goes to the global word itself.  A table too wide
// for the dense form counts its sums in the sparse table too and takes the
// size by a global atomicMax, only when it exceeds what the row holds.  The
// host derives size_hist[.][0] = groups - repeated, size_hist[.][1] = repeated
// - the buckets above it, and the size 1 of size_max.  Results never depend on
// which form ran.
//
// Traces longer than a chunk are listed by the walk and resolved by
// call_repeats_big_kernel, one workgroup per listed trace.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kRpWaves = 4;
constexpr int kRpThreads = kRpWaves * kWave;
// dynamic LDS of the dense counters: two workgroups of 35.75 + 40 KiB fit a CU's 160 KiB
constexpr uint32_t kDynLdsBudget = 40u * 1024u;
constexpr uint32_t kLdsSums = 3;  // groups | repeats | repeated, the first tables of RpArgs::tab
constexpr uint32_t kLdsTabs = 4;  // ... | largest n
// the sparse counters: (u64 word index into RpArgs::tab, count) pairs
constexpr uint32_t kSpSlots = 1024, kSpProbes = 8, kSpEmpty = 0xFFFFFFFFu;
static_assert(kSpSlots == 1u << 10, "sparse_add takes the top 10 bits of its hash");
constexpr uint32_t kTabs = 7;     // u64 tables
enum { kTGroups, kTRepeats, kTRepeated, kTRetried, kTRecovered, kTExhausted, kTAfter };
constexpr uint32_t kHistBins = ANOMOD_REPEAT_BINS;

// Per-wave LDS (every offset a multiple of 16).
constexpr int kRSid = 0;  // u64 span ids [kStage + kScanSlack], or two u32 planes of that length
constexpr int kRKey = kRSid + (kStage + (int)kScanSlack) * 8;  // u32 key words [kStage + kScanSlack]
constexpr int kRGrp = kRKey + (kStage + (int)kScanSlack) * 4;  // u32 group words [kStage]
constexpr int kRSvc = kRGrp + kStage * 4;                      // u16 services [kStage]
constexpr int kRFlag = kRSvc + kStage * 2;                     // u8 trace-start flags [kStage]
constexpr int kRMin = kRFlag + kStage;                         // u64 least e_end - 1 [kStage] (timed)
constexpr int kRBytes = kRMin;
constexpr int kRBytesTimed = kRMin + kStage * 8;
static_assert(kRKey % 16 == 0 && kRGrp % 16 == 0 && kRMin % 16 == 0 && kRBytes % 16 == 0,
              "wave staging must stay 16-B aligned");
static_assert(2 * (kRBytesTimed * kRpWaves + kSpSlots * 8u + kDynLdsBudget) <= 160u * 1024u,
              "LDS of a CU");

// Key word: parent position in the chunk | svc << 8 | kHas.  A head's key is
// 0: it equals no member's.  Group word: n | e << 16 — a chunk holds kStage
// spans, so neither half can carry into the other.
constexpr uint32_t kPosMask = 0xFFu, kSvcShift = 8, kHas = 1u << 24, kErrOne = 1u << 16;
static_assert(kStage <= 256, "the key's position field holds a chunk position");
static_assert(kStage <= 0xFFFF, "16 bits hold the members and the failures of a chunk's group");
// the leader scan reads kKeyScan keys per step, up to that many past the trace end
constexpr uint32_t kKeyScan = 16;
static_assert(kKeyScan <= kScanSlack && kKeyScan < 32, "key scan step: the staging slack");

constexpr unsigned long long kNoSlot = ~0ull;
constexpr unsigned long long kNoEnd = ~0ull;  // no error-flagged member with a start time (error_last)

struct RpArgs {
  unsigned long long* ctr;       // trace-segment counter of the dynamic tail
  unsigned long long* big;       // [0] listed traces, [1] their spans, [2] ticket
  unsigned long long* tab;       // u64 [kTabs][E]: groups | repeats | repeated | retried |
                                 // recovered | exhausted | after_error, then hist
  unsigned long long* hist;      // u64 [E][kHistBins] = tab + kTabs * E (buckets 0 and 1 are
                                 // derived by the host)
  uint32_t* smax;                // u32 [E] largest n >= 2
  uint32_t* gsize;               // [n_spans] or NULL (zeroed: heads write nothing)
  uint8_t* after;                // [n_spans] or NULL (zeroed)
  const uint32_t* dur_us;        // timed form
  const uint64_t* start_us;      // timed form (NULL: untimed)
  unsigned long long* big_list;  // (trace, scratch offset) per listed trace
  uint64_t big_cap;              // entries big_list holds
  unsigned long long* l_slot;    // [long spans] the span's group slot (kNoSlot: a head)
  unsigned long long* h_key;     // [2 * long spans] group keys (zeroed: empty)
  unsigned long long* h_ne;      // [2 * long spans] n | e << 32 (zeroed)
  unsigned long long* h_min;     // [2 * long spans] least e_end - 1 (all ones), timed form
  uint32_t S, E;
  uint32_t lds;                  // the chunk kernel's dense LDS counters (else the sparse table)
};

// A workgroup's LDS counters.
struct Counters {
  uint32_t* dense;  // [kLdsTabs][E], or NULL
  uint32_t* skey;   // [kSpSlots] word index into RpArgs::tab (kSpEmpty: free)
  uint32_t* scnt;   // [kSpSlots]
};

extern __shared__ __align__(16) unsigned char repeats_lds[];

template <bool TIMED>
struct Regs {
  uint64_t sid[kPer], pid[kPer];
  uint32_t sf[kPer];  // svc | flags << 16
  uint64_t st[TIMED ? kPer : 1];
};

template <bool TIMED>
__device__ __forceinline__ void load_regs(const uint64_t* __restrict__ span_id,
                                          const uint64_t* __restrict__ parent,
                                          const uint32_t* __restrict__ svcfl,
                                          const uint64_t* __restrict__ start_us, const Chunk& c,
                                          int lane, Regs<TIMED>& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by call_repeats_big_kernel
  const auto rsf = rsrc(svcfl + c.base, n * 4u);
  const auto rsid = rsrc(span_id + c.base, n * 8u);
  const auto rpid = rsrc(parent + c.base, n * 8u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.sid[r] = bload64(rsid, i * 8u);
    R.pid[r] = bload64(rpid, i * 8u);
  }
#pragma unroll
  for (int r = 0; r < kPer; ++r)
    R.sf[r] = bload32(rsf, ((uint32_t)lane + (uint32_t)(r * kWave)) * 4u);
  if constexpr (TIMED) {
    const auto rst = rsrc(start_us + c.base, n * 8u);
#pragma unroll
    for (int r = 0; r < kPer; ++r)
      R.st[r] = bload64(rst, ((uint32_t)lane + (uint32_t)(r * kWave)) * 8u);
  }
}

__device__ __forceinline__ bool sf_err(uint32_t sf) {
  return ((sf >> 16) & ANOMOD_FLAG_ERROR) != 0u;
}

// The last microsecond a failed call occupies, e_end - 1 = start + max(dur, 1)
// - 1: a member follows the failure iff its start is greater.  Kept instead of
// e_end so that every u64 start compares right: kNoEnd (all ones) is followed
// by nothing, whether it stands for "no failure" or is a failure's own last
// microsecond.  False when it lies past 2^64 - 1 (after every start).
__device__ __forceinline__ bool error_last(uint64_t start, uint32_t dur, unsigned long long& last) {
  last = start + (dur ? dur - 1u : 0u);
  return last >= start;
}

// Size bucket min(floor(log2 n), 7) of a group of n >= 1.
__device__ __forceinline__ uint32_t size_bucket(uint32_t n) {
  const uint32_t b = 31u - (uint32_t)__clz((int)n);
  return b < kHistBins - 1u ? b : kHistBins - 1u;
}

// v more in the u64 word a.tab[idx] (idx < 15 E < 2^32 - 1), through the
// workgroup's sparse table.  A wrapped u32 count carries into the global word.
__device__ __forceinline__ void sparse_add(const RpArgs& a, const Counters& C, uint32_t idx,
                                           uint32_t v) {
  uint32_t sl = (idx * 0x9E3779B1u) >> 22 & (kSpSlots - 1u);
  for (uint32_t p = 0; p < kSpProbes; ++p, sl = (sl + 1u) & (kSpSlots - 1u)) {
    const uint32_t seen = atomicCAS(&C.skey[sl], kSpEmpty, idx);
    if (seen == kSpEmpty || seen == idx) {
      const uint32_t old = atomicAdd(&C.scnt[sl], v);
      if (old + v < old) atomicAdd(&a.tab[idx], 1ull << 32);
      return;
    }
  }
  atomicAdd(&a.tab[idx], (unsigned long long)v);
}

// What one group of n members, e of them error-flagged, adds to the tables of
// its row.
__device__ __forceinline__ void count_group(const RpArgs& a, const Counters& C, uint32_t row,
                                            uint32_t n, uint32_t e) {
  const uint32_t E = a.E;
  auto add = [&](uint32_t t, uint32_t v) __attribute__((always_inline)) {
    if (C.dense) {
      const uint32_t old = atomicAdd(&C.dense[t * E + row], v);
      if (old + v < old) atomicAdd(&a.tab[(size_t)t * E + row], 1ull << 32);
    } else {
      sparse_add(a, C, t * E + row, v);
    }
  };
  add(kTGroups, 1u);
  if (n < 2u) return;
  add(kTRepeats, n - 1u);
  add(kTRepeated, 1u);
  if (C.dense)
    atomicMax(&C.dense[kLdsSums * E + row], n);
  else if (n > aload(&a.smax[row]))  // (the word only grows: a stale read costs one atomic)
    atomicMax(&a.smax[row], n);
  if (e) {
    sparse_add(a, C, kTRetried * E + row, 1u);
    sparse_add(a, C, (e < n ? kTRecovered : kTExhausted) * E + row, 1u);
  }
  if (n >= 4u) sparse_add(a, C, kTabs * E + row * kHistBins + size_bucket(n), 1u);
}

// The workgroup's counters: cleared (a barrier orders it before the first
// add), and flushed into the global tables (after a barrier).
__device__ __forceinline__ void clear_counters(const RpArgs& a, const Counters& C, int threads) {
  if (C.dense)
    for (uint32_t k = threadIdx.x; k < kLdsTabs * a.E; k += threads) C.dense[k] = 0u;
  for (uint32_t k = threadIdx.x; k < kSpSlots; k += threads) {
    C.skey[k] = kSpEmpty;
    C.scnt[k] = 0u;
  }
}
__device__ __forceinline__ void flush_counters(const RpArgs& a, const Counters& C, int threads) {
  if (C.dense) {
    const uint32_t n_sum = kLdsSums * a.E, n_ctr = kLdsTabs * a.E;
    for (uint32_t k = threadIdx.x; k < n_ctr; k += threads) {
      const uint32_t v = C.dense[k];
      if (!v) continue;
      if (k < n_sum) atomicAdd(&a.tab[k], (unsigned long long)v);
      else atomicMax(&a.smax[k - n_sum], v);
    }
  }
  for (uint32_t k = threadIdx.x; k < kSpSlots; k += threads)
    if (C.skey[k] != kSpEmpty && C.scnt[k]) atomicAdd(&a.tab[C.skey[k]], (unsigned long long)C.scnt[k]);
}

// First position of [a, b) whose key word equals key (-1: none), kKeyScan
// words per step: find_first over the u32 keys.
__device__ __forceinline__ int find_key(const uint32_t* lkey, uint32_t a, uint32_t b,
                                        uint32_t key) {
  for (uint32_t q0 = a; q0 < b; q0 += kKeyScan) {
    uint32_t v[kKeyScan];
#pragma unroll
    for (uint32_t j = 0; j < kKeyScan; ++j) v[j] = lkey[q0 + j];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < kKeyScan; ++j) m |= (v[j] == key ? 1u : 0u) << j;
    const uint32_t hi = (b - q0) < kKeyScan ? (b - q0) : kKeyScan;  // >= 1
    m &= (1u << hi) - 1u;
    if (m) return (int)(q0 + __ffs(m) - 1u);
  }
  return -1;
}

template <int SCAN, bool TIMED>
__device__ __forceinline__ void repeats_chunk(unsigned char* wsm, const Counters& C, int lane,
                                              const Chunk& c, const Regs<TIMED>& R,
                                              const RpArgs& a) {
  auto* lsid = reinterpret_cast<uint64_t*>(wsm + kRSid);
  auto* llo = reinterpret_cast<uint32_t*>(wsm + kRSid);
  uint32_t* lhi = llo + (kStage + kScanSlack);
  auto* lkey = reinterpret_cast<uint32_t*>(wsm + kRKey);
  auto* lgrp = reinterpret_cast<uint32_t*>(wsm + kRGrp);
  auto* lsvc = reinterpret_cast<uint16_t*>(wsm + kRSvc);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kRFlag);
  auto* lmin = reinterpret_cast<unsigned long long*>(wsm + kRMin);  // (timed form only)
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
    lgrp[i] = 0u;
    if constexpr (TIMED) lmin[i] = kNoEnd;
  }
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);  // (its wave syncs also publish the staging)
  // (a) parents and key words.  (Lanes past n hold zeros from the buffer
  // loads: no parent reference, key 0.)
  uint32_t key[kPer], ta[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    key[r] = 0u;
    ta[r] = 0u;
    if (R.pid[r] != 0ull) {
      uint32_t tb;
      trace_bounds(Sm, r, lane, c.n, ta[r], tb);
      const int q = find_parent<SCAN>(lsid, llo, lhi, ta[r], tb, i, R.pid[r]);
      if (q >= 0 && (uint32_t)q != i) key[r] = (uint32_t)q | (R.sf[r] & 0xFFFFu) << kSvcShift | kHas;
    }
    lkey[i] = key[r];
  }
  wave_sync();
  // (b) leaders; members and failures into the leader's group word.
  uint32_t lead[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    lead[r] = i;
    if (!key[r]) continue;
    lead[r] = (uint32_t)find_key(lkey, ta[r], i + 1u, key[r]);  // (found: the span's own at the latest)
    const bool err = sf_err(R.sf[r]);
    atomicAdd(&lgrp[lead[r]], err ? 1u | kErrOne : 1u);
    if constexpr (TIMED) {
      unsigned long long last;
      if (err && R.st[r] != 0ull && error_last(R.st[r], a.dur_us[c.base + i], last))
        atomicMin(&lmin[lead[r]], last);
    }
  }
  wave_sync();
  // (c) leaders count their group; members read its size and its first failure's end.
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if (!key[r]) continue;
    const uint32_t w = lgrp[lead[r]];
    const uint32_t n = w & 0xFFFFu, e = w >> 16;
    const uint32_t row = (uint32_t)lsvc[key[r] & kPosMask] * S + (R.sf[r] & 0xFFFFu);
    if (a.gsize) a.gsize[c.base + i] = n;
    if (lead[r] == i) count_group(a, C, row, n, e);
    if constexpr (TIMED) {
      if (R.st[r] != 0ull && R.st[r] > lmin[lead[r]]) {
        sparse_add(a, C, kTAfter * a.E + row, 1u);
        if (a.after) a.after[c.base + i] = 1;
      }
    }
  }
  wave_sync();  // the staging area is free for the next chunk
}

template <int SCAN, bool TIMED>
__global__ __launch_bounds__(kRpThreads, 3) void call_repeats_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint64_t* __restrict__ trace_ptr, uint64_t n_traces,
    RpArgs a) {
  constexpr int kWaveBytes = TIMED ? kRBytesTimed : kRBytes;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kWaveBytes * kRpWaves];
  const int lane = threadIdx.x & (kWave - 1);
  unsigned char* wsm = smem + (threadIdx.x / kWave) * kWaveBytes;
  __shared__ uint32_t sp_key[kSpSlots], sp_cnt[kSpSlots];
  const Counters C{a.lds ? reinterpret_cast<uint32_t*>(repeats_lds) : nullptr, sp_key, sp_cnt};
  clear_counters(a, C, kRpThreads);
  __syncthreads();
  walk_traces<kRpWaves, 4, Regs<TIMED>>(
      trace_ptr, n_traces, a.ctr,
      [&](const Chunk& c, Regs<TIMED>& R) __attribute__((always_inline)) {
        load_regs<TIMED>(span_id, parent, svcfl, a.start_us, c, lane, R);
      },
      [&](const Chunk& c, uint32_t, uint64_t, const Regs<TIMED>& R) __attribute__((always_inline)) {
        repeats_chunk<SCAN, TIMED>(wsm, C, lane, c, R, a);
      },
      // longer than kStage: listed for call_repeats_big_kernel
      [&](uint64_t t, uint32_t n) __attribute__((always_inline)) {
        list_long(a.big, a.big_list, a.big_cap, lane, t, n);
      });
  __syncthreads();
  flush_counters(a, C, kRpThreads);
}

// ---- long traces ----------------------------------------------------------
// One workgroup per listed trace (tickets).  Parent positions come from
// walk.h's windowed LDS id table (big_parents).  The groups of a trace of L
// spans live in a hash table of 2 L slots in global scratch (load <= 1/2, its
// own region per listed trace): a slot's key is parent position << 32 | svc +
// 1 (never 0: an empty slot), claimed by an agent-scope compare-and-swap and
// found again by linear probing; members add 1 | err << 32 to the slot's count
// word and, in the timed form, take the minimum e_end - 1 into its third word —
// u32 n and u32 e, nothing packed in 16 bits: a long group can hold more than
// 65,535 members.  The slot is the group's identity, so no result depends on
// the order of the inserts.  After the sweep barrier (sweep_sync) one sweep
// over the table classifies the groups and one over the spans reads each
// member's group; shared words are read by agent-scope loads, all served by
// L2.  A span's slot index stays with its owner (position % kBigThreads; plain
// stores and loads).  The counters go through the workgroup's sparse table:
// beside the 48 KiB of big_parents' id table no dense one fits a workgroup's
// default 64 KiB at TrainTicket's width.
__device__ __forceinline__ uint64_t group_slot(unsigned long long key, uint64_t n_slots) {
  return __umul64hi(key * 0x9E3779B97F4A7C15ull, n_slots);
}

template <bool TIMED>
__global__ __launch_bounds__(kBigThreads) void call_repeats_big_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint64_t* __restrict__ trace_ptr, RpArgs a) {
  __shared__ unsigned long long bkey[kBigSlots];
  __shared__ uint32_t bpos[kBigSlots];
  __shared__ unsigned long long s_j;
  const int tid = threadIdx.x;
  const uint64_t nbig = a.big[0] < a.big_cap ? a.big[0] : a.big_cap;
  const uint32_t S = a.S;
  __shared__ uint32_t sp_key[kSpSlots], sp_cnt[kSpSlots];
  const Counters C{nullptr, sp_key, sp_cnt};  // (the loop's first barrier orders the clear)
  clear_counters(a, C, kBigThreads);
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
    const uint64_t n_slots = 2ull * L;
    unsigned long long* slot = a.l_slot + off;
    unsigned long long* hkey = a.h_key + 2 * off;
    unsigned long long* hne = a.h_ne + 2 * off;
    unsigned long long* hmin = TIMED ? a.h_min + 2 * off : nullptr;
    // ---- parent positions, group slots, members and failures
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
      uint64_t pid[kBigPer];
      uint32_t pp[kBigPer];  // parent position in the trace (kNone: none)
      big_parents(span_id, parent, lo, L, b0, tid, bkey, bpos, pid, pp);
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
        if (i >= L) continue;
        if (pp[r] == kNone || pp[r] == (uint32_t)i) {  // a head
          slot[i] = kNoSlot;
          continue;
        }
        const uint32_t sf = svcfl[lo + i];
        const unsigned long long key = (unsigned long long)pp[r] << 32 | ((sf & 0xFFFFu) + 1u);
        uint64_t sl = group_slot(key, n_slots);
        while (true) {  // (ends: the table holds at most L keys in 2 L slots)
          unsigned long long seen = 0ull;
          if (__hip_atomic_compare_exchange_strong(&hkey[sl], &seen, key, __ATOMIC_RELAXED,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
              seen == key)
            break;
          sl = sl + 1u < n_slots ? sl + 1u : 0u;
        }
        slot[i] = sl;
        const bool err = sf_err(sf);
        __hip_atomic_fetch_add(&hne[sl], err ? 1ull | 1ull << 32 : 1ull, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (TIMED) {
          const uint64_t st = a.start_us[lo + i];
          unsigned long long last;
          if (err && st != 0ull && error_last(st, a.dur_us[lo + i], last))
            __hip_atomic_fetch_min(&hmin[sl], last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    sweep_sync();
    // ---- the groups: every claimed slot is one
    for (uint64_t sl = tid; sl < n_slots; sl += kBigThreads) {
      const unsigned long long key = aload(&hkey[sl]);
      if (key == 0ull) continue;
      const unsigned long long ne = aload(&hne[sl]);
      const uint32_t psvc = svcfl[lo + (uint32_t)(key >> 32)] & 0xFFFFu;
      count_group(a, C, psvc * S + ((uint32_t)key - 1u), (uint32_t)ne, (uint32_t)(ne >> 32));
    }
    // ---- the members
    if (a.gsize || TIMED) {
      for (uint64_t i = tid; i < L; i += kBigThreads) {
        const unsigned long long sl = slot[i];
        if (sl == kNoSlot) continue;
        if (a.gsize) a.gsize[lo + i] = (uint32_t)aload(&hne[sl]);
        if constexpr (TIMED) {
          const uint64_t st = a.start_us[lo + i];
          if (st != 0ull && st > aload(&hmin[sl])) {
            const unsigned long long key = aload(&hkey[sl]);
            const uint32_t psvc = svcfl[lo + (uint32_t)(key >> 32)] & 0xFFFFu;
            sparse_add(a, C, kTAfter * a.E + psvc * S + ((uint32_t)key - 1u), 1u);
            if (a.after) a.after[lo + i] = 1;
          }
        }
      }
    }
  }
  __syncthreads();
  flush_counters(a, C, kBigThreads);
}

using WalkFn = void (*)(const uint64_t*, const uint64_t*, const uint32_t*, const uint64_t*,
                        uint64_t, RpArgs);

WalkFn walk_kernel(int scan, bool timed) {
  if (timed)
    return scan == kScanFwd     ? call_repeats_kernel<kScanFwd, true>
           : scan == kScanSplit ? call_repeats_kernel<kScanSplit, true>
                                : call_repeats_kernel<kScanBidir, true>;
  return scan == kScanFwd     ? call_repeats_kernel<kScanFwd, false>
         : scan == kScanSplit ? call_repeats_kernel<kScanSplit, false>
                              : call_repeats_kernel<kScanBidir, false>;
}

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_call_repeats_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_call_repeats* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_call_repeats_spans: NULL argument");
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
  const bool timed = spans->start_us != nullptr;
  uint64_t* h_tab[kTabs] = {out->groups,    out->repeats,   out->repeated,   out->retried,
                            out->recovered, out->exhausted, out->after_error};
  out->grouped_spans = 0;
  out->max_size = 0;
  out->timed = timed ? 1u : 0u;
  // the spans that lie in traces (spans outside every trace are in no group:
  // their columns read 0)
  uint64_t in_traces[2];
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  if (in_traces[1] == in_traces[0]) {  // no span in any trace
    for (uint64_t* p : h_tab)
      if (p) memset(p, 0, E * 8);
    if (out->size_hist) memset(out->size_hist, 0, E * kHistBins * 8);
    if (out->size_max) memset(out->size_max, 0, E * 4);
    if (out->span_group_size && n) memset(out->span_group_size, 0, n * 4);
    if (out->span_after_error && n) memset(out->span_after_error, 0, n);
    return ANOMOD_OK;
  }

  // The call's workspace: a block of words (dynamic-tail counter, long-trace
  // counters, order-probe scratch) and a block of the tables (zeroed together,
  // downloaded in one copy) | the per-span columns (when asked for, zeroed) |
  // the long-trace list | the listed spans' slot indices (8 B per span) and
  // their traces' group tables: keys and count words (zeroed) and, in the
  // timed form, the least e_end - 1 (all ones), 2 slots per span.  The long traces
  // are counted first.
  CallWorkspace ws{ctx};
  const auto al = CallWorkspace::al;
  unsigned long long nlong[2] = {0ull, 0ull};
  if (int rc = ws.take(&ws.words, 256, "call-repeats")) return rc;
  auto* words = static_cast<unsigned long long*>(ws.words);
  if (int rc = count_long_traces(ctx, spans, words, nlong)) return rc;
  const size_t nl = (size_t)nlong[1];
  const size_t tab_bytes = E * 8 * kTabs + E * 8 * kHistBins + E * 4, b_tab = al(tab_bytes);
  const size_t b_size = out->span_group_size ? al(n * 4) : 0;
  const size_t b_after = out->span_after_error && timed ? al(n) : 0;
  const size_t b_list = al(nlong[0] * 16), b_slot = al(nl * 8), b_hash = al(nl * 32);
  const size_t b_min = timed ? al(nl * 16) : 0;
  if (int rc = ws.take(&ws.block, b_tab + b_size + b_after + b_list + b_slot + b_hash + b_min,
                       "call-repeats"))
    return rc;
  RpArgs a{};
  a.tab = ws.carve<unsigned long long>(b_tab);
  a.hist = a.tab + E * kTabs;
  a.smax = reinterpret_cast<uint32_t*>(a.hist + E * kHistBins);
  a.gsize = b_size ? ws.carve<uint32_t>(b_size) : nullptr;
  a.after = b_after ? ws.carve<uint8_t>(b_after) : nullptr;
  a.big_list = ws.carve<unsigned long long>(b_list);
  a.l_slot = ws.carve<unsigned long long>(b_slot);
  a.h_key = ws.carve<unsigned long long>(b_hash);
  a.h_ne = a.h_key + 2 * nl;
  a.h_min = timed ? ws.carve<unsigned long long>(b_min) : nullptr;
  a.dur_us = spans->dur_us;
  a.start_us = timed ? spans->start_us : nullptr;
  a.ctr = words;
  a.big = words + 1;
  a.big_cap = nlong[0];
  a.S = S;
  a.E = (uint32_t)E;
  const size_t lds_ctr = E * 4 * kLdsTabs;
  a.lds = lds_ctr <= kDynLdsBudget ? 1u : 0u;
  const size_t dyn = a.lds ? lds_ctr : 0;

  int scan = kScanFwd;
  if (int rc = pick_walk_scan(ctx, spans, S, words + 4, &scan)) return rc;
  const WalkFn fn = walk_kernel(scan, timed);
  const size_t wave_bytes = timed ? kRBytesTimed : kRBytes;
  if (wave_bytes * kRpWaves + kSpSlots * 8u + dyn > 64u * 1024u) {  // above the default limit of a workgroup
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    (void)hipGetLastError();
  }
  uint64_t grid = 0;
  if (int rc = walk_grid(ctx, fn, kRpThreads, &grid, dyn)) return rc;
  log_walk_kernel("call-repeats", "call_repeats_kernel", scan, nlong[0]);
  ANOMOD_HIP(ctx, hipMemsetAsync(words, 0, 64, ctx->stream));  // every counter
  ANOMOD_HIP(ctx, hipMemsetAsync(a.tab, 0, tab_bytes, ctx->stream));
  if (a.gsize) ANOMOD_HIP(ctx, hipMemsetAsync(a.gsize, 0, n * 4, ctx->stream));
  if (a.after) ANOMOD_HIP(ctx, hipMemsetAsync(a.after, 0, n, ctx->stream));
  if (nl) ANOMOD_HIP(ctx, hipMemsetAsync(a.h_key, 0, nl * 32, ctx->stream));
  if (nl && timed) ANOMOD_HIP(ctx, hipMemsetAsync(a.h_min, 0xFF, nl * 16, ctx->stream));
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kRpThreads), dyn, ctx->stream, spans->span_id,
                     spans->parent_span_id, spans->svc_flags, spans->trace_ptr, nt, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (nlong[0]) {
    const dim3 big_grid((unsigned)std::min<uint64_t>(nlong[0], 2ull * ctx->num_cus));
    if (timed)
      hipLaunchKernelGGL(call_repeats_big_kernel<true>, big_grid, dim3(kBigThreads), 0,
                         ctx->stream, spans->span_id, spans->parent_span_id, spans->svc_flags,
                         spans->trace_ptr, a);
    else
      hipLaunchKernelGGL(call_repeats_big_kernel<false>, big_grid, dim3(kBigThreads), 0,
                         ctx->stream, spans->span_id, spans->parent_span_id, spans->svc_flags,
                         spans->trace_ptr, a);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  std::vector<unsigned long long> h((tab_bytes + 7) / 8);  // u64 tables | size_hist | size_max
  ANOMOD_HIP(ctx, hipMemcpyAsync(h.data(), a.tab, tab_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (a.gsize)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->span_group_size, a.gsize, n * 4, hipMemcpyDeviceToHost,
                                   ctx->stream));
  if (a.after)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->span_after_error, a.after, n, hipMemcpyDeviceToHost,
                                   ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (out->span_after_error && !timed && n) memset(out->span_after_error, 0, n);
  // What the kernels leave to the host: the groups of size 1 (bucket 0, and
  // their size_max) and of sizes 2 and 3 (bucket 1), and the scalars.
  const unsigned long long* groups = h.data();
  const unsigned long long* repeats = groups + E;
  const unsigned long long* repeated = repeats + E;
  unsigned long long* hist = h.data() + E * kTabs;
  auto* smax = reinterpret_cast<uint32_t*>(hist + E * kHistBins);
  uint64_t total = 0;
  uint32_t top = 0;
  for (size_t r = 0; r < E; ++r) {
    unsigned long long from4 = 0;
    for (uint32_t b = 2; b < kHistBins; ++b) from4 += hist[r * kHistBins + b];
    hist[r * kHistBins] = groups[r] - repeated[r];
    hist[r * kHistBins + 1] = repeated[r] - from4;
    if (groups[r] && smax[r] == 0u) smax[r] = 1u;
    total += groups[r] + repeats[r];
    top = std::max(top, smax[r]);
  }
  out->grouped_spans = total;
  out->max_size = top;
  for (uint32_t k = 0; k < kTabs; ++k)
    if (h_tab[k]) memcpy(h_tab[k], h.data() + E * k, E * 8);
  if (out->size_hist) memcpy(out->size_hist, hist, E * kHistBins * 8);
  if (out->size_max) memcpy(out->size_max, smax, E * 4);
  return ANOMOD_OK;
}

}  // extern "C"
