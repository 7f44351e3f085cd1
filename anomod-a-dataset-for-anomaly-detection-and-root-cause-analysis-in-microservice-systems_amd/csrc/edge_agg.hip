// Call-graph edge aggregation — the hot path.
//
// Replaces the per-span Python loops of
//   SN_collection-scripts/Dataset/trace_data/jaeger_to_csv.py:21-90
//     (parent = spanID of the first CHILD_OF reference, :34-38; service
//      resolved through processID, :45-46; duration_us, :83)
//   TT_collection-scripts/T-Dataset/trace_collector.py:401-481
//     (_build_span_records: trace-local parent resolution; roots = spans
//      whose parent is not in the trace, :443)
//   TT_collection-scripts/T-Dataset/enhanced_trace_collector.py:216-296
//     (per-service counts / error counts / latency stats)
// and adds what the reference never computed: a (parent service -> child
// service) edge table with an integer log-linear latency histogram per edge
// and p50/p99 taken with the reference's nearest-rank index convention
// (monitor_http_responses.py:180-190, rank = (n*q)//100).
//
// Design (MI355X):
//  * one pass over the span SoA in HBM: 8 B span_id + 8 B parent_span_id +
//    4 B svc|flags + 4 B dur_us per span + 8 B trace_ptr per trace, read
//    with buffer loads (one scalar descriptor per column and chunk, 32-bit
//    lane offsets, out-of-chunk lanes read 0 — no per-lane address math);
//  * persistent grid, one 1024-thread workgroup per CU; every wave owns a
//    contiguous range of traces and walks it in chunks of <= 256 spans /
//    <= 64 traces, so parent resolution is trace-local in that wave's LDS
//    staging area (no inter-wave synchronisation inside the loop);
//  * parent lookup: ordered scan of the trace's staged ids (first match, the
//    reference rule), 10 ids per 5 x ds_read2_b64 step (a per-wave LDS hash
//    with ds_cmpst inserts measured 1.7x slower, and scanning a lane's 4
//    slots in lockstep 1.1-1.4x slower: register pressure);
//  * the E x 896 histogram does not fit LDS, so each workgroup privatises it
//    in an 8 Ki-slot LDS hash table (2048 buckets x 4 u32 keys, one
//    ds_read_b128 per lookup; u32 counts in a parallel array), flushed once
//    with u64 atomics;
//  * per-edge error/sum/min/max live in LDS (E <= 512) and are flushed once;
//  * all merges are integer adds / min / max: results are bit-exact and
//    independent of geometry, scheduling and shard count;
//  * a resident set is walked once: its first aggregation also stores every
//    span's parent row (u16, anomod_spans::parent_row), and its later ones
//    stream svc_flags + dur_us + the row, 10 B/span, into the same tables
//    (edge_row_kernel) — no ids, no trace bounds, no scan;
//  * a set whose first table touches few edges and bins (<= 512 edges with
//    spans, <= 32 Ki bins in their ranges: SN, LONG) also gets a u16 edge-code
//    column on its fifth aggregation, and from the sixth on streams codes +
//    dur_us, 6 B/span, into a directly indexed LDS histogram
//    (edge_dense_kernel) — no hash table.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>


#include "chunk.h"
#include "common.h"
#include "radix.h"

namespace anomod {
uint64_t env_cap(const char* name, uint64_t floor);  // edge_stream.hip
namespace {

using namespace chunk;
constexpr int kWavesPerWG = 16;
constexpr int kThreads = kWave * kWavesPerWG;
// LDS histogram table, two forms in the same 64 KiB (see ht_* below).
enum HistForm { kHtHbm = 0, kHtPair = 1, kHtCompact = 2,
                kHtKeys = 3 };  // exact-quantile mode: write (edge << 32 | dur) per span
constexpr int kPairBucketLog2 = 11;  // pair: 2048 buckets of 4 slots, keys | counts
constexpr uint32_t kPairSlots = 4u << kPairBucketLog2;
constexpr int kPairMaxProbe = 48;
constexpr int kCmpBucketLog2 = 12;   // compact: 4096 buckets of 4 (key | count << kb) slots
constexpr uint32_t kCmpSlots = 4u << kCmpBucketLog2;
constexpr int kHtBytes = 65536;
static_assert(kPairSlots * 8 == kHtBytes && kCmpSlots * 4 == kHtBytes, "64 KiB table");
constexpr uint32_t kLdsEdges = 512;
constexpr uint32_t kBins = ANOMOD_HIST_BINS;
// Experiment-only ablations (never set in the shipped build): 1 = no stats,
// 2 = no histogram (3 = neither: the span's values are only kept alive, so the
// record-based streams still load their columns), 4 = no parent lookup, 16 =
// stream the columns only (the chunk walk).  32 / 64 / 96 are 1 / 2 / 3 for
// edge_dense_kernel alone: the walk and the row stream keep their full tables,
// so the set still learns its layout and reaches the dense kernel.
#ifndef ANOMOD_ABL
#define ANOMOD_ABL 0
#endif

// LDS carve (bytes, every offset a multiple of 16).
constexpr int kOffHt = 0;                      // u32 keys (pair) | u32 slots (compact); 0 = empty
constexpr int kOffHc = kOffHt + (int)kPairSlots * 4;  // u32 counts (pair form)
constexpr uint32_t kSumReps = 8;                         // u64 sum replicas per edge
constexpr int kOffSum = kOffHt + kHtBytes;               // u64 [kLdsEdges][kSumReps]
// Per-edge stats in LDS, two forms.  Direct (E <= kLdsEdges: every SN-width
// table): (min, max) pairs and error counts indexed by edge.  Slot-hashed
// (wider tables, e.g. TrainTicket: E = 48 * 46 = 2208): kSlotEdges 16-B
// entries {edge + 1, min, max, errors} found by hashing the edge (linear
// probing, ds_cmpst inserts), the sum replicas indexed by slot — a trace set
// touches far fewer edges than E.
constexpr uint32_t kSlotEdges = 512;
// the slot form's sums reuse the direct form's replica area
constexpr uint32_t kSlotSumReps = (kLdsEdges * kSumReps) / kSlotEdges;
static_assert(kSlotSumReps >= 1 && (kSlotSumReps & (kSlotSumReps - 1)) == 0, "slot sum replicas");
constexpr int kOffMm = kOffSum + (int)(kLdsEdges * kSumReps) * 8;  // u32 (min, max) pairs | slots
constexpr int kOffErr = kOffMm + (int)kLdsEdges * 8;     // u32 error counts (direct form)
// Wide direct form (kLdsEdges < E <= kWideEdges, e.g. TrainTicket: E = 48 *
// 46 = 2208): one 16-B entry {u64 sum, u32 min, u32 max} per edge + u32
// error counts, indexed by edge (no slot hashing, no sum replicas).
constexpr uint32_t kWideEdges = 2304;
constexpr int kOffWideErr = kOffSum + (int)kWideEdges * 16;
constexpr int kStatsEnd = std::max({kOffMm + (int)(kLdsEdges * 12),   // direct
                                    kOffMm + (int)(kSlotEdges * 16),  // slot
                                    kOffWideErr + (int)kWideEdges * 4});  // wide
// u32 control words: [0] pair-form inserts that found their probe chain full
// (counted in HBM; added to tab.ovf once per workgroup at the flush)
constexpr int kOffCtl = (kStatsEnd + 15) & ~15;
constexpr int kOffWave = kOffCtl + 16;
// A workgroup of a first (form-unknown) aggregation whose pair table turned
// away this many inserts stops: its waves hand their remaining traces to the
// compact-form resume launch (edge_agg_kernel, kModeAuto / kModeResume).
constexpr uint32_t kSatFails = 64;
// kModeWideScan: kModeNormal with the wide parent scan (process_chunk)
enum LaunchMode : uint32_t { kModeNormal = 0, kModeAuto = 1, kModeResume = 2, kModeWideScan = 3 };
enum StatsForm { kStHbm = 0, kStDirect = 1, kStSlot = 2, kStWide = 3 };
constexpr int kWSid = 0;                          // u64 span ids [kStage + kScanSlack] (scan slack)
constexpr int kWSvc = kWSid + (kStage + chunk::kScanSlack) * 8;  // u16 services [kStage + 8]
constexpr int kWFlag = kWSvc + (kStage + 8) * 2;  // u8 trace-start flags [kStage]
constexpr int kWAuto = kWFlag + kStage;           // u64: kModeAuto, first trace of the chunk
constexpr int kWBytes = kWAuto + 16;
constexpr int kLdsBytes = kOffWave + kWavesPerWG * kWBytes;
static_assert(kWBytes % 16 == 0, "wave staging must stay 16-B aligned");
static_assert(kLdsBytes <= 160 * 1024, "LDS budget");

struct Table {
  unsigned long long* hist;  // [E * kBins]
  unsigned long long* err;   // [E]
  unsigned long long* sum;   // [E]
  unsigned int* mn;          // [E]
  unsigned int* mx;          // [E]
  unsigned long long* ctr;   // trace-segment counter of the dynamic tail (zeroed per launch)
  uint32_t kb;               // key bits of a histogram slot (count in the 32 - kb above)
  unsigned long long* keys;  // kHtKeys: [n_spans] edge << 32 | dur, by span position
  unsigned long long* big;       // long traces: [0] listed, [1] / [2] tickets of the
                                 // resolve / record kernels
  unsigned long long* big_list;  // long traces: trace indices
  uint16_t* bpar;            // parent rows by span position (S root, S + 1 orphan): call scratch
                             // the long-trace pass fills for its listed spans, or the set's
                             // parent-row column, which the chunk walk (ROWS) fills too
  uint64_t t_base;           // trace index of this launch's first trace
  unsigned long long* ovf;   // [0] spans whose pair-form probe chain was full (counted in
                             // HBM), [1] workgroups that stopped at a saturated pair table
  unsigned long long* left;  // kModeAuto: [2 j], [2 j + 1] = trace range j a stopped wave left
  unsigned long long* nleft; // [0] ranges left, [1] resume ticket
  uint32_t mode;             // LaunchMode
  uint32_t occupancy;        // compact form: report the fullest workgroup's used slots
                             // (tab.ovf[1], atomic max) at the flush
};

struct Cols {
  const uint64_t* __restrict__ span_id;
  const uint64_t* __restrict__ parent;
  const uint32_t* __restrict__ svcfl;  // svc | flags << 16
  const uint32_t* __restrict__ dur;
};

// Histogram increment of key = edge*kBins + bin + 1 in the workgroup's LDS.
//
// Pair form (E <= kLdsEdges, SN width): 2048 buckets of 4 slots, keys and u32
// counts in separate arrays, so one ds_read_b128 fetches a key's home
// bucket; a resident key costs that read + one fire-and-forget ds_add_u32 (0
// for lanes that miss, so no branch around it).  With the SN mix a
// workgroup holds ~3.6 k keys in 8 Ki slots and 0.02 % of spans miss their
// home bucket.  A launch covers < 2^32 spans, so u32 counts do not wrap.
//
// Compact form (wider tables: TrainTicket E = 2208, ~21 k keys per
// workgroup): 16 Ki u32 slots = key | count << kb (kb = the key's bit width,
// 21 for TrainTicket) in 4096 buckets; a key lives in its home bucket or the
// next one, both fetched by two ds_read_b128 in one round trip (95 % / 3.3 %
// of TrainTicket spans, simulated).  The add returns the old slot: a count
// field that was all ones wrapped, and that lane moves 2^(32-kb) counts to
// HBM (exact: one lane per wrap).  When both buckets are full of other keys
// the span counts in HBM at once (1.7 %), so no lane walks a probe chain.
//
// New keys take the first empty slot in probe order from the bucket start
// (ds_cmpst; a key never moves).
__device__ __forceinline__ uint32_t ht_hash(uint32_t key) { return key * 0x9E3779B1u; }

__device__ __attribute__((noinline)) void ht_insert_pair(uint32_t* hk, uint32_t* hc, uint32_t key,
                                                         uint32_t s,
                                                         unsigned long long* __restrict__ ghist,
                                                         uint32_t* ctl) {
  for (int probe = 0; probe < kPairMaxProbe; ++probe) {
    uint32_t cur = __hip_atomic_load(&hk[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == 0u) {
      const uint32_t prev = atomicCAS(&hk[s], 0u, key);
      cur = prev == 0u ? key : prev;
    }
    if (cur == key) {
      atomicAdd(&hc[s], 1u);
      return;
    }
    s = (s + 1u) & (kPairSlots - 1u);
  }
  atomicAdd(&ghist[key - 1u], 1ull);
  // counted per workgroup in LDS (one HBM add at the flush: a device-wide
  // counter bumped per span was itself a contended hot spot); a first
  // aggregation stops the workgroup at kSatFails, and the host switches the
  // set to the compact form
  atomicAdd(&ctl[0], 1u);
}

__device__ __forceinline__ void ht_wrap(uint32_t old, uint32_t key, uint32_t kb,
                                        unsigned long long* __restrict__ ghist) {
  if ((old >> kb) == (0xFFFFFFFFu >> kb)) atomicAdd(&ghist[key - 1u], 1ull << (32u - kb));
}

// Compact form, key not in its two buckets but one of them had room: claim
// the first empty slot of the 8 (or count where another lane just put it).
__device__ __attribute__((noinline)) void ht_insert_cmp(uint32_t* hk, uint32_t key, uint32_t b0,
                                                        uint32_t b1, uint32_t kb,
                                                        unsigned long long* __restrict__ ghist) {
  const uint32_t kmask = 0xFFFFFFFFu >> (32u - kb);
  for (int q = 0; q < 8; ++q) {
    const uint32_t s = (q < 4 ? b0 : b1) + (uint32_t)(q & 3);
    uint32_t cur = __hip_atomic_load(&hk[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == 0u) {
      const uint32_t prev = atomicCAS(&hk[s], 0u, key | (1u << kb));
      if (prev == 0u) return;  // new slot, count 1
      cur = prev;
    }
    if ((cur & kmask) == key) {
      ht_wrap(atomicAdd(&hk[s], 1u << kb), key, kb, ghist);
      return;
    }
  }
  atomicAdd(&ghist[key - 1u], 1ull);
}

using u32x2 = uint32_t __attribute__((ext_vector_type(2)));
using u32x4 = uint32_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t slot_home(uint32_t edge) {
  return (edge * 0x9E3779B1u) >> (32 - 9);  // kSlotEdges = 512
}

// The slot of `key` = edge + 1 past its home (linear probing; inserted on
// first sight); UINT32_MAX when kSlotProbe slots are taken by other edges
// (that span's stats then go to HBM).
constexpr int kSlotProbe = 32;
__device__ __attribute__((noinline)) uint32_t slot_find(uint32_t* st4, uint32_t key) {
  uint32_t s = slot_home(key - 1u) & ~3u;  // the home bucket first
  for (int probe = 0; probe < kSlotProbe; ++probe) {
    uint32_t cur = __hip_atomic_load(&st4[4u * s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cur == 0u) {
      const uint32_t prev = atomicCAS(&st4[4u * s], 0u, key);
      cur = prev == 0u ? key : prev;
    }
    if (cur == key) return s;
    s = (s + 1u) & (kSlotEdges - 1u);
  }
  return 0xFFFFFFFFu;
}

// The edge's stats position and current (min, max) in LDS, read before the
// span's histogram update so this read and the bucket read share one LDS
// round trip.  slot: the edge itself (direct), its table slot (slot form;
// UINT32_MAX = not at home, resolved by slot_find after the bucket read).
struct StatPeek {
  u32x2 mm;
  uint32_t slot;
};

template <int ST>
__device__ __forceinline__ StatPeek stat_peek(const unsigned char* smem, uint32_t edge) {
  if constexpr (ST == kStDirect && !(ANOMOD_ABL & 1)) {
    return {*reinterpret_cast<const u32x2*>(smem + kOffMm + 8u * edge), edge};
  } else if constexpr (ST == kStWide && !(ANOMOD_ABL & 1)) {
    return {*reinterpret_cast<const u32x2*>(smem + kOffSum + 16u * edge + 8u), edge};
  } else if constexpr (ST == kStSlot && !(ANOMOD_ABL & 1)) {
    // the home bucket of 4 entries (64 B, one round trip): simulated on the
    // TrainTicket mix, ~0 % of spans find their edge elsewhere (2.1 % with
    // 2-entry buckets, and a row with one such lane waits for its probe)
    const uint32_t s = slot_home(edge) & ~3u;
    const u32x4* ent = reinterpret_cast<const u32x4*>(smem + kOffMm + 16u * s);
    const u32x4 e0 = ent[0], e1 = ent[1], e2 = ent[2], e3 = ent[3];
    const uint32_t k = edge + 1u;
    const uint32_t j = e0.x == k ? 0u : e1.x == k ? 1u : e2.x == k ? 2u : e3.x == k ? 3u : 4u;
    const u32x4 e = j == 0u ? e0 : j == 1u ? e1 : j == 2u ? e2 : e3;
    return {u32x2{e.y, e.z}, j < 4u ? s + j : 0xFFFFFFFFu};
  } else {
    return {u32x2{0u, 0u}, edge};
  }
}

template <int ST>
__device__ __forceinline__ void stat_add(unsigned char* smem, uint32_t edge, uint32_t d,
                                         uint32_t fl, const Table& tab, StatPeek pk) {
  if constexpr (ANOMOD_ABL & 1) return;
  auto* lsum = reinterpret_cast<unsigned long long*>(smem + kOffSum);
  if constexpr (ST == kStDirect) {
    // Lanes of one wave-instruction share few edges, and same-address LDS
    // atomics serialise: the sum is spread over kSumReps replicas by lane,
    // and min / max (`mm`, read by stat_peek: a broadcast read) are only
    // updated when the span beats them — after warm-up almost never.  A stale
    // read only costs a redundant atomic.
    auto* lmm = reinterpret_cast<uint32_t*>(smem + kOffMm);
    auto* lerr = reinterpret_cast<uint32_t*>(smem + kOffErr);
    atomicAdd(&lsum[edge * kSumReps + (__lane_id() & (kSumReps - 1u))], (unsigned long long)d);
    if (d < pk.mm.x) atomicMin(&lmm[2u * edge], d);
    if (d > pk.mm.y) atomicMax(&lmm[2u * edge + 1u], d);
    if (fl & ANOMOD_FLAG_ERROR) atomicAdd(&lerr[edge], 1u);
    return;
  }
  if constexpr (ST == kStWide) {
    unsigned char* ent = smem + kOffSum + 16u * edge;
    atomicAdd(reinterpret_cast<unsigned long long*>(ent), (unsigned long long)d);
    if (d < pk.mm.x) atomicMin(reinterpret_cast<uint32_t*>(ent + 8), d);
    if (d > pk.mm.y) atomicMax(reinterpret_cast<uint32_t*>(ent + 12), d);
    if (fl & ANOMOD_FLAG_ERROR) atomicAdd(reinterpret_cast<uint32_t*>(smem + kOffWideErr) + edge, 1u);
    return;
  }
  if constexpr (ST == kStSlot) {
    uint32_t s = pk.slot;
    u32x2 mm = pk.mm;
    auto* st4 = reinterpret_cast<uint32_t*>(smem + kOffMm);
    if (s == 0xFFFFFFFFu) {
      s = slot_find(st4, edge + 1u);
      mm = u32x2{0xFFFFFFFFu, 0u};  // unknown: the atomics below decide
    }
    if (s != 0xFFFFFFFFu) {
      atomicAdd(&lsum[s * kSlotSumReps + (__lane_id() & (kSlotSumReps - 1u))],
                (unsigned long long)d);
      if (d < mm.x) atomicMin(&st4[4u * s + 1u], d);
      if (d > mm.y) atomicMax(&st4[4u * s + 2u], d);
      if (fl & ANOMOD_FLAG_ERROR) atomicAdd(&st4[4u * s + 3u], 1u);
      return;
    }
  }
  atomicAdd(&tab.sum[edge], (unsigned long long)d);
  atomicMin(&tab.mn[edge], d);
  atomicMax(&tab.mx[edge], d);
  if (fl & ANOMOD_FLAG_ERROR) atomicAdd(&tab.err[edge], 1ull);
}

// One span.
template <int HT, int ST>
__device__ __forceinline__ void record(unsigned char* smem, uint32_t edge, uint32_t d, uint32_t fl,
                                       const Table& tab) {
  if constexpr ((ANOMOD_ABL & 3) == 3) {  // keep the loads, do nothing
    if ((edge ^ d ^ (fl << 20)) == 0x9E3779B9u) tab.err[0] = d;
    return;
  }
  const StatPeek pk = stat_peek<ST>(smem, edge);
  const uint32_t key = edge * kBins + hist_bin(d) + 1u;
  if constexpr ((ANOMOD_ABL & 2) || HT == kHtHbm) {
    if constexpr (!(ANOMOD_ABL & 2)) atomicAdd(&tab.hist[key - 1u], 1ull);
    stat_add<ST>(smem, edge, d, fl, tab, pk);
  } else if constexpr (HT == kHtPair) {
    // plain 16-B read (other waves insert concurrently; a stale empty slot
    // only sends the lane down the insert path, which re-reads)
    auto* hk = reinterpret_cast<uint32_t*>(smem + kOffHt);
    auto* hc = reinterpret_cast<uint32_t*>(smem + kOffHc);
    const uint32_t s0 = (ht_hash(key) >> (32 - kPairBucketLog2)) * 4u;
    const u32x4 bk = *reinterpret_cast<const u32x4*>(hk + s0);
    const uint32_t j = bk.x == key ? 0u : bk.y == key ? 1u : bk.z == key ? 2u : 3u;
    const bool hit = (j < 3u) | (bk.w == key);
    atomicAdd(&hc[s0 + j], hit ? 1u : 0u);
    stat_add<ST>(smem, edge, d, fl, tab, pk);
    if (!hit) ht_insert_pair(hk, hc, key, s0, tab.hist, reinterpret_cast<uint32_t*>(smem + kOffCtl));
  } else {  // kHtCompact
    auto* hk = reinterpret_cast<uint32_t*>(smem + kOffHt);
    const uint32_t kmask = 0xFFFFFFFFu >> (32u - tab.kb);
    const uint32_t b = ht_hash(key) >> (32 - kCmpBucketLog2);
    const uint32_t s0 = b * 4u, s1 = ((b + 1u) & ((1u << kCmpBucketLog2) - 1u)) * 4u;
    const u32x4 x = *reinterpret_cast<const u32x4*>(hk + s0);
    const u32x4 y = *reinterpret_cast<const u32x4*>(hk + s1);
    const uint32_t j = (x.x & kmask) == key   ? s0
                       : (x.y & kmask) == key ? s0 + 1u
                       : (x.z & kmask) == key ? s0 + 2u
                       : (x.w & kmask) == key ? s0 + 3u
                       : (y.x & kmask) == key ? s1
                       : (y.y & kmask) == key ? s1 + 1u
                       : (y.z & kmask) == key ? s1 + 2u
                       : (y.w & kmask) == key ? s1 + 3u
                                              : 0xFFFFFFFFu;
    const bool hit = j != 0xFFFFFFFFu;
    const uint32_t old = atomicAdd(&hk[hit ? j : s0], hit ? (1u << tab.kb) : 0u);
    const bool room = (x.x == 0u) | (x.y == 0u) | (x.z == 0u) | (x.w == 0u) | (y.x == 0u) |
                      (y.y == 0u) | (y.z == 0u) | (y.w == 0u);
    stat_add<ST>(smem, edge, d, fl, tab, pk);
    if (hit) {
      ht_wrap(old, key, tab.kb, tab.hist);
    } else if (room) {
      ht_insert_cmp(hk, key, s0, s1, tab.kb, tab.hist);
    } else {
      atomicAdd(&tab.hist[key - 1u], 1ull);
    }
  }
}

// Span columns of a chunk held in registers while the previous chunk is
// processed (software pipeline, one chunk ahead).
struct Regs {
  uint64_t sid[kPer], pid[kPer];
  uint32_t dur[kPer], sf[kPer];  // sf = svc | flags << 16
};

__device__ __forceinline__ void load_regs(const Cols& col, const Chunk& c, int lane, Regs& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by the long-trace pass
  const auto rsid = rsrc(col.span_id + c.base, n * 8u);
  const auto rpid = rsrc(col.parent + c.base, n * 8u);
  const auto rsf = rsrc(col.svcfl + c.base, n * 4u);
  const auto rdur = rsrc(col.dur + c.base, n * 4u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.sid[r] = bload64(rsid, i * 8u);
    R.pid[r] = bload64(rpid, i * 8u);
    R.sf[r] = bload32(rsf, i * 4u);
    R.dur[r] = bload32(rdur, i * 4u);
  }
}

// First span of [a, b) whose id equals pid: kScan ids per step (ds_read2_b64
// from the trace start itself), matches folded into a bit mask.  First match
// in trace order (the reference rule: jaeger_to_csv.py:34-38 /
// trace_collector.py:424-443).
constexpr uint32_t kScan = 10;  // ids compared per step (kScan / 2 x ds_read2_b64)
static_assert(kScan % 2 == 0 && kScan <= 16, "scan step");
// The forward scan's step in the compact-form instantiations that also store
// parent rows (process_chunk ROWS): those forms sit at the 128-register limit
// with kScan, and the row store's scalar descriptor pushed them over it (1-2
// spilled registers); 8 ids per step fits.  They run once per set.
constexpr uint32_t kScanRows = 8;

template <uint32_t SCAN = kScan>
__device__ __forceinline__ int find_parent(const uint64_t* lsid, uint32_t a, uint32_t b,
                                           uint64_t pid) {
  static_assert(SCAN % 2 == 0 && SCAN <= chunk::kScanSlack, "scan step");
  for (uint32_t q0 = a; q0 < b; q0 += SCAN) {
    uint64_t v[SCAN];
#pragma unroll
    for (uint32_t j = 0; j < SCAN; ++j) v[j] = lsid[q0 + j];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < SCAN; ++j) m |= (v[j] == pid ? 1u : 0u) << j;
    const uint32_t hi = (b - q0) < SCAN ? (b - q0) : SCAN;  // >= 1
    m &= (1u << hi) - 1u;
    if (m) return (int)(q0 + __ffs(m) - 1u);
  }
  return -1;
}

// Scan widths of the bidirectional parent scan: (kFwd, kBwd) = (6, 4) for
// collector-ordered traces of tens of spans (SN / TrainTicket: 8 / 8 measured
// 2-10 % slower there); sets holding traces longer than a chunk first took
// (8, 8) (LONG: random ancestors in 128- and 256-span traces, 7.52 vs 8.09
// ms).  The TrainTicket-width and long-trace instantiations then gained from
// building the matches with selects (one LDS round trip per step): TT 2^27
// 17.8-18.4 vs 18.5-18.7 ms, LONG 2^23 7.24-7.29 vs 7.60-7.69
// (profiles/r05_experiments/parent_scan_sel_widths.log), and again from the
// split-word form (chunk.h find_parent_split: ids staged as u32 planes, low
// words compared, the candidate confirmed on its high word), whose cheaper
// steps pay for wider ones: TT 12 / 4 16.3-16.7 ms, LONG 12 / 4 6.96-7.04
// (split_scan_*.log).  The SN pair form gained nothing measurable from either
// and keeps the mask form over u64 ids at (kFwd, kBwd).
constexpr uint32_t kLFwd = 12, kLBwd = 4;  // the long-trace sets' widths
constexpr uint32_t kWFwd = 12, kWBwd = 4;  // TrainTicket width, split scan
// ROWS: also store every span's parent row into the set's parent-row column
// (tab.bpar, by span position): one buffer store per span row through a
// descriptor on the chunk's part of the column, with the lane offsets of the
// loads (lanes past the chunk are dropped by the descriptor's bound).
template <int HT, int ST, bool UNI, bool WIDE = false, bool ROWS = false>
__device__ __forceinline__ void process_chunk(unsigned char* smem, unsigned char* wsm, int lane,
                                              const Chunk& c, const Regs& R, uint32_t S,
                                              const Table& tab) {
  auto* lsid = reinterpret_cast<uint64_t*>(wsm + kWSid);
  auto* lsvc = reinterpret_cast<uint16_t*>(wsm + kWSvc);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kWFlag);
  // Unique-id sets in the TrainTicket-width and long-trace instantiations
  // stage ids as two u32 planes and scan low words (find_parent_split);
  // everything else stages u64 ids: unique-id sets then scan from both ends
  // (find_parent_bidir), other sets forward for the first match (find_parent).
  constexpr bool kSplit = UNI && (WIDE || ST == kStWide);
  auto* llo = reinterpret_cast<uint32_t*>(wsm + kWSid);
  uint32_t* lhi = llo + (kStage + chunk::kScanSlack);
  if constexpr (ANOMOD_ABL & 16) {  // stream only: keep the loads, do nothing
    uint64_t x = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) x ^= R.sid[r] ^ R.pid[r] ^ R.sf[r] ^ ((uint64_t)R.dur[r] << 7);
    if (x == 0x0123456789ABCDEFull) tab.err[0] = x;
    return;
  }
  // Stage ids / services (lanes past n hold zeros from the buffer loads);
  // mark trace starts.
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if constexpr (kSplit) {
      llo[i] = (uint32_t)R.sid[r];
      lhi[i] = (uint32_t)(R.sid[r] >> 32);
    } else {
      lsid[i] = R.sid[r];
    }
    lsvc[i] = (uint16_t)R.sf[r];
  }
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    uint32_t p = S;  // ROOT
    if (i < c.n && R.pid[r] != 0ull) {
      p = S + 1u;  // ORPHAN unless found in the trace
      if constexpr (!(ANOMOD_ABL & 4)) {
        uint32_t a, b;
        trace_bounds(Sm, r, lane, c.n, a, b);
        int q;
        if constexpr (kSplit && WIDE)
          q = find_parent_split<kLFwd, kLBwd>(llo, lhi, a, b, i, R.pid[r]);
        else if constexpr (kSplit)
          q = find_parent_split<kWFwd, kWBwd>(llo, lhi, a, b, i, R.pid[r]);
        else
          q = UNI ? find_parent_bidir<kFwd, kBwd>(lsid, a, b, i, R.pid[r])
                  : find_parent<(ROWS && HT == kHtCompact) ? kScanRows : kScan>(lsid, a, b,
                                                                                 R.pid[r]);
        if (q >= 0) p = lsvc[q];
      } else {  // ablation: a parent-like edge without the lookup (keeps key diversity)
        p = ((R.sf[r] & 0xFFFFu) + 1u + (uint32_t)(R.pid[r] & 1u)) % S;
      }
    }
    if constexpr (ROWS)
      __builtin_amdgcn_raw_buffer_store_b16((short)p, rsrc(tab.bpar + c.base, c.n * 2u),
                                            (int)(i * 2u), 0, 0);
    if constexpr (HT == kHtKeys) {
      if (i < c.n)
        tab.keys[c.base + i] = ((unsigned long long)(p * S + (R.sf[r] & 0xFFFFu)) << 32) | R.dur[r];
    } else {
      if (i < c.n) record<HT, ST>(smem, p * S + (R.sf[r] & 0xFFFFu), R.dur[r], R.sf[r] >> 16, tab);
    }
  }
  wave_sync();
}

// The workgroup's private LDS tables (histogram + per-edge stats), shared by
// the chunk walk and the long-trace pass: zeroed at the start, merged into
// the device table with integer atomics (order-free) at the end.
template <int HT, int ST>
__device__ __forceinline__ void tables_init(unsigned char* smem, uint32_t E, int tid) {
  if (tid < 4) reinterpret_cast<uint32_t*>(smem + kOffCtl)[tid] = 0u;
  if constexpr (HT == kHtPair || HT == kHtCompact) {
    auto* hk = reinterpret_cast<uint32_t*>(smem + kOffHt);  // both forms: 64 KiB of zeros
    for (uint32_t s = tid; s < (uint32_t)kHtBytes / 4u; s += kThreads) hk[s] = 0u;
  }
  if constexpr (ST == kStDirect) {
    auto* lsum = reinterpret_cast<unsigned long long*>(smem + kOffSum);
    auto* lmm = reinterpret_cast<uint32_t*>(smem + kOffMm);
    auto* lerr = reinterpret_cast<uint32_t*>(smem + kOffErr);
    for (uint32_t e = tid; e < E * kSumReps; e += kThreads) lsum[e] = 0ull;
    for (uint32_t e = tid; e < E; e += kThreads) {
      lerr[e] = 0u;
      lmm[2u * e] = 0xFFFFFFFFu;
      lmm[2u * e + 1u] = 0u;
    }
  }
  if constexpr (ST == kStWide) {
    auto* ent = reinterpret_cast<uint32_t*>(smem + kOffSum);
    auto* lerr = reinterpret_cast<uint32_t*>(smem + kOffWideErr);
    for (uint32_t e = tid; e < E; e += kThreads) {
      ent[4u * e] = 0u;
      ent[4u * e + 1u] = 0u;
      ent[4u * e + 2u] = 0xFFFFFFFFu;
      ent[4u * e + 3u] = 0u;
      lerr[e] = 0u;
    }
  }
  if constexpr (ST == kStSlot) {
    auto* lsum = reinterpret_cast<unsigned long long*>(smem + kOffSum);
    auto* st4 = reinterpret_cast<uint32_t*>(smem + kOffMm);
    for (uint32_t e = tid; e < kSlotEdges * kSlotSumReps; e += kThreads) lsum[e] = 0ull;
    for (uint32_t e = tid; e < kSlotEdges; e += kThreads) {
      st4[4u * e] = 0u;
      st4[4u * e + 1u] = 0xFFFFFFFFu;
      st4[4u * e + 2u] = 0u;
      st4[4u * e + 3u] = 0u;
    }
  }
}

template <int HT, int ST>
__device__ __forceinline__ void tables_flush(unsigned char* smem, uint32_t E, const Table& tab,
                                             int tid) {
  if constexpr (HT == kHtPair) {
    auto* hk = reinterpret_cast<uint32_t*>(smem + kOffHt);
    auto* hc = reinterpret_cast<uint32_t*>(smem + kOffHc);
    for (uint32_t s = tid; s < kPairSlots; s += kThreads) {
      const uint32_t cnt = hc[s];
      if (cnt) atomicAdd(&tab.hist[hk[s] - 1u], (unsigned long long)cnt);
    }
    if (tid == 0) {
      const uint32_t fails = reinterpret_cast<const uint32_t*>(smem + kOffCtl)[0];
      if (fails) atomicAdd(&tab.ovf[0], (unsigned long long)fails);
      if (tab.mode == kModeAuto && fails >= kSatFails) atomicAdd(&tab.ovf[1], 1ull);
    }
  }
  if constexpr (HT == kHtCompact) {
    auto* hk = reinterpret_cast<uint32_t*>(smem + kOffHt);
    const uint32_t kmask = 0xFFFFFFFFu >> (32u - tab.kb);
    uint32_t used = 0;
    for (uint32_t s = tid; s < kCmpSlots; s += kThreads) {
      const uint32_t w = hk[s];
      used += w ? 1u : 0u;
      if (w >> tab.kb) atomicAdd(&tab.hist[(w & kmask) - 1u], (unsigned long long)(w >> tab.kb));
    }
    if (tab.occupancy) {  // the workgroup's used slots -> tab.ovf[1] (max over workgroups)
      auto* ctl = reinterpret_cast<uint32_t*>(smem + kOffCtl);
      for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o);
      if ((tid & (kWave - 1)) == 0) atomicAdd(&ctl[1], used);
      __syncthreads();
      if (tid == 0) atomicMax(&tab.ovf[1], (unsigned long long)ctl[1]);
    }
  }
  if constexpr (ST == kStSlot) {
    auto* lsum = reinterpret_cast<unsigned long long*>(smem + kOffSum);
    auto* st4 = reinterpret_cast<uint32_t*>(smem + kOffMm);
    for (uint32_t s = tid; s < kSlotEdges; s += kThreads) {
      const uint32_t key = st4[4u * s];
      if (key) {
        const uint32_t e = key - 1u;
        unsigned long long sum = 0;
        for (uint32_t k = 0; k < kSlotSumReps; ++k) sum += lsum[s * kSlotSumReps + k];
        atomicAdd(&tab.sum[e], sum);
        if (st4[4u * s + 3u]) atomicAdd(&tab.err[e], (unsigned long long)st4[4u * s + 3u]);
        atomicMin(&tab.mn[e], st4[4u * s + 1u]);
        atomicMax(&tab.mx[e], st4[4u * s + 2u]);
      }
    }
  }
  if constexpr (ST == kStWide) {
    auto* ent = reinterpret_cast<uint32_t*>(smem + kOffSum);
    auto* lerr = reinterpret_cast<uint32_t*>(smem + kOffWideErr);
    for (uint32_t e = tid; e < E; e += kThreads) {
      const uint32_t mn = ent[4u * e + 2u], mx = ent[4u * e + 3u];
      if (mn != 0xFFFFFFFFu || mx != 0u) {
        atomicAdd(&tab.sum[e], *reinterpret_cast<const unsigned long long*>(ent + 4u * e));
        if (lerr[e]) atomicAdd(&tab.err[e], (unsigned long long)lerr[e]);
        atomicMin(&tab.mn[e], mn);
        atomicMax(&tab.mx[e], mx);
      }
    }
  }
  if constexpr (ST == kStDirect) {
    auto* lsum = reinterpret_cast<unsigned long long*>(smem + kOffSum);
    auto* lerr = reinterpret_cast<uint32_t*>(smem + kOffErr);
    auto* lmm = reinterpret_cast<uint32_t*>(smem + kOffMm);
    for (uint32_t e = tid; e < E; e += kThreads) {
      if (lmm[2u * e] != 0xFFFFFFFFu || lmm[2u * e + 1u] != 0u) {
        unsigned long long sum = 0;
        for (uint32_t k = 0; k < kSumReps; ++k) sum += lsum[e * kSumReps + k];
        atomicAdd(&tab.sum[e], sum);
        if (lerr[e]) atomicAdd(&tab.err[e], (unsigned long long)lerr[e]);
        atomicMin(&tab.mn[e], lmm[2u * e]);
        atomicMax(&tab.mx[e], lmm[2u * e + 1u]);
      }
    }
  }
}

// ---- long-trace pass: resolve, then record ---------------------------------
// Traces longer than kBigMin (<= kStage) do not go through a wave's staging
// area: the chunk walk only lists them (big_list[j] = trace index, big[0] =
// count), and two kernels handle them afterwards.
//
// edge_big_resolve_kernel holds a hash table of kResWin span ids at a time
// (id -> first position in the window, atomicMin, with that span's service)
// and nothing else (48 KiB: three 512-thread workgroups per CU).  A trace
// longer than a window is looked up kBigPer spans per thread against its
// windows in trace order, so the first window holding a span's parent
// reference gives the first match (the reference rule): O(L * ceil(L /
// kResWin)) work, O(L) for L <= kResWin.  Shorter traces are packed, up to
// kGroup of them, into ONE window: trace i owns table slots [2 off_i, 2 off_i
// + 2 L_i) (load 1/2; range reduction by multiply-shift, linear probing inside
// the region), so ids of different traces never meet, and a workgroup pays the
// load / insert / lookup round trips once per batch instead of once per
// trace.  It writes every listed span's parent row — or, in the exact-quantile
// mode, its key.
//
// edge_big_record_kernel streams the listed spans (16 traces per ticket, one
// load round trip per ticket) into the same private histogram / per-edge
// stats tables as the chunk walk, flushed once at the end.  Same first-match
// rule, same table forms.
//
// Why two kernels: with the histogram / stats tables AND the id table in one
// workgroup's LDS a CU runs one workgroup, and every batch's column loads,
// inserts, lookups and records follow each other with nothing to hide their
// latency (LONG at 2^23 traces: 3.74 ms for 1.3e8 listed spans).
constexpr int kBigThreads = kThreads;  // record kernel: the tables' init / flush loops assume it
// traces longer than this take the long-trace pass (<= kStage)
constexpr uint32_t kBigMin = 256;
constexpr int kBigPer = 8;  // spans per thread per lookup block
constexpr int kGroup = 4;   // traces per ticket (one atomic, their entries and bounds loaded together)
constexpr int kResThreads = 512;
// minimum waves per SIMD the compiler must fit the resolve kernel in (registers)
constexpr int kResMinWaves = 2;
constexpr uint32_t kResWin = 2048;                 // ids per table window
constexpr uint32_t kResSlots = 2 * kResWin;        // load <= 1/2
static_assert((kResSlots & (kResSlots - 1)) == 0, "power-of-two table");
__device__ __forceinline__ uint32_t res_slot(uint64_t id) {
  return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32) & (kResSlots - 1u);
}
constexpr int kResPer = (int)kResWin / kResThreads;  // spans per thread in a packed window
static_assert(kResWin % kResThreads == 0 && kResWin <= 65536, "window: whole rows, pos << 16 | svc");

// A packed trace's slot inside its own table region of `size` slots.
__device__ __forceinline__ uint32_t big_region_slot(uint64_t id, uint32_t size) {
  return __umulhi((uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32), size);
}

__device__ __forceinline__ void res_out(const Table& tab, uint64_t g, uint32_t p, uint32_t sf,
                                        uint32_t dr, uint32_t S) {
  if (tab.keys)
    tab.keys[g] = ((unsigned long long)(p * S + (sf & 0xFFFFu)) << 32) | dr;
  else
    tab.bpar[g] = (uint16_t)p;
}

// One trace longer than a window: blocks of kResThreads * kBigPer spans,
// each looked up against the trace's id windows in order.
__device__ void res_one(unsigned long long* bkey, uint32_t* bval,
                        const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
                        const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
                        uint64_t lo, uint64_t L, uint32_t S, const Table& tab) {
  const int tid = threadIdx.x;
  for (uint64_t b0 = 0; b0 < L; b0 += (uint64_t)kResThreads * kBigPer) {
    uint64_t pid[kBigPer];
    uint32_t psv[kBigPer];  // ~0: not found yet
    bool need = false;
#pragma unroll
    for (int r = 0; r < kBigPer; ++r) {
      const uint64_t i = b0 + (uint64_t)r * kResThreads + tid;
      pid[r] = i < L ? parent[lo + i] : 0ull;
      psv[r] = 0xFFFFFFFFu;
      need |= pid[r] != 0ull;
    }
    for (uint64_t w0 = 0; w0 < L; w0 += kResWin) {
      if (!__syncthreads_or(need)) break;  // also orders the previous clear
#pragma unroll
      for (int u = 0; u < kResPer; ++u) {
        const uint32_t k = (uint32_t)(u * kResThreads + tid);
        const uint64_t id = w0 + k < L ? span_id[lo + w0 + k] : 0ull;
        if (id == 0ull) continue;
        const uint32_t sv = svcfl[lo + w0 + k] & 0xFFFFu;
        for (uint32_t sl = res_slot(id);; sl = (sl + 1u) & (kResSlots - 1u)) {
          const unsigned long long prev = atomicCAS(&bkey[sl], 0ull, (unsigned long long)id);
          if (prev == 0ull || prev == id) {
            atomicMin(&bval[sl], (k << 16) | sv);  // the first position wins, with its service
            break;
          }
        }
      }
      __syncthreads();
      need = false;
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        if (pid[r] == 0ull || psv[r] != 0xFFFFFFFFu) continue;
        for (uint32_t sl = res_slot(pid[r]);; sl = (sl + 1u) & (kResSlots - 1u)) {
          const unsigned long long key = bkey[sl];
          if (key == pid[r]) {
            psv[r] = bval[sl] & 0xFFFFu;
            break;
          }
          if (key == 0ull) break;
        }
        need |= psv[r] == 0xFFFFFFFFu;
      }
      __syncthreads();
      for (uint32_t k = tid; k < kResSlots; k += kResThreads) {
        bkey[k] = 0ull;
        bval[k] = 0xFFFFFFFFu;
      }
    }
#pragma unroll
    for (int r = 0; r < kBigPer; ++r) {
      const uint64_t i = b0 + (uint64_t)r * kResThreads + tid;
      if (i >= L) continue;
      const uint32_t p = pid[r] == 0ull ? S : psv[r] == 0xFFFFFFFFu ? S + 1u : psv[r];
      res_out(tab, lo + i, p, tab.keys ? svcfl[lo + i] : 0u, tab.keys ? dur[lo + i] : 0u, S);
    }
  }
  __syncthreads();  // the last window's clear before the next user of the table
}

// Up to kGroup traces (bm: the group entries packed into this window,
// consecutive) in one window, each in a private table region [2 off_i,
// 2 off_i + 2 L_i).
__device__ void res_batch(unsigned long long* bkey, uint32_t* bval,
                          const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
                          const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
                          const uint64_t (&lo)[kGroup], const uint64_t (&L)[kGroup], uint32_t bm,
                          uint32_t S, const Table& tab) {
  const int tid = threadIdx.x;
  uint32_t off[kGroup + 1];
  off[0] = 0;
#pragma unroll
  for (int i = 0; i < kGroup; ++i) off[i + 1] = off[i] + (((bm >> i) & 1u) ? (uint32_t)L[i] : 0u);
  const uint32_t tot = off[kGroup];
  uint64_t id[kResPer], pid[kResPer], g[kResPer];
  uint32_t sv[kResPer], rb[kResPer], rs[kResPer], pos[kResPer];
  bool v[kResPer];
#pragma unroll
  for (int u = 0; u < kResPer; ++u) {
    const uint32_t q = (uint32_t)(u * kResThreads + tid);
    v[u] = q < tot;
    uint32_t a0 = 0, a1 = off[1];
    uint64_t tl = lo[0];
#pragma unroll
    for (int i = 1; i < kGroup; ++i)
      if (q >= off[i] && ((bm >> i) & 1u)) {
        a0 = off[i];
        a1 = off[i + 1];
        tl = lo[i];
      }
    pos[u] = q - a0;
    rb[u] = 2u * a0;
    rs[u] = 2u * (a1 - a0);
    g[u] = tl + pos[u];
    id[u] = v[u] ? span_id[g[u]] : 0ull;
    pid[u] = v[u] ? parent[g[u]] : 0ull;
    sv[u] = v[u] ? svcfl[g[u]] & 0xFFFFu : 0u;
  }
#pragma unroll
  for (int u = 0; u < kResPer; ++u) {
    if (!v[u] || id[u] == 0ull) continue;
    uint32_t r = big_region_slot(id[u], rs[u]);
    while (true) {
      const uint32_t sl = rb[u] + r;
      const unsigned long long prev = atomicCAS(&bkey[sl], 0ull, (unsigned long long)id[u]);
      if (prev == 0ull || prev == id[u]) {
        atomicMin(&bval[sl], (pos[u] << 16) | sv[u]);  // the first position wins
        break;
      }
      r = r + 1u == rs[u] ? 0u : r + 1u;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kResPer; ++u) {
    if (!v[u]) continue;
    uint32_t psv = 0xFFFFFFFFu;
    if (pid[u] != 0ull) {
      uint32_t r = big_region_slot(pid[u], rs[u]);
      for (uint32_t probe = 0; probe < rs[u]; ++probe) {
        const unsigned long long key = bkey[rb[u] + r];
        if (key == pid[u]) {
          psv = bval[rb[u] + r] & 0xFFFFu;
          break;
        }
        if (key == 0ull) break;
        r = r + 1u == rs[u] ? 0u : r + 1u;
      }
    }
    const uint32_t p = pid[u] == 0ull ? S : psv == 0xFFFFFFFFu ? S + 1u : psv;
    res_out(tab, g[u], p, tab.keys ? svcfl[g[u]] : 0u, tab.keys ? dur[g[u]] : 0u, S);
  }
  __syncthreads();  // every lookup done before the clear
  for (uint32_t k = tid; k < 2u * tot; k += kResThreads) {
    bkey[k] = 0ull;
    bval[k] = 0xFFFFFFFFu;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kResThreads, kResMinWaves) void edge_big_resolve_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ trace_ptr, uint32_t S, Table tab) {
  __shared__ unsigned long long bkey[kResSlots];  // 0 = empty (id 0 is never a parent ref)
  __shared__ uint32_t bval[kResSlots];            // (first position) << 16 | svc
  __shared__ unsigned long long s_g[kGroup][2];
  const int tid = threadIdx.x;
  const uint64_t nbig = tab.big[0];
  if (nbig == 0) return;
  for (uint32_t k = tid; k < kResSlots; k += kResThreads) {
    bkey[k] = 0ull;
    bval[k] = 0xFFFFFFFFu;
  }
  unsigned long long nlo = 0, nL = 0;
  auto fetch = [&]() {
    unsigned long long j = 0;
    if (tid == 0) j = atomicAdd(&tab.big[1], (unsigned long long)kGroup);
    j = __shfl(j, 0);
    nlo = nL = 0;
    if (tid < kGroup && j + tid < nbig) {
      const uint64_t t = tab.big_list[j + tid];
      nlo = trace_ptr[t];
      nL = trace_ptr[t + 1] - nlo;
    }
  };
  if (tid < kWave) fetch();
  while (true) {
    __syncthreads();
    if (tid < kGroup) {
      s_g[tid][0] = nlo;
      s_g[tid][1] = nL;
    }
    __syncthreads();
    uint64_t glo[kGroup], gL[kGroup];
    bool any = false;
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      glo[k] = s_g[k][0];
      gL[k] = s_g[k][1];
      any |= gL[k] != 0;
    }
    if (!any) break;
    if (tid < kWave) fetch();
    uint32_t left = 0;
#pragma unroll
    for (int q = 0; q < kGroup; ++q) left |= (gL[q] != 0 ? 1u : 0u) << q;
    while (left) {
      const int k = __ffs(left) - 1;
      uint64_t lk = 0, Lk = 0;
#pragma unroll
      for (int q = 0; q < kGroup; ++q)
        if (q == k) {
          lk = glo[q];
          Lk = gL[q];
        }
      if (Lk > kResWin) {
        res_one(bkey, bval, span_id, parent, svcfl, dur, lk, Lk, S, tab);
        left &= ~(1u << k);
        continue;
      }
      uint32_t bm = 0;
      uint64_t tot = 0;
#pragma unroll
      for (int q = 0; q < kGroup; ++q) {
        const bool chain = q == k || (q > 0 && ((bm >> (q - 1)) & 1u));
        if (q >= k && chain && ((left >> q) & 1u) && gL[q] <= kResWin && tot + gL[q] <= kResWin) {
          bm |= 1u << q;
          tot += gL[q];
        }
      }
      res_batch(bkey, bval, span_id, parent, svcfl, dur, glo, gL, bm, S, tab);
      left &= ~bm;
    }
  }
}

// The listed spans into the tables, kRecGroup traces per ticket (wave 0 keeps
// the next ticket's entries and bounds in flight).
constexpr int kRecGroup = 16;
constexpr int kRecPer = 4;  // listed spans per thread loaded together
template <int HT, int ST>
__global__ __launch_bounds__(kBigThreads) void edge_big_record_kernel(
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ trace_ptr, uint32_t S, uint32_t E, Table tab) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kOffWave];
  __shared__ unsigned long long s_lo[kRecGroup];
  __shared__ uint32_t s_off[kRecGroup + 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const uint64_t nbig = tab.big[0];
  if (nbig == 0) return;
  tables_init<HT, ST>(smem, E, tid);
  unsigned long long nlo = 0;
  uint32_t nL = 0;
  auto fetch = [&]() {
    unsigned long long j = 0;
    if (lane == 0) j = atomicAdd(&tab.big[2], (unsigned long long)kRecGroup);
    j = __shfl(j, 0);
    nlo = 0;
    nL = 0;
    if (lane < kRecGroup && j + lane < nbig) {
      const uint64_t t = tab.big_list[j + lane];
      nlo = trace_ptr[t];
      nL = (uint32_t)(trace_ptr[t + 1] - nlo);
    }
  };
  if (tid < kWave) fetch();
  while (true) {
    __syncthreads();  // the previous ticket is done with s_lo / s_off
    if (tid < kWave) {
      uint32_t inc = nL;  // inclusive scan over the ticket's traces
#pragma unroll
      for (int o = 1; o < kRecGroup; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
      }
      if (lane < kRecGroup) {
        s_lo[lane] = nlo;
        s_off[lane + 1] = inc;
      }
      if (lane == 0) s_off[0] = 0;
      fetch();  // the next ticket, overlapping this one's work
    }
    __syncthreads();
    const uint32_t tot = s_off[kRecGroup];
    if (tot == 0) break;  // tickets exhausted (listed traces are never empty)
    // the ticket's trace offsets in scalar registers (uniform; read once, not
    // per span)
    uint32_t off[kRecGroup];
#pragma unroll
    for (int i = 0; i < kRecGroup; ++i) off[i] = __builtin_amdgcn_readfirstlane(s_off[i]);
    // kRecPer spans per thread loaded together, then recorded (the records'
    // LDS / HBM atomics would otherwise keep the next loads behind them)
    for (uint32_t q0 = tid; q0 < tot; q0 += kRecPer * kBigThreads) {
      uint32_t sf[kRecPer], dr[kRecPer], pr[kRecPer];
#pragma unroll
      for (int j = 0; j < kRecPer; ++j) {
        const uint32_t q = q0 + (uint32_t)j * kBigThreads;
        int t = 0;
        uint32_t base = 0;
#pragma unroll
        for (int i = 1; i < kRecGroup; ++i) {
          const bool in = q >= off[i];
          t = in ? i : t;
          base = in ? off[i] : base;
        }
        const uint64_t g = s_lo[t] + (q - base);
        const bool v = q < tot;
        sf[j] = v ? svcfl[g] : 0u;
        dr[j] = v ? dur[g] : 0u;
        pr[j] = v ? tab.bpar[g] : 0xFFFFu;
      }
#pragma unroll
      for (int j = 0; j < kRecPer; ++j)
        if (pr[j] != 0xFFFFu) record<HT, ST>(smem, pr[j] * S + (sf[j] & 0xFFFFu), dr[j], sf[j] >> 16, tab);
    }
  }
  __syncthreads();
  tables_flush<HT, ST>(smem, E, tab, tid);
}

template <int HT, int ST, bool UNI, int MODE = kModeNormal, bool ROWS = false>
__global__ __launch_bounds__(kThreads) void edge_agg_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint64_t* __restrict__ trace_ptr, uint64_t n_traces, uint32_t S, uint32_t E, Table tab) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kLdsBytes];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = tid / kWave;
  const Cols col{span_id, parent, svcfl, dur};
  // Static share: the first n_static traces split evenly over the waves; the
  // last 1 / kDyn of the traces are handed out in segments of kDynSeg from a
  // global counter, so waves that finish early take the tail.
  constexpr uint64_t kDyn = 4, kDynSeg = 512;
  const uint64_t n_static = n_traces - n_traces / kDyn;
  // Resume launch (compact form) after a kModeAuto launch: the trace ranges
  // its stopped waves left, then the rest of the dynamic tail.  Nothing left
  // (no workgroup saturated): return before touching LDS.
  constexpr bool resume = MODE == kModeResume;
  const uint64_t n_left = resume ? tab.nleft[0] : 0;
  if (resume && n_left == 0 && n_static + *tab.ctr >= n_traces) return;

  tables_init<HT, ST>(smem, E, tid);
  __syncthreads();

  unsigned char* wsm = smem + kOffWave + wid * kWBytes;
  const uint64_t gw = (uint64_t)blockIdx.x * kWavesPerWG + wid;
  const uint64_t nw = (uint64_t)gridDim.x * kWavesPerWG;
  uint64_t t_begin = uniform64(n_static * gw / nw);
  uint64_t t_end = uniform64(n_static * (gw + 1) / nw);
  bool from_left = resume;
  auto next_left = [&]() {  // the next range a stopped wave left (false: none)
    unsigned long long j = 0;
    if (lane == 0) j = atomicAdd(&tab.nleft[1], 1ull);
    j = uniform64(__shfl(j, 0));
    if (j >= n_left) return false;
    t_begin = uniform64(tab.left[2 * j]);
    t_end = uniform64(tab.left[2 * j + 1]);
    return true;
  };
  if (resume && !next_left()) {
    from_left = false;
    t_begin = t_end = 0;
  }
  bool stopped = false;
  uint32_t* ctl = reinterpret_cast<uint32_t*>(smem + kOffCtl);

  while (true) {
  if (t_begin < t_end) {
    // Pipeline: the bounds of chunk c+2 and the span columns of chunk c+1 are
    // in flight while chunk c is resolved and recorded.
    uint64_t lo, hi;
    load_bounds(trace_ptr, t_begin, t_end, lane, lo, hi);
    Chunk cur = make_chunk(t_begin, t_end, lane, lo, hi, kBigMin);
    Regs R;
    load_regs(col, cur, lane, R);
    // kModeAuto: the first trace of the current chunk lives in the wave's LDS
    // word, not a register (a register more spilled the auto form's loop: 16 /
    // 48 B per lane, 12 % / 40 % slower than the pair form on SN / shuffled SN)
    uint64_t* wt_cur = reinterpret_cast<uint64_t*>(wsm + kWAuto);
    if (MODE == kModeAuto && lane == 0) *wt_cur = t_begin;
    uint64_t t_cur = t_begin;  // (other modes: a register)
    uint64_t t_next = t_begin + (cur.k ? cur.k : 1u);
    load_bounds(trace_ptr, t_next, t_end, lane, lo, hi);
    while (true) {
      // A first aggregation (kModeAuto) whose pair table saturated: leave
      // [first trace of the chunk, t_end) to the compact-form resume launch
      // and stop.
      if (MODE == kModeAuto &&
          (uint32_t)__builtin_amdgcn_readfirstlane(
              __hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >=
              kSatFails) {
        if (lane == 0) {
          const unsigned long long j = atomicAdd(&tab.nleft[0], 1ull);
          tab.left[2 * j] = *wt_cur;
          tab.left[2 * j + 1] = t_end;
        }
        stopped = true;
        break;
      }
      const bool has_next = t_next < t_end;
      const uint64_t t_nxt = t_next;
      if (MODE == kModeAuto && lane == 0 && has_next) wt_cur[1] = t_next;  // the next chunk's
      Chunk nxt{};
      Regs Rn;
      if (has_next) {
        nxt = make_chunk(t_next, t_end, lane, lo, hi, kBigMin);
        load_regs(col, nxt, lane, Rn);
        t_next += nxt.k ? nxt.k : 1u;
        load_bounds(trace_ptr, t_next, t_end, lane, lo, hi);
      }
      if (cur.k == 0) {  // a trace longer than kBigMin: listed for the long-trace pass
        if (lane == 0)
          tab.big_list[atomicAdd(&tab.big[0], 1ull)] =
              tab.t_base + (MODE == kModeAuto ? *wt_cur : t_cur);
      } else {
        process_chunk<HT, ST, UNI, MODE == kModeWideScan, ROWS>(smem, wsm, lane, cur, R, S, tab);
      }
      if (!has_next) break;
      cur = nxt;
      if (MODE == kModeAuto) {
        if (lane == 0) wt_cur[0] = wt_cur[1];
      } else {
        t_cur = t_nxt;
      }
      R = Rn;
    }
  }
  if (stopped) break;
  if (from_left) {
    if (next_left()) continue;
    from_left = false;
  }
  if (n_static == n_traces) break;
  unsigned long long g = 0;
  if (lane == 0) g = atomicAdd(tab.ctr, (unsigned long long)kDynSeg);
  g = __shfl(g, 0);
  t_begin = uniform64(n_static + g);
  if (t_begin >= n_traces) break;
  t_end = uniform64(t_begin + kDynSeg < n_traces ? t_begin + kDynSeg : n_traces);
  }
  __syncthreads();

  tables_flush<HT, ST>(smem, E, tab, tid);
}

// Edge records (the fused ungrouped aggregation, bucket.hip): one 8-B record
// per span — (parent row * S + service) << 33 | error << 32 | duration — into
// the chunk walk's LDS table forms.  A plain stream: 8 records per thread
// loaded together, then recorded; a record of all ones (the padding past n,
// and a caller's "no span here": common.h) is skipped.  The compact form also
// reports its largest workgroup occupancy (tab.ovf[1], atomic max), so a set
// learns whether the pair table would hold it.
constexpr int kRecLoad = 8;
template <int HT, int ST>
__global__ __launch_bounds__(kThreads) void edge_rec_kernel(const uint64_t* __restrict__ rec,
                                                            uint64_t n, uint32_t E, Table tab) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kOffWave];
  const int tid = threadIdx.x;
  tables_init<HT, ST>(smem, E, tid);
  __syncthreads();
  constexpr uint64_t kPerBlock = (uint64_t)kThreads * kRecLoad;
  for (uint64_t b0 = (uint64_t)blockIdx.x * kPerBlock; b0 < n; b0 += (uint64_t)gridDim.x * kPerBlock) {
    uint64_t x[kRecLoad];
#pragma unroll
    for (int j = 0; j < kRecLoad; ++j) {
      const uint64_t i = b0 + (uint64_t)(j * kThreads + tid);
      x[j] = i < n ? rec[i] : ~0ull;
    }
#pragma unroll
    for (int j = 0; j < kRecLoad; ++j)
      if (x[j] != ~0ull)
        record<HT, ST>(smem, (uint32_t)(x[j] >> 33), (uint32_t)x[j],
                       ((x[j] >> 32) & 1ull) ? ANOMOD_FLAG_ERROR : 0u, tab);
  }
  __syncthreads();
  tables_flush<HT, ST>(smem, E, tab, tid);  // (the caller sets tab.occupancy)
}

// A set whose parent rows are known (anomod_spans::parent_row): spans [lo, hi)
// of svc_flags, dur_us and the row column as a plain stream, 10 B/span, into
// the same table forms — no ids, no trace bounds, no scan.  A thread takes 4
// consecutive spans per load group (16 B + 16 B + 8 B), kRowLoad groups per
// round; the next round's loads are issued before this round's records.  The
// up to 3 spans before the first and after the last 4-aligned position are
// read one by one by the first workgroup (the columns are 256-B aligned, so
// alignment is that of the span position).  S0: the service count the rows
// were written with (rows S0 / S0 + 1 are root / orphan: this call's S / S +
// 1); a row of all ones is no span.  kHtKeys writes the exact-quantile keys
// (edge << 32 | dur by span position) instead of recording.
constexpr int kRowLoad = 2;
struct RowRegs {
  u32x4 sf[kRowLoad], dr[kRowLoad];
  u32x2 rw[kRowLoad];
};
template <int HT, int ST>
__global__ __launch_bounds__(kThreads) void edge_row_kernel(
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint16_t* __restrict__ rows, uint64_t lo, uint64_t hi, uint32_t S, uint32_t S0,
    uint32_t E, Table tab) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[HT == kHtKeys ? 16 : kOffWave];
  const int tid = threadIdx.x;
  if constexpr (HT != kHtKeys) {
    tables_init<HT, ST>(smem, E, tid);
    __syncthreads();
  }
  auto one = [&](uint64_t g, uint32_t sf, uint32_t d, uint32_t row) {
    if (row == 0xFFFFu) return;
    const uint32_t p = row >= S0 ? row - S0 + S : row;
    const uint32_t edge = p * S + (sf & 0xFFFFu);
    if constexpr (HT == kHtKeys)
      tab.keys[g] = ((unsigned long long)edge << 32) | d;
    else
      record<HT, ST>(smem, edge, d, sf >> 16, tab);
  };
  const uint64_t up = (lo + 3ull) & ~3ull;
  const uint64_t a0 = up < hi ? up : hi;                   // head [lo, a0)
  const uint64_t a1 = (hi & ~3ull) > a0 ? (hi & ~3ull) : a0;  // groups [a0, a1), tail [a1, hi)
  if (blockIdx.x == 0 && tid < 8) {
    const uint64_t g = tid < 4 ? lo + (uint64_t)tid : a1 + (uint64_t)(tid - 4);
    if (g < (tid < 4 ? a0 : hi)) one(g, svcfl[g], dur[g], rows[g]);
  }
  const uint64_t ng = (a1 - a0) / 4;
  const u32x4* sf4 = reinterpret_cast<const u32x4*>(svcfl + a0);
  const u32x4* dr4 = reinterpret_cast<const u32x4*>(dur + a0);
  const u32x2* rw2 = reinterpret_cast<const u32x2*>(rows + a0);
  // groups past the end re-read the last one (no branch around a load) and
  // take skip rows
  auto load = [&](uint64_t g0, RowRegs& R) {
#pragma unroll
    for (int j = 0; j < kRowLoad; ++j) {
      const uint64_t gi = g0 + (uint64_t)(j * kThreads + tid);
      const uint64_t gc = gi < ng ? gi : ng - 1;
      R.sf[j] = sf4[gc];
      R.dr[j] = dr4[gc];
      const u32x2 w = rw2[gc];
      R.rw[j] = gi < ng ? w : u32x2{0xFFFFFFFFu, 0xFFFFFFFFu};
    }
  };
  constexpr uint64_t kPerBlock = (uint64_t)kThreads * kRowLoad;
  uint64_t g0 = (uint64_t)blockIdx.x * kPerBlock;
  RowRegs cur;
  if (g0 < ng) load(g0, cur);
  while (g0 < ng) {
    const uint64_t gn = g0 + (uint64_t)gridDim.x * kPerBlock;
    RowRegs nxt = cur;
    if (gn < ng) load(gn, nxt);
#pragma unroll
    for (int j = 0; j < kRowLoad; ++j) {
      const uint64_t g = a0 + 4ull * (g0 + (uint64_t)(j * kThreads + tid));
      one(g, cur.sf[j].x, cur.dr[j].x, cur.rw[j].x & 0xFFFFu);
      one(g + 1, cur.sf[j].y, cur.dr[j].y, cur.rw[j].x >> 16);
      one(g + 2, cur.sf[j].z, cur.dr[j].z, cur.rw[j].y & 0xFFFFu);
      one(g + 3, cur.sf[j].w, cur.dr[j].w, cur.rw[j].y >> 16);
    }
    cur = nxt;
    g0 = gn;
  }
  if constexpr (HT != kHtKeys) {
    __syncthreads();
    tables_flush<HT, ST>(smem, E, tab, tid);  // (the caller sets tab.occupancy)
  }
}

// ---- dense stream: span words into a directly indexed histogram ------------
// A resident set touches a sliver of the E x kBins key space, and its own
// first table says which: every edge with spans gets a code (its rank among
// those edges) and the bin range [hist_bin(min), hist_bin(max)] of a cell
// array (DenseSet, common.h).  Once the set's u32 span-word column is written
// (edge_encode_kernel: code, error bit and duration by span position,
// span_word_pack in span_word.h; kWordSkip = no span) an aggregation reads that
// column alone, 4 B/span, and a span costs one 16-B LDS read of its code's
// entry {min, max, base - first_bin, first_bin | width << 16} — few
// distinct addresses, mostly a broadcast —, one ds_add_u32 on its cell, one
// returning ds_add_u32 on a sum replica (u32, by lane; a wrap is a carry
// counted per code: 64-bit LDS adds cost several times a 32-bit one) and one
// branch around the rare updates (carry, new extreme, error): no hash, no
// compare chain, no out-of-line insert.  The kernel is bound by instruction
// issue, not by LDS or HBM, so what is counted here are instructions per
// span.  A duration that does not fit its field (the escape value) is read
// from dur_us by that lane alone.  Correctness never rests on the learned
// ranges: a span whose bin lies outside its code's range (one unsigned
// compare) counts in tab.hist in HBM.  Two static LDS carves: small (<= 64
// codes, <= 8 Ki cells, 32 sum replicas: the SocialNetwork sets) and large
// (<= 512 codes, <= 32 Ki cells, 8 sum replicas, under 160 KiB).  A packed
// layout of the small carve whose cells fit twice takes a third, the small
// carve with 16 Ki entries (error cells, FMT 3 below).
constexpr uint32_t kDenseMaxEdges = 1u << 16;  // edge -> code table: at most 128 KiB
template <int TIER>
struct DenseCfg;
template <>
struct DenseCfg<0> {
  static constexpr uint32_t kCodes = 64, kCells = 8192, kReps = 32;
  static constexpr int kLoad = 4;  // load groups (4 spans each) per thread and round
};
template <>
struct DenseCfg<1> {
  static constexpr uint32_t kCodes = 512, kCells = 32768, kReps = 8;
  static constexpr int kLoad = 8;
};
// The small carve with error cells (FMT 3): kCells counts entries, two per cell.
template <>
struct DenseCfg<2> {
  static constexpr uint32_t kCodes = 64, kCells = 16384, kReps = 32;
  static constexpr int kLoad = 4;
};
static_assert(DenseCfg<1>::kCodes <= kWordNoCode, "the code field holds every code and the skip value");
static_assert(DenseCfg<0>::kCodes <= DenseCfg<1>::kCodes, "one word format for both tiers");
template <int TIER>
struct DenseLds {
  using C = DenseCfg<TIER>;
  static constexpr int kOffEnt = 0;                                       // u32x4 [kCodes]
  static constexpr int kOffCell = kOffEnt + (int)C::kCodes * 16;          // u32 [kCells]
  static constexpr int kOffSum = kOffCell + (int)C::kCells * 4;           // u32 [kCodes][kReps]
  static constexpr int kOffErr = kOffSum + (int)(C::kCodes * C::kReps) * 4;  // u32 [kCodes]
  static constexpr int kOffHi = kOffErr + (int)C::kCodes * 4;             // u32 [kCodes]: sum carries
  static constexpr int kBytes = kOffHi + (int)C::kCodes * 4;
  static_assert(kBytes <= 160 * 1024, "LDS budget");
  static_assert((C::kReps & (C::kReps - 1u)) == 0u && C::kReps <= (uint32_t)kWave, "replica by lane");
};
// A cell of the packed-word kernel (FMT 2), one u32: the owning code in the top
// byte (the word no longer carries it), a flag, and the count below.
constexpr uint32_t kPackCodeShift = 24, kPackFlag = 1u << 23, kPackCount = kPackFlag - 1u;
// hist_bin without its select: below 64 the exponent clamps to 0 and the bin
// is the value itself (the same bins; clz(0) = 32).
static_assert(ANOMOD_HIST_SUB_BITS == 5, "values below 2 << SUB_BITS are their own bins");
__device__ __forceinline__ uint32_t dense_bin(uint32_t v) {
  constexpr uint32_t kTop = 31u - ANOMOD_HIST_SUB_BITS;
  const uint32_t z = (uint32_t)__clz((int)v);
  const uint32_t e = kTop - (z < kTop ? z : kTop);
  return (e << ANOMOD_HIST_SUB_BITS) + (v >> e);
}
constexpr int kDenseSmallWgs = 2;  // workgroups per CU of the small carve
constexpr uint64_t kDenseMaxWgs = 1u << 16;  // (bounds the span cap arithmetic of a launch)
static_assert(kDenseSmallWgs * DenseLds<0>::kBytes <= 160 * 1024, "LDS budget");
static_assert(kDenseSmallWgs * DenseLds<2>::kBytes <= 160 * 1024, "LDS budget");
static_assert(DenseCfg<2>::kLoad == DenseCfg<0>::kLoad && DenseCfg<2>::kReps == DenseCfg<0>::kReps &&
                  DenseCfg<2>::kCodes == DenseCfg<0>::kCodes,
              "the launch bounds of the small carve hold for both of its forms");
// Plain row streams of a set between the call that learned its layout and the
// one that writes the word column.  The column is an investment — a pass of
// its own (10 B/span read, 3 or 4 written: about one row stream) and 3 or 4
// B/span of memory — that only a set which keeps being aggregated repays, so it is made
// at the set's fifth aggregation: the first four calls of every set run
// exactly the kernels they ran without the dense stream.
constexpr uint32_t kDenseAfterStreams = 3;

// The words a thread holds of one round: G load groups (PACK: of 8 span
// positions, the high halves in w and the low bytes in b).
template <int G, bool PACK>
struct DenseRegs {
  u32x4 w[G];
};
template <int G>
struct DenseRegs<G, true> {
  u32x4 w[G];
  u32x2 b[G];
};

// pack_join of half J & 1 of h and byte J & 3 of b in one byte permute: the
// selector's bytes pick b's byte, h's two bytes, and zero (v_perm_b32: 0 .. 3
// are the second operand's bytes, 4 .. 7 the first's, 12 is 0x00).
template <int J>
__device__ __forceinline__ uint32_t pack_pick(uint32_t h, uint32_t b) {
  constexpr uint32_t kSel = 0x0C000000u | (5u + 2u * (J & 1)) << 16 | (4u + 2u * (J & 1)) << 8 | (J & 3);
  return __builtin_amdgcn_perm(h, b, kSel);
}

// lay: 4 words per code {edge, first_bin, base, width} (DenseSet::host).
// (the small carve is held to 64 registers: two workgroups per CU)
//
// FMT 0, duration words: the per-span work described above.  FMT 1, cell
// words (span_word.h): bin, range check and cell index were resolved when the
// column was written, so a span costs one compare on its cell field (skip and
// escape are the two values no cell has), a ds_add_u32 on that cell, a
// non-returning ds_add_u32 of its residual on a sum replica, one 8-B read of
// its code's {min key, max key} and one branch around the rare updates (the
// error bit sits above the key: an error span compares above every max key).
// The sum needs no carry: a code's sum is sum(count[cell] * lo(bin(cell))),
// formed in u64 by the wave that flushes the code's cells, plus the residual
// replicas, which the host keeps below 2^32 by the spans it gives a launch
// (dense_sum_rounds).  An escaping lane reads dur_us and adds to the HBM
// tables directly; under the encoder's rule it is never inside its code's
// range (a bin in range has an exponent <= res_bits and a cell below the
// reserved values), so it never owns an LDS cell.
//
// FMT 2, packed words (span_word.h): the cell word in 24 bits, read as groups
// of 8 span positions from two planes — one 16-B load of the high halves (word
// as u16) and one 8-B load of the low bytes (wlo) — and taken apart through
// pack_fmt of the layout (fmt here).  The word has no code: a cell's u32 holds
// the owning code above its count, filled from lay.  An escape word carries
// its code in the residual field and goes to `direct`, which reads dur_us: a
// span outside its code's range counts in HBM as before; a wide span (in
// range, bin exponent above the residual width) counts in its LDS cell, so the
// histogram and count * lo(bin) stay in the flush, and gives d - lo(bin), d
// and the error to the HBM tables.  The at most 7 + 7 span positions of a
// launch outside its groups of 8 take `direct` too, so a replica never sees
// them.
//
// FMT 3, packed words with error cells (small carve only, DenseCfg<2>): the
// same column, but the cell array has 16 Ki entries and a cell two of them —
// its own, and 2^cell_bits above it the one its error spans count in; the
// entry of a word is w >> res_bits (pack_word_entry).  FMT 2 takes its rare
// branch for every error span, which at 0.5 % errors is 27 % of a wave's
// spans (1 - 0.995^64); here the error count of a code is the sum of its
// error entries, formed by the wave that flushes the code's cells, lerr is
// not used, and the branch is taken on the entry's flag alone.  A span that
// finds its cell strictly inside its code's range clears the flag of both
// entries of the cell.  `direct` counts in the cell's own entry and sends its
// error to tab.err, as in FMT 2.  A layout takes this form when
// 2^cell_bits + cells <= 16 Ki (dense_learn; ANOMOD_DENSE_ERRCELLS=0 keeps
// FMT 2); 75,264 B of LDS, still two workgroups per CU.
template <int TIER, int FMT>
__global__ __launch_bounds__(kThreads, TIER == 0 ? 8 : 4) void edge_dense_kernel(
    const uint32_t* __restrict__ dur, const uint32_t* __restrict__ word,
    const u32x4* __restrict__ lay, uint32_t ncodes, uint32_t ncells, CellFmt fmt, uint64_t lo,
    uint64_t hi, Table tab, const unsigned char* __restrict__ wlo) {
  static_assert(FMT != 3 || TIER == 0, "error cells: the small carve only");
  constexpr bool kPacked = FMT >= 2, kErrCells = FMT == 3;
  constexpr int kCarve = kErrCells ? 2 : TIER;
  using C = DenseCfg<kCarve>;
  using O = DenseLds<kCarve>;
  constexpr int kDenseLoad = C::kLoad;
  constexpr int kGroup = kPacked ? 8 : 4;                  // span positions of a load group
  constexpr int kGroups = kDenseLoad * 4 / kGroup;         // load groups per thread and round
  using Regs = DenseRegs<kGroups, kPacked>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[O::kBytes];
  const int tid = threadIdx.x;
  auto* lent = reinterpret_cast<u32x4*>(smem + O::kOffEnt);
  auto* lent1 = reinterpret_cast<uint32_t*>(smem + O::kOffEnt);
  auto* lkey = reinterpret_cast<u32x2*>(smem + O::kOffEnt);  // FMT 1, 2: {min key, max key}
  auto* lcell = reinterpret_cast<uint32_t*>(smem + O::kOffCell);
  auto* lsum = reinterpret_cast<uint32_t*>(smem + O::kOffSum);
  auto* lerr = reinterpret_cast<uint32_t*>(smem + O::kOffErr);
  auto* lhi = reinterpret_cast<uint32_t*>(smem + O::kOffHi);
  for (uint32_t c = tid; c < ncodes; c += kThreads) {
    if constexpr (FMT == 0) {
      const u32x4 l = lay[c];
      lent[c] = u32x4{0xFFFFFFFFu, 0u, l.z - l.y, l.y | (l.w << 16)};
      lhi[c] = 0u;
    } else {
      lkey[c] = u32x2{0xFFFFFFFFu, 0u};
    }
    if constexpr (!kErrCells) lerr[c] = 0u;
  }
  // FMT 3: the entry of a cell's error spans lies err_off above the cell's own
  const uint32_t err_off = kErrCells ? 1u << fmt.cell_bits : 0u;
  if constexpr (kPacked) {  // code and flag of every cell: a wave per code, its lanes over the code's cells
    for (uint32_t c = (uint32_t)tid / kWave; c < ncodes; c += kWavesPerWG) {
      const u32x4 l = lay[c];
      for (uint32_t k = (uint32_t)tid % kWave; k < l.w; k += kWave) {
        lcell[l.z + k] = c << kPackCodeShift | kPackFlag;
        if constexpr (kErrCells) lcell[err_off + l.z + k] = c << kPackCodeShift | kPackFlag;
      }
    }
  } else {
    for (uint32_t k = tid; k < ncells; k += kThreads) lcell[k] = 0u;
  }
  for (uint32_t k = tid; k < ncodes * C::kReps; k += kThreads) lsum[k] = 0u;
  __syncthreads();
  const uint32_t rep = __lane_id() & (C::kReps - 1u);
  const uint32_t key_bits = cell_key_bits(fmt), cell_esc = cell_escape(fmt);
  // An escaping span of a cell-word column: its duration from dur_us, its
  // counts to the HBM tables (exact, and rare: nothing here is tuned).
  // FMT 2: span g of code c without its word's help (an escape, or a position
  // outside the launch's groups of 8).  In range: its LDS cell, and d - lo(bin)
  // of the sum; the rest to the HBM tables.
  auto direct = [&](uint32_t c, bool err, uint64_t g) {
    const u32x4 l = lay[c];
    const uint32_t d = dur[g], bin = hist_bin(d), k = bin - l.y;
    uint32_t part = d;
    if (k < l.w) {
      if constexpr (!(ANOMOD_ABL & 64)) atomicAdd(&lcell[l.z + k], 1u);
      part = d - hist_lo(bin);
    } else {
      if constexpr (!(ANOMOD_ABL & 64)) atomicAdd(&tab.hist[(uint64_t)l.x * kBins + bin], 1ull);
    }
    if constexpr (!(ANOMOD_ABL & 32)) {
      atomicAdd(&tab.sum[l.x], (unsigned long long)part);
      atomicMin(&tab.mn[l.x], d);
      atomicMax(&tab.mx[l.x], d);
      if (err) atomicAdd(&tab.err[l.x], 1ull);
    }
  };
  auto escaped = [&](uint32_t w, uint64_t g) {
    if constexpr (kPacked) {
      const uint32_t c = pack_word_escape_code(fmt, w);
      if (c < ncodes) direct(c, pack_word_error(fmt, w), g);
      return;
    }
    const uint32_t c = cell_word_code(fmt, w);
    if (c >= ncodes) return;
    const uint32_t d = dur[g], edge = lay[c].x;
    if constexpr (!(ANOMOD_ABL & 64)) atomicAdd(&tab.hist[(uint64_t)edge * kBins + hist_bin(d)], 1ull);
    if constexpr (!(ANOMOD_ABL & 32)) {
      atomicAdd(&tab.sum[edge], (unsigned long long)d);
      atomicMin(&tab.mn[edge], d);
      atomicMax(&tab.mx[edge], d);
      if ((w >> key_bits) & 1u) atomicAdd(&tab.err[edge], 1ull);
    }
  };
  // FMT 3, a span that found its entry's flag set: it may be an extreme of its
  // code c.  Once its cell lies strictly between the code's min and max cells
  // no later span of the cell is one, with the error bit or without: the flag
  // goes from both entries of the cell, so an error span — too few per
  // workgroup and cell to clear a flag of their own — takes the branch no
  // more often than a plain one.
  auto extreme = [&](uint32_t w, uint32_t cell, uint32_t c) {
    const uint32_t key = w & low_mask(key_bits);
    u32x2 e = lkey[c];
    if (key < e.x) atomicMin(&lent1[2u * c], key);
    if (key > e.y) atomicMax(&lent1[2u * c + 1u], key);
    e = lkey[c];
    if (cell > (e.x >> fmt.res_bits) && cell < (e.y >> fmt.res_bits)) {
      atomicAnd(&lcell[cell], ~kPackFlag);
      atomicAnd(&lcell[err_off + cell], ~kPackFlag);
    }
  };
  // w: the span word of position g.  FMT 0: a code past the layout's
  // (kWordNoCode: no span here) is skipped, so no index below leaves the carve;
  // the escape load is taken by the lanes that need it only.  FMT 1: a cell
  // past the layout's is the skip or the escape value; a word with a cell of
  // the layout was written by edge_encode_kernel with a code of the layout.
  auto one = [&](uint32_t w, uint64_t g) {
    if constexpr (FMT >= 1) {
      const uint32_t cell = cell_word_cell(fmt, w);
      if (__builtin_expect(cell >= ncells, 0)) {
        if (cell == cell_esc) escaped(w, g);
        return;
      }
      if constexpr ((ANOMOD_ABL & 96) == 96) {  // keep the loads, do nothing
        if (w == (kPacked ? 0x9E3779u : 0x9E3779B9u)) tab.err[0] = w;
        return;
      }
      if constexpr (kErrCells) {
        // As FMT 2 below, but an error span counts in the error entry of its
        // cell (w >> res_bits = error << cell_bits | cell): the flush reads the
        // error count off the entries, and the branch is left to the spans
        // that may be an extreme.
        const uint32_t old = atomicAdd(&lcell[pack_word_entry(fmt, w)], 1u), c = old >> kPackCodeShift;
        if constexpr (!(ANOMOD_ABL & 32)) {
          atomicAdd(&lsum[c * C::kReps + rep], cell_word_residual(fmt, w));
          if (__builtin_expect((old & kPackFlag) != 0u, 0)) extreme(w, cell, c);
        }
        return;
      }
      if constexpr (FMT == 2) {
        // One returning add on the cell counts the span and brings the cell's
        // code and flag.  The flag says that a span in this cell may still be
        // an extreme of its code; the first span that finds its cell strictly
        // between the code's min and max cells (which only move apart) clears
        // it, so the {min key, max key} read is left to the tails of a code's
        // range.  Error spans take the branch for their count.
        const uint32_t old = atomicAdd(&lcell[cell], 1u), c = old >> kPackCodeShift;
        if constexpr (!(ANOMOD_ABL & 32)) {
          atomicAdd(&lsum[c * C::kReps + rep], cell_word_residual(fmt, w));
          // (nothing above the error bit in a packed word)
          if (__builtin_expect(((old & kPackFlag) | (w >> key_bits)) != 0u, 0)) {
            const uint32_t key = w & low_mask(key_bits);
            if (w != key) atomicAdd(&lerr[c], 1u);
            if (old & kPackFlag) {
              u32x2 e = lkey[c];
              if (key < e.x) atomicMin(&lent1[2u * c], key);
              if (key > e.y) atomicMax(&lent1[2u * c + 1u], key);
              e = lkey[c];
              if (cell > (e.x >> fmt.res_bits) && cell < (e.y >> fmt.res_bits))
                atomicAnd(&lcell[cell], ~kPackFlag);
            }
          }
        }
        return;
      }
      const uint32_t c = cell_word_code(fmt, w);
      if constexpr (!(ANOMOD_ABL & 64)) atomicAdd(&lcell[cell], 1u);
      if constexpr (!(ANOMOD_ABL & 32)) {
        atomicAdd(&lsum[c * C::kReps + rep], cell_word_residual(fmt, w));
        const u32x2 e = lkey[c];
        const uint32_t ek = cell_word_ekey(fmt, w);
        // one branch around the three rare updates: error count, new min key, new max key
        if (__builtin_expect((ek < e.x) | (ek > e.y), 0)) {
          const uint32_t key = ek & low_mask(key_bits);
          if (ek != key) atomicAdd(&lerr[c], 1u);
          if (key < e.x) atomicMin(&lent1[2u * c], key);
          if (key > e.y) atomicMax(&lent1[2u * c + 1u], key);
        }
      }
    } else {
      const uint32_t c = span_word_code(w);
      if (c >= ncodes) return;
      if constexpr ((ANOMOD_ABL & 96) == 96) {  // keep the loads, do nothing
        if (w == 0x9E3779B9u) tab.err[0] = w;
        return;
      }
      uint32_t d = span_word_dur(w);
      if (__builtin_expect(d == kWordDurEscape, 0)) d = dur[g];
      const u32x4 e = lent[c];
      const uint32_t bin = dense_bin(d);
      if constexpr (!(ANOMOD_ABL & 64)) {
        if (bin - (e.w & 0xFFFFu) < (e.w >> 16))
          atomicAdd(&lcell[e.z + bin], 1u);
        else
          atomicAdd(&tab.hist[(uint64_t)lay[c].x * kBins + bin], 1ull);
      }
      if constexpr (!(ANOMOD_ABL & 32)) {
        // the sum in u32 replicas: an add that wraps its replica (seen in the
        // value it returns) counts a carry of 2^32 for the code
        const uint32_t before = atomicAdd(&lsum[c * C::kReps + rep], d);
        const bool carry = before + d < d, err = span_word_error(w);
        // one branch around the four rare updates
        if (__builtin_expect(carry | err | (d < e.x) | (d > e.y), 0)) {
          if (carry) atomicAdd(&lhi[c], 1u);
          if (d < e.x) atomicMin(&lent1[4u * c], d);
          if (d > e.y) atomicMax(&lent1[4u * c + 1u], d);
          if (err) atomicAdd(&lerr[c], 1u);
        }
      }
    }
  };
  constexpr uint64_t kG = kGroup, kGm = kG - 1ull;
  const uint64_t up = (lo + kGm) & ~kGm;
  const uint64_t a0 = up < hi ? up : hi;                      // head [lo, a0)
  const uint64_t a1 = (hi & ~kGm) > a0 ? (hi & ~kGm) : a0;    // groups [a0, a1), tail [a1, hi)
  if (blockIdx.x == 0 && tid < 2 * kGroup) {
    const uint64_t g = tid < kGroup ? lo + (uint64_t)tid : a1 + (uint64_t)(tid - kGroup);
    if (g < (tid < kGroup ? a0 : hi)) {
      if constexpr (kPacked) {
        const uint32_t w = pack_join(reinterpret_cast<const uint16_t*>(word)[g], wlo[g]);
        const uint32_t cell = cell_word_cell(fmt, w);
        if (cell < ncells)
          direct(lcell[cell] >> kPackCodeShift, pack_word_error(fmt, w), g);
        else if (cell == cell_esc)
          escaped(w, g);
      } else {
        one(word[g], g);
      }
    }
  }
  const uint64_t ng = (a1 - a0) / kG;
  // (FMT 2: a0 is a multiple of 8, so both planes' groups are aligned)
  const u32x4* w4 = kPacked ? reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(word) + a0)
                             : reinterpret_cast<const u32x4*>(word + a0);
  // groups past the end re-read the last one (no branch around a load) and
  // take skip words
  auto load = [&](uint64_t g0, Regs& R) {
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
      const uint64_t gi = g0 + (uint64_t)(j * kThreads + tid);
      const uint64_t gc = gi < ng ? gi : ng - 1;
      const u32x4 w = w4[gc];
      R.w[j] = gi < ng ? w : u32x4{kWordSkip, kWordSkip, kWordSkip, kWordSkip};
      if constexpr (kPacked) {
        const u32x2 b = reinterpret_cast<const u32x2*>(wlo + a0)[gc];
        R.b[j] = gi < ng ? b : u32x2{kWordSkip, kWordSkip};
      }
    }
  };
  constexpr uint64_t kPerBlock = (uint64_t)kThreads * kGroups;
  uint64_t g0 = (uint64_t)blockIdx.x * kPerBlock;
  Regs cur;
  if (g0 < ng) load(g0, cur);
  while (g0 < ng) {
    const uint64_t gn = g0 + (uint64_t)gridDim.x * kPerBlock;
    Regs nxt = cur;
    if (gn < ng) load(gn, nxt);
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
      const uint64_t g = a0 + kG * (g0 + (uint64_t)(j * kThreads + tid));
      if constexpr (kPacked) {
        const u32x4 h = cur.w[j];
        const u32x2 b = cur.b[j];
        // span j of the group: half j & 1 of h[j / 2] above byte j & 3 of b[j / 4]
        one(pack_pick<0>(h.x, b.x), g);
        one(pack_pick<1>(h.x, b.x), g + 1);
        one(pack_pick<2>(h.y, b.x), g + 2);
        one(pack_pick<3>(h.y, b.x), g + 3);
        one(pack_pick<0>(h.z, b.y), g + 4);
        one(pack_pick<1>(h.z, b.y), g + 5);
        one(pack_pick<2>(h.w, b.y), g + 6);
        one(pack_pick<3>(h.w, b.y), g + 7);
      } else {
        one(cur.w[j].x, g);
        one(cur.w[j].y, g + 1);
        one(cur.w[j].z, g + 2);
        one(cur.w[j].w, g + 3);
      }
    }
    cur = nxt;
    g0 = gn;
  }
  __syncthreads();
  // Flush: a wave per code, its lanes over the code's cells (FMT 1, 2: and the
  // cells' share of the code's sum, count * lo(bin), in u64); then the stats
  // through code -> edge.  Integer atomics: the tables stay bit-exact.
  const uint32_t wave = (uint32_t)tid / kWave, lane = (uint32_t)tid % kWave;
  for (uint32_t c = wave; c < ncodes; c += kWavesPerWG) {
    const u32x4 l = lay[c];
    unsigned long long* h = tab.hist + (uint64_t)l.x * kBins + l.y;
    unsigned long long part = 0ull;
    uint32_t nerr = 0u;  // FMT 3: the code's error spans, off its cells' error entries
    for (uint32_t k = lane; k < l.w; k += kWave) {
      uint32_t cnt = kPacked ? lcell[l.z + k] & kPackCount : lcell[l.z + k];
      if constexpr (kErrCells) {
        const uint32_t n1 = lcell[err_off + l.z + k] & kPackCount;
        cnt += n1;
        nerr += n1;
      }
      if (cnt) {
        atomicAdd(&h[k], (unsigned long long)cnt);
        if constexpr (FMT >= 1) part += (unsigned long long)cnt * hist_lo(l.y + k);
      }
    }
    if constexpr (FMT >= 1 && !(ANOMOD_ABL & 32)) {
      for (int o = kWave / 2; o > 0; o >>= 1) part += __shfl_xor(part, o);
      if (lane == 0 && part) atomicAdd(&tab.sum[l.x], part);
      if constexpr (kErrCells) {
        for (int o = kWave / 2; o > 0; o >>= 1) nerr += __shfl_xor(nerr, o);
        if (lane == 0 && nerr) atomicAdd(&tab.err[l.x], (unsigned long long)nerr);
      }
    }
  }
  for (uint32_t c = tid; c < ncodes; c += kThreads) {
    if constexpr (FMT >= 1) {
      const u32x2 e = lkey[c];
      if (e.x != 0xFFFFFFFFu) {  // (a first span always lowers the min key)
        const u32x4 l = lay[c];
        unsigned long long sum = 0ull;
        for (uint32_t k = 0; k < C::kReps; ++k) sum += lsum[c * C::kReps + k];
        atomicAdd(&tab.sum[l.x], sum);
        if constexpr (!kErrCells)
          if (lerr[c]) atomicAdd(&tab.err[l.x], (unsigned long long)lerr[c]);
        atomicMin(&tab.mn[l.x], cell_key_dur(fmt, e.x, l.y, l.z));
        atomicMax(&tab.mx[l.x], cell_key_dur(fmt, e.y, l.y, l.z));
      }
    } else {
      const u32x4 e = lent[c];
      if (e.x != 0xFFFFFFFFu || e.y != 0u) {
        const uint32_t edge = lay[c].x;
        unsigned long long sum = (unsigned long long)lhi[c] << 32;
        for (uint32_t k = 0; k < C::kReps; ++k) sum += lsum[c * C::kReps + k];
        atomicAdd(&tab.sum[edge], sum);
        if (lerr[c]) atomicAdd(&tab.err[edge], (unsigned long long)lerr[c]);
        atomicMin(&tab.mn[edge], e.x);
        atomicMax(&tab.mx[edge], e.y);
      }
    }
  }
}

// The span-word column of spans [lo, hi) from the parent rows, svc_flags and
// dur_us through the edge -> code table (e2c, u16 per edge, 0xFFFF = the
// layout has no code for this edge: *bad is set and the set stays on the row
// stream).  cell_words: the code's layout entry (lay, a few KB, cached) says
// which cell the duration's bin is and cell_word_encode packs cell and
// residual, or the escape value; else duration words.  Four span positions per
// thread; positions outside [lo, hi) are left alone.
__global__ __launch_bounds__(256) void edge_encode_kernel(
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint16_t* __restrict__ rows, const uint16_t* __restrict__ e2c,
    const u32x4* __restrict__ lay, bool cell_words, CellFmt fmt, uint32_t* __restrict__ word,
    uint64_t lo, uint64_t hi, uint32_t S, uint32_t S0, uint32_t* __restrict__ bad) {
  const uint64_t q0 = lo & ~3ull;
  const uint64_t nq = (hi - q0 + 3ull) / 4ull;
  auto enc = [&](uint32_t sf, uint32_t d, uint32_t row) -> uint32_t {
    if (row == 0xFFFFu) return kWordSkip;
    const uint32_t p = row >= S0 ? row - S0 + S : row;
    const uint32_t c = e2c[p * S + (sf & 0xFFFFu)];
    if (c == 0xFFFFu) {
      *bad = 1u;
      return kWordSkip;
    }
    const bool err = ((sf >> 16) & ANOMOD_FLAG_ERROR) != 0u;
    if (!cell_words) return span_word_pack(c, err, d);
    const u32x4 l = lay[c];
    return cell_word_encode(fmt, c, err, d, l.y, l.z, l.w);
  };
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq;
       q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g = q0 + 4ull * q;
    if (g >= lo && g + 4ull <= hi) {
      const u32x4 sf = *reinterpret_cast<const u32x4*>(svcfl + g);
      const u32x4 dr = *reinterpret_cast<const u32x4*>(dur + g);
      const u32x2 rw = *reinterpret_cast<const u32x2*>(rows + g);
      u32x4 out;
      out.x = enc(sf.x, dr.x, rw.x & 0xFFFFu);
      out.y = enc(sf.y, dr.y, rw.x >> 16);
      out.z = enc(sf.z, dr.z, rw.y & 0xFFFFu);
      out.w = enc(sf.w, dr.w, rw.y >> 16);
      *reinterpret_cast<u32x4*>(word + g) = out;
    } else {
      for (uint64_t i = g < lo ? lo : g; i < g + 4ull && i < hi; ++i)
        word[i] = enc(svcfl[i], dur[i], rows[i]);
    }
  }
}

// The same for a packing layout (p = pack_fmt of its widths): the two planes of
// the packed words, eight span positions per thread — one 16-B store of the
// high halves, one 8-B store of the low bytes — and the wide spans counted
// into *wide, one atomic per wave.
__global__ __launch_bounds__(256) void edge_encode_pack_kernel(
    const uint32_t* __restrict__ svcfl, const uint32_t* __restrict__ dur,
    const uint16_t* __restrict__ rows, const uint16_t* __restrict__ e2c,
    const u32x4* __restrict__ lay, CellFmt p, uint16_t* __restrict__ whi,
    unsigned char* __restrict__ wlo, uint64_t lo, uint64_t hi, uint32_t S, uint32_t S0,
    uint32_t* __restrict__ bad, unsigned long long* __restrict__ wide) {
  const uint64_t q0 = lo & ~7ull;
  const uint64_t nq = (hi - q0 + 7ull) / 8ull;
  uint32_t nwide = 0u;
  auto enc = [&](uint32_t sf, uint32_t d, uint32_t row) -> uint32_t {
    if (row == 0xFFFFu) return kPackSkip;
    const uint32_t pr = row >= S0 ? row - S0 + S : row;
    const uint32_t c = e2c[pr * S + (sf & 0xFFFFu)];
    if (c == 0xFFFFu) {
      *bad = 1u;
      return kPackSkip;
    }
    const u32x4 l = lay[c];
    bool w = false;
    const uint32_t word = pack_word_encode(p, c, ((sf >> 16) & ANOMOD_FLAG_ERROR) != 0u, d, l.y, l.z,
                                           l.w, &w);
    nwide += w ? 1u : 0u;
    return word;
  };
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq;
       q += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t g = q0 + 8ull * q;
    if (g >= lo && g + 8ull <= hi) {
      const u32x4 s0 = *reinterpret_cast<const u32x4*>(svcfl + g);
      const u32x4 s1 = *reinterpret_cast<const u32x4*>(svcfl + g + 4);
      const u32x4 d0 = *reinterpret_cast<const u32x4*>(dur + g);
      const u32x4 d1 = *reinterpret_cast<const u32x4*>(dur + g + 4);
      const u32x4 rw = *reinterpret_cast<const u32x4*>(rows + g);
      const uint32_t w[8] = {enc(s0.x, d0.x, rw.x & 0xFFFFu), enc(s0.y, d0.y, rw.x >> 16),
                             enc(s0.z, d0.z, rw.y & 0xFFFFu), enc(s0.w, d0.w, rw.y >> 16),
                             enc(s1.x, d1.x, rw.z & 0xFFFFu), enc(s1.y, d1.y, rw.z >> 16),
                             enc(s1.z, d1.z, rw.w & 0xFFFFu), enc(s1.w, d1.w, rw.w >> 16)};
      u32x4 h;
      h.x = (w[0] >> 8) | (w[1] >> 8) << 16;
      h.y = (w[2] >> 8) | (w[3] >> 8) << 16;
      h.z = (w[4] >> 8) | (w[5] >> 8) << 16;
      h.w = (w[6] >> 8) | (w[7] >> 8) << 16;
      u32x2 b;
      b.x = (w[0] & 0xFFu) | (w[1] & 0xFFu) << 8 | (w[2] & 0xFFu) << 16 | w[3] << 24;
      b.y = (w[4] & 0xFFu) | (w[5] & 0xFFu) << 8 | (w[6] & 0xFFu) << 16 | w[7] << 24;
      *reinterpret_cast<u32x4*>(whi + g) = h;
      *reinterpret_cast<u32x2*>(wlo + g) = b;
    } else {
      for (uint64_t i = g < lo ? lo : g; i < g + 8ull && i < hi; ++i) {
        const uint32_t w = enc(svcfl[i], dur[i], rows[i]);
        whi[i] = pack_hi(w);
        wlo[i] = pack_lo(w);
      }
    }
  }
  for (int o = kWave / 2; o > 0; o >>= 1) nwide += __shfl_xor(nwide, o);
  if (threadIdx.x % kWave == 0 && nwide) atomicAdd(wide, (unsigned long long)nwide);
}

// Count + nearest-rank quantiles per edge from the merged histogram: one
// wave per edge, 14 contiguous bins per lane, wave prefix sum.
constexpr int kBinsPerLane = (kBins + kWave - 1) / kWave;

__device__ __forceinline__ double quantile_from(uint64_t r, uint64_t excl, uint64_t incl,
                                                const uint64_t* v, int lane) {
  // Called only by the lane whose [excl, incl) contains r.
  uint64_t c = excl;
  for (int j = 0; j < kBinsPerLane; ++j) {
    c += v[j];
    if (r < c) {
      uint32_t lo, hi;
      hist_bounds((uint32_t)(lane * kBinsPerLane + j), &lo, &hi);
      return 0.5 * ((double)lo + (double)hi);
    }
  }
  return 0.0;
}

// Clears the table before a launch: words [0, nz) to zero (hist | err | sum |
// mx | ctr | big) and the E minima to all ones.  One launch in place of two
// memsets, which the runtime splits into several fill kernels (~40 us of
// launches per aggregation, against ~4 us for this).
__global__ __launch_bounds__(256) void edge_table_init_kernel(unsigned long long* __restrict__ z,
                                                              uint64_t nz,
                                                              unsigned int* __restrict__ mn,
                                                              uint32_t E) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint4* z4 = reinterpret_cast<uint4*>(z);  // the table base is 256-B aligned
  for (uint64_t i = i0; i < nz / 2; i += stride) z4[i] = make_uint4(0u, 0u, 0u, 0u);
  if ((nz & 1u) && i0 == 0) z[nz - 1] = 0ull;
  for (uint64_t i = i0; i < E; i += stride) mn[i] = 0xFFFFFFFFu;
}

__global__ __launch_bounds__(kWave) void edge_finalize_kernel(Table tab,
                                                              unsigned long long* count,
                                                              double* p50, double* p99) {
  const uint32_t e = blockIdx.x;
  const int lane = threadIdx.x;
  const unsigned long long* h = tab.hist + (uint64_t)e * kBins;
  uint64_t v[kBinsPerLane];
  uint64_t s = 0;
#pragma unroll
  for (int j = 0; j < kBinsPerLane; ++j) {
    const int b = lane * kBinsPerLane + j;
    v[j] = (b < (int)kBins) ? h[b] : 0ull;
    s += v[j];
  }
  uint64_t incl = s;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint64_t y = __shfl_up(incl, off);
    if (lane >= off) incl += y;
  }
  const uint64_t total = __shfl(incl, kWave - 1);
  const uint64_t excl = incl - s;
  if (lane == 0) {
    count[e] = total;
    if (total == 0) {
      p50[e] = NAN;
      p99[e] = NAN;
    }
  }
  if (total == 0) return;
  const uint64_t r50 = total * 50ull / 100ull;
  const uint64_t r99 = total * 99ull / 100ull;
  if (r50 >= excl && r50 < incl) p50[e] = quantile_from(r50, excl, incl, v, lane);
  if (r99 >= excl && r99 < incl) p99[e] = quantile_from(r99, excl, incl, v, lane);
}

// Exact nearest-rank picks from the per-span keys sorted by (edge, dur): one
// thread per edge finds its segment by binary search and reads
// x[(c * q) // 100] (the reference's sorted(x)[int(c*q)],
// monitor_http_responses.py:180-190).
__global__ __launch_bounds__(256) void exact_pick_kernel(const unsigned long long* __restrict__ sk,
                                                         uint64_t n, uint32_t E,
                                                         const uint32_t* __restrict__ q_pct,
                                                         uint32_t nq, double* __restrict__ out,
                                                         unsigned long long* __restrict__ count) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= E) return;
  auto lower = [&](unsigned long long key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) / 2;
      if (sk[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  const uint64_t a = lower((unsigned long long)e << 32);
  const uint64_t b = lower((unsigned long long)(e + 1u) << 32);
  const uint64_t c = b - a;
  if (count) count[e] = c;
  // the reference's int(c * q) with q = q_pct / 100 as a double (the same
  // double as the literal 0.95, ...: IEEE division rounds correctly), the
  // product truncated as Python's int() does (monitor_http_responses.py:
  // 188-189; x[len // 2] at :186 is the same index for q = 50)
  for (uint32_t k = 0; k < nq; ++k)
    out[(uint64_t)e * nq + k] =
        c ? (double)(uint32_t)sk[a + (uint64_t)((double)c * ((double)q_pct[k] / 100.0))]
          : (double)NAN;
}

using KernelFn = void (*)(const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*,
                          const uint64_t*, uint64_t, uint32_t, uint32_t, Table);
using KernelFn1 = void (*)(const uint64_t*, uint64_t, uint32_t, Table);

// The histogram form a set asks for: 0 pair, 1 compact, -1 unknown (pair with
// the saturation hand-off to a compact resume launch) — its hint, or
// ANOMOD_HIST_FORM = pair / compact / auto (tests force each).
// ANOMOD_HIST_FORM=auto: a form-unknown set takes the r04 auto form (pair
// table, saturated workgroups resumed compact) instead of the probe.
bool auto_forced() {
  const char* f = getenv("ANOMOD_HIST_FORM");
  return f && !strcmp(f, "auto");
}

// The form probe of a first aggregation: spans it covers, workgroups it runs.
constexpr uint64_t kFormProbeSpans = 1ull << 19;
constexpr uint64_t kFormProbeGroups = 16;

int hist_form_of(const anomod_spans* s) {
  const char* f = getenv("ANOMOD_HIST_FORM");
  if (f && !strcmp(f, "compact")) return 1;
  if (f && !strcmp(f, "pair")) return 0;
  if (f && !strcmp(f, "auto")) return -1;
  return s->hist_form;
}

// Collector-order probe of a unique-id set: over its first kProbeSpans spans,
// the share of child spans whose parent is the span right before them
// (0.60-0.75 on the generators in collector order, 0.02-0.11 shuffled inside
// the traces; a pair across a trace boundary matches only by id collision).
constexpr uint64_t kProbeSpans = 1u << 20;
__global__ __launch_bounds__(256) void order_probe_kernel(const uint64_t* __restrict__ sid,
                                                          const uint64_t* __restrict__ pid,
                                                          uint64_t n,
                                                          unsigned long long* __restrict__ cnt) {
  uint32_t ch = 0, adj = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; i < n;
       i += (uint64_t)gridDim.x * 256) {
    const uint64_t p = pid[i];
    ch += p != 0ull ? 1u : 0u;
    adj += (p != 0ull && p == sid[i - 1]) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) {
    ch += __shfl_xor(ch, o);
    adj += __shfl_xor(adj, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&cnt[0], (unsigned long long)ch);
    atomicAdd(&cnt[1], (unsigned long long)adj);
  }
}

// The set's order probe when its order hint is unknown (the first
// aggregation of a unique-id set): the counts go to h[0..1] (pinned) once the
// caller waits; probe_order_take sets the hint from them.
bool need_order_probe(const anomod_spans* s) { return s->unique_ids && s->order < 0; }

int probe_order_launch(anomod_ctx* ctx, const anomod_spans* s, unsigned long long* d_cnt,
                       unsigned long long* h) {
  h[0] = h[1] = 0ull;
  const uint64_t n = std::min<uint64_t>(s->n_spans, kProbeSpans);
  if (n > 1) {
    ANOMOD_HIP(ctx, hipMemsetAsync(d_cnt, 0, 16, ctx->stream));
    hipLaunchKernelGGL(order_probe_kernel, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 256)),
                       dim3(256), 0, ctx->stream, s->span_id, s->parent_span_id, n, d_cnt);
    ANOMOD_HIP(ctx, hipGetLastError());
    ANOMOD_HIP(ctx, hipMemcpyAsync(h, d_cnt, 16, hipMemcpyDeviceToHost, ctx->stream));
  }
  return ANOMOD_OK;
}

void probe_order_take(const anomod_spans* s, const unsigned long long* h) {
  s->order = 4ull * h[1] >= h[0] ? 1 : 0;
}

// Sets the set's order hint when unknown (one small kernel and one host
// wait, the first aggregation of the set only).
int probe_order(anomod_ctx* ctx, const anomod_spans* s, unsigned long long* d_cnt) {
  if (!need_order_probe(s)) return ANOMOD_OK;
  // the pinned read-back (a ctx's first call may be this one: the exact
  // quantiles allocate no staging of their own)
  if (int rc = ensure_host_stage(ctx, 32)) return rc;
  unsigned long long* h = static_cast<unsigned long long*>(ctx->h_stage);
  if (int rc = probe_order_launch(ctx, s, d_cnt, h)) return rc;
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  probe_order_take(s, h);
  return ANOMOD_OK;
}

// Whether the bidirectional parent scan is used: a unique-id set in collector
// order (ANOMOD_UNIQUE_SCAN=0 forces the forward scan, =1 the bidirectional
// one whatever the order: tests, A/B).  Every other set takes the
// first-match forward scan, correct for any set.
bool use_unique(const anomod_spans* s) {
  const char* f = getenv("ANOMOD_UNIQUE_SCAN");
  if (f && !strcmp(f, "0")) return false;
  if (f && !strcmp(f, "1")) return s->unique_ids;
  return s->unique_ids && s->order == 1;
}

struct Pick {
  KernelFn fn;
  int ht, st;
  const char* name;
};

// mode: kModeAuto only for the pair forms, kModeResume only for the compact
// forms of the SN / TrainTicket widths (the instantiations that exist).
// rows: the instantiation that also fills the set's parent-row column (the
// forms of known-form launches only: kModeNormal / the wide scan).
Pick pick_kernel(uint32_t E, bool compact, bool uni, int mode = kModeNormal, bool long_set = false,
                 bool rows = false) {
  const uint64_t keys = (uint64_t)E * kBins + 1;  // largest stored key
  const bool lds_hist = keys < (1ull << 31);  // >= 1 count bit above the key
#define ANOMOD_PICK(H, S_, NAME)                                                               \
  return Pick{rows ? (uni ? edge_agg_kernel<H, S_, true, kModeNormal, true>                    \
                          : edge_agg_kernel<H, S_, false, kModeNormal, true>)                  \
                   : (uni ? edge_agg_kernel<H, S_, true> : edge_agg_kernel<H, S_, false>),     \
              H, S_, NAME}
#define ANOMOD_PICK_M(H, S_, M, NAME)                                                          \
  return Pick{uni ? edge_agg_kernel<H, S_, true, M> : edge_agg_kernel<H, S_, false, M>, H, S_, NAME}
  if (lds_hist && E <= kLdsEdges && mode == kModeResume)
    ANOMOD_PICK_M(kHtCompact, kStDirect, kModeResume, "edge_agg_kernel<lds_compact_hist,lds_stats,resume>");
  if (lds_hist && E <= kLdsEdges && !compact && mode == kModeAuto)
    ANOMOD_PICK_M(kHtPair, kStDirect, kModeAuto, "edge_agg_kernel<lds_hist,lds_stats,auto>");
  if (lds_hist && E > kLdsEdges && E <= kWideEdges && mode == kModeResume)
    ANOMOD_PICK_M(kHtCompact, kStWide, kModeResume, "edge_agg_kernel<lds_compact_hist,wide_stats,resume>");
  if (lds_hist && E > kLdsEdges && E <= kWideEdges && !compact && mode == kModeAuto)
    ANOMOD_PICK_M(kHtPair, kStWide, kModeAuto, "edge_agg_kernel<lds_hist,wide_stats,auto>");
  if (lds_hist && E <= kLdsEdges && compact && uni && long_set && mode == kModeNormal)
    return Pick{rows ? edge_agg_kernel<kHtCompact, kStDirect, true, kModeWideScan, true>
                     : edge_agg_kernel<kHtCompact, kStDirect, true, kModeWideScan>,
                kHtCompact, kStDirect, "edge_agg_kernel<lds_compact_hist,lds_stats,wide_scan>"};
  if (lds_hist && E <= kLdsEdges && compact)  // a set that overflowed the pair table
    ANOMOD_PICK(kHtCompact, kStDirect, "edge_agg_kernel<lds_compact_hist,lds_stats>");
  if (lds_hist && E <= kLdsEdges) ANOMOD_PICK(kHtPair, kStDirect, "edge_agg_kernel<lds_hist,lds_stats>");
  // TrainTicket width: the pair form while the set's keys fit it (whole-ms
  // SkyWalking latencies give a few thousand (edge, bin) keys per
  // workgroup), the compact form once it overflowed
  if (lds_hist && E <= kWideEdges && !compact)
    ANOMOD_PICK(kHtPair, kStWide, "edge_agg_kernel<lds_hist,wide_stats>");
  if (lds_hist && E <= kWideEdges)
    ANOMOD_PICK(kHtCompact, kStWide, "edge_agg_kernel<lds_compact_hist,wide_stats>");
  if (lds_hist) ANOMOD_PICK(kHtCompact, kStSlot, "edge_agg_kernel<lds_compact_hist,slot_stats>");
  ANOMOD_PICK(kHtHbm, kStHbm, "edge_agg_kernel<hbm_hist,hbm_stats>");
#undef ANOMOD_PICK
#undef ANOMOD_PICK_M
}

// ---- parent rows of a resident set ------------------------------------------
// Whether a call may fill / read the set's parent-row column: a grouped set
// that outlives the call, with none of the experiment overrides set
// (ANOMOD_HIST_FORM and ANOMOD_UNIQUE_SCAN ask for a walk kernel by name;
// ANOMOD_PARENT_ROWS=0 is the A/B switch).  Otherwise the call walks the
// traces as if the column did not exist.
bool rows_allowed(const anomod_spans* s) {
  const char* f = getenv("ANOMOD_PARENT_ROWS");
  if (f && !strcmp(f, "0")) return false;
  if (getenv("ANOMOD_HIST_FORM") || getenv("ANOMOD_UNIQUE_SCAN")) return false;
  return s->keep_rows && s->grouped;
}

bool rows_ready(const anomod_spans* s) {
  return rows_allowed(s) && s->parent_row && s->rows_done;
}

using RowFn = void (*)(const uint32_t*, const uint32_t*, const uint16_t*, uint64_t, uint64_t,
                       uint32_t, uint32_t, uint32_t, Table);
struct RowPick {
  RowFn fn;
  int ht;
  const char* name;
};

// The stream kernel of the table form pick_kernel gives the set.
RowPick pick_row_kernel(uint32_t E, bool compact) {
  const Pick pk = pick_kernel(E, compact, false);
  if (pk.ht == kHtPair && pk.st == kStDirect)
    return {edge_row_kernel<kHtPair, kStDirect>, kHtPair, "edge_row_kernel<lds_hist,lds_stats>"};
  if (pk.ht == kHtCompact && pk.st == kStDirect)
    return {edge_row_kernel<kHtCompact, kStDirect>, kHtCompact,
            "edge_row_kernel<lds_compact_hist,lds_stats>"};
  if (pk.ht == kHtPair && pk.st == kStWide)
    return {edge_row_kernel<kHtPair, kStWide>, kHtPair, "edge_row_kernel<lds_hist,wide_stats>"};
  if (pk.ht == kHtCompact && pk.st == kStWide)
    return {edge_row_kernel<kHtCompact, kStWide>, kHtCompact,
            "edge_row_kernel<lds_compact_hist,wide_stats>"};
  if (pk.ht == kHtCompact && pk.st == kStSlot)
    return {edge_row_kernel<kHtCompact, kStSlot>, kHtCompact,
            "edge_row_kernel<lds_compact_hist,slot_stats>"};
  return {edge_row_kernel<kHtHbm, kStHbm>, kHtHbm, "edge_row_kernel<hbm_hist,hbm_stats>"};
}

// The set's spans [rows_lo, rows_hi) through fn, at most max_launch_spans()
// per launch (the LDS tables' u32 counters).
int launch_rows(anomod_ctx* ctx, const anomod_spans* s, RowFn fn, uint32_t S, uint32_t E,
                const Table& tab) {
  int per_cu = 0;
  ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void*>(fn), kThreads, 0));
  const uint64_t cap = max_launch_spans();
  constexpr uint64_t kRound = (uint64_t)kThreads * kRowLoad * 4;  // spans per workgroup round
  for (uint64_t a = s->rows_lo; a < s->rows_hi; a += cap) {
    const uint64_t b = std::min<uint64_t>(s->rows_hi, a + cap);
    const uint64_t want = (b - a + kRound - 1) / kRound;
    const uint64_t grid = std::min<uint64_t>((uint64_t)ctx->num_cus * (per_cu > 0 ? per_cu : 1), want);
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, s->svc_flags,
                       s->dur_us, s->parent_row, a, b, S, s->rows_S, E, tab);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  return ANOMOD_OK;
}

// ---- dense stream of a resident set (edge_dense_kernel) ---------------------
// Spans of a workgroup round (every thread: kLoad groups of 4), and the rounds
// a workgroup of the cell-word kernel may run in one launch without a sum
// replica reaching 2^32.  A replica is fed by the kThreads / kReps threads
// that share its lane bits, 4 * kLoad residuals below 2^res_bits each per
// round, and by at most one head or tail span (workgroup 0, lanes 0 .. 7).
uint64_t dense_round_spans(int tier) {
  return (uint64_t)kThreads * 4 * (tier ? DenseCfg<1>::kLoad : DenseCfg<0>::kLoad);
}
uint64_t dense_sum_rounds(int tier, uint32_t res_bits) {
  const uint64_t per_rep = dense_round_spans(tier) / (tier ? DenseCfg<1>::kReps : DenseCfg<0>::kReps);
  const uint64_t top = low_mask(res_bits);  // the largest residual
  if (top == 0) return UINT64_MAX / dense_round_spans(tier) / kDenseMaxWgs;
  return std::min<uint64_t>((0xFFFFFFFFull / top - 1ull) / per_rep,
                            UINT64_MAX / dense_round_spans(tier) / kDenseMaxWgs);
}
// ANOMOD_EDGE_DENSE=0 is the A/B switch; everything that bypasses the parent
// rows bypasses this too (the callers ask rows_allowed first).
bool dense_allowed() {
  const char* f = getenv("ANOMOD_EDGE_DENSE");
  return !(f && !strcmp(f, "0"));
}
// ANOMOD_DENSE_PACK=0: a layout that would pack keeps 4-byte cell words (A/B).
bool pack_allowed() {
  const char* f = getenv("ANOMOD_DENSE_PACK");
  return !(f && !strcmp(f, "0"));
}
// ANOMOD_DENSE_ERRCELLS=0: a packed layout of the small carve keeps
// edge_dense_kernel<0, 2>, its error count in the span path (A/B).
bool errcells_allowed() {
  const char* f = getenv("ANOMOD_DENSE_ERRCELLS");
  return !(f && !strcmp(f, "0"));
}

// The set's layout for S from one of its own tables (count / min / max per
// edge, on the host): codes by edge order, bin ranges back to back in the
// cell array.  The set is dense when codes <= 512 and cells <= 32 Ki (small
// carve: <= 64 codes and <= 8 Ki cells); otherwise this S is remembered as
// not fitting and the set keeps the row stream.  ANOMOD_DENSE_SHRINK=1
// (tests) narrows every range by one bin at each end, so that the extremes
// take the kernel's out-of-range path.
void dense_learn(const anomod_spans* s, uint32_t S, uint32_t E, const unsigned long long* count,
                 const uint32_t* mn, const uint32_t* mx) {
  if (!s->dense) s->dense.reset(new DenseSet());
  DenseSet& d = *s->dense;
  d.state = DenseSet::kNone;
  d.S = S;
  d.codes = d.cells = 0;
  d.streams = 0;
  d.wgs_per_cu = 0;
  d.cell_words = d.pack = d.errcells = false;
  d.host.clear();
  const char* sh = getenv("ANOMOD_DENSE_SHRINK");
  const bool shrink = sh && !strcmp(sh, "1");
  uint64_t codes = 0, cells = 0;
  uint32_t max_exp = 0;  // the largest bin exponent of any range
  if (E <= kDenseMaxEdges) {
    for (uint32_t e = 0; e < E; ++e) {
      if (!count[e]) continue;
      uint32_t b0 = hist_bin(mn[e]), b1 = hist_bin(mx[e]);
      uint32_t width = b1 >= b0 ? b1 - b0 + 1u : 0u;  // (a table merged over ranks: still a range)
      if (shrink) {
        b0 += 1u;
        width = width > 2u ? width - 2u : 0u;
      }
      if (codes < DenseCfg<1>::kCodes) {
        const uint32_t ent[4] = {e, b0, (uint32_t)cells, width};
        d.host.insert(d.host.end(), ent, ent + 4);
      }
      ++codes;
      cells += width;
      if (width) max_exp = std::max(max_exp, hist_exp(b0 + width - 1u));
    }
  }
  const bool fits = E <= kDenseMaxEdges && codes >= 1 && codes <= DenseCfg<1>::kCodes &&
                    cells <= DenseCfg<1>::kCells;
  d.codes = (uint32_t)std::min<uint64_t>(codes, 0xFFFFFFFFull);
  d.cells = (uint32_t)std::min<uint64_t>(cells, 0xFFFFFFFFull);
  d.tier = codes <= DenseCfg<0>::kCodes && cells <= DenseCfg<0>::kCells ? 0 : 1;
  if (fits) {
    std::vector<uint16_t> e2c(((size_t)E + 1) & ~size_t(1), (uint16_t)0xFFFFu);
    for (uint32_t c = 0; c < (uint32_t)codes; ++c) e2c[d.host[4u * c]] = (uint16_t)c;
    const size_t at = d.host.size();
    d.host.resize(at + e2c.size() / 2);
    memcpy(d.host.data() + at, e2c.data(), e2c.size() * 2);
    d.state = DenseSet::kLearned;
    // Cell words when code, error bit, cell (and its two reserved values) and
    // the widest residual fit 32 bits, and the residuals of one workgroup round
    // fit a sum replica; else duration words and the per-span code as before.
    d.fmt = cell_fmt(d.codes, d.cells, max_exp);
    d.cell_words = cell_fmt_fits(d.fmt) && dense_sum_rounds(d.tier, d.fmt.res_bits) >= 1;
    // ... and packed, 3 B per span, when the layout also keeps to 256 codes and
    // 15 cell bits (span_word.h)
    d.pack = d.cell_words && pack_allowed() && pack_fmt_fits(d.fmt, d.codes);
    // ... read by the kernel with error cells when the small carve has room for
    // two entries per cell, the error entry 2^cell_bits above the cell's own
    d.errcells = d.pack && d.tier == 0 && errcells_allowed() &&
                 (1ull << d.fmt.cell_bits) + d.cells <= DenseCfg<2>::kCells;
  } else {
    d.host.clear();
  }
  if (log_kernel())  // (tests)
    fprintf(stderr, "anomod: edge dense layout S=%u codes=%u cells=%u: %s\n", S, d.codes, d.cells,
            !fits ? "does not fit, the set keeps the row stream" : d.tier ? "large" : "small");
  if (log_kernel() && fits) {
    if (d.cell_words)
      fprintf(stderr, "anomod: edge dense words S=%u format=cell code_bits=%u cell_bits=%u res_bits=%u\n",
              S, d.fmt.code_bits, d.fmt.cell_bits, d.fmt.res_bits);
    else
      fprintf(stderr, "anomod: edge dense words S=%u format=dur code_bits=%u cell_bits=0 res_bits=%u\n",
              S, kWordCodeBits, kWordDurBits);
    if (d.pack)
      fprintf(stderr, "anomod: edge dense pack S=%u bytes=3 cell_bits=%u res_bits=%u\n", S,
              pack_fmt(d.fmt).cell_bits, pack_fmt(d.fmt).res_bits);
    if (d.errcells)
      fprintf(stderr, "anomod: edge dense errcells S=%u entries=%u\n", S,
              (1u << d.fmt.cell_bits) + d.cells);
  }
}

// The transition call of a learned layout.  dense_alloc: device room for the layout and
// the word column (false: an allocation failed, the set stays on the row
// stream).  dense_encode: the layout to the device and the word column of
// [rows_lo, rows_hi), queued after the row stream of this call; the flag word
// comes back into *h_bad with the table.
size_t dense_flag_offset(const DenseSet& d) { return (d.host.size() * 4 + 7) & ~size_t(7); }
unsigned char* dense_lo_plane(const DenseSet& d, const anomod_spans* s) {
  return reinterpret_cast<unsigned char*>(d.word) + pack_lo_offset(s->n_spans);
}
bool dense_alloc(anomod_ctx* ctx, const anomod_spans* s) {
  DenseSet& d = *s->dense;
  // (the layout, then the encoder's flag word and its u64 count of wide spans)
  const size_t bytes = dense_flag_offset(d) + 16;
  if (d.dev_bytes < bytes) {
    if (d.dev) (void)hipFree(d.dev);
    d.dev = nullptr;
    d.dev_bytes = 0;
    if (dev_malloc(ctx, &d.dev, bytes) != hipSuccess) {
      (void)hipGetLastError();
      d.dev = nullptr;
      return false;
    }
    d.dev_bytes = bytes;
  }
  const size_t need = d.pack ? pack_column_bytes(s->n_spans) : s->n_spans * 4;
  if (d.word_bytes < need) {
    if (d.word) (void)hipFree(d.word);
    d.word = nullptr;
    d.word_bytes = 0;
    void* p = nullptr;
    if (dev_malloc(ctx, &p, need) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    d.word = static_cast<uint32_t*>(p);
    d.word_bytes = need;
  }
  return true;
}

int dense_encode(anomod_ctx* ctx, const anomod_spans* s, uint32_t S, uint32_t* h_bad) {
  DenseSet& d = *s->dense;
  auto* base = static_cast<uint32_t*>(d.dev);
  auto* d_bad = reinterpret_cast<uint32_t*>(static_cast<char*>(d.dev) + dense_flag_offset(d));
  ANOMOD_HIP(ctx, hipMemcpyAsync(base, d.host.data(), d.host.size() * 4, hipMemcpyHostToDevice,
                                 ctx->stream));
  ANOMOD_HIP(ctx, hipMemsetAsync(d_bad, 0, 16, ctx->stream));
  const uint64_t nq = (s->rows_hi - (s->rows_lo & ~3ull) + 3) / 4;
  if (nq && d.pack) {
    const uint64_t n8 = (s->rows_hi - (s->rows_lo & ~7ull) + 7) / 8;
    const uint64_t blocks = std::min<uint64_t>((n8 + 255) / 256, 64ull * ctx->num_cus);
    hipLaunchKernelGGL(edge_encode_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       s->svc_flags, s->dur_us, s->parent_row,
                       reinterpret_cast<const uint16_t*>(base + 4u * d.codes),
                       reinterpret_cast<const u32x4*>(base), pack_fmt(d.fmt),
                       reinterpret_cast<uint16_t*>(d.word), dense_lo_plane(d, s), s->rows_lo,
                       s->rows_hi, S, s->rows_S, d_bad,
                       reinterpret_cast<unsigned long long*>(d_bad + 2));
    ANOMOD_HIP(ctx, hipGetLastError());
  } else if (nq) {
    const uint64_t blocks = std::min<uint64_t>((nq + 255) / 256, 64ull * ctx->num_cus);
    hipLaunchKernelGGL(edge_encode_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       s->svc_flags, s->dur_us, s->parent_row,
                       reinterpret_cast<const uint16_t*>(base + 4u * d.codes),
                       reinterpret_cast<const u32x4*>(base), d.cell_words, d.fmt, d.word,
                       s->rows_lo, s->rows_hi, S, s->rows_S, d_bad);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  ANOMOD_HIP(ctx, hipMemcpyAsync(h_bad, d_bad, 16, hipMemcpyDeviceToHost, ctx->stream));
  return ANOMOD_OK;
}

// The set's spans [rows_lo, rows_hi) through the dense kernel of its tier and
// word format, at most max_launch_spans() per launch (u32 cells) and, with
// cell words, at most dense_sum_rounds() rounds per workgroup (u32 sum
// replicas without a carry).  ANOMOD_DENSE_WGS caps the grid (tests, A/B).
int launch_dense(anomod_ctx* ctx, const anomod_spans* s, const Table& tab) {
  DenseSet& d = *s->dense;
  const int f = d.pack ? (d.errcells ? 3 : 2) : d.cell_words ? 1 : 0;
  auto fn = d.tier ? (f == 2 ? edge_dense_kernel<1, 2> : f ? edge_dense_kernel<1, 1> : edge_dense_kernel<1, 0>)
            : f == 3 ? edge_dense_kernel<0, 3>
                     : (f == 2 ? edge_dense_kernel<0, 2> : f ? edge_dense_kernel<0, 1> : edge_dense_kernel<0, 0>);
  if (d.wgs_per_cu <= 0) {  // resident workgroups per CU, asked once per layout
    int per_cu = 0;
    ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                        &per_cu, reinterpret_cast<const void*>(fn), kThreads, 0));
    d.wgs_per_cu = std::max(1, std::min(d.tier == 0 ? kDenseSmallWgs : 1, per_cu));
  }
  const uint64_t wgs = std::min<uint64_t>(
      {(uint64_t)ctx->num_cus * d.wgs_per_cu, env_cap("ANOMOD_DENSE_WGS", 1), kDenseMaxWgs});
  const uint64_t kRound = dense_round_spans(d.tier);
  uint64_t cap = max_launch_spans();
  if (d.cell_words) {
    const uint64_t by_sum = dense_sum_rounds(d.tier, d.fmt.res_bits) * wgs * kRound;
    if (by_sum < cap) {
      cap = by_sum;
      if (log_kernel() && s->rows_hi - s->rows_lo > cap)  // (tests)
        fprintf(stderr, "anomod: edge dense sum bound: %llu spans per launch on %llu workgroups\n",
                (unsigned long long)cap, (unsigned long long)wgs);
    }
  }
  // (packed words: a cell counts in 23 bits a workgroup's rounds and its head and tail spans)
  if (d.pack) cap = std::min<uint64_t>(cap, (kPackCount - 14u) / kRound * kRound * wgs);
  for (uint64_t a = s->rows_lo; a < s->rows_hi; a += cap) {
    const uint64_t b = std::min<uint64_t>(s->rows_hi, a + cap);
    const uint64_t want = (b - a + kRound - 1) / kRound;
    const uint64_t grid = std::min<uint64_t>(wgs, want);
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, s->dur_us, d.word,
                       static_cast<const u32x4*>(d.dev), d.codes, d.cells,
                       d.pack ? pack_fmt(d.fmt) : d.fmt, a, b, tab,
                       d.pack ? dense_lo_plane(d, s) : nullptr);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  return ANOMOD_OK;
}

// Device table layout inside ctx->d_table: hist | err | sum (u64, one sum
// all-reduce) | mx (u32, zero-initialised with them: one memset) | pad |
// ctr (u64) | big counters (u64 x 3) + probe scratch (u64 x 2) | pair-table
// overflows + stopped workgroups (u64 x 2) | ranges left + resume ticket
// (u64 x 2; all zeroed with them) | count | p50 | p99 | mn | long-trace list |
// ranges left by stopped waves (u64 pairs) | long-trace parent rows (u16 per
// span).  [off_err, end_small) is copied to the host in one D2H.
struct Layout {
  uint64_t E;
  size_t off_hist, off_err, off_sum, off_mx, off_ctr, off_big, off_ovf, off_nleft, off_count,
      off_p50, off_p99, off_mn, end_small, off_left, bytes;
  size_t off_bpar = 0;
  Layout(uint64_t e, uint64_t big_cap, uint64_t n_spans = 0, uint64_t left_cap = 0) : E(e) {
    off_hist = 0;
    off_err = off_hist + E * kBins * 8;
    off_sum = off_err + E * 8;
    off_mx = off_sum + E * 8;
    off_ctr = (off_mx + E * 4 + 7) & ~size_t(7);
    off_big = off_ctr + 8;
    off_ovf = off_big + 40;  // listed, two tickets, two words of order-probe scratch
    off_nleft = off_ovf + 16;
    off_count = off_nleft + 16;
    off_p50 = off_count + E * 8;
    off_p99 = off_p50 + E * 8;
    off_mn = off_p99 + E * 8;
    end_small = off_mn + E * 4;
    off_left = ((end_small + 7) & ~size_t(7)) + big_cap * 8;
    bytes = off_left + left_cap * 16;
    off_bpar = bytes;                           // u16 parent rows, by span position
    if (big_cap) bytes += (n_spans * 2 + 7) & ~size_t(7);
  }
  size_t off_list() const { return (end_small + 7) & ~size_t(7); }
};

// Long traces (> kBigMin spans) a span set can hold: 0 when its longest trace
// is known to fit a chunk.
uint64_t big_capacity(const anomod_spans* s) {
  if (s->max_trace_len <= (uint64_t)kBigMin) return 0;
  const uint64_t by_spans = s->n_spans / (uint64_t)(kBigMin + 1);
  return by_spans < s->n_traces ? by_spans : s->n_traces;
}

// The long-trace pass after the chunk walk (no-op when nothing was listed),
// with the chunk walk's table forms.
template <int HT, int ST>
hipError_t launch_big(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S, uint32_t E,
                      const Table& tab) {
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void*>(edge_big_resolve_kernel), kResThreads, 0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(edge_big_resolve_kernel, dim3((unsigned)(ctx->num_cus * std::max(per_cu, 1))),
                     dim3(kResThreads), 0, ctx->stream, spans->span_id, spans->parent_span_id,
                     spans->svc_flags, spans->dur_us, spans->trace_ptr, S, tab);
  if ((e = hipGetLastError()) != hipSuccess || HT == kHtKeys) return e;
  hipLaunchKernelGGL((edge_big_record_kernel<HT, ST>), dim3((unsigned)ctx->num_cus),
                     dim3(kBigThreads), 0, ctx->stream, spans->svc_flags, spans->dur_us,
                     spans->trace_ptr, S, E, tab);
  return hipGetLastError();
}

hipError_t launch_big_for(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S, uint32_t E,
                          const Table& tab) {
  // the LDS tables' u32 counters hold < 2^32 records per workgroup: a set
  // whose listed traces could exceed a launch's bound records to HBM
  if (spans->n_spans >= max_launch_spans()) return launch_big<kHtHbm, kStHbm>(ctx, spans, S, E, tab);
  // the pair form only for a set known to fit it (a form-unknown set records
  // its long traces in the compact form, which has no probe chain)
  const Pick pk = pick_kernel(E, hist_form_of(spans) != 0, false);
  if (pk.ht == kHtPair && pk.st == kStDirect)
    return launch_big<kHtPair, kStDirect>(ctx, spans, S, E, tab);
  if (pk.ht == kHtCompact && pk.st == kStDirect)
    return launch_big<kHtCompact, kStDirect>(ctx, spans, S, E, tab);
  if (pk.ht == kHtPair && pk.st == kStWide)
    return launch_big<kHtPair, kStWide>(ctx, spans, S, E, tab);
  if (pk.ht == kHtCompact && pk.st == kStWide)
    return launch_big<kHtCompact, kStWide>(ctx, spans, S, E, tab);
  if (pk.ht == kHtCompact && pk.st == kStSlot)
    return launch_big<kHtCompact, kStSlot>(ctx, spans, S, E, tab);
  return launch_big<kHtHbm, kStHbm>(ctx, spans, S, E, tab);
}

// Pointers of every section of the device table for layout L.
Table table_at(anomod_ctx* ctx, const Layout& L, uint32_t E) {
  char* base = static_cast<char*>(ctx->d_table);
  Table tab{};  // keys = nullptr: the table forms, not the exact-quantile keys
  tab.hist = reinterpret_cast<unsigned long long*>(base + L.off_hist);
  tab.err = reinterpret_cast<unsigned long long*>(base + L.off_err);
  tab.sum = reinterpret_cast<unsigned long long*>(base + L.off_sum);
  tab.mn = reinterpret_cast<unsigned int*>(base + L.off_mn);
  tab.mx = reinterpret_cast<unsigned int*>(base + L.off_mx);
  tab.ctr = reinterpret_cast<unsigned long long*>(base + L.off_ctr);
  tab.big = reinterpret_cast<unsigned long long*>(base + L.off_big);
  tab.big_list = reinterpret_cast<unsigned long long*>(base + L.off_list());
  tab.bpar = reinterpret_cast<uint16_t*>(base + L.off_bpar);
  tab.ovf = reinterpret_cast<unsigned long long*>(base + L.off_ovf);
  tab.nleft = reinterpret_cast<unsigned long long*>(base + L.off_nleft);
  tab.left = reinterpret_cast<unsigned long long*>(base + L.off_left);
  tab.mode = kModeNormal;
  tab.occupancy = 0;
  tab.kb = 1;
  while (((uint64_t)E * kBins + 1) >> tab.kb) ++tab.kb;  // bits of the largest key
  return tab;
}

// hist | err | sum | mx | counters to zero, mn to all ones (one launch).
int table_clear(anomod_ctx* ctx, const Layout& L, const Table& tab, uint32_t E) {
  const uint64_t nz = L.off_count / 8;  // hist|err|sum|mx|ctr|big|ovf|nleft
  const uint64_t blocks = std::min<uint64_t>((nz / 2 + 255) / 256 + 1, 4ull * ctx->num_cus);
  hipLaunchKernelGGL(edge_table_init_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                     static_cast<unsigned long long*>(ctx->d_table), nz, tab.mn, E);
  ANOMOD_HIP(ctx, hipGetLastError());
  return ANOMOD_OK;
}

// After the aggregation kernels: the merge over an attached communicator, the
// quantiles, and the table to the caller's arrays; ovf[0..1] = the table's
// two overflow words.
int table_finish(anomod_ctx* ctx, const Layout& L, const Table& tab, uint32_t E,
                 anomod_edge_table* out, unsigned long long* ovf) {
  char* base = static_cast<char*>(ctx->d_table);
  auto* count = reinterpret_cast<unsigned long long*>(base + L.off_count);
  auto* p50 = reinterpret_cast<double*>(base + L.off_p50);
  auto* p99 = reinterpret_cast<double*>(base + L.off_p99);
  // Any attached communicator merges, a 1-rank one included (an identity
  // reduce, so the RCCL call sequence is exercised on a single-GPU box too).
  if (comm_attached(ctx)) {
    if (int rc = stage_begin(ctx, kStageEdgeReduce)) return rc;
    if (int rc = coll_begin(ctx)) return rc;
    // hist | err | sum are contiguous u64: one sum all-reduce.
    if (int rc = coll_allreduce(ctx, base, (size_t)E * kBins + 2ull * E, kCollU64, kCollSum))
      return rc;
    if (int rc = coll_allreduce(ctx, tab.mn, E, kCollU32, kCollMin)) return rc;
    if (int rc = coll_allreduce(ctx, tab.mx, E, kCollU32, kCollMax)) return rc;
    if (int rc = coll_end(ctx)) return rc;
    if (int rc = stage_end(ctx, kStageEdgeReduce)) return rc;
  }

  if (int rc = stage_begin(ctx, kStageEdgeFinal)) return rc;
  hipLaunchKernelGGL(edge_finalize_kernel, dim3(E), dim3(kWave), 0, ctx->stream, tab, count, p50,
                     p99);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (int rc = stage_end(ctx, kStageEdgeFinal)) return rc;

  // The per-edge vectors come back in one D2H into pinned staging, then
  // fan out on the host; the histogram (when asked for) goes straight.
  const size_t small = L.end_small - L.off_err;
  ANOMOD_HIP(ctx, hipMemcpyAsync(ctx->h_stage, base + L.off_err, small, hipMemcpyDeviceToHost,
                                 ctx->stream));
  if (out->hist)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->hist, tab.hist, (size_t)E * kBins * 8ull,
                                   hipMemcpyDeviceToHost, ctx->stream));
  if (int rc = stream_wait(ctx)) return rc;
  const char* hs = static_cast<const char*>(ctx->h_stage);
  auto fan = [&](void* dst, size_t off, size_t bytes) {  // off: device layout offset
    if (dst) memcpy(dst, hs + (off - L.off_err), bytes);
  };
  fan(out->count, L.off_count, E * 8ull);
  fan(out->errors, L.off_err, E * 8ull);
  fan(out->sum_us, L.off_sum, E * 8ull);
  fan(out->min_us, L.off_mn, E * 4ull);
  fan(out->max_us, L.off_mx, E * 4ull);
  fan(out->p50_us, L.off_p50, E * 8ull);
  fan(out->p99_us, L.off_p99, E * 8ull);
  memcpy(ovf, hs + (L.off_ovf - L.off_err), 16);
  return ANOMOD_OK;
}

}  // namespace

int edge_aggregate_records(anomod_ctx* ctx, const uint64_t* rec, uint64_t n, uint32_t S,
                           int8_t* hist_form, anomod_edge_table* out) {
  int local = ANOMOD_OK;
  ANOMOD_CHECK_LOCAL(ctx, local, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_CHECK_LOCAL(ctx, local, out->n_services == S, "out->n_services=%u != n_services=%u",
                     out->n_services, S);
  ANOMOD_CHECK_LOCAL(ctx, local, out->n_bins == kBins, "out->n_bins=%u != ANOMOD_HIST_BINS=%u",
                     out->n_bins, kBins);
  ANOMOD_CHECK_LOCAL(ctx, local, n < max_launch_spans(),
                     "%llu edge records: at most 2^32 - 2 per call", (unsigned long long)n);
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  const Layout L(E, 0);
  if (local == ANOMOD_OK) local = bind(ctx);
  if (local == ANOMOD_OK) local = ensure_table(ctx, L.bytes);
  if (local == ANOMOD_OK) local = ensure_host_stage(ctx, L.end_small - L.off_err);
  if (int rc = comm_agree(ctx, local)) return rc;
  const Table tab = table_at(ctx, L, E);
  if (int rc = table_clear(ctx, L, tab, E)) return rc;
  // the pair form for a set known to fit it, else the compact form (no probe
  // chain: nothing to saturate), which measures whether the pair form would do
  int form = *hist_form;
  if (const char* f = getenv("ANOMOD_HIST_FORM")) form = !strcmp(f, "pair") ? 0 : 1;
  const uint64_t keys = (uint64_t)E * kBins + 1;
  const bool lds_hist = keys < (1ull << 31);
  KernelFn1 fn = nullptr;
  int ht = kHtCompact;
#define ANOMOD_REC(H, S_) fn = edge_rec_kernel<H, S_>, ht = H
  if (!lds_hist) ANOMOD_REC(kHtHbm, kStHbm);
  else if (E <= kLdsEdges && form == 0) ANOMOD_REC(kHtPair, kStDirect);
  else if (E <= kLdsEdges) ANOMOD_REC(kHtCompact, kStDirect);
  else if (E <= kWideEdges && form == 0) ANOMOD_REC(kHtPair, kStWide);
  else if (E <= kWideEdges) ANOMOD_REC(kHtCompact, kStWide);
  else ANOMOD_REC(kHtCompact, kStSlot);
#undef ANOMOD_REC
  if (int rc = stage_begin(ctx, kStageEdgeAgg)) return rc;
  if (n > 0) {
    int per_cu = 0;
    ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                        &per_cu, reinterpret_cast<const void*>(fn), kThreads, 0));
    const uint64_t want = (n + (uint64_t)kThreads * kRecLoad - 1) / ((uint64_t)kThreads * kRecLoad);
    const uint64_t grid = std::min<uint64_t>((uint64_t)ctx->num_cus * (per_cu > 0 ? per_cu : 1), want);
    Table tr = tab;
    tr.occupancy = ht == kHtCompact;
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, rec, n, E, tr);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  if (int rc = stage_end(ctx, kStageEdgeAgg)) return rc;
  unsigned long long ovf[2] = {0ull, 0ull};
  if (int rc = table_finish(ctx, L, tab, E, out, ovf)) return rc;
  // what was learned: a compact run whose fullest workgroup used at most half
  // the pair table's slots says pair; a pair run that overflowed, compact
  if (n > 0 && lds_hist) {
    if (ht == kHtCompact && *hist_form < 0) *hist_form = ovf[1] <= kPairSlots / 2 ? 0 : 1;
    if (ht == kHtPair && ovf[0] * 64ull > n) *hist_form = 1;
  }
  return ANOMOD_OK;
}

bool span_rows_ready(const anomod_spans* s) { return rows_ready(s); }

int span_scan_choice(anomod_ctx* ctx, const anomod_spans* s, unsigned long long* d_cnt,
                     bool* unique) {
  if (int rc = probe_order(ctx, s, d_cnt)) return rc;
  *unique = use_unique(s);
  return ANOMOD_OK;
}

// ws words: [0] dynamic-tail counter, [1..3] long-trace counters, [4..5] order
// probe, [32..] long-trace list.
size_t span_edge_keys_ws_bytes(const anomod_spans* s) { return 256 + big_capacity(s) * 8; }

int span_edge_keys(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S,
                   unsigned long long* keys, unsigned long long* ws, bool use_rows) {
  if (!spans->n_spans || !spans->n_traces) return ANOMOD_OK;
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  Table tab{};
  tab.keys = keys;
  // a set with its parent rows: the keys from the row stream, no walk
  if (use_rows && rows_ready(spans)) {
    if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests)
      fprintf(stderr, "anomod: edge key kernel edge_row_kernel<keys>\n");
    return launch_rows(ctx, spans, edge_row_kernel<kHtKeys, kStHbm>, S, E, tab);
  }
  tab.ctr = ws;
  tab.big = ws + 1;
  tab.big_list = ws + 32;
  if (int rc = probe_order(ctx, spans, ws + 4)) return rc;
  KernelFn fn = use_unique(spans) ? edge_agg_kernel<kHtKeys, kStHbm, true>
                                  : edge_agg_kernel<kHtKeys, kStHbm, false>;
  int per_cu = 0;
  ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void*>(fn), kThreads, 0));
  const uint64_t grid = (uint64_t)ctx->num_cus * (uint64_t)(per_cu > 0 ? per_cu : 1);
  std::vector<uint64_t> cuts;
  if (int rc = span_launch_cuts(ctx, spans, max_launch_spans(), cuts)) return rc;
  ANOMOD_HIP(ctx, hipMemsetAsync(ws, 0, 32, ctx->stream));  // ctr + big counters
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {
    if (k > 0) ANOMOD_HIP(ctx, hipMemsetAsync(ws, 0, 8, ctx->stream));
    Table tk = tab;
    tk.t_base = cuts[k];
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream, spans->span_id,
                       spans->parent_span_id, spans->svc_flags, spans->dur_us,
                       spans->trace_ptr + cuts[k], cuts[k + 1] - cuts[k], S, E, tk);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  if (big_capacity(spans)) ANOMOD_HIP(ctx, (launch_big<kHtKeys, kStHbm>(ctx, spans, S, E, tab)));
  return ANOMOD_OK;
}

}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_edge_aggregate_spans(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S,
                                anomod_edge_table* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_edge_aggregate_spans: NULL argument");
  // Every check that can fail on one rank only (a shard's data, memory)
  // feeds the status agreement instead of returning early: with a
  // communicator attached the other ranks would otherwise wait in the
  // all-reduce below forever.
  int local = ANOMOD_OK;
  ANOMOD_CHECK_LOCAL(ctx, local, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_CHECK_LOCAL(ctx, local, out->n_services == S, "out->n_services=%u != n_services=%u",
                     out->n_services, S);
  ANOMOD_CHECK_LOCAL(ctx, local, out->n_bins == kBins, "out->n_bins=%u != ANOMOD_HIST_BINS=%u",
                     out->n_bins, kBins);
  ANOMOD_CHECK_LOCAL(ctx, local, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_CHECK_LOCAL(ctx, local, spans->grouped, "span set is not grouped by trace: "
                     "anomod_spans_group first (or anomod_edge_aggregate_ungrouped)");
  ANOMOD_CHECK_LOCAL(ctx, local, spans->n_spans == 0 || spans->max_svc < S,
                     "span service index %u >= n_services %u", spans->max_svc, S);
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  const uint64_t big_cap = big_capacity(spans);
  // Histogram form: a set known to fit the pair table takes it, a set that
  // overflowed it the compact form.  A set not aggregated before (form -1)
  // is probed: its first ~2^19 spans (kFormProbeSpans) run in the compact
  // form — no probe chain, nothing to saturate — on 16 workgroups (each then
  // sees ~32 k spans, near a full-size workgroup's key diversity) that
  // report their largest slot occupancy; at most half the pair table's
  // slots says pair.  The rest of the set runs in that form as an ordinary
  // launch: the probe's counts are part of the table.  A set of at most
  // 4 x 2^19 spans runs whole in the compact form and learns the same way.
  // The order probe of a unique-id set (probe_order_launch) runs beside it:
  // one host wait for both.  (r04 started form-unknown sets in a pair form
  // that stopped saturated workgroups and resumed them compact: its loop
  // spilled 16 / 48 B per lane, so a first call cost 12 % / 40 % more than
  // the pair form on SN / in-trace-shuffled SN; ANOMOD_HIST_FORM=auto keeps
  // it for tests.)
  int form = hist_form_of(spans);
  bool uni = use_unique(spans);  // (re-decided after an order probe)
  const bool pair_ok = pick_kernel(E, false, uni).ht == kHtPair;
  const bool autof = form < 0 && pair_ok && auto_forced();
  // (a set with traces longer than a chunk: LONG-like, the wide parent scan)
  const bool long_set = spans->max_trace_len != ~0ull && spans->max_trace_len > (uint64_t)kBigMin;
  // A unique-id collector-order set with long traces takes the wide parent
  // scan, which only the compact form has: nothing to probe for (r06: its
  // first call paid ~0.9 ms for a 16-workgroup probe over 2^19 LONG spans
  // whose answer was compact anyway, 1.16-1.20 x the warm call).
  if (form < 0 && pair_ok && !autof && long_set && uni) {
    form = 1;
    spans->hist_form = 1;
  }
  if (local == ANOMOD_OK) local = bind(ctx);
  // Parent rows.  The first-match parent of a span depends only on the set's
  // id columns and trace_ptr, which a resident set never changes: the first
  // aggregation of a set that outlives the call (`build`) walks the traces
  // once, in the ROWS instantiation that also stores every span's parent row
  // into the set's column (the long-trace pass writes its rows there too),
  // and every later one (`stream`) reads svc_flags, dur_us and the rows, 10
  // instead of 24 B/span (edge_row_kernel).  The walk is then never run again
  // for the set, so a form-unknown set is not probed: it runs whole in the
  // compact form with the occupancy report and learns its form from that
  // (`learn`), as sets of <= 4 x 2^19 spans always did.  When the column
  // cannot be allocated the call runs as before and the set stays without.
  const bool rows_ok = local == ANOMOD_OK && rows_allowed(spans) && spans->n_traces > 0;
  const bool stream = rows_ok && spans->parent_row && spans->rows_done;
  bool build = rows_ok && !stream;
  if (build && !spans->parent_row) {
    void* p = nullptr;
    if (dev_malloc(ctx, &p, spans->n_spans * 2) == hipSuccess) {
      spans->parent_row = static_cast<uint16_t*>(p);
    } else {
      (void)hipGetLastError();
      build = false;
    }
  }
  // Dense stream (edge_dense_kernel).  Whatever call learned a layout for
  // this S (`build`, or a row stream under another layout's S) is followed by
  // kDenseAfterStreams plain row streams, then by one that also writes the
  // span-word column (`dense_enc`), and from then on the set's aggregations at
  // this S read that column only (`dense_run`).  A call with another
  // S goes back to the row stream and learns that S's layout.
  const bool dense_try = rows_ok && dense_allowed();
  DenseSet* ds = spans->dense.get();
  const bool dense_run = stream && dense_try && ds && ds->state == DenseSet::kCoded && ds->S == S;
  const bool dense_wait = stream && dense_try && ds && ds->state == DenseSet::kLearned && ds->S == S;
  bool dense_enc = dense_wait && ds->streams >= kDenseAfterStreams;
  const bool learn = (build || stream) && !dense_run && form < 0 && pair_ok;
  const bool probe = form < 0 && pair_ok && !autof && spans->n_traces > 0 && !learn;
  // the probe's compact form (the forward scan when the order is still unknown)
  const Pick pc = pick_kernel(E, true, uni, kModeNormal, long_set);
  Pick pk = pick_kernel(E, form == 1 || learn, uni, autof ? kModeAuto : kModeNormal, long_set,
                        build);
  const Pick pr = autof ? pick_kernel(E, true, uni, kModeResume) : pk;  // the resume launch's form
  const RowPick rp = pick_row_kernel(E, form == 1 || learn);
  // As many workgroups as are resident at once (LDS / registers decide).
  int per_cu = 0, per_cu_r = 0;
  if (local == ANOMOD_OK &&
      (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(pk.fn),
                                                    kThreads, 0) != hipSuccess ||
       hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_r, reinterpret_cast<const void*>(pr.fn),
                                                    kThreads, 0) != hipSuccess)) {
    set_error(ctx, "occupancy query of %s failed", pk.name);
    local = ANOMOD_EHIP;
  }
  const uint64_t grid = (uint64_t)ctx->num_cus * (uint64_t)(per_cu > 0 ? per_cu : 1);
  const uint64_t grid_r = (uint64_t)ctx->num_cus * (uint64_t)(per_cu_r > 0 ? per_cu_r : 1);
  // (the long-trace pass writes its rows into the set's column when that is
  // being filled, and a stream call lists nothing)
  const Layout L(E, stream ? 0 : big_cap, build ? 0 : spans->n_spans,
                 autof ? grid * kWavesPerWG : 0);
  // (+ 16: the span range of a filled column)
  const size_t small = (L.end_small - L.off_err + 7) & ~size_t(7);
  if (local == ANOMOD_OK) local = ensure_table(ctx, L.bytes);
  if (local == ANOMOD_OK) local = ensure_host_stage(ctx, small + 32);  // + the encoder's flag and count
  if (int rc = comm_agree(ctx, local)) return rc;
  Table tab = table_at(ctx, L, E);
  if (build) tab.bpar = spans->parent_row;
  if (int rc = table_clear(ctx, L, tab, E)) return rc;

  // A first aggregation's probes (order, histogram form) run back to back
  // and are read back with one host wait.
  const bool oprobe = spans->n_traces > 0 && need_order_probe(spans) && !stream;
  auto* hst = static_cast<unsigned long long*>(ctx->h_stage);  // [0..1] order, [2] occupancy
  if (oprobe)  // scratch: the big counters' 4th and 5th words
    if (int rc = probe_order_launch(ctx, spans, tab.big + 3, hst)) return rc;
  if (!probe && oprobe) {
    ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    probe_order_take(spans, hst);
    uni = use_unique(spans);
    pk = pick_kernel(E, form == 1 || learn, uni, autof ? kModeAuto : kModeNormal, long_set, build);
  }
  auto* h_range = reinterpret_cast<uint64_t*>(static_cast<char*>(ctx->h_stage) + small);
  if (build) {  // the spans the traces cover: what the later calls stream
    ANOMOD_HIP(ctx, hipMemcpyAsync(h_range, spans->trace_ptr, 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
    ANOMOD_HIP(ctx, hipMemcpyAsync(h_range + 1, spans->trace_ptr + spans->n_traces, 8,
                                   hipMemcpyDeviceToHost, ctx->stream));
  }
  if (int rc = stage_begin(ctx, kStageEdgeAgg)) return rc;
  auto* h_bad = reinterpret_cast<uint32_t*>(h_range + 2);
  if (dense_run) {
    if (log_kernel())  // (tests)
      fprintf(stderr, "anomod: edge aggregation kernel edge_row_kernel<dense_hist,code_stats>\n");
    if (int rc = launch_dense(ctx, spans, tab)) return rc;
  } else if (stream) {
    if (dense_enc && !dense_alloc(ctx, spans)) {  // no memory: this S stays on the row stream
      dense_enc = false;
      ds->state = DenseSet::kNone;
    }
    if (log_kernel())  // (tests)
      fprintf(stderr, "anomod: edge aggregation kernel %s%s\n", rp.name,
              dense_enc ? " + edge codes" : "");
    Table tr = tab;
    tr.occupancy = learn;
    if (int rc = launch_rows(ctx, spans, rp.fn, S, E, tr)) return rc;
    if (dense_enc)
      if (int rc = dense_encode(ctx, spans, S, h_bad)) return rc;
  } else if (spans->n_traces > 0) {
    // A workgroup's LDS counters (histogram slots, errors) are u32 and the
    // dynamic tail may hand one workgroup any share of a launch, so a launch
    // covers < 2^32 spans: larger sets run as several launches over whole
    // trace ranges (split on the device trace_ptr).
    std::vector<uint64_t> cuts;
    if (int rc = span_launch_cuts(ctx, spans, max_launch_spans(), cuts)) return rc;
    if (probe) {
      const bool whole = spans->n_spans <= 4 * kFormProbeSpans;
      uint64_t P = cuts[1];
      unsigned pgrid = (unsigned)grid;
      if (!whole) {
        const uint64_t want = (kFormProbeSpans * spans->n_traces + spans->n_spans - 1) / spans->n_spans;
        P = std::min<uint64_t>(std::max<uint64_t>(want, 1), cuts[1]);
        pgrid = (unsigned)std::min<uint64_t>(grid, kFormProbeGroups);
      }
      Table tp = tab;
      tp.t_base = 0;
      tp.occupancy = 1;
      hipLaunchKernelGGL(pc.fn, dim3(pgrid), dim3(kThreads), 0, ctx->stream, spans->span_id,
                         spans->parent_span_id, spans->svc_flags, spans->dur_us, spans->trace_ptr,
                         P, S, E, tp);
      ANOMOD_HIP(ctx, hipGetLastError());
      ANOMOD_HIP(ctx, hipMemcpyAsync(hst + 2, tab.ovf + 1, 8, hipMemcpyDeviceToHost,
                                     ctx->stream));
      ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (oprobe) {
        probe_order_take(spans, hst);
        uni = use_unique(spans);
      }
      form = hst[2] <= kPairSlots / 2 ? 0 : 1;
      spans->hist_form = (int8_t)form;
      pk = pick_kernel(E, form == 1, uni, kModeNormal, long_set);
      // the rest from P on (ovf[1] back to 0: after the run it counts
      // pair-table overflows again)
      ANOMOD_HIP(ctx, hipMemsetAsync(tab.ctr, 0, 8, ctx->stream));
      ANOMOD_HIP(ctx, hipMemsetAsync(tab.ovf + 1, 0, 8, ctx->stream));
      cuts[0] = P;
    }
    if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests)
      fprintf(stderr, "anomod: edge aggregation kernel %s%s\n", pk.name,
              build ? " + parent rows" : "");
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
      if (cuts[k] >= cuts[k + 1]) continue;
      if (k > 0) {
        ANOMOD_HIP(ctx, hipMemsetAsync(tab.ctr, 0, 8, ctx->stream));
        if (autof) ANOMOD_HIP(ctx, hipMemsetAsync(tab.nleft, 0, 16, ctx->stream));
      }
      Table tk = tab;
      tk.t_base = cuts[k];
      tk.mode = autof ? kModeAuto : kModeNormal;
      tk.occupancy = learn;
      hipLaunchKernelGGL(pk.fn, dim3((unsigned)grid), dim3(kThreads), 0, ctx->stream,
                         spans->span_id, spans->parent_span_id, spans->svc_flags, spans->dur_us,
                         spans->trace_ptr + cuts[k], cuts[k + 1] - cuts[k], S, E, tk);
      ANOMOD_HIP(ctx, hipGetLastError());
      if (autof) {  // returns at once when no workgroup stopped
        tk.mode = kModeResume;
        hipLaunchKernelGGL(pr.fn, dim3((unsigned)grid_r), dim3(kThreads), 0, ctx->stream,
                           spans->span_id, spans->parent_span_id, spans->svc_flags, spans->dur_us,
                           spans->trace_ptr + cuts[k], cuts[k + 1] - cuts[k], S, E, tk);
        ANOMOD_HIP(ctx, hipGetLastError());
      }
    }
    if (big_cap) {
      Table tb = tab;
      tb.occupancy = learn;
      ANOMOD_HIP(ctx, launch_big_for(ctx, spans, S, E, tb));
    }
  }
  if (int rc = stage_end(ctx, kStageEdgeAgg)) return rc;
  unsigned long long ovf[2] = {0ull, 0ull};
  if (int rc = table_finish(ctx, L, tab, E, out, ovf)) return rc;
  if (build) {  // every launch ran: the column is complete
    spans->rows_S = S;
    spans->rows_lo = h_range[0];
    spans->rows_hi = h_range[1];
    spans->rows_done = true;
  }
  // a compact-form run that reported its fullest workgroup's slots: at most
  // half the pair table's says pair
  if (learn) spans->hist_form = ovf[1] <= kPairSlots / 2 ? 0 : 1;
  if (dense_enc) {  // an edge without a code (never from this set's own table): row stream
    ds->state = *h_bad ? DenseSet::kNone : DenseSet::kCoded;
    // More than 1/256 of the positions wide (each costs the dense kernel a
    // 32-B sector of dur_us): the set gives up the packed form and this call
    // writes the column again, as 4-byte cell words, for the calls after it.
    const unsigned long long wide = *reinterpret_cast<const unsigned long long*>(h_bad + 2);
    const unsigned long long n_enc = spans->rows_hi - spans->rows_lo;
    if (ds->pack && ds->state == DenseSet::kCoded && wide * 256ull > n_enc) {
      if (log_kernel())  // (tests)
        fprintf(stderr, "anomod: edge dense pack S=%u dropped: %llu wide of %llu spans\n", S, wide,
                n_enc);
      ds->pack = false;
      ds->wgs_per_cu = 0;  // (another kernel from here on)
      ds->state = DenseSet::kNone;
      if (dense_alloc(ctx, spans)) {
        if (int rc = dense_encode(ctx, spans, S, h_bad)) return rc;
        if (int rc = stream_wait(ctx)) return rc;
        ds->state = *h_bad ? DenseSet::kNone : DenseSet::kCoded;
      }
    }
  } else if (dense_wait) {
    ++ds->streams;
  } else if ((build || stream) && dense_try && !dense_run && !(ds && ds->S == S)) {
    const char* hs = static_cast<const char*>(ctx->h_stage);
    dense_learn(spans, S, E,
                reinterpret_cast<const unsigned long long*>(hs + (L.off_count - L.off_err)),
                reinterpret_cast<const uint32_t*>(hs + (L.off_mn - L.off_err)),
                reinterpret_cast<const uint32_t*>(hs + (L.off_mx - L.off_err)));
  }
  const int ran_ht = dense_run ? -1 : stream ? rp.ht : pk.ht;
  // The set's form from here on: compact when a workgroup of a first
  // aggregation stopped at a saturated pair table, or when more than 1/64 of
  // the spans were counted in HBM past a full one (the set touches more (edge,
  // bin) keys than 8 Ki slots hold, e.g. random call trees over every service
  // pair); else pair.  Same results either way.
  if (ran_ht == kHtPair) {
    if (ovf[1] > 0 || ovf[0] * 64ull > spans->n_spans) spans->hist_form = 1;
    else if (spans->hist_form < 0) spans->hist_form = 0;
  }
  return ANOMOD_OK;
}

int anomod_edge_quantiles_exact(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S,
                                const uint32_t* q_pct, uint32_t nq, double* out,
                                uint64_t* count) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && q_pct && out,
                 "anomod_edge_quantiles_exact: NULL argument");
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_REQUIRE(ctx, nq >= 1 && nq <= 16, "nq=%u outside [1, 16]", nq);
  for (uint32_t k = 0; k < nq; ++k)
    ANOMOD_REQUIRE(ctx, q_pct[k] <= 99, "q_pct[%u]=%u outside [0, 99]", k, q_pct[k]);
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_REQUIRE(ctx, spans->grouped, "span set is not grouped by trace: anomod_spans_group first");
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "span service index %u >= n_services %u", spans->max_svc, S);
  // one radix sort over every span's key (u32 tile offsets inside)
  ANOMOD_REQUIRE(ctx, spans->n_spans <= kMaxSortKeys,
                 "exact edge quantiles: %llu spans, at most 2^32 - 4097 per call",
                 (unsigned long long)spans->n_spans);
  if (int rc = bind(ctx)) return rc;
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  const uint64_t n = spans->n_spans;
  int kbits = 1;
  while ((uint64_t)E >> kbits) ++kbits;
  // One workspace: keys | sorted keys | sort temp | q | out | count | the key
  // walk's words (span_edge_keys: counters | long-trace list)
  const size_t sort_tmp = n ? radix_temp_bytes(n) : 0;
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t b_keys = al(n * 8), b_tmp = al(sort_tmp), b_q = al(nq * 4), b_out = al(E * nq * 8ull),
               b_cnt = al(E * 8ull);
  // (the ctx's scratch slot: reused by the next call instead of freed)
  char* w = nullptr;
  if (int rc = ensure_scratch(ctx, kScratchQuantiles,
                              2 * b_keys + b_tmp + b_q + b_out + b_cnt +
                                  span_edge_keys_ws_bytes(spans),
                              reinterpret_cast<void**>(&w)))
    return rc;
  auto* keys = reinterpret_cast<unsigned long long*>(w);
  auto* sorted = reinterpret_cast<unsigned long long*>(w + b_keys);
  void* tmp = w + 2 * b_keys;
  auto* d_q = reinterpret_cast<uint32_t*>(w + 2 * b_keys + b_tmp);
  auto* d_out = reinterpret_cast<double*>(w + 2 * b_keys + b_tmp + b_q);
  auto* d_cnt = reinterpret_cast<unsigned long long*>(w + 2 * b_keys + b_tmp + b_q + b_out);
  auto* d_ctr = reinterpret_cast<unsigned long long*>(w + 2 * b_keys + b_tmp + b_q + b_out + b_cnt);
  int rc = ANOMOD_OK;
  hipError_t e = hipMemcpyAsync(d_q, q_pct, nq * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && n && spans->n_traces) {
    // per-span (edge, latency) keys from the aggregation kernel's own walk and
    // parent rule, then one radix sort over edge|dur
    rc = span_edge_keys(ctx, spans, S, keys, d_ctr, true);
    int passes = 0;
    if (rc == ANOMOD_OK)
      e = radix_sort_u64(reinterpret_cast<const uint64_t*>(keys),
                         reinterpret_cast<uint64_t*>(sorted), n, 0, 32 + kbits, tmp, sort_tmp,
                         ctx->stream, &passes);
    if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests, timing)
      fprintf(stderr, "anomod: exact edge quantiles: %llu keys of %d bits, %d sort passes\n",
              (unsigned long long)n, 32 + kbits, passes);
  }
  if (e == hipSuccess && rc == ANOMOD_OK) {
    hipLaunchKernelGGL(exact_pick_kernel, dim3((E + 255) / 256), dim3(256), 0, ctx->stream,
                       sorted, spans->n_traces ? n : 0, E, d_q, nq, d_out, d_cnt);
    e = hipGetLastError();
  }
  if (e == hipSuccess && rc == ANOMOD_OK)
    e = hipMemcpyAsync(out, d_out, E * nq * 8ull, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && rc == ANOMOD_OK && count)
    e = hipMemcpyAsync(count, d_cnt, E * 8ull, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (rc != ANOMOD_OK) return rc;
  if (e != hipSuccess) {
    set_error(ctx, "exact edge quantiles failed: %s", hipGetErrorString(e));
    return ANOMOD_EHIP;
  }
  return ANOMOD_OK;
}

int anomod_edge_aggregate(anomod_ctx* ctx, const anomod_span_soa* soa, uint64_t n_spans,
                          const uint64_t* trace_ptr, uint64_t n_traces, anomod_edge_table* out) {
  ANOMOD_REQUIRE(nullptr, ctx && soa && out, "anomod_edge_aggregate: NULL argument");
  anomod_spans* s = nullptr;
  if (int rc = anomod_spans_upload(ctx, soa, n_spans, trace_ptr, n_traces, &s)) return rc;
  s->keep_rows = false;  // freed below: parent rows would never be read again
  const int rc = anomod_edge_aggregate_spans(ctx, s, out->n_services, out);
  anomod_spans_free(s);
  return rc;
}

int anomod_spans_parent_rows(anomod_ctx* ctx, const anomod_spans* spans, uint16_t* out_host,
                             uint32_t S) {
  ANOMOD_REQUIRE(nullptr, ctx && spans, "anomod_spans_parent_rows: NULL argument");
  ANOMOD_REQUIRE(ctx, out_host || spans->n_spans == 0, "anomod_spans_parent_rows: NULL destination");
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  if (!spans->parent_row || !spans->rows_done) {
    set_error(ctx, "span set holds no parent rows (no grouped aggregation filled them yet)");
    return ANOMOD_ESTATE;
  }
  ANOMOD_REQUIRE(ctx, spans->max_svc < S, "span service index %u >= n_services %u",
                 spans->max_svc, S);
  if (int rc = bind(ctx)) return rc;
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i < spans->n_spans; ++i) out_host[i] = 0xFFFFu;
  const uint64_t lo = spans->rows_lo, n = spans->rows_hi - lo;
  if (n) ANOMOD_HIP(ctx, hipMemcpy(out_host + lo, spans->parent_row + lo, n * 2, hipMemcpyDeviceToHost));
  for (uint64_t i = lo; i < lo + n; ++i)
    if (out_host[i] >= spans->rows_S) out_host[i] = (uint16_t)(out_host[i] - spans->rows_S + S);
  return ANOMOD_OK;
}

}  // extern "C"
