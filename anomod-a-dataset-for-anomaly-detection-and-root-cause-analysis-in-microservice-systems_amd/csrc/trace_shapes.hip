// Trace shape census of a grouped span set: a structural fingerprint per
// trace, the distinct fingerprints of the set and how many traces have each.
//
//   par(i)  = self time's parent (self_time.hip): the first span of i's trace,
//             in position order, whose span_id equals i's parent_span_id.  A
//             span without one is a head, of kind ROOT (reference 0), ORPHAN
//             (the reference names no span of the trace) or SELF (the first
//             match is i itself).
//   K(i)    = svc_key[svc(i)] ^ (use_errors && error flag ? kErrKey : 0)
//   P(i)    = seed(kind) * B + K(i) for a head, P(par(i)) * B + K(i) otherwise
//             (mod 2^64); a span whose parent chain never reaches a head (a
//             reference cycle, or a span hanging off one) is off the tree:
//             path_hash 0, in no shape, counted in off_tree_spans
//   shape[t] = sum of mix64(P(i)) over the on-tree spans of trace t (mod 2^64)
//   census  = the distinct shape[t], by count descending then value ascending,
//             each with its count, its traces of class != 0 and its smallest
//             trace index
//
// The recurrence is an affine map, so it composes: every span holds (anc, H,
// Mul) with P(i) = P(anc) * Mul + H — a non-head starts at (par, K, B), a head
// is done with H = P — and a pointer-jumping round replaces the span's state by
// its composition with its ancestor's (the ancestor's state of before the
// round).  ceil(log2 L) rounds finish every on-tree span of a trace of L
// spans; what is not done after them is off the tree.
//
// One chunk walk (walk.h: persistent waves, <= 256 spans / <= 64 whole traces
// per chunk, buffer loads, the columns of chunk c+1 in flight while chunk c is
// resolved) finds the parent positions in the
// wave's LDS, runs at most 8 rounds there and adds every on-tree span's
// mix64(P) to its trace's u64 LDS slot.  Traces longer than a chunk are listed
// by the walk and resolved by trace_shapes_big_kernel, one workgroup per listed
// trace, with the jump state double-buffered in global scratch.  The census is
// taken on the device: radix sort of the shapes, run boundaries compacted to
// (value, start) pairs, radix sort of (~count) << 32 | run index, and one pass
// over the traces for first_trace and abnormal.  Every value is a wrapping
// 64-bit integer: results are bit-exact for any launch geometry.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "group.h"
#include "radix.h"
#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kShWaves = 4;
constexpr int kShThreads = kShWaves * kWave;

constexpr uint64_t kB = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kSeedRoot = 0x243F6A8885A308D3ull;
constexpr uint64_t kSeedOrphan = 0x13198A2E03707344ull;
constexpr uint64_t kSeedSelf = 0xA4093822299F31D0ull;
constexpr uint64_t kErrKey = 0xD1B54A32D192ED03ull;

// Per-wave LDS (every offset a multiple of 16).  The ids are dead once the
// parents are found: their array then holds the H words of the jump state.
constexpr int kHSid = 0;  // u64 ids [kStage + kScanSlack] (or two u32 planes) | u64 H [kStage]
constexpr int kHMul = kHSid + (kStage + (int)kScanSlack) * 8;  // u64 Mul [kStage]
constexpr int kHAnc = kHMul + kStage * 8;    // u32 ancestor words [kStage]
constexpr int kHSlot = kHAnc + kStage * 4;   // u64 trace sums [kWave]
constexpr int kHFlag = kHSlot + kWave * 8;   // u8 trace-start flags [kStage]
constexpr int kHBytes = kHFlag + kStage;
static_assert(kHBytes % 16 == 0, "wave staging must stay 16-B aligned");

// chunk ancestor word: ancestor position, or kDone (P(i) = H)
constexpr uint32_t kPosMask = 0xFFFFu, kDone = 1u << 17;
// long-trace ancestor word: position in the trace, or kDoneBig
constexpr uint32_t kDoneBig = 0xFFFFFFFFu;

struct ShArgs {
  const unsigned long long* svc_key;  // [S]
  unsigned long long* shape;          // [n_traces]
  unsigned long long* path_hash;      // [n_spans] or NULL
  unsigned long long* ctr;            // trace-segment counter of the dynamic tail
  unsigned long long* big;            // [0] listed traces, [1] their spans, [2] ticket
  unsigned long long* off_tree;       // spans off the tree
  unsigned long long* big_list;       // (trace, scratch offset) per listed trace
  uint64_t big_cap;                   // entries big_list holds
  // jump state of the listed traces, two buffers of [counted long spans] each
  unsigned long long* l_h[2];
  unsigned long long* l_m[2];
  uint32_t* l_w[2];
  uint32_t use_errors;
};

struct Regs {
  uint64_t sid[kPer], pid[kPer];
  uint32_t sf[kPer];  // svc | flags << 16
};

__device__ __forceinline__ void load_regs(const uint64_t* __restrict__ span_id,
                                          const uint64_t* __restrict__ parent,
                                          const uint32_t* __restrict__ svcfl, const Chunk& c,
                                          int lane, Regs& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by trace_shapes_big_kernel
  const auto rsid = rsrc(span_id + c.base, n * 8u);
  const auto rpid = rsrc(parent + c.base, n * 8u);
  const auto rsf = rsrc(svcfl + c.base, n * 4u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.sid[r] = bload64(rsid, i * 8u);
    R.pid[r] = bload64(rpid, i * 8u);
    R.sf[r] = bload32(rsf, i * 4u);
  }
}

__device__ __forceinline__ uint64_t label_key(const ShArgs& a, uint32_t sf) {
  const uint64_t k = a.svc_key[sf & 0xFFFFu];
  return k ^ ((a.use_errors && ((sf >> 16) & ANOMOD_FLAG_ERROR)) ? kErrKey : 0ull);
}

// `end`: this lane's trace end relative to c.base (lanes < c.k); t0: the
// chunk's first trace; off: the wave's count of off-tree spans (per lane).
template <int SCAN>
__device__ __forceinline__ void shapes_chunk(unsigned char* wsm, int lane, const Chunk& c,
                                             uint32_t end, uint64_t t0, const Regs& R,
                                             const ShArgs& a, uint32_t& off) {
  auto* lsid = reinterpret_cast<uint64_t*>(wsm + kHSid);
  auto* llo = reinterpret_cast<uint32_t*>(wsm + kHSid);
  uint32_t* lhi = llo + (kStage + kScanSlack);
  auto* lH = reinterpret_cast<uint64_t*>(wsm + kHSid);  // after the parent phase
  auto* lM = reinterpret_cast<uint64_t*>(wsm + kHMul);
  auto* lw = reinterpret_cast<uint32_t*>(wsm + kHAnc);
  auto* lslot = reinterpret_cast<unsigned long long*>(wsm + kHSlot);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kHFlag);
  // Stage the ids (lanes past n hold zeros from the buffer loads), start the
  // label-key gathers and mark trace starts.
  uint64_t K[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if constexpr (SCAN == kScanSplit) {
      llo[i] = (uint32_t)R.sid[r];
      lhi[i] = (uint32_t)(R.sid[r] >> 32);
    } else {
      lsid[i] = R.sid[r];
    }
    K[r] = i < c.n ? label_key(a, R.sf[r]) : 0ull;
  }
  lslot[lane] = 0ull;
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);
  // Parent position, or the head's seed.
  uint32_t w[kPer];
  uint64_t H[kPer], M[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    uint64_t seed = kSeedRoot;
    int q = -1;
    if (i < c.n && R.pid[r] != 0ull) {
      seed = kSeedOrphan;  // unless found in the trace
      uint32_t ta, tb;
      trace_bounds(Sm, r, lane, c.n, ta, tb);
      q = find_parent<SCAN>(lsid, llo, lhi, ta, tb, i, R.pid[r]);
      if ((uint32_t)q == i) seed = kSeedSelf;
    }
    const bool has = q >= 0 && (uint32_t)q != i;
    M[r] = kB;
    if (i >= c.n) {  // not a span: done, in no shape
      w[r] = i | kDone;
      H[r] = 0ull;
    } else if (has) {
      w[r] = (uint32_t)q;
      H[r] = K[r];
    } else {
      w[r] = i | kDone;
      H[r] = seed * kB + K[r];
    }
  }
  wave_sync();  // the ids are dead: their array holds H from here on
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    lH[i] = H[r];
    lM[i] = M[r];
    lw[i] = w[r];
  }
  wave_sync();
  // Pointer jumping: 2^8 hops cover a chunk.  Read all, sync, write all.
  for (int round = 0; round < 8; ++round) {
    bool open = false;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      if (!(w[r] & kDone)) {
        const uint32_t p = w[r] & kPosMask;
        const uint64_t Ha = lH[p], Ma = lM[p];
        const uint32_t wa = lw[p];
        H[r] = Ha * M[r] + H[r];
        if (!(wa & kDone)) M[r] = Ma * M[r];
        w[r] = wa;
        open = true;
      }
    }
    if (!__ballot(open)) break;
    wave_sync();
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const uint32_t i = lane + r * kWave;
      lH[i] = H[r];
      lM[i] = M[r];
      lw[i] = w[r];
    }
    wave_sync();
  }
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    if (i >= c.n) continue;
    const bool on = (w[r] & kDone) != 0u;
    const uint64_t P = on ? H[r] : 0ull;
    if (on)
      atomicAdd(&lslot[trace_in_chunk(Sm, r, lane) & (kWave - 1u)], (unsigned long long)mix64(P));
    else
      off += 1u;
    if (a.path_hash) a.path_hash[c.base + i] = P;
  }
  wave_sync();
  // the traces of the chunk: lane l holds trace t0 + l (an empty trace owns no
  // slot: its shape is 0)
  if ((uint32_t)lane < c.k)
    a.shape[t0 + (uint64_t)lane] =
        c.start < end ? lslot[rank_at(Sm, c.start) & (kWave - 1u)] : 0ull;
  wave_sync();  // the staging area is free for the next chunk
}

template <int SCAN>
__global__ __launch_bounds__(kShThreads, 3) void trace_shapes_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint64_t* __restrict__ trace_ptr, uint64_t n_traces,
    ShArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kHBytes * kShWaves];
  const int lane = threadIdx.x & (kWave - 1);
  unsigned char* wsm = smem + (threadIdx.x / kWave) * kHBytes;
  uint32_t off = 0;
  walk_traces<kShWaves, 4, Regs>(
      trace_ptr, n_traces, a.ctr,
      [&](const Chunk& c, Regs& R) __attribute__((always_inline)) {
        load_regs(span_id, parent, svcfl, c, lane, R);
      },
      [&](const Chunk& c, uint32_t end, uint64_t t0, const Regs& R)
          __attribute__((always_inline)) { shapes_chunk<SCAN>(wsm, lane, c, end, t0, R, a, off); },
      // longer than kStage: listed for trace_shapes_big_kernel
      [&](uint64_t t, uint32_t n) __attribute__((always_inline)) {
        list_long(a.big, a.big_list, a.big_cap, lane, t, n);
      });
  for (int o = 32; o > 0; o >>= 1) off += (uint32_t)__shfl_xor((int)off, o);
  if (lane == 0 && off) atomicAdd(a.off_tree, (unsigned long long)off);
}

// ---- long traces ----------------------------------------------------------
// One workgroup per listed trace (tickets).  Parent positions come from
// walk.h's windowed LDS id table (big_parents).  The
// jump state (H, Mul, ancestor word) lives in global scratch in two buffers:
// a round reads one and writes the other.  A span's words are written by the
// thread that owns the span (position % kBigThreads) with agent-scope stores
// and read by any thread with agent-scope loads, all served by L2; every wave
// waits for its own stores before the barrier that separates two rounds
// (sweep_sync).  ceil(log2 L) rounds, fewer when a round finds no open span;
// then the trace sum by a workgroup reduction.
__global__ __launch_bounds__(kBigThreads) void trace_shapes_big_kernel(
    const uint64_t* __restrict__ span_id, const uint64_t* __restrict__ parent,
    const uint32_t* __restrict__ svcfl, const uint64_t* __restrict__ trace_ptr, ShArgs a) {
  __shared__ unsigned long long bkey[kBigSlots];
  __shared__ uint32_t bpos[kBigSlots];
  __shared__ unsigned long long s_j;
  __shared__ unsigned long long s_sum[kBigThreads / kWave];
  __shared__ unsigned long long s_off[kBigThreads / kWave];
  const int tid = threadIdx.x;
  const uint64_t nbig = a.big[0] < a.big_cap ? a.big[0] : a.big_cap;
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
    unsigned long long* hA = a.l_h[0] + off;
    unsigned long long* hB = a.l_h[1] + off;
    unsigned long long* mA = a.l_m[0] + off;
    unsigned long long* mB = a.l_m[1] + off;
    uint32_t* wA = a.l_w[0] + off;
    uint32_t* wB = a.l_w[1] + off;
    // ---- parent positions
    for (uint64_t b0 = 0; b0 < L; b0 += kBigThreads * kBigPer) {
      uint64_t pid[kBigPer];
      uint32_t pp[kBigPer];  // parent position in the trace (kNone: none)
      big_parents(span_id, parent, lo, L, b0, tid, bkey, bpos, pid, pp);
      // The span's starting state.
#pragma unroll
      for (int r = 0; r < kBigPer; ++r) {
        const uint64_t i = b0 + (uint64_t)r * kBigThreads + tid;
        if (i >= L) continue;
        const uint32_t q = pp[r];
        const uint64_t K = label_key(a, svcfl[lo + i]);
        const bool has = q != kNone && q != (uint32_t)i;
        const uint64_t seed = pid[r] == 0ull ? kSeedRoot : q == kNone ? kSeedOrphan : kSeedSelf;
        astore(&hA[i], (unsigned long long)(has ? K : seed * kB + K));
        astore(&mA[i], (unsigned long long)kB);
        astore(&wA[i], has ? q : kDoneBig);
      }
    }
    sweep_sync();
    // ---- pointer jumping between the two buffers
    for (uint64_t hops = 1; hops < L; hops <<= 1) {
      bool open = false;
      for (uint64_t i = tid; i < L; i += kBigThreads) {
        uint32_t w = aload(&wA[i]);
        unsigned long long H = aload(&hA[i]), M = aload(&mA[i]);
        if (w != kDoneBig) {
          const uint32_t wa = aload(&wA[w]);
          H = aload(&hA[w]) * M + H;
          if (wa != kDoneBig) M = aload(&mA[w]) * M;
          w = wa;
          open = true;
        }
        astore(&hB[i], H);
        astore(&mB[i], M);
        astore(&wB[i], w);
      }
      wait_stores();
      const bool any = __syncthreads_or(open);
      unsigned long long* xh = hA;
      hA = hB;
      hB = xh;
      unsigned long long* xm = mA;
      mA = mB;
      mB = xm;
      uint32_t* xw = wA;
      wA = wB;
      wB = xw;
      if (!any) break;
    }
    // ---- outputs
    unsigned long long sum = 0ull, noff = 0ull;
    for (uint64_t i = tid; i < L; i += kBigThreads) {
      const bool on = aload(&wA[i]) == kDoneBig;
      const unsigned long long P = on ? aload(&hA[i]) : 0ull;
      if (on)
        sum += mix64(P);
      else
        noff += 1ull;
      if (a.path_hash) a.path_hash[lo + i] = P;
    }
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o);
      noff += __shfl_xor(noff, o);
    }
    if ((tid & (kWave - 1)) == 0) {
      s_sum[tid / kWave] = sum;
      s_off[tid / kWave] = noff;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long s = 0ull, o = 0ull;
      for (int k = 0; k < kBigThreads / kWave; ++k) {
        s += s_sum[k];
        o += s_off[k];
      }
      a.shape[t] = s;
      if (o) atomicAdd(a.off_tree, o);
    }
  }
}

// ---- census -----------------------------------------------------------------
// Run boundaries of the sorted shapes, compacted to (value, start) pairs in
// select_f64_keys' form (radix.hip): per-tile counts, one block's exclusive
// scan of them, the write.
constexpr int kCTile = 4096;
constexpr int kCThreads = 256;
constexpr int kCRows = kCTile / kCThreads;
constexpr int kCW = kCThreads / kWave;

__device__ __forceinline__ bool run_start(const uint64_t* __restrict__ s, uint64_t n, uint64_t p) {
  return p < n && (p == 0 || s[p] != s[p - 1]);
}

__global__ __launch_bounds__(kCThreads) void run_count_kernel(const uint64_t* __restrict__ s,
                                                              uint64_t n,
                                                              uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t ws[kCW];
  const int tid = threadIdx.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * kCTile;
  uint32_t c = 0;
  for (int j = 0; j < kCRows; ++j)
    c += run_start(s, n, t0 + (uint64_t)(j * kCThreads + tid)) ? 1u : 0u;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((tid & 63) == 0) ws[tid / kWave] = c;
  __syncthreads();
  if (tid == 0) {
    uint32_t sum = 0;
    for (int i = 0; i < kCW; ++i) sum += ws[i];
    tcnt[blockIdx.x] = sum;
  }
}

// one block: exclusive scan of the tile counts (in place), total to *count
__global__ __launch_bounds__(1024) void run_scan_kernel(uint32_t* __restrict__ tcnt, uint64_t tiles,
                                                        unsigned long long* __restrict__ count) {
  __shared__ uint64_t wsum[16];
  __shared__ uint64_t carry;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint64_t b0 = 0; b0 < tiles; b0 += 1024) {
    const uint64_t t = b0 + tid;
    const uint64_t x = t < tiles ? tcnt[t] : 0u;
    uint64_t inc = x;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint64_t y = __shfl_up(inc, o);
      if (lane >= o) inc += y;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint64_t pre = carry;
    for (int ww = 0; ww < w; ++ww) pre += wsum[ww];
    if (t < tiles) tcnt[t] = (uint32_t)(pre + inc - x);
    __syncthreads();
    if (tid == 1023) carry = pre + inc;
    __syncthreads();
  }
  if (tid == 0) *count = carry;
}

__global__ __launch_bounds__(kCThreads) void run_write_kernel(const uint64_t* __restrict__ s,
                                                              uint64_t n,
                                                              const uint32_t* __restrict__ toff,
                                                              uint64_t* __restrict__ run_val,
                                                              uint32_t* __restrict__ run_pos) {
  __shared__ uint32_t ws[kCRows][kCW];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
  const uint64_t t0 = (uint64_t)blockIdx.x * kCTile;
  uint32_t below[kCRows];
#pragma unroll
  for (int j = 0; j < kCRows; ++j) {
    const bool keep = run_start(s, n, t0 + (uint64_t)(j * kCThreads + tid));
    const uint64_t b = __ballot(keep);
    below[j] = keep ? (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) : 0xFFFFFFFFu;
    if (lane == 0) ws[j][w] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  uint32_t run = toff[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kCRows; ++j) {
    uint32_t pre = run;
    for (int ww = 0; ww < w; ++ww) pre += ws[j][ww];
    for (int ww = 0; ww < kCW; ++ww) run += ws[j][ww];
    if (below[j] != 0xFFFFFFFFu) {
      const uint64_t p = t0 + (uint64_t)(j * kCThreads + tid);
      run_val[(uint64_t)pre + below[j]] = s[p];
      run_pos[(uint64_t)pre + below[j]] = (uint32_t)p;  // (n <= kMaxSortKeys < 2^32)
    }
  }
}

__device__ __forceinline__ uint32_t run_len(const uint32_t* __restrict__ run_pos, uint64_t R,
                                            uint64_t n, uint64_t r) {
  return (uint32_t)((r + 1 < R ? (uint64_t)run_pos[r + 1] : n) - (uint64_t)run_pos[r]);
}

// Rank keys: ascending order of (~count) << 32 | run index is count
// descending, then run index (= shape value) ascending.
__global__ __launch_bounds__(256) void rank_key_kernel(const uint32_t* __restrict__ run_pos,
                                                       uint64_t R, uint64_t n,
                                                       uint64_t* __restrict__ key) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < R) key[r] = ((uint64_t)(~run_len(run_pos, R, n, r)) << 32) | r;
}

// first_trace and abnormal per run from one pass over the traces: the run of
// shape[t] by binary search, lanes of equal run combined within the wave (the
// lowest lane holds the smallest trace), the waves' partial results combined
// in a workgroup LDS table keyed by run, and the table's entries sent to the
// global arrays when it runs full and at the end.
constexpr uint32_t kClsSlots = 1024;
constexpr uint32_t kClsFull = kClsSlots / 2;  // a tile adds <= 256 entries: load <= 3/4

__device__ __forceinline__ void cls_flush(uint32_t* tkey, uint32_t* tfirst, uint32_t* tabn,
                                          uint32_t* occ, unsigned long long* __restrict__ first,
                                          unsigned long long* __restrict__ abn) {
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kClsSlots; k += 256) {
    if (tkey[k]) {
      const uint32_t r = tkey[k] - 1u;
      atomicMin(&first[r], (unsigned long long)tfirst[k]);
      if (tabn[k]) atomicAdd(&abn[r], (unsigned long long)tabn[k]);
    }
    tkey[k] = 0u;
    tfirst[k] = 0xFFFFFFFFu;
    tabn[k] = 0u;
  }
  if (threadIdx.x == 0) *occ = 0u;
  __syncthreads();
}

__global__ __launch_bounds__(256) void shape_class_kernel(
    const uint64_t* __restrict__ shape, const uint8_t* __restrict__ cls, uint64_t n_traces,
    const uint64_t* __restrict__ run_val, uint64_t R, unsigned long long* __restrict__ first,
    unsigned long long* __restrict__ abn) {
  __shared__ uint32_t tkey[kClsSlots];  // run index + 1 (0: empty)
  __shared__ uint32_t tfirst[kClsSlots];
  __shared__ uint32_t tabn[kClsSlots];
  __shared__ uint32_t occ;
  const int lane = threadIdx.x & (kWave - 1);
  for (uint32_t k = threadIdx.x; k < kClsSlots; k += 256) {
    tkey[k] = 0u;
    tfirst[k] = 0xFFFFFFFFu;
    tabn[k] = 0u;
  }
  if (threadIdx.x == 0) occ = 0u;
  const uint64_t tiles = (n_traces + 255) / 256;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();
    const uint32_t filled = occ;  // every thread reads it before any insert of the tile
    __syncthreads();
    if (filled >= kClsFull) cls_flush(tkey, tfirst, tabn, &occ, first, abn);  // (block-uniform)
    const uint64_t t = tile * 256 + threadIdx.x;
    const bool valid = t < n_traces;
    uint32_t r = 0;
    bool bad = false;
    if (valid) {
      const uint64_t v = shape[t];
      uint64_t lo = 0, hi = R;  // the last run with run_val <= v (it equals v)
      while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (run_val[mid] <= v) lo = mid;
        else hi = mid;
      }
      r = (uint32_t)lo;
      bad = cls && cls[t] != 0;
    }
    uint64_t todo = __ballot(valid);
    while (todo) {
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const uint32_t rl = (uint32_t)__shfl((int)r, leader);
      const uint64_t same = __ballot(valid && r == rl);
      const uint32_t nab = (uint32_t)__popcll(__ballot(valid && r == rl && bad));
      if (lane == leader) {
        for (uint32_t sl = (rl * 0x9E3779B1u) >> 22;; sl = (sl + 1u) & (kClsSlots - 1u)) {
          const uint32_t prev = atomicCAS(&tkey[sl], 0u, rl + 1u);
          if (prev == 0u) atomicAdd(&occ, 1u);
          if (prev == 0u || prev == rl + 1u) {
            atomicMin(&tfirst[sl], (uint32_t)t);  // (n_traces < 2^32)
            if (nab) atomicAdd(&tabn[sl], nab);
            break;
          }
        }
      }
      todo &= ~same;
    }
  }
  cls_flush(tkey, tfirst, tabn, &occ, first, abn);
}

// The first m shapes in census order.
__global__ __launch_bounds__(256) void census_gather_kernel(
    const uint64_t* __restrict__ ranked, uint64_t m, const uint64_t* __restrict__ run_val,
    const uint32_t* __restrict__ run_pos, uint64_t R, uint64_t n,
    const unsigned long long* __restrict__ first, const unsigned long long* __restrict__ abn,
    uint64_t* __restrict__ o_shape, uint64_t* __restrict__ o_count, uint64_t* __restrict__ o_abn,
    uint64_t* __restrict__ o_first) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const uint64_t r = ranked[k] & 0xFFFFFFFFull;
  o_shape[k] = run_val[r];
  o_count[k] = run_len(run_pos, R, n, r);
  o_abn[k] = abn[r];
  o_first[k] = first[r];
}

using WalkFn = void (*)(const uint64_t*, const uint64_t*, const uint32_t*, const uint64_t*,
                        uint64_t, ShArgs);

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_trace_shapes_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_trace_shapes* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_trace_shapes_spans: NULL argument");
  const uint32_t S = out->n_services;
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "span service index %u >= n_services %u", spans->max_svc, S);
  ANOMOD_REQUIRE(ctx, spans->n_spans < max_launch_spans(), "%llu spans: at most 2^32 - 2 per call",
                 (unsigned long long)spans->n_spans);
  ANOMOD_REQUIRE(ctx, spans->n_traces <= kMaxSortKeys, "%llu traces: at most %llu per call",
                 (unsigned long long)spans->n_traces, (unsigned long long)kMaxSortKeys);
  ANOMOD_REQUIRE(ctx, out->cap == 0 || (out->shape && out->count && out->abnormal &&
                                        out->first_trace),
                 "cap=%llu with a NULL census array", (unsigned long long)out->cap);
  if (!spans->grouped) {
    set_error(ctx, "span set is not grouped by trace: anomod_spans_group first");
    return ANOMOD_ESTATE;
  }
  if (int rc = bind(ctx)) return rc;

  const uint64_t n = spans->n_spans, nt = spans->n_traces;
  out->n_shapes = 0;
  out->off_tree_spans = 0;
  if (nt == 0) {
    if (out->path_hash && n) memset(out->path_hash, 0, n * 8);
    return ANOMOD_OK;
  }
  // the spans that lie in traces (spans outside every trace are in no shape:
  // their path_hash reads 0)
  uint64_t in_traces[2];
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  const uint64_t n_in = in_traces[1] - in_traces[0];
  if (n_in == 0) {  // only empty traces: one shape, 0
    uint64_t bad = 0;
    if (out->trace_class)
      for (uint64_t t = 0; t < nt; ++t) bad += out->trace_class[t] != 0;
    out->n_shapes = 1;
    if (out->cap) {
      out->shape[0] = 0;
      out->count[0] = nt;
      out->abnormal[0] = bad;
      out->first_trace[0] = 0;
    }
    if (out->trace_shape) memset(out->trace_shape, 0, nt * 8);
    if (out->path_hash && n) memset(out->path_hash, 0, n * 8);
    return ANOMOD_OK;
  }

  // The call's workspace: a block of words (dynamic-tail counter, long-trace
  // counters, off-tree counter, order-probe scratch, run count) and a block of
  // label keys | shapes | path hashes (when asked for) | long-trace list | the
  // listed spans' jump state (40 B per span) | the census arrays (sized to the
  // traces).  The long traces are counted first.
  CallWorkspace ws{ctx};
  const auto al = CallWorkspace::al;
  unsigned long long nlong[2] = {0ull, 0ull};
  if (int rc = ws.take(&ws.words, 256, "trace-shapes")) return rc;
  auto* words = static_cast<unsigned long long*>(ws.words);
  if (int rc = count_long_traces(ctx, spans, words, nlong)) return rc;
  const size_t nl = (size_t)nlong[1];
  const uint64_t m_max = std::min<uint64_t>(out->cap, nt);
  const uint64_t ctiles = (nt + kCTile - 1) / kCTile;
  const size_t b_key = al((size_t)S * 8), b_shape = al(nt * 8);
  const size_t b_ph = out->path_hash ? al(n * 8) : 0;
  const size_t b_list = al(nlong[0] * 16), b_l8 = al(nl * 8), b_l4 = al(nl * 4);
  const size_t b_sort = radix_temp_bytes(nt), b_t8 = al(nt * 8), b_t4 = al(nt * 4);
  const size_t b_tcnt = al(ctiles * 4), b_cls = out->trace_class ? al(nt) : 0;
  const size_t b_out = al(m_max * 8);
  if (int rc = ws.take(&ws.block,
                       b_key + b_shape + b_ph + b_list + 4 * b_l8 + 2 * b_l4 + b_sort + 4 * b_t8 +
                           b_t4 + b_tcnt + b_cls + 4 * b_out,
                       "trace-shapes"))
    return rc;
  ShArgs a{};
  auto* d_key = ws.carve<unsigned long long>(b_key);
  a.svc_key = d_key;
  a.shape = ws.carve<unsigned long long>(b_shape);
  a.path_hash = out->path_hash ? ws.carve<unsigned long long>(b_ph) : nullptr;
  a.big_list = ws.carve<unsigned long long>(b_list);
  a.l_h[0] = ws.carve<unsigned long long>(b_l8);
  a.l_h[1] = ws.carve<unsigned long long>(b_l8);
  a.l_m[0] = ws.carve<unsigned long long>(b_l8);
  a.l_m[1] = ws.carve<unsigned long long>(b_l8);
  a.l_w[0] = ws.carve<uint32_t>(b_l4);
  a.l_w[1] = ws.carve<uint32_t>(b_l4);
  void* d_sort = ws.carve(b_sort);
  auto* d_sorted = ws.carve<uint64_t>(b_t8);  // later the rank keys
  auto* d_run_val = ws.carve<uint64_t>(b_t8);
  auto* d_first = ws.carve<unsigned long long>(b_t8);
  auto* d_abn = ws.carve<unsigned long long>(b_t8);
  auto* d_run_pos = ws.carve<uint32_t>(b_t4);
  auto* d_tcnt = ws.carve<uint32_t>(b_tcnt);
  auto* d_cls = out->trace_class ? ws.carve<uint8_t>(b_cls) : nullptr;
  uint64_t* d_out[4];
  for (auto& p : d_out) p = ws.carve<uint64_t>(b_out);
  a.ctr = words;
  a.big = words + 1;
  a.off_tree = words + 6;
  unsigned long long* d_runs = words + 7;
  a.big_cap = nlong[0];
  a.use_errors = out->use_errors ? 1u : 0u;

  // the label keys and the trace classes (the copies read pageable host
  // memory: they have left it when the calls return)
  std::vector<uint64_t> own_key;
  const uint64_t* h_key = out->svc_key;
  if (!h_key) {
    own_key.resize(S);
    for (uint32_t s = 0; s < S; ++s) own_key[s] = mix64((uint64_t)s + 1);
    h_key = own_key.data();
  }
  ANOMOD_HIP(ctx, hipMemcpyAsync(d_key, h_key, (size_t)S * 8, hipMemcpyHostToDevice, ctx->stream));
  if (d_cls)
    ANOMOD_HIP(ctx, hipMemcpyAsync(d_cls, out->trace_class, nt, hipMemcpyHostToDevice, ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));

  int scan = kScanFwd;
  if (int rc = pick_walk_scan(ctx, spans, S, words + 4, &scan)) return rc;
  const WalkFn fn = scan == kScanFwd     ? trace_shapes_kernel<kScanFwd>
                    : scan == kScanSplit ? trace_shapes_kernel<kScanSplit>
                                         : trace_shapes_kernel<kScanBidir>;
  uint64_t grid = 0;
  if (int rc = walk_grid(ctx, fn, kShThreads, &grid)) return rc;
  log_walk_kernel("trace-shapes", "trace_shapes_kernel", scan, nlong[0]);
  ANOMOD_HIP(ctx, hipMemsetAsync(words, 0, 64, ctx->stream));  // every counter
  if (a.path_hash && n_in < n) ANOMOD_HIP(ctx, hipMemsetAsync(a.path_hash, 0, n * 8, ctx->stream));
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kShThreads), 0, ctx->stream, spans->span_id,
                     spans->parent_span_id, spans->svc_flags, spans->trace_ptr, nt, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (nlong[0]) {
    hipLaunchKernelGGL(trace_shapes_big_kernel,
                       dim3((unsigned)std::min<uint64_t>(nlong[0], 2ull * ctx->num_cus)),
                       dim3(kBigThreads), 0, ctx->stream, spans->span_id, spans->parent_span_id,
                       spans->svc_flags, spans->trace_ptr, a);
    ANOMOD_HIP(ctx, hipGetLastError());
  }

  // ---- census: sorted shapes -> runs -> ranking
  const uint64_t* d_shape = reinterpret_cast<const uint64_t*>(a.shape);
  ANOMOD_HIP(ctx, radix_sort_u64(d_shape, d_sorted, nt, 0, 64, d_sort, b_sort, ctx->stream));
  hipLaunchKernelGGL(run_count_kernel, dim3((unsigned)ctiles), dim3(kCThreads), 0, ctx->stream,
                     d_sorted, nt, d_tcnt);
  hipLaunchKernelGGL(run_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_tcnt, ctiles, d_runs);
  hipLaunchKernelGGL(run_write_kernel, dim3((unsigned)ctiles), dim3(kCThreads), 0, ctx->stream,
                     d_sorted, nt, d_tcnt, d_run_val, d_run_pos);
  ANOMOD_HIP(ctx, hipGetLastError());
  unsigned long long h_words[2] = {0ull, 0ull};  // off-tree spans, runs
  ANOMOD_HIP(ctx, hipMemcpyAsync(h_words, words + 6, 16, hipMemcpyDeviceToHost, ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t R = h_words[1];
  out->off_tree_spans = h_words[0];
  out->n_shapes = R;
  const uint64_t m = std::min<uint64_t>(out->cap, R);
  if (m) {
    uint64_t* d_rank = d_sorted;  // the sorted shapes are dead: the runs hold them
    hipLaunchKernelGGL(rank_key_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0,
                       ctx->stream, d_run_pos, R, nt, d_rank);
    ANOMOD_HIP(ctx, hipGetLastError());
    ANOMOD_HIP(ctx, radix_sort_u64(d_rank, d_rank, R, 0, 64, d_sort, b_sort, ctx->stream));
    ANOMOD_HIP(ctx, hipMemsetAsync(d_first, 0xFF, R * 8, ctx->stream));
    ANOMOD_HIP(ctx, hipMemsetAsync(d_abn, 0, R * 8, ctx->stream));
    hipLaunchKernelGGL(shape_class_kernel,
                       dim3((unsigned)std::min<uint64_t>((nt + 255) / 256, 4ull * ctx->num_cus)),
                       dim3(256), 0, ctx->stream, d_shape, d_cls, nt, d_run_val, R, d_first, d_abn);
    hipLaunchKernelGGL(census_gather_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0,
                       ctx->stream, d_rank, m, d_run_val, d_run_pos, R, nt, d_first, d_abn,
                       d_out[0], d_out[1], d_out[2], d_out[3]);
    ANOMOD_HIP(ctx, hipGetLastError());
    uint64_t* h_out[4] = {out->shape, out->count, out->abnormal, out->first_trace};
    for (int k = 0; k < 4; ++k)
      ANOMOD_HIP(ctx, hipMemcpyAsync(h_out[k], d_out[k], m * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out->trace_shape)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->trace_shape, d_shape, nt * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
  if (out->path_hash)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->path_hash, a.path_hash, n * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANOMOD_OK;
}

}  // extern "C"
