// Trace spectrum of a grouped span set: every trace is labelled normal or
// abnormal, and per class the traces that hold at least one span of each
// service / of each edge row are counted (the coverage counts of
// spectrum-based root-cause ranking).
//
//   row(i)  = the edge row anomod_edge_aggregate_spans counts span i in
//   bad(i)  = dur_us[i] > thr_us[row(i)]  ||  use_errors && error flag of i
//   trace t is abnormal when any of its spans is bad
//
// Two passes.  Pass 1 is the aggregation kernels' own walk in its key form
// (span_edge_keys, edge_agg.hip): keys[i] = row << 32 | dur_us by span
// position.  Pass 2 (spectrum_kernel) is a chunk walk (walk.h: persistent
// waves, <= 256 spans / <= 64 whole traces per chunk, the columns of chunk
// c+1 in flight while chunk c is resolved) that reads 12 B per span (key 8,
// svc|flags 4) and 8 B per trace, and writes 1 B per trace:
//   * every trace of the chunk owns a slot (the rank of its start flag); a
//     bad span sets the slot's class byte in the wave's LDS;
//   * a trace counts once per row and once per service: exactly one of its
//     spans claims each.  Rows are claimed in a per-wave LDS table of 512
//     slots keyed slot << 20 | row (compare-and-swap on an empty slot, linear
//     probing: the span that finds its key already there is a repeat),
//     services in a per-wave bitmap of ceil(S / 32) words per trace slot
//     (the span that sets the bit).  A claim adds 1 to the counter of the
//     trace's class, every bad span adds 1 to bad_spans[row];
//   * lane l of the chunk's first k lanes stores the class byte of trace l and
//     the wave keeps the two class totals in registers.
// Counters are privatised per workgroup in LDS as u32 ([2][E] + [2][S] + [E],
// beside a copy of the thresholds; a workgroup's range holds < 2^32 spans
// because the call does) and flushed once with u64 global atomics; a table
// too wide for the LDS budget counts with global atomics directly, so results
// never depend on which form ran.
//
// Traces longer than a chunk are skipped by the walk and taken by
// spectrum_long_kernel, which sweeps trace_ptr itself: one workgroup per long
// trace, an LDS bitmap of E row bits and S service bits, two sweeps of the
// trace (find the class, then count the newly set bits).  E <= 2^19 keeps the
// row bitmap within 64 KiB.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;
constexpr int kSpWaves = 8;
constexpr int kSpThreads = kSpWaves * kWave;
constexpr uint32_t kMaxRows = 1u << 19;           // the long-trace pass's row bitmap: 64 KiB
constexpr uint32_t kClaim = 2 * kStage;           // row-claim slots per wave (load <= 1/2)
constexpr uint32_t kClaimBits = 9;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;          // (a claim key has 26 bits)
constexpr uint32_t kDynLdsBudget = 44u * 1024u;   // dynamic LDS (+ 19 KiB static < 64 KiB)
constexpr uint32_t kU32Max = 0xFFFFFFFFu;
static_assert(kClaim == 1u << kClaimBits && kClaim % kWave == 0, "power-of-two claim table");

// Per-wave static LDS (every offset a multiple of 16).
constexpr int kPTab = 0;                         // u32 row-claim table [kClaim]
constexpr int kPFlag = kPTab + (int)kClaim * 4;  // u8 trace-start flags [kStage]
constexpr int kPCls = kPFlag + kStage;           // u8 class per trace of the chunk [kWave]
constexpr int kPBytes = kPCls + kWave;
static_assert(kPFlag % 16 == 0 && kPCls % 16 == 0 && kPBytes % 16 == 0,
              "wave staging must stay 16-B aligned");
// Dynamic LDS: per wave the service bits of the chunk's traces, u32 [kWave][ceil(S / 32)];
// then, with LDS counters, the counters [3 E + 2 S] and the thresholds [E].
__host__ __device__ inline uint32_t svc_words(uint32_t S) { return (S + 31u) / 32u; }

struct SpecArgs {
  const unsigned long long* keys;  // [n] row << 32 | dur_us by span position
  const uint32_t* svcfl;           // [n] svc | flags << 16
  const uint32_t* thr;             // [E] or NULL (no latency threshold)
  unsigned long long* ctr;         // trace-segment counter of the dynamic tail
  unsigned long long* misc;        // [0] normal traces, [1] abnormal, [2] spans whose key names no row
  unsigned long long* tab;         // edge_traces [2][E] | svc_traces [2][S] | bad_spans [E]
  uint8_t* cls;                    // [n_traces] or NULL
  uint32_t S, E;
  uint32_t use_errors;
  uint32_t lds;                    // counters privatised in LDS (else global atomics)
};

extern __shared__ __align__(16) unsigned char spec_lds[];

__device__ __forceinline__ bool span_bad(const SpecArgs& a, uint32_t row, uint32_t dur, uint32_t sf) {
  const uint32_t thr = a.thr ? a.thr[row] : kU32Max;
  return dur > thr || (a.use_errors && ((sf >> 16) & ANOMOD_FLAG_ERROR));
}

struct Regs {
  unsigned long long key[kPer];
  uint32_t sf[kPer];
};

__device__ __forceinline__ void load_regs(const SpecArgs& a, const Chunk& c, int lane, Regs& R) {
  const uint32_t n = c.k ? c.n : 0u;  // a long trace is read by spectrum_long_kernel
  const auto rkey = rsrc(a.keys + c.base, n * 8u);
  const auto rsf = rsrc(a.svcfl + c.base, n * 4u);
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = (uint32_t)lane + (uint32_t)(r * kWave);
    R.key[r] = bload64(rkey, i * 8u);
    R.sf[r] = bload32(rsf, i * 4u);
  }
}

// One counter, in the workgroup's LDS copy or straight in the global table.
__device__ __forceinline__ void count(const SpecArgs& a, uint32_t* lctr, uint32_t idx) {
  if (a.lds) atomicAdd(&lctr[idx], 1u);
  else atomicAdd(&a.tab[idx], 1ull);
}

// `end`: this lane's trace end relative to c.base (lanes < c.k); t0: the
// chunk's first trace; nT: the wave's class totals.  lsvc: the wave's service
// bits; lthr: the workgroup's LDS copy of the thresholds (with the LDS counters).
__device__ __forceinline__ void spectrum_chunk(unsigned char* wsm, uint32_t* lsvc, uint32_t* lctr,
                                               const uint32_t* lthr, int lane, const Chunk& c,
                                               uint32_t end, uint64_t t0, const Regs& R,
                                               const SpecArgs& a, unsigned long long (&nT)[2],
                                               uint32_t& invalid) {
  auto* ltab = reinterpret_cast<uint32_t*>(wsm + kPTab);
  auto* lflag = reinterpret_cast<uint8_t*>(wsm + kPFlag);
  auto* lcls = reinterpret_cast<uint8_t*>(wsm + kPCls);
  const uint32_t S = a.S, E = a.E, wsv = svc_words(S);
  lcls[lane] = 0;
#pragma unroll
  for (uint32_t j = 0; j < kClaim / kWave; ++j) ltab[lane + j * kWave] = kEmpty;
  for (uint32_t j = 0; j < wsv; ++j) lsvc[lane + j * kWave] = 0u;
  uint32_t row[kPer], svc[kPer];
  bool live[kPer], bad[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    const uint32_t i = lane + r * kWave;
    const uint32_t dur = (uint32_t)R.key[r];
    row[r] = (uint32_t)(R.key[r] >> 32);
    svc[r] = R.sf[r] & 0xFFFFu;
    const bool in = i < c.n;
    live[r] = in && row[r] < E && svc[r] < S;  // (always, for keys of span_edge_keys)
    invalid += in && !live[r] ? 1u : 0u;
    uint32_t thr = kU32Max;
    if (live[r]) thr = a.lds ? lthr[row[r]] : a.thr ? a.thr[row[r]] : kU32Max;
    bad[r] = live[r] && (dur > thr || (a.use_errors && ((R.sf[r] >> 16) & ANOMOD_FLAG_ERROR)));
  }
  uint64_t Sm[kPer];
  start_masks(lflag, c, lane, Sm);  // (its wave syncs also publish the cleared tables)
  // Every trace of the chunk owns a slot, the rank of its start flag (empty
  // traces share the flag of the trace after them and own none).  A bad span
  // sets its slot's class byte.  Exactly one span per (slot, row) claims the
  // row — the one whose compare-and-swap finds its probe slot empty — and one
  // per (slot, service) the service: the one that sets the bit.
  uint32_t rk[kPer];
  bool own_row[kPer], own_svc[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    rk[r] = trace_in_chunk(Sm, r, lane) & (kWave - 1u);  // (< 64: a chunk holds <= 64 traces)
    own_row[r] = own_svc[r] = false;
    if (!live[r]) continue;
    if (bad[r]) lcls[rk[r]] = 1;
    const uint32_t key = rk[r] << 20 | row[r];  // row < 2^19
    // (<= kStage keys in kClaim slots: a probe always ends)
    for (uint32_t sl = (key * 0x9E3779B1u) >> (32u - kClaimBits);; sl = (sl + 1u) & (kClaim - 1u)) {
      const uint32_t prev = atomicCAS(&ltab[sl], kEmpty, key);
      own_row[r] = prev == kEmpty;
      if (prev == kEmpty || prev == key) break;
    }
    const uint32_t bit = 1u << (svc[r] & 31u);
    own_svc[r] = !(atomicOr(&lsvc[rk[r] * wsv + (svc[r] >> 5)], bit) & bit);
  }
  wave_sync();
  // the traces of the chunk: lane l holds trace t0 + l
  {
    const bool mine = (uint32_t)lane < c.k;
    const bool nonempty = mine && c.start < end;  // an empty trace: normal
    const bool abn = nonempty && lcls[nonempty ? rank_at(Sm, c.start) & (kWave - 1u) : 0u] != 0;
    if (mine && a.cls) a.cls[t0 + (uint64_t)lane] = abn ? 1 : 0;
    const uint32_t n1 = (uint32_t)__popcll(__ballot(abn));
    nT[1] += n1;
    nT[0] += c.k - n1;
  }
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    if (!live[r]) continue;
    const uint32_t cl = lcls[rk[r]];
    if (own_row[r]) count(a, lctr, cl * E + row[r]);
    if (own_svc[r]) count(a, lctr, 2u * E + cl * S + svc[r]);
    if (bad[r]) count(a, lctr, 2u * E + 2u * S + row[r]);
  }
  wave_sync();  // the tables are free for the next chunk
}

__global__ __launch_bounds__(kSpThreads) void spectrum_kernel(
    const uint64_t* __restrict__ trace_ptr, uint64_t n_traces, SpecArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kPBytes * kSpWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  unsigned char* wsm = smem + wid * kPBytes;
  const uint32_t n_svc = kWave * svc_words(a.S);  // service-bit words per wave
  uint32_t* lsvc = reinterpret_cast<uint32_t*>(spec_lds) + wid * n_svc;
  uint32_t* lctr = reinterpret_cast<uint32_t*>(spec_lds) + kSpWaves * n_svc;
  const uint32_t n_ctr = 3u * a.E + 2u * a.S;
  const uint32_t* lthr = lctr + n_ctr;  // [E], with the LDS counters
  if (a.lds) {
    for (uint32_t k = threadIdx.x; k < n_ctr; k += kSpThreads) lctr[k] = 0u;
    for (uint32_t k = threadIdx.x; k < a.E; k += kSpThreads)
      lctr[n_ctr + k] = a.thr ? a.thr[k] : kU32Max;
  }
  __syncthreads();
  unsigned long long nT[2] = {0ull, 0ull};
  uint32_t invalid = 0;
  walk_traces<kSpWaves, 4, Regs>(
      trace_ptr, n_traces, a.ctr,
      [&](const Chunk& c, Regs& R) __attribute__((always_inline)) { load_regs(a, c, lane, R); },
      [&](const Chunk& c, uint32_t end, uint64_t t0, const Regs& R)
          __attribute__((always_inline)) {
            spectrum_chunk(wsm, lsvc, lctr, lthr, lane, c, end, t0, R, a, nT, invalid);
          },
      // longer than kStage: spectrum_long_kernel's
      [](uint64_t, uint32_t) __attribute__((always_inline)) {});
  for (int o = 32; o > 0; o >>= 1) invalid += (uint32_t)__shfl_xor((int)invalid, o);
  if (lane == 0) {
    if (nT[0]) atomicAdd(a.misc, nT[0]);
    if (nT[1]) atomicAdd(a.misc + 1, nT[1]);
    if (invalid) atomicAdd(a.misc + 2, (unsigned long long)invalid);
  }
  if (a.lds) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n_ctr; k += kSpThreads) {
      const uint32_t v = lctr[k];
      if (v) atomicAdd(&a.tab[k], (unsigned long long)v);
    }
  }
}

// ---- long traces ----------------------------------------------------------
// Every workgroup sweeps trace_ptr in tiles of kLongThreads traces and takes
// the tile's traces longer than a chunk one at a time.  spec_lds: row bits
// [ceil(E / 32)] | service bits [ceil(S / 32)], clear between traces.
constexpr int kLongThreads = 512;

__global__ __launch_bounds__(kLongThreads) void spectrum_long_kernel(
    const uint64_t* __restrict__ trace_ptr, uint64_t n_traces, SpecArgs a) {
  auto* bits = reinterpret_cast<uint32_t*>(spec_lds);
  __shared__ uint32_t s_n;
  __shared__ uint16_t s_list[kLongThreads];
  const uint32_t tid = threadIdx.x;
  const uint32_t S = a.S, E = a.E;
  const uint32_t we = (E + 31u) / 32u, words = we + (S + 31u) / 32u;
  for (uint32_t k = tid; k < words; k += kLongThreads) bits[k] = 0u;
  unsigned long long nT[2] = {0ull, 0ull};  // thread 0's
  uint32_t invalid = 0;
  for (uint64_t t0 = (uint64_t)blockIdx.x * kLongThreads; t0 < n_traces;
       t0 += (uint64_t)gridDim.x * kLongThreads) {
    bool is_long = false;
    if (t0 + tid < n_traces)
      is_long = trace_ptr[t0 + tid + 1] - trace_ptr[t0 + tid] > (uint64_t)kStage;
    const uint32_t n_long = (uint32_t)__syncthreads_count(is_long);
    if (!n_long) continue;
    if (tid == 0) s_n = 0u;
    __syncthreads();
    if (is_long) s_list[atomicAdd(&s_n, 1u)] = (uint16_t)tid;
    __syncthreads();  // (also: the bitmap is clear)
    for (uint32_t j = 0; j < n_long; ++j) {
      const uint64_t t = t0 + s_list[j];
      const uint64_t lo = trace_ptr[t];
      const uint32_t L = (uint32_t)(trace_ptr[t + 1] - lo);  // the call takes < 2^32 spans
      // sweep 1: the class
      bool any_bad = false;
      for (uint32_t i = tid; i < L; i += kLongThreads) {
        const unsigned long long key = a.keys[lo + i];
        const uint32_t sf = a.svcfl[lo + i];
        const uint32_t row = (uint32_t)(key >> 32);
        if (row < E && (sf & 0xFFFFu) < S) any_bad |= span_bad(a, row, (uint32_t)key, sf);
      }
      const uint32_t cl = __syncthreads_or(any_bad) ? 1u : 0u;
      // sweep 2: the rows / services the trace sets for the first time
      for (uint32_t i = tid; i < L; i += kLongThreads) {
        const unsigned long long key = a.keys[lo + i];
        const uint32_t sf = a.svcfl[lo + i];
        const uint32_t row = (uint32_t)(key >> 32), svc = sf & 0xFFFFu;
        if (!(row < E && svc < S)) {
          ++invalid;
          continue;
        }
        const uint32_t mr = 1u << (row & 31u), ms = 1u << (svc & 31u);
        if (!(atomicOr(&bits[row >> 5], mr) & mr)) atomicAdd(&a.tab[cl * E + row], 1ull);
        if (!(atomicOr(&bits[we + (svc >> 5)], ms) & ms))
          atomicAdd(&a.tab[2u * E + cl * S + svc], 1ull);
        if (span_bad(a, row, (uint32_t)key, sf)) atomicAdd(&a.tab[2u * E + 2u * S + row], 1ull);
      }
      if (tid == 0) {
        nT[cl] += 1ull;
        if (a.cls) a.cls[t] = (uint8_t)cl;
      }
      __syncthreads();
      for (uint32_t k = tid; k < words; k += kLongThreads) bits[k] = 0u;
      __syncthreads();
    }
  }
  if (tid == 0) {
    if (nT[0]) atomicAdd(a.misc, nT[0]);
    if (nT[1]) atomicAdd(a.misc + 1, nT[1]);
  }
  if (invalid) atomicAdd(a.misc + 2, (unsigned long long)invalid);
}

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_trace_spectrum_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                anomod_trace_spectrum* out) {
  ANOMOD_REQUIRE(nullptr, ctx && spans && out, "anomod_trace_spectrum_spans: NULL argument");
  const uint32_t S = out->n_services;
  ANOMOD_REQUIRE(ctx, S >= 1 && (uint64_t)(S + ANOMOD_ROOT_ROWS) * S <= kMaxRows,
                 "anomod_trace_spectrum_spans: n_services=%u gives %llu edge rows, outside "
                 "[3, 2^19]", S, (unsigned long long)(S + ANOMOD_ROOT_ROWS) * S);
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device,
                 "anomod_trace_spectrum_spans: span set lives on another device");
  if (!spans->grouped) {
    set_error(ctx, "span set is not grouped by trace: anomod_spans_group first");
    return ANOMOD_ESTATE;
  }
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "anomod_trace_spectrum_spans: span service index %u >= n_services %u",
                 spans->max_svc, S);
  ANOMOD_REQUIRE(ctx, spans->n_spans < (1ull << 32) - 1,
                 "anomod_trace_spectrum_spans: %llu spans: at most 2^32 - 2 per call",
                 (unsigned long long)spans->n_spans);
  if (int rc = bind(ctx)) return rc;
  const uint64_t nt = spans->n_traces;
  // the spans that lie in traces (an upload may leave spans outside every
  // trace: the aggregation counts none of them)
  uint64_t in_traces[2];
  if (int rc = trace_span_range(ctx, spans, in_traces, "anomod_trace_spectrum_spans: ")) return rc;
  const uint64_t n = in_traces[1] > in_traces[0] ? in_traces[1] : 0;
  const size_t n_tab = 3ull * E + 2ull * S;
  out->n_traces[0] = out->n_traces[1] = 0;
  if (n == 0) {  // no span in any trace: every trace is empty, hence normal
    out->n_traces[0] = nt;
    if (out->edge_traces) memset(out->edge_traces, 0, 2ull * E * 8);
    if (out->svc_traces) memset(out->svc_traces, 0, 2ull * S * 8);
    if (out->bad_spans) memset(out->bad_spans, 0, (size_t)E * 8);
    if (out->trace_abnormal && nt) memset(out->trace_abnormal, 0, nt);
    return ANOMOD_OK;
  }

  // The call's workspace, freed when it returns (after the stream's work):
  // keys | the key walk's words | counters (dynamic tail, class totals,
  // invalid keys) + the tables (zeroed together) | thresholds | class bytes.
  const char* lg = getenv("ANOMOD_LOG_KERNEL");  // (tests, timing)
  const bool log = lg && lg[0] == '1';
  // (walk.h's CallWorkspace with the two times logged)
  struct TimedBlock {
    anomod_ctx* ctx;
    bool log;
    void* block = nullptr;
    ~TimedBlock() {
      if (!block) return;
      (void)hipStreamSynchronize(ctx->stream);
      const double t0 = host_now_ms();
      (void)hipFree(block);
      if (log) fprintf(stderr, "anomod: spectrum workspace freed in %.3f ms\n", host_now_ms() - t0);
    }
  } ws{ctx, log};
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t b_keys = al(n * 8), b_ws = al(span_edge_keys_ws_bytes(spans));
  const size_t b_tab = 256 + al(n_tab * 8);
  const size_t b_thr = out->thr_us ? al((size_t)E * 4) : 0;
  const size_t b_cls = out->trace_abnormal ? al(nt) : 0;
  const size_t bytes = b_keys + b_ws + b_tab + b_thr + b_cls;
  const double t_alloc = host_now_ms();
  if (dev_malloc(ctx, &ws.block, bytes) != hipSuccess) {
    (void)hipGetLastError();
    ws.block = nullptr;
    set_error(ctx, "hipMalloc(%zu) for the trace-spectrum workspace failed", bytes);
    return ANOMOD_ENOMEM;
  }
  if (log)
    fprintf(stderr, "anomod: spectrum workspace of %zu bytes allocated in %.3f ms\n", bytes,
            host_now_ms() - t_alloc);
  char* w = static_cast<char*>(ws.block);
  auto* words = reinterpret_cast<unsigned long long*>(w + b_keys + b_ws);
  SpecArgs a{};
  a.keys = reinterpret_cast<unsigned long long*>(w);
  a.svcfl = spans->svc_flags;
  a.ctr = words;
  a.misc = words + 1;
  a.tab = words + 32;
  a.thr = out->thr_us ? reinterpret_cast<uint32_t*>(w + b_keys + b_ws + b_tab) : nullptr;
  a.cls = out->trace_abnormal ? reinterpret_cast<uint8_t*>(w + b_keys + b_ws + b_tab + b_thr)
                              : nullptr;
  a.S = S;
  a.E = E;
  a.use_errors = out->use_errors ? 1u : 0u;
  // dynamic LDS: the waves' service bits, then the counters and a copy of the thresholds
  const size_t lds_svc = (size_t)kSpWaves * kWave * svc_words(S) * 4, lds_ctr = (n_tab + E) * 4;
  a.lds = lds_svc + lds_ctr <= kDynLdsBudget ? 1u : 0u;
  ANOMOD_HIP(ctx, hipMemsetAsync(words, 0, b_tab, ctx->stream));
  if (a.thr)
    ANOMOD_HIP(ctx, hipMemcpyAsync(const_cast<uint32_t*>(a.thr), out->thr_us, (size_t)E * 4,
                                   hipMemcpyHostToDevice, ctx->stream));
  if (int rc = span_edge_keys(ctx, spans, S, const_cast<unsigned long long*>(a.keys),
                              reinterpret_cast<unsigned long long*>(w + b_keys)))
    return rc;
  const size_t dyn = lds_svc + (a.lds ? lds_ctr : 0);
  if (dyn > kDynLdsBudget) {  // (S > 704) above the default limit with the kernel's static part
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(spectrum_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    (void)hipGetLastError();
  }
  uint64_t grid = 0;
  if (int rc = walk_grid(ctx, spectrum_kernel, kSpThreads, &grid, dyn)) return rc;
  // (unknown longest trace: the long pass looks for itself)
  const bool long_pass = spans->max_trace_len > (uint64_t)kStage;
  if (log)
    fprintf(stderr, "anomod: spectrum_kernel counters in %s, long pass %s\n",
            a.lds ? "LDS" : "global memory", long_pass ? "on" : "off");
  hipLaunchKernelGGL(spectrum_kernel, dim3((unsigned)grid), dim3(kSpThreads), dyn, ctx->stream,
                     spans->trace_ptr, nt, a);
  ANOMOD_HIP(ctx, hipGetLastError());
  if (long_pass) {
    const size_t bits = ((size_t)(E + 31u) / 32u + (S + 31u) / 32u) * 4;
    if (bits > 60u * 1024u) {  // above the default dynamic-LDS limit with the kernel's static part
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(spectrum_long_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bits);
      (void)hipGetLastError();
    }
    const uint64_t tiles = (nt + kLongThreads - 1) / kLongThreads;
    hipLaunchKernelGGL(spectrum_long_kernel,
                       dim3((unsigned)std::min<uint64_t>(tiles, 2ull * ctx->num_cus)),
                       dim3(kLongThreads), bits, ctx->stream, spans->trace_ptr, nt, a);
    ANOMOD_HIP(ctx, hipGetLastError());
  }
  unsigned long long misc[3] = {0ull, 0ull, 0ull};
  ANOMOD_HIP(ctx, hipMemcpyAsync(misc, a.misc, 24, hipMemcpyDeviceToHost, ctx->stream));
  if (out->edge_traces)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->edge_traces, a.tab, 2ull * E * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
  if (out->svc_traces)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->svc_traces, a.tab + 2ull * E, 2ull * S * 8,
                                   hipMemcpyDeviceToHost, ctx->stream));
  if (out->bad_spans)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->bad_spans, a.tab + 2ull * E + 2ull * S, (size_t)E * 8,
                                   hipMemcpyDeviceToHost, ctx->stream));
  if (a.cls)
    ANOMOD_HIP(ctx, hipMemcpyAsync(out->trace_abnormal, a.cls, nt, hipMemcpyDeviceToHost,
                                   ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (misc[2]) {
    set_error(ctx, "trace spectrum: %llu spans carry no edge key (internal error)", misc[2]);
    return ANOMOD_ESTATE;
  }
  out->n_traces[0] = misc[0];
  out->n_traces[1] = misc[1];
  return ANOMOD_OK;
}

}  // extern "C"
