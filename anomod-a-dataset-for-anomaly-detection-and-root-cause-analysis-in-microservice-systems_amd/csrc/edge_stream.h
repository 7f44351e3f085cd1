// The shared edge stream (internal): what the windowed table (edge_windows.hip),
// the per-window quantiles (edge_window_quantiles.hip), the edge load
// (edge_load.hip) and the edge exemplars (edge_exemplars.hip) have in common.
// Each is a persistent stream over span positions: every workgroup owns one
// contiguous range of whole batches, a lane takes four spans of a batch, and
// the edge row of a span comes from one of two sources:
//   keys  span_edge_keys (the aggregation's own walk, edge_agg.hip) wrote
//         edge << 32 | dur_us by span position
//   rows  the set holds complete parent rows (anomod_spans::parent_row): row,
//         svc|flags and dur_us are read in place
// The device side is the batch loader of both forms, the window rule, the
// sliding LDS window ring and the tail counters; the host side (edge_stream.hip)
// is the argument checks, the source decision, the workspace cursor, the launch
// geometry and the read-back of the counters.  What a pass does with a span —
// its cells, lists and flush bodies — stays in its own file.
#pragma once

#include "common.h"
#include "walk.h"

namespace anomod {
namespace {
namespace stream {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // no window / no edge / no slot of the tile

// The spans of this workgroup: [*lo, *hi) of [0, n), per_wg a multiple of the batch.
__device__ __forceinline__ void wg_range(uint64_t per_wg, uint64_t n, uint64_t* lo, uint64_t* hi) {
  *lo = (uint64_t)blockIdx.x * per_wg;
  *hi = *lo + per_wg < n ? *lo + per_wg : n;
}

// A lane's four spans of the batch of THREADS * 4 at b (a multiple of the batch
// size), in runs of RUN consecutive positions: RUN = 2, the keys form (two
// pairs, THREADS pairs apart: 16-B loads of 8-B columns); RUN = 4, the rows
// form (16 B of a 4-B column).  load() sets live[j]: the span is inside
// [begin, hi), begin = trace_ptr[0] (an upload may leave spans outside every
// trace).  A full batch is loaded as aligned non-temporal vectors of up to
// 16 B, dead heads included; the last partial batch of a range span by span,
// 0 where not live.
template <int THREADS, int RUN>
struct Lanes {
  static constexpr int kBatch = THREADS * 4;
  uint64_t p0, hi, begin;
  bool full, live[4];
  __device__ __forceinline__ Lanes(uint64_t b, uint64_t hi_, uint64_t begin_, uint32_t tid)
      : p0(b + (uint64_t)tid * RUN), hi(hi_), begin(begin_), full(b + kBatch <= hi_) {}
  __device__ __forceinline__ uint64_t pos(int j) const {
    return p0 + (uint64_t)((j / RUN) * THREADS * RUN + j % RUN);
  }
  // Every column a pass reads, as (column, values[4]) pairs in one call: the
  // loads of a full batch then sit in one branch and are all issued before the
  // first use.  (With a call per column the compiler sank the later columns'
  // loads behind the window ring's barrier, + 13 % on edge_windows_kernel; with
  // each column unpacked right after its load it waited for one column before
  // it asked for the next, + 30 % on edge_exemplars_kernel<rows>; with the live
  // flags of both branches formed ahead of them as one expression the
  // exemplars kernels were 3 - 5 % and edge_windows_kernel 2 % slower.)
  template <typename... Cols>
  __device__ __forceinline__ void load(Cols... cols) {
    if (full) {
#pragma unroll
      for (int j = 0; j < 4; ++j) live[j] = pos(j) >= begin;
      vec(cols...);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) live[j] = pos(j) < hi && pos(j) >= begin;
      tail(cols...);
    }
  }
  __device__ __forceinline__ void vec() const {}
  template <typename T, typename... More>
  __device__ __forceinline__ void vec(const T* col, T* v, More... more) const {
    constexpr int VE = RUN * sizeof(T) > 16 ? 16 / sizeof(T) : RUN;
    typedef T V __attribute__((ext_vector_type(VE)));
    const auto nt = [&](int j) {
      return __builtin_nontemporal_load(reinterpret_cast<const V*>(col + pos(j)));
    };
    const V x = nt(0);
    if constexpr (VE == 4) {
      vec(more...);  // (the other columns' loads, before this one's first use)
      v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
      const V y = nt(2);
      vec(more...);
      v[0] = x.x, v[1] = x.y, v[2] = y.x, v[3] = y.y;
    }
  }
  __device__ __forceinline__ void tail() const {}
  template <typename T, typename... More>
  __device__ __forceinline__ void tail(const T* col, T* v, More... more) const {
    // The mirror image of vec(): loads in the order of the arguments, values
    // handed over in the reverse order.  Where the two branches of load() ended
    // with stores to different arrays the compiler merged them into one store
    // through a pointer to either, and both arrays stayed in scratch (24 B/lane
    // in window_cell_keys_kernel and edge_load_kernel<keys>).
    T t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = live[j] ? col[pos(j)] : T(0);
    tail(more...);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = t[j];
  }
  // the positions of the batch inside the range, live or not (a column
  // rewritten in place: each position is read and written by one lane)
  template <typename T>
  __device__ __forceinline__ void store(T* col, const T v[4]) const {
    constexpr int VE = RUN * sizeof(T) > 16 ? 16 / sizeof(T) : RUN;
    typedef T V __attribute__((ext_vector_type(VE)));
    if (full) {
#pragma unroll
      for (int j = 0; j < 4; j += VE) {
        V x;
#pragma unroll
        for (int k = 0; k < VE; ++k) x[k] = v[j + k];
        *reinterpret_cast<V*>(col + pos(j)) = x;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (pos(j) < hi) col[pos(j)] = v[j];
    }
  }
};

// The keys form: edge row and duration of the lane's four spans; `more`: the
// companion columns of the pass (start times, svc|flags), loaded with the keys.
template <int THREADS, typename... More>
__device__ __forceinline__ void load_keys(Lanes<THREADS, 2>& L, const unsigned long long* keys,
                                          uint32_t edge[4], uint32_t dur[4], More... more) {
  unsigned long long key[4];
  L.load(keys, key, more...);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    edge[j] = (uint32_t)(key[j] >> 32);
    dur[j] = (uint32_t)key[j];
  }
}

// The rows form: svc|flags, duration and edge row p * S + svc (kNone: no edge
// of a table of S services) of the lane's four spans; `more` as above.
template <int THREADS, typename... More>
__device__ __forceinline__ void load_rows(Lanes<THREADS, 4>& L, const uint16_t* rows,
                                          const uint32_t* svcfl, const uint32_t* dur_us, uint32_t S,
                                          uint32_t S0, uint32_t edge[4], uint32_t dur[4],
                                          uint32_t sf[4], More... more) {
  uint16_t row[4];
  L.load(more..., svcfl, sf, dur_us, dur, rows, row);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // root / orphan codes of the aggregation that wrote the rows -> this call's
    const uint32_t p = row[j] >= S0 ? row[j] - S0 + S : row[j];
    const uint32_t svc = sf[j] & 0xFFFFu;
    edge[j] = p < S + ANOMOD_ROOT_ROWS && svc < S ? p * S + svc : kNone;
  }
}

// The window a span starts in, kNone outside [t0, t0 + T * step): start < t0
// first (unsigned), then the quotient against T — t0 + T * step may pass 2^64
// and is never formed.
__device__ __forceinline__ uint32_t window_of(uint64_t start, uint64_t t0, uint64_t step,
                                              uint32_t T) {
  const uint64_t q = start >= t0 ? (start - t0) / step : (uint64_t)T;
  return q < (uint64_t)T ? (uint32_t)q : kNone;
}

// Sliding tile of Wt consecutive windows in LDS: a ring of Wt window slots
// (the cells of a slot are the pass's own) anchored at the smallest window of
// the current batch; window w of the tile [base, base + Wt) lives in slot
// (slot0 + w - base) mod Wt.  When the stream moves past a window its slot is
// flushed by the pass's flush_slot(slot, w), which also leaves the slot clean.
// A window outside the tile has no slot: the pass sends it to global atomics,
// so correctness never depends on the hit rate; Wt = 0 is the all-global
// kernel.  Every call below is made by the whole workgroup (uniform).
struct WindowRing {
  uint32_t Wt;
  bool anchored = false;
  uint32_t base = 0, slot0 = 0;
  // batch minima, three deep: batch `it` collects in [it % 3] while a late
  // wave may still read [(it - 1) % 3]
  static __device__ __forceinline__ uint32_t* s_min() {
    __shared__ uint32_t m[3];
    return m;
  }
  // before the barrier that follows the pass's own zeroing of its cells
  __device__ __forceinline__ void init(uint32_t tid) const {
    if (tid < 3) s_min()[tid] = kNone;
  }
  // Once per batch, between the batch's window computation and its LDS
  // atomics: moves the anchor to the batch's smallest window.  lmin: the
  // lane's smallest window, kNone when it has none.
  template <typename Flush>
  __device__ __forceinline__ void advance(uint32_t it, uint32_t lmin, uint32_t tid,
                                          Flush&& flush_slot) {
    if (!Wt) return;
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)lmin, o);
      lmin = lmin < other ? lmin : other;
    }
    if ((tid & 63u) == 0 && lmin != kNone) atomicMin(&s_min()[it % 3u], lmin);
    __syncthreads();  // also: the previous batch's LDS atomics have landed
    const uint32_t bmin = s_min()[it % 3u];
    if (tid == 0) s_min()[(it + 2u) % 3u] = kNone;  // read last in batch it - 1
    if (bmin == kNone) return;
    if (!anchored) {
      anchored = true;
      base = bmin;
    } else if (bmin > base) {
      const uint32_t adv = bmin - base;
      const uint32_t nf = adv < Wt ? adv : Wt;
      for (uint32_t k = 0; k < nf; ++k) {
        const uint32_t s = slot0 + k;
        flush_slot(s >= Wt ? s - Wt : s, base + k);
      }
      slot0 = adv < Wt ? (slot0 + adv >= Wt ? slot0 + adv - Wt : slot0 + adv) : 0u;
      base = bmin;
      __syncthreads();  // slots are clean before anyone reuses them
    }
  }
  // the slot of window w, kNone when w is outside the tile
  __device__ __forceinline__ uint32_t slot_of(uint32_t w) const {
    if (!(anchored && w >= base && w - base < Wt)) return kNone;
    const uint32_t s = slot0 + (w - base);
    return s >= Wt ? s - Wt : s;
  }
  // after the last batch: what the tile still holds, bounded by T
  template <typename Flush>
  __device__ __forceinline__ void finish(uint32_t T, Flush&& flush_slot) const {
    if (!Wt) return;
    __syncthreads();
    if (anchored)
      for (uint32_t k = 0; k < Wt && (uint64_t)base + k < T; ++k) {
        const uint32_t s = slot0 + k;
        flush_slot(s >= Wt ? s - Wt : s, base + k);
      }
  }
};

// A per-lane tail counter (spans outside the window range, spans that name no
// edge row) summed over the wave and added to *word by its first lane.
__device__ __forceinline__ void count_add(unsigned long long* word, uint32_t v, uint32_t tid) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  if ((tid & 63u) == 0 && v) atomicAdd(word, (unsigned long long)v);
}

}  // namespace stream
}  // namespace

// ---- host side of a stream call (edge_stream.hip) ----------------------------------
constexpr uint64_t kStreamMaxRange = 1ull << 31;  // spans per workgroup (u32 LDS counts)

// Value of a numeric environment cap (tests, A/B), "no cap" when unset or not
// a number; at least `floor` (a workgroup cap must be at least 1).
uint64_t env_cap(const char* name, uint64_t floor = 0);

// S, T and step of a windowed table: *E = the edge rows of S services.
int stream_table_args(anomod_ctx* ctx, uint32_t S, uint32_t T, uint64_t step, uint32_t* E);
// The span set of a stream call: on the ctx's device, grouped (else
// `ungrouped_rc`), with a start column when the pass needs one, services below
// S; then the spans that lie in traces (walk.h: trace_span_range; the
// aggregation counts no other): in_traces, *n = in_traces[1], 0 when empty.
int stream_set_args(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S, bool need_start,
                    int ungrouped_rc, uint64_t in_traces[2], uint64_t* n);

// Where a call that has both forms takes its edge rows from.  rows: the set
// holds complete parent rows over exactly the spans in traces; else the keys
// form, whose keys (b_keys bytes) and key-walk words (b_ws) open the call's
// workspace and are written by fill() on the ctx stream.
struct EdgeSource {
  bool rows;
  size_t b_keys, b_ws;
  unsigned long long* keys = nullptr;
  EdgeSource(const anomod_spans* spans, const uint64_t in_traces[2], uint64_t n);
  int fill(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S, char* workspace);
};

// Cursor over a workspace of 256-B aligned pieces.
struct Carve {
  char* p;
  static size_t al(size_t x) { return CallWorkspace::al(x); }
  template <typename T = char>
  T* take(size_t bytes, bool want = true) {
    char* q = want ? p : nullptr;
    if (want) p += bytes;
    return reinterpret_cast<T*>(q);
  }
};

// Persistent workgroups over n positions, one contiguous range of whole
// batches each: per_cu workgroups a CU, at most `cap`, ranges of at most
// max_range spans (then more workgroups than are resident).  *per_wg spans a
// workgroup, the grid as the return value.
uint64_t stream_grid(const anomod_ctx* ctx, uint64_t n, uint64_t batch, int per_cu, uint64_t cap,
                     uint64_t max_range, uint64_t* per_wg);
// The same with per_cu from the kernel's occupancy and the cap from `wgs_env`.
template <typename Fn>
int stream_geometry(anomod_ctx* ctx, Fn fn, int threads, size_t lds, uint64_t n,
                    const char* wgs_env, uint64_t* per_wg, uint64_t* grid) {
  int per_cu = 0;
  ANOMOD_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void*>(fn), threads, lds));
  *grid = stream_grid(ctx, n, (uint64_t)threads * 4, per_cu > 0 ? per_cu : 1, env_cap(wgs_env, 1),
                      kStreamMaxRange, per_wg);
  return ANOMOD_OK;
}

// Under log_kernel() (tests): the geometry of one stream launch on stderr,
//   anomod: stream KERNEL<FORM>[, tile N windows][, lists PLACE], grid G, P spans per workgroup
// tile < 0: a kernel without a window ring; lists NULL: one without lists.
void stream_log(const char* kernel, const char* form, int64_t tile, const char* lists,
                uint64_t grid, uint64_t per_wg);

// A result table queued back to the host when the caller asked for it (dst != NULL).
hipError_t stream_back(anomod_ctx* ctx, void* dst, const void* src, size_t bytes);
// The end of a call: the two counter words back (after the tables the caller
// queued), the wait for the stream, and misc[bad] != 0 reported as
// "`pass`: N spans carry no edge `what` (internal error)", ANOMOD_ESTATE.
int stream_finish(anomod_ctx* ctx, const unsigned long long* d_misc, int bad, const char* pass,
                  const char* what, unsigned long long misc[2]);

}  // namespace anomod
