// Internal shared definitions of libanomod (not part of the public ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/anomod.h"
#include "span_word.h"

namespace anomod {

// Error plumbing: a per-thread message for ctx-less failures, a per-ctx one
// otherwise (anomod_last_error).
void set_error(anomod_ctx* ctx, const char* fmt, ...);
// ANOMOD_LOG_KERNEL=1 (tests, timing): a call names the kernels it picked on stderr.
inline bool log_kernel() {
  const char* lg = getenv("ANOMOD_LOG_KERNEL");
  return lg && lg[0] == '1';
}

struct GroupWs;   // group.hip
struct Uploader;  // upload.hip

// One host -> device copy of the upload pipeline (upload.hip): kind 0 copies
// n bytes from a; kind 1 packs n elements of svc (u16, a) | flags (u16, b) << 16
// into u32 words.
struct UpItem {
  void* dst;
  const void* a;
  const void* b;
  uint64_t n;
  int kind;
};

enum Stage { kStageEdgeAgg = 0, kStageEdgeFinal = 1, kStageEdgeReduce = 2, kStageEwma = 3,
             kStagePagerank = 4, kStageTraceStruct = 5, kStageSegments = 6, kStageSummary = 7,
             kStageGroup = 8, kStageEdgeWindows = 9, kStageEdgeWindowKernel = 10,
             kStageEdgeLoad = 11, kStageEdgeLoadKernel = 12, kStageEdgeLoadScan = 13,
             kStageEdgeExemplars = 14, kStageEdgeExemplarsKernel = 15, kStageSeriesCorr = 16,
             kNumStages = 17 };

// Host wall-clock slots (anomod_ctx_host_ms): the last occurrence of each
// one-off setup step, or of a call phase the stage events cannot see.
enum HostSlot { kHostGroupAlloc = ANOMOD_HOST_GROUP_ALLOC, kHostGroupPinned = ANOMOD_HOST_GROUP_PINNED,
                kHostGroupWall = ANOMOD_HOST_GROUP_WALL, kHostUploadSetup = ANOMOD_HOST_UPLOAD_SETUP,
                kHostSetAlloc = ANOMOD_HOST_SET_ALLOC, kNumHostSlots = ANOMOD_HOST_SLOTS };

// Dense edge stream of a resident set (edge_agg.hip): the layout the set
// learned from one of its own edge tables — every edge with spans gets a code
// (its rank among those edges) and the bin range [hist_bin(min), hist_bin(max)]
// of a cell array — and the span-word column written through it, in one of the
// three formats of span_word.h: u32 words of code, error bit and either cell +
// residual or the duration of every span position, or the cell word packed into
// 3 bytes, in two planes.  Owned by the set (anomod_spans::dense) and released
// with it; the device to free on is the one current in free_spans.
struct DenseSet {
  enum State { kNone = 0,      // this S was looked at and does not fit (or was rejected)
               kLearned = 1,   // host layout ready, word column not written yet
               kCoded = 2 };   // layout on the device, word column written
  int state = kNone;
  uint32_t S = 0;              // the service count the layout was learned under
  uint32_t codes = 0, cells = 0;
  uint32_t streams = 0;        // row streams at S since the layout was learned
  int tier = 0;                // 0 = small, 1 = large LDS carve
  int wgs_per_cu = 0;          // dense kernel workgroups per CU (0: not asked yet)
  bool cell_words = false;     // the column holds cell words (fmt), else duration words
  bool pack = false;           // ... as packed words (pack_fmt(fmt)): 3 B per span position
  bool errcells = false;       // packed, small carve: the kernel keeps a cell's error spans in
                               // an entry of their own (edge_dense_kernel<0, 3>)
  CellFmt fmt = {0, 0, 0};
  // host layout: 4 words per code {edge, first_bin, base, width}, then the
  // edge -> code table (u16, 0xFFFF = no code) packed two per word
  std::vector<uint32_t> host;
  void* dev = nullptr;         // the same on the device + the encoder's flag and wide count
  size_t dev_bytes = 0;
  uint32_t* word = nullptr;    // [n_spans]: span words of this S; kWordSkip = no span here
                               // (pack: u16 [n_spans], then u8 [n_spans] at pack_lo_offset)
  size_t word_bytes = 0;
  DenseSet() = default;
  DenseSet(const DenseSet&) = delete;
  DenseSet& operator=(const DenseSet&) = delete;
  ~DenseSet() {
    if (dev) (void)hipFree(dev);
    if (word) (void)hipFree(word);
  }
};

}  // namespace anomod

struct anomod_ctx {
  int device = 0;
  int num_cus = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_begin[anomod::kNumStages] = {};
  hipEvent_t ev_end[anomod::kNumStages] = {};
  bool stage_recorded[anomod::kNumStages] = {};
  double host_ms[anomod::kNumHostSlots] = {};        // anomod_ctx_host_ms
  uint64_t host_count[anomod::kNumHostSlots] = {};
  std::string err;
  // RCCL communicator (one process per GPU) ...
  ncclComm_t comm = nullptr;
  // ... or a host transport (anomod_ctx_attach_host_comm: ranks sharing a
  // device, or a host-side library such as gloo)
  anomod_host_allreduce_fn host_allreduce = nullptr;
  anomod_host_allgather_fn host_allgather = nullptr;
  void* host_user = nullptr;
  void* h_coll = nullptr;      // pinned staging of host-transport collectives
  size_t coll_bytes = 0;
  int nranks = 1;
  int rank = 0;
  bool comm_aborted = false;   // set once the communicator was aborted
  double comm_timeout_s = 300; // ANOMOD_RCCL_TIMEOUT_S
  int* d_status = nullptr;     // device word of the status agreement
  int* h_status = nullptr;     // pinned host twin
  // Trace-grouping workspace (segmented radix sort of ungrouped span sets).
  anomod::GroupWs* group_ws = nullptr;
  int group_path = 0, group_levels = 0, group_bits = 0;  // anomod_ctx_group_info
  // Grow-only device scratch of the calls that need a large one-call
  // workspace (anomod::ScratchSlot).  Freeing a block of tens of GB costs the
  // driver's wipe of it (~30 ms/GB, in hipFree or in a later allocation:
  // scripts/r06/time_cold2.py), so a call reuses its slot instead of
  // allocating and freeing; released with the ctx, or when an allocation
  // would otherwise fail (release_scratch).
  void* scratch[5] = {};
  size_t scratch_bytes[5] = {};
  // Cached device workspace for the edge table.
  void* d_table = nullptr;
  size_t table_bytes = 0;
  // Pinned host staging for the edge table's small per-edge vectors (one D2H).
  void* h_stage = nullptr;
  size_t stage_bytes = 0;
  // Upload pipeline (worker threads, their streams and pinned buffers) and
  // the grow-only device span set anomod_edge_aggregate_host fills.
  anomod::Uploader* uploader = nullptr;
  anomod_spans* host_set = nullptr;
  uint64_t host_set_spans = 0, host_set_traces = 0;  // its capacity
};

struct anomod_spans {
  int device = 0;
  uint64_t n_spans = 0;
  uint64_t n_traces = 0;
  uint32_t max_svc = 0;      // largest service index present (host-validated)
  // longest trace in spans when known (upload, synthetic generation);
  // UINT64_MAX = unknown.  Lets a call skip the long-trace pass when no
  // trace outgrows a wave chunk.
  uint64_t max_trace_len = ~0ull;
  // Histogram form of the SN / TrainTicket-width edge kernels: 0 = pair (8 Ki
  // slots, right for sets that touch a few thousand (edge, bin) keys per
  // workgroup), 1 = compact (16 Ki packed slots), -1 = not known yet — the
  // aggregation then starts in the pair form and any workgroup whose table
  // saturates hands its remaining traces to a compact-form resume launch
  // (edge_agg.hip); the outcome is kept here for the set's next aggregation.
  mutable int8_t hist_form = -1;
  // Span ids are unique within every trace (declared by the producer: the
  // synthetic generator by construction, anomod_spans_set_unique_ids for
  // decoded / uploaded sets).  Lets the parent lookups scan from both ends
  // (any match is the first match).  false = unknown: forward scan only.
  bool unique_ids = false;
  // Parent-scan order hint for unique-id sets: 1 = collector order (most
  // child spans right after their parent: the bidirectional scan), 0 = not
  // (spans shuffled inside their traces: the forward scan), -1 = unknown —
  // probed on the device at the first aggregation (edge_agg.hip probe_order).
  mutable int8_t order = -1;
  bool grouped = true;       // false: spans in arrival order, trace_ptr = NULL
                             // (anomod_spans_upload_ungrouped; group first)
  uint64_t* trace_hash = nullptr;
  uint64_t* span_id = nullptr;
  uint64_t* parent_span_id = nullptr;
  uint32_t* svc_flags = nullptr;  // svc | flags << 16 (one 4-B load per span)
  uint32_t* dur_us = nullptr;
  uint64_t* trace_ptr = nullptr;  // [n_traces + 1]
  uint64_t* start_us = nullptr;   // [n_spans] epoch microseconds, or none (edge_windows.hip)
  // Parent rows (edge_agg.hip): the service row of every span's first-match
  // parent, by span position, for the spans inside [rows_lo, rows_hi) =
  // [trace_ptr[0], trace_ptr[n_traces]) — rows_S for a root span, rows_S + 1
  // for an orphan, rows_S = the service count of the aggregation that filled
  // it (a reader with another S maps them to its own S / S + 1; service
  // indices stay below both).  Filled by the set's first grouped aggregation
  // (the id columns and trace_ptr of a resident set never change), complete
  // once rows_done; later aggregations stream svc_flags, dur_us and this
  // column instead of walking the traces.  Allocated on demand (2 B/span); a
  // set that lives for one call (keep_rows = false) never gets one.
  mutable uint16_t* parent_row = nullptr;  // [n_spans]
  mutable bool rows_done = false;
  mutable uint32_t rows_S = 0;
  mutable uint64_t rows_lo = 0, rows_hi = 0;
  bool keep_rows = true;
  // Dense edge stream (edge_agg.hip): layout and span-word column, both
  // functions of the id columns, trace_ptr, svc_flags and the S of the call —
  // none of which a resident set changes (the words also hold dur_us, which it
  // does not change either) — learned from the set's own table.
  // Only a set that streams its parent rows ever gets one.
  mutable std::unique_ptr<anomod::DenseSet> dense;
};

#define ANOMOD_HIP(ctx, expr)                                                               \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      anomod::set_error((ctx), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),      \
                        __FILE__, __LINE__);                                                \
      return ANOMOD_EHIP;                                                                   \
    }                                                                                       \
  } while (0)

#define ANOMOD_RCCL(ctx, expr)                                                              \
  do {                                                                                      \
    ncclResult_t _r = (expr);                                                               \
    if (_r != ncclSuccess) {                                                                \
      anomod::set_error((ctx), "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(_r),     \
                        __FILE__, __LINE__);                                                \
      return ANOMOD_ERCCL;                                                                  \
    }                                                                                       \
  } while (0)

#define ANOMOD_REQUIRE(ctx, cond, ...)                                                      \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      anomod::set_error((ctx), __VA_ARGS__);                                                \
      return ANOMOD_EINVAL;                                                                 \
    }                                                                                       \
  } while (0)

// ANOMOD_REQUIRE for the checks before a collective: instead of returning,
// record the first failure in `local` (passed to comm_agree afterwards, so
// the other ranks learn of it instead of waiting in the collective).
#define ANOMOD_CHECK_LOCAL(ctx, local, cond, ...)                                           \
  do {                                                                                      \
    if ((local) == ANOMOD_OK && !(cond)) {                                                  \
      anomod::set_error((ctx), __VA_ARGS__);                                                \
      (local) = ANOMOD_EINVAL;                                                              \
    }                                                                                       \
  } while (0)

namespace anomod {

// Make ctx's device current on this host thread.
int bind(anomod_ctx* ctx);
// hipEvent bracketing of a stage on the ctx stream.
int stage_begin(anomod_ctx* ctx, Stage s);
int stage_end(anomod_ctx* ctx, Stage s);
// Host wall clock (ms since an arbitrary origin) and the record of a slot.
double host_now_ms();
void host_record(anomod_ctx* ctx, HostSlot s, double ms);
// Wait for the ctx stream.  With a communicator attached, RCCL's async
// error state is polled while waiting and the communicator is aborted on an
// error or after ctx->comm_timeout_s (a dead peer must not hang the rank).
int stream_wait(anomod_ctx* ctx);
// Status agreement before a collective: every rank passes its local status
// (ANOMOD_OK or an error it would otherwise return early with) and gets back
// ANOMOD_OK only when every rank is OK — so either all ranks enter the data
// collective or none does.  A no-op returning local_rc without a communicator.
int comm_agree(anomod_ctx* ctx, int local_rc);
// Collectives on the ctx stream over whichever transport is attached (RCCL,
// or the host callbacks: staged through pinned memory, synchronous).
// comm_attached: a live transport of any kind.  coll_begin / coll_end bracket
// the calls RCCL should issue as one group.
enum CollType { kCollI32 = ANOMOD_DTYPE_I32, kCollU32 = ANOMOD_DTYPE_U32,
                kCollU64 = ANOMOD_DTYPE_U64, kCollF64 = ANOMOD_DTYPE_F64 };
enum CollOp { kCollSum = ANOMOD_OP_SUM, kCollMin = ANOMOD_OP_MIN, kCollMax = ANOMOD_OP_MAX };
bool comm_attached(const anomod_ctx* ctx);
int coll_begin(anomod_ctx* ctx);
int coll_end(anomod_ctx* ctx);
int coll_allreduce(anomod_ctx* ctx, void* dbuf, size_t count, CollType t, CollOp op);
// in place: this rank's block of count_per_rank elements sits at rank * count_per_rank
int coll_allgather(anomod_ctx* ctx, void* dbuf, size_t count_per_rank, CollType t);
// Trace cut points 0 = c_0 < ... < c_k = n_traces of a span set such that
// every range [c_i, c_{i+1}) holds at most max_spans spans or is a single
// trace (kernels with per-workgroup u32 counters launch once per range).
// 2^32 - 1, or ANOMOD_MAX_LAUNCH_SPANS (tests: forces the multi-launch path).
uint64_t max_launch_spans();
int span_launch_cuts(anomod_ctx* ctx, const anomod_spans* s, uint64_t max_spans,
                     std::vector<uint64_t>& cuts);
// Span-set storage (synth.hip): every array of a set of n_spans spans /
// n_traces traces (trace_hash optional), and its release.
int alloc_spans(anomod_ctx* ctx, uint64_t n_spans, uint64_t n_traces, bool with_hash,
                anomod_spans** out);
void free_spans(anomod_spans* s);
// Trace-grouping workspace (group.hip), released with the ctx.
void free_group_ws(anomod_ctx* ctx);
// Host -> device copies through the pinned staging pipeline (upload.hip);
// *max_svc = the largest service index a kind-1 item packed.  Returns after
// every copy landed.  free_uploader releases the pipeline with the ctx.
int upload_items(anomod_ctx* ctx, const UpItem* items, int n_items, uint32_t* max_svc);
void free_uploader(anomod_ctx* ctx);
// Edge table of n per-span edge records (the fused ungrouped aggregation:
// (parent row * S + service) << 33 | error << 32 | duration, csrc/bucket.hip;
// a record of all ones is no span and is skipped: critical_path.hip writes it
// for the spans off the path) into `out`, merged over an attached
// communicator; *hist_form is the set's
// histogram-form hint (read, and updated with what the run learned).
int edge_aggregate_records(anomod_ctx* ctx, const uint64_t* rec, uint64_t n, uint32_t S,
                           int8_t* hist_form, anomod_edge_table* out);
// Per-span edge keys of a grouped set (edge_agg.hip): keys[i] = edge row << 32
// | dur_us by span position, from the aggregation kernels' own walk and parent
// rule (order probe, chunk walk per launch cut, long-trace pass), queued on
// the ctx stream.  ws: device words the walk uses, span_edge_keys_ws_bytes
// of them, 8-B aligned.
size_t span_edge_keys_ws_bytes(const anomod_spans* s);
// use_rows: a set that holds its parent rows (anomod_spans::parent_row) gets
// the keys from the row stream instead (the exact edge quantiles).
int span_edge_keys(anomod_ctx* ctx, const anomod_spans* s, uint32_t S, unsigned long long* keys,
                   unsigned long long* ws, bool use_rows = false);
// Whether the set holds complete parent rows a call may stream now
// (anomod_spans::parent_row filled, none of the walk overrides of edge_agg.hip
// set): positions [rows_lo, rows_hi), codes rows_S / rows_S + 1 for root / orphan.
bool span_rows_ready(const anomod_spans* s);
// The parent scan the edge kernels use for a grouped set (edge_agg.hip):
// *unique = the scans from both ends apply (ids declared unique, collector
// order).  An unknown order hint is probed first, as at the set's first
// aggregation (d_cnt: two device words; one small kernel and a host wait).
int span_scan_choice(anomod_ctx* ctx, const anomod_spans* s, unsigned long long* d_cnt,
                     bool* unique);
// Grow-only device workspace owned by the ctx.
int ensure_table(anomod_ctx* ctx, size_t bytes);
enum ScratchSlot { kScratchQuantiles = 0, kScratchTraceStruct = 1, kScratchTsLong = 2,
                   kScratchUpload = 3, kScratchEdgeWindows = 4, kNumScratch = 5 };
// *out = the slot's block of at least `bytes` (grown when smaller; on
// failure the slots outside `keep` (a mask; this slot is always kept) are
// released and the allocation retried once).
int ensure_scratch(anomod_ctx* ctx, ScratchSlot slot, size_t bytes, void** out,
                   unsigned keep = 0u);
// Frees every scratch slot whose bit is clear in `keep`.  Returns the bytes freed.
size_t release_scratch(anomod_ctx* ctx, unsigned keep = 0u);
// hipMalloc with one retry after the ctx's scratch was released.
hipError_t dev_malloc(anomod_ctx* ctx, void** p, size_t bytes);
int ensure_host_stage(anomod_ctx* ctx, size_t bytes);

// (hist_bin / hist_bounds and the span-word formats: span_word.h)

}  // namespace anomod
