/*
 * anomod.h — C ABI of the MI355X-native AnoMod RCA-feature engine (libanomod.so).
 *
 * The reference (EvoTestOps/AnoMod, /root/reference) has no FFI: its hot path is
 * a CLI + file boundary driven by bash.  Each entry point below
 * names the reference code it replaces (path:line relative to the reference
 * root).  Everything is `extern "C"`, plain pointers and sizes; no torch types.
 *
 * Conventions
 *  - Every function returns an int status: ANOMOD_OK (0) or a negative code; a
 *    human-readable message is available from anomod_last_error(ctx) (or
 *    anomod_last_error(NULL) for errors raised before a ctx exists).
 *  - Host buffers are caller-owned; no pointer is retained after a call
 *    returns and inputs are never mutated (unlike trace_collector.py:415, which
 *    mutates the span dicts it is handed).
 *  - Empty input (n == 0) is not an error: outputs are zero/empty tables and
 *    status is ANOMOD_OK (mirrors jaeger_to_csv.py:92-97, which writes a
 *    header-only CSV and exits 0).
 *  - One ctx per host thread; a ctx owns one HIP device, one stream and,
 *    optionally, one RCCL communicator.
 */
#ifndef ANOMOD_H
#define ANOMOD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANOMOD_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------- */
#define ANOMOD_OK 0
#define ANOMOD_EINVAL (-1)  /* bad argument / shape                           */
#define ANOMOD_EHIP (-2)    /* HIP runtime error (no device, launch failure)  */
#define ANOMOD_ERCCL (-3)   /* RCCL error                                     */
#define ANOMOD_ENOMEM (-4)  /* device or host allocation failed               */
#define ANOMOD_ESTATE (-5)  /* call not valid in this state                   */

/* ---- span flags (anomod_span_soa.flags) --------------------------------- */
/* Error bit.  SN/Jaeger: tags["error"] == true or http.status_code >= 500
 * (tags kept at jaeger_to_csv.py:55-67,88).  TT/SkyWalking: isError
 * (trace_collector.py:471).                                                 */
#define ANOMOD_FLAG_ERROR 0x1u

/* ---- latency histogram (build-defined) ---------------
 * Integer log-linear ("HDR") binning of a u32 microsecond latency v:
 *   v <  64 : bin = v                                 (exact)
 *   v >= 64 : e = floor(log2 v) - 5 ; bin = 32*e + (v >> e)
 * 32 sub-buckets per octave (<= 3.1 % relative bin width), 896 bins cover the
 * whole u32 range.                                                          */
#define ANOMOD_HIST_SUB_BITS 5
#define ANOMOD_HIST_BINS 896

/* ---- edge table layout ---------------------------------------------------
 * For S services the table has E = (S + 2) * S rows; row = p * S + c where c
 * is the child span's service and p is the parent span's service, or
 *   p == S     : ROOT   — the span carries no parent reference
 *                (jaeger_to_csv.py:34-38 leaves parent_span_id = '';
 *                 trace_collector.py:427-437 yields parent_node None)
 *   p == S + 1 : ORPHAN — a parent reference that names no span of the same
 *                trace (trace_collector.py:443 counts these among the roots). */
#define ANOMOD_ROOT_ROWS 2

typedef struct anomod_ctx anomod_ctx;       /* device + stream + comm      */
typedef struct anomod_spans anomod_spans;   /* device-resident span set    */
typedef struct anomod_series anomod_series; /* device-resident metric matrix */
typedef struct anomod_graph anomod_graph;   /* device-resident CSR graph   */

/* Span set in struct-of-arrays form, grouped by trace: the spans of trace t
 * are [trace_ptr[t], trace_ptr[t+1]).  span_id 0 is reserved; a
 * parent_span_id of 0 means "no parent reference".  Collectors already emit
 * spans grouped by trace (jaeger_to_csv.py:21-32 iterates trace -> spans;
 * trace_collector.py:539-546 emits per-trace span lists).                   */
typedef struct {
  const uint64_t* trace_hash;      /* [n] shard key (may be NULL)          */
  const uint64_t* span_id;         /* [n]                                  */
  const uint64_t* parent_span_id;  /* [n]                                  */
  const uint16_t* svc;             /* [n] service index (< n_services)     */
  const uint16_t* flags;           /* [n] ANOMOD_FLAG_*                    */
  const uint32_t* dur_us;          /* [n] latency in microseconds          */
} anomod_span_soa;

/* Writable twin of anomod_span_soa (download / host generation targets). */
typedef struct {
  uint64_t* trace_hash;
  uint64_t* span_id;
  uint64_t* parent_span_id;
  uint16_t* svc;
  uint16_t* flags;
  uint32_t* dur_us;
} anomod_span_soa_out;

/* Per-edge aggregate.  Every pointer may be NULL (that output is skipped).
 * Arrays have E = (n_services + 2) * n_services rows; hist has E * n_bins. */
typedef struct {
  uint32_t n_services;  /* in : S                                         */
  uint32_t n_bins;      /* in : must equal ANOMOD_HIST_BINS               */
  uint64_t* count;      /* [E] spans on the edge                          */
  uint64_t* errors;     /* [E] spans with ANOMOD_FLAG_ERROR               */
  uint64_t* sum_us;     /* [E] sum of latencies                           */
  uint32_t* min_us;     /* [E] UINT32_MAX when count == 0                 */
  uint32_t* max_us;     /* [E] 0 when count == 0                          */
  uint64_t* hist;       /* [E * n_bins] latency histogram                 */
  double* p50_us;       /* [E] histogram quantile, rank (n*50)//100       */
  double* p99_us;       /* [E] histogram quantile, rank (n*99)//100       */
} anomod_edge_table;

/* ---- library / context ---------------------------------------------------*/
int anomod_abi_version(void);
const char* anomod_last_error(const anomod_ctx* ctx);
int anomod_device_count(int* out);
int anomod_ctx_create(int device, anomod_ctx** out);
int anomod_ctx_destroy(anomod_ctx* ctx);
int anomod_ctx_synchronize(anomod_ctx* ctx);
/* Milliseconds of the last launch of a stage, measured with hipEvents on the
 * ctx stream.  stage: 0 = edge aggregation kernel, 1 = edge finalize kernel,
 * 2 = edge all-reduce, 3 = ewma kernel, 4 = pagerank iterations,
 * 5 = trace-structure kernel, 6 = segment-summary kernel,
 * 7 = value summary (select + sort + sum + picks),
 * 8 = trace grouping of an ungrouped span set (radix passes + copy + trace_ptr),
 * 9 = edge-window pass (per-span edge keys + the window kernel),
 * 10 = the window kernel of stage 9 alone,
 * 11 = edge-load pass (keys form: per-span edge keys; the stream kernel; the
 *      scan), 12 = its stream kernel alone, 13 = its scan alone,
 * 14 = edge-exemplars pass (keys form: per-span edge keys; the stream kernel;
 *      the gather), 15 = its stream kernel alone,
 * 16 = series-correlation kernel.                                           */
int anomod_ctx_stage_ms(const anomod_ctx* ctx, int stage, double* ms);
/* Host wall milliseconds of the last occurrence of a one-off setup step or of
 * a call phase the stage events above cannot see, and how many times it
 * happened on this ctx (count may be NULL; a caller compares counts around a
 * call to learn whether that call paid it).  Slots: */
#define ANOMOD_HOST_GROUP_ALLOC 0  /* grouping workspace: device hipMalloc     */
#define ANOMOD_HOST_GROUP_PINNED 1 /* grouping workspace: pinned read-back     */
#define ANOMOD_HOST_GROUP_WALL 2   /* an ungrouped aggregation's grouping:
                                      first launch to counters read back       */
#define ANOMOD_HOST_UPLOAD_SETUP 3 /* upload pipeline: threads, streams, pinned
                                      buffers                                  */
#define ANOMOD_HOST_SET_ALLOC 4    /* the device set anomod_edge_aggregate_host
                                      keeps: (re)allocation                    */
#define ANOMOD_HOST_SLOTS 5
int anomod_ctx_host_ms(const anomod_ctx* ctx, int slot, double* ms, uint64_t* count);

/* ---- histogram helpers (host) ------------------------------------------- */
uint32_t anomod_hist_bin(uint32_t v);
int anomod_hist_bin_bounds(uint32_t bin, uint32_t* lo, uint32_t* hi);

/* ---- span sets -----------------------------------------------------------*/
/* Span ids unique within every trace: the producer's declaration (the
 * synthetic generator sets it by construction; the native decoders report it
 * per decoded document, anomod_decoded_unique_ids).  With it, parent
 * lookups may stop at the nearest match from either end of the trace (any
 * match is the first match).  Declaring it for a set that holds a duplicated
 * id inside a trace gives unspecified parents for those spans.  Default 0
 * (unknown: the first-match scan).  Grouping and shuffling keep it.         */
int anomod_spans_set_unique_ids(anomod_spans* spans, int unique);
int anomod_spans_unique_ids(const anomod_spans* spans, int* unique);
/* Order hint of a unique-id set (a performance hint the library keeps):
 * 1 = collector order, most child spans right after their parent (the
 * bidirectional scan from the trace start and from the span pays off);
 * 0 = not (e.g. spans shuffled inside their traces: the forward scan);
 * -1 = not known yet — the first aggregation probes the set's first 2^20
 * spans on the device.  Generated sets are 1; results never depend on it.   */
int anomod_spans_scan_order(const anomod_spans* spans, int* order);
/* 1 once an aggregation of this set overflowed the workgroups' 8 Ki-slot
 * (pair-form) LDS histogram: its later aggregations use the 16 Ki packed-slot
 * (compact) form (same results; a performance hint the library keeps).     */
int anomod_spans_hist_compact(const anomod_spans* spans, int* compact);
/* Both hints of a set, for callers that keep a span set on the host and
 * upload it per call (the Python SpanSet does): *scan_order as
 * anomod_spans_scan_order; *hist_form 0 = pair, 1 = compact, -1 = not known
 * yet (the aggregation starts in the pair form and a workgroup whose table
 * saturates hands its remaining traces to a compact-form launch — no
 * first-call cliff either way).  set_hints puts learned values on a freshly
 * uploaded set (each in [-1, 1]); results never depend on them.           */
int anomod_spans_hints(const anomod_spans* spans, int* scan_order, int* hist_form);
int anomod_spans_set_hints(anomod_spans* spans, int scan_order, int hist_form);
/* Diagnostic: the parent rows a resident grouped set keeps once its first
 * anomod_edge_aggregate_spans has run — per span position, the service index
 * of the span's first-match parent inside its trace, n_services for a root
 * span (parent reference 0), n_services + 1 for an orphan (reference not in
 * the trace) — copied to out_host[n_spans]; positions outside every trace
 * read 0xFFFF.  Later aggregations and anomod_edge_quantiles_exact of the
 * set read this column (2 B/span of HBM, allocated by that first call; a
 * failed allocation only leaves the set without it) instead of resolving the
 * parents again; unique ids, hints and start times do not affect it.
 * ANOMOD_ESTATE when the set holds none: no aggregation yet, a call run with
 * ANOMOD_PARENT_ROWS=0 / ANOMOD_HIST_FORM / ANOMOD_UNIQUE_SCAN set, an
 * ungrouped set, or the column could not be allocated.
 * A set that streams its rows may also keep a second derived column, the u32
 * span words of the dense stream (edge code, error bit and duration of every
 * span position; 4 B/span more, written by the set's fifth
 * aggregation at a service count when the edges and histogram bins its first
 * table touched fit a directly indexed LDS histogram: at most 512 edges with
 * spans and 32 Ki bins in their ranges); its aggregations from the sixth on
 * then read that column alone, 4 B/span (a duration that does not fit a
 * word's 21-bit field is read from dur_us).  Same tables bit for bit;
 * ANOMOD_EDGE_DENSE=0 switches it off, everything that bypasses the rows
 * bypasses it, and this column keeps its encoding and every other reader.   */
int anomod_spans_parent_rows(anomod_ctx* ctx, const anomod_spans* spans, uint16_t* out_host,
                             uint32_t n_services);
/* Copy a host span set to HBM.  Replaces the in-memory hand-off between
 * json.load and the per-span loop of jaeger_to_csv.py:12-32 /
 * trace_collector.py:519-531.                                              */
int anomod_spans_upload(anomod_ctx* ctx, const anomod_span_soa* soa, uint64_t n_spans,
                        const uint64_t* trace_ptr, uint64_t n_traces, anomod_spans** out);
int anomod_spans_info(const anomod_spans* spans, uint64_t* n_spans, uint64_t* n_traces);
int anomod_spans_download(anomod_ctx* ctx, const anomod_spans* spans,
                          const anomod_span_soa_out* dst, uint64_t* trace_ptr);
int anomod_spans_free(anomod_spans* spans);
/* Optional start-time column of a set: epoch microseconds per span, by span
 * position (Jaeger startTime, jaeger_to_csv.py:41-43; SkyWalking
 * start_timestamp_ms * 1000) — the time axis of anomod_edge_windows_spans.
 * A set has none until set_start_us / fill_start_synthetic gives it one, and
 * the sets made by anomod_spans_group, anomod_spans_shuffle and
 * anomod_spans_generate carry none (a regrouped copy does not inherit it).
 * get_start_us: ANOMOD_ESTATE when the set has none.                        */
int anomod_spans_set_start_us(anomod_ctx* ctx, anomod_spans* spans,
                              const uint64_t* start_us /* [n_spans], host */);
int anomod_spans_has_start_us(const anomod_spans* spans, int* has);
int anomod_spans_get_start_us(anomod_ctx* ctx, const anomod_spans* spans, uint64_t* dst);
/* Synthetic start times, generated on the device (grouped sets only): span i
 * at position pos of trace t gets
 *   t0_us + (t * period_us) / n_traces + pos * gap_us
 * (u64 arithmetic) — traces spread evenly over one period, in order.
 * ANOMOD_EINVAL unless n_traces * period_us < 2^63.                         */
int anomod_spans_fill_start_synthetic(anomod_ctx* ctx, anomod_spans* spans, uint64_t t0_us,
                                      uint64_t period_us, uint64_t gap_us);

/* ---- ungrouped span sets (BASELINE.json north_star (2)) ------------------
 * Spans that arrive interleaved across traces — the Elasticsearch path of
 * enhanced_trace_collector.py:80-90,109-110 pulls sw_segment-* hits sorted by
 * start_time over all traces — carry their trace only in trace_hash (equal
 * hash = same trace).  anomod_spans_group groups them on the device with a
 * segmented radix sort: traces ordered by mix64(trace_hash) ascending (the
 * SplitMix64 finaliser), the spans of a trace in arrival order (stable), so
 * every grouped-set kernel then sees each trace's spans in the order they
 * arrived (first-match parent rule, trace_collector.py:424-443).            */
int anomod_spans_upload_ungrouped(anomod_ctx* ctx, const anomod_span_soa* soa, uint64_t n_spans,
                                  anomod_spans** out);
int anomod_spans_grouped(const anomod_spans* spans, int* grouped);
int anomod_spans_group(anomod_ctx* ctx, const anomod_spans* ungrouped, anomod_spans** grouped);
/* How the ctx's last grouping ran (csrc/group.hip, csrc/bucket.hip):
 * *path = 1 bucket path (two stable MSD scatters over the top *bits bits of
 * mix64(trace_hash), then one workgroup per bucket), 2 the same scatters then
 * the per-bucket hash join of anomod_edge_aggregate_ungrouped (edge records,
 * no grouped columns), 0 LSD path (8-bit radix passes + bucket fix-up);
 * *levels = scatter levels / radix passes run;
 * *bits = bucket bits (bucket path) or 8 * passes.  All 0 before any grouping. */
int anomod_ctx_group_info(const anomod_ctx* ctx, int* path, int* levels, int* bits);
/* Size the ctx's grouping workspace (grow-only, kept until the ctx is
 * destroyed) for sets of up to n_spans spans ahead of their first
 * aggregation: ~58 B per span for the ungrouped aggregation's join path,
 * + 32 B with both_records (grouping into columns, the LSD path).  A
 * workspace of tens of GB can take seconds to obtain from the driver when
 * the memory it gets was in use earlier in the process; reserving it when the
 * set is made keeps that out of the aggregation call.  Context.upload_ungrouped
 * and Context.shuffle (interleaving) in the Python package reserve for the
 * set they return.                                                         */
int anomod_ctx_reserve_grouping(anomod_ctx* ctx, uint64_t n_spans, int both_records);
/* Rearranged copies of a grouped set (synthetic arrival orders for tests
 * and benchmarks): window_traces = 0 shuffles the spans inside every trace
 * (the result stays grouped); window_traces = W interleaves the spans of
 * every W consecutive traces in a random order (the result is ungrouped).  */
int anomod_spans_shuffle(anomod_ctx* ctx, const anomod_spans* grouped, uint64_t seed,
                         uint64_t window_traces, anomod_spans** out);

/* ---- synthetic workload ----------------------*/
#define ANOMOD_TOPO_SN 0 /* DeathStarBench SocialNetwork, 12 services        */
#define ANOMOD_TOPO_TT 1 /* TrainTicket, 46 services                         */
#define ANOMOD_TOPO_LONG 2 /* SN services, traces of 16..4000 spans (stress) */

typedef struct {
  uint32_t topology;          /* ANOMOD_TOPO_*                               */
  uint32_t fault_service;     /* service index with an injected fault, or
                                 UINT32_MAX for a normal run                 */
  uint64_t seed;              /* Philox4x32-10 key                           */
  uint32_t fault_latency_mult;/* latency multiplier on the faulty service    */
  uint32_t p_error_ppm;       /* base error probability (parts per million)  */
  uint32_t p_fault_error_ppm; /* error probability on the faulty service     */
  uint32_t p_orphan_ppm;      /* probability a non-root span loses its parent*/
} anomod_synth_spec;

int anomod_synth_n_services(uint32_t topology, uint32_t* out);
/* Service name of index i (sorted-name order, cf. trace_collector.py:536). */
const char* anomod_synth_service_name(uint32_t topology, uint32_t i);
/* Host generation (same code path as the device generator): first count the
 * spans of traces [0, n_traces) of shard `shard`, then fill caller buffers.
 * dst arrays have n_spans entries, trace_ptr has n_traces + 1.             */
int anomod_synth_count_host(const anomod_synth_spec* spec, uint64_t shard, uint64_t n_traces,
                            uint64_t* n_spans);
int anomod_synth_generate_host(const anomod_synth_spec* spec, uint64_t shard, uint64_t n_traces,
                               const anomod_span_soa_out* dst, uint64_t* trace_ptr);
/* Device generation straight into HBM (no PCIe), bit-identical to host.    */
int anomod_spans_generate(anomod_ctx* ctx, const anomod_synth_spec* spec, uint64_t shard,
                          uint64_t n_traces, anomod_spans** out);

/* ---- native trace-file decoders --------------------
 * Parse a whole file image (caller's bytes, UTF-8 JSON) into span columns
 * without a Python object per span:
 *   anomod_decode_jaeger      Jaeger /api/traces dump (all_traces.json), the
 *                             columns jaeger_to_csv.py:21-90 derives
 *   anomod_decode_skywalking  trace_collector.py collector payload
 *                             ({metadata, traces:[{summary, spans}]}, :564-578)
 * services (may be NULL): the service-name list to index against; NULL =
 * the sorted distinct names of the file.  Ids: Jaeger spanIDs of 1-16 hex
 * digits are their value, other ids xxh64 | 2^63; SkyWalking node ids become
 * dense per-trace ids (first occurrence + 1; a parent naming no node of the
 * trace = UINT64_MAX).  trace_hash = xxh64 of the trace id.                 */
typedef struct anomod_decoded anomod_decoded;
int anomod_decode_jaeger(const char* json, uint64_t len, const char* const* services,
                         uint32_t n_services, anomod_decoded** out);
int anomod_decode_skywalking(const char* json, uint64_t len, const char* const* services,
                             uint32_t n_services, anomod_decoded** out);
int anomod_decoded_info(const anomod_decoded* d, uint64_t* n_spans, uint64_t* n_traces,
                        uint32_t* n_services);
/* *unique = 1 when no trace of the document holds a span id twice (checked
 * exactly while decoding: Jaeger spanIDs after their id mapping, SkyWalking
 * node ids), else 0 — what anomod_spans_set_unique_ids takes.              */
int anomod_decoded_unique_ids(const anomod_decoded* d, int* unique);
const char* anomod_decoded_service(const anomod_decoded* d, uint32_t i);
int anomod_decoded_columns(const anomod_decoded* d, const anomod_span_soa_out* dst,
                           uint64_t* trace_ptr /* [n_traces + 1] */);
/* Start time of every span in epoch microseconds: Jaeger startTime, SkyWalking
 * start_timestamp_ms * 1000; 0 when the value is missing, negative, not an
 * integer, or does not fit a u64.                                          */
int anomod_decoded_start_us(const anomod_decoded* d, uint64_t* dst /* [n_spans] */);
int anomod_decoded_free(anomod_decoded* d);
/* The 64-bit id hash of the decoders (xxh64, seed 0; 0 maps to 1).       */
uint64_t anomod_hash64(const char* s, uint64_t len);

/* ---- native metric-file decoders --------------
 * Prometheus CSVs -> the time-major series matrix X[T][S] (f32, NaN = no
 * sample) the EWMA/z kernels read:
 *   anomod_decode_metric_long_csv   TT long CSV of metric_collector.py:400-478
 *                                   (series = (metric_name, sorted non-empty
 *                                   labels); rows de-duplicated on (series,
 *                                   timestamp), first kept, :420-423)
 *   anomod_decode_prometheus_csvs   SN metric directory, one CSV per query as
 *                                   fetch_prometheus_metrics.py:47-67,99 writes
 *                                   it (series = (file stem, 'metric' label
 *                                   string); naive datetimes read as local time)
 * Timestamps are the sorted distinct values of all rows; series are sorted
 * by (name, labels).  The same rules as anomod/decode.py's Python decoders. */
typedef struct anomod_metrics anomod_metrics;
int anomod_decode_metric_long_csv(const char* data, uint64_t len, anomod_metrics** out);
/* the same from a file path (mapped, not read; pieces faulted in by the
 * parser threads) */
int anomod_decode_metric_long_csv_file(const char* path, anomod_metrics** out);
int anomod_decode_prometheus_csvs(const char* const* data, const uint64_t* lens,
                                  const char* const* stems, uint32_t n_files,
                                  anomod_metrics** out);
int anomod_metrics_info(const anomod_metrics* m, uint64_t* T, uint64_t* S);
int anomod_metrics_matrix(const anomod_metrics* m, float* X /* [T][S] */,
                          double* timestamps /* [T] */);
const char* anomod_metrics_series_name(const anomod_metrics* m, uint64_t s);
uint32_t anomod_metrics_series_nlabels(const anomod_metrics* m, uint64_t s);
const char* anomod_metrics_series_label(const anomod_metrics* m, uint64_t s, uint32_t j,
                                        const char** value);
/* every series at once: name \0 (label name \0 label value \0) x nlabels[s],
 * series after series; *bytes = the size needed.  buf == NULL or cap < *bytes
 * writes nothing but *bytes (and nlabels, when given: [S]). */
int anomod_metrics_series_packed(const anomod_metrics* m, char* buf, uint64_t cap,
                                 uint32_t* nlabels, uint64_t* bytes);
int anomod_metrics_free(anomod_metrics* m);

/* ---- edge aggregation (the hot path) -------------------------------------
 * Call-graph edge table with per-edge latency histogram, count, errors,
 * sum/min/max and p50/p99.  Replaces and extends the per-span loops of
 * jaeger_to_csv.py:21-90 (parent = first CHILD_OF ref, service from
 * processID) and trace_collector.py:401-481 (_build_span_records parent
 * resolution) + the per-service aggregation of
 * enhanced_trace_collector.py:216-296.  Integer results are bit-exact and
 * independent of launch geometry, shard count and span order within a trace
 * set.  When a communicator is attached the table is summed over all ranks
 * (RCCL all-reduce) before quantiles are taken.                            */
int anomod_edge_aggregate_spans(anomod_ctx* ctx, const anomod_spans* spans, uint32_t n_services,
                                anomod_edge_table* out);
/* Edge table of a host span set grouped by trace (trace_ptr), in one call:
 * the columns go to a device set the ctx keeps and regrows only when a
 * larger set comes (no trace_hash: the aggregation reads none) through the
 * pinned staging pipeline (worker threads pack svc|flags into pinned
 * buffers, several DMA streams), then anomod_edge_aggregate_spans.  The
 * set's hints (anomod_spans_hints) go in through *scan_order / *hist_form
 * and come back with what the call learned; unique_ids as
 * anomod_spans_set_unique_ids.  The product path's one conversion per
 * experiment (collect_trace.sh:70: each dump is converted once, then every
 * feature comes from it).                                                  */
int anomod_edge_aggregate_host(anomod_ctx* ctx, const anomod_span_soa* soa, uint64_t n_spans,
                               const uint64_t* trace_ptr, uint64_t n_traces, uint32_t n_services,
                               int unique_ids, int* scan_order, int* hist_form,
                               anomod_edge_table* out);
/* Edge table of an ungrouped set; a grouped set is aggregated as is.  By
 * default the set is bucketed by trace (the grouping's two scatter levels) and
 * each bucket finds its spans' parents by an LDS hash join on (trace, span id),
 * writing one edge record per span that the table is taken from (no grouped
 * columns).  A set whose buckets hold several traces of thousands of spans,
 * or ANOMOD_UNGROUPED_FUSED=0, takes group (anomod_spans_group, into a
 * workspace the ctx keeps) then aggregate.  Same table either way. */
int anomod_edge_aggregate_ungrouped(anomod_ctx* ctx, const anomod_spans* spans,
                                    uint32_t n_services, anomod_edge_table* out);
/* Exact per-edge order statistics (SURVEY.md §8a a11 cross-check mode): the
 * same per-span edges as the aggregation, one radix sort of (edge, latency)
 * keys, then per edge x[int(c * q)] of its sorted latencies with q the double
 * q_pct[k] / 100.0 and the product truncated — the reference's
 * sorted(x)[int(n*q)] for any q_pct (monitor_http_responses.py:180-190).
 * out: [E][nq] doubles (NaN for an empty edge); count: [E] (may be NULL).
 * Needs a grouped set of at most 2^32 - 4097 spans (one sort); q_pct[k] in
 * [0, 99], nq <= 16.                                                        */
int anomod_edge_quantiles_exact(anomod_ctx* ctx, const anomod_spans* spans, uint32_t n_services,
                                const uint32_t* q_pct, uint32_t nq, double* out, uint64_t* count);
/* Per-window edge table of a grouped set with a start-time column: the edge
 * of a span is the row anomod_edge_aggregate_spans puts it in, its window
 *   w = (start_us - t0_us) / step_us   (integer floor)
 * and cell w * E + row accumulates count, errors, latency sum and max.  A
 * span with start_us < t0_us or w >= n_windows is counted in `outside` and
 * in no cell.  Every result is an integer, bit-exact for any launch
 * geometry.  A set without a start column gives ANOMOD_ESTATE; n == 0 gives
 * zeros.  The call is rank-local: no collective runs even with a
 * communicator attached (the cells are integers: a caller sums the ranks'
 * tables itself, max for max_us).                                          */
typedef struct {
  uint32_t n_services;   /* in : S; E = (S + 2) * S as in anomod_edge_table      */
  uint32_t n_windows;    /* in : T in [1, 65536], T * E <= 2^24, else EINVAL      */
  uint64_t t0_us;        /* in                                                   */
  uint64_t step_us;      /* in : >= 1                                            */
  uint64_t* count;       /* [T * E], cell = w * E + edge row; each may be NULL   */
  uint64_t* errors;
  uint64_t* sum_us;
  uint32_t* max_us;      /* 0 for an empty cell                                  */
  uint64_t outside;      /* out: spans with start < t0 or start >= t0 + T * step */
} anomod_edge_windows;
int anomod_edge_windows_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_edge_windows* out);
/* Edge load of a grouped set with a start-time column: per (window, edge row)
 * the time the edge's calls were open inside the window and the calls still
 * open when the window opens — the saturation signal the start-window tables
 * above cannot carry (they book a call in the window it starts in only).
 * Rows, inputs and the "in traces" rule are those of
 * anomod_edge_windows_spans: S, E = (S + 2) * S, T = n_windows in [1, 65536]
 * with T * E <= 2^24, t0_us, step_us >= 1.  All integers.  For a span i at a
 * position inside [trace_ptr[0], trace_ptr[n_traces]):
 *   s = start_us[i],  e = min(s + dur_us[i], 2^64 - 1)   (saturating add)
 *   window w = [lo_w, hi_w) = [t0 + w * step, t0 + (w + 1) * step), evaluated
 *   as if in unbounded integers (t0 + T * step may pass 2^64)
 * and with cell = w * E + row, row = the edge row the aggregation puts the
 * span in:
 *   busy_us[cell] = sum over the row's spans of max(0, min(e, hi_w) - max(s, lo_w))
 *                   (busy_us / step_us = the mean number of calls in flight)
 *   carried[cell] = the row's spans with s < lo_w < e: open when the window
 *                   opens (a span that starts exactly at lo_w is that
 *                   window's arrival, not carried into it)
 *   outside       = the spans in traces that add to no cell of either table:
 *                   dur == 0, e <= t0, or s >= t0 + T * step (and a start
 *                   of 2^64 - 1, where e saturates onto s)
 * A span that starts before t0 but reaches into the range is clipped, not
 * dropped — deliberately unlike `outside` of anomod_edge_windows_spans.
 * Spans outside every trace are in no cell and not in `outside`.  busy_us
 * cannot overflow (fewer than 2^32 spans a call, each shorter than 2^32 us);
 * both tables are additive over any split of the traces, and the call is
 * rank-local: no collective runs even with a communicator attached.  Every
 * result is bit-exact for any launch geometry.  The work per span does not
 * depend on how many windows it covers (difference tables and one scan along
 * w).  A set that holds its parent rows (a resident set after its first
 * aggregation) is read as one stream of 18 B a span; any other grouped set
 * takes its edges from the aggregation's walk first.  The call neither fills
 * the row column nor changes the set's hints beyond what
 * anomod_edge_windows_spans does.  Validation and error codes are those of
 * anomod_edge_windows_spans (ANOMOD_ESTATE without a start column); n == 0
 * gives zeros; a NULL table is skipped.                                      */
typedef struct {
  uint32_t n_services;   /* in : S; E = (S + 2) * S as in anomod_edge_table      */
  uint32_t n_windows;    /* in : T in [1, 65536], T * E <= 2^24, else EINVAL      */
  uint64_t t0_us;        /* in                                                   */
  uint64_t step_us;      /* in : >= 1                                            */
  uint64_t* busy_us;     /* [T * E], cell = w * E + edge row; may be NULL        */
  uint64_t* carried;     /* [T * E]; may be NULL                                 */
  uint64_t outside;      /* out                                                  */
} anomod_edge_load;
int anomod_edge_load_spans(anomod_ctx* ctx, const anomod_spans* spans, anomod_edge_load* out);
/* Windows per segment of the edge-load scan along w (tests place T at its
 * borders).                                                                 */
uint32_t anomod_edge_load_scan_segment(void);
/* Edge exemplars of a grouped set: the K slowest calls of every edge row, to
 * be carried back to their traces (SpanSet.trace_ids / select_traces).  All
 * values are integers and exact.  Rows, the "in traces" rule and the edge of
 * a span are those of anomod_edge_aggregate_spans / anomod_edge_load_spans:
 * S, E = (S + 2) * S.  For every edge row e, take the spans of that row at
 * positions inside [trace_ptr[0], trace_ptr[n_traces]); when which == 1, only
 * those with ANOMOD_FLAG_ERROR.  Order them by dur_us descending, then by span
 * position ascending: the first min(K, number of such spans) are the row's
 * exemplars, in that order, in slots e * K .. e * K + n_found[e] - 1; the
 * row's other slots are unused.  Ties are part of the contract: they are
 * decided by position, never by arrival, so the result is a pure function of
 * the set — it does not depend on launch geometry, workgroup count, the form
 * the kernel takes or how its atomics interleave.  dur_us of a row's first
 * slot is the row's max_us.  Every output pointer may be NULL.  A start
 * column is not required (start_us is 0 without one).  Validation, error
 * codes and texts are those of anomod_edge_load_spans where they overlap
 * (grouped set, device, max_svc < S, S in [1, 4096]); n == 0 gives zeros and
 * the unused-slot values.  At most 2^32 - 2 spans in traces a call, else
 * ANOMOD_EINVAL.  A set that holds its parent rows is read as one stream of
 * 10 B a span; any other grouped set takes its edges from the aggregation's
 * walk first.  The call is rank-local (a caller merges the ranks' lists by
 * (dur_us descending, rank, position)) and neither fills the row column nor
 * changes the set's hints beyond what anomod_edge_load_spans does.          */
typedef struct {
  uint32_t n_services;  /* in : S, E = (S + 2) * S                                  */
  uint32_t k;           /* in : K in [1, 64], E * K <= 2^24, else EINVAL             */
  uint32_t which;       /* in : 0 every span, 1 spans with ANOMOD_FLAG_ERROR; else EINVAL */
  uint32_t* n_found;    /* [E]     min(K, qualifying spans of the row)               */
  uint64_t* position;   /* [E * K] span position; 2^64 - 1 in an unused slot         */
  uint64_t* trace;      /* [E * K] t with trace_ptr[t] <= position < trace_ptr[t+1]; */
                        /*         2^64 - 1 unused                                   */
  uint64_t* span_id;    /* [E * K] 0 unused                                          */
  uint32_t* dur_us;     /* [E * K] 0 unused                                          */
  uint16_t* flags;      /* [E * K] 0 unused                                          */
  uint64_t* start_us;   /* [E * K] 0 unused or when the set has no start column      */
} anomod_edge_exemplars;
int anomod_edge_exemplars_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                anomod_edge_exemplars* out);
/* Per-window edge latency quantiles of a grouped set with a start-time
 * column: the rows and the window rule of anomod_edge_windows_spans (a span
 * outside [0, n_windows) is counted in `outside` and lies in no cell; a span
 * at a position outside [trace_ptr[0], trace_ptr[n_traces]) lies in no cell
 * and is not counted).  For cell w * E + row holding c spans with sorted
 * latencies x[0..c):
 *   count[cell]         = c
 *   q_us[cell * nq + k] = x[(u64)((double)c * ((double)q_pct[k] / 100.0))]
 * — the index rule of anomod_edge_quantiles_exact, the reference's
 * sorted(x)[int(n*q)] — and 0 in every q_us entry of an empty cell (count
 * tells it from a cell whose latencies are 0).  One radix sort of
 * (cell, latency) keys: every result is an integer, bit-exact for any launch
 * geometry.  ANOMOD_ESTATE for a set without a start column or an ungrouped
 * set; ANOMOD_EINVAL for a service index >= S, n_windows / step_us / nq /
 * q_pct out of range, or more than 2^32 - 4097 spans in traces; n == 0 gives
 * zeros.  The workspace (24 B a span plus the tables) is allocated for the
 * call and freed on return.  The call is rank-local: no collective runs even
 * with a communicator attached (quantiles do not merge).  The set's hints
 * are read and updated only as anomod_edge_windows_spans does.              */
typedef struct {
  uint32_t n_services;    /* in : S; E = (S + 2) * S as in anomod_edge_table     */
  uint32_t n_windows;     /* in : T in [1, 65536], T * E <= 2^24, else EINVAL    */
  uint64_t t0_us;         /* in                                                  */
  uint64_t step_us;       /* in : >= 1                                           */
  uint32_t nq;            /* in : 1..8                                           */
  const uint32_t* q_pct;  /* in : [nq] host, each in [0, 99]                     */
  uint64_t* count;        /* [T * E] host, may be NULL                           */
  uint32_t* q_us;         /* [T * E * nq] host, cell-major; 0 for an empty cell  */
  uint64_t outside;       /* out                                                 */
} anomod_edge_window_quantiles;
int anomod_edge_window_quantiles_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                       anomod_edge_window_quantiles* out);
/* Self-time (exclusive latency) edge table of a grouped set.  The parent of
 * span i is the first span of its trace, in position order, whose span_id
 * equals i's parent_span_id — the edge table's rule, duplicated ids
 * included; a root (reference 0), an orphan (no such span) and a span whose
 * first match is itself have none.  With child_sum(j) the u64 sum of dur_us
 * over the spans whose parent is j,
 *   self_us[i] = dur_us[i] - min(dur_us[i], child_sum(i))
 * (children that overlap in time are summed, not merged: a fan-out parent
 * saturates to 0).  `out` has the layout and rows of the edge table of
 * anomod_edge_aggregate_spans — a self-referencing span sits in the row that
 * table gives it — with sum / min / max / hist / p50 / p99 taken over self_us;
 * count and errors equal that table's.  Every result is an integer, bit-exact
 * for any launch geometry.  NULL outputs are skipped; n == 0 gives an empty
 * table; a service index >= n_services is ANOMOD_EINVAL, an ungrouped set
 * ANOMOD_ESTATE; at most 2^32 - 2 spans per call.  With a communicator
 * attached the table is merged over the ranks and self_us stays rank-local.
 * The set's histogram-form hint is neither read nor changed.                */
int anomod_edge_self_time_spans(anomod_ctx* ctx, const anomod_spans* spans, uint32_t n_services,
                                anomod_edge_table* out,
                                uint32_t* self_us /* [n_spans] host, may be NULL */);
/* Critical path of a grouped set with a start-time column, and its edge
 * table: which spans determined the end-to-end latency of their trace, and
 * how much each added.  With s(i) = start_us[i], e(i) = s(i) + dur_us[i]
 * (u64, saturating) and par(i) the parent rule of the self-time call, a span
 * of a trace without a parent is a head (roots, orphans, self-references).
 * A child c of p = par(c) covers [a, b) = [max(s(c), s(p)), min(e(c), e(p)))
 * and is eligible when a < b.  The selection at p starts at cur = e(p) and
 * repeatedly takes, among the eligible children with b <= cur, the one with
 * the largest b (the smallest position among equal b), selects it and
 * continues at cur = a of it.  on_path is the least set holding every head
 * and every selected span whose parent is on the path (a span whose parent
 * chain never reaches a head — a reference cycle — is off it), and
 *   cp_us[i] = dur_us[i] - sum of (b - a) over the selected children of i
 * for i on the path, 0 otherwise.  `out` has the layout and rows of the edge
 * table of anomod_edge_aggregate_spans; count and errors are taken over the
 * on-path spans only, sum / min / max / hist / p50 / p99 over their cp_us.
 * Every result is an integer, bit-exact for any launch geometry.  NULL
 * outputs are skipped; n == 0 gives an empty table; spans outside every
 * trace read 0 / 0; a service index >= n_services is ANOMOD_EINVAL, a set
 * without a start column or an ungrouped set ANOMOD_ESTATE; at most 2^32 - 2
 * spans per call.  With a communicator attached the table is merged over the
 * ranks, cp_us and on_path stay rank-local.  The set's histogram-form hint
 * is neither read nor changed; an unknown order hint is probed as in the
 * self-time call.                                                           */
int anomod_edge_critical_path_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                    uint32_t n_services, anomod_edge_table* out,
                                    uint32_t* cp_us /* [n_spans] host, may be NULL */,
                                    uint8_t* on_path /* [n_spans] host, may be NULL */);
/* Trace spectrum of a grouped set: every trace is labelled normal (class 0)
 * or abnormal (class 1), and per class the traces that pass through each
 * service and each edge row are counted.  With row(i) the edge row
 * anomod_edge_aggregate_spans counts span i in (duplicated ids, orphans and
 * self-references land where that table puts them),
 *   bad(i) = dur_us[i] > thr_us[row(i)]                      (strict)
 *            || use_errors && (flags[i] & ANOMOD_FLAG_ERROR)
 * and trace t is abnormal when any of its spans is bad.  thr_us[r] ==
 * UINT32_MAX never fires; thr_us == NULL stands for UINT32_MAX in every row.
 * An empty trace is normal and covers nothing.  svc_traces[k][s] counts the
 * traces of class k holding at least one span of service s (a trace counts
 * once per service), edge_traces[k][r] the same per edge row, bad_spans[r]
 * every bad span of row r.  Every result is an integer, bit-exact for any
 * launch geometry.  NULL outputs are skipped; n == 0 gives zeros (every trace
 * normal); an ungrouped set is ANOMOD_ESTATE; a service index >= n_services
 * or E = (S + 2) * S > 2^19 (S >= 724: the long-trace pass keeps one bit per
 * row in 64 KiB of LDS) is ANOMOD_EINVAL; at most 2^32 - 2 spans per call.
 * The call is rank-local: no collective runs even with a communicator
 * attached (a caller sums the ranks' integer tables itself).  The set's hints
 * are read and updated only as anomod_edge_windows_spans does (the order
 * probe of a first walk).                                                   */
typedef struct {
  uint32_t n_services;     /* in : S; E = (S + 2) * S as in anomod_edge_table    */
  uint32_t use_errors;     /* in : non-zero: an error-flagged span is bad        */
  const uint32_t* thr_us;  /* in : [E] host latency thresholds, or NULL          */
  uint64_t n_traces[2];    /* out: traces per class                              */
  uint64_t* svc_traces;    /* [2 * S] host, class-major; each may be NULL        */
  uint64_t* edge_traces;   /* [2 * E] host, class-major                          */
  uint64_t* bad_spans;     /* [E] host                                           */
  uint8_t* trace_abnormal; /* [n_traces] host: the class of every trace          */
} anomod_trace_spectrum;
int anomod_trace_spectrum_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                anomod_trace_spectrum* out);
/* Trace shape census of a grouped set: a structural fingerprint per trace,
 * the distinct fingerprints of the set and how many traces have each.  All
 * arithmetic is on u64, mod 2^64; mix64 is the SplitMix64 finaliser.  With
 * par(i) the parent rule of the self-time call, a span without a parent is a
 * head of kind ROOT (reference 0), ORPHAN (the reference names no span of the
 * trace) or SELF (the first match is the span itself).  With the label key
 *   K(i) = svc_key[svc(i)]
 *          ^ (use_errors && (flags[i] & ANOMOD_FLAG_ERROR) ? 0xD1B54A32D192ED03 : 0)
 * (svc_key == NULL stands for svc_key[s] = mix64(s + 1)) and B =
 * 0x9E3779B97F4A7C15, the call-path hash is
 *   P(i) = seed(kind) * B + K(i)   for a head (seeds: ROOT 0x243F6A8885A308D3,
 *          ORPHAN 0x13198A2E03707344, SELF 0xA4093822299F31D0)
 *   P(i) = P(par(i)) * B + K(i)    otherwise.
 * A span whose parent chain never reaches a head (a reference cycle, or a
 * span hanging off one) is off the tree: path_hash 0, in no shape, counted in
 * off_tree_spans.  trace_shape[t] is the sum of mix64(P(i)) over the on-tree
 * spans of trace t (0 for a trace with none): the multiset of labelled
 * root-to-span call paths.  It ignores span order — with unique ids it is
 * invariant under any permutation of the spans inside a trace — and equates
 * trees that differ only in how equal-label siblings share their children;
 * it separates trees that differ in any call path, as far as a 64-bit hash
 * without an adversarial guarantee does.  The census lists the distinct
 * trace_shape values by count descending, then value ascending: per shape its
 * count, the traces with trace_class[t] != 0 (abnormal) and the smallest
 * trace index (first_trace).  Bit-exact for any launch geometry.  NULL
 * outputs are skipped; cap == 0 with NULL arrays is a size query (n_shapes);
 * a set without traces gives n_shapes 0, a set of only empty traces one
 * shape, 0.  Spans outside every trace read path_hash 0 and are not counted.
 * An ungrouped set is ANOMOD_ESTATE; a service index >= n_services is
 * ANOMOD_EINVAL; at most 2^32 - 2 spans and 2^32 - 4097 traces per call.  The
 * call is rank-local: no collective runs even with a communicator attached.
 * The set's histogram-form hint is neither read nor changed; an unknown order
 * hint is probed as in the self-time call.                                  */
typedef struct {
  uint32_t n_services;        /* in : S                                              */
  uint32_t use_errors;        /* in : non-zero: the error flag is part of the label  */
  const uint64_t* svc_key;    /* in : [S] host, or NULL (mix64(s + 1))               */
  const uint8_t* trace_class; /* in : [n_traces] host, or NULL (every trace class 0) */
  uint64_t cap;               /* in : shapes the four arrays below hold              */
  uint64_t n_shapes;          /* out: distinct shapes of the set                     */
  uint64_t off_tree_spans;    /* out                                                 */
  uint64_t* shape;            /* [cap] first min(cap, n_shapes) in census order      */
  uint64_t* count;            /* [cap]                                               */
  uint64_t* abnormal;         /* [cap]                                               */
  uint64_t* first_trace;      /* [cap]                                               */
  uint64_t* trace_shape;      /* [n_traces] host, may be NULL                        */
  uint64_t* path_hash;        /* [n_spans] host, may be NULL                         */
} anomod_trace_shapes;
int anomod_trace_shapes_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_trace_shapes* out);
/* Error origins of a grouped set: where failures start, how far they travel
 * up their callers and whether they reach the trace's entry.  Collectors mark
 * a failing leaf and every caller that failed because of it alike; this call
 * tells them apart.  With err(i) = flags[i] & ANOMOD_FLAG_ERROR, par(i) the
 * parent rule of the self-time call (a ROOT, an ORPHAN and a SELF reference
 * have no parent and are heads; duplicated ids resolve to the first carrier),
 * row(i) the edge row of anomod_edge_aggregate_spans and kid_err(j) the
 * number of error-flagged spans whose parent is j:
 *   class(i) = ANOMOD_ERR_CLEAN       !err(i) && kid_err(i) == 0
 *              ANOMOD_ERR_ORIGIN       err(i) && kid_err(i) == 0
 *              ANOMOD_ERR_PROPAGATED   err(i) && kid_err(i) >  0
 *              ANOMOD_ERR_ABSORBER    !err(i) && kid_err(i) >  0
 * The chain of an error-flagged span follows up(i) = par(i) while that
 * parent exists and carries the flag; hops(i) counts the steps to the span
 * without an up, top(i), and
 *   fate(i)  = ANOMOD_FATE_SURFACED   top(i) is a head
 *              ANOMOD_FATE_CONTAINED  top(i) has a parent (which carries no flag)
 *              ANOMOD_FATE_LOOP       the chain never ends: a reference cycle of
 *                                     two or more error-flagged spans, or a span
 *                                     hanging off one; hops(i) = 0
 * (a SELF reference is a head, so a one-span cycle is no loop); a span
 * without the flag has fate 0 and hops 0.  Per edge row, over the spans of
 * the row that lie in traces: origin / propagated count the spans of those
 * classes (origin + propagated equals the edge table's errors, row by row),
 * stopped the error-flagged spans with hops 0 and fate CONTAINED (the edge on
 * which a failure was stopped), surfaced the ORIGIN spans of fate SURFACED,
 * absorbers the ABSORBER spans, hops_sum / hops_max the hops of the ORIGIN
 * spans (hops_max 0 for a row without one).  error_spans counts the
 * error-flagged spans in traces, loop_spans those of fate LOOP.  span_state[i]
 * = class | fate << 2 and span_hops[i] by span position; spans outside every
 * trace read 0 / 0 and are not counted.  Every result is an integer, bit-exact
 * for any launch geometry.  NULL outputs are skipped; n == 0 gives zeros; an
 * ungrouped set is ANOMOD_ESTATE; a service index >= n_services is
 * ANOMOD_EINVAL; at most 2^32 - 2 spans per call.  The call is rank-local: no
 * collective runs even with a communicator attached (a caller sums the ranks'
 * tables itself, taking the maximum for hops_max).  The set's histogram-form
 * hint is neither read nor changed; an unknown order hint is probed as in the
 * self-time call.                                                           */
#define ANOMOD_ERR_CLEAN 0u
#define ANOMOD_ERR_ORIGIN 1u
#define ANOMOD_ERR_PROPAGATED 2u
#define ANOMOD_ERR_ABSORBER 3u
#define ANOMOD_FATE_SURFACED 1u
#define ANOMOD_FATE_CONTAINED 2u
#define ANOMOD_FATE_LOOP 3u
typedef struct {
  uint32_t n_services;   /* in : S; E = (S + 2) * S as in anomod_edge_table      */
  uint64_t error_spans;  /* out                                                  */
  uint64_t loop_spans;   /* out                                                  */
  uint64_t* origin;      /* [E] host; each array may be NULL                     */
  uint64_t* propagated;  /* [E]                                                  */
  uint64_t* stopped;     /* [E]                                                  */
  uint64_t* surfaced;    /* [E]                                                  */
  uint64_t* absorbers;   /* [E]                                                  */
  uint64_t* hops_sum;    /* [E]                                                  */
  uint32_t* hops_max;    /* [E]                                                  */
  uint8_t* span_state;   /* [n_spans] host, may be NULL                          */
  uint32_t* span_hops;   /* [n_spans] host, may be NULL                          */
} anomod_error_origins;
int anomod_error_origins_spans(anomod_ctx* ctx, const anomod_spans* spans,
                               anomod_error_origins* out);
/* Call repeats of a grouped set: how often one parent span called the same
 * callee service more than once — a retry after a failure, a retry storm, an
 * N+1 loop over a result set.  The edge table counts every span once; this
 * call says how many logical calls they were.  With err(i) = flags[i] &
 * ANOMOD_FLAG_ERROR and par(i) the parent rule of the self-time call (a ROOT,
 * an ORPHAN and a SELF reference have no parent and are heads; duplicated ids
 * resolve to the first carrier), a span with a parent belongs to the group
 *   G(j, c) = { i : par(i) = j, svc[i] = c }
 * — one parent span's calls to one callee service; heads belong to no group.
 * All members of a group share the edge row r = svc[j] * S + c, one of the
 * first S * S rows of anomod_edge_aggregate_spans.  With n the size of a
 * group and e its error-flagged members, per edge row over the groups of the
 * row:
 *   groups      the groups (the logical calls)
 *   repeats     sum of n - 1
 *   repeated    groups with n >= 2
 *   retried     groups with n >= 2 and e >= 1
 *   recovered   groups with n >= 2 and 1 <= e < n (some attempt went through)
 *   exhausted   groups with n >= 2 and e == n
 *   size_max    the largest n (0 for a row without a group)
 *   size_hist   [row][b] groups by b = min(floor(log2 n), ANOMOD_REPEAT_BINS -
 *               1): sizes 1, 2-3, 4-7, ..., 64-127, >= 128
 *   after_error members that started after a failure of their group had ended:
 *               with e_end(m) = start_us[m] + max(dur_us[m], 1) — a failed
 *               call occupies at least one microsecond, so a span never
 *               follows itself; a sum past 2^64 - 1 lies after every start —
 *               member i counts iff start_us[i] != 0 and start_us[i] >= the
 *               least e_end(m) over the members m of its group with err(m)
 *               and start_us[m] != 0; a group without such an m counts
 *               nothing, and so does a parallel fan-out with equal starts.
 *               All zero for a set without a start-time column (timed = 0).
 * groups + repeats of a row is the number of its spans that have a parent (on
 * the first S * S rows the edge table's count, for a set without a
 * self-reference; 0 on the ROOT and ORPHAN rows); retried = recovered +
 * exhausted; size_hist sums to groups over b, and size_hist[r][0] = groups[r]
 * - repeated[r].  grouped_spans is the sum of groups + repeats over the rows,
 * max_size the largest group of the set, timed 1 iff the set has start times.
 * span_group_size[i] is n of span i's group (0 for a head), span_after_error[i]
 * 1 iff span i is counted in after_error, by span position; spans outside
 * every trace read 0 / 0 and are in no group.  Every result is an integer,
 * bit-exact for any launch geometry.  NULL outputs are skipped; n == 0 gives
 * zeros; an ungrouped set is ANOMOD_ESTATE; a service index >= n_services is
 * ANOMOD_EINVAL; at most 2^32 - 2 spans per call.  The call is rank-local: no
 * collective runs even with a communicator attached (a caller sums the ranks'
 * tables itself, taking the maximum for size_max).  The set's histogram-form
 * hint is neither read nor changed; an unknown order hint is probed as in the
 * self-time call.                                                           */
#define ANOMOD_REPEAT_BINS 8u
typedef struct {
  uint32_t n_services;       /* in : S; E = (S + 2) * S as in anomod_edge_table    */
  uint32_t max_size;         /* out                                                */
  uint32_t timed;            /* out                                                */
  uint64_t grouped_spans;    /* out                                                */
  uint64_t* groups;          /* [E] host; each array may be NULL                   */
  uint64_t* repeats;         /* [E]                                                */
  uint64_t* repeated;        /* [E]                                                */
  uint64_t* retried;         /* [E]                                                */
  uint64_t* recovered;       /* [E]                                                */
  uint64_t* exhausted;       /* [E]                                                */
  uint64_t* after_error;     /* [E]                                                */
  uint64_t* size_hist;       /* [E * ANOMOD_REPEAT_BINS] row-major                 */
  uint32_t* size_max;        /* [E]                                                */
  uint32_t* span_group_size; /* [n_spans] host, may be NULL                        */
  uint8_t* span_after_error; /* [n_spans] host, may be NULL                        */
} anomod_call_repeats;
int anomod_call_repeats_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_call_repeats* out);
/* Call transit of a grouped set with start times: the time lost between two
 * services — from the moment the caller's client span opens to the moment the
 * callee's server span starts, and from the callee's end back to the caller's
 * end.  Retransmits, waiting for a connection, name resolution and a caller
 * that gives up early all live there; the callee's duration and self time do
 * not move.
 *   Spans.   s(i) = start_us[i], e(i) = s(i) + dur_us[i] (u64, saturating at
 *            2^64 - 1, as the critical-path call).
 *   Parent.  par(i) is the parent rule of the self-time call: the first span
 *            of i's trace, in position order, whose id equals i's parent
 *            reference; none for reference 0, for a reference that names no
 *            span of the trace, and when the first match is i itself;
 *            duplicated ids resolve to the first carrier.
 *   Call.    A span with a parent is a call.  kids(j) is the number of calls
 *            whose parent is j.
 *   Paired.  A call c with p = par(c) is paired iff kids(p) == 1: the parent
 *            span exists only to make this call (a client / exit span).
 *            Unpaired calls are counted in `calls` only: their gaps would
 *            include the parent's other work and are not transit.
 *   Row.     The row of a call is r = svc[p] * S + svc[c], one of the first
 *            S * S rows of anomod_edge_aggregate_spans.  The ROOT and ORPHAN
 *            rows stay empty in every output.
 *   Untimed. A paired call is untimed when start_us[c] == 0 || start_us[p] ==
 *            0.  It adds untimed[r] += 1 and nothing else.
 *   A paired, timed call:
 *            s(c) >= s(p): one record in the request table with value
 *            min(s(c) - s(p), 2^32 - 1).  Otherwise the call is early:
 *            early[r] += 1, early_us[r] += min(s(p) - s(c), 2^32 - 1), no
 *            request record (the callee's clock runs behind the caller's: per
 *            edge, how far the timing columns can be trusted).
 *            e(c) <= e(p): one record in the response table with value
 *            min(e(p) - e(c), 2^32 - 1).  Otherwise the call is late
 *            (abandoned: the caller gave up while the callee still worked):
 *            late[r] += 1, late_us[r] += min(e(c) - e(p), 2^32 - 1), no
 *            response record.
 *            The two tests are independent: equal starts give a request of 0,
 *            equal ends a response of 0.
 *   Tables.  request and response are anomod_edge_tables with the layout,
 *            histogram bins, p50 / p99 and finalize of every other edge table.
 *            count / errors are taken over the recorded calls, with the error
 *            bit being the call's own ANOMOD_FLAG_ERROR; sum / min / max /
 *            hist over the recorded values.
 *   Counts.  untimed, early, late, early_us, late_us are u64 [E].
 *   Scalars. calls is the spans with a parent, paired those that are paired.
 *   Optional per-span columns, by span position: span_req_us u32 and
 *            span_resp_us u32, both 0 where nothing was recorded; span_state
 *            u8 = ANOMOD_TRANSIT_CALL | _PAIRED | _TIMED | _EARLY | _LATE;
 *            spans outside every trace read 0.
 * Per row: request.count + early + untimed = the paired calls of the row;
 * response.count + late = request.count + early; calls = the edge table's
 * count over the first S * S rows minus the self-referencing spans.  Every
 * result is an integer, bit-exact for any launch geometry.  The two tables
 * are required, every other pointer may be NULL (that output is skipped);
 * n == 0 gives empty tables and zeros; an ungrouped set or a set without a
 * start column is ANOMOD_ESTATE; a service index >= n_services is
 * ANOMOD_EINVAL; at most 2^32 - 2 spans per call.  With a communicator
 * attached the two tables are merged over the ranks (they go through the
 * record aggregation of the other edge tables, whose status agreement every
 * rank must reach, so every rank makes the call); the count arrays, the
 * scalars and the per-span columns stay rank-local (a caller sums the ranks'
 * arrays itself).  The set's histogram-form hint is neither read nor changed;
 * an unknown order hint is probed as in the self-time call.                 */
#define ANOMOD_TRANSIT_CALL 1u
#define ANOMOD_TRANSIT_PAIRED 2u
#define ANOMOD_TRANSIT_TIMED 4u
#define ANOMOD_TRANSIT_EARLY 8u
#define ANOMOD_TRANSIT_LATE 16u
typedef struct {
  uint32_t n_services;         /* in : S; E = (S + 2) * S as in anomod_edge_table  */
  uint64_t calls;              /* out                                              */
  uint64_t paired;             /* out                                              */
  anomod_edge_table* request;  /* required                                         */
  anomod_edge_table* response; /* required                                         */
  uint64_t* untimed;           /* [E] host; each array may be NULL                 */
  uint64_t* early;             /* [E]                                              */
  uint64_t* late;              /* [E]                                              */
  uint64_t* early_us;          /* [E]                                              */
  uint64_t* late_us;           /* [E]                                              */
  uint32_t* span_req_us;       /* [n_spans] host, may be NULL                      */
  uint32_t* span_resp_us;      /* [n_spans] host, may be NULL                      */
  uint8_t* span_state;         /* [n_spans] host, may be NULL                      */
} anomod_call_transit;
int anomod_call_transit_spans(anomod_ctx* ctx, const anomod_spans* spans,
                              anomod_call_transit* out);
/* One-shot host convenience: upload + aggregate + download.               */
int anomod_edge_aggregate(anomod_ctx* ctx, const anomod_span_soa* soa, uint64_t n_spans,
                          const uint64_t* trace_ptr, uint64_t n_traces, anomod_edge_table* out);

/* ---- trace structure -------------------------------
 * Per span and per trace, what _build_span_records / collect_traces compute
 * one dict at a time (trace_collector.py:401-481, 536-547).  Spans are nodes
 * keyed by their id; with duplicated ids the reference keeps the LAST span's
 * parent (:437) while every span joins its own parent's child list (:438-439).
 *   parent_pos  position in the trace of the node's parent (first span whose
 *               id equals the parent reference of the LAST span carrying the
 *               node's id), ANOMOD_NO_PARENT when the reference is 0 or names
 *               no span of the trace (:427-437, :443)
 *   depth       the BFS of :441-449: the node's deepest visit from the roots,
 *               i.e. the longest path along "node of a span's own parent
 *               reference -> the span's node" (with unique ids: the distance
 *               along the parents); 0 when no root reaches the node (:477) or
 *               a cycle the BFS reaches feeds it (the reference never ends)
 *   n_children  spans whose own parent reference names the node (:438-439)
 *   span_flags  ANOMOD_SPAN_ROOT | ANOMOD_SPAN_FIRST (first span with its id)
 *   n_roots     distinct root nodes of the trace (len(root_span_node_ids))
 *   svc_mask    services_involved (:536): bit s of word s/64, ceil(S/64) words
 * Every pointer may be NULL (that output is skipped).                      */
#define ANOMOD_NO_PARENT 0xFFFFFFFFu
#define ANOMOD_SPAN_ROOT 0x1u
#define ANOMOD_SPAN_FIRST 0x2u
typedef struct {
  uint32_t n_services;  /* in : S (sizes svc_mask)                          */
  uint32_t* parent_pos; /* [n_spans]                                        */
  uint32_t* depth;      /* [n_spans]                                        */
  uint32_t* n_children; /* [n_spans]                                        */
  uint8_t* span_flags;  /* [n_spans]                                        */
  uint32_t* n_roots;    /* [n_traces]                                       */
  uint64_t* svc_mask;   /* [n_traces * ceil(S / 64)]                        */
} anomod_trace_struct_out;
int anomod_trace_structure_spans(anomod_ctx* ctx, const anomod_spans* spans,
                                 anomod_trace_struct_out* out);
int anomod_trace_structure(anomod_ctx* ctx, const anomod_span_soa* soa, uint64_t n_spans,
                           const uint64_t* trace_ptr, uint64_t n_traces,
                           anomod_trace_struct_out* out);

/* ---- segment summary -------------------------------
 * analyze_trace_patterns (enhanced_trace_collector.py:216-296) over columnar
 * segment records: svc / endpoint are indices into the caller's name lists
 * (service_name decoded as extract_trace_info does, :130-150), is_error the
 * raw value, latency and start_time in ms.
 *   service_counts[s], endpoint_counts[e]  call counts (:246-253)
 *   error_count        records with is_error == 1 (:256-257)
 *   latency_*          count / sum / min / max over latency > 0 (:260-283;
 *                      avg = sum / count)
 *   start_*            count / min / max over start_time != 0 (:265-270)
 * min/max are 0 when their count is 0.                                      */
typedef struct {
  uint32_t n_services;       /* in : service ids are < n_services          */
  uint32_t n_endpoints;      /* in : endpoint ids are < n_endpoints        */
  uint64_t* service_counts;  /* [n_services] (may be NULL)                 */
  uint64_t* endpoint_counts; /* [n_endpoints] (may be NULL)                */
  uint64_t total;            /* out                                        */
  uint64_t error_count;      /* out                                        */
  uint64_t latency_count;    /* out                                        */
  int64_t latency_sum, latency_min, latency_max; /* out                    */
  uint64_t start_count;      /* out                                        */
  int64_t start_min, start_max; /* out                                     */
} anomod_segment_summary_out;
int anomod_segment_summary(anomod_ctx* ctx, const uint32_t* svc, const uint32_t* endpoint,
                           const int32_t* is_error, const int64_t* latency,
                           const int64_t* start_time, uint64_t n, anomod_segment_summary_out* out);

/* ---- API-response summary ----------------------------
 * Latency statistics of monitor_http_responses.py generate_summary
 * (:150-207) and enhanced_openapi_monitor.py generate_reports (:318-332):
 * the selected values (positive_only: v > 0, as generate_summary :167-169;
 * else every non-NaN value, as generate_reports :324) sorted, then
 *   min = x[0], max = x[c-1], median = x[c//2],
 *   p95 = x[int(c*0.95)], p99 = x[int(c*0.99)]   (f64 product, truncated)
 * exactly, and sum over the sorted values (fixed tree order: reproducible,
 * within c*2^-53 relative of Python's left-to-right sum).  All 0 when c = 0.
 * n <= 2^32 - 4097 (the sort's limit).                                     */
typedef struct {
  uint64_t count;             /* out: values selected                      */
  double min, max, sum;       /* out                                       */
  double median, p95, p99;    /* out                                       */
} anomod_value_summary_out;
int anomod_value_summary(anomod_ctx* ctx, const double* values, uint64_t n, int positive_only,
                         anomod_value_summary_out* out);
/* The device sort under the exact-order-statistic paths (the exact per-edge
 * quantiles and the value summary above): a stable LSD radix sort of n u64
 * keys by bits [begin_bit, end_bit) (every key < 2^end_bit), hand-written
 * for CDNA4 (csrc/radix.hip).  Host buffers in and out (may alias);
 * *passes (may be NULL) = 8-bit digit passes run (digits equal in every key
 * are skipped).  n <= 2^32 - 4097 (u32 tile offsets).                      */
int anomod_sort_u64(anomod_ctx* ctx, const uint64_t* keys, uint64_t n, int begin_bit,
                    int end_bit, uint64_t* sorted, int* passes);
/* generate_summary's distributions in the same pass: status_id / ctype_id
 * index the caller's first-appearance lists of status codes and content
 * types (content_type.split(';')[0], 'unknown' when absent: :163-173),
 * has_error = the response carries an 'error' key (:176-177); latency is
 * the value summary of latency_ms > 0.                                       */
typedef struct {
  uint32_t n_status;          /* in : status ids are < n_status            */
  uint32_t n_ctype;           /* in : content-type ids are < n_ctype       */
  uint64_t* status_counts;    /* [n_status] out                            */
  uint64_t* ctype_counts;     /* [n_ctype] out                             */
  uint64_t error_count;       /* out                                       */
  anomod_value_summary_out latency; /* out                                 */
} anomod_response_summary_out;
int anomod_response_summary(anomod_ctx* ctx, const uint32_t* status_id, const uint32_t* ctype_id,
                            const uint8_t* has_error, const double* latency_ms, uint64_t n,
                            anomod_response_summary_out* out);

/* ---- windowed EWMA / z-score -------------------------
 * X is time-major [T][S] f32 (NaN = missing sample).  Per series:
 *   d_t = x_t - m_{t-1};  z_t = d_t / sqrt(v_{t-1} + eps)
 *   m_t = m_{t-1} + alpha*d_t;  v_t = (1-alpha)*(v_{t-1} + alpha*d_t^2)
 * with m = x, v = 0, z = 0 at the first valid sample; NaN samples leave the
 * state untouched and score 0.  Z[w][s] = max |z_t| over t in window w of W
 * steps (T must be a multiple of W).  m/v equal pandas
 * Series.ewm(alpha, adjust=False).mean() / .var(bias=True).  alpha in (0, 1];
 * eps >= 2^-126 (FLT_MIN; smaller, 0 included, is ANOMOD_EINVAL: the f32
 * reciprocal square root needs a normal v + eps).  Samples are |x| <= 2^62
 * or NaN; beyond that nothing is checked and a series whose variance leaves
 * the f32 range scores 0.  The metric
 * matrix replaces the long CSV rows of metric_collector.py:427-443 and
 * fetch_prometheus_metrics.py:53-67.                                       */
int anomod_ewma_z(anomod_ctx* ctx, const float* X, uint64_t T, uint64_t S, float alpha,
                  uint32_t W, float eps, float* Z);
/* Device-resident streaming variant: X stays in HBM, the (m, v, n) state is
 * carried across calls so T can be processed in chunks.  upload takes
 * row-major host X[T][S]; the device copy is laid out for the kernel that
 * reads it (16-step tiles for the sequential kernel, rows for the
 * time-parallel one; ANOMOD_EWMA_MODE=1/2/3 forces sequential-tiles /
 * time-parallel / sequential-rows) — opaque to the caller.                */
int anomod_series_create(anomod_ctx* ctx, uint64_t T, uint64_t S, anomod_series** out);
int anomod_series_upload(anomod_ctx* ctx, anomod_series* ser, const float* X);
int anomod_series_fill_synthetic(anomod_ctx* ctx, anomod_series* ser, uint64_t seed,
                                 uint64_t t0);
int anomod_series_reset_state(anomod_ctx* ctx, anomod_series* ser);
/* The resident matrix back as host rows X[T][S] (whatever the device layout). */
int anomod_series_download(anomod_ctx* ctx, const anomod_series* ser, float* X);
int anomod_series_ewma_z(anomod_ctx* ctx, anomod_series* ser, float alpha, uint32_t W,
                         float eps, float* Z_host /* may be NULL */);
int anomod_series_free(anomod_series* ser);

/* ---- series correlation ---------------------------------------------------
 * Pearson correlation of every column of X[T][S] (f32) against K target
 * columns Y[T][K] (host, row-major, f32), pairwise-complete over missing
 * samples, in one pass over X.
 *  - Pair set.  Step t is a pair of (k, s) iff X[t][s] and Y[t][k] are both
 *    finite; NaN and +-inf are missing.  n[k][s] is the size of that set.
 *  - Pivots.  px_s is the first finite X[t][s] of the call, whatever Y holds;
 *    py_k is the first finite Y[t][k].
 *  - Sums.  Over the pair set, in f64 and in step order: sum x', sum y',
 *    sum x'^2, sum y'^2, sum x'y' with x' = (double)x - px, y' = (double)y - py.
 *    sxx = sum x'^2 - (sum x')^2 / n, syy likewise,
 *    sxy = sum x'y' - sum x' sum y' / n.
 *  - Result.  r[k][s] = NaN when n < max(min_pairs, 2) or sxx <= 0 or
 *    syy <= 0 (a constant series: x' is exactly 0); otherwise
 *    sxy / sqrt(sxx * syy) clamped to [-1, 1].  A series with no finite
 *    sample gives n = 0, r = NaN.
 *  - Samples are |x| <= 2^62 or missing, as for EWMA.
 *  - Accuracy: |r - r_exact| <= 8 T 2^-53 max(kx, ky) + 2^-50 with
 *    kx = sum (x - px)^2 / sum (x - mean)^2 over the pair set, ky likewise
 *    (derivation in csrc/series_corr.hip).
 *  - K == 0, K > ANOMOD_CORR_MAX_TARGETS, a NULL ser / X / Y / r or T >= 2^32
 *    is ANOMOD_EINVAL; T == 0 or S == 0 is ANOMOD_OK with nothing written.
 *    n may be NULL.
 *  - The call reads the resident matrix in the layout it has (tiles or rows),
 *    re-lays nothing, leaves the EWMA state (m, v, n) alone: a later
 *    anomod_series_ewma_z gives the bits it would have given without it.
 *  - The same input gives the same bits from run to run and from either
 *    layout; the order of summation depends on T and S only.
 * Stage 16 of anomod_ctx_stage_ms times the kernel.                         */
#define ANOMOD_CORR_MAX_TARGETS 8
int anomod_series_correlate(anomod_ctx* ctx, const anomod_series* ser,
                            const float* Y /* host, row-major [T][K] */, uint32_t K,
                            uint32_t min_pairs, double* r /* [K][S] */,
                            uint32_t* n /* [K][S], may be NULL */);
/* Host convenience, as anomod_ewma_z is to anomod_series_ewma_z: X is host
 * rows [T][S], uploaded for the one call (it must fit the device).          */
int anomod_correlate(anomod_ctx* ctx, const float* X, uint64_t T, uint64_t S, const float* Y,
                     uint32_t K, uint32_t min_pairs, double* r, uint32_t* n);

/* ---- personalized PageRank RCA -----------------------
 * networkx 3.4.2 pagerank convention: out-edge CSR (row = caller) with
 * weights; rows are normalised by out-weight; dangling mass is sent along
 * the personalization p; x0 = 1/N;
 *   x <- alpha*(x A + sum_{dangling} x * p) + (1 - alpha)*p
 * A row whose weights sum to 0 (no edges, or only zero-weight edges) is
 * dangling: its edges contribute nothing.  Every other edge weight is
 * (float)((double)w / out-weight), the out-weight summed in double.
 * stop when ||x - x_last||_1 < N*tol (tol > 0) or after `iters` iterations.
 * iters_done = iterations executed; status ANOMOD_OK even when tol was not
 * reached (caller checks iters_done == iters).                            */
int anomod_pagerank(anomod_ctx* ctx, const uint32_t* row_ptr, const uint32_t* col,
                    const float* w, uint32_t N, const double* p, double alpha, uint32_t iters,
                    double tol, double* x_out, uint32_t* iters_done);
int anomod_graph_create(anomod_ctx* ctx, const uint32_t* row_ptr, const uint32_t* col,
                        const float* w, uint32_t N, anomod_graph** out);
int anomod_graph_synthetic(anomod_ctx* ctx, uint32_t N, uint32_t mean_degree, uint64_t seed,
                           anomod_graph** out);
/* The same synthetic graph as host CSR (config 5: Pareto out-degrees of the
 * given mean, 2 % dangling, call-count weights): *nnz always; with every
 * array NULL a size query, else row_ptr [N + 1], col / w [cap >= nnz].     */
int anomod_graph_synthetic_csr(uint32_t N, uint32_t mean_degree, uint64_t seed,
                               uint32_t* row_ptr, uint32_t* col, float* w, uint64_t cap,
                               uint64_t* nnz);
int anomod_graph_info(const anomod_graph* g, uint32_t* N, uint64_t* nnz);
int anomod_graph_pagerank(anomod_ctx* ctx, anomod_graph* g, const double* p, double alpha,
                          uint32_t iters, double tol, double* x_out, uint32_t* iters_done);
/* Which path the last anomod_graph_pagerank / _batch solve of g took: 1 =
 * replayed hipGraph of per-iteration launches (fixed iterations; a batch:
 * per-iteration launches), 2 = per-iteration
 * launches with a host read-back of the L1 change (tolerance), 3 = one
 * persistent launch (grid barrier); | 4 = the persistent launch timed out at
 * its grid barrier (a workgroup never became resident, e.g. another process
 * held CUs) and the solve was rerun from x0 on path 1 or 2 — same result
 * bits.  fallbacks = such reruns over the graph's lifetime.              */
#define ANOMOD_PPR_PATH_GRAPH 1
#define ANOMOD_PPR_PATH_READBACK 2
#define ANOMOD_PPR_PATH_PERSISTENT 3
#define ANOMOD_PPR_PATH_FALLBACK 4
int anomod_graph_last_solve(const anomod_graph* g, uint32_t* path, uint32_t* fallbacks);
/* K (<= 16) personalizations solved together (replica mode, SURVEY.md §8e:
 * one vector per experiment / fault hypothesis): the CSR is read once per
 * iteration for all K.  P and X are [K][N]; every column equals its
 * anomod_graph_pagerank solve bit for bit (same arithmetic and reduction
 * order).  tol > 0: each vector stops at its own convergence iteration
 * (later iterations carry it unchanged); iters_done = iterations run.  One
 * persistent launch (grid barrier) when the batch's workgroups are all
 * resident (N = 10^5: K <= 16), else one launch per iteration.             */
int anomod_graph_pagerank_batch(anomod_ctx* ctx, anomod_graph* g, const double* P, uint32_t K,
                                double alpha, uint32_t iters, double tol, double* X,
                                uint32_t* iters_done);
/* Row-sharded solve (SURVEY.md §8e "sharded" series): with a communicator
 * attached (anomod_ctx_attach_comm) each rank computes its share of whole
 * 256-row blocks of the pull SpMV and every iteration ends in one grouped
 * RCCL exchange — u64 sums of the fixed-point dangling / L1 partials and an
 * in-place all-gather of the new vector.  Without a communicator,
 * virtual_shards = G > 1 runs the same G-way row split on this one device
 * (the single-GPU rehearsal of the sharded path).  Every rank returns the
 * whole vector, equal bit for bit to anomod_graph_pagerank's per-launch
 * solve for any G (same blocks, same integer-summed scalars).           */
int anomod_graph_pagerank_sharded(anomod_ctx* ctx, anomod_graph* g, const double* p,
                                  double alpha, uint32_t iters, double tol,
                                  uint32_t virtual_shards, double* x_out, uint32_t* iters_done);
int anomod_graph_free(anomod_graph* g);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ---------------------*/
#define ANOMOD_UNIQUE_ID_BYTES 128
int anomod_comm_unique_id(uint8_t* out /* ANOMOD_UNIQUE_ID_BYTES */);
int anomod_ctx_attach_comm(anomod_ctx* ctx, const uint8_t* unique_id, int nranks, int rank);
int anomod_ctx_comm_info(const anomod_ctx* ctx, int* nranks, int* rank);

/* Host collective transport instead of RCCL (ranks that share one device —
 * RCCL refuses two ranks on a GPU —, or any host-side library such as gloo):
 * libanomod stages every collective through pinned host memory and calls
 *   allreduce(user, buf, count, dtype, op): in place over all ranks
 *   allgather(user, buf, bytes_per_rank): buf holds nranks blocks, this
 *     rank's (at rank * bytes_per_rank) filled; afterwards all are
 * returning 0 on success.  The same calls, in the same order, as the RCCL
 * path (status agreement, edge-table merge, sharded PageRank exchange). */
#define ANOMOD_DTYPE_I32 0
#define ANOMOD_DTYPE_U32 1
#define ANOMOD_DTYPE_U64 2
#define ANOMOD_DTYPE_F64 3
#define ANOMOD_OP_SUM 0
#define ANOMOD_OP_MIN 1
#define ANOMOD_OP_MAX 2
typedef int (*anomod_host_allreduce_fn)(void* user, void* buf, uint64_t count, int dtype, int op);
typedef int (*anomod_host_allgather_fn)(void* user, void* buf, uint64_t bytes_per_rank);
int anomod_ctx_attach_host_comm(anomod_ctx* ctx, int nranks, int rank,
                                anomod_host_allreduce_fn allreduce,
                                anomod_host_allgather_fn allgather, void* user);

#ifdef __cplusplus
}
#endif
#endif /* ANOMOD_H */
