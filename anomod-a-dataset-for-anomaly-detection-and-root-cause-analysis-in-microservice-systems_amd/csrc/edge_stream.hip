// Host side of an edge stream call (edge_stream.h): argument checks, the
// source of the edge rows, the launch geometry and the counters' read-back.
#include <algorithm>
#include <cstdlib>

#include "edge_stream.h"

namespace anomod {

uint64_t env_cap(const char* name, uint64_t floor) {
  const char* e = getenv(name);
  if (!e || !*e) return 0xFFFFFFFFull;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  if (*end) return 0xFFFFFFFFull;
  return std::max<uint64_t>(v, floor);
}

int stream_table_args(anomod_ctx* ctx, uint32_t S, uint32_t T, uint64_t step, uint32_t* E) {
  ANOMOD_REQUIRE(ctx, S >= 1 && S <= 4096, "n_services=%u out of range [1, 4096]", S);
  *E = (S + ANOMOD_ROOT_ROWS) * S;
  ANOMOD_REQUIRE(ctx, T >= 1 && T <= 65536, "n_windows=%u outside [1, 65536]", T);
  ANOMOD_REQUIRE(ctx, (uint64_t)T * *E <= (1ull << 24), "n_windows * edge rows = %u * %u > 2^24", T,
                 *E);
  ANOMOD_REQUIRE(ctx, step >= 1, "step_us must be at least 1");
  return ANOMOD_OK;
}

int stream_set_args(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S, bool need_start,
                    int ungrouped_rc, uint64_t in_traces[2], uint64_t* n) {
  ANOMOD_REQUIRE(ctx, spans->device == ctx->device, "span set lives on another device");
  if (!spans->grouped) {
    set_error(ctx, "span set is not grouped by trace: anomod_spans_group first");
    return ungrouped_rc;
  }
  if (need_start && !spans->start_us) {
    set_error(ctx, "span set has no start-time column: anomod_spans_set_start_us first");
    return ANOMOD_ESTATE;
  }
  ANOMOD_REQUIRE(ctx, spans->n_spans == 0 || spans->max_svc < S,
                 "span service index %u >= n_services %u", spans->max_svc, S);
  if (spans->n_traces && spans->n_spans)
    if (int rc = bind(ctx)) return rc;
  if (int rc = trace_span_range(ctx, spans, in_traces)) return rc;
  *n = in_traces[1] > in_traces[0] ? in_traces[1] : 0;
  return ANOMOD_OK;
}

EdgeSource::EdgeSource(const anomod_spans* spans, const uint64_t in_traces[2], uint64_t n)
    : rows(span_rows_ready(spans) && spans->rows_lo == in_traces[0] &&
           spans->rows_hi == in_traces[1]),
      b_keys(rows ? 0 : Carve::al(n * 8)),
      b_ws(rows ? 0 : Carve::al(span_edge_keys_ws_bytes(spans))) {}

int EdgeSource::fill(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S, char* workspace) {
  if (rows) return ANOMOD_OK;  // (the row column is not filled from here)
  keys = reinterpret_cast<unsigned long long*>(workspace);
  return span_edge_keys(ctx, spans, S, keys,
                        reinterpret_cast<unsigned long long*>(workspace + b_keys));
}

uint64_t stream_grid(const anomod_ctx* ctx, uint64_t n, uint64_t batch, int per_cu, uint64_t cap,
                     uint64_t max_range, uint64_t* per_wg) {
  const uint64_t batches = (n + batch - 1) / batch;
  uint64_t grid = std::min<uint64_t>((uint64_t)ctx->num_cus * per_cu, batches);
  grid = std::min<uint64_t>(grid, cap);
  *per_wg = (batches + grid - 1) / grid * batch;
  if (*per_wg > max_range) *per_wg = max_range;
  return (n + *per_wg - 1) / *per_wg;
}

void stream_log(const char* kernel, const char* form, int64_t tile, const char* lists,
                uint64_t grid, uint64_t per_wg) {
  if (!log_kernel()) return;
  char ring[40] = "", place[40] = "";
  if (tile >= 0) snprintf(ring, sizeof ring, ", tile %lld windows", (long long)tile);
  if (lists) snprintf(place, sizeof place, ", lists %s", lists);
  fprintf(stderr, "anomod: stream %s<%s>%s%s, grid %llu, %llu spans per workgroup\n", kernel, form,
          ring, place, (unsigned long long)grid, (unsigned long long)per_wg);
}

hipError_t stream_back(anomod_ctx* ctx, void* dst, const void* src, size_t bytes) {
  return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
}

int stream_finish(anomod_ctx* ctx, const unsigned long long* d_misc, int bad, const char* pass,
                  const char* what, unsigned long long misc[2]) {
  misc[0] = misc[1] = 0ull;
  ANOMOD_HIP(ctx, hipMemcpyAsync(misc, d_misc, 16, hipMemcpyDeviceToHost, ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!misc[bad]) return ANOMOD_OK;
  set_error(ctx, "%s: %llu spans carry no edge %s (internal error)", pass, misc[bad], what);
  return ANOMOD_ESTATE;
}

}  // namespace anomod
