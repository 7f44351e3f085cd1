// Host side of a span-walk call (walk.h): the trace range of a set, the
// call's workspace, the long-trace count and the scan choice.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "walk.h"

namespace anomod {
namespace {

using namespace chunk;

// Traces and spans of the set that outgrow a chunk: cnt[0] traces, cnt[1]
// spans (sizes the long-trace list and the per-span scratch before the walk).
__global__ __launch_bounds__(256) void long_count_kernel(const uint64_t* __restrict__ trace_ptr,
                                                         uint64_t n_traces,
                                                         unsigned long long* __restrict__ cnt) {
  unsigned long long nt = 0, ns = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n_traces;
       t += (uint64_t)gridDim.x * 256) {
    const uint64_t L = trace_ptr[t + 1] - trace_ptr[t];
    if (L > (uint64_t)kStage) {
      nt += 1;
      ns += L;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    nt += __shfl_xor(nt, o);
    ns += __shfl_xor(ns, o);
  }
  if ((threadIdx.x & 63) == 0 && nt) {
    atomicAdd(&cnt[0], nt);
    atomicAdd(&cnt[1], ns);
  }
}

}  // namespace

int trace_span_range(anomod_ctx* ctx, const anomod_spans* spans, uint64_t in_traces[2],
                     const char* who) {
  in_traces[0] = in_traces[1] = 0;
  const uint64_t n = spans->n_spans, nt = spans->n_traces;
  if (!(nt && n)) return ANOMOD_OK;
  ANOMOD_HIP(ctx, hipMemcpyAsync(in_traces, spans->trace_ptr, 8, hipMemcpyDeviceToHost,
                                 ctx->stream));
  ANOMOD_HIP(ctx, hipMemcpyAsync(in_traces + 1, spans->trace_ptr + nt, 8, hipMemcpyDeviceToHost,
                                 ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (in_traces[0] <= in_traces[1] && in_traces[1] <= n) return ANOMOD_OK;
  set_error(ctx, "%strace_ptr range [%llu, %llu) outside the set's %llu spans", who,
            (unsigned long long)in_traces[0], (unsigned long long)in_traces[1],
            (unsigned long long)n);
  in_traces[0] = in_traces[1] = 0;
  return ANOMOD_EINVAL;
}

CallWorkspace::~CallWorkspace() {
  if (!words && !block) return;
  (void)hipStreamSynchronize(ctx->stream);
  if (words) (void)hipFree(words);
  if (block) (void)hipFree(block);
}

int CallWorkspace::take(void** p, size_t bytes, const char* what) {
  if (dev_malloc(ctx, p, bytes) == hipSuccess) return ANOMOD_OK;
  (void)hipGetLastError();
  *p = nullptr;
  set_error(ctx, "hipMalloc(%zu) for the %s workspace failed", bytes, what);
  return ANOMOD_ENOMEM;
}

int count_long_traces(anomod_ctx* ctx, const anomod_spans* spans, unsigned long long* d_words,
                      unsigned long long nlong[2]) {
  nlong[0] = nlong[1] = 0ull;
  if (spans->max_trace_len <= (uint64_t)kStage) return ANOMOD_OK;
  const uint64_t nt = spans->n_traces;
  ANOMOD_HIP(ctx, hipMemsetAsync(d_words, 0, 16, ctx->stream));
  hipLaunchKernelGGL(long_count_kernel,
                     dim3((unsigned)std::min<uint64_t>((nt + 255) / 256, 4ull * ctx->num_cus)),
                     dim3(256), 0, ctx->stream, spans->trace_ptr, nt, d_words);
  ANOMOD_HIP(ctx, hipGetLastError());
  ANOMOD_HIP(ctx, hipMemcpyAsync(nlong, d_words, 16, hipMemcpyDeviceToHost, ctx->stream));
  ANOMOD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANOMOD_OK;
}

int pick_walk_scan(anomod_ctx* ctx, const anomod_spans* spans, uint32_t S,
                   unsigned long long* d_cnt, int* scan) {
  // The scan the edge kernels would use for the set (its order hint is probed
  // when unknown: the value the first aggregation would find).
  bool uni = false;
  if (int rc = span_scan_choice(ctx, spans, d_cnt, &uni)) return rc;
  const uint32_t E = (S + ANOMOD_ROOT_ROWS) * S;
  const bool long_set = spans->max_trace_len != ~0ull && spans->max_trace_len > (uint64_t)kStage;
  *scan = !uni ? kScanFwd : (E > kNarrowRows || long_set) ? kScanSplit : kScanBidir;
  return ANOMOD_OK;
}

const char* scan_name(int scan) {
  return scan == kScanFwd ? "forward" : scan == kScanSplit ? "split" : "bidir";
}

void log_walk_kernel(const char* pass, const char* kernel, int scan, unsigned long long n_long) {
  if (const char* lg = getenv("ANOMOD_LOG_KERNEL"); lg && lg[0] == '1')  // (tests)
    fprintf(stderr, "anomod: %s kernel %s<%s>, %llu long traces\n", pass, kernel, scan_name(scan),
            n_long);
}

}  // namespace anomod
