// Pearson correlation of every column of a resident series matrix against up
// to ANOMOD_CORR_MAX_TARGETS target columns (include/anomod.h
// anomod_series_correlate; build-defined — the reference exports raw series
// only).  One pass over X: 4 B/sample read, K * 12 B per series written.
//
// One series per lane down T, as the sequential EWMA kernel: 32-step register
// blocks, two in flight, read from whichever layout the matrix has (float4
// loads from the 16-step tiles, one 256-B row segment per load from rows).
// Neither the matrix nor the EWMA state is written.
//
// The targets are prepared on the host: Yd[t][k] = (double)Y[t][k] - py_k with
// py_k the first finite Y[t][k], NaN where Y[t][k] is not finite.  Every lane
// of every wave reads the same Yd[t][*], at an address built from kernel
// arguments and loop counters only, so the loads are scalar loads (s_load_*)
// and a target costs no vector register.
//
// A lane carries px (its first finite sample) and per target the five sums of
// the contract and the pair count: 5 K f64 + K u32, 88 VGPRs at K = 8 beside
// the 64 of the two sample blocks (allocated: 340 with the AGPRs the compiler
// parks values in, no scratch: DESIGN.md §2.22).  A step that is no pair adds
// +0.0 to each sum, which changes no bit of it, so a block in which every
// lane's samples are finite (the dense form: no selects) and the general form
// give the same bits; both walk t in order, so the two layouts do as well.
// The dense form also needs every target present in the block (a flag per
// block from the host), so it has no branch and the scalar loads of a block's
// targets can run ahead of their use.
//
// Accuracy (pairs of |x| <= 2^62):
//   |r - r_exact| <= 8 T 2^-53 max(kx, ky) + 2^-50,
//   kx = sum (x - px)^2 / sum (x - mean)^2 over the pair set, ky likewise.
// Each f64 sum of <= T terms is within T 2^-53 of its absolute-value sum
// (first order); sxx = sum x'^2 - (sum x')^2 / n subtracts two terms each
// <= sum x'^2 = kx sxx, so sxx, syy and (by Cauchy-Schwarz on the absolute
// sums) sxy carry <= 3 T 2^-53 max(kx, ky) relative to sqrt(sxx syy);
// r = sxy / sqrt(sxx syy) combines them as e_xy + (e_xx + e_yy) / 2, |r| <= 1:
// <= 6 T 2^-53 k, rounded up to 8 for the second-order terms; 2^-50 covers the
// product, square root, divide and clamp (each correctly rounded).
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.h"
#include "series.h"

namespace anomod {
namespace {

constexpr int kCorrU = 32;                                      // steps per load block
constexpr int kCorrTiles = kTile >= kCorrU ? 1 : kCorrU / kTile;  // tiles per load block
constexpr int kCorrSteps = kCorrTiles * kTile;
// the prefetch of the block after the last one stays inside the allocation
static_assert(2 * kCorrTiles <= kPadTiles && 2 * kCorrSteps <= kPadTiles * kTile, "prefetch slack");

template <int K>
struct CorrAcc {
  double px;
  bool have;  // px is set
  double sx[K], sy[K], sxx[K], syy[K], sxy[K];
  uint32_t n[K];
};

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) <= FLT_MAX; }

// One step, any sample: the pivot is the first finite sample whatever Y holds;
// a (sample, target) that is no pair contributes +0.0 and no count.
template <int K>
__device__ __forceinline__ void corr_step(CorrAcc<K>& a, float x, const double* __restrict__ y) {
  const bool xf = finite_f32(x);
  const double xd = (double)x;
  a.px = (xf && !a.have) ? xd : a.px;
  a.have = a.have || xf;
  const double xp = xd - a.px;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double yk = y[k];
    const bool pair = xf && yk == yk;
    const double xm = pair ? xp : 0.0, ym = pair ? yk : 0.0;
    a.sx[k] += xm;
    a.sy[k] += ym;
    a.sxx[k] = fma(xm, xm, a.sxx[k]);
    a.syy[k] = fma(ym, ym, a.syy[k]);
    a.sxy[k] = fma(xm, ym, a.sxy[k]);
    a.n[k] += pair ? 1u : 0u;
  }
}

// The same step where every (sample, target) is a pair: a finite sample of a
// lane whose pivot is set, every target present.  The pair arm of corr_step
// with the same expressions, so the same bits; the caller adds the block's
// steps to n.
template <int K>
__device__ __forceinline__ void corr_step_dense(CorrAcc<K>& a, float x,
                                                const double* __restrict__ y) {
  const double xp = (double)x - a.px;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double yk = y[k];
    a.sx[k] += xp;
    a.sy[k] += yk;
    a.sxx[k] = fma(xp, xp, a.sxx[k]);
    a.syy[k] = fma(yk, yk, a.syy[k]);
    a.sxy[k] = fma(xp, yk, a.sxy[k]);
  }
}

// r of one (target, series) from its sums, as the contract states it.
__device__ __forceinline__ double corr_finish(double sx, double sy, double sxx, double syy,
                                              double sxy, uint32_t n, uint32_t min_pairs) {
#pragma clang fp contract(off)
  if (n < (min_pairs > 2u ? min_pairs : 2u)) return NAN;
  const double dn = (double)n;
  const double cxx = sxx - sx * sx / dn;
  const double cyy = syy - sy * sy / dn;
  const double cxy = sxy - sx * sy / dn;
  if (!(cxx > 0.0) || !(cyy > 0.0)) return NAN;
  const double r = cxy / sqrt(cxx * cyy);
  return fmin(fmax(r, -1.0), 1.0);
}

// kTiled: X is the tiled layout (series.h), else rows X[T][S].  Yd: [T][K]
// prepared targets; ydense[b] != 0: block b lies inside T and no target misses
// a step of it.  r, n: [K][S].
template <int K, bool kTiled>
__global__ __launch_bounds__(64) void series_corr_kernel(const float* __restrict__ X, uint64_t T,
                                                          uint64_t S,
                                                          const double* __restrict__ Yd,
                                                          const uint32_t* __restrict__ ydense,
                                                          uint32_t min_pairs,
                                                          double* __restrict__ r,
                                                          uint32_t* __restrict__ n) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  CorrAcc<K> a;
  a.px = 0.0;
  a.have = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    a.sx[k] = a.sy[k] = a.sxx[k] = a.syy[k] = a.sxy[k] = 0.0;
    a.n[k] = 0u;
  }
  float4 b0[kCorrSteps / 4], b1[kCorrSteps / 4];
  // unconditional loads of block `blk` (steps blk * kCorrSteps ..): the block
  // after the last one lies in the allocation's slack and is never consumed
  auto load = [&](float4* buf, uint64_t blk) {
    if constexpr (kTiled) {
#pragma unroll
      for (int j = 0; j < kCorrTiles; ++j)
#pragma unroll
        for (int q = 0; q < kTile / 4; ++q)
          buf[j * (kTile / 4) + q] = *reinterpret_cast<const float4*>(
              X + tile_off(blk * kCorrTiles + j, S, s, q));
    } else {
      const float* col = X + blk * kCorrSteps * S + s;
#pragma unroll
      for (int i = 0; i < kCorrSteps / 4; ++i)
        buf[i] = make_float4(col[(4 * i) * S], col[(4 * i + 1) * S], col[(4 * i + 2) * S],
                             col[(4 * i + 3) * S]);
    }
  };
  bool started = false;  // every lane of the wave has its pivot
  auto consume = [&](const float4* buf, uint64_t blk) __attribute__((always_inline)) {
    const uint64_t t0 = blk * kCorrSteps;
    const double* y = Yd + t0 * K;
    if (t0 + kCorrSteps <= T) {  // whole block inside T (wave-uniform)
      bool dense = false;
      if (started && ydense[blk] != 0u) {
        float acc = 0.f;  // x - x is 0 for a finite x, NaN otherwise
#pragma unroll
        for (int i = 0; i < kCorrSteps / 4; ++i)
          acc += ((buf[i].x - buf[i].x) + (buf[i].y - buf[i].y)) +
                 ((buf[i].z - buf[i].z) + (buf[i].w - buf[i].w));
        dense = __all(acc == 0.f);
      }
      if (dense) {
#pragma unroll
        for (int i = 0; i < kCorrSteps / 4; ++i) {
          corr_step_dense<K>(a, buf[i].x, y + (4 * i) * K);
          corr_step_dense<K>(a, buf[i].y, y + (4 * i + 1) * K);
          corr_step_dense<K>(a, buf[i].z, y + (4 * i + 2) * K);
          corr_step_dense<K>(a, buf[i].w, y + (4 * i + 3) * K);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) a.n[k] += (uint32_t)kCorrSteps;
      } else {
#pragma unroll
        for (int i = 0; i < kCorrSteps / 4; ++i) {
          corr_step<K>(a, buf[i].x, y + (4 * i) * K);
          corr_step<K>(a, buf[i].y, y + (4 * i + 1) * K);
          corr_step<K>(a, buf[i].z, y + (4 * i + 2) * K);
          corr_step<K>(a, buf[i].w, y + (4 * i + 3) * K);
        }
        started = started || __all(a.have);
      }
    } else {  // the last block: steps past T hold padding or nothing defined
#pragma unroll
      for (int i = 0; i < kCorrSteps / 4; ++i) {
        const float xs[4] = {buf[i].x, buf[i].y, buf[i].z, buf[i].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (t0 + 4 * i + e < T) corr_step<K>(a, xs[e], y + (4 * i + e) * K);
      }
    }
  };
  const uint64_t nb = (T + kCorrSteps - 1) / kCorrSteps;
  load(b0, 0);
  uint64_t blk = 0;
  while (blk < nb) {
    load(b1, blk + 1);
    consume(b0, blk);
    if (++blk >= nb) break;
    load(b0, blk + 1);
    consume(b1, blk);
    ++blk;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    r[(uint64_t)k * S + s] =
        corr_finish(a.sx[k], a.sy[k], a.sxx[k], a.syy[k], a.sxy[k], a.n[k], min_pairs);
    n[(uint64_t)k * S + s] = a.n[k];
  }
}

template <int K>
void launch_corr(anomod_ctx* ctx, const anomod_series* ser, const double* Yd,
                 const uint32_t* ydense, uint32_t min_pairs, double* r, uint32_t* n) {
  const unsigned strips = (unsigned)((ser->S + 63) / 64);
  if (ser->tiled)
    hipLaunchKernelGGL((series_corr_kernel<K, true>), dim3(strips), dim3(64), 0, ctx->stream,
                       ser->X, ser->T, ser->S, Yd, ydense, min_pairs, r, n);
  else
    hipLaunchKernelGGL((series_corr_kernel<K, false>), dim3(strips), dim3(64), 0, ctx->stream,
                       ser->X, ser->T, ser->S, Yd, ydense, min_pairs, r, n);
}

int check_targets(anomod_ctx* ctx, const char* who, uint32_t K) {
  ANOMOD_REQUIRE(ctx, K >= 1 && K <= ANOMOD_CORR_MAX_TARGETS,
                 "%s: K=%u targets outside 1 .. %d", who, K, ANOMOD_CORR_MAX_TARGETS);
  return ANOMOD_OK;
}

}  // namespace
}  // namespace anomod

using namespace anomod;

extern "C" {

int anomod_series_correlate(anomod_ctx* ctx, const anomod_series* ser, const float* Y, uint32_t K,
                            uint32_t min_pairs, double* r, uint32_t* n) {
  ANOMOD_REQUIRE(nullptr, ctx, "anomod_series_correlate: NULL ctx");
  ANOMOD_REQUIRE(ctx, ser && Y && r, "anomod_series_correlate: NULL argument");
  if (int rc = check_targets(ctx, "anomod_series_correlate", K)) return rc;
  const uint64_t T = ser->T, S = ser->S;
  ANOMOD_REQUIRE(ctx, T < (1ull << 32), "anomod_series_correlate: T=%llu must be below 2^32",
                 (unsigned long long)T);
  if (T == 0 || S == 0) return ANOMOD_OK;
  if (int rc = bind(ctx)) return rc;
  // the kernels exist for 1, 2, 4 and 8 targets: pad with targets of all zeros
  // (their sums are separate registers and their results are not copied out)
  uint32_t Kt = 1;
  while (Kt < K) Kt *= 2;
  const uint64_t nb = (T + kCorrSteps - 1) / kCorrSteps;
  std::vector<double> yd((size_t)T * Kt, 0.0);
  std::vector<uint32_t> ydense(nb, 0u);
  for (uint64_t b = 0; (b + 1) * kCorrSteps <= T; ++b) ydense[b] = 1u;
  for (uint32_t k = 0; k < K; ++k) {
    bool have = false;
    double py = 0.0;
    for (uint64_t t = 0; t < T; ++t) {
      const float y = Y[t * K + k];
      if (!(std::fabs(y) <= FLT_MAX)) {
        yd[t * Kt + k] = (double)NAN;
        ydense[t / kCorrSteps] = 0u;
        continue;
      }
      if (!have) {
        py = (double)y;
        have = true;
      }
      yd[t * Kt + k] = (double)y - py;
    }
  }
  const size_t ybytes = yd.size() * 8, rbytes = (size_t)Kt * S * 8, nbytes = (size_t)Kt * S * 4;
  const size_t fbytes = ydense.size() * 4;
  char* dbuf = nullptr;  // Yd | r | n | ydense
  if (dev_malloc(ctx, (void**)&dbuf, ybytes + rbytes + nbytes + fbytes) != hipSuccess) {
    set_error(ctx, "hipMalloc(%zu) for the correlation targets and results failed",
              ybytes + rbytes + nbytes + fbytes);
    return ANOMOD_ENOMEM;
  }
  double* d_y = reinterpret_cast<double*>(dbuf);
  double* d_r = reinterpret_cast<double*>(dbuf + ybytes);
  uint32_t* d_n = reinterpret_cast<uint32_t*>(dbuf + ybytes + rbytes);
  uint32_t* d_f = reinterpret_cast<uint32_t*>(dbuf + ybytes + rbytes + nbytes);
  hipError_t e = hipMemcpyAsync(d_y, yd.data(), ybytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_f, ydense.data(), fbytes, hipMemcpyHostToDevice, ctx->stream);
  int rc = ANOMOD_OK;
  if (e == hipSuccess) rc = stage_begin(ctx, kStageSeriesCorr);
  if (e == hipSuccess && rc == ANOMOD_OK) {
    switch (Kt) {
      case 1: launch_corr<1>(ctx, ser, d_y, d_f, min_pairs, d_r, d_n); break;
      case 2: launch_corr<2>(ctx, ser, d_y, d_f, min_pairs, d_r, d_n); break;
      case 4: launch_corr<4>(ctx, ser, d_y, d_f, min_pairs, d_r, d_n); break;
      default: launch_corr<8>(ctx, ser, d_y, d_f, min_pairs, d_r, d_n); break;
    }
    e = hipGetLastError();
    if (e == hipSuccess) rc = stage_end(ctx, kStageSeriesCorr);
  }
  if (e == hipSuccess && rc == ANOMOD_OK)
    e = hipMemcpyAsync(r, d_r, (size_t)K * S * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && rc == ANOMOD_OK && n)
    e = hipMemcpyAsync(n, d_n, (size_t)K * S * 4, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  (void)hipFree(dbuf);
  if (rc != ANOMOD_OK) return rc;
  if (e != hipSuccess) {
    set_error(ctx, "series correlation failed: %s", hipGetErrorString(e));
    return ANOMOD_EHIP;
  }
  return ANOMOD_OK;
}

int anomod_correlate(anomod_ctx* ctx, const float* X, uint64_t T, uint64_t S, const float* Y,
                     uint32_t K, uint32_t min_pairs, double* r, uint32_t* n) {
  ANOMOD_REQUIRE(nullptr, ctx, "anomod_correlate: NULL ctx");
  ANOMOD_REQUIRE(ctx, X && Y && r, "anomod_correlate: NULL argument");
  if (int rc = check_targets(ctx, "anomod_correlate", K)) return rc;
  ANOMOD_REQUIRE(ctx, T < (1ull << 32), "anomod_correlate: T=%llu must be below 2^32",
                 (unsigned long long)T);
  if (T == 0 || S == 0) return ANOMOD_OK;
  anomod_series* ser = nullptr;
  if (int rc = anomod_series_create(ctx, T, S, &ser)) return rc;
  int rc = anomod_series_upload(ctx, ser, X);
  if (rc == ANOMOD_OK) rc = anomod_series_correlate(ctx, ser, Y, K, min_pairs, r, n);
  anomod_series_free(ser);
  return rc;
}

}  // extern "C"
