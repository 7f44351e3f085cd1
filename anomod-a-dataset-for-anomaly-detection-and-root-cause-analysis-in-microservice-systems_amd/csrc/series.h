// The device-resident series matrix and its two layouts, shared by the
// kernels that read it (ewma.hip, series_corr.hip).  Not part of the public ABI.
#pragma once

#include "common.h"

struct anomod_series {
  int device = 0;
  uint64_t T = 0, S = 0;
  float* X = nullptr;      // [T][S] rows or [ceil(T/16)][S][16] tiles (sized for the tiles)
  bool tiled = false;
  float* Z = nullptr;      // [T/W][S] (allocated lazily for the largest W seen)
  size_t z_cap = 0;
  double* m = nullptr;     // [S]
  double* v = nullptr;     // [S]
  uint32_t* n = nullptr;   // [S] valid samples seen
};

namespace anomod {

#ifndef ANOMOD_EWMA_TILE
#define ANOMOD_EWMA_TILE 16
#endif
constexpr int kTile = ANOMOD_EWMA_TILE;  // steps per tile (one lane's contiguous run)
static_assert(kTile % 16 == 0 && 64 % kTile == 0, "tile steps");
#ifndef ANOMOD_EWMA_QMAJOR
#define ANOMOD_EWMA_QMAJOR 1
#endif
// Float index of steps 4q .. 4q+3 of series s in tile `tile` (a tile holds
// kTile steps of every series: S * kTile floats).  q-major (default): the
// float4 groups of one q for all series contiguous, so a wave's load
// instruction reads 1 KiB contiguously; series-major (ANOMOD_EWMA_QMAJOR=0,
// the r01/r02 layout): each series' kTile steps contiguous.
__host__ __device__ __forceinline__ uint64_t tile_off(uint64_t tile, uint64_t S, uint64_t s,
                                                      uint64_t q) {
  if constexpr (ANOMOD_EWMA_QMAJOR) return tile * S * kTile + (q * S + s) * 4;
  else return (tile * S + s) * kTile + 4 * q;
}
#ifndef ANOMOD_ZT_TILES
#define ANOMOD_ZT_TILES 4
#endif
constexpr int kZtTiles = ANOMOD_ZT_TILES;  // tiles per load block (two blocks in flight)
// Slack tiles past ceil(T/16) a prefetch may read.  X is allocated with them
// in either layout ((padded steps + kPadTiles * kTile) * S floats), so a
// reader of rows may run kPadTiles * kTile rows past T as well.
constexpr int kPadTiles = 2 * kZtTiles;

}  // namespace anomod
