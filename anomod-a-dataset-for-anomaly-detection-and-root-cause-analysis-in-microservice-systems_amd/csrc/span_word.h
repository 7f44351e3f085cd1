// The integer latency histogram's bins and the three span-word formats of the
// dense edge stream (edge_agg.hip).  Plain C++ with no HIP dependency: the
// library includes it through common.h, and the host test of the formats
// (fuzz/span_word_check.cpp) builds it alone.
#pragma once

#include <cstdint>

#include "../../include/anomod.h"

#if defined(__HIPCC__)
#define ANOMOD_HD __host__ __device__
#else
#define ANOMOD_HD
#endif

namespace anomod {

// ---- integer latency histogram (ANOMOD_HIST_*) --------------------------
ANOMOD_HD inline uint32_t hist_bin(uint32_t v) {
  if (v < 64u) return v;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lg = 31u - (uint32_t)__clz((int)v);
#else
  const uint32_t lg = 31u - (uint32_t)__builtin_clz(v);
#endif
  const uint32_t e = lg - ANOMOD_HIST_SUB_BITS;
  return (e << ANOMOD_HIST_SUB_BITS) + (v >> e);
}

ANOMOD_HD inline void hist_bounds(uint32_t bin, uint32_t* lo, uint32_t* hi) {
  if (bin < 64u) {
    *lo = bin;
    *hi = bin;
    return;
  }
  const uint32_t e = (bin >> ANOMOD_HIST_SUB_BITS) - 1u;
  const uint64_t m = (uint64_t)(bin & ((1u << ANOMOD_HIST_SUB_BITS) - 1u)) +
                     (1u << ANOMOD_HIST_SUB_BITS);
  *lo = (uint32_t)(m << e);
  *hi = (uint32_t)(((m + 1) << e) - 1);
}

// A bin of exponent e spans 2^e durations (hi - lo + 1): 0 for bins below 64.
ANOMOD_HD inline uint32_t hist_exp(uint32_t bin) {
  return bin < 64u ? 0u : (bin >> ANOMOD_HIST_SUB_BITS) - 1u;
}
ANOMOD_HD inline uint32_t hist_lo(uint32_t bin) {
  uint32_t lo, hi;
  hist_bounds(bin, &lo, &hi);
  return lo;
}

// ---- span word of the dense edge stream (edge_agg.hip) -------------------
// One u32 per span position: code << 22 | error << 21 | duration.  The code
// field holds every code a layout can own (0 .. 511) and kWordNoCode, which
// none can: "no span here, skip"; the word of all ones is such a word.  A
// duration above kWordDurMax does not fit: its field is all ones
// (kWordDurEscape) and the reader takes dur_us at that position instead, so
// no result rests on durations being small.
constexpr uint32_t kWordDurBits = 21, kWordCodeBits = 10;
constexpr uint32_t kWordErrBit = 1u << kWordDurBits;
constexpr uint32_t kWordCodeShift = kWordDurBits + 1u;
constexpr uint32_t kWordDurEscape = (1u << kWordDurBits) - 1u;
constexpr uint32_t kWordDurMax = kWordDurEscape - 1u;  // the largest duration a word holds
constexpr uint32_t kWordNoCode = (1u << kWordCodeBits) - 1u;
constexpr uint32_t kWordSkip = 0xFFFFFFFFu;
static_assert(kWordCodeBits + 1u + kWordDurBits == 32u, "a span word is 32 bits");
ANOMOD_HD inline uint32_t span_word_pack(uint32_t code, bool error, uint32_t dur) {
  return code << kWordCodeShift | (error ? kWordErrBit : 0u) |
         (dur <= kWordDurMax ? dur : kWordDurEscape);
}
ANOMOD_HD inline uint32_t span_word_code(uint32_t w) { return w >> kWordCodeShift; }
ANOMOD_HD inline bool span_word_error(uint32_t w) { return (w & kWordErrBit) != 0u; }
// the duration field; kWordDurEscape: read dur_us at the span's position
ANOMOD_HD inline uint32_t span_word_dur(uint32_t w) { return w & kWordDurEscape; }

// ---- cell word: the second format, bin and range resolved at encode time --
// For a layout whose fields fit 32 bits the word holds, from the top,
//   code | error | cell | residual        (unused bits above the code: 0)
// cell: the absolute index of the span's cell in the layout's cell array,
// base + hist_bin(d) - first_bin; residual: d - lo(bin), e bits for a bin of
// exponent e.  The widths belong to the layout (CellFmt): code_bits holds
// every code, cell_bits every cell and two reserved values, res_bits the
// largest exponent of the layout's ranges.  Within one code (cell, residual)
// — the key, one mask — grows strictly with d, so the reader keeps min and max
// as keys and turns them back into durations once (cell_key_dur); the error
// bit sits directly above the key, so a span with the error bit compares above
// every key.  Reserved cells: all ones = "no span here" (kWordSkip is such a
// word under every width), all ones - 1 = escape: the span is not in its
// code's range (or its residual or cell does not fit) and the reader takes
// dur_us at that position; its code and error fields are valid.
struct CellFmt {
  uint32_t code_bits, cell_bits, res_bits;
};
ANOMOD_HD inline uint32_t low_mask(uint32_t bits) { return bits >= 32u ? ~0u : (1u << bits) - 1u; }
// bits to hold the values 0 .. n - 1
ANOMOD_HD inline uint32_t bits_for(uint64_t n) {
  uint32_t b = 0;
  while (b < 64u && (1ull << b) < n) ++b;
  return b;
}
// The widths of a layout of `codes` codes and `cells` cells whose widest bin
// has exponent max_exp.
ANOMOD_HD inline CellFmt cell_fmt(uint32_t codes, uint32_t cells, uint32_t max_exp) {
  return CellFmt{bits_for(codes), bits_for((uint64_t)cells + 2u), max_exp};
}
// (the code is read with one shift by key bits + 1, which has to stay below 32:
// the one layout this leaves out has a single code and a key of 31 bits)
ANOMOD_HD inline bool cell_fmt_fits(CellFmt f) {
  return f.code_bits + 1u + f.cell_bits + f.res_bits <= 32u && f.cell_bits + f.res_bits < 31u;
}
ANOMOD_HD inline uint32_t cell_key_bits(CellFmt f) { return f.cell_bits + f.res_bits; }
ANOMOD_HD inline uint32_t cell_skip(CellFmt f) { return low_mask(f.cell_bits); }
ANOMOD_HD inline uint32_t cell_escape(CellFmt f) { return low_mask(f.cell_bits) - 1u; }
ANOMOD_HD inline uint32_t cell_word_pack(CellFmt f, uint32_t code, bool error, uint32_t cell,
                                         uint32_t residual) {
  const uint32_t kb = cell_key_bits(f);
  return code << (kb + 1u) | (error ? 1u << kb : 0u) | cell << f.res_bits | residual;
}
// The word of duration d under code's layout entry {first_bin, base, width}.
ANOMOD_HD inline uint32_t cell_word_encode(CellFmt f, uint32_t code, bool error, uint32_t d,
                                           uint32_t first_bin, uint32_t base, uint32_t width) {
  const uint32_t bin = hist_bin(d), k = bin - first_bin, cell = base + k;
  if (k < width && hist_exp(bin) <= f.res_bits && cell < cell_escape(f))
    return cell_word_pack(f, code, error, cell, d - hist_lo(bin));
  return cell_word_pack(f, code, error, cell_escape(f), 0u);
}
ANOMOD_HD inline uint32_t cell_word_code(CellFmt f, uint32_t w) {
  return w >> (cell_key_bits(f) + 1u);  // (nothing above the code but in a skip word)
}
ANOMOD_HD inline uint32_t cell_word_cell(CellFmt f, uint32_t w) {
  return (w >> f.res_bits) & low_mask(f.cell_bits);
}
ANOMOD_HD inline uint32_t cell_word_residual(CellFmt f, uint32_t w) { return w & low_mask(f.res_bits); }
// the key with the error bit above it
ANOMOD_HD inline uint32_t cell_word_ekey(CellFmt f, uint32_t w) {
  return w & low_mask(cell_key_bits(f) + 1u);
}
// The duration of a key of a code whose range starts at first_bin, cell base.
ANOMOD_HD inline uint32_t cell_key_dur(CellFmt f, uint32_t key, uint32_t first_bin, uint32_t base) {
  return hist_lo(first_bin + (key >> f.res_bits) - base) + (key & low_mask(f.res_bits));
}

// ---- packed word: the third format, a cell word in 24 bits ------------------
// The codes of a layout own back-to-back ranges of its cell array, so the
// absolute cell already names the code, and almost no span needs the widest
// residual.  For a layout of widths f the packed word holds, from the top,
//   error | cell | residual              (unused bits above the error bit: 0)
// with the same cell and the same two reserved cells, in pack_fmt(f): no code
// field and pr = min(max(res_bits, code_bits), 23 - cell_bits) residual bits,
// 1 + cell_bits + pr <= 24.  Every cell-word function above reads it through
// pack_fmt(f) (the code aside).  A span escapes when it is not in its code's
// range, as before, and also when its bin's exponent exceeds pr (a wide span:
// in range, but its residual does not fit); an escape word keeps the error
// bit and carries the code in the residual field, which is therefore never
// narrower than code_bits, and has room for the 256 codes a packing layout may
// have because cell_bits <= 15.  Within a code the key still grows strictly
// with d over the spans that do not escape.
// The column keeps the word in two planes, the high 16 bits as u16 and the low
// 8 as u8 by span position (pack_split / pack_join): 3 B per span.
constexpr uint32_t kPackBits = 24, kPackMaxCodes = 256, kPackMaxCellBits = 15;
constexpr uint32_t kPackSkip = (1u << kPackBits) - 1u;  // all ones: a skip word under every width
ANOMOD_HD inline bool pack_fmt_fits(CellFmt f, uint32_t codes) {
  return cell_fmt_fits(f) && codes <= kPackMaxCodes && f.cell_bits <= kPackMaxCellBits;
}
ANOMOD_HD inline CellFmt pack_fmt(CellFmt f) {
  const uint32_t room = kPackBits - 1u - f.cell_bits;
  const uint32_t want = f.res_bits > f.code_bits ? f.res_bits : f.code_bits;
  return CellFmt{0u, f.cell_bits, want < room ? want : room};
}
// The packed word of duration d under code's layout entry; p = pack_fmt(f).
// *wide is set for an escaping span that lies inside the code's range.
ANOMOD_HD inline uint32_t pack_word_encode(CellFmt p, uint32_t code, bool error, uint32_t d,
                                           uint32_t first_bin, uint32_t base, uint32_t width,
                                           bool* wide) {
  const uint32_t bin = hist_bin(d), k = bin - first_bin, cell = base + k;
  const bool in_range = k < width && cell < cell_escape(p);
  *wide = in_range && hist_exp(bin) > p.res_bits;
  if (in_range && !*wide) return cell_word_pack(p, 0u, error, cell, d - hist_lo(bin));
  return cell_word_pack(p, 0u, error, cell_escape(p), code);
}
// the code an escape word carries
ANOMOD_HD inline uint32_t pack_word_escape_code(CellFmt p, uint32_t w) { return w & low_mask(p.res_bits); }
ANOMOD_HD inline bool pack_word_error(CellFmt p, uint32_t w) { return ((w >> cell_key_bits(p)) & 1u) != 0u; }
// The entry of a word with a cell of the layout in a cell array that keeps the
// error spans of a cell apart, 2^cell_bits entries above the cell's own:
// error << cell_bits | cell, one shift (nothing above the error bit in a
// packed word).  Below 2^cell_bits + cells.
ANOMOD_HD inline uint32_t pack_word_entry(CellFmt p, uint32_t w) { return w >> p.res_bits; }
ANOMOD_HD inline uint16_t pack_hi(uint32_t w) { return (uint16_t)(w >> 8); }
ANOMOD_HD inline uint8_t pack_lo(uint32_t w) { return (uint8_t)(w & 0xFFu); }
ANOMOD_HD inline uint32_t pack_join(uint32_t hi16, uint32_t lo8) { return hi16 << 8 | lo8; }
// byte offset of the u8 plane in a column of n span positions (16-B aligned)
ANOMOD_HD inline uint64_t pack_lo_offset(uint64_t n) { return (2ull * n + 15ull) & ~15ull; }
ANOMOD_HD inline uint64_t pack_column_bytes(uint64_t n) { return pack_lo_offset(n) + n; }

}  // namespace anomod
