// Host check of the cell-word format (span_word.h), built with
// -fsanitize=address,undefined by `make wordcheck`: pack / unpack / key
// functions at every bin exponent and at the borders of the bins, the escape
// rule restated independently, key order against duration order, and the skip
// word under every width combination.  Prints "ok <checks>" and exits 0, or
// names the first failure and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../span_word.h"

using namespace anomod;

static unsigned long long g_checks = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    ++g_checks;                                       \
    if (!(cond)) {                                    \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                   \
      fprintf(stderr, "\n");                          \
      exit(1);                                        \
    }                                                 \
  } while (0)

// first and last bin of exponent e (e = 0: the bins below 64, one value each)
static void exp_bins(uint32_t e, uint32_t* first, uint32_t* last) {
  if (e == 0) {
    *first = 0;
    *last = 63;
  } else {
    *first = (e + 1) << ANOMOD_HIST_SUB_BITS;
    *last = *first + (1u << ANOMOD_HIST_SUB_BITS) - 1;
  }
}

// One duration under one code entry: round trip, or escape exactly when the
// rule (restated here, not taken from cell_word_encode) says so.
static void one(CellFmt f, uint32_t code, bool error, uint32_t d, uint32_t first_bin, uint32_t base,
                uint32_t width) {
  const uint32_t bin = hist_bin(d);
  uint32_t lo, hi;
  hist_bounds(bin, &lo, &hi);
  CHECK(lo <= d && d <= hi, "d=%u bin=%u", d, bin);
  const uint32_t e = bin < 64 ? 0 : (bin >> ANOMOD_HIST_SUB_BITS) - 1;
  CHECK(hi - lo + 1 == 1ull << e, "bin %u spans %u", bin, hi - lo + 1);
  const bool in_range = bin >= first_bin && bin - first_bin < width;
  const bool fits = in_range && e <= f.res_bits &&
                    (uint64_t)base + (bin - first_bin) < (1ull << f.cell_bits) - 2;
  const uint32_t w = cell_word_encode(f, code, error, d, first_bin, base, width);
  const uint32_t kb = cell_key_bits(f);
  CHECK(w != kWordSkip && cell_word_cell(f, w) != cell_skip(f), "d=%u encodes as a skip word", d);
  CHECK(cell_word_code(f, w) == code, "code %u -> %u (d=%u)", code, cell_word_code(f, w), d);
  CHECK(((cell_word_ekey(f, w) >> kb) & 1u) == (error ? 1u : 0u), "error bit (d=%u)", d);
  if (!fits) {
    CHECK(cell_word_cell(f, w) == cell_escape(f), "d=%u must escape (bin %u, e %u)", d, bin, e);
    return;
  }
  const uint32_t cell = cell_word_cell(f, w);
  CHECK(cell == base + bin - first_bin, "cell %u (d=%u)", cell, d);
  CHECK(cell_word_residual(f, w) == d - lo, "residual (d=%u)", d);
  const uint32_t key = cell_word_ekey(f, w) & low_mask(kb);
  CHECK(key == (cell << f.res_bits | (d - lo)), "key (d=%u)", d);
  CHECK(cell_key_dur(f, key, first_bin, base) == d, "round trip %u -> %u", d,
        cell_key_dur(f, key, first_bin, base));
  // the error bit lifts the word's compare value above every plain key
  if (error) CHECK(cell_word_ekey(f, w) > low_mask(kb), "ekey of an error span (d=%u)", d);
}

int main() {
  // -- every exponent, the borders of its first and last bin ----------------
  for (uint32_t e = 0; e <= 26; ++e) {
    uint32_t b0, b1;
    exp_bins(e, &b0, &b1);
    std::vector<uint32_t> ds;
    for (uint32_t b : {b0, b1}) {
      uint32_t lo, hi;
      hist_bounds(b, &lo, &hi);
      for (uint64_t d : {(uint64_t)lo, (uint64_t)hi, (uint64_t)lo + 1, (uint64_t)hi + 1,
                         (uint64_t)lo - 1, (uint64_t)hi - 1})
        if (d <= 0xFFFFFFFFull) ds.push_back((uint32_t)d);  // (not 0 - 1, not 2^32)
    }
    // residual widths below, at and above the exponent; ranges that hold the
    // exponent's bins wholly, partly and not at all; bases that push the last
    // cells into the reserved values
    for (uint32_t res_bits : {e ? e - 1 : 0u, e, e + 1 <= 26 ? e + 1 : 26u}) {
      for (uint32_t codes : {1u, 2u, 64u, 512u}) {
        const uint32_t code = codes - 1;
        struct R {
          uint32_t first, width;
        };
        const uint32_t nb = b1 - b0 + 1;
        for (R r : {R{b0, nb}, R{b0 ? b0 - 1 : 0, nb + 2}, R{b0 + 1, nb > 2 ? nb - 2 : 0}, R{b0, 1},
                    R{b1, 1}, R{b1 + 1 < ANOMOD_HIST_BINS ? b1 + 1 : 0, 1}, R{0, 0}}) {
          for (uint32_t base : {0u, 5u, 100u}) {
            for (uint32_t spare : {0u, 1u, 40u}) {  // cells the layout has past this range
              const uint32_t cells = base + r.width + spare;
              CellFmt f = cell_fmt(codes, cells, res_bits);
              if (!cell_fmt_fits(f)) continue;
              CHECK((1ull << f.cell_bits) >= (uint64_t)cells + 2, "cell_bits %u for %u cells",
                    f.cell_bits, cells);
              for (uint32_t d : ds)
                for (bool err : {false, true}) one(f, code, err, d, r.first, base, r.width);
              // a format one cell bit short: the top cells collide with the reserved values
              if (f.cell_bits > 1) {
                CellFmt g = f;
                g.cell_bits -= 1;
                for (uint32_t d : ds) one(g, code, true, d, r.first, base, r.width);
              }
            }
          }
        }
      }
    }
  }
  // -- key order equals duration order within a code ------------------------
  {
    // a code over all bins up to exponent 11 (the SocialNetwork shape)
    uint32_t b0, b1;
    exp_bins(11, &b0, &b1);
    const uint32_t first = 17, width = b1 - first + 1, base = 300;
    CellFmt f = cell_fmt(35, base + width, 11);
    CHECK(cell_fmt_fits(f), "SN-like format");
    uint32_t lo, hi, prev_key = 0;
    hist_bounds(first, &lo, &hi);
    const uint32_t d0 = lo;
    hist_bounds(b1, &lo, &hi);
    for (uint32_t d = d0; d <= hi; ++d) {
      const uint32_t w = cell_word_encode(f, 34, (d & 7u) == 0u, d, first, base, width);
      CHECK(cell_word_cell(f, w) < cell_escape(f), "d=%u escapes", d);
      const uint32_t key = cell_word_ekey(f, w) & low_mask(cell_key_bits(f));
      if (d > d0) CHECK(key > prev_key, "key order at d=%u", d);
      CHECK(cell_key_dur(f, key, first, base) == d, "round trip at d=%u", d);
      prev_key = key;
    }
  }
  // -- all ones is a skip word under every width combination ----------------
  for (uint32_t cb = 0; cb <= 10; ++cb)
    for (uint32_t lb = 1; lb <= 17; ++lb)
      for (uint32_t rb = 0; rb <= 26; ++rb) {
        CellFmt f{cb, lb, rb};
        if (!cell_fmt_fits(f)) {
          CHECK(cb + 1 + lb + rb > 32 || lb + rb >= 31, "fits rule %u %u %u", cb, lb, rb);
          continue;
        }
        CHECK(cell_word_cell(f, kWordSkip) == cell_skip(f), "skip under %u %u %u", cb, lb, rb);
        CHECK(cell_skip(f) != cell_escape(f) && cell_escape(f) + 1 == cell_skip(f), "reserved");
      }
  {  // one code and one cell: code_bits 0, cell_bits 2
    CellFmt f = cell_fmt(1, 1, 0);
    CHECK(f.code_bits == 0 && f.cell_bits == 2 && cell_fmt_fits(f), "one code, one cell");
    CHECK(cell_word_cell(f, kWordSkip) == cell_skip(f), "skip, one code and one cell");
    one(f, 0, true, 7, 7, 0, 1);
    one(f, 0, false, 8, 7, 0, 1);
  }
  CHECK(!cell_fmt_fits(CellFmt{9, 16, 7}) && cell_fmt_fits(CellFmt{9, 15, 7}), "33 and 32 bits");
  CHECK(!cell_fmt_fits(CellFmt{0, 5, 26}) && cell_fmt_fits(CellFmt{0, 4, 26}), "code shift below 32");
  printf("ok %llu\n", g_checks);
  return 0;
}
