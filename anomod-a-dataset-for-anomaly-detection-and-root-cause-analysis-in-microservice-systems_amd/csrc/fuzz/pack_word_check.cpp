// Host check of the packed-word format (span_word.h), built with
// -fsanitize=address,undefined by `make packcheck`: pack and unpack against an
// independent restatement of the rule over random layouts, the field extremes,
// the reserved values under every width, key order against duration order
// within a code, the code an escape word carries, and the split into the two
// planes of the column with its rejoin.  Prints "ok <checks>" and exits 0, or
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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return g_rng * 0x2545F4914F6CDD1Dull;
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

struct Code {
  uint32_t first, base, width;
};

// The rule, restated: widths of the 24-bit word from the layout's counts.
struct Widths {
  bool packs;
  uint32_t cell_bits, pr;
};
static Widths widths(uint32_t codes, uint32_t cells, uint32_t max_exp) {
  uint32_t code_bits = 0, cell_bits = 0;
  while ((1ull << code_bits) < codes) ++code_bits;
  while ((1ull << cell_bits) < (uint64_t)cells + 2) ++cell_bits;
  const bool cell_words = code_bits + 1 + cell_bits + max_exp <= 32 && cell_bits + max_exp < 31;
  Widths w;
  w.packs = cell_words && codes <= 256 && cell_bits <= 15;
  w.cell_bits = cell_bits;
  const uint32_t want = max_exp > code_bits ? max_exp : code_bits;  // an escape word holds a code
  w.pr = want < 23 - cell_bits ? want : 23 - cell_bits;
  return w;
}

// One duration under one code of a packing layout: the word, its two planes,
// and what a reader takes from it.
static void one(CellFmt f, Widths m, uint32_t code, const Code& c, bool error, uint32_t d) {
  const CellFmt p = pack_fmt(f);
  CHECK(p.code_bits == 0 && p.cell_bits == m.cell_bits && p.res_bits == m.pr, "pack_fmt %u %u",
        p.cell_bits, p.res_bits);
  const uint32_t kb = m.cell_bits + m.pr;
  CHECK(1 + kb <= 24 && code < (1u << m.pr), "24 bits, and room for a code (kb=%u pr=%u)", kb, m.pr);
  const uint32_t bin = hist_bin(d);
  uint32_t lo, hi;
  hist_bounds(bin, &lo, &hi);
  const uint32_t e = bin < 64 ? 0 : (bin >> ANOMOD_HIST_SUB_BITS) - 1;
  const bool in_range = bin >= c.first && bin - c.first < c.width;
  const bool is_wide = in_range && e > m.pr;
  bool wide = !is_wide;
  const uint32_t w = pack_word_encode(p, code, error, d, c.first, c.base, c.width, &wide);
  CHECK(wide == is_wide, "wide flag (d=%u)", d);
  CHECK(w < (1u << 24), "24 bits (d=%u)", d);
  CHECK(w != kPackSkip, "d=%u encodes as a skip word", d);
  CHECK(w >> (kb + 1) == 0, "bits above the error bit (d=%u)", d);
  CHECK(pack_word_error(p, w) == error && ((w >> kb) & 1u) == (error ? 1u : 0u), "error bit (d=%u)", d);
  // the two planes and back
  const uint16_t h = pack_hi(w);
  const uint8_t l = pack_lo(w);
  CHECK(h == (w >> 8) && l == (w & 0xFF) && pack_join(h, l) == w, "planes (w=%06x)", w);
  const uint32_t cell = (w >> m.pr) & ((1u << m.cell_bits) - 1);
  CHECK(cell == cell_word_cell(p, w), "cell field");
  if (!in_range || is_wide) {
    CHECK(cell == (1u << m.cell_bits) - 2, "d=%u must escape (bin %u, e %u)", d, bin, e);
    CHECK((w & ((1u << m.pr) - 1)) == code && pack_word_escape_code(p, w) == code,
          "the code of an escape word: %u", code);
    return;
  }
  CHECK(cell == c.base + bin - c.first, "cell %u (d=%u)", cell, d);
  CHECK(cell < (1u << m.cell_bits) - 2, "a cell, not a reserved value");
  CHECK(cell_word_residual(p, w) == d - lo && d - lo < (1u << m.pr), "residual (d=%u)", d);
  const uint32_t key = cell_word_ekey(p, w) & low_mask(kb);
  CHECK(key == (cell << m.pr | (d - lo)), "key (d=%u)", d);
  CHECK(cell_key_dur(p, key, c.first, c.base) == d, "round trip %u", d);
  if (error) CHECK(cell_word_ekey(p, w) > low_mask(kb), "ekey of an error span (d=%u)", d);
}

int main() {
  // -- random layouts against the restated rule ------------------------------
  unsigned packed = 0, wide_layouts = 0;
  for (int it = 0; it < 4000; ++it) {
    const uint32_t codes = it % 7 == 0 ? 256u : it % 11 == 0 ? 257u : 1u + below(300);
    const uint32_t top_exp = below(27);
    std::vector<Code> lay;
    uint32_t cells = 0, max_exp = 0;
    const uint32_t span = it % 5 == 0 ? 200u : 12u;  // bins per range, at most
    for (uint32_t c = 0; c < codes; ++c) {
      const uint32_t last_bin = top_exp == 0 ? below(64) : ((top_exp + 1) << 5) + below(32);
      const uint32_t width = 1 + below(span);
      const uint32_t last = below(4) ? (last_bin > below(40) ? last_bin - below(40) : last_bin) : last_bin;
      const uint32_t first = last + 1 >= width ? last + 1 - width : 0;
      lay.push_back(Code{first, cells, last - first + 1});
      cells += last - first + 1;
      const uint32_t e = hist_exp(last);
      if (e > max_exp) max_exp = e;
    }
    const Widths m = widths(codes, cells, max_exp);
    const CellFmt f = cell_fmt(codes, cells, max_exp);
    CHECK(pack_fmt_fits(f, codes) == m.packs, "rule: %u codes %u cells exp %u", codes, cells, max_exp);
    if (!m.packs) continue;
    ++packed;
    if (m.pr < max_exp) ++wide_layouts;
    for (uint32_t c : {0u, codes - 1, below(codes)}) {
      const Code& k = lay[c];
      uint32_t lo, hi;
      std::vector<uint32_t> ds;
      for (uint32_t b : {k.first, k.first + k.width - 1, k.first + below(k.width)}) {
        hist_bounds(b, &lo, &hi);
        for (uint64_t d : {(uint64_t)lo, (uint64_t)hi, (uint64_t)lo - 1, (uint64_t)hi + 1,
                           (uint64_t)lo + below(hi - lo + 1)})
          if (d <= 0xFFFFFFFFull) ds.push_back((uint32_t)d);
      }
      // the residual borders at pr inside a bin of exponent pr and pr + 1
      for (uint32_t e : {m.pr, m.pr + 1}) {
        if (e > 26 || e == 0) continue;
        hist_bounds((e + 1) << 5, &lo, &hi);
        const uint32_t step = 1u << m.pr;
        for (uint32_t d : {lo, lo + step - 1, lo + step, hi}) ds.push_back(d);
      }
      ds.push_back(0u);
      ds.push_back(0xFFFFFFFFu);
      for (uint32_t d : ds)
        for (bool err : {false, true}) one(f, m, c, k, err, d);
    }
  }
  CHECK(packed > 500 && wide_layouts > 50, "coverage: %u packed, %u with wide bins", packed, wide_layouts);
  // -- field extremes ---------------------------------------------------------
  {  // 15 cell bits, 8 residual bits, code 255 in an escape word with the error bit
    const uint32_t cells = (1u << 15) - 2;
    const CellFmt f = cell_fmt(256, cells, 8);  // 8 + 1 + 15 + 8: the last layout cell words take
    CHECK(f.cell_bits == 15 && pack_fmt_fits(f, 256), "15 cell bits pack");
    const CellFmt p = pack_fmt(f);
    CHECK(p.res_bits == 8 && cell_key_bits(p) == 23, "pr = 8");
    const Widths m = widths(256, cells, 8);
    // the last cell, every residual bit, the error bit: the largest word that is a span
    uint32_t lo, hi;
    hist_bounds(9u << 5, &lo, &hi);  // the first bin of exponent 8
    const Code last{9u << 5, cells - 1, 1};
    one(f, m, 255, last, true, hi);
    bool wide = false;
    const uint32_t w = pack_word_encode(p, 255, true, hi, last.first, last.base, last.width, &wide);
    CHECK(w == (1u << 23 | (cells - 1) << 8 | 0xFF) && w < kPackSkip - 0x1FF, "the largest span word %06x", w);
    one(f, m, 0, Code{0, 0, 1}, false, 0);  // the smallest: word 0
    CHECK(pack_word_encode(p, 0, false, 0, 0, 0, 1, &wide) == 0u, "the smallest span word");
    // out of range and wide, code 255 and code 0
    one(f, m, 255, last, true, hi + 1);
    one(f, m, 0, Code{12u << 5, 7, 40}, true, 1u << 16);
    CHECK(cell_fmt_fits(cell_fmt(257, 1000, 8)) && !pack_fmt_fits(cell_fmt(257, 1000, 8), 257) &&
              pack_fmt_fits(cell_fmt(256, 1000, 8), 256),
          "257 codes");
    CHECK(cell_fmt_fits(cell_fmt(16, cells + 1, 8)) && !pack_fmt_fits(cell_fmt(16, cells + 1, 8), 16) &&
              pack_fmt_fits(cell_fmt(16, cells, 8), 16),
          "16 cell bits");
    CHECK(!pack_fmt_fits(cell_fmt(2, 100, 26), 2) == !cell_fmt_fits(cell_fmt(2, 100, 26)), "cell words first");
  }
  // -- the reserved values under every width ----------------------------------
  for (uint32_t lb = 1; lb <= 15; ++lb)
    for (uint32_t rb = 0; rb <= 26; ++rb) {
      const CellFmt f{8, lb, rb};
      if (!cell_fmt_fits(f)) continue;
      const CellFmt p = pack_fmt(f);
      CHECK(1 + p.cell_bits + p.res_bits <= 24 && p.res_bits >= 8 &&
                p.res_bits == ((rb > 8 ? rb : 8) < 23 - lb ? (rb > 8 ? rb : 8) : 23 - lb),
            "widths");
      CHECK(cell_word_cell(p, kPackSkip) == cell_skip(p), "skip under %u %u", lb, rb);
      CHECK(pack_join(0xFFFF, 0xFF) == kPackSkip && pack_hi(kPackSkip) == 0xFFFF && pack_lo(kPackSkip) == 0xFF,
            "the skip word's planes");
      CHECK(cell_escape(p) + 1 == cell_skip(p), "reserved");
      for (uint32_t code : {0u, 1u, 255u})
        for (bool err : {false, true}) {
          const uint32_t w = cell_word_pack(p, 0, err, cell_escape(p), code);
          CHECK(w != kPackSkip && cell_word_cell(p, w) == cell_escape(p) &&
                    pack_word_escape_code(p, w) == code && pack_word_error(p, w) == err,
                "escape word under %u %u", lb, rb);
        }
    }
  // -- key order equals duration order within a code ---------------------------
  {  // the SocialNetwork shape: 13 cell bits, exponents up to 11, pr = 10
    const uint32_t first = 17, last = (12u << 5) + 31, width = last - first + 1, base = 300;
    const CellFmt f = cell_fmt(35, 5654, 11);
    CHECK(pack_fmt_fits(f, 35) && pack_fmt(f).res_bits == 10, "SN-like layout");
    const CellFmt p = pack_fmt(f);
    uint32_t lo, hi, prev_key = 0, wides = 0;
    hist_bounds(first, &lo, &hi);
    const uint32_t d0 = lo;
    hist_bounds(last, &lo, &hi);
    bool have = false;
    for (uint32_t d = d0; d <= hi; ++d) {
      bool wide = false;
      const uint32_t w = pack_word_encode(p, 34, (d & 7u) == 0u, d, first, base, width, &wide);
      if (cell_word_cell(p, w) == cell_escape(p)) {
        CHECK(wide && hist_exp(hist_bin(d)) == 11, "d=%u escapes", d);
        ++wides;
        continue;
      }
      const uint32_t key = cell_word_ekey(p, w) & low_mask(cell_key_bits(p));
      if (have) CHECK(key > prev_key, "key order at d=%u", d);
      CHECK(cell_key_dur(p, key, first, base) == d, "round trip at d=%u", d);
      prev_key = key;
      have = true;
    }
    CHECK(wides == 32u << 11, "every duration of exponent 11 is wide: %u", wides);
  }
  // -- the column's planes -----------------------------------------------------
  for (uint64_t n : {0ull, 1ull, 7ull, 8ull, 9ull, 1000ull, (1ull << 33) + 5})
    CHECK(pack_lo_offset(n) % 16 == 0 && pack_lo_offset(n) >= 2 * n && pack_lo_offset(n) < 2 * n + 16 &&
              pack_column_bytes(n) == pack_lo_offset(n) + n,
          "planes of %llu positions", (unsigned long long)n);
  printf("ok %llu\n", g_checks);
  return 0;
}
