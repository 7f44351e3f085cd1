// Host check of the error cells of the dense edge stream (span_word.h,
// edge_dense_kernel<0, 3> in edge_agg.hip), built with
// -fsanitize=address,undefined by `make errcellcheck`.  Over random layouts and
// durations, for every word pack_word_encode returns with a cell of the
// layout, pack_word_entry equals an independent restatement, error *
// 2^cell_bits + cell, and lies below 2^cell_bits + cells; and over random span
// lists an exact host model of the kernel's span path and flush — two entries
// per cell, the error count read off the error entries, the sum from
// count * lo(bin) and the residuals, min and max from keys, escapes taken
// from the duration — reproduces count, errors, sum, min, max and histogram
// of a direct computation.  Prints "ok <checks>" and exits 0, or names the
// first failure and exits 1.
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

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
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
struct Stats {
  uint64_t count = 0, err = 0, sum = 0;
  uint32_t mn = 0xFFFFFFFFu, mx = 0;
  std::vector<uint64_t> hist = std::vector<uint64_t>(ANOMOD_HIST_BINS, 0);
};

constexpr uint32_t kEntries = 16384;               // the carve's entries
constexpr uint32_t kFlag = 1u << 23, kCount = kFlag - 1u, kCodeShift = 24;

// A layout of `codes` codes with ranges of at most `span` bins below exponent
// top_exp + 1; false when it does not pack or the carve has no room for it.
static bool make_layout(uint32_t codes, uint32_t top_exp, uint32_t span, std::vector<Code>* lay,
                        CellFmt* f, uint32_t* cells_out) {
  lay->clear();
  uint32_t cells = 0, max_exp = 0;
  for (uint32_t c = 0; c < codes; ++c) {
    const uint32_t last = top_exp == 0 ? below(64) : ((top_exp + 1) << 5) + below(32);
    const uint32_t width = 1 + below(span);
    const uint32_t first = last + 1 >= width ? last + 1 - width : 0;
    lay->push_back(Code{first, cells, last - first + 1});
    cells += last - first + 1;
    if (hist_exp(last) > max_exp) max_exp = hist_exp(last);
  }
  *f = cell_fmt(codes, cells, max_exp);
  *cells_out = cells;
  return pack_fmt_fits(*f, codes) && codes <= 64 && cells <= 8192 &&
         (1ull << f->cell_bits) + cells <= kEntries;
}

// A duration for code k: mostly inside its range, sometimes just outside it.
static uint32_t draw(const Code& k) {
  uint32_t lo, hi;
  const uint32_t pick = below(16);
  uint32_t bin = k.first + below(k.width);
  if (pick == 0 && k.first > 0) bin = k.first - 1;
  if (pick == 1 && k.first + k.width < ANOMOD_HIST_BINS) bin = k.first + k.width;
  hist_bounds(bin, &lo, &hi);
  const uint32_t at = below(4);
  return at == 0 ? lo : at == 1 ? hi : lo + below(hi - lo + 1);
}

int main() {
  unsigned layouts = 0, with_wide = 0;
  unsigned long long escapes = 0, flagged = 0, plain = 0;
  for (int it = 0; it < 3000; ++it) {
    const uint32_t codes = 1u + below(64), top_exp = below(14);
    std::vector<Code> lay;
    CellFmt f;
    uint32_t cells;
    if (!make_layout(codes, top_exp, it % 3 == 0 ? 120u : 10u, &lay, &f, &cells)) continue;
    ++layouts;
    const CellFmt p = pack_fmt(f);
    const uint32_t err_off = 1u << p.cell_bits, kb = cell_key_bits(p);
    CHECK(err_off + cells <= kEntries && cells <= cell_escape(p), "the carve holds %u cells twice", cells);
    if (p.res_bits < f.res_bits) ++with_wide;
    // the kernel's start: both entries of every cell hold the code and the flag
    std::vector<uint32_t> ent(kEntries, 0xDEADBEEFu);
    for (uint32_t c = 0; c < codes; ++c)
      for (uint32_t k = 0; k < lay[c].width; ++k)
        ent[lay[c].base + k] = ent[err_off + lay[c].base + k] = c << kCodeShift | kFlag;
    std::vector<uint32_t> kmin(codes, 0xFFFFFFFFu), kmax(codes, 0u);
    std::vector<uint64_t> lsum(codes, 0);
    std::vector<Stats> model(codes), direct(codes);  // model: what the kernel leaves in the tables
    const uint32_t n = 200 + below(3000), perr = below(4) == 0 ? 2u : 1u + below(300);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t c = below(codes), d = draw(lay[c]);
      const bool error = below(perr) == 0;
      Stats& r = direct[c];
      ++r.count, r.err += error, r.sum += d, ++r.hist[hist_bin(d)];
      if (d < r.mn) r.mn = d;
      if (d > r.mx) r.mx = d;
      bool wide = false;
      const uint32_t w = pack_word_encode(p, c, error, d, lay[c].first, lay[c].base, lay[c].width, &wide);
      const uint32_t cell = cell_word_cell(p, w);
      Stats& m = model[c];
      if (cell >= cells) {  // an escape word: the kernel's `direct`
        CHECK(cell == cell_escape(p) && pack_word_escape_code(p, w) == c && pack_word_error(p, w) == error,
              "escape word of d=%u", d);
        ++escapes;
        const uint32_t bin = hist_bin(d), k = bin - lay[c].first;
        uint32_t part = d;
        if (k < lay[c].width) {
          CHECK(wide, "in range and escaping: wide (d=%u)", d);
          ++ent[lay[c].base + k];  // the plain entry; the flag stays
          part = d - hist_lo(bin);
        } else {
          ++m.hist[bin];
        }
        m.sum += part, m.err += error;
        if (d < m.mn) m.mn = d;
        if (d > m.mx) m.mx = d;
        continue;
      }
      // -- the entry index against its restatement ---------------------------
      const uint32_t entry = pack_word_entry(p, w);
      const uint32_t want = (error ? 1u : 0u) * (1u << p.cell_bits) + cell;
      CHECK(entry == want, "entry %u of word %06x, want %u", entry, w, want);
      CHECK(entry < err_off + cells && entry < kEntries, "entry %u below %u + %u", entry, err_off, cells);
      CHECK(cell == lay[c].base + hist_bin(d) - lay[c].first, "cell of d=%u", d);
      // -- the span path -------------------------------------------------------
      const uint32_t old = ent[entry]++;
      CHECK(old >> kCodeShift == c, "the entry names code %u, not %u", old >> kCodeShift, c);
      CHECK((old & kCount) < kCount, "count bound");
      lsum[c] += cell_word_residual(p, w);
      if (old & kFlag) {
        ++flagged;
        const uint32_t key = w & low_mask(kb);
        if (key < kmin[c]) kmin[c] = key;
        if (key > kmax[c]) kmax[c] = key;
        if (cell > (kmin[c] >> p.res_bits) && cell < (kmax[c] >> p.res_bits)) {
          ent[cell] &= ~kFlag;  // no later span of this cell is an extreme, with the error bit or without
          ent[err_off + cell] &= ~kFlag;
        }
      } else {
        ++plain;
        const uint32_t key = w & low_mask(kb);
        CHECK(key > kmin[c] && key < kmax[c], "a span past a cleared flag is no extreme (d=%u)", d);
      }
    }
    // -- the flush: two entries per cell ---------------------------------------
    for (uint32_t c = 0; c < codes; ++c) {
      Stats& m = model[c];
      for (uint32_t k = 0; k < lay[c].width; ++k) {
        const uint32_t n0 = ent[lay[c].base + k] & kCount, n1 = ent[err_off + lay[c].base + k] & kCount;
        CHECK(ent[lay[c].base + k] >> kCodeShift == c && ent[err_off + lay[c].base + k] >> kCodeShift == c,
              "the code byte survives the counts");
        m.hist[lay[c].first + k] += (uint64_t)n0 + n1;
        m.sum += ((uint64_t)n0 + n1) * hist_lo(lay[c].first + k);
        m.err += n1;
      }
      if (kmin[c] != 0xFFFFFFFFu) {
        m.sum += lsum[c];
        const uint32_t a = cell_key_dur(p, kmin[c], lay[c].first, lay[c].base);
        const uint32_t b = cell_key_dur(p, kmax[c], lay[c].first, lay[c].base);
        if (a < m.mn) m.mn = a;
        if (b > m.mx) m.mx = b;
      } else {
        CHECK(lsum[c] == 0, "residuals without a first span");
      }
      const Stats& r = direct[c];
      for (uint32_t b = 0; b < ANOMOD_HIST_BINS; ++b) {
        CHECK(m.hist[b] == r.hist[b], "hist[%u][%u]: %llu, want %llu", c, b, (unsigned long long)m.hist[b],
              (unsigned long long)r.hist[b]);
        m.count += m.hist[b];
      }
      CHECK(m.count == r.count, "count[%u]: %llu, want %llu", c, (unsigned long long)m.count,
            (unsigned long long)r.count);
      CHECK(m.err == r.err, "errors[%u]: %llu, want %llu", c, (unsigned long long)m.err,
            (unsigned long long)r.err);
      CHECK(m.sum == r.sum, "sum[%u]: %llu, want %llu", c, (unsigned long long)m.sum,
            (unsigned long long)r.sum);
      CHECK(m.mn == r.mn && m.mx == r.mx, "min/max[%u]: %u %u, want %u %u", c, m.mn, m.mx, r.mn, r.mx);
    }
    // entries no cell owns were never touched
    for (uint32_t k = cells; k < err_off; ++k) CHECK(ent[k] == 0xDEADBEEFu, "entry %u", k);
    for (uint32_t k = err_off + cells; k < kEntries; ++k) CHECK(ent[k] == 0xDEADBEEFu, "entry %u", k);
  }
  CHECK(layouts > 500 && with_wide > 20, "coverage: %u layouts, %u with wide bins", layouts, with_wide);
  CHECK(escapes > 10000 && flagged > 10000 && plain > 10000, "coverage: %llu escapes, %llu flagged, %llu plain",
        escapes, flagged, plain);
  // -- the borders of the rule: 13 cell bits and 8190 cells fill the carve ------
  {
    const CellFmt f = cell_fmt(64, 8190, 8);
    CHECK(f.cell_bits == 13 && (1u << f.cell_bits) + 8190 == kEntries - 2, "8190 cells: 16382 entries");
    CHECK(cell_fmt(64, 8191, 8).cell_bits == 14 && (1u << 14) + 8191 > kEntries, "8191 cells: 14 cell bits");
    const CellFmt p = pack_fmt(f);
    bool wide = false;
    const uint32_t w = pack_word_encode(p, 63, true, 5, 5, 8189, 1, &wide);
    CHECK(pack_word_entry(p, w) == 8192 + 8189 && !wide, "the last error entry");
    const CellFmt q = pack_fmt(cell_fmt(3, 30, 4));  // 5 cell bits
    CHECK(q.cell_bits == 5, "5 cell bits");
    const uint32_t v = pack_word_encode(q, 2, true, 70, 60, 20, 10, &wide);
    CHECK(pack_word_entry(q, v) == (1u << 5 | (20 + hist_bin(70) - 60)), "error << 5 | cell");
  }
  printf("ok %llu\n", g_checks);
  return 0;
}
