// Stand-alone round-trip check of the packed span word (csrc/gsr_span_word.h), host compiler only.
// tests/test_span_word.py builds and runs it; exit status 0 and a line "ok <cases> <encodable>" = pass.
#include <stdio.h>
#include <stdlib.h>

#include "gsr_span_word.h"

struct Case {
  int row0, rows;
  int t0[5], t1[5];
};

static long n_cases = 0, n_enc = 0;

// The rule, stated apart from the encoder: 1..4 rows, every row index, t0 and kept tile column below 128, at most
// 15 kept tiles per row.
static bool fits(const Case& c) {
  if (c.rows < 1 || c.rows > 4 || c.row0 < 0 || c.row0 + c.rows - 1 >= 128) return false;
  for (int i = 0; i < c.rows; ++i) {
    const int len = c.t1[i] - c.t0[i];
    if (c.t0[i] < 0 || c.t0[i] >= 128 || len < 0 || len > 15) return false;
    if (len > 0 && c.t1[i] - 1 >= 128) return false;
  }
  return true;
}

static void check(const Case& c) {
  uint64_t w = gsr::span_word_head(c.row0, c.rows);
  for (int i = 0; i < c.rows; ++i) w = gsr::span_word_put(w, i, c.t0[i], c.t1[i]);
  ++n_cases;
  bool bad = false;
  if (!fits(c)) {
    bad = w != GSR_SPAN_NONE || gsr::span_word_ok(w);
  } else {
    ++n_enc;
    bad = w == GSR_SPAN_NONE || !gsr::span_word_ok(w) || gsr::span_word_row0(w) != c.row0 ||
          gsr::span_word_rows(w) != c.rows;
    int kept = 0, want = 0;
    for (int i = 0; !bad && i < c.rows; ++i) {
      int t0 = -1, t1 = -1;
      gsr::span_word_row(w, i, t0, t1);
      bad = t0 != c.t0[i] || t1 != c.t1[i];
      kept += t1 - t0;
      want += c.t1[i] - c.t0[i];
    }
    bad = bad || kept != want;
  }
  if (bad) {
    printf("FAIL row0 %d rows %d word %016llx fits %d:", c.row0, c.rows, (unsigned long long)w, (int)fits(c));
    for (int i = 0; i < c.rows; ++i) printf(" [%d,%d)", c.t0[i], c.t1[i]);
    printf("\n");
    exit(1);
  }
}

int main() {
  const int coords[] = {0, 1, 63, 112, 113, 126, 127, 128};
  const int nc = (int)(sizeof(coords) / sizeof(coords[0]));
  // every (t0, length 0..16) of row i against every (t0, length) of row j, the other rows at a base span, for
  // 1..5 rows and every first row of the list (which holds 0, 126, 127, 128)
  const int base[][2] = {{0, 0}, {5, 3}, {113, 15}, {127, 0}};
  for (int rows = 1; rows <= 5; ++rows)
    for (int r0 = 0; r0 < nc; ++r0)
      for (int b = 0; b < 4; ++b)
        for (int i = 0; i < rows; ++i)
          for (int j = i; j < rows; ++j)
            for (int ti = 0; ti < nc; ++ti)
              for (int li = 0; li <= 16; ++li)
                for (int tj = 0; tj < (j == i ? 1 : nc); ++tj)
                  for (int lj = 0; lj <= (j == i ? 0 : 16); ++lj) {
                    Case c;
                    c.row0 = coords[r0], c.rows = rows;
                    for (int k = 0; k < rows; ++k) c.t0[k] = base[b][0], c.t1[k] = base[b][0] + base[b][1];
                    c.t0[i] = coords[ti], c.t1[i] = coords[ti] + li;
                    if (j != i) c.t0[j] = coords[tj], c.t1[j] = coords[tj] + lj;
                    check(c);
                  }
  // every row empty: encodable, kept count 0 (checked by check(): the decoded lengths sum to 0)
  for (int rows = 1; rows <= 4; ++rows) {
    Case c;
    c.row0 = 3, c.rows = rows;
    for (int k = 0; k < rows; ++k) c.t0[k] = c.t1[k] = 9;
    if (!fits(c)) return 2;
    check(c);
    uint64_t w = gsr::span_word_head(c.row0, rows);
    for (int k = 0; k < rows; ++k) w = gsr::span_word_put(w, k, 9, 9);
    int kept = 0;
    for (int k = 0; k < rows; ++k) {
      int t0, t1;
      gsr::span_word_row(w, k, t0, t1);
      kept += t1 - t0;
    }
    if (!gsr::span_word_ok(w) || kept != 0) return 3;
  }
  // out-of-range arguments of the encoder itself, and a "not encodable" word stays one
  if (gsr::span_word_head(0, 0) != GSR_SPAN_NONE || gsr::span_word_head(-1, 1) != GSR_SPAN_NONE ||
      gsr::span_word_head(125, 4) != GSR_SPAN_NONE || gsr::span_word_head(124, 4) == GSR_SPAN_NONE ||
      gsr::span_word_put(GSR_SPAN_NONE, 0, 1, 2) != GSR_SPAN_NONE ||
      gsr::span_word_put(gsr::span_word_head(0, 4), 4, 1, 2) != GSR_SPAN_NONE ||
      gsr::span_word_put(gsr::span_word_head(0, 1), 0, 5, 4) != GSR_SPAN_NONE ||
      gsr::span_word_put(gsr::span_word_head(0, 1), 0, -1, 4) != GSR_SPAN_NONE)
    return 4;
  // seeded random rows over the whole ranges
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](int n) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((s >> 33) % (unsigned long long)n);
  };
  for (int it = 0; it < 400000; ++it) {
    Case c;
    c.rows = 1 + rnd(5);
    c.row0 = rnd(8) ? rnd(126) : 120 + rnd(10);
    for (int k = 0; k < c.rows; ++k) {
      c.t0[k] = rnd(8) ? rnd(114) : 110 + rnd(20);
      c.t1[k] = c.t0[k] + (rnd(16) ? rnd(16) : rnd(18));
    }
    check(c);
  }
  printf("ok %ld %ld\n", n_cases, n_enc);
  return n_enc > 0 && n_enc < n_cases ? 0 : 5;
}
