// gsr_span_word.h — the packed span word of a (view, Gaussian): the kept tile span [t0, t1) of every rectangle
// row (span_row, gsr_common.h) in one 64-bit word, written by the preprocess beside the record and gathered by the
// emission in the record's place (8 B of a 16-entry line instead of 48 B of a random 128-B line).
// Host + device, and plain C++ (no HIP types: tests compile this header with the host compiler alone).
//
//   bit  0         valid (a word of 0 = "not encodable": the emission evaluates the rows from the record)
//   bits [1, 8)    first rectangle row
//   bits [8, 10)   rectangle rows - 1 (1 .. 4 rows)
//   row i:  bits [10 + 11 i, +7) t0,  bits [17 + 11 i, +4) t1 - t0      (54 bits used)
//
// Encodable: 1 .. 4 rectangle rows, every row index and kept tile column < 128, every t0 < 128, every row at most
// 15 kept tiles.  A row with an empty span is encodable (length 0, its t0 kept as span_row returns it).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GSR_SPAN_HD __host__ __device__ __forceinline__
#else
#define GSR_SPAN_HD static inline
#endif

#define GSR_SPAN_ROWS 4     // rectangle rows a word holds
#define GSR_SPAN_LEN 15     // kept tiles of a row
#define GSR_SPAN_COORD 128  // tile rows and columns below this
#define GSR_SPAN_NONE 0ull  // "not encodable"

namespace gsr {

// Encoder, in the order the preprocess walks the rows: the head (first row, row count), then every row i.
// Either returns GSR_SPAN_NONE when the Gaussian does not fit, and span_word_put keeps a GSR_SPAN_NONE.
GSR_SPAN_HD uint64_t span_word_head(int row0, int rows) {
  if (rows < 1 || rows > GSR_SPAN_ROWS || row0 < 0 || row0 + rows > GSR_SPAN_COORD) return GSR_SPAN_NONE;
  return 1ull | (uint64_t)row0 << 1 | (uint64_t)(rows - 1) << 8;
}
GSR_SPAN_HD uint64_t span_word_put(uint64_t w, int i, int t0, int t1) {
  if (w == GSR_SPAN_NONE || i < 0 || i >= GSR_SPAN_ROWS) return GSR_SPAN_NONE;
  const int len = t1 - t0;
  if (t0 < 0 || t0 >= GSR_SPAN_COORD || len < 0 || len > GSR_SPAN_LEN || t1 > GSR_SPAN_COORD) return GSR_SPAN_NONE;
  return w | ((uint64_t)t0 | (uint64_t)len << 7) << (10 + 11 * i);
}

// Decoder (w != GSR_SPAN_NONE; row i < span_word_rows(w)).
GSR_SPAN_HD bool span_word_ok(uint64_t w) { return (w & 1ull) != 0ull; }
GSR_SPAN_HD int span_word_row0(uint64_t w) { return (int)(w >> 1) & 127; }
GSR_SPAN_HD int span_word_rows(uint64_t w) { return ((int)(w >> 8) & 3) + 1; }
GSR_SPAN_HD void span_word_row(uint64_t w, int i, int& t0, int& t1) {
  const uint32_t f = (uint32_t)(w >> (10 + 11 * i));
  t0 = (int)(f & 127u);
  t1 = t0 + (int)(f >> 7 & 15u);
}

}  // namespace gsr
