// hnsw_bits_plan.h -- the word counts of the bit rows (hnsw_rows_bits.hip) and of the query rows their walks read.  Plain arithmetic
// on plain numbers, so that a host program can check it (tests/cpp/test_bits_plan.cpp).
#pragma once
#include <cstdint>

namespace hnsw_host {

// floats of a float32 row: rows are multiples of 64 B
inline int64_t padded_stride(int d) { return ((int64_t)d + 15) / 16 * 16; }
// NW: 16-word steps of a bit row (d <= 512: 64 bytes a row, else 128) -- the knn kernel's NCH for that format
inline int bit_words(int d) { return d > 512 ? 2 : 1; }
// words of a query row of option "bit_query_bits" 4: four bit planes, each packed as a row's bits are (16 * NW words a plane)
inline int64_t bit_plane_words(int d) { return 64 * (int64_t)bit_words(d); }
// Words (floats) per row of the matrix a walk over codes reads its queries from -- what its allocation, the query transform and
// SearchArgs.q_stride share.  The sq8 codes read float queries and the Hamming walk the first 16 * NW words of such a row: the
// padded stride.  The planes of a 4-bit query are 64 * NW words, which is MORE than the padded stride of a narrow row (d = 20: 64
// against 32), so they get a stride of their own.
inline int64_t walk_query_words(int d, bool planes) { return planes ? bit_plane_words(d) : padded_stride(d); }

} // namespace hnsw_host
