// hnsw_rows_plan.h -- the index's lossy row copies (half rows, sq8 codes, per-dimension sq8 codes, 1-bit codes): what each one is to
// the host, what its option accepts and refuses, and which rows the knn searches read.  Plain decisions over plain numbers, so that
// a host program can check them against the code they replaced (tests/cpp/test_rows_plan.cpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hnsw_mi355x.h"

namespace hnsw_host {

// Which lossy copy an option turned on (hnsw_index::lossy_on): one value, so at most one is on.  The byte rows and the split rows
// are not among them: they are exact, made without being asked for, and have rules of their own.
enum LossyRows : int { LOSSY_NONE = 0, LOSSY_HALF, LOSSY_SQ8, LOSSY_SQ8_DIM, LOSSY_BITS, LOSSY_KINDS };

struct LossyRowsDesc {
    const char *option;            // the option that turns the copy on
    int rows;                      // HNSW_ROWS_*: hnsw_index_info.row_format while the searches read it
    // null: the option takes any integer (> 0 on; 0 off, the copy kept; < 0 off, the copy freed); else it takes lo..hi only, and
    // this is what the refusal says of them
    const char *values;
    int64_t lo, hi;
    bool value_is_mode;            // a value > 0 is the copy's parameter (bit_mode): another one makes the copy again, and 0 always frees it
    const char *byte_rows;         // what the refusal while the byte rows are read says of them
    const char *set_other;         // how the refusal while another copy is on names that option the second time; null: by its name
    bool codes;                    // the walk's distances are those of a code space (walks_codes): queries transformed, always re-ranked
    int value_bits;                // bits a stored value takes: hnsw_index_row_bytes is ceil(d * value_bits / 8)
    int knn_rows_l2, knn_rows;     // the knn kernel's ROWS under L2 and under the other metrics (variant_full)
};
// [LossyRows]; LOSSY_NONE stands for the exact rows as far as they share a value (float32 and split rows; the byte rows: one byte)
constexpr LossyRowsDesc k_lossy_rows[LOSSY_KINDS] = {
    {nullptr, HNSW_ROWS_F32, nullptr, 0, 0, false, nullptr, nullptr, false, 32, -1, -1},
    {"half_rows", HNSW_ROWS_HALF, nullptr, 0, 0, false, "which are exact and half the size of half rows", "it", false, 16, 4, 4},
    // (the kernel reads the sq8 codes as it reads byte rows; the per-dimension codes under L2 are a weighted distance, a kernel
    // family of its own, and byte rows under the inner product)
    {"sq8_rows", HNSW_ROWS_SQ8, nullptr, 0, 0, false, "which are exact and the same size", nullptr, true, 8, 2, 2},
    {"sq8_dim_rows", HNSW_ROWS_SQ8_DIM, "1 (on), 0 (off) or -1 (off, the copy freed)", -1, 1, false, "which are exact and the same size", nullptr,
     true, 8, 5, 2},
    {"bit_rows", HNSW_ROWS_BITS, "0 (off), 1 (thresholds at the column means) or 2 (at zero)", 0, 2, true, "which are exact", nullptr, true, 1, 6, 6},
};

// the copy an option name turns on, the copy a row format is; LOSSY_NONE: not one of them
inline LossyRows lossy_rows_by_option(const char *name) {
    for (int k = LOSSY_HALF; k < LOSSY_KINDS; ++k) if (!strcmp(name, k_lossy_rows[k].option)) return (LossyRows)k;
    return LOSSY_NONE;
}
inline LossyRows lossy_rows_of_format(int row_format) {
    for (int k = LOSSY_HALF; k < LOSSY_KINDS; ++k) if (k_lossy_rows[k].rows == row_format) return (LossyRows)k;
    return LOSSY_NONE;
}

// The rows the knn searches read, in this order of precedence: the byte rows (exact, the smallest) unless option byte_rows is 0,
// the lossy copy that is on (once it exists: an index emptied by hnsw_index_remove has none until it grows again), the split rows
// unless option split_rows is 0 or less, the plain float32 rows.
inline int bound_rows(bool byte_rows_off, bool has_byte_rows, LossyRows on, bool on_exists, bool split_rows_off, bool has_split_rows) {
    if (!byte_rows_off && has_byte_rows) return HNSW_ROWS_BYTES;
    if (on != LOSSY_NONE && on_exists) return k_lossy_rows[on].rows;
    return !split_rows_off && has_split_rows ? HNSW_ROWS_SPLIT : HNSW_ROWS_F32;
}

// What hnsw_index_set_option does with one of the four options: a refusal (code, message; nothing changes), or the steps to take
// and the switch afterwards.  The view is bound again and the shapes forgotten either way.
struct RowsOptionPlan {
    int code = HNSW_OK;
    char message[192] = "";
    bool make = false;             // make the copy first (the bit rows: under mode `value`, in place of a copy of the other mode) ...
    bool release = false;          // ... or release its tables and parameters, once the launches that read them are over
    LossyRows on = LOSSY_NONE;     // hnsw_index::lossy_on and ::bit_mode afterwards
    int bit_mode = 0;
};
// row_format: what the searches read now; exists: does the option's own copy; a copy is turned on only over exact rows that are not
// the byte rows (which are exact and no larger: "byte_rows" 0 first), with no other copy on, and not under option filter_collect
inline RowsOptionPlan plan_rows_option(LossyRows option, int64_t value, int row_format, LossyRows on, bool exists, int bit_mode, bool filter_collect) {
    const LossyRowsDesc &d = k_lossy_rows[option];
    RowsOptionPlan p;
    p.on = on; p.bit_mode = bit_mode;
    auto refuse = [&p](const char *fmt, auto... args) { p.code = HNSW_ERR_BAD_ARG; snprintf(p.message, sizeof p.message, fmt, args...); return p; };
    if (d.values && (value < d.lo || value > d.hi)) return refuse("%s=%lld: %s", d.option, (long long)value, d.values);
    if (value > 0) {
        if (row_format == HNSW_ROWS_BYTES) return refuse("%s: the index searches its byte rows, %s (set byte_rows 0 first)", d.option, d.byte_rows);
        if (on != LOSSY_NONE && on != option)
            return refuse("%s: option %s is on (set %s 0 first)", d.option, k_lossy_rows[on].option, d.set_other ? d.set_other : k_lossy_rows[on].option);
        if (filter_collect) return refuse("%s: option filter_collect is on, which needs exact rows (set filter_collect 0 first)", d.option);
        p.make = !exists || (d.value_is_mode && bit_mode != (int)value);   // (a refusal -- NaN, infinity, a range -- leaves the index as it was)
        p.on = option;
        if (d.value_is_mode) p.bit_mode = (int)value;
    } else {
        p.release = exists && (value < 0 || d.value_is_mode);
        if (on == option) p.on = LOSSY_NONE;
        if (d.value_is_mode) p.bit_mode = 0;
    }
    return p;
}

} // namespace hnsw_host
