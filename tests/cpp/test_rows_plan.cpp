// hnsw_rows_plan.h against the code it replaced: bind_view's chain of negations, the four ladders of hnsw_index_set_option (their
// messages character for character), variant_full's switch and hnsw_index_row_bytes' expression, each restated here as it stood
// when every lossy copy had a switch of its own.  Host code only: build with -fsanitize=address,undefined and run
// (tests/test_half_rows_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_rows_plan.h"

#include <cstdarg>
#include <cstdio>
#include <string>

using namespace hnsw_host;

namespace {

// ---- the state as it was kept: three booleans and bit_mode, a table pointer per copy ---------------------------------------------
struct Old {
    bool byte_rows_off = false, split_rows_off = false, half_rows_on = false, sq8_on = false, sq8d_on = false, filter_collect = false;
    int bit_mode = 0, row_format = HNSW_ROWS_F32;
    bool X8 = false, Xh = false, Xq = false, Xqd = false, Xb = false, Xm = false;     // does the table exist
    // what a call did besides the switches
    bool made = false, released = false;
    std::string error;
};
int fail(Old &o, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    o.error = buf;
    return code;
}
bool codes_on(const Old &o) { return o.sq8_on || o.sq8d_on || o.bit_mode != 0; }
const char *codes_option(const Old &o) {
    if (o.bit_mode != 0 || o.row_format == HNSW_ROWS_BITS) return "bit_rows";
    return o.sq8d_on || o.row_format == HNSW_ROWS_SQ8_DIM ? "sq8_dim_rows" : "sq8_rows";
}

// bind_view: which rows it bound, and what of the view followed from them
struct OldView { int row_format; char x8; bool Xm, writes_Xh, writes_sq8s; int stride8_unit; bool stride8_bit_words; };
OldView old_bind_view(const Old &idx) {
    const bool bytes = !idx.byte_rows_off && idx.X8, sq8 = !bytes && idx.sq8_on && idx.Xq, sq8d = !bytes && !sq8 && idx.sq8d_on && idx.Xqd,
               bits = !bytes && !sq8 && !sq8d && idx.bit_mode != 0 && idx.Xb, half = !bytes && !sq8 && !sq8d && !bits && idx.half_rows_on && idx.Xh;
    OldView v{};
    v.x8 = bytes ? '8' : sq8 ? 'q' : sq8d ? 'd' : bits ? 'b' : 0;
    v.writes_Xh = half;
    v.stride8_bit_words = bits; v.stride8_unit = bits ? 64 : (half ? 128 : 64);
    v.Xm = idx.split_rows_off || half || sq8 || sq8d || bits ? false : idx.Xm;
    v.writes_sq8s = sq8d;
    v.row_format = bytes ? HNSW_ROWS_BYTES : sq8 ? HNSW_ROWS_SQ8 : sq8d ? HNSW_ROWS_SQ8_DIM : bits ? HNSW_ROWS_BITS : half ? HNSW_ROWS_HALF : v.Xm ? HNSW_ROWS_SPLIT : HNSW_ROWS_F32;
    return v;
}

// hnsw_index_set_option's four branches (make_*_rows: the table exists afterwards; release: it does not)
int old_set_option(Old *idx, const std::string &name, int64_t value) {
    if (name == "half_rows") {
        if (value > 0) {
            if (idx->row_format == HNSW_ROWS_BYTES)
                return fail(*idx, HNSW_ERR_BAD_ARG, "half_rows: the index searches its byte rows, which are exact and half the size of half rows "
                                                    "(set byte_rows 0 first)");
            if (codes_on(*idx)) return fail(*idx, HNSW_ERR_BAD_ARG, "half_rows: option %s is on (set it 0 first)", codes_option(*idx));
            if (idx->filter_collect) return fail(*idx, HNSW_ERR_BAD_ARG, "half_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->Xh) { idx->made = true; idx->Xh = true; }
            idx->half_rows_on = true;
        } else {
            if (value < 0 && idx->Xh) { idx->released = true; idx->Xh = false; }
            idx->half_rows_on = false;
        }
        return HNSW_OK;
    }
    if (name == "sq8_rows") {
        if (value > 0) {
            if (idx->row_format == HNSW_ROWS_BYTES)
                return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_rows: the index searches its byte rows, which are exact and the same size (set byte_rows 0 first)");
            if (idx->half_rows_on) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_rows: option half_rows is on (set half_rows 0 first)");
            if (idx->sq8d_on) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_rows: option sq8_dim_rows is on (set sq8_dim_rows 0 first)");
            if (idx->bit_mode) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_rows: option bit_rows is on (set bit_rows 0 first)");
            if (idx->filter_collect) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->Xq) { idx->made = true; idx->Xq = true; }
            idx->sq8_on = true;
        } else {
            if (value < 0 && idx->Xq) { idx->released = true; idx->Xq = false; }
            idx->sq8_on = false;
        }
        return HNSW_OK;
    }
    if (name == "sq8_dim_rows") {
        if (value < -1 || value > 1) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_dim_rows=%lld: 1 (on), 0 (off) or -1 (off, the copy freed)", (long long)value);
        if (value > 0) {
            if (idx->row_format == HNSW_ROWS_BYTES)
                return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_dim_rows: the index searches its byte rows, which are exact and the same size (set byte_rows 0 first)");
            if (idx->half_rows_on) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_dim_rows: option half_rows is on (set half_rows 0 first)");
            if (idx->sq8_on) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_dim_rows: option sq8_rows is on (set sq8_rows 0 first)");
            if (idx->bit_mode) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_dim_rows: option bit_rows is on (set bit_rows 0 first)");
            if (idx->filter_collect) return fail(*idx, HNSW_ERR_BAD_ARG, "sq8_dim_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->Xqd) { idx->made = true; idx->Xqd = true; }
            idx->sq8d_on = true;
        } else {
            if (value < 0 && idx->Xqd) { idx->released = true; idx->Xqd = false; }
            idx->sq8d_on = false;
        }
        return HNSW_OK;
    }
    if (name == "bit_rows") {
        if (value < 0 || value > 2) return fail(*idx, HNSW_ERR_BAD_ARG, "bit_rows=%lld: 0 (off), 1 (thresholds at the column means) or 2 (at zero)", (long long)value);
        if (value > 0) {
            if (idx->row_format == HNSW_ROWS_BYTES)
                return fail(*idx, HNSW_ERR_BAD_ARG, "bit_rows: the index searches its byte rows, which are exact (set byte_rows 0 first)");
            if (idx->half_rows_on) return fail(*idx, HNSW_ERR_BAD_ARG, "bit_rows: option half_rows is on (set half_rows 0 first)");
            if (idx->sq8_on) return fail(*idx, HNSW_ERR_BAD_ARG, "bit_rows: option sq8_rows is on (set sq8_rows 0 first)");
            if (idx->sq8d_on) return fail(*idx, HNSW_ERR_BAD_ARG, "bit_rows: option sq8_dim_rows is on (set sq8_dim_rows 0 first)");
            if (idx->filter_collect) return fail(*idx, HNSW_ERR_BAD_ARG, "bit_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->Xb || idx->bit_mode != (int)value) { idx->made = true; idx->Xb = true; }
            idx->bit_mode = (int)value;
        } else {
            if (idx->Xb) { idx->released = true; idx->Xb = false; }
            idx->bit_mode = 0;
        }
        return HNSW_OK;
    }
    return -100;
}

// variant_full's cases of the four formats, and hnsw_index_row_bytes
int old_variant_full(int row_format, int metric) {
    switch (row_format) {
    case HNSW_ROWS_BYTES: case HNSW_ROWS_SQ8: return 2;
    case HNSW_ROWS_SQ8_DIM: return metric == HNSW_METRIC_L2 ? 5 : 2;
    case HNSW_ROWS_BITS: return 6;
    case HNSW_ROWS_SPLIT: return 3;
    case HNSW_ROWS_HALF: return 4;
    default: return -1;
    }
}
bool old_walks_codes(int f) { return f == HNSW_ROWS_SQ8 || f == HNSW_ROWS_SQ8_DIM || f == HNSW_ROWS_BITS; }
int64_t old_row_bytes(int f, int d) {
    if (f == HNSW_ROWS_BITS) return ((int64_t)d + 7) / 8;
    return (int64_t)d * (f == HNSW_ROWS_BYTES || old_walks_codes(f) ? 1 : f == HNSW_ROWS_HALF ? 2 : 4);
}
// ... and as the library computes them from the table now
int64_t new_row_bytes(int f, int d) {
    const int bits = f == HNSW_ROWS_BYTES ? 8 : k_lossy_rows[lossy_rows_of_format(f)].value_bits;
    return ((int64_t)d * bits + 7) / 8;
}

// the switch as the old fields
void set_switch(Old &o, LossyRows on, int bit_mode) {
    o.half_rows_on = on == LOSSY_HALF; o.sq8_on = on == LOSSY_SQ8; o.sq8d_on = on == LOSSY_SQ8_DIM; o.bit_mode = bit_mode;
}
// ... and back: LOSSY_KINDS if more than one is on
LossyRows get_switch(const Old &o) {
    const int count = (o.half_rows_on ? 1 : 0) + (o.sq8_on ? 1 : 0) + (o.sq8d_on ? 1 : 0) + (o.bit_mode != 0 ? 1 : 0);
    if (count > 1) return LOSSY_KINDS;
    return o.half_rows_on ? LOSSY_HALF : o.sq8_on ? LOSSY_SQ8 : o.sq8d_on ? LOSSY_SQ8_DIM : o.bit_mode ? LOSSY_BITS : LOSSY_NONE;
}
void set_tables(Old &o, unsigned exist) {
    o.Xh = (exist >> LOSSY_HALF) & 1u; o.Xq = (exist >> LOSSY_SQ8) & 1u; o.Xqd = (exist >> LOSSY_SQ8_DIM) & 1u; o.Xb = (exist >> LOSSY_BITS) & 1u;
}

} // namespace

int main() {
    long cases = 0, differ = 0;
    auto expect = [&](bool ok, const char *what) { ++cases; if (!ok) { if (++differ <= 20) std::printf("DIFFERS: %s\n", what); } };

    // ---- the table itself -----------------------------------------------------------------------------------------------------------
    const int formats[] = {HNSW_ROWS_F32, HNSW_ROWS_BYTES, HNSW_ROWS_SPLIT, HNSW_ROWS_HALF, HNSW_ROWS_SQ8, HNSW_ROWS_SQ8_DIM, HNSW_ROWS_BITS};
    for (int f : formats) {
        const LossyRows k = lossy_rows_of_format(f);
        const bool lossy = f == HNSW_ROWS_HALF || f == HNSW_ROWS_SQ8 || f == HNSW_ROWS_SQ8_DIM || f == HNSW_ROWS_BITS;
        expect((k != LOSSY_NONE) == lossy && (!lossy || k_lossy_rows[k].rows == f), "a format's copy");
        expect(k_lossy_rows[k].codes == old_walks_codes(f), "walks_codes");
        if (lossy)
            for (int metric : {HNSW_METRIC_L2, HNSW_METRIC_IP, HNSW_METRIC_COSINE})
                expect((metric == HNSW_METRIC_L2 ? k_lossy_rows[k].knn_rows_l2 : k_lossy_rows[k].knn_rows) == old_variant_full(f, metric), "the kernel's ROWS");
        for (int d = 1; d <= 1030; ++d) expect(new_row_bytes(f, d) == old_row_bytes(f, d), "row bytes");
    }
    for (int k = LOSSY_HALF; k < LOSSY_KINDS; ++k)
        expect(lossy_rows_by_option(k_lossy_rows[k].option) == k, "an option's copy");
    expect(lossy_rows_by_option("byte_rows") == LOSSY_NONE && lossy_rows_by_option("") == LOSSY_NONE, "other options");

    // ---- precedence: every state of the six inputs, the five values of the switch ---------------------------------------------------
    for (int on = LOSSY_NONE; on < LOSSY_KINDS; ++on)
        for (int mode = 1; mode <= 2; ++mode)
            for (unsigned exist = 0; exist < (1u << LOSSY_KINDS); exist += 2)          // (bit 0, LOSSY_NONE, stays clear)
                for (int rest = 0; rest < 16; ++rest) {
                    Old o;
                    o.byte_rows_off = rest & 1; o.X8 = rest & 2; o.split_rows_off = rest & 4; o.Xm = rest & 8;
                    set_switch(o, (LossyRows)on, on == LOSSY_BITS ? mode : 0);
                    set_tables(o, exist);
                    const OldView v = old_bind_view(o);
                    const int f = bound_rows(o.byte_rows_off, o.X8, (LossyRows)on, (exist >> on) & 1u, o.split_rows_off, o.Xm);
                    expect(f == v.row_format, "the bound rows");
                    // what bind_view derives from the bound format now, against what the chain gave
                    const LossyRows bound = lossy_rows_of_format(f);
                    expect(v.Xm == (!o.split_rows_off && bound == LOSSY_NONE && o.Xm), "Xm in the view");
                    expect(v.x8 == (f == HNSW_ROWS_BYTES ? '8' : f == HNSW_ROWS_SQ8 ? 'q' : f == HNSW_ROWS_SQ8_DIM ? 'd' : f == HNSW_ROWS_BITS ? 'b' : 0), "X8 in the view");
                    expect(v.writes_Xh == (f == HNSW_ROWS_HALF) && v.writes_sq8s == (f == HNSW_ROWS_SQ8_DIM), "Xh and sq8s are written with their copy only");
                    expect(v.stride8_bit_words == (f == HNSW_ROWS_BITS) && v.stride8_unit == (f == HNSW_ROWS_HALF ? 128 : 64), "stride8");
                }

    // ---- the option plan: every option, every value in -2..3, every reachable state ---------------------------------------------------
    // reachable: at most one copy on (the bit rows are on exactly while bit_mode is 1 or 2), filter_collect not on together with a
    // copy, the byte rows read only where option byte_rows is not 0
    for (int option = LOSSY_HALF; option < LOSSY_KINDS; ++option)
        for (int64_t value = -2; value <= 3; ++value)
            for (int bytes = 0; bytes < 2; ++bytes)
                for (int on = LOSSY_NONE; on < LOSSY_KINDS; ++on)
                    for (int bit_mode = 0; bit_mode <= 2; ++bit_mode)
                        for (unsigned exist = 0; exist < (1u << LOSSY_KINDS); exist += 2)
                            for (int collect = 0; collect < 2; ++collect) {
                                if ((on == LOSSY_BITS) != (bit_mode != 0)) continue;
                                if (collect && on != LOSSY_NONE) continue;
                                Old o;
                                o.byte_rows_off = !bytes; o.X8 = bytes; o.filter_collect = collect;
                                set_switch(o, (LossyRows)on, bit_mode);
                                set_tables(o, exist);
                                o.row_format = old_bind_view(o).row_format;
                                const Old before = o;
                                const int code = old_set_option(&o, k_lossy_rows[option].option, value);
                                const RowsOptionPlan p = plan_rows_option((LossyRows)option, value, before.row_format, (LossyRows)on, (exist >> option) & 1u, bit_mode, collect);
                                expect(p.code == code, "the code");
                                expect(o.error == p.message, "the message");
                                if (code != HNSW_OK) {
                                    expect(!o.made && !o.released && get_switch(o) == on && o.bit_mode == bit_mode, "a refusal changes nothing");
                                    continue;
                                }
                                expect(p.make == o.made && p.release == o.released && !(p.make && p.release), "make / release");
                                expect(p.on == get_switch(o) && p.bit_mode == o.bit_mode, "the switch afterwards");
                                // the tables afterwards: made ones exist, released ones do not, the others are untouched
                                unsigned after = exist;
                                if (p.make) after |= 1u << option;
                                if (p.release) after &= ~(1u << option);
                                Old t;
                                set_tables(t, after);
                                expect(t.Xh == o.Xh && t.Xq == o.Xq && t.Xqd == o.Xqd && t.Xb == o.Xb, "the tables afterwards");
                            }
    std::printf("rows plan %s: %ld cases, %ld differ\n", differ ? "FAILED" : "ok", cases, differ);
    return differ ? 1 : 0;
}
