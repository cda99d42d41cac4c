// hnsw_scan_bytes_plan.h (option "scan_bytes"): when a scan may take the matrix kernels, and the scratch of a piece's query codes and
// terms.  Host arithmetic only: build with -fsanitize=address,undefined and run (tests/test_scan_bytes_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_scan_bytes_plan.h"

#include <cstdio>
#include <initializer_list>

int main() {
    using namespace hnsw_host;
    int bad = 0, cases = 0;
    auto expect = [&](bool ok, const char *what) { ++cases; if (!ok) { ++bad; std::printf("FAILED: %s\n", what); } };
    // the predicate: every condition is needed
    expect(scan_bytes_eligible(1, true, 128, false), "option on, byte rows, d 128, no per-query filters");
    expect(scan_bytes_eligible(1, true, 1, false) && scan_bytes_eligible(1, true, 256, false), "d 1 and d 256");
    expect(!scan_bytes_eligible(0, true, 128, false), "option off (the default)");
    expect(!scan_bytes_eligible(1, false, 128, false), "no byte rows");
    expect(!scan_bytes_eligible(1, true, 257, false) && !scan_bytes_eligible(1, true, 0, false), "d out of range");
    expect(!scan_bytes_eligible(1, true, 128, true), "per-query filters keep the float scan");
    // rows and codes: 64 * NCH bytes, never shorter than d
    for (int d = 1; d <= SCAN_BYTES_MAX_D; ++d) {
        const int rb = scan_bytes_row_bytes(d), nch = ((d + 3) / 4 + 15) / 16;
        expect(rb >= d && rb % 64 == 0 && rb == 64 * (nch == 3 ? 4 : nch), "row bytes");
    }
    // scratch: the terms lie behind the codes, aligned, and everything is inside total
    for (int64_t piece : {1ll, 33ll, 1000ll, 16384ll})
        for (int d : {3, 64, 65, 128, 200, 256}) {
            const ScanBytesScratch s = scan_bytes_scratch(piece, d);
            expect(s.codes == piece * scan_bytes_row_bytes(d) && s.terms_at >= s.codes && s.terms_at % 16 == 0 && s.terms_at < s.codes + 16 &&
                       s.total == s.terms_at + 4 * piece,
                   "scratch layout");
        }
    // the grid covers the queries and the slabs
    for (int64_t v : {1ll, 32ll, 33ll, 10000ll})
        expect(scan_bytes_tiles(v) * SCAN_BYTES_TILE >= v && (scan_bytes_tiles(v) - 1) * SCAN_BYTES_TILE < v &&
                   scan_bytes_slab_groups(v) * SCAN_BYTES_WAVES >= v && (scan_bytes_slab_groups(v) - 1) * SCAN_BYTES_WAVES < v,
               "grid");
    std::printf("scan bytes plan %s: %d cases, %d failed\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
