// group_plan (ocaml-hnsw_amd/csrc/hnsw_group_plan.h) against a naive restatement over a grid of (n_labels, m, T): the piece is the
// largest multiple of T, found by counting up, whose cells (8 * n_labels bytes per query) fit SCAN_SCRATCH and that is not more
// than m rounded up to whole tiles -- one tile when not even T queries fit.  Then what the driver relies on: walking the queries
// piece by piece puts every query in exactly one launch.  Host arithmetic only: build with -fsanitize=address,undefined and run
// (tests/test_grouped_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_group_plan.h"

#include <cstdio>
#include <vector>

static int64_t naive_piece(int T, int64_t m, int64_t n_labels) {
    int64_t piece = T;                       // never below one tile
    while (piece < m && (piece + T) * 8 * n_labels <= hnsw_host::SCAN_SCRATCH) piece += T;
    return piece;
}

int main() {
    int cases = 0, bad = 0;
    for (int64_t n_labels : {1ll, 7ll, 1000ll, 100000ll, 1000000ll, 4194304ll, 4194305ll, 8388608ll, 33554432ll, 2147483647ll})
        for (int64_t m : {1ll, 3ll, 4ll, 8ll, 9ll, 63ll, 64ll, 1000ll, 10007ll})
            for (int T : {4, 8}) {          // scan_tile's two values
                const hnsw_host::GroupPlan g = hnsw_host::group_plan(2003, 0, T, m, n_labels, 10);
                const int64_t want = naive_piece(T, m, n_labels);
                bool ok = g.piece == want && g.piece % T == 0 && g.piece >= T;
                // within the scratch bound whenever T queries fit
                if ((int64_t)T * 8 * n_labels <= hnsw_host::SCAN_SCRATCH) ok = ok && g.piece * 8 * n_labels <= hnsw_host::SCAN_SCRATCH;
                else ok = ok && g.piece == T;
                // the rows' cut covers the table
                ok = ok && g.slabs >= 1 && g.slabs * g.slab_rows >= 2003;
                // every query lies in exactly one piece
                std::vector<int> seen((size_t)m, 0);
                for (int64_t q0 = 0; q0 < m; q0 += g.piece) {
                    const int64_t nq = std::min(g.piece, m - q0);
                    ok = ok && nq >= 1 && q0 % T == 0;
                    for (int64_t q = q0; q < q0 + nq; ++q) ++seen[(size_t)q];
                }
                for (int s : seen) ok = ok && s == 1;
                if (!ok) {
                    ++bad;
                    std::printf("n_labels %lld m %lld T %d: piece %lld (naive %lld) slabs %lld x %lld\n", (long long)n_labels, (long long)m, T,
                                (long long)g.piece, (long long)want, (long long)g.slabs, (long long)g.slab_rows);
                }
                ++cases;
            }
    // an empty table has no slab
    if (hnsw_host::group_plan(0, 0, 8, 5, 3, 1).slabs != 0) ++bad;
    std::printf("group plan %s: %d cases, %d differ\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
