// scan_plan (ocaml-hnsw_amd/csrc/hnsw_scan_plan.h) against the two loops it replaced (the slab rule they called moved as it was: it
// is here as their callee, what is cross-checked is the piece loop and its arguments), copied below as they stood in
// hnsw_scan.hip (scan_search: lists of 2 * k words per cell, 16 384 queries at most) and hnsw_range.hip (plan_exact: a count and
// an offset per cell, no cap).  Host arithmetic only: build with -fsanitize=address,undefined and run (tests/test_brute_force_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_scan_plan.h"

#include <cstdio>

namespace old {

constexpr int64_t SCAN_SCRATCH = 256ll << 20;

int64_t scan_slab_rows(int64_t n, int scan_slabs, int64_t tiles, int k) {
    constexpr int64_t SCAN_TARGET_WAVES = 8192;
    int64_t slabs = scan_slabs > 0 ? scan_slabs : (SCAN_TARGET_WAVES + tiles - 1) / tiles;
    if (scan_slabs <= 0) slabs = std::min(slabs, std::max<int64_t>(1, n / 256));
    slabs = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slabs, 1024), std::max<int64_t>(1, 65536 / k)));
    return std::max<int64_t>(1, (n + slabs - 1) / slabs);
}

void scan_search(int64_t n, int scan_slabs, int T, int64_t nq, int k, int64_t &piece, int64_t &slab_rows, int64_t &slabs) {
    piece = std::min<int64_t>(nq, 16384);
    for (;;) {
        slab_rows = scan_slab_rows(n, scan_slabs, (piece + T - 1) / T, k);
        slabs = n > 0 ? (n + slab_rows - 1) / slab_rows : 0;
        const int64_t per_query = std::max<int64_t>(slabs, 1) * 2 * k * 8;
        if (piece * per_query <= SCAN_SCRATCH || piece <= T) break;
        piece = std::max<int64_t>(T, SCAN_SCRATCH / per_query / T * T);
    }
}

void plan_exact(int64_t n, int scan_slabs, int T, int64_t m, int64_t &piece, int64_t &slab_rows, int64_t &slabs) {
    piece = m;
    for (;;) {
        slab_rows = scan_slab_rows(n, scan_slabs, (piece + T - 1) / T, 1);
        slabs = n > 0 ? (n + slab_rows - 1) / slab_rows : 0;
        const int64_t per_query = std::max<int64_t>(slabs, 1) * 16;
        if (piece * per_query <= SCAN_SCRATCH || piece <= T) break;
        piece = std::max<int64_t>(T, SCAN_SCRATCH / per_query / T * T);
    }
}

} // namespace old

int main() {
    int cases = 0, bad = 0;
    for (int64_t n : {0ll, 1ll, 255ll, 517ll, 1000000ll})
        for (int64_t m : {1ll, 9ll, 16385ll, 1000000ll})
            for (int k : {1, 10, 1024})
                for (int scan_slabs : {0, 1, 3, 1024})
                    for (int T : {4, 8}) {      // scan_tile's two values
                        int64_t kp, kr, ks, rp, rr, rs;       // piece, slab_rows, slabs: the k-scan's and the range scan's
                        old::scan_search(n, scan_slabs, T, m, k, kp, kr, ks);
                        old::plan_exact(n, scan_slabs, T, m, rp, rr, rs);
                        const hnsw_host::ScanPlan a = hnsw_host::scan_plan(n, scan_slabs, T, m, k, 2 * (int64_t)k * 8, 16384);
                        const hnsw_host::ScanPlan b = hnsw_host::scan_plan(n, scan_slabs, T, m, 1, 16, m);
                        if (a.piece != kp || a.slab_rows != kr || a.slabs != ks || b.piece != rp || b.slab_rows != rr || b.slabs != rs) {
                            ++bad;
                            std::printf("n %lld m %lld k %d scan_slabs %d T %d: k-scan %lld %lld %lld (was %lld %lld %lld), range %lld %lld %lld (was %lld %lld %lld)\n",
                                        (long long)n, (long long)m, k, scan_slabs, T, (long long)a.piece, (long long)a.slab_rows, (long long)a.slabs,
                                        (long long)kp, (long long)kr, (long long)ks, (long long)b.piece, (long long)b.slab_rows, (long long)b.slabs,
                                        (long long)rp, (long long)rr, (long long)rs);
                        }
                        // what the kernels rely on: the slabs cover the rows, a piece is at least one query
                        if (a.piece < 1 || b.piece < 1 || a.slabs * a.slab_rows < n || b.slabs * b.slab_rows < n) ++bad;
                        ++cases;
                    }
    std::printf("scan plan %s: %d cases, %d differ\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
