// hnsw_scan_bytes_plan.h, the range scan's part (option "scan_bytes" 2, hnsw_range_bytes.hip): which option values send which scans
// through the byte kernels, and the integer bound of a key interval.  Built with -fsanitize=address,undefined (tests/test_range_bytes_api.py).
#include "../../ocaml-hnsw_amd/csrc/hnsw_scan_bytes_plan.h"

#include <cstdio>
#include <initializer_list>

int main() {
    using namespace hnsw_host;
    int bad = 0, cases = 0;
    auto expect = [&](bool ok, const char *what) { ++cases; if (!ok) { ++bad; std::printf("FAILED: %s\n", what); } };
    for (int option : {-1, 0, 1, 2, 3}) {       // 0: nothing; 1: the k-scans only; 2: both; anything else: nothing
        expect(scan_bytes_eligible(option, true, 128, false) == (option == 1 || option == 2), "the k-scans: 1 and 2");
        expect(range_bytes_eligible(option, true, 128, false) == (option == 2), "the range scans: 2 alone");
    }
    expect(range_bytes_eligible(2, true, 1, false) && range_bytes_eligible(2, true, 256, false) && !range_bytes_eligible(2, false, 128, false) &&
               !range_bytes_eligible(2, true, 257, false) && !range_bytes_eligible(2, true, 0, false) && !range_bytes_eligible(2, true, 128, true),
           "the k-scan's other conditions hold for the range scans");
    // the key is the scans': the bits of the float the integer is (L2), of 1 - product (IP: products 0, 1, 2)
    expect(range_bytes_key(0, 0) == 0u && range_bytes_key(0, 16646400) == 0x4B7E0100u && range_bytes_key(1, 0) == 0xBF800000u &&
               range_bytes_key(1, -1) == 0x80000000u && range_bytes_key(1, -2) == 0x407FFFFFu, "keys");
    expect((int64_t)RANGE_BYTES_NO_ROW - (1ll << 23) > (1ll << 26) && (int64_t)RANGE_BYTES_NO_HIT < -(1ll << 27), "sentinels out of the values' reach");
    for (int metric : {0, 1}) {
        const int32_t lo = metric == 0 ? 0 : -RANGE_BYTES_MAX_M, hi = metric == 0 ? RANGE_BYTES_MAX_M : 0;
        const uint32_t klo = metric == 0 ? 0u : 0x007FFFFFu;        // range_key_bounds' first key
        bool mono = range_bytes_key(metric, lo) >= klo;
        for (int32_t m = lo; m < hi; ++m) mono = mono && range_bytes_key(metric, m) < range_bytes_key(metric, m + 1);
        expect(mono, "strictly monotone over the whole range");
        // {m : klo <= key(m) <= khi} is exactly {m <= bound} for a khi on a key, just below it, just above it: key(m) - 1 admits m - 1
        // and not m, key(m) + 1 admits m + 1 only where that is m + 1's key
        int32_t b = 0;
        for (int32_t m : {lo, lo + 1, lo + 7, (lo + hi) / 2, hi - 12345, hi - 1, hi})
            for (int off : {-1, 0, 1}) {
                const uint32_t km = range_bytes_key(metric, m), khi = km + (uint32_t)off;
                if (km == 0u && off < 0) continue;      // (no key lies below L2's zero)
                const bool some = range_bytes_bound(metric, klo, khi, &b);
                const int32_t want = off < 0 ? m - 1 : (off > 0 && m < hi && range_bytes_key(metric, m + 1) <= khi) ? m + 1 : m;
                expect(want < lo ? !some : (some && b == want), "the bound of a key interval");
            }
        expect(range_bytes_bound(metric, klo, metric == 0 ? 0x7F800000u : 0xFF800000u, &b) && b == hi, "a radius that admits all");
        expect(!range_bytes_bound(metric, 1u, 0u, &b), "a radius that admits nothing (range_key_bounds' empty interval)");
    }
    std::printf("range bytes plan %s: %d cases, %d failed\n", bad ? "FAILED" : "ok", cases, bad);
    return bad ? 1 : 0;
}
