// hnsw_range.hip -- range search: every stored vector within distance `radius` of a query (hnsw_range_search_batch,
// hnsw_range_brute_force_batch, hnsw_range_result_*).  The result has no fixed k: per query a segment of (id, distance) pairs,
// ascending under the exact scan's order, found through lims [nq + 1].  The search composes pieces that exist already -- the
// ladder's loop and its W over the float32 rows (Ladder::run, Ladder::walk_exact, hnsw_filter.hip) -- with a stage body that keeps
// every stage's W, a select rule of its own and a scan that selects by a distance bound instead of by rank:
//   ladder   e = ef, 2 ef, ... 1024: a query is served at the first e whose W is not saturated (the walk ran out of graph, or W's
//            last member is out of range); its segment is W's in-range prefix.  Only the queries still saturated are walked again,
//            gathered into one compact batch;
//   exact    a query saturated at e = 1024, and every query of the brute-force form, gets the exact range scan.
//
// Kernels.
//   hnsw_range_scan_kernel<NCH, METRIC, PASS>  the exact scan's body (hnsw_scan_device.hip.h: grid, tile, rows in flight, the bits of
//                           hnsw_distance_batch) with a selection that keeps no order (RangeHits).  A row is a hit iff
//                           key_to_dist(key) <= radius; keys are monotone in distance, so that is lo <= key <= hi for two keys the
//                           wave finds first (range_key_bounds).  PASS 0 counts the hits per (query, slab); PASS 1 runs the same
//                           loop and writes the word (key << 32 | row) of each hit at the (query, slab)'s offset plus the hit's
//                           position among the slab's hits in id order (ballot, prefix count): the layout is deterministic.
//   hnsw_range_scan_masked_kernel<NCH, METRIC, PASS>  the same two passes over the rows an allow-mask names (the filtered range
//                           calls; the plain ones while nodes are marked deleted): RangeHits<.., MASKED = true>, whose skip / admits
//                           are ScanMask's, as every policy's -- a disallowed row is never counted, stored or sorted, and a mask
//                           word without a set bit is stepped over unloaded.
//   range_count_kernel      per exact-stage query the sum of its slabs' counts (from the exclusive sum), its counters and stage.
//   range_unpack_kernel     the sorted words of an exact-stage query as ids (+ id_base) and key_to_dist.
//   range_select_kernel     one wave per walked query: |W| and the length of W's in-range prefix, 64 entries per pass (ballot).
//                           Served: its count, stage and row.  Under a mask the stage test is the same one (the mask has no say in
//                           "saturated"); a served query records the prefix length and the number of allowed members in it: the
//                           second is its segment length.  Saturated: appended to the short list (ladder_settle); the ladder
//                           gathers them for the next walk.
//   range_fill_kernel       the served queries' prefixes from their stages' W to lims[q], once every size is known.  Under a mask:
//                           the allowed members of the prefix, compacted by ballot and prefix count, 64 entries per pass, in W's order.
// Between the scan's passes: an exclusive sum of the counts (hipcub::DeviceScan), the grand total read on the host, the result
// allocated.  After the fill hipcub::DeviceSegmentedRadixSort orders each exact-stage segment by its 64-bit words: ascending words
// = the total order (distance key, node id), no drops however many ties.  Vector stores only.  All scratch is the handle's
// (LadderBufs, RangeBufs): one filtered, range, grouped or paged call in flight per handle; lims, ids, distances and counters belong to the
// hnsw_range_result.
#include "hnsw_internal.h"
#include "hnsw_scan_device.hip.h"

#include <hipcub/hipcub.hpp>

namespace hnsw_dev {

struct RangeScanArgs {
    const float *Q;            // the queries of this launch
    int64_t q_stride, nq;
    int32_t n_slabs;
    int64_t slab_rows;         // slab s = rows [s * slab_rows, min(n, (s + 1) * slab_rows))
    float radius;
    uint64_t *counts;          // PASS 0: [nq][n_slabs] hits
    const uint64_t *offs;      // PASS 1: [nq * n_slabs + 1] the exclusive sum of counts
    const int64_t *xoff;       // PASS 1: [nq] where query i's words start ...
    uint64_t *words;           // ... in here
};

// The keys [lo, hi] whose distance is <= radius (hi < lo: none).  key_to_dist is monotone over the keys of real distances -- [0,
// +inf] for L2, [-inf, +inf] for the inner product; the keys outside are NaNs, never in range -- so the hits are an interval, found
// with the comparison the definition names: 32 steps of uniform work per wave instead of a square root per evaluation.
template <int METRIC> __device__ __forceinline__ void range_key_bounds(float radius, uint32_t &lo, uint32_t &hi) {
    const uint32_t first = METRIC == 0 ? 0u : 0x007FFFFFu, last = METRIC == 0 ? 0x7F800000u : 0xFF800000u;
    lo = first;
    if (!(key_to_dist<METRIC>(first) <= radius)) { lo = 1u; hi = 0u; return; }
    uint32_t a = first, b = last;              // a is in range; the answer lies in [a, b]
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1) + 1u;
        if (key_to_dist<METRIC>(mid) <= radius) a = mid; else b = mid - 1u;
    }
    hi = a;
}

// The hits of one (tile, slab) wave (scan_slab's Select): counted (PASS 0), or written where PASS 0's counts say (PASS 1)
// MASKED: only the rows the mask allows (skip and admits: ScanMask).
template <int NCH, int METRIC, int PASS, bool MASKED = false> struct RangeHits : ScanMask<MASKED> {
    static constexpr int T = scan_tile(NCH);
    const RangeScanArgs &a;
    uint32_t klo, khi;
    int64_t q0, slab;
    int tq, lane;
    // per query of the tile: its hits so far in this slab (wave-uniform); PASS 1: where its words go and how many PASS 0 counted
    int cnt[T], lim[T];
    uint64_t *dst[T];

    __device__ __forceinline__ explicit RangeHits(const RangeScanArgs &a_, const uint32_t *mask_ = nullptr) : ScanMask<MASKED>(mask_), a(a_) {}
    __device__ __forceinline__ void begin(int64_t q0_, int tq_, int64_t slab_) {
        q0 = q0_; tq = tq_; slab = slab_;
        lane = threadIdx.x & 63;
        range_key_bounds<METRIC>(a.radius, klo, khi);
        klo = (uint32_t)uniform((int)klo); khi = (uint32_t)uniform((int)khi);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            cnt[t] = 0;
            dst[t] = nullptr;
            lim[t] = 0;
            if (PASS == 1 && t < tq) {
                const int64_t at = (q0 + t) * a.n_slabs;
                dst[t] = a.words + a.xoff[q0 + t] + (int64_t)(a.offs[at + slab] - a.offs[at]);
                lim[t] = (int)(a.offs[at + slab + 1] - a.offs[at + slab]);
            }
        }
    }
    __device__ __forceinline__ void take(int t, uint32_t key, int64_t row, bool ok) {
        // a query past the tile's end has no hits; the rows of a batch lie in lane order: r ascending = id ascending
        const bool hit = (lane & 15) == 0 && ok && t < tq && key >= klo && key <= khi;
        const uint64_t m = ballot(hit);
        if (m) {
            if (PASS == 1) {
                const int pos = cnt[t] + popc(m & ((1ull << lane) - 1ull));
                if (hit && pos < lim[t]) dst[t][pos] = ((uint64_t)key << 32) | (uint32_t)row;
            }
            cnt[t] += popc(m);
        }
    }
    __device__ __forceinline__ void batch_end() {}
    __device__ __forceinline__ void end() {
        if (PASS == 0 && lane == 0) {
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (t < tq) a.counts[(q0 + t) * a.n_slabs + slab] = (uint64_t)cnt[t];
        }
    }
};

template <int NCH, int METRIC, int PASS>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_range_scan_kernel(const IndexView iv, const RangeScanArgs a) {
    RangeHits<NCH, METRIC, PASS> sel(a);
    scan_slab<NCH, METRIC>(iv, a.Q, a.q_stride, a.nq, a.n_slabs, a.slab_rows, sel);
}

// ... restricted to the rows `mask` allows (a kernel argument: scalar loads, wave-uniform tests)
template <int NCH, int METRIC, int PASS>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_range_scan_masked_kernel(const IndexView iv, const RangeScanArgs a, const uint32_t *mask) {
    RangeHits<NCH, METRIC, PASS, true> sel(a, mask);
    scan_slab<NCH, METRIC>(iv, a.Q, a.q_stride, a.nq, a.n_slabs, a.slab_rows, sel);
}

struct RangeCountArgs {
    const uint64_t *offs;      // [m * n_slabs + 1]
    int64_t m;
    int32_t n_slabs;
    const int32_t *map;        // [m] row i belongs to query map[i]; null: to query i
    uint32_t n;                // the rows scanned (under a mask: the allowed ones)
    int32_t fresh;             // 1: the query took no walk: out_nd starts from 0 and out_nh is 0
    int64_t *cnt, *xcnt;       // [nq] by query, [m] by row
    uint32_t *out_nd, *out_nh, *out_stage;
};

__global__ void __launch_bounds__(256)
range_count_kernel(const RangeCountArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.m) return;
    const int64_t q = a.map ? a.map[i] : i;
    const int64_t c = (int64_t)(a.offs[(i + 1) * a.n_slabs] - a.offs[i * a.n_slabs]);
    a.cnt[q] = c;
    a.xcnt[i] = c;
    exact_settle(a.out_nd, a.out_nh, a.out_stage, q, a.n, a.fresh != 0);
}

// one wave per exact-stage query: sorted words -> ids and distances at lims[q]
template <int METRIC>
__global__ void __launch_bounds__(64)
range_unpack_kernel(const uint64_t *words, const int64_t *xoff, int64_t m, const int32_t *map, const int64_t *lims, int32_t id_base,
                    int32_t *ids, float *dist) {
    const int64_t i = blockIdx.x;
    if (i >= m) return;
    const int64_t q = map ? map[i] : i;
    const int64_t from = xoff[i], c = xoff[i + 1] - from, to = lims[q];
    for (int64_t j = threadIdx.x; j < c; j += 64) {
        const uint64_t e = words[from + j];
        ids[to + j] = (int32_t)(uint32_t)e + id_base;
        dist[to + j] = key_to_dist<METRIC>((uint32_t)(e >> 32));
    }
}

struct RangeSelectArgs {
    const int32_t *wids;       // [m][e] the stage's W per query, id_base-based, ascending, filled entries < id_base
    const float *wdist;        // [m][e]
    int64_t m;
    int32_t e;
    const int32_t *map;        // [m] row i belongs to query map[i]; null: to query i
    float radius;
    int32_t id_base;
    int64_t *cnt;              // [nq] a served query's segment length
    int32_t *src;              // [nq] ... and its row of this stage's W
    LadderOut out;             // (its evaluations: the re-rank's included)
    const uint32_t *mask;      // null, or the allow-mask (ceil(n / 32) words): the segment is the allowed members of the prefix
    int64_t n;
    int32_t *pre;              // [nq] under a mask: the served query's prefix length
};

__global__ void __launch_bounds__(64)
range_select_kernel(const RangeSelectArgs a) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= a.m) return;
    const int64_t q = a.map ? a.map[i] : i;
    const MaskWords bits = mask_words(a.mask);
    int in = 0, al = 0;        // W is ascending: its members in range are a prefix; al: the allowed ones among them
    for (int j0 = 0; j0 < a.e; j0 += 64) {
        const int j = j0 + lane;
        const bool hit = j < a.e && a.wids[i * a.e + j] >= a.id_base && a.wdist[i * a.e + j] <= a.radius;
        in += popc(ballot(hit));
        if (a.mask) al += popc(ballot(hit && node_allowed(bits, a.n, a.id_base, a.wids[i * a.e + j])));
    }
    // saturated: |W| = e and its last member is in range, that is all e entries are -- whatever the mask says
    if (lane == 0) {
        if (in < a.e) {
            a.cnt[q] = a.mask ? al : in;
            a.src[q] = (int32_t)i;
            if (a.mask) a.pre[q] = in;
        }
        ladder_settle(a.out, i, q, in < a.e);
    }
}

struct RangeFillArgs {
    const int32_t *wids[hnsw_host::RANGE_STAGES];    // per stage its W ...
    const float *wdist[hnsw_host::RANGE_STAGES];
    int32_t e[hnsw_host::RANGE_STAGES];              // ... and its row length
    int32_t n_stages;
    int64_t nq;
    const uint32_t *stage;     // [nq]
    const int32_t *src;        // [nq]
    const int64_t *lims;       // [nq + 1]
    int32_t *ids;
    float *dist;
    const uint32_t *mask;      // null, or the allow-mask: only the allowed members of the prefix [0, pre[q]) are copied
    int64_t n;
    int32_t id_base;
    const int32_t *pre;        // [nq]
};

__global__ void __launch_bounds__(64)
range_fill_kernel(const RangeFillArgs a) {
    const int64_t q = blockIdx.x;
    if (q >= a.nq) return;
    const uint32_t s = a.stage[q];
    if (s >= (uint32_t)a.n_stages) return;          // the exact stage writes its own
    const int64_t to = a.lims[q], c = a.lims[q + 1] - to, from = (int64_t)a.src[q] * a.e[s];
    if (a.mask) {               // W's order kept: an entry's place is the number of allowed entries before it
        const MaskWords bits = mask_words(a.mask);
        const int lane = threadIdx.x, pre = a.pre[q];
        int64_t at = 0;
        for (int j0 = 0; j0 < pre && at < c; j0 += 64) {
            const int j = j0 + lane;
            const int32_t id = j < pre ? a.wids[s][from + j] : a.id_base - 1;
            const bool ok = j < pre && node_allowed(bits, a.n, a.id_base, id);
            const uint64_t m = ballot(ok);
            const int64_t pos = at + popc(m & ((1ull << lane) - 1ull));
            if (ok && pos < c) {
                a.ids[to + pos] = id;
                a.dist[to + pos] = a.wdist[s][from + j];
            }
            at += popc(m);
        }
        return;
    }
    for (int64_t j = threadIdx.x; j < c; j += 64) {
        a.ids[to + j] = a.wids[s][from + j];
        a.dist[to + j] = a.wdist[s][from + j];
    }
}

} // namespace hnsw_dev

using hnsw_dev::IndexView;
using namespace hnsw_host;

namespace {

// out[0 .. count) = the exclusive sum of in[0 .. count) on st (count >= 1), through the handle's temporary storage
template <class T, class U>
int exclusive_sum(RangeBufs &rb, const T *in, U *out, int64_t count, hipStream_t st) {
    if (count > 0x7FFFFFFFLL) return fail(HNSW_ERR_UNSUPPORTED, "%lld counts to sum: too many for one range call", (long long)count);
    size_t bytes = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)count, st) != hipSuccess) return fail(HNSW_ERR_HIP, "scan sizing failed");
    int rc;
    if ((rc = rb.cub.ensure(std::max<size_t>(bytes, 16)))) return rc;
    bytes = rb.cub.bytes;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(rb.cub.p, bytes, in, out, (int)count, st);
    return e == hipSuccess ? HNSW_OK : fail(HNSW_ERR_HIP, "exclusive sum failed: %s", hipGetErrorString(e));
}

// The queries of the exact stage -- (Q, map): m rows, row i belonging to query map[i] (null: to query i) -- and how they are cut.
// A piece's counts and offsets fit SCAN_SCRATCH bytes of the handle's scratch, as the k-scan's lists do.
struct ExactPlan : ScanCut {
    const float *Q = nullptr;
    int64_t m = 0, q_stride = 0;
    const int32_t *map = nullptr;
    const uint32_t *mask = nullptr;    // the call's allow-mask (device words), null: every row
    int64_t n_allowed = 0;             // ... and how many rows it allows: what the exact stage adds to out_ndist (no mask: n)
    // (a count and an offset per (query, slab) cell)
    void cut(const hnsw_index *idx) { static_cast<ScanCut &>(*this) = scan_cut(idx, m, 1, 16, m); }
};

int launch_range_scan(const hnsw_index *idx, const ExactPlan &x, int pass, int64_t nq, const hnsw_dev::RangeScanArgs &a, hipStream_t st) {
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(x.nch, [&](auto NCH) {
        if (x.mask && pass == 0) hipLaunchKernelGGL((hnsw_dev::hnsw_range_scan_masked_kernel<NCH, METRIC, 0>), x.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, idx->iv, a, x.mask);
        else if (x.mask) hipLaunchKernelGGL((hnsw_dev::hnsw_range_scan_masked_kernel<NCH, METRIC, 1>), x.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, idx->iv, a, x.mask);
        else if (pass == 0) hipLaunchKernelGGL((hnsw_dev::hnsw_range_scan_kernel<NCH, METRIC, 0>), x.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, idx->iv, a);
        else hipLaunchKernelGGL((hnsw_dev::hnsw_range_scan_kernel<NCH, METRIC, 1>), x.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, idx->iv, a);
    }); });
    return launched("range scan kernel");
}

// PASS 0 for the rows [i0, i0 + mp) of x and the exclusive sum of its counts (rb.offs: [mp * slabs + 1])
int exact_count_piece(hnsw_index *idx, const ExactPlan &x, float radius, int64_t i0, int64_t mp, hipStream_t st) {
    RangeBufs &rb = idx->range_scratch;
    const int64_t cells = mp * x.slabs;
    hnsw_dev::RangeScanArgs a{x.Q + i0 * x.q_stride, x.q_stride, mp, (int32_t)x.slabs, x.slab_rows, radius, (uint64_t *)rb.counts.p, nullptr, nullptr, nullptr};
    HIP_TRY(hipMemsetAsync((uint64_t *)rb.counts.p + cells, 0, 8, st));       // (the sum's last entry is the piece's total)
    int rc;
    if ((rc = launch_range_scan(idx, x, 0, mp, a, st))) return rc;
    return exclusive_sum(rb, (const uint64_t *)rb.counts.p, (uint64_t *)rb.offs.p, cells + 1, st);
}

// The sizes of the exact stage's segments: cnt[q] and xcnt[i] for every row of x, the queries' counters and stage
int exact_count(hnsw_index *idx, const ExactPlan &x, float radius, bool fresh, hipStream_t st) {
    RangeBufs &rb = idx->range_scratch;
    int rc;
    if ((rc = rb.xcnt.ensure((size_t)(x.m + 1) * 8)) || (rc = rb.xoff.ensure((size_t)(x.m + 1) * 8))) return rc;
    if (x.slabs == 0) {         // no rows: every segment is empty (a sum of one zero stands for the offsets)
        if ((rc = rb.offs.ensure(16))) return rc;
        HIP_TRY(hipMemsetAsync(rb.offs.p, 0, 16, st));
        const hnsw_dev::RangeCountArgs ca{(const uint64_t *)rb.offs.p, x.m, 0, x.map, 0u, fresh, (int64_t *)rb.cnt.p, (int64_t *)rb.xcnt.p,
                                          (uint32_t *)rb.nd.p, (uint32_t *)rb.nh.p, (uint32_t *)rb.stage.p};
        hipLaunchKernelGGL(hnsw_dev::range_count_kernel, dim3((unsigned)((x.m + 255) / 256)), dim3(256), 0, st, ca);
        return launched("range count kernel");
    }
    if ((rc = rb.counts.ensure((size_t)(x.piece * x.slabs + 1) * 8)) || (rc = rb.offs.ensure((size_t)(x.piece * x.slabs + 1) * 8))) return rc;
    for (int64_t i0 = 0; i0 < x.m; i0 += x.piece) {
        const int64_t mp = std::min(x.piece, x.m - i0);
        if ((rc = exact_count_piece(idx, x, radius, i0, mp, st))) return rc;
        const hnsw_dev::RangeCountArgs ca{(const uint64_t *)rb.offs.p, mp, (int32_t)x.slabs, x.map ? x.map + i0 : nullptr, (uint32_t)x.n_allowed, fresh,
                                          x.map ? (int64_t *)rb.cnt.p : (int64_t *)rb.cnt.p + i0, (int64_t *)rb.xcnt.p + i0,
                                          x.map ? (uint32_t *)rb.nd.p : (uint32_t *)rb.nd.p + i0, x.map ? (uint32_t *)rb.nh.p : (uint32_t *)rb.nh.p + i0,
                                          x.map ? (uint32_t *)rb.stage.p : (uint32_t *)rb.stage.p + i0};
        hipLaunchKernelGGL(hnsw_dev::range_count_kernel, dim3((unsigned)((mp + 255) / 256)), dim3(256), 0, st, ca);
        if ((rc = launched("range count kernel"))) return rc;
    }
    return HNSW_OK;
}

// PASS 1, the sort and the unpacking for the rows of x, whose sizes exact_count found: ids and distances at r's lims
int exact_fill(hnsw_index *idx, const ExactPlan &x, float radius, hnsw_range_result *r, hipStream_t st) {
    RangeBufs &rb = idx->range_scratch;
    int rc;
    HIP_TRY(hipMemsetAsync((int64_t *)rb.xcnt.p + x.m, 0, 8, st));
    if ((rc = exclusive_sum(rb, (const int64_t *)rb.xcnt.p, (int64_t *)rb.xoff.p, x.m + 1, st))) return rc;
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, (const int64_t *)rb.xoff.p + x.m, 8, hipMemcpyDeviceToHost, st));
    if ((rc = synced(st, "range scan"))) return rc;
    if (total == 0) return HNSW_OK;     // (at most r->total: within int)
    if ((rc = rb.words[0].ensure((size_t)total * 8)) || (rc = rb.words[1].ensure((size_t)total * 8))) return rc;
    for (int64_t i0 = 0; i0 < x.m; i0 += x.piece) {
        const int64_t mp = std::min(x.piece, x.m - i0);
        // (one piece: its offsets are still in place)
        if (x.piece < x.m && (rc = exact_count_piece(idx, x, radius, i0, mp, st))) return rc;
        const hnsw_dev::RangeScanArgs a{x.Q + i0 * x.q_stride, x.q_stride, mp, (int32_t)x.slabs, x.slab_rows, radius, nullptr,
                                        (const uint64_t *)rb.offs.p, (const int64_t *)rb.xoff.p + i0, (uint64_t *)rb.words[0].p};
        if ((rc = launch_range_scan(idx, x, 1, mp, a, st))) return rc;
    }
    // each segment by its words: (distance key, node id) ascending
    size_t bytes = 0;
    const int64_t *xo = (const int64_t *)rb.xoff.p;
    if (hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)total, (int)x.m, xo, xo + 1, 0, 64,
                                                   st) != hipSuccess)
        return fail(HNSW_ERR_HIP, "segmented sort sizing failed");
    if ((rc = rb.cub.ensure(std::max<size_t>(bytes, 16)))) return rc;
    bytes = rb.cub.bytes;
    const hipError_t e = hipcub::DeviceSegmentedRadixSort::SortKeys(rb.cub.p, bytes, (const uint64_t *)rb.words[0].p, (uint64_t *)rb.words[1].p, (int)total,
                                                                    (int)x.m, xo, xo + 1, 0, 64, st);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "segmented sort failed: %s", hipGetErrorString(e));
    with_metric(idx->info.metric, [&](auto METRIC) {
        hipLaunchKernelGGL(hnsw_dev::range_unpack_kernel<METRIC>, dim3((unsigned)x.m), dim3(64), 0, st, (const uint64_t *)rb.words[1].p, xo, x.m, x.map,
                           (const int64_t *)r->lims.p, idx->iv.id_base, (int32_t *)r->ids.p, (float *)r->dist.p);
    });
    return launched("range unpack kernel");
}

// The ladder for the batch (Q, nq, q_stride) on st: cnt / src / stage / nd / nh of the served queries in the handle's scratch,
// the saturated ones left in x (gathered); e_of: the row length of each stage walked.  d_stage: see knn_search.
int range_ladder(hnsw_index *idx, const hnsw_filter *f, const hnsw_range_params &p, const float *Q, int64_t nq, int64_t q_stride, float *d_stage, hipStream_t st,
                 ExactPlan &x, std::vector<int32_t> &e_of) {
    RangeBufs &rb = idx->range_scratch;
    Ladder L(idx, Q, nq, q_stride, p.ef, p.semantics, d_stage, st, "range search");
    LadderLeft left;
    int rc;
    rc = L.run(true, [&](Ladder &, int64_t m, int e) -> int {
        DevBuf &Wi = rb.wids[L.stage], &Wd = rb.wdist[L.stage];
        if ((rc = Wi.ensure((size_t)m * e * 4)) || (rc = Wd.ensure((size_t)m * e * 4))) return rc;
        e_of.push_back(e);
        if ((rc = L.walk_exact((int32_t *)Wi.p, (float *)Wd.p, HNSW_FILL_OHNSW))) return rc;
        const hnsw_dev::RangeSelectArgs sa{(const int32_t *)Wi.p, (const float *)Wd.p, m, e, L.map, p.radius, idx->iv.id_base, (int64_t *)rb.cnt.p,
                                           (int32_t *)rb.src.p, L.out((uint32_t *)rb.nd.p, (uint32_t *)rb.nh.p, (uint32_t *)rb.stage.p),
                                           f ? (const uint32_t *)f->bits.p : nullptr, idx->iv.n, (int32_t *)rb.pre.p};
        hipLaunchKernelGGL(hnsw_dev::range_select_kernel, dim3((unsigned)m), dim3(64), 0, st, sa);
        return launched("range select kernel");
    }, left);
    x.m = 0;
    if (rc || left == LadderLeft::none) return rc;
    x.Q = L.Qj; x.m = L.m; x.q_stride = L.qs; x.map = L.map;
    return HNSW_OK;
}

// All four entry points: p null = the brute-force form (every query is the exact stage's); f null = no mask (the unfiltered entry
// points on a handle without marked nodes).  *out is set on success only.
int range_call(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride, const hnsw_range_params *p, float radius, hnsw_range_result **out) {
    HIP_TRY(hipSetDevice(idx->device));
    std::unique_ptr<hnsw_range_result> r(new hnsw_range_result());
    r->device = idx->device;
    r->nq = nq;
    int rc;
    if ((rc = r->lims.ensure((size_t)(nq + 1) * 8))) return rc;
    if (nq == 0) {
        HIP_TRY(hipMemset(r->lims.p, 0, 8));
        *out = r.release();
        return HNSW_OK;
    }
    if (f && f->n_allowed == 0) {       // no node allowed: no walk, every segment empty
        if ((rc = r->nd.ensure((size_t)nq * 4)) || (rc = r->nh.ensure((size_t)nq * 4)) || (rc = r->stage.ensure((size_t)nq * 4)) ||
            (rc = r->ids.ensure(4)) || (rc = r->dist.ensure(4)))
            return rc;
        HIP_TRY(hipMemset(r->lims.p, 0, (size_t)(nq + 1) * 8));
        HIP_TRY(hipMemset(r->nd.p, 0, (size_t)nq * 4));
        HIP_TRY(hipMemset(r->nh.p, 0, (size_t)nq * 4));
        HIP_TRY(hipMemset(r->stage.p, 0xFF, (size_t)nq * 4));
        HIP_TRY(hipDeviceSynchronize());
        *out = r.release();
        return HNSW_OK;
    }
    RangeBufs &rb = idx->range_scratch;
    if ((rc = rb.cnt.ensure((size_t)(nq + 1) * 8)) || (rc = rb.src.ensure((size_t)nq * 4)) || (rc = rb.pre.ensure((size_t)nq * 4)) || (rc = rb.stage.ensure((size_t)nq * 4)) ||
        (rc = rb.nd.ensure((size_t)nq * 4)) || (rc = rb.nh.ensure((size_t)nq * 4)) || (rc = r->nd.ensure((size_t)nq * 4)) ||
        (rc = r->nh.ensure((size_t)nq * 4)) || (rc = r->stage.ensure((size_t)nq * 4)))
        return rc;
    HostCall c;
    bool q_in_place = false;
    if ((rc = c.begin(idx, queries, nq, q_stride, 1, nullptr, nullptr, nullptr, nullptr, false, &q_in_place))) return rc;
    hipStream_t st = idx->hs[0];
    // from here on work is queued that reads the caller's queries: no return without a synchronisation
    ExactPlan x;
    x.mask = f ? (const uint32_t *)f->bits.p : nullptr;
    x.n_allowed = f ? f->n_allowed : idx->iv.n;
    std::vector<int32_t> e_of;
    if (p) {
        rc = range_ladder(idx, f, *p, c.b.Q, nq, q_stride, q_in_place ? (float *)idx->scratch.q.p : nullptr, st, x, e_of);
    } else {
        x.Q = c.b.Q; x.m = nq; x.q_stride = q_stride; x.map = nullptr;
    }
    if (!rc && x.m > 0) {
        x.cut(idx);
        rc = exact_count(idx, x, radius, !p, st);
    }
    // every query's size is known: lims, the grand total, the result's buffers
    int64_t total = 0;
    if (!rc && hipMemsetAsync((int64_t *)rb.cnt.p + nq, 0, 8, st) != hipSuccess) rc = fail(HNSW_ERR_HIP, "memset failed");
    if (!rc) rc = exclusive_sum(rb, (const int64_t *)rb.cnt.p, (int64_t *)r->lims.p, nq + 1, st);
    if (!rc && hipMemcpyAsync(&total, (const int64_t *)r->lims.p + nq, 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(HNSW_ERR_HIP, "total download failed");
    if (!rc) rc = synced(st, "range search");
    if (!rc && total > 0x7FFFFFFFLL) rc = fail(HNSW_ERR_UNSUPPORTED, "%lld results: more than 2^31 - 1 in one call", (long long)total);
    if (!rc) {
        r->total = total;
        if (!(rc = r->ids.ensure((size_t)std::max<int64_t>(total, 1) * 4))) rc = r->dist.ensure((size_t)std::max<int64_t>(total, 1) * 4);
    }
    if (!rc && p && total > 0) {
        hnsw_dev::RangeFillArgs fa{};
        fa.n_stages = (int32_t)e_of.size();
        for (int s = 0; s < fa.n_stages; ++s) {
            fa.wids[s] = (const int32_t *)rb.wids[s].p; fa.wdist[s] = (const float *)rb.wdist[s].p; fa.e[s] = e_of[(size_t)s];
        }
        fa.nq = nq; fa.stage = (const uint32_t *)rb.stage.p; fa.src = (const int32_t *)rb.src.p; fa.lims = (const int64_t *)r->lims.p;
        fa.ids = (int32_t *)r->ids.p; fa.dist = (float *)r->dist.p;
        fa.mask = x.mask; fa.n = idx->iv.n; fa.id_base = idx->iv.id_base; fa.pre = (const int32_t *)rb.pre.p;
        hipLaunchKernelGGL(hnsw_dev::range_fill_kernel, dim3((unsigned)nq), dim3(64), 0, st, fa);
        rc = launched("range fill kernel");
    }
    if (!rc && x.m > 0 && total > 0) rc = exact_fill(idx, x, radius, r.get(), st);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(r->nd.p, rb.nd.p, (size_t)nq * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(r->nh.p, rb.nh.p, (size_t)nq * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(r->stage.p, rb.stage.p, (size_t)nq * 4, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) rc = hip_fail(e, "counter copy");
    }
    const int rs = synced(st, p ? "range search" : "range scan");
    if (rc || rs) return rc ? rc : rs;
    *out = r.release();
    return HNSW_OK;
}

int check_range(const hnsw_index *idx, int64_t nq, int64_t q_stride, const float *queries, float radius) {
    if (std::isnan(radius)) return fail(HNSW_ERR_BAD_ARG, "the radius is NaN");
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    if (nq == 0) return HNSW_OK;
    if (!queries) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    if (q_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "q_stride < d");
    return HNSW_OK;
}

} // namespace

extern "C" {

// the two ladder entry points: `filtered` = f is the caller's and is checked; else f is null and the handle's marks decide
static int32_t range_search_entry(hnsw_index *idx, bool filtered, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                  const hnsw_range_params *params, hnsw_range_result **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (!params) return fail(HNSW_ERR_BAD_ARG, "null params");
    if (std::isnan(params->radius)) return fail(HNSW_ERR_BAD_ARG, "the radius is NaN");
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (params->ef < 1) return fail(HNSW_ERR_BAD_ARG, "ef must be >= 1 (ef=%d)", params->ef);
    if (params->ef > 1024) return fail(HNSW_ERR_UNSUPPORTED, "ef=%d > 1024 not supported", params->ef);
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "the k farthest of W (HNSW_SEM_FUNCTOR_NEAREST_K) have no range meaning");
    if (params->semantics != HNSW_SEM_OHNSW && params->semantics != HNSW_SEM_FUNCTOR) return fail(HNSW_ERR_BAD_ARG, "bad semantics %d", params->semantics);
    if (idx->iv.entry_point < 0) return fail(HNSW_ERR_EMPTY_INDEX, "range search: empty hgraph");
    int rc = check_range(idx, nq, q_stride, queries, params->radius);
    if (rc) return rc;
    if (filtered && (rc = check_filter(idx, f))) return rc;
    return range_call(idx, filtered ? f : live_filter(idx), queries, nq, q_stride, params, params->radius, out);
}

static int32_t range_brute_entry(hnsw_index *idx, bool filtered, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                 float radius, hnsw_range_result **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (std::isnan(radius)) return fail(HNSW_ERR_BAD_ARG, "the radius is NaN");
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    int rc = check_range(idx, nq, q_stride, queries, radius);
    if (rc) return rc;
    if (filtered && (rc = check_filter(idx, f))) return rc;
    return range_call(idx, filtered ? f : live_filter(idx), queries, nq, q_stride, nullptr, radius, out);
}

int32_t hnsw_range_search_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, const hnsw_range_params *params,
                                hnsw_range_result **out) {
    return range_search_entry(idx, false, nullptr, queries, nq, q_stride, params, out);
}

int32_t hnsw_range_search_batch_filtered(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                         const hnsw_range_params *params, hnsw_range_result **out) {
    return range_search_entry(idx, true, f, queries, nq, q_stride, params, out);
}

int32_t hnsw_range_brute_force_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, float radius, hnsw_range_result **out) {
    return range_brute_entry(idx, false, nullptr, queries, nq, q_stride, radius, out);
}

int32_t hnsw_range_brute_force_batch_filtered(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                              float radius, hnsw_range_result **out) {
    return range_brute_entry(idx, true, f, queries, nq, q_stride, radius, out);
}

// the result's functions (the bodies: RangeRecord, hnsw_internal.h)
int32_t hnsw_range_result_size(const hnsw_range_result *r, int64_t *nq, int64_t *total) { return RangeRecord<int32_t>::size(r, nq, total); }
int32_t hnsw_range_result_fetch(hnsw_range_result *r, int64_t *lims, int32_t *ids, float *dist, uint32_t *out_ndist, uint32_t *out_nhops,
                                uint32_t *out_stage) {
    return RangeRecord<int32_t>::fetch(r, lims, ids, dist, out_ndist, out_nhops, out_stage);
}
int32_t hnsw_range_result_device(hnsw_range_result *r, const int64_t **d_lims, const int32_t **d_ids, const float **d_dist) {
    return RangeRecord<int32_t>::device_pointers(r, d_lims, d_ids, d_dist);
}
int32_t hnsw_range_result_destroy(hnsw_range_result *r) { delete r; return HNSW_OK; }

} // extern "C"
