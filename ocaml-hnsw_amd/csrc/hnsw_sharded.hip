// hnsw_sharded.hip -- one data set PARTITIONED over several GPUs: each listed device holds a slice of the rows with a graph of its
// own, every query visits all slices, and the per-slice answers are merged on the first device under the library's total order
// (distance, global id).  hnsw_multi (hnsw_multi.hip) replicates the index and splits the batch: that scales throughput; this
// scales capacity.  The structure of a call is search_and_gather's: per-device streams, one flag word per device, a single host
// round trip, knn_repair for a flagged shard -- with peer copies to devices[0] and the merge kernel where hnsw_multi has its
// exchange.  No RCCL: the copies are 8 bytes * nq * k per shard.
// The calls that are host-driven ladders on a single index -- filtered k-NN, range search -- run the public single-index call per
// shard on a host thread of its own (on_shards) and merge what comes back: rows by the same merge kernel, range segments by the
// rank merge (hnsw_merge_segments_kernel).  A sharded filter is the global mask cut into one ordinary filter per shard.
#include "hnsw_internal.h"

#include <atomic>
#include <system_error>
#include <thread>

using namespace hnsw_host;

namespace hnsw_dev {

constexpr int MERGE_LISTS = 64;          // one lane per list: the wave width

// n_lists lists per query, each [nq][k_in], ascending under (distance, id), padding (id < id_base) at the end
struct MergeArgs {
    const int32_t *ids;                  // [n_lists][nq][k_in], id_base-based ids local to the list
    const float *dist;                   // [n_lists][nq][k_in]
    const uint32_t *nd, *nh;             // [n_lists][nq] counters to sum per query, or null
    const uint32_t *stg;                 // [n_lists][nq] a counter to reduce with max (unsigned) per query, or null
    int64_t nq;
    int32_t n_lists, k_in, k_out, id_base, fill;
    int64_t *out_ids;                    // [nq][k_out]: first_row[list] + id
    float *out_dist;                     // [nq][k_out]
    uint32_t *out_nd, *out_nh, *out_stg; // [nq], written when nd / nh / stg are given
    int64_t first_row[MERGE_LISTS];
};

// float bits -> a word whose unsigned order is the floats' IEEE order (negative distances: the inner product's range)
__device__ __forceinline__ uint32_t merge_key(float d) {
    const uint32_t b = __float_as_uint(d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    const uint32_t r = (uint32_t)reduce16_i32((int32_t)v);
    return rdlane(r, 0) + rdlane(r, 16) + rdlane(r, 32) + rdlane(r, 48);
}

// One wave per query; lane g owns list g and keeps its head as (key, global id): the order-preserving word of the distance and
// the 64-bit global id -- 96 bits, not one 64-bit word, because a sharded table may hold more than 2^32 rows.  k_out rounds: the
// wave takes the minimum key (wave_min_u32: DPP inside the rows, the four row results through scalar registers); only when
// several heads share it -- equal distances across lists -- two more minima over the halves of the global id pick the winner.
// The winning lane stores the result and loads its list's next entry.  A list is exhausted at its k_in-th entry or at its first
// padding entry.  The lists are read by per-lane strided loads: nq * n_lists * k_in * 8 bytes in all, each read once.
__global__ void __launch_bounds__(MERGE_LISTS)
hnsw_merge_lists_kernel(const MergeArgs a) {
    const int64_t q = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const bool mine = lane < a.n_lists;
    const int64_t row = mine ? ((int64_t)lane * a.nq + q) * a.k_in : 0;
    const int64_t first = mine ? a.first_row[lane] : 0;
    int pos = 0;
    bool live = false;
    uint32_t key = 0xFFFFFFFFu, ghi = 0xFFFFFFFFu, glo = 0xFFFFFFFFu;
    int64_t gid = 0;
    float d = 0.0f;
    auto load_head = [&]() {
        live = false;
        if (mine && pos < a.k_in) {
            const int32_t id = a.ids[row + pos];
            if (id >= a.id_base) {
                live = true;
                d = a.dist[row + pos];
                key = merge_key(d);
                gid = first + id;
                const uint64_t u = (uint64_t)gid ^ 0x8000000000000000ull;      // signed order as unsigned order
                ghi = (uint32_t)(u >> 32); glo = (uint32_t)u;
            }
        }
    };
    load_head();
    int r = 0;
    for (; r < a.k_out; ++r) {
        if (__ballot(live) == 0ull) break;                                       // every list exhausted: the rest is filled
        const uint32_t kmin = wave_min_u32(live ? key : 0xFFFFFFFFu);
        bool cand = live && key == kmin;
        unsigned long long m = __ballot(cand);
        if (__popcll(m) > 1) {                                                   // (wave-uniform) equal distances: the lowest global id
            const uint32_t hmin = wave_min_u32(cand ? ghi : 0xFFFFFFFFu);
            cand = cand && ghi == hmin;
            const uint32_t lmin = wave_min_u32(cand ? glo : 0xFFFFFFFFu);
            cand = cand && glo == lmin;
            m = __ballot(cand);                                                  // (the same global id in two lists: the lower list)
        }
        const int w = __ffsll((long long)m) - 1;
        if (lane == w) {
            a.out_ids[q * a.k_out + r] = gid;
            a.out_dist[q * a.k_out + r] = d;
            ++pos;
            load_head();
        }
    }
    for (int j = r + lane; j < a.k_out; j += MERGE_LISTS) {
        a.out_ids[q * a.k_out + j] = -1;
        a.out_dist[q * a.k_out + j] = a.fill == HNSW_FILL_OHNSW ? __uint_as_float(0x7FC00000u) : __uint_as_float(0x7F800000u);
    }
    if (a.nd) {
        const uint32_t s = wave_sum_u32(mine ? a.nd[(int64_t)lane * a.nq + q] : 0u);
        if (lane == 0) a.out_nd[q] = s;
    }
    if (a.nh) {
        const uint32_t s = wave_sum_u32(mine ? a.nh[(int64_t)lane * a.nq + q] : 0u);
        if (lane == 0) a.out_nh[q] = s;
    }
    if (a.stg) {                                                                 // (the maximum: the minimum of the complements)
        const uint32_t s = ~wave_min_u32(mine ? ~a.stg[(int64_t)lane * a.nq + q] : 0xFFFFFFFFu);
        if (lane == 0) a.out_stg[q] = s;
    }
}

// ---- the merge of variable-length sorted segments (the sharded range calls, hnsw_merge_segments) -----------------------------------
// n_lists range results over the same nq queries: list g's segment for query q is the entries [lims_g[q], lims_g[q + 1]) of its ids
// and distances, ascending by distance, no padding.  The lists' arrays lie one behind the other in one table per kind.
//
// Entries of EQUAL distance are expected in ascending id order, and almost always are.  Not always: a single-index range segment is
// ordered by the scan's pre-rounding key, two different keys can round to one float distance (the header's ROUNDING EXCEPTION), and
// then two entries of one distance stand in key order, the higher id first.  The merged order is (distance, global id) on the
// returned floats, so such a pair is put right here: a pre-pass flags every (list, query) whose segment holds such a descent, and
// only for a flagged segment the merge counts inside the run of equal distances entry by entry instead of by binary search.
constexpr int SEG_BLOCK = 256;

struct SegArgs {
    const int64_t *lims;                 // [n_lists][nq + 1]: each list's own prefix sums
    const int32_t *ids;                  // list g's ids from entry base[g] on, id_base-based and local to the list
    const float *dist;                   // ... and its distances
    int64_t nq;
    int32_t n_lists;
    uint8_t *flags;                      // [n_lists][nq], zeroed: 1 = the segment has equal distances with descending ids
    int64_t *out_ids;                    // [sum of the lists' totals]: first_row[list] + id
    float *out_dist;
    int64_t base[MERGE_LISTS], first_row[MERGE_LISTS];
};

// the query of entry e of a list with the prefix sums lg (lg[nq] > e): lg[q] <= e < lg[q + 1]
__device__ __forceinline__ int64_t segment_of(const int64_t *lg, int64_t nq, int64_t e) {
    int64_t lo = 0, hi = nq;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (lg[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// The pre-pass, one thread per entry (grid as the merge's): an entry whose successor has the same distance and a lower id flags its
// (list, query), if the successor belongs to the same query.  Plain stores of one value; the search for the query only at a descent.
__global__ void __launch_bounds__(SEG_BLOCK)
hnsw_merge_segments_flag_kernel(const SegArgs a) {
    const int g = (int)blockIdx.y;
    const int64_t *const lg = a.lims + (int64_t)g * (a.nq + 1);
    const int64_t e = (int64_t)blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (e + 1 >= lg[a.nq]) return;
    const int64_t at = a.base[g] + e;
    if (merge_key(a.dist[at]) != merge_key(a.dist[at + 1]) || a.ids[at] <= a.ids[at + 1]) return;
    const int64_t q = segment_of(lg, a.nq, e);
    if (e + 1 < lg[q + 1]) a.flags[(int64_t)g * a.nq + q] = 1;
}

// A rank merge, one thread per input entry (grid y = the list, grid x over that list's entries: consecutive lanes load consecutive
// ids and distances).  The thread finds its query q by a binary search of its flat index in its list's lims, loads its entry ONCE,
// and its place in q's merged segment is
//     sum over h of lims_h[q]  +  its index in its own segment  +  for every other list h the number of entries of S_h(q) before it,
// where "before" is < under (merge_key(distance), global id as 64 bits) for h > g and <= for h < g: equal global ids in two lists
// keep the lower list first, and the places of all entries of q are a permutation of q's merged segment.  Each count is one binary
// search in S_h(q) (the distance is probed; the id only where the distances are equal).  A flagged S_h(q) -- the own segment
// included -- is counted in two parts instead: the entries of a smaller distance (a binary search on the distance alone, which is
// ascending whatever the ids do), then the run of this distance entry by entry, under (global id, list, index).  No atomics, no
// loop as long as a segment (a run of one distance in a flagged segment is the longest), nothing that depends on the launch
// geometry; empty segments and lists cost two loads of lims.  A place is < lims_out[q + 1] whatever the entries hold (each count is
// at most |S_h(q)|): distances out of order give a wrong order, never a store out of bounds.
__global__ void __launch_bounds__(SEG_BLOCK)
hnsw_merge_segments_kernel(const SegArgs a) {
    const int g = (int)blockIdx.y;
    const int64_t stride = a.nq + 1;
    const int64_t *const lg = a.lims + (int64_t)g * stride;
    const int64_t e = (int64_t)blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (e >= lg[a.nq]) return;
    const int64_t q = segment_of(lg, a.nq, e);
    const float d = a.dist[a.base[g] + e];
    const int64_t gid = a.first_row[g] + a.ids[a.base[g] + e];
    const uint32_t key = merge_key(d);
    int64_t pos = 0;
    for (int h = 0; h < a.n_lists; ++h) {
        const int64_t *const lh = a.lims + (int64_t)h * stride;
        const int64_t b = lh[q], t = lh[q + 1];
        pos += b;
        if (b == t) continue;
        const bool flagged = a.flags[(int64_t)h * a.nq + q] != 0;
        if (h == g && !flagged) { pos += e - b; continue; }
        const float *const dh = a.dist + a.base[h];
        const int32_t *const ih = a.ids + a.base[h];
        const int64_t first = a.first_row[h];
        int64_t x = b, y = t;                                    // the entries of [b, x) are before this one, those of [y, t) are not
        if (!flagged) {
            while (x < y) {
                const int64_t mid = x + ((y - x) >> 1);
                const uint32_t km = merge_key(dh[mid]);
                bool before = km < key;
                if (km == key) {
                    const int64_t gm = first + ih[mid];
                    before = gm < gid || (gm == gid && h < g);
                }
                if (before) x = mid + 1; else y = mid;
            }
            pos += x - b;
            continue;
        }
        while (x < y) {                                          // x: the first entry whose distance is not smaller
            const int64_t mid = x + ((y - x) >> 1);
            if (merge_key(dh[mid]) < key) x = mid + 1; else y = mid;
        }
        pos += x - b;
        for (int64_t j = x; j < t && merge_key(dh[j]) == key; ++j) {
            const int64_t gm = first + ih[j];
            pos += (gm < gid || (gm == gid && (h < g || (h == g && j < e)))) ? 1 : 0;
        }
    }
    a.out_ids[pos] = gid;
    a.out_dist[pos] = d;
}

struct SegSumArgs {
    const int64_t *lims;                 // [n_lists][nq + 1]
    const uint32_t *nd, *nh, *stg;       // [n_lists][nq] the lists' counters, or null (all three): the merged counters read as 0
    int64_t nq;
    int32_t n_lists;
    int64_t *out_lims;                   // [nq + 1]: the sum of the lists' lims, itself a prefix sum
    uint32_t *out_nd, *out_nh, *out_stg; // [nq]: sum, sum, unsigned maximum
};

__global__ void __launch_bounds__(SEG_BLOCK)
hnsw_merge_segments_sum_kernel(const SegSumArgs a) {
    const int64_t q = (int64_t)blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (q > a.nq) return;
    int64_t l = 0;
    uint32_t nd = 0, nh = 0, stg = 0;
    for (int g = 0; g < a.n_lists; ++g) {
        l += a.lims[(int64_t)g * (a.nq + 1) + q];
        if (a.nd && q < a.nq) {
            nd += a.nd[(int64_t)g * a.nq + q];
            nh += a.nh[(int64_t)g * a.nq + q];
            stg = max(stg, a.stg[(int64_t)g * a.nq + q]);
        }
    }
    a.out_lims[q] = l;
    if (q < a.nq) { a.out_nd[q] = nd; a.out_nh[q] = nh; a.out_stg[q] = stg; }
}

} // namespace hnsw_dev

struct hnsw_sharded {
    // the shards.  buf[g]: the whole batch, its [nq][k] results, counters and flag word; done[g]: what the copies to devices[0] wait for
    DeviceGroup grp;
    std::vector<int64_t> lo;             // [G + 1]: shard g holds the rows [lo[g], lo[g + 1])
    // on devices[0]: every shard's results and counters ([G][nq][k], [G][nq]) and the merged rows.  One call in flight per handle.
    DevBuf gIds, gDist, gNd, gNh, mIds, mDist, mNd, mNh;
    // ... the filtered search's stages ([G][nq] and merged), the range calls' concatenated lims ([G][nq + 1])
    DevBuf gSt, mSt, gLims, gFlags;      // (gFlags: the segment merge's pre-pass, [G][nq] bytes)
};

// a mask over the global rows of one hnsw_sharded, cut into one ordinary filter per shard (which it owns)
struct hnsw_sharded_filter {
    const hnsw_sharded *owner = nullptr;
    std::vector<hnsw_filter *> parts;    // [G]
    ~hnsw_sharded_filter() { for (hnsw_filter *f : parts) (void)hnsw_filter_destroy(f); }
};

namespace {

using hnsw_dev::MergeArgs;
using hnsw_dev::MERGE_LISTS;
static_assert(MERGE_LISTS == SEG_LISTS, "a SegPlan holds as many lists as SegArgs");

int launch_merge(const MergeArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(hnsw_dev::hnsw_merge_lists_kernel, dim3((unsigned)a.nq), dim3(MERGE_LISTS), 0, st, a);
    return launched("merge kernel");
}

// shard g's [nq][k] results (and its counters, with_counters) into its slice of the tables on devices[0], on devices[0]'s stream
int copy_shard(hnsw_sharded *s, int g, int64_t nq, int k, bool with_counters) {
    const int d0 = s->grp.devices[0], dg = s->grp.devices[(size_t)g];
    const BatchBufs &b = s->grp.buf[(size_t)g];
    hipStream_t st = s->grp.streams[0];
    const size_t rows = (size_t)nq * k, rbytes = rows * 4, cbytes = (size_t)nq * 4;
    HIP_TRY(hipMemcpyPeerAsync((int32_t *)s->gIds.p + (size_t)g * rows, d0, b.ids.p, dg, rbytes, st));
    HIP_TRY(hipMemcpyPeerAsync((float *)s->gDist.p + (size_t)g * rows, d0, b.dist.p, dg, rbytes, st));
    if (with_counters) {
        HIP_TRY(hipMemcpyPeerAsync((uint32_t *)s->gNd.p + (size_t)g * nq, d0, b.nd.p, dg, cbytes, st));
        HIP_TRY(hipMemcpyPeerAsync((uint32_t *)s->gNh.p + (size_t)g * nq, d0, b.nh.p, dg, cbytes, st));
    }
    return HNSW_OK;
}

// the tables of one k-NN call on devices[0] (the current device): every shard's rows and counters, the merged rows and counters
int ensure_merge_tables(hnsw_sharded *s, int64_t nq, int k) {
    const size_t G = s->grp.size(), rows = (size_t)nq * k;
    int rc;
    if ((rc = s->gIds.ensure(G * rows * 4)) || (rc = s->gDist.ensure(G * rows * 4)) || (rc = s->gNd.ensure(G * nq * 4)) ||
        (rc = s->gNh.ensure(G * nq * 4)) || (rc = s->gSt.ensure(G * nq * 4)) || (rc = s->mIds.ensure(rows * 8)) || (rc = s->mDist.ensure(rows * 4)) ||
        (rc = s->mNd.ensure((size_t)nq * 4)) || (rc = s->mNh.ensure((size_t)nq * 4)) || (rc = s->mSt.ensure((size_t)nq * 4)))
        return rc;
    return HNSW_OK;
}

// ... of one range call: every shard's lims and counters ([G][nq + 1], [G][nq]) and the `entries` ids and distances of all shards
int ensure_range_tables(hnsw_sharded *s, int64_t nq, int64_t entries) {
    const size_t G = s->grp.size(), ebytes = (size_t)std::max<int64_t>(entries, 1) * 4, cbytes = std::max<size_t>(G * (size_t)nq * 4, 4);
    int rc;
    if ((rc = s->gLims.ensure(G * (size_t)(nq + 1) * 8)) || (rc = s->gIds.ensure(ebytes)) || (rc = s->gDist.ensure(ebytes)) ||
        (rc = s->gNd.ensure(cbytes)) || (rc = s->gNh.ensure(cbytes)) || (rc = s->gSt.ensure(cbytes)))
        return rc;
    return HNSW_OK;
}

// The end of every sharded k-NN call: the shards' rows lie in the tables on devices[0] (or are queued there on streams[0]); the
// merge kernel, ONE download into the caller's arrays, the wait.  with_stage: the third counter table, reduced with max.
int merge_and_download(hnsw_sharded *s, int64_t nq, int k, int32_t fill, bool with_counters, bool with_stage, int64_t *out_ids, float *out_dist,
                       uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_st) {
    const int G = (int)s->grp.size();
    const size_t rows = (size_t)nq * k;
    HIP_TRY(hipSetDevice(s->grp.devices[0]));
    hipStream_t st = s->grp.streams[0];
    MergeArgs a{(const int32_t *)s->gIds.p, (const float *)s->gDist.p, with_counters ? (const uint32_t *)s->gNd.p : nullptr,
                with_counters ? (const uint32_t *)s->gNh.p : nullptr, with_stage ? (const uint32_t *)s->gSt.p : nullptr, nq, G, k, k,
                s->grp[0]->iv.id_base, fill, (int64_t *)s->mIds.p, (float *)s->mDist.p, (uint32_t *)s->mNd.p, (uint32_t *)s->mNh.p,
                (uint32_t *)s->mSt.p, {}};
    for (int g = 0; g < G; ++g) a.first_row[g] = s->lo[(size_t)g];
    const int rc = launch_merge(a, st);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(out_ids, s->mIds.p, rows * 8, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(out_dist, s->mDist.p, rows * 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess && with_counters && out_nd) e = hipMemcpyAsync(out_nd, s->mNd.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess && with_counters && out_nh) e = hipMemcpyAsync(out_nh, s->mNh.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess && with_stage && out_st) e = hipMemcpyAsync(out_st, s->mSt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "result download");
    if (es != hipSuccess) return hip_fail(es, "sharded search");
    return HNSW_OK;
}

// Every shard answers the whole batch on its own device and stream (`search`: what is queued on shard g's stream behind the
// upload), the answers go to devices[0] behind an event, after the one host round trip `repair` re-does a flagged shard, then the
// merge and the download.  Both sharded entry points.
template <class Search, class Repair>
int search_and_merge(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, int k, int32_t fill, bool with_counters,
                     int64_t *out_ids, float *out_dist, uint32_t *out_nd, uint32_t *out_nh, Search &&search, Repair &&repair) {
    const int G = (int)s->grp.size();
    const int d = s->grp[0]->iv.d;
    const size_t qbytes = query_bytes(nq, q_stride, d);
    int rc;
    // ---- every allocation first: nothing below returns with work queued that it does not wait for ----
    if ((rc = s->grp.ensure_streams())) return rc;
    for (int g = 0; g < G; ++g) {
        HIP_TRY(hipSetDevice(s->grp.devices[(size_t)g]));
        if ((rc = s->grp.buf[(size_t)g].ensure(nq, qbytes, k))) return rc;
    }
    HIP_TRY(hipSetDevice(s->grp.devices[0]));
    if ((rc = ensure_merge_tables(s, nq, k))) return rc;
    auto queued = [&]() -> int {
        for (int g = 0; g < G; ++g) {
            const BatchBufs &b = s->grp.buf[(size_t)g];
            hipStream_t st = s->grp.streams[(size_t)g];
            HIP_TRY(hipSetDevice(s->grp.devices[(size_t)g]));
            s->grp.hFlags[g] = 0;
            const KnnBatch batch = b.batch(nq, q_stride, k);
            HIP_TRY(hipMemsetAsync(batch.any_flag, 0, 4, st));
            HIP_TRY(hipMemcpyAsync(b.q.p, queries, qbytes, hipMemcpyHostToDevice, st));
            // COSINE: the device's uploaded copy becomes N(Q) in place, once, for the search and for a repair after it
            int r = is_cosine(s->grp[(size_t)g]) ? cosine_normalise(batch.Q, nq, d, q_stride, (float *)b.q.p, q_stride, nullptr, nullptr, st) : HNSW_OK;
            if (!r) r = search(s->grp[(size_t)g], batch, st);
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(&s->grp.hFlags[g], batch.any_flag, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(s->grp.done[(size_t)g], st));
        }
        // the copies run on devices[0]'s stream, each behind its shard's search
        HIP_TRY(hipSetDevice(s->grp.devices[0]));
        for (int g = 0; g < G; ++g) {
            hipEvent_t ev = s->grp.done[(size_t)g];
            HIP_TRY(hipStreamWaitEvent(s->grp.streams[0], ev, 0));
            int r = copy_shard(s, g, nq, k, with_counters);
            if (r) return r;
        }
        return HNSW_OK;
    };
    rc = queued();
    const int rs = s->grp.sync_all();             // the one host round trip (also after a failure: nothing stays queued)
    if (rc || (rc = rs)) return rc;
    for (int g = 0; g < G; ++g) {
        if (!(s->grp.hFlags[g] & 1u)) continue;
        // (rare) the shard's launch flagged a tie overflow: its flagged queries are searched again, complete on return, and the
        // shard's rows are sent once more
        HIP_TRY(hipSetDevice(s->grp.devices[(size_t)g]));
        if ((rc = repair(s->grp[(size_t)g], s->grp.buf[(size_t)g].batch(nq, q_stride, k)))) return rc;
        HIP_TRY(hipSetDevice(s->grp.devices[0]));
        if ((rc = copy_shard(s, g, nq, k, with_counters))) { (void)s->grp.sync_all(); return rc; }
    }
    return merge_and_download(s, nq, k, fill, with_counters, false, out_ids, out_dist, out_nd, out_nh, nullptr);
}

int check_shard_count(int32_t n_shards) {
    if (n_shards < 1 || n_shards > MERGE_LISTS) return fail(HNSW_ERR_BAD_ARG, "n_shards=%d must be in 1..64", n_shards);
    return HNSW_OK;
}

// idx becomes the next shard of s (which owns it from here on): every shard agrees with the first on d, metric and id_base
int adopt_shard(hnsw_sharded *s, hnsw_index *idx, int device) {
    (void)s->grp.adopt(idx, device);     // never grown, shrunk or marked on its own: every later shard's first_row would move
    s->lo.push_back(s->lo.back() + idx->iv.n);
    const hnsw_index *first = s->grp[0];
    if (idx->iv.d != first->iv.d || idx->info.metric != first->info.metric || idx->iv.id_base != first->iv.id_base)
        return fail(HNSW_ERR_BAD_ARG, "shard %d (d=%d metric=%d id_base=%d) does not agree with shard 0 (d=%d metric=%d id_base=%d)",
                    (int)s->grp.size() - 1, idx->iv.d, idx->info.metric, idx->iv.id_base, first->iv.d, first->info.metric, first->iv.id_base);
    return HNSW_OK;
}

// make(g, &idx) creates shard g; on any error every shard made so far is destroyed and *out stays NULL
template <class Make> int make_shards(const int32_t *devices, int32_t n_shards, hnsw_sharded **out, Make &&make) {
    hnsw_sharded *s = new hnsw_sharded();
    s->lo.push_back(0);
    for (int g = 0; g < n_shards; ++g) {
        hnsw_index *idx = nullptr;
        int rc = make(g, &idx);
        if (!rc) rc = adopt_shard(s, idx, devices[g]);
        if (rc) { (void)hnsw_sharded_destroy(s); return rc; }   // (the message of the failing call stays)
    }
    *out = s;
    return HNSW_OK;
}

// ---- the calls that are host-driven ladders on a single index: filtered k-NN and the range calls ----------------------------------
constexpr int SHARD_THREADS = 16;        // host threads that drive shard calls at a time

// call(g) for every shard, each on a host thread whose current device is the shard's: at most SHARD_THREADS threads, which take the
// shards in order off one counter; all are joined before this returns.  The single-index calls they make are complete on return
// and touch only their own handle (its scratch, its stream; the library's one process-wide table, the registered host ranges, is
// behind a mutex).  The error message is thread-local: a failing shard's is taken on its thread, and the lowest-numbered failing
// shard's code and message become this thread's.  One shard, or no thread to be had: on the calling thread, in order.
template <class Call> int on_shards(hnsw_sharded *s, Call &&call) {
    const int G = (int)s->grp.size();
    std::vector<int> rc((size_t)G, HNSW_OK);
    std::vector<std::string> msg((size_t)G);
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int g; (g = next.fetch_add(1)) < G;) {
            const hipError_t e = hipSetDevice(s->grp.devices[(size_t)g]);
            rc[(size_t)g] = e == hipSuccess ? call(g) : hip_fail(e, "hipSetDevice");
            if (rc[(size_t)g]) msg[(size_t)g] = hnsw_last_error();
        }
    };
    std::vector<std::thread> threads;
    if (G > 1) {
        try {
            for (int t = 0; t < std::min(G, SHARD_THREADS); ++t) threads.emplace_back(work);
        } catch (const std::system_error &) {}       // (the threads that did start take every shard)
    }
    if (threads.empty()) work();
    for (std::thread &t : threads) t.join();
    for (int g = 0; g < G; ++g)
        if (rc[(size_t)g]) return fail(rc[(size_t)g], "%s", msg[(size_t)g].c_str());
    return HNSW_OK;
}

// what both k-NN entry points check first, in this order: the handle, the batch against shard 0 (check_batch), the semantics, the
// params against every later shard (an empty shard refuses what shard 0 let through)
int check_sharded_knn(const hnsw_sharded *s, const hnsw_search_params *params, int64_t nq, int64_t q_stride, bool buffers) {
    if (!s || s->grp.members.empty()) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    int rc = check_batch(s->grp[0], params, nq, q_stride, buffers);
    if (rc) return rc;
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "HNSW_SEM_FUNCTOR_NEAREST_K: the k farthest of W have no merged meaning over shards");
    for (size_t g = 1; g < s->grp.size(); ++g) if ((rc = check_params(s->grp[g], params))) return rc;
    return HNSW_OK;
}

int check_sharded_filter(const hnsw_sharded *s, const hnsw_sharded_filter *f) {
    if (!f) return fail(HNSW_ERR_BAD_ARG, "null sharded filter");
    if (f->owner != s || f->parts.size() != s->grp.size()) return fail(HNSW_ERR_BAD_ARG, "the filter was made for another hnsw_sharded");
    return HNSW_OK;
}

struct RangeResultDeleter { void operator()(hnsw_range_result *r) const { (void)hnsw_range_result_destroy(r); } };
using RangeResultPtr = std::unique_ptr<hnsw_range_result, RangeResultDeleter>;

// the two refusals of a SegPlan, in the words of the callers
int seg_list_too_long(int g, int64_t entries) {
    return fail(HNSW_ERR_UNSUPPORTED, "list %d has %lld entries: more than 2^31 - 1", g, (long long)entries);
}
int seg_sum_too_long(const SegPlan &p) {
    return fail(HNSW_ERR_UNSUPPORTED, "%lld merged results: more than 2^31 - 1 in one call", (long long)p.sum);
}

// The merge of p's lists (closed: the sum fits) over nq queries, which lie on `device` (current) in one table per kind -- lims
// [n_lists][nq + 1], list g's ids and distances from entry p.base[g] on -- queued on st and waited for: r's buffers are allocated
// here.  nd / nh / stg: the lists' counters ([n_lists][nq], device), or all null.  flags: scratch for the pre-pass ([n_lists][nq] bytes).
int merge_segments_on_device(int device, hipStream_t st, const SegPlan &p, int64_t nq, const int64_t *lims, const int32_t *ids, const float *dist,
                             const uint32_t *nd, const uint32_t *nh, const uint32_t *stg, DevBuf &flags, hnsw_sharded_range_result *r) {
    hnsw_dev::SegArgs a{};
    a.lims = lims; a.ids = ids; a.dist = dist;
    a.nq = nq;
    a.n_lists = p.n_lists;
    std::copy(p.base, p.base + p.n_lists, a.base);
    std::copy(p.first_row, p.first_row + p.n_lists, a.first_row);
    const int64_t total = p.sum, longest = p.longest;
    r->device = device;
    r->nq = a.nq;
    r->total = total;
    const size_t cnt = (size_t)std::max<int64_t>(a.nq, 1) * 4;
    int rc;
    if ((rc = r->lims.ensure((size_t)(a.nq + 1) * 8)) || (rc = r->ids.ensure((size_t)std::max<int64_t>(total, 1) * 8)) ||
        (rc = r->dist.ensure((size_t)std::max<int64_t>(total, 1) * 4)) || (rc = r->nd.ensure(cnt)) || (rc = r->nh.ensure(cnt)) || (rc = r->stage.ensure(cnt)))
        return rc;
    const hnsw_dev::SegSumArgs sa{a.lims, nd, nh, stg, a.nq, a.n_lists, (int64_t *)r->lims.p, (uint32_t *)r->nd.p, (uint32_t *)r->nh.p, (uint32_t *)r->stage.p};
    hipLaunchKernelGGL(hnsw_dev::hnsw_merge_segments_sum_kernel, dim3((unsigned)((a.nq + 1 + hnsw_dev::SEG_BLOCK - 1) / hnsw_dev::SEG_BLOCK)),
                       dim3(hnsw_dev::SEG_BLOCK), 0, st, sa);
    rc = launched("segment sum kernel");
    if (!rc && longest > 0) {
        const size_t fbytes = (size_t)a.n_lists * (size_t)a.nq;
        if ((rc = flags.ensure(fbytes))) { (void)hipStreamSynchronize(st); return rc; }
        a.flags = (uint8_t *)flags.p;
        a.out_ids = (int64_t *)r->ids.p;
        a.out_dist = (float *)r->dist.p;
        const dim3 grid((unsigned)((longest + hnsw_dev::SEG_BLOCK - 1) / hnsw_dev::SEG_BLOCK), (unsigned)a.n_lists);
        if (hipMemsetAsync(flags.p, 0, fbytes, st) != hipSuccess) rc = fail(HNSW_ERR_HIP, "memset failed");
        if (!rc) {
            hipLaunchKernelGGL(hnsw_dev::hnsw_merge_segments_flag_kernel, grid, dim3(hnsw_dev::SEG_BLOCK), 0, st, a);
            rc = launched("segment flag kernel");
        }
        if (!rc) {
            hipLaunchKernelGGL(hnsw_dev::hnsw_merge_segments_kernel, grid, dim3(hnsw_dev::SEG_BLOCK), 0, st, a);
            rc = launched("segment merge kernel");
        }
    }
    const int rs = synced(st, "segment merge");
    return rc ? rc : rs;
}

// Both sharded range calls once s, f and out are checked: `call` makes shard g's single-index call (complete on return, its result on
// the shard's device); the results go to devices[0] by peer copies on streams[0], one table per kind, and are merged there.
template <class Call> int sharded_range(hnsw_sharded *s, int64_t nq, hnsw_sharded_range_result **out, Call &&call) {
    const int G = (int)s->grp.size();
    std::vector<RangeResultPtr> part((size_t)G);
    int rc = on_shards(s, [&](int g) {
        hnsw_range_result *r = nullptr;
        const int c = call(g, &r);
        part[(size_t)g].reset(r);
        return c;
    });
    if (rc) return rc;                   // (the shard results are destroyed with `part`)
    SegPlan plan;
    for (int g = 0; g < G; ++g)          // (a single-index result never has more than 2^31 - 1 entries)
        if (plan.add(part[(size_t)g]->total, s->lo[(size_t)g])) return seg_list_too_long(g, part[(size_t)g]->total);
    if (plan.close()) return seg_sum_too_long(plan);
    if ((rc = s->grp.ensure_streams())) return rc;
    const int d0 = s->grp.devices[0];
    HIP_TRY(hipSetDevice(d0));
    hipStream_t st = s->grp.streams[0];
    const size_t lbytes = (size_t)(nq + 1) * 8, cbytes = (size_t)nq * 4;
    if ((rc = ensure_range_tables(s, nq, plan.sum))) return rc;
    auto copies = [&]() -> int {
        for (int g = 0; g < G; ++g) {
            const hnsw_range_result &p = *part[(size_t)g];
            const size_t ebytes = (size_t)p.total * 4;
            HIP_TRY(hipMemcpyPeerAsync((char *)s->gLims.p + (size_t)g * lbytes, d0, p.lims.p, p.device, lbytes, st));
            if (ebytes) {
                HIP_TRY(hipMemcpyPeerAsync((int32_t *)s->gIds.p + plan.base[g], d0, p.ids.p, p.device, ebytes, st));
                HIP_TRY(hipMemcpyPeerAsync((float *)s->gDist.p + plan.base[g], d0, p.dist.p, p.device, ebytes, st));
            }
            if (cbytes) {
                HIP_TRY(hipMemcpyPeerAsync((char *)s->gNd.p + (size_t)g * cbytes, d0, p.nd.p, p.device, cbytes, st));
                HIP_TRY(hipMemcpyPeerAsync((char *)s->gNh.p + (size_t)g * cbytes, d0, p.nh.p, p.device, cbytes, st));
                HIP_TRY(hipMemcpyPeerAsync((char *)s->gSt.p + (size_t)g * cbytes, d0, p.stage.p, p.device, cbytes, st));
            }
        }
        return HNSW_OK;
    };
    if ((rc = copies())) { (void)hipStreamSynchronize(st); return rc; }     // (nothing stays queued that reads a shard result)
    std::unique_ptr<hnsw_sharded_range_result> r(new hnsw_sharded_range_result());
    rc = merge_segments_on_device(d0, st, plan, nq, (const int64_t *)s->gLims.p, (const int32_t *)s->gIds.p, (const float *)s->gDist.p,
                                  nq ? (const uint32_t *)s->gNd.p : nullptr, (const uint32_t *)s->gNh.p, (const uint32_t *)s->gSt.p, s->gFlags, r.get());
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    *out = r.release();
    return HNSW_OK;
}

} // namespace

extern "C" {

int32_t hnsw_sharded_build(const float *vectors, int64_t n, int32_t d, int64_t row_stride, const hnsw_build_params *params,
                           const int32_t *devices, int32_t n_shards, hnsw_sharded **out) {
    if (out) *out = nullptr;
    if (!vectors || !params || !devices || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    int rc = check_shard_count(n_shards);
    if (rc) return rc;
    if (n < n_shards) return fail(HNSW_ERR_BAD_ARG, "n=%lld < n_shards=%d: a shard would be empty", (long long)n, n_shards);
    auto lo = [&](int g) { return shard_lo(n, g, n_shards); };
    return make_shards(devices, n_shards, out, [&](int g, hnsw_index **idx) {
        hnsw_build_params p = *params;
        p.seed = params->seed + (uint64_t)g;
        return hnsw_build(vectors + lo(g) * row_stride, lo(g + 1) - lo(g), d, row_stride, &p, devices[g], idx);
    });
}

int32_t hnsw_sharded_create(const hnsw_index_desc *const *descs, const int32_t *devices, int32_t n_shards, hnsw_sharded **out) {
    if (out) *out = nullptr;
    if (!descs || !devices || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    int rc = check_shard_count(n_shards);
    if (rc) return rc;
    for (int g = 0; g < n_shards; ++g) if (!descs[g]) return fail(HNSW_ERR_BAD_ARG, "descs[%d] is null", g);
    return make_shards(devices, n_shards, out, [&](int g, hnsw_index **idx) { return hnsw_index_create(descs[g], devices[g], idx); });
}

int32_t hnsw_sharded_load(const char *const *paths, const int32_t *devices, int32_t n_shards, hnsw_sharded **out) {
    if (out) *out = nullptr;
    if (!paths || !devices || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    int rc = check_shard_count(n_shards);
    if (rc) return rc;
    for (int g = 0; g < n_shards; ++g) if (!paths[g]) return fail(HNSW_ERR_BAD_ARG, "paths[%d] is null", g);
    return make_shards(devices, n_shards, out, [&](int g, hnsw_index **idx) { return hnsw_index_load(paths[g], devices[g], idx); });
}

int32_t hnsw_sharded_destroy(hnsw_sharded *s) {
    if (!s) return HNSW_OK;
    (void)s->grp.sync_all();
    s->grp.release();
    delete s;
    return HNSW_OK;
}

int32_t hnsw_sharded_num_shards(const hnsw_sharded *s, int32_t *n_shards) {
    if (!s || !n_shards) return fail(HNSW_ERR_BAD_ARG, "null argument");
    *n_shards = (int32_t)s->grp.size();
    return HNSW_OK;
}

int32_t hnsw_sharded_shard(hnsw_sharded *s, int32_t g, hnsw_index **out, int64_t *first_row) {
    if (!s || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (g < 0 || g >= (int32_t)s->grp.size()) return fail(HNSW_ERR_BAD_ARG, "shard %d out of range", g);
    *out = s->grp[(size_t)g];
    if (first_row) *first_row = s->lo[(size_t)g];
    return HNSW_OK;
}

int32_t hnsw_sharded_get_info(const hnsw_sharded *s, int64_t *n, int32_t *d, int32_t *metric, int32_t *id_base, int64_t *device_bytes) {
    if (!s) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    int64_t bytes = 0;
    for (const IndexPtr &idx : s->grp.members) {
        hnsw_index_info info;
        const int rc = hnsw_index_get_info(idx.get(), &info);
        if (rc) return rc;
        bytes += info.device_bytes;
    }
    if (n) *n = s->lo.back();
    if (d) *d = s->grp[0]->iv.d;
    if (metric) *metric = s->grp[0]->info.metric;
    if (id_base) *id_base = s->grp[0]->iv.id_base;
    if (device_bytes) *device_bytes = bytes;
    return HNSW_OK;
}

int32_t hnsw_sharded_set_option(hnsw_sharded *s, const char *name, int64_t value) {
    if (!s || !name) return fail(HNSW_ERR_BAD_ARG, "null argument");
    std::vector<int64_t> before(s->grp.size(), 0);
    for (size_t g = 0; g < s->grp.size(); ++g) {
        int rc = get_option(s->grp[g], name, &before[g]);
        if (!rc) rc = hnsw_index_set_option(s->grp[g], name, value);
        if (rc) {
            const std::string msg = hnsw_last_error();          // shard g's refusal is what the caller reads
            for (size_t h = 0; h < g; ++h) (void)hnsw_index_set_option(s->grp[h], name, before[h]);
            return fail(rc, "%s", msg.c_str());
        }
    }
    return HNSW_OK;
}

int32_t hnsw_sharded_search_batch(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params,
                                  int64_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops) {
    const int rc = check_sharded_knn(s, params, nq, q_stride, queries && out_ids && out_dist);
    if (rc || nq == 0) return rc;
    return search_and_merge(
        s, queries, nq, q_stride, params->k, params->fill, true, out_ids, out_dist, out_ndist, out_nhops,
        [&](hnsw_index *idx, const KnnBatch &b, hipStream_t st) { return knn_search(idx, params, b, st); },
        [&](hnsw_index *idx, const KnnBatch &b) { return knn_repair(idx, params, b, nullptr); });
}

int32_t hnsw_sharded_brute_force_batch(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                                       int64_t *out_ids, float *out_dist) {
    if (!s || s->grp.members.empty()) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    const int rc = check_scan(s->grp[0], nq, q_stride, k, fill, queries && out_ids && out_dist);
    if (rc || nq == 0) return rc;
    return search_and_merge(
        s, queries, nq, q_stride, k, fill, false, out_ids, out_dist, nullptr, nullptr,
        [&](hnsw_index *idx, const KnnBatch &b, hipStream_t st) { return scan_search(idx, b, k, fill, st); },
        [](hnsw_index *, const KnnBatch &) { return (int)HNSW_OK; });            // (the scan flags nothing)
}

int32_t hnsw_merge_lists(int32_t device, const int32_t *ids, const float *dist, const int64_t *first_row, int32_t n_lists, int64_t nq,
                         int32_t k_in, int32_t k_out, int32_t id_base, int32_t fill, int64_t *out_ids, float *out_dist) {
    if (n_lists < 1 || n_lists > MERGE_LISTS) return fail(HNSW_ERR_BAD_ARG, "n_lists=%d must be in 1..64", n_lists);
    if (k_in < 1 || k_in > 1024 || k_out < 1 || k_out > 1024)
        return fail(HNSW_ERR_BAD_ARG, "k_in=%d and k_out=%d must be in 1..1024", k_in, k_out);
    if (fill != HNSW_FILL_OHNSW && fill != HNSW_FILL_BA) return fail(HNSW_ERR_BAD_ARG, "bad fill %d", fill);
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    if (nq == 0) return HNSW_OK;
    if (!ids || !dist || !first_row || !out_ids || !out_dist) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    for (int g = 1; g < n_lists; ++g)
        if (first_row[g] < first_row[g - 1]) return fail(HNSW_ERR_BAD_ARG, "first_row must be non-decreasing (list %d)", g);
    HIP_TRY(hipSetDevice(device));
    const size_t in = (size_t)n_lists * nq * k_in * 4, rows = (size_t)nq * k_out;
    DevBuf dIds, dDist, oIds, oDist;
    int rc;
    if ((rc = dIds.ensure(in)) || (rc = dDist.ensure(in)) || (rc = oIds.ensure(rows * 8)) || (rc = oDist.ensure(rows * 4))) return rc;
    HIP_TRY(hipMemcpy(dIds.p, ids, in, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dDist.p, dist, in, hipMemcpyHostToDevice));
    MergeArgs a{(const int32_t *)dIds.p, (const float *)dDist.p, nullptr, nullptr, nullptr, nq, n_lists, k_in, k_out, id_base, fill,
                (int64_t *)oIds.p, (float *)oDist.p, nullptr, nullptr, nullptr, {}};
    for (int g = 0; g < n_lists; ++g) a.first_row[g] = first_row[g];
    if ((rc = launch_merge(a, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out_ids, oIds.p, rows * 8, hipMemcpyDeviceToHost));       // (the null stream: behind the kernel)
    HIP_TRY(hipMemcpy(out_dist, oDist.p, rows * 4, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

// ---- sharded filter, filtered k-NN, range search ------------------------------------------------------------------------------------

int32_t hnsw_sharded_filter_create(hnsw_sharded *s, const uint32_t *bits, int64_t n_bits, hnsw_sharded_filter **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (!s || s->grp.members.empty()) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    if (n_bits != s->lo.back())
        return fail(HNSW_ERR_BAD_ARG, "the filter has %lld bits, the sharded index %lld rows", (long long)n_bits, (long long)s->lo.back());
    if (n_bits > 0 && !bits) return fail(HNSW_ERR_BAD_ARG, "null bits");
    std::unique_ptr<hnsw_sharded_filter> f(new hnsw_sharded_filter());      // (owns the parts made so far: any return frees them)
    f->owner = s;
    std::vector<uint32_t> part;
    for (size_t g = 0; g < s->grp.size(); ++g) {
        const int64_t lo = s->lo[g], n = s->lo[g + 1] - lo;      // shard g's bits [lo_g, lo_{g+1}) moved down to bit 0
        part.resize((size_t)std::max<int64_t>((n + 31) / 32, 1));
        cut_mask(bits, n_bits, lo, n, part.data());
        hnsw_filter *pf = nullptr;
        const int rc = hnsw_filter_create(s->grp[g], part.data(), n, &pf);
        if (rc) return rc;
        f->parts.push_back(pf);
    }
    *out = f.release();
    return HNSW_OK;
}

int32_t hnsw_sharded_filter_destroy(hnsw_sharded_filter *f) {
    delete f;
    return HNSW_OK;
}

int32_t hnsw_sharded_filter_count(const hnsw_sharded_filter *f, int64_t *n_allowed) {
    if (!f || !n_allowed) return fail(HNSW_ERR_BAD_ARG, "null sharded filter or null n_allowed");
    int64_t c = 0;
    for (const hnsw_filter *p : f->parts) c += p->n_allowed;
    *n_allowed = c;
    return HNSW_OK;
}

int32_t hnsw_sharded_filter_part(const hnsw_sharded_filter *f, int32_t g, const hnsw_filter **out) {
    if (!f || !out) return fail(HNSW_ERR_BAD_ARG, "null sharded filter or null out");
    if (g < 0 || g >= (int32_t)f->parts.size()) return fail(HNSW_ERR_BAD_ARG, "shard %d out of range", g);
    *out = f->parts[(size_t)g];
    return HNSW_OK;
}

int32_t hnsw_sharded_search_batch_filtered(hnsw_sharded *s, const hnsw_sharded_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                           const hnsw_search_params *params, int64_t *out_ids, float *out_dist, uint32_t *out_ndist,
                                           uint32_t *out_nhops, uint32_t *out_stage) {
    int rc = check_sharded_knn(s, params, nq, q_stride, queries && out_ids && out_dist);
    if (rc || (rc = check_sharded_filter(s, f))) return rc;
    if (nq == 0) return HNSW_OK;
    // The single-index call is a host-driven ladder that answers into host arrays: every shard's rows and counters pass through
    // these, then go to the tables on devices[0] in one copy per table
    const size_t G = s->grp.size(), k = (size_t)params->k, rows = (size_t)nq * k;
    std::vector<int32_t> ids(G * rows);
    std::vector<float> dist(G * rows);
    std::vector<uint32_t> cnt(3 * G * (size_t)nq);
    uint32_t *const nd = cnt.data(), *const nh = nd + G * (size_t)nq, *const stg = nh + G * (size_t)nq;
    rc = on_shards(s, [&](int g) {
        const size_t z = (size_t)g;
        return (int)hnsw_search_batch_filtered(s->grp[z], f->parts[z], queries, nq, q_stride, params, ids.data() + z * rows, dist.data() + z * rows,
                                               nd + z * (size_t)nq, nh + z * (size_t)nq, stg + z * (size_t)nq);
    });
    if (rc || (rc = s->grp.ensure_streams())) return rc;
    HIP_TRY(hipSetDevice(s->grp.devices[0]));
    if ((rc = ensure_merge_tables(s, nq, (int)k))) return rc;
    hipStream_t st = s->grp.streams[0];
    hipError_t e = hipMemcpyAsync(s->gIds.p, ids.data(), G * rows * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->gDist.p, dist.data(), G * rows * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->gNd.p, nd, G * (size_t)nq * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->gNh.p, nh, G * (size_t)nq * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->gSt.p, stg, G * (size_t)nq * 4, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return hip_fail(e, "shard rows upload"); }
    return merge_and_download(s, nq, (int)k, params->fill, true, true, out_ids, out_dist, out_ndist, out_nhops, out_stage);
}

int32_t hnsw_sharded_range_search_batch(hnsw_sharded *s, const hnsw_sharded_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                        const hnsw_range_params *params, hnsw_sharded_range_result **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (!s || s->grp.members.empty()) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    int rc;
    if (f && (rc = check_sharded_filter(s, f))) return rc;
    return sharded_range(s, nq, out, [&](int g, hnsw_range_result **r) {
        hnsw_index *idx = s->grp[(size_t)g];
        return (int)(f ? hnsw_range_search_batch_filtered(idx, f->parts[(size_t)g], queries, nq, q_stride, params, r)
                       : hnsw_range_search_batch(idx, queries, nq, q_stride, params, r));
    });
}

int32_t hnsw_sharded_range_brute_force_batch(hnsw_sharded *s, const hnsw_sharded_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                             float radius, hnsw_sharded_range_result **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (!s || s->grp.members.empty()) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    int rc;
    if (f && (rc = check_sharded_filter(s, f))) return rc;
    return sharded_range(s, nq, out, [&](int g, hnsw_range_result **r) {
        hnsw_index *idx = s->grp[(size_t)g];
        return (int)(f ? hnsw_range_brute_force_batch_filtered(idx, f->parts[(size_t)g], queries, nq, q_stride, radius, r)
                       : hnsw_range_brute_force_batch(idx, queries, nq, q_stride, radius, r));
    });
}

// the result's functions (the bodies: RangeRecord, hnsw_internal.h)
int32_t hnsw_sharded_range_result_size(const hnsw_sharded_range_result *r, int64_t *nq, int64_t *total) { return RangeRecord<int64_t>::size(r, nq, total); }
int32_t hnsw_sharded_range_result_fetch(hnsw_sharded_range_result *r, int64_t *lims, int64_t *ids, float *dist, uint32_t *out_ndist,
                                        uint32_t *out_nhops, uint32_t *out_stage) {
    return RangeRecord<int64_t>::fetch(r, lims, ids, dist, out_ndist, out_nhops, out_stage);
}
int32_t hnsw_sharded_range_result_device(hnsw_sharded_range_result *r, const int64_t **d_lims, const int64_t **d_ids, const float **d_dist) {
    return RangeRecord<int64_t>::device_pointers(r, d_lims, d_ids, d_dist);
}
int32_t hnsw_sharded_range_result_destroy(hnsw_sharded_range_result *r) { delete r; return HNSW_OK; }

int32_t hnsw_merge_segments(int32_t device, int32_t n_lists, int64_t nq, const int64_t *const *lims, const int32_t *const *ids,
                            const float *const *dist, const int64_t *first_row, int32_t id_base, hnsw_sharded_range_result **out) {
    (void)id_base;                       // (segments carry no padding: nothing to tell from a real id)
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (n_lists < 1 || n_lists > MERGE_LISTS) return fail(HNSW_ERR_BAD_ARG, "n_lists=%d must be in 1..64", n_lists);
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    if (!lims || !first_row) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    SegPlan plan;
    for (int g = 0; g < n_lists; ++g) {
        if (g > 0 && first_row[g] < first_row[g - 1]) return fail(HNSW_ERR_BAD_ARG, "first_row must be non-decreasing (list %d)", g);
        if (!lims[g]) return fail(HNSW_ERR_BAD_ARG, "lims[%d] is null", g);
        int64_t q = 0;
        switch (check_lims(lims[g], nq, &q)) {
        case LIMS_START: return fail(HNSW_ERR_BAD_ARG, "lims[%d] must start at 0", g);
        case LIMS_DECREASE: return fail(HNSW_ERR_BAD_ARG, "lims[%d] must be non-decreasing (query %lld)", g, (long long)q);
        case LIMS_OK: break;
        }
        const int64_t t = lims[g][nq];
        if (t > 0 && (!ids || !dist || !ids[g] || !dist[g])) return fail(HNSW_ERR_BAD_ARG, "list %d has entries and no ids or distances", g);
        if (plan.add(t, first_row[g])) return seg_list_too_long(g, t);
    }
    if (plan.close()) return seg_sum_too_long(plan);
    HIP_TRY(hipSetDevice(device));
    const size_t lbytes = (size_t)(nq + 1) * 8, ebytes = (size_t)std::max<int64_t>(plan.sum, 1) * 4;
    DevBuf dLims, dIds, dDist;
    int rc;
    if ((rc = dLims.ensure((size_t)n_lists * lbytes)) || (rc = dIds.ensure(ebytes)) || (rc = dDist.ensure(ebytes))) return rc;
    for (int g = 0; g < n_lists; ++g) {
        HIP_TRY(hipMemcpy((char *)dLims.p + (size_t)g * lbytes, lims[g], lbytes, hipMemcpyHostToDevice));
        if (plan.total[g] == 0) continue;
        HIP_TRY(hipMemcpy((int32_t *)dIds.p + plan.base[g], ids[g], (size_t)plan.total[g] * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((float *)dDist.p + plan.base[g], dist[g], (size_t)plan.total[g] * 4, hipMemcpyHostToDevice));
    }
    std::unique_ptr<hnsw_sharded_range_result> r(new hnsw_sharded_range_result());
    DevBuf flags;
    if ((rc = merge_segments_on_device(device, nullptr, plan, nq, (const int64_t *)dLims.p, (const int32_t *)dIds.p, (const float *)dDist.p, nullptr, nullptr,
                                       nullptr, flags, r.get())))       // (the null stream: behind the copies)
        return rc;
    *out = r.release();
    return HNSW_OK;
}

} // extern "C"
