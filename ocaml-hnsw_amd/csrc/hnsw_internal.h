// hnsw_internal.h -- shared host-side declarations of libhnsw_mi355x.so (not part of the ABI).
#pragma once
#include "../../include/hnsw_mi355x.h"
#include "hnsw_device.hip.h"
#include "hnsw_scan_plan.h"
#include "hnsw_filter_plan.h"
#include "hnsw_remove_plan.h"
#include "hnsw_mark_plan.h"
#include "hnsw_shard_plan.h"
#include "hnsw_group_plan.h"
#include "hnsw_bits_plan.h"
#include "hnsw_keys_plan.h"
#include "hnsw_by_id_plan.h"
#include "hnsw_upsert_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

struct hnsw_index;

namespace hnsw_host {

// ---- a kernel's compile-time shape from run-time numbers ----------------------------------------------------------------
// NCH = float4 chunks per lane (pick_nch), RB = 4-row batches in flight per wave, NSLOT = key registers per lane that hold W
// (pick_nslot / pick_nslot_knn).  Every launch site goes through with_nch / with_nslot / with_metric, which hand the run-time
// number to a generic lambda as a std::integral_constant, and takes its RB from rows_in_flight.

// RB for d <= 128 (NCH = 2): measured on C2: 4 (6 waves/SIMD) >= 3 (7) >= 2 (8): the batch is memory-bound, not occupancy-bound
constexpr int RB_NCH2 = 4;
// RB by NCH, for float32 rows and for the compact rows (bytes: a quarter of the registers per row; halves: half of them, and
// they take the byte rows' counts: not measured against other counts).  NCH 2 takes RB_NCH2 whatever the row format.
constexpr int rows_in_flight(int nch, bool compact = false) {
    return nch == 1 ? 8 : nch == 2 ? RB_NCH2 : nch == 4 ? (compact ? 4 : 2) : nch == 8 ? (compact ? 2 : 1) : 1;
}
// rows of 65..256 dimensions (NCH 2 and 4: the shapes with hand-scheduled loops) also have the knn kernel's W in three and six
// registers (pick_nslot_knn)
constexpr bool has_odd_nslot(int nch) { return nch == 2 || nch == 4; }

// ... and for the per-dimension codes' L2 walk (ROWS 5, hnsw_rows_sq8_dim.hip): a row in flight is a byte row's registers, but the
// lane also holds NCH float4 of scales beside the query.  The byte rows' counts: with them no instance uses scratch memory
// (DESIGN.md has the register table); NCH 16 holds one batch (its widest instance stands at 256 VGPRs).
constexpr int rows_in_flight_sq8_dim(int nch) { return nch == 1 ? 8 : nch == 2 ? RB_NCH2 : nch == 4 ? 4 : nch == 8 ? 2 : 1; }

// ... and for the walk over the 1-bit codes (ROWS 6, hnsw_rows_bits.hip): a row in flight is NW = 1 or 2 dwords per lane, so the
// limit is ids in flight, not registers: 8 batches, the most eval_round issues, for both widths (DESIGN.md has the register table).
constexpr int rows_in_flight_bits(int /*nw*/) { return 8; }
// (NW = bit_words(d), the 16-word steps of a bit row and the knn kernel's NCH for that format: hnsw_bits_plan.h)

template <int V> using Int = std::integral_constant<int, V>;
// f(Int<NCH>) for the NCH that pick_nch returned
template <class F> auto with_nch(int nch, F &&f) {
    switch (nch) {
    case 1: return f(Int<1>{});
    case 2: return f(Int<2>{});
    case 4: return f(Int<4>{});
    case 8: return f(Int<8>{});
    default: return f(Int<16>{});
    }
}
// f(Int<NSLOT>) for nslot out of the kernel family's own list S0, S...; the last of the list also takes what is not listed
template <int S0, int... S, class F> auto with_nslot(int nslot, F &&f) {
    if constexpr (sizeof...(S) > 0) { if (nslot != S0) return with_nslot<S...>(nslot, f); }
    return f(Int<S0>{});
}
// ... the knn kernel's list for rows of NCH chunks per lane
template <int NCH, class F> auto with_nslot_knn(int nslot, F &&f) {
    if constexpr (has_odd_nslot(NCH)) return with_nslot<1, 2, 3, 4, 6, 8, 16>(nslot, f);
    else return with_nslot<1, 2, 4, 8, 16>(nslot, f);
}
// f(Int<0>) for HNSW_METRIC_L2, f(Int<1>) for the inner product -- and for HNSW_METRIC_COSINE, the inner product over unit rows
template <class F> auto with_metric(int metric, F &&f) { return metric == HNSW_METRIC_L2 ? f(Int<0>{}) : f(Int<1>{}); }

// The knn kernel's variant objects (hnsw_search_variants.hip compiled once per line): X(metric, accept rule, row format -- see
// variant_full).  build.py's VARIANTS is the same list (tests/test_abi_load.py compares them).
#define HNSW_SEARCH_VARIANTS(X) \
    X(0, 0, 0) X(0, 0, 1) X(0, 0, 2) X(0, 0, 3) X(0, 0, 4) \
    X(0, 1, 0) X(0, 1, 1) X(0, 1, 2) X(0, 1, 3) X(0, 1, 4) \
    X(1, 0, 0) X(1, 0, 1) X(1, 0, 2) X(1, 0, 3) X(1, 0, 4) \
    X(1, 1, 0) X(1, 1, 1) X(1, 1, 2) X(1, 1, 3) X(1, 1, 4)
// The collect kernel's variant objects (option "filter_collect"; hnsw_collect_variants.hip compiled once per line), same triples:
// the row formats whose walk distances are exact over X (0 .. 3).  build.py's COLLECT_VARIANTS is the same list.
#define HNSW_COLLECT_VARIANTS(X) \
    X(0, 0, 0) X(0, 0, 1) X(0, 0, 2) X(0, 0, 3) \
    X(0, 1, 0) X(0, 1, 1) X(0, 1, 2) X(0, 1, 3) \
    X(1, 0, 0) X(1, 0, 1) X(1, 0, 2) X(1, 0, 3) \
    X(1, 1, 0) X(1, 1, 1) X(1, 1, 2) X(1, 1, 3)

int fail(int code, const char *fmt, ...);
// the code and message of a failed HIP call
inline int hip_fail(hipError_t e, const char *what) {
    return fail(e == hipErrorOutOfMemory ? HNSW_ERR_OOM : HNSW_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

#define HIP_TRY(expr)                                                       \
    do {                                                                    \
        hipError_t e__ = (expr);                                            \
        if (e__ != hipSuccess) return ::hnsw_host::hip_fail(e__, #expr);    \
    } while (0)

// the answer of the kernel launch just made / of waiting for st
inline int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HNSW_OK : fail(HNSW_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}
inline int synced(hipStream_t st, const char *what) {
    const hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? HNSW_OK : fail(HNSW_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

// ---- owners ---------------------------------------------------------------------------------------------------------------
// Every device allocation, page-locked block, stream and event of the host side is held by one of these move-only types, whose
// destructor frees it (swallowing HIP's answer: a destructor reports nothing and never calls fail()).  A function's scratch is a
// local owner, so any return frees it; the handles' resources are members.  None may have static or thread-local storage: the
// runtime can be gone when such a destructor runs.

// a device allocation and its byte count
struct DevMem {
    void *p = nullptr;
    size_t bytes = 0;
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevMem &operator=(DevMem &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevMem() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};
// ... that grows on demand and is reused (bytes: its capacity)
struct DevBuf : DevMem {
    int ensure(size_t need) {
        if (need <= bytes) return HNSW_OK;
        release();
        HIP_TRY(hipMalloc(&p, need));
        bytes = need;
        return HNSW_OK;
    }
};
// ... of an exact size, such as one device table of an index: bytes is what hnsw_index_info.device_bytes counts for it.  An empty
// table still gets an allocation (16 bytes at least: kernels may be handed its pointer), which is not counted.
struct Table : DevMem {
    hipError_t alloc(size_t b) {
        release();
        const hipError_t e = hipMalloc(&p, std::max<size_t>(b, 16));
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
        bytes = b;
        return hipSuccess;
    }
};
// ... of one word that a checking kernel sets or clears
struct DevFlag : DevMem {
    hipError_t alloc() { release(); return hipMalloc(&p, 16); }
    hipError_t set(int32_t v) { return hipMemcpy(p, &v, 4, hipMemcpyHostToDevice); }
    hipError_t get(int32_t *v) const { return hipMemcpy(v, p, 4, hipMemcpyDeviceToHost); }
};
// a stream, an event or a page-locked block: the handle h and the call that gives it back
template <class T, auto Free> struct Owned {
    T h{};
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = T{}; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) { reset(); h = o.h; o.h = T{}; }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() { if (h) (void)Free(h); h = T{}; }
    operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
template <class T> struct Pinned : Owned<T *, hipHostFree> {
    hipError_t alloc(size_t bytes, unsigned flags) { this->reset(); return hipHostMalloc((void **)&this->h, bytes, flags); }
};

// What a range call returns, on one device: lims [nq + 1], ids and distances [total], the per-query counters [nq].  Id: int32 ids
// local to one index (hnsw_range_result), int64 global ids (hnsw_sharded_range_result); those two derive from it and stay distinct
// ABI types, whose _size / _fetch / _device functions are the three below (r null: HNSW_ERR_BAD_ARG).
template <class Id> struct RangeRecord {
    int device = -1;
    int64_t nq = 0, total = 0;
    DevBuf lims, ids, dist, nd, nh, stage;
    static int size(const RangeRecord *r, int64_t *nq, int64_t *total) {
        if (!r) return fail(HNSW_ERR_BAD_ARG, "null result");
        if (nq) *nq = r->nq;
        if (total) *total = r->total;
        return HNSW_OK;
    }
    static int fetch(const RangeRecord *r, int64_t *lims, Id *ids, float *dist, uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage) {
        if (!r) return fail(HNSW_ERR_BAD_ARG, "null result");
        if (!lims && !ids && !dist && !out_ndist && !out_nhops && !out_stage) return HNSW_OK;
        HIP_TRY(hipSetDevice(r->device));
        if (lims) HIP_TRY(hipMemcpy(lims, r->lims.p, (size_t)(r->nq + 1) * 8, hipMemcpyDeviceToHost));
        if (ids && r->total > 0) HIP_TRY(hipMemcpy(ids, r->ids.p, (size_t)r->total * sizeof(Id), hipMemcpyDeviceToHost));
        if (dist && r->total > 0) HIP_TRY(hipMemcpy(dist, r->dist.p, (size_t)r->total * 4, hipMemcpyDeviceToHost));
        if (r->nq > 0) {
            if (out_ndist) HIP_TRY(hipMemcpy(out_ndist, r->nd.p, (size_t)r->nq * 4, hipMemcpyDeviceToHost));
            if (out_nhops) HIP_TRY(hipMemcpy(out_nhops, r->nh.p, (size_t)r->nq * 4, hipMemcpyDeviceToHost));
            if (out_stage) HIP_TRY(hipMemcpy(out_stage, r->stage.p, (size_t)r->nq * 4, hipMemcpyDeviceToHost));
        }
        return HNSW_OK;
    }
    static int device_pointers(const RangeRecord *r, const int64_t **d_lims, const Id **d_ids, const float **d_dist) {
        if (!r) return fail(HNSW_ERR_BAD_ARG, "null result");
        if (d_lims) *d_lims = (const int64_t *)r->lims.p;
        if (d_ids) *d_ids = (const Id *)r->ids.p;
        if (d_dist) *d_dist = (const float *)r->dist.p;
        return HNSW_OK;
    }
};

// Every device table an index holds: the vectors and the graph, and the copies derived from them -- byte rows (X8, hnsw_rows8.hip),
// half rows (Xh, hnsw_rows16.hip), sq8 rows (Xq, hnsw_rows_sq8.hip), per-dimension sq8 rows (Xqd with their tables qd_lo / qd_s,
// hnsw_rows_sq8_dim.hip), bit rows (Xb with their thresholds bit_t, hnsw_rows_bits.hip), split rows (Xm / tail0, hnsw_rows_split.hip), locality codes
// (lcode / lcode0, hnsw_locality.hip); a derived table that does not exist has p == nullptr.  bind_view points the handle's IndexView at them.
struct IndexTables {
    Table X, X8, Xh, Xq, Xqd, qd_lo, qd_s, Xb, bit_t, Xm, tail0, lcode, lcode0, nbr0, nbrU, off, lvl, ref;
    template <class Self, class F> static void each(Self &t, F f) {
        static constexpr Table IndexTables::*all[] = {&IndexTables::X, &IndexTables::X8, &IndexTables::Xh, &IndexTables::Xq, &IndexTables::Xqd,
                                                      &IndexTables::qd_lo, &IndexTables::qd_s, &IndexTables::Xb, &IndexTables::bit_t, &IndexTables::Xm,
                                                      &IndexTables::tail0, &IndexTables::lcode, &IndexTables::lcode0, &IndexTables::nbr0, &IndexTables::nbrU,
                                                      &IndexTables::off, &IndexTables::lvl, &IndexTables::ref};
        for (Table IndexTables::*m : all) f(t.*m);
    }
    void release() { each(*this, [](Table &t) { t.release(); }); }
    size_t bytes() const { size_t s = 0; each(*this, [&](const Table &t) { s += t.bytes; }); return s; }
};

// where one knn launch reads its queries and writes its results (device addresses; nd / nh / st / any_flag may be null)
struct KnnBatch {
    const float *Q;
    int64_t nq, q_stride;
    int32_t *ids;
    float *dist;
    uint32_t *nd, *nh, *st, *any_flag;
};

// bytes of a [nq][q_stride] float matrix up to the end of its last query's d values
inline size_t query_bytes(int64_t nq, int64_t q_stride, int d) { return ((size_t)(nq - 1) * q_stride + d) * sizeof(float); }

// the device buffers of one batch of nq queries: the queries (qbytes), k ids and distances per query, the per-query counters
// and status words, and the launch's "any query flagged" word; scan: the per-slab lists of the exact scan (hnsw_scan.hip), sized
// by that call
struct BatchBufs {
    DevBuf q, ids, dist, nd, nh, st, flag, scan;
    // these buffers as a batch of nq queries whose results go to rows row0.. of ids / dist (a multi shard's slice of the table)
    KnnBatch batch(int64_t nq, int64_t q_stride, int k, int64_t row0 = 0) const {
        return {(const float *)q.p, nq, q_stride, (int32_t *)ids.p + row0 * k, (float *)dist.p + row0 * k,
                (uint32_t *)nd.p, (uint32_t *)nh.p, (uint32_t *)st.p, (uint32_t *)flag.p};
    }
    int ensure(int64_t nq, size_t qbytes, int k) {
        int rc;
        if ((rc = q.ensure(qbytes)) || (rc = ids.ensure((size_t)nq * k * 4)) || (rc = dist.ensure((size_t)nq * k * 4)) ||
            (rc = nd.ensure((size_t)nq * 4)) || (rc = nh.ensure((size_t)nq * 4)) || (rc = st.ensure((size_t)nq * 4)) || (rc = flag.ensure(16)))
            return rc;
        return HNSW_OK;
    }
    void release() { for (DevBuf *b : {&q, &ids, &dist, &nd, &nh, &st, &flag, &scan}) b->release(); }
};

// an owned index handle: one under construction (destroyed unless released to the caller), or a member of a device group
struct IndexDeleter { void operator()(::hnsw_index *idx) const { (void)hnsw_index_destroy(idx); } };
using IndexPtr = std::unique_ptr<::hnsw_index, IndexDeleter>;

// The per-device half of a multi-device handle (hnsw_multi: replicas, hnsw_sharded: shards): member g is an index on devices[g]
// (a device may be listed several times) with a stream, an event "member g's work is enqueued up to here", the buffers of one
// batch and a pinned host word for its launch's "any query flagged" word.  Streams, events, buffers and words are made by the
// first call that needs them (ensure_streams).  One call in flight per group.
struct DeviceGroup {
    std::vector<IndexPtr> members;
    std::vector<int> devices;
    std::vector<Stream> streams;         // [G], each made on its device
    std::vector<Event> done;             // [G]
    std::vector<BatchBufs> buf;          // [G], each on its device
    Pinned<uint32_t> hFlags;             // [G]
    ~DeviceGroup() { release(); }
    size_t size() const { return members.size(); }
    ::hnsw_index *operator[](size_t g) const { return members[g].get(); }
    // idx, on `device`, becomes the next member: the group owns it from here on, and it is never grown, shrunk or marked on its own
    // (hnsw_index::multi_replica)
    int adopt(::hnsw_index *idx, int device);
    // all or nothing: a failure leaves the group as it was, so the next call tries again
    int ensure_streams() {
        const size_t G = members.size();
        if (streams.size() == G) return HNSW_OK;
        std::vector<Stream> s(G);
        std::vector<Event> e(G);
        Pinned<uint32_t> flags;
        if (!hFlags) HIP_TRY(flags.alloc(G * sizeof(uint32_t), hipHostMallocPortable));
        for (size_t g = 0; g < G; ++g) {
            HIP_TRY(hipSetDevice(devices[g]));
            HIP_TRY(hipStreamCreateWithFlags(&s[g].h, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&e[g].h, hipEventDisableTiming));
        }
        streams = std::move(s); done = std::move(e);
        buf.resize(G);
        if (flags) hFlags = std::move(flags);
        return HNSW_OK;
    }
    // waits for EVERY stream, whatever the others answer ("nothing stays queued"), and reports the first failure
    int sync_all() {
        int rc = HNSW_OK;
        for (size_t g = 0; g < streams.size(); ++g) {
            hipError_t e = hipSetDevice(devices[g]);
            if (e == hipSuccess) e = hipStreamSynchronize(streams[g]);
            if (e != hipSuccess && !rc) rc = hip_fail(e, "hipStreamSynchronize");
        }
        return rc;
    }
    // per device, with that device current: the buffers, the stream, the event; then the members.  Harmless twice.
    void release() {
        for (size_t g = 0; g < devices.size(); ++g) {
            (void)hipSetDevice(devices[g]);
            if (g < buf.size()) buf[g].release();
            if (g < streams.size()) streams[g].reset();
            if (g < done.size()) done[g].reset();
        }
        buf.clear(); streams.clear(); done.clear();
        hFlags.reset();
        for (IndexPtr &m : members) m.reset();
        members.clear(); devices.clear();
    }
};

// the walk's side of a refined search (option "refine"): the first c members of W per query -- ids and distances [nq][c] -- and the
// walk's evaluation counts [nq], which the re-rank reads; ids also stages hnsw_rerank_batch's candidates.  Beside them qt: the
// queries the walk reads while the index searches its sq8 rows (Q', [nq][padded_stride(d)] floats: sq8_transform_queries; the bit
// rows against a 4-bit query: [nq][walk_query_stride] words of bit planes), sized by knn_search.  Not index tables: not counted in device_bytes.
struct RefineBufs {
    DevBuf ids, dist, nd, qt;
    int ensure(int64_t nq, int c) {
        int rc;
        if ((rc = ids.ensure((size_t)nq * c * 4)) || (rc = dist.ensure((size_t)nq * c * 4)) || (rc = nd.ensure((size_t)nq * 4))) return rc;
        return HNSW_OK;
    }
};

// Scratch of the ladder that the filtered, range, grouped and paged searches all climb (Ladder, hnsw_filter.hip), sized on demand
// by the call; not index tables: not counted in device_bytes.  One host thread uses a handle and every such call is synchronous,
// so one LadderBufs serves them all.
struct LadderBufs {
    DevBuf wnd, wnh, wst;                // one stage's walk: evaluations, hops, status of its m queries
    DevBuf list[2], count;               // the queries still unserved, written by one stage and read by the next; how many
    DevBuf q;                            // their vectors, gathered ([m][padded_stride(d)])
    // half rows / codes (Ladder::walk_exact; range, grouped, paged): one stage's walk before its re-rank ([m][e] ids and
    // distances); the re-rank's evaluation counts after it ([m])
    DevBuf cand, cdist, rnd;
};
// ... of the filtered calls; the grouped and the paged calls use wids / wdist, rids / rdist and stage for the same purposes
struct FilterBufs {
    DevBuf wids, wdist;                  // one stage's W ([m][e] ids and distances)
    DevBuf cnt, cand;                    // filtered: per walked query its allowed members of W; half rows / codes: the masked W the re-rank reads
    DevBuf rids, rdist, rnd;             // a compact [m][k] result (filtered: re-rank, exact scan; grouped: exact stage) before its rows go to their queries
    DevBuf stage;                        // out_stage [nq]: filtered, grouped and paged (ladder_host_call downloads it)
    // hnsw_search_batch_filtered_each: the masks' device addresses [n_filters], query_filter [nq]; the exact stage's rows
    // (filter_plan): row -> query, tile -> filter, and per row the evaluations to add and whether the query took no walk
    DevBuf masks, which, rows;
};
// ... of the grouped calls (hnsw_group.hip) alone
struct GroupBufs {
    DevBuf best;                         // the exact stage: best[piece][n_labels] words (key << 32 | row), all ones = no node yet
    DevBuf lab, rlab;                    // out_labels [nq][k]; the labels column of a compact [m][k] result
    DevBuf part_words, part_lab;         // ... of a row of many cells: the k smallest words of each of its stripes and their labels
};
// ... of the paged calls (hnsw_after.hip) alone
struct AfterBufs {
    DevBuf lo;                           // the cursors as bounds in word space (uint64 [nq], by query)
};
// ... of the range calls alone.  What a caller keeps (lims, ids, distances, counters) belongs to the hnsw_range_result instead.
constexpr int RANGE_STAGES = 11;         // the longest ladder: ef = 1, 2, 4, ... 1024
struct RangeBufs {
    DevBuf wids[RANGE_STAGES], wdist[RANGE_STAGES];  // every stage's W ([m][e], half rows / codes: re-ranked), kept until the fill
    DevBuf cnt, src, stage, nd, nh;                  // per query: segment length (int64 [nq + 1]), its row of its stage's W, counters
    DevBuf pre;                                      // ... under a mask: the length of the in-range prefix the segment was taken from
    DevBuf counts, offs;                             // the exact scan: hits per (query, slab) (uint64 [m][slabs] + 1) and their exclusive sum
    DevBuf xcnt, xoff;                               // ... segment lengths of the exact-stage queries and where their words start ([m + 1])
    DevBuf words[2], cub;                            // ... the hits as (key << 32 | row), unsorted and sorted; hipcub's temporary storage
};

// The keys an index owns (hnsw_keys.hip): key_of [n] int64 in row order, and the lookup table -- the n pairs (key, node) in
// ascending SIGNED key order as two columns, sorted [n] int64 and node [n] int32 -- rebuilt from key_of whenever that changes.
// Owned by the handle as the live mask is: not index tables, not counted in device_bytes (hnsw_index_keys_info reports bytes()).
struct KeyTables {
    Table key_of, sorted, node;
    int64_t n = 0;
    size_t bytes() const { return key_of.bytes + sorted.bytes + node.bytes; }
};
// where a keyed host call writes its rows: [nq][k] keys, missing where the search wrote its fill id
struct KeysOut {
    int64_t *keys;
    int64_t missing;
};

// A host call whose queries are ROWS OF THE INDEX (hnsw_by_id.hip): ids [nq], id_base-based and already validated by the entry
// point.  drop_self: the call runs k + 1 wide (the k handed to HostCall::begin is that k + 1) into the handle's scratch and the
// drop-self epilogue writes the caller's [nq][k] rows (the rule: hnsw_by_id_plan.h).
struct RowsIn {
    const int32_t *ids;
    bool drop_self;
};
// ... its scratch: the queries' own ids on the device [nq], and the compacted [nq][k] ids and distances of a drop-self call before
// their download (keys: the handle's key_scratch).  Not index tables: not counted in device_bytes.
struct ByIdBufs {
    DevBuf self, ids, dist;
};
// A host call that ends in the selection of hnsw_diverse.hip (hnsw_search_batch_diverse, hnsw_brute_force_batch_diverse): the inner
// call runs as wide as the pool (the k handed to HostCall::begin) into the handle's scratch, never into the caller's arrays, and
// HostCall::finish queues the selection kernel over those rows and downloads its [nq][k] rows into ids / dist / div (div optional)
struct DiverseOut {
    int32_t k;
    float lambda;
    int32_t fill;
    int32_t *ids;
    float *dist, *div;
};
// ... its scratch: the selection's [nq][k] rows before their download (div: also hnsw_diversify_batch's).  Not index tables: not
// counted in device_bytes.
struct DiverseBufs {
    DevBuf ids, dist, div;
};

inline int env_int(const char *name, int dflt) {
    const char *s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}
inline int pick_nch(int nchunks) {
    const int per_lane = (nchunks + 15) / 16;
    for (int c : {1, 2, 4, 8, 16}) if (per_lane <= c) return c;
    return 0;
}
inline int pick_nslot(int ef) {
    for (int s : {1, 2, 4, 8, 16}) if (ef <= 64 * s) return s;
    return 0;
}
// ... of the knn kernel: where has_odd_nslot, W also comes in three (ef 129..192) and six (ef 257..384) registers -- a W window
// that needs three registers pays for three (pop chain, flag masks, registers), not for four; the other row widths, the builder
// and the layer operators keep powers of two (pick_nslot)
inline int pick_nslot_knn(int ef, int nch) {
    if (has_odd_nslot(nch)) { for (int s : {1, 2, 3, 4, 6, 8, 16}) if (ef <= 64 * s) return s; return 0; }
    return pick_nslot(ef);
}
// index of a slot count in per-shape tables (hnsw_index::shape)
inline int slot_class(int nslot) {
    switch (nslot) { case 1: return 0; case 2: return 1; case 3: return 2; case 4: return 3; case 6: return 4; case 8: return 5; default: return 6; }
}
constexpr int SLOT_CLASSES = 7;
// (padded_stride(d), the floats of a row -- rows are multiples of 64 B --: hnsw_bits_plan.h)

// The graph tables of an index of n nodes: X (max(n, 1) rows of `stride` floats), nbr0 ([n][S0]) and nbrU ([max(rowsU, 1)][SU])
// with every slot empty (-1), off / lvl / ref (max(n, 1) entries each, written by upload_upper_layout)
int alloc_graph_tables(IndexTables &t, int64_t n, int64_t stride, int S0, int SU, int64_t rowsU);
// The upper-row layout of m nodes of levels lvl[0..m): a node's rows of layers 1..lvl lie side by side, the nodes' in order from
// row `row0` on.  ref[j] = {first row or -1, level} (IndexView::upper_ref); returns the row count after them.
int64_t upper_layout(const uint8_t *lvl, int64_t m, int64_t row0, std::vector<int2> &ref);
// ... written into off / lvl / ref of the nodes [n0, n0 + ref.size())
int upload_upper_layout(IndexTables &t, int64_t n0, const std::vector<int2> &ref);

// copies [n][row_stride] host rows into n zero-padded rows of a device table (rows of padded_stride(d) floats)
int upload_rows(const float *vectors, int64_t n, int d, int64_t row_stride, float *dst);

} // namespace hnsw_host

// one submitted batch (hnsw_search_submit / hnsw_search_wait): its own device buffers and stream
struct hnsw_request {
    hnsw_index *idx = nullptr;
    int64_t nq = 0, q_stride = 0;
    hnsw_search_params params{};
    hnsw_host::BatchBufs buf;
    hnsw_host::RefineBufs refine;        // its walk's results while option "refine" is active
    int stream = 0;
};

// an allow-mask over the nodes of one index (hnsw_filter_create): bit v of the device copy = node v (0-based) may be returned
struct hnsw_filter {
    const hnsw_index *idx = nullptr;     // the handle it was made for ...
    int64_t n = 0;                       // ... and that handle's n then: a grown index refuses it
    uint64_t epoch = 0;                  // ... and its graph epoch then: an index changed since refuses it
    int64_t n_allowed = 0;               // set bits below n (filter_popcount_kernel)
    // ceil(n / 32) words, the positions >= n of the last one clear; behind them (8-byte aligned) the mask's own device address:
    // the table of one filter that the single-filter call hands the kernels
    hnsw_host::DevBuf bits;
    static size_t table_offset(int64_t n) { return ((size_t)std::max<int64_t>((n + 31) / 32, 1) * 4 + 7) / 8 * 8; }
    const uint32_t *const *table() const { return (const uint32_t *const *)((const char *)bits.p + table_offset(n)); }
};

// one label per node of one index (hnsw_labels_create): the groups of hnsw_search_batch_grouped.  Bound to the handle, its n and
// its graph epoch as a filter is.
struct hnsw_labels {
    const hnsw_index *idx = nullptr;
    int64_t n = 0;
    uint64_t epoch = 0;
    int32_t n_labels = 0;
    int64_t n_labelled = 0, n_groups = 0;    // nodes with a label >= 0; labels a node carries (labels_prepare_kernel)
    hnsw_host::DevBuf lab;                   // [n] int32, -1 where the node has no label or was marked deleted at creation
};

// what a range call returns: lims, ids, distances and the per-query counters on the device of the index they came from
// (hnsw_range.hip; the sharded range calls read the counters where they lie: hnsw_sharded.hip)
struct hnsw_range_result : hnsw_host::RangeRecord<int32_t> {};
// ... and a sharded range call and hnsw_merge_segments: int64 global ids, on one device; it keeps no reference to the handle it came from
struct hnsw_sharded_range_result : hnsw_host::RangeRecord<int64_t> {};

struct hnsw_index {
    int device = -1;
    hnsw_dev::IndexView iv{};
    hnsw_index_info info{};
    hnsw_host::IndexTables tables;       // every device table: device_bytes is their sum (hnsw_index_get_info)
    // locality codes (tables.lcode / lcode0): built when the visited set first runs as bitmap blocks.  lcode_state: 0 not built
    // yet, 1 built, -1 cannot be built (no upper layer to derive an order from)
    int lcode_state = 0;
    int blk_mode = -1;                   // option "visited_blocks": -1 automatic (measured per kernel shape on the index's own vectors), 0 never, 1 always
    // What the handle decided for each shape of the knn kernel, [slot_class(NSLOT)][accept rule]; everything else a shape depends
    // on (n, row format, options "vt_bits" / "visited_blocks") forgets them when it changes (forget_shapes)
    struct ShapeChoice {
        int blk = -1;                    // the visited structure (knn_blk_bits): -1 undecided, 0 tag cache, else log2 of the block slots
        int vt_bits = 0;                 // log2 tags of the grown tag cache (knn_vt_bits), 0 = not computed yet
        int per_cu = -1;                 // waves of the kernel one CU holds when each asks for `lds` bytes (resident_queries): -1 not
        size_t lds = 0;                  //  asked yet, 0 unknown.  lds is compared: the blocks can be lost to a failed allocation
    } shape[hnsw_host::SLOT_CLASSES][2];
    // keep_visited: all but the visited-structure choices (what survives an insert that kept the row format)
    void forget_shapes(bool keep_visited = false) {
        for (auto &c : shape) for (ShapeChoice &s : c) s = ShapeChoice{keep_visited ? s.blk : -1};
    }
    int cus = 0;                         // the device's CUs (0 = not read yet)
    hnsw_host::BatchBufs scratch;                            // scratch for the host-buffer entry points
    hnsw_host::Pinned<uint32_t> hFlag;                       // the "any query flagged" word in pinned host memory (zero-copy calls)
    uint32_t *hFlagDev = nullptr;                            //  and its device address
    hnsw_host::Pinned<char> hSmall;                          // page-locked block for small host-buffer calls (hnsw_search_batch: queries, ids, distances, counters)
    char *hSmallDev = nullptr;
    // option "device_fallback_slab_bytes": a slab of the caller's chosen size for the exactness fallback of
    // hnsw_search_batch_device, run on the caller's stream without a host round trip (dFbMap: the flagged queries' list)
    hnsw_host::DevBuf dFbSlab, dFbMap;
    int64_t fb_queries = 0;                                  // how many flagged queries one launch can repair (slab bytes / (4 n))
    hnsw_host::Stream hs[4];                                 // streams of the chunked host-buffer search and of requests (lazy)
    std::vector<hnsw_request *> free_requests;               // finished requests keep their buffers for the next submit
    std::vector<std::unique_ptr<hnsw_request>> all_requests; // every request ever created (released with the index)
    int live_requests = 0, next_stream = 0;
    bool time_kernels = false;           // option "time_kernels": event triples around the launches of each device-entry call
    std::vector<hnsw_host::Event> tev;        // [3 * recorded calls]: before the pre-pass, before the search kernel, after it
    size_t tev_used = 0;
    std::vector<char> tev_ordered;       // per recorded call: did the ordering pre-pass run
    // scratch of the ordering pre-pass, one block per caller stream (kept between calls: work on one
    // stream is ordered, so the block is free again when the next call on that stream needs it)
    struct OrderScratch { hipStream_t st; hnsw_host::Table block; };
    std::vector<OrderScratch> order_scratch;
    // HNSW_METRIC_COSINE: N(Q) of the batch a call was handed, one matrix per caller stream (cosine_queries, hnsw_cosine.hip); kept
    // between calls as order_scratch is.  Not an index table: not counted in device_bytes.
    struct CosineScratch { hipStream_t st; hnsw_host::DevBuf q; };
    std::vector<CosineScratch> cosine_scratch;
    int order_mode = -1;                 // option "order_queries": -1 automatic (batches larger than half of what the chip holds: resident_queries), 0 never, 1 always
    // option "head_queries": rows [0, H) of a host call's batch searched unordered on hs[1] while the rest's pre-pass runs
    // (head_rows, hnsw_capi.hip): -1 automatic, 0 never, > 0 that many (at most nq - 1)
    int64_t head_queries = -1;
    int vt_bits_override = 0;
    int lds_pad = -1;                    // option "lds_pad": extra LDS bytes per search wave (-1 = balanced_lds_pad's choice)
    int scan_slabs = 0;                  // option "scan_slabs": row slabs of the exact scans (0 = scan_slab_rows' choice)
    std::vector<std::pair<int, int>> prepared;   // (ef, accept rule) of every hnsw_index_prepare: what hnsw_index_save writes down
    // what the options "byte_rows" / "split_rows" asked for (bind_view leaves an unused copy out of the view), so that
    // hnsw_index_insert, which makes the row copies again, keeps their effect: byte_rows 0, split_rows 0 (off), split_rows -1
    // (off and freed for good)
    bool byte_rows_off = false, split_rows_off = false, split_rows_freed = false;
    // option "half_rows": the knn searches read tables.Xh (1), or it is off (0, -1).  Not a default: half rows change results.
    // hnsw_index_insert makes the copy again while it is on.
    bool half_rows_on = false;
    // option "refine": 0 off; 1..1024 / -1: while the knn searches read the half rows, the head of W (max(k, refine) members, -1: all
    // ef) is re-ranked over the float32 rows (refine_count, hnsw_rerank.hip).  refine_scratch: the walk's results of the calls that
    // bring no scratch of their own (every entry point but submit / wait).
    int refine = 0;
    hnsw_host::RefineBufs refine_scratch;
    // option "sq8_rows": the knn searches walk tables.Xq, the 8-bit codes of x ~ sq8_lo + sq8_scale * code (1), or it is off (0, -1).
    // sq8_lo / sq8_scale describe tables.Xq whenever it exists.  hnsw_index_insert quantises the whole grown table again while it is on.
    bool sq8_on = false;
    float sq8_lo = 0.0f, sq8_scale = 1.0f;
    // option "sq8_dim_rows": the knn searches walk tables.Xqd, the 8-bit codes of x_i ~ lo_i + s_i * code under one affine map per
    // dimension (1), or it is off (0, -1).  sq8d_lo / sq8d_scale ([d] each; on the device tables.qd_lo / qd_s in the lane grid)
    // describe tables.Xqd whenever it exists.  hnsw_index_insert and hnsw_index_remove quantise the whole table again while it is on.
    bool sq8d_on = false;
    std::vector<float> sq8d_lo, sq8d_scale;
    // option "bit_rows": the knn searches walk tables.Xb, one bit per dimension (x_i > t_i) under Hamming distance; 1: t = the column
    // means, 2: t = 0; 0: off, and the copy is freed.  bit_t ([d]; on the device tables.bit_t, [512 * NW] floats) describes tables.Xb
    // whenever it exists.  hnsw_index_insert and hnsw_index_remove quantise the whole table again while it is on.
    int bit_mode = 0;
    std::vector<float> bit_t;
    // option "bit_query_bits": 4 = while the searches walk tables.Xb, the query keeps 4 bits a dimension (four bit planes of codes in
    // -7..7, bits_asym_transform_queries) and the walk's key is the inner product's (the knn kernel's ROWS 7, hnsw_bits_asym_walk.hip);
    // 0 = one bit, the Hamming walk.  The rows are the same copy either way.  Accepted, without effect, while other rows are walked.
    // Not saved.
    int bit_query_bits = 0;
    // option "filter_collect": the filtered searches answer from every node the walk evaluates, not from the final W only
    // (hnsw_search_collect_kernel; k <= 128, exact-row formats: it excludes half_rows and sq8_rows).  Not saved.
    bool filter_collect = false;
    // the stages of the filtered, range, grouped and paged calls (ladder_scratch: of all four; who uses what of the others: beside
    // the types), the range calls' exact scan: ONE such call in flight per handle
    hnsw_host::LadderBufs ladder_scratch;
    hnsw_host::FilterBufs filter_scratch;
    hnsw_host::RangeBufs range_scratch;
    hnsw_host::GroupBufs group_scratch;
    hnsw_host::AfterBufs after_scratch;
    bool multi_replica = false;          // owned by an hnsw_multi (hnsw_multi_replica) or an hnsw_sharded (hnsw_sharded_shard): not grown or shrunk on its own (hnsw_index_insert, hnsw_index_remove)
    // the graph epoch: every successful hnsw_index_insert and hnsw_index_remove moves it on (adopt_graph).  A filter records the
    // epoch it was made in: n alone would let a mask through after "remove 5, insert 5"
    uint64_t epoch = 0;
    // Soft deletion (hnsw_soft_delete.hip).  live: a filter this handle owns over the mask of the nodes NOT marked deleted, made by
    // the first hnsw_index_mark_deleted and kept current (its n and epoch are the handle's; its n_allowed is n - n_deleted); null
    // on a handle never marked.  While n_deleted > 0 the searches answer under it (live_filter); at 0 every call takes its plain
    // path.  Not an index table: not counted in device_bytes.
    std::unique_ptr<hnsw_filter> live;
    int64_t n_deleted = 0;
    // Keys (hnsw_keys.hip): null on a handle never given keys, which every entry point then treats as before; else one key per
    // node, n entries, moved with the nodes by adopt_graph.  key_scratch: the [nq][k] keys of a keyed host call before their download.
    std::unique_ptr<hnsw_host::KeyTables> keys;
    hnsw_host::DevBuf key_scratch;
    // Searches by stored item (hnsw_by_id.hip): scratch of the host calls whose queries are rows of the index, and option
    // "graph_chunk_rows": the nodes hnsw_knn_graph searches per inner call (>= 1)
    hnsw_host::ByIdBufs by_id_scratch;
    hnsw_host::DiverseBufs diverse_scratch;                  // the diversified searches (hnsw_diverse.hip)
    int64_t graph_chunk_rows = hnsw_host::GRAPH_CHUNK_ROWS;
};

namespace hnsw_dev {

// (MaskWords / mask_words, a mask's words as a kernel reads them: hnsw_device.hip.h, beside the collect kernel's use of them)

// is the id_base-based id one of the n nodes (a filled entry of W is not) ...
__device__ __forceinline__ bool is_node(int64_t n, int32_t id_base, int32_t id) {
    const int64_t v = (int64_t)id - id_base;
    return v >= 0 && v < n;
}
// ... and allowed by the mask -- the test of the four select kernels; group_label and after_eligible, whose mask is optional, put
// their own conditions on top
__device__ __forceinline__ bool node_allowed(MaskWords bits, int64_t n, int32_t id_base, int32_t id) {
    const int64_t v = (int64_t)id - id_base;
    return is_node(n, id_base, id) && ((bits[v >> 5] >> (v & 31)) & 1u);
}

// The counters of a query the exact stage answers (the scatter kernel, after_merge_kernel, range_count_kernel): `add` evaluations
// on top of its walks' -- fresh: it took no walk, they start from 0 and it made no hop -- and the exact stage's number
__device__ __forceinline__ void exact_settle(uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_stage, int64_t q, uint32_t add, bool fresh) {
    out_nd[q] = (fresh ? 0u : out_nd[q]) + add;
    if (fresh) out_nh[q] = 0u;
    out_stage[q] = 0xFFFFFFFFu;
}

// The end of a ladder stage's select kernel (filter_, range_, group_, after_select_kernel), one lane per walked query: row i of the
// stage's batch belongs to query q.  Its walk's counters go to the query's; served, it gets the stage's number, else a place in
// the short list through one atomic counter (the host sorts the list: the next stage's order, and with it nothing a caller can
// see, depends on who came first).
struct LadderOut {
    const uint32_t *wnd, *wnh; // [m] the stage's evaluations and hops
    uint32_t stage;            // what a served query's out_stage becomes
    int32_t accumulate;        // out_nd / out_nh: 0 = set (the first walk), 1 = add
    uint32_t *out_nd, *out_nh, *out_stage;   // [nq]
    int32_t *short_list;       // the queries (map's numbering) that are not served ...
    uint32_t *short_count;     // ... and how many
};
__device__ __forceinline__ void ladder_settle(const LadderOut &o, int64_t i, int64_t q, bool served) {
    o.out_nd[q] = (o.accumulate ? o.out_nd[q] : 0u) + o.wnd[i];
    o.out_nh[q] = (o.accumulate ? o.out_nh[q] : 0u) + o.wnh[i];
    if (served) o.out_stage[q] = o.stage;
    else o.short_list[atomicAdd(o.short_count, 1u)] = (int32_t)q;     // (at most m entries: one per block)
}

// filter_scatter_kernel (hnsw_filter.hip; scatter_rows launches it): rows of a compact result to the rows of the queries they belong to
struct ScatterArgs {
    const int32_t *rids;       // [m][k] compact results
    const float *rdist;
    const int32_t *rlab;       // null, or their labels column (the grouped calls), which goes to out_labels
    int64_t m;
    int32_t k;
    const int32_t *map;        // [m] row i belongs to query map[i] (< 0: a padding row, dropped); null: to query i
    const int32_t *cnt;        // null: every row; else only the rows with cnt[i] >= k (the served ones)
    const uint32_t *add;       // null, or [m]: evaluations to add to out_nd
    uint32_t add_const;        // ... plus this many
    int32_t exact;             // 1: the exact stage's rows, their counters by exact_settle; 0: a stage's re-ranked rows, out_nd += add
    const int32_t *fresh_of;   // exact: null, or [m]: `fresh` per row
    int32_t fresh;             // exact: 1: the query took no walk
    int32_t *out_ids;          // [nq][k]
    float *out_dist;
    int32_t *out_labels;
    uint32_t *out_nd, *out_nh, *out_stage;
};

} // namespace hnsw_dev

namespace hnsw_host {

inline int DeviceGroup::adopt(::hnsw_index *idx, int device) {
    idx->multi_replica = true;
    members.emplace_back(idx);
    devices.push_back(device);
    return HNSW_OK;
}

// hnsw_capi.hip: IndexView's table pointers from idx->tables (X8 / Xm left out while option byte_rows / split_rows is 0; Xh in
// the view while option half_rows is 1 and no byte rows are: it takes the place of Xm; Xq in the byte rows' place while option
// sq8_rows is 1 and no byte rows are: Xm steps aside too; Xqd there, and qd_s in tail0's place, while option sq8_dim_rows is 1
// and no byte rows are; Xb there while option bit_rows is on and no byte rows are), and the hnsw_index_info fields that
// restate the view (n, max_degree0, max_layer, entry_point, row_stride_bytes, row_format).  Called by every change of the tables
// or of those options.
void bind_view(::hnsw_index *idx);
// hnsw_capi.hip: the end of hnsw_index_create and hnsw_build, once the graph tables are complete: the view bound, the row copies
// made, the first search's one-time costs paid.  *out = idx on success.
int finish_index(IndexPtr idx, int32_t expected_ef, int32_t expected_semantics, ::hnsw_index **out);

// hnsw_capi.hip: hnsw_index_create; stored_rows: desc->vectors are rows a handle held (hnsw_index_load): a COSINE index takes them
// as they are -- N is not idempotent bit for bit
int create_index(const hnsw_index_desc *desc, int32_t device, bool stored_rows, ::hnsw_index **out);

// ---- HNSW_METRIC_COSINE (hnsw_cosine.hip): an IP index over N(X) whose entry points hand N(Q) on --------------------------------
// The normalise kernel on `st`: out row i = N(in row i) (include/hnsw_mi355x.h), d values per row; pad_rows: index rows, zero from d
// to the row's end (out_stride = padded_stride(d)).  `in` may be a registered host matrix seen from the device; in == out (same
// stride) is allowed.  norms (optional, [n]); bad_flag (optional, one word the caller set to 0xFFFFFFFF): the least row whose sum of
// squares is NaN or infinite.
int cosine_normalise(const float *in, int64_t n, int d, int64_t in_stride, float *out, int64_t out_stride, float *norms, uint32_t *bad_flag,
                     hipStream_t st, bool pad_rows = false);
// ... in place over the m freshly uploaded rows `rows` of an index's float32 table (rows of padded_stride(d) floats), waited for:
// HNSW_ERR_BAD_ARG ("...: <what>") naming the first row i of the m whose sum of squares is not finite
int cosine_store_rows(float *rows, int64_t m, int d, const char *what);
// Where a call reads its queries: the caller's device matrix for L2 and IP (nothing queued); for COSINE the handle's scratch matrix
// of stream `st`, filled with N(Q) by the kernel queued there (same stride).  Called ONCE per public call, at the entry point,
// before the first internal consumer: knn_search, scan_search, Ladder, launch_rerank, the range scans, knn_repair and the sq8 query
// transform all receive an already-normalised device matrix.
int cosine_queries(::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, hipStream_t st, const float **out_Q, int64_t *out_stride);
inline bool is_cosine(const ::hnsw_index *idx) { return idx->info.metric == HNSW_METRIC_COSINE; }

// hnsw_build.hip: HNSW_ERR_BAD_ARG ("...: <verb>") for a graph whose upper rows list a node that is not on that layer, or whose
// entry point is not on the top layer: what hnsw_index_insert and hnsw_index_remove ask before they follow the rows (n > 0)
int check_upper_rows(const ::hnsw_index *idx, const char *verb);
// hnsw_build.hip: the end of hnsw_index_insert and hnsw_index_remove: nx's graph tables become idx's (see there)
// new_id: how the nodes were renumbered (hnsw_index_remove: RemovePlan::new_id; null: ids kept, hnsw_index_insert) -- what the
// marks of soft deletion follow
// append_keys (hnsw_index_insert_keyed, [nx->iv.n - idx->iv.n]): the keys of the new nodes -- what the keys follow
int adopt_graph(::hnsw_index *idx, IndexPtr &nx, bool carry_codes, int32_t expected_ef, int32_t expected_semantics,
                const int32_t *new_id = nullptr, const int64_t *append_keys = nullptr);
// hnsw_build.hip: hnsw_index_insert once the keyed question is settled: keys null on a handle without keys, else one per vector
int insert_vectors(::hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride, const hnsw_build_params *p, const int64_t *keys);

// hnsw_build.hip: what hnsw_index_insert refuses of its arguments before anything is built, for an index that holds n_old nodes with
// top layer max_layer when the m vectors arrive (see there)
int check_insert(const ::hnsw_index *idx, int64_t n_old, int max_layer, const float *vectors, int64_t m, int64_t row_stride,
                 const hnsw_build_params *p);
// hnsw_build.hip: the two parts of one insert attempt.  insert_graph: tables for idx's nodes + m, idx's graph copied into them,
// then grow_graph_in_place, which inserts m vectors behind the nx->iv.n nodes nx holds in tables already sized for them
// (grown_upper_rows: the upper rows that takes).  The upsert runs the second part alone on the tables its removal half filled.
int64_t grown_upper_rows(const hnsw_build_params *p, int64_t n_old, int64_t m, int64_t rowsU_old);
int grow_graph_in_place(::hnsw_index *nx, const float *vectors, int64_t m, int64_t row_stride, const hnsw_build_params *p,
                        int64_t rem_scale, bool *rem_overflow);
int insert_graph(const ::hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride, const hnsw_build_params *p,
                 int64_t rem_scale, bool *rem_overflow, IndexPtr &out);
// hnsw_remove.hip: one removal attempt: out = a new handle with the repaired graph of idx's live nodes, in tables sized for
// n_tables nodes and rowsU_tables upper rows (see there).  idx is only read.
int remove_graph(const ::hnsw_index *idx, const RemovePlan &plan, int64_t n_tables, int64_t rowsU_tables, IndexPtr &out);
// hnsw_upsert.hip: hnsw_index_upsert_keyed / hnsw_index_update once the call's rows are split (UpsertPlan, |P| > 0): the removal of
// P and the insert of the m vectors in front of ONE adopt_graph.  keys: one per vector on a keyed handle, else null.
int upsert_vectors(::hnsw_index *idx, const UpsertPlan &up, const float *vectors, int64_t m, int64_t row_stride,
                   const hnsw_build_params *p, const int64_t *keys);

// hnsw_rows8.hip: if every value of tables.X is an integer in 0..255, build the byte copy (tables.X8, iv.stride8)
int make_byte_rows(::hnsw_index *idx);
// hnsw_rows16.hip: the half copy of tables.X (tables.Xh): HNSW_ERR_UNSUPPORTED, nothing allocated, when a value is NaN or
// rounds to an fp16 infinity; HNSW_ERR_OOM when there is no room for it.  Leaves the view to the caller (bind_view).
int make_half_rows(::hnsw_index *idx);
// hnsw_rows_sq8.hip: the 8-bit codes of tables.X under one affine map (tables.Xq, sq8_lo, sq8_scale), all or nothing:
// HNSW_ERR_UNSUPPORTED when a value is NaN or infinite or max - min overflows; HNSW_ERR_OOM when there is no room.  Leaves the
// view to the caller (bind_view).
int make_sq8_rows(::hnsw_index *idx);
// ... and nq queries moved to the codes' space on `st`: Qt ([nq][padded_stride(d)] floats) = (Q - lo) / scale for L2, Q for the
// inner product, zero beyond d.  Q may be a registered host matrix seen from the device; stage (optional, [nq][q_stride] device
// floats) then receives the queries as they were read.  Q == Qt (same stride) is allowed.
int sq8_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st);
// hnsw_rows_sq8_dim.hip: the 8-bit codes of tables.X under one affine map per dimension (tables.Xqd / qd_lo / qd_s, sq8d_lo,
// sq8d_scale), all or nothing: HNSW_ERR_UNSUPPORTED, naming the first such column, when a value is NaN or infinite, a column's
// max - min overflows or its step rounds to 0; HNSW_ERR_OOM when there is no room.  Leaves the view to the caller (bind_view).
int make_sq8_dim_rows(::hnsw_index *idx);
// ... and nq queries as the walk over those codes reads them, on `st`: Qt ([nq][padded_stride(d)] floats) = Q - lo for L2, s * Q
// for the inner product, zero beyond d.  Q, stage and Q == Qt: as sq8_transform_queries.
int sq8_dim_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st);
// ... the transform of whichever codes the index walks (walks_codes)
inline int codes_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st);
// hnsw_sq8_dim_walk.hip, one object per accept rule (0 Ohnsw, 1 functor): the knn kernel's ROWS = 5 instances, the L2 walk over
// those codes -- what a variant object of hnsw_search_variants.hip exports, for the one metric the format has a kernel for
hipError_t search_launch_sq8_dim_0(int nch, int nslot, const hnsw_dev::IndexView &iv, const hnsw_dev::SearchArgs &a, hipStream_t st);
hipError_t search_launch_sq8_dim_1(int nch, int nslot, const hnsw_dev::IndexView &iv, const hnsw_dev::SearchArgs &a, hipStream_t st);
int search_occupancy_sq8_dim_0(int nch, int nslot, size_t lds, int blk);
int search_occupancy_sq8_dim_1(int nch, int nslot, size_t lds, int blk);
// hnsw_rows_bits.hip: the 1-bit codes of tables.X (tables.Xb / bit_t, idx->bit_t) under thresholds of `mode` (1: the column means,
// 2: zero), all or nothing: HNSW_ERR_UNSUPPORTED, naming the first such column, when a value is NaN or infinite (mode 1);
// HNSW_ERR_OOM when there is no room.  Leaves the option's value and the view to the caller (bind_view).
int make_bit_rows(::hnsw_index *idx, int mode);
// ... and nq queries as the walk over those codes reads them, on `st`: the first 16 * NW words of every Qt row ([nq][padded_stride(d)]
// floats) are the query's bits q_i > t_i, zero beyond d.  Q and stage: as sq8_transform_queries; Q == Qt is NOT allowed.
int bits_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st);
// ... and as the walk of option bit_query_bits 4 reads them: every Qt row is bit_plane_words(d) = 64 * NW words, the four bit planes
// p0..p3 of the query's codes v = p0 + 2 p1 + 4 p2 - 8 p3 (include/hnsw_mi355x.h: the rule), each packed as a row's bits are.  One
// wave per query.  Q and stage: as sq8_transform_queries; Q == Qt is NOT allowed.  codes (optional, [nq][d] int8, device): the v_i
// themselves; Qt may then be null.
int bits_asym_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, int8_t *codes,
                                hipStream_t st);
// hnsw_bits_asym_walk.hip, one object per accept rule: the knn kernel's ROWS = 7 instances, the walk over the same codes against
// those planes under the inner product's key; nch here is NW
hipError_t search_launch_bits_asym_0(int nch, int nslot, const hnsw_dev::IndexView &iv, const hnsw_dev::SearchArgs &a, hipStream_t st);
hipError_t search_launch_bits_asym_1(int nch, int nslot, const hnsw_dev::IndexView &iv, const hnsw_dev::SearchArgs &a, hipStream_t st);
int search_occupancy_bits_asym_0(int nch, int nslot, size_t lds, int blk);
int search_occupancy_bits_asym_1(int nch, int nslot, size_t lds, int blk);
// hnsw_bits_walk.hip, one object per accept rule (0 Ohnsw, 1 functor): the knn kernel's ROWS = 6 instances, the Hamming walk over
// those codes under every metric; nch here is NW
hipError_t search_launch_bits_0(int nch, int nslot, const hnsw_dev::IndexView &iv, const hnsw_dev::SearchArgs &a, hipStream_t st);
hipError_t search_launch_bits_1(int nch, int nslot, const hnsw_dev::IndexView &iv, const hnsw_dev::SearchArgs &a, hipStream_t st);
int search_occupancy_bits_0(int nch, int nslot, size_t lds, int blk);
int search_occupancy_bits_1(int nch, int nslot, size_t lds, int blk);
// hnsw_rows_split.hip: if a row ends 1..32 bytes past a 128-byte line (and there are no byte rows), build the split copy
// (tables.Xm / tail0, iv.stride_m / main_chunks / tail_chunks); call after make_byte_rows, graph in place
int make_split_rows(::hnsw_index *idx);

// hnsw_order.hip: the descent alone for nq device-resident queries: d_entry[q] = the node the greedy descent reaches on layer
// to_layer (lib/ohnsw.ml:865-867 stopped there); d_scratch: 4 * nq words
int descent_entries(::hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride, int32_t to_layer, int32_t *d_entry,
                    uint32_t *d_scratch, hipStream_t st);
// hnsw_capi.hip: the one-time costs of a process's first search (code objects, the handle's stream and flag word), paid at
// index construction: one query through the plain and the ordered launch
int warm_up(::hnsw_index *idx);
// hnsw_capi.hip: hnsw_index_prepare for construction paths (expected_ef): failures are swallowed, a search reports its own
void prepare_quietly(::hnsw_index *idx, int32_t ef, int32_t semantics);
// hnsw_capi.hip: a saved decision of the visited structure for the shape of (ef, rule): blocks (true) or the tag cache
void adopt_blk_choice(::hnsw_index *idx, int32_t ef, int32_t semantics, bool blocks);
// ... and the decisions a handle has made so far, as (ef representative of the shape, rule, blocks?) triples
void list_blk_choices(const ::hnsw_index *idx, std::vector<int32_t> &out3);
// hnsw_layer_ops.hip: Ohnsw.search_k on one layer for device-resident targets (one start node each, W bounded by ef): the
// nearest node found per target
int layer_nearest_device(::hnsw_index *idx, int32_t layer, const float *d_targets, int64_t t_stride, int64_t nq, const int32_t *d_qmap,
                         int64_t n_launch, const int32_t *d_starts, int32_t ef, int32_t *d_out_ids, float *d_out_dist);
// hnsw_locality.hip: builds tables.lcode / lcode0 once; lcode_state says how it went.  The per-slot table lcode0
// (n * max_degree0 * 4 bytes) exists only while a kernel shape uses the bitmap blocks or is being measured: drop_lcode0 frees
// it, materialise_lcode0 (also reached through build_locality_codes) makes it again from lcode.
int build_locality_codes(::hnsw_index *idx);
int materialise_lcode0(::hnsw_index *idx);
void drop_lcode0(::hnsw_index *idx);
int adopt_locality_codes(::hnsw_index *idx, const int32_t *codes);
// hnsw_index_insert: the codes of `from` (n_old nodes) carried over to the grown `to`, whose new nodes v get code v (still a
// permutation); the per-slot table is made again over to's rows if `from` had one.  Not enough memory is an error here
// (HNSW_ERR_OOM): a handle whose kernel shapes run the bitmap blocks cannot go on without them.
int extend_locality_codes(const ::hnsw_index *from, ::hnsw_index *to);

// Longest-first ordering of a large batch (hnsw_order.hip): runs the descent kernel and a radix sort
// on `st`; on success *block points to the handle's scratch for that stream (nothing to release)
// whose parts are returned in the other pointers.
// d_stage (optional): d_queries is the caller's registered HOST matrix seen from the device (zero-copy); the descent kernel
// then leaves a device-resident copy of every query there for the search kernel
int order_longest_first(::hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride, float *d_stage, hipStream_t st,
                        void **block, const int32_t **qmap, const int32_t **pre_entry, const uint32_t **pre_key,
                        const uint32_t **pre_nd, int32_t *pre_layer);

// hnsw_capi.hip: parameter / handle checks shared by every search entry point (HNSW_ERR_BAD_ARG, HNSW_ERR_EMPTY_INDEX, ...)
int check_params(const ::hnsw_index *idx, const hnsw_search_params *p);
// ... and of the batch entry points, in this order: the params and the handle, 0 <= nq <= INT32_MAX, then -- unless nq is 0, which
// passes -- the buffers (`buffers`: none of the required ones is null) and q_stride >= d
int check_batch(const ::hnsw_index *idx, const hnsw_search_params *p, int64_t nq, int64_t q_stride, bool buffers);
// hnsw_capi.hip: hnsw_search_batch_device for a KnnBatch, whose any_flag word (optional) collects status bit 0 of the launch.
// d_stage (optional, [nq][q_stride] device floats): b.Q points into registered host memory (see order_longest_first).
// While option "refine" is active or the index searches its sq8 rows (refine_count) the walk writes its first c members of W into
// `walk` (null: the handle's refine_scratch) and the re-rank kernel, queued behind it, writes b's ids, distances and evaluation
// counts.  Over sq8 rows the walk -- ordering pre-pass, device fallback and knn_repair's re-run included -- reads the queries in
// code space (walk->qt), the re-rank the caller's.
// raw_walk: no re-rank whatever the options say -- b receives the walk's own W[0..k) and counters (sq8 rows: the queries still go
// through walk->qt); what hnsw_search_batch_filtered masks and re-ranks itself (hnsw_filter.hip).
// collect (with raw_walk only; exact-row formats, p->k <= 128): the launch is the collect kernel's -- b receives R, the first p->k
// allowed nodes of all the walk of p->ef evaluates (option "filter_collect"), under the masks collect names.
int knn_search(::hnsw_index *idx, const hnsw_search_params *p, const KnnBatch &b, hipStream_t st, float *d_stage = nullptr,
               RefineBufs *walk = nullptr, bool raw_walk = false, const hnsw_dev::CollectArgs *collect = nullptr);
// hnsw_capi.hip: the exactness fallback of the host-buffer entry points (see rerun_overflowed) for a batch knn_search ran:
// rewrites the rows of the queries it flagged in b.st (refine active: their rows of `walk`, then the batch is re-ranked again)
int knn_repair(::hnsw_index *idx, const hnsw_search_params *p, const KnnBatch &b, hipStream_t st, RefineBufs *walk = nullptr,
               bool raw_walk = false, const hnsw_dev::CollectArgs *collect = nullptr);
// hnsw_rerank.hip: the re-rank kernel on `st` for device-resident arguments (hnsw_rerank_batch_device, unchecked); nd_out
// (optional): nd_out[q] = (nd_in ? nd_in[q] : 0) + the number of candidates evaluated
int launch_rerank(::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, const int32_t *cand, int32_t cand_stride, int32_t k,
                  int32_t fill, int32_t *out_ids, float *out_dist, const uint32_t *nd_in, uint32_t *nd_out, hipStream_t st);
// hnsw_diverse.hip: the selection kernel on `st` for device-resident arguments (hnsw_diversify_batch_device, unchecked; out_div optional)
int launch_diversify(::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, const int32_t *cand, int32_t cand_stride, int32_t k,
                     float lambda, int32_t fill, int32_t *out_ids, float *out_dist, float *out_div, hipStream_t st);
// hnsw_scan.hip: the exact scan of b's queries on `st` into b.ids / b.dist (hnsw_brute_force_batch_device, with its checks).  masks
// (optional, a device table of masks of ceil(n / 32) device words each): only the rows whose bit is set are candidates, in the mask
// of the query's tile -- masks[tile_filter[t]] for the t-th tile of scan_tile(NCH) queries (tile_filter: device, one entry per
// tile), masks[0] for every tile when tile_filter is null.  row_query (optional, device, [b.nq]): rows whose entry is negative are
// padding of the caller's layout; their rows of b.ids / b.dist are left unwritten.
int scan_search(::hnsw_index *idx, const KnnBatch &b, int32_t k, int32_t fill, hipStream_t st, const uint32_t *const *masks = nullptr,
                const int32_t *tile_filter = nullptr, const int32_t *row_query = nullptr);
// hnsw_scan.hip: what the exact scans check of a call, as check_batch does for the knn searches (k in 1..1024, the fill, nq, then -- unless
// nq is 0 -- the buffers and q_stride)
int check_scan(const ::hnsw_index *idx, int64_t nq, int64_t q_stride, int32_t k, int32_t fill, bool buffers);
// hnsw_scan.hip: how an exact scan of m queries of this index is cut (scan_plan: k for the slab rule, bytes per (query, slab)
// cell, the first piece's cap), the kernels' NCH and tile, and the grid of a launch of nq <= piece queries
struct ScanCut : ScanPlan {
    int nch = 0, T = 0;
    dim3 grid(int64_t nq) const;
};
ScanCut scan_cut(const ::hnsw_index *idx, int64_t m, int k, int64_t cell_bytes, int64_t cap);
// the walk reads codes (sq8 rows, per-dimension sq8 rows, bit rows): its queries are moved to the codes' space first, its distances mean
// nothing to a caller, and it always ends in the re-rank over the float32 rows
inline bool walks_codes(const ::hnsw_index *idx) {
    return idx->info.row_format == HNSW_ROWS_SQ8 || idx->info.row_format == HNSW_ROWS_SQ8_DIM || idx->info.row_format == HNSW_ROWS_BITS;
}
// ... and is either option on (even while byte rows stand in front of the codes)?  Its name, for messages
inline bool codes_on(const ::hnsw_index *idx) { return idx->sq8_on || idx->sq8d_on || idx->bit_mode != 0; }
inline const char *codes_option(const ::hnsw_index *idx) {
    if (idx->bit_mode != 0 || idx->info.row_format == HNSW_ROWS_BITS) return "bit_rows";
    return idx->sq8d_on || idx->info.row_format == HNSW_ROWS_SQ8_DIM ? "sq8_dim_rows" : "sq8_rows";
}
// ... does it walk the bit rows against the 4-bit query's planes (option bit_query_bits 4; the kernel's ROWS 7)?
inline bool walks_bit_planes(const ::hnsw_index *idx) { return idx->info.row_format == HNSW_ROWS_BITS && idx->bit_query_bits == 4; }
// floats (words) per row of the matrix the walk over codes reads its queries from (RefineBufs::qt) -- what its allocation, the
// transform and SearchArgs.q_stride share (walk_query_words, hnsw_bits_plan.h: the planes' rows have a stride of their own)
inline int64_t walk_query_stride(const ::hnsw_index *idx) { return walk_query_words(idx->iv.d, walks_bit_planes(idx)); }
inline int codes_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st) {
    if (walks_bit_planes(idx)) return bits_asym_transform_queries(idx, Q, nq, q_stride, Qt, stage, nullptr, st);
    if (idx->info.row_format == HNSW_ROWS_BITS) return bits_transform_queries(idx, Q, nq, q_stride, Qt, stage, st);
    return idx->info.row_format == HNSW_ROWS_SQ8_DIM ? sq8_dim_transform_queries(idx, Q, nq, q_stride, Qt, stage, st)
                                                     : sq8_transform_queries(idx, Q, nq, q_stride, Qt, stage, st);
}
// the walk's distances are not exact over X (half rows, codes): what is kept of W is re-ranked over the float32 rows
inline bool walk_is_inexact(const ::hnsw_index *idx) { return idx->info.row_format == HNSW_ROWS_HALF || walks_codes(idx); }
// the filter the unfiltered searches answer under: the live nodes while some are marked deleted, else none
inline const ::hnsw_filter *live_filter(const ::hnsw_index *idx) { return idx->n_deleted > 0 ? idx->live.get() : nullptr; }
// What every entry point checks of an object bound to a handle, its n and its graph epoch -- a filter, a labels object -- (null,
// foreign, outgrown, stale: HNSW_ERR_BAD_ARG); noun and plural: how the messages name it
template <class Bound> int check_bound(const ::hnsw_index *idx, const Bound *h, const char *noun, bool plural) {
    const char *const was = plural ? "were" : "was";
    if (!h) return fail(HNSW_ERR_BAD_ARG, "null %s", noun);
    if (h->idx != idx) return fail(HNSW_ERR_BAD_ARG, "the %s %s made for another index", noun, was);
    if (h->n != idx->iv.n)
        return fail(HNSW_ERR_BAD_ARG, "the %s %s made for %lld nodes, the index has grown to %lld", noun, was, (long long)h->n, (long long)idx->iv.n);
    if (h->epoch != idx->epoch)
        return fail(HNSW_ERR_BAD_ARG, "the %s %s made before the index last changed (hnsw_index_insert / hnsw_index_remove / hnsw_index_mark_deleted): %s stale",
                    noun, was, plural ? "they are" : "it is");
    return HNSW_OK;
}
inline int check_filter(const ::hnsw_index *idx, const ::hnsw_filter *f) { return check_bound(idx, f, "filter", false); }
inline int check_labels(const ::hnsw_index *idx, const ::hnsw_labels *l) { return check_bound(idx, l, "labels", true); }
// hnsw_filter.hip: a filter of idx's n nodes (and epoch) with its mask allocated (not initialised) and the mask's own address behind it
int new_filter(const ::hnsw_index *idx, int64_t n, std::unique_ptr<::hnsw_filter> &f);
// hnsw_filter.hip: f's n_allowed counted on the device (filter_popcount_kernel; the bits past n cleared); and_with (optional, device
// words): the mask is ANDed with it first
int count_filter(::hnsw_filter *f, const uint32_t *and_with);
// hnsw_soft_delete.hip: the live mask an index of n_new nodes gets when nx replaces idx's graph (adopt_graph, before the swap):
// new_id (host, [idx->iv.n], 0-based, -1 = removed; null: every node keeps its id and the nodes from idx->iv.n on are new and live).
// out stays null when idx has no marked node.
int renumbered_live_filter(const ::hnsw_index *idx, const int32_t *new_id, int64_t n_new, std::unique_ptr<::hnsw_filter> &out);
// hnsw_keys.hip: the key tables an index of n_new nodes gets when nx replaces idx's graph (adopt_graph, before the swap), lookup
// table included: new_id as above (keys_renumber_kernel; null: the old keys kept in place and append_keys, n_new - idx->iv.n of
// them, behind).  Both at once (the upsert): the survivors under new_id and append_keys, n_new - survivors of them, behind the
// survivors, in the same launch; one sort for the lookup table.  out stays null when idx has no keys and none are appended.
int renumbered_keys(const ::hnsw_index *idx, const int32_t *new_id, int64_t n_new, const int64_t *append_keys, std::unique_ptr<KeyTables> &out);
// hnsw_keys.hip: keys_translate_kernel on st: d_out[i] = the key of node d_ids[i] - id_base, or missing where that is no node (m entries)
int keys_translate(const ::hnsw_index *idx, const int32_t *d_ids, int64_t m, int64_t missing, int64_t *d_out, hipStream_t st);
// hnsw_filter.hip: the escalation the filtered, range, grouped and paged searches run -- e = ef, 2 ef, ... 1024: the batch is walked
// with (ef = k = e, raw_walk), the caller's select kernel serves what it can and appends the other queries to the short list
// (ladder_settle) and only those, gathered into one compact batch, are walked again.  run is the loop; a search is one stage body
// handed to it and what it does with the batch run leaves.  Everything is queued on st and waited for where the host needs a
// number (the tie-overflow word, the short count).  A failure returns with work queued: the entry points synchronise st before
// they return it.
// what run leaves for the exact stage: nothing (every query was served), or the batch (Qj, m, qs, map) -- `walked`: queries still
// short at e = 1024, their counters hold their walks'; `fresh`: nobody walked, the batch is still the caller's (exact_settle's fresh)
enum class LadderLeft { none, walked, fresh };
struct Ladder {
    ::hnsw_index *idx;
    const float *Q;                      // the caller's batch (device address) ...
    int64_t nq, q_stride;
    int32_t semantics;
    float *d_stage;                      // ... see knn_search
    hipStream_t st;
    const char *what;                    // the call's name in messages
    // the batch of the current stage: at first the caller's, later the short queries of the stage before, row i belonging to
    // query map[i] (null: to query i); after the ladder what is left for the exact stage
    const float *Qj;
    int64_t m, qs;
    const int32_t *map = nullptr;
    int e, stage = 0;
    KnnBatch wb{};                       // the stage's walk: W where the caller wants it, counters and status in the ladder's scratch
    uint32_t n_short = 0;
    // option "filter_collect" (set by the filtered search before the first walk): collect_k > 0: a stage's walk is the collect
    // kernel's, which writes [m][collect_k] rows -- R under masks[which[query]] -- instead of W's [m][e]
    int collect_k = 0;
    const uint32_t *const *collect_masks = nullptr;
    const int32_t *collect_which = nullptr;
    Ladder(::hnsw_index *idx_, const float *Q_, int64_t nq_, int64_t q_stride_, int ef, int32_t semantics_, float *d_stage_, hipStream_t st_,
           const char *what_)
        : idx(idx_), Q(Q_), nq(nq_), q_stride(q_stride_), semantics(semantics_), d_stage(d_stage_), st(st_), what(what_), Qj(Q_), m(nq_),
          qs(q_stride_), e(ef) {}
    // stage 0 for the `count` queries of `list` only (host, ascending): gathered, as a later stage's batch is
    int start_from(const int32_t *list, int64_t count);
    // The loop.  walks false: nobody walks, the batch goes to the exact stage as it is.  Else, until nobody is short or e cannot
    // grow: stage(*this, m, e) sizes the caller's buffers, walks and launches the caller's select kernel; the short queries are
    // counted and, if any, become the next stage's batch.  left: what is left for the exact stage.
    template <class Stage> int run(bool walks, Stage &&stage, LadderLeft &left) {
        left = walks ? LadderLeft::none : LadderLeft::fresh;
        for (bool more = walks; more;) {
            int rc;
            if ((rc = stage(*this, m, e)) || (rc = count_short())) return rc;
            if (n_short == 0) break;
            if ((rc = advance(more))) return rc;
            if (!more) left = LadderLeft::walked;
        }
        return HNSW_OK;
    }
    // W_e of the batch into wids / wdist ([m][e]): the host form's search of (ef = e, k = e), its tie-overflow repair included,
    // without a re-rank; the short counter zeroed; evals = the walk's evaluation counts
    int walk(int32_t *wids, float *wdist, int32_t fill);
    // W_e of the batch OVER THE FLOAT32 ROWS into Wi / Wd ([m][e]): walk, and for half rows and codes -- whose walk lands in the
    // ladder's own cand / cdist -- the re-rank of all its members (launch_rerank with k := e); evals = the evaluations of both.
    // The two halves apart, for a caller that turns some of wb.ids into padding between them (the grouped search).
    int walk_exact(int32_t *Wi, float *Wd, int32_t fill) {
        const int rc = walk_raw(Wi, Wd, fill);
        return rc ? rc : rerank_all(Wi, Wd, fill);
    }
    int walk_raw(int32_t *Wi, float *Wd, int32_t fill);
    int rerank_all(int32_t *Wi, float *Wd, int32_t fill);
    const uint32_t *evals = nullptr;     // [m] the stage's evaluations to add: what out() hands ladder_settle
    // what the select kernel's ladder_settle takes
    hnsw_dev::LadderOut out(uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_stage) const;
    // after the select kernel: n_short, read once per walk (a stage body that needs the number may ask before run does)
    int count_short();
    // the queries of the batch the last stage left (host, ascending)
    const std::vector<int32_t> &batch_queries() const { return shorts; }
private:
    // the n_short > 0 short queries, ascending, become the batch; false: they were short at e = 1024, the ladder is over
    int advance(bool &more);
    int gather();                        // the m queries of `map` become the rows of the ladder's own matrix
    int cur = 0;                         // which list buffer `map` is
    bool counted = false;                // n_short is this walk's
    std::vector<int32_t> shorts;
};
// hnsw_filter.hip: filter_scatter_kernel on st, one wave per row of a; what: the kernel's name in a launch failure's message
int scatter_rows(const hnsw_dev::ScatterArgs &a, hipStream_t st, const char *what);
// hnsw_capi.hip: hnsw_search_batch; ko (optional): the rows go to ko->keys as keys and out_ids may be null (hnsw_search_batch_keyed);
// out_stage (optional): as the filtered call writes it while nodes are marked, zero otherwise
// rows (optional; queries is then null and q_stride padded_stride(d)): the queries are rows of the index, gathered on the device
// (RowsIn; hnsw_search_batch_by_id)
// dv (optional; out_ids and out_dist are then null and params->k is the pool): the rows stay on the device and the selection's go to
// dv's arrays (DiverseOut; hnsw_search_batch_diverse)
int knn_host_call(::hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params, int32_t *out_ids,
                  float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage, const KeysOut *ko, const RowsIn *rows = nullptr,
                  const DiverseOut *dv = nullptr);
// hnsw_filter.hip: hnsw_search_batch_filtered; ko, dv: likewise
int filtered_host_call(::hnsw_index *idx, const ::hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params,
                       int32_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage, const KeysOut *ko,
                       const RowsIn *rows = nullptr, const DiverseOut *dv = nullptr);
// hnsw_capi.hip: the value that puts option `name` of hnsw_index_set_option back where it is now (HNSW_ERR_BAD_ARG: no such option)
int get_option(const ::hnsw_index *idx, const char *name, int64_t *value);
// hnsw_capi.hip: queues the copies of a batch's results into the host arrays that are not null
hipError_t knn_download(const KnnBatch &b, int k, int32_t *ids, float *dist, uint32_t *nd, uint32_t *nh, hipStream_t st);
// hnsw_capi.hip: the handle's stream (hs[0]) and flag word of the host-buffer calls, made on first use
int ensure_host_call_state(::hnsw_index *idx);

// hnsw_capi.hip: where the device reads the host array [p, p + bytes): in place when it lies in a range of hnsw_host_alloc /
// hnsw_host_register, else in `stage`, grown to hold it (resolve: allocates, queues nothing), after upload has queued the copy
// ... or, a third source, ROWS OF THE INDEX: dev is `stage`, sized for nq rows of padded_stride(d) floats (resolve_rows: allocates,
// queues nothing), which upload fills by the gather kernel behind the upload of the nq ids (hnsw_by_id.hip) -- no row crosses the link
struct HostInput {
    const void *dev = nullptr, *from = nullptr;     // from: the host array while it still has to be copied to dev, else null
    size_t bytes = 0;
    ::hnsw_index *rows_of = nullptr;                // rows of this index: their ids on the host, where those go on the device, how many
    const int32_t *row_ids = nullptr;
    int32_t *d_row_ids = nullptr;
    int64_t n_rows = 0;
    int resolve(const void *p, size_t n, DevBuf &stage);
    int resolve_rows(::hnsw_index *idx, const int32_t *ids, int64_t nq, DevBuf &stage);
    int upload(hipStream_t st) const;
};
// hnsw_by_id.hip: the gather kernel on `st`: row j of d_out (out_stride floats apart) = the first `width` floats of the float32 row
// of node d_ids[j] - id_base (tables.X; width <= padded_stride(d)), zeros where that is no node
int gather_rows(const ::hnsw_index *idx, const int32_t *d_ids, int64_t m, int32_t width, float *d_out, int64_t out_stride, hipStream_t st);
// hnsw_by_id.hip: the drop-self epilogue on `st` over the inner rows d_ids / d_dist [nq][k + 1]: the [nq][k] rows with each query's
// own id (d_self [nq]) removed into out_dist and out_ids -- or, out_keys not null, into out_keys as the index's keys
// (hnsw_index_keys_of's rule with `missing`).  The outputs may be page-locked host matrices seen from the device.
int drop_self_rows(const ::hnsw_index *idx, const int32_t *d_ids, const float *d_dist, const int32_t *d_self, int64_t nq, int32_t k,
                   int32_t *out_ids, int64_t *out_keys, int64_t missing, float *out_dist, hipStream_t st);
// hnsw_keys.hip: the 0-based nodes of m keys of a keyed handle (host arrays; -1: no node has the key)
int keys_find_nodes(const ::hnsw_index *idx, const int64_t *keys, int64_t m, std::vector<int32_t> &nodes);
// hnsw_capi.hip: the matrices of one synchronous host-buffer call on the handle's stream hs[0] (rules: beside HostCall::begin)
struct HostCall {
    KnnBatch b{};                                   // what the kernels read and write
    int k = 0;
    bool small = false;                             // the handle's page-locked block holds the queries and every result
    // the caller's arrays that finish still has to fill -- by download, `small`: out of the block --, null where the device
    // writes in place (or the caller passed none)
    int32_t *ids = nullptr;
    float *dist = nullptr;
    uint32_t *nd = nullptr, *nh = nullptr;
    // a keyed call (set before begin, out_ids then null): finish translates the device-resident ids into the handle's key_scratch
    // and downloads that into ko->keys; such a call never takes the small block
    const KeysOut *ko = nullptr;
    // the queries are rows of the index (set before begin, `queries` then null and q_stride padded_stride(d)): begin gathers them
    // into scratch.q and from there the call is the device-resident one, as a COSINE call is -- no head split, no zero-copy reads,
    // no small block.  rows->drop_self: begin's k is the inner k + 1, the kernels write scratch, and finish runs the drop-self
    // epilogue over it into drop_ids (or drop_keys) / drop_dist -- the caller's page-locked matrices in place, else the handle's
    // by_id_scratch / key_scratch, downloaded from there
    const RowsIn *rows = nullptr;
    // a diverse call (set before begin, out_ids and out_dist then null, k the pool): finish runs the selection over the device-resident
    // rows into the handle's diverse_scratch and downloads that into dv's arrays; such a call never takes the small block
    const DiverseOut *dv = nullptr;
    int32_t *drop_ids = nullptr;
    int64_t *drop_keys = nullptr;
    float *drop_dist = nullptr;
    // *q_in_place: the device reads the queries from host memory (the knn call then hands knn_search scratch.q to stage them in)
    int begin(::hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int k, int32_t *out_ids, float *out_dist,
              uint32_t *out_nd, uint32_t *out_nh, bool allow_small, bool *q_in_place = nullptr);
    // the results into those arrays: the download queued on st, ONE synchronisation (of st; null: of the device), the copy out of
    // the block; a failed synchronisation reads "<what> failed: ..."
    int finish(::hnsw_index *idx, const char *what, hipStream_t st);
};
// a further [nq][..] column a ladder host call downloads from the handle's scratch (the grouped calls' labels)
struct HostColumn {
    void *host;
    const DevBuf *dev;
    size_t bytes;
    const char *noun;                               // in "<noun> download failed"
};
// The frame of the filtered, grouped and paged host calls, graph and brute-force forms: HostCall::begin (ko / rows / dv: see HostCall),
// body(batch, d_stage, st) -- d_stage: see knn_search -- on the handle's stream, the downloads of `extra` (optional) and of
// out_stage (optional; from filter_scratch.stage), then finish(what).  An error after begin waits for the stream before it returns.
template <class Body>
int ladder_host_call(::hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int k, int32_t *out_ids, float *out_dist,
                     uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_stage, bool allow_small, const KeysOut *ko, const RowsIn *rows,
                     const DiverseOut *dv, const HostColumn *extra, const char *what, Body &&body) {
    HostCall c;
    c.ko = ko;
    c.rows = rows;
    c.dv = dv;
    bool q_in_place = false;
    int rc;
    if ((rc = c.begin(idx, queries, nq, q_stride, k, out_ids, out_dist, out_nd, out_nh, allow_small, &q_in_place))) return rc;
    hipStream_t st = idx->hs[0];
    // (from here on copies are queued that read the caller's arrays: no return without a synchronisation)
    rc = body(c.b, q_in_place ? (float *)idx->scratch.q.p : nullptr, st);
    if (!rc && extra && hipMemcpyAsync(extra->host, extra->dev->p, extra->bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(HNSW_ERR_HIP, "%s download failed", extra->noun);
    if (!rc && out_stage && hipMemcpyAsync(out_stage, idx->filter_scratch.stage.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(HNSW_ERR_HIP, "stage download failed");
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    return c.finish(idx, what, st);
}

// log2 entries of the per-query LDS visited cache (never changes results)
inline int search_vt_bits(const hnsw_index *idx, int ef) {
    int b = idx->vt_bits_override;
    if (b <= 0) {
        // Re-encounters of a node come soon after its first evaluation, so the cache need not
        // grow with ef: 2^11 tags (4 KiB, 32 waves/CU) cost 3.5 % re-evaluations on C2 and 2.6 %
        // at ef = 512 (measured), while 2^13 halves the resident waves.  One step more once the
        // W registers cap the occupancy anyway.
        b = ef <= 256 ? 11 : 12;
    }
    b = std::max(4, std::min(16, b));
    while (b < 16 && ((int64_t)0xFFFF << (b - 1)) < idx->iv.n) ++b;   // 16-bit tags must identify ids exactly, 0xFFFF = empty way
    return b;
}

// Exactness fallback of the host-buffer entry points: a query whose stack of tied, evicted, still
// expandable entries outgrew its 64 LDS slots (status bit 0) is searched again with a global slab
// that can hold every node.  launch(qmap, count, slab, slab_cap) starts the kernel for `count`
// flagged queries; it is synchronised here.
template <class Launch>
int rerun_overflowed(hnsw_index *idx, int64_t nq, const uint32_t *d_status, Launch &&launch) {
    std::vector<uint32_t> st((size_t)nq);
    HIP_TRY(hipMemcpy(st.data(), d_status, (size_t)nq * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> flagged;
    for (int64_t i = 0; i < nq; ++i) if (st[(size_t)i] & 1u) flagged.push_back((int32_t)i);
    if (flagged.empty()) return HNSW_OK;
    const int64_t n = idx->iv.n;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(256, (512ll << 20) / (n * 4 + 1)));
    DevBuf dMap, dSlab;
    int rc;
    if ((rc = dMap.ensure((size_t)chunk * 4)) || (rc = dSlab.ensure((size_t)chunk * n * 4))) return rc;
    for (size_t f0 = 0; f0 < flagged.size(); f0 += (size_t)chunk) {
        const int64_t c = (int64_t)std::min<size_t>((size_t)chunk, flagged.size() - f0);
        HIP_TRY(hipMemcpy(dMap.p, flagged.data() + f0, (size_t)c * 4, hipMemcpyHostToDevice));
        if ((rc = launch((const int32_t *)dMap.p, c, (uint32_t *)dSlab.p, (int32_t)n))) return rc;
        HIP_TRY(hipDeviceSynchronize());
    }
    return HNSW_OK;
}

} // namespace hnsw_host
