// hnsw_sharded.hip -- one data set PARTITIONED over several GPUs: each listed device holds a slice of the rows with a graph of its
// own, every query visits all slices, and the per-slice answers are merged on the first device under the library's total order
// (distance, global id).  hnsw_multi (hnsw_multi.hip) replicates the index and splits the batch: that scales throughput; this
// scales capacity.  The structure of a call is search_and_gather's: per-device streams, one flag word per device, a single host
// round trip, knn_repair for a flagged shard -- with peer copies to devices[0] and the merge kernel where hnsw_multi has its
// exchange.  No RCCL: the copies are 8 bytes * nq * k per shard.
#include "hnsw_internal.h"

using namespace hnsw_host;

namespace hnsw_dev {

constexpr int MERGE_LISTS = 64;          // one lane per list: the wave width

// n_lists lists per query, each [nq][k_in], ascending under (distance, id), padding (id < id_base) at the end
struct MergeArgs {
    const int32_t *ids;                  // [n_lists][nq][k_in], id_base-based ids local to the list
    const float *dist;                   // [n_lists][nq][k_in]
    const uint32_t *nd, *nh;             // [n_lists][nq] counters to sum per query, or null
    int64_t nq;
    int32_t n_lists, k_in, k_out, id_base, fill;
    int64_t *out_ids;                    // [nq][k_out]: first_row[list] + id
    float *out_dist;                     // [nq][k_out]
    uint32_t *out_nd, *out_nh;           // [nq], written when nd / nh are given
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
}

} // namespace hnsw_dev

struct hnsw_sharded {
    std::vector<hnsw_index *> shards;
    std::vector<int> devices;
    std::vector<int64_t> lo;             // [G + 1]: shard g holds the rows [lo[g], lo[g + 1])
    std::vector<Stream> streams;         // [G], made by the first search
    std::vector<Event> done;             // [G] "shard g's search is enqueued up to here": what the copies to devices[0] wait for
    std::vector<BatchBufs> buf;          // [G] on its device: the whole batch, its [nq][k] results, counters and flag word
    Pinned<uint32_t> hFlags;             // [G] the launches' "any query flagged" words on the host
    // on devices[0]: every shard's results and counters ([G][nq][k], [G][nq]) and the merged rows.  One call in flight per handle.
    DevBuf gIds, gDist, gNd, gNh, mIds, mDist, mNd, mNh;
};

namespace {

using hnsw_dev::MergeArgs;
using hnsw_dev::MERGE_LISTS;

int launch_merge(const MergeArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(hnsw_dev::hnsw_merge_lists_kernel, dim3((unsigned)a.nq), dim3(MERGE_LISTS), 0, st, a);
    return launched("merge kernel");
}

int ensure_streams(hnsw_sharded *s) {
    const size_t G = s->shards.size();
    if (s->streams.size() == G) return HNSW_OK;
    s->streams.clear(); s->done.clear();
    s->buf.resize(G);
    if (!s->hFlags) HIP_TRY(s->hFlags.alloc(G * sizeof(uint32_t), hipHostMallocPortable));
    std::vector<Stream> streams(G);
    std::vector<Event> done(G);
    for (size_t g = 0; g < G; ++g) {
        HIP_TRY(hipSetDevice(s->devices[g]));
        HIP_TRY(hipStreamCreateWithFlags(&streams[g].h, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&done[g].h, hipEventDisableTiming));
    }
    s->streams = std::move(streams); s->done = std::move(done);
    return HNSW_OK;
}

int sync_all(hnsw_sharded *s) {
    int rc = HNSW_OK;
    for (size_t g = 0; g < s->streams.size(); ++g) {
        hipError_t e = hipSetDevice(s->devices[g]);
        if (e == hipSuccess) e = hipStreamSynchronize(s->streams[g]);
        if (e != hipSuccess && !rc) rc = hip_fail(e, "hipStreamSynchronize");
    }
    return rc;
}

// shard g's [nq][k] results (and its counters, with_counters) into its slice of the tables on devices[0], on devices[0]'s stream
int copy_shard(hnsw_sharded *s, int g, int64_t nq, int k, bool with_counters) {
    const int d0 = s->devices[0], dg = s->devices[(size_t)g];
    const BatchBufs &b = s->buf[(size_t)g];
    hipStream_t st = s->streams[0];
    const size_t rows = (size_t)nq * k, rbytes = rows * 4, cbytes = (size_t)nq * 4;
    HIP_TRY(hipMemcpyPeerAsync((int32_t *)s->gIds.p + (size_t)g * rows, d0, b.ids.p, dg, rbytes, st));
    HIP_TRY(hipMemcpyPeerAsync((float *)s->gDist.p + (size_t)g * rows, d0, b.dist.p, dg, rbytes, st));
    if (with_counters) {
        HIP_TRY(hipMemcpyPeerAsync((uint32_t *)s->gNd.p + (size_t)g * nq, d0, b.nd.p, dg, cbytes, st));
        HIP_TRY(hipMemcpyPeerAsync((uint32_t *)s->gNh.p + (size_t)g * nq, d0, b.nh.p, dg, cbytes, st));
    }
    return HNSW_OK;
}

// Every shard answers the whole batch on its own device and stream (`search`: what is queued on shard g's stream behind the
// upload), the answers go to devices[0] behind an event, after the one host round trip `repair` re-does a flagged shard, then the
// merge and the download.  Both sharded entry points.
template <class Search, class Repair>
int search_and_merge(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, int k, int32_t fill, bool with_counters,
                     int64_t *out_ids, float *out_dist, uint32_t *out_nd, uint32_t *out_nh, Search &&search, Repair &&repair) {
    const int G = (int)s->shards.size();
    const int d = s->shards[0]->iv.d;
    const size_t qbytes = query_bytes(nq, q_stride, d), rows = (size_t)nq * k;
    int rc;
    // ---- every allocation first: nothing below returns with work queued that it does not wait for ----
    if ((rc = ensure_streams(s))) return rc;
    for (int g = 0; g < G; ++g) {
        HIP_TRY(hipSetDevice(s->devices[(size_t)g]));
        if ((rc = s->buf[(size_t)g].ensure(nq, qbytes, k))) return rc;
    }
    HIP_TRY(hipSetDevice(s->devices[0]));
    if ((rc = s->gIds.ensure((size_t)G * rows * 4)) || (rc = s->gDist.ensure((size_t)G * rows * 4)) || (rc = s->gNd.ensure((size_t)G * nq * 4)) ||
        (rc = s->gNh.ensure((size_t)G * nq * 4)) || (rc = s->mIds.ensure(rows * 8)) || (rc = s->mDist.ensure(rows * 4)) ||
        (rc = s->mNd.ensure((size_t)nq * 4)) || (rc = s->mNh.ensure((size_t)nq * 4)))
        return rc;
    auto queued = [&]() -> int {
        for (int g = 0; g < G; ++g) {
            const BatchBufs &b = s->buf[(size_t)g];
            hipStream_t st = s->streams[(size_t)g];
            HIP_TRY(hipSetDevice(s->devices[(size_t)g]));
            s->hFlags[g] = 0;
            const KnnBatch batch = b.batch(nq, q_stride, k);
            HIP_TRY(hipMemsetAsync(batch.any_flag, 0, 4, st));
            HIP_TRY(hipMemcpyAsync(b.q.p, queries, qbytes, hipMemcpyHostToDevice, st));
            int r = search(s->shards[(size_t)g], batch, st);
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(&s->hFlags[g], batch.any_flag, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(s->done[(size_t)g], st));
        }
        // the copies run on devices[0]'s stream, each behind its shard's search
        HIP_TRY(hipSetDevice(s->devices[0]));
        for (int g = 0; g < G; ++g) {
            hipEvent_t ev = s->done[(size_t)g];
            HIP_TRY(hipStreamWaitEvent(s->streams[0], ev, 0));
            int r = copy_shard(s, g, nq, k, with_counters);
            if (r) return r;
        }
        return HNSW_OK;
    };
    rc = queued();
    const int rs = sync_all(s);             // the one host round trip (also after a failure: nothing stays queued)
    if (rc || (rc = rs)) return rc;
    for (int g = 0; g < G; ++g) {
        if (!(s->hFlags[g] & 1u)) continue;
        // (rare) the shard's launch flagged a tie overflow: its flagged queries are searched again, complete on return, and the
        // shard's rows are sent once more
        HIP_TRY(hipSetDevice(s->devices[(size_t)g]));
        if ((rc = repair(s->shards[(size_t)g], s->buf[(size_t)g].batch(nq, q_stride, k)))) return rc;
        HIP_TRY(hipSetDevice(s->devices[0]));
        if ((rc = copy_shard(s, g, nq, k, with_counters))) { (void)sync_all(s); return rc; }
    }
    HIP_TRY(hipSetDevice(s->devices[0]));
    hipStream_t st = s->streams[0];
    MergeArgs a{(const int32_t *)s->gIds.p, (const float *)s->gDist.p, with_counters ? (const uint32_t *)s->gNd.p : nullptr,
                with_counters ? (const uint32_t *)s->gNh.p : nullptr, nq, G, k, k, s->shards[0]->iv.id_base, fill,
                (int64_t *)s->mIds.p, (float *)s->mDist.p, (uint32_t *)s->mNd.p, (uint32_t *)s->mNh.p, {}};
    for (int g = 0; g < G; ++g) a.first_row[g] = s->lo[(size_t)g];
    rc = launch_merge(a, st);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(out_ids, s->mIds.p, rows * 8, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(out_dist, s->mDist.p, rows * 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess && with_counters && out_nd) e = hipMemcpyAsync(out_nd, s->mNd.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess && with_counters && out_nh) e = hipMemcpyAsync(out_nh, s->mNh.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "result download");
    if (es != hipSuccess) return hip_fail(es, "sharded search");
    return HNSW_OK;
}

int check_shard_count(int32_t n_shards) {
    if (n_shards < 1 || n_shards > MERGE_LISTS) return fail(HNSW_ERR_BAD_ARG, "n_shards=%d must be in 1..64", n_shards);
    return HNSW_OK;
}

// idx becomes the next shard of s (which owns it from here on): every shard agrees with the first on d, metric and id_base
int adopt_shard(hnsw_sharded *s, hnsw_index *idx, int device) {
    idx->multi_replica = true;           // never grown, shrunk or marked on its own: every later shard's first_row would move
    s->shards.push_back(idx);
    s->devices.push_back(device);
    s->lo.push_back(s->lo.back() + idx->iv.n);
    const hnsw_index *first = s->shards[0];
    if (idx->iv.d != first->iv.d || idx->info.metric != first->info.metric || idx->iv.id_base != first->iv.id_base)
        return fail(HNSW_ERR_BAD_ARG, "shard %d (d=%d metric=%d id_base=%d) does not agree with shard 0 (d=%d metric=%d id_base=%d)",
                    (int)s->shards.size() - 1, idx->iv.d, idx->info.metric, idx->iv.id_base, first->iv.d, first->info.metric, first->iv.id_base);
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

} // namespace

extern "C" {

int32_t hnsw_sharded_build(const float *vectors, int64_t n, int32_t d, int64_t row_stride, const hnsw_build_params *params,
                           const int32_t *devices, int32_t n_shards, hnsw_sharded **out) {
    if (out) *out = nullptr;
    if (!vectors || !params || !devices || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    int rc = check_shard_count(n_shards);
    if (rc) return rc;
    if (n < n_shards) return fail(HNSW_ERR_BAD_ARG, "n=%lld < n_shards=%d: a shard would be empty", (long long)n, n_shards);
    auto lo = [&](int g) { return (int64_t)((__int128)n * g / n_shards); };      // sharding.shard_bounds
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
    (void)sync_all(s);
    for (size_t g = 0; g < s->buf.size(); ++g) {
        (void)hipSetDevice(s->devices[g]);
        s->buf[g].release();
        if (g < s->streams.size()) s->streams[g].reset();
        if (g < s->done.size()) s->done[g].reset();
    }
    for (hnsw_index *idx : s->shards) (void)hnsw_index_destroy(idx);
    delete s;
    return HNSW_OK;
}

int32_t hnsw_sharded_num_shards(const hnsw_sharded *s, int32_t *n_shards) {
    if (!s || !n_shards) return fail(HNSW_ERR_BAD_ARG, "null argument");
    *n_shards = (int32_t)s->shards.size();
    return HNSW_OK;
}

int32_t hnsw_sharded_shard(hnsw_sharded *s, int32_t g, hnsw_index **out, int64_t *first_row) {
    if (!s || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (g < 0 || g >= (int32_t)s->shards.size()) return fail(HNSW_ERR_BAD_ARG, "shard %d out of range", g);
    *out = s->shards[(size_t)g];
    if (first_row) *first_row = s->lo[(size_t)g];
    return HNSW_OK;
}

int32_t hnsw_sharded_get_info(const hnsw_sharded *s, int64_t *n, int32_t *d, int32_t *metric, int32_t *id_base, int64_t *device_bytes) {
    if (!s) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    int64_t bytes = 0;
    for (const hnsw_index *idx : s->shards) {
        hnsw_index_info info;
        const int rc = hnsw_index_get_info(idx, &info);
        if (rc) return rc;
        bytes += info.device_bytes;
    }
    if (n) *n = s->lo.back();
    if (d) *d = s->shards[0]->iv.d;
    if (metric) *metric = s->shards[0]->info.metric;
    if (id_base) *id_base = s->shards[0]->iv.id_base;
    if (device_bytes) *device_bytes = bytes;
    return HNSW_OK;
}

int32_t hnsw_sharded_set_option(hnsw_sharded *s, const char *name, int64_t value) {
    if (!s || !name) return fail(HNSW_ERR_BAD_ARG, "null argument");
    std::vector<int64_t> before(s->shards.size(), 0);
    for (size_t g = 0; g < s->shards.size(); ++g) {
        int rc = get_option(s->shards[g], name, &before[g]);
        if (!rc) rc = hnsw_index_set_option(s->shards[g], name, value);
        if (rc) {
            const std::string msg = hnsw_last_error();          // shard g's refusal is what the caller reads
            for (size_t h = 0; h < g; ++h) (void)hnsw_index_set_option(s->shards[h], name, before[h]);
            return fail(rc, "%s", msg.c_str());
        }
    }
    return HNSW_OK;
}

int32_t hnsw_sharded_search_batch(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params,
                                  int64_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops) {
    if (!s || s->shards.empty()) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    int rc = check_batch(s->shards[0], params, nq, q_stride, queries && out_ids && out_dist);
    if (rc) return rc;
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "HNSW_SEM_FUNCTOR_NEAREST_K: the k farthest of W have no merged meaning over shards");
    for (size_t g = 1; g < s->shards.size(); ++g) if ((rc = check_params(s->shards[g], params))) return rc;   // (an empty shard)
    if (nq == 0) return HNSW_OK;
    return search_and_merge(
        s, queries, nq, q_stride, params->k, params->fill, true, out_ids, out_dist, out_ndist, out_nhops,
        [&](hnsw_index *idx, const KnnBatch &b, hipStream_t st) { return knn_search(idx, params, b, st); },
        [&](hnsw_index *idx, const KnnBatch &b) { return knn_repair(idx, params, b, nullptr); });
}

int32_t hnsw_sharded_brute_force_batch(hnsw_sharded *s, const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                                       int64_t *out_ids, float *out_dist) {
    if (!s || s->shards.empty()) return fail(HNSW_ERR_BAD_ARG, "null hnsw_sharded");
    const int rc = check_scan(s->shards[0], nq, q_stride, k, fill, queries && out_ids && out_dist);
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
    MergeArgs a{(const int32_t *)dIds.p, (const float *)dDist.p, nullptr, nullptr, nq, n_lists, k_in, k_out, id_base, fill,
                (int64_t *)oIds.p, (float *)oDist.p, nullptr, nullptr, {}};
    for (int g = 0; g < n_lists; ++g) a.first_row[g] = first_row[g];
    if ((rc = launch_merge(a, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out_ids, oIds.p, rows * 8, hipMemcpyDeviceToHost));       // (the null stream: behind the kernel)
    HIP_TRY(hipMemcpy(out_dist, oDist.p, rows * 4, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

} // extern "C"
