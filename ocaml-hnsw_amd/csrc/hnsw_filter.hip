// hnsw_filter.hip -- filtered k-NN search: an allow-mask over the nodes (hnsw_filter_*) and hnsw_search_batch_filtered, which
// composes pieces that exist already -- the unchanged walk (knn_search with k := ef: W stays on the device), the re-rank kernel
// (hnsw_rerank.hip) and the exact scan (hnsw_scan.hip, its masked form) -- into the definition the header gives:
//   ladder   e = ef, 2 ef, ... 1024: a query is served at the first e whose W holds k allowed nodes; only the queries still short
//            are walked again, gathered into one compact batch;
//   exact    a query still short at e = 1024, and every query when fewer than k nodes are allowed, gets the masked exact scan.
// The ladder itself (Ladder: the walk of a stage, the short list, the gathered batch) is here too; the range search
// (hnsw_range.hip) runs the same one with its own select rule.
//
// Kernels.
//   filter_popcount_kernel  the uploaded mask: clears the bits past n in its last word and counts the rest.
//   filter_select_kernel    one wave per walked query: tests the bit of each member of W, 64 entries per pass (ballot, prefix
//                           count).  A query with k allowed members is SERVED: its first k allowed (id, distance) pairs go to its
//                           output row (rows whose walk distances are exact over X: float32, bytes, split), or its W with the
//                           disallowed entries turned into padding goes to the re-rank's candidate matrix (half, sq8).  Others
//                           are appended to the short list (ladder_settle).
//   ladder_gather_kernel    the short queries' vectors as one compact, zero-padded matrix: the next walk's / the exact stage's batch.
//   filter_scatter_kernel   rows of a compact result (re-rank, scan) to the rows of the queries they belong to.
// No LDS, vector stores only.  All scratch is the handle's (LadderBufs, FilterBufs): one filtered or range call in flight per handle.
#include "hnsw_internal.h"

namespace hnsw_dev {

__global__ void __launch_bounds__(256)
filter_popcount_kernel(uint32_t *bits, int64_t words, int64_t n, unsigned long long *count) {
    int c = 0;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
        uint32_t v = bits[w];
        if (w == words - 1 && (n & 31)) {           // positions >= n of the last word are not nodes
            v &= (1u << (n & 31)) - 1u;
            bits[w] = v;
        }
        c += __builtin_popcount(v);
    }
    for (int s = 32; s > 0; s >>= 1) c += __shfl_down(c, s, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

struct SelectArgs {
    const int32_t *wids;       // [m][e] the walk's W per query, id_base-based, filled entries < id_base
    const float *wdist;        // [m][e]
    int64_t m;
    int32_t e, k;
    const int32_t *map;        // [m] row i belongs to query map[i]; null: to query i
    const uint32_t *bits;      // the mask
    int64_t n;
    int32_t id_base;
    int32_t *out_ids;          // [nq][k]
    float *out_dist;
    int32_t *cand;             // null, or [m][e]: the re-rank's candidates instead of out_ids / out_dist
    int32_t *cnt;              // [m] allowed members of W
    LadderOut out;
};

__device__ __forceinline__ bool filter_allows(const SelectArgs &a, int32_t id) {
    const int64_t v = (int64_t)id - a.id_base;
    return v >= 0 && v < a.n && ((a.bits[v >> 5] >> (v & 31)) & 1u);
}

__global__ void __launch_bounds__(64)
filter_select_kernel(const SelectArgs a) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= a.m) return;
    const int64_t q = a.map ? a.map[i] : i;
    const int32_t *const wi = a.wids + i * a.e;
    int cnt = 0;
    for (int j0 = 0; j0 < a.e; j0 += 64) {
        const int j = j0 + lane;
        cnt += popc(ballot(j < a.e && filter_allows(a, wi[j])));
    }
    const bool served = cnt >= a.k;
    if (a.cand) {               // W with everything but a served query's allowed members as padding
        for (int j = lane; j < a.e; j += 64) {
            const int32_t id = wi[j];
            a.cand[i * a.e + j] = served && filter_allows(a, id) ? id : a.id_base - 1;
        }
    } else if (served) {        // the first k allowed members, in W's order
        int at = 0;
        for (int j0 = 0; j0 < a.e && at < a.k; j0 += 64) {
            const int j = j0 + lane;
            const int32_t id = j < a.e ? wi[j] : a.id_base - 1;
            const bool ok = j < a.e && filter_allows(a, id);
            const uint64_t m = ballot(ok);
            const int pos = at + popc(m & ((1ull << lane) - 1ull));
            if (ok && pos < a.k) {
                a.out_ids[q * a.k + pos] = id;
                a.out_dist[q * a.k + pos] = a.wdist[i * a.e + j];
            }
            at += popc(m);
        }
    }
    if (lane == 0) {
        a.cnt[i] = cnt;
        ladder_settle(a.out, i, q, served);
    }
}

// out[i] = Q[list[i]], rows of out_stride floats, zero beyond d
__global__ void __launch_bounds__(64)
ladder_gather_kernel(const float *Q, int64_t q_stride, int32_t d, const int32_t *list, int64_t m, float *out, int64_t out_stride) {
    const int64_t i = blockIdx.x;
    if (i >= m) return;
    const float *qp = Q + (int64_t)list[i] * q_stride;
    for (int64_t c = threadIdx.x; c < out_stride; c += 64) out[i * out_stride + c] = c < d ? qp[c] : 0.f;
}

struct ScatterArgs {
    const int32_t *rids;       // [m][k] compact results
    const float *rdist;
    int64_t m;
    int32_t k;
    const int32_t *map;        // [m] row i belongs to query map[i]; null: to query i
    const int32_t *cnt;        // null: every row; else only the rows with cnt[i] >= k (the served ones)
    const uint32_t *add;       // null, or [m]: evaluations to add to out_nd
    uint32_t add_const;        // ... plus this many
    int32_t fresh;             // 1: the query took no walk: out_nd starts from 0 and out_nh is 0
    int32_t set_stage;         // 1: out_stage[q] = stage
    uint32_t stage;
    int32_t *out_ids;          // [nq][k]
    float *out_dist;
    uint32_t *out_nd, *out_nh, *out_stage;
};

__global__ void __launch_bounds__(64)
filter_scatter_kernel(const ScatterArgs a) {
    const int64_t i = blockIdx.x;
    if (i >= a.m || (a.cnt && a.cnt[i] < a.k)) return;
    const int64_t q = a.map ? a.map[i] : i;
    for (int j = threadIdx.x; j < a.k; j += 64) {
        a.out_ids[q * a.k + j] = a.rids[i * a.k + j];
        a.out_dist[q * a.k + j] = a.rdist[i * a.k + j];
    }
    if (threadIdx.x == 0) {
        a.out_nd[q] = (a.fresh ? 0u : a.out_nd[q]) + (a.add ? a.add[i] : 0u) + a.add_const;
        if (a.fresh) a.out_nh[q] = 0u;
        if (a.set_stage) a.out_stage[q] = a.stage;
    }
}

} // namespace hnsw_dev

using hnsw_dev::IndexView;
using namespace hnsw_host;

namespace hnsw_host {

int Ladder::walk(int32_t *wids, float *wdist, int32_t fill) {
    LadderBufs &lb = idx->ladder_scratch;
    int rc;
    if ((rc = lb.wnd.ensure((size_t)m * 4)) || (rc = lb.wnh.ensure((size_t)m * 4)) || (rc = lb.wst.ensure((size_t)m * 4)) ||
        (rc = lb.list[0].ensure((size_t)nq * 4)) || (rc = lb.list[1].ensure((size_t)nq * 4)) || (rc = lb.count.ensure(16)))
        return rc;
    const hnsw_search_params wp{e, e, fill, semantics};
    wb = KnnBatch{Qj, m, qs, wids, wdist, (uint32_t *)lb.wnd.p, (uint32_t *)lb.wnh.p, (uint32_t *)lb.wst.p, idx->hFlagDev};
    *(volatile uint32_t *)idx->hFlag = 0;
    if ((rc = knn_search(idx, &wp, wb, st, stage == 0 ? d_stage : nullptr, nullptr, true))) return rc;
    if ((rc = synced(st, what))) return rc;
    if ((*(volatile uint32_t *)idx->hFlag & 1u) && (rc = knn_repair(idx, &wp, wb, st, nullptr, true))) return rc;
    HIP_TRY(hipMemsetAsync(lb.count.p, 0, 4, st));
    return HNSW_OK;
}

hnsw_dev::LadderOut Ladder::out(const uint32_t *wnd, uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_stage) const {
    const LadderBufs &lb = idx->ladder_scratch;
    return {wnd, wb.nh, (uint32_t)stage, stage > 0, out_nd, out_nh, out_stage, (int32_t *)lb.list[cur ^ 1].p, (uint32_t *)lb.count.p};
}

int Ladder::count_short() {
    HIP_TRY(hipMemcpyAsync(&n_short, idx->ladder_scratch.count.p, 4, hipMemcpyDeviceToHost, st));
    return synced(st, what);
}

int Ladder::advance(bool &more) {
    LadderBufs &lb = idx->ladder_scratch;
    const int64_t pad = padded_stride(idx->iv.d);
    int rc;
    shorts.resize(n_short);
    HIP_TRY(hipMemcpy(shorts.data(), lb.list[cur ^ 1].p, (size_t)n_short * 4, hipMemcpyDeviceToHost));
    std::sort(shorts.begin(), shorts.end());
    HIP_TRY(hipMemcpy(lb.list[cur ^ 1].p, shorts.data(), (size_t)n_short * 4, hipMemcpyHostToDevice));
    cur ^= 1;
    map = (const int32_t *)lb.list[cur].p;
    m = n_short;
    if ((rc = lb.q.ensure((size_t)m * pad * sizeof(float)))) return rc;
    hipLaunchKernelGGL(hnsw_dev::ladder_gather_kernel, dim3((unsigned)m), dim3(64), 0, st, Q, q_stride, idx->iv.d, map, m, (float *)lb.q.p, pad);
    if ((rc = launched("ladder gather kernel"))) return rc;
    Qj = (const float *)lb.q.p;
    qs = pad;
    more = e < 1024;                    // else: still short with the largest W the library walks
    e = std::min(1024, 2 * e);
    ++stage;
    return HNSW_OK;
}

} // namespace hnsw_host

namespace {

// The ladder and the exact stage for a batch HostCall::begin has placed (c.b): the results are in c.b's rows and fb.stage on return.
int filtered_search(hnsw_index *idx, const hnsw_filter *f, const hnsw_search_params &p, const KnnBatch &b, float *d_stage, hipStream_t st) {
    FilterBufs &fb = idx->filter_scratch;
    const int k = p.k;
    const bool rerank = walk_is_inexact(idx);
    int rc;
    if ((rc = fb.stage.ensure((size_t)b.nq * 4)) || (rc = fb.rids.ensure((size_t)b.nq * k * 4)) || (rc = fb.rdist.ensure((size_t)b.nq * k * 4)) ||
        (rc = fb.rnd.ensure((size_t)b.nq * 4)))
        return rc;
    uint32_t *const d_stage_out = (uint32_t *)fb.stage.p;
    Ladder L(idx, b.Q, b.nq, b.q_stride, p.ef, p.semantics, d_stage, st, "filtered search");
    const bool walked = f->n_allowed >= k;
    for (bool more = walked; more;) {
        const int64_t m = L.m;
        const int e = L.e;
        if ((rc = fb.wids.ensure((size_t)m * e * 4)) || (rc = fb.wdist.ensure((size_t)m * e * 4)) || (rc = fb.cnt.ensure((size_t)m * 4)) ||
            (rerank && (rc = fb.cand.ensure((size_t)m * e * 4))))
            return rc;
        if ((rc = L.walk((int32_t *)fb.wids.p, (float *)fb.wdist.p, p.fill))) return rc;
        const hnsw_dev::SelectArgs sa{L.wb.ids, L.wb.dist, m, e, k, L.map, (const uint32_t *)f->bits.p, f->n, idx->iv.id_base, b.ids, b.dist,
                                      rerank ? (int32_t *)fb.cand.p : nullptr, (int32_t *)fb.cnt.p, L.out(L.wb.nd, b.nd, b.nh, d_stage_out)};
        hipLaunchKernelGGL(hnsw_dev::filter_select_kernel, dim3((unsigned)m), dim3(64), 0, st, sa);
        if ((rc = launched("filter select kernel")) || (rc = L.count_short())) return rc;
        if (rerank && (int64_t)L.n_short < m) {
            // the served queries' allowed members over the float32 rows, then their rows to where they belong
            if ((rc = launch_rerank(idx, L.Qj, m, L.qs, (const int32_t *)fb.cand.p, e, k, p.fill, (int32_t *)fb.rids.p, (float *)fb.rdist.p, nullptr,
                                    (uint32_t *)fb.rnd.p, st)))
                return rc;
            const hnsw_dev::ScatterArgs sc{(const int32_t *)fb.rids.p, (const float *)fb.rdist.p, m, k, L.map, (const int32_t *)fb.cnt.p,
                                           (const uint32_t *)fb.rnd.p, 0u, 0, 0, 0u, b.ids, b.dist, b.nd, b.nh, d_stage_out};
            hipLaunchKernelGGL(hnsw_dev::filter_scatter_kernel, dim3((unsigned)m), dim3(64), 0, st, sc);
            // (waited for here: a failure of theirs is this stage's, not the next walk's)
            if ((rc = launched("filter scatter kernel")) || (rc = synced(st, "filtered search"))) return rc;
        }
        if (L.n_short == 0) return HNSW_OK;
        if ((rc = L.advance(more))) return rc;
    }
    // the exact stage: the k smallest allowed nodes under (distance, id) for the L.m queries of (L.Qj, L.map)
    if ((rc = scan_search(idx, {L.Qj, L.m, L.qs, (int32_t *)fb.rids.p, (float *)fb.rdist.p, nullptr, nullptr, nullptr, nullptr}, k, p.fill, st,
                          (const uint32_t *)f->bits.p)))
        return rc;
    const hnsw_dev::ScatterArgs sc{(const int32_t *)fb.rids.p, (const float *)fb.rdist.p, L.m, k, L.map, nullptr, nullptr, (uint32_t)f->n_allowed,
                                   !walked, 1, 0xFFFFFFFFu, b.ids, b.dist, b.nd, b.nh, d_stage_out};
    hipLaunchKernelGGL(hnsw_dev::filter_scatter_kernel, dim3((unsigned)L.m), dim3(64), 0, st, sc);
    return launched("filter scatter kernel");
}

} // namespace

extern "C" {

int32_t hnsw_filter_create(hnsw_index *idx, const uint32_t *bits, int64_t n_bits, hnsw_filter **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (n_bits != idx->iv.n) return fail(HNSW_ERR_BAD_ARG, "the filter has %lld bits, the index %lld nodes", (long long)n_bits, (long long)idx->iv.n);
    if (n_bits > 0 && !bits) return fail(HNSW_ERR_BAD_ARG, "null bits");
    HIP_TRY(hipSetDevice(idx->device));
    std::unique_ptr<hnsw_filter> f(new hnsw_filter());
    f->idx = idx;
    f->n = n_bits;
    const int64_t words = (n_bits + 31) / 32;
    int rc;
    if ((rc = f->bits.ensure((size_t)std::max<int64_t>(words, 1) * 4))) return rc;
    if (words > 0) {
        DevBuf count;
        if ((rc = count.ensure(8))) return rc;
        HIP_TRY(hipMemcpy(f->bits.p, bits, (size_t)words * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(count.p, 0, 8));
        const unsigned blocks = (unsigned)std::min<int64_t>(1024, (words + 255) / 256);
        hipLaunchKernelGGL(hnsw_dev::filter_popcount_kernel, dim3(blocks), dim3(256), 0, nullptr, (uint32_t *)f->bits.p, words, n_bits,
                           (unsigned long long *)count.p);
        if ((rc = launched("filter popcount kernel"))) return rc;
        unsigned long long c = 0;
        HIP_TRY(hipMemcpy(&c, count.p, 8, hipMemcpyDeviceToHost));
        f->n_allowed = (int64_t)c;
    }
    *out = f.release();
    return HNSW_OK;
}

int32_t hnsw_filter_destroy(hnsw_filter *f) {
    if (!f) return HNSW_OK;
    delete f;
    return HNSW_OK;
}

int32_t hnsw_filter_count(const hnsw_filter *f, int64_t *n_allowed) {
    if (!f || !n_allowed) return fail(HNSW_ERR_BAD_ARG, "null filter or null n_allowed");
    *n_allowed = f->n_allowed;
    return HNSW_OK;
}

int32_t hnsw_search_batch_filtered(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                   const hnsw_search_params *params, int32_t *out_ids, float *out_dist, uint32_t *out_ndist,
                                   uint32_t *out_nhops, uint32_t *out_stage) {
    int rc = check_batch(idx, params, nq, q_stride, queries && out_ids && out_dist);
    if (rc) return rc;
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "the k farthest of W (HNSW_SEM_FUNCTOR_NEAREST_K) have no filtered meaning");
    if (!f) return fail(HNSW_ERR_BAD_ARG, "null filter");
    if (f->idx != idx) return fail(HNSW_ERR_BAD_ARG, "the filter was made for another index");
    if (f->n != idx->iv.n)
        return fail(HNSW_ERR_BAD_ARG, "the filter was made for %lld nodes, the index has grown to %lld", (long long)f->n, (long long)idx->iv.n);
    if (nq == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(idx->device));
    HostCall c;
    bool q_in_place = false;
    if ((rc = c.begin(idx, queries, nq, q_stride, params->k, out_ids, out_dist, out_ndist, out_nhops, true, &q_in_place))) return rc;
    hipStream_t st = idx->hs[0];
    rc = filtered_search(idx, f, *params, c.b, q_in_place ? (float *)idx->scratch.q.p : nullptr, st);
    if (!rc && out_stage && hipMemcpyAsync(out_stage, idx->filter_scratch.stage.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(HNSW_ERR_HIP, "stage download failed");
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    return c.finish(idx, "filtered search", st);
}

} // extern "C"
