// hnsw_filter.hip -- filtered k-NN search: an allow-mask over the nodes (hnsw_filter_*), hnsw_search_batch_filtered and its
// one-filter-per-query form hnsw_search_batch_filtered_each (one driver: the first is the table of one filter), which compose pieces that exist already -- the unchanged walk (knn_search with k := ef: W stays on the device), the re-rank kernel
// (hnsw_rerank.hip) and the exact scan (hnsw_scan.hip, its masked form) -- into the definition the header gives:
//   ladder   e = ef, 2 ef, ... 1024: a query is served at the first e whose W holds k allowed nodes; only the queries still short
//            are walked again, gathered into one compact batch;
//   exact    a query still short at e = 1024, and every query whose filter allows fewer than k nodes, gets the masked exact scan:
//            one launch sequence for all filters, the queries ordered by (filter, query) and laid out so that no scan tile spans
//            two filters (hnsw_filter_plan.h).
// The ladder itself (Ladder: the loop, the walk of a stage and its re-rank over the float32 rows, the short list, the gathered
// batch) is here too, and so is the scatter kernel: the range, grouped and paged searches (hnsw_range.hip, hnsw_group.hip,
// hnsw_after.hip) run the same loop, each with a stage body and a select rule of its own.
// Option "filter_collect" (k <= 128, exact rows) changes the stage test only: a stage's walk is the collect kernel's
// (hnsw_search_collect_kernel), whose [m][k] rows hold R -- the first k allowed nodes of everything the walk evaluated -- and the
// select kernel, run with e := k, serves the queries whose R is full.
//
// Kernels.
//   filter_popcount_kernel  the uploaded mask: clears the bits past n in its last word and counts the rest; with a second operand
//                           (the live mask of a handle with nodes marked deleted) the mask is ANDed with it first.
//   filter_label_kernel     hnsw_filter_create_by_label: all masks and their counts in one pass over the nodes' labels; a node
//                           marked deleted counts as label -1.
//   filter_select_kernel    one wave per walked query: tests the bit of each member of W in the query's own mask, 64 entries per pass (ballot, prefix
//                           count).  A query with k allowed members is SERVED: its first k allowed (id, distance) pairs go to its
//                           output row (rows whose walk distances are exact over X: float32, bytes, split), or its W with the
//                           disallowed entries turned into padding goes to the re-rank's candidate matrix (half, sq8).  Others
//                           are appended to the short list (ladder_settle).
//   ladder_gather_kernel    the short queries' vectors as one compact, zero-padded matrix: the next walk's / the exact stage's batch
//                           (a padding row of the exact stage's layout: the zero vector).
//   filter_scatter_kernel   rows of a compact result (re-rank, scan; the grouped exact stage's, with their labels column) to the rows
//                           of the queries they belong to; padding rows are dropped.
// No LDS, vector stores only.  All scratch is the handle's (LadderBufs, FilterBufs): one filtered, range, grouped or paged call in
// flight per handle.
#include "hnsw_internal.h"

namespace hnsw_dev {

__global__ void __launch_bounds__(256)
filter_popcount_kernel(uint32_t *bits, int64_t words, int64_t n, unsigned long long *count, const uint32_t *and_with) {
    int c = 0;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
        uint32_t v = bits[w];
        const uint32_t keep = (and_with ? and_with[w] : ~0u) &
                              (w == words - 1 && (n & 31) ? (1u << (n & 31)) - 1u : ~0u);     // positions >= n of the last word are not nodes
        if ((v & keep) != v) {
            v &= keep;
            bits[w] = v;
        }
        c += __builtin_popcount(v);
    }
    for (int s = 32; s > 0; s >>= 1) c += __shfl_down(c, s, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

// One pass over the labels builds every label's mask and count: masks[l] (ceil(n / 32) words, zeroed before) gets bit v iff
// labels[v] == l; a label of -1 is in no mask.  A wave takes 64 consecutive nodes, that is two whole words of every mask, and
// loops over the distinct labels among them: the label of the first lane not yet done (readlane), the ballot of the lanes that
// carry it -- its two halves are those two words of that label's mask, stored by lanes 0 and 32.  A (label, word) pair has one
// writer, this wave, so the masks need no atomics; the counts take one atomicAdd per (wave, label).  Nodes >= n carry no label,
// and neither does a node whose bit of `live` (optional: the live mask of a handle with nodes marked deleted) is clear.
__global__ void __launch_bounds__(256)
filter_label_kernel(const int32_t *labels, int64_t n, int64_t words, uint32_t *const *masks, unsigned long long *counts, const uint32_t *live) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = base + lane;
        const int32_t lab = v < n && (!live || ((live[v >> 5] >> (v & 31)) & 1u)) ? labels[v] : -1;
        uint64_t todo = ballot(lab >= 0);
        while (todo) {
            const int32_t l = __builtin_amdgcn_readlane(lab, (int)__builtin_ctzll(todo));
            const uint64_t m = ballot(lab == l);
            todo &= ~m;
            const int64_t w = (base >> 5) + (lane >> 5);
            const uint32_t half = (uint32_t)(m >> (lane & 32));
            if ((lane & 31) == 0 && half && w < words) masks[l][w] = half;
            if (lane == 0) atomicAdd(counts + l, (unsigned long long)popc(m));
        }
    }
}

struct SelectArgs {
    const int32_t *wids;       // [m][e] the walk's W per query, id_base-based, filled entries < id_base
    const float *wdist;        // [m][e]
    int64_t m;
    int32_t e, k;
    const int32_t *map;        // [m] row i belongs to query map[i]; null: to query i
    const uint32_t *const *masks;  // the masks; query q's is masks[which[q]], masks[0] when which is null
    const int32_t *which;      // [nq], by query (map's numbering), not by row
    int64_t n;
    int32_t id_base;
    int32_t *out_ids;          // [nq][k]
    float *out_dist;
    int32_t *cand;             // null, or [m][e]: the re-rank's candidates instead of out_ids / out_dist
    int32_t *cnt;              // [m] allowed members of W
    LadderOut out;
};

__global__ void __launch_bounds__(64)
filter_select_kernel(const SelectArgs a) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= a.m) return;
    const int64_t q = a.map ? a.map[i] : i;
    const MaskWords bits = mask_words(a.masks[a.which ? a.which[q] : 0]);
    const int32_t *const wi = a.wids + i * a.e;
    int cnt = 0;
    for (int j0 = 0; j0 < a.e; j0 += 64) {
        const int j = j0 + lane;
        cnt += popc(ballot(j < a.e && node_allowed(bits, a.n, a.id_base, wi[j])));
    }
    const bool served = cnt >= a.k;
    if (a.cand) {               // W with everything but a served query's allowed members as padding
        for (int j = lane; j < a.e; j += 64) {
            const int32_t id = wi[j];
            a.cand[i * a.e + j] = served && node_allowed(bits, a.n, a.id_base, id) ? id : a.id_base - 1;
        }
    } else if (served) {        // the first k allowed members, in W's order
        int at = 0;
        for (int j0 = 0; j0 < a.e && at < a.k; j0 += 64) {
            const int j = j0 + lane;
            const int32_t id = j < a.e ? wi[j] : a.id_base - 1;
            const bool ok = j < a.e && node_allowed(bits, a.n, a.id_base, id);
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

// out[i] = Q[list[i]], rows of out_stride floats, zero beyond d; list[i] < 0 (a padding row): all zero
__global__ void __launch_bounds__(64)
ladder_gather_kernel(const float *Q, int64_t q_stride, int32_t d, const int32_t *list, int64_t m, float *out, int64_t out_stride) {
    const int64_t i = blockIdx.x;
    if (i >= m) return;
    const int64_t q = list[i];
    const float *qp = Q + (q < 0 ? 0 : q) * q_stride;
    for (int64_t c = threadIdx.x; c < out_stride; c += 64) out[i * out_stride + c] = q >= 0 && c < d ? qp[c] : 0.f;
}

__global__ void __launch_bounds__(64)
filter_scatter_kernel(const ScatterArgs a) {
    const int64_t i = blockIdx.x;
    if (i >= a.m || (a.cnt && a.cnt[i] < a.k)) return;
    const int64_t q = a.map ? a.map[i] : i;
    if (q < 0) return;
    for (int j = threadIdx.x; j < a.k; j += 64) {
        a.out_ids[q * a.k + j] = a.rids[i * a.k + j];
        a.out_dist[q * a.k + j] = a.rdist[i * a.k + j];
        if (a.rlab) a.out_labels[q * a.k + j] = a.rlab[i * a.k + j];
    }
    if (threadIdx.x == 0) {
        const uint32_t add = (a.add ? a.add[i] : 0u) + a.add_const;
        if (a.exact) exact_settle(a.out_nd, a.out_nh, a.out_stage, q, add, a.fresh_of ? a.fresh_of[i] != 0 : a.fresh != 0);
        else a.out_nd[q] += add;
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
    // (option "filter_collect": the same walk of ef = e; its rows are R's collect_k entries, not W's e)
    const hnsw_search_params wp{e, collect_k ? collect_k : e, fill, semantics};
    const hnsw_dev::CollectArgs ca{collect_masks, collect_which, map};
    const hnsw_dev::CollectArgs *const collect = collect_k ? &ca : nullptr;
    wb = KnnBatch{Qj, m, qs, wids, wdist, (uint32_t *)lb.wnd.p, (uint32_t *)lb.wnh.p, (uint32_t *)lb.wst.p, idx->hFlagDev};
    evals = wb.nd;
    counted = false;
    *(volatile uint32_t *)idx->hFlag = 0;
    // (d_stage: only the caller's own matrix can lie in host memory, never a gathered batch)
    if ((rc = knn_search(idx, &wp, wb, st, map ? nullptr : d_stage, nullptr, true, collect))) return rc;
    if ((rc = synced(st, what))) return rc;
    if ((*(volatile uint32_t *)idx->hFlag & 1u) && (rc = knn_repair(idx, &wp, wb, st, nullptr, true, collect))) return rc;
    HIP_TRY(hipMemsetAsync(lb.count.p, 0, 4, st));
    return HNSW_OK;
}

int Ladder::walk_raw(int32_t *Wi, float *Wd, int32_t fill) {
    if (!walk_is_inexact(idx)) return walk(Wi, Wd, fill);
    LadderBufs &lb = idx->ladder_scratch;
    int rc;
    if ((rc = lb.cand.ensure((size_t)m * e * 4)) || (rc = lb.cdist.ensure((size_t)m * e * 4)) || (rc = lb.rnd.ensure((size_t)m * 4))) return rc;
    return walk((int32_t *)lb.cand.p, (float *)lb.cdist.p, fill);
}

int Ladder::rerank_all(int32_t *Wi, float *Wd, int32_t fill) {
    if (!walk_is_inexact(idx)) return HNSW_OK;
    uint32_t *const rnd = (uint32_t *)idx->ladder_scratch.rnd.p;
    const int rc = launch_rerank(idx, Qj, m, qs, wb.ids, e, e, fill, Wi, Wd, wb.nd, rnd, st);
    evals = rnd;
    return rc;
}

hnsw_dev::LadderOut Ladder::out(uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_stage) const {
    const LadderBufs &lb = idx->ladder_scratch;
    return {evals, wb.nh, (uint32_t)stage, stage > 0, out_nd, out_nh, out_stage, (int32_t *)lb.list[cur ^ 1].p, (uint32_t *)lb.count.p};
}

int Ladder::count_short() {
    if (counted) return HNSW_OK;
    counted = true;
    HIP_TRY(hipMemcpyAsync(&n_short, idx->ladder_scratch.count.p, 4, hipMemcpyDeviceToHost, st));
    return synced(st, what);
}

int Ladder::gather() {
    LadderBufs &lb = idx->ladder_scratch;
    const int64_t pad = padded_stride(idx->iv.d);
    int rc;
    if ((rc = lb.q.ensure((size_t)m * pad * sizeof(float)))) return rc;
    hipLaunchKernelGGL(hnsw_dev::ladder_gather_kernel, dim3((unsigned)m), dim3(64), 0, st, Q, q_stride, idx->iv.d, map, m, (float *)lb.q.p, pad);
    if ((rc = launched("ladder gather kernel"))) return rc;
    Qj = (const float *)lb.q.p;
    qs = pad;
    return HNSW_OK;
}

int Ladder::start_from(const int32_t *list, int64_t count) {
    LadderBufs &lb = idx->ladder_scratch;
    int rc;
    if ((rc = lb.list[0].ensure((size_t)nq * 4)) || (rc = lb.list[1].ensure((size_t)nq * 4))) return rc;
    HIP_TRY(hipMemcpy(lb.list[cur].p, list, (size_t)count * 4, hipMemcpyHostToDevice));
    map = (const int32_t *)lb.list[cur].p;
    m = count;
    return gather();
}

int Ladder::advance(bool &more) {
    LadderBufs &lb = idx->ladder_scratch;
    int rc;
    shorts.resize(n_short);
    HIP_TRY(hipMemcpy(shorts.data(), lb.list[cur ^ 1].p, (size_t)n_short * 4, hipMemcpyDeviceToHost));
    std::sort(shorts.begin(), shorts.end());
    HIP_TRY(hipMemcpy(lb.list[cur ^ 1].p, shorts.data(), (size_t)n_short * 4, hipMemcpyHostToDevice));
    cur ^= 1;
    map = (const int32_t *)lb.list[cur].p;
    m = n_short;
    if ((rc = gather())) return rc;
    more = e < 1024;                    // else: still short with the largest W the library walks
    e = std::min(1024, 2 * e);
    ++stage;
    return HNSW_OK;
}

int scatter_rows(const hnsw_dev::ScatterArgs &a, hipStream_t st, const char *what) {
    hipLaunchKernelGGL(hnsw_dev::filter_scatter_kernel, dim3((unsigned)a.m), dim3(64), 0, st, a);
    return launched(what);
}

// a filter of n nodes for idx (its epoch) with its mask allocated (not initialised) and the mask's own address behind it
int new_filter(const hnsw_index *idx, int64_t n, std::unique_ptr<hnsw_filter> &f) {
    f.reset(new hnsw_filter());
    f->idx = idx;
    f->n = n;
    f->epoch = idx->epoch;
    const size_t off = hnsw_filter::table_offset(f->n);
    int rc;
    if ((rc = f->bits.ensure(off + 8))) return rc;
    const void *self = f->bits.p;
    HIP_TRY(hipMemcpy((char *)f->bits.p + off, &self, 8, hipMemcpyHostToDevice));
    return HNSW_OK;
}

// n_allowed of f's mask, ANDed with and_with first (optional)
int count_filter(hnsw_filter *f, const uint32_t *and_with) {
    const int64_t words = (f->n + 31) / 32;
    f->n_allowed = 0;
    if (words == 0) return HNSW_OK;
    DevBuf count;
    int rc;
    if ((rc = count.ensure(8))) return rc;
    HIP_TRY(hipMemset(count.p, 0, 8));
    const unsigned blocks = (unsigned)std::min<int64_t>(1024, (words + 255) / 256);
    hipLaunchKernelGGL(hnsw_dev::filter_popcount_kernel, dim3(blocks), dim3(256), 0, nullptr, (uint32_t *)f->bits.p, words, f->n,
                       (unsigned long long *)count.p, and_with);
    if ((rc = launched("filter popcount kernel"))) return rc;
    unsigned long long c = 0;
    HIP_TRY(hipMemcpy(&c, count.p, 8, hipMemcpyDeviceToHost));
    f->n_allowed = (int64_t)c;
    return HNSW_OK;
}

} // namespace hnsw_host

namespace {

// The filters of one call: a table of n filters and, per query, which of them it is answered under (host: which, device: d_which;
// both null: every query under filters[0], the single-filter call).  d_masks: the masks' device addresses [n].
struct FilterSet {
    const hnsw_filter *const *filters;
    int32_t n;
    const int32_t *which;
    const uint32_t *const *d_masks;
    const int32_t *d_which;
    int32_t index_of(int64_t q) const { return which ? which[q] : 0; }
    const hnsw_filter &of(int64_t q) const { return *filters[index_of(q)]; }
};

// The exact stage for the queries of `rest` (short at the ladder's end) and of `fresh` (no walk: their filters allow fewer than k
// nodes), whatever their filters: the rows by (filter, query) with no tile of the scan spanning two filters (filter_plan), gathered
// from the caller's batch, ONE masked scan, and the rows back to their queries.
int exact_stage_each(hnsw_index *idx, const FilterSet &fs, const hnsw_search_params &p, const KnnBatch &b, const std::vector<int32_t> &rest,
                     const std::vector<int32_t> &fresh, uint32_t *d_stage_out, hipStream_t st) {
    FilterBufs &fb = idx->filter_scratch;
    LadderBufs &lb = idx->ladder_scratch;
    const int k = p.k, T = scan_cut(idx, 1, k, 2 * (int64_t)k * 8, 16384).T;      // (the tile of the scan's kernels)
    std::vector<std::pair<int32_t, int32_t>> pairs;
    pairs.reserve(rest.size() + fresh.size());
    for (const std::vector<int32_t> *list : {&rest, &fresh})
        for (int32_t q : *list) pairs.emplace_back(fs.index_of(q), q);
    const FilterRows rows = filter_plan(std::move(pairs), T);
    const int64_t R = (int64_t)rows.row_query.size(), tiles = (int64_t)rows.tile_filter.size();
    // one upload: row -> query, tile -> filter, per row the evaluations to add (its filter's n_allowed) and whether it took no walk
    std::vector<int32_t> up((size_t)(3 * R + tiles), 0);
    std::vector<char> is_fresh((size_t)b.nq, 0);
    for (int32_t q : fresh) is_fresh[(size_t)q] = 1;
    for (int64_t i = 0; i < R; ++i) {
        const int32_t q = rows.row_query[(size_t)i];
        up[(size_t)i] = q;
        if (q < 0) continue;
        up[(size_t)(R + i)] = (int32_t)(uint32_t)fs.of(q).n_allowed;
        up[(size_t)(2 * R + i)] = is_fresh[(size_t)q];
    }
    std::copy(rows.tile_filter.begin(), rows.tile_filter.end(), up.begin() + 3 * R);
    const int64_t pad = padded_stride(idx->iv.d);
    int rc;
    if ((rc = fb.rows.ensure(up.size() * 4)) || (rc = lb.q.ensure((size_t)R * pad * sizeof(float))) || (rc = fb.rids.ensure((size_t)R * k * 4)) ||
        (rc = fb.rdist.ensure((size_t)R * k * 4)))
        return rc;
    HIP_TRY(hipMemcpy(fb.rows.p, up.data(), up.size() * 4, hipMemcpyHostToDevice));
    const int32_t *const d_rows = (const int32_t *)fb.rows.p;
    hipLaunchKernelGGL(hnsw_dev::ladder_gather_kernel, dim3((unsigned)R), dim3(64), 0, st, b.Q, b.q_stride, idx->iv.d, d_rows, R, (float *)lb.q.p, pad);
    if ((rc = launched("ladder gather kernel"))) return rc;
    if ((rc = scan_search(idx, {(const float *)lb.q.p, R, pad, (int32_t *)fb.rids.p, (float *)fb.rdist.p, nullptr, nullptr, nullptr, nullptr}, k, p.fill, st,
                          fs.d_masks, d_rows + 3 * R, d_rows)))
        return rc;
    return scatter_rows({(const int32_t *)fb.rids.p, (const float *)fb.rdist.p, nullptr, R, k, d_rows, nullptr, (const uint32_t *)(d_rows + R), 0u, 1,
                         d_rows + 2 * R, 0, b.ids, b.dist, nullptr, b.nd, b.nh, d_stage_out},
                        st, "filter scatter kernel");
}

// The ladder and the exact stage for a batch HostCall::begin has placed (c.b): the results are in c.b's rows and fb.stage on return.
int filtered_search(hnsw_index *idx, const FilterSet &fs, const hnsw_search_params &p, const KnnBatch &b, float *d_stage, hipStream_t st) {
    FilterBufs &fb = idx->filter_scratch;
    const int k = p.k;
    const bool rerank = walk_is_inexact(idx);
    int rc;
    if ((rc = fb.stage.ensure((size_t)b.nq * 4)) || (rc = fb.rids.ensure((size_t)b.nq * k * 4)) || (rc = fb.rdist.ensure((size_t)b.nq * k * 4)) ||
        (rc = fb.rnd.ensure((size_t)b.nq * 4)))
        return rc;
    uint32_t *const d_stage_out = (uint32_t *)fb.stage.p;
    Ladder L(idx, b.Q, b.nq, b.q_stride, p.ef, p.semantics, d_stage, st, "filtered search");
    // option "filter_collect" (k <= 128, exact rows): a stage's walk hands back R -- the first k allowed nodes of all it evaluated --
    // in [m][k] rows, and the select kernel below, run with e := k, counts R's real entries: its stage test is |R| >= k
    const bool collect = idx->filter_collect && k <= 128 && !rerank;
    if (collect) { L.collect_k = k; L.collect_masks = fs.d_masks; L.collect_which = fs.d_which; }
    // who walks: the queries whose filter allows k nodes.  Everybody (the common case, and either all or none of a single-filter
    // call): stage 0 is the caller's batch in place; some: stage 0 starts from their list, the others wait for the exact stage
    std::vector<int32_t> walkers, fresh;
    if (fs.which) for (int64_t q = 0; q < b.nq; ++q) (fs.of(q).n_allowed >= k ? walkers : fresh).push_back((int32_t)q);
    const bool walked = fs.which ? !walkers.empty() : fs.filters[0]->n_allowed >= k;
    if (walked && !fresh.empty() && (rc = L.start_from(walkers.data(), (int64_t)walkers.size()))) return rc;
    LadderLeft left;
    rc = L.run(walked, [&](Ladder &, int64_t m, int e) -> int {
        if (collect) e = k;                   // entries per row of the stage's walk
        if ((rc = fb.wids.ensure((size_t)m * e * 4)) || (rc = fb.wdist.ensure((size_t)m * e * 4)) || (rc = fb.cnt.ensure((size_t)m * 4)) ||
            (rerank && (rc = fb.cand.ensure((size_t)m * e * 4))))
            return rc;
        if ((rc = L.walk((int32_t *)fb.wids.p, (float *)fb.wdist.p, p.fill))) return rc;
        const hnsw_dev::SelectArgs sa{L.wb.ids, L.wb.dist, m, e, k, L.map, fs.d_masks, fs.d_which, idx->iv.n, idx->iv.id_base, b.ids, b.dist,
                                      rerank ? (int32_t *)fb.cand.p : nullptr, (int32_t *)fb.cnt.p, L.out(b.nd, b.nh, d_stage_out)};
        hipLaunchKernelGGL(hnsw_dev::filter_select_kernel, dim3((unsigned)m), dim3(64), 0, st, sa);
        if ((rc = launched("filter select kernel")) || (rc = L.count_short())) return rc;
        if (rerank && (int64_t)L.n_short < m) {
            // the served queries' allowed members over the float32 rows, then their rows to where they belong
            if ((rc = launch_rerank(idx, L.Qj, m, L.qs, (const int32_t *)fb.cand.p, e, k, p.fill, (int32_t *)fb.rids.p, (float *)fb.rdist.p, nullptr,
                                    (uint32_t *)fb.rnd.p, st)) ||
                (rc = scatter_rows({(const int32_t *)fb.rids.p, (const float *)fb.rdist.p, nullptr, m, k, L.map, (const int32_t *)fb.cnt.p,
                                    (const uint32_t *)fb.rnd.p, 0u, 0, nullptr, 0, b.ids, b.dist, nullptr, b.nd, b.nh, d_stage_out},
                                   st, "filter scatter kernel")))
                return rc;
            // (waited for here: a failure of theirs is this stage's, not the next walk's)
            return synced(st, "filtered search");
        }
        return HNSW_OK;
    }, left);
    if (rc || (left == LadderLeft::none && fresh.empty())) return rc;
    if (fs.which) return exact_stage_each(idx, fs, p, b, left == LadderLeft::walked ? L.batch_queries() : std::vector<int32_t>(), fresh, d_stage_out, st);
    // the exact stage under one filter: the k smallest allowed nodes under (distance, id) for the L.m queries of (L.Qj, L.map) -- the
    // batch the ladder left --, which need no other layout
    if ((rc = scan_search(idx, {L.Qj, L.m, L.qs, (int32_t *)fb.rids.p, (float *)fb.rdist.p, nullptr, nullptr, nullptr, nullptr}, k, p.fill, st, fs.d_masks)))
        return rc;
    return scatter_rows({(const int32_t *)fb.rids.p, (const float *)fb.rdist.p, nullptr, L.m, k, L.map, nullptr, nullptr, (uint32_t)fs.filters[0]->n_allowed, 1,
                         nullptr, left == LadderLeft::fresh, b.ids, b.dist, nullptr, b.nd, b.nh, d_stage_out},
                        st, "filter scatter kernel");
}

// both search entry points once their arguments are checked (nq > 0).  fs.d_masks / fs.d_which are allocated; host_masks (the
// per-query form): what they hold is still to be uploaded, from there and from fs.which, on the call's stream
int filtered_call(hnsw_index *idx, const FilterSet &fs, const uint32_t *const *host_masks, const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params,
                  int32_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage, const KeysOut *ko = nullptr,
                  const RowsIn *rows = nullptr, const DiverseOut *dv = nullptr) {
    return ladder_host_call(idx, queries, nq, q_stride, params->k, out_ids, out_dist, out_ndist, out_nhops, out_stage, true, ko, rows, dv, nullptr,
                            "filtered search", [&](const KnnBatch &b, float *d_stage, hipStream_t st) -> int {
        if (host_masks) {
            hipError_t e = hipMemcpyAsync(const_cast<uint32_t **>(fs.d_masks), host_masks, (size_t)fs.n * 8, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(const_cast<int32_t *>(fs.d_which), fs.which, (size_t)nq * 4, hipMemcpyHostToDevice, st);
            if (e != hipSuccess) return hip_fail(e, "filter table upload");
        }
        return filtered_search(idx, fs, *params, b, d_stage, st);
    });
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
    std::unique_ptr<hnsw_filter> f;
    int rc;
    if ((rc = new_filter(idx, idx->iv.n, f))) return rc;
    const int64_t words = (n_bits + 31) / 32;
    if (words > 0) {
        HIP_TRY(hipMemcpy(f->bits.p, bits, (size_t)words * 4, hipMemcpyHostToDevice));
        // (while nodes are marked deleted the mask is ANDed with the live mask: a current filter never allows a marked node)
        const hnsw_filter *const live = live_filter(idx);
        if ((rc = count_filter(f.get(), live ? (const uint32_t *)live->bits.p : nullptr))) return rc;
    }
    *out = f.release();
    return HNSW_OK;
}

int32_t hnsw_filter_create_by_label(hnsw_index *idx, const int32_t *labels, int64_t n, int32_t n_labels, hnsw_filter **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    if (n_labels < 1) return fail(HNSW_ERR_BAD_ARG, "n_labels must be >= 1 (n_labels=%d)", n_labels);
    for (int32_t l = 0; l < n_labels; ++l) out[l] = nullptr;
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (n != idx->iv.n) return fail(HNSW_ERR_BAD_ARG, "%lld labels, the index has %lld nodes", (long long)n, (long long)idx->iv.n);
    if (n > 0 && !labels) return fail(HNSW_ERR_BAD_ARG, "null labels");
    for (int64_t v = 0; v < n; ++v)
        if (labels[v] < -1 || labels[v] >= n_labels)
            return fail(HNSW_ERR_BAD_ARG, "label %d of node %lld is outside -1 .. %d", labels[v], (long long)v, n_labels - 1);
    HIP_TRY(hipSetDevice(idx->device));
    // (owners until the end: any return before it frees them all)
    std::vector<std::unique_ptr<hnsw_filter>> fs((size_t)n_labels);
    std::vector<uint32_t *> masks((size_t)n_labels);
    const int64_t words = (n + 31) / 32;
    int rc;
    for (int32_t l = 0; l < n_labels; ++l) {
        if ((rc = new_filter(idx, idx->iv.n, fs[(size_t)l]))) return rc;
        masks[(size_t)l] = (uint32_t *)fs[(size_t)l]->bits.p;
        if (words > 0) HIP_TRY(hipMemsetAsync(masks[(size_t)l], 0, (size_t)words * 4, nullptr));
    }
    if (n > 0) {
        DevBuf d_labels, d_masks, d_counts;
        if ((rc = d_labels.ensure((size_t)n * 4)) || (rc = d_masks.ensure((size_t)n_labels * 8)) || (rc = d_counts.ensure((size_t)n_labels * 8))) return rc;
        HIP_TRY(hipMemcpy(d_labels.p, labels, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_masks.p, masks.data(), (size_t)n_labels * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(d_counts.p, 0, (size_t)n_labels * 8));
        const unsigned blocks = (unsigned)std::min<int64_t>(4096, (n + 255) / 256);
        hipLaunchKernelGGL(hnsw_dev::filter_label_kernel, dim3(blocks), dim3(256), 0, nullptr, (const int32_t *)d_labels.p, n, words,
                           (uint32_t *const *)d_masks.p, (unsigned long long *)d_counts.p,
                           live_filter(idx) ? (const uint32_t *)live_filter(idx)->bits.p : nullptr);
        if ((rc = launched("filter label kernel"))) return rc;
        std::vector<unsigned long long> counts((size_t)n_labels);
        HIP_TRY(hipMemcpy(counts.data(), d_counts.p, (size_t)n_labels * 8, hipMemcpyDeviceToHost));
        for (int32_t l = 0; l < n_labels; ++l) fs[(size_t)l]->n_allowed = (int64_t)counts[(size_t)l];
    }
    for (int32_t l = 0; l < n_labels; ++l) out[l] = fs[(size_t)l].release();
    return HNSW_OK;
}

int32_t hnsw_filter_bits(const hnsw_filter *f, uint32_t *out) {
    if (!f || !out) return fail(HNSW_ERR_BAD_ARG, "null filter or null out");
    const int64_t words = (f->n + 31) / 32;
    if (words == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(f->idx->device));
    HIP_TRY(hipMemcpy(out, f->bits.p, (size_t)words * 4, hipMemcpyDeviceToHost));
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
    return filtered_host_call(idx, f, queries, nq, q_stride, params, out_ids, out_dist, out_ndist, out_nhops, out_stage, nullptr);
}

} // extern "C"

int hnsw_host::filtered_host_call(hnsw_index *idx, const hnsw_filter *f, const float *queries, int64_t nq, int64_t q_stride,
                                  const hnsw_search_params *params, int32_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops,
                                  uint32_t *out_stage, const KeysOut *ko, const RowsIn *rows, const DiverseOut *dv) {
    int rc = check_batch(idx, params, nq, q_stride, (rows ? rows->ids != nullptr : queries != nullptr) &&
                                                        (dv ? dv->ids && dv->dist : (ko ? ko->keys != nullptr : out_ids != nullptr) && out_dist));
    if (rc) return rc;
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "the k farthest of W (HNSW_SEM_FUNCTOR_NEAREST_K) have no filtered meaning");
    if ((rc = check_filter(idx, f))) return rc;
    if (nq == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(idx->device));
    // the table of one filter: the mask's own address, on the device since the filter was made
    return filtered_call(idx, FilterSet{&f, 1, nullptr, f->table(), nullptr}, nullptr, queries, nq, q_stride, params, out_ids, out_dist, out_ndist, out_nhops,
                         out_stage, ko, rows, dv);
}

extern "C" {

int32_t hnsw_search_batch_filtered_each(hnsw_index *idx, const hnsw_filter *const *filters, int32_t n_filters, const int32_t *query_filter,
                                        const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params, int32_t *out_ids,
                                        float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage) {
    int rc = check_batch(idx, params, nq, q_stride, queries && out_ids && out_dist);
    if (rc) return rc;
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "the k farthest of W (HNSW_SEM_FUNCTOR_NEAREST_K) have no filtered meaning");
    if (n_filters < 1) return fail(HNSW_ERR_BAD_ARG, "n_filters must be >= 1 (n_filters=%d)", n_filters);
    if (!filters) return fail(HNSW_ERR_BAD_ARG, "null filters");
    for (int32_t l = 0; l < n_filters; ++l)
        if ((rc = check_filter(idx, filters[l]))) return rc;
    if (nq == 0) return HNSW_OK;
    if (!query_filter) return fail(HNSW_ERR_BAD_ARG, "null query_filter");
    for (int64_t q = 0; q < nq; ++q)
        if (query_filter[q] < 0 || query_filter[q] >= n_filters)
            return fail(HNSW_ERR_BAD_ARG, "query_filter[%lld] = %d is outside 0 .. %d", (long long)q, query_filter[q], n_filters - 1);
    HIP_TRY(hipSetDevice(idx->device));
    FilterBufs &fb = idx->filter_scratch;
    std::vector<const uint32_t *> masks((size_t)n_filters);
    for (int32_t l = 0; l < n_filters; ++l) masks[(size_t)l] = (const uint32_t *)filters[l]->bits.p;
    if ((rc = fb.masks.ensure((size_t)n_filters * 8)) || (rc = fb.which.ensure((size_t)nq * 4))) return rc;
    return filtered_call(idx, FilterSet{filters, n_filters, query_filter, (const uint32_t *const *)fb.masks.p, (const int32_t *)fb.which.p}, masks.data(),
                         queries, nq, q_stride, params, out_ids, out_dist, out_ndist, out_nhops, out_stage);
}

} // extern "C"
