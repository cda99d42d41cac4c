// hnsw_after.hip -- paged k-NN search: the next k after a (distance, id) cursor (hnsw_search_batch_after,
// hnsw_brute_force_batch_after).  The order is the one a caller can hold: (ord(returned float distance), node id) -- a coarsening
// of the exact scan's (key, id), from which it differs only among nodes whose L2 distances are equal while their squared sums are
// not (hnsw_after_plan.h: ord, the word of a pair, the cursor as a bound in word space).  The search composes pieces that exist
// already -- the ladder's loop and its W over the float32 rows (Ladder::run, Ladder::walk_exact, hnsw_filter.hip), the exact scan's body
// (hnsw_scan_device.hip.h), the host frame (ladder_host_call) -- with one stage body, one select rule and one selection policy:
//   ladder   e = ef, 2 ef, ... 1024: a query is served at the first e whose W holds k ELIGIBLE members (after its cursor, allowed,
//            live); its row is the first k of them under the paged order.  Only the queries still short are walked again;
//   exact    a query still short at e = 1024, every query when fewer than k nodes are allowed, and every query of the brute-force
//            form gets the paged exact scan.
//
// Kernels.
//   after_select_kernel     one wave per walked query, 64 entries of W per pass (ballot, prefix count): counts the eligible members
//                           and, for a served query, writes the first k of them.  W ascends in (key, id), so D is non-decreasing
//                           along it and W's order is the paged order except inside a run of equal D, where an entry's place is
//                           corrected by the eligible members of its run with a larger id before it and a smaller id behind it.
//                           Counters, stage and the short list: ladder_settle.
//   hnsw_after_scan_kernel<NCH, METRIC, MASKED>  scan_slab with ScanAfter, the twin of ScanTopK whose words are distance-words
//                           (ord(key_to_dist(key)) << 32 | row) and which admits a word only above the query's own bound lo[t].
//                           The cheap reject stays one compare in key space: against the largest key whose distance is not above
//                           the threshold word's (l2_key_hi; under the inner product the word's upper half IS the key), recomputed
//                           when a flush lowers the threshold: no square root per (row, query) pair.
//   after_merge_kernel<METRIC>  hnsw_scan_merge_kernel over distance-words: one workgroup per query merges its slabs' lists and writes
//                           ids (+ id_base), distances (ord's inverse) and the fill to the row of the query it belongs to, with the
//                           exact stage's counters.
// No LDS in the select kernel, vector stores only.  All scratch is the handle's (LadderBufs; FilterBufs' wids / wdist / stage;
// AfterBufs; scratch.scan): one filtered, range, grouped or paged call in flight per handle.  out_next is plain arithmetic over the finished rows (next_cursor), on the host.
#include "hnsw_internal.h"
#include "hnsw_scan_device.hip.h"
#include "hnsw_after_plan.h"

namespace hnsw_dev {

// the upper half of the distance-word of a key: ord of the float hnsw_distance_batch returns for it
template <int METRIC> __device__ __forceinline__ uint32_t after_key_ord(uint32_t key) {
    if (METRIC != 0) return key;                    // (dist_to_key<1> is ord of the distance itself)
    return hnsw_after::ord(key_to_dist<0>(key));
}

struct AfterScanArgs {
    ScanArgs s;                // as the k-scan's: lists [nq][n_slabs][2][k], here of distance-words
    const uint64_t *lo;        // by query: only words above lo[query] are candidates
    const int32_t *map;        // row i of the call's batch belongs to query map[i]; null: to query i
    int64_t row0;              // the launch's first row among the call's
};

// The paged top-k selection of one (tile, slab) wave (scan_slab's Select): ScanTopK over distance-words with a lower bound per
// query of the tile.  thr[t]: the word of the k-th smallest admitted candidate so far (all ones until there are k); khi[t] (L2): the
// largest KEY whose distance-word's upper half is not above thr[t]'s.
template <int NCH, int METRIC, bool MASKED> struct ScanAfter : ScanMask<MASKED> {
    static constexpr int T = scan_tile(NCH);
    static constexpr int LIMIT = SCAN_BUF - 4 * scan_rows(NCH);
    const AfterScanArgs &a;
    uint64_t (*bufs)[SCAN_BUF], *sorted, *lists0;
    int64_t list_step;
    uint64_t thr[T], lo[T];
    uint32_t khi[METRIC == 0 ? T : 1];
    int cnt[T], tq, lane;
    uint32_t par;
    bool full;

    __device__ __forceinline__ ScanAfter(const AfterScanArgs &a_, const uint32_t *mask_) : ScanMask<MASKED>(mask_), a(a_) {}
    __device__ __forceinline__ void begin(int64_t q0, int tq_, int64_t slab) {
        __shared__ uint64_t bufs_all[SCAN_WAVES][T][SCAN_BUF];
        __shared__ uint64_t sorted_all[SCAN_WAVES][SCAN_BUF];
        lane = threadIdx.x & 63;
        bufs = bufs_all[threadIdx.x >> 6];
        sorted = sorted_all[threadIdx.x >> 6];
        tq = tq_;
        lists0 = a.s.lists + ((q0 * a.s.n_slabs + slab) * 2) * (int64_t)a.s.k;
        list_step = (int64_t)a.s.n_slabs * 2 * a.s.k;
        par = 0;
        full = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            // a query past the tile's end never has a survivor (no word is below 0)
            thr[t] = t < tq ? SCAN_EMPTY : 0ull;
            if (METRIC == 0) khi[t] = t < tq ? 0xFFFFFFFFu : 0u;
            cnt[t] = 0;
            lo[t] = SCAN_EMPTY;
            if (t < tq) {
                const int64_t i = a.row0 + q0 + t;
                lo[t] = scan_uniform64(a.lo[a.map ? a.map[i] : i]);
                for (int j = lane; j < a.s.k; j += 64) lists0[t * list_step + j] = SCAN_EMPTY;
            }
        }
        scan_wave_sync();
    }
    __device__ __forceinline__ void take(int t, uint32_t key, int64_t row, bool ok) {
        const uint32_t bound = METRIC == 0 ? khi[METRIC == 0 ? t : 0] : (uint32_t)(thr[t] >> 32);
        if (ballot(key <= bound)) {                              // rare: some row of the four may be among the k smallest
            const uint64_t e = ((uint64_t)after_key_ord<METRIC>(key) << 32) | (uint32_t)row;
            const bool in = (lane & 15) == 0 && ok && e > lo[t] && e < thr[t];
            const uint64_t m = ballot(in);
            if (in) bufs[t][cnt[t] + popc(m & ((1ull << lane) - 1ull))] = e;
            cnt[t] += popc(m);
            full = full || cnt[t] > LIMIT;
        }
    }
    // merges query t's buffer into its list, which lowers its threshold and with it the key bound
    __device__ __forceinline__ void flush(int t) {
        uint64_t *const A = lists0 + t * list_step;
        const bool p = (par >> t) & 1u;
        scan_flush(bufs[t], sorted, cnt[t], A + (p ? a.s.k : 0), A + (p ? 0 : a.s.k), a.s.k, lane);
        par ^= 1u << t;
        cnt[t] = 0;
        thr[t] = scan_uniform64((A + (p ? 0 : a.s.k))[a.s.k - 1]);
        if (METRIC == 0) {
            // (a threshold that is no distance of a real sum -- a NaN -- bounds nothing in key space)
            const float D = hnsw_after::ord_inverse((uint32_t)(thr[t] >> 32));
            const int64_t hi = thr[t] == SCAN_EMPTY || D != D ? 0xFFFFFFFFll : hnsw_after::l2_key_hi(D);
            khi[METRIC == 0 ? t : 0] = (uint32_t)uniform((int)(uint32_t)(hi < 0 ? 0 : hi));
        }
    }
    __device__ __forceinline__ void batch_end() {
        if (!full) return;
        full = false;
#pragma unroll
        for (int t = 0; t < T; ++t) if (cnt[t] > LIMIT) flush(t);
    }
    // what is left in the buffers; the result belongs in the first half
    __device__ __forceinline__ void end() {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t >= tq) continue;
            if (cnt[t] > 0) flush(t);
            uint64_t *const A = lists0 + t * list_step;
            if ((par >> t) & 1u) for (int j = lane; j < a.s.k; j += 64) A[j] = A[a.s.k + j];
        }
    }
};

template <int NCH, int METRIC, bool MASKED>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_after_scan_kernel(const IndexView iv, const AfterScanArgs a, const uint32_t *mask) {
    ScanAfter<NCH, METRIC, MASKED> sel(a, mask);
    scan_slab<NCH, METRIC>(iv, a.s.Q, a.s.q_stride, a.s.nq, a.s.n_slabs, a.s.slab_rows, sel);
}

struct AfterMergeArgs {
    const uint64_t *lists;     // [m][n_slabs][2][k] distance-words, the first half of each the slab's k smallest, ascending, padded
    int32_t n_slabs, k, fill, id_base;
    const int32_t *map;        // row i of the call's batch belongs to query map[i]; null: to query i
    int64_t row0;
    int32_t *out_ids;          // [nq][k] by query
    float *out_dist;
    // the exact stage's counters (out_nd null: none): exact_settle
    uint32_t *out_nd, *out_nh, *out_stage;
    uint32_t add;
    int32_t fresh;
};

// One workgroup per row of the launch: hnsw_scan_merge_kernel's rule (no word above the smallest of the lists' k-th words can be
// among the k smallest of the union; a word's place is the number of smaller words over all lists) over distance-words.
template <int METRIC>
__global__ void __launch_bounds__(256)
after_merge_kernel(const AfterMergeArgs a) {
    __shared__ unsigned long long bound;
    __shared__ int total;
    const int64_t i = blockIdx.x;
    const int64_t q = a.map ? a.map[a.row0 + i] : a.row0 + i;
    const int k = a.k, n_slabs = a.n_slabs;
    const uint64_t *L = a.lists + i * n_slabs * 2 * (int64_t)k;
    const int64_t step = 2 * (int64_t)k;
    if (threadIdx.x == 0) { bound = SCAN_EMPTY; total = 0; }
    __syncthreads();
    {
        unsigned long long b = SCAN_EMPTY;
        int real = 0;
        for (int s = threadIdx.x; s < n_slabs; s += blockDim.x) {
            const uint64_t kth = L[s * step + k - 1];
            b = kth < b ? kth : b;
            real += scan_lower_bound(L + s * step, k, SCAN_EMPTY);
        }
        if (b != SCAN_EMPTY) atomicMin(&bound, b);
        if (real) atomicAdd(&total, real);
    }
    __syncthreads();
    const uint64_t top = bound;
    const int64_t words = (int64_t)n_slabs * k;
    for (int64_t w = threadIdx.x; w < words; w += blockDim.x) {
        const int s = (int)(w / k), j = (int)(w % k);
        const uint64_t e = L[s * step + j];
        if (e == SCAN_EMPTY || e > top) continue;
        int rank = 0;
        for (int o = 0; o < n_slabs && rank < k; ++o) rank += o == s ? j : scan_lower_bound(L + o * step, k, e);
        if (rank < k) {
            a.out_ids[q * k + rank] = (int32_t)(uint32_t)e + a.id_base;
            a.out_dist[q * k + rank] = hnsw_after::ord_inverse((uint32_t)(e >> 32));
        }
    }
    const int have = total < k ? total : k;
    for (int j = have + threadIdx.x; j < k; j += blockDim.x) {
        a.out_ids[q * k + j] = -1;
        a.out_dist[q * k + j] = a.fill == 0 ? __uint_as_float(0x7FC00000u) : __uint_as_float(0x7F800000u);
    }
    if (threadIdx.x == 0 && a.out_nd) exact_settle(a.out_nd, a.out_nh, a.out_stage, q, a.add, a.fresh != 0);
}

struct AfterSelectArgs {
    const int32_t *wids;       // [m][e] the stage's W per query (half rows / codes: re-ranked), id_base-based, ascending in (key, id),
    const float *wdist;        // [m][e]   filled entries < id_base
    int64_t m;
    int32_t e, k;
    const int32_t *map;        // [m] row i belongs to query map[i]; null: to query i
    const uint32_t *mask;      // null, or the allow-mask (ceil(n / 32) words)
    int64_t n;
    int32_t id_base;
    const uint64_t *lo;        // [nq] by query: the cursors as bounds in word space
    int32_t *out_ids;          // [nq][k]
    float *out_dist;
    LadderOut out;
};

// is entry j of the row a node, allowed, and after the cursor
__device__ __forceinline__ bool after_eligible(const AfterSelectArgs &a, MaskWords bits, uint64_t lo, const int32_t *wi, const float *wd, int j) {
    if (!is_node(a.n, a.id_base, wi[j]) || (a.mask && !node_allowed(bits, a.n, a.id_base, wi[j]))) return false;
    return hnsw_after::word(wd[j], (uint32_t)((int64_t)wi[j] - a.id_base)) > lo;
}

__global__ void __launch_bounds__(64)
after_select_kernel(const AfterSelectArgs a) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= a.m) return;
    const int64_t q = a.map ? a.map[i] : i;
    const MaskWords bits = mask_words(a.mask);
    const uint64_t lo = a.lo[q];
    const int32_t *const wi = a.wids + i * a.e;
    const float *const wd = a.wdist + i * a.e;
    int cnt = 0;
    for (int j0 = 0; j0 < a.e; j0 += 64) {
        const int j = j0 + lane;
        cnt += popc(ballot(j < a.e && after_eligible(a, bits, lo, wi, wd, j)));
    }
    const bool served = cnt >= a.k;
    if (served) {
        int at = 0;             // eligible members before this pass, in W's order
        for (int j0 = 0; j0 < a.e; j0 += 64) {
            const int j = j0 + lane;
            const bool ok = j < a.e && after_eligible(a, bits, lo, wi, wd, j);
            const uint64_t m = ballot(ok);
            if (ok) {
                int pos = at + popc(m & ((1ull << lane) - 1ull));
                // inside the run of equal D: the place by id among the run's eligible members
                const int32_t id = wi[j];
                const uint32_t db = __float_as_uint(wd[j]);
                for (int o = j - 1; o >= 0 && __float_as_uint(wd[o]) == db; --o)
                    if (wi[o] > id && after_eligible(a, bits, lo, wi, wd, o)) --pos;
                for (int o = j + 1; o < a.e && __float_as_uint(wd[o]) == db; ++o)
                    if (wi[o] < id && after_eligible(a, bits, lo, wi, wd, o)) ++pos;
                if (pos < a.k) {
                    a.out_ids[q * a.k + pos] = id;
                    a.out_dist[q * a.k + pos] = wd[j];
                }
            }
            at += popc(m);
            // k places are taken and no run goes on into the next pass: what follows lies behind them
            if (at >= a.k && (j0 + 64 >= a.e || __float_as_uint(wd[j0 + 63]) != __float_as_uint(wd[j0 + 64]))) break;
        }
    }
    if (lane == 0) ladder_settle(a.out, i, q, served);
}

} // namespace hnsw_dev

using hnsw_dev::IndexView;
using namespace hnsw_host;

namespace {

// The paged exact scan on st for the m rows of (Q, map) -- row i belongs to query map[i] (null: to query i) --, cut as the k-scan cuts
// its queries (scan_cut; the lists are the handle's scratch.scan): the first k eligible nodes under the paged order to the queries'
// rows of out_ids / out_dist, filled per `fill`.  out_nd (optional): the exact stage's counters too (AfterMergeArgs).
int after_scan(hnsw_index *idx, const float *Q, int64_t m, int64_t q_stride, const int32_t *map, int32_t k, int32_t fill, hipStream_t st,
               const uint32_t *mask, int32_t *out_ids, float *out_dist, uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_stage, uint32_t add,
               bool fresh) {
    const IndexView &iv = idx->iv;
    const ScanCut c = scan_cut(idx, m, k, 2 * (int64_t)k * 8, 16384);
    const uint64_t *const lo = (const uint64_t *)idx->after_scratch.lo.p;
    int rc;
    if ((rc = idx->scratch.scan.ensure((size_t)(c.piece * std::max<int64_t>(c.slabs, 1) * 2 * k * 8)))) return rc;
    for (int64_t q0 = 0; q0 < m; q0 += c.piece) {
        const int64_t nq = std::min(c.piece, m - q0);
        const hnsw_dev::AfterScanArgs a{{Q + q0 * q_stride, q_stride, nq, k, (int32_t)c.slabs, c.slab_rows, (uint64_t *)idx->scratch.scan.p}, lo, map, q0};
        if (c.slabs > 0) {
            with_metric(idx->info.metric, [&](auto METRIC) { with_nch(c.nch, [&](auto NCH) {
                if (mask) hipLaunchKernelGGL((hnsw_dev::hnsw_after_scan_kernel<NCH, METRIC, true>), c.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a, mask);
                else hipLaunchKernelGGL((hnsw_dev::hnsw_after_scan_kernel<NCH, METRIC, false>), c.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a, mask);
            }); });
            if ((rc = launched("paged scan kernel"))) return rc;
        }
        const hnsw_dev::AfterMergeArgs ma{a.s.lists, a.s.n_slabs, k, fill, iv.id_base, map, q0, out_ids, out_dist, out_nd, out_nh, out_stage, add, fresh};
        with_metric(idx->info.metric, [&](auto METRIC) {
            hipLaunchKernelGGL(hnsw_dev::after_merge_kernel<METRIC>, dim3((unsigned)nq), dim3(256), 0, st, ma);
        });
        if ((rc = launched("paged merge kernel"))) return rc;
    }
    return HNSW_OK;
}

// The ladder and the exact stage for a batch HostCall::begin has placed (b): the rows in b's, the stages in the filtered search's
// fb.stage on return.  f: the mask the call answers under (the caller's filter, else the live mask, else none).
int after_search(hnsw_index *idx, const hnsw_filter *f, const hnsw_search_params &p, const KnnBatch &b, float *d_stage, hipStream_t st) {
    FilterBufs &fb = idx->filter_scratch;
    const int k = p.k;
    const uint32_t *const mask = f ? (const uint32_t *)f->bits.p : nullptr;
    const int64_t n_allowed = f ? f->n_allowed : idx->iv.n;
    uint32_t *const d_stage_out = (uint32_t *)fb.stage.p;
    Ladder L(idx, b.Q, b.nq, b.q_stride, p.ef, p.semantics, d_stage, st, "paged search");
    LadderLeft left;
    int rc;
    // (fewer than k allowed nodes: no cursor leaves k eligible ones, every query is the exact stage's, unwalked)
    rc = L.run(n_allowed >= k, [&](Ladder &, int64_t m, int e) -> int {
        if ((rc = fb.wids.ensure((size_t)m * e * 4)) || (rc = fb.wdist.ensure((size_t)m * e * 4))) return rc;
        int32_t *const Wi = (int32_t *)fb.wids.p;
        float *const Wd = (float *)fb.wdist.p;
        if ((rc = L.walk_exact(Wi, Wd, HNSW_FILL_OHNSW))) return rc;
        const hnsw_dev::AfterSelectArgs sa{Wi, Wd, m, e, k, L.map, mask, idx->iv.n, idx->iv.id_base, (const uint64_t *)idx->after_scratch.lo.p, b.ids, b.dist,
                                           L.out(b.nd, b.nh, d_stage_out)};
        hipLaunchKernelGGL(hnsw_dev::after_select_kernel, dim3((unsigned)m), dim3(64), 0, st, sa);
        return launched("paged select kernel");
    }, left);
    if (rc || left == LadderLeft::none) return rc;
    // the L.m queries of (L.Qj, L.map): the batch the ladder left
    return after_scan(idx, L.Qj, L.m, L.qs, L.map, k, p.fill, st, mask, b.ids, b.dist, b.nd, b.nh, d_stage_out, (uint32_t)n_allowed, left == LadderLeft::fresh);
}

// what both entry points check of the cursors, on the host, before any launch
int check_cursors(const hnsw_cursor *after, int64_t nq) {
    if (!after) return HNSW_OK;
    for (int64_t q = 0; q < nq; ++q)
        if (std::isnan(after[q].dist)) return fail(HNSW_ERR_BAD_ARG, "after[%lld].dist is NaN", (long long)q);
    return HNSW_OK;
}

// both entry points once their arguments are checked (nq > 0).  params null: the brute-force form (k, fill)
int after_call(hnsw_index *idx, const hnsw_filter *f, const hnsw_cursor *after, const float *queries, int64_t nq, int64_t q_stride,
               const hnsw_search_params *params, int32_t k, int32_t fill, int32_t *out_ids, float *out_dist, hnsw_cursor *out_next,
               uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage) {
    HIP_TRY(hipSetDevice(idx->device));
    const hnsw_cursor start = HNSW_CURSOR_START;
    const int32_t id_base = idx->iv.id_base;
    std::vector<uint64_t> lo((size_t)nq);
    for (int64_t q = 0; q < nq; ++q) {
        const hnsw_cursor &c = after ? after[q] : start;
        lo[(size_t)q] = hnsw_after::cursor_word(c.dist, c.id, id_base);
    }
    int rc;
    if ((rc = idx->after_scratch.lo.ensure((size_t)nq * 8)) || (rc = idx->filter_scratch.stage.ensure((size_t)nq * 4))) return rc;
    rc = ladder_host_call(idx, queries, nq, q_stride, k, out_ids, out_dist, out_ndist, out_nhops, params ? out_stage : nullptr, params != nullptr, nullptr,
                          nullptr, nullptr, nullptr, params ? "paged search" : "paged scan", [&](const KnnBatch &b, float *d_stage, hipStream_t st) -> int {
        if (hipMemcpyAsync(idx->after_scratch.lo.p, lo.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(HNSW_ERR_HIP, "cursor upload failed");
        if (params) return after_search(idx, f, *params, b, d_stage, st);
        return after_scan(idx, b.Q, nq, q_stride, nullptr, k, fill, st, f ? (const uint32_t *)f->bits.p : nullptr, b.ids, b.dist, nullptr, nullptr, nullptr, 0u,
                          true);
    });
    if (rc) return rc;
    if (out_next)
        for (int64_t q = 0; q < nq; ++q) {
            const hnsw_cursor &in = after ? after[q] : start;
            hnsw_after::next_cursor(out_ids + q * k, out_dist + q * k, k, id_base, in.dist, in.id, &out_next[q].dist, &out_next[q].id);
        }
    return HNSW_OK;
}

} // namespace

extern "C" {

int32_t hnsw_search_batch_after(hnsw_index *idx, const hnsw_filter *f, const hnsw_cursor *after, const float *queries, int64_t nq, int64_t q_stride,
                                const hnsw_search_params *params, int32_t *out_ids, float *out_dist, hnsw_cursor *out_next, uint32_t *out_ndist,
                                uint32_t *out_nhops, uint32_t *out_stage) {
    int rc = check_batch(idx, params, nq, q_stride, queries && out_ids && out_dist);
    if (rc) return rc;
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "the k farthest of W (HNSW_SEM_FUNCTOR_NEAREST_K) have no paged meaning");
    if (f && (rc = check_filter(idx, f))) return rc;
    if ((rc = check_cursors(after, nq))) return rc;
    if (nq == 0) return HNSW_OK;
    return after_call(idx, f ? f : live_filter(idx), after, queries, nq, q_stride, params, params->k, params->fill, out_ids, out_dist, out_next,
                      out_ndist, out_nhops, out_stage);
}

int32_t hnsw_brute_force_batch_after(hnsw_index *idx, const hnsw_filter *f, const hnsw_cursor *after, const float *queries, int64_t nq,
                                     int64_t q_stride, int32_t k, int32_t fill, int32_t *out_ids, float *out_dist, hnsw_cursor *out_next) {
    int rc = check_scan(idx, nq, q_stride, k, fill, queries && out_ids && out_dist);
    if (rc) return rc;
    if (f && (rc = check_filter(idx, f))) return rc;
    if ((rc = check_cursors(after, nq))) return rc;
    if (nq == 0) return HNSW_OK;
    return after_call(idx, f ? f : live_filter(idx), after, queries, nq, q_stride, nullptr, k, fill, out_ids, out_dist, out_next, nullptr, nullptr, nullptr);
}

} // extern "C"
