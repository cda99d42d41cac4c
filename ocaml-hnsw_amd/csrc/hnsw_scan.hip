// hnsw_scan.hip -- the exact k-nearest scan: brute_force_knn_l2 (benchmark/dataset.ml:15-30) over the float32 rows an index
// holds, with the index's metric and the search kernels' own arithmetic (hnsw_brute_force_batch / _device).
//
// Three kernels.
//   hnsw_scan_kernel<NCH, METRIC>: the scan body of hnsw_scan_device.hip.h (grid, tile, rows in flight, the distance bits) with
//     the top-k selection below (ScanTopK).  A candidate is the 64-bit word (ordered distance key << 32 | node): ascending words
//     = the total order (distance, id).  Per query the wave holds the word of the k-th smallest candidate its slab has shown so
//     far (all ones until there are k); the common path is ONE compare of the new key against that word's upper half, for the
//     wave's four rows at once.  Survivors are appended to the query's 64-entry LDS buffer; a buffer that may not take another
//     round is merged into the query's sorted list of k words in global memory (scan_flush: never drops a word that is among the
//     k smallest, never gives up), which lowers the threshold.  The list lives in two halves, read from one and written to the
//     other.
//   hnsw_scan_masked_kernel<NCH, METRIC>: the same scan over the rows an allow-mask names (the exact stage of the filtered
//     searches, hnsw_filter.hip): ScanTopK<NCH, true>, its mask taken per tile of queries from a table of masks (a table of one
//     for hnsw_search_batch_filtered; hnsw_search_batch_filtered_each lays its queries out so that no tile spans two filters).
//   hnsw_scan_merge_kernel<METRIC>: one workgroup per query merges the slabs' lists under the same order and writes ids
//     (+ id_base), distances (key_to_dist) and the fill.
// Nothing here depends on how the rows are cut into slabs or the queries into tiles: every list is the exact k smallest of its
// slab, and the merge takes the exact k smallest of their union.
#include "hnsw_internal.h"
#include "hnsw_scan_device.hip.h"

namespace hnsw_dev {

// (SCAN_BUF, SCAN_EMPTY, ScanArgs, scan_flush and its helpers: hnsw_scan_device.hip.h -- the paged scan, hnsw_after.hip, keeps its lists the same way)

// The top-k selection of one (tile, slab) wave (scan_slab's Select).  MASKED: only the rows the mask allows (skip and admits: ScanMask).
template <int NCH, bool MASKED> struct ScanTopK : ScanMask<MASKED> {
    static constexpr int T = scan_tile(NCH);
    static constexpr int LIMIT = SCAN_BUF - 4 * scan_rows(NCH);   // a buffer up to here takes the survivors of one more pass over the UB batches
    const ScanArgs &a;
    // per query of the tile: its list's two halves, which half is current (bit t of par), the threshold word, the buffer's fill
    uint64_t (*bufs)[SCAN_BUF], *sorted, *lists0;
    int64_t list_step;
    uint64_t thr[T];
    int cnt[T], tq, lane;
    uint32_t par;
    bool full;

    __device__ __forceinline__ ScanTopK(const ScanArgs &a_, const uint32_t *mask_) : ScanMask<MASKED>(mask_), a(a_) {}
    __device__ __forceinline__ void begin(int64_t q0, int tq_, int64_t slab) {
        __shared__ uint64_t bufs_all[SCAN_WAVES][T][SCAN_BUF];
        __shared__ uint64_t sorted_all[SCAN_WAVES][SCAN_BUF];
        lane = threadIdx.x & 63;
        bufs = bufs_all[threadIdx.x >> 6];
        sorted = sorted_all[threadIdx.x >> 6];
        tq = tq_;
        lists0 = a.lists + ((q0 * a.n_slabs + slab) * 2) * (int64_t)a.k;
        list_step = (int64_t)a.n_slabs * 2 * a.k;
        par = 0;
        full = false;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            // a query past the tile's end never has a survivor (no word is below 0)
            thr[t] = t < tq ? SCAN_EMPTY : 0ull;
            cnt[t] = 0;
            if (t < tq) for (int j = lane; j < a.k; j += 64) lists0[t * list_step + j] = SCAN_EMPTY;
        }
        scan_wave_sync();
    }
    __device__ __forceinline__ void take(int t, uint32_t key, int64_t row, bool ok) {
        if (ballot(key <= (uint32_t)(thr[t] >> 32))) {           // rare: some row of the four may be among the k smallest
            const uint64_t e = ((uint64_t)key << 32) | (uint32_t)row;
            const bool in = (lane & 15) == 0 && ok && e < thr[t];
            const uint64_t m = ballot(in);
            if (in) bufs[t][cnt[t] + popc(m & ((1ull << lane) - 1ull))] = e;
            cnt[t] += popc(m);
            full = full || cnt[t] > LIMIT;
        }
    }
    // merges query t's buffer into its list, which lowers its threshold
    __device__ __forceinline__ void flush(int t) {
        uint64_t *const A = lists0 + t * list_step;
        const bool p = (par >> t) & 1u;
        scan_flush(bufs[t], sorted, cnt[t], A + (p ? a.k : 0), A + (p ? 0 : a.k), a.k, lane);
        par ^= 1u << t;
        cnt[t] = 0;
        thr[t] = scan_uniform64((A + (p ? 0 : a.k))[a.k - 1]);
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
            if ((par >> t) & 1u) for (int j = lane; j < a.k; j += 64) A[j] = A[a.k + j];
        }
    }
};

template <int NCH, int METRIC>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_scan_kernel(const IndexView iv, const ScanArgs a) {
    ScanTopK<NCH, false> sel(a, nullptr);
    scan_slab<NCH, METRIC>(iv, a.Q, a.q_stride, a.nq, a.n_slabs, a.slab_rows, sel);
}

// ... restricted to the rows a mask allows (the filtered searches' exact stage).  The mask is the tile's: masks[tile_filter[tile0 +
// blockIdx.x]], masks[0] without a tile_filter; tile0 = the number of the launch's first tile among the call's.  Both loads are
// scalar (blockIdx.x is the tile), so skip and admits stay wave-uniform tests of one mask.
template <int NCH, int METRIC>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_scan_masked_kernel(const IndexView iv, const ScanArgs a, const uint32_t *const *masks, const int32_t *tile_filter, int64_t tile0) {
    ScanTopK<NCH, true> sel(a, masks[tile_filter ? tile_filter[tile0 + blockIdx.x] : 0]);
    scan_slab<NCH, METRIC>(iv, a.Q, a.q_stride, a.nq, a.n_slabs, a.slab_rows, sel);
}

// One workgroup per query.  lists: [nq][n_slabs][2][k], the first half of each the slab's k smallest words, ascending, padded.
// No word above the smallest of the lists' k-th words can be among the k smallest of the union (that list alone has k words
// not above it), so only the words up to it are ranked: a word's place is the number of smaller words over all lists.
// row_query (optional, [nq]): a query whose entry is negative is a padding row of the caller's layout: nothing is merged or written.
template <int METRIC>
__global__ void __launch_bounds__(256)
hnsw_scan_merge_kernel(const uint64_t *lists, int32_t n_slabs, int32_t k, int32_t fill, int32_t id_base, int32_t *out_ids, float *out_dist,
                       const int32_t *row_query) {
    __shared__ unsigned long long bound;
    __shared__ int total;
    const int64_t q = blockIdx.x;
    if (row_query && row_query[q] < 0) return;      // (the whole workgroup: before the first barrier)
    const uint64_t *L = lists + q * n_slabs * 2 * (int64_t)k;
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
            out_ids[q * k + rank] = (int32_t)(uint32_t)e + id_base;
            out_dist[q * k + rank] = key_to_dist<METRIC>((uint32_t)(e >> 32));
        }
    }
    const int have = total < k ? total : k;
    for (int j = have + threadIdx.x; j < k; j += blockDim.x) {
        out_ids[q * k + j] = -1;
        out_dist[q * k + j] = fill == 0 ? __uint_as_float(0x7FC00000u) : __uint_as_float(0x7F800000u);
    }
}

} // namespace hnsw_dev

namespace hnsw_host {

using hnsw_dev::IndexView;
using hnsw_dev::ScanArgs;

// the cut of an exact scan of m queries of this index (scan_plan) and the tile its kernels take; grid: a launch of nq <= piece queries
ScanCut scan_cut(const hnsw_index *idx, int64_t m, int k, int64_t cell_bytes, int64_t cap) {
    const int nch = pick_nch(idx->iv.nchunks), T = hnsw_dev::scan_tile(nch);
    return {scan_plan(idx->iv.n, idx->scan_slabs, T, m, k, cell_bytes, cap), nch, T};
}
dim3 ScanCut::grid(int64_t nq) const {
    return dim3((unsigned)((nq + T - 1) / T), (unsigned)((slabs + hnsw_dev::SCAN_WAVES - 1) / hnsw_dev::SCAN_WAVES));
}

int check_scan(const hnsw_index *idx, int64_t nq, int64_t q_stride, int32_t k, int32_t fill, bool buffers) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (k < 1) return fail(HNSW_ERR_BAD_ARG, "k must be >= 1 (k=%d)", k);
    if (k > 1024) return fail(HNSW_ERR_UNSUPPORTED, "k=%d > 1024 not supported", k);
    if (fill != HNSW_FILL_OHNSW && fill != HNSW_FILL_BA) return fail(HNSW_ERR_BAD_ARG, "bad fill %d", fill);
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    if (nq == 0) return HNSW_OK;
    if (!buffers) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    if (q_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "q_stride < d");
    return HNSW_OK;
}

// the scan of b's queries on `st`: the queries in pieces whose lists (two halves of k words per cell) fit SCAN_SCRATCH
int scan_search(hnsw_index *idx, const KnnBatch &b, int32_t k, int32_t fill, hipStream_t st, const uint32_t *const *masks, const int32_t *tile_filter,
                const int32_t *row_query) {
    int rc = check_scan(idx, b.nq, b.q_stride, k, fill, b.Q && b.ids && b.dist);
    if (rc || b.nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    const IndexView &iv = idx->iv;
    const ScanCut c = scan_cut(idx, b.nq, k, 2 * (int64_t)k * 8, 16384);
    if ((rc = idx->scratch.scan.ensure((size_t)(c.piece * std::max<int64_t>(c.slabs, 1) * 2 * k * 8)))) return rc;
    for (int64_t q0 = 0; q0 < b.nq; q0 += c.piece) {
        const int64_t nq = std::min(c.piece, b.nq - q0);
        // a piece's first query is its first tile's first: scan_plan cuts pieces of a multiple of T queries (or makes one piece), so
        // tile q0 / T of the call is tile 0 of this launch and tile_filter, numbered over the call's tiles, can be read from there
        if (q0 % c.T) return fail(HNSW_ERR_HIP, "scan piece of %lld queries is no multiple of the tile (%d)", (long long)c.piece, c.T);
        ScanArgs a{b.Q + q0 * b.q_stride, b.q_stride, nq, k, (int32_t)c.slabs, c.slab_rows, (uint64_t *)idx->scratch.scan.p};
        if (c.slabs > 0) {
            with_metric(idx->info.metric, [&](auto METRIC) { with_nch(c.nch, [&](auto NCH) {
                if (masks) hipLaunchKernelGGL((hnsw_dev::hnsw_scan_masked_kernel<NCH, METRIC>), c.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a, masks, tile_filter, q0 / c.T);
                else hipLaunchKernelGGL((hnsw_dev::hnsw_scan_kernel<NCH, METRIC>), c.grid(nq), dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a);
            }); });
            if ((rc = launched("scan kernel"))) return rc;
        }
        with_metric(idx->info.metric, [&](auto METRIC) {
            hipLaunchKernelGGL(hnsw_dev::hnsw_scan_merge_kernel<METRIC>, dim3((unsigned)nq), dim3(256), 0, st, a.lists, a.n_slabs, k, fill, iv.id_base, b.ids + q0 * k, b.dist + q0 * k,
                               row_query ? row_query + q0 : nullptr);
        });
        if ((rc = launched("scan merge kernel"))) return rc;
    }
    return HNSW_OK;
}

} // namespace hnsw_host

using namespace hnsw_host;

extern "C" {

int32_t hnsw_brute_force_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                                      int32_t *d_ids, float *d_dist, void *stream) {
    // (while nodes are marked deleted: the k smallest LIVE nodes, the masked scan under the handle's live mask)
    const hnsw_filter *const live = idx ? live_filter(idx) : nullptr;
    if (idx && is_cosine(idx)) {            // N(Q) on the caller's stream first
        int rc = check_scan(idx, nq, q_stride, k, fill, d_queries && d_ids && d_dist);
        if (rc || nq == 0) return rc;
        HIP_TRY(hipSetDevice(idx->device));
        if ((rc = cosine_queries(idx, d_queries, nq, q_stride, (hipStream_t)stream, &d_queries, &q_stride))) return rc;
    }
    return scan_search(idx, {d_queries, nq, q_stride, d_ids, d_dist, nullptr, nullptr, nullptr, nullptr}, k, fill, (hipStream_t)stream,
                       live ? live->table() : nullptr);
}

int32_t hnsw_brute_force_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                               int32_t *out_ids, float *out_dist) {
    int rc = check_scan(idx, nq, q_stride, k, fill, queries && out_ids && out_dist);
    if (rc || nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    HostCall c;
    if ((rc = c.begin(idx, queries, nq, q_stride, k, out_ids, out_dist, nullptr, nullptr, false))) return rc;
    const hnsw_filter *const live = live_filter(idx);
    rc = scan_search(idx, c.b, k, fill, idx->hs[0], live ? live->table() : nullptr);
    if (rc) { (void)hipStreamSynchronize(idx->hs[0]); return rc; }
    return c.finish(idx, "scan", idx->hs[0]);
}

} // extern "C"
