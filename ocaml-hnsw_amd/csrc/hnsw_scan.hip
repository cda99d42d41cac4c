// hnsw_scan.hip -- the exact k-nearest scan: brute_force_knn_l2 (benchmark/dataset.ml:15-30) over the float32 rows an index
// holds, with the index's metric and the search kernels' own arithmetic (hnsw_brute_force_batch / _device).
//
// Three kernels.
//   hnsw_scan_kernel<NCH, METRIC>: grid (query tiles) x (groups of SCAN_WAVES row slabs), one wave per (tile, slab).  A wave
//     keeps the chunks of the T queries of its tile in registers (NCH <= 4) or shares them with the other waves of its
//     workgroup through LDS (NCH >= 8, as hnsw_distance_kernel does) and walks the rows of its slab in id order, 4 * UB rows
//     in flight: one 16-lane group per row, lane l16 on the float4 chunks l16, l16 + 16, ... -- the lane grid, the fmaf chain
//     and the reduce16 tree of every other kernel here, so the sums are the same bits.  Every row chunk loaded is used for all
//     T queries.  The workgroups of one slab group are consecutive in dispatch order (blockIdx.x is the tile), so the rows of
//     a slab are fetched from HBM once per XCD and otherwise come out of L2.
//     Selection: a candidate is the 64-bit word (ordered distance key << 32 | node): ascending words = the total order
//     (distance, id).  Per query the wave holds the word of the k-th smallest candidate its slab has shown so far (all ones
//     until there are k); the common path is ONE compare of the new key against that word's upper half, for the wave's four
//     rows at once.  Survivors are appended to the query's 64-entry LDS buffer; a buffer that may not take another round
//     is merged into the query's sorted list of k words in global memory (scan_flush: never drops a word that is among the
//     k smallest, never gives up), which lowers the threshold.  The list lives in two halves, read from one and written
//     to the other.
//   hnsw_scan_masked_kernel<NCH, METRIC>: the same scan over the rows an allow-mask names (hnsw_search_batch_filtered's exact
//     stage, hnsw_filter.hip).  Both kernels are the one body of hnsw_scan_slab.inc, so that the unmasked one stays the code it was.
//   hnsw_scan_merge_kernel<METRIC>: one workgroup per query merges the slabs' lists under the same order and writes ids
//     (+ id_base), distances (key_to_dist) and the fill.
// Nothing here depends on how the rows are cut into slabs or the queries into tiles: every list is the exact k smallest of its
// slab, and the merge takes the exact k smallest of their union.
#include "hnsw_internal.h"

namespace hnsw_dev {

constexpr int SCAN_WAVES = 4;          // waves per workgroup, one slab each
constexpr int SCAN_BUF = 64;           // survivor words per query and wave (LDS)
constexpr uint64_t SCAN_EMPTY = ~0ull; // no candidate: above every real word
// queries per tile: T * NCH * 4 VGPRs hold them for NCH <= 4 (64 at most); through LDS the tile costs T * NCH * 256 bytes
__host__ __device__ constexpr int scan_tile(int nch) { return nch <= 2 ? 8 : nch == 4 ? 4 : 8; }
// batches of four rows in flight per wave: UB * NCH * 4 VGPRs
__host__ __device__ constexpr int scan_rows(int nch) { return nch == 1 ? 4 : nch <= 4 ? 2 : 1; }

// waves per SIMD the register allocator must leave room for
__host__ __device__ constexpr int scan_min_waves(int nch) { return nch == 1 || nch == 8 ? 4 : nch == 16 ? 2 : 3; }

struct ScanArgs {
    const float *Q;        // the queries of this launch
    int64_t q_stride, nq;
    int32_t k, n_slabs;
    int64_t slab_rows;     // slab s = rows [s * slab_rows, min(n, (s + 1) * slab_rows))
    uint64_t *lists;       // [nq][n_slabs][2][k]: the first half holds the result
};

// what one lane wrote to LDS or global memory, seen by the other lanes of its wave
__device__ __forceinline__ void scan_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint64_t scan_uniform64(uint64_t v) {
    return ((uint64_t)(uint32_t)uniform((int)(v >> 32)) << 32) | (uint32_t)uniform((int)(uint32_t)v);
}
// number of words below e in the ascending words p[0 .. n)
__device__ __forceinline__ int scan_lower_bound(const uint64_t *p, int n, uint64_t e) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p[mid] < e) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Merges the cnt (<= 64, distinct) words of buf into the ascending list cur[0 .. k) (padded with SCAN_EMPTY); the k smallest of
// the union go to oth[0 .. k), ascending and padded.  sorted: 64 words of LDS scratch.  The words are distinct (a node occurs
// once), so a word's place in the union is its place in its own sequence plus the number of smaller words in the other one.
__device__ __forceinline__ void scan_flush(const uint64_t *buf, uint64_t *sorted, int cnt, const uint64_t *cur, uint64_t *oth,
                                           int k, int lane) {
    scan_wave_sync();
    const uint64_t e = lane < cnt ? buf[lane] : SCAN_EMPTY;
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += buf[j] < e ? 1 : 0;
    if (lane < cnt) sorted[rank] = e;
    scan_wave_sync();
    if (lane < cnt) {
        const int pos = rank + scan_lower_bound(cur, k, e);
        if (pos < k) oth[pos] = e;
    }
    for (int j = lane; j < k; j += 64) {
        const uint64_t le = cur[j];
        const int pos = j + scan_lower_bound(sorted, cnt, le);   // (padding: all cnt words are below it)
        if (pos < k) oth[pos] = le;
    }
    scan_wave_sync();
}

template <int NCH, int METRIC>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_scan_kernel(const IndexView iv, const ScanArgs a) {
#define SCAN_MASKED 0
#include "hnsw_scan_slab.inc"
#undef SCAN_MASKED
}

// ... restricted to the rows a mask allows (hnsw_search_batch_filtered's exact stage)
template <int NCH, int METRIC>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_scan_masked_kernel(const IndexView iv, const ScanArgs a, const uint32_t *mask) {
#define SCAN_MASKED 1
#include "hnsw_scan_slab.inc"
#undef SCAN_MASKED
}

// One workgroup per query.  lists: [nq][n_slabs][2][k], the first half of each the slab's k smallest words, ascending, padded.
// No word above the smallest of the lists' k-th words can be among the k smallest of the union (that list alone has k words
// not above it), so only the words up to it are ranked: a word's place is the number of smaller words over all lists.
template <int METRIC>
__global__ void __launch_bounds__(256)
hnsw_scan_merge_kernel(const uint64_t *lists, int32_t n_slabs, int32_t k, int32_t fill, int32_t id_base, int32_t *out_ids, float *out_dist) {
    __shared__ unsigned long long bound;
    __shared__ int total;
    const int64_t q = blockIdx.x;
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

hipError_t launch_scan(int metric, int nch, dim3 grid, const IndexView &iv, const ScanArgs &a, const uint32_t *mask, hipStream_t st) {
    with_metric(metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
        if (mask) hipLaunchKernelGGL((hnsw_dev::hnsw_scan_masked_kernel<NCH, METRIC>), grid, dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a, mask);
        else hipLaunchKernelGGL((hnsw_dev::hnsw_scan_kernel<NCH, METRIC>), grid, dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a);
    }); });
    return hipGetLastError();
}

// How the table is cut for a launch of `tiles` query tiles: enough (tile, slab) waves to fill the chip twice over, slabs of 256
// rows at least, no more lists per query than the merge reads quickly (slabs * k <= 65 536, 1024 slabs).  Option "scan_slabs"
// overrides the count.  Results do not depend on it.
int64_t scan_slab_rows(const hnsw_index *idx, int64_t tiles, int k) {
    constexpr int64_t SCAN_TARGET_WAVES = 8192;
    const int64_t n = idx->iv.n;
    int64_t slabs = idx->scan_slabs > 0 ? idx->scan_slabs : (SCAN_TARGET_WAVES + tiles - 1) / tiles;
    if (idx->scan_slabs <= 0) slabs = std::min(slabs, std::max<int64_t>(1, n / 256));
    slabs = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slabs, 1024), std::max<int64_t>(1, 65536 / k)));
    return std::max<int64_t>(1, (n + slabs - 1) / slabs);
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

// the scan of b's queries on `st`: the queries in pieces whose lists fit SCAN_SCRATCH bytes of the handle's scratch
int scan_search(hnsw_index *idx, const KnnBatch &b, int32_t k, int32_t fill, hipStream_t st, const uint32_t *mask) {
    int rc = check_scan(idx, b.nq, b.q_stride, k, fill, b.Q && b.ids && b.dist);
    if (rc || b.nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    constexpr int64_t SCAN_SCRATCH = 256ll << 20;
    const IndexView &iv = idx->iv;
    const int nch = pick_nch(iv.nchunks), T = hnsw_dev::scan_tile(nch);
    int64_t piece = std::min<int64_t>(b.nq, 16384);
    int64_t slab_rows = 0, slabs = 0;
    for (;;) {      // (a smaller piece has fewer tiles and may be cut into more slabs: settle on a piece that fits)
        slab_rows = scan_slab_rows(idx, (piece + T - 1) / T, k);
        slabs = iv.n > 0 ? (iv.n + slab_rows - 1) / slab_rows : 0;
        const int64_t per_query = std::max<int64_t>(slabs, 1) * 2 * k * 8;
        if (piece * per_query <= SCAN_SCRATCH || piece <= T) break;
        piece = std::max<int64_t>(T, SCAN_SCRATCH / per_query / T * T);
    }
    if ((rc = idx->scratch.scan.ensure((size_t)(piece * std::max<int64_t>(slabs, 1) * 2 * k * 8)))) return rc;
    for (int64_t q0 = 0; q0 < b.nq; q0 += piece) {
        const int64_t nq = std::min(piece, b.nq - q0);
        ScanArgs a{b.Q + q0 * b.q_stride, b.q_stride, nq, k, (int32_t)slabs, slab_rows, (uint64_t *)idx->scratch.scan.p};
        if (slabs > 0) {
            const dim3 grid((unsigned)((nq + T - 1) / T), (unsigned)((slabs + hnsw_dev::SCAN_WAVES - 1) / hnsw_dev::SCAN_WAVES));
            const hipError_t e = launch_scan(idx->info.metric, nch, grid, iv, a, mask, st);
            if (e != hipSuccess) return fail(HNSW_ERR_HIP, "scan kernel launch failed: %s", hipGetErrorString(e));
        }
        with_metric(idx->info.metric, [&](auto METRIC) {
            hipLaunchKernelGGL(hnsw_dev::hnsw_scan_merge_kernel<METRIC>, dim3((unsigned)nq), dim3(256), 0, st, a.lists, a.n_slabs, k, fill, iv.id_base, b.ids + q0 * k, b.dist + q0 * k);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(HNSW_ERR_HIP, "scan merge kernel launch failed: %s", hipGetErrorString(e));
    }
    return HNSW_OK;
}

} // namespace hnsw_host

using namespace hnsw_host;

extern "C" {

int32_t hnsw_brute_force_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                                      int32_t *d_ids, float *d_dist, void *stream) {
    return scan_search(idx, {d_queries, nq, q_stride, d_ids, d_dist, nullptr, nullptr, nullptr, nullptr}, k, fill, (hipStream_t)stream);
}

int32_t hnsw_brute_force_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t fill,
                               int32_t *out_ids, float *out_dist) {
    int rc = check_scan(idx, nq, q_stride, k, fill, queries && out_ids && out_dist);
    if (rc || nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    HostCall c;
    if ((rc = c.begin(idx, queries, nq, q_stride, k, out_ids, out_dist, nullptr, nullptr, false))) return rc;
    rc = scan_search(idx, c.b, k, fill, idx->hs[0]);
    if (rc) { (void)hipStreamSynchronize(idx->hs[0]); return rc; }
    return c.finish(idx, "scan", idx->hs[0]);
}

} // extern "C"
