// hnsw_scan_matrix.hip -- the exact k-nearest scan of float rows through fp32 matrix instructions (option "scan_matrix").
//
// The float scan's key comes from a fixed fmaf chain per 16-lane group and the reduce16 tree (hnsw_scan_device.hip.h); no matrix
// instruction sums in that order.  So the matrix unit never makes a key here.  It SCREENS: per (row, query) pair it yields a proven
// bound (hnsw_scan_matrix_plan.h) and a pair is dropped only when that bound shows its exact key above the
// query's current k-th word.  Every pair that is not dropped is evaluated by the scan's own chain (scan_chain, reduce16,
// dist_to_key) and enters the lists with that key: the lists, scan_flush and hnsw_scan_merge_kernel are the float scan's, and so
// are the ids and the distance bits.  Only the speed depends on the bound being tight.
//
// Two kernels in front of the unchanged float kernels and hnsw_scan_merge_kernel.
//   hnsw_scan_matrix_queries_kernel<METRIC>: one wave per query.  Writes the query's term of the screen (its squared norm folded
//     with the margin) and -- the last wave to finish -- the handle's path word: 3 when every value of the launch's queries is
//     finite, else 1 (the float kernels, launched behind with the same lists, return unless it is 1).  The range scan's matrix
//     kernel (hnsw_range_matrix.hip) takes its query terms and its path word from the same prepass (scan_matrix_prepass).
//   hnsw_scan_matrix_kernel<NCH, METRIC, MASKED>: grid (tiles of 32 queries) x (groups of slabs), one wave per (tile, slab),
//     scan_matrix_waves(NCH) waves per workgroup.  Rows are taken as 64 * NCH floats wide (NCH = pick_nch, at most 8: d <= 512).
//     Tile, operands, pipeline, row norms, screen: scan_matrix_load_tile and scan_matrix_walk (hnsw_scan_matrix_device.hip.h has
//       the lane maps), which the range scan's matrix kernel walks too: the tile's 32 queries in LDS, 32-row blocks straight from
//       global memory, one multiply-add (L2) or subtract (IP) and one compare per accumulator against the lane's bound.
//     Survivors go, as bare row numbers, into the query's 64-word LDS buffer.  A buffer that may not take another block (and, at
//       the slab's end, every buffer) gets its exact keys: one 16-lane group per pair, eight pairs a round, the row read again
//       (from L2) and the query's chunks from the tile.  A word not below the query's k-th word is discarded, the others are
//       packed in place and merged into the query's list by scan_flush, and the bound is refreshed.  (The k-th word changes only
//       at a merge, so an earlier key would drop nothing more.)
#include "hnsw_internal.h"
#include "hnsw_scan_matrix_device.hip.h"

namespace hnsw_dev {

using namespace hnsw_host;      // the plan header's constants and the rule

struct ScanMatrixArgs {
    const float *X;        // [n][stride] zero-padded rows
    int64_t stride, n;
    int32_t d, nchunks;
    const float *Q;        // the queries of this launch
    int64_t q_stride, nq;
    const float *qterm;    // [nq] as the prepass wrote them
    int32_t k, n_slabs;
    int64_t slab_rows;
    uint64_t *lists;
    const uint32_t *path;  // the handle's path word
    float eps;             // scan_matrix_eps(d)
};

// state: the byte prepass's three words (hnsw_scan_bytes.hip): [0] the path word, [1] "a value was not finite" of the launch in
// flight, [2] its finished waves.  One exact scan is in flight per handle.
template <int METRIC>
__global__ void __launch_bounds__(256)
hnsw_scan_matrix_queries_kernel(const float *Q, int64_t q_stride, int64_t nq, int32_t d, float eps, float *qterm, uint32_t *state) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    bool ok = true;
    if (q < nq) {
        float s = 0.f;
        for (int e = lane; e < d; e += 64) {
            const float v = Q[q * q_stride + e];
            ok = ok && __builtin_fabsf(v) <= FLT_MAX;
            s = __builtin_fmaf(v, v, s);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) qterm[q] = scan_matrix_query_term(METRIC, s, eps);
    }
    const bool bad = ballot(!ok) != 0ull;
    if (lane == 0) scan_prepass_publish(state, bad, (uint32_t)SCAN_PATH_MATRIX);
}

// the bound a lane compares its accumulators' screen values against: from the query's k-th word so far and the query's term
template <int METRIC> __device__ __forceinline__ float scan_matrix_lane_bound(uint64_t thr, float qterm) {
    if (thr == SCAN_EMPTY) return __builtin_inff();         // fewer than k words so far: every row survives
    const uint32_t key = (uint32_t)(thr >> 32);
    return scan_matrix_bound(METRIC, METRIC == 0 ? __uint_as_float(key) : key_to_dist<1>(key), qterm);
}

template <int NCH, int METRIC, bool MASKED>
__global__ void __launch_bounds__(64 * scan_matrix_waves(NCH))
hnsw_scan_matrix_kernel(const ScanMatrixArgs a, const uint32_t *const *masks) {
    constexpr int T = SCAN_MATRIX_TILE, W = scan_matrix_waves(NCH);
    constexpr int PITCH = scan_matrix_pitch(NCH);
    static_assert(SCAN_BUF == 64 && SCAN_MATRIX_WAVE_BYTES == T * SCAN_BUF * 8 + SCAN_BUF * 8 + T * 4 + 32 * 4, "the plan header's LDS");
    __shared__ __attribute__((aligned(16))) float tile[T * PITCH];
    __shared__ uint64_t bufs_all[W][T][SCAN_BUF];
    __shared__ uint64_t sorted_all[W][SCAN_BUF];
    __shared__ int cnt_all[W][T];
    __shared__ __attribute__((aligned(16))) float rterm_all[W][32];
    if (*a.path != (uint32_t)SCAN_PATH_MATRIX) return;          // (the whole workgroup: before the barrier)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31;                    // the lane's query column
    const int64_t q0 = (int64_t)blockIdx.x * T;
    const int tq = (int)(a.nq - q0 < T ? a.nq - q0 : T);
    scan_matrix_load_tile<NCH, W>(tile, a.Q, a.q_stride, q0, tq, a.d);
    __syncthreads();
    const int64_t slab = (int64_t)blockIdx.y * W + uniform(wave);
    if (slab >= a.n_slabs) return;              // (after the only workgroup barrier)
    const int64_t r0 = slab * a.slab_rows, r1 = r0 + a.slab_rows < a.n ? r0 + a.slab_rows : a.n;
    const MaskWords mask = mask_words(MASKED ? masks[0] : nullptr);
    uint64_t (*const bufs)[SCAN_BUF] = bufs_all[wave];
    uint64_t *const sorted = sorted_all[wave];
    int *const cnt = cnt_all[wave];
    float *const rterm = rterm_all[wave];
    const int nchunks = a.nchunks;

    const float cq = j < tq ? a.qterm[q0 + j] : 0.f;
    uint64_t *const lists0 = a.lists + ((q0 * a.n_slabs + slab) * 2) * (int64_t)a.k;
    const int64_t list_step = (int64_t)a.n_slabs * 2 * a.k;
    for (int t = 0; t < tq; ++t) for (int i = lane; i < a.k; i += 64) lists0[t * list_step + i] = SCAN_EMPTY;
    if (lane < T) cnt[lane] = 0;
    scan_wave_sync();
    uint64_t thr = j < tq ? SCAN_EMPTY : 0ull;                  // the query's k-th word so far (no word is below 0)
    float bound = j < tq ? __builtin_inff() : -__builtin_inff();
    uint32_t par = 0;                                           // bit t: query t's current list is the second half

    // merges query t's buffer of c words into its list
    auto flush = [&](int t, int c) {
        if (c == 0) { if (lane == 0) cnt[t] = 0; return; }
        uint64_t *const A = lists0 + t * list_step;
        const bool p = (par >> t) & 1u;
        scan_flush(bufs[t], sorted, c, A + (p ? a.k : 0), A + (p ? 0 : a.k), a.k, lane);
        par ^= 1u << t;
        if (lane == 0) cnt[t] = 0;
    };
    // The c bare row numbers of query t's buffer get their exact keys, eight pairs a round (one 16-lane group per pair, two pairs per
    // group so that two rows' loads are in flight); a word not below the query's k-th word is discarded, the others are packed in
    // place, never ahead of what the round read.  Returns how many words are left.  (Deferred to the buffer's merge: the k-th word
    // changes only there, so nothing is gained by knowing a key sooner.)
    auto evaluate = [&](int t, int c) -> int {
        const uint64_t thr_t = ((uint64_t)rdlane((uint32_t)(thr >> 32), t) << 32) | rdlane((uint32_t)thr, t);
        const float *const qrow = tile + t * PITCH;
        int w = 0;
        for (int i = 0; i < c; i += 8) {
            uint32_t row[2], key[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) { const int at = i + 4 * u + (lane >> 4); row[u] = (uint32_t)bufs[t][at < c ? at : 0]; }
            scan_lds_sync();
#pragma unroll
            for (int u = 0; u < 2; ++u) key[u] = scan_matrix_exact_key<NCH, METRIC>(a.X + (uint64_t)row[u] * (uint64_t)a.stride, nchunks, qrow, lane & 15);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint64_t e = ((uint64_t)key[u] << 32) | row[u];
                const bool in = (lane & 15) == 0 && i + 4 * u + (lane >> 4) < c && e < thr_t;
                const uint64_t m = ballot(in);
                if (in) bufs[t][w + popc(m & ((1ull << lane) - 1ull))] = e;
                w += popc(m);
            }
        }
        return w;
    };

    // a full buffer is evaluated and merged; after a block's merges the lanes refresh their bounds
    scan_matrix_walk<NCH, METRIC, MASKED>(a.X, a.stride, nchunks, a.eps, r0, r1, mask, tile, rterm, bufs, cnt, tq, bound,
        [&](int t, int c) { flush(t, evaluate(t, c)); },
        [&] {
            if (j < tq) {
                thr = (lists0 + j * list_step + (((par >> j) & 1u) ? a.k : 0))[a.k - 1];
                bound = scan_matrix_lane_bound<METRIC>(thr, cq);
            }
        });
    // what is left in the buffers; the result belongs in the first half
    scan_wave_sync();
    for (int t = 0; t < tq; ++t) {
        const int c = uniform(cnt[t]);
        if (c > 0) flush(t, evaluate(t, c));
        uint64_t *const A = lists0 + t * list_step;
        if ((par >> t) & 1u) for (int i = lane; i < a.k; i += 64) A[i] = A[a.k + i];
    }
}

} // namespace hnsw_dev

namespace hnsw_host {

int scan_matrix_prepass(hnsw_index *idx, const float *Q, int64_t q_stride, int64_t nq, int nch, hipStream_t st, const float **qterm_out,
                        const uint32_t **path) {
    int rc = ensure_scan_state(idx, st);
    if (rc) return rc;
    const hnsw_dev::IndexView &iv = idx->iv;
    if (nch != scan_matrix_nch(iv.d)) return fail(HNSW_ERR_HIP, "matrix scan: %d chunks per lane for d=%d", nch, iv.d);
    if ((rc = idx->scratch.scan_codes.ensure((size_t)scan_matrix_scratch(nq)))) return rc;
    float *const qterm = (float *)idx->scratch.scan_codes.p;
    uint32_t *const state = (uint32_t *)idx->scratch.scan_state.p;
    with_metric(idx->info.metric, [&](auto METRIC) {
        hipLaunchKernelGGL(hnsw_dev::hnsw_scan_matrix_queries_kernel<METRIC>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, Q, q_stride, nq, iv.d,
                           scan_matrix_eps(iv.d), qterm, state);
    });
    if ((rc = launched("matrix scan query prepass"))) return rc;
    *qterm_out = qterm;
    *path = state;
    return HNSW_OK;
}

int scan_matrix_launch(hnsw_index *idx, const float *Q, int64_t q_stride, int64_t nq, int32_t k, int nch, int64_t slabs, int64_t slab_rows,
                       uint64_t *lists, const uint32_t *const *masks, hipStream_t st, const uint32_t **path) {
    const float *qterm = nullptr;
    const uint32_t *state = nullptr;
    int rc = scan_matrix_prepass(idx, Q, q_stride, nq, nch, st, &qterm, &state);
    if (rc) return rc;
    const hnsw_dev::IndexView &iv = idx->iv;
    const float eps = scan_matrix_eps(iv.d);
    const hnsw_dev::ScanMatrixArgs a{iv.X, iv.stride, iv.n, iv.d, iv.nchunks, Q, q_stride, nq, qterm, k, (int32_t)slabs, slab_rows, lists, state, eps};
    const dim3 grid((unsigned)scan_matrix_tiles(nq), (unsigned)scan_matrix_slab_groups(slabs, nch));
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
        if constexpr (NCH <= 8) {
            if (masks) hipLaunchKernelGGL((hnsw_dev::hnsw_scan_matrix_kernel<NCH, METRIC, true>), grid, dim3(64 * scan_matrix_waves(NCH)), 0, st, a, masks);
            else hipLaunchKernelGGL((hnsw_dev::hnsw_scan_matrix_kernel<NCH, METRIC, false>), grid, dim3(64 * scan_matrix_waves(NCH)), 0, st, a, masks);
        }
    }); });
    if ((rc = launched("matrix scan kernel"))) return rc;
    *path = state;
    return HNSW_OK;
}

} // namespace hnsw_host
