// hnsw_range_matrix.hip -- the exact range scan of float rows through fp32 matrix instructions (option "scan_matrix"): both passes
// of hnsw_range.hip's scan, plain and masked, screened the way hnsw_scan_matrix.hip screens the k-scan.
//
// The matrix unit never makes a key.  Per (row, query) pair it yields the proven bound of hnsw_scan_matrix_plan.h (DESIGN.md section
// 3) and the pair is dropped only when that bound shows its exact key above khi, the largest key in range (range_key_bounds).  A pair
// that is not dropped gets the float scan's own key (scan_matrix_exact_key: scan_chain, reduce16, dist_to_key) and is a hit iff
// klo <= key <= khi: RangeHits' test on RangeHits' key.  So every (query, slab) cell holds the float range scan's count and words;
// the exclusive sums, range_count_kernel, the segmented sort and range_unpack_kernel around it are untouched.
//
// What makes the range scan the screen's best case: the threshold is one fixed key interval from the slab's first row on.  There are
// no lists to fill with k exact evaluations first, no threshold that tightens only at a merge, no merge: the lane's bound is computed
// once per wave, and on a selective radius almost every pair costs one multiply-add and one compare of its accumulator.
//
//   hnsw_range_scan_matrix_kernel<NCH, METRIC, PASS, MASKED>: grid (tiles of 32 queries) x (groups of slabs), one wave per (tile,
//     slab), range_matrix_waves(NCH) waves per workgroup; the slabs are the float range scan's (ExactPlan), so a cell is a cell.
//     Tile, A operand, pipeline, row norms, screen: the k-scan's, scan_matrix_load_tile and scan_matrix_walk
//       (hnsw_scan_matrix_device.hip.h has the lane maps) -- the tile in LDS as float32 with pitch 64 NCH + 4; 32-row blocks aligned
//       to a mask word straight from global memory; +inf for a masked or out-of-slab row; a mask word without a set bit stepped over
//       unloaded.
//     Survivors: bare 32-bit row numbers in the query's buffer of 64 (8 KB per wave).  A buffer that may not take another block's
//       32 (and, at the slab's end, every buffer) is evaluated: one 16-lane group per pair, eight pairs a round.
//     Hits: lane t carries query t's hit count for the cell (every update is wave-uniform: a ballot's population count).  PASS 0
//       writes it to counts[(q0 + t) n_slabs + slab].  PASS 1 writes a hit's word (key << 32 | row) at the cell's offset plus the
//       count so far plus the hit's place in its round's ballot, guarded by the cell's PASS-0 count as RangeHits guards it.  The
//       order inside a cell differs from the float kernel's id order; the words are distinct and the segmented sort orders every
//       segment afterwards.  Vector stores only.
// The prepass is the k-scan's (hnsw_scan_matrix_queries_kernel: the queries' terms, the path word): the kernel returns at once unless
// the word is 3, and the float range kernels launched behind it run only when it is 1.
#include "hnsw_internal.h"
#include "hnsw_scan_matrix_device.hip.h"

namespace hnsw_dev {

using namespace hnsw_host;      // the plan header's constants and the rule

struct RangeMatrixArgs {
    const float *X;        // [n][stride] zero-padded rows
    int64_t stride, n;
    int32_t d, nchunks;
    const float *qterm;    // [nq] as the prepass wrote them
    const uint32_t *path;  // the handle's path word
    float eps;             // scan_matrix_eps(d)
    RangeScanArgs r;       // the pass's queries, cut, radius and cells: what the float range kernels get
};

template <int NCH, int METRIC, int PASS, bool MASKED>
__global__ void __launch_bounds__(64 * range_matrix_waves(NCH))
hnsw_range_scan_matrix_kernel(const RangeMatrixArgs a, const uint32_t *mask_) {
    constexpr int T = SCAN_MATRIX_TILE, W = range_matrix_waves(NCH), BUF = RANGE_MATRIX_BUF;
    constexpr int PITCH = scan_matrix_pitch(NCH);
    static_assert(T == 32 && RANGE_MATRIX_WAVE_BYTES == T * BUF * 4 + T * 4 + 32 * 4, "the plan header's LDS per wave");
    static_assert(range_matrix_lds_bytes(NCH) == T * PITCH * 4 + W * RANGE_MATRIX_WAVE_BYTES && range_matrix_lds_bytes(NCH) <= SCAN_MATRIX_LDS_MAX,
                  "the plan header's LDS budget");
    static_assert(W == (scan_matrix_piece(NCH) == 64 ? 8 : 4), "two waves per SIMD only with the short stage");
    __shared__ __attribute__((aligned(16))) float tile[T * PITCH];
    __shared__ uint32_t bufs_all[W][T][BUF];
    __shared__ int cnt_all[W][T];
    __shared__ __attribute__((aligned(16))) float rterm_all[W][32];
    if (*a.path != (uint32_t)SCAN_PATH_MATRIX) return;          // (the whole workgroup: before the barrier)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31;                    // the lane's query column
    const int64_t q0 = (int64_t)blockIdx.x * T;
    const int tq = (int)(a.r.nq - q0 < T ? a.r.nq - q0 : T);
    scan_matrix_load_tile<NCH, W>(tile, a.r.Q, a.r.q_stride, q0, tq, a.d);
    __syncthreads();
    const int64_t slab = (int64_t)blockIdx.y * W + uniform(wave);
    if (slab >= a.r.n_slabs) return;            // (after the only workgroup barrier)
    const int64_t r0 = slab * a.r.slab_rows, r1 = r0 + a.r.slab_rows < a.n ? r0 + a.r.slab_rows : a.n;
    const MaskWords mask = mask_words(MASKED ? mask_ : nullptr);
    uint32_t (*const bufs)[BUF] = bufs_all[wave];
    int *const cnt = cnt_all[wave];
    float *const rterm = rterm_all[wave];
    const int nchunks = a.nchunks;

    // the key interval of the radius, once per wave; the lane's bound from its upper end, fixed for the whole slab
    uint32_t klo, khi;
    range_key_bounds<METRIC>(a.r.radius, klo, khi);
    klo = (uint32_t)uniform((int)klo); khi = (uint32_t)uniform((int)khi);
    uint64_t *const cell_count = a.r.counts + (q0 + lane) * a.r.n_slabs + slab;    // lane t < tq: query t's cell
    if (khi < klo) {                            // no key is in range
        if (PASS == 0 && lane < tq) *cell_count = 0ull;
        return;
    }
    const float bound = j < tq ? scan_matrix_bound(METRIC, range_matrix_threshold(METRIC, khi), a.qterm[q0 + j]) : -__builtin_inff();
    // lane t < tq: query t's hits in this cell so far; PASS 1: where its words go and how many PASS 0 counted
    int hits = 0, lim = 0;
    int64_t dst = 0;
    if (PASS == 1 && lane < tq) {
        const int64_t at = (q0 + lane) * a.r.n_slabs;
        dst = a.r.xoff[q0 + lane] + (int64_t)(a.r.offs[at + slab] - a.r.offs[at]);
        lim = (int)(a.r.offs[at + slab + 1] - a.r.offs[at + slab]);
    }
    if (lane < T) cnt[lane] = 0;
    scan_wave_sync();

    // The c (>= 1) row numbers of query t's buffer get their exact keys, eight pairs a round (one 16-lane group per pair, two pairs
    // per group so that two rows' loads are in flight); a key inside the interval is a hit: counted, and in PASS 1 written.
    auto evaluate = [&](int t, int c) {
        const float *const qrow = tile + t * PITCH;
        int at_hit = __builtin_amdgcn_readlane(hits, t);
        const int lim_t = __builtin_amdgcn_readlane(lim, t);
        uint64_t *const out = a.r.words + (int64_t)(((uint64_t)rdlane((uint32_t)((uint64_t)dst >> 32), t) << 32) | rdlane((uint32_t)dst, t));
        for (int i = 0; i < c; i += 8) {
            uint32_t row[2], key[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) { const int at = i + 4 * u + (lane >> 4); row[u] = bufs[t][at < c ? at : 0]; }
            scan_lds_sync();
#pragma unroll
            for (int u = 0; u < 2; ++u) key[u] = scan_matrix_exact_key<NCH, METRIC>(a.X + (uint64_t)row[u] * (uint64_t)a.stride, nchunks, qrow, lane & 15);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bool hit = (lane & 15) == 0 && i + 4 * u + (lane >> 4) < c && key[u] >= klo && key[u] <= khi;
                const uint64_t m = ballot(hit);
                if (PASS == 1) {
                    const int pos = at_hit + popc(m & ((1ull << lane) - 1ull));
                    if (hit && pos < lim_t) out[pos] = ((uint64_t)key[u] << 32) | row[u];
                }
                at_hit += popc(m);
            }
        }
        if (lane == t) hits = at_hit;
        if (lane == 0) cnt[t] = 0;
    };

    // a full buffer is evaluated; the bound never moves
    scan_matrix_walk<NCH, METRIC, MASKED>(a.X, a.stride, nchunks, a.eps, r0, r1, mask, tile, rterm, bufs, cnt, tq, bound, evaluate, [] {});
    // what is left in the buffers, then the cell's count
    scan_wave_sync();
    for (int t = 0; t < tq; ++t) {
        const int c = uniform(cnt[t]);
        if (c > 0) evaluate(t, c);
    }
    if (PASS == 0 && lane < tq) *cell_count = (uint64_t)hits;
}

} // namespace hnsw_dev

namespace hnsw_host {

int range_matrix_launch(hnsw_index *idx, int pass, int nch, const hnsw_dev::RangeScanArgs &r, const uint32_t *mask, hipStream_t st, const uint32_t **path) {
    const hnsw_dev::IndexView &iv = idx->iv;
    const float *qterm = (const float *)idx->scratch.scan_codes.p;
    const uint32_t *state = (const uint32_t *)idx->scratch.scan_state.p;
    int rc;
    // PASS 1 follows the PASS 0 of the same queries on the same stream: their terms and the path word are still in place
    if (pass == 0 && (rc = scan_matrix_prepass(idx, r.Q, r.q_stride, r.nq, nch, st, &qterm, &state))) return rc;
    if (!qterm || !state || nch != scan_matrix_nch(iv.d)) return fail(HNSW_ERR_HIP, "matrix range scan: pass %d without its prepass (d=%d)", pass, iv.d);
    const hnsw_dev::RangeMatrixArgs a{iv.X, iv.stride, iv.n, iv.d, iv.nchunks, qterm, state, scan_matrix_eps(iv.d), r};
    const dim3 grid((unsigned)scan_matrix_tiles(r.nq), (unsigned)range_matrix_slab_groups(r.n_slabs, nch));
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) { with_range_pass(pass, mask != nullptr, [&](auto PASS, auto MASKED) {
        if constexpr (NCH <= 8)
            hipLaunchKernelGGL((hnsw_dev::hnsw_range_scan_matrix_kernel<NCH, METRIC, PASS, MASKED>), grid, dim3(64 * range_matrix_waves(NCH)), 0, st, a, mask);
    }); }); });
    if ((rc = launched("matrix range scan kernel"))) return rc;
    *path = state;
    return HNSW_OK;
}

} // namespace hnsw_host
