// hnsw_group.hip -- grouped k-NN search: one label per node (hnsw_labels_*), hnsw_search_batch_grouped -- the k nearest DISTINCT
// labels, each represented by its nearest node -- and the exact form hnsw_brute_force_batch_grouped.  One stage body and select rule
// for the ladder's loop (Ladder::run, hnsw_filter.hip) and one selection policy of the one exact-scan body (scan_slab,
// hnsw_scan_device.hip.h), inside the shared host frame (ladder_host_call), as the header defines it:
//   ladder   e = ef, 2 ef, ... 1024: a query is served at the first e whose W holds eligible nodes of k distinct labels (eligible:
//            label >= 0 and, with a filter, allowed); its answer is the first eligible member of each of the first k labels, in
//            W's order.  Half rows and codes: the eligible members of W are re-ranked over the float32 rows first (the two halves
//            of Ladder::walk_exact, group_cand_kernel between them) and the select reads the re-ranked rows.
//   exact    a query still short at e = 1024, and every query when there are fewer than k groups (or the filter allows fewer than
//            k nodes): per label the smallest eligible node under (key, id), then the k smallest of those.
//
// Kernels.
//   labels_prepare_kernel   the uploaded labels: -1 where the live mask has no bit; counts the labelled nodes and the labels in use.
//   group_cand_kernel       W with the ineligible entries turned into padding, in place: the re-rank's candidate matrix.
//   group_select_kernel     one wave per walked query, 64 entries of W per pass: an entry is a representative iff it is eligible
//                           and its label is neither among those accepted so far (kept in LDS, at most k) nor in an earlier lane
//                           of the pass (the readlane / ballot loop of filter_label_kernel).  Stops at k.  A served query's ids,
//                           distances and labels go to its output row; others are appended to the short list (ladder_settle).
//   hnsw_group_scan_kernel  scan_slab with ScanGroupBest: best[query][label] = min(key << 32 | row) over the eligible rows, one
//                           vector atomicMin on global memory per improvement (a plain load filters the rest).
//   group_pick_kernel       the k smallest real words of a query's best row -- a radix select over the word's eight bytes finds
//                           the k-th smallest, the words up to it are ranked in LDS -- become ids, key_to_dist and labels, then
//                           the fill; a row of more than 16 384 cells in stripes, one workgroup each, whose k words are picked
//                           from by a second launch.
// The exact stage's compact rows, with their labels column, go to their queries through the filtered search's scatter kernel (scatter_rows).
// Vector stores only.  Scratch is the handle's (LadderBufs; FilterBufs' wids / wdist / rids / rdist / stage; GroupBufs): one filtered,
// range, grouped or paged call in flight.
#include "hnsw_internal.h"
#include "hnsw_scan_device.hip.h"

namespace hnsw_dev {

constexpr uint64_t GROUP_EMPTY = ~0ull;    // no node of this label yet: above every real word

__global__ void __launch_bounds__(256)
labels_prepare_kernel(int32_t *labels, int64_t n, const uint32_t *live, uint32_t *seen, unsigned long long *counts) {
    int labelled = 0, groups = 0;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        int32_t lab = labels[v];
        if (live && !((live[v >> 5] >> (v & 31)) & 1u)) {
            lab = -1;
            labels[v] = -1;
        }
        if (lab >= 0) {
            ++labelled;
            if (atomicExch(seen + lab, 1u) == 0u) ++groups;
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        labelled += __shfl_down(labelled, s, 64);
        groups += __shfl_down(groups, s, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (labelled) atomicAdd(counts, (unsigned long long)labelled);
        if (groups) atomicAdd(counts + 1, (unsigned long long)groups);
    }
}

// what makes a member of W eligible: the labels, the mask (null: none), the id range
struct GroupEligible {
    const int32_t *labels;     // [n]
    const uint32_t *mask;      // null, or ceil(n / 32) words
    int64_t n;
    int32_t id_base;
};
// the label of an eligible entry, -1 for every other
__device__ __forceinline__ int32_t group_label(const GroupEligible &g, int32_t id) {
    if (!is_node(g.n, g.id_base, id) || (g.mask && !node_allowed(mask_words(g.mask), g.n, g.id_base, id))) return -1;
    return g.labels[(int64_t)id - g.id_base];
}

// (cand may be wids: an entry is read and written by the same lane)
__global__ void __launch_bounds__(64)
group_cand_kernel(const int32_t *wids, int64_t m, int32_t e, const GroupEligible g, int32_t *cand) {
    const int64_t i = blockIdx.x;
    if (i >= m) return;
    for (int j = threadIdx.x; j < e; j += 64) {
        const int32_t id = wids[i * e + j];
        cand[i * e + j] = group_label(g, id) >= 0 ? id : g.id_base - 1;
    }
}

struct GroupSelectArgs {
    const int32_t *wids;       // [m][e] W per query (half rows, codes: re-ranked), id_base-based, other entries < id_base
    const float *wdist;        // [m][e]
    int64_t m;
    int32_t e, k;              // k <= e <= 1024
    const int32_t *map;        // [m] row i belongs to query map[i]; null: to query i
    GroupEligible g;
    int32_t *out_ids;          // [nq][k]
    float *out_dist;
    int32_t *out_labels;
    LadderOut out;
};

__global__ void __launch_bounds__(64)
group_select_kernel(const GroupSelectArgs a) {
    __shared__ int32_t acc_lab[1024], acc_id[1024];
    __shared__ float acc_dist[1024];
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= a.m) return;
    const int64_t q = a.map ? a.map[i] : i;
    const int32_t *const wi = a.wids + i * a.e;
    int at = 0;                 // representatives accepted so far (the same in all lanes)
    for (int j0 = 0; j0 < a.e && at < a.k; j0 += 64) {
        const int j = j0 + lane;
        const int32_t id = j < a.e ? wi[j] : a.g.id_base - 1;
        const int32_t lab = j < a.e ? group_label(a.g, id) : -1;
        bool fresh = lab >= 0;
        for (int t = 0; t < at && fresh; ++t) fresh = acc_lab[t] != lab;
        // the first lane of each label still fresh
        bool rep = false;
        uint64_t todo = ballot(fresh);
        while (todo) {
            const int32_t l = __builtin_amdgcn_readlane(lab, (int)__builtin_ctzll(todo));
            const uint64_t same = ballot(fresh && lab == l);
            rep = rep || lane == (int)__builtin_ctzll(same);
            todo &= ~same;
        }
        const uint64_t reps = ballot(rep);
        const int pos = at + popc(reps & ((1ull << lane) - 1ull));
        if (rep && pos < a.k) {
            acc_lab[pos] = lab;
            acc_id[pos] = id;
            acc_dist[pos] = a.wdist[i * a.e + j];
        }
        at += popc(reps);
        __syncthreads();        // (one wave: the accepted labels, seen by every lane before the next pass)
    }
    const bool served = at >= a.k;
    if (served) {
        for (int j = lane; j < a.k; j += 64) {
            a.out_ids[q * a.k + j] = acc_id[j];
            a.out_dist[q * a.k + j] = acc_dist[j];
            a.out_labels[q * a.k + j] = acc_lab[j];
        }
    }
    if (lane == 0) ladder_settle(a.out, i, q, served);
}

struct GroupScanArgs {
    const float *Q;            // the queries of this launch
    int64_t q_stride, nq;
    int32_t n_slabs;
    int64_t slab_rows;
    const int32_t *labels;     // [n]
    const uint32_t *mask;      // MASKED: ceil(n / 32) words
    unsigned long long *best;  // [nq][n_labels], GROUP_EMPTY before the launch
    int64_t n_labels;
};

// The per-label minimum of one (tile, slab) wave (scan_slab's Select).  A row is a candidate when it is one of the slab's, its mask
// bit is set (MASKED) and its label is >= 0; its word (key << 32 | row) goes to the cell of (query, label) by atomicMin when a
// plain load finds the cell above it.  Ascending words = the total order (distance, id), so the cell ends as the label's smallest
// eligible node whatever the slabs' order.
template <int NCH, bool MASKED> struct ScanGroupBest : ScanMask<MASKED> {
    const GroupScanArgs &a;
    unsigned long long *rows;  // the cells of the tile's first query
    int tq, lane;
    int32_t lab;               // the label of the row admits was last asked about
    __device__ __forceinline__ ScanGroupBest(const GroupScanArgs &a_) : ScanMask<MASKED>(a_.mask), a(a_) {}
    __device__ __forceinline__ void begin(int64_t q0, int tq_, int64_t) {
        lane = threadIdx.x & 63;
        tq = tq_;
        rows = a.best + q0 * a.n_labels;
        lab = -1;
    }
    __device__ __forceinline__ bool admits(int64_t row, bool in_slab) {
        // (the label of a row past the slab's end is never loaded: such a row may lie past the table's)
        lab = ScanMask<MASKED>::admits(row, in_slab) ? a.labels[row] : -1;
        return lab >= 0;
    }
    __device__ __forceinline__ void take(int t, uint32_t key, int64_t row, bool ok) {
        if ((lane & 15) == 0 && ok && t < tq) {     // (a query past the tile's end has no cells)
            const unsigned long long word = ((unsigned long long)key << 32) | (uint32_t)row;
            unsigned long long *const cell = rows + t * a.n_labels + lab;
            if (word < *cell) atomicMin(cell, word);
        }
    }
    __device__ __forceinline__ void batch_end() {}
    __device__ __forceinline__ void end() {}
};

template <int NCH, int METRIC, bool MASKED>
__global__ void __launch_bounds__(64 * SCAN_WAVES, scan_min_waves(NCH))
hnsw_group_scan_kernel(const IndexView iv, const GroupScanArgs a) {
    ScanGroupBest<NCH, MASKED> sel(a);
    scan_slab<NCH, METRIC>(iv, a.Q, a.q_stride, a.nq, a.n_slabs, a.slab_rows, sel);
}

// The k smallest real words of one stripe of a query's row, one workgroup per (query, stripe): words = the query's row of `len`
// words (its best cells, or the stripes' partial results), stripe s = words [s * stripe, min(len, (s + 1) * stripe)).  The k-th
// smallest word of the stripe by a radix select, most significant byte first (the words still in play are those that share the
// bytes chosen so far); the real words up to it -- at most k: real words are distinct, a node occurs once -- are collected in LDS
// with their labels (word_lab, or the word's index in the row when that is null), ranked among themselves and written out:
// FINAL (one stripe: the grid's y is 1) as ids, key_to_dist and labels with the fill behind them, else as the stripe's k words and
// labels, padded with GROUP_EMPTY, for the FINAL launch over [stripes][k] words per query.
template <int METRIC, bool FINAL>
__global__ void __launch_bounds__(256)
group_pick_kernel(const unsigned long long *words, const int32_t *word_lab, int64_t len, int64_t stripe, int32_t k, int32_t fill, int32_t id_base,
                  int32_t *out_ids, float *out_dist, int32_t *out_labels, unsigned long long *part_words, int32_t *part_lab) {
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long sel[1024];
    __shared__ int32_t sel_lab[1024];
    __shared__ unsigned long long prefix;
    __shared__ uint32_t need, cnt;
    const int64_t q = blockIdx.x, s0 = (int64_t)blockIdx.y * stripe;
    const int64_t m = len - s0 < stripe ? len - s0 : stripe;       // words of this stripe (>= 1: the grid has no empty stripe)
    const unsigned long long *const row = words + q * len + s0;
    const int tid = threadIdx.x;
    if (tid == 0) { prefix = 0ull; need = (uint32_t)k; cnt = 0u; }
    unsigned long long thr = GROUP_EMPTY;           // fewer than k words: every real word is wanted
    if (m >= k) {
        for (int p = 0; p < 8; ++p) {
            const int shift = 56 - 8 * p;
            hist[tid] = 0u;
            __syncthreads();
            const unsigned long long pre = prefix;
            for (int64_t j = tid; j < m; j += 256) {
                const unsigned long long w = row[j];
                if (p == 0 || (w >> (shift + 8)) == (pre >> (shift + 8))) atomicAdd(&hist[(w >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {     // the byte under which the need-th word of those in play lies
                uint32_t below = 0u;
                int b = 0;
                while (b < 255 && below + hist[b] < need) below += hist[b++];
                need -= below;
                prefix = pre | ((unsigned long long)b << shift);
            }
            __syncthreads();
        }
        thr = prefix;
    }
    __syncthreads();
    for (int64_t j = tid; j < m; j += 256) {
        const unsigned long long w = row[j];
        if (w != GROUP_EMPTY && w <= thr) {
            const uint32_t at = atomicAdd(&cnt, 1u);
            if (at < 1024u) { sel[at] = w; sel_lab[at] = word_lab ? word_lab[q * len + s0 + j] : (int32_t)(s0 + j); }
        }
    }
    __syncthreads();
    const int have = (int)(cnt < (uint32_t)k ? cnt : (uint32_t)k);
    const int64_t o = FINAL ? q * k : (q * gridDim.y + blockIdx.y) * k;
    for (int j = tid; j < have; j += 256) {
        const unsigned long long w = sel[j];
        int rank = 0;
        for (int i = 0; i < have; ++i) rank += sel[i] < w ? 1 : 0;
        if (FINAL) {
            out_ids[o + rank] = (int32_t)(uint32_t)w + id_base;
            out_dist[o + rank] = key_to_dist<METRIC>((uint32_t)(w >> 32));
            out_labels[o + rank] = sel_lab[j];
        } else {
            part_words[o + rank] = w;
            part_lab[o + rank] = sel_lab[j];
        }
    }
    for (int j = have + tid; j < k; j += 256) {
        if (FINAL) {
            out_ids[o + j] = -1;
            out_dist[o + j] = fill == 0 ? __uint_as_float(0x7FC00000u) : __uint_as_float(0x7F800000u);
            out_labels[o + j] = -1;
        } else {
            part_words[o + j] = GROUP_EMPTY;
            part_lab[o + j] = -1;
        }
    }
}

} // namespace hnsw_dev

using namespace hnsw_host;

namespace {

constexpr int64_t GROUP_STRIPE = 16384;     // cells of a best row one workgroup of the pick takes

hnsw_dev::GroupEligible eligible_of(const hnsw_index *idx, const hnsw_labels *l, const hnsw_filter *f) {
    return {(const int32_t *)l->lab.p, f ? (const uint32_t *)f->bits.p : nullptr, idx->iv.n, idx->iv.id_base};
}

// The exact stage for the m device-resident queries of (Q, qs): per label the smallest eligible node under (key, id) over the
// float32 rows, of those the k smallest into ids / dist / lab ([m][k], device), the fill behind them.  The queries go in pieces
// whose cells fit SCAN_SCRATCH (group_plan).
int group_exact(hnsw_index *idx, const hnsw_labels *l, const hnsw_filter *f, const float *Q, int64_t m, int64_t qs, int32_t k, int32_t fill,
                int32_t *ids, float *dist, int32_t *lab, hipStream_t st) {
    const hnsw_dev::IndexView &iv = idx->iv;
    const int nch = pick_nch(iv.nchunks), T = hnsw_dev::scan_tile(nch);
    const GroupPlan g = group_plan(iv.n, idx->scan_slabs, T, m, l->n_labels, k);
    int rc;
    // (a row of more than GROUP_STRIPE cells is picked from in stripes, one workgroup each, 1024 stripes at most: their k words and
    // labels per query)
    const int64_t want = std::min<int64_t>(1024, ((int64_t)l->n_labels + GROUP_STRIPE - 1) / GROUP_STRIPE);
    const int64_t stripe = ((int64_t)l->n_labels + want - 1) / want, stripes = ((int64_t)l->n_labels + stripe - 1) / stripe;
    GroupBufs &gb = idx->group_scratch;
    if ((rc = gb.best.ensure((size_t)g.piece * (size_t)l->n_labels * 8)) ||
        (stripes > 1 && ((rc = gb.part_words.ensure((size_t)g.piece * stripes * k * 8)) || (rc = gb.part_lab.ensure((size_t)g.piece * stripes * k * 4)))))
        return rc;
    unsigned long long *const best = (unsigned long long *)gb.best.p, *const part_words = (unsigned long long *)gb.part_words.p;
    int32_t *const part_lab = (int32_t *)gb.part_lab.p;
    for (int64_t q0 = 0; q0 < m; q0 += g.piece) {
        const int64_t nq = std::min(g.piece, m - q0);
        HIP_TRY(hipMemsetAsync(best, 0xFF, (size_t)nq * (size_t)l->n_labels * 8, st));
        if (g.slabs > 0) {
            const hnsw_dev::GroupScanArgs a{Q + q0 * qs, qs, nq, (int32_t)g.slabs, g.slab_rows, (const int32_t *)l->lab.p,
                                            f ? (const uint32_t *)f->bits.p : nullptr, best, l->n_labels};
            const dim3 grid((unsigned)((nq + T - 1) / T), (unsigned)((g.slabs + hnsw_dev::SCAN_WAVES - 1) / hnsw_dev::SCAN_WAVES));
            with_metric(idx->info.metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
                if (f) hipLaunchKernelGGL((hnsw_dev::hnsw_group_scan_kernel<NCH, METRIC, true>), grid, dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a);
                else hipLaunchKernelGGL((hnsw_dev::hnsw_group_scan_kernel<NCH, METRIC, false>), grid, dim3(64 * hnsw_dev::SCAN_WAVES), 0, st, iv, a);
            }); });
            if ((rc = launched("group scan kernel"))) return rc;
        }
        with_metric(idx->info.metric, [&](auto METRIC) {
            const unsigned long long *words = best;
            const int32_t *word_lab = nullptr;
            int64_t len = l->n_labels;
            if (stripes > 1) {      // a long row: its stripes' k smallest first, side by side, then the k smallest of those
                hipLaunchKernelGGL((hnsw_dev::group_pick_kernel<METRIC, false>), dim3((unsigned)nq, (unsigned)stripes), dim3(256), 0, st, words, word_lab, len,
                                   stripe, k, fill, iv.id_base, nullptr, nullptr, nullptr, part_words, part_lab);
                words = part_words; word_lab = part_lab; len = stripes * k;
            }
            hipLaunchKernelGGL((hnsw_dev::group_pick_kernel<METRIC, true>), dim3((unsigned)nq, 1u), dim3(256), 0, st, words, word_lab, len, len, k, fill,
                               iv.id_base, ids + q0 * k, dist + q0 * k, lab + q0 * k, nullptr, nullptr);
        });
        if ((rc = launched("group pick kernel"))) return rc;
    }
    return HNSW_OK;
}

// The ladder and the exact stage for a batch HostCall::begin has placed (b): the results are in b's rows, gb.lab and fb.stage on return.
int grouped_search(hnsw_index *idx, const hnsw_labels *l, const hnsw_filter *f, const hnsw_search_params &p, const KnnBatch &b, float *d_stage,
                   hipStream_t st) {
    FilterBufs &fb = idx->filter_scratch;
    GroupBufs &gb = idx->group_scratch;
    const int k = p.k;
    const bool rerank = walk_is_inexact(idx);
    int rc;
    if ((rc = fb.stage.ensure((size_t)b.nq * 4)) || (rc = gb.lab.ensure((size_t)b.nq * k * 4))) return rc;
    uint32_t *const d_stage_out = (uint32_t *)fb.stage.p;
    int32_t *const d_lab = (int32_t *)gb.lab.p;
    const hnsw_dev::GroupEligible ge = eligible_of(idx, l, f);
    Ladder L(idx, b.Q, b.nq, b.q_stride, p.ef, p.semantics, d_stage, st, "grouped search");
    // with fewer than k groups (or allowed nodes) no W can serve a query: nobody walks, everybody gets the exact stage
    const bool walked = l->n_groups >= k && (!f || f->n_allowed >= k);
    LadderLeft left;
    rc = L.run(walked, [&](Ladder &, int64_t m, int e) -> int {
        if ((rc = fb.wids.ensure((size_t)m * e * 4)) || (rc = fb.wdist.ensure((size_t)m * e * 4))) return rc;
        int32_t *const Wi = (int32_t *)fb.wids.p;
        float *const Wd = (float *)fb.wdist.p;
        if ((rc = L.walk_raw(Wi, Wd, p.fill))) return rc;
        if (rerank) {
            // only the ELIGIBLE members of W go over the float32 rows (the others as padding); the select reads the re-ranked rows
            hipLaunchKernelGGL(hnsw_dev::group_cand_kernel, dim3((unsigned)m), dim3(64), 0, st, L.wb.ids, m, e, ge, L.wb.ids);
            if ((rc = launched("group candidate kernel")) || (rc = L.rerank_all(Wi, Wd, p.fill))) return rc;
        }
        const hnsw_dev::GroupSelectArgs sa{Wi, Wd, m, e, k, L.map, ge, b.ids, b.dist, d_lab, L.out(b.nd, b.nh, d_stage_out)};
        hipLaunchKernelGGL(hnsw_dev::group_select_kernel, dim3((unsigned)m), dim3(64), 0, st, sa);
        return launched("group select kernel");
    }, left);
    if (rc || left == LadderLeft::none) return rc;
    // the exact stage for the L.m queries of (L.Qj, L.map): the batch the ladder left
    if ((rc = fb.rids.ensure((size_t)L.m * k * 4)) || (rc = fb.rdist.ensure((size_t)L.m * k * 4)) || (rc = gb.rlab.ensure((size_t)L.m * k * 4))) return rc;
    if ((rc = group_exact(idx, l, f, L.Qj, L.m, L.qs, k, p.fill, (int32_t *)fb.rids.p, (float *)fb.rdist.p, (int32_t *)gb.rlab.p, st))) return rc;
    return scatter_rows({(const int32_t *)fb.rids.p, (const float *)fb.rdist.p, (const int32_t *)gb.rlab.p, L.m, k, L.map, nullptr, nullptr,
                         (uint32_t)(f ? f->n_allowed : l->n_labelled), 1, nullptr, left == LadderLeft::fresh, b.ids, b.dist, d_lab, b.nd, b.nh, d_stage_out},
                        st, "group scatter kernel");
}

} // namespace

extern "C" {

int32_t hnsw_labels_create(hnsw_index *idx, const int32_t *labels, int64_t n, int32_t n_labels, hnsw_labels **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (n_labels < 1) return fail(HNSW_ERR_BAD_ARG, "n_labels must be >= 1 (n_labels=%d)", n_labels);
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (n != idx->iv.n) return fail(HNSW_ERR_BAD_ARG, "%lld labels, the index has %lld nodes", (long long)n, (long long)idx->iv.n);
    if (n > 0 && !labels) return fail(HNSW_ERR_BAD_ARG, "null labels");
    for (int64_t v = 0; v < n; ++v)
        if (labels[v] < -1 || labels[v] >= n_labels)
            return fail(HNSW_ERR_BAD_ARG, "label %d of node %lld is outside -1 .. %d", labels[v], (long long)v, n_labels - 1);
    HIP_TRY(hipSetDevice(idx->device));
    std::unique_ptr<hnsw_labels> l(new hnsw_labels());
    l->idx = idx;
    l->n = n;
    l->epoch = idx->epoch;
    l->n_labels = n_labels;
    int rc;
    if ((rc = l->lab.ensure((size_t)std::max<int64_t>(n, 1) * 4))) return rc;
    if (n > 0) {
        DevBuf seen, counts;
        if ((rc = seen.ensure((size_t)n_labels * 4)) || (rc = counts.ensure(16))) return rc;
        HIP_TRY(hipMemcpy(l->lab.p, labels, (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(seen.p, 0, (size_t)n_labels * 4));
        HIP_TRY(hipMemset(counts.p, 0, 16));
        const hnsw_filter *const live = live_filter(idx);
        const unsigned blocks = (unsigned)std::min<int64_t>(4096, (n + 255) / 256);
        hipLaunchKernelGGL(hnsw_dev::labels_prepare_kernel, dim3(blocks), dim3(256), 0, nullptr, (int32_t *)l->lab.p, n,
                           live ? (const uint32_t *)live->bits.p : nullptr, (uint32_t *)seen.p, (unsigned long long *)counts.p);
        if ((rc = launched("labels prepare kernel"))) return rc;
        unsigned long long c[2] = {0, 0};
        HIP_TRY(hipMemcpy(c, counts.p, 16, hipMemcpyDeviceToHost));
        l->n_labelled = (int64_t)c[0];
        l->n_groups = (int64_t)c[1];
    }
    *out = l.release();
    return HNSW_OK;
}

int32_t hnsw_labels_destroy(hnsw_labels *l) {
    if (!l) return HNSW_OK;
    delete l;
    return HNSW_OK;
}

int32_t hnsw_labels_info(const hnsw_labels *l, int32_t *n_labels, int64_t *n_labelled, int64_t *n_groups) {
    if (!l) return fail(HNSW_ERR_BAD_ARG, "null labels");
    if (n_labels) *n_labels = l->n_labels;
    if (n_labelled) *n_labelled = l->n_labelled;
    if (n_groups) *n_groups = l->n_groups;
    return HNSW_OK;
}

int32_t hnsw_labels_get(const hnsw_labels *l, int32_t *out) {
    if (!l || !out) return fail(HNSW_ERR_BAD_ARG, "null labels or null out");
    if (l->n == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(l->idx->device));
    HIP_TRY(hipMemcpy(out, l->lab.p, (size_t)l->n * 4, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

int32_t hnsw_search_batch_grouped(hnsw_index *idx, const hnsw_labels *labels, const hnsw_filter *f, const float *queries, int64_t nq,
                                  int64_t q_stride, const hnsw_search_params *params, int32_t *out_ids, float *out_dist, int32_t *out_labels,
                                  uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage) {
    int rc = check_batch(idx, params, nq, q_stride, queries && out_ids && out_dist && out_labels);
    if (rc) return rc;
    if (params->semantics == HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "the k farthest of W (HNSW_SEM_FUNCTOR_NEAREST_K) have no grouped meaning");
    if ((rc = check_labels(idx, labels)) || (f && (rc = check_filter(idx, f)))) return rc;
    if (nq == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(idx->device));
    const HostColumn lab{out_labels, &idx->group_scratch.lab, (size_t)nq * params->k * 4, "labels"};
    return ladder_host_call(idx, queries, nq, q_stride, params->k, out_ids, out_dist, out_ndist, out_nhops, out_stage, true, nullptr, nullptr, nullptr, &lab,
                            "grouped search", [&](const KnnBatch &b, float *d_stage, hipStream_t st) -> int {
        return grouped_search(idx, labels, f, *params, b, d_stage, st);
    });
}

int32_t hnsw_brute_force_batch_grouped(hnsw_index *idx, const hnsw_labels *labels, const hnsw_filter *f, const float *queries, int64_t nq,
                                       int64_t q_stride, int32_t k, int32_t fill, int32_t *out_ids, float *out_dist, int32_t *out_labels) {
    int rc = check_scan(idx, nq, q_stride, k, fill, queries && out_ids && out_dist && out_labels);
    if (rc) return rc;
    if ((rc = check_labels(idx, labels)) || (f && (rc = check_filter(idx, f)))) return rc;
    if (nq == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(idx->device));
    if ((rc = idx->group_scratch.lab.ensure((size_t)nq * k * 4))) return rc;
    const HostColumn lab{out_labels, &idx->group_scratch.lab, (size_t)nq * k * 4, "labels"};
    return ladder_host_call(idx, queries, nq, q_stride, k, out_ids, out_dist, nullptr, nullptr, nullptr, false, nullptr, nullptr, nullptr, &lab, "grouped scan",
                            [&](const KnnBatch &b, float *, hipStream_t st) -> int {
        return group_exact(idx, labels, f, b.Q, nq, b.q_stride, k, fill, b.ids, b.dist, (int32_t *)idx->group_scratch.lab.p, st);
    });
}

} // extern "C"
