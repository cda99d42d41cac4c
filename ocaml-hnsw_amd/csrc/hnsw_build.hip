// hnsw_build.hip -- host driver of the batched GPU graph builder + graph export.
//
// Restates Ohnsw.build_batch_bigarray / Ohnsw.insert (lib/ohnsw.ml:766-857) batch-wise on the
// device (kernels: hnsw_build_device.hip.h).  The level law is the reference's
// (round_nearest(-ln(U) * 1/ln M), lib/ohnsw.ml:781,844); the RNG is this library's own seeded
// splitmix64 (OCaml's Random cannot and need not be reproduced: search parity is defined GIVEN a
// graph).  A node that raises max_layer ends its batch and becomes the entry point (:832-836).
#include "hnsw_build_device.hip.h"
#include "hnsw_internal.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

using namespace hnsw_host;
using hnsw_dev::BatchView;
using hnsw_dev::BuildView;
using hnsw_dev::IndexView;
using hnsw_dev::MergeArgs;
using hnsw_dev::SelectArgs;
using hnsw_dev::SelectOpArgs;

namespace {

inline uint64_t splitmix64(uint64_t *s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
inline double rng_unit(uint64_t *s) { return ((double)(splitmix64(s) >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

// The builder's launches.  Its construction search keeps W in 1, 2, 4 or 8 registers (efc <= 512: check_build_params).
hipError_t launch_search(int metric, int nch, int nslot, const BuildView &bv, const BatchView &bt, hipStream_t st) {
    const size_t lds = hnsw_dev::wave_lds_words(bv.vt_bits) * sizeof(uint32_t);
    with_metric(metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) { with_nslot<1, 2, 4, 8>(nslot, [&](auto NSLOT) {
        hipLaunchKernelGGL((hnsw_dev::build_search_kernel<NCH, rows_in_flight(NCH), NSLOT, METRIC>), dim3((unsigned)bt.B), dim3(64), lds, st, bv, bt);
    }); }); });
    return hipGetLastError();
}
hipError_t launch_select(int metric, int nch, const BuildView &bv, const BatchView &bt, const SelectArgs &sa, hipStream_t st) {
    const size_t lds = (2 * (size_t)bv.cand_stride + 64) * sizeof(uint32_t);
    with_metric(metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
        hipLaunchKernelGGL((hnsw_dev::build_select_kernel<NCH, METRIC>), dim3((unsigned)(sa.rec_end - sa.rec_begin)), dim3(64), lds, st, bv, bt, sa);
    }); });
    return hipGetLastError();
}
hipError_t launch_merge(int metric, int nch, const BuildView &bv, const MergeArgs &ma, hipStream_t st) {
    with_metric(metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
        hipLaunchKernelGGL((hnsw_dev::build_merge_kernel<NCH, rows_in_flight(NCH), METRIC>), dim3((unsigned)ma.n_edges), dim3(64), 0, st, bv, ma);
    }); });
    return hipGetLastError();
}
hipError_t launch_link(int metric, int nch, const BuildView &bv, const hnsw_dev::LinkArgs &la, hipStream_t st) {
    with_metric(metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
        hipLaunchKernelGGL((hnsw_dev::build_link_sequential_kernel<NCH, rows_in_flight(NCH), METRIC>), dim3(1), dim3(64), 0, st, bv, la);
    }); });
    return hipGetLastError();
}

} // namespace

// ---- levels (lib/ohnsw.ml:781): node i's draw is the i-th of one splitmix64 stream, i.e. the mix of the state
// seed + i * 0x9E3779B97F4A7C15; the first node draws nothing (:774-778).  A function of (seed, i) alone, so an index grown
// by hnsw_index_insert gets the levels hnsw_build of all its vectors would have given it, however the inserts were split.
static uint8_t node_level(uint64_t seed, int64_t i, double level_mult) {
    if (i == 0) return 0;
    uint64_t s = seed + (uint64_t)(i - 1) * 0x9E3779B97F4A7C15ULL;    // splitmix64 advances the state before mixing
    const double u = rng_unit(&s);
    const int l = (int)std::floor(-std::log(u) * level_mult + 0.5);
    return (uint8_t)std::min(l, 15);
}

// log2 entries of the construction search's visited cache for a graph of n nodes
static int build_vt_bits(int efc, int64_t n) {
    int b = efc <= 256 ? 11 : 12;
    while (b < 16 && ((int64_t)0xFFFF << (b - 1)) < n) ++b;   // tags identify ids exactly, 0xFFFF = empty way
    return b;
}

// The batch loop of the builder: inserts the nodes at positions [pos0, n) into the tables of bv (bv.iv.n == n; rows of the nodes
// before pos0 hold their graph, compacted or with holes; rows of the others are empty), batch by batch in node order (fold_cols,
// lib/ohnsw.ml:848), and compacts every row at the end.  lvl[j - pos0] is node j's level; *cur_max / *entry are the graph's
// state before pos0 and after n.  One attempt with a removal buffer of rem_scale * (2 * max_batch * 2M) entries; *rem_overflow
// tells the caller that some step produced more removals than that (the tables are then to be discarded, never patched).
// hnsw_build runs it from pos0 = 1 on fresh tables, hnsw_index_insert from the old node count on grown copies.
static int32_t run_batches(BuildView &bv, const uint8_t *lvl, int64_t pos0, int64_t n, int lcap, const hnsw_build_params *p,
                           int64_t rem_scale, bool *rem_overflow, int *cur_max_io, int *entry_io) {
    *rem_overflow = false;
    const int M = p->num_connections, efc = p->num_nodes_search_construction;
    const int nch = pick_nch(bv.iv.nchunks);
    const int S0 = 2 * M, SU = M;
    const int bdiv = p->batch_div > 0 ? p->batch_div : 16;
    const int bmax = p->max_batch > 0 ? p->max_batch : 8192;
    const int cand_stride = (efc + 63) / 64 * 64;
    const int nslot = pick_nslot(efc);
    const int64_t maxrec = (int64_t)bmax * lcap;
    const int64_t max_edges = (int64_t)bmax * S0;
    const int64_t rem_cap = max_edges * 2 * rem_scale;
    const int64_t rowsU = bv.iv.rowsU;
    uint32_t rem_over = 0;
    Stream st;
    Table dNodes, dRecOf, dRecNode, dCandId, dCandKey, dCandCnt, dEdges, dEdgesSorted, dRem, dRemCnt, dTemp;
    size_t temp_bytes = 0;
    Pinned<int32_t> hp_nodes[2], hp_rec_of[2], hp_rec_node[2];
    Event ev[2];
    int64_t batch_no = 0;
    std::vector<int32_t> rec_begin((size_t)lcap + 1, 0);
    int cur_max = *cur_max_io, entry = *entry_io;
    bv.efc = efc; bv.cand_stride = cand_stride;
    bv.vt_bits = build_vt_bits(efc, n);

    HIP_TRY(hipStreamCreate(&st.h));
    HIP_TRY(dNodes.alloc((size_t)bmax * 4));
    HIP_TRY(dRecOf.alloc((size_t)bmax * lcap * 4));
    HIP_TRY(dRecNode.alloc((size_t)maxrec * 4));
    HIP_TRY(dCandId.alloc((size_t)maxrec * cand_stride * 4));
    HIP_TRY(dCandKey.alloc((size_t)maxrec * cand_stride * 4));
    HIP_TRY(dCandCnt.alloc((size_t)maxrec * 4));
    HIP_TRY(dEdges.alloc((size_t)max_edges * 8));
    HIP_TRY(dEdgesSorted.alloc((size_t)max_edges * 8));
    HIP_TRY(dRem.alloc((size_t)rem_cap * 8));
    HIP_TRY(dRemCnt.alloc(16));
    HIP_TRY(hipMemset(dRemCnt.p, 0, 16));
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, temp_bytes, (uint64_t *)dEdges.p, (uint64_t *)dEdgesSorted.p, (int)max_edges, 0, 64, st));
    HIP_TRY(dTemp.alloc(temp_bytes));

    for (int k = 0; k < 2; ++k) {   // pinned, double buffered: batch b+2 waits for batch b's uploads
        HIP_TRY(hp_nodes[k].alloc((size_t)bmax * 4, hipHostMallocDefault));
        HIP_TRY(hp_rec_of[k].alloc((size_t)bmax * lcap * 4, hipHostMallocDefault));
        HIP_TRY(hp_rec_node[k].alloc((size_t)maxrec * 4, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&ev[k].h, hipEventDisableTiming));
    }

    // ---- batches, in node order (fold_cols, lib/ohnsw.ml:848) ----
    for (int64_t pos = pos0; pos < n;) {
        int64_t bsz = std::max<int64_t>(1, std::min<int64_t>(bmax, pos / bdiv));
        int64_t end = std::min(n, pos + bsz);
        for (int64_t j = pos; j < end; ++j)
            if ((int)lvl[(size_t)(j - pos0)] > cur_max) { end = j + 1; break; }       // :832-836
        const int B = (int)(end - pos);
        const int kb = (int)(batch_no & 1);
        if (batch_no >= 2) HIP_TRY(hipEventSynchronize(ev[kb]));
        int32_t *h_nodes = hp_nodes[kb], *h_rec_of = hp_rec_of[kb], *h_rec_node = hp_rec_node[kb];
        // records: (layer, batch slot) for layer <= min(level, cur_max), ordered by layer then slot
        int nrec = 0;
        std::fill(h_rec_of, h_rec_of + (size_t)B * lcap, -1);
        for (int l = 0; l <= cur_max; ++l) {
            rec_begin[(size_t)l] = nrec;
            for (int i = 0; i < B; ++i) {
                h_nodes[i] = (int32_t)(pos + i);
                if ((int)lvl[(size_t)(pos + i - pos0)] >= l) { h_rec_of[(size_t)i * lcap + l] = nrec; h_rec_node[nrec] = (int32_t)(pos + i); nrec++; }
            }
        }
        rec_begin[(size_t)cur_max + 1] = nrec;
        HIP_TRY(hipMemcpyAsync(dNodes.p, h_nodes, (size_t)B * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dRecOf.p, h_rec_of, (size_t)B * lcap * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dRecNode.p, h_rec_node, (size_t)nrec * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(ev[kb], st));

        BatchView bt{};
        bt.nodes = (const int32_t *)dNodes.p; bt.rec_of = (const int32_t *)dRecOf.p; bt.B = B; bt.lcap = lcap;
        bt.cur_max_layer = cur_max; bt.entry = entry;
        bt.cand_id = (int32_t *)dCandId.p; bt.cand_key = (uint32_t *)dCandKey.p; bt.cand_cnt = (int32_t *)dCandCnt.p;
        bv.iv.max_layer = cur_max; bv.iv.entry_point = entry;
        HIP_TRY(launch_search(p->metric, nch, nslot, bv, bt, st));

        for (int l = cur_max; l >= 0; --l) {
            const int rb = rec_begin[(size_t)l], re = rec_begin[(size_t)l + 1];
            if (re == rb) continue;
            const int R = l == 0 ? S0 : SU;                                    // :818
            SelectArgs sa{};
            sa.rec_node = (const int32_t *)dRecNode.p; sa.rec_begin = rb; sa.rec_end = re; sa.layer = l; sa.R = R;
            sa.edges = (uint64_t *)dEdges.p;
            HIP_TRY(launch_select(p->metric, nch, bv, bt, sa, st));
            if (B == 1) {
                // a batch of one node: the link step of Ohnsw.insert exactly, neighbour by neighbour (:820-829)
                hnsw_dev::LinkArgs la{};
                la.q = (int32_t)pos; la.layer = l; la.R = R;
                HIP_TRY(launch_link(p->metric, nch, bv, la, st));
                continue;
            }
            const int n_edges = (re - rb) * R;
            size_t tb = temp_bytes;
            HIP_TRY(hipcub::DeviceRadixSort::SortKeys(dTemp.p, tb, (uint64_t *)dEdges.p, (uint64_t *)dEdgesSorted.p, n_edges, 0, 64, st));
            HIP_TRY(hipMemsetAsync(dRemCnt.p, 0, 4, st));
            MergeArgs ma{};
            ma.edges = (const uint64_t *)dEdgesSorted.p; ma.n_edges = n_edges; ma.layer = l; ma.R = R;
            ma.removals = (uint64_t *)dRem.p; ma.rem_cnt = (uint32_t *)dRemCnt.p; ma.rem_cap = (uint32_t)rem_cap;
            HIP_TRY(launch_merge(p->metric, nch, bv, ma, st));
            // one thread per possible removal: the count is only known on the device (clamped to the buffer there)
            const unsigned rem_threads = (unsigned)std::min<int64_t>(std::max<int64_t>((int64_t)n_edges * 2, 4096), rem_cap);
            hipLaunchKernelGGL(hnsw_dev::build_unlink_kernel, dim3((rem_threads + 255) / 256), dim3(256), 0, st, bv,
                               (const uint64_t *)dRem.p, (const uint32_t *)dRemCnt.p, (uint32_t)rem_cap, l);
            HIP_TRY(hipGetLastError());
        }
        if ((int)lvl[(size_t)(end - 1 - pos0)] > cur_max) { cur_max = lvl[(size_t)(end - 1 - pos0)]; entry = (int)(end - 1); } // :832-836
        pos = end;
        batch_no++;
    }
    hipLaunchKernelGGL(hnsw_dev::build_compact_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, bv.nbr0_w, n, S0);
    if (rowsU > 0)
        hipLaunchKernelGGL(hnsw_dev::build_compact_kernel, dim3((unsigned)((rowsU + 3) / 4)), dim3(256), 0, st, bv.nbrU_w, rowsU, SU);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&rem_over, (const uint32_t *)dRemCnt.p + 1, 4, hipMemcpyDeviceToHost));
    if (rem_over) { *rem_overflow = true; return fail(HNSW_ERR_DEGREE_OVERFLOW, "a build step produced %u symmetric removals, more than the %lld the buffer holds", rem_over, (long long)rem_cap); }
    *cur_max_io = cur_max; *entry_io = entry;
    return HNSW_OK;
}

// the builder's parameter checks, shared by hnsw_build and hnsw_index_insert
static int32_t check_build_params(const hnsw_build_params *p) {
    if (p->metric != HNSW_METRIC_L2 && p->metric != HNSW_METRIC_IP && p->metric != HNSW_METRIC_COSINE) return fail(HNSW_ERR_BAD_ARG, "bad metric");
    const int M = p->num_connections, efc = p->num_nodes_search_construction;
    if (M < 2 || 2 * M > 64) return fail(HNSW_ERR_UNSUPPORTED, "num_connections=%d must be in 2..32", M);
    if (efc < 1 || efc > 512) return fail(HNSW_ERR_UNSUPPORTED, "num_nodes_search_construction=%d must be in 1..512", efc);
    return HNSW_OK;
}

// One attempt of hnsw_build (see run_batches for rem_scale / rem_overflow).
static int32_t build_attempt(const float *vectors, int64_t n, int32_t d, int64_t row_stride,
                             const hnsw_build_params *p, int32_t device, hnsw_index **out,
                             int64_t rem_scale, bool *rem_overflow) {
    *rem_overflow = false;
    if (!out || !p) return fail(HNSW_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (n < 1 || n > 0x7FFFFFF0LL) return fail(HNSW_ERR_BAD_ARG, "n=%lld out of range", (long long)n);
    if (!vectors || d < 1 || row_stride < d) return fail(HNSW_ERR_BAD_ARG, "bad vectors/d/row_stride");
    { const int32_t rcp = check_build_params(p); if (rcp) return rcp; }
    const int M = p->num_connections;
    const int nchunks = (d + 3) / 4;
    const int nch = pick_nch(nchunks);
    if (!nch) return fail(HNSW_ERR_UNSUPPORTED, "d=%d > 1024 not supported", d);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(HNSW_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (device < 0 || device >= ndev) return fail(HNSW_ERR_BAD_ARG, "device %d out of range", device);
    HIP_TRY(hipSetDevice(device));

    const double level_mult = 1.0 / std::log((double)M);                                  // :844
    std::vector<uint8_t> lvl((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) lvl[(size_t)i] = node_level(p->seed, i, level_mult);
    int lcap = 1;
    for (int64_t i = 0; i < n; ++i) lcap = std::max(lcap, (int)lvl[(size_t)i] + 1);
    std::vector<int2> ref;
    const int64_t rowsU = upper_layout(lvl.data(), n, 0, ref);

    IndexPtr idx(new hnsw_index());
    idx->device = device;
    int rc;
    const int S0 = 2 * M, SU = M;
    const int64_t stride = padded_stride(d);
    BuildView bv{};
    int cur_max = 0, entry = 0;                 // node 0 is the first entry point
    IndexView &iv = idx->iv;

    if ((rc = alloc_graph_tables(idx->tables, n, stride, S0, SU, rowsU)) ||
        (rc = upload_rows(vectors, n, d, row_stride, (float *)idx->tables.X.p)) || (rc = upload_upper_layout(idx->tables, 0, ref))) return rc;
    // COSINE: the graph is built over N(X), which is what the table holds from here on
    if (p->metric == HNSW_METRIC_COSINE && (rc = cosine_store_rows((float *)idx->tables.X.p, n, d, "nothing built"))) return rc;
    iv.stride = stride; iv.n = n; iv.d = d; iv.nchunks = nchunks; iv.S0 = S0; iv.SU = SU; iv.rowsU = rowsU;
    iv.max_layer = 0; iv.entry_point = 0; iv.id_base = p->id_base;
    bind_view(idx.get());
    bv.iv = iv; bv.nbr0_w = (int32_t *)idx->tables.nbr0.p; bv.nbrU_w = (int32_t *)idx->tables.nbrU.p;
    if ((rc = run_batches(bv, lvl.data() + 1, 1, n, lcap, p, rem_scale, rem_overflow, &cur_max, &entry))) return rc;
    iv.max_layer = cur_max; iv.entry_point = entry;
    hnsw_index_info &inf = idx->info;
    inf.d = d; inf.metric = p->metric; inf.id_base = p->id_base; inf.max_degree = SU; inf.device = device;
    return finish_index(std::move(idx), p->expected_ef, p->expected_semantics, out);
}

namespace {
// one thread per slot of the wider table: row r of `src` (width ws, compacted) becomes row r of `dst` (width wd >= ws) in the
// same order, the new slots empty
__global__ void __launch_bounds__(256)
widen_rows_kernel(const int32_t *src, int64_t rows, int32_t ws, int32_t *dst, int32_t wd) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * wd) return;
    const int64_t r = e / wd;
    const int j = (int)(e - r * wd);
    dst[e] = j < ws ? src[r * ws + j] : -1;
}

// flag[0] = 1 if an upper-layer row lists a node that is not on that layer, or the entry point is not on the top layer.  The
// builder WRITES into the rows of the nodes it finds on a layer, so a graph handed to hnsw_index_create that breaks this would
// send it outside the tables; hnsw_index_insert refuses such a graph instead.
__global__ void __launch_bounds__(256)
upper_rows_check_kernel(const int2 *upper_ref, const int32_t *nbrU, int32_t SU, int64_t n, int32_t entry, int32_t max_layer, int32_t *flag) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int2 ref = upper_ref[v];
    if (v == entry && ref.y < max_layer) flag[0] = 1;
    for (int l = 1; l <= ref.y; ++l) {
        const int32_t *row = nbrU + ((int64_t)ref.x + (l - 1)) * SU;
        for (int j = 0; j < SU; ++j) {
            const int32_t u = row[j];
            if (u >= 0 && (u >= n || upper_ref[u].y < l)) flag[0] = 1;
        }
    }
}

hipError_t widen_rows(const void *src, int64_t rows, int ws, void *dst, int wd) {
    if (rows <= 0) return hipSuccess;
    if (ws == wd) return hipMemcpy(dst, src, (size_t)rows * ws * 4, hipMemcpyDeviceToDevice);
    const int64_t total = rows * wd;
    hipLaunchKernelGGL(widen_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr,
                       (const int32_t *)src, rows, ws, (int32_t *)dst, wd);
    return hipGetLastError();
}
} // namespace

namespace hnsw_host {

// insert's and remove's check of a graph they are about to read layer by layer (upper_rows_check_kernel)
int check_upper_rows(const hnsw_index *idx, const char *verb) {
    DevFlag flag;
    int32_t bad = 0;
    HIP_TRY(flag.alloc());
    hipError_t e = flag.set(0);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(upper_rows_check_kernel, dim3((unsigned)((idx->iv.n + 255) / 256)), dim3(256), 0, nullptr, idx->iv.upper_ref,
                           idx->iv.nbrU, idx->iv.SU, idx->iv.n, idx->iv.entry_point, idx->iv.max_layer, (int32_t *)flag.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = flag.get(&bad);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "upper-row check failed: %s", hipGetErrorString(e));
    if (bad) return fail(HNSW_ERR_BAD_ARG, "the graph lists a node on a layer it is not on (or its entry point is not on the top layer): %s", verb);
    return HNSW_OK;
}

// The tail hnsw_index_insert and hnsw_index_remove share: nx holds the new graph (vectors, rows, layout, view) built beside idx's.
// What the handle derives from the graph is made again for it: the byte rows if ALL vectors are byte-valued, the split
// rows (per-slot tails follow the changed adjacency) unless option split_rows -1 freed them for good, the half rows while
// option half_rows is 1 (new vectors that do not fit fp16 refuse the whole insert; at 0 the copy is not carried over), the
// sq8 rows while option sq8_rows is 1 (the WHOLE table is quantised again: new vectors may widen the range; a range that
// overflows refuses the whole insert), the per-dimension sq8 rows while option sq8_dim_rows is 1 (likewise), the locality codes (carry_codes: carried over as extend_locality_codes does; else dropped
// and built on demand).  Then the tables are swapped in and the graph epoch moves on.  On any error idx is as it was.
int adopt_graph(hnsw_index *idx, IndexPtr &nx, bool carry_codes, int32_t expected_ef, int32_t expected_semantics, const int32_t *new_id,
                const int64_t *append_keys) {
    int32_t rc = make_byte_rows(nx.get());
    if (!rc && !idx->split_rows_freed) rc = make_split_rows(nx.get());
    if (!rc && idx->half_rows_on && nx->iv.n > 0) rc = make_half_rows(nx.get());
    if (!rc && idx->sq8_on && nx->iv.n > 0) rc = make_sq8_rows(nx.get());
    if (!rc && idx->sq8d_on && nx->iv.n > 0) rc = make_sq8_dim_rows(nx.get());
    if (!rc && idx->bit_mode && nx->iv.n > 0) rc = make_bit_rows(nx.get(), idx->bit_mode);   // (option bit_rows: likewise; mode 1's means move)
    if (!rc && carry_codes) rc = extend_locality_codes(idx, nx.get());
    // soft deletion: the marks move with their nodes; the new live mask is complete before anything is swapped
    std::unique_ptr<hnsw_filter> live;
    if (!rc) rc = renumbered_live_filter(idx, new_id, nx->iv.n, live);
    // keys: they move with their nodes too (on the device: keys_renumber_kernel), lookup table and all, before anything is swapped
    std::unique_ptr<KeyTables> keys;
    if (!rc) rc = renumbered_keys(idx, new_id, nx->iv.n, append_keys, keys);
    if (rc) {
        nx.reset();
        (void)hipGetLastError();                    // (a failed allocation must not surface in the next call on this handle)
        return rc;
    }
    // swap: work still in flight on caller streams (hnsw_search_batch_device) reads the old tables
    {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return fail(HNSW_ERR_HIP, "hipDeviceSynchronize failed: %s", hipGetErrorString(e));
    }
    const int rows_before = idx->info.row_format;
    const int64_t n = nx->iv.n;
    std::swap(idx->tables, nx->tables);                    // (nx takes the old tables with it)
    idx->iv = nx->iv;
    idx->info = nx->info;
    idx->sq8_lo = nx->sq8_lo; idx->sq8_scale = nx->sq8_scale;   // (of the swapped-in codes, if any)
    idx->sq8d_lo = std::move(nx->sq8d_lo); idx->sq8d_scale = std::move(nx->sq8d_scale);
    idx->bit_t = std::move(nx->bit_t);
    bind_view(idx);                                        // the options keep their effect
    idx->lcode_state = nx->lcode_state;                    // 1: carried over; 0: built on demand (also where the old graph could not)
    nx.reset();
    idx->epoch++;                                          // filters made for the graph before are refused from now on
    idx->n_deleted = live ? n - live->n_allowed : 0;
    if (live) live->epoch = idx->epoch;
    idx->live = std::move(live);                           // (null when nothing is marked any more)
    idx->keys = std::move(keys);                           // (null on a handle without keys)
    // the per-shape decisions that follow n or the row format
    idx->forget_shapes(/*keep_visited=*/carry_codes && rows_before == idx->info.row_format);
    if (idx->fb_queries > 0 && n > 0) idx->fb_queries = std::min<int64_t>((int64_t)idx->dFbSlab.bytes / (n * 4), 65536);
    // the new index is searched at the steady-state rate from its first call, as a loaded one
    (void)warm_up(idx);
    const std::vector<std::pair<int, int>> shapes = idx->prepared;
    for (const auto &pr : shapes) prepare_quietly(idx, pr.first, pr.second);
    prepare_quietly(idx, expected_ef, expected_semantics);
    return HNSW_OK;
}

} // namespace hnsw_host

// The levels and the upper-row layout of m nodes appended behind n_old nodes that hold rowsU_old upper rows: node n_old + j draws
// position n_old + j's level.  Shared by hnsw_index_insert and the insert half of hnsw_index_upsert_keyed / hnsw_index_update.
namespace {
struct GrowPlan {
    std::vector<uint8_t> lvl;          // [m]
    std::vector<int2> ref;             // [m]: (first upper row or -1, level)
    int64_t rowsU = 0;                 // upper rows afterwards
    int lcap_new = 1;                  // 1 + the highest new level
};
GrowPlan grow_plan(const hnsw_build_params *p, int64_t n_old, int64_t m, int64_t rowsU_old) {
    GrowPlan g;
    const double level_mult = 1.0 / std::log((double)p->num_connections);
    g.lvl.resize((size_t)m);
    for (int64_t j = 0; j < m; ++j) g.lvl[(size_t)j] = node_level(p->seed, n_old + j, level_mult);
    for (uint8_t l : g.lvl) g.lcap_new = std::max(g.lcap_new, (int)l + 1);
    g.rowsU = upper_layout(g.lvl.data(), m, rowsU_old, g.ref);
    return g;
}
} // namespace

int64_t hnsw_host::grown_upper_rows(const hnsw_build_params *p, int64_t n_old, int64_t m, int64_t rowsU_old) {
    return grow_plan(p, n_old, m, n_old > 0 ? rowsU_old : 0).rowsU;
}

// "Grow in place": nx holds a graph of n_old = nx->iv.n nodes (rows compacted or with holes, widths nx->iv.S0 / SU = 2M / M) in
// tables that alloc_graph_tables sized for n_old + m nodes and grown_upper_rows upper rows, the rows behind the graph empty;
// nx->info names its metric.  The m vectors are uploaded behind the stored ones (COSINE: normalised), their layout written, and
// run_batches inserts them from position n_old on those same tables.  On an error nx is to be discarded, never patched.
int hnsw_host::grow_graph_in_place(hnsw_index *nx, const float *vectors, int64_t m, int64_t row_stride, const hnsw_build_params *p,
                                   int64_t rem_scale, bool *rem_overflow) {
    *rem_overflow = false;
    IndexTables &t = nx->tables;
    IndexView &iv = nx->iv;
    const int64_t n_old = iv.n, n = n_old + m, stride = iv.stride;
    const int M = p->num_connections;
    const GrowPlan g = grow_plan(p, n_old, m, n_old > 0 ? iv.rowsU : 0);
    int cur_max = n_old > 0 ? iv.max_layer : 0, entry = n_old > 0 ? iv.entry_point : 0;
    const int lcap = std::max(cur_max + 1, g.lcap_new);
    int rc;
    BuildView bv{};
    if ((rc = upload_rows(vectors, m, iv.d, row_stride, (float *)t.X.p + n_old * stride))) return rc;
    // COSINE: the new rows only -- the old ones are N(X) already (row numbers in the message: of the m new vectors)
    if (nx->info.metric == HNSW_METRIC_COSINE && (rc = cosine_store_rows((float *)t.X.p + n_old * stride, m, iv.d, "nothing inserted"))) return rc;
    if ((rc = upload_upper_layout(t, n_old, g.ref))) return rc;
    iv.n = n; iv.S0 = 2 * M; iv.SU = M; iv.rowsU = g.rowsU; iv.max_layer = cur_max; iv.entry_point = entry;
    bind_view(nx);                                                      // (the derived tables are the caller's)
    bv.iv = iv; bv.nbr0_w = (int32_t *)t.nbr0.p; bv.nbrU_w = (int32_t *)t.nbrU.p;
    if (n > 1 && (rc = run_batches(bv, g.lvl.data() + (n_old > 0 ? 0 : 1), std::max<int64_t>(n_old, 1), n, lcap, p, rem_scale,
                                   rem_overflow, &cur_max, &entry))) return rc;
    iv.max_layer = cur_max; iv.entry_point = entry;
    nx->info.max_degree = M;
    bind_view(nx);
    return HNSW_OK;
}

// One attempt of hnsw_index_insert: a new handle `out` with the graph of idx grown by the m vectors.  "Make tables + copy old":
// idx's tables copied (rows widened to 2M / M) into tables sized for n_old + m nodes; then grow_graph_in_place.  idx is only read.
// The derived tables (byte / split rows, locality codes) are the caller's.
int hnsw_host::insert_graph(const hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride, const hnsw_build_params *p,
                            int64_t rem_scale, bool *rem_overflow, IndexPtr &out) {
    *rem_overflow = false;
    out.reset();
    const IndexView &ov = idx->iv;
    const int64_t n_old = ov.n, n = n_old + m;
    const int M = p->num_connections, S0 = 2 * M, SU = M;
    const int S0o = ov.S0, SUo = ov.SU;
    const int64_t stride = ov.stride, rowsU_old = n_old > 0 ? ov.rowsU : 0;
    const int64_t rowsU = grown_upper_rows(p, n_old, m, rowsU_old);
    if (rowsU > 0x7FFFFFF0LL) return fail(HNSW_ERR_UNSUPPORTED, "too many upper rows");

    IndexPtr nx(new hnsw_index());
    nx->device = idx->device;
    int rc;
    const IndexTables &ot = idx->tables;
    IndexTables &t = nx->tables;
    if ((rc = alloc_graph_tables(t, n, stride, S0, SU, rowsU))) return rc;
    if (n_old > 0) {
        HIP_TRY(hipMemcpy(t.X.p, ot.X.p, (size_t)n_old * stride * 4, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(t.off.p, ot.off.p, (size_t)n_old * 4, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(t.lvl.p, ot.lvl.p, (size_t)n_old, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(t.ref.p, ot.ref.p, (size_t)n_old * sizeof(int2), hipMemcpyDeviceToDevice));
    }
    HIP_TRY(widen_rows(ot.nbr0.p, n_old, S0o, t.nbr0.p, S0));
    HIP_TRY(widen_rows(ot.nbrU.p, rowsU_old, SUo, t.nbrU.p, SU));
    nx->iv = ov;                                                        // d, stride, nchunks, id_base; n_old, top and entry
    nx->iv.S0 = S0; nx->iv.SU = SU; nx->iv.rowsU = rowsU_old;
    nx->info = idx->info;                                               // d, metric, id_base, device
    if ((rc = grow_graph_in_place(nx.get(), vectors, m, row_stride, p, rem_scale, rem_overflow))) return rc;
    out = std::move(nx);
    return HNSW_OK;
}

extern "C" {

int32_t hnsw_build(const float *vectors, int64_t n, int32_t d, int64_t row_stride,
                   const hnsw_build_params *p, int32_t device, hnsw_index **out) {
    // Removals (links dropped when a neighbour's row is re-selected) are buffered per step; a step that
    // produces more than the buffer holds invalidates the attempt -- a dropped removal would leave an
    // asymmetric link, which Graph.Test.invariant (lib/ohnsw.ml:217-225) forbids -- and the build is repeated
    // with four times the room (deterministic: same graph as if the buffer had been large from the start).
    int32_t rc = HNSW_OK;
    for (int64_t scale = 1; scale <= 64; scale *= 4) {
        bool overflow = false;
        rc = build_attempt(vectors, n, d, row_stride, p, device, out, scale, &overflow);
        if (!overflow) return rc;
    }
    return rc;   // HNSW_ERR_DEGREE_OVERFLOW with the message of the last attempt
}

int32_t hnsw_index_insert(hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride, const hnsw_build_params *p) {
    if (idx && idx->keys)
        return fail(HNSW_ERR_BAD_ARG, "the index has keys and must never hold a node without one: hnsw_index_insert_keyed (the keyed call) inserts into it");
    return insert_vectors(idx, vectors, m, row_stride, p, nullptr);
}

} // extern "C"

// What hnsw_index_insert refuses of its arguments before anything is built (m > 0): idx holds n_old nodes with top layer max_layer
// when the m vectors arrive -- its own, or, for the insert half of an upsert, what the removal half will leave.
int hnsw_host::check_insert(const hnsw_index *idx, int64_t n_old, int max_layer, const float *vectors, int64_t m, int64_t row_stride,
                            const hnsw_build_params *p) {
    const int64_t n = n_old + m;
    if (!vectors) return fail(HNSW_ERR_BAD_ARG, "null vectors");
    if (n > 0x7FFFFFF0LL) return fail(HNSW_ERR_BAD_ARG, "n=%lld out of range", (long long)n);
    if (row_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "row_stride=%lld < d=%d", (long long)row_stride, idx->iv.d);
    if (p->metric != idx->info.metric) return fail(HNSW_ERR_BAD_ARG, "metric %d differs from the index's %d", p->metric, idx->info.metric);
    if (p->id_base != idx->iv.id_base) return fail(HNSW_ERR_BAD_ARG, "id_base %d differs from the index's %d", p->id_base, idx->iv.id_base);
    { const int32_t rcp = check_build_params(p); if (rcp) return rcp; }
    const int M = p->num_connections;
    if (n_old > 0 && idx->iv.S0 > 2 * M)
        return fail(HNSW_ERR_BAD_ARG, "max_degree0=%d of the index is wider than 2 * num_connections=%d", idx->iv.S0, 2 * M);
    if (n_old > 0 && max_layer > 0 && idx->iv.SU > M)
        return fail(HNSW_ERR_BAD_ARG, "max_degree=%d of the index is wider than num_connections=%d", idx->iv.SU, M);
    if (n_old > 0 && idx->iv.entry_point < 0) return fail(HNSW_ERR_BAD_ARG, "the index has nodes but no entry point");
    if (idx->live_requests > 0) return fail(HNSW_ERR_BAD_ARG, "%d submitted requests not waited for (hnsw_search_wait first)", idx->live_requests);
    if (idx->multi_replica) return fail(HNSW_ERR_BAD_ARG, "the index is a replica of an hnsw_multi: inserting into one replica would desynchronise the others");
    if (idx->fb_queries > 0 && (int64_t)idx->dFbSlab.bytes / (n * 4) < 1)
        return fail(HNSW_ERR_BAD_ARG, "device_fallback_slab_bytes=%lld holds no query of the grown index: one needs 4 n = %lld bytes",
                    (long long)idx->dFbSlab.bytes, (long long)(n * 4));
    // option sq8_rows is on: the codes are made again over the grown table, which needs every value finite -- asked before the
    // graph is grown, not after
    if (codes_on(idx))
        for (int64_t i = 0; i < m; ++i)
            for (int32_t j = 0; j < idx->iv.d; ++j)
                if (!std::isfinite(vectors[i * row_stride + j]))
                    return fail(HNSW_ERR_UNSUPPORTED, "%s: value %d of new vector %lld is NaN or infinite: nothing inserted", codes_option(idx), j, (long long)i);
    return HNSW_OK;
}

int hnsw_host::insert_vectors(hnsw_index *idx, const float *vectors, int64_t m, int64_t row_stride, const hnsw_build_params *p, const int64_t *keys) {
    if (!idx || !p) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (m == 0) return HNSW_OK;
    const int64_t n_old = idx->iv.n;
    { const int32_t rcc = check_insert(idx, n_old, idx->iv.max_layer, vectors, m, row_stride, p); if (rcc) return rcc; }
    HIP_TRY(hipSetDevice(idx->device));
    if (n_old > 0) { const int32_t rcu = check_upper_rows(idx, "not grown"); if (rcu) return rcu; }

    // the grown graph, in tables of its own: on any error idx is as it was (overflow: again from idx's tables, 4x the room)
    IndexPtr nx;
    int32_t rc = HNSW_OK;
    for (int64_t scale = 1; scale <= 64; scale *= 4) {
        bool overflow = false;
        rc = insert_graph(idx, vectors, m, row_stride, p, scale, &overflow, nx);
        if (!overflow) break;
    }
    if (rc) {
        nx.reset();
        (void)hipGetLastError();
        return rc;
    }
    return adopt_graph(idx, nx, /*carry_codes=*/true, p->expected_ef, p->expected_semantics, nullptr, keys);
}

extern "C" {

// ---- select_neighbours operator ----------------------------------------------------------------------
int32_t hnsw_select_neighbours_batch(hnsw_index *idx, const float *targets, int64_t nb, int64_t t_stride,
                                     const int32_t *cand, const int32_t *cand_cnt, int32_t cand_stride,
                                     int32_t num_neighbours, int32_t keep_all_if_few, const int32_t *cand_degree,
                                     int32_t *out, int32_t *out_cnt) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (nb == 0) return HNSW_OK;
    if (nb < 0 || !targets || !cand || !cand_cnt || !out || !out_cnt) return fail(HNSW_ERR_BAD_ARG, "bad buffers");
    if (t_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "t_stride < d");
    if (num_neighbours < 1 || num_neighbours > 64) return fail(HNSW_ERR_UNSUPPORTED, "num_neighbours must be in 1..64");
    if (cand_stride < 1 || cand_stride > 1024) return fail(HNSW_ERR_UNSUPPORTED, "cand_stride must be in 1..1024");
    const int base = idx->iv.id_base;
    std::vector<int32_t> c0((size_t)nb * cand_stride, 0);
    for (int64_t b = 0; b < nb; ++b) {
        if (cand_cnt[b] < 0 || cand_cnt[b] > cand_stride) return fail(HNSW_ERR_BAD_ARG, "cand_cnt out of range");
        if (keep_all_if_few && cand_cnt[b] <= num_neighbours && cand_cnt[b] > 64) return fail(HNSW_ERR_UNSUPPORTED, "keep-all needs <= 64 candidates");
        if (cand_degree) {
            int forced = 0;
            for (int j = 0; j < cand_cnt[b]; ++j) forced += cand_degree[b * cand_stride + j] <= 1;
            // forced >= M: the reference's loop only checks the bound after an addition, so it can
            // return more than num_neighbours (hnsw_algo.ml:591-592, 600-606); refuse instead of truncating
            if (forced >= num_neighbours && cand_cnt[b] > num_neighbours)
                return fail(HNSW_ERR_DEGREE_OVERFLOW, "do_not_isolate forces %d >= num_neighbours=%d candidates", forced, num_neighbours);
        }
        for (int j = 0; j < cand_cnt[b]; ++j) {
            const int64_t v = (int64_t)cand[b * cand_stride + j] - base;
            if (v < 0 || v >= idx->iv.n) return fail(HNSW_ERR_BAD_ARG, "Vector.get: candidate id out of range");
            c0[(size_t)(b * cand_stride + j)] = (int32_t)v;
        }
    }
    HIP_TRY(hipSetDevice(idx->device));
    DevBuf dT, dC, dN, dO, dOc, dDg;
    int rc;
    const size_t tbytes = ((size_t)(nb - 1) * t_stride + idx->iv.d) * 4;
    if ((rc = dT.ensure(tbytes)) || (rc = dC.ensure(c0.size() * 4)) || (rc = dN.ensure((size_t)nb * 4)) ||
        (rc = dO.ensure((size_t)nb * num_neighbours * 4)) || (rc = dOc.ensure((size_t)nb * 4))) return rc;
    if (cand_degree) {
        if ((rc = dDg.ensure((size_t)nb * cand_stride * 4))) return rc;
        if (hipMemcpy(dDg.p, cand_degree, (size_t)nb * cand_stride * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(HNSW_ERR_HIP, "upload failed");
    }
    if (hipMemcpy(dT.p, targets, tbytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dC.p, c0.data(), c0.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dN.p, cand_cnt, (size_t)nb * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(HNSW_ERR_HIP, "upload failed");
    // (COSINE: the uploaded copy becomes N(targets) in place)
    if (is_cosine(idx) && (rc = cosine_normalise((const float *)dT.p, nb, idx->iv.d, t_stride, (float *)dT.p, t_stride, nullptr, nullptr, nullptr))) return rc;
    SelectOpArgs sa{};
    sa.targets = (const float *)dT.p; sa.t_stride = t_stride; sa.cand = (const int32_t *)dC.p; sa.cand_cnt = (const int32_t *)dN.p;
    sa.cand_stride = cand_stride; sa.nb = (int32_t)nb; sa.R = num_neighbours; sa.keep_all_if_few = keep_all_if_few;
    sa.out = (int32_t *)dO.p; sa.out_cnt = (int32_t *)dOc.p; sa.cand_deg = cand_degree ? (const int32_t *)dDg.p : nullptr;
    const size_t lds = ((size_t)4 * cand_stride + 128) * 4;
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(pick_nch(idx->iv.nchunks), [&](auto NCH) {
        hipLaunchKernelGGL((hnsw_dev::select_neighbours_kernel<NCH, rows_in_flight(NCH), METRIC>), dim3((unsigned)nb), dim3(64), lds, 0, idx->iv, sa);
    }); });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dO.p, (size_t)nb * num_neighbours * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_cnt, dOc.p, (size_t)nb * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "select_neighbours failed: %s", hipGetErrorString(e));
    for (int64_t i = 0; i < nb * num_neighbours; ++i) if (out[i] >= 0) out[i] += base;
    return HNSW_OK;
}

// ---- export (the inverse of hnsw_index_create's flatten) ------------------------------------------
int32_t hnsw_index_export_layer0(const hnsw_index *idx, int32_t *deg0, int32_t *nbr0) {
    if (!idx || !deg0 || !nbr0) return fail(HNSW_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n; const int S0 = idx->iv.S0; const int base = idx->iv.id_base;
    HIP_TRY(hipMemcpy(nbr0, idx->tables.nbr0.p, (size_t)n * S0 * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
        int w = 0;
        int32_t *row = nbr0 + i * S0;
        for (int j = 0; j < S0; ++j) if (row[j] >= 0) row[w++] = row[j] + base;
        deg0[i] = w;
        for (int j = w; j < S0; ++j) row[j] = -1;
    }
    return HNSW_OK;
}

int32_t hnsw_index_export_upper_count(const hnsw_index *idx, int32_t layer, int64_t *n_nodes) {
    if (!idx || !n_nodes) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (layer < 1 || layer > idx->iv.max_layer) return fail(HNSW_ERR_BAD_ARG, "layer %d out of range", layer);
    HIP_TRY(hipSetDevice(idx->device));
    std::vector<uint8_t> lvl((size_t)idx->iv.n);
    HIP_TRY(hipMemcpy(lvl.data(), idx->tables.lvl.p, (size_t)idx->iv.n, hipMemcpyDeviceToHost));
    int64_t c = 0;
    for (int64_t i = 0; i < idx->iv.n; ++i) c += lvl[(size_t)i] >= layer;
    *n_nodes = c;
    return HNSW_OK;
}

int32_t hnsw_index_export_upper(const hnsw_index *idx, int32_t layer, int64_t *nodes, int32_t *deg, int32_t *nbr) {
    if (!idx || !nodes || !deg || !nbr) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (layer < 1 || layer > idx->iv.max_layer) return fail(HNSW_ERR_BAD_ARG, "layer %d out of range", layer);
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n; const int SU = idx->iv.SU; const int base = idx->iv.id_base;
    std::vector<uint8_t> lvl((size_t)n);
    std::vector<int32_t> off((size_t)n), rows((size_t)std::max<int64_t>(idx->iv.rowsU, 1) * SU);
    HIP_TRY(hipMemcpy(lvl.data(), idx->tables.lvl.p, (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(off.data(), idx->tables.off.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rows.data(), idx->tables.nbrU.p, rows.size() * 4, hipMemcpyDeviceToHost));
    int64_t s = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (lvl[(size_t)i] < layer) continue;
        const int32_t *row = &rows[((size_t)off[(size_t)i] + (layer - 1)) * SU];
        int w = 0;
        for (int j = 0; j < SU; ++j) if (row[j] >= 0) nbr[s * SU + w++] = row[j] + base;
        for (int j = w; j < SU; ++j) nbr[s * SU + j] = -1;
        nodes[s] = i + base; deg[s] = w;
        s++;
    }
    return HNSW_OK;
}


// ---- per-layer degree statistics: Hgraph.Stats (lib/hnsw.ml:353-375) -----------------------------
// min_max_connectivity (:361-368) folds the layer's connections map from (1000000, -1, 0, 0., []): min / max / mean of
// the neighbour-list lengths and the list of nodes without a neighbour.  One thread per node over the device-resident
// tables; the keys of layer l >= 1 are the nodes whose level reaches l (upper_ref), of layer 0 every node.
namespace {
struct StatsAcc { unsigned long long cnt, sum, iso; int mi, ma; };

__global__ void __launch_bounds__(256)
layer_stats_kernel(const int32_t *nbr0, int32_t S0, const int32_t *nbrU, int32_t SU, const int2 *upper_ref, int64_t n,
                   int32_t layer, StatsAcc *acc, int64_t *iso_ids, unsigned long long iso_cap) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t *row; int w;
    if (layer == 0) { row = nbr0 + i * S0; w = S0; }
    else {
        const int2 ref = upper_ref[i];
        if (ref.y < layer) return;                                   // not a key of this layer
        row = nbrU + ((int64_t)ref.x + (layer - 1)) * SU; w = SU;
    }
    int dg = 0;
    for (int j = 0; j < w; ++j) dg += row[j] >= 0;                   // Neighbours.length
    atomicAdd(&acc->cnt, 1ull); atomicAdd(&acc->sum, (unsigned long long)dg);
    atomicMin(&acc->mi, dg); atomicMax(&acc->ma, dg);
    if (dg == 0) {
        const unsigned long long at = atomicAdd(&acc->iso, 1ull);
        if (at < iso_cap) iso_ids[at] = i;
    }
}

// runs the kernel once; with iso != nullptr also collects the isolated nodes (0-based, unordered)
int layer_stats_device(const hnsw_index *idx, int32_t layer, StatsAcc *out, std::vector<int64_t> *iso) {
    if (layer < 0 || layer > idx->iv.max_layer) return fail(HNSW_ERR_BAD_ARG, "layer %d out of range", layer);
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n;
    StatsAcc h{0, 0, 0, 1000000, -1};
    if (n == 0) { *out = h; if (iso) iso->clear(); return HNSW_OK; }
    DevBuf dAcc, dIso;
    int rc;
    if ((rc = dAcc.ensure(sizeof(StatsAcc)))) return rc;
    unsigned long long cap = 0;
    for (int pass = 0; pass < 2; ++pass) {                          // second pass only when there are isolated nodes to list
        HIP_TRY(hipMemcpy(dAcc.p, &h, sizeof h, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(layer_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, idx->iv.nbr0, idx->iv.S0,
                           idx->iv.nbrU, idx->iv.SU, idx->iv.upper_ref, n, layer, (StatsAcc *)dAcc.p, (int64_t *)dIso.p, cap);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out, dAcc.p, sizeof *out, hipMemcpyDeviceToHost));
        if (!iso || out->iso == 0 || pass == 1) break;
        cap = out->iso;
        if ((rc = dIso.ensure((size_t)cap * 8))) return rc;
    }
    if (iso) {
        iso->resize((size_t)out->iso);
        if (out->iso) HIP_TRY(hipMemcpy(iso->data(), dIso.p, (size_t)out->iso * 8, hipMemcpyDeviceToHost));
    }
    return HNSW_OK;
}
} // namespace

int32_t hnsw_index_layer_stats(const hnsw_index *idx, int32_t layer, hnsw_layer_stats *out) {
    if (!idx || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    StatsAcc a;
    int rc = layer_stats_device(idx, layer, &a, nullptr);
    if (rc) return rc;
    out->num_nodes = (int64_t)a.cnt; out->min_degree = a.mi; out->max_degree = a.ma;       // empty layer: 1000000 / -1 / nan, as the fold's
    out->mean_degree = (double)a.sum / (double)a.cnt;                                      // initial value leaves them (0. /. 0.)
    out->num_isolated = (int64_t)a.iso;
    return HNSW_OK;
}

int32_t hnsw_index_layer_isolated(const hnsw_index *idx, int32_t layer, int64_t *ids, int64_t cap, int64_t *count) {
    if (!idx || !count || cap < 0 || (cap > 0 && !ids)) return fail(HNSW_ERR_BAD_ARG, "null argument");
    StatsAcc a;
    std::vector<int64_t> iso;
    int rc = layer_stats_device(idx, layer, &a, &iso);
    if (rc) return rc;
    std::sort(iso.begin(), iso.end(), [](int64_t x, int64_t y) { return x > y; });   // key :: isolated during an ascending fold: descending ids
    *count = (int64_t)iso.size();
    for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t)iso.size()); ++i) ids[i] = iso[(size_t)i] + idx->iv.id_base;
    return HNSW_OK;
}

// ---- flattened-index file: header + vectors + layer 0 + upper layers (little endian) ---------------
namespace {
struct FileHeader {
    char magic[8];        // "HNSWMI35"
    uint32_t version;     // 1: vectors + graph; 2: + the trailer "PREP" (decisions, locality codes)
    int32_t d, metric, id_base, max_degree0, max_degree, max_layer, reserved;
    int64_t n, entry_point;
};
bool wr(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }
bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
} // namespace

int32_t hnsw_index_save(const hnsw_index *idx, const char *path) {
    if (!idx || !path) return fail(HNSW_ERR_BAD_ARG, "null argument");
    // (a file that brings deleted vectors back is the one outcome to rule out; the format has no place for the marks)
    if (idx->n_deleted > 0)
        return fail(HNSW_ERR_BAD_ARG, "%lld marked nodes are not saved: compact or unmark first", (long long)idx->n_deleted);
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n; const int d = idx->iv.d; const int S0 = idx->iv.S0, SU = idx->iv.SU;
    FILE *f = fopen(path, "wb");
    if (!f) return fail(HNSW_ERR_BAD_ARG, "cannot open %s for writing", path);
    FileHeader h{};
    memcpy(h.magic, "HNSWMI35", 8); h.version = 2; h.d = d; h.metric = idx->info.metric; h.id_base = idx->iv.id_base;
    h.max_degree0 = S0; h.max_degree = idx->info.max_degree; h.max_layer = idx->iv.max_layer; h.n = n;
    h.entry_point = idx->info.entry_point;
    bool ok = wr(f, &h, sizeof h);
    {   // vectors, unpadded, in chunks
        const int64_t stride = idx->iv.stride;
        const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / (stride * 4));
        std::vector<float> stage((size_t)chunk * stride), packed((size_t)chunk * d);
        for (int64_t r0 = 0; ok && r0 < n; r0 += chunk) {
            const int64_t nr = std::min(chunk, n - r0);
            if (hipMemcpy(stage.data(), (const float *)idx->tables.X.p + r0 * stride, (size_t)nr * stride * 4, hipMemcpyDeviceToHost) != hipSuccess) { ok = false; break; }
            for (int64_t i = 0; i < nr; ++i) memcpy(&packed[(size_t)i * d], &stage[(size_t)i * stride], (size_t)d * 4);
            ok = wr(f, packed.data(), (size_t)nr * d * 4);
        }
    }
    std::vector<int32_t> deg0((size_t)std::max<int64_t>(n, 1)), nbr0((size_t)std::max<int64_t>(n, 1) * S0);
    if (ok && n > 0) ok = hnsw_index_export_layer0(idx, deg0.data(), nbr0.data()) == HNSW_OK;
    ok = ok && wr(f, deg0.data(), (size_t)n * 4) && wr(f, nbr0.data(), (size_t)n * S0 * 4);
    for (int l = 1; ok && l <= idx->iv.max_layer; ++l) {
        int64_t c = 0;
        ok = hnsw_index_export_upper_count(idx, l, &c) == HNSW_OK;
        std::vector<int64_t> nodes((size_t)std::max<int64_t>(c, 1));
        std::vector<int32_t> deg((size_t)std::max<int64_t>(c, 1)), nbr((size_t)std::max<int64_t>(c, 1) * SU);
        ok = ok && hnsw_index_export_upper(idx, l, nodes.data(), deg.data(), nbr.data()) == HNSW_OK;
        ok = ok && wr(f, &c, 8) && wr(f, nodes.data(), (size_t)c * 8) && wr(f, deg.data(), (size_t)c * 4) && wr(f, nbr.data(), (size_t)c * SU * 4);
    }
    {   // format 2: what the handle has learnt -- the locality codes (if built) and the visited-structure decisions per kernel shape
        std::vector<int32_t> dec;
        list_blk_choices(idx, dec);
        for (const auto &pr : idx->prepared) {                       // prepared shapes without a decision of their own (W in one / two registers): kept
            bool have = false;
            for (size_t i = 0; i + 2 < dec.size(); i += 3) have = have || (dec[i] == pr.first && dec[i + 1] == (pr.second ? 1 : 0));
            if (!have) { dec.push_back(pr.first); dec.push_back(pr.second); dec.push_back(-1); }
        }
        const uint32_t n_dec = (uint32_t)(dec.size() / 3), has_codes = idx->lcode_state == 1 && idx->tables.lcode.p ? 1u : 0u;
        ok = ok && wr(f, "PREP", 4) && wr(f, &n_dec, 4) && wr(f, dec.data(), dec.size() * 4) && wr(f, &has_codes, 4);
        if (ok && has_codes) {
            std::vector<int32_t> codes((size_t)n);
            ok = hipMemcpy(codes.data(), idx->tables.lcode.p, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess && wr(f, codes.data(), (size_t)n * 4);
        }
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) return fail(HNSW_ERR_HIP, "writing %s failed", path);
    return HNSW_OK;
}

int32_t hnsw_index_load(const char *path, int32_t device, hnsw_index **out) {
    if (!path || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(HNSW_ERR_BAD_ARG, "cannot open %s", path);
    FileHeader h{};
    if (!rd(f, &h, sizeof h) || memcmp(h.magic, "HNSWMI35", 8) != 0 || (h.version != 1 && h.version != 2)) { fclose(f); return fail(HNSW_ERR_BAD_ARG, "%s is not a flattened hnsw index (format 1 or 2)", path); }
    if (h.n < 0 || h.n > 0x7FFFFFF0LL || h.d < 1 || h.max_degree0 < 1 || h.max_degree0 > 64 || h.max_layer < 0 || h.max_layer > 255) { fclose(f); return fail(HNSW_ERR_BAD_ARG, "%s: corrupt header", path); }
    const int64_t n = h.n;
    const int SU = h.max_layer > 0 ? h.max_degree : 1;
    if (h.max_layer > 0 && (SU < 1 || SU > 64)) { fclose(f); return fail(HNSW_ERR_BAD_ARG, "%s: corrupt header", path); }
    std::vector<float> X((size_t)std::max<int64_t>(n, 1) * h.d);
    std::vector<int32_t> deg0((size_t)std::max<int64_t>(n, 1)), nbr0((size_t)std::max<int64_t>(n, 1) * h.max_degree0);
    bool ok = rd(f, X.data(), (size_t)n * h.d * 4) && rd(f, deg0.data(), (size_t)n * 4) && rd(f, nbr0.data(), (size_t)n * h.max_degree0 * 4);
    std::vector<std::vector<int64_t>> nodes((size_t)h.max_layer);
    std::vector<std::vector<int32_t>> deg((size_t)h.max_layer), nbr((size_t)h.max_layer);
    std::vector<hnsw_layer_desc> layers((size_t)std::max(h.max_layer, 1));
    for (int l = 0; ok && l < h.max_layer; ++l) {
        int64_t c = 0;
        ok = rd(f, &c, 8) && c >= 0 && c <= n;
        if (!ok) break;
        nodes[(size_t)l].resize((size_t)std::max<int64_t>(c, 1)); deg[(size_t)l].resize((size_t)std::max<int64_t>(c, 1)); nbr[(size_t)l].resize((size_t)std::max<int64_t>(c, 1) * SU);
        ok = rd(f, nodes[(size_t)l].data(), (size_t)c * 8) && rd(f, deg[(size_t)l].data(), (size_t)c * 4) && rd(f, nbr[(size_t)l].data(), (size_t)c * SU * 4);
        layers[(size_t)l] = hnsw_layer_desc{c, nodes[(size_t)l].data(), deg[(size_t)l].data(), nbr[(size_t)l].data()};
    }
    // format 2: decisions and codes (an unreadable trailer is ignored: everything in it can be made again)
    std::vector<int32_t> dec, codes;
    if (ok && h.version >= 2) {
        char tag[4];
        uint32_t n_dec = 0, has_codes = 0;
        bool tok = rd(f, tag, 4) && memcmp(tag, "PREP", 4) == 0 && rd(f, &n_dec, 4) && n_dec <= 64;
        if (tok) { dec.resize((size_t)n_dec * 3); tok = rd(f, dec.data(), dec.size() * 4) && rd(f, &has_codes, 4); }
        if (tok && has_codes == 1 && n > 0) { codes.resize((size_t)n); tok = rd(f, codes.data(), (size_t)n * 4); }
        if (tok && !codes.empty()) {          // a permutation of 0 .. n-1, or not used
            std::vector<uint8_t> seen((size_t)n, 0);
            for (int64_t i = 0; tok && i < n; ++i) {
                const int32_t c = codes[(size_t)i];
                tok = c >= 0 && c < n && !seen[(size_t)c];
                if (tok) seen[(size_t)c] = 1;
            }
        }
        if (!tok) { dec.clear(); codes.clear(); }
    }
    fclose(f);
    if (!ok) return fail(HNSW_ERR_BAD_ARG, "%s: truncated or corrupt", path);
    hnsw_index_desc d{};
    d.vectors = X.data(); d.n = n; d.d = h.d; d.row_stride = h.d; d.metric = h.metric; d.id_base = h.id_base;
    d.max_degree0 = h.max_degree0; d.max_degree = h.max_degree; d.max_layer = h.max_layer; d.entry_point = h.entry_point;
    d.deg0 = deg0.data(); d.nbr0 = nbr0.data(); d.upper = layers.data();
    const int rc = create_index(&d, device, /*stored_rows=*/true, out);   // re-validates every id and degree; COSINE rows stay as saved
    if (rc) return rc;
    hnsw_index *idx = *out;
    if (!codes.empty()) (void)adopt_locality_codes(idx, codes.data());
    for (size_t i = 0; i + 2 < dec.size(); i += 3)
        if (dec[i + 2] >= 0) adopt_blk_choice(idx, dec[i], dec[i + 1], dec[i + 2] > 0);
    // every saved shape is prepared again (residency, code objects); its decision is already in place, nothing is measured
    for (size_t i = 0; i + 2 < dec.size(); i += 3) prepare_quietly(idx, dec[i], dec[i + 1]);
    return HNSW_OK;
}

} // extern "C"
