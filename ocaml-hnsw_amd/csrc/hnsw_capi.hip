// hnsw_capi.hip -- host side of libhnsw_mi355x.so: the C ABI of include/hnsw_mi355x.h.
//
// Flattens the reference's graph containers (Ohnsw.Hgraph.t lib/ohnsw.ml:307-312 /
// Hnsw.Ba.Hgraph.t lib/hnsw.ml:342-348, as handed over by the OCaml shim) into HBM-resident
// tables and launches the gfx950 kernels of hnsw_device.hip.h.  No CPU fallback: without a
// usable device every compute entry point fails with HNSW_ERR_NO_DEVICE.
#include "hnsw_internal.h"

#include <mutex>

using hnsw_dev::IndexView;
using hnsw_dev::SearchArgs;
using namespace hnsw_host;

// probe queries of the visited-structure measurement (knn_blk_bits): query j = the midpoint between node j * step's vector and
// its first layer-0 neighbour's (the node's own vector if it has none); rows of `stride` floats, padding zero as in the table
__global__ void __launch_bounds__(64)
probe_queries_kernel(const IndexView iv, int64_t step, float *out) {
    const int64_t v = (int64_t)blockIdx.x * step;
    const int32_t nb = iv.nbr0[v * iv.S0];
    const int64_t u = nb >= 0 ? (int64_t)nb : v;
    for (int64_t i = threadIdx.x; i < iv.stride; i += 64)
        out[(int64_t)blockIdx.x * iv.stride + i] = 0.5f * (iv.X[v * iv.stride + i] + iv.X[u * iv.stride + i]);
}

// The flagged queries of a launch (status bit 0), listed on the device: map[0 .. cap) = their indices, -1 beyond the count
// (the re-run kernel's blocks with a -1 entry leave at once); map[cap] = how many there were.  One workgroup.
__global__ void __launch_bounds__(1024)
flagged_list_kernel(const uint32_t *status, int64_t nq, int32_t *map, int32_t cap) {
    __shared__ int32_t count;
    if (threadIdx.x == 0) count = 0;
    for (int i = threadIdx.x; i < cap; i += blockDim.x) map[i] = -1;
    __syncthreads();
    for (int64_t q = threadIdx.x; q < nq; q += blockDim.x)
        if (status[q] & 1u) { const int at = atomicAdd(&count, 1); if (at < cap) map[at] = (int32_t)q; }
    __syncthreads();
    if (threadIdx.x == 0) map[cap] = count;
}

namespace hnsw_host {

thread_local std::string g_last_error;

// Host ranges obtained through hnsw_host_alloc / hnsw_host_register, with the device address the runtime gave them.  The
// host-buffer entry points access a caller's matrix directly from the device (zero-copy) only when it lies inside one of
// THESE ranges: what the runtime's pointer queries say about memory somebody else pinned (or pinned once and freed) is not
// trusted with a kernel's loads and stores.
//
// A range also remembers who may still be READING it: an entry point that returns before the device is done with the
// caller's matrix (hnsw_search_batch_h2d: the kernels read it in place; hnsw_search_submit: the upload is a DMA out of it)
// leaves an event behind its last reader on that stream (range_reader_enqueued).  hnsw_host_unregister / hnsw_host_free wait
// for those events before the pages are unpinned or freed: unregistering early is slow, never a GPU page fault (round 4's
// second suite abort was exactly that: DESIGN.md section 7).
struct InFlight { hipStream_t st; hipEvent_t ev; };
enum { RANGE_ALLOCATED = 0, RANGE_REGISTERED = 1, RANGE_FOREIGN = 2 };   // hipHostMalloc / hipHostRegister by this library / pinned by somebody else
struct HostRange { const char *p; size_t bytes; char *dev; int kind; std::vector<InFlight> readers; };
std::mutex g_ranges_mu;
std::vector<HostRange> g_ranges;

// the device address of [p, p + bytes) if it lies in one of these ranges, else null (as for a null p)
void *registered_device_address(const void *p, size_t bytes) {
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(g_ranges_mu);
    for (const HostRange &r : g_ranges)
        if (r.dev && (const char *)p >= r.p && (const char *)p + bytes <= r.p + r.bytes) return r.dev + ((const char *)p - r.p);
    return nullptr;
}

// `st` (of the current device) has just been given work that reads [p, p + bytes) after the entry point returns
void range_reader_enqueued(const void *p, size_t bytes, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_ranges_mu);
    for (HostRange &r : g_ranges) {
        if (!((const char *)p >= r.p && (const char *)p + bytes <= r.p + r.bytes)) continue;
        // Whatever goes wrong with the event, the guarantee stands: without an event behind the reader the stream is drained
        // HERE, before the entry point returns (slow, never a page unpinned under a running kernel).
        for (InFlight &f : r.readers)
            if (f.st == st) {      // work on one stream is ordered: the later record covers the earlier reader
                if (hipEventRecord(f.ev, st) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(st); }
                return;
            }
        InFlight f{st, nullptr};
        if (hipEventCreateWithFlags(&f.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(st); return; }
        if (hipEventRecord(f.ev, st) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(f.ev); (void)hipStreamSynchronize(st); return; }
        r.readers.push_back(f);
        return;
    }
}

void remember_range(const void *p, size_t bytes, void *dev, int kind) {
    std::lock_guard<std::mutex> lk(g_ranges_mu);
    g_ranges.push_back({(const char *)p, bytes, (char *)dev, kind, {}});
}
// takes the range that STARTS at p off the list (no launch can pick it for direct access any more) and waits for the
// readers that earlier asynchronous calls left on it; false: no such range
bool retire_range(const void *p, int *kind) {
    std::vector<InFlight> readers;
    {
        std::lock_guard<std::mutex> lk(g_ranges_mu);
        size_t i = 0;
        while (i < g_ranges.size() && g_ranges[i].p != (const char *)p) ++i;
        if (i == g_ranges.size()) return false;
        *kind = g_ranges[i].kind;
        readers.swap(g_ranges[i].readers);
        g_ranges.erase(g_ranges.begin() + (long)i);
    }
    for (InFlight &f : readers) {
        if (hipEventSynchronize(f.ev) != hipSuccess) (void)hipGetLastError();
        (void)hipEventDestroy(f.ev);
    }
    return true;
}

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int upload_rows(const float *vectors, int64_t n, int d, int64_t row_stride, float *dst) {
    const int64_t stride = padded_stride(d);
    if (n == 0) return HNSW_OK;
    if (stride == row_stride) {
        if (hipMemcpy(dst, vectors, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return fail(HNSW_ERR_HIP, "vector upload failed");
        return HNSW_OK;
    }
    const int64_t chunk_rows = std::max<int64_t>(1, (64ll << 20) / (stride * 4));
    std::vector<float> stage((size_t)std::min(chunk_rows, n) * stride);
    for (int64_t r0 = 0; r0 < n; r0 += chunk_rows) {
        const int64_t nr = std::min(chunk_rows, n - r0);
        std::fill(stage.begin(), stage.begin() + (size_t)nr * stride, 0.0f);
        for (int64_t i = 0; i < nr; ++i)
            memcpy(&stage[(size_t)i * stride], vectors + (r0 + i) * row_stride, sizeof(float) * (size_t)d);
        if (hipMemcpy(dst + r0 * stride, stage.data(), (size_t)nr * stride * 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail(HNSW_ERR_HIP, "vector upload failed");
    }
    return HNSW_OK;
}

int alloc_graph_tables(IndexTables &t, int64_t n, int64_t stride, int S0, int SU, int64_t rowsU) {
    const size_t n1 = (size_t)std::max<int64_t>(n, 1), nbr0_bytes = (size_t)n * S0 * 4, nbrU_bytes = (size_t)std::max<int64_t>(rowsU, 1) * SU * 4;
    HIP_TRY(t.X.alloc(n1 * stride * sizeof(float)));
    HIP_TRY(t.nbr0.alloc(nbr0_bytes));
    HIP_TRY(hipMemset(t.nbr0.p, 0xFF, nbr0_bytes));
    HIP_TRY(t.nbrU.alloc(nbrU_bytes));
    HIP_TRY(hipMemset(t.nbrU.p, 0xFF, nbrU_bytes));
    HIP_TRY(t.off.alloc(n1 * 4));
    HIP_TRY(t.lvl.alloc(n1));
    HIP_TRY(t.ref.alloc(n1 * sizeof(int2)));
    return HNSW_OK;
}

int64_t upper_layout(const uint8_t *lvl, int64_t m, int64_t row0, std::vector<int2> &ref) {
    ref.resize((size_t)m);
    int64_t rows = row0;
    for (int64_t j = 0; j < m; ++j) {
        ref[(size_t)j] = make_int2(lvl[j] ? (int32_t)rows : -1, (int)lvl[j]);
        rows += lvl[j];
    }
    return rows;
}

int upload_upper_layout(IndexTables &t, int64_t n0, const std::vector<int2> &ref) {
    const size_t m = ref.size();
    std::vector<int32_t> off(m);
    std::vector<uint8_t> lvl(m);
    for (size_t j = 0; j < m; ++j) { off[j] = ref[j].x; lvl[j] = (uint8_t)ref[j].y; }
    HIP_TRY(hipMemcpy((int32_t *)t.off.p + n0, off.data(), m * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((uint8_t *)t.lvl.p + n0, lvl.data(), m, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((int2 *)t.ref.p + n0, ref.data(), m * sizeof(int2), hipMemcpyHostToDevice));
    return HNSW_OK;
}


// ---- kernel dispatch ---------------------------------------------------------------------------
// the knn kernel's variants live in hnsw_search_variants.hip, one object per (metric, accept rule, row shape)
#define HNSW_V_DECLARE(m, s, f)                                                                                             \
    hipError_t search_launch_##m##_##s##_##f(int nch, int nslot, const IndexView &iv, const SearchArgs &a, hipStream_t st); \
    int search_occupancy_##m##_##s##_##f(int nch, int nslot, size_t lds, int blk);
#define HNSW_V_ENTRY(m, s, f) {m, s, f, search_launch_##m##_##s##_##f, search_occupancy_##m##_##s##_##f},
HNSW_SEARCH_VARIANTS(HNSW_V_DECLARE)
typedef hipError_t (*search_launch_fn)(int, int, const IndexView &, const SearchArgs &, hipStream_t);
typedef int (*search_occupancy_fn)(int, int, size_t, int);
const struct { int metric, semf, rows; search_launch_fn launch; search_occupancy_fn occupancy; } k_variants[] = {HNSW_SEARCH_VARIANTS(HNSW_V_ENTRY)};
#undef HNSW_V_DECLARE
#undef HNSW_V_ENTRY
// ... and the collect kernel's (option "filter_collect") in hnsw_collect_variants.hip, by the same triples
#define HNSW_C_DECLARE(m, s, f) \
    hipError_t collect_launch_##m##_##s##_##f(int nch, int nslot, const IndexView &iv, const SearchArgs &a, const hnsw_dev::CollectArgs &c, hipStream_t st);
#define HNSW_C_ENTRY(m, s, f) {m, s, f, collect_launch_##m##_##s##_##f},
HNSW_COLLECT_VARIANTS(HNSW_C_DECLARE)
typedef hipError_t (*collect_launch_fn)(int, int, const IndexView &, const SearchArgs &, const hnsw_dev::CollectArgs &, hipStream_t);
const struct { int metric, semf, rows; collect_launch_fn launch; } k_collect_variants[] = {HNSW_COLLECT_VARIANTS(HNSW_C_ENTRY)};
#undef HNSW_C_DECLARE
#undef HNSW_C_ENTRY

// the knn kernel's row format: 2 = byte rows (hnsw_rows8.hip) and the sq8 codes (hnsw_rows_sq8.hip: the same kernels), 3 = split
// fp32 rows (hnsw_rows_split.hip), 4 = half rows (hnsw_rows16.hip), else plain fp32 rows, 1 = every chunk of the lane grid inside
// the row.  (From the record bind_view keeps: byte, sq8 and half rows share IndexView's pointer.)  5 = the per-dimension sq8 codes
// under L2 (hnsw_rows_sq8_dim.hip: a weighted distance; under the inner product they are byte rows to the kernel, 2).  6 = the
// 1-bit codes (hnsw_rows_bits.hip), under every metric.
inline int variant_full(const hnsw_index *idx) {
    switch (idx->info.row_format) {
    case HNSW_ROWS_BYTES: case HNSW_ROWS_SQ8: return 2;
    case HNSW_ROWS_SQ8_DIM: return idx->info.metric == HNSW_METRIC_L2 ? 5 : 2;
    case HNSW_ROWS_BITS: return 6;
    case HNSW_ROWS_SPLIT: return 3;
    case HNSW_ROWS_HALF: return 4;
    default: return idx->iv.nchunks == 16 * pick_nch(idx->iv.nchunks) ? 1 : 0;
    }
}

// The knn kernel a search of (ef, accept rule) on this handle runs: its place on the (NCH, NSLOT) grid, its row of the handle's
// per-shape decisions (hnsw_index::shape) and the variant object's entry points.  Resolved once per call by the entry points and
// handed down.
struct KnnShape {
    int ef, semf, nch, nslot, slot_class;
    search_launch_fn launch;
    search_occupancy_fn occupancy;
    collect_launch_fn collect;           // the collect kernel of the same shape; null: the row format has none (half, sq8)
    // waves of the kernel (blk: of its bitmap-block twin) one CU holds when each asks for `lds` bytes, 0 = unknown
    int waves_per_cu(size_t lds, bool blk = false) const { return occupancy(nch, nslot, lds, blk); }
    hnsw_index::ShapeChoice &choice(hnsw_index *idx) const { return idx->shape[slot_class][semf]; }
};
KnnShape knn_shape(const hnsw_index *idx, int ef, int semantics) {
    KnnShape sh{};
    sh.ef = ef; sh.semf = semantics ? 1 : 0;
    const int metric = idx->info.metric == HNSW_METRIC_L2 ? 0 : 1, rows = variant_full(idx);
    // (bit rows: the kernel's NCH is NW, the 16-word steps of a row, not the float32 row's chunks per lane)
    sh.nch = rows == 6 ? bit_words(idx->iv.d) : pick_nch(idx->iv.nchunks);
    sh.nslot = pick_nslot_knn(ef, sh.nch); sh.slot_class = slot_class(sh.nslot);
    for (const auto &v : k_variants)
        if (v.metric == metric && v.semf == sh.semf && v.rows == rows) { sh.launch = v.launch; sh.occupancy = v.occupancy; }
    for (const auto &v : k_collect_variants)
        if (v.metric == metric && v.semf == sh.semf && v.rows == rows) sh.collect = v.launch;
    if (rows == 5) {                     // hnsw_sq8_dim_walk.hip: one object per accept rule, L2 only
        sh.launch = sh.semf ? search_launch_sq8_dim_1 : search_launch_sq8_dim_0;
        sh.occupancy = sh.semf ? search_occupancy_sq8_dim_1 : search_occupancy_sq8_dim_0;
    }
    if (rows == 6) {                     // hnsw_bits_walk.hip: one object per accept rule, the one Hamming walk under every metric
        sh.launch = sh.semf ? search_launch_bits_1 : search_launch_bits_0;
        sh.occupancy = sh.semf ? search_occupancy_bits_1 : search_occupancy_bits_0;
        if (walks_bit_planes(idx)) {     // option bit_query_bits 4: hnsw_bits_asym_walk.hip, the kernel's ROWS 7 over the same rows and shapes
            sh.launch = sh.semf ? search_launch_bits_asym_1 : search_launch_bits_asym_0;
            sh.occupancy = sh.semf ? search_occupancy_bits_asym_1 : search_occupancy_bits_asym_0;
        }
    }
    return sh;
}

hipError_t launch_distance(const hnsw_index *idx, const float *Q, int64_t qs, int64_t nq, const int32_t *ids, int32_t m, float *out, hipStream_t st) {
    // blockIdx.y strides over a query's ids: enough blocks to fill the chip twice over (8 192 waves: what it holds at four waves
    // per SIMD, twice), no more -- every block starts by loading its query, and a block that then evaluates thirty-two batches
    // amortises that better than one that evaluates four (bench_dist's shape, profiles/r06_dist_ab.txt: 6.07 / 5.77 TB/s at 8 192
    // waves on two boxes, 5.85 / 5.76 at 65 536 -- rounds 1-5's grid: within the noise of one box)
    constexpr int64_t DIST_WAVES = 8192;
    const int64_t per_query = std::max<int64_t>(1, (DIST_WAVES + std::max<int64_t>(nq, 1) - 1) / std::max<int64_t>(nq, 1));
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(256, (m + 15) / 16), per_query));
    dim3 grid((unsigned)nq, gy), block(64);
    with_metric(idx->info.metric, [&](auto METRIC) {
        with_nch(pick_nch(idx->iv.nchunks), [&](auto NCH) {
            hipLaunchKernelGGL((hnsw_dev::hnsw_distance_kernel<NCH, METRIC>), grid, block, 0, st, idx->iv, Q, qs, nq, ids, m, out);
        });
    });
    return hipGetLastError();
}

// log2 entries of the knn kernel's visited cache: search_vt_bits' choice, then grown for free.  A kernel variant whose
// REGISTERS cap it at few waves per CU (C3's split-row kernel: 106 VGPRs, 16 waves) leaves LDS unused; a larger cache then
// costs no residency and saves re-evaluations, which on clustered data are many (1.18 M x 100 unit vectors around 256
// directions, M 32, ef 256: 8239 evaluations per query with 2^11 tags against 5015 in the oracle, 6592 with 2^12: 5.22 ->
// 4.36 ms per 10 k batch; 2^13 would halve the residency: 5.17 ms).  So: the largest cache (up to 2^14 tags) that keeps the
// waves per CU the variant reaches with the base size.  Never changes results; "vt_bits" still overrides.
int knn_vt_bits(hnsw_index *idx, const KnnShape &sh) {
    const int base = search_vt_bits(idx, sh.ef);
    if (idx->vt_bits_override) return base;
    int &grown = sh.choice(idx).vt_bits;      // (a slot class lies on one side of search_vt_bits' ef boundary: one base per entry)
    if (grown) return grown;
    const int occ0 = sh.waves_per_cu(hnsw_dev::wave_lds_words(base) * sizeof(uint32_t));
    int b = base;
    while (occ0 > 0 && b < 14 && sh.waves_per_cu(hnsw_dev::wave_lds_words(b + 1) * sizeof(uint32_t)) >= occ0) ++b;
    return grown = b;
}

// collect: the collect kernel of the shape instead (a shape without one is an error, never the plain kernel)
int launch_search_args(hnsw_index *idx, const KnnShape &sh, const SearchArgs &a, hipStream_t st, const hnsw_dev::CollectArgs *collect = nullptr) {
    if (collect && (!sh.collect || a.k > 128))
        return fail(HNSW_ERR_UNSUPPORTED, "no collect kernel for row format %d, k=%d", idx->info.row_format, a.k);
    hipError_t e = collect ? sh.collect(sh.nch, sh.nslot, idx->iv, a, *collect, st) : sh.launch(sh.nch, sh.nslot, idx->iv, a, st);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "search kernel launch failed: %s", hipGetErrorString(e));
    return HNSW_OK;
}

// the SearchArgs of a plain launch over the batch: every query in its row, nothing ordered, no global slab.  The caller passes
// the visited structure's sizes (knn_vt_bits, knn_blk_bits) because knn_blk_bits' own measurement launches through here.
SearchArgs knn_args(const hnsw_search_params &p, const KnnBatch &b, int vt_bits, int blk_bits) {
    SearchArgs a{};
    a.Q = b.Q; a.q_stride = b.q_stride; a.nq = b.nq; a.ef = p.ef; a.k = p.k; a.fill = p.fill; a.sem = p.semantics;
    a.vt_bits = vt_bits; a.blk_bits = blk_bits;
    a.out_ids = b.ids; a.out_dist = b.dist; a.out_ndist = b.nd; a.out_nhops = b.nh; a.out_status = b.st;
    a.any_flag = b.any_flag;
    a.prio_tail = 0x7FFFFFFF;
    return a;
}

// Visited as bitmap blocks over the locality codes (visited_blocks_mem_add; hnsw_locality.hip) for the kernels with W in four
// or more registers (ef > 128: the walks that visit several times what the tag cache holds): log2 of the block slots, or 0 =
// the tag cache.  The slots are as many as fit the LDS of the waves per CU the variant reaches with the tag cache (C5's and
// C3's kernels, 16 waves per CU: 2^8 blocks = 65 536 codes).
// Which of the two forgets less depends on the DATA -- on clustered vectors the blocks end C5's shape's 40 % repeated
// evaluations (1-4 % left); on structureless vectors no numbering has locality, a block holds one visited node and the tag
// cache wins -- so unless the caller decides (option "visited_blocks" 0 / 1), the handle MEASURES, once
// per kernel shape: 256 of the index's own vectors are searched both ways and the evaluations counted; the blocks are taken
// when they save at least 5 %.  The measurement (and building the codes: one descent per node per upper layer, a sort) runs
// inside the first search call that needs the answer and synchronises the device; indices of fewer than 200 000 nodes are
// not measured (a walk cannot visit much more than the tag cache holds).  Never changes results.
// The per-slot code table (n * max_degree0 * 4 bytes: 2.56 GB for 10 M nodes at M 32) is only worth its memory while some kernel
// shape of the handle runs the bitmap blocks.  After a measurement that chose the tag cache -- structureless data -- it is freed
// again unless another shape took the blocks; the per-node codes (n * 4 bytes) stay, so a later measurement for another shape
// re-makes the table with one fill kernel instead of the whole build.  Only called with the device idle (the measurement
// synchronises; nothing in flight reads the table when no shape has chosen it).
void release_unused_lcode0(hnsw_index *idx) {
    if (!idx->tables.lcode0.p) return;
    if (idx->blk_mode == 1) return;                  // the caller asked for blocks wherever they can run: keep the table
    for (auto &c : idx->shape) if (c[0].blk > 0 || c[1].blk > 0) return;
    drop_lcode0(idx);
}

// the largest block directory (log2 slots) that keeps the waves per CU of this shape's kernel, 0 = the shape cannot run the blocks
int blk_capacity_bits(hnsw_index *idx, const KnnShape &sh) {
    if (sh.nslot < 3) return 0;
    const int vt = knn_vt_bits(idx, sh);
    // (the waves per CU of the tag-cache kernel, or of the block kernel at its smallest directory if its registers allow fewer)
    const int occ0 = std::min(sh.waves_per_cu(hnsw_dev::wave_lds_words(vt) * sizeof(uint32_t)),
                              sh.waves_per_cu(hnsw_dev::search_lds_words(vt, 6) * sizeof(uint32_t), true));
    int bits = 0;
    for (int b = 6; b <= 10; ++b)
        if (hnsw_dev::wave_lds_words_blocks(b) * sizeof(uint32_t) <= 65536 && occ0 > 0 &&
            sh.waves_per_cu(hnsw_dev::search_lds_words(vt, b) * sizeof(uint32_t), true) >= occ0) bits = b;
    if (bits == 0) return 0;
    {   // HNSW_BLK_BITS (tests): a smaller directory than fits, down to one set of eight slots -- evictions and contested slots on small graphs
        const int forced = env_int("HNSW_BLK_BITS", 0);
        if (forced >= 3) bits = std::min(bits, forced);
    }
    return bits;
}

// do the knn searches gather byte rows (the byte rows, or codes -- the per-dimension codes' L2 kernel loads what the byte-row
// kernels load, and is treated as they are; the bit rows are smaller still and bound by a hop's latency all the more)?  Not "one
// byte per dimension": hnsw_index_row_bytes asks the format.
inline bool walks_bytes(const hnsw_index *idx) { return idx->info.row_format == HNSW_ROWS_BYTES || walks_codes(idx); }

// does option "visited_blocks" at -1 consider this shape at all?
bool blk_auto_eligible(const hnsw_index *idx, int nslot) {
    if (idx->iv.n < 200000) return false;
    // Left to itself the handle only considers the FLOAT32 shapes whose hand-scheduled loop has the block filter (rows of 65..256
    // dimensions -- full, ragged or split --, W in three to eight registers: C3's and C5's kernels): those kernels are bound by
    // row requests, so fewer evaluations are less time.  The byte-row loops have the filter too (an explicit "visited_blocks" 1
    // runs it, and the C++ loop of every other shape), but a byte-row kernel is bound by the LATENCY of a hop, and the filter's
    // four dependent LDS round trips and ~90 vector instructions cost a hop more than the evaluations it saves: the harder
    // SIFT-like set at ef 192, 8 % fewer evaluations, 0.98 -> 1.10 ms per 10 k batch (profiles/r05_ab_bytes_blocks.txt).
    // (The sq8 codes run the byte-row kernels.)
    return !walks_bytes(idx) && idx->iv.nchunks > 16 && idx->iv.nchunks <= 64 && nslot <= 8;
}

int knn_blk_bits(hnsw_index *idx, const KnnShape &sh) {
    const int ef = sh.ef, semf = sh.semf, nslot = sh.nslot;
    const int mode = idx->blk_mode;
    if (mode == 0 || nslot < 3 || idx->lcode_state < 0) return 0;
    if (mode < 0 && !blk_auto_eligible(idx, nslot)) return 0;
    int &choice = sh.choice(idx).blk;
    if (choice >= 0) return choice;
    const int bits = blk_capacity_bits(idx, sh), vt = knn_vt_bits(idx, sh);
    if (bits == 0) return choice = 0;
    if (build_locality_codes(idx) != HNSW_OK || idx->lcode_state != 1 || !idx->tables.lcode0.p) return choice = 0;
    if (mode == 1) return choice = bits;
    // measure: 256 probe queries -- the midpoint between every (n / 256)-th vector of the index and its first layer-0 neighbour:
    // where queries of the data's own distribution fall, without being stored vectors themselves (a stored vector finds itself
    // at distance 0 and its walk is shorter than a real query's) -- searched both ways, k = 1, evaluations counted
    const int64_t nq = std::min<int64_t>(256, idx->iv.n), step = idx->iv.n / nq;
    DevBuf out, probes;
    if (out.ensure((size_t)nq * 16) != HNSW_OK || probes.ensure((size_t)nq * idx->iv.stride * 4) != HNSW_OK) return choice = 0;
    hipLaunchKernelGGL(probe_queries_kernel, dim3((unsigned)nq), dim3(64), 0, nullptr, idx->iv, step, (float *)probes.p);
    uint64_t sum[2] = {0, 0};
    bool ok = hipGetLastError() == hipSuccess;
    // (sq8 rows: the probes are midpoints of float32 vectors and the walk reads code space -- moved there in place.  Not reached
    // today: blk_auto_eligible leaves the byte-row kernels, sq8's among them, out of the measurement, and "visited_blocks" 1
    // returns above.  Kept so that measuring them one day does not search float32 probes in code space.  The bit rows refuse a
    // transform in place -- their query rows have a stride of their own, walk_query_stride -- and so answer "tags" here.)
    if (ok && walks_codes(idx))
        ok = codes_transform_queries(idx, (const float *)probes.p, nq, idx->iv.stride, (float *)probes.p, nullptr, nullptr) == HNSW_OK;
    hnsw_search_params p{};
    p.ef = ef; p.k = 1; p.fill = HNSW_FILL_OHNSW; p.semantics = semf;
    const KnnBatch b{(const float *)probes.p, nq, idx->iv.stride, (int32_t *)out.p, (float *)out.p + nq, (uint32_t *)out.p + 2 * nq,
                     (uint32_t *)out.p + 3 * nq, nullptr, nullptr};
    for (int pass = 0; pass < 2 && ok; ++pass) {
        SearchArgs a = knn_args(p, b, vt, pass ? bits : 0);
        std::vector<uint32_t> nd((size_t)nq);
        ok = launch_search_args(idx, sh, a, nullptr) == HNSW_OK && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(nd.data(), b.nd, (size_t)nq * 4, hipMemcpyDeviceToHost) == hipSuccess;
        for (uint32_t v : nd) sum[pass] += v;
    }
    if (!ok) { (void)hipGetLastError(); choice = 0; release_unused_lcode0(idx); return 0; }
    choice = (double)sum[1] <= 0.95 * (double)sum[0] ? bits : 0;
    release_unused_lcode0(idx);     // the tags won and no other shape uses the blocks: the per-slot table (GBs at 10 M nodes) goes again
    if (env_int("HNSW_DEBUG_VISITED", 0))
        fprintf(stderr, "hnsw: visited set for ef %d (W in %d registers, rule %d): tag cache %.0f evaluations per probe query, 2^%d blocks %.0f -> %s\n",
                ef, nslot, semf, (double)sum[0] / (double)nq, bits, (double)sum[1] / (double)nq, choice ? "blocks" : "tags");
    return choice;
}
// LDS bytes of one search wave of this shape (no padding)
size_t knn_lds_bytes(hnsw_index *idx, const KnnShape &sh) {
    return hnsw_dev::search_lds_words(knn_vt_bits(idx, sh), knn_blk_bits(idx, sh)) * sizeof(uint32_t);
}

// how many one-wave workgroups of this shape's kernel are resident at once (no LDS padding): on the device (1 << 40 when that is
// unknown: never reorder) and on one CU (0 when unknown)
struct Residency { int64_t queries; int per_cu; };
Residency resident_queries(hnsw_index *idx, const KnnShape &sh) {
    // the answer depends on the kernel's registers and LDS: asked once per shape (hnsw_index::shape)
    const size_t lds = knn_lds_bytes(idx, sh);
    if (idx->cus <= 0 && hipDeviceGetAttribute(&idx->cus, hipDeviceAttributeMultiprocessorCount, idx->device) != hipSuccess) { (void)hipGetLastError(); idx->cus = 0; }
    hnsw_index::ShapeChoice &c = sh.choice(idx);
    if (c.per_cu < 0 || c.lds != lds) { c.per_cu = std::max(0, sh.waves_per_cu(lds, knn_blk_bits(idx, sh) > 0)); c.lds = lds; }
    if (c.per_cu > 0 && idx->cus > 0) return {(int64_t)c.per_cu * idx->cus, c.per_cu};
    return {(int64_t)1 << 40, 0};
}

// LDS bytes to request beyond what a search wave uses, for a launch of nq > resident queries (longest first).
// With one workgroup per query the chip holds `resident` of them and the launch is ceil(nq / resident) passes of
// which the last is part empty: on C2 (10 000 queries, 7168 resident) 4336 waves run one query and stop while 2832
// run two, and the second half of the launch has under half the chip's memory requests in flight.  Holding
// nq / passes queries at a time instead gives every slot the same share of the walk and the launch ends together
// (C2: 0.78 -> 0.74 ms per call).  The only per-launch handle on residency is the LDS a workgroup asks for:
// gfx950 hands LDS out in 1280-byte granules, 128 per CU, so k granules per wave hold floor(128 / k) waves.
// Chosen: the fewest waves per CU that still cover nq / passes.
int balanced_lds_pad(hnsw_index *idx, const KnnShape &sh, int64_t nq) {
    const int64_t base = (int64_t)knn_lds_bytes(idx, sh);
    if (idx->lds_pad >= 0)       // option "lds_pad": clamped to what a workgroup may ask for beside its own scratch
        return (int)std::max<int64_t>(0, std::min<int64_t>(std::min(idx->lds_pad, 32768), 65536 - base));
    const Residency res = resident_queries(idx, sh);
    const int64_t resident = res.queries;
    if (nq <= resident || res.per_cu <= 0) return 0;
    // byte rows: a quarter of the bytes per evaluation, the launch is bound by the latency of a hop, not by the
    // memory system, and holds as many queries as the registers allow (C2: 0.60 ms per call at 8192 held, 0.65 at 5376)
    if (walks_bytes(idx)) return 0;
    constexpr int64_t GRANULE = 1280, GRANULES_PER_CU = 128;
    const int64_t passes = (nq + resident - 1) / resident;
    const int64_t want_per_cu = (nq + passes * idx->cus - 1) / (passes * idx->cus);
    const int64_t k0 = (base + GRANULE - 1) / GRANULE;
    int64_t best = k0;
    for (int64_t k = k0; k * GRANULE <= 65536; ++k) {         // a workgroup may ask for 64 KiB at most
        const int64_t w = std::min<int64_t>(res.per_cu, GRANULES_PER_CU / k);
        if (w < want_per_cu) break;
        best = k;
    }
    int64_t pad = best > k0 ? best * GRANULE - base : 0;
    // The granule arithmetic above is gfx950's (1280-byte granules, 128 per CU: profiles/r02_residency_sweep.txt).  The
    // runtime has the last word: the padded request must still hold the wanted waves per CU by ITS count, and fit the
    // largest dynamic LDS a workgroup may ask for; otherwise the padding is stepped back.
    if (pad > 0) {
        int max_lds = 0;
        if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, idx->device) != hipSuccess) { (void)hipGetLastError(); max_lds = 65536; }
        const bool blk = knn_blk_bits(idx, sh) > 0;
        while (pad > 0 && (base + pad > max_lds || sh.waves_per_cu((size_t)(base + pad), blk) < want_per_cu)) pad = pad > GRANULE ? pad - GRANULE : 0;
    }
    return (int)pad;
}

// Issue priorities of an ordered launch (SearchArgs::prio_head / prio_tail; the kernel's comment says why): the first
// eighth of the blocks that start at once (the walks predicted longest) and, when the launch is one full pass and a
// partial second one, the blocks that have to wait for a slot.  HNSW_PRIO="head,tail" overrides the bounds (tuning).
void launch_priorities(hnsw_index *idx, const KnnShape &sh, int64_t nq, SearchArgs &a) {
    a.prio_head = 0; a.prio_tail = 0x7FFFFFFF;
    if (const char *e = getenv("HNSW_PRIO")) {
        int h = 0, t = 0x7FFFFFFF;
        if (sscanf(e, "%d,%d", &h, &t) >= 1) { a.prio_head = h; a.prio_tail = t; }
        return;
    }
    const Residency res = resident_queries(idx, sh);
    const int64_t resident = res.queries;
    if (res.per_cu <= 0) return;
    a.prio_head = (int32_t)(std::min(nq, resident) / 8);
    if (nq > resident && nq < 2 * resident) a.prio_tail = (int32_t)resident;
}

// Option "refine": how many members of W a search of (ef, k) re-ranks over the float32 rows, 0 = none -- the option is off, or the
// searches read rows whose distances are exact over X already (bytes, split, float32).  Over sq8 rows the walk's distances are
// those of code space, which mean nothing to a caller: such a search is ALWAYS re-ranked, refine 0 takes the k first of W.
int refine_count(const hnsw_index *idx, const hnsw_search_params *p) {
    const int format = idx->info.row_format;
    if (!walks_codes(idx) && (idx->refine == 0 || format != HNSW_ROWS_HALF)) return 0;
    return idx->refine < 0 ? p->ef : std::min(p->ef, std::max(p->k, idx->refine));
}
// The queries a walk over codes reads: b's moved to the codes' space in walk.qt (made here when `transform` -- sq8 rows: Q' =
// (Q - lo) / scale for L2, Q for the inner product; per-dimension sq8 rows: Q - lo for L2, s o Q for the inner product; stage: see
// sq8_transform_queries; bit rows: the query's bits, or its four bit planes under option bit_query_bits), at the stride
// walk_query_stride names -- the padded stride, or the plane rows' own.  Every launch that walks the codes -- the
// ordering pre-pass, the search, the device fallback, knn_repair's re-run -- goes through here; the re-rank keeps the caller's.
int sq8_walk_queries(hnsw_index *idx, RefineBufs &walk, KnnBatch *wb, bool transform, float *stage, hipStream_t st) {
    const int64_t stride = walk_query_stride(idx);
    if (transform) {
        int rc;
        if ((rc = walk.qt.ensure((size_t)wb->nq * stride * sizeof(float))) ||
            (rc = codes_transform_queries(idx, wb->Q, wb->nq, wb->q_stride, (float *)walk.qt.p, stage, st))) return rc;
    }
    wb->Q = (const float *)walk.qt.p; wb->q_stride = stride;
    return HNSW_OK;
}
// ... the walk of such a search: b with k := c, its results and evaluation counts in `walk`
int refine_walk(const KnnBatch &b, int c, RefineBufs &walk, KnnBatch *wb) {
    const int rc = walk.ensure(b.nq, c);
    if (rc) return rc;
    *wb = b;
    wb->ids = (int32_t *)walk.ids.p; wb->dist = (float *)walk.dist.p;
    if (b.nd) wb->nd = (uint32_t *)walk.nd.p;
    return HNSW_OK;
}
// ... and its second half: the c candidates per query re-ranked into b's [nq][k] arrays, b.nd = the walk's count + the candidates
int refine_rerank(hnsw_index *idx, const hnsw_search_params &p, const KnnBatch &b, const KnnBatch &wb, int c, hipStream_t st) {
    return launch_rerank(idx, b.Q, b.nq, b.q_stride, wb.ids, c, p.k, p.fill, b.ids, b.dist, b.nd ? wb.nd : nullptr, b.nd, st);
}

int check_params(const hnsw_index *idx, const hnsw_search_params *p) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (!p) return fail(HNSW_ERR_BAD_ARG, "null params");
    if (p->ef < 1 || p->k < 1) return fail(HNSW_ERR_BAD_ARG, "ef and k must be >= 1 (ef=%d k=%d)", p->ef, p->k);
    if (p->k > p->ef)
        return fail(HNSW_ERR_BAD_ARG, "k=%d > ef=%d: the reference silently misbehaves here "
                    "(lib/hnsw_algo.ml:257-258); rejected", p->k, p->ef);
    if (p->ef > 1024) return fail(HNSW_ERR_UNSUPPORTED, "ef=%d > 1024 not supported", p->ef);
    if (p->fill != HNSW_FILL_OHNSW && p->fill != HNSW_FILL_BA) return fail(HNSW_ERR_BAD_ARG, "bad fill %d", p->fill);
    if (p->semantics != HNSW_SEM_OHNSW && p->semantics != HNSW_SEM_FUNCTOR && p->semantics != HNSW_SEM_FUNCTOR_NEAREST_K)
        return fail(HNSW_ERR_BAD_ARG, "bad semantics %d", p->semantics);
    if (p->semantics == HNSW_SEM_FUNCTOR_NEAREST_K && refine_count(idx, p) > 0)
        return fail(HNSW_ERR_BAD_ARG, "option %s is active: the k farthest of W (HNSW_SEM_FUNCTOR_NEAREST_K) have no refined meaning",
                    walks_codes(idx) ? codes_option(idx) : "refine");
    if (idx->iv.entry_point < 0) return fail(HNSW_ERR_EMPTY_INDEX, "knn: empty hgraph");
    return HNSW_OK;
}

// the checks of the batch entry points, in this order: the params and the handle, 0 <= nq <= INT32_MAX, then -- unless nq is
// 0, which passes -- the buffers (`buffers`: none of the required ones is null) and q_stride >= d
int check_batch(const hnsw_index *idx, const hnsw_search_params *p, int64_t nq, int64_t q_stride, bool buffers) {
    int rc = check_params(idx, p);
    if (rc) return rc;
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    if (nq == 0) return HNSW_OK;
    if (!buffers) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    if (q_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "q_stride < d");
    return HNSW_OK;
}

// The exactness fallback's launch: the `c` flagged queries listed in qmap are searched again, each with `cap` slots of `slab`
// for its tie list; their results, counters and status words overwrite their rows of the batch.  Its arguments are the plain
// launch's and nothing of an ordered one: the pre-pass's entries and key, the LDS padding and the priorities describe the order
// of all nq queries in the first launch, not of this list.
int launch_rerun(hnsw_index *idx, const hnsw_search_params &p, const KnnBatch &b, const int32_t *qmap, int64_t c, uint32_t *slab,
                 int32_t cap, hipStream_t st, const hnsw_dev::CollectArgs *collect = nullptr) {
    const KnnShape sh = knn_shape(idx, p.ef, p.semantics);
    SearchArgs a = knn_args(p, b, knn_vt_bits(idx, sh), knn_blk_bits(idx, sh));
    a.nq = c; a.qmap = qmap; a.q_limit = b.nq; a.ovf_g = slab; a.ovf_gcap = cap;
    a.any_flag = nullptr;                   // (the host has read the word already; a re-run query cannot overflow)
    return launch_search_args(idx, sh, a, st, collect);
}

int knn_search(hnsw_index *idx, const hnsw_search_params *caller_params, const KnnBatch &caller_b, hipStream_t st, float *d_stage,
               RefineBufs *walk, bool raw_walk, const hnsw_dev::CollectArgs *collect) {
    int rc = check_batch(idx, caller_params, caller_b.nq, caller_b.q_stride, caller_b.Q && caller_b.ids && caller_b.dist);
    if (rc || caller_b.nq == 0) return rc;
    if (collect && !raw_walk) return fail(HNSW_ERR_BAD_ARG, "a collect walk is a raw walk");
    HIP_TRY(hipSetDevice(idx->device));
    // refine active: everything below is today's search with k := c into the walk's scratch; the re-rank at the end answers the caller
    const int refine_c = raw_walk ? 0 : refine_count(idx, caller_params);
    hnsw_search_params walk_params = *caller_params;
    KnnBatch b = caller_b;
    if (refine_c > 0) {
        walk_params.k = refine_c;
        if ((rc = refine_walk(caller_b, refine_c, walk ? *walk : idx->refine_scratch, &b))) return rc;
    }
    const hnsw_search_params *params = &walk_params;
    const KnnShape sh = knn_shape(idx, params->ef, params->semantics);
    // A batch larger than the chip holds at once is searched longest walk first (hnsw_order.hip):
    // per-query results are unchanged, the launch's drain phase is made of short walks.
    void *block = nullptr;
    Event *ev = nullptr;
    if (idx->time_kernels && idx->tev_used + 3 <= 3 * 4096) {
        while (idx->tev.size() < idx->tev_used + 3) {
            Event e;
            HIP_TRY(hipEventCreate(&e.h));
            idx->tev.push_back(std::move(e));
        }
        ev = &idx->tev[idx->tev_used];      // claimed (tev_used advanced) only once all three are recorded
        HIP_TRY(hipEventRecord(ev[0], st));
    }
    const bool sq8 = walks_codes(idx);                            // (then refine_c > 0, unless raw_walk)
    const float *rerank_Q = nullptr;                              // sq8: the caller's queries, which the re-rank reads
    if (sq8) {                                                    // (behind ev[0]: timed with the pre-pass, or with the search when there is none)
        if ((rc = sq8_walk_queries(idx, walk ? *walk : idx->refine_scratch, &b, true, d_stage, st))) return rc;
        rerank_Q = d_stage ? d_stage : caller_b.Q;               // (the transform left a device copy of a host-resident matrix)
        d_stage = nullptr;                                        // Q' is device-resident
    }
    SearchArgs a = knn_args(*params, b, knn_vt_bits(idx, sh), knn_blk_bits(idx, sh));
    const int mode = idx->order_mode;
    // Ordered when more than half of what the chip holds: a batch that fits is faster too with its long walks
    // dispatched first and spread over the CUs (C2, 7168 queries: 0.59 -> 0.45 ms byte rows, 0.68 -> 0.65 ms fp32);
    // below that the pre-pass costs more than it returns.
    if (mode != 0 && (mode == 1 || 2 * b.nq > resident_queries(idx, sh).queries)) {
        rc = order_longest_first(idx, b.Q, b.nq, b.q_stride, d_stage, st, &block, &a.qmap, &a.pre_entry, &a.pre_key, &a.pre_nd, &a.pre_layer);
        if (rc) return rc;
        if (d_stage) a.Q = d_stage;        // the descent kernel left a device-resident copy of the (host-resident) queries
        a.q_limit = b.nq;
        a.lds_pad = balanced_lds_pad(idx, sh, b.nq);
        launch_priorities(idx, sh, b.nq, a);
    }
    if (ev) HIP_TRY(hipEventRecord(ev[1], st));
    rc = launch_search_args(idx, sh, a, st, collect);
    if (!rc && idx->fb_queries > 0 && b.st && !b.any_flag) {
        // opt-in exact mode of the device-pointer entry point (option "device_fallback_slab_bytes"): the queries the launch
        // flagged are listed on the device and searched again with the slab, on the caller's stream, no host round trip.
        // The re-run rewrites their results, counters and status words (bit 0 clear: a slab slot per node cannot overflow);
        // with more flagged queries than the slab holds, the ones left over keep their flag.  Two small launches per call.
        const int32_t cap = (int32_t)idx->fb_queries;
        hipLaunchKernelGGL(flagged_list_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t *)b.st, b.nq, (int32_t *)idx->dFbMap.p, cap);
        if (hipGetLastError() != hipSuccess) return fail(HNSW_ERR_HIP, "flagged-query listing failed");
        KnnBatch read = b;
        read.Q = a.Q;                       // the queries as the search read them (the staged copy when there is one)
        // (at most min(cap, nq) queries can be listed: no more blocks than that; the blocks past the count leave at once)
        rc = launch_rerun(idx, *params, read, (const int32_t *)idx->dFbMap.p, std::min<int64_t>(cap, b.nq), (uint32_t *)idx->dFbSlab.p,
                          (int32_t)std::min<int64_t>(idx->iv.n, 0x7FFFFFFF), st, collect);
    }
    if (!rc && refine_c > 0) {              // (behind the device fallback; reads the queries as the search read them, sq8: the caller's)
        KnnBatch to = caller_b;
        to.Q = sq8 ? rerank_Q : a.Q;
        rc = refine_rerank(idx, *caller_params, to, b, refine_c, st);
    }
    if (ev && !rc) {
        HIP_TRY(hipEventRecord(ev[2], st));
        idx->tev_used += 3;                 // an early return above leaves the triple unclaimed: nothing half-recorded is ever read
        idx->tev_ordered.resize(idx->tev_used / 3);
        idx->tev_ordered[idx->tev_used / 3 - 1] = block != nullptr;
    }
    return rc;
}

int knn_repair(hnsw_index *idx, const hnsw_search_params *p, const KnnBatch &b, hipStream_t st, RefineBufs *walk, bool raw_walk,
               const hnsw_dev::CollectArgs *collect) {
    const int refine_c = raw_walk ? 0 : refine_count(idx, p);
    hnsw_search_params wp = *p;
    KnnBatch wb = b;
    if (refine_c > 0 || walks_codes(idx)) {
        // the walk's results are where knn_search left them (raw_walk: in b itself): its flagged rows are rewritten there
        int rc = HNSW_OK;
        if (refine_c > 0) {
            wp.k = refine_c;
            rc = refine_walk(b, refine_c, walk ? *walk : idx->refine_scratch, &wb);
        }
        // (sq8 rows: the re-run walks the codes with the queries knn_search moved to code space)
        if (!rc && walks_codes(idx)) rc = sq8_walk_queries(idx, walk ? *walk : idx->refine_scratch, &wb, false, nullptr, st);
        if (rc) return rc;
    }
    const int rc = rerun_overflowed(idx, b.nq, b.st, [&](const int32_t *qmap, int64_t c, uint32_t *slab, int32_t cap) {
        return launch_rerun(idx, wp, wb, qmap, c, slab, cap, st, collect);
    });
    if (rc || refine_c == 0) return rc;
    // every query again (the same answer for those not repaired), and complete on return as the re-run is: callers go on to
    // other streams (hnsw_multi's exchange)
    const int rr = refine_rerank(idx, *p, b, wb, refine_c, st);
    if (rr) return rr;
    HIP_TRY(hipStreamSynchronize(st));
    return HNSW_OK;
}

hipError_t knn_download(const KnnBatch &b, int k, int32_t *ids, float *dist, uint32_t *nd, uint32_t *nh, hipStream_t st) {
    const size_t rbytes = (size_t)b.nq * k * 4, cbytes = (size_t)b.nq * 4;
    hipError_t e = hipSuccess;
    if (ids) e = hipMemcpyAsync(ids, b.ids, rbytes, hipMemcpyDeviceToHost, st);
    if (dist && e == hipSuccess) e = hipMemcpyAsync(dist, b.dist, rbytes, hipMemcpyDeviceToHost, st);
    if (nd && e == hipSuccess) e = hipMemcpyAsync(nd, b.nd, cbytes, hipMemcpyDeviceToHost, st);
    if (nh && e == hipSuccess) e = hipMemcpyAsync(nh, b.nh, cbytes, hipMemcpyDeviceToHost, st);
    return e;
}

// the handle's stream for the host-buffer call and its page-locked "any query flagged" word
int ensure_host_call_state(hnsw_index *idx) {
    if (!idx->hs[0]) HIP_TRY(hipStreamCreateWithFlags(&idx->hs[0].h, hipStreamNonBlocking));
    if (!idx->hFlag) {
        HIP_TRY(idx->hFlag.alloc(64, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void **)&idx->hFlagDev, idx->hFlag, 0));
    }
    return HNSW_OK;
}

int HostInput::resolve(const void *p, size_t n, DevBuf &stage) {
    bytes = n; from = nullptr;
    if ((dev = registered_device_address(p, n))) return HNSW_OK;
    const int rc = stage.ensure(n);
    dev = stage.p; from = p;
    return rc;
}
int HostInput::resolve_rows(hnsw_index *idx, const int32_t *ids, int64_t nq, DevBuf &stage) {
    bytes = (size_t)nq * padded_stride(idx->iv.d) * sizeof(float); from = nullptr;
    int rc;
    if ((rc = stage.ensure(bytes)) || (rc = idx->by_id_scratch.self.ensure((size_t)nq * 4))) return rc;
    dev = stage.p;
    rows_of = idx; row_ids = ids; d_row_ids = (int32_t *)idx->by_id_scratch.self.p; n_rows = nq;
    return HNSW_OK;
}
int HostInput::upload(hipStream_t st) const {
    if (from) HIP_TRY(hipMemcpyAsync(const_cast<void *>(dev), from, bytes, hipMemcpyHostToDevice, st));
    if (rows_of) {      // the ids up, then whole padded rows of the float32 table: what a staged copy of the same vectors holds, zeros behind d
        HIP_TRY(hipMemcpyAsync(d_row_ids, row_ids, (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
        const int64_t stride = padded_stride(rows_of->iv.d);
        return gather_rows(rows_of, d_row_ids, n_rows, (int32_t)stride, (float *)const_cast<void *>(dev), stride, st);
    }
    return HNSW_OK;
}

// A synchronous host-buffer call uploads, runs and downloads on the handle's stream hs[0], with ONE stream synchronisation at
// the end.  Each matrix of the caller is in place, in the small block or staged:
//  * IN PLACE: a page-locked matrix (hnsw_host_alloc / hnsw_host_register) is not copied at all.  The device reads the queries
//    straight from it -- each query once, by the wave that searches it (the descent pre-pass keeps a device copy for the search
//    kernel), so the 5 MB of a 10 k x 128 batch cross PCIe UNDER the descent instead of before it -- and writes each query's
//    results straight into the caller's matrices as the query finishes: no download step.  Ids and distances: both or neither.
//  * SMALL BLOCK (allow_small: the knn call): a small batch from ordinary memory (a single query: Ohnsw.knn, test/test.ml:122)
//    -- nothing registered; queries, results, counters of at most SMALL_BLOCK bytes each -- goes through a page-locked block of
//    the handle's own: the host copies the queries in, the device reads them and writes the results there, the host copies them
//    out.  What is left of the call is one launch and one synchronisation.
//  * STAGED: the rest goes through the handle's scratch by hipMemcpyAsync.  (Chunks on two streams to overlap copies and search
//    measured 1.08 against 1.06 ms in round 1.)
// The knn call (hnsw_search_batch) on queries IN PLACE, where the batch would be ordered, runs in TWO parts (option "head_queries",
// head_rows): the step is roughly "arrival of the last query over the link + the longest walk", and during the pre-pass --
// descent waves waiting for their queries: 0.1 ms of a 10 k batch -- the chip is almost empty.  So rows [0, H) are the HEAD: one
// plain, unordered launch on hs[1] with nothing in front of it, each wave fetching its own query, descending and walking while the
// link is the bottleneck; rows [H, nq) go through the ordered sequence on hs[0] as a batch of their own (qmap, q_limit, LDS
// padding and priorities are those of nq - H queries; the staged copy is their part of scratch.q).  The ordered launch then shares
// the chip with H fewer walks and has fewer late starters or none.  The parts meet at the END only: the host synchronises hs[1]
// before finish queues its download on hs[0] and synchronises that, so a staged counter array is copied behind both parts; both
// launches store into the one hFlag word and knn_repair runs on the whole batch behind the synchronisation.  No cross-stream
// edge anywhere in the call (profiles/r06_split_ab.txt paid for those).  An error in either part drains both streams before the
// call returns.  Measured: profiles/head_split_ab.txt.
// Every allocation is made before the first asynchronous copy is queued (a further input, as hnsw_rerank_batch's candidates, is
// resolved before begin and uploaded after it); once one is queued no return without a synchronisation: it reads or writes the
// caller's arrays.
constexpr size_t SMALL_BLOCK = 32768;

int HostCall::begin(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int k_, int32_t *out_ids, float *out_dist,
                    uint32_t *out_nd, uint32_t *out_nh, bool allow_small, bool *q_in_place) {
    // (a drop-self call: the kernels' rows are k_ wide, the caller's one entry narrower)
    const bool drop = rows && rows->drop_self;
    const size_t qbytes = query_bytes(nq, q_stride, idx->iv.d), rbytes = (size_t)nq * (drop ? k_ - 1 : k_) * 4, cbytes = (size_t)nq * 4;
    int rc;
    HostInput q;
    if ((rc = idx->scratch.ensure(nq, qbytes, k_)) || (rc = ensure_host_call_state(idx)) ||
        (rc = rows ? q.resolve_rows(idx, rows->ids, nq, idx->scratch.q) : q.resolve(queries, qbytes, idx->scratch.q)) ||
        (ko && (rc = idx->key_scratch.ensure(rbytes * 2))))
        return rc;
    if (dv) {           // (the selection's rows, dv->k wide)
        const size_t sbytes = (size_t)nq * dv->k * 4;
        DiverseBufs &db = idx->diverse_scratch;
        if ((rc = db.ids.ensure(sbytes)) || (rc = db.dist.ensure(sbytes)) || (dv->div && (rc = db.div.ensure(sbytes)))) return rc;
    }
    int32_t *zi = (int32_t *)registered_device_address(out_ids, rbytes);
    float *zd = (float *)registered_device_address(out_dist, rbytes);
    uint32_t *znd = (uint32_t *)registered_device_address(out_nd, cbytes), *znh = (uint32_t *)registered_device_address(out_nh, cbytes);
    if (drop) {
        // the epilogue's outputs: the caller's page-locked matrices in place (ids, or keys, and distances: both or neither), else
        // the handle's scratch; the kernels themselves write the k_ wide rows of scratch.ids / scratch.dist
        int64_t *zk = ko ? (int64_t *)registered_device_address(ko->keys, rbytes * 2) : nullptr;
        const bool in_place = zd && (ko ? zk != nullptr : zi != nullptr);
        ByIdBufs &bb = idx->by_id_scratch;
        if (!in_place && ((rc = bb.dist.ensure(rbytes)) || (!ko && (rc = bb.ids.ensure(rbytes))))) return rc;
        drop_dist = in_place ? zd : (float *)bb.dist.p;
        drop_ids = ko ? nullptr : in_place ? zi : (int32_t *)bb.ids.p;
        drop_keys = !ko ? nullptr : in_place ? zk : (int64_t *)idx->key_scratch.p;
        if (in_place) out_ids = nullptr, out_dist = nullptr;      // (complete when the epilogue is: nothing to download)
        zi = nullptr; zd = nullptr;
    }
    if (!zi || !zd) zi = nullptr, zd = nullptr;
    small = allow_small && !ko && !dv && q.from && !zi && !znd && !znh && qbytes <= SMALL_BLOCK && rbytes <= SMALL_BLOCK && cbytes <= SMALL_BLOCK;
    if (small) {
        if (!idx->hSmall) {
            HIP_TRY(idx->hSmall.alloc(5 * SMALL_BLOCK, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer((void **)&idx->hSmallDev, idx->hSmall, 0));
        }
        memcpy(idx->hSmall, queries, qbytes);
        char *s = idx->hSmallDev;
        q = HostInput{s};
        zi = (int32_t *)(s + SMALL_BLOCK); zd = (float *)(s + 2 * SMALL_BLOCK);
        if (out_nd) znd = (uint32_t *)(s + 3 * SMALL_BLOCK);
        if (out_nh) znh = (uint32_t *)(s + 4 * SMALL_BLOCK);
    }
    // the batch on the device: the scratch buffers, but for what the kernels read or write in place (or in the block) ...
    k = k_;
    b = idx->scratch.batch(nq, q_stride, k);
    b.Q = (const float *)q.dev;
    if (zi) b.ids = zi, b.dist = zd;
    if (znd) b.nd = znd;
    if (znh) b.nh = znh;
    // ... and the caller's arrays that are not complete when the kernels are
    ids = zi && !small ? nullptr : out_ids; dist = zi && !small ? nullptr : out_dist;
    nd = znd && !small ? nullptr : out_nd; nh = znh && !small ? nullptr : out_nh;
    if (q_in_place) *q_in_place = !q.from && !rows;
    if ((rc = q.upload(idx->hs[0])) || !is_cosine(idx)) return rc;
    // COSINE: the kernels read N(Q) in the handle's scratch, normalised on hs[0] from wherever the queries are (a page-locked
    // matrix in place, the block, the staged copy): from here on the call is the device-resident one -- no zero-copy reads by the
    // search, no head split (a failure here waits for the upload: it reads the caller's matrix)
    int64_t qs = q_stride;
    if ((rc = cosine_queries(idx, b.Q, nq, q_stride, idx->hs[0], &b.Q, &qs))) (void)hipStreamSynchronize(idx->hs[0]);
    if (q_in_place) *q_in_place = false;
    return rc;
}

int HostCall::finish(hnsw_index *idx, const char *what, hipStream_t st) {
    const bool drop = rows && rows->drop_self;
    // (a drop-self call downloads the counters here and its rows from where the epilogue below leaves them)
    hipError_t ed = small ? hipSuccess : knn_download(b, k, drop ? nullptr : ids, drop ? nullptr : dist, nd, nh, st);
    int rk = HNSW_OK;
    if (drop && ed == hipSuccess) {
        // the k wide inner rows where the search left them -> the k - 1 wide rows without each query's own id, as ids or as keys in
        // the same pass; then their download unless they were written in place (begin left ids / dist / ko's in_place accordingly)
        const size_t rbytes = (size_t)b.nq * (k - 1) * 4;
        rk = drop_self_rows(idx, b.ids, b.dist, (const int32_t *)idx->by_id_scratch.self.p, b.nq, k - 1, drop_ids, drop_keys, ko ? ko->missing : 0,
                            drop_dist, st);
        if (!rk && ids) ed = hipMemcpyAsync(ids, drop_ids, rbytes, hipMemcpyDeviceToHost, st);
        if (!rk && dist && ed == hipSuccess) ed = hipMemcpyAsync(dist, drop_dist, rbytes, hipMemcpyDeviceToHost, st);
        if (!rk && ko && drop_keys == (int64_t *)idx->key_scratch.p && ed == hipSuccess)
            ed = hipMemcpyAsync(ko->keys, drop_keys, rbytes * 2, hipMemcpyDeviceToHost, st);
    } else if (dv && ed == hipSuccess) {           // the selection over the rows where the inner call left them, then its rows' download
        const DiverseBufs &db = idx->diverse_scratch;
        const size_t sbytes = (size_t)b.nq * dv->k * 4;
        rk = launch_diversify(idx, b.Q, b.nq, b.q_stride, b.ids, k, dv->k, dv->lambda, dv->fill, (int32_t *)db.ids.p, (float *)db.dist.p,
                              dv->div ? (float *)db.div.p : nullptr, st);
        if (!rk) ed = hipMemcpyAsync(dv->ids, db.ids.p, sbytes, hipMemcpyDeviceToHost, st);
        if (!rk && ed == hipSuccess) ed = hipMemcpyAsync(dv->dist, db.dist.p, sbytes, hipMemcpyDeviceToHost, st);
        if (!rk && dv->div && ed == hipSuccess) ed = hipMemcpyAsync(dv->div, db.div.p, sbytes, hipMemcpyDeviceToHost, st);
    } else if (ko && ed == hipSuccess) {           // the rows as keys: one launch over the ids where the search left them, then their download
        rk = keys_translate(idx, b.ids, b.nq * k, ko->missing, (int64_t *)idx->key_scratch.p, st);
        if (!rk) ed = hipMemcpyAsync(ko->keys, idx->key_scratch.p, (size_t)b.nq * k * 8, hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = st ? hipStreamSynchronize(st) : hipDeviceSynchronize();
    if (rk) return rk;
    if (ed != hipSuccess) return hip_fail(ed, "result download");
    if (es != hipSuccess) return fail(HNSW_ERR_HIP, "%s failed: %s", what, hipGetErrorString(es));
    if (small) {
        const size_t rbytes = (size_t)b.nq * k * 4, cbytes = (size_t)b.nq * 4;
        memcpy(ids, idx->hSmall + SMALL_BLOCK, rbytes); memcpy(dist, idx->hSmall + 2 * SMALL_BLOCK, rbytes);
        if (nd) memcpy(nd, idx->hSmall + 3 * SMALL_BLOCK, cbytes);
        if (nh) memcpy(nh, idx->hSmall + 4 * SMALL_BLOCK, cbytes);
    }
    return HNSW_OK;
}

// One query (node 0's vector, k 1) through the plain and through the ordered launch on the handle's stream, results discarded:
// what loads the code objects of the shape of p (and makes the handle's stream and flag word)
int trial_search(hnsw_index *idx, hnsw_search_params p) {
    int rc = ensure_host_call_state(idx);
    if (rc) return rc;
    DevBuf out;
    if ((rc = out.ensure(64))) return rc;
    p.k = 1;
    const KnnBatch b{idx->iv.X, 1, idx->iv.stride, (int32_t *)out.p, (float *)out.p + 1, nullptr, nullptr, (uint32_t *)out.p + 2, nullptr};
    const int mode = idx->order_mode;
    for (int ordered = 0; ordered < 2 && !rc; ++ordered) {
        idx->order_mode = ordered;
        rc = knn_search(idx, &p, b, idx->hs[0]);
    }
    idx->order_mode = mode;
    const hipError_t e = hipStreamSynchronize(idx->hs[0]);
    if (!rc && e != hipSuccess) rc = fail(HNSW_ERR_HIP, "the trial search failed: %s", hipGetErrorString(e));
    return rc;
}

// The one-time costs of a process's FIRST search belong to index construction, which the reference's benchmark times on its own
// (benchmark/benchmark.ml:66-80 before :89-96): the code objects of the search kernels and of the ordering pre-pass (the
// runtime loads a translation unit's code when its first kernel is launched: 1.4 ms and 5.2 ms, tools/cold_probe.py), the
// handle's stream and flag word: a trial search at ef 1.  HNSW_WARM_UP=0 leaves them to the first call (7 ms instead of
// 0.6 ms for a 10 k batch).
int warm_up(hnsw_index *idx) {
    if (!env_int("HNSW_WARM_UP", 1) || idx->iv.n < 1 || idx->iv.entry_point < 0) return HNSW_OK;
    // Nothing here is needed for a valid index: a failure (a stream, 64 bytes, a dummy launch) clears the HIP error and leaves the
    // one-time costs to the first search call, which reports its own errors.  Callers ignore the return value.
    hnsw_search_params p{};
    p.ef = 1; p.k = 1; p.fill = HNSW_FILL_OHNSW; p.semantics = HNSW_SEM_OHNSW;
    const int rc = trial_search(idx, p);
    if (rc) (void)hipGetLastError();
    return rc;
}

void bind_view(hnsw_index *idx) {
    const IndexTables &t = idx->tables;
    IndexView &iv = idx->iv;
    // the knn searches read, in this order of precedence: byte rows (exact, the smallest), sq8 rows (option sq8_rows 1: in the
    // byte rows' place, for the same kernels) or half rows (option half_rows 1; the two options exclude each other), split rows, the
    // plain float32 rows
    // (the per-dimension codes, option sq8_dim_rows 1, and the 1-bit codes, option bit_rows 1 / 2, likewise; the four options
    // exclude each other)
    const bool bytes = !idx->byte_rows_off && t.X8.p, sq8 = !bytes && idx->sq8_on && t.Xq.p, sq8d = !bytes && !sq8 && idx->sq8d_on && t.Xqd.p,
               bits = !bytes && !sq8 && !sq8d && idx->bit_mode != 0 && t.Xb.p, half = !bytes && !sq8 && !sq8d && !bits && idx->half_rows_on && t.Xh.p;
    iv.X = (const float *)t.X.p;
    iv.X8 = bytes ? (const uint8_t *)t.X8.p : sq8 ? (const uint8_t *)t.Xq.p : sq8d ? (const uint8_t *)t.Xqd.p : bits ? (const uint8_t *)t.Xb.p : nullptr;
    if (half) iv.Xh = (const uint2 *)t.Xh.p;
    iv.stride8 = bits ? 64 * bit_words(iv.d) : (half ? 128 : 64) * pick_nch(iv.nchunks);
    iv.Xm = idx->split_rows_off || half || sq8 || sq8d || bits ? nullptr : (const float *)t.Xm.p;
    iv.tail0 = (const float *)t.tail0.p;
    if (sq8d) iv.sq8s = (const float *)t.qd_s.p;              // (in tail0's place: no split rows are read while the codes are)
    iv.nbr0 = (const int32_t *)t.nbr0.p; iv.nbrU = (const int32_t *)t.nbrU.p;
    iv.upper_off = (const int32_t *)t.off.p; iv.upper_lvl = (const uint8_t *)t.lvl.p; iv.upper_ref = (const int2 *)t.ref.p;
    iv.lcode = (const int32_t *)t.lcode.p; iv.lcode0 = (const int32_t *)t.lcode0.p;
    hnsw_index_info &inf = idx->info;
    inf.n = iv.n; inf.max_degree0 = iv.S0; inf.max_layer = iv.max_layer; inf.entry_point = (int64_t)iv.entry_point + iv.id_base;
    inf.row_stride_bytes = iv.stride * 4;
    inf.row_format = bytes ? HNSW_ROWS_BYTES : sq8 ? HNSW_ROWS_SQ8 : sq8d ? HNSW_ROWS_SQ8_DIM : bits ? HNSW_ROWS_BITS : half ? HNSW_ROWS_HALF : iv.Xm ? HNSW_ROWS_SPLIT : HNSW_ROWS_F32;
}

int finish_index(IndexPtr owned, int32_t expected_ef, int32_t expected_semantics, hnsw_index **out) {
    hnsw_index *idx = owned.get();
    bind_view(idx);
    int rc = make_byte_rows(idx);           // the index serves searches from the byte copy where the data allows
    if (!rc) rc = make_split_rows(idx);     // ... or from split rows where a row ends just past a 128-byte line
    if (rc) return rc;
    (void)warm_up(idx);                     // ... and its first search call does not pay for the process's code loading (an optimisation:
    prepare_quietly(idx, expected_ef, expected_semantics);      //  failures are left to the first search) nor for its shape's one-time decisions
    *out = owned.release();
    return HNSW_OK;
}

void prepare_quietly(hnsw_index *idx, int32_t ef, int32_t semantics) {
    if (ef <= 0 || idx->iv.n < 1 || idx->iv.entry_point < 0) return;
    hnsw_search_params p{};
    p.ef = ef; p.k = 1; p.fill = HNSW_FILL_OHNSW; p.semantics = semantics;
    const std::string keep = g_last_error;
    if (hnsw_index_prepare(idx, &p) != HNSW_OK) { (void)hipGetLastError(); g_last_error = keep; }     // an optimisation: the search reports its own errors
}
void adopt_blk_choice(hnsw_index *idx, int32_t ef, int32_t semantics, bool blocks) {
    if (ef < 1 || ef > 1024) return;
    const KnnShape sh = knn_shape(idx, ef, semantics);
    int &choice = sh.choice(idx).blk;
    if (sh.nslot < 3 || choice >= 0) return;
    int bits = 0;
    if (blocks && idx->lcode_state == 1 && (bits = blk_capacity_bits(idx, sh)) > 0 && materialise_lcode0(idx) == HNSW_OK && idx->tables.lcode0.p) {
        choice = bits;
        return;
    }
    if (!blocks) choice = 0;       // (blocks that cannot be honoured here stay undecided: measured on demand)
}
void list_blk_choices(const hnsw_index *idx, std::vector<int32_t> &out3) {
    static const int rep_ef[SLOT_CLASSES] = {64, 128, 192, 256, 384, 512, 1024};     // an ef of every slot class
    const int nch = pick_nch(idx->iv.nchunks);
    for (int c = 0; c < SLOT_CLASSES; ++c)
        for (int s = 0; s < 2; ++s) {
            const int blk = idx->shape[c][s].blk;
            if (blk < 0 || slot_class(pick_nslot_knn(rep_ef[c], nch)) != c) continue;    // (undecided, or no such slot count for these rows)
            out3.push_back(rep_ef[c]); out3.push_back(s); out3.push_back(blk > 0 ? 1 : 0);
        }
}
} // namespace hnsw_host

// ---- ABI ---------------------------------------------------------------------------------------
extern "C" {

// the forms that cannot run the ladder (device buffers, h2d, submit) on a handle with nodes marked deleted
static int marked_unsupported(const hnsw_index *idx, const char *call) {
    return fail(HNSW_ERR_UNSUPPORTED, "%s: %lld nodes are marked deleted and this form cannot search around them: compact or unmark first", call,
                (long long)idx->n_deleted);
}

int32_t hnsw_abi_version(void) { return HNSW_ABI_VERSION; }
const char *hnsw_last_error(void) { return hnsw_host::g_last_error.c_str(); }

int32_t hnsw_device_count(int32_t *count) {
    if (!count) return fail(HNSW_ERR_BAD_ARG, "null count");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); return fail(HNSW_ERR_NO_DEVICE, "no HIP device: %s", hipGetErrorString(e)); }
    *count = c;
    return HNSW_OK;
}

int32_t hnsw_index_create(const hnsw_index_desc *d, int32_t device, hnsw_index **out) { return create_index(d, device, false, out); }

} // extern "C"

int hnsw_host::create_index(const hnsw_index_desc *d, int32_t device, bool stored_rows, hnsw_index **out) {
    if (!d || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (d->n < 0 || d->n > 0x7FFFFFF0LL) return fail(HNSW_ERR_BAD_ARG, "n=%lld out of range", (long long)d->n);
    if (d->d < 1) return fail(HNSW_ERR_BAD_ARG, "d=%d", d->d);
    if (d->row_stride < d->d) return fail(HNSW_ERR_BAD_ARG, "row_stride < d");
    if (d->metric != HNSW_METRIC_L2 && d->metric != HNSW_METRIC_IP && d->metric != HNSW_METRIC_COSINE) return fail(HNSW_ERR_BAD_ARG, "bad metric %d", d->metric);
    if (d->max_degree0 < 1 || d->max_degree0 > 64) return fail(HNSW_ERR_UNSUPPORTED, "max_degree0=%d must be in 1..64", d->max_degree0);
    if (d->max_layer < 0 || d->max_layer > 255) return fail(HNSW_ERR_BAD_ARG, "max_layer=%d", d->max_layer);
    if (d->max_layer > 0 && (d->max_degree < 1 || d->max_degree > 64)) return fail(HNSW_ERR_UNSUPPORTED, "max_degree=%d must be in 1..64", d->max_degree);
    if (d->n > 0 && (!d->vectors || !d->deg0 || !d->nbr0)) return fail(HNSW_ERR_BAD_ARG, "null vectors/deg0/nbr0");
    if (d->max_layer > 0 && !d->upper) return fail(HNSW_ERR_BAD_ARG, "null upper");
    const int nchunks = (d->d + 3) / 4;
    if (pick_nch(nchunks) == 0) return fail(HNSW_ERR_UNSUPPORTED, "d=%d > 1024 not supported", d->d);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(HNSW_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (device < 0 || device >= ndev) return fail(HNSW_ERR_BAD_ARG, "device %d out of range (have %d)", device, ndev);

    const int64_t n = d->n;
    const int32_t base = d->id_base;
    const int S0 = d->max_degree0, SU = d->max_layer > 0 ? d->max_degree : 1;
    int64_t ep = d->entry_point - base;
    if (n == 0 || ep < 0) ep = -1;
    if (ep >= n) return fail(HNSW_ERR_BAD_ARG, "Hgraph.set_entry_point: invalid node"); /* lib/ohnsw.ml:343 */

    // ---- layer 0: validate, rebase to 0, pad with -1 ----
    std::vector<int32_t> nbr0((size_t)n * S0, -1);
    for (int64_t i = 0; i < n; ++i) {
        const int dg = d->deg0[i];
        if (dg < 0) return fail(HNSW_ERR_BAD_ARG, "deg0[%lld] < 0", (long long)i);
        if (dg > S0) return fail(HNSW_ERR_DEGREE_OVERFLOW, "node %lld has %d layer-0 neighbours > max_degree0=%d", (long long)i + base, dg, S0);
        for (int j = 0; j < dg; ++j) {
            const int64_t v = (int64_t)d->nbr0[i * S0 + j] - base;
            if (v < 0 || v >= n) return fail(HNSW_ERR_BAD_ARG, "Vector.get: neighbour id %lld of node %lld out of range", (long long)v + base, (long long)i + base); /* lib/ohnsw.ml:25 */
            nbr0[(size_t)i * S0 + j] = (int32_t)v;
        }
    }
    // ---- upper layers: per node, rows for layers 1..lvl(node), contiguous ----
    std::vector<uint8_t> lvl((size_t)std::max<int64_t>(n, 1), 0);
    for (int l = 1; l <= d->max_layer; ++l) {
        const hnsw_layer_desc &L = d->upper[l - 1];
        if (L.n_nodes < 0 || (L.n_nodes > 0 && (!L.nodes || !L.deg || !L.nbr))) return fail(HNSW_ERR_BAD_ARG, "layer %d: null arrays", l);
        for (int64_t s = 0; s < L.n_nodes; ++s) {
            const int64_t v = L.nodes[s] - base;
            if (v < 0 || v >= n) return fail(HNSW_ERR_BAD_ARG, "layer %d: node id out of range", l);
            lvl[(size_t)v] = (uint8_t)std::max<int>(lvl[(size_t)v], l);
        }
    }
    std::vector<int2> ref;
    const int64_t rowsU = upper_layout(lvl.data(), (int64_t)lvl.size(), 0, ref);
    if (rowsU > 0x7FFFFFF0LL) return fail(HNSW_ERR_UNSUPPORTED, "too many upper rows");
    std::vector<int32_t> nbrU((size_t)std::max<int64_t>(rowsU, 1) * SU, -1);
    for (int l = 1; l <= d->max_layer; ++l) {
        const hnsw_layer_desc &L = d->upper[l - 1];
        for (int64_t s = 0; s < L.n_nodes; ++s) {
            const int64_t v = L.nodes[s] - base;
            const int dg = L.deg[s];
            if (dg < 0) return fail(HNSW_ERR_BAD_ARG, "layer %d: negative degree", l);
            if (dg > SU) return fail(HNSW_ERR_DEGREE_OVERFLOW, "node %lld has %d neighbours on layer %d > max_degree=%d", (long long)v + base, dg, l, SU);
            int32_t *row = &nbrU[((size_t)ref[(size_t)v].x + (l - 1)) * SU];
            for (int j = 0; j < dg; ++j) {
                const int64_t u = (int64_t)L.nbr[s * SU + j] - base;
                if (u < 0 || u >= n) return fail(HNSW_ERR_BAD_ARG, "layer %d: neighbour id out of range", l);
                row[j] = (int32_t)u;
            }
        }
    }

    HIP_TRY(hipSetDevice(device));
    IndexPtr idx(new hnsw_index());
    idx->device = device;
    IndexTables &t = idx->tables;
    // ---- vectors: rows zero-padded to a multiple of 64 B so every float4 chunk is in bounds ----
    const int64_t stride = padded_stride(d->d);
    int rc = alloc_graph_tables(t, n, stride, S0, SU, rowsU);
    if (!rc) rc = upload_rows(d->vectors, n, d->d, d->row_stride, (float *)t.X.p);
    // COSINE: the table holds N(X) (rows a handle stored already are N(X): hnsw_index_load)
    if (!rc && d->metric == HNSW_METRIC_COSINE && !stored_rows) rc = cosine_store_rows((float *)t.X.p, n, d->d, "no index made");
    if (!rc && hipMemcpy(t.nbr0.p, nbr0.data(), nbr0.size() * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(HNSW_ERR_OOM, "graph upload failed");
    if (!rc && hipMemcpy(t.nbrU.p, nbrU.data(), nbrU.size() * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail(HNSW_ERR_OOM, "graph upload failed");
    if (!rc) rc = upload_upper_layout(t, 0, ref);
    if (rc) return rc;
    IndexView &iv = idx->iv;
    iv.stride = stride; iv.n = n; iv.d = d->d; iv.nchunks = nchunks; iv.S0 = S0; iv.SU = SU; iv.rowsU = rowsU;
    iv.max_layer = d->max_layer; iv.entry_point = (int32_t)ep; iv.id_base = base;
    hnsw_index_info &inf = idx->info;
    inf.d = d->d; inf.metric = d->metric; inf.id_base = base; inf.max_degree = d->max_degree; inf.device = device;
    return finish_index(std::move(idx), d->expected_ef, d->expected_semantics, out);
}

extern "C" {

int32_t hnsw_index_destroy(hnsw_index *idx) {
    if (!idx) return HNSW_OK;
    if (idx->device >= 0) (void)hipSetDevice(idx->device);     // current before any member is freed
    (void)hipDeviceSynchronize();                               // requests never waited for
    delete idx;
    return HNSW_OK;
}

int32_t hnsw_index_get_info(const hnsw_index *idx, hnsw_index_info *info) {
    if (!idx || !info) return fail(HNSW_ERR_BAD_ARG, "null argument");
    *info = idx->info;
    info->device_bytes = (int64_t)idx->tables.bytes();
    return HNSW_OK;
}

int32_t hnsw_index_locality_codes(hnsw_index *idx, int32_t *out) {
    if (!idx || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    int rc = build_locality_codes(idx);
    if (rc) return rc;
    if (idx->lcode_state != 1) return fail(HNSW_ERR_UNSUPPORTED, "no locality codes: the index has no upper layer (or no room for the tables)");
    HIP_TRY(hipMemcpy(out, idx->tables.lcode.p, (size_t)idx->iv.n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    release_unused_lcode0(idx);              // introspection needs the per-node codes only
    return HNSW_OK;
}

int32_t hnsw_index_visited_blocks(hnsw_index *idx, const hnsw_search_params *params, int32_t *log2_slots) {
    if (!log2_slots) return fail(HNSW_ERR_BAD_ARG, "null argument");
    int rc = check_params(idx, params);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    *log2_slots = knn_blk_bits(idx, knn_shape(idx, params->ef, params->semantics));
    return HNSW_OK;
}

int32_t hnsw_index_prepare(hnsw_index *idx, const hnsw_search_params *params) {
    int rc = check_params(idx, params);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    // the visited structure of this kernel shape (codes, measurement) and its residency, kept in the handle
    (void)resident_queries(idx, knn_shape(idx, params->ef, params->semantics));
    // the code object of the shape's translation unit
    if ((rc = trial_search(idx, *params))) return rc;
    const std::pair<int, int> key(params->ef, params->semantics);
    if (std::find(idx->prepared.begin(), idx->prepared.end(), key) == idx->prepared.end()) idx->prepared.push_back(key);
    return HNSW_OK;
}

int32_t hnsw_index_row_bytes(const hnsw_index *idx, int64_t *row_bytes) {
    if (!idx || !row_bytes) return fail(HNSW_ERR_BAD_ARG, "null argument");
    const int f = idx->info.row_format;
    if (f == HNSW_ROWS_BITS) { *row_bytes = ((int64_t)idx->iv.d + 7) / 8; return HNSW_OK; }   // (codes, but not a byte per dimension)
    *row_bytes = (int64_t)idx->iv.d * (f == HNSW_ROWS_BYTES || walks_codes(idx) ? 1 : f == HNSW_ROWS_HALF ? 2 : 4);
    return HNSW_OK;
}

int32_t hnsw_index_set_option(hnsw_index *idx, const char *name, int64_t value) {
    if (!idx || !name) return fail(HNSW_ERR_BAD_ARG, "null argument");
    // (an option that changes the kernel variant or its LDS makes the per-shape decisions stale -- forget_shapes --: the visited
    // structure's directory size follows the variant's occupancy, the residency follows the LDS)
    if (!strcmp(name, "vt_bits")) { idx->vt_bits_override = (int)value; idx->forget_shapes(); return HNSW_OK; }
    if (!strcmp(name, "lds_pad")) { idx->lds_pad = value < 0 ? -1 : (int)std::min<int64_t>(value, 32768); return HNSW_OK; }
    if (!strcmp(name, "byte_rows")) {     // 0: search the fp32 rows even where a byte copy exists; otherwise: use it where it exists
        idx->byte_rows_off = value == 0;
        bind_view(idx);
        idx->forget_shapes();
        return HNSW_OK;
    }
    if (!strcmp(name, "split_rows")) {    // 0: search the plain fp32 rows even where a split copy exists; -1: ... and free the copy; otherwise: use it where it exists
        if (value < 0 && idx->tables.Xm.p) {
            HIP_TRY(hipSetDevice(idx->device));
            HIP_TRY(hipDeviceSynchronize());             // launches that still read the copy
            idx->tables.Xm.release(); idx->tables.tail0.release();
        }
        idx->split_rows_off = value <= 0;
        idx->split_rows_freed = idx->split_rows_freed || value < 0;
        bind_view(idx);
        idx->forget_shapes();
        return HNSW_OK;
    }
    if (!strcmp(name, "half_rows")) {     // 1: search the fp16 copy (made now if missing); 0: the fp32 / split rows again, the copy kept; -1: ... and freed
        if (value > 0) {
            if (idx->info.row_format == HNSW_ROWS_BYTES)
                return fail(HNSW_ERR_BAD_ARG, "half_rows: the index searches its byte rows, which are exact and half the size of half rows "
                                              "(set byte_rows 0 first)");
            if (codes_on(idx)) return fail(HNSW_ERR_BAD_ARG, "half_rows: option %s is on (set it 0 first)", codes_option(idx));
            if (idx->filter_collect) return fail(HNSW_ERR_BAD_ARG, "half_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->tables.Xh.p) {
                const int rc = make_half_rows(idx);     // (a refusal -- NaN, fp16 overflow -- leaves the index as it was)
                if (rc) return rc;
            }
            idx->half_rows_on = true;
        } else {
            if (value < 0 && idx->tables.Xh.p) {
                HIP_TRY(hipSetDevice(idx->device));
                HIP_TRY(hipDeviceSynchronize());         // launches that still read the copy
                idx->tables.Xh.release();
            }
            idx->half_rows_on = false;
        }
        bind_view(idx);
        idx->forget_shapes();
        return HNSW_OK;
    }
    if (!strcmp(name, "sq8_rows")) {      // 1: walk the 8-bit codes (made now if missing), re-rank over the fp32 rows; 0: the previous rows again, the codes kept; -1: ... and freed
        if (value > 0) {
            if (idx->info.row_format == HNSW_ROWS_BYTES)
                return fail(HNSW_ERR_BAD_ARG, "sq8_rows: the index searches its byte rows, which are exact and the same size (set byte_rows 0 first)");
            if (idx->half_rows_on) return fail(HNSW_ERR_BAD_ARG, "sq8_rows: option half_rows is on (set half_rows 0 first)");
            if (idx->sq8d_on) return fail(HNSW_ERR_BAD_ARG, "sq8_rows: option sq8_dim_rows is on (set sq8_dim_rows 0 first)");
            if (idx->bit_mode) return fail(HNSW_ERR_BAD_ARG, "sq8_rows: option bit_rows is on (set bit_rows 0 first)");
            if (idx->filter_collect) return fail(HNSW_ERR_BAD_ARG, "sq8_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->tables.Xq.p) {
                const int rc = make_sq8_rows(idx);      // (a refusal -- NaN, infinity, range overflow -- leaves the index as it was)
                if (rc) return rc;
            }
            idx->sq8_on = true;
        } else {
            if (value < 0 && idx->tables.Xq.p) {
                HIP_TRY(hipSetDevice(idx->device));
                HIP_TRY(hipDeviceSynchronize());         // launches that still read the copy
                idx->tables.Xq.release();
            }
            idx->sq8_on = false;
        }
        bind_view(idx);
        idx->forget_shapes();
        return HNSW_OK;
    }
    if (!strcmp(name, "sq8_dim_rows")) {  // as "sq8_rows", the codes under one affine map per dimension (hnsw_rows_sq8_dim.hip)
        if (value < -1 || value > 1) return fail(HNSW_ERR_BAD_ARG, "sq8_dim_rows=%lld: 1 (on), 0 (off) or -1 (off, the copy freed)", (long long)value);
        if (value > 0) {
            if (idx->info.row_format == HNSW_ROWS_BYTES)
                return fail(HNSW_ERR_BAD_ARG, "sq8_dim_rows: the index searches its byte rows, which are exact and the same size (set byte_rows 0 first)");
            if (idx->half_rows_on) return fail(HNSW_ERR_BAD_ARG, "sq8_dim_rows: option half_rows is on (set half_rows 0 first)");
            if (idx->sq8_on) return fail(HNSW_ERR_BAD_ARG, "sq8_dim_rows: option sq8_rows is on (set sq8_rows 0 first)");
            if (idx->bit_mode) return fail(HNSW_ERR_BAD_ARG, "sq8_dim_rows: option bit_rows is on (set bit_rows 0 first)");
            if (idx->filter_collect) return fail(HNSW_ERR_BAD_ARG, "sq8_dim_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->tables.Xqd.p) {
                const int rc = make_sq8_dim_rows(idx);  // (a refusal -- NaN, infinity, a column's range -- leaves the index as it was)
                if (rc) return rc;
            }
            idx->sq8d_on = true;
        } else {
            if (value < 0 && idx->tables.Xqd.p) {
                HIP_TRY(hipSetDevice(idx->device));
                HIP_TRY(hipDeviceSynchronize());         // launches that still read the copy
                idx->tables.Xqd.release(); idx->tables.qd_lo.release(); idx->tables.qd_s.release();
                idx->sq8d_lo.clear(); idx->sq8d_scale.clear();
            }
            idx->sq8d_on = false;
        }
        bind_view(idx);
        idx->forget_shapes();
        return HNSW_OK;
    }
    if (!strcmp(name, "bit_rows")) {      // 1-bit codes walked under Hamming distance (hnsw_rows_bits.hip): 1 = thresholds at the column means, 2 = at zero
        if (value < 0 || value > 2) return fail(HNSW_ERR_BAD_ARG, "bit_rows=%lld: 0 (off), 1 (thresholds at the column means) or 2 (at zero)", (long long)value);
        if (value > 0) {
            if (idx->info.row_format == HNSW_ROWS_BYTES)
                return fail(HNSW_ERR_BAD_ARG, "bit_rows: the index searches its byte rows, which are exact (set byte_rows 0 first)");
            if (idx->half_rows_on) return fail(HNSW_ERR_BAD_ARG, "bit_rows: option half_rows is on (set half_rows 0 first)");
            if (idx->sq8_on) return fail(HNSW_ERR_BAD_ARG, "bit_rows: option sq8_rows is on (set sq8_rows 0 first)");
            if (idx->sq8d_on) return fail(HNSW_ERR_BAD_ARG, "bit_rows: option sq8_dim_rows is on (set sq8_dim_rows 0 first)");
            if (idx->filter_collect) return fail(HNSW_ERR_BAD_ARG, "bit_rows: option filter_collect is on, which needs exact rows (set filter_collect 0 first)");
            if (!idx->tables.Xb.p || idx->bit_mode != (int)value) {
                HIP_TRY(hipSetDevice(idx->device));
                HIP_TRY(hipDeviceSynchronize());         // launches that still read a copy of the other mode
                const int rc = make_bit_rows(idx, (int)value);   // (a refusal -- NaN, infinity -- leaves the index as it was)
                if (rc) return rc;
            }
            idx->bit_mode = (int)value;
        } else {
            if (idx->tables.Xb.p) {
                HIP_TRY(hipSetDevice(idx->device));
                HIP_TRY(hipDeviceSynchronize());         // launches that still read the copy
                idx->tables.Xb.release(); idx->tables.bit_t.release();
                idx->bit_t.clear();
            }
            idx->bit_mode = 0;
        }
        bind_view(idx);
        idx->forget_shapes();
        return HNSW_OK;
    }
    if (!strcmp(name, "bit_query_bits")) {   // 4: the walk over the bit rows keeps the query at 4 bits a dimension (hnsw_bits_asym_walk.hip); 0: at one
        if (value != 0 && value != 4) return fail(HNSW_ERR_BAD_ARG, "bit_query_bits=%lld: 0 (off) or 4", (long long)value);
        idx->bit_query_bits = (int)value;   // (takes effect while the searches walk the bit rows, as refine does for half rows; not saved)
        idx->forget_shapes();               // (another kernel of the same shape: its residency may differ)
        return HNSW_OK;
    }
    if (!strcmp(name, "refine")) {        // 0: off; 1..1024: re-rank max(k, value) members of W over the float32 rows; -1: all ef (half and sq8 rows only)
        if (value < -1 || value > 1024) return fail(HNSW_ERR_BAD_ARG, "refine=%lld: 0 (off), 1..1024 candidates or -1 (all of W)", (long long)value);
        idx->refine = (int)value;
        return HNSW_OK;
    }
    if (!strcmp(name, "filter_collect")) {   // 1: the filtered searches answer from every node the walk evaluates (k <= 128, exact rows); 0: from the final W
        if (value != 0 && value != 1) return fail(HNSW_ERR_BAD_ARG, "filter_collect=%lld: 0 (off) or 1", (long long)value);
        if (value == 1 && (idx->half_rows_on || codes_on(idx)))   // (on, even while byte rows stand in front of them: "byte_rows" 0 would bring them back)
            return fail(HNSW_ERR_BAD_ARG, "filter_collect: option %s is on, and a walk over those rows has no exact distances (set it 0 first)",
                        codes_on(idx) ? codes_option(idx) : "half_rows");
        idx->filter_collect = value == 1;
        return HNSW_OK;
    }
    if (!strcmp(name, "time_kernels")) { idx->time_kernels = value != 0; return HNSW_OK; }
    if (!strcmp(name, "visited_blocks")) {   // -1: measured per kernel shape (default); 0: the tag cache; 1: bitmap blocks wherever the codes can be built
        idx->blk_mode = value < 0 ? -1 : (value ? 1 : 0);
        idx->forget_shapes();               // (the LDS per wave, hence the residency, may differ)
        return HNSW_OK;
    }
    if (!strcmp(name, "device_fallback_slab_bytes")) {
        // room for the tie lists of value / (4 n) flagged queries per call (a flagged query may need a slot per node)
        HIP_TRY(hipSetDevice(idx->device));
        HIP_TRY(hipDeviceSynchronize());
        idx->dFbSlab.release(); idx->dFbMap.release(); idx->fb_queries = 0;
        if (value <= 0) return HNSW_OK;
        const int64_t per_query = std::max<int64_t>(idx->iv.n, 1) * 4;
        const int64_t q = std::min<int64_t>(value / per_query, 65536);
        if (q < 1) return fail(HNSW_ERR_BAD_ARG, "device_fallback_slab_bytes=%lld holds no query: one needs 4 n = %lld bytes", (long long)value, (long long)per_query);
        int rc;
        DevBuf slab, map;                    // (members only once both exist: a failed allocation leaves both empty)
        if ((rc = slab.ensure((size_t)(q * per_query))) || (rc = map.ensure((size_t)(q + 1) * 4))) return rc;
        idx->dFbSlab = std::move(slab); idx->dFbMap = std::move(map);
        idx->fb_queries = q;
        return HNSW_OK;
    }
    if (!strcmp(name, "order_queries")) { idx->order_mode = value < 0 ? -1 : (value ? 1 : 0); return HNSW_OK; }
    if (!strcmp(name, "head_queries")) { idx->head_queries = std::max<int64_t>(-1, std::min<int64_t>(value, 0x7FFFFFFF)); return HNSW_OK; }
    if (!strcmp(name, "scan_slabs")) { idx->scan_slabs = (int)std::max<int64_t>(0, std::min<int64_t>(value, 1024)); return HNSW_OK; }
    if (!strcmp(name, "graph_chunk_rows")) {         // the nodes hnsw_knn_graph searches per inner call (hnsw_by_id.hip)
        if (value < 1) return fail(HNSW_ERR_BAD_ARG, "graph_chunk_rows=%lld: a chunk holds at least one node", (long long)value);
        idx->graph_chunk_rows = std::min<int64_t>(value, 0x7FFFFFFF);
        return HNSW_OK;
    }
    return fail(HNSW_ERR_BAD_ARG, "unknown option %s", name);
}

} // extern "C"

// The value hnsw_index_set_option would have to be given to put option `name` back where it is now (not a public call:
// hnsw_sharded_set_option undoes a half-applied option with it).  What -1 freed stays freed: "half_rows" / "sq8_rows" read 0 then.
int hnsw_host::get_option(const hnsw_index *idx, const char *name, int64_t *value) {
    if (!idx || !name || !value) return fail(HNSW_ERR_BAD_ARG, "null argument");
    const struct { const char *name; int64_t value; } now[] = {
        {"vt_bits", idx->vt_bits_override}, {"lds_pad", idx->lds_pad}, {"byte_rows", idx->byte_rows_off ? 0 : 1},
        {"split_rows", idx->split_rows_freed ? -1 : idx->split_rows_off ? 0 : 1}, {"half_rows", idx->half_rows_on ? 1 : 0},
        {"sq8_rows", idx->sq8_on ? 1 : 0}, {"sq8_dim_rows", idx->sq8d_on ? 1 : 0}, {"bit_rows", idx->bit_mode}, {"bit_query_bits", idx->bit_query_bits}, {"refine", idx->refine}, {"time_kernels", idx->time_kernels ? 1 : 0},
        {"visited_blocks", idx->blk_mode}, {"device_fallback_slab_bytes", (int64_t)idx->dFbSlab.bytes},
        {"order_queries", idx->order_mode}, {"head_queries", idx->head_queries}, {"scan_slabs", idx->scan_slabs}, {"graph_chunk_rows", idx->graph_chunk_rows}, {"filter_collect", idx->filter_collect ? 1 : 0}};
    for (const auto &o : now) if (!strcmp(name, o.name)) { *value = o.value; return HNSW_OK; }
    return fail(HNSW_ERR_BAD_ARG, "unknown option %s", name);
}

extern "C" {

int32_t hnsw_search_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride,
                                 const hnsw_search_params *params, int32_t *d_ids, float *d_dist,
                                 uint32_t *d_ndist, uint32_t *d_nhops, uint32_t *d_status, void *stream) {
    if (idx && idx->n_deleted > 0) return marked_unsupported(idx, "hnsw_search_batch_device");
    if (idx && is_cosine(idx)) {            // N(Q) on the caller's stream first; everything behind reads the handle's scratch
        int rc = check_batch(idx, params, nq, q_stride, d_queries && d_ids && d_dist);
        if (rc || nq == 0) return rc;
        HIP_TRY(hipSetDevice(idx->device));
        if ((rc = cosine_queries(idx, d_queries, nq, q_stride, (hipStream_t)stream, &d_queries, &q_stride))) return rc;
    }
    return knn_search(idx, params, {d_queries, nq, q_stride, d_ids, d_dist, d_ndist, d_nhops, d_status, nullptr}, (hipStream_t)stream);
}

int32_t hnsw_index_kernel_times(hnsw_index *idx, double *search_ms, double *prepass_ms, int32_t *calls) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    HIP_TRY(hipSetDevice(idx->device));
    double s = 0, p = 0;
    const size_t n = idx->tev_used / 3;
    for (size_t i = 0; i < n; ++i) {
        float a = 0, b = 0;
        HIP_TRY(hipEventSynchronize(idx->tev[3 * i + 2]));
        HIP_TRY(hipEventElapsedTime(&a, idx->tev[3 * i], idx->tev[3 * i + 1]));
        HIP_TRY(hipEventElapsedTime(&b, idx->tev[3 * i + 1], idx->tev[3 * i + 2]));
        if (idx->tev_ordered[i]) p += a;
        s += b;
    }
    idx->tev_used = 0;
    if (search_ms) *search_ms = n ? s / (double)n : 0.0;
    if (prepass_ms) *prepass_ms = n ? p / (double)n : 0.0;
    if (calls) *calls = (int32_t)n;
    return HNSW_OK;
}

// Option "head_queries": how many rows [0, H) of a host call's batch are searched as its HEAD (hnsw_search_batch), 0 = none.
// Only where the call reads its query matrix in place, would order the whole batch, and is a plain knn walk (no re-rank: refine,
// sq8 rows).  -1: H_AUTO below.
int64_t head_rows(hnsw_index *idx, const hnsw_search_params *p, int64_t nq) {
    if (idx->head_queries == 0 || nq < 2 || refine_count(idx, p) > 0 || walks_codes(idx)) return 0;
    const Residency res = resident_queries(idx, knn_shape(idx, p->ef, p->semantics));
    const int mode = idx->order_mode;
    if (mode == 0 || (mode != 1 && 2 * nq <= res.queries)) return 0;          // the batch would not be ordered
    if (idx->head_queries > 0) return std::min<int64_t>(idx->head_queries, nq - 1);
    if (res.per_cu <= 0) return 0;
    // H_AUTO (profiles/head_split_ab.txt, byte rows at ef 128, R = 8192): a batch the chip holds at once loses 4-6 % to a head
    // of any size -- its walks take slots and memory requests from the descent waves and there are no late starters to save --;
    // with nq - R late starters the split wins, 3 % at nq = 1.2 R and 8-10 % from 1.5 R on.  So: only when the late starters are a
    // fifth of R or more; then the head that leaves the ordered part a whole number of passes of R, if that head is 0.3 to 0.5
    // of the batch (more loses again: the descent starves), else 0.3 of the batch.
    const int64_t R = res.queries;
    if (5 * (nq - R) < R) return 0;
    const int64_t passes = (7 * nq / 10) / R, h = nq - passes * R;
    return passes >= 1 && 2 * h <= nq ? h : 3 * nq / 10;
}

int32_t hnsw_search_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                          const hnsw_search_params *params, int32_t *out_ids, float *out_dist,
                          uint32_t *out_ndist, uint32_t *out_nhops) {
    return knn_host_call(idx, queries, nq, q_stride, params, out_ids, out_dist, out_ndist, out_nhops, nullptr, nullptr);
}

} // extern "C"

int hnsw_host::knn_host_call(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, const hnsw_search_params *params,
                             int32_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops, uint32_t *out_stage, const KeysOut *ko,
                             const RowsIn *rows, const DiverseOut *dv) {
    int rc = check_batch(idx, params, nq, q_stride, (rows ? rows->ids != nullptr : queries != nullptr) &&
                                                        (dv ? dv->ids && dv->dist : (ko ? ko->keys != nullptr : out_ids != nullptr) && out_dist));
    if (rc) return rc;
    // nodes are marked deleted: the filtered search under the handle's live mask, ladder, exact stage and all
    if (idx->n_deleted > 0)
        return filtered_host_call(idx, idx->live.get(), queries, nq, q_stride, params, out_ids, out_dist, out_ndist, out_nhops, out_stage, ko, rows, dv);
    if (nq == 0) return rc;
    if (out_stage) memset(out_stage, 0, (size_t)nq * 4);
    HIP_TRY(hipSetDevice(idx->device));
    // Where the matrices live: HostCall::begin.  The search is ordered longest walk first when the batch is larger than the chip
    // holds; whether any query needs the exactness fallback comes back as one word (pinned host memory, the kernel stores it),
    // not as a scan of nq status words.
    HostCall c;
    c.ko = ko;
    c.rows = rows;
    c.dv = dv;
    bool q_in_place = false;
    if ((rc = c.begin(idx, queries, nq, q_stride, params->k, out_ids, out_dist, out_ndist, out_nhops, true, &q_in_place))) return rc;
    hipStream_t st = idx->hs[0];
    c.b.any_flag = idx->hFlagDev;
    *(volatile uint32_t *)idx->hFlag = 0;
    // The head of the batch (head_rows; the comment above HostCall::begin): a plain launch on hs[1] in which every wave reads its
    // own query over the link, descends and walks -- nothing in front of it, so its walks run while the main part's pre-pass waits
    // for the link -- and the ordered sequence on hs[0] for the rows behind it; the two meet at the end only.
    const int64_t H = q_in_place ? head_rows(idx, params, nq) : 0;
    if (H > 0) {
        if (!idx->hs[1]) HIP_TRY(hipStreamCreateWithFlags(&idx->hs[1].h, hipStreamNonBlocking));
        KnnBatch head = c.b, rest = c.b;
        head.nq = H;
        rest.nq = nq - H; rest.Q += H * q_stride; rest.ids += H * params->k; rest.dist += H * params->k;
        rest.nd += H; rest.nh += H; rest.st += H;
        const KnnShape sh = knn_shape(idx, params->ef, params->semantics);
        rc = launch_search_args(idx, sh, knn_args(*params, head, knn_vt_bits(idx, sh), knn_blk_bits(idx, sh)), idx->hs[1]);
        if (!rc) {
            const int mode = idx->order_mode;
            idx->order_mode = 1;            // (the whole batch would be ordered: so is the part)
            rc = knn_search(idx, params, rest, st, (float *)idx->scratch.q.p + H * q_stride);
            idx->order_mode = mode;
        }
        // the join, from the host (cheaper than an event hs[0] waits for: profiles/head_split_ab.txt): the head, which began
        // 0.1 ms before the ordered launch, has ended long before it; finish's download is queued behind this
        const hipError_t eh = hipStreamSynchronize(idx->hs[1]);
        if (!rc && eh != hipSuccess) rc = fail(HNSW_ERR_HIP, "search failed: %s", hipGetErrorString(eh));
    } else
        rc = knn_search(idx, params, c.b, st, q_in_place ? (float *)idx->scratch.q.p : nullptr);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    if ((rc = c.finish(idx, "search", st))) return rc;
    if (*(volatile uint32_t *)idx->hFlag & 1u) {      // (the flag: written by the kernel, pinned host memory)
        // Exactness fallback for queries whose tie-overflow stack outgrew its LDS slots (rare: the rows of the whole batch
        // are then copied out again, on the null stream)
        if ((rc = knn_repair(idx, params, c.b, nullptr))) return rc;
        return c.finish(idx, "result download", nullptr);
    }
    return HNSW_OK;
}

extern "C" {

int32_t hnsw_search_batch_h2d(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                              const hnsw_search_params *params, int32_t *d_ids, float *d_dist,
                              uint32_t *d_ndist, uint32_t *d_nhops, uint32_t *d_status, void *stream) {
    int rc = check_batch(idx, params, nq, q_stride, queries && d_ids && d_dist);
    if (rc) return rc;
    if (idx->n_deleted > 0) return marked_unsupported(idx, "hnsw_search_batch_h2d");
    if (nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    const size_t qbytes = query_bytes(nq, q_stride, idx->iv.d);
    if ((rc = idx->scratch.q.ensure(qbytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HostInput q;
    if ((rc = q.resolve(queries, qbytes, idx->scratch.q)) || (rc = q.upload(st))) return rc;
    // registered matrix: read by the device directly, the pre-pass (when there is one) leaves the device copy in sQ
    const float *dq = (const float *)q.dev;
    const bool cosine = is_cosine(idx);     // N(Q) from the matrix where it lies into the handle's scratch: the search reads that
    if (cosine) rc = cosine_queries(idx, dq, nq, q_stride, st, &dq, &q_stride);
    if (!rc)
        rc = knn_search(idx, params, {dq, nq, q_stride, d_ids, d_dist, d_ndist, d_nhops, d_status, nullptr},
                        st, q.from || cosine ? nullptr : (float *)idx->scratch.q.p);
    // the call returns while the device still reads the caller's matrix (in place, or as the source of the DMA above): the
    // range remembers it, so that hnsw_host_unregister / hnsw_host_free wait instead of pulling the pages from under a kernel
    range_reader_enqueued(queries, qbytes, st);
    return rc;
}

int32_t hnsw_search_submit(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                           const hnsw_search_params *params, hnsw_request **out) {
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    *out = nullptr;
    int rc = check_batch(idx, params, nq, q_stride, queries != nullptr);
    if (rc) return rc;
    if (idx->n_deleted > 0) return marked_unsupported(idx, "hnsw_search_submit");
    if (nq == 0) return fail(HNSW_ERR_BAD_ARG, "nq=0: nothing to submit");
    HIP_TRY(hipSetDevice(idx->device));
    hnsw_request *r;
    if (!idx->free_requests.empty()) { r = idx->free_requests.back(); idx->free_requests.pop_back(); }
    else { idx->all_requests.emplace_back(new hnsw_request()); r = idx->all_requests.back().get(); }
    auto give_back = [&](int code) { idx->free_requests.push_back(r); return code; };
    r->idx = idx; r->nq = nq; r->q_stride = q_stride; r->params = *params;
    r->stream = idx->next_stream; idx->next_stream = (idx->next_stream + 1) & 3;
    if (!idx->hs[r->stream] && hipStreamCreateWithFlags(&idx->hs[r->stream].h, hipStreamNonBlocking) != hipSuccess)
        return give_back(fail(HNSW_ERR_HIP, "hipStreamCreate failed"));
    const size_t qbytes = query_bytes(nq, q_stride, idx->iv.d);
    if ((rc = r->buf.ensure(nq, qbytes, params->k))) return give_back(rc);
    hipStream_t st = idx->hs[r->stream];
    const KnnBatch b = r->buf.batch(nq, q_stride, params->k);
    if (hipMemcpyAsync(r->buf.q.p, queries, qbytes, hipMemcpyHostToDevice, st) != hipSuccess)
        return give_back(fail(HNSW_ERR_HIP, "query upload failed"));
    range_reader_enqueued(queries, qbytes, st);    // page-locked source: the DMA above outlives this call (see hnsw_host_unregister)
    if (hipMemsetAsync(b.any_flag, 0, 4, st) != hipSuccess) return give_back(fail(HNSW_ERR_HIP, "hipMemsetAsync failed"));
    // COSINE: the request's own copy becomes N(Q) in place, so that hnsw_search_wait's repair reads what the search read
    if (is_cosine(idx) && (rc = cosine_normalise(b.Q, nq, idx->iv.d, q_stride, (float *)r->buf.q.p, q_stride, nullptr, nullptr, st)))
        return give_back(rc);
    if ((rc = knn_search(idx, params, b, st, nullptr, &r->refine))) return give_back(rc);
    // the results follow the search on the request's stream: hnsw_search_wait only has to wait for them
    idx->live_requests++;
    *out = r;
    return HNSW_OK;
}

int32_t hnsw_search_wait(hnsw_request *r, int32_t *out_ids, float *out_dist, uint32_t *out_ndist, uint32_t *out_nhops) {
    if (!r || !r->idx) return fail(HNSW_ERR_BAD_ARG, "null request");
    hnsw_index *idx = r->idx;
    // the request goes back to the pool only once its stream is idle, whatever failed: a later submit reuses its buffers
    auto done = [&](int code) { r->idx = nullptr; idx->live_requests--; idx->free_requests.push_back(r); return code; };
    if (!out_ids || !out_dist) {
        if (hipSetDevice(idx->device) == hipSuccess) (void)hipStreamSynchronize(idx->hs[r->stream]);
        return done(fail(HNSW_ERR_BAD_ARG, "null result buffers"));
    }
    if (hipSetDevice(idx->device) != hipSuccess) return done(fail(HNSW_ERR_HIP, "hipSetDevice failed"));
    hipStream_t st = idx->hs[r->stream];
    const int k = r->params.k;
    const KnnBatch b = r->buf.batch(r->nq, r->q_stride, k);
    // results and the "any query flagged" word in one go; the exactness fallback (as in hnsw_search_batch) only if set
    uint32_t flag = 0;
    hipError_t e = knn_download(b, k, out_ids, out_dist, out_ndist, out_nhops, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, b.any_flag, 4, hipMemcpyDeviceToHost, st);
    // synchronise whatever happened: copies already queued target the caller's arrays and `flag` (a stack word)
    { const hipError_t es = hipStreamSynchronize(st); if (e == hipSuccess) e = es; }
    if (e != hipSuccess) return done(fail(HNSW_ERR_HIP, "search failed: %s", hipGetErrorString(e)));
    if (!(flag & 1u)) return done(HNSW_OK);
    const int rc = knn_repair(idx, &r->params, b, st, &r->refine);
    if (rc) return done(rc);
    e = knn_download(b, k, out_ids, out_dist, out_ndist, out_nhops, st);
    { const hipError_t es = hipStreamSynchronize(st); if (e == hipSuccess) e = es; }
    if (e != hipSuccess) return done(fail(HNSW_ERR_HIP, "result download failed: %s", hipGetErrorString(e)));
    return done(HNSW_OK);
}

int32_t hnsw_host_register(void *p, int64_t bytes) {
    if (!p || bytes <= 0) return fail(HNSW_ERR_BAD_ARG, "hnsw_host_register: null buffer or bytes <= 0");
    const char *b = (const char *)p, *e_ = b + bytes;
    {   // this library's own list decides about overlaps (the runtime answers "success" for an array that merely STARTS
        // inside an existing registration and leaves the rest pageable: measured on ROCm 7.2)
        std::lock_guard<std::mutex> lk(g_ranges_mu);
        for (const HostRange &r : g_ranges) {
            if (b >= r.p && e_ <= r.p + r.bytes) return HNSW_OK;          // registered already: twice is not an error
            if (b < r.p + r.bytes && r.p < e_)
                return fail(HNSW_ERR_BAD_ARG, "hnsw_host_register: part of the %lld-byte array is registered already, the rest is not "
                            "(unregister the shorter range first)", (long long)bytes);
        }
    }
    auto locked = [](const void *q) {
        hipPointerAttribute_t a{};
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        return a.type == hipMemoryTypeHost;
    };
    hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        // Page-locked by somebody else -- registered (hipErrorHostMemoryAlreadyRegistered) or allocated page-locked (hipHostMalloc,
        // a torch pin_memory tensor: the runtime then answers "invalid argument") --: theirs to unpin.  Copies out of it run at
        // pinned speed anyway; the library neither maps it for direct access nor ever unregisters it.
        if (e == hipErrorHostMemoryAlreadyRegistered || (locked(b) && locked(e_ - 1))) {
            remember_range(p, (size_t)bytes, nullptr, RANGE_FOREIGN);
            return HNSW_OK;
        }
        return fail(HNSW_ERR_HIP, "hipHostRegister(%lld bytes) failed: %s", (long long)bytes, hipGetErrorString(e));
    }
    // "success" is believed only if every page answers as page-locked host memory (at most 4096 probes: the step grows with
    // the array) -- a foreign registration that covers only the array's beginning, or its two ends, leaves pageable pages
    // that a kernel's loads would fault on
    const size_t step = std::max<size_t>(4096, (((size_t)bytes / 4096) + 4095) / 4096 * 4096);
    bool whole = locked(e_ - 1);
    for (size_t o = 0; whole && o < (size_t)bytes; o += step) whole = locked(b + o);
    if (!whole) {
        if (hipHostUnregister(p) != hipSuccess) (void)hipGetLastError();
        return fail(HNSW_ERR_BAD_ARG, "hnsw_host_register: part of the %lld-byte array is registered already (by someone else), the rest is not",
                    (long long)bytes);
    }
    void *dev = nullptr;
    if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; }   // no mapping: copies only
    remember_range(p, (size_t)bytes, dev, RANGE_REGISTERED);
    return HNSW_OK;
}

int32_t hnsw_host_unregister(void *p) {
    if (!p) return fail(HNSW_ERR_BAD_ARG, "hnsw_host_unregister: null buffer");
    int kind = 0;
    {   // a block of hnsw_host_alloc is freed with hnsw_host_free, not unregistered
        std::lock_guard<std::mutex> lk(g_ranges_mu);
        for (const HostRange &r : g_ranges)
            if (r.p == (const char *)p && r.kind == RANGE_ALLOCATED) return fail(HNSW_ERR_BAD_ARG, "hnsw_host_unregister: this block came from hnsw_host_alloc (hnsw_host_free releases it)");
    }
    if (!retire_range(p, &kind))       // (waits for the asynchronous calls that still read the range)
        return fail(HNSW_ERR_BAD_ARG, "hnsw_host_unregister: no range registered through hnsw_host_register starts at %p", p);
    if (kind == RANGE_FOREIGN) return HNSW_OK;                 // not this library's registration to undo
    hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(HNSW_ERR_HIP, "hipHostUnregister failed: %s", hipGetErrorString(e)); }
    return HNSW_OK;
}

int32_t hnsw_host_alloc(void **out, int64_t bytes) {
    if (!out || bytes <= 0) return fail(HNSW_ERR_BAD_ARG, "hnsw_host_alloc: null out or bytes <= 0");
    *out = nullptr;
    void *p = nullptr, *dev = nullptr;
    hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocPortable | hipHostMallocMapped);
    if (e != hipSuccess) { (void)hipGetLastError(); return hip_fail(e, ("hipHostMalloc(" + std::to_string(bytes) + " bytes)").c_str()); }
    if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; }
    remember_range(p, (size_t)bytes, dev, RANGE_ALLOCATED);
    *out = p;
    return HNSW_OK;
}

int32_t hnsw_host_free(void *p) {
    if (!p) return HNSW_OK;
    int kind = 0;
    {
        std::lock_guard<std::mutex> lk(g_ranges_mu);
        bool mine = false;
        for (const HostRange &r : g_ranges) mine = mine || (r.p == (const char *)p && r.kind == RANGE_ALLOCATED);
        if (!mine) return fail(HNSW_ERR_BAD_ARG, "hnsw_host_free: %p is not a block of hnsw_host_alloc", p);
    }
    (void)retire_range(p, &kind);      // (waits for the asynchronous calls that still read the block)
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(HNSW_ERR_HIP, "hipHostFree failed: %s", hipGetErrorString(e)); }
    return HNSW_OK;
}

int32_t hnsw_knn(hnsw_index *idx, const float *query, const hnsw_search_params *params,
                 int32_t *out_ids, float *out_dist, int32_t *out_count) {
    if (!idx || !query) return fail(HNSW_ERR_BAD_ARG, "null argument");
    int rc = hnsw_search_batch(idx, query, 1, idx->iv.d, params, out_ids, out_dist, nullptr, nullptr);
    if (rc) return rc;
    if (out_count) {
        int c = 0;
        while (c < params->k && out_ids[c] >= idx->iv.id_base) ++c;
        *out_count = c;
    }
    return HNSW_OK;
}

int32_t hnsw_distance_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride,
                                   const int32_t *d_ids, int32_t m, float *d_out, void *stream) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (nq == 0 || m == 0) return HNSW_OK;
    if (nq < 0 || m < 0 || !d_queries || !d_ids || !d_out) return fail(HNSW_ERR_BAD_ARG, "bad buffers");
    if (q_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "q_stride < d");
    HIP_TRY(hipSetDevice(idx->device));
    // (COSINE: N(Q) first, here for the host form too, which uploads its matrix and calls this one)
    const int rc = cosine_queries(idx, d_queries, nq, q_stride, (hipStream_t)stream, &d_queries, &q_stride);
    if (rc) return rc;
    const hipError_t e = launch_distance(idx, d_queries, q_stride, nq, d_ids, m, d_out, (hipStream_t)stream);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "distance kernel launch failed: %s", hipGetErrorString(e));
    return HNSW_OK;
}

int32_t hnsw_distance_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride,
                            const int32_t *ids, int32_t m, float *out) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (nq == 0 || m == 0) return HNSW_OK;
    if (nq < 0 || m < 0 || !queries || !ids || !out) return fail(HNSW_ERR_BAD_ARG, "bad buffers");
    for (int64_t i = 0; i < nq * m; ++i) {
        const int64_t v = (int64_t)ids[i] - idx->iv.id_base;
        if (v < 0 || v >= idx->iv.n) return fail(HNSW_ERR_BAD_ARG, "Vector.get: id out of range");
    }
    HIP_TRY(hipSetDevice(idx->device));
    int rc;
    const size_t qbytes = query_bytes(nq, q_stride, idx->iv.d);
    if ((rc = idx->scratch.q.ensure(qbytes)) || (rc = idx->scratch.ids.ensure((size_t)nq * m * 4)) || (rc = idx->scratch.dist.ensure((size_t)nq * m * 4))) return rc;
    HIP_TRY(hipMemcpy(idx->scratch.q.p, queries, qbytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(idx->scratch.ids.p, ids, (size_t)nq * m * 4, hipMemcpyHostToDevice));
    rc = hnsw_distance_batch_device(idx, (const float *)idx->scratch.q.p, nq, q_stride, (const int32_t *)idx->scratch.ids.p, m, (float *)idx->scratch.dist.p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, idx->scratch.dist.p, (size_t)nq * m * 4, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

} // extern "C"
