// hnsw_range_bytes.hip -- the exact range scan of byte-valued data through 8-bit matrix instructions (option "scan_bytes" 2): both
// passes of hnsw_range.hip's scan, plain and masked, over the byte rows (tables.X8), the way hnsw_scan_bytes.hip serves the k-scan.
//
// Byte rows against byte-valued queries at d <= 256: every sum is an integer below 2^24, the float range scan's sum IS that integer,
// and here the matrix unit makes it.  So -- unlike the float screen of hnsw_range_matrix.hip -- the matrix unit makes the key itself:
// no survivor buffer, no exact re-evaluation.  And unlike the byte k-scan there are no lists, no buffers and no scan_flush: the bound
// is one integer per lane, fixed from the slab's first row on.  Every (query, slab) cell holds the float range scan's count and its
// words; the exclusive sums, range_count_kernel, the segmented sort and range_unpack_kernel around it are untouched.
//
//   hnsw_range_scan_bytes_kernel<NCH, METRIC, PASS, MASKED>: grid (tiles of 32 queries) x (groups of RANGE_BYTES_WAVES slabs), one
//     wave per (tile, slab); the slabs are the float range scan's (ExactPlan), so a cell is a cell.  Returns at once unless the path
//     word is 2 (the float range kernels, launched behind it into the same cells, return unless it is 1).
//     Operands, pipeline, row terms: the byte k-scan's (hnsw_scan_bytes.hip has the lane maps and the algebra), restated here:
//       through one shared walk the k-scan's NCH 2 instances ran 2 to 4 % slower (profiles/scan_walk_refactor.txt) -- 32-row blocks
//       aligned to a mask word straight from
//       tables.X8, lane l on 16 contiguous bytes of row l % 32 per step, x xor 0x80 as the A operand; the tile's codes in 8 NCH
//       registers as B for the whole slab; v_mfma_i32_32x32x32_i8; the next candidate block's loads in flight during the multiply;
//       row terms from the raw registers by v_dot4_u32_u8, one ds_bpermute across the halves, 128 bytes of LDS into the accumulator
//       layout (lane l: query l % 32, rows 8 g + 4 (l / 32) + c of the block).  No per-row table.  That LDS is all a wave has: four
//       waves per workgroup, occupancy set by registers.
//     Bound: the hits of a query are the integers m (L2: the squared distance, IP: minus the inner product) whose key lies in
//       [klo, khi] (range_key_bounds).  The key is monotone in m, so they are the m <= M; M is found once per wave by bisection on
//       the keys (range_bytes_bound, hnsw_scan_bytes_plan.h), and the lane's bound is M less its query's term.  One subtract and one
//       compare per accumulator.  A row that is no candidate (outside the slab, masked out, a clamped repeat) carries a row term
//       above every bound; a query column past the tile's end, and every column when no key is in range, a bound below every value.
//     PASS 0: a lane counts its column's hits in a register; the two halves of a column are added once, at the slab's end, and the
//       sum goes to counts[(q0 + j) n_slabs + slab].  No LDS traffic beside the row terms.
//     PASS 1: a hit's word is dist_to_key((float)integer) << 32 | row, the byte k-scan's key.  The two lanes of a column exchange
//       their hit counts of the block (one ds_bpermute, only in a block with a hit): the lower half writes first, the upper half
//       behind it, at the cell's offset plus the column's running count, guarded by the cell's PASS-0 count as RangeHits guards it.
//       The order inside a cell is not id order; the words are distinct and the segmented sort orders every segment afterwards.
//       Vector stores only.
#include "hnsw_internal.h"
#include "hnsw_scan_device.hip.h"

namespace hnsw_dev {

using namespace hnsw_host;      // the plan header's constants and the bound

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

struct RangeBytesArgs {
    const uint8_t *X8;     // [n][64 * NCH] byte rows
    int64_t n;
    const uint8_t *codes;  // [nq][64 * NCH] the queries of this launch, as the prepass wrote them
    const int32_t *terms;  // [nq]
    const uint32_t *path;  // the handle's path word
    RangeScanArgs r;       // the pass's queries, cut, radius and cells: what the float range kernels get
};

template <int NCH, int METRIC, int PASS, bool MASKED>
__global__ void __launch_bounds__(64 * RANGE_BYTES_WAVES)
hnsw_range_scan_bytes_kernel(const RangeBytesArgs a, const uint32_t *mask_) {
    constexpr int S = 2 * NCH;                  // matrix instructions per block: 32 bytes of every row each
    constexpr int RB = 64 * NCH;                // bytes per row and per query's codes
    constexpr int T = SCAN_BYTES_TILE;
    static_assert(NCH == 1 || NCH == 2 || NCH == 4, "rows of 64, 128 or 256 bytes");
    static_assert(T == 32, "a tile is the N of one 32x32x32 matrix instruction");
    __shared__ __attribute__((aligned(16))) int rterm_all[RANGE_BYTES_WAVES][32];
    if (*a.path != (uint32_t)SCAN_PATH_BYTES) return;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;     // the lane's query column (and row of the A operand); which half of the k range
    const int64_t q0 = (int64_t)blockIdx.x * T;
    const int tq = (int)(a.r.nq - q0 < T ? a.r.nq - q0 : T);
    const int64_t slab = (int64_t)blockIdx.y * RANGE_BYTES_WAVES + uniform(wave);
    if (slab >= a.r.n_slabs) return;            // (no workgroup barrier anywhere)
    const int64_t r0 = slab * a.r.slab_rows, r1 = r0 + a.r.slab_rows < a.n ? r0 + a.r.slab_rows : a.n;
    const MaskWords mask = mask_words(MASKED ? mask_ : nullptr);
    int *const rterm = rterm_all[wave];
    const int jq = j < tq ? j : tq - 1;         // a query column past the tile's end reads the last one's and never has a hit

    // the key interval of the radius and the largest integer inside it, once per wave
    uint32_t klo, khi;
    range_key_bounds<METRIC>(a.r.radius, klo, khi);
    int32_t top = 0;
    const bool some = uniform((int)range_bytes_bound(METRIC, (uint32_t)uniform((int)klo), (uint32_t)uniform((int)khi), &top)) != 0;
    uint64_t *const cell_count = a.r.counts + (q0 + jq) * a.r.n_slabs + slab;
    if (!some) {                                // no key is in range
        if (PASS == 0 && h == 0 && j < tq) *cell_count = 0ull;
        return;
    }
    const int cq = a.terms[q0 + jq];
    const int bound = j < tq ? uniform(top) - cq : RANGE_BYTES_NO_HIT;      // fixed for the whole slab
    // the column's hits in this cell so far (PASS 0: this lane's half of them); PASS 1: where its words go, how many PASS 0 counted
    int hits = 0, lim = 0;
    uint64_t *out = a.r.words;
    if (PASS == 1) {
        const int64_t at = (q0 + jq) * a.r.n_slabs;
        out += a.r.xoff[q0 + jq] + (int64_t)(a.r.offs[at + slab] - a.r.offs[at]);
        lim = (int)(a.r.offs[at + slab + 1] - a.r.offs[at + slab]);
    }
    // the tile's codes: B for the whole slab
    v4i b[S];
    {
        const uint8_t *qp = a.codes + (q0 + jq) * RB + 16 * h;
#pragma unroll
        for (int s = 0; s < S; ++s) b[s] = *reinterpret_cast<const v4i *>(qp + 32 * s);
    }

    // the rows of the 32-row block at `base` that may be candidates: in the slab, and allowed (wave-uniform)
    auto candidates = [&](int64_t base) -> uint32_t {
        const int lo = r0 > base ? (int)(r0 - base) : 0;
        const int64_t left = r1 - base;
        uint32_t w = (left >= 32 ? ~0u : ((1u << (int)left) - 1u)) & (~0u << lo);
        if constexpr (MASKED) w &= (uint32_t)uniform((int)mask[base >> 5]);
        return w;
    };
    // the lane's 16 bytes per step of row base + j, clamped into the slab (a clamped row is no candidate)
    auto load = [&](v4i (&x)[S], int64_t base) {
        int64_t row = base + j;
        row = row < r0 ? r0 : row;
        row = row < r1 ? row : r1 - 1;
        const uint8_t *rp = a.X8 + (uint64_t)row * RB + 16 * h;
#pragma unroll
        for (int s = 0; s < S; ++s) x[s] = *reinterpret_cast<const v4i *>(rp + 32 * s);
    };

    int64_t base = r0 & ~31ll;
    uint32_t vw = 0;
    while (base < r1 && (vw = candidates(base)) == 0u) base += 32;
    v4i an[S];
    if (base < r1) load(an, base);
    while (base < r1) {
        const int64_t cur = base;
        const uint32_t cw = vw;
        // the operand, and the lane's part of the row's term from the raw bytes
        v4i ax[S];
        uint32_t s1 = 0, s2 = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t u = (uint32_t)an[s][c];
                s1 = __builtin_amdgcn_udot4(u, 0x01010101u, s1, false);
                if (METRIC == 0) s2 = __builtin_amdgcn_udot4(u, u, s2, false);
                ax[s][c] = (int)(u ^ 0x80808080u);
            }
        }
        base += 32;
        while (base < r1 && (vw = candidates(base)) == 0u) base += 32;
        if (base < r1) load(an, base);

        int rt = METRIC == 0 ? (int)s2 - 256 * (int)s1 : -128 * (int)s1;
        rt += __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, rt);      // the other half of the row
        if (!((cw >> j) & 1u)) rt = SCAN_BYTES_NO_ROW;                  // no candidate: above every bound
        if (h == 0) rterm[j] = rt;
        scan_lds_sync();

        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < S; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ax[s], b[s], acc, 0, 0, 0);

        // accumulator v of the lane: row 8 (v / 4) + 4 h + v % 4 of the block, query j
        int tv[16];
        int nb = 0;                             // the lane's hits in this block
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4i rr = *reinterpret_cast<const v4i *>(rterm + 8 * g + 4 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int v = 4 * g + c;
                tv[v] = METRIC == 0 ? rr[c] - 2 * acc[v] : rr[c] - acc[v];
                nb += tv[v] <= bound ? 1 : 0;
            }
        }
        if (PASS == 0) {
            hits += nb;
        } else if (ballot(nb != 0)) {           // rare on a selective radius
            const int other = __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, nb);
            int pos = hits + (h ? other : 0);   // the lower half of the column writes first
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                if (tv[v] <= bound) {
                    const int m = tv[v] + cq;
                    const float sum = METRIC == 0 ? (float)m : (float)(-m);
                    if (pos < lim) out[pos] = ((uint64_t)dist_to_key<METRIC>(sum) << 32) | (uint32_t)(cur + 8 * (v >> 2) + 4 * h + (v & 3));
                    ++pos;
                }
            }
            hits += nb + other;
        }
    }
    if (PASS == 0) {
        hits += __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, hits);
        if (h == 0 && j < tq) *cell_count = (uint64_t)hits;
    }
}

} // namespace hnsw_dev

namespace hnsw_host {

int range_bytes_launch(hnsw_index *idx, int pass, int nch, const hnsw_dev::RangeScanArgs &r, const uint32_t *mask, hipStream_t st, const uint32_t **path) {
    const int d = idx->iv.d;
    // PASS 1 follows the PASS 0 of the same queries on the same stream: their codes, their terms and the path word are still in place
    const uint8_t *codes = (const uint8_t *)idx->scratch.scan_codes.p;
    const int32_t *terms = codes ? (const int32_t *)(codes + scan_bytes_scratch(r.nq, d).terms_at) : nullptr;
    const uint32_t *state = (const uint32_t *)idx->scratch.scan_state.p;
    int rc;
    if (pass == 0 && (rc = scan_bytes_prepass(idx, r.Q, r.q_stride, r.nq, st, &codes, &terms, &state))) return rc;
    if (!codes || !state || 64 * nch != scan_bytes_row_bytes(d) || idx->scratch.scan_codes.bytes < (size_t)scan_bytes_scratch(r.nq, d).total)
        return fail(HNSW_ERR_HIP, "byte range scan: pass %d without its prepass (d=%d)", pass, d);
    const hnsw_dev::RangeBytesArgs a{(const uint8_t *)idx->tables.X8.p, idx->iv.n, codes, terms, state, r};
    const dim3 grid((unsigned)scan_bytes_tiles(r.nq), (unsigned)range_bytes_slab_groups(r.n_slabs)), block(64 * RANGE_BYTES_WAVES);
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) { with_range_pass(pass, mask != nullptr, [&](auto PASS, auto MASKED) {
        if constexpr (NCH <= 4) hipLaunchKernelGGL((hnsw_dev::hnsw_range_scan_bytes_kernel<NCH, METRIC, PASS, MASKED>), grid, block, 0, st, a, mask);
    }); }); });
    if ((rc = launched("byte range scan kernel"))) return rc;
    *path = state;
    return HNSW_OK;
}

} // namespace hnsw_host
