// hnsw_scan_matrix_device.hip.h -- what the two kernels that screen float rows with fp32 matrix instructions share (option
// "scan_matrix": the k-scan, hnsw_scan_matrix.hip, and the range scan, hnsw_range_matrix.hip): the accumulator type, the tile's load,
// the walk over the 32-row blocks of one (tile, slab) wave -- from the first block to the survivors' row numbers in the queries'
// buffers -- and the exact evaluation of a pair the screen could not drop: the float scan's own arithmetic, so the key is its key.
// What a full buffer's rows become is the caller's business; the lane maps and the pipeline are here once.
#pragma once
#include "hnsw_scan_device.hip.h"
#include "hnsw_scan_matrix_plan.h"

namespace hnsw_dev {

typedef float v16f __attribute__((ext_vector_type(16)));

// The tile, once per workgroup of W waves: the tq queries from q0 on as float32 at pitch scan_matrix_pitch(NCH), zero beyond d and
// beyond the tile's last query.  (The caller's workgroup barrier follows.)
template <int NCH, int W>
__device__ __forceinline__ void scan_matrix_load_tile(float *tile, const float *Q, int64_t q_stride, int64_t q0, int tq, int d) {
    constexpr int T = hnsw_host::SCAN_MATRIX_TILE, KW = hnsw_host::scan_matrix_width(NCH), PITCH = hnsw_host::scan_matrix_pitch(NCH);
    for (int c = threadIdx.x; c < T * (KW / 4); c += 64 * W) {
        const int t = c / (KW / 4), e0 = 4 * (c % (KW / 4));
        const float *qp = Q + (q0 + (t < tq ? t : 0)) * q_stride;
        float4 v;
        v.x = (t < tq && e0 + 0 < d) ? qp[e0 + 0] : 0.f; v.y = (t < tq && e0 + 1 < d) ? qp[e0 + 1] : 0.f;
        v.z = (t < tq && e0 + 2 < d) ? qp[e0 + 2] : 0.f; v.w = (t < tq && e0 + 3 < d) ? qp[e0 + 3] : 0.f;
        *reinterpret_cast<float4 *>(tile + t * PITCH + e0) = v;
    }
}

// The exact key of (row, the query whose chunks lie at qrow in the tile), by one 16-lane group: scan_slab's arithmetic -- lane l16 on
// the chunks l16, l16 + 16, ..., zero beyond the row's end, the fmaf chain, the tree.
template <int NCH, int METRIC>
__device__ __forceinline__ uint32_t scan_matrix_exact_key(const float *rp, int nchunks, const float *qrow, int l16) {
    float4 z[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = i * 16 + l16;
        z[i] = *reinterpret_cast<const float4 *>(rp + 4 * (c < nchunks ? c : 0));
    }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = i * 16 + l16;
        if (c >= nchunks) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc = scan_chain<METRIC>(acc, z[i], *reinterpret_cast<const float4 *>(qrow + 4 * c));
    }
    return dist_to_key<METRIC>(reduce16(acc));
}

// One wave, the rows [r0, r1) of its slab (rows of X, `stride` floats apart, nchunks float4 of real dimensions each) against the tq
// queries of its tile, v_mfma_f32_32x32x2_f32.
//   B operand: the tile in LDS (scan_matrix_load_tile), shared by the workgroup's waves; the row pitch is padded by 4 floats so that
//     the lanes of one ds_read_b128 pass spread over the banks.
//   A operand: a block of 32 rows (aligned to 32, so that it is one mask word) straight from global memory, float4 per lane: lane
//     (j = l % 32, h = l / 32) holds floats [8 s + 4 h, + 4) of row base + j at step s and reads the same floats of query j from the
//     tile; component c of the pair feeds one matrix instruction (k = 8 s + c and 8 s + 4 + c: which k a register stands for does
//     not matter, both operands use one map and the sum is over all k).  One load, four instructions.
//   Pipeline: a stage is a block's piece of scan_matrix_piece(NCH) floats per row (32 or 64 VGPRs); the next stage's loads -- the
//     block's next piece or the next candidate block's first -- are in flight while this one is multiplied; a block whose mask word
//     (cut to the slab) has no set bit is stepped over unloaded.  16 accumulators.
//   Row norms: fma over the lane's floats of the operand registers and one cross-half exchange; they reach the accumulator layout
//     (lane l: query l % 32, rows 8 g + 4 (l / 32) + c of the block) through the wave's 128 bytes of LDS at rterm (16-byte aligned).
//     No table of norms exists: insert, remove, upsert and compact have nothing to maintain.  A masked or out-of-slab row's term
//     is +inf: above every bound.
//   Screen: one multiply-add (L2) or subtract (IP) and one compare per accumulator against the lane's `bound`, which the caller
//     owns and may change in settled().  Survivors go, as bare row numbers, into their query's buffer bufs[j] (BUF words, cnt[j] of
//     them in use; a row of the block survives once per query, so a buffer that holds at most BUF - 32 takes one more block).
//   After a block that left buffers fuller than that: full(t, c) for each such query t and its c words -- it must leave cnt[t] at 0
//     -- then, once, settled().  What is left in the buffers at the slab's end is the caller's.
template <int NCH, int METRIC, bool MASKED, class E, int BUF, class Full, class Settled>
__device__ __forceinline__ void scan_matrix_walk(const float *X, int64_t stride, int nchunks, float eps, int64_t r0, int64_t r1, const MaskWords &mask,
                                                 const float *tile, float *rterm, E (*bufs)[BUF], int *cnt, int tq, const float &bound,
                                                 Full &&full, Settled &&settled) {
    using namespace hnsw_host;      // the plan header's constants and the rule
    constexpr int PITCH = scan_matrix_pitch(NCH);
    constexpr int PF = scan_matrix_piece(NCH), SP = PF / 8;     // floats of a row per stage; steps (float4 per lane) per stage
    constexpr int LIMIT = BUF - 32;                             // a buffer up to here takes the survivors of one more block
    static_assert(NCH == 1 || NCH == 2 || NCH == 4 || NCH == 8, "rows of 64 to 512 floats");
    const int lane = threadIdx.x & 63;
    const int j = lane & 31, h = lane >> 5;     // the lane's query column (and row of the A operand); which half of a step's k range
    const int np = (4 * nchunks + PF - 1) / PF;                 // stages per block: the pieces that hold a real dimension

    // the rows of the 32-row block at `base` that may be candidates: in the slab, and allowed (wave-uniform)
    auto candidates = [&](int64_t base) -> uint32_t {
        const int lo = r0 > base ? (int)(r0 - base) : 0;
        const int64_t left = r1 - base;
        uint32_t w = (left >= 32 ? ~0u : ((1u << (int)left) - 1u)) & (~0u << lo);
        if constexpr (MASKED) w &= (uint32_t)uniform((int)mask[base >> 5]);
        return w;
    };
    // piece p of row base + j, the lane's float4 per step; the row clamped into the slab (a clamped row is no candidate) and a chunk
    // past the row's end clamped to its first (zeroed before use)
    auto load = [&](float4 (&x)[SP], int64_t base, int p) {
        int64_t row = base + j;
        row = row < r0 ? r0 : row;
        row = row < r1 ? row : r1 - 1;
        const float *rp = X + (uint64_t)row * (uint64_t)stride;
#pragma unroll
        for (int s = 0; s < SP; ++s) {
            const int c = 2 * (SP * p + s) + h;
            x[s] = *reinterpret_cast<const float4 *>(rp + 4 * (c < nchunks ? c : 0));
        }
    };

    int64_t base = r0 & ~31ll;
    uint32_t vw = 0;
    while (base < r1 && (vw = candidates(base)) == 0u) base += 32;
    float4 an[SP];
    if (base < r1) load(an, base, 0);
    while (base < r1) {
        const int64_t cur = base;
        const uint32_t cw = vw;
        v16f acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float nx = 0.f;
        for (int p = 0; p < np; ++p) {
            float4 ax[SP];
#pragma unroll
            for (int s = 0; s < SP; ++s) ax[s] = an[s];
            if (p + 1 < np) load(an, cur, p + 1);
            else {
                base += 32;
                while (base < r1 && (vw = candidates(base)) == 0u) base += 32;
                if (base < r1) load(an, base, 0);
            }
            if (p == np - 1) {                  // only the last piece reaches past the row's end
#pragma unroll
                for (int s = 0; s < SP; ++s) if (2 * (SP * p + s) + h >= nchunks) ax[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            const float *bp = tile + j * PITCH + PF * p + 4 * h;
#pragma unroll
            for (int s = 0; s < SP; ++s) {
                const float4 b = *reinterpret_cast<const float4 *>(bp + 8 * s);
                nx = __builtin_fmaf(ax[s].x, ax[s].x, nx); nx = __builtin_fmaf(ax[s].y, ax[s].y, nx);
                nx = __builtin_fmaf(ax[s].z, ax[s].z, nx); nx = __builtin_fmaf(ax[s].w, ax[s].w, nx);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[s].x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[s].y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[s].z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[s].w, b.w, acc, 0, 0, 0);
            }
        }

        nx += __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __float_as_int(nx)));   // the other half of the row
        float rt = scan_matrix_row_term(METRIC, nx, eps);
        if (!((cw >> j) & 1u)) rt = __builtin_inff();           // no candidate: above every bound
        if (h == 0) rterm[j] = rt;
        scan_lds_sync();

        // accumulator v of the lane: row 8 (v / 4) + 4 h + v % 4 of the block, query j
        float tv[16];
        bool any = false;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 rr = *reinterpret_cast<const float4 *>(rterm + 8 * g + 4 * h);
            tv[4 * g + 0] = scan_matrix_value(METRIC, rr.x, acc[4 * g + 0]);
            tv[4 * g + 1] = scan_matrix_value(METRIC, rr.y, acc[4 * g + 1]);
            tv[4 * g + 2] = scan_matrix_value(METRIC, rr.z, acc[4 * g + 2]);
            tv[4 * g + 3] = scan_matrix_value(METRIC, rr.w, acc[4 * g + 3]);
#pragma unroll
            for (int c = 0; c < 4; ++c) any = any || scan_matrix_survives(tv[4 * g + c], bound);
        }
        if (ballot(any)) {                      // rare once the lists are full, or on a selective radius
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int ri = 8 * (v >> 2) + 4 * h + (v & 3);
                if (scan_matrix_survives(tv[v], bound) && ((cw >> ri) & 1u) && j < tq) bufs[j][atomicAdd(&cnt[j], 1)] = (uint32_t)(cur + ri);
            }
            scan_wave_sync();
            const int c = cnt[j];               // (at most LIMIT + 32 = BUF: a row of the block survives once per query)
            uint32_t need = (uint32_t)ballot(h == 0 && c > LIMIT);
            if (need) {
                while (need) {
                    const int t = __builtin_ctz(need);
                    need &= need - 1u;
                    full(t, __builtin_amdgcn_readlane(c, t));
                }
                scan_wave_sync();
                settled();
            }
        }
    }
}

} // namespace hnsw_dev
