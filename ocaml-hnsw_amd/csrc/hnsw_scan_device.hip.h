// hnsw_scan_device.hip.h -- the one body of the exact scans: the k-scan and its masked form (hnsw_scan.hip), the range scan's
// two passes (hnsw_range.hip), the grouped scan (hnsw_group.hip) and the paged scan (hnsw_after.hip).  scan_slab walks the rows of one (tile, slab) wave and hands the key of every (row, query) pair to
// a selection policy; what is kept of them is the policy's business, the arithmetic is here once: the lane grid, the fmaf chain,
// the reduce16 tree and dist_to_key of every other kernel, so the keys are the bits of hnsw_distance_batch.
#pragma once
#include "hnsw_device.hip.h"

namespace hnsw_dev {

constexpr int SCAN_WAVES = 4;          // waves per workgroup, one slab each
// queries per tile: T * NCH * 4 VGPRs hold them for NCH <= 4 (64 at most); through LDS the tile costs T * NCH * 256 bytes
__host__ __device__ constexpr int scan_tile(int nch) { return nch <= 2 ? 8 : nch == 4 ? 4 : 8; }
// batches of four rows in flight per wave: UB * NCH * 4 VGPRs
__host__ __device__ constexpr int scan_rows(int nch) { return nch == 1 ? 4 : nch <= 4 ? 2 : 1; }
// waves per SIMD the register allocator must leave room for: a floor, not the count a kernel gets (NCH 16 holds 3 where its LDS
// allows them: profiles/scan_family_resources.txt)
__host__ __device__ constexpr int scan_min_waves(int nch) { return nch == 1 || nch == 8 ? 4 : nch == 16 ? 2 : 3; }

// Grid: (query tiles) x (groups of SCAN_WAVES row slabs), one wave per (tile, slab); slab s = rows [s * slab_rows, min(n, (s + 1)
// * slab_rows)).  A wave keeps the chunks of the T queries of its tile in registers (NCH <= 4) or shares them with the other
// waves of its workgroup through LDS (NCH >= 8, as hnsw_distance_kernel does) and walks its rows in id order, 4 * UB rows in
// flight: one 16-lane group per row, lane l16 on the float4 chunks l16, l16 + 16, ...  Every row chunk loaded is used for all T
// queries.  The workgroups of one slab group are consecutive in dispatch order (blockIdx.x is the tile), so the rows of a slab are
// fetched from HBM once per XCD and otherwise come out of L2.
// Select, with q0 the tile's first query and tq (>= 1: the grid has no empty tile) how many it has:
//   begin(q0, tq, slab)        once, before the first row
//   skip(base)                 wave-uniform: the 32 rows of base's mask word hold no candidate and are stepped over unloaded
//   admits(row, in_slab)       once per row: may it be a candidate (in_slab: the row is one of the slab's, not the clamped repeat)
//   take(t, key, row, ok)      the key of (row, query t of the tile), ok = what admits said; the 16 lanes of a row agree on key
//   batch_end()                after the 4 * UB rows of one pass
//   end()                      after the last row
template <int NCH, int METRIC, class Select>
__device__ __forceinline__ void scan_slab(const IndexView &iv, const float *Q, int64_t q_stride, int64_t nq, int32_t n_slabs, int64_t slab_rows,
                                          Select &sel) {
    constexpr int T = scan_tile(NCH), UB = scan_rows(NCH);
    constexpr bool QLDS = NCH >= 8;
    __shared__ float4 qs[QLDS ? T * 16 * NCH : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane >> 4, l16 = lane & 15;
    const int64_t q0 = (int64_t)blockIdx.x * T;
    const int tq = (int)(nq - q0 < T ? nq - q0 : T);

    float4 qv[QLDS ? 1 : T][QLDS ? 1 : NCH];
    if constexpr (QLDS) {       // the workgroup loads the tile once, zero beyond d and beyond the tile's last query
        for (int c = threadIdx.x; c < T * 16 * NCH; c += 64 * SCAN_WAVES) {
            const int t = c / (16 * NCH), e0 = 4 * (c % (16 * NCH));
            const float *qp = Q + (q0 + (t < tq ? t : 0)) * q_stride;
            float4 v;
            v.x = (t < tq && e0 + 0 < iv.d) ? qp[e0 + 0] : 0.f; v.y = (t < tq && e0 + 1 < iv.d) ? qp[e0 + 1] : 0.f;
            v.z = (t < tq && e0 + 2 < iv.d) ? qp[e0 + 2] : 0.f; v.w = (t < tq && e0 + 3 < iv.d) ? qp[e0 + 3] : 0.f;
            qs[c] = v;
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int t = 0; t < T; ++t) load_query<NCH>(qv[t], Q + (q0 + (t < tq ? t : 0)) * q_stride, iv.d, l16);
    }
    const int64_t slab = (int64_t)blockIdx.y * SCAN_WAVES + uniform(wave);      // (said to be the same in all lanes: the row loop, its
                                                                                    // bounds and a skipped mask word then cost scalar registers only)
    if (slab >= n_slabs) return;                    // (after the only workgroup barrier)
    const int64_t r0 = slab * slab_rows, r1 = r0 + slab_rows < iv.n ? r0 + slab_rows : iv.n;
    sel.begin(q0, tq, slab);

    const uint32_t stride_b = (uint32_t)iv.stride * 4u;
    for (int64_t base = r0; base < r1; base += 4 * UB) {
        if (sel.skip(base)) { base = (base | 31) + 1 - 4 * UB; continue; }
        float4 v[UB][NCH];
#pragma unroll
        for (int u = 0; u < UB; ++u) {              // past the slab's end: its last row again, dropped below
            const int64_t row = base + 4 * u + r;
            const char *rp = reinterpret_cast<const char *>(iv.X) + (uint64_t)(row < r1 ? row : r1 - 1) * stride_b;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = i * 16 + l16;
                v[u][i] = *reinterpret_cast<const float4 *>(rp + 16u * (uint32_t)(c < iv.nchunks ? c : 0));
            }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {         // lanes past the row end add exactly 0 (their query chunk is 0)
                // (an assignment under a test, not a select per component: as selects the counting pass of the range scan takes 84
                // VGPRs for 67 at NCH 1, five waves per SIMD for seven; with the loop still on vector registers that cost 6 % at d 32)
                if ((i * 16 + l16) >= iv.nchunks) v[u][i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            const int64_t row = base + 4 * u + r;
            const bool ok = sel.admits(row, row < r1);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                // (the tile in LDS is read here, every time: left alone the compiler hoists T * NCH float4 reads out of the loops)
                if constexpr (QLDS) asm volatile("" ::: "memory");
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const float4 z = v[u][i];
                    const float4 qi = QLDS ? qs[(t * NCH + i) * 16 + l16] : qv[QLDS ? 0 : t][QLDS ? 0 : i];
                    if (METRIC == 0) {
                        float dx = z.x - qi.x; acc = __builtin_fmaf(dx, dx, acc);
                        float dy = z.y - qi.y; acc = __builtin_fmaf(dy, dy, acc);
                        float dz = z.z - qi.z; acc = __builtin_fmaf(dz, dz, acc);
                        float dw = z.w - qi.w; acc = __builtin_fmaf(dw, dw, acc);
                    } else {
                        acc = __builtin_fmaf(z.x, qi.x, acc);
                        acc = __builtin_fmaf(z.y, qi.y, acc);
                        acc = __builtin_fmaf(z.z, qi.z, acc);
                        acc = __builtin_fmaf(z.w, qi.w, acc);
                    }
                }
                sel.take(t, dist_to_key<METRIC>(reduce16(acc)), row, ok);
            }
        }
        sel.batch_end();
    }
    sel.end();
}

// The mask members of every selection policy (ScanTopK, ScanAfter, ScanGroupBest, RangeHits), as a base.  MASKED: `mask` holds one
// bit per row, bit row & 31 of word row >> 5, ceil(n / 32) words; a row whose bit is clear is no candidate, and a 32-row word
// without a set bit is stepped over without loading its rows.  The unmasked form holds nothing: its kernels are what they would be
// if there were no masks.
template <bool MASKED> struct ScanMask {
    MaskWords mask;
    __device__ __forceinline__ explicit ScanMask(const uint32_t *mask_) : mask(mask_words(mask_)) {}
    __device__ __forceinline__ bool skip(int64_t base) const { return uniform((int)mask[base >> 5]) == 0; }
    __device__ __forceinline__ bool admits(int64_t row, bool in_slab) const { return in_slab && ((mask[row >> 5] >> (row & 31)) & 1u); }
};
template <> struct ScanMask<false> {
    __device__ __forceinline__ explicit ScanMask(const uint32_t *) {}
    __device__ __forceinline__ bool skip(int64_t) const { return false; }
    __device__ __forceinline__ bool admits(int64_t, bool in_slab) const { return in_slab; }
};

// ---- what the scans that keep the k smallest words per (query, slab) share (ScanTopK, hnsw_scan.hip; ScanAfter, hnsw_after.hip) ----

constexpr int SCAN_BUF = 64;           // survivor words per query and wave (LDS)
constexpr uint64_t SCAN_EMPTY = ~0ull; // no candidate: above every real word

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

} // namespace hnsw_dev
