// hnsw_scan_bytes.hip -- the exact k-nearest scan of byte-valued data through 8-bit matrix instructions (option "scan_bytes").
//
// Byte rows (tables.X8, hnsw_rows8.hip) against byte-valued queries, d <= 256: every product and every partial sum is an integer
// below 2^24, so the float scan's fmaf chain (hnsw_scan_device.hip.h) never rounds and its sum is THE integer sum.  This file
// computes that integer with v_mfma_i32_32x32x32_i8 and hands dist_to_key the same float: same keys, same lists, same results.
//
// Two kernels in front of the unchanged hnsw_scan_merge_kernel.
//   hnsw_scan_bytes_queries_kernel<METRIC>: one wave per query.  Writes the query's codes q' = q - 128 as int8 in the byte-row
//     layout (64 * NCH bytes, ZERO beyond d), its integer term (below), and -- the last wave to finish -- the handle's path word:
//     2 when every value of the launch's queries is an integer in 0..255 (-0.0 counts as 0), else 1.  The range scan's byte kernels
//     (hnsw_range_bytes.hip; option value 2) take their codes, terms and path word from the same prepass (scan_bytes_prepass).
//   hnsw_scan_bytes_kernel<NCH, METRIC, MASKED>: the grid of the float scan with tiles of 32 queries: one wave per (tile, slab),
//     SCAN_BYTES_WAVES waves per workgroup.  Returns at once unless the path word is 2 (the float kernels, launched behind it
//     with the same lists, return unless it is 1).
//     A operand: a block of 32 rows (aligned to 32, so that it is one mask word), straight from global memory: lane l holds 16
//       contiguous bytes of row l % 32 per step -- bytes [32 s + 16 (l / 32), + 16) at step s, 2 * NCH steps -- made signed by
//       x' = x xor 0x80.  The next block's loads are in flight while this one is multiplied.
//     B operand: the tile's codes, the same bytes of query l % 32, held in 8 * NCH registers for the whole slab.  (Which k a
//       lane's byte stands for inside the instruction does not matter: both operands use the same map and the sum is over all k.)
//     A padded row byte is -128 after the xor and meets a zero code: it adds nothing.
//     With acc = sum x'q' over the row:   sum xq = acc + 128 sum q' + 128 sum x,
//       L2^2 = (sum x^2 - 256 sum x) - 2 acc + (sum q^2 - 256 sum q'),   all sums over the real dimensions.
//     The row terms (sum x, sum x^2) come from the raw operand registers by v_dot4_u32_u8 -- the zero padding adds nothing -- and
//     one cross-half exchange; they reach the accumulator layout (lane l: query l % 32, rows 8 a + 4 (l / 32) + b of the block)
//     through 128 bytes of LDS.  No table of row terms exists: insert, remove, upsert and compact have nothing to maintain.
//     Selection: m = the metric's integer rank value (L2: the squared distance, IP: minus the inner product) is monotone in the
//     key, so the common path is one integer subtract and one compare per accumulator against a per-lane bound (the query's k-th
//     word so far, as an integer, less the query's term).  Survivors (rare) become (dist_to_key((float)integer) << 32 | row)
//     words in the query's LDS buffer; a buffer that may not take another block is merged into the query's list by scan_flush.
//     Lists: exactly the float scan's ([nq][n_slabs][2][k], ascending, padded with SCAN_EMPTY, result in the first half).
#include "hnsw_internal.h"
#include "hnsw_scan_device.hip.h"

namespace hnsw_dev {

using hnsw_host::SCAN_BYTES_TILE;
using hnsw_host::SCAN_BYTES_WAVES;

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

struct ScanBytesArgs {
    const uint8_t *X8;     // [n][64 * NCH] byte rows
    int64_t n;
    const uint8_t *codes;  // [nq][64 * NCH] the queries of this launch, as the prepass wrote them
    const int32_t *terms;  // [nq]
    int64_t nq;
    int32_t k, n_slabs;
    int64_t slab_rows;
    uint64_t *lists;
    const uint32_t *path;  // the handle's path word
};

// state: [0] the path word, [1] "a value was no byte" of the launch in flight, [2] its finished waves; [1] and [2] are 0 between launches.
// The three words belong to the handle, as the lists and the codes do (scratch.scan, scratch.scan_codes): ONE exact scan in flight
// per handle -- two on different streams would share the counters and the lists -- and a prepass that never finished would leave
// [1] and [2] set for the handle's later scans.
__global__ void hnsw_scan_bytes_state_kernel(uint32_t *state) { state[0] = state[1] = state[2] = state[3] = 0u; }
template <int METRIC>
__global__ void __launch_bounds__(256)
hnsw_scan_bytes_queries_kernel(const float *Q, int64_t q_stride, int64_t nq, int32_t d, int32_t row_bytes, uint8_t *codes, int32_t *terms,
                               uint32_t *state) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    bool ok = true;
    if (q < nq) {
        int32_t s1 = 0, s2 = 0;     // sum q', sum q^2 over the lane's real dimensions
        uint32_t u = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * lane + j;
            if (e < d) {
                const float v = Q[q * q_stride + e];
                const bool byte = v >= 0.0f && v <= 255.0f && v == truncf(v);
                const int c = byte ? (int)v : 0;
                ok = ok && byte;
                s1 += c - 128;
                s2 += c * c;
                u |= (uint32_t)((c - 128) & 0xFF) << (8 * j);
            }
        }
        if (4 * lane < row_bytes) reinterpret_cast<uint32_t *>(codes + q * row_bytes)[lane] = u;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
        if (lane == 0) terms[q] = METRIC == 0 ? s2 - 256 * s1 : -128 * s1;
    }
    const bool bad = ballot(!ok) != 0ull;
    if (lane == 0) scan_prepass_publish(state, bad, (uint32_t)hnsw_host::SCAN_PATH_BYTES);
}

// the bound a lane compares its accumulators' rank values (less the query's term cq) against: the rank value of the query's k-th word
template <int METRIC> __device__ __forceinline__ int scan_bytes_bound(uint64_t thr, int cq) {
    if (thr == SCAN_EMPTY) return 0x7FFFFFFF;               // fewer than k words so far: every row survives
    const uint32_t key = (uint32_t)(thr >> 32);
    // (exact both ways: the keys of the list were made from integers below 2^24)
    const int m = METRIC == 0 ? (int)__uint_as_float(key) : -(int)(1.0f - key_to_dist<1>(key));
    return m - cq;
}

template <int NCH, int METRIC, bool MASKED>
__device__ __forceinline__ void scan_bytes_slab(const ScanBytesArgs &a, const uint32_t *mask_) {
    constexpr int S = 2 * NCH;                  // matrix instructions per block: 32 bytes of every row each
    constexpr int RB = 64 * NCH;                // bytes per row and per query's codes
    constexpr int T = SCAN_BYTES_TILE;
    constexpr int LIMIT = SCAN_BUF - 32;        // a buffer up to here takes the survivors of one more block
    static_assert(NCH == 1 || NCH == 2 || NCH == 4, "rows of 64, 128 or 256 bytes");
    __shared__ uint64_t bufs_all[SCAN_BYTES_WAVES][T][SCAN_BUF];
    __shared__ uint64_t sorted_all[SCAN_BYTES_WAVES][SCAN_BUF];
    __shared__ int cnt_all[SCAN_BYTES_WAVES][T];
    __shared__ __attribute__((aligned(16))) int rterm_all[SCAN_BYTES_WAVES][32];
    if (*a.path != (uint32_t)hnsw_host::SCAN_PATH_BYTES) return;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;     // the lane's query column (and row of the A operand); which half of the k range
    const int64_t q0 = (int64_t)blockIdx.x * T;
    const int tq = (int)(a.nq - q0 < T ? a.nq - q0 : T);
    const int64_t slab = (int64_t)blockIdx.y * SCAN_BYTES_WAVES + uniform(wave);
    if (slab >= a.n_slabs) return;              // (no workgroup barrier anywhere)
    const int64_t r0 = slab * a.slab_rows, r1 = r0 + a.slab_rows < a.n ? r0 + a.slab_rows : a.n;
    const MaskWords mask = mask_words(mask_);
    uint64_t (*const bufs)[SCAN_BUF] = bufs_all[wave];
    uint64_t *const sorted = sorted_all[wave];
    int *const cnt = cnt_all[wave];
    int *const rterm = rterm_all[wave];

    // the tile: a query past its end reads the last one's codes and never has a survivor
    const int jq = j < tq ? j : tq - 1;
    v4i b[S];
    {
        const uint8_t *qp = a.codes + (q0 + jq) * RB + 16 * h;
#pragma unroll
        for (int s = 0; s < S; ++s) b[s] = *reinterpret_cast<const v4i *>(qp + 32 * s);
    }
    const int cq = a.terms[q0 + jq];
    uint64_t *const lists0 = a.lists + ((q0 * a.n_slabs + slab) * 2) * (int64_t)a.k;
    const int64_t list_step = (int64_t)a.n_slabs * 2 * a.k;
    for (int t = 0; t < tq; ++t) for (int i = lane; i < a.k; i += 64) lists0[t * list_step + i] = SCAN_EMPTY;
    if (lane < T) cnt[lane] = 0;
    scan_wave_sync();
    uint64_t thr = j < tq ? SCAN_EMPTY : 0ull;                          // the query's k-th word so far (no word is below 0)
    int bound = j < tq ? 0x7FFFFFFF : (int)0x80000000;
    uint32_t par = 0;                                                   // bit t: query t's current list is the second half

    // merges query t's buffer of c words into its list
    auto flush = [&](int t, int c) {
        uint64_t *const A = lists0 + t * list_step;
        const bool p = (par >> t) & 1u;
        scan_flush(bufs[t], sorted, c, A + (p ? a.k : 0), A + (p ? 0 : a.k), a.k, lane);
        par ^= 1u << t;
        if (lane == 0) cnt[t] = 0;
    };
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
        if (!((cw >> j) & 1u)) rt = hnsw_host::SCAN_BYTES_NO_ROW;       // no candidate: above every bound a full list sets
        if (h == 0) rterm[j] = rt;
        scan_lds_sync();

        v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < S; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ax[s], b[s], acc, 0, 0, 0);

        // accumulator v of the lane: row 8 (v / 4) + 4 h + v % 4 of the block, query j
        int tv[16];
        bool any = false;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int *const rr = rterm + 8 * g + 4 * h;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int v = 4 * g + c;
                tv[v] = METRIC == 0 ? rr[c] - 2 * acc[v] : rr[c] - acc[v];
                any = any || tv[v] <= bound;
            }
        }
        if (ballot(any)) {                      // rare once the lists are full
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int ri = 8 * (v >> 2) + 4 * h + (v & 3);
                if (tv[v] <= bound && ((cw >> ri) & 1u)) {
                    const int m = tv[v] + cq;
                    const float sum = METRIC == 0 ? (float)m : (float)(-m);
                    const uint64_t e = ((uint64_t)dist_to_key<METRIC>(sum) << 32) | (uint32_t)(cur + ri);
                    if (e < thr) bufs[j][atomicAdd(&cnt[j], 1)] = e;
                }
            }
            scan_wave_sync();
            const int c = cnt[j];
            uint32_t need = (uint32_t)ballot(h == 0 && c > LIMIT);
            if (need) {
                while (need) {
                    const int t = __builtin_ctz(need);
                    need &= need - 1u;
                    flush(t, __builtin_amdgcn_readlane(c, t));
                }
                scan_wave_sync();
                if (j < tq) {
                    thr = (lists0 + j * list_step + (((par >> j) & 1u) ? a.k : 0))[a.k - 1];
                    bound = scan_bytes_bound<METRIC>(thr, cq);
                }
            }
        }
    }
    // what is left in the buffers; the result belongs in the first half
    scan_wave_sync();
    for (int t = 0; t < tq; ++t) {
        const int c = uniform(cnt[t]);
        if (c > 0) flush(t, c);
        uint64_t *const A = lists0 + t * list_step;
        if ((par >> t) & 1u) for (int i = lane; i < a.k; i += 64) A[i] = A[a.k + i];
    }
}

template <int NCH, int METRIC>
__global__ void __launch_bounds__(64 * SCAN_BYTES_WAVES)
hnsw_scan_bytes_kernel(const ScanBytesArgs a) {
    scan_bytes_slab<NCH, METRIC, false>(a, nullptr);
}
// ... restricted to the rows masks[0] allows (the single-mask filtered exact stage, a marked index's live mask)
template <int NCH, int METRIC>
__global__ void __launch_bounds__(64 * SCAN_BYTES_WAVES)
hnsw_scan_bytes_masked_kernel(const ScanBytesArgs a, const uint32_t *const *masks) {
    scan_bytes_slab<NCH, METRIC, true>(a, masks[0]);
}

} // namespace hnsw_dev

namespace hnsw_host {

// the handle's path word and the prepass's two counters, zeroed once by a one-thread kernel on the stream of the first launch that
// reads them (no blocking copy; a kernel, not a memset node, so the launch may also be recorded)
int ensure_scan_state(hnsw_index *idx, hipStream_t st) {
    if (idx->scratch.scan_state.p) return HNSW_OK;
    int rc = idx->scratch.scan_state.ensure(16);
    if (rc) return rc;
    hipLaunchKernelGGL(hnsw_dev::hnsw_scan_bytes_state_kernel, dim3(1), dim3(1), 0, st, (uint32_t *)idx->scratch.scan_state.p);
    if ((rc = launched("scan state kernel"))) { idx->scratch.scan_state.release(); return rc; }
    return HNSW_OK;
}

// the prepass of nq queries: their codes and terms into scratch.scan_codes, the path word (the k-scan's pieces; the range scan's PASS 0)
int scan_bytes_prepass(hnsw_index *idx, const float *Q, int64_t q_stride, int64_t nq, hipStream_t st, const uint8_t **codes_out, const int32_t **terms_out,
                       const uint32_t **path) {
    int rc = ensure_scan_state(idx, st);
    if (rc) return rc;
    const int d = idx->iv.d;
    const ScanBytesScratch s = scan_bytes_scratch(nq, d);
    if ((rc = idx->scratch.scan_codes.ensure((size_t)s.total))) return rc;
    uint8_t *const codes = (uint8_t *)idx->scratch.scan_codes.p;
    int32_t *const terms = (int32_t *)(codes + s.terms_at);
    uint32_t *const state = (uint32_t *)idx->scratch.scan_state.p;
    with_metric(idx->info.metric, [&](auto METRIC) {
        hipLaunchKernelGGL(hnsw_dev::hnsw_scan_bytes_queries_kernel<METRIC>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, Q, q_stride, nq, d,
                           scan_bytes_row_bytes(d), codes, terms, state);
    });
    if ((rc = launched("scan query prepass"))) return rc;
    *codes_out = codes; *terms_out = terms; *path = state;
    return HNSW_OK;
}

int scan_bytes_launch(hnsw_index *idx, const float *Q, int64_t q_stride, int64_t nq, int32_t k, int nch, int64_t slabs, int64_t slab_rows,
                      uint64_t *lists, const uint32_t *const *masks, hipStream_t st, const uint32_t **path) {
    const uint8_t *codes = nullptr;
    const int32_t *terms = nullptr;
    const uint32_t *state = nullptr;
    int rc = scan_bytes_prepass(idx, Q, q_stride, nq, st, &codes, &terms, &state);
    if (rc) return rc;
    const hnsw_dev::ScanBytesArgs a{(const uint8_t *)idx->tables.X8.p, idx->iv.n, codes, terms, nq, k, (int32_t)slabs, slab_rows, lists, state};
    const dim3 grid((unsigned)scan_bytes_tiles(nq), (unsigned)scan_bytes_slab_groups(slabs));
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
        if constexpr (NCH <= 4) {
            if (masks) hipLaunchKernelGGL((hnsw_dev::hnsw_scan_bytes_masked_kernel<NCH, METRIC>), grid, dim3(64 * SCAN_BYTES_WAVES), 0, st, a, masks);
            else hipLaunchKernelGGL((hnsw_dev::hnsw_scan_bytes_kernel<NCH, METRIC>), grid, dim3(64 * SCAN_BYTES_WAVES), 0, st, a);
        }
    }); });
    if ((rc = launched("byte scan kernel"))) return rc;
    *path = state;
    return HNSW_OK;
}

} // namespace hnsw_host

extern "C" int32_t hnsw_index_scan_path(hnsw_index *idx, int32_t *out) {
    using namespace hnsw_host;
    if (!idx || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (idx->scan_path_known >= 0 || !idx->scratch.scan_state.p) { *out = std::max(idx->scan_path_known, 0); return HNSW_OK; }
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipDeviceSynchronize());            // (the launch may be on any stream, the caller's included)
    uint32_t word = 0;
    HIP_TRY(hipMemcpy(&word, idx->scratch.scan_state.p, 4, hipMemcpyDeviceToHost));
    *out = (int32_t)word;
    return HNSW_OK;
}
