// hnsw_rows_sq8.hip -- sq8 rows: a copy of the vectors as 8-bit codes under ONE affine map, for float data that is not byte-valued.
// The byte-row kernels (ROWS = 2, hnsw_rows8.hip) gather a quarter of the bytes of float32 rows and have the hand-scheduled hop
// loops, but only data whose every value is an integer in 0..255 reaches them.  Uniform scalar quantisation gives any finite
// float table such rows: with lo = min X, hi = max X, s = (hi - lo) / 255 (1 when hi == lo)
//     code(x) = min(255, max(0, rint((x - lo) / s)))        x^ = lo + s * code(x)
// in float32, round to nearest, ties to even.  Because the map is the same for every dimension and every row,
//     |x^ - q|^2 = s^2 |code(x) - (q - lo) / s|^2           <x^, q> = lo * sum(q) + s * <code(x), q>          (s > 0)
// so an L2 search over X^ is an L2 search over the codes B with the query moved to code space (q' = (q - lo) / s), and an
// inner-product search over X^ orders as one over B with the query as it is (q' = q).  The walk is therefore the UNCHANGED byte-row
// search over B with q' -- bit for bit the search over B.astype(float32), descent included -- and its distances, which live in
// code space, never reach the caller: an sq8 search always ends in the exact re-rank over the float32 rows (hnsw_rerank.hip,
// refine_count in hnsw_capi.hip).  The copy is made on request only (option "sq8_rows").  The float32 rows stay: the builder,
// the layer operators, hnsw_distance_batch, the exact scan and hnsw_index_insert's searches use them.
// (A scale per dimension quantises finer, but its L2 distance is a weighted one: a kernel family of its own, option "sq8_dim_rows",
// hnsw_rows_sq8_dim.hip.)
#include "hnsw_internal.h"

using namespace hnsw_host;

namespace {

// a float's bits as an unsigned key of the same order (-0 below +0); NaN and the infinities lie outside [key(-max), key(max)]
__device__ __forceinline__ uint32_t order_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
inline float key_value(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// minimum and maximum over a block of 256 threads: the wave's by the DPP reduction every kernel here uses (wave_min_u32; the
// maximum is the complement of the complements' minimum), the four waves' through LDS: *out = {min key, max key, was any value
// not finite, 0}, one 16-byte store by thread 0
__device__ __forceinline__ void block_min_max(uint32_t mn, uint32_t mx, bool bad, uint4 *out) {
    __shared__ uint32_t part[3][4];
    mn = hnsw_dev::wave_min_u32(mn);
    mx = ~hnsw_dev::wave_min_u32(~mx);
    const bool wbad = __ballot(bad) != 0;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = mn; part[1][wave] = mx; part[2][wave] = wbad ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint4 r = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
#pragma unroll
        for (int w = 0; w < 4; ++w) { r.x = min(r.x, part[0][w]); r.y = max(r.y, part[1][w]); r.z |= part[2][w]; }
        *out = r;
    }
}

// The finite check and the range in ONE pass over X: each thread folds the d real values of the float4 chunks it strides over
// (16-byte loads, a row's chunks side by side; the zero padding past d is left out), each block leaves one partial.  Minimum and
// maximum do not depend on the order they are taken in: the result is the same bits whatever the grid.
__global__ void __launch_bounds__(256)
sq8_range_kernel(const float4 *X, int64_t n, int32_t d, int32_t row_chunks, int32_t used_chunks, uint4 *part) {
    const int64_t total = n * (int64_t)used_chunks;
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
    bool bad = false;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = w / used_chunks;
        const int c = (int)(w - row * used_chunks);
        const float4 t = X[row * row_chunks + c];
        const uint32_t b[4] = {__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z), __float_as_uint(t.w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * c + j >= d) continue;
            bad = bad || (b[j] & 0x7FFFFFFFu) >= 0x7F800000u;
            const uint32_t k = order_key(b[j]);
            mn = k < mn ? k : mn; mx = k > mx ? k : mx;
        }
    }
    block_min_max(mn, mx, bad, part + blockIdx.x);
}
// the second stage: one block folds the partials
__global__ void __launch_bounds__(256)
sq8_range_final_kernel(const uint4 *part, int32_t nparts, uint4 *out) {
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
    bool bad = false;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        const uint4 p = part[i];
        mn = p.x < mn ? p.x : mn; mx = p.y > mx ? p.y : mx; bad = bad || p.z != 0u;
    }
    block_min_max(mn, mx, bad, out);
}

// (x - lo) / s: two correctly rounded float32 operations, nothing contracted (numpy: (x - lo) / s on float32 arrays)
__device__ __forceinline__ float to_code_space(float x, float lo, float s) { return __fdiv_rn(__fsub_rn(x, lo), s); }

// one thread per dword of the code rows: bytes 4c..4c+3 of a row are the codes of dims 4c..4c+3 (0 beyond d), as hnsw_rows8.hip
// lays its bytes out; a thread reads its four values as one float4 (the lane grid can be wider than the float32 row: zeros there)
__global__ void __launch_bounds__(256)
pack_sq8_rows_kernel(const float4 *X, int64_t n, int32_t d, int32_t row_chunks, float lo, float s, uint32_t *Xq, int32_t words_per_row) {
    const int64_t total = n * (int64_t)words_per_row;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = w / words_per_row;
        const int c = (int)(w - row * words_per_row);
        uint32_t u = 0;
        if (4 * c < d) {
            const float4 t = X[row * row_chunks + c];
            const float v[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * c + j >= d) continue;
                const float code = fminf(255.0f, fmaxf(0.0f, rintf(to_code_space(v[j], lo, s))));
                u |= (uint32_t)code << (8 * j);
            }
        }
        Xq[w] = u;
    }
}

// The queries of a batch moved to code space: one thread per float4 of Qt ([nq][4 * out_chunks] floats, zero beyond d).  Q is the
// caller's matrix at the caller's stride -- device memory, or a page-locked host matrix read in place, each value once --;
// `vec`: its rows are 16-byte aligned.  identity (the inner product): q' = q.  stage (optional, [nq][q_stride]): the d values of
// every query as they were read, for the re-rank behind the walk (a host-resident matrix is then read only here).
// Q == Qt with q_stride == 4 * out_chunks is allowed: a thread writes the chunk it read.
__global__ void __launch_bounds__(256)
sq8_query_kernel(const float *Q, int64_t q_stride, int64_t nq, int32_t d, int32_t out_chunks, float lo, float s, int32_t identity,
                 int32_t vec, float4 *Qt, float *stage) {
    const int64_t total = nq * (int64_t)out_chunks;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = w / out_chunks;
        const int e0 = 4 * (int)(w - q * out_chunks);
        const float *src = Q + q * q_stride + e0;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec && e0 + 4 <= d) {
            const float4 t = *reinterpret_cast<const float4 *>(src);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            if (stage) *reinterpret_cast<float4 *>(stage + q * q_stride + e0) = t;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e0 + j >= d) continue;
                v[j] = src[j];
                if (stage) stage[q * q_stride + e0 + j] = v[j];
            }
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = e0 + j >= d ? 0.0f : identity ? v[j] : to_code_space(v[j], lo, s);
        Qt[w] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

unsigned grid_for(int64_t threads, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, (threads + 255) / 256)); }

} // namespace

namespace hnsw_host {

int make_sq8_rows(::hnsw_index *idx) {
    if (!idx || !idx->tables.X.p || idx->iv.n <= 0) return fail(HNSW_ERR_BAD_ARG, "sq8 rows: the index has no vectors");
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n;
    const int32_t d = idx->iv.d, row_chunks = (int32_t)(idx->iv.stride / 4), used_chunks = (d + 3) / 4;
    const int32_t row_bytes = 64 * pick_nch(idx->iv.nchunks);     // the lane grid of the byte kernels: 16 lanes x NCH dwords
    // ---- the range, and whether every value is finite ----
    const unsigned parts = grid_for(n * (int64_t)used_chunks, 1024);
    DevBuf red;
    int rc;
    if ((rc = red.ensure(((size_t)parts + 1) * sizeof(uint4)))) return rc;
    uint4 *part = (uint4 *)red.p, *result = part + parts;
    hipLaunchKernelGGL(sq8_range_kernel, dim3(parts), dim3(256), 0, 0, (const float4 *)idx->tables.X.p, n, d, row_chunks, used_chunks, part);
    hipLaunchKernelGGL(sq8_range_final_kernel, dim3(1), dim3(256), 0, 0, (const uint4 *)part, (int32_t)parts, result);
    hipError_t e = hipGetLastError();
    uint4 r{};
    if (e == hipSuccess) e = hipMemcpy(&r, result, sizeof r, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "sq8-row range failed: %s", hipGetErrorString(e));
    if (r.z) return fail(HNSW_ERR_UNSUPPORTED, "sq8 rows: a value is NaN or infinite");
    const float lo = key_value(r.x) + 0.0f, hi = key_value(r.y) + 0.0f;     // (+ 0: a bound of -0 is reported as +0)
    const float range = hi - lo;
    if (!std::isfinite(range)) return fail(HNSW_ERR_UNSUPPORTED, "sq8 rows: the range of the values, %g .. %g, overflows float32", (double)lo, (double)hi);
    const float s = hi == lo ? 1.0f : range / 255.0f;
    if (!(s > 0.0f)) return fail(HNSW_ERR_UNSUPPORTED, "sq8 rows: the range of the values, %g .. %g, is too narrow to divide into 255 steps", (double)lo, (double)hi);
    // ---- the codes, in a table of their own until they are complete ----
    Table Xq;
    e = Xq.alloc((size_t)n * (size_t)row_bytes);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? HNSW_ERR_OOM : HNSW_ERR_HIP, "sq8 rows: no room for %lld bytes: %s",
                    (long long)(n * row_bytes), hipGetErrorString(e));
    const int32_t words = row_bytes / 4;
    hipLaunchKernelGGL(pack_sq8_rows_kernel, dim3(grid_for(n * (int64_t)words, 65536)), dim3(256), 0, 0, (const float4 *)idx->tables.X.p, n, d,
                       row_chunks, lo, s, (uint32_t *)Xq.p, words);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "sq8-row packing failed: %s", hipGetErrorString(e));
    idx->tables.Xq = std::move(Xq);
    idx->sq8_lo = lo; idx->sq8_scale = s;
    return HNSW_OK;
}

int sq8_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st) {
    const int32_t out_chunks = (int32_t)(padded_stride(idx->iv.d) / 4);
    const bool vec = q_stride % 4 == 0 && (uintptr_t)Q % 16 == 0 && (!stage || (uintptr_t)stage % 16 == 0);
    hipLaunchKernelGGL(sq8_query_kernel, dim3(grid_for(nq * (int64_t)out_chunks, 65536)), dim3(256), 0, st, Q, q_stride, nq, idx->iv.d, out_chunks,
                       idx->sq8_lo, idx->sq8_scale, idx->info.metric == HNSW_METRIC_L2 ? 0 : 1, vec ? 1 : 0, (float4 *)Qt, stage);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "sq8 query transform launch failed: %s", hipGetErrorString(e));
    return HNSW_OK;
}

} // namespace hnsw_host

extern "C" {

int32_t hnsw_index_sq8_params(const hnsw_index *idx, float *lo, float *scale) {
    if (!idx || !lo || !scale) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (!idx->tables.Xq.p) return fail(HNSW_ERR_BAD_ARG, "the index has no sq8 rows (option sq8_rows 1 makes them)");
    *lo = idx->sq8_lo; *scale = idx->sq8_scale;
    return HNSW_OK;
}

int32_t hnsw_index_sq8_codes(const hnsw_index *idx, uint8_t *out) {
    if (!idx || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (!idx->tables.Xq.p) return fail(HNSW_ERR_BAD_ARG, "the index has no sq8 rows (option sq8_rows 1 makes them)");
    HIP_TRY(hipSetDevice(idx->device));
    const size_t n = (size_t)idx->iv.n, d = (size_t)idx->iv.d, row_bytes = 64 * (size_t)pick_nch(idx->iv.nchunks);
    // the first d bytes of every row straight into the caller's [n][d] array: the padding stays behind
    HIP_TRY(hipMemcpy2D(out, d, idx->tables.Xq.p, row_bytes, d, n, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

} // extern "C"
