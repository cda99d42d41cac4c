// hnsw_rows_sq8_dim.hip -- per-dimension sq8 rows: a copy of the vectors as 8-bit codes under one affine map PER DIMENSION.
// hnsw_rows_sq8.hip quantises the whole table under one map (lo, s over all n * d values); where the columns do not share a range --
// a handful of outliers in one column is enough -- that map spends its 256 codes on the widest column and is blind in the others.
// Here, for each dimension i, with lo_i = min, hi_i = max over column i and s_i = (hi_i - lo_i) / 255 (1 when hi_i == lo_i)
//     code_i(x) = min(255, max(0, rint((x_i - lo_i) / s_i)))        x^_i = lo_i + s_i * code_i(x)
// in float32, round to nearest, ties to even.  The maps differ by dimension, so code space is no longer a scaled copy of X^:
//     <x^, q> = sum(lo_i q_i) + <code(x), s o q>         the first term is constant per query: the inner-product walk is the
//                                                        UNCHANGED byte-row search (ROWS = 2) over the codes with q' = s o q;
//     |x^ - q|^2 = sum((s_i code_i(x) - (q_i - lo_i))^2) a weighted distance: the knn kernel's ROWS = 5 (hnsw_device.hip.h:
//                                                        hop_round; instances: hnsw_sq8_dim_walk.hip) multiplies each code by its
//                                                        scale -- held in registers beside the query -- and walks with q'' = q - lo.
// Either walk's distances never reach the caller: as over sq8 rows the search always ends in the exact re-rank over the float32
// rows (refine_count in hnsw_capi.hip).  The copy is made on request only (option "sq8_dim_rows"); the float32 rows stay for
// everything that is not a knn walk.
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

// a column chunk's running answer: the four dimensions' minimum and maximum keys, and which of them met a value that is not finite
struct ChunkRange {
    uint4 mn, mx, bad;
    __device__ __forceinline__ void clear() { mn = make_uint4(~0u, ~0u, ~0u, ~0u); mx = make_uint4(0u, 0u, 0u, 0u); bad = mx; }
    __device__ __forceinline__ void fold(const ChunkRange &o) {
        mn.x = min(mn.x, o.mn.x); mn.y = min(mn.y, o.mn.y); mn.z = min(mn.z, o.mn.z); mn.w = min(mn.w, o.mn.w);
        mx.x = max(mx.x, o.mx.x); mx.y = max(mx.y, o.mx.y); mx.z = max(mx.z, o.mx.z); mx.w = max(mx.w, o.mx.w);
        bad.x |= o.bad.x; bad.y |= o.bad.y; bad.z |= o.bad.z; bad.w |= o.bad.w;
    }
    __device__ __forceinline__ void value(uint32_t b, uint32_t &lo, uint32_t &hi, uint32_t &flag) {
        const uint32_t k = order_key(b);
        lo = min(lo, k); hi = max(hi, k); flag |= (b & 0x7FFFFFFFu) >= 0x7F800000u ? 1u : 0u;
    }
    __device__ __forceinline__ void row(const float4 t) {
        value(__float_as_uint(t.x), mn.x, mx.x, bad.x); value(__float_as_uint(t.y), mn.y, mx.y, bad.y);
        value(__float_as_uint(t.z), mn.z, mx.z, bad.z); value(__float_as_uint(t.w), mn.w, mx.w, bad.w);
    }
};

// The finite check and all d ranges in ONE pass over X, column-wise.  A block of 256 threads is 256 / CW row lanes x CW column
// chunks (CW: the power of two that holds the row's used float4 chunks, at most 256 -- d <= 1024): thread t folds chunk t % CW of
// the rows blockIdx.x * RL + t / CW, + gridDim.x * RL, ... (a row's chunks side by side: 16-byte loads, coalesced), the block's row
// lanes meet in LDS, and each block leaves one partial per chunk: part[blockIdx.x][3][used_chunks] (minima, maxima, flags).  The
// padding dimensions of the last chunk read the rows' zeros and are never looked at.  Minimum and maximum do not depend on the
// order they are taken in: the result is the same bits whatever the grid.
__global__ void __launch_bounds__(256)
sq8_dim_range_kernel(const float4 *X, int64_t n, int32_t row_chunks, int32_t used_chunks, int32_t cw, uint4 *part) {
    __shared__ uint4 sh[3][256];
    const int t = threadIdx.x, c = t & (cw - 1), rl = t / cw, RL = 256 / cw;
    ChunkRange acc;
    acc.clear();
    if (c < used_chunks)
        for (int64_t row = (int64_t)blockIdx.x * RL + rl; row < n; row += (int64_t)gridDim.x * RL) acc.row(X[row * row_chunks + c]);
    sh[0][t] = acc.mn; sh[1][t] = acc.mx; sh[2][t] = acc.bad;
    __syncthreads();
    if (t < used_chunks) {           // (t < cw: row lane 0 of chunk t)
        for (int r = 1; r < RL; ++r) {
            ChunkRange o;
            o.mn = sh[0][r * cw + t]; o.mx = sh[1][r * cw + t]; o.bad = sh[2][r * cw + t];
            acc.fold(o);
        }
        uint4 *out = part + (int64_t)blockIdx.x * 3 * used_chunks;
        out[t] = acc.mn; out[used_chunks + t] = acc.mx; out[2 * used_chunks + t] = acc.bad;
    }
}
// the second stage: one block, one thread per chunk, folds the partials: out[3][used_chunks]
__global__ void __launch_bounds__(256)
sq8_dim_range_final_kernel(const uint4 *part, int32_t nparts, int32_t used_chunks, uint4 *out) {
    const int t = threadIdx.x;
    if (t >= used_chunks) return;
    ChunkRange acc;
    acc.clear();
    for (int i = 0; i < nparts; ++i) {
        const uint4 *p = part + (int64_t)i * 3 * used_chunks;
        ChunkRange o;
        o.mn = p[t]; o.mx = p[used_chunks + t]; o.bad = p[2 * used_chunks + t];
        acc.fold(o);
    }
    out[t] = acc.mn; out[used_chunks + t] = acc.mx; out[2 * used_chunks + t] = acc.bad;
}

// (x - lo) / s: two correctly rounded float32 operations, nothing contracted (numpy: (x - lo) / s on float32 arrays)
__device__ __forceinline__ float to_code(float x, float lo, float s) {
    return fminf(255.0f, fmaxf(0.0f, rintf(__fdiv_rn(__fsub_rn(x, lo), s))));
}

// one thread per dword of the code rows: bytes 4c..4c+3 of a row are the codes of dims 4c..4c+3 (0 beyond d), as hnsw_rows8.hip lays
// its bytes out; lo4 / s4: the per-dimension tables in the lane grid, one float4 per dword of a row
__global__ void __launch_bounds__(256)
pack_sq8_dim_rows_kernel(const float4 *X, int64_t n, int32_t d, int32_t row_chunks, const float4 *lo4, const float4 *s4, uint32_t *Xq,
                         int32_t words_per_row) {
    const int64_t total = n * (int64_t)words_per_row;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = w / words_per_row;
        const int c = (int)(w - row * words_per_row);
        uint32_t u = 0;
        if (4 * c < d) {
            const float4 t = X[row * row_chunks + c], l = lo4[c], s = s4[c];
            const float v[4] = {t.x, t.y, t.z, t.w}, lv[4] = {l.x, l.y, l.z, l.w}, sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * c + j >= d) continue;
                u |= (uint32_t)to_code(v[j], lv[j], sv[j]) << (8 * j);
            }
        }
        Xq[w] = u;
    }
}

// The queries of a batch as the walk reads them: one thread per float4 of Qt ([nq][4 * out_chunks] floats, zero beyond d).  Q is the
// caller's matrix at the caller's stride -- device memory, or a page-locked host matrix read in place, each value once --; `vec`:
// its rows are 16-byte aligned.  scaled = 0 (L2): q'' = q - lo; 1 (the inner product): q' = s * q; each one rounded operation.
// stage (optional, [nq][q_stride]): the d values of every query as they were read, for the re-rank behind the walk.  Q == Qt with
// q_stride == 4 * out_chunks is allowed: a thread writes the chunk it read.
__global__ void __launch_bounds__(256)
sq8_dim_query_kernel(const float *Q, int64_t q_stride, int64_t nq, int32_t d, int32_t out_chunks, const float4 *lo4, const float4 *s4,
                     int32_t scaled, int32_t vec, float4 *Qt, float *stage) {
    const int64_t total = nq * (int64_t)out_chunks;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = w / out_chunks;
        const int c = (int)(w - q * out_chunks), e0 = 4 * c;
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
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (e0 < d) {                // (the tables cover the lane grid, which holds every chunk below d)
            const float4 m = scaled ? s4[c] : lo4[c];
            const float mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) if (e0 + j < d) o[j] = scaled ? __fmul_rn(mv[j], v[j]) : __fsub_rn(v[j], mv[j]);
        }
        Qt[w] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

unsigned grid_for(int64_t threads, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, (threads + 255) / 256)); }

} // namespace

namespace hnsw_host {

int make_sq8_dim_rows(::hnsw_index *idx) {
    if (!idx || !idx->tables.X.p || idx->iv.n <= 0) return fail(HNSW_ERR_BAD_ARG, "sq8 dim rows: the index has no vectors");
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n;
    const int32_t d = idx->iv.d, row_chunks = (int32_t)(idx->iv.stride / 4), used_chunks = (d + 3) / 4;
    const int32_t row_bytes = 64 * pick_nch(idx->iv.nchunks);     // the lane grid of the byte kernels: 16 lanes x NCH dwords
    if (used_chunks > 256 || row_bytes <= 0) return fail(HNSW_ERR_UNSUPPORTED, "sq8 dim rows: d=%d is wider than the lane grid", d);
    // ---- the d ranges, and which columns hold a value that is not finite ----
    int32_t cw = 1;
    while (cw < used_chunks) cw *= 2;
    const int32_t RL = 256 / cw;
    const unsigned parts = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (n + RL - 1) / RL));
    DevBuf red;
    int rc;
    if ((rc = red.ensure(((size_t)parts + 1) * 3 * (size_t)used_chunks * sizeof(uint4)))) return rc;
    uint4 *part = (uint4 *)red.p, *result = part + (size_t)parts * 3 * used_chunks;
    hipLaunchKernelGGL(sq8_dim_range_kernel, dim3(parts), dim3(256), 0, 0, (const float4 *)idx->tables.X.p, n, row_chunks, used_chunks, cw, part);
    hipLaunchKernelGGL(sq8_dim_range_final_kernel, dim3(1), dim3(256), 0, 0, (const uint4 *)part, (int32_t)parts, used_chunks, result);
    hipError_t e = hipGetLastError();
    std::vector<uint32_t> r((size_t)12 * used_chunks);           // [3][used_chunks][4]
    if (e == hipSuccess) e = hipMemcpy(r.data(), result, r.size() * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "sq8-dim-row range failed: %s", hipGetErrorString(e));
    const size_t lanes = (size_t)row_bytes;                       // floats of a per-dimension table in the lane grid
    std::vector<float> lo((size_t)d), s((size_t)d), lo_grid(lanes, 0.0f), s_grid(lanes, 0.0f);
    for (int32_t i = 0; i < d; ++i) {
        if (r[(size_t)8 * used_chunks + i]) return fail(HNSW_ERR_UNSUPPORTED, "sq8 dim rows: column %d holds a value that is NaN or infinite", i);
        const float l = key_value(r[(size_t)i]) + 0.0f, h = key_value(r[(size_t)4 * used_chunks + i]) + 0.0f;   // (+ 0: a bound of -0 is reported as +0)
        const float range = h - l;
        if (!std::isfinite(range))
            return fail(HNSW_ERR_UNSUPPORTED, "sq8 dim rows: column %d: the range of its values, %g .. %g, overflows float32", i, (double)l, (double)h);
        const float step = h == l ? 1.0f : range / 255.0f;
        if (!(step > 0.0f))
            return fail(HNSW_ERR_UNSUPPORTED, "sq8 dim rows: column %d: the range of its values, %g .. %g, is too narrow to divide into 255 steps", i,
                        (double)l, (double)h);
        lo[(size_t)i] = lo_grid[(size_t)i] = l; s[(size_t)i] = s_grid[(size_t)i] = step;
    }
    // ---- the tables and the codes, in tables of their own until they are complete ----
    Table Xqd, qd_lo, qd_s;
    if ((e = qd_lo.alloc(lanes * 4)) == hipSuccess && (e = qd_s.alloc(lanes * 4)) == hipSuccess) e = Xqd.alloc((size_t)n * (size_t)row_bytes);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? HNSW_ERR_OOM : HNSW_ERR_HIP, "sq8 dim rows: no room for %lld bytes: %s",
                    (long long)(n * row_bytes), hipGetErrorString(e));
    e = hipMemcpy(qd_lo.p, lo_grid.data(), lanes * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(qd_s.p, s_grid.data(), lanes * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "sq8-dim-row tables failed: %s", hipGetErrorString(e));
    const int32_t words = row_bytes / 4;
    hipLaunchKernelGGL(pack_sq8_dim_rows_kernel, dim3(grid_for(n * (int64_t)words, 65536)), dim3(256), 0, 0, (const float4 *)idx->tables.X.p, n, d,
                       row_chunks, (const float4 *)qd_lo.p, (const float4 *)qd_s.p, (uint32_t *)Xqd.p, words);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "sq8-dim-row packing failed: %s", hipGetErrorString(e));
    idx->tables.Xqd = std::move(Xqd); idx->tables.qd_lo = std::move(qd_lo); idx->tables.qd_s = std::move(qd_s);
    idx->sq8d_lo = std::move(lo); idx->sq8d_scale = std::move(s);
    return HNSW_OK;
}

int sq8_dim_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st) {
    const int32_t out_chunks = (int32_t)(padded_stride(idx->iv.d) / 4);
    const bool vec = q_stride % 4 == 0 && (uintptr_t)Q % 16 == 0 && (!stage || (uintptr_t)stage % 16 == 0);
    hipLaunchKernelGGL(sq8_dim_query_kernel, dim3(grid_for(nq * (int64_t)out_chunks, 65536)), dim3(256), 0, st, Q, q_stride, nq, idx->iv.d, out_chunks,
                       (const float4 *)idx->tables.qd_lo.p, (const float4 *)idx->tables.qd_s.p, idx->info.metric == HNSW_METRIC_L2 ? 0 : 1,
                       vec ? 1 : 0, (float4 *)Qt, stage);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "sq8-dim query transform launch failed: %s", hipGetErrorString(e));
    return HNSW_OK;
}

} // namespace hnsw_host

extern "C" {

int32_t hnsw_index_sq8_dim_params(const hnsw_index *idx, float *lo, float *scale) {
    if (!idx || !lo || !scale) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (!idx->tables.Xqd.p) return fail(HNSW_ERR_BAD_ARG, "the index has no per-dimension sq8 rows (option sq8_dim_rows 1 makes them)");
    const size_t d = (size_t)idx->iv.d;
    memcpy(lo, idx->sq8d_lo.data(), d * 4); memcpy(scale, idx->sq8d_scale.data(), d * 4);
    return HNSW_OK;
}

int32_t hnsw_index_sq8_dim_codes(const hnsw_index *idx, uint8_t *out) {
    if (!idx || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (!idx->tables.Xqd.p) return fail(HNSW_ERR_BAD_ARG, "the index has no per-dimension sq8 rows (option sq8_dim_rows 1 makes them)");
    HIP_TRY(hipSetDevice(idx->device));
    const size_t n = (size_t)idx->iv.n, d = (size_t)idx->iv.d, row_bytes = 64 * (size_t)pick_nch(idx->iv.nchunks);
    // the first d bytes of every row straight into the caller's [n][d] array: the padding stays behind
    HIP_TRY(hipMemcpy2D(out, d, idx->tables.Xqd.p, row_bytes, d, n, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

} // extern "C"
