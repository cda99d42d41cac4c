// hnsw_rows_bits.hip -- bit rows: a copy of the vectors as ONE BIT per dimension, bit i = x_i > t_i, walked under Hamming distance
// (option "bit_rows": binary quantisation).  The walk's cost is the 128-byte lines per evaluated row: a 1024-dimensional float32 row
// is 32 of them, its sq8 codes 8, its bits ONE (a 512-dimensional row half a line).  Thresholds: the column means (mode 1) or zero
// (mode 2, sign bits).  A stored row is 16 * NW dwords, NW = ceil(d / 512): dimension i is bit i % 32 of dword i / 32, zero beyond d;
// lane l16 of a 16-lane group reads dword 16 j + l16 in step j (the knn kernel's ROWS = 6, hnsw_device.hip.h: hop_round; instances:
// hnsw_bits_walk.hip).  The walk's distances never reach the caller: as over sq8 rows the search always ends in the exact re-rank
// over the float32 rows under the index's real metric (refine_count in hnsw_capi.hip).  The copy is made on request only; the
// float32 rows stay for everything that is not a knn walk.
// Option "bit_query_bits" 4 walks the SAME rows against a query kept at 4 bits a dimension (bit_query_planes_kernel makes its codes and
// bit planes here; the walk is the knn kernel's ROWS = 7, hnsw_bits_asym_walk.hip): an asymmetric distance, the inner product of the
// query's codes with the +-1 vector a row's bits stand for.
#include "hnsw_internal.h"

using namespace hnsw_host;

namespace {

// a column chunk's running answer: the four dimensions' sums in float64, and which of them met a value that is not finite
struct ChunkSum {
    double sx, sy, sz, sw;
    uint4 bad;
    __device__ __forceinline__ void clear() { sx = sy = sz = sw = 0.0; bad = make_uint4(0u, 0u, 0u, 0u); }
    __device__ __forceinline__ void fold(const ChunkSum &o) {
        sx += o.sx; sy += o.sy; sz += o.sz; sw += o.sw;
        bad.x |= o.bad.x; bad.y |= o.bad.y; bad.z |= o.bad.z; bad.w |= o.bad.w;
    }
    static __device__ __forceinline__ uint32_t not_finite(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) >= 0x7F800000u ? 1u : 0u; }
    __device__ __forceinline__ void row(const float4 t) {
        sx += (double)t.x; sy += (double)t.y; sz += (double)t.z; sw += (double)t.w;
        bad.x |= not_finite(t.x); bad.y |= not_finite(t.y); bad.z |= not_finite(t.z); bad.w |= not_finite(t.w);
    }
};

// The finite check and all d column sums in ONE pass over X: the block shape of the per-dimension sq8 range pass.  A block of 256
// threads is 256 / CW row lanes x CW column chunks (CW: the power of two that holds the row's used float4 chunks, at most 256 --
// d <= 1024): thread t folds chunk t % CW of the rows blockIdx.x * RL + t / CW, + gridDim.x * RL, ... (16-byte loads, a row's chunks
// side by side), the block's row lanes meet in LDS in ascending order, and each block leaves one partial per chunk:
// psum[blockIdx.x][used_chunks] (double4 as four doubles), pbad[blockIdx.x][used_chunks].  A float64 sum depends on its order: the
// grid is a function of (n, d) alone (make_bit_rows), so the same table gives the same sums on every call.
__global__ void __launch_bounds__(256)
bit_colsum_kernel(const float4 *X, int64_t n, int32_t row_chunks, int32_t used_chunks, int32_t cw, double *psum, uint4 *pbad) {
    __shared__ double shs[4][256];
    __shared__ uint4 shb[256];
    const int t = threadIdx.x, c = t & (cw - 1), rl = t / cw, RL = 256 / cw;
    ChunkSum acc;
    acc.clear();
    if (c < used_chunks)
        for (int64_t row = (int64_t)blockIdx.x * RL + rl; row < n; row += (int64_t)gridDim.x * RL) acc.row(X[row * row_chunks + c]);
    shs[0][t] = acc.sx; shs[1][t] = acc.sy; shs[2][t] = acc.sz; shs[3][t] = acc.sw; shb[t] = acc.bad;
    __syncthreads();
    if (t < used_chunks) {           // (t < cw: row lane 0 of chunk t)
        for (int r = 1; r < RL; ++r) {
            const int o = r * cw + t;
            ChunkSum p;
            p.sx = shs[0][o]; p.sy = shs[1][o]; p.sz = shs[2][o]; p.sw = shs[3][o]; p.bad = shb[o];
            acc.fold(p);
        }
        double *out = psum + ((int64_t)blockIdx.x * used_chunks + t) * 4;
        out[0] = acc.sx; out[1] = acc.sy; out[2] = acc.sz; out[3] = acc.sw;
        pbad[(int64_t)blockIdx.x * used_chunks + t] = acc.bad;
    }
}
// the second stage: one block, one thread per chunk, folds the partials in ascending block order: sum[used_chunks][4], bad[used_chunks]
__global__ void __launch_bounds__(256)
bit_colsum_final_kernel(const double *psum, const uint4 *pbad, int32_t nparts, int32_t used_chunks, double *sum, uint4 *bad) {
    const int t = threadIdx.x;
    if (t >= used_chunks) return;
    ChunkSum acc;
    acc.clear();
    for (int i = 0; i < nparts; ++i) {
        const double *p = psum + ((int64_t)i * used_chunks + t) * 4;
        ChunkSum o;
        o.sx = p[0]; o.sy = p[1]; o.sz = p[2]; o.sw = p[3]; o.bad = pbad[(int64_t)i * used_chunks + t];
        acc.fold(o);
    }
    sum[4 * t + 0] = acc.sx; sum[4 * t + 1] = acc.sy; sum[4 * t + 2] = acc.sz; sum[4 * t + 3] = acc.sw;
    bad[t] = acc.bad;
}

// 64 consecutive dimensions of one row of M ([rows][stride] floats) as two words of bits: one wave per unit, lane l tests dimension
// 64 u + l (a coalesced 256-byte read; beyond d: 0), the ballot is the two words, lane 0 stores them.  thr: [64 * units_per_row]
// floats, the thresholds in dimension order, 0 beyond d.  out: [rows][out_stride] dwords; units_per_row = 8 * NW covers the whole
// stored row, its zero padding included.  stage (optional, [rows][stride]): the d values of every row as they were read (the queries
// of a page-locked host matrix: each value crosses the bus once).
__global__ void __launch_bounds__(256)
bit_pack_kernel(const float *M, int64_t stride, int64_t rows, int32_t d, int32_t units_per_row, const float *thr, uint32_t *out,
                int64_t out_stride, float *stage) {
    const int lane = threadIdx.x & 63;
    const int64_t total = rows * (int64_t)units_per_row, waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < total; w += waves) {
        const int64_t row = w / units_per_row;
        const int u = (int)(w - row * units_per_row), dim = 64 * u + lane;
        bool bit = false;
        if (dim < d) {
            const float x = M[row * stride + dim];
            if (stage) stage[row * stride + dim] = x;
            bit = x > thr[dim];                 // equality: 0; -0 against +0: equal; NaN: 0
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(bit);
        if (lane == 0) *reinterpret_cast<uint2 *>(out + row * out_stride + 2 * u) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
}

// Option "bit_query_bits" 4: one row of M as its 4-bit codes (include/hnsw_mi355x.h states the rule): one wave per row, lane l holds
// y_i = fl(x_i - t_i) of the dimensions 64 u + l (d <= 1024: at most 16 registers); a = max |y_i| over the wave, r = fl(7 / a) -- a
// correctly rounded division --, v_i = rint(fl(y_i * r)) half-to-even, in -7..7; every code is 0 when a = 0, a y_i is NaN or infinite,
// or r is infinite.  out (optional, [rows][out_stride] dwords): the four bit planes of the two's-complement nibbles, plane p in words
// 2 * units_per_row * p .. of the row, each packed as bit_pack_kernel packs bits (a ballot is two words; units_per_row = 8 * NW
// covers a plane with its zero padding).  codes (optional, [rows][d] int8): the v_i themselves.  thr, stage: as bit_pack_kernel.
__global__ void __launch_bounds__(256)
bit_query_planes_kernel(const float *M, int64_t stride, int64_t rows, int32_t d, int32_t units_per_row, const float *thr, uint32_t *out,
                        int64_t out_stride, float *stage, int8_t *codes) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;                       // (wave-uniform)
    float y[16];
    float a = 0.0f;
    bool bad = false;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int dim = 64 * u + lane;
        y[u] = 0.0f;
        if (u < units_per_row && dim < d) {
            const float x = M[row * stride + dim];
            if (stage) stage[row * stride + dim] = x;
            y[u] = x - thr[dim];
            const float m = fabsf(y[u]);
            bad = bad || !(m < __builtin_inff());  // NaN or infinite
            a = fmaxf(a, m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    const float r = __fdiv_rn(7.0f, a);
    const bool zero = __builtin_amdgcn_ballot_w64(bad) != 0 || !(a > 0.0f) || !(r < __builtin_inff());
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        if (u < units_per_row) {                   // (wave-uniform)
            const int dim = 64 * u + lane;
            const int v = zero ? 0 : (int)rintf(__fmul_rn(y[u], r));
            if (codes && dim < d) codes[row * d + dim] = (int8_t)v;
            if (out) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint64_t m = __builtin_amdgcn_ballot_w64(((v >> p) & 1) != 0);
                    if (lane == 0)
                        *reinterpret_cast<uint2 *>(out + row * out_stride + 2 * units_per_row * p + 2 * u) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
                }
            }
        }
    }
}

unsigned grid_for_waves(int64_t waves, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, (waves + 3) / 4)); }

} // namespace

namespace hnsw_host {

int make_bit_rows(::hnsw_index *idx, int mode) {
    if (!idx || !idx->tables.X.p || idx->iv.n <= 0) return fail(HNSW_ERR_BAD_ARG, "bit rows: the index has no vectors");
    if (mode != 1 && mode != 2) return fail(HNSW_ERR_BAD_ARG, "bit rows: mode %d", mode);
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n;
    const int32_t d = idx->iv.d, row_chunks = (int32_t)(idx->iv.stride / 4), used_chunks = (d + 3) / 4;
    if (d > 1024) return fail(HNSW_ERR_UNSUPPORTED, "bit rows: d=%d is wider than two 16-word steps", d);
    const int32_t nw = bit_words(d), row_words = 16 * nw;
    const size_t lanes = (size_t)512 * nw;                        // floats of the threshold table: one per bit of a stored row
    std::vector<float> t((size_t)d, 0.0f), t_grid(lanes, 0.0f);
    {
        // ---- the d column sums (float64), and which columns hold a value that is not finite (refused under either mode: the
        // re-rank behind the walk orders by float32 distances); the grid follows from (n, d) alone ----
        int32_t cw = 1;
        while (cw < used_chunks) cw *= 2;
        const int32_t RL = 256 / cw;
        const unsigned parts = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (n + RL - 1) / RL));
        const size_t cells = ((size_t)parts + 1) * (size_t)used_chunks;
        DevBuf red;
        int rc;
        if ((rc = red.ensure(cells * (4 * sizeof(double) + sizeof(uint4))))) return rc;
        double *psum = (double *)red.p, *sum = psum + (size_t)parts * used_chunks * 4;
        uint4 *pbad = (uint4 *)(psum + cells * 4), *bad = pbad + (size_t)parts * used_chunks;
        hipLaunchKernelGGL(bit_colsum_kernel, dim3(parts), dim3(256), 0, 0, (const float4 *)idx->tables.X.p, n, row_chunks, used_chunks, cw, psum, pbad);
        hipLaunchKernelGGL(bit_colsum_final_kernel, dim3(1), dim3(256), 0, 0, (const double *)psum, (const uint4 *)pbad, (int32_t)parts, used_chunks, sum, bad);
        hipError_t e = hipGetLastError();
        std::vector<double> hs((size_t)4 * used_chunks);
        std::vector<uint32_t> hb((size_t)4 * used_chunks);
        if (e == hipSuccess) e = hipMemcpy(hs.data(), sum, hs.size() * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hb.data(), bad, hb.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(HNSW_ERR_HIP, "bit-row column sums failed: %s", hipGetErrorString(e));
        for (int32_t i = 0; i < d; ++i) {
            if (hb[(size_t)i]) return fail(HNSW_ERR_UNSUPPORTED, "bit rows: column %d holds a value that is NaN or infinite", i);
            if (mode == 1) t[(size_t)i] = t_grid[(size_t)i] = (float)(hs[(size_t)i] / (double)n);
        }
    }
    // ---- the thresholds and the codes, in tables of their own until they are complete ----
    Table Xb, bit_t;
    hipError_t e = bit_t.alloc(lanes * 4);
    if (e == hipSuccess) e = Xb.alloc((size_t)n * (size_t)row_words * 4);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? HNSW_ERR_OOM : HNSW_ERR_HIP, "bit rows: no room for %lld bytes: %s",
                    (long long)(n * row_words * 4), hipGetErrorString(e));
    e = hipMemcpy(bit_t.p, t_grid.data(), lanes * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "bit-row thresholds failed: %s", hipGetErrorString(e));
    const int32_t units = 8 * nw;
    hipLaunchKernelGGL(bit_pack_kernel, dim3(grid_for_waves(n * (int64_t)units, 65536)), dim3(256), 0, 0, (const float *)idx->tables.X.p,
                       (int64_t)idx->iv.stride, n, d, units, (const float *)bit_t.p, (uint32_t *)Xb.p, (int64_t)row_words, (float *)nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "bit-row packing failed: %s", hipGetErrorString(e));
    idx->tables.Xb = std::move(Xb); idx->tables.bit_t = std::move(bit_t);
    idx->bit_t = std::move(t);
    return HNSW_OK;
}

int bits_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, hipStream_t st) {
    if ((const void *)Q == (const void *)Qt) return fail(HNSW_ERR_UNSUPPORTED, "bit rows: the query bits cannot be made in place");
    const int32_t units = 8 * bit_words(idx->iv.d);               // (16 * NW words <= padded_stride(d): they fit the head of a Qt row)
    hipLaunchKernelGGL(bit_pack_kernel, dim3(grid_for_waves(nq * (int64_t)units, 65536)), dim3(256), 0, st, Q, q_stride, nq, idx->iv.d, units,
                       (const float *)idx->tables.bit_t.p, (uint32_t *)Qt, padded_stride(idx->iv.d), stage);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "bit-row query transform launch failed: %s", hipGetErrorString(e));
    return HNSW_OK;
}

int bits_asym_transform_queries(const ::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, float *Qt, float *stage, int8_t *codes,
                                hipStream_t st) {
    if (Qt && (const void *)Q == (const void *)Qt) return fail(HNSW_ERR_UNSUPPORTED, "bit rows: the query planes cannot be made in place");
    if (nq <= 0) return HNSW_OK;
    const int32_t units = 8 * bit_words(idx->iv.d);               // (a Qt row is bit_plane_words(d) = 4 planes * 2 * units words)
    hipLaunchKernelGGL(bit_query_planes_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, Q, q_stride, nq, idx->iv.d, units,
                       (const float *)idx->tables.bit_t.p, (uint32_t *)Qt, bit_plane_words(idx->iv.d), stage, codes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "bit-row query planes launch failed: %s", hipGetErrorString(e));
    return HNSW_OK;
}

} // namespace hnsw_host

extern "C" {

int32_t hnsw_index_bit_query_codes(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int8_t *out) {
    if (!idx || !queries || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    if (q_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "q_stride < d");
    if (!idx->bit_mode || !idx->tables.Xb.p) return fail(HNSW_ERR_BAD_ARG, "the index has no bit rows (option bit_rows 1 or 2 makes them)");
    if (nq == 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(idx->device));
    const size_t d = (size_t)idx->iv.d;
    DevBuf q, codes;
    int rc;
    if ((rc = q.ensure((size_t)nq * d * 4)) || (rc = codes.ensure((size_t)nq * d))) return rc;
    HIP_TRY(hipMemcpy2D(q.p, d * 4, queries, (size_t)q_stride * 4, d * 4, (size_t)nq, hipMemcpyHostToDevice));
    // (COSINE: the codes are those of N(Q), as the searches make them behind the index's own normalisation)
    if (is_cosine(idx) && (rc = cosine_normalise((const float *)q.p, nq, idx->iv.d, (int64_t)d, (float *)q.p, (int64_t)d, nullptr, nullptr, nullptr))) return rc;
    if ((rc = bits_asym_transform_queries(idx, (const float *)q.p, nq, (int64_t)d, nullptr, nullptr, (int8_t *)codes.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out, codes.p, (size_t)nq * d, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

int32_t hnsw_index_bit_params(const hnsw_index *idx, float *t) {
    if (!idx || !t) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (!idx->bit_mode || !idx->tables.Xb.p) return fail(HNSW_ERR_BAD_ARG, "the index has no bit rows (option bit_rows 1 or 2 makes them)");
    memcpy(t, idx->bit_t.data(), (size_t)idx->iv.d * 4);
    return HNSW_OK;
}

int32_t hnsw_index_bit_codes(const hnsw_index *idx, uint32_t *out) {
    if (!idx || !out) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (!idx->bit_mode || !idx->tables.Xb.p) return fail(HNSW_ERR_BAD_ARG, "the index has no bit rows (option bit_rows 1 or 2 makes them)");
    HIP_TRY(hipSetDevice(idx->device));
    const size_t n = (size_t)idx->iv.n, used = ((size_t)idx->iv.d + 31) / 32 * 4, row_bytes = 64 * (size_t)bit_words(idx->iv.d);
    // the first ceil(d / 32) words of every row straight into the caller's array: the padding words stay behind
    HIP_TRY(hipMemcpy2D(out, used, idx->tables.Xb.p, row_bytes, used, n, hipMemcpyDeviceToHost));
    return HNSW_OK;
}

} // extern "C"
