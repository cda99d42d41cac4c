// hnsw_cosine.hip -- HNSW_METRIC_COSINE: the normaliser N of include/hnsw_mi355x.h on the device, its placement in front of the
// data (cosine_store_rows) and of a call's queries (cosine_queries), hnsw_normalise_batch and hnsw_index_get_rows.
//
// A COSINE index is an IP index over N(X) whose entry points hand N(Q) on: every kernel behind them is the METRIC = 1 kernel
// (with_metric), nothing reads a norm in the hop loop.
#include "hnsw_internal.h"

namespace hnsw_dev {

// One 16-lane group (one DPP row) per row, four rows per wave, NORM_WAVES waves per workgroup.  Lane l16 holds the chunks
// c = 16 i + l16 of its row as the distance kernels do (load_query), sums v * v per lane with the fused multiply-adds of
// eval_nb's inner-product chain and the groups' partial sums with reduce16: <x,x> in the order of every distance of the library.
// VEC: `in` and `out` are 16-byte aligned with strides that are multiples of four floats -- whole chunks move as one dwordx4;
// otherwise (odd strides, an unaligned host matrix) value by value.  The values, and so the bits of N(x), are the same either way.
// in == out is allowed: a group reads all of its row before it writes any of it.
constexpr int NORM_WAVES = 4;
constexpr int NORM_ROWS = 4 * NORM_WAVES;     // rows per workgroup

template <int NCH, bool VEC>
__global__ void __launch_bounds__(64 * NORM_WAVES)
cosine_normalise_kernel(const float *in, int64_t n, int32_t d, int64_t in_stride, float *out, int64_t out_stride, int32_t pad_to,
                        float *norms, uint32_t *bad_flag) {
    const int l16 = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * NORM_ROWS + (threadIdx.x >> 4);
    if (row >= n) return;                     // (a whole 16-lane group leaves: the DPP row below is all in or all out)
    const float *src = in + row * in_stride;
    float4 v[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {           // zero beyond d
        const int e0 = 4 * (i * 16 + l16);
        if (VEC && e0 + 4 <= d) v[i] = *reinterpret_cast<const float4 *>(src + e0);
        else {
            v[i].x = (e0 + 0 < d) ? src[e0 + 0] : 0.f;
            v[i].y = (e0 + 1 < d) ? src[e0 + 1] : 0.f;
            v[i].z = (e0 + 2 < d) ? src[e0 + 2] : 0.f;
            v[i].w = (e0 + 3 < d) ? src[e0 + 3] : 0.f;
        }
    }
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        acc = __builtin_fmaf(v[i].x, v[i].x, acc);
        acc = __builtin_fmaf(v[i].y, v[i].y, acc);
        acc = __builtin_fmaf(v[i].z, v[i].z, acc);
        acc = __builtin_fmaf(v[i].w, v[i].w, acc);
    }
    const float s = reduce16(acc);            // every lane of the group: the same bits
    const bool zero = s == 0.0f, bad = !(s - s == 0.0f);          // bad: NaN or infinite
    // the correctly rounded square root (sqrtf, as key_to_dist takes it: v_sqrt_f32 and its correction steps -- __fsqrt_rn is the
    // bare approximate instruction in this toolchain) and IEEE divisions: the bits of N(x) are those of the header's definition
    const float norm = sqrtf(s);
    const float nan = __uint_as_float(0x7FC00000u);
    float *dst = out + row * out_stride;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int e0 = 4 * (i * 16 + l16);
        float4 o;
        o.x = bad ? nan : zero ? 0.0f : v[i].x / norm;
        o.y = bad ? nan : zero ? 0.0f : v[i].y / norm;
        o.z = bad ? nan : zero ? 0.0f : v[i].z / norm;
        o.w = bad ? nan : zero ? 0.0f : v[i].w / norm;
        // index rows: zero from d to pad_to (= the row stride: a multiple of 16 floats); else only the row's d values are written
        if (e0 + 0 >= d) o.x = 0.0f;
        if (e0 + 1 >= d) o.y = 0.0f;
        if (e0 + 2 >= d) o.z = 0.0f;
        if (e0 + 3 >= d) o.w = 0.0f;
        const int end = pad_to > d ? pad_to : d;
        if (VEC && e0 + 4 <= end) *reinterpret_cast<float4 *>(dst + e0) = o;
        else {
            if (e0 + 0 < end) dst[e0 + 0] = o.x;
            if (e0 + 1 < end) dst[e0 + 1] = o.y;
            if (e0 + 2 < end) dst[e0 + 2] = o.z;
            if (e0 + 3 < end) dst[e0 + 3] = o.w;
        }
    }
    if (l16 == 0) {
        if (norms) norms[row] = bad ? s : norm;
        if (bad && bad_flag) atomicMin(bad_flag, (uint32_t)row);  // the FIRST such row (rows < 2^31)
    }
}

// rows ids[j] (0-based) of the float32 table, d values each, into the compact out [m][d]: one thread per value
__global__ void __launch_bounds__(256)
gather_rows_kernel(const float *X, int64_t stride, int32_t d, const int32_t *ids, int64_t m, float *out) {
    const int64_t total = m * d;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = e / d;
        const int32_t c = (int32_t)(e - j * d);
        out[e] = X[(int64_t)ids[j] * stride + c];
    }
}

} // namespace hnsw_dev

namespace hnsw_host {

int cosine_normalise(const float *in, int64_t n, int d, int64_t in_stride, float *out, int64_t out_stride, float *norms, uint32_t *bad_flag,
                     hipStream_t st, bool pad_rows) {
    if (n <= 0) return HNSW_OK;
    const int nch = pick_nch((d + 3) / 4);
    if (!nch) return fail(HNSW_ERR_UNSUPPORTED, "d=%d > 1024 not supported", d);
    const int32_t pad_to = pad_rows ? (int32_t)std::min<int64_t>(padded_stride(d), out_stride) : d;
    // 16-byte moves where both matrices allow them.  (A padded row's end, out_stride, is a multiple of 16 floats then.)
    const bool vec = in_stride % 4 == 0 && out_stride % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
    const dim3 grid((unsigned)((n + hnsw_dev::NORM_ROWS - 1) / hnsw_dev::NORM_ROWS)), block(64 * hnsw_dev::NORM_WAVES);
    with_nch(nch, [&](auto NCH) {
        if (vec) hipLaunchKernelGGL((hnsw_dev::cosine_normalise_kernel<NCH, true>), grid, block, 0, st, in, n, d, in_stride, out, out_stride, pad_to, norms, bad_flag);
        else hipLaunchKernelGGL((hnsw_dev::cosine_normalise_kernel<NCH, false>), grid, block, 0, st, in, n, d, in_stride, out, out_stride, pad_to, norms, bad_flag);
    });
    return launched("normalise kernel");
}

int cosine_store_rows(float *rows, int64_t m, int d, const char *what) {
    if (m <= 0) return HNSW_OK;
    const int64_t stride = padded_stride(d);
    DevFlag flag;
    uint32_t bad = 0xFFFFFFFFu;
    HIP_TRY(flag.alloc());
    HIP_TRY(flag.set(-1));
    int rc = cosine_normalise(rows, m, d, stride, rows, stride, nullptr, (uint32_t *)flag.p, nullptr, true);
    if (rc) return rc;
    HIP_TRY(flag.get((int32_t *)&bad));       // (the one read of the flag; it also waits for the kernel)
    if (bad != 0xFFFFFFFFu)
        return fail(HNSW_ERR_BAD_ARG, "cosine: the sum of squares of row %lld is NaN or infinite: %s", (long long)bad, what);
    return HNSW_OK;
}

int cosine_queries(::hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, hipStream_t st, const float **out_Q, int64_t *out_stride) {
    *out_Q = Q; *out_stride = q_stride;
    if (idx->info.metric != HNSW_METRIC_COSINE || nq <= 0 || !Q) return HNSW_OK;
    // one block per caller stream, kept between calls: work on one stream is ordered (as order_scratch)
    DevBuf *buf = nullptr;
    for (auto &s : idx->cosine_scratch) if (s.st == st) buf = &s.q;
    if (!buf) {
        idx->cosine_scratch.emplace_back();
        idx->cosine_scratch.back().st = st;
        buf = &idx->cosine_scratch.back().q;
    }
    int rc = buf->ensure(query_bytes(nq, q_stride, idx->iv.d));
    if (rc) return rc;
    if ((rc = cosine_normalise(Q, nq, idx->iv.d, q_stride, (float *)buf->p, q_stride, nullptr, nullptr, st, false))) return rc;
    *out_Q = (const float *)buf->p;
    return HNSW_OK;
}

} // namespace hnsw_host

using namespace hnsw_host;

extern "C" {

int32_t hnsw_normalise_batch(int32_t device, const float *in, int64_t n, int32_t d, int64_t in_stride, float *out, int64_t out_stride,
                             float *out_norms) {
    if (n < 0) return fail(HNSW_ERR_BAD_ARG, "n=%lld < 0", (long long)n);
    if (d < 1) return fail(HNSW_ERR_BAD_ARG, "d=%d", d);
    if (pick_nch((d + 3) / 4) == 0) return fail(HNSW_ERR_UNSUPPORTED, "d=%d > 1024 not supported", d);
    if (n == 0) return HNSW_OK;
    if (n > 0x7FFFFFF0LL) return fail(HNSW_ERR_BAD_ARG, "n=%lld out of range", (long long)n);
    if (!in || !out) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    if (in_stride < d || out_stride < d) return fail(HNSW_ERR_BAD_ARG, "stride < d");
    // (the matrix goes through the device in pieces: a piece's rows are written before the next piece is read)
    if (in == out && in_stride != out_stride) return fail(HNSW_ERR_BAD_ARG, "out is in: the strides must be equal (in_stride=%lld out_stride=%lld)", (long long)in_stride, (long long)out_stride);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(HNSW_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (device < 0 || device >= ndev) return fail(HNSW_ERR_BAD_ARG, "device %d out of range (have %d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    // in pieces of at most 64 MiB of input: the rows at the caller's stride in, the d values of each row out
    const int64_t piece = std::max<int64_t>(1, (64ll << 20) / (in_stride * 4));
    DevBuf dIn, dOut, dNorm;
    const int64_t rows = std::min(piece, n);
    int rc;
    if ((rc = dIn.ensure(query_bytes(rows, in_stride, d))) || (rc = dOut.ensure((size_t)rows * d * 4)) || (out_norms && (rc = dNorm.ensure((size_t)rows * 4))))
        return rc;
    for (int64_t r0 = 0; r0 < n; r0 += piece) {
        const int64_t nr = std::min(piece, n - r0);
        HIP_TRY(hipMemcpy(dIn.p, in + r0 * in_stride, query_bytes(nr, in_stride, d), hipMemcpyHostToDevice));
        if ((rc = cosine_normalise((const float *)dIn.p, nr, d, in_stride, (float *)dOut.p, d, out_norms ? (float *)dNorm.p : nullptr, nullptr, nullptr, false)))
            return rc;
        HIP_TRY(hipMemcpy2D(out + r0 * out_stride, (size_t)out_stride * 4, dOut.p, (size_t)d * 4, (size_t)d * 4, (size_t)nr, hipMemcpyDeviceToHost));
        if (out_norms) HIP_TRY(hipMemcpy(out_norms + r0, dNorm.p, (size_t)nr * 4, hipMemcpyDeviceToHost));
    }
    return HNSW_OK;
}

int32_t hnsw_index_get_rows(const hnsw_index *idx, const int64_t *ids, int64_t m, float *out, int64_t out_stride) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    const int64_t n = idx->iv.n;
    const int d = idx->iv.d;
    if (!ids && m != n) return fail(HNSW_ERR_BAD_ARG, "null ids: all rows in order, m must be n=%lld (m=%lld)", (long long)n, (long long)m);
    if (m == 0) return HNSW_OK;
    if (!out) return fail(HNSW_ERR_BAD_ARG, "null out");
    if (out_stride < d) return fail(HNSW_ERR_BAD_ARG, "out_stride < d");
    HIP_TRY(hipSetDevice(idx->device));
    if (!ids) {
        HIP_TRY(hipMemcpy2D(out, (size_t)out_stride * 4, idx->tables.X.p, (size_t)idx->iv.stride * 4, (size_t)d * 4, (size_t)n, hipMemcpyDeviceToHost));
        return HNSW_OK;
    }
    std::vector<int32_t> id0((size_t)m);
    for (int64_t j = 0; j < m; ++j) {
        const int64_t v = ids[j] - idx->iv.id_base;
        if (v < 0 || v >= n) return fail(HNSW_ERR_BAD_ARG, "Vector.get: id %lld out of range", (long long)ids[j]);
        id0[(size_t)j] = (int32_t)v;
    }
    // in pieces of at most 64 MiB of rows
    const int64_t piece = std::max<int64_t>(1, (64ll << 20) / ((int64_t)d * 4));
    const int64_t rows = std::min(piece, m);
    DevBuf dIds, dOut;
    int rc;
    if ((rc = dIds.ensure((size_t)rows * 4)) || (rc = dOut.ensure((size_t)rows * d * 4))) return rc;
    for (int64_t r0 = 0; r0 < m; r0 += piece) {
        const int64_t nr = std::min(piece, m - r0);
        HIP_TRY(hipMemcpy(dIds.p, id0.data() + r0, (size_t)nr * 4, hipMemcpyHostToDevice));
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(65536, (nr * d + 255) / 256));
        hipLaunchKernelGGL(hnsw_dev::gather_rows_kernel, dim3(blocks), dim3(256), 0, nullptr, (const float *)idx->tables.X.p, idx->iv.stride, d,
                           (const int32_t *)dIds.p, nr, (float *)dOut.p);
        if ((rc = launched("gather rows kernel"))) return rc;
        HIP_TRY(hipMemcpy2D(out + r0 * out_stride, (size_t)out_stride * 4, dOut.p, (size_t)d * 4, (size_t)d * 4, (size_t)nr, hipMemcpyDeviceToHost));
    }
    return HNSW_OK;
}

} // extern "C"
