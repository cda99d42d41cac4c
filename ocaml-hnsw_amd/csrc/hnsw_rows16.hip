// hnsw_rows16.hip -- half rows: a copy of the vectors rounded to fp16, for float data that is not byte-valued.
// The knn searches are bound by the bytes they gather per evaluation (profiles/r04_gather_ceiling.txt): a float32 row of
// d = 128 is four 128-byte lines, d = 96 or 100 three (plus a partial fourth).  The half copy stores chunk c of a row (dims
// 4c..4c+3) as 8 bytes in the knn kernel's lane grid -- rows of 128 * NCH bytes, zero padded -- so each of a 16-lane
// group's NCH loads is one whole line: two lines per evaluation for d <= 128.  The knn kernel's ROWS = 4 variants
// (hnsw_device.hip.h: hop_round) convert each half back to float (exact) and run the unchanged float32 arithmetic, so
// their results are those of the same search over Xh = X rounded to fp16, bit for bit.  That is not the search over X:
// the copy is made on request only (option "half_rows"), never by default.  The float32 rows stay: the builder, the layer
// operators, hnsw_distance_batch and hnsw_index_insert's searches use them.
#include "hnsw_internal.h"

using namespace hnsw_host;

namespace {

// the magnitude bits from which a float32 rounds to an fp16 infinity: 65520 = 65504 + half an fp16 step (a tie, which
// round-to-nearest-even sends up); NaN and +-inf lie above it too
constexpr uint32_t HALF_OVERFLOW_BITS = 0x477FF000u;

// float32 -> fp16 bits, round to nearest, ties to even; fp16 subnormals and the sign of zero kept (numpy's astype(float16)).
// Integer arithmetic: the result does not depend on the device's rounding or denormal modes.  |x| < 65520 and not NaN.
__device__ __forceinline__ uint32_t f32_to_f16_rne(uint32_t x) {
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a >= 0x38800000u) {                  // |x| >= 2^-14: a normal fp16.  Exponent rebiased (127 -> 15), 13 bits rounded off
        const uint32_t r = a - 0x38000000u;  // (a carry out of the mantissa steps the exponent: still the right bits)
        return sign | ((r + 0x0FFFu + ((r >> 13) & 1u)) >> 13);
    }
    if (a <= 0x33000000u) return sign;       // |x| <= 2^-25: half the smallest subnormal or less rounds to (signed) zero
    // an fp16 subnormal: |x| / 2^-24 rounded, |x| = mant * 2^(e - 150) with the implicit bit, e in 102..112
    const uint32_t e = a >> 23, mant = (a & 0x7FFFFFu) | 0x800000u, sh = 126u - e;   // sh in 14..24
    const uint32_t q = mant >> sh, rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
}

// flag[0] is cleared when a value is NaN or rounds to an fp16 infinity
__global__ void __launch_bounds__(256)
rows_fit_half_kernel(const float *X, int64_t stride, int64_t n, int32_t d, int32_t *flag) {
    const int64_t total = n * (int64_t)d;
    bool ok = true;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / d;
        ok = ok && (__float_as_uint(X[row * stride + (e - row * d)]) & 0x7FFFFFFFu) < HALF_OVERFLOW_BITS;
    }
    if (!ok) flag[0] = 0;
}

// one thread per chunk of the half rows: halves 4c..4c+3 of a row are dims 4c..4c+3 (0 beyond d), low half first
__global__ void __launch_bounds__(256)
pack_half_rows_kernel(const float *X, int64_t stride, int64_t n, int32_t d, uint2 *Xh, int32_t chunks_per_row) {
    const int64_t total = n * (int64_t)chunks_per_row;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = w / chunks_per_row;
        const int c = (int)(w - row * chunks_per_row);
        uint32_t h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * c + j;
            h[j] = e < d ? f32_to_f16_rne(__float_as_uint(X[row * stride + e])) : 0u;
        }
        Xh[w] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    }
}

} // namespace

namespace hnsw_host {

int make_half_rows(::hnsw_index *idx) {
    if (!idx || !idx->tables.X.p || idx->iv.n <= 0) return HNSW_OK;
    HIP_TRY(hipSetDevice(idx->device));
    const int64_t n = idx->iv.n;
    const int32_t d = idx->iv.d;
    const int32_t chunks = 16 * pick_nch(idx->iv.nchunks);        // the lane grid of the kernel: 16 lanes x NCH chunks of 8 bytes
    DevFlag flag;
    int32_t ok = 0;
    HIP_TRY(flag.alloc());
    hipError_t e = flag.set(1);
    if (e == hipSuccess) {
        const int blocks = (int)std::min<int64_t>(65536, (n * (int64_t)d + 255) / 256);
        hipLaunchKernelGGL(rows_fit_half_kernel, dim3((unsigned)std::max(1, blocks)), dim3(256), 0, 0,
                           (const float *)idx->tables.X.p, idx->iv.stride, n, d, (int32_t *)flag.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = flag.get(&ok);
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "half-row check failed: %s", hipGetErrorString(e));
    if (!ok) return fail(HNSW_ERR_UNSUPPORTED, "half rows: a value is NaN or rounds to an fp16 infinity (|x| >= 65520)");
    Table &Xh = idx->tables.Xh;
    e = Xh.alloc((size_t)n * (size_t)chunks * 8);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? HNSW_ERR_OOM : HNSW_ERR_HIP, "half rows: no room for %lld bytes: %s",
                    (long long)(n * chunks * 8), hipGetErrorString(e));
    const int blocks = (int)std::min<int64_t>(65536, (n * (int64_t)chunks + 255) / 256);
    hipLaunchKernelGGL(pack_half_rows_kernel, dim3((unsigned)std::max(1, blocks)), dim3(256), 0, 0,
                       (const float *)idx->tables.X.p, idx->iv.stride, n, d, (uint2 *)Xh.p, chunks);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { Xh.release(); return fail(HNSW_ERR_HIP, "half-row packing failed: %s", hipGetErrorString(e)); }
    return HNSW_OK;
}

} // namespace hnsw_host
