// hnsw_rerank.hip -- exact re-ranking of given candidates (hnsw_rerank_batch / _device), and with it the refine step of the
// half-row searches (option "refine", hnsw_capi.hip): per query a list of up to 1024 node ids is evaluated against the FLOAT32
// rows (iv.X, whatever rows the knn searches read) and the k smallest under (distance, id) are returned.
//
// hnsw_rerank_kernel<NCH, METRIC>: one wave per query.
//   1. The row of candidate ids is compacted into LDS: entries below id_base (padding) or past the last node are dropped.
//   2. eval_candidates -- the 16-lane groups, fmaf chain and reduce16 tree of every other kernel here, so a pair's key is the
//      bits hnsw_distance_batch and the float32 searches give it -- leaves the ordered keys in LDS.
//   3. The 64-bit words (key << 32 | node) are sorted in LDS by a bitonic network over the next power of two (padded with
//      all-ones words): ascending words = the total order (distance, id) of hnsw_brute_force_batch.  Nothing is ever dropped,
//      so equal distances come lowest id first however many there are.
//   4. The first k words are written as id + id_base and key_to_dist; past the real candidates the fill.
// LDS per wave: 16 bytes per candidate slot (words, ids, keys) of the power of two at or above cand_stride, plus the evaluation's
// 64 scratch words: 2.3 KB at 128 candidates (the registers bound the residency), 16.6 KB at 1024 (nine waves per CU).
#include "hnsw_internal.h"

namespace hnsw_dev {

struct RerankArgs {
    const float *Q;
    int64_t q_stride, nq;
    const int32_t *cand;       // [nq][cand_stride], id_base-based
    int32_t cand_stride;
    int32_t cap;               // candidate slots in LDS: a power of two, 64 <= cap, cand_stride <= cap <= 1024
    int32_t k, fill;
    int32_t *out_ids;          // [nq][k]
    float *out_dist;
    const uint32_t *nd_in;     // optional (the refine step): out_nd[q] = nd_in[q] + the number of candidates evaluated
    uint32_t *nd_out;
};

constexpr uint64_t RERANK_EMPTY = ~0ull;   // no candidate: above every real word

__host__ __device__ inline size_t rerank_lds_bytes(int cap) { return (size_t)cap * 16 + 64 * 4; }

template <int NCH, int METRIC>
__global__ void __launch_bounds__(64)
hnsw_rerank_kernel(const IndexView iv, const RerankArgs a) {
    extern __shared__ uint64_t rerank_lds[];
    constexpr int RB = hnsw_host::rows_in_flight(NCH);
    const int lane = threadIdx.x, r = lane >> 4, l16 = lane & 15;
    const int64_t q = blockIdx.x;
    if (q >= a.nq) return;
    uint64_t *const words = rerank_lds;                                        // [cap]
    int32_t *const ids = reinterpret_cast<int32_t *>(words + a.cap);           // [cap]
    uint32_t *const keys = reinterpret_cast<uint32_t *>(ids + a.cap);          // [cap]
    uint32_t *const trash = keys + a.cap;                                      // [64]

    float4 qv[NCH];
    load_query<NCH>(qv, a.Q + q * a.q_stride, iv.d, l16);

    // 1. the real candidates, 0-based, in the order given
    const int32_t *row = a.cand + q * (int64_t)a.cand_stride;
    int cnt = 0;
    for (int j0 = 0; j0 < a.cand_stride; j0 += 64) {
        const int j = j0 + lane;
        const int64_t v = j < a.cand_stride ? (int64_t)row[j] - iv.id_base : -1;
        const bool real = v >= 0 && v < iv.n;
        const uint64_t m = ballot(real);
        if (real) ids[cnt + popc(m & ((1ull << lane) - 1ull))] = (int32_t)v;
        cnt += popc(m);
    }
    __syncthreads();

    // 2. their keys over the float32 rows
    eval_candidates<NCH, RB, METRIC>(iv, qv, ids, keys, trash, cnt, r, l16);
    __syncthreads();

    // 3. sorted as (key, node) words
    int P = 2;
    while (P < cnt) P <<= 1;           // (P <= cap: cnt <= cand_stride <= cap, a power of two)
    for (int j = lane; j < P; j += 64) words[j] = j < cnt ? ((uint64_t)keys[j] << 32) | (uint32_t)ids[j] : RERANK_EMPTY;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int dist = size >> 1; dist > 0; dist >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int lo = ((t & ~(dist - 1)) << 1) | (t & (dist - 1)), hi = lo | dist;
                const uint64_t x = words[lo], y = words[hi];
                if ((x > y) == ((lo & size) == 0)) { words[lo] = y; words[hi] = x; }
            }
            __syncthreads();
        }
    }

    // 4. the first k
    for (int j = lane; j < a.k; j += 64) {
        int32_t oid = -1;
        float od = a.fill == 0 ? __uint_as_float(0x7FC00000u) : __uint_as_float(0x7F800000u);
        if (j < cnt) {
            const uint64_t e = words[j];
            oid = (int32_t)(uint32_t)e + iv.id_base;
            od = key_to_dist<METRIC>((uint32_t)(e >> 32));
        }
        a.out_ids[q * a.k + j] = oid;
        a.out_dist[q * a.k + j] = od;
    }
    if (lane == 0 && a.nd_out) a.nd_out[q] = (a.nd_in ? a.nd_in[q] : 0u) + (uint32_t)cnt;
}

} // namespace hnsw_dev

namespace hnsw_host {

using hnsw_dev::RerankArgs;

int check_rerank(const hnsw_index *idx, int64_t nq, int64_t q_stride, int32_t cand_stride, int32_t k, int32_t fill, bool buffers) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (cand_stride < 1) return fail(HNSW_ERR_BAD_ARG, "cand_stride must be >= 1 (cand_stride=%d)", cand_stride);
    if (cand_stride > 1024) return fail(HNSW_ERR_UNSUPPORTED, "cand_stride=%d > 1024 not supported", cand_stride);
    if (k < 1 || k > cand_stride) return fail(HNSW_ERR_BAD_ARG, "k must be in 1..cand_stride (k=%d cand_stride=%d)", k, cand_stride);
    if (fill != HNSW_FILL_OHNSW && fill != HNSW_FILL_BA) return fail(HNSW_ERR_BAD_ARG, "bad fill %d", fill);
    if (nq < 0 || nq > 0x7FFFFFFFLL) return fail(HNSW_ERR_BAD_ARG, "nq=%lld out of range", (long long)nq);
    if (nq == 0) return HNSW_OK;
    if (!buffers) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    if (q_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "q_stride < d");
    return HNSW_OK;
}

int launch_rerank(hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, const int32_t *cand, int32_t cand_stride, int32_t k,
                  int32_t fill, int32_t *out_ids, float *out_dist, const uint32_t *nd_in, uint32_t *nd_out, hipStream_t st) {
    int cap = 64;
    while (cap < cand_stride) cap <<= 1;
    const RerankArgs a{Q, q_stride, nq, cand, cand_stride, cap, k, fill, out_ids, out_dist, nd_in, nd_out};
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(pick_nch(idx->iv.nchunks), [&](auto NCH) {
        hipLaunchKernelGGL((hnsw_dev::hnsw_rerank_kernel<NCH, METRIC>), dim3((unsigned)nq), dim3(64), hnsw_dev::rerank_lds_bytes(cap), st, idx->iv, a);
    }); });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HNSW_ERR_HIP, "re-rank kernel launch failed: %s", hipGetErrorString(e));
    return HNSW_OK;
}

} // namespace hnsw_host

using namespace hnsw_host;

extern "C" {

int32_t hnsw_rerank_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride, const int32_t *d_cand,
                                 int32_t cand_stride, int32_t k, int32_t fill, int32_t *d_ids, float *d_dist, void *stream) {
    int rc = check_rerank(idx, nq, q_stride, cand_stride, k, fill, d_queries && d_cand && d_ids && d_dist);
    if (rc || nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    if ((rc = cosine_queries(idx, d_queries, nq, q_stride, (hipStream_t)stream, &d_queries, &q_stride))) return rc;     // (COSINE: N(Q) first)
    return launch_rerank(idx, d_queries, nq, q_stride, d_cand, cand_stride, k, fill, d_ids, d_dist, nullptr, nullptr, (hipStream_t)stream);
}

int32_t hnsw_rerank_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, const int32_t *cand, int32_t cand_stride,
                          int32_t k, int32_t fill, int32_t *out_ids, float *out_dist) {
    int rc = check_rerank(idx, nq, q_stride, cand_stride, k, fill, queries && cand && out_ids && out_dist);
    if (rc || nq == 0) return rc;
    const int64_t top = (int64_t)idx->iv.id_base + idx->iv.n;
    for (int64_t i = 0; i < nq * cand_stride; ++i)         // (below id_base: padding)
        if (cand[i] >= top) return fail(HNSW_ERR_BAD_ARG, "Vector.get: candidate id %d out of range", cand[i]);
    HIP_TRY(hipSetDevice(idx->device));
    HostInput cd;                                          // the candidates: in place, or staged in refine_scratch.ids
    HostCall c;
    if ((rc = cd.resolve(cand, (size_t)nq * cand_stride * 4, idx->refine_scratch.ids)) ||
        (rc = c.begin(idx, queries, nq, q_stride, k, out_ids, out_dist, nullptr, nullptr, false))) return rc;
    hipStream_t st = idx->hs[0];
    if (!(rc = cd.upload(st)))
        rc = launch_rerank(idx, c.b.Q, nq, q_stride, (const int32_t *)cd.dev, cand_stride, k, fill, c.b.ids, c.b.dist, nullptr, nullptr, st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    return c.finish(idx, "re-rank", st);
}

} // extern "C"
