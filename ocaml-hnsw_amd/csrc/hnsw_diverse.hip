// hnsw_diverse.hip -- diversified k-NN: greedy maximal marginal relevance over a pool of candidates, on the device
// (hnsw_diversify_batch / _device, and the two searches that run it behind their inner call: hnsw_search_batch_diverse,
// hnsw_brute_force_batch_diverse).  The definition: include/hnsw_mi355x.h, the last section; the plain arithmetic: hnsw_diverse_plan.h.
//
// hnsw_diversify_kernel<NCH, METRIC>: one wave per query.
//   1. The row of candidate ids is compacted into LDS and (2.) evaluated against the query over the FLOAT32 rows, then the words
//      (key << 32 | node) are sorted -- the first three steps of hnsw_rerank_kernel, so a candidate's position is its rank in
//      hnsw_rerank_batch's row and its key the bits of hnsw_distance_batch.
//   3. The candidates become the ACTIVE list, four columns in LDS: node, relevance key, rank, m (+inf).  Pick 1 is rank 0.  A round:
//      the last pick's float32 row is loaded the way a query is (load_query, into the registers the query no longer needs),
//      eval_candidates runs over the active nodes -- a dense list, so its groups of four stay full --, every lane folds the pair
//      distance into m and forms g (hnsw_diverse::score: three rounded operations) for its candidates, and the wave takes the minimum
//      of the words (g ordered, rank, slot) by DPP row rotations and four lane reads.  The winner is written out and its slot refilled
//      from the end of the list: the list stays dense, its order means nothing (the rank travels in the column).
//   4. Past the picks the fill.
// LDS per wave: hnsw_diverse::lds_bytes -- 20 bytes per slot of the power of two at or above cand_stride plus the evaluation's 64
// scratch words.  The sort's words are dead once the columns are filled and rank and m live in their place.
#include "hnsw_internal.h"
#include "hnsw_diverse_plan.h"

namespace hnsw_dev {

struct DiverseArgs {
    const float *Q;
    int64_t q_stride, nq;
    const int32_t *cand;       // [nq][cand_stride], id_base-based
    int32_t cand_stride;
    int32_t cap;               // candidate slots in LDS: hnsw_diverse::slots_for(cand_stride)
    int32_t k, fill;
    float lambda, mu;
    int32_t *out_ids;          // [nq][k], in selection order
    float *out_dist;
    float *out_div;            // optional
};

constexpr uint64_t DIVERSE_EMPTY = ~0ull;  // no candidate: above every real word

// the smaller of two 64-bit words held as halves, this lane's against the lane's that the DPP control names
template <int CTRL> __device__ __forceinline__ void dpp_min_u64(uint32_t &hi, uint32_t &lo) {
    const uint32_t th = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, 0xF, 0xF, true);
    const uint32_t tl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, 0xF, 0xF, true);
    const bool less = th < hi || (th == hi && tl < lo);
    hi = less ? th : hi;
    lo = less ? tl : lo;
}
// minimum over the wave (wave-uniform result; every lane takes part): wave_min_u32's shape for 64-bit words
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t w) {
    uint32_t hi = (uint32_t)(w >> 32), lo = (uint32_t)w;
    dpp_min_u64<0x128>(hi, lo);   // row_ror:8
    dpp_min_u64<0x124>(hi, lo);   // row_ror:4
    dpp_min_u64<0x122>(hi, lo);   // row_ror:2
    dpp_min_u64<0x121>(hi, lo);   // row_ror:1
    uint64_t best = ((uint64_t)rdlane(hi, 0) << 32) | rdlane(lo, 0);
#pragma unroll
    for (int row = 16; row < 64; row += 16) {
        const uint64_t o = ((uint64_t)rdlane(hi, row) << 32) | rdlane(lo, row);
        best = o < best ? o : best;
    }
    return best;
}

template <int NCH, int METRIC>
__global__ void __launch_bounds__(64)
hnsw_diversify_kernel(const IndexView iv, const DiverseArgs a) {
    extern __shared__ uint64_t diverse_lds[];
    constexpr int RB = hnsw_host::rows_in_flight(NCH);
    const int lane = threadIdx.x, r = lane >> 4, l16 = lane & 15;
    const int64_t q = blockIdx.x;
    if (q >= a.nq) return;
    uint64_t *const words = diverse_lds;                                       // [cap] the sort; then rank and m of the active list
    int32_t *const ids = reinterpret_cast<int32_t *>(words + a.cap);           // [cap] nodes: as given, then the active list's
    uint32_t *const keys = reinterpret_cast<uint32_t *>(ids + a.cap);          // [cap] relevance keys, likewise
    uint32_t *const pkeys = keys + a.cap;                                      // [cap] a round's pair keys
    uint32_t *const trash = pkeys + a.cap;                                     // [64]
    int32_t *const rank = reinterpret_cast<int32_t *>(words);                  // [cap]
    float *const m = reinterpret_cast<float *>(rank + a.cap);                  // [cap]

    float4 qv[NCH];
    load_query<NCH>(qv, a.Q + q * a.q_stride, iv.d, l16);

    // 1. the real candidates, 0-based, in the order given
    const int32_t *row = a.cand + q * (int64_t)a.cand_stride;
    int cnt = 0;
    for (int j0 = 0; j0 < a.cand_stride; j0 += 64) {
        const int j = j0 + lane;
        const int64_t v = j < a.cand_stride ? (int64_t)row[j] - iv.id_base : -1;
        const bool real = v >= 0 && v < iv.n;
        const uint64_t mask = ballot(real);
        if (real) ids[cnt + popc(mask & ((1ull << lane) - 1ull))] = (int32_t)v;
        cnt += popc(mask);
    }
    __syncthreads();

    // 2. their keys over the float32 rows, sorted as (key, node) words: position = rank
    eval_candidates<NCH, RB, METRIC>(iv, qv, ids, keys, trash, cnt, r, l16);
    __syncthreads();
    int P = 2;
    while (P < cnt) P <<= 1;           // (P <= cap: cnt <= cand_stride <= cap, a power of two)
    for (int j = lane; j < P; j += 64) words[j] = j < cnt ? ((uint64_t)keys[j] << 32) | (uint32_t)ids[j] : DIVERSE_EMPTY;
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

    // 3. the active list in rank order: nodes and relevance keys out of the words, then rank and m over the words
    for (int j = lane; j < cnt; j += 64) {
        const uint64_t e = words[j];
        ids[j] = (int32_t)(uint32_t)e;
        keys[j] = (uint32_t)(e >> 32);
    }
    __syncthreads();
    for (int j = lane; j < cnt; j += 64) { rank[j] = j; m[j] = __uint_as_float(0x7F800000u); }
    __syncthreads();

    const int picks = a.k < cnt ? a.k : cnt;
    int32_t *const oi = a.out_ids + q * a.k;
    float *const od = a.out_dist + q * a.k;
    float *const ov = a.out_div ? a.out_div + q * a.k : nullptr;
    int na = cnt;                      // the active list's length (wave-uniform)
    int slot = 0;                      // where the pick about to be written sits in it
    for (int t = 0; t < picks; ++t) {
        if (t > 0) {
            eval_candidates<NCH, RB, METRIC>(iv, qv, ids, pkeys, trash, na, r, l16);
            __syncthreads();
            uint64_t best = DIVERSE_EMPTY;
            for (int j = lane; j < na; j += 64) {
                const float dv = key_to_dist<METRIC>(pkeys[j]);
                const float mo = m[j], mn = dv < mo ? dv : mo;
                m[j] = mn;
                const float g = hnsw_diverse::score(a.lambda, a.mu, key_to_dist<METRIC>(keys[j]), mn);
                const uint64_t w = hnsw_diverse::pick_word(g, (uint32_t)rank[j], (uint32_t)j);
                best = w < best ? w : best;
            }
            slot = (int)(wave_min_u64(best) & 0xFFFFu);
            __syncthreads();
        }
        // the pick: written out, its row the next round's query, its slot refilled from the end of the list
        const int32_t s = ids[slot];
        const uint32_t sk = keys[slot];
        const float sm = m[slot];
        const int last = na - 1;
        const int32_t li = ids[last], lr = rank[last];
        const uint32_t lk = keys[last];
        const float lm = m[last];
        __syncthreads();
        if (lane == 0) {
            oi[t] = s + iv.id_base;
            od[t] = key_to_dist<METRIC>(sk);
            if (ov) ov[t] = sm;
            ids[slot] = li; keys[slot] = lk; rank[slot] = lr; m[slot] = lm;
        }
        na = last;
        __syncthreads();
        if (t + 1 < picks) load_query<NCH>(qv, iv.X + (int64_t)s * iv.stride, iv.d, l16);
    }

    // 4. past the picks the fill
    const float ff = a.fill == 0 ? __uint_as_float(0x7FC00000u) : __uint_as_float(0x7F800000u);
    for (int j = picks + lane; j < a.k; j += 64) {
        oi[j] = -1;
        od[j] = ff;
        if (ov) ov[j] = ff;
    }
}

} // namespace hnsw_dev

namespace hnsw_host {

using hnsw_dev::DiverseArgs;

int check_diversify(const hnsw_index *idx, int64_t nq, int64_t q_stride, int32_t cand_stride, int32_t k, float lambda, int32_t fill, bool buffers) {
    const char *why = nullptr;
    const int rc = hnsw_diverse::check_args(nq, cand_stride, k, fill, lambda, &why);
    if (rc) return fail(rc, why, cand_stride, k);
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (nq == 0) return HNSW_OK;
    if (!buffers) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    if (q_stride < idx->iv.d) return fail(HNSW_ERR_BAD_ARG, "q_stride < d");
    return HNSW_OK;
}

int launch_diversify(hnsw_index *idx, const float *Q, int64_t nq, int64_t q_stride, const int32_t *cand, int32_t cand_stride, int32_t k,
                     float lambda, int32_t fill, int32_t *out_ids, float *out_dist, float *out_div, hipStream_t st) {
    const int cap = hnsw_diverse::slots_for(cand_stride);
    const DiverseArgs a{Q, q_stride, nq, cand, cand_stride, cap, k, fill, lambda, hnsw_diverse::mu_of(lambda), out_ids, out_dist, out_div};
    with_metric(idx->info.metric, [&](auto METRIC) { with_nch(pick_nch(idx->iv.nchunks), [&](auto NCH) {
        hipLaunchKernelGGL((hnsw_dev::hnsw_diversify_kernel<NCH, METRIC>), dim3((unsigned)nq), dim3(64), hnsw_diverse::lds_bytes(cap), st, idx->iv, a);
    }); });
    return launched("diversify kernel");
}

// the pool of a diverse search: k <= pool <= top (ef, or 1024 for the exact scan)
static int check_pool(int32_t k, int32_t pool, int32_t top, const char *top_name) {
    if (pool > 1024) return fail(HNSW_ERR_UNSUPPORTED, "pool=%d > 1024 not supported", pool);
    if (pool < k || pool > top) return fail(HNSW_ERR_BAD_ARG, "pool must lie in k..%s (k=%d pool=%d %s=%d)", top_name, k, pool, top_name, top);
    return HNSW_OK;
}
static int check_lambda(float lambda) {
    return hnsw_diverse::lambda_ok(lambda) ? HNSW_OK : fail(HNSW_ERR_BAD_ARG, "lambda must lie in [0, 1] and not be NaN");
}

} // namespace hnsw_host

using namespace hnsw_host;

extern "C" {

int32_t hnsw_diversify_batch_device(hnsw_index *idx, const float *d_queries, int64_t nq, int64_t q_stride, const int32_t *d_cand,
                                    int32_t cand_stride, int32_t k, float lambda, int32_t fill, int32_t *d_ids, float *d_dist, float *d_div,
                                    void *stream) {
    int rc = check_diversify(idx, nq, q_stride, cand_stride, k, lambda, fill, d_queries && d_cand && d_ids && d_dist);
    if (rc || nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    if ((rc = cosine_queries(idx, d_queries, nq, q_stride, (hipStream_t)stream, &d_queries, &q_stride))) return rc;     // (COSINE: N(Q) first)
    return launch_diversify(idx, d_queries, nq, q_stride, d_cand, cand_stride, k, lambda, fill, d_ids, d_dist, d_div, (hipStream_t)stream);
}

int32_t hnsw_diversify_batch(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, const int32_t *cand, int32_t cand_stride,
                             int32_t k, float lambda, int32_t fill, int32_t *out_ids, float *out_dist, float *out_div) {
    int rc = check_diversify(idx, nq, q_stride, cand_stride, k, lambda, fill, queries && cand && out_ids && out_dist);
    if (rc || nq == 0) return rc;
    const int64_t top = (int64_t)idx->iv.id_base + idx->iv.n;
    for (int64_t i = 0; i < nq * cand_stride; ++i)         // (below id_base: padding)
        if (cand[i] >= top) return fail(HNSW_ERR_BAD_ARG, "Vector.get: candidate id %d out of range", cand[i]);
    HIP_TRY(hipSetDevice(idx->device));
    HostInput cd;                                          // the candidates: in place, or staged in refine_scratch.ids
    HostCall c;
    const size_t rbytes = (size_t)nq * k * 4;
    if ((rc = cd.resolve(cand, (size_t)nq * cand_stride * 4, idx->refine_scratch.ids)) || (out_div && (rc = idx->diverse_scratch.div.ensure(rbytes))) ||
        (rc = c.begin(idx, queries, nq, q_stride, k, out_ids, out_dist, nullptr, nullptr, false))) return rc;
    hipStream_t st = idx->hs[0];
    float *const d_div = out_div ? (float *)idx->diverse_scratch.div.p : nullptr;
    if (!(rc = cd.upload(st)))
        rc = launch_diversify(idx, c.b.Q, nq, q_stride, (const int32_t *)cd.dev, cand_stride, k, lambda, fill, c.b.ids, c.b.dist, d_div, st);
    if (!rc && out_div && hipMemcpyAsync(out_div, d_div, rbytes, hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(HNSW_ERR_HIP, "diversity download failed");
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    return c.finish(idx, "diversify", st);
}

int32_t hnsw_search_batch_diverse(hnsw_index *idx, const hnsw_filter *filter, const float *queries, int64_t nq, int64_t q_stride,
                                  const hnsw_search_params *params, int32_t pool, float lambda, int32_t *out_ids, float *out_dist, float *out_div,
                                  uint32_t *out_nd, uint32_t *out_nh, uint32_t *out_status) {
    int rc = check_lambda(lambda);
    if (rc) return rc;
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (!params) return fail(HNSW_ERR_BAD_ARG, "null params");
    if ((rc = check_pool(params->k, pool, params->ef, "ef"))) return rc;
    if (nq > 0 && !(queries && out_ids && out_dist)) return fail(HNSW_ERR_BAD_ARG, "null buffer");
    // the inner call at k := pool, its rows left on the device; HostCall::finish runs the selection over them and downloads [nq][k]
    hnsw_search_params inner = *params;
    inner.k = pool;
    const DiverseOut dv{params->k, lambda, params->fill, out_ids, out_dist, out_div};
    if (filter) return filtered_host_call(idx, filter, queries, nq, q_stride, &inner, nullptr, nullptr, out_nd, out_nh, out_status, nullptr, nullptr, &dv);
    return knn_host_call(idx, queries, nq, q_stride, &inner, nullptr, nullptr, out_nd, out_nh, out_status, nullptr, nullptr, &dv);
}

int32_t hnsw_brute_force_batch_diverse(hnsw_index *idx, const float *queries, int64_t nq, int64_t q_stride, int32_t k, int32_t pool, float lambda,
                                       int32_t fill, int32_t *out_ids, float *out_dist, float *out_div) {
    int rc = check_lambda(lambda);
    if (rc || (rc = check_scan(idx, nq, q_stride, k, fill, queries && out_ids && out_dist)) || (rc = check_pool(k, pool, 1024, "1024")) || nq == 0) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    const DiverseOut dv{k, lambda, fill, out_ids, out_dist, out_div};
    HostCall c;
    c.dv = &dv;
    if ((rc = c.begin(idx, queries, nq, q_stride, pool, nullptr, nullptr, nullptr, nullptr, false))) return rc;
    const hnsw_filter *const live = live_filter(idx);
    rc = scan_search(idx, c.b, pool, fill, idx->hs[0], live ? live->table() : nullptr);
    if (rc) { (void)hipStreamSynchronize(idx->hs[0]); return rc; }
    return c.finish(idx, "diverse scan", idx->hs[0]);
}

} // extern "C"
