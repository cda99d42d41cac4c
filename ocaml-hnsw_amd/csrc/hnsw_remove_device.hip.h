// hnsw_remove_device.hip.h -- gfx950 kernels of hnsw_index_remove (the contract: include/hnsw_mi355x.h, "hard deletion").
//
// Every kernel READS THE OLD TABLES ONLY (rv.iv) and writes tables of the new index or scratch of its own, so no result depends on
// the order in which nodes are processed; nothing depends on atomic arrival order either (there is no atomic here).
//   remove_copy     every live row, every layer: its live entries, order kept, renumbered, into the new tables; flags the rows
//                   that listed a removed node (the TOUCHED nodes of that layer)
//   remove_gather   the vectors of the live nodes into the new table
//   per layer, one wave per touched node u (the host lists them in ascending id order):
//   remove_propose  PROPOSE: live(u), C(u) gathered from the removed neighbours' rows (first occurrence kept, at most 1024 with
//                   live(u)), eval_candidates, rank sort by (key, id), select_heuristic with kept0 = |live(u)|: S(u), and the
//                   proposals (target << 32 | proposer), which the host groups per target with a radix sort
//   remove_offer    OFFER: U(u) = S(u) + the proposers of u, ordered by (hnsw_distance_batch's value, id); T(u) = its first
//                   cap - |live(u)| entries
//   remove_agree    AGREE: the w of T(u) with u in T(w), in T's order, appended to u's new row
#pragma once

#include "hnsw_build_device.hip.h"

namespace hnsw_dev {

constexpr int REMOVE_CAND = 1024;        // |live(u)| + |C(u)| stops here: what select_neighbours_kernel takes at most
constexpr int REMOVE_ROW = 64;           // entries of a row of S / T (a cap is at most 64)

struct RemoveView {
    IndexView iv;                        // the OLD index
    const int32_t *new_id;               // [iv.n] new 0-based id, -1 = removed
    int32_t *nbr0_new, *nbrU_new;        // the new index's rows (every slot -1 before remove_copy) ...
    const int2 *ref_new;                 // ... and its upper layout, by new id
};
struct RemoveLayer {
    const int32_t *list;                 // [t] the touched nodes of the layer (old ids), ascending
    int32_t t, layer, cap;
    const int32_t *tidx;                 // [iv.n] position in list, -1 = not touched on this layer
    int32_t *nlive;                      // [t] |live(u)|
    int32_t *S;                          // [t][REMOVE_ROW] S(u) (old ids) in selection order, -1 padded
    uint64_t *props;                     // [t][cap] (w << 32 | u) for w in S(u), ~0 = none
    const uint64_t *props_sorted;        // the same, ascending
    int32_t *T;                          // [t][REMOVE_ROW] T(u) (old ids) in order, -1 padded
};

__device__ __forceinline__ const int32_t *old_row(const IndexView &iv, int layer, int node, int &width) {
    if (layer == 0) { width = iv.S0; return iv.nbr0 + (int64_t)node * iv.S0; }
    width = iv.SU;
    return iv.nbrU + ((int64_t)iv.upper_ref[node].x + (layer - 1)) * iv.SU;
}
__device__ __forceinline__ int32_t *new_row(const RemoveView &rv, int layer, int new_node) {
    if (layer == 0) return rv.nbr0_new + (int64_t)new_node * rv.iv.S0;
    return rv.nbrU_new + ((int64_t)rv.ref_new[new_node].x + (layer - 1)) * rv.iv.SU;
}
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// One wave per old node (four per block).  touched: [layers][iv.n] bytes, zero before.
__global__ void __launch_bounds__(256) remove_copy_kernel(const RemoveView rv, uint8_t *touched, int32_t layers) {
    const IndexView &iv = rv.iv;
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= iv.n) return;
    const int nv = rv.new_id[v];
    if (nv < 0) return;
    const int top = iv.upper_ref[v].y;
    for (int l = 0; l <= top && l < layers; ++l) {
        int width;
        const int32_t *row = old_row(iv, l, (int)v, width);
        const int e = lane < width ? row[lane] : -1;
        const bool valid = e >= 0 && e < iv.n;
        const int ne = valid ? rv.new_id[e] : -1;
        const uint64_t lm = ballot(ne >= 0), dm = ballot(valid && ne < 0);
        if (ne >= 0) new_row(rv, l, nv)[popc(lm & lanes_below(lane))] = ne;
        if (lane == 0 && dm != 0ull) touched[(int64_t)l * iv.n + v] = 1;
    }
}

// one thread per float4 of the old table
__global__ void __launch_bounds__(256) remove_gather_kernel(const float4 *X, int64_t n, int32_t stride4, const int32_t *new_id, float4 *Xn) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * stride4) return;
    const int64_t v = e / stride4;
    const int nv = new_id[v];
    if (nv >= 0) Xn[(int64_t)nv * stride4 + (e - v * stride4)] = X[e];
}

__global__ void __launch_bounds__(256) remove_index_kernel(const int32_t *list, int32_t t, int32_t *tidx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < t) tidx[list[i]] = i;
}

// ---- PROPOSE --------------------------------------------------------------------------------------------------------------
// LDS: (4 * 1024 + 128) words, as select_neighbours_kernel at 1024 candidates.
template <int NCH, int RB, int METRIC>
__global__ void __launch_bounds__(64) remove_propose_kernel(const RemoveView rv, const RemoveLayer la) {
    extern __shared__ uint32_t lds[];
    constexpr int CS = REMOVE_CAND;
    int32_t *c_id = reinterpret_cast<int32_t *>(lds);
    uint32_t *c_key = lds + CS;
    int32_t *s_id = reinterpret_cast<int32_t *>(lds + 2 * CS);
    uint32_t *s_key = lds + 3 * CS;
    int32_t *k_id = reinterpret_cast<int32_t *>(lds + 4 * CS);
    uint32_t *trash = lds + 4 * CS + 64;
    const IndexView &iv = rv.iv;
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    if (i >= la.t) return;
    const int u = la.list[i];
    int nl, nd;
    {   // live(u) -> k_id (forced, in row order); u's removed neighbours, in row order -> s_id (free until the sort)
        int width;
        const int32_t *row = old_row(iv, la.layer, u, width);
        const int e = lane < width ? row[lane] : -1;
        const bool valid = e >= 0 && e < iv.n;
        const bool lv = valid && rv.new_id[e] >= 0;
        const uint64_t lm = ballot(lv), dm = ballot(valid && !lv);
        nl = popc(lm); nd = popc(dm);
        if (lv) k_id[popc(lm & lanes_below(lane))] = e;
        if (valid && !lv) s_id[popc(dm & lanes_below(lane))] = e;
    }
    __syncthreads();
    // C(u): each removed neighbour's row in row order; live, not u, not in live(u), first occurrence only
    const int room = CS - nl;
    int nc = 0;
    int32_t *rtmp = reinterpret_cast<int32_t *>(trash);
    for (int a = 0; a < nd && nc < room; ++a) {
        int wr;
        const int32_t *rr = old_row(iv, la.layer, s_id[a], wr);
        const int w = lane < wr ? rr[lane] : -1;
        rtmp[lane] = w;
        __syncthreads();
        bool ok = w >= 0 && w < iv.n && w != u;
        ok = ok && rv.new_id[w] >= 0;
        for (int t = 0; t < lane; ++t) ok = ok && rtmp[t] != w;
        for (int t = 0; t < nl; ++t) ok = ok && k_id[t] != w;
        for (int t = 0; t < nc; ++t) ok = ok && c_id[t] != w;
        const uint64_t m = ballot(ok);
        const int pos = nc + popc(m & lanes_below(lane));
        __syncthreads();
        if (ok && pos < room) c_id[pos] = w;
        nc += popc(m);
        nc = nc < room ? nc : room;
        __syncthreads();
    }
    float4 qv[NCH];
    load_row<NCH>(qv, iv, u, lane & 15);
    __syncthreads();
    for (int base = 0; base < nc; base += 64) {   // eval works on lists of <= 64
        const int m = nc - base < 64 ? nc - base : 64;
        eval_candidates<NCH, RB, METRIC>(iv, qv, c_id + base, c_key + base, trash, m, lane >> 4, lane & 15);
    }
    __syncthreads();
    for (int j = lane; j < nc; j += 64) {         // rank sort by (key, id)
        const uint64_t mk = ((uint64_t)c_key[j] << 32) | (uint32_t)c_id[j];
        int rank = 0;
        for (int t = 0; t < nc; ++t) rank += ((((uint64_t)c_key[t] << 32) | (uint32_t)c_id[t]) < mk);
        s_id[rank] = c_id[j];
        s_key[rank] = c_key[j];
    }
    __syncthreads();
    const int kept = select_heuristic<NCH, METRIC>(iv, s_id, s_key, nc, la.cap, k_id, lane, nl);
    __syncthreads();
    const int ns = kept - nl;
    const int w = lane < ns ? k_id[nl + lane] : -1;
    la.S[(int64_t)i * REMOVE_ROW + lane] = w;
    if (lane < la.cap) la.props[(int64_t)i * la.cap + lane] = w >= 0 ? (((uint64_t)(uint32_t)w << 32) | (uint32_t)u) : ~0ull;
    if (lane == 0) la.nlive[i] = nl;
}

// the order of OFFER: hnsw_distance_batch's value (key_to_dist of the key) as ordered bits -- the square root of L2 can round two
// keys to one distance, which then tie on the id
template <int METRIC> __device__ __forceinline__ uint32_t offer_key(uint32_t key) {
    if (METRIC == 0) return __float_as_uint(key_to_dist<0>(key));
    return key;
}

// ---- OFFER ----------------------------------------------------------------------------------------------------------------
// The best cap - |live(u)| of U(u) under (distance, id), whatever the number of proposers: the list so far and the next 64
// members are merged by a rank sort of at most 128, as build_merge_kernel merges a hub's pending links.
template <int NCH, int RB, int METRIC>
__global__ void __launch_bounds__(64) remove_offer_kernel(const RemoveView rv, const RemoveLayer la, int64_t n_props) {
    __shared__ int32_t u_id[128];
    __shared__ uint32_t u_key[128];
    __shared__ int32_t s_id[128];
    __shared__ uint32_t s_key[128];
    __shared__ int32_t lv_id[64];
    __shared__ int32_t sv_id[64];
    __shared__ uint32_t trash[64];
    const IndexView &iv = rv.iv;
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    if (i >= la.t) return;
    const int u = la.list[i];
    const int nl = la.nlive[i];
    const int R = la.cap - nl;                    // >= 1: a touched row lists a removed node
    {
        int width;
        const int32_t *row = old_row(iv, la.layer, u, width);
        const int e = lane < width ? row[lane] : -1;
        const bool lv = e >= 0 && e < iv.n && rv.new_id[e] >= 0;
        const uint64_t lm = ballot(lv);
        if (lv) lv_id[popc(lm & lanes_below(lane))] = e;
    }
    const int sv = la.S[(int64_t)i * REMOVE_ROW + lane];
    const int ns = popc(ballot(sv >= 0));          // S rows are compact
    sv_id[lane] = sv;
    // the proposers of u: the segment of keys (u << 32 | w) in the sorted proposals
    int64_t lo = 0, hi = n_props;
    const uint64_t first = (uint64_t)(uint32_t)u << 32;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (la.props_sorted[mid] < first) lo = mid + 1; else hi = mid;
    }
    float4 qv[NCH];
    load_row<NCH>(qv, iv, u, lane & 15);
    __syncthreads();
    int nb = 0;                                    // the best so far: u_id / u_key [0, nb), ascending
    bool more = true;
    for (int64_t base = lo - 64; more; base += 64) {
        int m;
        if (base < lo) {                           // first S(u) itself ...
            if (lane < ns) u_id[nb + lane] = sv;
            m = ns;
        } else {                                   // ... then 64 proposals at a time: those not in live(u), not in S(u)
            const int64_t j = base + lane;
            const uint64_t key = j < n_props ? la.props_sorted[j] : ~0ull;
            const bool mine = key != ~0ull && (int)(key >> 32) == u;
            const int w = (int)(key & 0xFFFFFFFFu);
            bool ok = mine;
            for (int t = 0; t < nl; ++t) ok = ok && lv_id[t] != w;
            for (int t = 0; t < ns; ++t) ok = ok && sv_id[t] != w;
            const uint64_t om = ballot(ok);
            if (ok) u_id[nb + popc(om & lanes_below(lane))] = w;
            m = popc(om);
            more = popc(ballot(mine)) == 64;
        }
        __syncthreads();
        if (m > 0) {
            eval_candidates<NCH, RB, METRIC>(iv, qv, u_id + nb, u_key + nb, trash, m, lane >> 4, lane & 15);
            __syncthreads();
            if (lane < m) u_key[nb + lane] = offer_key<METRIC>(u_key[nb + lane]);
            __syncthreads();
            const int nu = nb + m;
            for (int j = lane; j < nu; j += 64) {
                const uint64_t mk = ((uint64_t)u_key[j] << 32) | (uint32_t)u_id[j];
                int rank = 0;
                for (int t = 0; t < nu; ++t) rank += ((((uint64_t)u_key[t] << 32) | (uint32_t)u_id[t]) < mk);
                s_id[rank] = u_id[j];
                s_key[rank] = u_key[j];
            }
            __syncthreads();
            nb = nu < R ? nu : R;
            if (lane < nb) { u_id[lane] = s_id[lane]; u_key[lane] = s_key[lane]; }
            __syncthreads();
        }
    }
    la.T[(int64_t)i * REMOVE_ROW + lane] = lane < nb ? u_id[lane] : -1;
}

// ---- AGREE ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) remove_agree_kernel(const RemoveView rv, const RemoveLayer la) {
    const int lane = threadIdx.x;
    const int i = blockIdx.x;
    if (i >= la.t) return;
    const int u = la.list[i];
    const int nl = la.nlive[i];
    const int w = la.T[(int64_t)i * REMOVE_ROW + lane];
    const int wi = w >= 0 ? la.tidx[w] : -1;       // an untouched w has no T: it takes no new link
    bool ok = false;
    if (wi >= 0) for (int t = 0; t < REMOVE_ROW; ++t) ok = ok || la.T[(int64_t)wi * REMOVE_ROW + t] == u;
    const uint64_t m = ballot(ok);
    if (ok) new_row(rv, la.layer, rv.new_id[u])[nl + popc(m & lanes_below(lane))] = rv.new_id[w];
}

} // namespace hnsw_dev
