// hnsw_upsert.hip -- hnsw_index_upsert_keyed / hnsw_index_update: replace or add vectors in one all-or-nothing call (the contract:
// include/hnsw_mi355x.h).  THE DEFINITION is the two-call sequence hnsw_index_remove(P) + hnsw_index_insert(X); this file chains the
// bodies of those two calls in front of ONE adopt_graph:
//   host      the call's rows are split into P (rows that replace a stored node) and new ones (hnsw_upsert_plan.h; the keyed call
//             asks the lookup table once: keys_find_kernel, absent allowed), and everything either call refuses is asked here,
//             before anything is built -- the insert's checks against the node count and top layer the removal WILL leave
//             (remove_plan is plain numbers);
//   device    remove_graph (hnsw_remove.hip) repairs the graph of the kept nodes in tables already sized for the final node count
//             and upper-row count, grow_graph_in_place (hnsw_build.hip) uploads the m vectors behind them and runs the builder's
//             batches from position n_old - |P| on those same tables: old index + new index, two copies at the peak, as either
//             call alone.  (Rows narrower than 2M / M -- a graph flattened from elsewhere -- or an emptied index take the exact-size
//             removal and insert_graph's widening copy instead.)
//   tail      adopt_graph once: row copies and codes over the final table, marks moved under new_id with the m new nodes live, keys
//             moved under new_id with the call's keys behind them (keys_renumber_kernel, one launch, one sort), swap, epoch + 1.
// A degree overflow of the builder (run_batches' removal buffer) discards the attempt's tables and runs the removal again before
// the batches get four times the room: the removal is deterministic and reads only the old handle, and keeping its result aside
// would be a third copy.  No kernel of its own: the launches are the removal's, the builder's and the keys'.
#include "hnsw_internal.h"

using namespace hnsw_host;

namespace {

// one attempt: out = the graph of idx without up's replaced nodes, grown by the m vectors.  idx is only read.
int upsert_attempt(const hnsw_index *idx, const RemovePlan &plan, const float *vectors, int64_t m, int64_t row_stride,
                   const hnsw_build_params *p, int64_t rem_scale, bool *rem_overflow, IndexPtr &out) {
    *rem_overflow = false;
    out.reset();
    const int M = p->num_connections;
    const bool in_place = plan.n > 0 && idx->iv.S0 == 2 * M && idx->iv.SU == M;
    int rc;
    IndexPtr nx;
    if (!in_place) {
        // nothing kept, or rows to be widened: the removal in tables of its own size, then the insert's copy (the header: a third copy)
        if ((rc = remove_graph(idx, plan, plan.n, plan.rowsU, nx))) return rc;
        return insert_graph(nx.get(), vectors, m, row_stride, p, rem_scale, rem_overflow, out);
    }
    const int64_t rowsU = grown_upper_rows(p, plan.n, m, plan.rowsU);
    if (rowsU > 0x7FFFFFF0LL) return fail(HNSW_ERR_UNSUPPORTED, "too many upper rows");
    if ((rc = remove_graph(idx, plan, plan.n + m, rowsU, nx))) return rc;
    if ((rc = grow_graph_in_place(nx.get(), vectors, m, row_stride, p, rem_scale, rem_overflow))) return rc;
    out = std::move(nx);
    return HNSW_OK;
}

void fill_identity(const hnsw_index *idx, int32_t *out_new_id) {
    if (out_new_id) for (int64_t v = 0; v < idx->iv.n; ++v) out_new_id[v] = (int32_t)v + idx->iv.id_base;
}

} // namespace

int hnsw_host::upsert_vectors(hnsw_index *idx, const UpsertPlan &up, const float *vectors, int64_t m, int64_t row_stride,
                              const hnsw_build_params *p, const int64_t *keys) {
    const int64_t n_old = idx->iv.n;
    // what hnsw_index_remove asks ...
    if (idx->live_requests > 0) return fail(HNSW_ERR_BAD_ARG, "%d submitted requests not waited for (hnsw_search_wait first)", idx->live_requests);
    if (idx->multi_replica) return fail(HNSW_ERR_BAD_ARG, "the index is a replica of an hnsw_multi: changing one replica would desynchronise the others");
    if (idx->iv.entry_point < 0) return fail(HNSW_ERR_BAD_ARG, "the index has nodes but no entry point");
    HIP_TRY(hipSetDevice(idx->device));
    { const int32_t rcu = check_upper_rows(idx, "not changed"); if (rcu) return rcu; }
    std::vector<uint8_t> lvl((size_t)n_old);
    HIP_TRY(hipMemcpy(lvl.data(), idx->tables.lvl.p, (size_t)n_old, hipMemcpyDeviceToHost));
    const RemovePlan plan = remove_plan(lvl.data(), up.dead.data(), n_old, idx->iv.entry_point);
    // ... and what hnsw_index_insert asks of the index the removal will leave: plan.n nodes under top layer plan.max_layer
    { const int32_t rcc = check_insert(idx, plan.n, plan.max_layer, vectors, m, row_stride, p); if (rcc) return rcc; }

    // the new graph, in tables of its own: on any error idx is as it was (overflow: the removal again, the batches with 4x the room)
    IndexPtr nx;
    int32_t rc = HNSW_OK;
    for (int64_t scale = 1; scale <= 64; scale *= 4) {
        bool overflow = false;
        rc = upsert_attempt(idx, plan, vectors, m, row_stride, p, scale, &overflow, nx);
        if (!overflow) break;
    }
    if (rc) {
        nx.reset();
        (void)hipGetLastError();
        return rc;
    }
    // the locality codes are dropped and built on demand, as hnsw_index_remove leaves them for the insert that follows it
    return adopt_graph(idx, nx, /*carry_codes=*/false, p->expected_ef, p->expected_semantics, plan.new_id.data(), keys);
}

extern "C" {

int32_t hnsw_index_upsert_keyed(hnsw_index *idx, const float *vectors, const int64_t *keys, int64_t m, int64_t row_stride,
                                const hnsw_build_params *params, uint8_t *out_replaced, int32_t *out_new_id) {
    if (!idx || !params) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (!idx->keys && idx->iv.n > 0)
        return fail(HNSW_ERR_BAD_ARG, "hnsw_index_upsert_keyed: the index has %lld nodes and no keys (hnsw_index_set_keys first)", (long long)idx->iv.n);
    if (m == 0) { fill_identity(idx, out_new_id); return HNSW_OK; }
    if (!keys) return fail(HNSW_ERR_BAD_ARG, "null keys");
    if (!vectors) return fail(HNSW_ERR_BAD_ARG, "null vectors");
    int64_t dup = 0;
    if (upsert_duplicate_key(keys, m, &dup))
        return fail(HNSW_ERR_BAD_ARG, "hnsw_index_upsert_keyed: key %lld appears twice in the call (the smallest duplicated key): nothing changed", (long long)dup);
    // the partition into stored and absent keys: one lookup launch
    std::vector<int32_t> nodes((size_t)m, -1);
    int rc;
    if (idx->keys && (rc = keys_find_nodes(idx, keys, m, nodes))) return rc;
    UpsertPlan up;
    int64_t bad = 0;
    if (upsert_split(nodes.data(), m, idx->iv.n, /*absent_ok=*/true, up, &bad) != UPSERT_OK)
        return fail(HNSW_ERR_HIP, "hnsw_index_upsert_keyed: the key lookup named node %d for keys[%lld]: the key tables are damaged", nodes[(size_t)bad], (long long)bad);
    // no stored key: the call IS hnsw_index_insert_keyed (codes carried over, as there)
    rc = up.n_replaced == 0 ? insert_vectors(idx, vectors, m, row_stride, params, keys) : upsert_vectors(idx, up, vectors, m, row_stride, params, keys);
    if (rc) return rc;
    if (out_replaced) upsert_fill_replaced(up, out_replaced);
    if (out_new_id) upsert_fill_new_id(up, idx->iv.id_base, out_new_id);
    return HNSW_OK;
}

int32_t hnsw_index_update(hnsw_index *idx, const int64_t *ids, const float *vectors, int64_t m, int64_t row_stride,
                          const hnsw_build_params *params, int32_t *out_new_id) {
    if (!idx || !params) return fail(HNSW_ERR_BAD_ARG, "null argument");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    if (idx->keys)
        return fail(HNSW_ERR_BAD_ARG, "the index has keys and must never hold a node without one: hnsw_index_upsert_keyed (the keyed call) updates it");
    if (m == 0) { fill_identity(idx, out_new_id); return HNSW_OK; }
    if (!ids) return fail(HNSW_ERR_BAD_ARG, "null ids");
    if (!vectors) return fail(HNSW_ERR_BAD_ARG, "null vectors");
    const int64_t n_old = idx->iv.n;
    const int32_t base = idx->iv.id_base;
    std::vector<int32_t> nodes((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t v = ids[i] - base;
        if (v < 0 || v >= n_old) return fail(HNSW_ERR_BAD_ARG, "ids[%lld]=%lld is not a stored node", (long long)i, (long long)ids[i]);
        nodes[(size_t)i] = (int32_t)v;
    }
    UpsertPlan up;
    int64_t bad = 0;
    if (upsert_split(nodes.data(), m, n_old, /*absent_ok=*/false, up, &bad) != UPSERT_OK)
        return fail(HNSW_ERR_BAD_ARG, "ids[%lld]=%lld appears twice", (long long)bad, (long long)ids[bad]);
    const int rc = upsert_vectors(idx, up, vectors, m, row_stride, params, nullptr);
    if (rc) return rc;
    if (out_new_id) upsert_fill_new_id(up, base, out_new_id);
    return HNSW_OK;
}

} // extern "C"
