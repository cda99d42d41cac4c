// hnsw_remove.hip -- hnsw_index_remove: hard deletion with a graph repair on the device (the contract: include/hnsw_mi355x.h).
//
// The host checks the arguments and the graph, plans the numbers (hnsw_remove_plan.h: new ids, the live nodes' upper layout, the
// new top and entry), builds the new graph tables BESIDE the old ones with the kernels of hnsw_remove_device.hip.h -- which read
// the old tables only -- and hands them to adopt_graph, the tail it shares with hnsw_index_insert (row copies, swap, epoch).
#include "hnsw_remove_device.hip.h"
#include "hnsw_internal.h"

#include <hipcub/hipcub.hpp>

using namespace hnsw_host;
using hnsw_dev::RemoveLayer;
using hnsw_dev::RemoveView;
using hnsw_dev::REMOVE_ROW;

// One attempt: `out` = a new handle with the repaired graph of idx's live nodes (plan: remove_plan of idx's levels).  idx is only
// read.  The derived tables are the caller's (adopt_graph).  n_tables / rowsU_tables: the nodes and upper rows the new tables are
// sized for -- plan.n / plan.rowsU for hnsw_index_remove; more for the removal half of an upsert, whose insert half grows the graph
// on these same tables (grow_graph_in_place: the rows behind the live part stay empty here).
int hnsw_host::remove_graph(const hnsw_index *idx, const RemovePlan &plan, int64_t n_tables, int64_t rowsU_tables, IndexPtr &out) {
    out.reset();
    if (n_tables < plan.n || rowsU_tables < plan.rowsU) return fail(HNSW_ERR_BAD_ARG, "remove: tables smaller than the live graph");
    const hnsw_dev::IndexView &ov = idx->iv;
    const int64_t n_old = ov.n, n = plan.n;
    const int S0 = ov.S0, SU = ov.SU;
    const int metric = idx->info.metric, nch = pick_nch(ov.nchunks);
    IndexPtr nx(new hnsw_index());
    nx->device = idx->device;
    IndexTables &t = nx->tables;
    int rc;
    if ((rc = alloc_graph_tables(t, n_tables, ov.stride, S0, SU, rowsU_tables))) return rc;
    if (n > 0) {
        std::vector<int2> ref((size_t)n);
        for (int64_t j = 0; j < n; ++j) ref[(size_t)j] = make_int2(plan.upper_row[(size_t)j], (int)plan.level[(size_t)j]);
        if ((rc = upload_upper_layout(t, 0, ref))) return rc;
    }
    hnsw_dev::IndexView &iv = nx->iv;
    iv = ov;                                                            // d, stride, nchunks, id_base, S0, SU
    iv.n = n; iv.rowsU = plan.rowsU; iv.max_layer = plan.max_layer; iv.entry_point = plan.entry;
    nx->info = idx->info;                                               // d, metric, id_base, device, max_degree
    if (n > 0) {
        Stream st;
        HIP_TRY(hipStreamCreate(&st.h));
        const int layers = ov.max_layer + 1;
        Table dNew, dTouched, dList, dCount, dTidx, dNlive, dS, dT, dProps, dSorted, dTemp;
        HIP_TRY(dNew.alloc((size_t)n_old * 4));
        HIP_TRY(dTouched.alloc((size_t)layers * n_old));
        HIP_TRY(dList.alloc((size_t)n_old * 4));
        HIP_TRY(dCount.alloc(16));
        HIP_TRY(dTidx.alloc((size_t)n_old * 4));
        HIP_TRY(hipMemcpyAsync(dNew.p, plan.new_id.data(), (size_t)n_old * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(dTouched.p, 0, (size_t)layers * n_old, st));
        RemoveView rv{};
        rv.iv = ov; rv.new_id = (const int32_t *)dNew.p;
        rv.nbr0_new = (int32_t *)t.nbr0.p; rv.nbrU_new = (int32_t *)t.nbrU.p; rv.ref_new = (const int2 *)t.ref.p;
        hipLaunchKernelGGL(hnsw_dev::remove_copy_kernel, dim3((unsigned)((n_old + 3) / 4)), dim3(256), 0, st, rv, (uint8_t *)dTouched.p, layers);
        if ((rc = launched("remove copy kernel"))) return rc;
        const int64_t stride4 = ov.stride / 4, total4 = n_old * stride4;
        hipLaunchKernelGGL(hnsw_dev::remove_gather_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, (const float4 *)ov.X, n_old,
                           (int32_t)stride4, (const int32_t *)dNew.p, (float4 *)t.X.p);
        if ((rc = launched("remove gather kernel"))) return rc;

        size_t select_bytes = 0;
        hipcub::CountingInputIterator<int32_t> every(0);
        HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, select_bytes, every, (const uint8_t *)dTouched.p, (int32_t *)dList.p, (int32_t *)dCount.p,
                                              (int)n_old, st));
        HIP_TRY(dTemp.alloc(select_bytes));
        for (int l = 0; l <= plan.max_layer; ++l) {
            // the touched nodes of the layer, ascending
            size_t tb = dTemp.bytes;
            HIP_TRY(hipcub::DeviceSelect::Flagged(dTemp.p, tb, every, (const uint8_t *)dTouched.p + (size_t)l * n_old, (int32_t *)dList.p,
                                                  (int32_t *)dCount.p, (int)n_old, st));
            int32_t cnt = 0;
            HIP_TRY(hipMemcpyAsync(&cnt, dCount.p, 4, hipMemcpyDeviceToHost, st));
            if ((rc = synced(st, "remove: touched list"))) return rc;
            if (cnt == 0) continue;
            const int cap = l == 0 ? S0 : SU;
            const int64_t n_props = (int64_t)cnt * cap;
            if (n_props > 0x7FFFFFF0LL) return fail(HNSW_ERR_UNSUPPORTED, "%d touched nodes on layer %d: too many proposals for one sort", cnt, l);
            Table dSortTemp;
            size_t sort_bytes = 0;
            if (dNlive.bytes < (size_t)cnt * 4) {
                HIP_TRY(dNlive.alloc((size_t)cnt * 4));
                HIP_TRY(dS.alloc((size_t)cnt * REMOVE_ROW * 4));
                HIP_TRY(dT.alloc((size_t)cnt * REMOVE_ROW * 4));
            }
            if (dProps.bytes < (size_t)n_props * 8) {
                HIP_TRY(dProps.alloc((size_t)n_props * 8));
                HIP_TRY(dSorted.alloc((size_t)n_props * 8));
            }
            HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (uint64_t *)dProps.p, (uint64_t *)dSorted.p, (int)n_props, 0, 64, st));
            HIP_TRY(dSortTemp.alloc(sort_bytes));
            HIP_TRY(hipMemsetAsync(dTidx.p, 0xFF, (size_t)n_old * 4, st));
            hipLaunchKernelGGL(hnsw_dev::remove_index_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (const int32_t *)dList.p, cnt,
                               (int32_t *)dTidx.p);
            if ((rc = launched("remove index kernel"))) return rc;
            RemoveLayer la{};
            la.list = (const int32_t *)dList.p; la.t = cnt; la.layer = l; la.cap = cap; la.tidx = (const int32_t *)dTidx.p;
            la.nlive = (int32_t *)dNlive.p; la.S = (int32_t *)dS.p; la.props = (uint64_t *)dProps.p; la.props_sorted = (const uint64_t *)dSorted.p;
            la.T = (int32_t *)dT.p;
            const size_t lds = ((size_t)4 * hnsw_dev::REMOVE_CAND + 128) * 4;
            with_metric(metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
                hipLaunchKernelGGL((hnsw_dev::remove_propose_kernel<NCH, rows_in_flight(NCH), METRIC>), dim3((unsigned)cnt), dim3(64), lds, st, rv, la);
            }); });
            if ((rc = launched("remove propose kernel"))) return rc;
            HIP_TRY(hipcub::DeviceRadixSort::SortKeys(dSortTemp.p, sort_bytes, (uint64_t *)dProps.p, (uint64_t *)dSorted.p, (int)n_props, 0, 64, st));
            with_metric(metric, [&](auto METRIC) { with_nch(nch, [&](auto NCH) {
                hipLaunchKernelGGL((hnsw_dev::remove_offer_kernel<NCH, rows_in_flight(NCH), METRIC>), dim3((unsigned)cnt), dim3(64), 0, st, rv, la, n_props);
            }); });
            if ((rc = launched("remove offer kernel"))) return rc;
            hipLaunchKernelGGL(hnsw_dev::remove_agree_kernel, dim3((unsigned)cnt), dim3(64), 0, st, rv, la);
            if ((rc = launched("remove agree kernel"))) return rc;
            if ((rc = synced(st, "remove: repair"))) return rc;      // (the sort's temporary storage is freed at the end of the round)
        }
        if ((rc = synced(st, "remove"))) return rc;
    }
    bind_view(nx.get());
    out = std::move(nx);
    return HNSW_OK;
}

extern "C" int32_t hnsw_index_remove(hnsw_index *idx, const int64_t *ids, int64_t m, int32_t *out_new_id) {
    if (!idx) return fail(HNSW_ERR_BAD_ARG, "null index");
    if (m < 0) return fail(HNSW_ERR_BAD_ARG, "m=%lld < 0", (long long)m);
    const int64_t n_old = idx->iv.n;
    const int32_t base = idx->iv.id_base;
    if (m == 0) {
        if (out_new_id) for (int64_t v = 0; v < n_old; ++v) out_new_id[v] = (int32_t)v + base;
        return HNSW_OK;
    }
    if (!ids) return fail(HNSW_ERR_BAD_ARG, "null ids");
    std::vector<uint8_t> dead((size_t)n_old, 0);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t v = ids[i] - base;
        if (v < 0 || v >= n_old) return fail(HNSW_ERR_BAD_ARG, "ids[%lld]=%lld is not a stored node", (long long)i, (long long)ids[i]);
        if (dead[(size_t)v]) return fail(HNSW_ERR_BAD_ARG, "ids[%lld]=%lld appears twice", (long long)i, (long long)ids[i]);
        dead[(size_t)v] = 1;
    }
    if (idx->live_requests > 0) return fail(HNSW_ERR_BAD_ARG, "%d submitted requests not waited for (hnsw_search_wait first)", idx->live_requests);
    if (idx->multi_replica) return fail(HNSW_ERR_BAD_ARG, "the index is a replica of an hnsw_multi: removing from one replica would desynchronise the others");
    if (idx->iv.entry_point < 0) return fail(HNSW_ERR_BAD_ARG, "the index has nodes but no entry point");
    HIP_TRY(hipSetDevice(idx->device));
    { const int32_t rcu = check_upper_rows(idx, "not shrunk"); if (rcu) return rcu; }

    std::vector<uint8_t> lvl((size_t)n_old);
    HIP_TRY(hipMemcpy(lvl.data(), idx->tables.lvl.p, (size_t)n_old, hipMemcpyDeviceToHost));
    const RemovePlan plan = remove_plan(lvl.data(), dead.data(), n_old, idx->iv.entry_point);

    // the shrunk graph, in tables of its own: on any error idx is as it was
    IndexPtr nx;
    int32_t rc = remove_graph(idx, plan, plan.n, plan.rowsU, nx);
    if (rc) {
        nx.reset();
        (void)hipGetLastError();
        return rc;
    }
    // byte rows (they may appear now), split, half and sq8 rows (either kind) follow as after an insert; the locality codes are dropped and
    // built again on demand
    if ((rc = adopt_graph(idx, nx, /*carry_codes=*/false, 0, 0, plan.new_id.data()))) return rc;
    if (out_new_id) for (int64_t v = 0; v < n_old; ++v) out_new_id[v] = plan.new_id[(size_t)v] + base;      // removed: id_base - 1
    return HNSW_OK;
}
