// hnsw_upsert_plan.h -- the arithmetic of hnsw_index_upsert_keyed / hnsw_index_update that is plain numbers (host only, no HIP): the
// split of a call's rows into the ones that REPLACE a stored node (P) and the ones that are new, the node counts that follow from it
// (live nodes after the removal, nodes at the end, the first new position), the refusals that need no device (two equal keys in the
// call, naming the smallest; a node named twice or out of range), and the out_replaced / out_new_id fills.
// tests/cpp/test_upsert_plan.cpp checks it against a naive restatement under AddressSanitizer and UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hnsw_host {

struct UpsertPlan {
    int64_t n_old = 0;                 // nodes before the call
    int64_t n_replaced = 0;            // |P|
    int64_t n_live = 0;                // n_old - |P|: the nodes the removal half keeps, = the first new position
    int64_t n_final = 0;               // n_live + m: every row of the call becomes a node, at n_live + i in the call's row order
    std::vector<uint8_t> dead;         // [n_old]: non-zero = the node is in P
    std::vector<int64_t> removed;      // [|P|]: P's nodes, 0-based, in the call's order (what the removal half is handed)
    std::vector<uint8_t> replaced;     // [m]: 1 = row i replaces a stored node
};

enum { UPSERT_OK = 0, UPSERT_OUT_OF_RANGE = 1, UPSERT_TWICE = 2 };

// keys[0..m): is a key there twice?  *dup = the smallest such key (as hnsw_index_set_keys names it)
inline bool upsert_duplicate_key(const int64_t *keys, int64_t m, int64_t *dup) {
    if (m < 2) return false;
    std::vector<int64_t> sorted(keys, keys + m);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t i = 0; i + 1 < m; ++i)
        if (sorted[(size_t)i] == sorted[(size_t)i + 1]) { *dup = sorted[(size_t)i]; return true; }
    return false;
}

// nodes[i]: the 0-based node row i of the call names, -1 = none (a key that is not stored).  absent_ok: the keyed call, where such a
// row is a new node; the call by id refuses it.  UPSERT_OUT_OF_RANGE: nodes[*bad] is no node of [0, n_old) (or -1 where that is
// refused); UPSERT_TWICE: nodes[*bad] was named by an earlier row.  On either, p is not to be used.
inline int upsert_split(const int32_t *nodes, int64_t m, int64_t n_old, bool absent_ok, UpsertPlan &p, int64_t *bad) {
    p = UpsertPlan();
    p.n_old = n_old;
    p.dead.assign((size_t)n_old, 0);
    p.replaced.assign((size_t)m, 0);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t v = nodes[i];
        if (v == -1 && absent_ok) continue;
        if (v < 0 || v >= n_old) { *bad = i; return UPSERT_OUT_OF_RANGE; }
        if (p.dead[(size_t)v]) { *bad = i; return UPSERT_TWICE; }
        p.dead[(size_t)v] = 1;
        p.replaced[(size_t)i] = 1;
        p.removed.push_back(v);
    }
    p.n_replaced = (int64_t)p.removed.size();
    p.n_live = n_old - p.n_replaced;
    p.n_final = p.n_live + m;
    return UPSERT_OK;
}

// out_new_id [n_old], id_base-based as hnsw_index_remove writes it: a kept node's id afterwards (its id minus the replaced nodes below
// it), id_base - 1 for a replaced node.  The m new nodes are not in it: they take n_live + i + id_base.
inline void upsert_fill_new_id(const UpsertPlan &p, int32_t id_base, int32_t *out) {
    int32_t next = 0;
    for (int64_t v = 0; v < p.n_old; ++v) out[v] = p.dead[(size_t)v] ? id_base - 1 : id_base + next++;
}

inline void upsert_fill_replaced(const UpsertPlan &p, uint8_t *out) {
    for (size_t i = 0; i < p.replaced.size(); ++i) out[i] = p.replaced[i];
}

} // namespace hnsw_host
