"""One live handle driven through a SEQUENCE of different mutation calls with options switched in between, and held after EVERY
step to two yardsticks:

  1. tests/mutation_model.py (pinned by tests/test_mutation_model.py): what the handle holds -- n, the float32 rows' bits, keys,
     marks, the ids each call returns -- and the float64 reference of the exact scan and the exact range scan over the live rows;
  2. a fresh TWIN: a new handle made by hnsw_index_create from the handle's own export and the model's rows, given the same
     options, keys and marks.  It has the same graph and rows with every piece of derived state made from scratch (row copies and
     their parameters, locality codes, key table, live mask, prepared shapes, the scans' prepass state), so whatever the mutated
     handle answers the twin must answer with the same bits: ids, distance bits, hop counts, ladder stages, range lims.
     Evaluation counts are not compared: the lossy visited cache may differ.

Every comparison is equality.  The data lie on a grid whose sums are exact in fp32 (integers in -8..8 over 8; the byte world:
integers 0..15), so the float64 reference is comparable bit for bit; exact duplicates and a query that is a stored row are planted.
The COSINE world leaves the float64 reference out (not bit-comparable after a division): hg.rows() == H.normalise(model rows), and
the twin in full.

Filters and labels: hnsw_mi355x.h, soft deletion, EPOCH: "A successful call that changes at least one bit moves the handle's graph
epoch on: filters made before it are refused"; hnsw_index_set_keys "does not move the graph epoch: filters and labels stay valid".
So a filter and a labels object made before a step are refused after it exactly when the step moved a row or a mark (a step that
only marks included), and accepted after every other step: options, keys, a refused call, compact with nothing marked.

Which script holds which call and option (every world runs every script; a step adapts to the keys: "insert" is insert_batch on a
handle without keys and insert_batch_keyed on one with, "upsert" / "update" likewise; CALLS lists what each script must have made):

  A  scan_bytes 1, scan_matrix 1, scan_slabs 3; insert_batch of 1 row and of 70 rows (the byte world: rows with a value of 0.5, so
     byte rows -> float32 rows and scan_path 2 -> 3); remove_batch of one id; mark_deleted; unmark_deleted of part; a refused
     remove_batch (id out of range); update_batch; remove_batch of exactly the 70 rows (-> byte rows, scan_path 2); compact with
     marks; compact with none; remove_batch of the entry point
  B  set_keys; byte_rows 0, half_rows 1, refine -1, order_queries 1, scan_matrix 1; insert_batch_keyed; a refused insert of
     70000.0 under half_rows (COSINE normalises it into range: a duplicate key there); upsert_batch_keyed with half the keys stored,
     with a stored key whose node is marked, with none stored; mark_deleted_keys; unmark_deleted_keys of part; half_rows 0,
     byte_rows 1, filter_collect 1, scan_matrix 0, scan_bytes 1; remove_keys of a random 20 %; compact
  C  byte_rows 0, sq8_rows 1, refine -1, visited_blocks 1 (every check searches at ef 200, so the per-slot codes exist before the
     next mutation); insert; a refused NaN row under sq8_rows; remove_batch of a block that holds the whole top layer; sq8_rows 0,
     sq8_dim_rows 1, split_rows 0; set_keys; a refused duplicate key; sq8_dim_rows 0, bit_rows 1, bit_query_bits 4, split_rows 1;
     clear_keys; update_batch; set_keys again; upsert_batch_keyed with all keys stored
  S1, S2  ten steps drawn with default_rng(seed) from MENU (inserts of 1 and 70, removals of one / the entry point / 20 %, marks,
     unmarks, compact, upsert or update, set_keys, clear_keys, the scan options, one lossy row option at a time)"""
import os
import tempfile
from collections import OrderedDict

import numpy as np
import pytest
from mutation_model import Model
from test_gpu_remove import _graph_invariants, _same_export

pytestmark = pytest.mark.gpu

M, EFC, SEED = 8, 40, 3
N0, NQ, N_MAX = 600, 33, 900        # 33 queries: one full scan tile plus one
ROWS_F32, ROWS_BYTES, ROWS_SPLIT = 0, 2, 3
FLOAT, BYTES, MATRIX = 1, 2, 3      # scan_path()
COSINE = 2
LOSSY = ("half_rows", "sq8_rows", "sq8_dim_rows", "bit_rows", "filter_collect")
eq = np.testing.assert_array_equal

# name -> (d, metric, the value that tags the 70 rows of "insert_tagged" in column 0: off the world's grid, exact in fp32)
WORLDS = {"f32": (24, 0, 1.5), "ip": (100, 1, 1.5), "bytes": (70, 0, 0.5), "cosine": (24, COSINE, 1.5)}

A = [("opts", [("scan_bytes", 1), ("scan_matrix", 1), ("scan_slabs", 3)]),
     ("insert", 1, 101),
     ("insert_tagged", 70, 102),
     ("remove", "one"),
     ("mark", 40, 5),
     ("unmark_part",),
     ("refused", "bad_id"),
     ("update", 30, 103),
     ("remove", "tagged"),
     ("compact",),
     ("compact",),
     ("remove", "entry")]
B = [("set_keys", 1),
     ("opts", [("byte_rows", 0), ("half_rows", 1), ("refine", -1), ("order_queries", 1), ("scan_matrix", 1)]),
     ("insert", 70, 201),
     ("refused", "big_half"),
     ("upsert", "half", 40, 202),
     ("mark_keys", 30, 6),
     ("upsert", "marked", 10, 203),
     ("unmark_keys_part",),
     ("opts", [("half_rows", 0), ("byte_rows", 1), ("filter_collect", 1), ("scan_matrix", 0), ("scan_bytes", 1)]),
     ("remove_keys", "random20"),
     ("upsert", "none", 20, 204),
     ("compact",)]
C = [("opts", [("byte_rows", 0), ("sq8_rows", 1), ("refine", -1), ("visited_blocks", 1)]),
     ("insert", 70, 301),
     ("refused", "nan_sq8"),
     ("remove", "top_block"),
     ("opts", [("sq8_rows", 0), ("sq8_dim_rows", 1), ("split_rows", 0)]),
     ("set_keys", 2),
     ("refused", "dup_key"),
     ("opts", [("sq8_dim_rows", 0), ("bit_rows", 1), ("bit_query_bits", 4), ("split_rows", 1)]),
     ("clear_keys",),
     ("update", 20, 302),
     ("set_keys", 3),
     ("upsert", "all", 30, 303)]
MENU = [("insert", 1, 401), ("insert", 70, 402), ("insert", 70, 403), ("remove", "one"), ("remove", "entry"), ("remove", "random20"),
        ("remove_keys", "random20"), ("mark", 40, 8), ("mark_keys", 25, 9), ("unmark_part",), ("unmark_keys_part",), ("compact",),
        ("upsert", "half", 30, 404), ("upsert", "marked", 10, 405), ("update", 20, 406), ("set_keys", 4), ("clear_keys",),
        ("opts", [("scan_matrix", 1), ("scan_bytes", 1)]), ("opts", [("scan_matrix", 0), ("scan_bytes", 0), ("scan_slabs", 3)]),
        ("lossy", "half_rows"), ("lossy", "sq8_rows"), ("lossy", "sq8_dim_rows"), ("lossy", "bit_rows"), ("lossy", "filter_collect"),
        ("lossy", None)]


def _drawn(seed):
    return [MENU[i] for i in np.random.default_rng(seed).integers(0, len(MENU), size=10)]


SCRIPTS = {"A": A, "B": B, "C": C, "S1": _drawn(1), "S2": _drawn(2)}
# what a fixed script must have called, whatever else it did (the table of the docstring, held)
CALLS = {"A": {"insert_batch", "remove_batch", "mark_deleted", "unmark_deleted", "update_batch", "compact", "refused bad_id"},
         "B": {"set_keys", "insert_batch_keyed", "upsert_batch_keyed", "mark_deleted_keys", "unmark_deleted_keys", "remove_keys", "compact"},
         "C": {"insert_batch", "remove_batch", "set_keys", "clear_keys", "update_batch", "upsert_batch_keyed", "refused nan_sq8",
               "refused dup_key"},
         "S1": set(), "S2": set()}
SUBST = {("cosine", "big_half"): "dup_key"}     # COSINE stores 70000.0 normalised, in fp16 range: nothing to refuse


@pytest.fixture(scope="module")
def H():
    import ocaml_hnsw_amd as H
    H.load()
    assert H.device_count() >= 1, "GPU tests need a HIP device"
    return H


def _gen(world, m, seed):
    d = WORLDS[world][0]
    rng = np.random.default_rng(seed)
    if world == "bytes":
        return rng.integers(0, 16, size=(m, d)).astype(np.float32)
    return (rng.integers(-8, 9, size=(m, d)) / 8.0).astype(np.float32)


_data = {}


def _world(world):
    """(X [600][d], Q [33][d]): three exact duplicates of row 12, one of them also a query"""
    if world not in _data:
        X, Q = _gen(world, N0, 7), _gen(world, NQ, 8)
        X[[77, 300, 599]] = X[12]
        Q[7] = X[12]
        X.setflags(write=False)
        Q.setflags(write=False)
        _data[world] = (X, Q)
    return _data[world]


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a.view(np.uint64) if a.dtype.names else a


def _byte_valued(a):
    return bool(((a == np.rint(a)) & (a >= 0) & (a <= 255)).all())


class Run:
    """one script on one world: the handle, the model, and what the script set"""

    def __init__(self, H, world, name):
        self.H, self.world, self.name = H, world, name
        self.d, self.metric, self.marker = WORLDS[world]
        X, self.Q = _world(world)
        self.hg = H.Ohnsw.build_batch_bigarray(X, M, EFC, seed=SEED, metric=self.metric)
        self.model = Model(X, metric=min(self.metric, 1))
        self.opts = OrderedDict()       # the options in the order they were last set: what a twin is given
        self.next_key = 10 ** 6
        self.called = set()
        self.stage0 = self.later = False
        self.trace = []                 # (row_format, scan_path) after every step
        self.ctx = "%s / %s, before any step" % (world, name)

    # ---- helpers ----
    def set_opt(self, name, value, hg=None):
        (hg or self.hg).set_option(name, value)
        if hg is None:
            self.opts.pop(name, None)
            self.opts[name] = value

    def dress(self, hg):
        """give another handle over the same rows the options, keys and marks of the model"""
        for name, value in self.opts.items():
            hg.set_option(name, value)
        if self.model.keys is not None:
            hg.set_keys(self.model.keys)
        if self.model.marked.any():
            hg.mark_deleted(np.flatnonzero(self.model.marked))
        return hg

    def select(self, kind):
        n, hg = self.model.n, self.hg
        if kind == "one":
            return np.array([n // 2])
        if kind == "entry":
            return np.array([hg.entry_point])
        if kind == "random20":
            return np.random.default_rng(5).choice(n, size=n // 5, replace=False)
        if kind == "tagged":
            return np.flatnonzero(self.model.rows[:, 0] == np.float32(self.marker))
        if kind == "top_block":         # the whole top layer in one block of ids; blocks of 17 around each node where they lie far apart
            top = hg.upper[-1][0]
            if top.max() - top.min() < n // 4:
                return np.arange(top.min(), top.max() + 1)
            return np.unique(np.clip(np.add.outer(top, np.arange(-8, 9)), 0, n - 1))
        raise ValueError(kind)

    def fresh_keys(self, m):
        self.next_key += m
        return np.arange(self.next_key - m, self.next_key, dtype=np.int64)

    def insert(self, X):
        H, hg, model = self.H, self.hg, self.model
        if model.keys is None:
            self.called.add("insert_batch")
            eq(H.Ohnsw.insert_batch(hg, X, M, EFC, seed=SEED), model.insert(X), err_msg=self.ctx)
        else:
            kk = self.fresh_keys(len(X))
            self.called.add("insert_batch_keyed")
            eq(H.Ohnsw.insert_batch_keyed(hg, X, kk, M, EFC, seed=SEED), model.insert_keyed(X, kk), err_msg=self.ctx)

    def refused(self, what):
        H, hg, model = self.H, self.hg, self.model
        what = SUBST.get((self.world, what), what)
        if what == "dup_key" and model.keys is None:
            what = "bad_id"
        X = _gen(self.world, 2, 77)
        self.called.add("refused " + what)
        if what == "bad_id":
            with pytest.raises(H.InvalidArgument):
                H.Ohnsw.remove_batch(hg, [0, model.n])
            return
        if what == "dup_key":
            with pytest.raises(H.InvalidArgument):
                H.Ohnsw.insert_batch_keyed(hg, X, [self.next_key, self.next_key], M, EFC, seed=SEED)
            return
        assert self.opts.get({"nan_sq8": "sq8_rows", "big_half": "half_rows"}[what]) == 1, self.ctx
        X[1, 3] = np.nan if what == "nan_sq8" else 70000.0
        with pytest.raises((H.InvalidArgument, H.Failure)):
            if model.keys is None:
                H.Ohnsw.insert_batch(hg, X, M, EFC, seed=SEED)
            else:
                H.Ohnsw.insert_batch_keyed(hg, X, [self.next_key, self.next_key + 1], M, EFC, seed=SEED)

    def upsert(self, kind, m, seed):
        H, hg, model = self.H, self.hg, self.model
        rng = np.random.default_rng(seed)
        if model.keys is None:          # update_batch is the same call by id
            ids = rng.choice(model.n, size=m, replace=False)
            X = _gen(self.world, m, seed)
            self.called.add("update_batch")
            eq(H.Ohnsw.update_batch(hg, ids, X, M, EFC, seed=SEED), model.update(ids, X), err_msg=self.ctx)
            return
        stored = model.keys
        if kind == "half":
            kk = np.concatenate([rng.choice(stored, size=m // 2, replace=False), self.fresh_keys(m - m // 2)])
        elif kind == "none":
            kk = self.fresh_keys(m)
        elif kind == "all":
            kk = rng.choice(stored, size=m, replace=False)
        else:                           # stored keys of marked nodes, stored keys of live ones, one new key
            marked, live = stored[model.marked], stored[~model.marked]
            kk = np.concatenate([marked[:m], live[:m], self.fresh_keys(1)])
        kk = rng.permutation(kk)
        X = _gen(self.world, len(kk), seed)
        self.called.add("upsert_batch_keyed")
        replaced, new_id = H.Ohnsw.upsert_batch_keyed(hg, X, kk, M, EFC, seed=SEED)
        want_replaced, want_new_id = model.upsert_keyed(X, kk)
        eq(replaced, want_replaced, err_msg=self.ctx)
        eq(new_id, want_new_id, err_msg=self.ctx)

    # ---- one step: the call on the handle and on the model, what it returns compared ----
    def apply(self, step):
        H, hg, model = self.H, self.hg, self.model
        op, keyed = step[0], model.keys is not None
        if op == "opts":
            for name, value in step[1]:
                self.set_opt(name, value)
        elif op == "lossy":             # one lossy row option at a time: the others off first, the byte rows out of the way
            for name in LOSSY:
                if self.opts.get(name, 0):
                    self.set_opt(name, 0)
            if step[1] is None:
                self.set_opt("byte_rows", 1)
            else:
                self.set_opt("byte_rows", 0)
                self.set_opt("refine", -1)
                self.set_opt(step[1], 1)
        elif op == "insert":
            self.insert(_gen(self.world, step[1], step[2]))
        elif op == "insert_tagged":
            X = _gen(self.world, step[1], step[2])
            X[:, 0] = self.marker
            self.insert(X)
        elif op in ("remove", "remove_keys"):
            ids = self.select(step[1])
            if op == "remove_keys" and keyed:
                kk = model.keys[ids]
                self.called.add("remove_keys")
                eq(hg.remove_keys(kk), model.remove_keys(kk), err_msg=self.ctx)
            else:
                self.called.add("remove_batch")
                eq(H.Ohnsw.remove_batch(hg, ids), model.remove(ids), err_msg=self.ctx)
        elif op in ("mark", "mark_keys"):
            ids = np.random.default_rng(step[2]).choice(model.n, size=step[1], replace=False)
            if op == "mark_keys" and keyed:
                self.called.add("mark_deleted_keys")
                hg.mark_deleted_keys(model.keys[ids])
                model.mark_keys(model.keys[ids])
            else:
                self.called.add("mark_deleted")
                hg.mark_deleted(ids)
                model.mark(ids)
        elif op in ("unmark_part", "unmark_keys_part"):
            ids = np.flatnonzero(model.marked)[::2]
            if op == "unmark_keys_part" and keyed:
                self.called.add("unmark_deleted_keys")
                hg.unmark_deleted_keys(model.keys[ids])
                model.unmark_keys(model.keys[ids])
            else:
                self.called.add("unmark_deleted")
                hg.unmark_deleted(ids)
                model.unmark(ids)
        elif op == "compact":
            self.called.add("compact")
            eq(hg.compact(), model.compact(), err_msg=self.ctx)
        elif op == "upsert":
            self.upsert(step[1], step[2], step[3])
        elif op == "update":
            self.upsert("half", step[1], step[2])
        elif op == "set_keys":
            kk = np.random.default_rng(step[1]).permutation(model.n).astype(np.int64) * 3 - 1000
            self.called.add("set_keys")
            hg.set_keys(kk)
            model.set_keys(kk)
        elif op == "clear_keys":
            self.called.add("clear_keys")
            hg.clear_keys()
            model.clear_keys()
        elif op == "refused":
            self.refused(step[1])
        else:
            raise ValueError(op)

    # ---- the checks after every step, written once ----
    def answers(self, hg, mask, radius, by_id):
        """every search form that goes through derived state -> name: the arrays to compare (no evaluation counts)"""
        O, Q = self.H.Ohnsw, self.Q
        out = OrderedDict()

        def keep(name, res, which):
            out[name] = [_bits(res[i]) for i in which]

        keep("knn ef 16", O.knn_batch_bigarray(hg, 10, Q, ef=16, counters=True), (0, 1, 3))
        keep("knn ef 200", O.knn_batch_bigarray(hg, 10, Q, ef=200, counters=True), (0, 1, 3))
        out["Ba.knn_batch"] = [_bits(self.H.Ba.knn_batch(hg, Q, 16, 10))]
        keep("filtered", O.knn_batch_filtered(hg, 10, Q, mask, ef=16, counters=True), (0, 1, 3, 4))
        keep("range", O.range_search(hg, radius, Q, ef=16, counters=True), (0, 1, 2, 4, 5))
        labels = hg.labels(np.arange(self.model.n) % 7)
        keep("grouped", O.knn_batch_grouped(hg, 5, Q, labels, ef=16, counters=True), (0, 1, 2, 4, 5))
        labels.release()
        page = O.knn_batch_after(hg, 10, Q, None, ef=16, counters=True)
        keep("after, page 1", page, (0, 1, 2, 4, 5))
        keep("after, page 2", O.knn_batch_after(hg, 10, Q, page[2], ef=16, counters=True), (0, 1, 2, 4, 5))
        keep("diverse", O.knn_batch_diverse(hg, 10, Q, 32, 0.5, counters=True), (0, 1, 2, 4, 5))
        keep("brute_force_diverse", O.brute_force_diverse(hg, 10, Q, 32, 0.5), (0, 1, 2))
        keep("by id", O.knn_batch_by_id(hg, 10, by_id, ef=16, exclude_self=True, counters=True), (0, 1, 3))
        keep("brute_force_by_id", O.brute_force_by_id(hg, 10, by_id, exclude_self=True), (0, 1))
        if self.model.keys is not None:
            keep("keyed", O.knn_batch_keyed(hg, 10, Q, ef=16, counters=True), (0, 1, 3, 4))
        return out

    def expected_path(self):
        rows = self.model.rows
        if self.opts.get("scan_bytes", 0) and self.metric != COSINE and self.d <= 256 and _byte_valued(rows) and _byte_valued(self.Q):
            return BYTES
        return MATRIX if self.opts.get("scan_matrix", 0) else FLOAT

    def check(self):
        H, hg, model, Q, c = self.H, self.hg, self.model, self.Q, self.ctx
        O = H.Ohnsw
        # -- against the model: what the handle holds
        assert hg.n == model.n == hg.info().n and model.n <= N_MAX, c
        want_rows = H.normalise(model.rows) if self.metric == COSINE else model.rows
        eq(_bits(hg.rows()), _bits(want_rows), err_msg=c + ": rows")
        absent = np.array([5 * 10 ** 8, -5 * 10 ** 8, 2 ** 62], np.int64)
        if model.keys is None:
            assert hg.keys_info()[0] is False, c
        else:
            eq(hg.keys(), model.keys, err_msg=c + ": keys")
            probe = np.concatenate([model.keys, absent])
            eq(hg.find_keys(probe), model.find_keys(probe), err_msg=c + ": find_keys")
        eq(hg.deleted_mask(), model.marked, err_msg=c + ": marks")
        assert hg.deleted_count() == int(model.marked.sum()), c
        # -- the graph and its statistics
        hg.export()
        _graph_invariants(hg, M)
        st = hg.stats()
        assert st["num_nodes"] == model.n and st["layer_sizes"][0] == model.n, c
        for l, (nodes, deg, nbr) in enumerate(hg.upper):
            cl = st["layer_connectivity"][l + 1]
            assert st["layer_sizes"][l + 1] == len(nodes) and (cl["min"], cl["max"]) == (int(deg.min()), int(deg.max())), c
        c0 = st["layer_connectivity"][0]
        assert (c0["min"], c0["max"]) == (int(hg.deg0.min()), int(hg.deg0.max())) and c0["mean"] == hg.deg0.sum() / model.n, c
        # -- the exact scan: as the script left the scan options, against float64; with both off, the same bits
        ks = (1, 10, min(model.n_live, 40))
        scans = [O.brute_force_knn(hg, k, Q) + (hg.scan_path(),) for k in ks]
        for name in ("scan_matrix", "scan_bytes"):
            hg.set_option(name, 0)
        plain = [O.brute_force_knn(hg, k, Q) + (hg.scan_path(),) for k in ks]
        for name in ("scan_matrix", "scan_bytes"):
            hg.set_option(name, self.opts.get(name, 0))
        for k, (ids, dist, path), (ids0, dist0, path0) in zip(ks, scans, plain):
            ck = "%s: brute_force_knn k %d" % (c, k)
            assert (path, path0) == (self.expected_path(), FLOAT), ck
            eq(ids, ids0, err_msg=ck + ", scan options on against off")
            eq(_bits(dist), _bits(dist0), err_msg=ck + ", scan options on against off")
            if self.metric != COSINE:
                rids, rdist = model.scan(Q, k)
                eq(ids, rids, err_msg=ck + " against float64")
                eq(_bits(dist), _bits(rdist), err_msg=ck + " against float64")
        radius = np.float32(np.median(scans[1][1][:, 9]))           # the median 10th-neighbour distance
        lims, ids, dist = O.brute_force_range(hg, radius, Q)
        if self.metric != COSINE:
            rlims, rids, rdist = model.range(Q, radius)
            eq(lims, rlims, err_msg=c + ": brute_force_range lims")
            eq(ids, rids, err_msg=c + ": brute_force_range ids")
            eq(_bits(dist), _bits(rdist), err_msg=c + ": brute_force_range distances")
        # -- against the twin
        twin = self.dress(H.Hgraph(model.rows.copy(), hg.deg0, hg.nbr0, hg.upper, entry_point=hg.entry_point, id_base=0,
                                   max_degree=hg.max_degree, metric=self.metric))
        assert twin.info().row_format == hg.info().row_format, c
        # about 10 % of the nodes under a fixed seed, and all of W of the planted query's own walk at ef 16: while nothing is marked
        # that query finds k allowed nodes in its first W (stage 0); the others climb the ladder
        mask = np.random.default_rng(12).random(model.n) < 0.1
        w = O.knn_batch_bigarray(hg, 16, Q[7:8], ef=16)[0][0]
        mask[w[w >= 0]] = True
        live = np.flatnonzero(~model.marked)
        by_id = live[np.random.default_rng(13).choice(len(live), size=NQ, replace=False)]
        mine, theirs = self.answers(hg, mask, radius, by_id), self.answers(twin, mask, radius, by_id)
        twin.release()
        for name in mine:
            assert len(mine[name]) == len(theirs[name])
            for j, (a, b) in enumerate(zip(mine[name], theirs[name])):
                eq(a, b, err_msg="%s: %s, output %d, the handle against its fresh twin" % (c, name, j))
        stage = mine["filtered"][3]
        self.stage0, self.later = self.stage0 or bool((stage == 0).any()), self.later or bool((stage > 0).any())
        self.trace.append((hg.info().row_format, scans[0][2]))

    def stale(self, flt, labels, moved):
        """a filter and a labels object made before the step: refused iff the step moved a row or a mark"""
        H, hg, Q = self.H, self.hg, self.Q[:2]
        if moved:
            with pytest.raises(H.InvalidArgument):
                H.Ohnsw.knn_batch_filtered(hg, 5, Q, flt, ef=16)
            with pytest.raises(H.InvalidArgument):
                H.Ohnsw.knn_batch_grouped(hg, 3, Q, labels, ef=16)
        else:
            H.Ohnsw.knn_batch_filtered(hg, 5, Q, flt, ef=16)
            H.Ohnsw.knn_batch_grouped(hg, 3, Q, labels, ef=16)
        flt.release()
        labels.release()

    def finish(self):
        """unmark or compact, save, load: the same export and bits; then the same 50 rows into both: the same export"""
        H, hg, model, Q = self.H, self.hg, self.model, self.Q
        self.ctx = "%s / %s, at the end" % (self.world, self.name)
        if model.marked.any():
            if int(model.marked.sum()) % 2:
                eq(hg.compact(), model.compact(), err_msg=self.ctx)
            else:
                ids = np.flatnonzero(model.marked)
                hg.unmark_deleted(ids)
                model.unmark(ids)
            self.check()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "sequence.hnsw")
            hg.save(path)
            again = self.dress(H.Hgraph.load(path))
        _same_export(again.export(), hg.export())
        eq(_bits(again.rows()), _bits(hg.rows()), err_msg=self.ctx)
        for ef in (16, 200):
            for a, b in zip(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=ef, counters=True)[::3],
                            H.Ohnsw.knn_batch_bigarray(again, 10, Q, ef=ef, counters=True)[::3]):
                eq(a, b, err_msg="%s: the loaded copy, ef %d" % (self.ctx, ef))
            eq(_bits(H.Ohnsw.knn_batch_bigarray(hg, 10, Q, ef=ef)[1]), _bits(H.Ohnsw.knn_batch_bigarray(again, 10, Q, ef=ef)[1]),
               err_msg="%s: the loaded copy, ef %d" % (self.ctx, ef))
        X = _gen(self.world, 50, 999)
        if model.keys is None:
            H.Ohnsw.insert_batch(again, X, M, EFC, seed=SEED)
        else:
            H.Ohnsw.insert_batch_keyed(again, X, np.arange(self.next_key, self.next_key + 50), M, EFC, seed=SEED)
        self.insert(X)
        _same_export(again.export(), hg.export())
        eq(_bits(again.rows()), _bits(hg.rows()), err_msg=self.ctx)
        again.release()


@pytest.mark.parametrize("name", sorted(SCRIPTS))
@pytest.mark.parametrize("world", sorted(WORLDS))
def test_a_mutation_sequence_against_the_model_and_a_fresh_twin(H, world, name):
    steps = SCRIPTS[name]
    assert 8 <= len(steps) <= 12
    run = Run(H, world, name)
    hg, model = run.hg, run.model
    want_format = {"ip": ROWS_SPLIT, "bytes": ROWS_BYTES}.get(world)
    assert want_format is None or hg.info().row_format == want_format
    run.check()
    run.stage0 = run.later = False      # the stages count in the steps' own checks
    for i, step in enumerate(steps):
        run.ctx = "%s / %s, step %d %r of %r" % (world, name, i, step, steps)
        before = model.state()
        flt, labels = hg.filter(np.arange(model.n) % 2 == 0), hg.labels(np.arange(model.n) % 7)
        run.apply(step)
        run.stale(flt, labels, model.state() != before)
        run.check()
    assert run.stage0 and run.later, "%s / %s: the filtered search never saw both a stage-0 query and a later stage" % (world, name)
    assert CALLS[name] <= run.called, (CALLS[name] - run.called, world, name)
    if (world, name) == ("bytes", "A"):
        # trace[0] is the fresh handle; step 2 inserts the rows with a value of 0.5, step 8 removes exactly those
        formats, paths = [t[0] for t in run.trace], [t[1] for t in run.trace]
        assert formats[2] == ROWS_BYTES and formats[3] in (ROWS_F32, ROWS_SPLIT) and formats[8] == formats[3] and formats[9] == ROWS_BYTES, formats
        assert (paths[2], paths[3], paths[8], paths[9]) == (BYTES, MATRIX, MATRIX, BYTES), paths
    run.finish()
    hg.release()
