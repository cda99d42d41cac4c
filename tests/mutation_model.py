"""A model of what a live index HOLDS, in plain numpy (no GPU, no graph): the float32 rows in id order, the int64 keys (or none) and
the marks, moved through every mutation call by the words of include/hnsw_mi355x.h -- removal deletes rows and renumbers the
survivors in order (NUMBERING), compact is the removal of the marked rows, an upsert is remove_keys of the stored keys followed by
an append of the whole call in call order, update the same by id, new and replaced rows are live, marks and keys travel with their
rows.  A call the header refuses raises ValueError and changes nothing.  Ids are 0-based (id_base 0).

The model also gives the float64 reference of the exact scan over its LIVE rows: the k smallest under (squared sum or negated dot
product, id), distances rounded to float32 once (what _reference of tests/test_gpu_scan_matrix.py does), and the range form of it.
tests/test_mutation_model.py pins all of this on hand-written cases; tests/test_gpu_mutation_sequences.py holds the library to it."""
import numpy as np

L2, IP = 0, 1


class Model:
    def __init__(self, rows, metric=L2, keys=None):
        self.rows = np.array(rows, dtype=np.float32)
        assert self.rows.ndim == 2
        self.metric = metric
        self.marked = np.zeros(len(self.rows), bool)
        self.keys = None
        if keys is not None:
            self.set_keys(keys)

    # ---- what it holds ----
    @property
    def n(self):
        return len(self.rows)

    @property
    def n_live(self):
        return int((~self.marked).sum())

    def state(self):
        """rows and marks as bytes: equal before and after a call <=> the call moved no node and no mark"""
        return self.rows.tobytes(), self.marked.tobytes()

    # ---- checks shared by the calls ----
    def _ids(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= self.n):
            raise ValueError("an id out of range")
        if len(np.unique(ids)) != len(ids):
            raise ValueError("an id twice")
        return ids

    def _distinct(self, keys):
        keys = np.asarray(keys, np.int64).reshape(-1)
        if len(np.unique(keys)) != len(keys):
            raise ValueError("a key twice")
        return keys

    def _need_keys(self):
        if self.keys is None:
            raise ValueError("the index has no keys")

    def find_keys(self, keys):
        """the id under each key, -1 where no node has it"""
        self._need_keys()
        keys = np.asarray(keys, np.int64).reshape(-1)
        where = {int(k): v for v, k in enumerate(self.keys)}
        return np.array([where.get(int(k), -1) for k in keys], np.int64)

    def _stored(self, keys):
        ids = self.find_keys(keys)
        if (ids < 0).any():
            raise ValueError("an absent key")
        return ids

    # ---- keys ----
    def set_keys(self, keys):
        keys = self._distinct(keys)
        if len(keys) != self.n:
            raise ValueError("one key per node")
        self.keys = keys.copy()

    def clear_keys(self):
        self.keys = None

    # ---- growth ----
    def _append(self, X, keys):
        X = np.asarray(X, np.float32).reshape(-1, self.rows.shape[1])
        first = self.n
        self.rows = np.concatenate([self.rows, X])
        self.marked = np.concatenate([self.marked, np.zeros(len(X), bool)])
        if keys is not None:
            self.keys = np.concatenate([self.keys, keys])
        return np.arange(first, first + len(X), dtype=np.int64)

    def insert(self, X):
        if self.keys is not None:
            raise ValueError("an index with keys takes the keyed call")
        return self._append(X, None)

    def insert_keyed(self, X, keys):
        keys = self._distinct(keys)
        if self.keys is None and self.n:
            raise ValueError("the index has nodes and no keys")
        if len(keys) != len(X):
            raise ValueError("one key per row")
        if self.keys is None:
            self.keys = np.zeros(0, np.int64)
        if np.isin(keys, self.keys).any():
            raise ValueError("a stored key")
        return self._append(X, keys)

    # ---- removal ----
    def remove(self, ids):
        """-> new_id [n_old] int32: the id each old node has afterwards, -1 for a removed one"""
        ids = self._ids(ids)
        dead = np.zeros(self.n, bool)
        dead[ids] = True
        new_id = np.where(dead, -1, np.cumsum(~dead) - 1).astype(np.int32)
        self.rows, self.marked = self.rows[~dead], self.marked[~dead]
        if self.keys is not None:
            self.keys = self.keys[~dead]
        return new_id

    def remove_keys(self, keys):
        return self.remove(self._stored(self._distinct(keys)))

    def compact(self):
        return self.remove(np.flatnonzero(self.marked))

    # ---- marks ----
    def mark(self, ids):
        self.marked[self._ids(ids)] = True

    def unmark(self, ids):
        self.marked[self._ids(ids)] = False

    def mark_keys(self, keys):
        self.mark(self._stored(self._distinct(keys)))

    def unmark_keys(self, keys):
        self.unmark(self._stored(self._distinct(keys)))

    # ---- replace ----
    def upsert_keyed(self, X, keys):
        """-> (replaced [m] bool, new_id [n_old] int32)"""
        keys = self._distinct(keys)
        if self.keys is None and self.n:
            raise ValueError("the index has nodes and no keys")
        if len(keys) != len(X):
            raise ValueError("one key per row")
        if self.keys is None:
            self.keys = np.zeros(0, np.int64)
        replaced = np.isin(keys, self.keys)
        new_id = self.remove(self.find_keys(keys[replaced]))
        self._append(X, keys)
        return replaced, new_id

    def update(self, ids, X):
        if self.keys is not None:
            raise ValueError("an index with keys takes the keyed call")
        ids = self._ids(ids)
        if len(ids) != len(X):
            raise ValueError("one id per row")
        new_id = self.remove(ids)
        self._append(X, None)
        return new_id

    # ---- the exact scan over the live rows, in float64 ----
    def _order(self, Q):
        live = np.flatnonzero(~self.marked)
        x, q = self.rows[live].astype(np.float64), np.asarray(Q, np.float32).astype(np.float64)
        s = ((q[:, None, :] - x[None, :, :]) ** 2).sum(2) if self.metric == L2 else q @ x.T
        dist = np.sqrt(s).astype(np.float32) if self.metric == L2 else np.float32(1) - s.astype(np.float32)
        order = np.lexsort((np.broadcast_to(live, s.shape), s if self.metric == L2 else -s), axis=1)
        return live[order].astype(np.int32), np.take_along_axis(dist, order, 1)

    def scan(self, Q, k):
        """-> (ids [nq][k] int32, distances [nq][k] float32): -1 / NaN past the live rows"""
        ids, dist = self._order(Q)
        nq, have = len(ids), min(k, ids.shape[1])
        oi, od = np.full((nq, k), -1, np.int32), np.full((nq, k), np.nan, np.float32)
        oi[:, :have], od[:, :have] = ids[:, :have], dist[:, :have]
        return oi, od

    def range(self, Q, radius):
        """-> (lims [nq + 1] int64, ids, distances): per query the live rows with distance <= radius, in the scan's order"""
        ids, dist = self._order(Q)
        keep = dist <= np.float32(radius)
        lims = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
        return lims, ids[keep], dist[keep]
