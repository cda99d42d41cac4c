"""tests/mutation_model.py pinned on hand-written cases: every expected array is written out.  The model is the yardstick of
tests/test_gpu_mutation_sequences.py, and a library compared with a wrong model proves nothing.  No GPU."""
import numpy as np
import pytest
from mutation_model import IP, L2, Model

R = [[0, 0], [1, 0], [0, 2], [3, 0], [0, 4], [5, 5]]
K = [10, 11, 12, 13, 14, 15]
eq = np.testing.assert_array_equal


def _holds(m, rows, keys, marked):
    eq(m.rows, np.array(rows, np.float32))
    assert m.rows.dtype == np.float32 and m.n == len(rows)
    if keys is None:
        assert m.keys is None
    else:
        eq(m.keys, np.array(keys, np.int64))
        assert m.keys.dtype == np.int64
    eq(m.marked, np.array(marked, bool))
    assert m.n_live == len(rows) - sum(marked)


def test_removal_deletes_rows_and_renumbers_the_survivors_in_order():
    m = Model(R, keys=K)
    new_id = m.remove([4, 1])
    eq(new_id, [0, -1, 1, 2, -1, 3])
    assert new_id.dtype == np.int32
    _holds(m, [[0, 0], [0, 2], [3, 0], [5, 5]], [10, 12, 13, 15], [0, 0, 0, 0])
    eq(m.remove([]), [0, 1, 2, 3])
    eq(m.remove_keys([15, 10]), [-1, 0, 1, -1])
    _holds(m, [[0, 2], [3, 0]], [12, 13], [0, 0])


def test_marks_travel_with_their_rows_through_a_removal():
    m = Model(R)
    m.mark([5, 2])
    eq(m.remove([0]), [-1, 0, 1, 2, 3, 4])
    _holds(m, R[1:], None, [0, 1, 0, 0, 1])
    eq(m.remove([1]), [0, -1, 1, 2, 3])                 # a marked node removed: its mark is gone with it
    _holds(m, [[1, 0], [3, 0], [0, 4], [5, 5]], None, [0, 0, 0, 1])


def test_compact_is_the_removal_of_the_marked_rows():
    m = Model(R, keys=K)
    m.mark([3, 1])
    eq(m.compact(), [0, -1, 1, -1, 2, 3])
    _holds(m, [[0, 0], [0, 2], [0, 4], [5, 5]], [10, 12, 14, 15], [0, 0, 0, 0])
    eq(m.compact(), [0, 1, 2, 3])                       # nothing marked: the identity
    _holds(m, [[0, 0], [0, 2], [0, 4], [5, 5]], [10, 12, 14, 15], [0, 0, 0, 0])


def test_unmark_of_part_of_the_marked_ids_by_id_and_by_key():
    m = Model(R, keys=K)
    m.mark([1, 2, 3])
    m.unmark([2, 0])                                    # node 0 was live: it stays as it is
    _holds(m, R, K, [0, 1, 0, 1, 0, 0])
    m.mark_keys([15, 11])                               # key 11 is marked already
    _holds(m, R, K, [0, 1, 0, 1, 0, 1])
    m.unmark_keys([13])
    _holds(m, R, K, [0, 1, 0, 0, 0, 1])


def test_inserted_rows_are_appended_live():
    m = Model(R)
    m.mark([5])
    eq(m.insert([[7, 7]]), [6])
    _holds(m, R + [[7, 7]], None, [0, 0, 0, 0, 0, 1, 0])
    m = Model(R, keys=K)
    eq(m.insert_keyed([[7, 7], [8, 8]], [21, 20]), [6, 7])
    _holds(m, R + [[7, 7], [8, 8]], K + [21, 20], [0] * 8)


def test_upsert_with_half_the_keys_stored():
    m = Model(R, keys=K)
    replaced, new_id = m.upsert_keyed([[9, 9], [8, 8], [7, 7]], [12, 30, 15])
    eq(replaced, [True, False, True])
    eq(new_id, [0, 1, -1, 2, 3, -1])
    _holds(m, [[0, 0], [1, 0], [3, 0], [0, 4], [9, 9], [8, 8], [7, 7]], [10, 11, 13, 14, 12, 30, 15], [0] * 7)


def test_upsert_of_a_marked_key_comes_back_live_and_the_other_marks_move():
    m = Model(R, keys=K)
    m.mark([2, 3])
    replaced, new_id = m.upsert_keyed([[9, 9]], [12])
    eq(replaced, [True])
    eq(new_id, [0, 1, -1, 2, 3, 4])
    _holds(m, [[0, 0], [1, 0], [3, 0], [0, 4], [5, 5], [9, 9]], [10, 11, 13, 14, 15, 12], [0, 0, 1, 0, 0, 0])


def test_upsert_with_no_key_stored_and_with_all_stored():
    m = Model(R, keys=K)
    replaced, new_id = m.upsert_keyed([[6, 6]], [40])
    eq(replaced, [False])
    eq(new_id, [0, 1, 2, 3, 4, 5])
    _holds(m, R + [[6, 6]], K + [40], [0] * 7)
    m = Model(R, keys=K)
    m.mark([0])
    X = [[1, 1], [2, 2], [3, 3], [4, 4], [5, 5], [6, 6]]
    replaced, new_id = m.upsert_keyed(X, K[::-1])
    eq(replaced, [True] * 6)
    eq(new_id, [-1] * 6)
    _holds(m, X, [15, 14, 13, 12, 11, 10], [0] * 6)       # the whole call in call order


def test_update_is_the_same_by_id():
    m = Model(R)
    m.mark([0, 1])
    eq(m.update([4, 0], [[6, 6], [7, 7]]), [-1, 0, 1, 2, -1, 3])
    _holds(m, [[1, 0], [0, 2], [3, 0], [5, 5], [6, 6], [7, 7]], None, [1, 0, 0, 0, 0, 0])


def test_a_refused_call_changes_nothing():
    m = Model(R, keys=K)
    m.mark([4])
    refused = [lambda: m.insert_keyed([[1, 1], [2, 2]], [20, 20]), lambda: m.insert_keyed([[1, 1]], [10]), lambda: m.insert([[1, 1]]),
               lambda: m.remove([6]), lambda: m.remove([-1]), lambda: m.remove([1, 1]), lambda: m.remove_keys([99]),
               lambda: m.mark([0, 6]), lambda: m.unmark([2, 2]), lambda: m.mark_keys([10, 99]), lambda: m.unmark_keys([99]),
               lambda: m.update([0], [[1, 1]]), lambda: m.upsert_keyed([[1, 1], [2, 2]], [50, 50]), lambda: m.set_keys([1, 2, 3]),
               lambda: m.set_keys([1, 2, 3, 4, 5, 5])]
    for call in refused:
        with pytest.raises(ValueError):
            call()
        _holds(m, R, K, [0, 0, 0, 0, 1, 0])
    bare = Model(R)
    for call in (lambda: bare.insert_keyed([[1, 1]], [1]), lambda: bare.upsert_keyed([[1, 1]], [1]), lambda: bare.find_keys([1]),
                 lambda: bare.remove_keys([1]), lambda: bare.update([1, 1], [[1, 1], [2, 2]]), lambda: bare.update([6], [[1, 1]])):
        with pytest.raises(ValueError):
            call()
        _holds(bare, R, None, [0] * 6)


def test_keys_are_found_set_cleared_and_set_again():
    m = Model(R, keys=K)
    eq(m.find_keys([13, 99, 10, 13]), [3, -1, 0, 3])
    assert m.find_keys([13]).dtype == np.int64
    m.remove([1])
    eq(m.find_keys([13, 11, 10]), [2, -1, 0])
    m.clear_keys()
    _holds(m, [R[0]] + R[2:], None, [0] * 5)
    eq(m.insert([[2, 2]]), [5])                          # an index that never had keys
    m.set_keys([-1, 0, 2 ** 63 - 1, -2 ** 63, 5, 7])
    eq(m.find_keys([2 ** 63 - 1, -2 ** 63, 1]), [2, 3, -1])


def test_the_scan_orders_by_squared_sum_then_id_over_the_live_rows():
    m = Model(R)
    ids, dist = m.scan([[0, 0]], 3)
    eq(ids, [[0, 1, 2]])
    eq(dist, np.array([[0, 1, 2]], np.float32))
    assert ids.dtype == np.int32 and dist.dtype == np.float32
    m.mark([0])
    ids, dist = m.scan([[0, 0], [5, 5]], 3)
    eq(ids, [[1, 2, 3], [5, 4, 3]])
    eq(dist, np.sqrt(np.array([[1, 4, 9], [0, 26, 29]], np.float64)).astype(np.float32))
    t = Model([[1, 0], [0, 1], [1, 0], [0, 0], [2, 0]])   # three rows at one distance: lowest id first
    ids, dist = t.scan([[0, 0]], 7)
    eq(ids, [[3, 0, 1, 2, 4, -1, -1]])
    eq(dist, np.array([[0, 1, 1, 1, 2, np.nan, np.nan]], np.float32))
    t.mark([1, 3])
    eq(t.scan([[0, 0]], 2)[0], [[0, 2]])


def test_the_scan_under_inner_product_orders_by_the_negated_dot_product():
    m = Model(R, metric=IP)
    ids, dist = m.scan([[1, 1]], 3)
    eq(ids, [[5, 4, 3]])
    eq(dist, np.array([[-9, -3, -2]], np.float32))
    t = Model([[1, 0], [0, 1], [1, 1], [0, 1]], metric=IP)   # dots 1 1 2 1 with [1, 1]: ties by id
    ids, dist = t.scan([[1, 1]], 4)
    eq(ids, [[2, 0, 1, 3]])
    eq(dist, np.array([[-1, 0, 0, 0]], np.float32))


def test_the_range_is_the_in_range_prefix_of_the_scan():
    m = Model(R, metric=L2)
    lims, ids, dist = m.range([[0, 0], [5, 5]], 2)
    eq(lims, [0, 3, 4])
    eq(ids, [0, 1, 2, 5])
    eq(dist, np.array([0, 1, 2, 0], np.float32))
    assert lims.dtype == np.int64 and ids.dtype == np.int32
    m.mark([1, 5])
    lims, ids, dist = m.range([[0, 0], [5, 5]], 3)
    eq(lims, [0, 3, 3])
    eq(ids, [0, 2, 3])
    eq(dist, np.array([0, 2, 3], np.float32))
