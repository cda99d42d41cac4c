"""The bytes hnsw_index_info.device_bytes counts for an index, restated from the sizes of its device tables (test helper)."""

ROWS_BYTES, ROWS_SPLIT = 2, 3


def base_bytes(hg, created=False):
    """the vectors and the graph: max(n, 1) rows of the padded stride, the layer-0 adjacency, max(rowsU, 1) upper rows, and
    off (4) + lvl (1) + ref (8) bytes per node.  `hg` must be exported (its upper layers give rowsU).  An index made by
    hnsw_index_create with no upper layer has upper rows of one slot; a built or grown one has rows of max_degree."""
    inf = hg.info()
    n, S0 = inf.n, inf.max_degree0
    stride = inf.row_stride_bytes // 4
    SU = inf.max_degree if inf.max_layer > 0 or not created else 1
    rowsU = sum(len(nodes) for nodes, _, _ in hg.upper)
    return max(n, 1) * stride * 4 + n * S0 * 4 + max(rowsU, 1) * SU * 4 + 13 * max(n, 1)


def byte_row_bytes(n, d):
    c = -(-d // 4)
    nch = next(x for x in (1, 2, 4, 8, 16) if 16 * x >= c)
    return n * 64 * nch


def split_row_bytes(n, d, S0):
    c = -(-d // 4)
    T = c % 8
    return n * 16 * (c - T) + n * S0 * 16 * T if T in (1, 2) and c >= 9 else 0


def expected(hg, d, created=False):
    """base plus the row copy that hg.info().row_format reports (byte rows switched off by option still count: pass them
    yourself)"""
    inf = hg.info()
    extra = 0
    if inf.row_format == ROWS_BYTES:
        extra = byte_row_bytes(inf.n, d)
    elif inf.row_format == ROWS_SPLIT:
        extra = split_row_bytes(inf.n, d, inf.max_degree0)
    return base_bytes(hg, created) + extra
