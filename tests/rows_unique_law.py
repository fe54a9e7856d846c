"""The law of ugs_sampler.rows.unique_rows (include/ugs_mi355.h at ugs_rows_unique_begin) in plain numpy, with one dict of tuples
per graph, and the input generators its tests share.  No GPU and no library call here."""
import numpy as np

MAX_ROWS_PER_GRAPH = 4096


def key_bits(k):
    return min(31, 128 // k)


def row_key(row, by):
    """The key of a row: its entries in order ("sequence") or sorted ascending ("set"); -1 is a value like any other."""
    t = tuple(int(v) for v in row)
    return t if by == "sequence" else tuple(sorted(t))


def check_limits(nodes, sample_ptr, ptr):
    """What the kernels refuse: the first offending graph or row, as the text of the refusal's name, or None."""
    R, k = nodes.shape
    b = key_bits(k)
    for g in range(len(sample_ptr) - 1):
        rows = int(sample_ptr[g + 1] - sample_ptr[g])
        if rows > 0 and rows > MAX_ROWS_PER_GRAPH:
            return f"graph {g}"
        if rows > 0 and int(ptr[g + 1] - ptr[g]) + 1 > (1 << b):
            return f"graph {g}"
    for g in range(len(sample_ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        for r in range(int(sample_ptr[g]), int(sample_ptr[g + 1])):
            for v in nodes[r]:
                if v != -1 and not lo <= v < hi:
                    return f"row {r}"
    return None


def unique_rows(nodes, edge_index, edge_ptr, sample_ptr, edge_src, ptr, by="set"):
    """The seven arrays of the law, int64: (nodes_u [U, k], edge_index_u [2, Eu], edge_ptr_u [U + 1], sample_ptr_u [G + 1],
    edge_src_u [Eu] (empty where edge_src is), count [U], inverse [R])."""
    assert by in ("set", "sequence")
    nodes = np.asarray(nodes, dtype=np.int64)
    edge_index = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    edge_ptr = np.asarray(edge_ptr, dtype=np.int64)
    sample_ptr = np.asarray(sample_ptr, dtype=np.int64)
    edge_src = np.asarray(edge_src, dtype=np.int64)
    R, k = nodes.shape
    G = len(sample_ptr) - 1
    assert check_limits(nodes, sample_ptr, ptr) is None
    kept, count, inverse = [], [], np.zeros(R, dtype=np.int64)
    sample_ptr_u = np.zeros(G + 1, dtype=np.int64)
    for g in range(G):
        seen = {}                                           # key -> position in the result
        for r in range(int(sample_ptr[g]), int(sample_ptr[g + 1])):
            key = row_key(nodes[r], by)
            if key not in seen:
                seen[key] = len(kept)
                kept.append(r)
                count.append(0)
            count[seen[key]] += 1
            inverse[r] = seen[key]
        sample_ptr_u[g + 1] = len(kept)
    U = len(kept)
    nodes_u = nodes[kept].reshape(U, k) if U else np.zeros((0, k), dtype=np.int64)
    spans = [np.arange(int(edge_ptr[r]), int(edge_ptr[r + 1])) for r in kept]
    cols = np.concatenate(spans).astype(np.int64) if spans else np.zeros(0, dtype=np.int64)
    edge_ptr_u = np.zeros(U + 1, dtype=np.int64)
    if U:
        edge_ptr_u[1:] = np.cumsum([len(s) for s in spans])
    edge_index_u = edge_index[:, cols]
    edge_src_u = edge_src[cols] if edge_src.size else np.zeros(0, dtype=np.int64)
    return (np.ascontiguousarray(nodes_u), np.ascontiguousarray(edge_index_u), edge_ptr_u, sample_ptr_u, np.ascontiguousarray(edge_src_u),
            np.asarray(count, dtype=np.int64), inverse)


# ---- generators ----
def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def with_edges(nodes, rng, max_edges=4, edge_src=True):
    """edge_index, edge_ptr and edge_src for rows `nodes`: every row gets 0..max_edges entries with values that tell its row and
    position, so that a span copied to the wrong place, or from the wrong row, shows."""
    R = nodes.shape[0]
    lens = rng.integers(0, max_edges + 1, size=R) if R else np.zeros(0, dtype=np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Es = int(edge_ptr[-1])
    row_of = np.repeat(np.arange(R), lens).astype(np.int64)
    pos = np.arange(Es, dtype=np.int64) - edge_ptr[row_of] if Es else np.zeros(0, dtype=np.int64)
    edge_index = np.stack([row_of * 1000 + pos, -(row_of * 1000 + pos) - 7]).astype(np.int64).reshape(2, Es)
    src = (row_of * 31 + pos * 3 + 5).astype(np.int64) if edge_src else np.zeros(0, dtype=np.int64)
    return edge_index, edge_ptr, src


def random_case(rng, rows_per_graph, k, graph_sizes=None, distinct=6, minus_one=0.1, max_edges=4, edge_src=True):
    """A batch with rows_per_graph[g] rows in graph g, drawn from `distinct` base rows per graph and permuted at random, so that
    rows repeat as sets and, less often, as sequences; some entries are -1 and some rows are all -1."""
    G = len(rows_per_graph)
    sizes = list(graph_sizes) if graph_sizes is not None else [int(rng.integers(max(k, 2), 3 * k + 2)) for _ in range(G)]
    b = key_bits(k)
    sizes = [min(n, (1 << b) - 1) for n in sizes]
    ptr = ptr_of(sizes)
    rows = []
    for g, cnt in enumerate(rows_per_graph):
        n = sizes[g]
        base = rng.integers(0, n, size=(max(distinct, 1), k)) + ptr[g]
        base[rng.random(base.shape) < minus_one] = -1
        if distinct > 1:
            base[0, :] = -1
        for _ in range(cnt):
            row = base[int(rng.integers(0, base.shape[0]))].copy()
            if rng.random() < 0.6:
                rng.shuffle(row)
            rows.append(row)
    nodes = np.array(rows, dtype=np.int64).reshape(len(rows), k)
    sample_ptr = ptr_of(rows_per_graph)
    edge_index, edge_ptr, src = with_edges(nodes, rng, max_edges, edge_src)
    return nodes, edge_index, edge_ptr, sample_ptr, src, ptr


def kept_fraction(nodes, sample_ptr, by):
    total = 0
    for g in range(len(sample_ptr) - 1):
        total += len({row_key(nodes[r], by) for r in range(int(sample_ptr[g]), int(sample_ptr[g + 1]))})
    return total / max(nodes.shape[0], 1)
