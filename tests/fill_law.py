"""fill_law.py -- the edge phase of a step restated from the reference (src/sampler.cpp:232-287 and the batch extension's column
rule), not from the kernels: given the rows of vertices a walk picked (`nodes`), the induced edge entries of every complete row
in (vertex j, adjacency position) order, numbered by mode.  Plain Python is the law; a numpy form of the same rule is checked
against it on every small case (tests/test_fill_law.py) and serves the calls of tens of thousands of rows.

`census` names, per row, the path the row-reading fill kernels (fill_row in ugs_kernels.hip) take for it, so that the inputs of
tests/fill_paths.py can be chosen -- and asserted -- by class.  The constants below restate the kernels'; test_fill_law.py reads
them back from the sources."""
import collections

import numpy as np

SUB_CHUNKS = 4              # sub-chunks of GS entries per chunk of fill_row
GS_NARROW, GS_WIDE = 8, 64  # lanes per row of ugs_fill<8> / ugs_fill_scan<8> and of ugs_fill<64>
LOOKUP_REGS = 8             # k up to here: member lookup and row prefix in registers; above: loops over LDS
TILE_ROWS = 32              # rows per tile of ugs_fill_scan<8>
SUM_ROWS = 8                # rows per sum word the walk leaves (wsum)
TRIP_TILES = 8 * 256        # tiles whose sums one trip of the `before` loop loads (8 sixteen-byte loads x 256 threads)
FUSED_MAX_ROWS = 131072     # largest row count of the fused scan (and of the packed step)
GRID_PER_CU = 8             # blocks per CU at which the fill grids are capped
STAGE_ITEMS = 64            # directed items per row of the walk's staging (UGS_STAGE_ITEMS)
PACKED_STAGING_BYTES = 192 << 20
MODES = ("sample", "graph", "global", "batch")


def graph_of(ptr):
    """batch vertex -> graph index, -1 for ids that belong to no graph"""
    ptr = [int(x) for x in ptr]
    g = [-1] * max(ptr[-1], 0)
    for i in range(len(ptr) - 1):
        for v in range(max(ptr[i], 0), ptr[i + 1]):
            g[v] = i
    return g


def adjacency(edge_index, ptr):
    """Per batch vertex 0 .. ptr[-1] - 1 its (neighbour, column) entries in column order; of a column's two entries the source's
    comes first, a self loop gives two equal entries.  Columns that leave the batch or join two graphs give nothing."""
    n = max(int(ptr[-1]), 0)
    g = graph_of(ptr)
    adj = [[] for _ in range(n)]
    for c in range(len(edge_index[0])):
        u, v = int(edge_index[0][c]), int(edge_index[1][c])
        if not (0 <= u < n and 0 <= v < n) or g[u] < 0 or g[u] != g[v]:
            continue
        adj[u].append((v, c))
        adj[v].append((u, c))
    return adj


def endpoints(mode, k, m, row_abs, row_rel, j, l, row):
    if mode == "sample":
        return j, l
    if mode == "graph":
        i = row_abs % m
        return i * k + j, i * k + l
    if mode == "batch":
        return row_rel * k + j, row_rel * k + l
    assert mode == "global", mode
    return int(row[j]), int(row[l])


def row_entries(adj, row, extra_node_offset=0):
    """The flattened adjacency entries of a complete row: [(j, neighbour, column, l or None)], l = first position of the
    neighbour in the row.  (No walk puts a vertex into a row twice; for such a row the reference's map would name the last
    position, the fill's contract is rows of distinct vertices.)"""
    loc = [int(v) - extra_node_offset for v in row]
    first = {}
    for j, v in enumerate(loc):
        first.setdefault(v, j)
    return [(j, w, c, first.get(w)) for j, v in enumerate(loc) for w, c in adj[v]]


def edge_phase(edge_index, ptr, nodes, m, k, mode, row_begin=0, extra_node_offset=0, adj=None):
    """(edge_ptr [rows + 1], edge_index [2, total], edge_src [total]) of the rows `nodes` [rows, k] (batch ids + extra_node_offset,
    -1 in a row = incomplete: skipped)."""
    adj = adjacency(edge_index, ptr) if adj is None else adj
    nodes = np.asarray(nodes, np.int64).reshape(-1, k)
    eptr, eu, ev, es = [0], [], [], []
    for r, row in enumerate(nodes):
        if (row >= 0).all():
            for j, _, c, l in row_entries(adj, row, extra_node_offset):
                if l is not None:
                    a, b = endpoints(mode, k, m, row_begin + r, r, j, l, row)
                    eu.append(a), ev.append(b), es.append(c)
        eptr.append(len(es))
    return np.array(eptr, np.int64), np.array([eu, ev], np.int64).reshape(2, -1), np.array(es, np.int64)


def csr(edge_index, ptr):
    """The adjacency as arrays (rowptr [n + 1], neighbour, column), built by sorting instead of appending."""
    ei, ptr = np.asarray(edge_index, np.int64).reshape(2, -1), np.asarray(ptr, np.int64)
    n = max(int(ptr[-1]), 0)
    u, v = ei[0], ei[1]
    gu, gv = np.searchsorted(ptr, u, "right") - 1, np.searchsorted(ptr, v, "right") - 1
    ok = (u >= 0) & (u < n) & (v >= 0) & (v < n) & (gu == gv) & (gu >= 0)
    c = np.nonzero(ok)[0]
    owner = np.stack([u[c], v[c]], 1).ravel()
    other = np.stack([v[c], u[c]], 1).ravel()
    order = np.argsort(owner, kind="stable")
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=rowptr[1:])
    return rowptr, other[order], np.repeat(c, 2)[order]


def edge_phase_np(edge_index, ptr, nodes, m, k, mode, row_begin=0, extra_node_offset=0, graph=None):
    """edge_phase, vectorised (the same rule; `graph` = csr(edge_index, ptr) if the caller has it)."""
    rowptr, nbr, col = csr(edge_index, ptr) if graph is None else graph
    nodes = np.asarray(nodes, np.int64).reshape(-1, k)
    rows_c = np.nonzero((nodes >= 0).all(1))[0]
    V = nodes[rows_c] - extra_node_offset
    deg = (rowptr[V + 1] - rowptr[V]).ravel()
    T = int(deg.sum())
    pair = np.repeat(np.arange(deg.size), deg)
    pos = np.repeat(rowptr[V].ravel(), deg) + np.arange(T) - np.repeat(np.cumsum(deg) - deg, deg)
    rr, j = pair // k, pair % k
    eq = V[rr] == nbr[pos][:, None]
    hit = eq.any(1)
    rr, j, l, src = rr[hit], j[hit], eq.argmax(1)[hit], col[pos][hit]
    edge_ptr = np.zeros(len(nodes) + 1, np.int64)
    cnt = np.zeros(len(nodes), np.int64)
    cnt[rows_c] = np.bincount(rr, minlength=len(rows_c))
    np.cumsum(cnt, out=edge_ptr[1:])
    rel = rows_c[rr]
    if mode == "sample":
        a, b = j, l
    elif mode == "graph":
        i = (row_begin + rel) % m
        a, b = i * k + j, i * k + l
    elif mode == "batch":
        a, b = rel * k + j, rel * k + l
    else:
        assert mode == "global", mode
        a, b = nodes[rel, j], nodes[rel, l]
    return edge_ptr, np.stack([a, b]).astype(np.int64).reshape(2, -1), src.astype(np.int64)


# ---- census: the path of every row through fill_row<GS> ----------------------------------------------------------------------
T_CLASSES = ("T odd", "T % GS == GS - 1", "T % GS == 0", "T % GS == 1", "T % 4GS == 4GS - 1", "T % 4GS == 0", "T % 4GS == 1")
ROW_CLASSES = ("k <= 8", "k > 8", "1 chunk", "2 chunks", ">= 3 chunks", "sub-chunk without a hit", "full sub-chunk of hits",
               "hits == 64", "hits == 66")
ROWS_CLASSES = ("incomplete row", "complete row without a hit", "hitless row between rows with hits",
                "incomplete row between rows with hits")
IMPOSSIBLE = ("hits == 65",)   # a column inside a row gives two entries (one per endpoint, or both at a looped vertex): hits are even


def row_classes(hit, k, GS):
    """Classes of one complete row with at least one hit; hit[e] = flattened entry e is a hit."""
    T, out = len(hit), []
    kc = "k <= 8" if k <= LOOKUP_REGS else "k > 8"
    out.append(kc)
    chunk = SUB_CHUNKS * GS
    t = []
    if T % 2:
        t.append("T odd")
    for name, mod in (("GS", GS), ("4GS", chunk)):
        for r, label in ((mod - 1, f"{name} - 1"), (0, "0"), (1, "1")):
            if T % mod == r:
                t.append(f"T % {name} == {label}")
    out += t + [f"{kc}, {x}" for x in t]
    chunks = -(-T // chunk)
    out.append("1 chunk" if chunks == 1 else "2 chunks" if chunks == 2 else ">= 3 chunks")
    subs = [hit[s:s + GS] for s in range(0, T, GS)]
    if any(not any(s) for s in subs):
        out.append("sub-chunk without a hit")
    if any(len(s) == GS and all(s) for s in subs):
        out.append("full sub-chunk of hits")
    n = sum(hit)
    if n in (64, 65, 66):
        out.append(f"hits == {n}")
    return out


def census(edge_index, ptr, nodes, k, GS, extra_node_offset=0, adj=None):
    """Counter: class -> rows of `nodes` that reach it under fill_row<GS>."""
    adj = adjacency(edge_index, ptr) if adj is None else adj
    nodes = np.asarray(nodes, np.int64).reshape(-1, k)
    out, kind = collections.Counter(), []
    for row in nodes:
        if not (row >= 0).all():
            out["incomplete row"] += 1
            kind.append("i")
            continue
        hit = [l is not None for _, _, _, l in row_entries(adj, row, extra_node_offset)]
        if not any(hit):
            out["complete row without a hit"] += 1
            kind.append("0")
            continue
        kind.append("h")
        out.update(row_classes(hit, k, GS))
    with_hits = [r for r, x in enumerate(kind) if x == "h"]
    if with_hits:
        between = kind[with_hits[0]:with_hits[-1]]
        out["hitless row between rows with hits"] += between.count("0")
        out["incomplete row between rows with hits"] += between.count("i")
    return out


# ---- row counts of the fused step ---------------------------------------------------------------------------------------------
def fused_tiles(rows):
    return -(-rows // TILE_ROWS)


def fused_grid(rows, cus):
    return max(1, min(fused_tiles(rows), GRID_PER_CU * cus))


def packed_words(rows, k):
    """int64 words of the packed step's staging: 3 x the bound of 2 k (k - 1) entries per row"""
    return 3 * rows * 2 * k * (k - 1)


def may_pack(rows, k):
    """begin_common's rule for a batch of small graphs"""
    return k >= 2 and 0 < rows <= FUSED_MAX_ROWS and packed_words(rows, k) * 8 <= PACKED_STAGING_BYTES
