"""preproc_law.py -- what the device preprocessing stages (csrc/ugs_preproc.hip: pre_keys, pre_entries, pre_widen, pre_roots,
pre_assemble) must leave for one graph, in plain Python and numpy: no GPU, no project library.

The law takes the columns, n, k and the host's degree order (order[vi] = vertex, index_of[vertex] = vi) as given: order_by_degree
stays on the host on both paths and tests/test_cabi_and_host.py holds it to the oracle.  `degree_order` restates it (stable
ascending sort by CSR degree) so that the inputs of tests/preproc_paths.py can be chosen and censused without the oracle;
tests/test_preproc_law.py asserts that it is the oracle's order on every input.

  csr(ei, n)                         indptr, indices, edge_col of the symmetrised multigraph
  suffix_deg / reach / bucket_b      the root stage and the weights through which reach shows in preproc_dump
  graph_law(ei, n, k)                all of it as one dict, plus Z, the count of non-zero weights and the relaxation level
  plan_arrays(law, colmap)           what a plan must hold for the graph (Plan.graph_csr)
  owned_columns(ei, lo, hi)          the column map of one graph of a batch
  census(ei, n, k)                   which of the paths of tests/preproc_paths.py an input reaches"""
import collections

import numpy as np

KMAX = 32          # UGS_KMAX: slots of pre_roots' private list
BLOCK = 256        # threads per block of every kernel of ugs_preproc.hip
DEFAULT_MIN_COLS = 1 << 21


def key_bits(n):
    """bits of the radix sort: the smallest b >= 1 with 2^b > n, so that the sentinel key n keeps its value (at most 32)"""
    bits = 1
    while bits < 32 and (1 << bits) <= n:
        bits += 1
    return bits


def kept(ei, n):
    """mask of the columns that count: both endpoints inside [0, n) as 64-bit values"""
    u, v = np.asarray(ei[0], np.int64), np.asarray(ei[1], np.int64)
    return (u >= 0) & (u < n) & (v >= 0) & (v < n)


def csr(ei, n):
    """rows in column order, a column's source-side entry (row u, neighbour v) before its target-side entry (row v, neighbour u)"""
    rows = collections.defaultdict(list)
    keep = kept(ei, n)
    for j in np.flatnonzero(keep).tolist():
        u, v = int(ei[0][j]), int(ei[1][j])
        rows[u].append((v, j))
        rows[v].append((u, j))
    deg = np.zeros(n, np.int64)
    for r, row in rows.items():
        deg[r] = len(row)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices, edge_col = np.zeros(int(indptr[n]), np.int32), np.zeros(int(indptr[n]), np.int32)
    for r, row in rows.items():
        a = int(indptr[r])
        indices[a:a + len(row)] = [w for w, _ in row]
        edge_col[a:a + len(row)] = [j for _, j in row]
    return indptr, indices, edge_col


def degree_order(indptr):
    """the host's order: stable ascending sort by (CSR degree, vertex id)"""
    order = np.argsort(np.diff(indptr), kind="stable").astype(np.int32)
    index_of = np.empty(len(order), np.int32)
    index_of[order] = np.arange(len(order), dtype=np.int32)
    return order, index_of


def suffix_deg(indptr, indices, order, index_of):
    """per order position vi: entries of order[vi]'s row whose neighbour has rank >= vi (a self loop's two entries both count)"""
    n = len(order)
    row_rank = np.repeat(index_of, np.diff(indptr))
    return np.bincount(row_rank[index_of[indices] >= row_rank], minlength=n).astype(np.int32)[:n]


def reached(indptr, indices, index_of, v, vi, k, suffix_only=True, bound=None):
    """the vertices the bounded breadth-first search from v collects, in order: neighbours of rank < vi are not entered, a vertex
    is entered once, and the search -- the scan of a row included -- stops as soon as `bound` (default k) vertices are held"""
    bound = k if bound is None else bound
    got, mark = [v], {v}
    h = 0
    while h < len(got) and len(got) < bound:
        u = got[h]
        h += 1
        for p in range(int(indptr[u]), int(indptr[u + 1])):
            if len(got) >= bound:
                break
            w = int(indices[p])
            if (suffix_only and index_of[w] < vi) or w in mark:
                continue
            mark.add(w)
            got.append(w)
    return got


def reach(indptr, indices, order, index_of, k):
    """per order position: does the root reach k vertices inside its suffix graph?  (k <= 1: every root holds itself already)"""
    n = len(order)
    out = np.zeros(n, bool)
    if k <= 1:
        out[:] = True
        return out
    deg = np.diff(indptr)
    for vi in np.flatnonzero(deg[order] > 0).tolist():          # a root with an empty row holds one vertex: not k >= 2
        out[vi] = len(reached(indptr, indices, index_of, int(order[vi]), vi, k)) >= k
    return out


def bucket_b(sdeg, rch, k):
    """max(1, sdeg)^(k-1) by repeated multiplication where the root reaches, 0 elsewhere"""
    d = np.maximum(sdeg, 1).astype(np.float64)
    b = np.ones(len(d), np.float64)
    for _ in range(1, k):
        b = b * d
    return np.where(rch, b, 0.0)


def graph_law(ei, n, k, order=None, index_of=None):
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    indptr, indices, edge_col = csr(ei, n)
    if order is None:
        order, index_of = degree_order(indptr)
    sdeg = suffix_deg(indptr, indices, order, index_of)
    rch = reach(indptr, indices, order, index_of, k)
    b = bucket_b(sdeg, rch, k)
    Z = 0.0
    for x in b[b > 0.0].tolist():                                # summed in order position order
        Z += x
    nonzero = int(np.count_nonzero(b > 0.0))
    if nonzero:
        level, viable = 0, np.zeros(0, np.int32)
    else:
        viable = np.flatnonzero(sdeg > 0).astype(np.int32)
        level = 1
        if len(viable) == 0:
            level, viable = 2, np.arange(n, dtype=np.int32)
    return {"n": n, "k": k, "E": ei.shape[1], "indptr": indptr, "indices": indices, "edge_col": edge_col, "order": np.asarray(order, np.int32),
            "index_of": np.asarray(index_of, np.int32), "suffix_deg": sdeg, "reach": rch, "bucket_b": b, "Z": Z, "nonzero": nonzero,
            "level": level, "viable_vi": viable, "viable_v": np.asarray(order, np.int32)[viable]}


def info_of(law):
    return {"num_nodes": law["n"], "num_edges_stored": len(law["indices"]), "Z": law["Z"], "bucket_count_nonzero": law["nonzero"]}


def plan_arrays(law, colmap=None):
    """the graph's rows as a plan holds them: adj = (nbr, nbr_rank), adjf = (nbr_f, nbr_col); colmap = batch column of each of the
    graph's own columns (None: the graph's own numbering)"""
    col = law["edge_col"] if colmap is None else np.asarray(colmap, np.int64)[law["edge_col"]].astype(np.int32)
    return {"rowptr": law["indptr"], "nbr": law["indices"], "nbr_rank": law["index_of"][law["indices"]], "nbr_f": law["indices"], "nbr_col": col}


def owned_columns(ei, lo, hi):
    """batch columns with both endpoints in [lo, hi), ascending: the graph's column map"""
    u, v = ei[0], ei[1]
    return np.flatnonzero((u >= lo) & (u < hi) & (v >= lo) & (v < hi)).astype(np.int64)


def takes_device_path(n, E, k, forced=True):
    """does preprocess_on_device take the graph (a device present and with room)?"""
    return n >= 1 and 1 <= E < (1 << 30) and k <= KMAX and (forced or E >= DEFAULT_MIN_COLS)


# ---- census ------------------------------------------------------------------------------------------------------------------------
def census(ei, n, k, law=None):
    """Counter of the paths of the five kernels that the input reaches (the classes tests/test_preproc_law.py lists)"""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    law = law or graph_law(ei, n, k)
    c = collections.Counter()
    E, nnz = ei.shape[1], len(law["indices"])
    u, v = ei[0], ei[1]
    keep = kept(ei, n)
    skipped = int(np.count_nonzero(~keep))
    # key width
    c["bits == %d" % key_bits(n)] += 1
    if n & (n - 1) == 0 and skipped:
        c["sentinel n at a power of two, n == %d" % n] += 1
    # skipped columns, by kind
    bad_u, bad_v = (u < 0) | (u >= n), (v < 0) | (v >= n)
    c["skip: u < 0"] += int(np.count_nonzero(u < 0))
    c["skip: v < 0"] += int(np.count_nonzero(v < 0))
    c["skip: u == n"] += int(np.count_nonzero(u == n))
    c["skip: v == n"] += int(np.count_nonzero(v == n))
    c["skip: u == 2^40"] += int(np.count_nonzero(u == 1 << 40))
    c["skip: low 32 bits in range"] += int(np.count_nonzero((bad_u & ((u & 0xFFFFFFFF) < n) & (u > 0) & ~bad_v) | (bad_v & ((v & 0xFFFFFFFF) < n) & (v > 0) & ~bad_u)))
    c["skip: one bad endpoint, source"] += int(np.count_nonzero(bad_u & ~bad_v))
    c["skip: one bad endpoint, target"] += int(np.count_nonzero(~bad_u & bad_v))
    if E >= 1 and nnz == 0:
        c["every column skipped"] += 1
    # launch edges: one thread per column / entry / row pointer word / root, blocks of BLOCK
    for name, val, at in (("E", E, (1, BLOCK - 1, BLOCK, BLOCK + 1)), ("nnz", nnz, (BLOCK - 2, BLOCK, BLOCK + 2)),
                          ("widen n + 1", n + 1, (BLOCK, BLOCK + 1)), ("roots n", n, (BLOCK, BLOCK + 1))):
        if val in at:
            c["%s == %d" % (name, val)] += 1
    if nnz in (BLOCK - 1, BLOCK + 1):
        c["nnz odd"] += 1                                        # cannot happen: two entries per kept column
    # row order
    pairs = collections.Counter(zip(u[keep].tolist(), v[keep].tolist()))
    c["column repeated both ways"] += sum(1 for (a, b), t in pairs.items() if a < b and t >= 5 and pairs.get((b, a), 0) >= 5)
    c["repeated self loop"] += sum(1 for (a, b), t in pairs.items() if a == b and t >= 2)
    deg = np.diff(law["indptr"])
    if nnz and n > 1:
        c["isolated vertex 0"] += int(deg[0] == 0)
        c["isolated vertex n - 1"] += int(deg[n - 1] == 0)
        c["run of equal indptr"] += int(np.count_nonzero((deg[:-1] == 0) & (deg[1:] == 0)) > 0)
    c["row of >= 3000 entries"] += int(np.count_nonzero(deg >= 3000))
    # roots
    indptr, indices, order, index_of, sdeg = law["indptr"], law["indices"], law["order"], law["index_of"], law["suffix_deg"]
    tag = "k == %d: " % k
    if k == 1:
        c["k == 1"] += 1
    if k <= 0:
        c["k <= 0"] += 1
    if k > KMAX:
        c["k > 32"] += 1
        c["k > 32: root reaches"] += int(np.count_nonzero(law["reach"]))
        c["k > 32: root does not reach"] += int(np.count_nonzero(~law["reach"]))
    if n < k:
        c["n < k"] += 1
    c["level %d" % law["level"]] += 1
    if 2 <= k <= KMAX and nnz <= 20000:
        for vi in np.flatnonzero(deg[order] > 0).tolist():
            r = int(order[vi])
            comp = len(reached(indptr, indices, index_of, r, vi, k, bound=k + 2))             # the suffix component, counted up to k + 2
            for d, nm in ((-1, "k - 1"), (0, "k"), (1, "k + 1")):
                if comp == k + d:
                    c[tag + "suffix component of " + nm] += 1
            if comp < k and sdeg[vi] > 0 and len(reached(indptr, indices, index_of, r, vi, k, suffix_only=False)) >= k:
                c[tag + "only the suffix filter keeps the root from reaching"] += 1
            if comp < k and any(_most_repeated(law, x, vi) > k for x in reached(indptr, indices, index_of, r, vi, k)):
                c[tag + "neighbour repeated more than k times, component below k"] += 1
            if r in indices[indptr[r]:indptr[r + 1]]:
                c[tag + "self loop at a root"] += 1
            if comp >= k:                                                                       # where did the list fill?
                got, mark = [r], {r}
                h = 0
                while len(got) < k:
                    x = got[h]
                    h += 1
                    for p in range(int(indptr[x]), int(indptr[x + 1])):
                        w = int(indices[p])
                        if index_of[w] >= vi and w not in mark:
                            mark.add(w)
                            got.append(w)
                            if len(got) == k:
                                if p < indptr[x + 1] - 1 and indptr[x + 1] - indptr[x] > k:
                                    c[tag + "list fills inside a row longer than k"] += 1
                                break
    return c


def _most_repeated(law, x, vi):
    """the largest number of entries of x's row that name one neighbour of rank >= vi"""
    row = law["indices"][law["indptr"][x]:law["indptr"][x + 1]]
    row = row[law["index_of"][row] >= vi]
    return int(np.bincount(row).max()) if len(row) else 0
