"""fill_paths.py -- the inputs that pin the row-reading fill (fill_row in ugs_fill<8> / ugs_fill<64>) and the scan folded into it
(ugs_fill_scan<8>), shared by the CPU tests (tests/test_fill_law.py: law, census, device model, mutants) and the GPU tests
(tests/test_gpu_fill_paths.py).  Every case names the census classes (fill_law.census) it is there for, per lane width; the
generator seeds and call seeds were found by running the census over the oracle's rows for candidate seeds, and both test files
assert the classes again, so an input that stops reaching its path fails instead of losing coverage."""
import collections
import functools
import random

import numpy as np

import fill_law as L

Case = collections.namedtuple("Case", "name ei ptr m k seed reaches8 reaches64")


def mixed_graph(rnd, n, p, rev=0.3, rep=0.15, loops=0.1):
    """A connected multigraph as (n, columns): a random tree, every other pair with probability p in a random direction, then a
    share of reversed copies, of repeated columns and of self loops; columns shuffled.  Degrees come out odd and even."""
    cols = [(rnd.randrange(v), v) for v in range(1, n)]
    have = {frozenset(c) for c in cols}
    for u in range(n):
        for v in range(u + 1, n):
            if frozenset((u, v)) not in have and rnd.random() < p:
                cols.append((u, v) if rnd.random() < 0.5 else (v, u))
    extra = [(v, u) for u, v in cols if rnd.random() < rev]
    extra += [c for c in cols if rnd.random() < rep]
    extra += [(v, v) for v in range(n) if rnd.random() < loops]
    cols += extra
    rnd.shuffle(cols)
    return n, cols


def batch_of(graphs):
    cols, ptr = [], [0]
    for n, cs in graphs:
        cols += [(u + ptr[-1], v + ptr[-1]) for u, v in cs]
        ptr.append(ptr[-1] + n)
    return np.array(cols, np.int64).reshape(-1, 2).T.copy(), np.array(ptr, np.int64)


def small(gen_seed):
    """graphs of 3 .. 40 vertices: the 8-lane tier's own"""
    rnd = random.Random(gen_seed)
    return batch_of([mixed_graph(rnd, n, p) for n, p in ((3, 0.9), (6, 0.7), (12, 0.5), (24, 0.35), (40, 0.3), (33, 0.15))])


def mid(gen_seed):
    """degrees near 36: seven or eight adjacency rows flatten to about 256 entries, one chunk of the 64-lane form"""
    rnd = random.Random(gen_seed)
    return batch_of([mixed_graph(rnd, 52, 0.5, rev=0.15, rep=0.1), mixed_graph(rnd, 60, 0.45, rev=0.1, rep=0.1),
                     mixed_graph(rnd, 45, 0.6, rev=0.1, rep=0.1)])


def wide(gen_seed):
    rnd = random.Random(gen_seed)
    return batch_of([mixed_graph(rnd, 70, 0.5), mixed_graph(rnd, 40, 1.0, rev=0.1, rep=0.05, loops=0.05), mixed_graph(rnd, 120, 0.25)])


def clique(k, copies=1):
    """K_k, every pair once as a column (u < v), `copies` times"""
    return k, [(u, v) for u in range(k) for v in range(u + 1, k)] * copies


def exactly(k, columns, gen_seed):
    """A connected multigraph on exactly k vertices with `columns` columns: every complete row holds all of them, 2 * columns hits."""
    rnd = random.Random(gen_seed)
    cols = [(rnd.randrange(v), v) for v in range(1, k)]
    pairs = [(u, v) for u in range(k) for v in range(u + 1, k) if (u, v) not in cols]
    rnd.shuffle(pairs)
    cols += pairs[:columns - len(cols)]
    while len(cols) < columns:
        cols.append(rnd.choice(cols)[::-1])
    rnd.shuffle(cols)
    return k, cols


def clique_batch(k, graphs, repeated=0):
    """`graphs` complete graphs on exactly k vertices with both directions of every pair as columns: every row is complete and
    holds 2 k (k - 1) entries, the packed step's bound exactly; `repeated` columns of the first graph once more put it above."""
    n, cols = clique(k)
    both = cols + [(v, u) for u, v in cols]
    return batch_of([(n, both + both[:repeated])] + [(n, both)] * (graphs - 1))


# name: (batch, m, k, call seed, classes at 8 lanes, classes at 64 lanes)
T_ALL = tuple(L.T_CLASSES)
_SPEC = {
    "small_k16": (lambda: small(0), 8, 16, 2,
                  ("k > 8", ">= 3 chunks", "sub-chunk without a hit", "full sub-chunk of hits", "incomplete row")
                  + tuple(f"k > 8, {c}" for c in T_ALL),
                  ("k > 8", "1 chunk", "2 chunks", "sub-chunk without a hit", "incomplete row", "k > 8, T odd", "k > 8, T % GS == GS - 1",
                   "k > 8, T % GS == 0", "k > 8, T % GS == 1", "k > 8, T % 4GS == 4GS - 1")),
    "small_k3": (lambda: small(1), 8, 3, 0,
                 ("k <= 8", "1 chunk", "2 chunks") + tuple(f"k <= 8, {c}" for c in T_ALL),
                 ("k <= 8", "k <= 8, T odd", "k <= 8, T % GS == GS - 1", "k <= 8, T % GS == 0", "k <= 8, T % GS == 1")),
    "small_k1": (lambda: small(1), 8, 1, 3, ("complete row without a hit", "hitless row between rows with hits", "k <= 8"),
                 ("complete row without a hit", "hitless row between rows with hits", "k <= 8")),
    # graphs of fewer than k vertices between larger ones: incomplete rows between rows with hits
    "gaps_k9": (lambda: batch_of([mixed_graph(random.Random(5), n, 0.5) for n in (12, 4, 15, 8, 20)]), 5, 9, 2,
                ("incomplete row between rows with hits", "k > 8"), ("incomplete row between rows with hits", "k > 8")),
    "small_k32": (lambda: small(0), 8, 32, 0, ("k > 8", ">= 3 chunks", "incomplete row"), ("k > 8", "full sub-chunk of hits")),
    "small_k2": (lambda: small(2), 8, 2, 1, ("k <= 8", "1 chunk"), ("k <= 8", "1 chunk")),
    "small_k8": (lambda: small(2), 8, 8, 3, ("k <= 8", ">= 3 chunks", "incomplete row"), ("k <= 8", "1 chunk")),
    "small_k9": (lambda: small(2), 8, 9, 4, ("k > 8", ">= 3 chunks", "incomplete row"), ("k > 8", "1 chunk")),
    "mid_k7": (lambda: mid(0), 16, 7, 0, ("k <= 8", ">= 3 chunks"),
               ("k <= 8", "1 chunk", "2 chunks", "k <= 8, T % 4GS == 4GS - 1", "k <= 8, T % 4GS == 0", "k <= 8, T % 4GS == 1")),
    "wide_k16": (lambda: wide(4), 16, 16, 5, ("k > 8", ">= 3 chunks"),
                 ("k > 8", ">= 3 chunks", "k > 8, T % 4GS == 0", "k > 8, T % 4GS == 1")),
    # K8 on exactly 8 vertices, every column three times: 168 entries, all hits -- two full ballots of 64 lanes
    "k8_cliques": (lambda: batch_of([clique(8, 3)] * 2), 8, 8, 7, ("k <= 8", "full sub-chunk of hits", "k <= 8, T % GS == 0"),
                   ("k <= 8", "full sub-chunk of hits", "1 chunk")),
    # rows of exactly 64 and 66 hits (65 cannot occur, fill_law.IMPOSSIBLE): graphs of exactly k vertices with 32 and 33 columns
    "hits_k9": (lambda: batch_of([exactly(9, 32, 1), exactly(9, 33, 2)]), 6, 9, 5, ("hits == 64", "hits == 66", "k > 8"),
                ("hits == 64", "hits == 66", "k > 8")),
    "hits_k8": (lambda: batch_of([exactly(8, 32, 3), exactly(8, 33, 4)]), 6, 8, 6, ("hits == 64", "hits == 66", "k <= 8"),
                ("hits == 64", "hits == 66", "k <= 8")),
}
CASE_NAMES = tuple(_SPEC)
PERMUTE_SEED = 20261


@functools.lru_cache(maxsize=None)
def case(name):
    gen, m, k, seed, r8, r64 = _SPEC[name]
    ei, ptr = gen()
    ei.setflags(write=False), ptr.setflags(write=False)
    return Case(name, ei, ptr, m, k, seed, tuple(r8), tuple(r64))


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def oracle_of(name, mode):
    """oracle.sample_batch of the case: computed once, shared, read-only"""
    import oracle
    c = case(name)
    return frozen([np.ascontiguousarray(a, dtype=np.int64) for a in oracle.sample_batch(c.ei, c.ptr, c.m, c.k, mode, c.seed)])


@functools.lru_cache(maxsize=None)
def adjacency_of(name):
    c = case(name)
    return L.adjacency(c.ei, c.ptr)


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """(oracle rows, permuted rows): the oracle's rows of all G m walks and a copy of them with the vertices of every complete row
    permuted by a fixed seed -- rows no walk produces (the fill's contract is a connected subset of one graph, in any order).
    Row r of the copy keeps its place, so that `row / m` still names its graph."""
    c = case(name)
    nodes = oracle_of(name, "global")[0]
    rnd = random.Random(PERMUTE_SEED)
    perm = nodes.copy()
    for row in perm:
        if (row >= 0).all():
            vs = row.tolist()
            rnd.shuffle(vs)
            row[:] = vs
    return frozen([nodes, perm])


@functools.lru_cache(maxsize=None)
def census_of(name, GS, permuted=False):
    c = case(name)
    return L.census(c.ei, c.ptr, rows_of(name)[1 if permuted else 0], c.k, GS, adj=adjacency_of(name))


@functools.lru_cache(maxsize=None)
def law_of(name, mode, permuted=False, row_begin=0, row_count=None, extra=0):
    """fill_law.edge_phase of rows [row_begin, row_begin + row_count) of the case's oracle (or permuted) rows"""
    c = case(name)
    nodes = rows_of(name)[1 if permuted else 0]
    row_count = len(nodes) - row_begin if row_count is None else row_count
    part = nodes[row_begin:row_begin + row_count]
    part = np.where(part >= 0, part + extra, part)
    return frozen(list(L.edge_phase(c.ei, c.ptr, part, c.m, c.k, mode, row_begin, extra, adj=adjacency_of(name))))


def one_graph():
    """a batch of one graph: the kernels' num_graphs == 1 shortcut"""
    return batch_of([mixed_graph(random.Random(9), 30, 0.3)])


# ---- the packed step at its bound ----------------------------------------------------------------------------------------------
PACKED = {"at_bound": (5, 4, 8, 0), "above_bound": (5, 4, 8, 1)}    # name: (k, graphs, m, repeated columns)


def packed_batch(name):
    k, G, m, rep = PACKED[name]
    ei, ptr = clique_batch(k, G, rep)
    return ei, ptr, m, k


# ---- row counts of the fused step ---------------------------------------------------------------------------------------------
FUSED_K, FUSED_GRAPHS, FUSED_M = 3, 32, 4100         # 131 200 rows of a tu_batch(18, 20, 32)-shaped batch


def fused_row_counts(cus):
    """Row counts of Plan.step that put the scan folded into the fill on each of its paths, for a device of `cus` CUs.  The trip of
    the `before` loop is 2048 tiles whatever the device; the tile loop's stride is the grid, 8 blocks per CU -- at the MI355X's
    256 CUs both edges fall on 65 536 rows."""
    small = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 42, 43, 44, 45, 46, 52, 60]    # every residue mod 8; 8-row sums = 1, 2, 3 mod 4
    trip = L.TRIP_TILES * L.TILE_ROWS
    stride = L.GRID_PER_CU * cus * L.TILE_ROWS
    edges = {trip, trip + 1, trip + L.TILE_ROWS + 1, L.FUSED_MAX_ROWS, L.FUSED_MAX_ROWS + 1}
    if stride < L.FUSED_MAX_ROWS:
        edges |= {stride, stride + 1, stride + L.TILE_ROWS + 1}
    return small + sorted(edges)


@functools.lru_cache(maxsize=None)
def fused_batch():
    import ugs_workloads as wl
    ei, ptr = wl.tu_batch(18, 20, FUSED_GRAPHS)
    return frozen([np.ascontiguousarray(ei, dtype=np.int64), np.ascontiguousarray(ptr, dtype=np.int64)])


@functools.lru_cache(maxsize=None)
def fused_reference(mode, seed):
    """(nodes, edge_ptr, edge_index, edge_src) of ALL 131 200 rows: the oracle's rows and the law's edge outputs of them (numpy
    form), computed once per (mode, seed) and shared.  A row range's outputs are slices: none of the three reference modes
    depends on where a call begins."""
    import oracle
    ei, ptr = fused_batch()
    nodes = np.ascontiguousarray(oracle.sample_batch(ei, ptr, FUSED_M, FUSED_K, "global", seed)[0], dtype=np.int64)
    eptr, eidx, esrc = L.edge_phase_np(ei, ptr, nodes, FUSED_M, FUSED_K, mode)
    return frozen([nodes, eptr, eidx, esrc])


def fused_slice(mode, seed, row_begin, row_count):
    nodes, eptr, eidx, esrc = fused_reference(mode, seed)
    lo, hi = int(eptr[row_begin]), int(eptr[row_begin + row_count])
    return nodes[row_begin:row_begin + row_count], eptr[row_begin:row_begin + row_count + 1] - lo, eidx[:, lo:hi], esrc[lo:hi]


# ---- capacities below the total ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capacities(name, GS):
    """{what: ld} for the case's oracle rows: the total, one below it, a value that cuts a row in two, one that cuts between two
    hits of ONE sub-chunk's ballot (fill_row<GS>), and 1."""
    c = case(name)
    nodes = rows_of(name)[0]
    eptr = law_of(name, "sample")[0]
    total = int(eptr[-1])
    out = {"total": total, "total - 1": total - 1, "1": 1}
    for r, row in enumerate(nodes):
        n = int(eptr[r + 1] - eptr[r])
        if n >= 2 and "inside a row" not in out and r > 0 and eptr[r] > 0:
            out["inside a row"] = int(eptr[r]) + n // 2
        if n >= 2 and "inside a ballot" not in out:
            hit = [l is not None for _, _, _, l in L.row_entries(adjacency_of(name), row)]
            seen = 0
            for s in range(0, len(hit), GS):
                h = sum(hit[s:s + GS])
                if h >= 2 and int(eptr[r]) + seen + 1 > 1:
                    out["inside a ballot"] = int(eptr[r]) + seen + 1
                    break
                seen += h
    return out
