"""preproc_paths.py -- the inputs that pin the device preprocessing kernels (csrc/ugs_preproc.hip) path by path, shared by the CPU
tests (tests/test_preproc_law.py: law against the oracle, census, device model, mutants) and the GPU tests
(tests/test_gpu_preproc_paths.py).  Every case names in `reaches` the census classes (preproc_law.census) it is there for, each the
smallest input that reaches them; both test files assert the classes again, so an input that stops reaching its path fails
instead of losing coverage.

Case: one graph for create_preproc (ei, n, k).  Batch: the inputs of the plan assembly (pre_assemble and the split branch of
assemble_plan), graphs as (n, local columns) with the census classes of each graph worked out by `batch_census`."""
import collections
import functools
import random

import numpy as np

import preproc_law as L

Case = collections.namedtuple("Case", "name ei n k reaches")
TWO40, TRUNC3 = 1 << 40, (1 << 32) + 3


def arr(pairs):
    return np.ascontiguousarray(np.array(pairs, np.int64).reshape(-1, 2).T)


def random_cols(n, cols, seed, extra=()):
    """`cols` random columns over [0, n) (loops and repeats allowed) that touch vertex 0 and vertex n - 1, then `extra`, shuffled"""
    r = random.Random(seed)
    e = [(0, n - 1)] + [(r.randrange(n), r.randrange(n)) for _ in range(cols - 1)] + list(extra)
    r.shuffle(e)
    return arr(e)


def skipped_kinds(n):
    """one column of each skipped kind, each with its other endpoint in range, and one with both outside"""
    return [(-1, 0), (0, -1), (n, 0), (0, n), (TWO40, 0), (TRUNC3, 0), (0, TRUNC3), (-1, n)]


def roots_graph(k, seed):
    """components whose lowest-ranked vertex sees a suffix graph of exactly k - 1, k and k + 1 vertices (paths); a vertex with a
    repeated self loop and k - 1 leaves (the leaves rank below it: its component has k vertices, its suffix graph one, its suffix
    degree counts the loop's entries twice); a pair joined by k + 1 copies of one column and a lone vertex with k + 1 self loops
    (only the `seen` test keeps the list from filling); a star of k + 8 leaves (a leaf's search fills the list inside the hub's row).
    Vertex ids permuted, columns shuffled."""
    e, base = [], 0
    for s in (k - 1, k, k + 1):
        e += [(base + i, base + i + 1) for i in range(s - 1)]
        base += s
    e += [(base, base)] * 2 + [(base, base + 1 + i) for i in range(k - 1)]
    base += k
    e += [(base, base + 1)] * (k + 1)
    base += 2
    e += [(base, base)] * (k + 1)
    base += 1
    e += [(base + 1 + i, base) for i in range(k + 8)]
    base += k + 9
    r = random.Random(seed)
    perm = list(range(base))
    r.shuffle(perm)
    e = [(perm[u], perm[v]) for u, v in e]
    r.shuffle(e)
    return arr(e), base


ROOT_CLASSES = ("suffix component of k - 1", "suffix component of k", "suffix component of k + 1", "only the suffix filter keeps the root from reaching",
                "neighbour repeated more than k times, component below k", "self loop at a root", "list fills inside a row longer than k")


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, ei, n, k, *reaches):
        out.append(Case(name, np.ascontiguousarray(np.asarray(ei, np.int64).reshape(2, -1)), n, k, tuple(reaches)))

    # ---- key width: the sentinel key n at powers of two (one more bit than n - 1 needs), and the widths either side
    add("kw_n1", arr([(0, 0), (1, 0), (0, 0), (0, -1), (TWO40, 0)]), 1, 2, "bits == 1", "sentinel n at a power of two, n == 1", "n < k")
    add("kw_n2", arr([(2, 0), (0, 1), (0, 2), (1, 0), (-1, 1), (1, 1)]), 2, 2, "bits == 2", "sentinel n at a power of two, n == 2")
    add("kw_n256", random_cols(256, 300, 1, skipped_kinds(256)), 256, 3, "bits == 9", "sentinel n at a power of two, n == 256",
        "widen n + 1 == 257", "roots n == 256")
    add("kw_n65536", random_cols(65536, 300, 2, skipped_kinds(65536)), 65536, 3, "bits == 17", "sentinel n at a power of two, n == 65536")
    add("kw_n255", random_cols(255, 300, 3), 255, 3, "bits == 8", "widen n + 1 == 256")
    add("kw_n257", random_cols(257, 300, 4), 257, 3, "bits == 9", "roots n == 257")
    add("kw_n65535", random_cols(65535, 300, 5), 65535, 3, "bits == 16")
    add("kw_n65537", random_cols(65537, 300, 6), 65537, 3, "bits == 17")
    add("kw_n1048577", random_cols((1 << 20) + 1, 300, 7), (1 << 20) + 1, 3, "bits == 21")
    # ---- skipped columns, one of each kind among kept ones
    add("skip_kinds", random_cols(10, 12, 8, skipped_kinds(10)), 10, 3, "skip: u < 0", "skip: v < 0", "skip: u == n", "skip: v == n", "skip: u == 2^40",
        "skip: low 32 bits in range", "skip: one bad endpoint, source", "skip: one bad endpoint, target")
    add("all_skipped", arr([(-1, 0), (5, 1), (TWO40, 2), (3, TRUNC3)]), 5, 2, "every column skipped", "level 2")
    # ---- launch edges: one thread per column, per entry, per row pointer word, per root
    add("E_1", arr([(0, 1)]), 3, 2, "E == 1")
    for E in (255, 256, 257):
        add("E_%d" % E, random_cols(40, E, 10 + E), 40, 3, "E == %d" % E)
    for E in (127, 128, 129):
        add("nnz_%d" % (2 * E), random_cols(40, E, 20 + E), 40, 3, "nnz == %d" % (2 * E))
    # ---- row order
    add("repeated_both_ways", arr([(1, 2), (2, 1), (0, 1), (1, 2), (2, 1), (2, 3), (1, 2), (2, 1), (4, 1), (1, 2), (2, 1), (1, 2), (2, 1), (3, 4)]), 6, 3,
        "column repeated both ways")
    add("self_loops", arr([(3, 3), (0, 3), (3, 3), (1, 1), (3, 2), (3, 3), (1, 2), (1, 1)]), 5, 3, "repeated self loop", "k == 3: self loop at a root")
    add("isolated_ends", arr([(2, 3), (3, 4), (5, 2), (4, 5), (2, 4)]), 8, 3, "isolated vertex 0", "isolated vertex n - 1", "run of equal indptr")
    add("hub_3000", np.array([[0] * 3000, list(range(1, 3001))], np.int64), 3001, 5, "row of >= 3000 entries", "k == 5: list fills inside a row longer than k")
    # ---- roots
    for k in (2, 3, 32):
        ei, n = roots_graph(k, 30 + k)
        add("roots_k%d" % k, ei, n, k, *["k == %d: %s" % (k, c) for c in ROOT_CLASSES])
    add("k_1", arr([(0, 1), (1, 2), (3, 3), (2, 0)]), 5, 1, "k == 1")
    add("k_0", arr([(0, 1), (1, 2), (3, 3), (2, 0)]), 5, 0, "k <= 0")           # like k == 1 on both paths: every root reaches, every weight is 1
    # ---- relaxation levels
    add("n_lt_k", arr([(0, 1), (1, 2), (2, 0)]), 3, 5, "n < k", "level 1")
    add("loops_only", arr([(0, 0), (2, 2), (2, 2), (-1, 1)]), 4, 2, "level 1")
    # ---- k above the kernel's list: the host stages take the graph
    path = np.array([list(range(0, 999)), list(range(1, 1000))], np.int64)
    for k in (33, 40):
        add("path1000_k%d" % k, path, 1000, k, "k > 32", "k > 32: root reaches", "k > 32: root does not reach")
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def law_of(name):
    c = case(name)
    return L.graph_law(c.ei, c.n, c.k)


@functools.lru_cache(maxsize=None)
def census_of(name):
    c = case(name)
    return L.census(c.ei, c.n, c.k, law_of(name))


# ---- plan assembly -----------------------------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "name graphs shuffle cached k")     # graphs: (n, local columns); cached: indices the LRU holds from a host-path call
ASSEMBLY_K = 3


def er(n, p, seed):
    r = random.Random(seed)
    e = [(u, v) for u in range(n) for v in range(u + 1, n) if r.random() < p]
    return n, arr(e + [(v, u) for u, v in e] + [(0, 0), (1, 0), (1, 0)])


@functools.lru_cache(maxsize=None)
def batches():
    held = er(45, 0.2, 53)
    return (
        # unshuffled: graph 0's columns are the batch's first, in order (identity map, dropped); graph 4's are offset (non-identity)
        Batch("assembly_in_order", (er(30, 0.2, 51), held, (5, np.zeros((2, 0), np.int64)), (0, np.zeros((2, 0), np.int64)), er(300, 0.02, 52)), False, (1,), ASSEMBLY_K),
        # shuffled: every fresh graph has a non-identity map
        Batch("assembly_shuffled", (er(25, 0.3, 54), held, er(60, 0.1, 55)), True, (1,), ASSEMBLY_K),
    )


def batch(name):
    return next(b for b in batches() if b.name == name)


def batch_arrays(b):
    cols, ptr = [], [0]
    for n, ei in b.graphs:
        cols.append(np.asarray(ei, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1)
    if b.shuffle:
        ei = ei[:, np.random.default_rng(9).permutation(ei.shape[1])]
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


def local_graph(ei, ptr, g):
    """graph g as the general path slices it out of the batch: (n, its columns in batch order with local ids, its column map)"""
    cm = L.owned_columns(ei, ptr[g], ptr[g + 1])
    return int(ptr[g + 1] - ptr[g]), np.ascontiguousarray(ei[:, cm] - ptr[g]), cm


def batch_census(b):
    """per graph: the class of its piece in the plan the general path assembles with the device preprocessing forced"""
    ei, ptr = batch_arrays(b)
    out = []
    for g, (n, _) in enumerate(b.graphs):
        cm = L.owned_columns(ei, ptr[g], ptr[g + 1])
        if n <= 0 or n < b.k:
            out.append("degenerate graph")
        elif g in b.cached:
            out.append("host piece: graph held by the LRU")
        elif len(cm) == 0:
            out.append("host piece: graph without columns")
        elif np.array_equal(cm, np.arange(len(cm))):
            out.append("device piece: identity column map")
        else:
            out.append("device piece: non-identity column map")
    return out
