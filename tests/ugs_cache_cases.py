"""ugs_cache_cases.py -- the inputs of the ugs_sampler.GraphCache tests, shared by tests/test_ugs_cache_law.py (CPU: the law of every
case from the oracle alone, and its census class) and tests/test_gpu_ugs_cache.py.  No GPU and no product import here: only the
oracle, in batch_law.

A case is a small dataset -- graphs as (local columns [2, E], n) -- and one batch over it: `picks` names the dataset graph at every
batch position (a graph may be named twice), `first` is ptr[0].  `there_for` says which class of input the case is in the list
for, and `census` what the oracle's preprocessing must report for each PICKED graph: (degenerate, level, candidate bound), level
and bound None for a degenerate graph.  The tests assert the census again, so a case that stops being what it is there for fails."""
import collections
import functools
import random

import numpy as np

import ugs_workloads as wl

Case = collections.namedtuple("Case", "name there_for graphs picks first m k mode seed seeds census tier")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
NONE = np.zeros((2, 0), np.int64)
S_WALKS = ("ugs_walk_lds<8,32>", "ugs_walk_lds<16,32>", "ugs_walk_lds<8,64>", "ugs_walk_lds<16,64>")
LDS_WALKS = ("ugs_walk_lds<8,64>", "ugs_walk_lds<64,448>", "ugs_walk_lds<64,704>", "ugs_walk_lds<64,1024>", "ugs_walk_lds<64,1408>",
             "ugs_walk_lds<64,2048>")                                # by first tier 0 ... 5, for a batch whose bound exceeds 64
TIER_CAP = (64, 448, 704, 1024, 1408, 2048)


def arr(pairs):
    return np.ascontiguousarray(np.array(pairs, np.int64).reshape(-1, 2).T)


def both(pairs):
    return arr(list(pairs) + [(v, u) for u, v in pairs])


def dataset_index(position):
    """the index a dataset graph is added under: never its position in the list, never a batch position"""
    return 100 + 7 * position


def adding_order(count, seed):
    order = list(range(count))
    random.Random(seed).shuffle(order)
    if count > 1 and order == sorted(order):
        order.reverse()
    return order


DUMMY = (3, both([(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]), 4)      # (index, columns, n): added first, so that no base in the store is 0


def tu(n, e, seed):
    return wl.tu_graph(n, e, seed), n


def ring(n):
    return both([(v, (v + 1) % n) for v in range(n)]), n


def star(leaves):
    return both([(0, v) for v in range(1, leaves + 1)]), leaves + 1


def dense(n, p, seed, hubs=0):
    """test_gpu_ugs_graphs._dense_case's recipe for one graph, its columns kept together: G(n, p) plus a path, optionally `hubs`
    vertices joined to everything, both directions, three loops"""
    rng = random.Random(seed)
    e = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    e += [(v - 1, v) for v in range(1, n)]
    e += [(h, v) for h in range(hubs) for v in range(hubs, n)]
    e = e + [(v, u) for u, v in e]
    e += [(rng.randrange(n),) * 2 for _ in range(3)]
    return arr(e), n


def max_degree(cols, n):
    deg = np.bincount(cols[0], minlength=n) + np.bincount(cols[1], minlength=n) if n > 0 else np.zeros(1, np.int64)
    return int(deg.max()) if deg.size else 0


def bound_of(cols, n, k):
    """the candidate bound choose_tier works with: min(n - 1, (k - 1) * largest CSR degree)"""
    return max(0, min(n - 1, (k - 1) * max_degree(cols, n)))


def collate(case):
    """the batch B of the contract: the picked graphs' columns, graph by graph in batch order, each shifted by ptr[g]; and coff"""
    ptr, cols, coff = [case.first], [], [0]
    for p in case.picks:
        a, n = case.graphs[p]
        cols.append(a + ptr[-1])
        ptr.append(ptr[-1] + n)
        coff.append(coff[-1] + a.shape[1])
    ei = np.concatenate(cols, axis=1) if cols else NONE
    return np.ascontiguousarray(ei), np.array(ptr, np.int64), np.array(coff, np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, there_for, graphs, picks, m, k, mode="sample", seed=42, seeds=None, census=None, first=0, tier=None):
        assert census is not None and len(census) == len(picks)
        out.append(Case(name, there_for, tuple(graphs), tuple(picks), first, m, k, mode, seed, None if seeds is None else tuple(seeds),
                        tuple(census), tier))

    live = lambda g, k, level=0: (False, level, bound_of(g[0], g[1], k))    # noqa: E731
    gone = (True, None, None)

    r6 = ring(6)
    add("ring6_k3", "the smallest healthy graph", [r6], [0], 4, 3, census=[live(r6, 3)])
    p4 = (both([(0, 1), (1, 2), (2, 3)]), 4)
    add("n_eq_k", "n == k: every walk takes the whole graph", [p4, r6], [0, 1], 5, 4, "global", 7, census=[live(p4, 4), live(r6, 4)], first=5)
    a, b = tu(12, 16, 1), tu(9, 11, 2)
    small, nothing, no_cols = (both([(0, 1), (1, 2)]), 3), (NONE, 0), (NONE, 6)
    add("degenerate_between", "n < k, n == 0 and E == 0 graphs between healthy ones", [a, small, nothing, no_cols, b], [0, 1, 2, 3, 4], 3, 4, "graph", 11,
        census=[live(a, 4), gone, gone, live(no_cols, 4, 2), live(b, 4)])
    loops_only, empty5 = (arr([(0, 0), (2, 2), (2, 2)]), 4), (NONE, 5)
    alias = star(5)                                                      # weights 5 for the hub and 1 for ... : alias rows with prob < 1
    add("levels_k2", "preproc_paths' relaxation levels with their columns in range: loops only (level 1), no column kept (level 2), and a level 0 "
        "graph whose alias table has rows with prob < 1", [loops_only, empty5, alias], [0, 1, 2], 6, 2, "sample", 3,
        census=[live(loops_only, 2, 1), live(empty5, 2, 2), live(alias, 2)])
    tri = (arr([(0, 1), (1, 2), (2, 0)]), 3)
    c5 = tu(14, 20, 5)
    add("n_lt_k_k5", "preproc_paths' n_lt_k: a triangle at k = 5", [tri, c5], [0, 1], 4, 5, "global", -3, census=[gone, live(c5, 5)])
    multi = (arr([(0, 1), (1, 0), (0, 1), (1, 2), (2, 2), (2, 3), (3, 4), (4, 0), (2, 1), (4, 3)]), 5)
    add("repeated_columns", "duplicate and reversed columns and a loop: edge_src has several entries per undirected pair", [a, multi], [0, 1], 6, 3, "sample", 13,
        census=[live(a, 3), live(multi, 3)])
    add("same_graph_twice", "one dataset graph at two batch positions", [a, b], [0, 1, 0], 4, 4, "global", 21, census=[live(a, 4), live(b, 4), live(a, 4)], first=3)
    tus = [tu(8 + g % 9, 10 + g % 11, 30 + g) for g in range(33)]
    for mode in ("sample", "graph", "global"):
        add("g33_m3_" + mode, "G m = 99: no multiple of the fill's 32-row tiles or the walk's 8-row sums; mode " + mode, tus, list(range(33)), 3, 4, mode, 17,
            census=[live(g, 4) for g in tus])
    add("m1", "m == 1", tus[:5], [4, 2, 0], 1, 5, "sample", 9, census=[live(tus[g], 5) for g in (4, 2, 0)])
    add("seeds_zero_and_negative", "per-graph seeds with 0, negative values and the ends of the C int range", tus[:6], [5, 1, 3, 0, 2], 4, 4, "graph",
        seeds=[0, -1, -(2 ** 31), 2 ** 31 - 1, 42], census=[live(tus[g], 4) for g in (5, 1, 3, 0, 2)])
    s70 = star(70)
    add("star70_k3", "candidate bound 70 > 64: the batch leaves tier S's certain range", [s70, a], [1, 0], 5, 3, "sample", 5, census=[live(a, 3), live(s70, 3)])
    d70, d150 = dense(70, 0.15, 70), dense(150, 0.15, 150)
    add("dense70", "a dense graph of 70 vertices, under every first tier", [d70, b], [0, 1], 3, 6, "global", 42, seeds=[42, -7],
        census=[live(d70, 6), live(b, 6)], tier="every")
    add("dense150", "a dense graph of 150 vertices, under every first tier", [b, d150], [1, 0], 3, 8, "sample", 0, census=[live(d150, 8), live(b, 8)], tier="every")
    hubs = dense(2600, 0.0, 2600, hubs=3)
    add("three_hubs_2600", "candidate bound 2599 > 2048: rows reach the global-memory tier", [hubs], [0], 3, 4, "graph", 42, census=[live(hubs, 4)], tier="global")
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def batch_law(c):
    """the right-hand side of the contract: the oracle on the collated batch with a fresh LRU (per-graph seeds: its one-graph loop
    over the batch on one fresh LRU, the law of ugs_sampler.sample_graphs)"""
    import oracle
    import ugs_graphs_law
    ei, ptr, _ = collate(c)
    if c.seeds is None:
        return oracle.sample_batch(ei, ptr, c.m, c.k, c.mode, c.seed)
    cache = oracle.Cache()
    out = ugs_graphs_law.oracle_loop(ei, ptr, c.m, c.k, c.mode, c.seeds, cache)
    cache.close()
    return out


def rebased(blocks, ptr, coff, m, k, mode):
    """The concatenation of one-graph results -- each on the graph's own columns and ptr [0, n] -- as the batch's result: nodes and
    ("global") edge endpoints moved by ptr[g], edge_src by coff[g], edge_ptr by the entries ahead.  "sample" endpoints are row
    positions and "graph" endpoints i k + j with i the row inside its graph: neither moves."""
    G = len(blocks)
    nodes = [np.where(b[0] >= 0, b[0] + ptr[g], b[0]) for g, b in enumerate(blocks)]
    eidx = [b[1] + (ptr[g] if mode == "global" else 0) for g, b in enumerate(blocks)]
    esrc = [b[4] + coff[g] for g, b in enumerate(blocks)]
    eptr, base = [np.zeros(1, np.int64)], 0
    for b in blocks:
        eptr.append(b[2][1:] + base)
        base += int(b[2][-1])
    return (np.concatenate(nodes, axis=0) if G else np.zeros((0, k), np.int64), np.concatenate(eidx, axis=1) if G else NONE, np.concatenate(eptr),
            np.arange(G + 1, dtype=np.int64) * m, np.concatenate(esrc) if G else np.zeros(0, np.int64))
