"""rwr_paths.py -- the inputs that pin rwr_sampler's kernel paths, shared by the CPU tests (tests/test_rwr_law.py: census, device
model, mutants) and the GPU tests (tests/test_gpu_rwr_paths.py).  Every case names in `reaches` the census classes
(rwr_law.census) it is there for; the seeds were found by running the census over candidate seeds, and both test files assert the
classes again, so an input that stops reaching its path fails instead of losing coverage."""
import collections
import functools
import random

import numpy as np

import rwr_law as R
import ugs_workloads as wl

Case = collections.namedtuple("Case", "name ei ptr m k seed p seeds reaches")


def batch_of(graphs, first=0, extra=()):
    """(ei, ptr) of graphs given as (n, columns local to the graph); `extra` columns are appended as they are (batch ids)."""
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(np.asarray(ei, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    if len(extra):
        cols.append(np.asarray(extra, np.int64).reshape(-1, 2).T)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


def path_plus(n, columns, seed):
    """A path over n vertices, one column per edge, plus random one-directional columns (loops and duplicates allowed) up to
    `columns` columns: n + 1 + 2 * columns + (n + 3) // 4 CSR words."""
    rnd = random.Random(seed)
    und = [(i, i + 1) for i in range(n - 1)]
    und += [(rnd.randrange(n), rnd.randrange(n)) for _ in range(columns - len(und))]
    return n, np.array(und, np.int64).T


def pairs_and_loop(pairs):
    """`pairs` two-vertex components and one vertex with a loop: every seed has edges and is doomed for k >= 3."""
    und = [(2 * i, 2 * i + 1) for i in range(pairs)] + [(2 * pairs, 2 * pairs)]
    return 2 * pairs + 1, np.array(und, np.int64).T


def paths_and_isolated(k, isolated, seed):
    """A path of k - 1 vertices (doomed), a path of k vertices (live) and isolated vertices, columns shuffled, both directions."""
    und = [(i, i + 1) for i in range(k - 2)] + [(k - 1 + i, k + i) for i in range(k - 1)]
    und += [(v, u) for u, v in und]
    random.Random(seed).shuffle(und)
    return 2 * k - 1 + isolated, np.array(und, np.int64).reshape(-1, 2).T


def tu(n, e, seed):
    return n, wl.tu_graph(n, e, seed)


def first_seed_landing_on(n, vertex, g=0):
    """The smallest batch seed whose graph g seeds its first walk at `vertex`."""
    return next(s for s in range(1 << 20) if R.draw((s + g) & R.M64, 1) % n == vertex)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, batch, m, k, seed, p, reaches, seeds=None):
        out.append(Case(name, batch[0], batch[1], m, k, seed, p, seeds, tuple(reaches)))

    # CSR placement: A fills csr[] to the last word, B is one word over; neither is first in the batch
    A, B = path_plus(2002, 2844, 1), path_plus(2003, 2844, 2)
    placed = batch_of([tu(12, 14, 1), A, B, tu(12, 14, 2)], first=3)
    classes = ["csr_words == 8192", "csr_words == 8193", "lds, vbase > 0", "global, vbase > 0", "spec == 2"]
    add("placement", placed, 20, 6, 5, 0.2, classes)
    add("placement_graph_seeds", placed, 20, 6, 0, 0.2, classes, seeds=(11, (1 << 64) - 1, 1 << 63, 7))
    # B followed by a graph whose vertex 3 is doomed, B's first walk seeded at its last vertex (the LDS bound's mutant reads there)
    tail = (12, np.concatenate([np.array([[0, 1], [1, 2]], np.int64), wl.tu_graph(8, 9, 3) + 4], axis=1))
    add("placement_last_vertex", batch_of([B, tail]), 20, 6, first_seed_landing_on(2003, 2002), 0.2, ["csr_words == 8193", "global"])
    # speculation cap and window edges (m = 24: W = 512; m = 16: W = 256)
    for s, m, reaches in CAP_CASES:
        add(f"cap_s{s}_m{m}", batch_of([tu(30, 29, s)]), m, 8, s, 0.5, reaches)
    # k = 1: every walk is its seed draw, the chain lands on base + W at every slide
    nine = batch_of([tu(9, 10, 4)])
    for p in (0.2, 0.0, 1.0):
        add(f"k1_p{p}", nine, 2100, 1, 6, p, ["spec == 4", "offset W - 1", "lands on base + W", "slides"])
    # p = 1 on a live graph: every walk restarts T times and fails, through the cap and lane 0's redo; p = 0: never restarts
    add("p1_live", batch_of([tu(6, 7, 2)]), 20, 4, 9, 1.0, ["live_failed", "capped", "L > 66"])
    add("p0_live", batch_of([tu(12, 14, 5)]), 10, 5, 2, 0.0, ["L < 64"])
    # the doomed closed form: T = 4550 puts the T-th step next to the first round's end at p = 0.2
    doom = batch_of([pairs_and_loop(45)])
    for seed, reaches in DOOM_SEEDS:
        add(f"doomed91_s{seed}", doom, 48, 5, seed, 0.2, reaches)
    add("doomed91_p0", doom, 48, 5, 3, 0.0, ["round 1"])
    add("doomed91_p1", doom, 48, 5, 3, 1.0, ["round 0"])
    add("doomed199_round2", batch_of([pairs_and_loop(99)]), 10, 5, 3, 0.2, ["round >= 2"])
    # 18 live vertices and one pair, k = 5: a doomed walk now and then between live ones, met on the window's last offset
    mixed = batch_of([(20, np.concatenate([wl.tu_graph(18, 20, 1), np.array([[18], [19]], np.int64)], axis=1))])
    for seed, reaches in MIXED_SEEDS:
        add(f"mixed20_s{seed}", mixed, 16, 5, seed, 0.2, reaches)
    # KM dispatch: n == k (T = 10 k^2), n == k - 1 (no draws) between two live graphs, one larger
    for k in (8, 9, 16, 17, 32, 33, 64):
        km = min(w for w in R.KM_WIDTHS if k <= w)
        batch = batch_of([tu(k, 4 * k, k), tu(k - 1, 4 * k, k + 1), tu(k + 7, 4 * k + 28, k + 2)], first=2)
        add(f"km_k{k}", batch, 3, k, k, 0.1, [f"KM == {km}", "T0"] + (["k == KM"] if k == km else []))
    # union-find threshold: components of exactly k - 1 and k vertices
    for k in (9, 64):
        add(f"components_k{k}", batch_of([paths_and_isolated(k, 3, k)]), UF_SEEDS[k][0], k, UF_SEEDS[k][1], 0.0,
            ["component == k - 1", "component == k", "doomed_isolated"] + (["round >= 2", "last_in_lane"] if k == 64 else []))
    # sort width: NV an exact power of two, with columns that cross graphs or leave the batch (their key is NV)
    odd = lambda lo, hi: [(lo, hi - 1), (hi, lo), (hi + 5, hi + 6), (-1, lo)]
    add("nv1", batch_of([(1, [[0], [0]])], first=4, extra=[(4, 5), (3, 4)]), 5, 1, 1, 0.2, ["dropped columns, NV a power of two"])
    add("nv2", batch_of([(1, [[0], [0]]), (1, [[], []])], extra=[(0, 1), (1, 0), (2, 2)]), 5, 1, 1, 0.2, ["dropped columns, NV a power of two"])
    add("nv256", batch_of([tu(16, 20, g) for g in range(16)], first=7, extra=odd(7, 263) + [(22, 23), (23, 22)]), 5, 4, 3, 0.2,
        ["dropped columns, NV a power of two"])
    add("nv4096", batch_of([tu(64, 80, g) for g in range(64)], extra=odd(0, 4096) + [(63, 64)]), 2, 5, 4, 0.2,
        ["dropped columns, NV a power of two"])
    add("all_dropped", batch_of([(4, [[], []]), (4, [[], []])], first=1, extra=[(1, 5), (8, 2), (9, 9), (0, 1)]), 3, 2, 8, 0.2,
        ["every column dropped", "dropped columns, NV a power of two", "doomed_isolated"])
    # rows of one graph on both sides of a block edge of rwr_rows / rwr_fill: 40 graphs x 7 rows
    add("rows_across_blocks", wl.tu_batch(10, 12, 40, dataset_seed=3), 7, 4, 12, 0.2, ["L < 64"])
    return tuple(out)


# (tu_graph seed = call seed, m, classes): found by the census over seeds 0 .. 99
CAP_CASES = (
    (8, 24, ("L == 64", "capped", "window with capped and uncapped walks", "L > 66", "L > W", "spec == 2")),
    (15, 24, ("L in (65, 66)", "capped")),
    (24, 24, ("L in (65, 66)", "L == 65 uncapped")),
    (22, 24, ("offset W - 1",)),
    (38, 24, ("lands on base + W",)),
    (10, 16, ("lands on base + W", "spec == 1", "L > W")),
)
# call seeds of the 91-vertex doomed graph (found over seeds 0 .. 11) and where the T-th step of some walk falls there
DOOM_SEEDS = (
    (3, ("lane == 255 and j == 31, bit 0", "lane == 255 and j == 31, bit 1", "lane == 0 and j == 0 and round > 0", "j == 31, bit 0",
         "j == 31, bit 1", "j == 0", "last_in_lane", "round 0", "round 1", "doomed_row0", "doomed_row_last", "doomed_twice", "spec == 3")),
    (1, ("lane == 255 and j == 31, bit 1", "lane == 0 and j == 0 and round > 0")),
    (7, ("j == 31, bit 0", "lane == 255 and j == 31, bit 1", "last_in_lane")),
)
# call seeds of the 20-vertex graph, found over seeds 0 .. 1999
MIXED_SEEDS = (
    (1451, ("doomed at offset W - 1", "doomed_row_last", "doomed_twice")),
    (1567, ("doomed at offset W - 1", "doomed_row0", "L == 65 uncapped")),
)
UF_SEEDS = {9: (8, 1), 64: (5, 8)}                                 # k: (m, call seed); k = 64 with two doomed walks only (T = 83200)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def census_starts_of(name):
    c = case(name)
    return R.census_starts(c.ei, c.ptr, c.m, c.k, c.seed, c.p, c.seeds)


def census_of(name):
    return census_starts_of(name)[0]


def graph_seed(c, g):
    return (c.seed + g) & R.M64 if c.seeds is None else int(c.seeds[g]) & R.M64


@functools.lru_cache(maxsize=None)
def sequential_of(name):
    """Per graph with n >= k: rwr_law.sequential_starts for m + 1 walks (the last entry: the draws the m walks consumed)."""
    c = case(name)
    adjs = R.adjacency(c.ei[0], c.ei[1], c.ptr)
    return [R.sequential_starts(adj, c.k, c.p, graph_seed(c, g), c.m + 1)[:c.m + 1] if len(adj) >= c.k else None
            for g, adj in enumerate(adjs)]


@functools.lru_cache(maxsize=None)
def law_of(name, mode):
    """rwr_law.sample_batch of the case: computed once, shared, never modified (the arrays are read-only)."""
    c = case(name)
    out = R.sample_batch(c.ei, c.ptr, c.m, c.k, mode, c.seed, c.p, c.seeds)
    for a in out:
        a.setflags(write=False)
    return out
