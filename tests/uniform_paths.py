"""uniform_paths.py -- the inputs that pin the mask-form kernel paths of uniform_sampler (ugs_uniform.hip), shared by the CPU tests
(tests/test_uniform_paths_law.py: census, device model, mutants) and the GPU tests (tests/test_gpu_uniform_paths.py).  Every case
names in `reaches` the census classes (uniform_law.census) it is there for, and both test files assert them again, so an input that
stops reaching its path fails instead of losing coverage.

`what` says which entry the case goes through: "batch" (sample_batch, one generator), "graphs" (sample_graphs, a seed per graph),
"enumerate" (enumerate_graphs: every key's position) or "count" (count_graphs).  Search and sort paths use the last two, draws, rows
and fill the first two."""
import collections
import functools
import math
import random

import numpy as np

import uniform_enum_law as EL
import uniform_law as U

Case = collections.namedtuple("Case", "name what ei ptr m k seed seeds modes counts reaches")
M64 = U.M64


def und(pairs):
    """Both directions of every pair, as columns."""
    p = np.array(list(pairs), np.int64).reshape(-1, 2)
    return np.concatenate([p, p[:, ::-1]]).T


def one_way(pairs):
    return np.array(list(pairs), np.int64).reshape(-1, 2).T


def batch_of(graphs, first=0, extra=(), shuffle=None):
    """(ei, ptr) of graphs given as (n, columns local to the graph); `extra` columns are appended as they are (batch ids);
    `shuffle`: the seed of a permutation of all columns."""
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(np.asarray(ei, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    if len(extra):
        cols.append(np.asarray(extra, np.int64).reshape(-1, 2).T)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    if shuffle is not None:
        ei = ei[:, np.array(random.Random(shuffle).sample(range(ei.shape[1]), ei.shape[1]), np.int64)]
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


def path(order):
    return [(a, b) for a, b in zip(order, order[1:])]


def complete(n):
    return [(u, v) for u in range(n) for v in range(u + 1, n)]


def stars(extra=()):
    """Vertex 0 joined to the leaves 1..37, 38 to 1..10, 39 to 11 and 12, 40 to 13: at k = 4 the bucket of root 0 holds exactly
    8192 sets (41 vertices, 8312 sets); with (41, 40) added, 8193 (42 vertices, 8313 sets)."""
    return ([(0, i) for i in range(1, 38)] + [(38, i) for i in range(1, 11)] + [(39, 11), (39, 12), (40, 13)] + list(extra))


G8192 = (41, one_way(stars()))
G8193 = (42, one_way(stars([(41, 40)])))
# roots with buckets of 1 key (vertex 4: {4, 5, 6, 7}), of 3 and 5 keys (no power of two), of 2 and of 0, at k = 4
SMALL_ROOTS = (8, und(path([0, 1, 2, 3]) + [(1, 4)] + path([4, 5, 6, 7])))
EMPTY = (0, np.zeros((2, 0), np.int64))


def draw_graph(g):
    """Graph g of the draw batches: every third one two vertices without an edge (no set at k = 2); the others K_7 (21 sets) and K_6
    (15 sets), so that a wrong generator word shows in the draw, but every twelfth a single edge (one set)."""
    if g % 3 == 2:
        return 2, np.zeros((2, 0), np.int64)
    if g % 12 == 1:
        return 2, one_way([(1, 0)])
    return (7, one_way(complete(7))) if g % 3 == 0 else (6, und(complete(6)))


def draw_batch(G):
    return batch_of([draw_graph(g) for g in range(G)])


def natural_path_63():
    """0 - 1 - ... - 63 with 63 also joined to 10 and carrying a loop: vertex 63 is a root, a first extension (of 10 and of 62)
    and an endpoint of the rows' edges."""
    return 64, np.concatenate([und(path(range(64)) + [(10, 63)]), one_way([(63, 63)])], axis=1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, what, batch, k, reaches, m=0, seed=0, seeds=None, modes=("sample",), counts=None):
        out.append(Case(name, what, batch[0], batch[1], m, k, seed, seeds, tuple(modes), counts, tuple(reaches)))

    # ---- columns: strays of every kind, empty graphs first / between / last, ptr[0] = 3, a loop, a duplicate, columns in any order
    ring = (6, np.concatenate([und(path([0, 1, 2, 3, 4, 5, 0])), one_way([(0, 0), (2, 3), (2, 3)])], axis=1))
    mixed = [EMPTY, ring, EMPTY, (5, und(path(range(5)))), (2, und([(0, 1)])), EMPTY]
    strays = [(4, 10), (1, 4), (16, 17), (5, 16), (-1, 4), (9, -2)]
    columns = batch_of(mixed, first=3, extra=strays, shuffle=1)
    col_classes = ["stray_cross", "stray_below", "stray_above", "stray_negative", "empty_graph_first", "empty_graph_middle",
                   "empty_graph_last", "ptr0_nonzero", "loop_column", "duplicate_column", "columns_shuffled", "k3", "graph_n_lt_k"]
    add("columns_enum", "enumerate", columns, 3, col_classes + ["loop_in_subset", "items_le_16384"], modes=("sample", "global"))
    add("columns_batch", "batch", columns, 3, col_classes + ["empties_between", "G_le_320", "sample", "global"], m=5, seed=7,
        modes=("sample", "global"))
    # ---- the column sort's bit count: G a power of two and stray columns (key G), before, between and after the graphs' columns
    tri = (3, und(path([0, 1, 2, 0])))          # root buckets of 2, 1 and 0 keys at k = 2
    for G in (1, 2, 4, 256):
        last = 3 * G
        extra = [(last, 0), (0, last), (1, last + 5), (-3, 1)] + ([(2, 3), (3 * G - 1, 0), (4, 1)] if G > 1 else [])
        ei, ptr = batch_of([tri] * G, extra=extra)
        ei = np.concatenate([ei[:, -3:], ei[:, :-3]], axis=1)        # strays in front too
        add(f"G{G}_stray", "enumerate", (np.ascontiguousarray(ei), ptr), 2, ["G_pow2_with_stray", "k2", "bucket_2", "bucket_1", "bucket_0"],
            modes=("global",))
    # ---- search
    loops = (5, np.concatenate([und(path([0, 1, 2])), one_way([(3, 3), (1, 1)])], axis=1))
    add("k1_loops", "enumerate", batch_of([loops, (1, np.zeros((2, 0), np.int64))]), 1, ["k1", "row_without_edges", "loop_in_subset", "bucket_1"],
        modes=("sample", "global"))
    add("k1_batch", "batch", batch_of([loops, (1, np.zeros((2, 0), np.int64))]), 1, ["k1", "size_1", "seed_all_ones"], m=9, seed=M64)
    k12 = batch_of([(12, one_way(complete(12)))])
    add("K12_k8", "enumerate", k12, 8, ["k8", "bucket_np2", "bucket_pow2"], modes=("sample",))
    add("K12_k9", "enumerate", k12, 9, ["k9", "bucket_np2"], modes=("global",))
    add("K12_k9_batch", "batch", k12, 9, ["k9"], m=7, seed=3)
    inner = list(range(32)) + [63] + list(range(32, 63))             # 63 an interior vertex
    tail = [62, 63] + list(range(62))                                # 63 the only extension of root 62
    add("path64_k64", "enumerate", batch_of([(64, und(path(inner)))], first=2), 64, ["k_eq_n_64", "k_ge_33", "root_63", "w0_63", "edge_at_vertex_63"])
    add("path64_k33", "enumerate", batch_of([(64, und(path(tail)))]), 33, ["k_ge_33", "root_63", "w0_63", "bucket_1"], modes=("global",))
    add("path64_k33_batch", "batch", batch_of([(64, und(path(inner)))]), 33, ["k_ge_33", "edge_at_vertex_63"], m=6, seed=11)
    v63 = batch_of([natural_path_63()])
    add("v63_k3", "enumerate", v63, 3, ["root_63", "w0_63", "edge_at_vertex_63", "loop_in_subset", "k3"], modes=("sample", "global"))
    add("v63_k2_batch", "batch", v63, 2, ["root_63", "w0_63", "edge_at_vertex_63", "k2"], m=200, seed=5, modes=("sample",))
    add("K30_k6_count", "count", batch_of([(30, one_way(complete(30))), (5, und(path(range(5))))]), 6, ["item_ge_4096", "graph_n_lt_k"],
        counts=(math.comb(30, 6), 0))
    add("K18_k6", "enumerate", batch_of([(18, one_way(complete(18)))]), 6, ["rows_cross_256", "bucket_np2"], modes=("sample",))
    # ---- the two sort routes at their boundary: alone, and as neighbours with small buckets in the same call
    sort_reach = ["bucket_0", "bucket_1", "bucket_np2"]
    add("sort_8192", "enumerate", batch_of([G8192]), 4, sort_reach + ["bucket_8192"], modes=("global",))
    add("sort_8193", "enumerate", batch_of([G8193]), 4, sort_reach + ["bucket_8193"], modes=("global",))
    add("sort_pair", "enumerate", batch_of([G8192, G8193, SMALL_ROOTS], first=1), 4,
        sort_reach + ["bucket_8192", "bucket_8193", "small_and_large_in_one_call"], modes=("sample",))
    add("sort_pair_batch", "batch", batch_of([SMALL_ROOTS, G8193, G8192]), 4, ["small_and_large_in_one_call"], m=50, seed=2, modes=("global",))
    # ---- draws from one generator: the compaction over blocks of 320 graphs and the generator's blocks of 312 outputs
    add("draw_312", "batch", draw_batch(468), 2, ["eq_312", "empties_between", "items_gt_16384", "rows_cross_256", "size_1"], m=1, seed=9)
    add("draw_313", "batch", draw_batch(469), 2, ["eq_313", "empties_between"], m=1, seed=9, modes=("global",))
    add("draw_624", "batch", draw_batch(468), 2, ["eq_624"], m=2, seed=0)
    add("draw_625", "batch", draw_batch(937), 2, ["eq_625", "G_gt_640", "empties_between"], m=1, seed=M64)
    add("draw_G320", "batch", draw_batch(320), 2, ["G_eq_320", "G_le_320", "seed_0"], m=3, seed=0, modes=("global",))
    add("draw_G321", "batch", draw_batch(321), 2, ["G_eq_321", "seed_all_ones"], m=3, seed=M64)
    add("draw_m0", "batch", draw_batch(5), 2, ["m0"], m=0, seed=1)
    # ---- a generator per graph: m at the block boundary, a twist inside one graph's draws, graphs that draw nothing
    own = batch_of([ring, (4, np.zeros((2, 0), np.int64)), (2, und([(0, 1)])), (5, und(path(range(5))))], first=1)
    seeds = (0, 5, 6, M64)
    add("graphs_m312", "graphs", own, 3, ["m_eq_312", "graph_without_sets", "graph_n_lt_k"], m=312, seeds=seeds)
    add("graphs_m313", "graphs", own, 3, ["m_eq_313", "graph_without_sets"], m=313, seeds=seeds, modes=("global",))
    add("graphs_m700", "graphs", own, 3, ["m_gt_624", "graph_without_sets", "rows_cross_256"], m=700, seeds=(1 << 63, 1, 2, 3))
    return tuple(out)


ON_DEVICE = ("columns_batch", "G256_stray", "sort_pair", "draw_625", "graphs_m313", "path64_k64")   # also run with device inputs


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def census_of(name):
    c = case(name)
    what = {"batch": "sample", "graphs": "sample"}.get(c.what, c.what)
    out = set()
    for mode in c.modes:
        out |= U.census(c.ei, c.ptr, c.m, c.k, c.seeds if c.what == "graphs" else c.seed, c.what != "batch", what, mode)
    return frozenset(out)


def graphs_law(ei, ptr, m, k, mode, seeds):
    """sample_graphs as one-graph law calls over the batch's columns, edge_ptr re-based"""
    nodes, eidx, eptr, esrc = [], [], [np.zeros(1, np.int64)], []
    G = len(ptr) - 1
    for g in range(G):
        one = U.sample_batch(ei, ptr[g:g + 2], m, k, mode, seeds[g])
        nodes.append(one[0]); eidx.append(one[1]); esrc.append(one[4])
        eptr.append(one[2][1:] + eptr[-1][-1])
    return (np.concatenate(nodes).reshape(G * m, k), np.concatenate(eidx + [np.zeros((2, 0), np.int64)], axis=1),
            np.concatenate(eptr), np.arange(G + 1, dtype=np.int64) * m, np.concatenate(esrc + [np.zeros(0, np.int64)]))


@functools.lru_cache(maxsize=None)
def law_of(name, mode):
    """The law's tensors of the case: computed once, shared, never modified (the arrays are read-only).  batch / graphs: the five
    of uniform_law.sample_batch; enumerate: uniform_enum_law's six (the last: counts); count: (counts,)."""
    c = case(name)
    if c.what == "batch":
        out = U.sample_batch(c.ei, c.ptr, c.m, c.k, mode, c.seed)
    elif c.what == "graphs":
        out = graphs_law(c.ei, c.ptr, c.m, c.k, mode, c.seeds)
    elif c.what == "enumerate":
        out = EL.enumerate_graphs(c.ei, c.ptr, c.k, mode)
    else:
        out = (np.array(c.counts, np.int64),)                        # the closed form, stated with the case
    for a in out:
        a.setflags(write=False)
    return out
