"""uniform_wide_paths.py -- the inputs that pin the wide-form kernel paths of uniform_sampler (ugs_uniform.hip: graphs of 65 to 1024
vertices, and smaller ones below the mask threshold), shared by the CPU tests (tests/test_uniform_wide_paths_law.py: census, device
model, mutants) and the GPU tests (tests/test_gpu_uniform_wide_paths.py).  Every case names in `reaches` the census classes
(uniform_wide_law.census) it is there for, and both test files assert them again, so an input that stops reaching its path fails
instead of losing coverage.

`what` says which entry the case goes through: "batch" (sample_batch, one generator), "graphs" (sample_graphs, a seed per graph),
"enumerate" (enumerate_graphs: every key's position, and count_graphs beside it), "count" (count_graphs alone, against a closed
form) or "refused" (enumerate_graphs one set past max_rows: "split the call", and the next call is served).  Every case runs with
the vertex limit at 1024 and the mask threshold at `mask_vertices`.  `closed`: {graph: its number of sets} for a graph past the device
budget, `failed`: the flags sample_graphs / enumerate_graphs must report."""
import collections
import functools
import math

import numpy as np

import uniform_enum_law as EL
import uniform_law as U
import uniform_wide_law as W
from uniform_paths import batch_of, complete, one_way, path, und

Case = collections.namedtuple("Case", "name what ei ptr m k seed seeds modes counts reaches max_rows mask_vertices closed failed")
LIMIT = 1024
NONE = np.zeros((2, 0), np.int64)
EMPTY = (0, NONE)


def sparse(n, extra=()):
    """A path over all n vertices with a chord from every ninth vertex (most of them across words), given both ways, and `extra`
    columns given once"""
    chords = [(i, (i * 37 + 11) % n) for i in range(0, n, 9) if (i * 37 + 11) % n != i]
    return n, np.concatenate([und(path(range(n)) + chords), one_way(list(extra)).reshape(2, -1)], axis=1)


def hub1024():
    """Hub 0 joined to vertices in the words 0, 1, 3, 7, 9 and 15 (every difference of two of them has the bits 1, 2, 4 and 8
    somewhere), 63 and 1023 among them; second levels on both sides of vertex 512 again; 1023 gains the lower vertices 2 and 300;
    63 is a root whose only higher neighbour lies in the next word; loops at 0 and 1023, a duplicate and columns given one way."""
    spokes = [(0, v) for v in (5, 63, 70, 200, 450, 600, 1023)]
    second = [(5, 100), (5, 520), (5, 900), (1023, 2), (1023, 300), (450, 700), (450, 130), (63, 64), (600, 1000), (600, 20)]
    return 1024, np.concatenate([und(spokes + second), one_way([(0, 0), (1023, 1023), (5, 100), (900, 901), (901, 902)])], axis=1)


def star130():
    """Hub 0 with the leaves 1 ... 129 (three trips of the slot loop; at k = 3 the hub's bucket holds C(129, 2) = 8256 keys) and a
    few edges among the first leaves for small buckets beside it"""
    return 130, one_way([(0, i) for i in range(1, 130)] + [(1, 2), (1, 3), (1, 4), (2, 3), (127, 128), (128, 129)])


def cluster256():
    """K_17 on the vertices 128 ... 144 of 256: at k = 8 the fields are 8 bits wide, every key has bit 63 set, root 128 holds
    C(16, 7) = 11440 keys and root 129 C(15, 7) = 6435"""
    return 256, one_way([(128 + u, 128 + v) for u, v in complete(17)])


def k10_across_words():
    """K_10 on the vertices 58 ... 67 of 70: 63 is a root, a first extension and a member in every place"""
    return 70, one_way([(58 + u, 58 + v) for u, v in complete(10)])


def chunks40():
    """A one-way path over the first 40 of 66 vertices: 39 columns (three chunks of 16), column 15 = (15, 16), column 16 = (16, 17)"""
    return 66, one_way(path(range(40)))


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, what, batch, k, reaches, m=0, seed=0, seeds=None, modes=("sample",), counts=None, max_rows=1 << 22, mask_vertices=64,
            closed=None, failed=None):
        G = len(batch[1]) - 1
        out.append(Case(name, what, batch[0], batch[1], m, k, seed, seeds, tuple(modes), counts, tuple(reaches), max_rows, mask_vertices,
                        tuple(sorted((closed or {}).items())), tuple(failed) if failed is not None else (False,) * G))

    # ---- the slot loop: 64, 65 and more higher neighbours, the r-th member in every place
    k66 = batch_of([(66, one_way(complete(66)))])
    add("K66_k3", "enumerate", k66, 3, ["wide_only", "W2", "k3", "deg64", "deg65", "deg1", "deg0", "rth_above_lowest_lane", "rth_inside_word",
                                        "rth_bit63", "root_bit63", "root_two_lanes", "root_shr1", "last_two_lanes", "last_shr1", "bucket_0",
                                        "bucket_1", "bucket_np2", "rows_cross_256", "adj_bit63", "adj_last_word"])
    add("K66_k4_count", "count", k66, 4, ["k4", "deg65", "lane_flush_remainder"], counts=(math.comb(66, 4),))
    add("K70_k3", "enumerate", batch_of([(70, one_way(complete(70)))], first=5), 3, ["deg65", "deg64", "ptr0_nonzero", "global"], modes=("global",))
    add("K34_k5_count_narrow", "count", batch_of([(34, one_way(complete(34)))]), 5, ["k5", "item_gt_4096", "lane_flush_remainder"],
        counts=(math.comb(34, 5),), mask_vertices=0)
    star = batch_of([star130()])
    add("star130_k2", "enumerate", star, 2, ["k2", "W_np2", "last_two_lanes", "last_shr1", "last_shr2", "bucket_0", "bucket_1", "bucket_np2"],
        modes=("sample", "global"))
    add("star130_k3", "enumerate", star, 3, ["deg_ge129", "deg0", "deg1", "small_and_large_buckets", "rth_above_lowest_lane", "bucket_np2"],
        modes=("global",))
    # ---- 16 words per vertex: the prefix sums over lanes on both sides of 8, 4, 2 and 1, vertex 1023, bit 63
    hub = batch_of([hub1024()], first=2)
    scans = ["root_two_lanes", "root_shr1", "root_shr2", "root_shr4", "root_shr8", "last_two_lanes", "last_shr1", "last_shr2", "last_shr4", "last_shr8"]
    add("hub1024_k3", "enumerate", hub, 3, scans + ["W16", "n1024", "adj_v1023", "adj_last_word", "adj_bit63", "adj_loop", "adj_duplicate", "adj_reversed",
                                                   "root_bit63", "root_ext_later_word", "root_lower_in_word", "rth_bit63", "rth_inside_word", "key_insert_after_root",
                                                   "row_with_loop", "deg1", "deg0"], modes=("sample", "global"))
    add("hub1024_k4", "enumerate", hub, 4, scans + ["k4", "take_lane_above0", "key_insert_middle", "key_insert_after_root", "ext_gains_below_taken",
                                                   "row_with_loop"], modes=("sample", "global"))
    add("hub1024_k4_batch", "batch", hub, 4, ["W16", "n1024", "sample", "global"], m=40, seed=3, modes=("sample", "global"))
    # ---- every level: k = 5, 6, 7 across the first word boundary, k = 8 with whole-width keys and both sort routes
    k10 = batch_of([k10_across_words()], first=1)
    for k in (5, 6, 7):
        add(f"K10_k{k}", "enumerate", k10, k, [f"k{k}", "root_bit63", "rth_bit63"], modes=("sample",))
    add("cluster256_k8", "enumerate", batch_of([cluster256()]), 8, ["k8", "key_bit63", "n256", "small_and_large_buckets"], modes=("global",))
    add("cluster256_k8_batch", "batch", batch_of([EMPTY, cluster256()]), 8, ["k8", "key_bit63", "nepos_ne_g", "empty_before_wide"], m=50, seed=8,
        modes=("sample",))
    # ---- the sizes at which the field width changes, in one call, with loops, duplicates and one-way columns
    sized = [sparse(128, [(5, 5), (127, 127), (3, 4)]), sparse(129, [(128, 128)]), sparse(256), sparse(257, [(256, 0)]), sparse(512), sparse(513)]
    sizes = batch_of(sized, first=7, shuffle=3)
    size_classes = ["n128", "n129", "n256", "n257", "n512", "n513", "W2", "W_np2", "adj_loop", "adj_duplicate", "adj_reversed", "adj_bit63",
                    "adj_last_word", "ptr0_nonzero", "wide_only"]
    add("sizes_enum", "enumerate", sizes, 3, size_classes + ["rows_cross_256", "row_with_loop", "bucket_2", "bucket_np2"], modes=("sample", "global"))
    add("sizes_batch", "batch", sizes, 3, size_classes + ["sample", "global"], m=9, seed=12, modes=("sample", "global"))
    add("sizes_graphs", "graphs", sizes, 4, size_classes + ["per_graph_seeds", "k4"], m=5, seeds=(0, 1, U.M64, 1 << 63, 5, 6), modes=("global",))
    # ---- mask and wide graphs in one call: gstart is not monotonic in g, graphs that draw nothing in front of a wide one
    small = (2, und([(0, 1)]))
    mixed = [sparse(66), (10, und(path(range(10)))), sparse(70, [(69, 69)]), small, sparse(65), EMPTY, sparse(67), (12, und(path(range(12)))), EMPTY]
    layout = batch_of(mixed, first=3, shuffle=5)
    layout_classes = ["mask_before_wide", "mask_after_wide", "wide_mask_wide", "small_before_wide", "empty_before_wide", "ptr0_nonzero", "W2"]
    add("layout_enum", "enumerate", layout, 3, layout_classes + ["rows_cross_256"], modes=("sample", "global"))
    add("layout_batch", "batch", layout, 3, layout_classes + ["nepos_ne_g", "sample", "global"], m=7, seed=21, modes=("sample", "global"))
    add("layout_graphs", "graphs", layout, 3, layout_classes + ["per_graph_seeds"], m=6, seeds=tuple(range(40, 49)), modes=("sample",))
    # ---- k = 1: the set {0} has key 0; rows without edges; a wide graph without a column
    loops = (70, np.concatenate([und([(0, 1), (1, 2), (63, 64)]), one_way([(3, 3), (0, 0), (69, 69)])], axis=1))
    k1 = batch_of([EMPTY, loops, (66, NONE)])
    add("k1_enum", "enumerate", k1, 1, ["k1", "k1_set0", "row_without_edges", "row_with_loop", "empty_before_wide", "bucket_1"], modes=("sample", "global"))
    add("k1_batch", "batch", k1, 1, ["k1", "k1_set0", "row_without_edges", "row_with_loop", "nepos_ne_g", "pop_cols_0", "rows_cross_256"], m=200, seed=1,
        modes=("sample", "global"))
    # ---- the population's lane groups: 15, 16 and 17 columns, three chunks, hits in lane 15 of a chunk and lane 0 of the next
    cols = [(66, one_way(path(range(16)))), (66, one_way(path(range(17)))), (66, one_way(path(range(18)))), chunks40()]
    add("pop_cols_batch", "batch", batch_of(cols, first=1), 3, ["pop_cols_15", "pop_cols_16", "pop_cols_17", "pop_chunks_several",
                                                               "pop_hit_lane15_then_lane0", "wide_only"], m=40, seed=4, modes=("sample", "global"))
    add("pop_cols_graphs", "graphs", batch_of(cols), 3, ["pop_cols_15", "pop_cols_16", "pop_cols_17", "pop_chunks_several", "per_graph_seeds"], m=12,
        seeds=(9, 8, 7, 6), modes=("sample",))
    # ---- the budget: exactly max_rows is served, one more is refused as a whole, a graph past the device budget fails alone
    two = batch_of([sparse(66), sparse(68)])
    total = sum(len(s) for s in EL.graph_sets(two[0], two[1], 3))
    add("enum_at_max_rows", "enumerate", two, 3, ["enum_at_max_rows"], max_rows=total, modes=("sample",))
    add("enum_over_max_rows", "refused", two, 3, ["enum_over_max_rows"], max_rows=total - 1, modes=("sample",))
    k100 = (100, one_way(complete(100)))
    add("graphs_over_budget", "graphs", batch_of([sparse(66), k100, (9, und(path(range(9))))]), 6, ["graph_over_budget_alone", "k6", "per_graph_seeds"],
        m=4, seeds=(1, 2, 3), closed={1: math.comb(100, 6)}, failed=(False, True, False))
    return tuple(out)


ON_DEVICE = ("K66_k3", "hub1024_k4", "layout_batch", "layout_graphs", "pop_cols_batch")   # also run with device inputs


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def census_of(name):
    c = case(name)
    what = {"batch": "sample", "graphs": "sample", "refused": "enumerate"}.get(c.what, c.what)
    out = set()
    for mode in c.modes:
        out |= W.census(c.ei, c.ptr, c.m, c.k, c.seeds if c.what == "graphs" else c.seed, c.what == "graphs", what, mode, LIMIT,
                        c.mask_vertices, c.max_rows, dict(c.closed))
    return frozenset(out)


def graphs_law(c, mode):
    """sample_graphs as one-graph law calls over the batch's columns, edge_ptr re-based; a failed graph gives m rows of -1"""
    G, m, k = len(c.ptr) - 1, c.m, c.k
    nodes, eidx, eptr, esrc = [], [], [np.zeros(1, np.int64)], []
    for g in range(G):
        if c.failed[g]:
            one = (np.full((m, k), -1, np.int64), np.zeros((2, 0), np.int64), np.zeros(m + 1, np.int64), None, np.zeros(0, np.int64))
        else:
            one = W.sample_batch(c.ei, c.ptr[g:g + 2], m, k, mode, c.seeds[g])
        nodes.append(one[0]); eidx.append(one[1]); esrc.append(one[4])
        eptr.append(one[2][1:] + eptr[-1][-1])
    return (np.concatenate(nodes).reshape(G * m, k), np.concatenate(eidx + [np.zeros((2, 0), np.int64)], axis=1),
            np.concatenate(eptr), np.arange(G + 1, dtype=np.int64) * m, np.concatenate(esrc + [np.zeros(0, np.int64)]))


@functools.lru_cache(maxsize=None)
def law_of(name, mode):
    """The law's tensors of the case: computed once, shared, never modified (the arrays are read-only).  batch / graphs: the five
    of uniform_wide_law.sample_batch; enumerate: uniform_enum_law's six (the last: counts); count: (counts,); refused: ()."""
    c = case(name)
    if c.what == "batch":
        out = W.sample_batch(c.ei, c.ptr, c.m, c.k, mode, c.seed)
    elif c.what == "graphs":
        out = graphs_law(c, mode)
    elif c.what == "enumerate":
        out = EL.enumerate_graphs(c.ei, c.ptr, c.k, mode)
    elif c.what == "count":
        out = (np.array(c.counts, np.int64),)                        # the closed form, stated with the case
    else:
        out = ()
    for a in out:
        a.setflags(write=False)
    return out
