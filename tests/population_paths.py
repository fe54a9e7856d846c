"""population_paths.py -- the inputs that pin what only uniform_sampler.PopulationCache runs (ugs_uniform.hip): the mask-form rows and
fill of a cached call (uni_pop_pairs, uni_pop_rows, uni_pop_fill), the copy of a graph's keys at add time (uni_pop_store), the
adjacency fingerprint and its check (pop_fingerprint, uni_pop_check) and the loop fingerprint of a WL population (uni_pop_loops).
Shared by tests/test_population_paths_law.py (CPU: census, device model, mutants) and tests/test_gpu_population_paths.py.  Nothing
here calls the library.

draw_cases()   sampling calls through a population.  The first ones are the "batch" and "graphs" cases of tests/uniform_paths.py
               as they are (their law is uniform_paths.law_of, their classes uniform_law.census); the others are new, with the classes
               of ROW_CLASSES, computed by `row_census` from the inputs and the law's draws.
STORE          one add of graphs with 8312 and 8313 keys beside small, failed and set-less ones, and a draw of 4000 rows from them.
check_cases()  a batch, the same batch with some graphs' adjacency altered, the graph the check must name (CHECK_CLASSES).
loop_cases()   the same for the loop vertices of a WL population (LOOP_CLASSES).
"""
import collections
import functools

import numpy as np

import uniform_distinct_law as D
import uniform_enum_law as EL
import uniform_law as U
import uniform_paths as UP
import uniform_wide_law as W
import uniform_wide_paths as WP
from uniform_paths import batch_of, one_way, path, und

LANES, ROW_BLOCK, STORE_Y = 16, 256, 32                             # POP_LANES, UNI_BLOCK, the store grid's y
STORE_TRIP = STORE_Y * ROW_BLOCK                                     # keys one trip of uni_pop_store copies per graph
LOOP_WORDS = 16                                                     # UGS_UNI_WIDE_MAX_N / 64
NONE = np.zeros((2, 0), np.int64)
EMPTY = (0, NONE)

# ---------------------------------------------------------------- draws ----------------------------------------------------------------
Draw = collections.namedtuple("Draw", "name what ei ptr m k seed seeds modes reaches failed limit source")

ROW_CLASSES = tuple([f"lane_ge10_writes_{c}" for c in (1, 2, 3, 4)] + [f"lane15_writes_{c}" for c in (1, 2, 3, 4)] + [
    "all_16_lanes_write", "k_eq_16", "k_eq_17", "k_ge_33", "minus_one_n_lt_k_k_gt_16", "minus_one_empty_graph_k_gt_16",
    "minus_one_edgeless_graph_k_gt_16", "minus_one_failed_graph_k_gt_16", "distinct_minus_one_inside_live_graph_k_gt_16",
    "group_spans_two_graphs", "rows_not_multiple_of_16", "nepos_ne_g", "per_graph_seeds", "edge_endpoint_63_as_u", "edge_endpoint_63_as_v",
    "loop_at_63"])


def natural_path(n):
    return n, und(path(range(n)))


@functools.lru_cache(maxsize=None)
def draw_cases():
    out = []
    for c in UP.cases():
        if c.what in ("batch", "graphs"):
            G = len(c.ptr) - 1
            out.append(Draw(c.name, c.what, c.ei, c.ptr, c.m, c.k, c.seed, c.seeds, c.modes, c.reaches, (False,) * G, 64, "uniform_paths"))

    def add(name, what, batch, k, m, reaches, seed=0, seeds=None, modes=("sample", "global"), failed=None, limit=64):
        G = len(batch[1]) - 1
        out.append(Draw(name, what, batch[0], batch[1], m, k, seed, seeds, tuple(modes), tuple(reaches), tuple(failed) if failed else (False,) * G,
                        limit, "population"))

    # ---- the member windows of the lanes 10 ... 15: the sets of a path of 64 at k = 33 end at every vertex from 32 to 63
    add("path64_k33_lanes", "batch", batch_of([UP.natural_path_63()], first=3), 33, 200,
        [f"lane_ge10_writes_{c}" for c in (1, 2, 3, 4)] + [f"lane15_writes_{c}" for c in (1, 2, 3, 4)] +
        ["k_ge_33", "edge_endpoint_63_as_u", "edge_endpoint_63_as_v", "loop_at_63", "rows_not_multiple_of_16"], seed=6)
    add("path64_k64_all_lanes", "batch", batch_of([natural_path(64), natural_path(64)]), 64, 3,
        ["all_16_lanes_write", "lane15_writes_4", "k_ge_33", "group_spans_two_graphs", "rows_not_multiple_of_16"], seed=1)
    three = [natural_path(20), natural_path(18), natural_path(25)]
    add("paths_k16", "batch", batch_of(three, first=1), 16, 5, ["k_eq_16", "group_spans_two_graphs", "rows_not_multiple_of_16"], seed=2)
    add("paths_k17", "graphs", batch_of(three), 17, 5, ["k_eq_17", "per_graph_seeds", "group_spans_two_graphs"], seeds=(4, 5, U.M64))
    # ---- rows of -1 at k > 16: the second trip of the loop that writes them, every way a row comes to be one
    dead = [EMPTY, natural_path(10), (20, NONE), natural_path(20), (3, NONE), natural_path(19)]
    add("minus_one_k17_batch", "batch", batch_of(dead, first=2), 17, 6,
        ["minus_one_n_lt_k_k_gt_16", "minus_one_empty_graph_k_gt_16", "minus_one_edgeless_graph_k_gt_16", "nepos_ne_g", "k_eq_17",
         "group_spans_two_graphs", "rows_not_multiple_of_16"], seed=3)
    add("minus_one_k33_batch", "batch", batch_of([natural_path(32), natural_path(40)]), 33, 3, ["minus_one_n_lt_k_k_gt_16", "k_ge_33", "nepos_ne_g"], seed=4)
    add("minus_one_failed_k17_graphs", "graphs", batch_of([natural_path(70), natural_path(20), natural_path(66)]), 17, 5,
        ["minus_one_failed_graph_k_gt_16", "per_graph_seeds", "k_eq_17"], seeds=(7, 8, 9), failed=(True, False, True))
    add("distinct_k17", "distinct", batch_of([natural_path(20), natural_path(18), natural_path(16), natural_path(30)], first=1), 17, 6,
        ["distinct_minus_one_inside_live_graph_k_gt_16", "minus_one_n_lt_k_k_gt_16", "per_graph_seeds", "k_eq_17", "group_spans_two_graphs"],
        seeds=(11, 12, 13, 14))
    return tuple(out)


def draw_case(name):
    return next(c for c in draw_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def graph_masks(name):
    """S_g of every graph of the case as uniform_law.sorted_masks gives it; () for a graph that has none or failed"""
    c = draw_case(name)
    out = []
    for g in range(len(c.ptr) - 1):
        lo, n = int(c.ptr[g]), int(c.ptr[g + 1] - c.ptr[g])
        live = 1 <= c.k <= n <= 64 and not c.failed[g]
        out.append(tuple(int(x) for x in U.sorted_masks(U.graph_adjacency(c.ei[0], c.ei[1], lo, n), c.k)) if live else ())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def draw_rows(name):
    """The law's draws: for every row of the call (graph, vertex mask), mask 0 for a row of -1"""
    c = draw_case(name)
    sets, G, m = graph_masks(name), len(c.ptr) - 1, c.m
    rows = []
    if c.what == "batch":
        gen = U.mt19937_64(c.seed & U.M64)
        for g in range(G):
            rows += [(g, sets[g][U.lemire(gen, len(sets[g]))] if sets[g] else 0) for _ in range(m)]
    elif c.what == "graphs":
        for g in range(G):
            gen = U.mt19937_64(int(c.seeds[g]) & U.M64)
            rows += [(g, sets[g][U.lemire(gen, len(sets[g]))] if sets[g] else 0) for _ in range(m)]
    else:
        for g in range(G):
            rows += [(g, sets[g][d] if d >= 0 else 0) for d in D.law(int(c.seeds[g]) & D.M64, len(sets[g]), m)]
    return tuple(rows)


def bucket(c, g):
    """graph g's columns in batch column order: (batch column, local u, local v)"""
    lo, hi = int(c.ptr[g]), int(c.ptr[g + 1])
    inside = np.nonzero((c.ei[0] >= lo) & (c.ei[0] < hi) & (c.ei[1] >= lo) & (c.ei[1] < hi))[0]
    return [(int(q), int(c.ei[0, q]) - lo, int(c.ei[1, q]) - lo) for q in inside]


@functools.lru_cache(maxsize=None)
def row_census(name):
    """The classes of ROW_CLASSES the case reaches in uni_pop_rows / uni_pop_fill, from the input and the law's draws"""
    c = draw_case(name)
    rows, sets, G, k, m = draw_rows(name), graph_masks(name), len(c.ptr) - 1, c.k, c.m
    out = set()
    hit = lambda cls, cond=True: out.add(cls) if cond else None      # noqa: E731
    sizes = np.diff(c.ptr)
    buckets = {g: bucket(c, g) for g in range(G)}
    live_graph = [bool(sets[g]) for g in range(G)]
    for g, mask in set(rows):
        if mask:
            per_lane = [bin((mask >> (4 * l)) & 15).count("1") for l in range(LANES)]
            for l in range(10, LANES):
                hit(f"lane_ge10_writes_{per_lane[l]}", per_lane[l] > 0)
            hit(f"lane15_writes_{per_lane[15]}", per_lane[15] > 0)
            hit("all_16_lanes_write", all(per_lane))
            hit("k_eq_16", k == 16)
            hit("k_eq_17", k == 17)
            hit("k_ge_33", k >= 33)
            for _, u, v in buckets[g]:
                if mask >> u & mask >> v & 1:
                    hit("edge_endpoint_63_as_u", u == 63 and v != 63)
                    hit("edge_endpoint_63_as_v", v == 63 and u != 63)
                    hit("loop_at_63", u == v == 63)
        elif k > 16:
            hit("minus_one_failed_graph_k_gt_16", c.failed[g])
            hit("minus_one_empty_graph_k_gt_16", sizes[g] == 0)
            hit("minus_one_n_lt_k_k_gt_16", 0 < sizes[g] < k and not c.failed[g])
            hit("minus_one_edgeless_graph_k_gt_16", sizes[g] >= k and not buckets[g] and not c.failed[g])
            hit("distinct_minus_one_inside_live_graph_k_gt_16", c.what == "distinct" and live_graph[g])
    # (a workgroup's 16 rows r ... r + 15, the last workgroup's fewer)
    hit("group_spans_two_graphs", m > 0 and LANES % m != 0 and any(r // m != min(r + LANES - 1, G * m - 1) // m for r in range(0, G * m, LANES)))
    hit("rows_not_multiple_of_16", (G * m) % LANES != 0)
    hit("per_graph_seeds", c.what != "batch" and G * m > 0)
    hit("nepos_ne_g", c.what == "batch" and m > 0 and any(live_graph[g] and not all(live_graph[:g]) for g in range(G)))
    return frozenset(out)


def distinct_law(c, mode):
    """The seven tensors of sample_distinct: the rows uniform_distinct_law.law names, taken from uniform_enum_law's enumeration"""
    G, m, k = len(c.ptr) - 1, c.m, c.k
    nodes_e, eidx_e, eptr_e, sptr_e, esrc_e, counts = EL.enumerate_graphs(c.ei, c.ptr, k, mode)
    nodes, eu, es, eptr = np.full((G * m, k), -1, np.int64), [], [], [0]
    for g in range(G):
        for j, d in enumerate(D.law(int(c.seeds[g]) & D.M64, int(counts[g]), m)):
            if d >= 0:
                r = int(sptr_e[g]) + d
                nodes[g * m + j] = nodes_e[r]
                eu.append(eidx_e[:, eptr_e[r]:eptr_e[r + 1]])
                es.append(esrc_e[eptr_e[r]:eptr_e[r + 1]])
            eptr.append(eptr[-1] + (int(eptr_e[r + 1] - eptr_e[r]) if d >= 0 else 0))
    return (nodes, np.concatenate(eu + [NONE], axis=1), np.array(eptr, np.int64), np.arange(G + 1, dtype=np.int64) * m,
            np.concatenate(es + [np.zeros(0, np.int64)]), np.zeros(G, bool), np.minimum(counts, m).astype(np.int64))


@functools.lru_cache(maxsize=None)
def draw_law(name, mode):
    """The law's tensors of a draw case (read-only, shared): five, or the seven of sample_distinct"""
    c = draw_case(name)
    if c.source == "uniform_paths":
        return UP.law_of(name, mode)
    if c.what == "batch":
        out = U.sample_batch(c.ei, c.ptr, c.m, c.k, mode, c.seed)
    elif c.what == "graphs":
        out = WP.graphs_law(c, mode)
    else:
        out = distinct_law(c, mode)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- store ----------------------------------------------------------------
Store = collections.namedtuple("Store", "k m seed graphs sizes failed_at ei ptr order")
STORE_CLASSES = ("store_second_trip", "draw_index_ge_8192", "draw_index_le_8191_in_same_graph")


@functools.lru_cache(maxsize=None)
def store_case():
    """Added in one call, in this order: G8192 (8312 sets at k = 4), a graph of 70 vertices (it fails under the default vertex
    limit), G8193 (8313 sets), a graph without sets, SMALL_ROOTS.  The batch that is drawn from leaves the failed graph out."""
    graphs = [UP.G8192, natural_path(70), UP.G8193, (3, NONE), UP.SMALL_ROOTS]
    order = [2, 4, 3, 0]                                             # positions in `graphs` of the batch's graphs
    ei, ptr = batch_of([graphs[i] for i in order], first=1)
    sizes = [len(U.esu_masks(U.graph_adjacency(e[0], e[1], 0, n), 4)) if n <= 64 else -1 for n, e in graphs]
    ei.setflags(write=False)
    return Store(4, 4000, 13, tuple(graphs), tuple(sizes), 1, ei, ptr, tuple(order))


@functools.lru_cache(maxsize=None)
def store_draws():
    """[(graph of the batch, draw index)] of the store case's rows, by the law's generator"""
    c = store_case()
    gen, out = U.mt19937_64(c.seed), []
    for g, i in enumerate(c.order):
        out += [(g, U.lemire(gen, c.sizes[i])) for _ in range(c.m if c.sizes[i] > 0 else 0)]
    return tuple(out)


def store_census():
    c = store_case()
    draws = store_draws()
    out = set()
    if max(c.sizes) > STORE_TRIP:
        out.add("store_second_trip")
    for g in {g for g, d in draws if d >= STORE_TRIP}:
        out.add("draw_index_ge_8192")
        if any(h == g and d < STORE_TRIP for h, d in draws):
            out.add("draw_index_le_8191_in_same_graph")
    return out


@functools.lru_cache(maxsize=None)
def store_law(mode):
    c = store_case()
    out = U.sample_batch(c.ei, c.ptr, c.m, c.k, mode, c.seed)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- the adjacency check ----------------------------------------------------------------
Check = collections.namedtuple("Check", "name graphs ei ptr bad expect k limit what failed reaches")
CHECK_CLASSES = ("words_le_256", "words_gt_256", "diff_word_index_ge_256", "diff_in_last_word", "n1024", "mask_n64_diff_at_bit_63",
                 "same_words_other_positions", "two_graphs_differ_first_named", "differing_graph_first", "differing_graph_last",
                 "form0_graph_skipped", "mask_and_wide_in_one_batch", "degree_sequence_kept")
CHECK_M, CHECK_SEED = 3, 17


def form_of(n, k, limit, failed=False):
    """0: not enumerated (no set, or failed), 1: one 64-bit word per vertex, 2: (n + 63) / 64 words per vertex"""
    if failed or k < 1 or n < k or n > limit:
        return 0
    return 2 if n > 64 else 1


def bitmap_words(n, cols, form):
    """The adjacency bitmap of a graph as uni_adj / uni_wadj leave it: loops join nothing, both directions are set"""
    if form == 0:
        return []
    W_ = 1 if form == 1 else (n + 63) >> 6
    words = [0] * (n * W_)
    for u, v in zip(*np.asarray(cols).tolist()):
        if u != v:
            words[u * W_ + (v >> 6)] |= 1 << (v & 63)
            words[v * W_ + (u >> 6)] |= 1 << (u & 63)
    return words


def replaced(cols, old, new):
    """the columns of the undirected pair `old` (either direction) become the pair `new`, direction kept"""
    out = np.array(cols, np.int64)
    a, b = old
    fwd, bwd = (out[0] == a) & (out[1] == b), (out[0] == b) & (out[1] == a)
    assert fwd.any() or bwd.any()
    out[:, fwd] = np.array([[new[0]], [new[1]]])
    out[:, bwd] = np.array([[new[1]], [new[0]]])
    return out


@functools.lru_cache(maxsize=None)
def check_cases():
    out = []

    def add(name, graphs, altered, expect, reaches, k=2, what="batch", failed=(), first=0):
        """altered: {graph: its columns in the altered batch}"""
        limit = 1024 if any(n > 64 and g not in failed for g, (n, _) in enumerate(graphs)) else 64
        ei, ptr = batch_of(graphs, first=first)
        bad = batch_of([(n, altered.get(g, e)) for g, (n, e) in enumerate(graphs)], first=first)[0]
        for a in (ei, ptr, bad):
            a.setflags(write=False)
        out.append(Check(name, tuple(graphs), ei, ptr, bad, expect, k, limit, what, tuple(failed), tuple(reaches)))

    small = [natural_path(12), (9, und(path(range(9)) + [(0, 8)])), natural_path(7)]
    add("mask_flip", small, {1: replaced(small[1][1], (3, 4), (3, 5))}, 1, ["words_le_256"], first=2)
    w130 = WP.sparse(130)
    add("wide130_last_word", [w130], {0: replaced(w130[1], (128, 129), (0, 1))}, 0,
        ["words_gt_256", "diff_word_index_ge_256", "diff_in_last_word", "differing_graph_first", "differing_graph_last"])
    p1024 = natural_path(1024)
    add("path1024_row_1023", [p1024], {0: replaced(p1024[1], (1022, 1023), (0, 1))}, 0, ["n1024", "words_gt_256", "diff_in_last_word", "diff_word_index_ge_256"])
    p64 = natural_path(64)
    add("mask64_bit_63", [natural_path(5), p64], {1: replaced(p64[1], (62, 63), (0, 1))}, 1, ["mask_n64_diff_at_bit_63", "differing_graph_last"])
    # the rows of 0 and 1 exchanged, and with them those of 2 and 3: the same words at other places
    cross = (6, und([(0, 2), (1, 3), (4, 5)]))
    add("rows_exchanged_mask", [natural_path(4), cross], {1: und([(0, 3), (1, 2), (4, 5)])}, 1, ["same_words_other_positions", "degree_sequence_kept"])
    wcross = (130, und([(0, 128), (1, 129)] + path(range(2, 128))))
    add("rows_exchanged_wide", [wcross, natural_path(4)], {0: und([(0, 129), (1, 128)] + path(range(2, 128)))}, 0,
        ["same_words_other_positions", "words_gt_256", "differing_graph_first"])
    five = [natural_path(8), natural_path(9), natural_path(10), natural_path(11), natural_path(6)]
    add("two_graphs_differ", five, {3: replaced(five[3][1], (1, 2), (1, 3)), 1: replaced(five[1][1], (4, 5), (3, 5))}, 1,
        ["two_graphs_differ_first_named"], first=1)
    add("first_graph_differs", five, {0: replaced(five[0][1], (6, 7), (5, 7))}, 0, ["differing_graph_first"])
    add("last_graph_differs", five, {4: replaced(five[4][1], (0, 1), (0, 2))}, 4, ["differing_graph_last"])
    skipped = [natural_path(70), (1, NONE), natural_path(9), natural_path(10)]
    add("failed_graph_ahead", skipped, {2: replaced(skipped[2][1], (7, 8), (6, 8))}, 2, ["form0_graph_skipped"], what="graphs", failed=(0,))
    mixed = [natural_path(10), WP.sparse(66), natural_path(12), WP.sparse(70)]
    add("mask_and_wide", mixed, {3: replaced(mixed[3][1], (68, 69), (67, 69)), 2: replaced(mixed[2][1], (10, 11), (9, 11))}, 2,
        ["mask_and_wide_in_one_batch", "two_graphs_differ_first_named"], k=3, first=4)
    ring = (10, und(path(list(range(10)) + [0])))
    add("edge_swap", [ring], {0: replaced(replaced(ring[1], (0, 1), (0, 6)), (5, 6), (5, 1))}, 0, ["degree_sequence_kept"])
    return tuple(out)


def check_case(name):
    return next(c for c in check_cases() + loop_cases() if c.name == name)


def graph_cols(c, ei, g):
    lo, hi = int(c.ptr[g]), int(c.ptr[g + 1])
    inside = (ei[0] >= lo) & (ei[0] < hi) & (ei[1] >= lo) & (ei[1] < hi)
    return ei[:, inside] - lo


def forms(c):
    return [form_of(n, c.k, c.limit, g in c.failed) for g, (n, _) in enumerate(c.graphs)]


def plain_adjacency(src, dst, lo, n):
    """uniform_law.graph_adjacency without the loops: the undirected non-loop pairs"""
    return [x & ~(1 << v) for v, x in enumerate(U.graph_adjacency(src, dst, lo, n))]


def adjacency_law(c, ei):
    """The smallest enumerated graph whose adjacency (undirected non-loop pairs) is not the added graph's; None: none"""
    for g, (n, e) in enumerate(c.graphs):
        if forms(c)[g] and plain_adjacency(ei[0], ei[1], int(c.ptr[g]), n) != plain_adjacency(e[0], e[1], 0, n):
            return g
    return None


@functools.lru_cache(maxsize=None)
def check_census(name):
    c = check_case(name)
    out = set()
    hit = lambda cls, cond=True: out.add(cls) if cond else None      # noqa: E731
    fm, G = forms(c), len(c.graphs)
    differing = []
    for g, (n, e) in enumerate(c.graphs):
        if not fm[g]:
            continue
        a, b = bitmap_words(n, e, fm[g]), bitmap_words(n, graph_cols(c, c.bad, g), fm[g])
        hit("words_le_256", len(a) <= ROW_BLOCK)
        hit("words_gt_256", len(a) > ROW_BLOCK)
        diff = [i for i in range(len(a)) if a[i] != b[i]]
        if not diff:
            continue
        differing.append(g)
        hit("diff_word_index_ge_256", min(diff) >= ROW_BLOCK)
        hit("diff_in_last_word", len(a) - 1 in diff)
        hit("n1024", n == 1024)
        hit("mask_n64_diff_at_bit_63", fm[g] == 1 and n == 64 and any((a[i] ^ b[i]) >> 63 for i in diff))
        hit("same_words_other_positions", sorted(x for x in a if x) == sorted(x for x in b if x))
        hit("degree_sequence_kept", [bin(x).count("1") for x in a] == [bin(x).count("1") for x in b] if fm[g] == 1 else False)
    hit("two_graphs_differ_first_named", len(differing) >= 2)
    hit("differing_graph_first", differing[0] == 0)
    hit("differing_graph_last", differing[-1] == G - 1)
    hit("form0_graph_skipped", any(g in c.failed for g in range(differing[0])))
    hit("mask_and_wide_in_one_batch", 1 in fm and 2 in fm)
    return frozenset(out)


def check_law(c, mode):
    """the law's tensors of the unaltered batch"""
    if c.what == "batch":
        return W.sample_batch(c.ei, c.ptr, CHECK_M, c.k, mode, CHECK_SEED)
    failed = tuple(g in c.failed for g in range(len(c.graphs)))
    as_case = collections.namedtuple("G", "ei ptr m k seeds failed")(c.ei, c.ptr, CHECK_M, c.k, check_seeds(c), failed)
    return WP.graphs_law(as_case, mode)


def check_seeds(c):
    return tuple(CHECK_SEED + 3 * g for g in range(len(c.graphs)))


# ---------------------------------------------------------------- the loop vertices of a WL population ----------------------------------------------------------------
LOOP_CLASSES = ("loop_word_0", "loop_word_ge_1", "loop_at_1023", "loop_sets_differ_only_in_word_index", "duplicate_loop_columns",
                "bucket_gt_256_columns", "two_graphs_differ_first_named", "mask_and_wide")
LOOP_ITERATIONS = 2


def with_loops(graph, loops):
    n, e = graph
    return n, np.concatenate([e, one_way([(v, v) for v in loops]).reshape(2, -1)], axis=1)


@functools.lru_cache(maxsize=None)
def loop_cases():
    """Check tuples again: `graphs` carry the loops that are added, `bad` the batch with other loops; the adjacency is the same"""
    out = []

    def add(name, plain, stored, batch, expect, reaches, k=2, first=0):
        """stored / batch: {graph: its loop vertices, in column order}"""
        graphs = [with_loops(g, stored.get(i, ())) for i, g in enumerate(plain)]
        limit = 1024 if any(n > 64 for n, _ in graphs) else 64
        ei, ptr = batch_of(graphs, first=first)
        bad = batch_of([with_loops(g, batch.get(i, stored.get(i, ()))) for i, g in enumerate(plain)], first=first)[0]
        for a in (ei, ptr, bad):
            a.setflags(write=False)
        out.append(Check(name, tuple(graphs), ei, ptr, bad, expect, k, limit, "batch", (), tuple(reaches)))

    p12, p130, p1024 = natural_path(12), natural_path(130), natural_path(1024)
    add("loop_moves_in_word_0", [natural_path(5), p12], {1: (5,)}, {1: (6,)}, 1, ["loop_word_0"], first=1)
    add("loop_0_stored_64_given", [p130], {0: (0,)}, {0: (64,)}, 0, ["loop_sets_differ_only_in_word_index", "loop_word_ge_1"])
    add("loop_64_stored_0_given", [p130, p12], {0: (64,)}, {0: (0,)}, 0, ["loop_sets_differ_only_in_word_index", "loop_word_ge_1", "mask_and_wide"])
    add("loop_at_1023", [p1024], {0: (1023,)}, {0: (1023, 1022)}, 0, ["loop_at_1023", "loop_word_ge_1"])
    add("loop_given_twice", [p12, natural_path(9)], {0: (3, 3), 1: (2,)}, {0: (4, 4)}, 0, ["duplicate_loop_columns", "loop_word_0"])
    # 33 vertices, 256 edge columns ahead of the loop column: the loop lies in the second trip over the graph's bucket
    many = (33, und(path(range(33)) * 4))
    add("loop_past_256_columns", [many], {0: (7,)}, {0: (8,)}, 0, ["bucket_gt_256_columns", "loop_word_0"], k=3)
    four = [p12, natural_path(70), natural_path(8), natural_path(9)]
    add("loops_of_two_graphs_differ", four, {1: (69,), 3: (1,)}, {1: (68,), 3: (2,)}, 1, ["two_graphs_differ_first_named", "mask_and_wide", "loop_word_ge_1"], first=2)
    return tuple(out)


def loop_set(cols):
    return sorted({int(u) for u, v in zip(*np.asarray(cols).tolist()) if u == v})


def loops_law(c, ei):
    """The smallest enumerated graph whose set of loop vertices is not the added graph's; None: none"""
    for g, (n, e) in enumerate(c.graphs):
        if forms(c)[g] and loop_set(graph_cols(c, ei, g)) != loop_set(e):
            return g
    return None


@functools.lru_cache(maxsize=None)
def loop_census(name):
    c = check_case(name)
    out = set()
    hit = lambda cls, cond=True: out.add(cls) if cond else None      # noqa: E731
    fm, differing = forms(c), []
    for g, (n, e) in enumerate(c.graphs):
        given = graph_cols(c, c.bad, g)
        a, b = loop_set(e), loop_set(given)
        for cols in (e, given):
            loops = [int(u) for u, v in zip(*np.asarray(cols).tolist()) if u == v]
            hit("duplicate_loop_columns", len(loops) > len(set(loops)))
            at = [q for q, (u, v) in enumerate(zip(*np.asarray(cols).tolist())) if u == v]
            hit("bucket_gt_256_columns", cols.shape[1] > ROW_BLOCK and any(q >= ROW_BLOCK for q in at))
        if a == b or not fm[g]:
            continue
        differing.append(g)
        hit("loop_word_0", any(v < 64 for v in a + b))
        hit("loop_word_ge_1", any(v >= 64 for v in a + b))
        hit("loop_at_1023", 1023 in a + b)
        hit("loop_sets_differ_only_in_word_index", sorted(v & 63 for v in a) == sorted(v & 63 for v in b) and
            sorted(1 << (v & 63) for v in a) == sorted(1 << (v & 63) for v in b))
    hit("two_graphs_differ_first_named", len(differing) >= 2)
    hit("mask_and_wide", 1 in fm and 2 in fm)
    return frozenset(out)
