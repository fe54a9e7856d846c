"""wl_paths.py -- the inputs that pin the paths of ugs_wl.hip (hash kernel in degree and label mode, lookup kernel), shared by the
CPU tests (tests/test_wl_paths_law.py: census, device model, mutants) and the GPU tests (tests/test_gpu_wl_paths.py).  Every case
names in `reaches` the census classes (wl_law.census, wl_law.lookup_census) it is there for, and both test files assert them
again, so an input that stops reaching its path fails instead of losing coverage.

A case is (name, form, arrays, iterations, labels, reaches).  form "degree" and "labels": arrays = (nodes [S, k], edge_index [2, E],
edge_ptr [S + 1]) as int64 numpy arrays, `labels` the start labels by vertex id (a list of ints) or None.  form "lookup": arrays =
(vocab: hex string -> id, digests: hex strings, statuses), crafted directly, so that equal high words need no real hash.
The shapes are the smallest at which the path exists: k <= 32, 9 / 17 / 33 rows where one row more than a workgroup holds is
the point, a few dozen rows otherwise, label tables of at most 64 entries, lookup tables of at most 17 keys.  Rows found by search
come from a fixed seed's stream of graphs; the census asserts what was found."""
import collections
import functools
import random

import numpy as np

import wl_feature_law as FL
import wl_law as L

Case = collections.namedtuple("Case", "name form arrays iterations labels reaches")
# the mutant of tests/wl_device_model.py a case is there to kill, beside the classes it reaches
KILLS = {
    "compress_at_word15": "later_blocks", "t_not_rounded": "final_stream", "carry_dropped": "final_stream",
    "finish_no_zero_fill": "final_stream", "rank_no_tiebreak": "g16_17rows", "cmp_signed": "label_values",
    "degree_numeric": "g32_9rows", "loop_once": "k32_complete", "single_item_no_comma": "g8_33rows",
    "hex_quarters_swapped": "label_values", "slot_is_vertex": "label_values", "ballot_wave": "bad_endpoints",
    "first_trip_only": "k32_complete", "ptr_unchecked": "bad_edge_ptr", "endpoint_cast32": "bad_endpoints",
    "lookup_ignore_lo": "lookup_17", "lookup_signed": "lookup_17", "lookup_ignore_status": "lookup_17",
}


def both(es):
    return [e for u, v in es for e in ((u, v), (v, u))]


def path(n):
    return [(u, u + 1) for u in range(n - 1)]


def cycle(n):
    return path(n) + [(n - 1, 0)]


def complete(n):
    return [(u, v) for u in range(n) for v in range(u + 1, n)]


def star(leaves, centre=0):
    return [(centre, centre + 1 + i) for i in range(leaves)]


def pack(entries, k, ptr=None):
    """(nodes, edge_index, edge_ptr) from entries (row, edges): row = the number of valid ids (100, 101, ... in the first slots)
    or the k slots themselves; `ptr` replaces the running edge_ptr."""
    nodes = np.full((len(entries), k), -1, np.int64)
    cols, run = [], [0]
    for r, (row, es) in enumerate(entries):
        if isinstance(row, int):
            nodes[r, :row] = 100 + np.arange(row)
        else:
            nodes[r, :len(row)] = row
        cols += list(es)
        run.append(len(cols))
    ei = np.array([[a for a, _ in cols], [b for _, b in cols]], np.int64).reshape(2, -1)
    return nodes, np.ascontiguousarray(ei), np.array(run if ptr is None else ptr, np.int64)


def random_graph(rng, n):
    """Edges on 0..n-1 of mixed density, one entry per edge."""
    p = rng.choice([0.5, 1.0, 2.0, 4.0, 40.0]) / max(n - 1, 1)
    return [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]


@functools.lru_cache(maxsize=None)
def found_rows(seed, nmax, iterations, wanted, tries=4000):
    """The first rows of the seed's stream of random graphs that between them reach the classes `wanted`, each kept for the
    classes it adds (greedy, in stream order)."""
    rng, missing, rows = random.Random(seed), set(wanted), []
    for _ in range(tries):
        n = rng.randrange(1, nmax + 1)
        entry = (n, tuple(random_graph(rng, n)))
        got = L.census(*pack([entry], nmax), iterations) & missing
        if got:
            rows.append(entry)
            missing -= got
        if not missing:
            return tuple(rows)
    raise AssertionError("seed %d reaches no row for %s" % (seed, sorted(missing)))


FINAL_STREAM = ("final.word_complete", "final.word_straddle", "final.block_straddle", "final.opens_block", "final.flush_nothing",
                "final.flush_stores", "final.flush_opens_block", "final.finish_partial_word")
# the three rows of test_gpu_wl.py's block messages: a vertex of degree 3, 7, 11 sends 128, 256, 384 bytes from iteration 2 on
LATER_BLOCKS = [(4, both(complete(4))), (8, both(star(7))), (12, both(star(11)))]
# string order: vertex 0 has a neighbour of degree 2 and one of degree 10, "10" < "2"
STRING_ORDER = (13, both([(0, 1), (1, 2), (0, 3)] + [(3, 4 + i) for i in range(9)]))
# vertex 0: "7" + six times "1" + "10": the 2-byte piece starts at byte 7 of word 0
DEG1_STRADDLE = (17, both(star(6) + [(0, 7)] + [(7, 8 + i) for i in range(9)]))
LABELS8 = [0, 0xffffffff, 0x80000000, 0xabc, 0x12345678, 7, 0x7fffffff, 0xdeadbeef]
LABELS64 = [random.Random(64).randrange(1 << 32) for _ in range(64)]
GOOD5 = [(5, both(path(5))), (4, both(star(3))), (5, both(cycle(5))), (3, [(0, 1), (1, 2)])]


def lookup_17():
    eq, top = 5 << 64, (1 << 63 | 9) << 64
    keys = [7, eq | 1, eq | 10, eq | (1 << 63 | 3), top | 4, (1 << 128) - 1]
    keys += [(3 * j + 11) << 64 | (j * 0x9e3779b97f4a7c15 & L.M64) for j in range(11)]
    vocab = {"%032x" % x: 100 + j for j, x in enumerate(keys)}
    rows = [(7, 0), ((1 << 128) - 1, 0), (eq | 1, 0), (eq | 10, 0), (eq | (1 << 63 | 3), 0), (eq | 5, 0), (eq | (1 << 63 | 1), 0),
            (top | 4, 0), (top | 5, 0), (12 << 64, 0), (3, 0), (eq | 10, 1), (top | 4, 2), (7, 3), (eq | 1, 0)]
    return vocab, ["%032x" % d for d, _ in rows], [s for _, s in rows]


def lookup_16():
    keys = [(j * j + 1) << 64 | j for j in range(16)]
    vocab = {"%032x" % x: 2 * j for j, x in enumerate(keys)}
    digests = [keys[0], keys[15], keys[8], keys[8] + 1, keys[3] - 1, 0, keys[15] + 1]
    return vocab, ["%032x" % d for d in digests], [0] * len(digests)


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(16)
    k16 = []
    for _ in range(16):
        n = rng.randrange(2, 17)
        k16.append((n, random_graph(rng, n)))
    one = "%032x" % (9 << 64 | 9)
    return (
        Case("g8_33rows", "degree", pack([(0 if j == 10 else j % 8 + 1, path(j % 8 + 1)) for j in range(33)], 8), 1, None,
             ("group_8", "k_8", "rows_plus1_g8", "n_1", "n_lt_k", "n_eq_k", "last_group_of_wave", "row_empty", "iter_1",
              "final_1_item", "deg1.finish_one_word", "deg1.flush_stores", "deg1.finish_partial_word")),
        Case("g16_17rows", "degree", pack([(j % 7 + 3, cycle(j % 7 + 3)) for j in range(17)], 9), 2, None,
             ("group_16", "k_9", "rows_plus1_g16", "labels_all_equal")),
        Case("k16_16rows", "degree", pack(k16, 16), 3, None,
             ("k_16", "rows_fill_block", "labels_ties_and_distinct", "count_1", "final_many")),
        Case("g32_9rows", "degree", pack([STRING_ORDER, DEG1_STRADDLE, (8, both(star(7)))] + [(j, both(path(j))) for j in range(2, 8)], 17),
             1, None, ("group_32", "k_17", "rows_plus1_g32", "string_order_differs", "deg_2digit", "deg1.word_straddle",
                       "deg1.word_complete", "deg1.flush_nothing")),
        Case("k32_complete", "degree", pack([(32, complete(32)), (32, complete(32) + [(0, 0)])], 32), 1, None,
             ("k_32", "deg_33", "loop_counts_twice", "count_2digit", "count_32", "edges_second_trip")),
        Case("edge_forms", "degree", pack([(5, []), (4, [(0, 1), (0, 1), (1, 2)]), (4, [(0, 1), (1, 0), (2, 3)]), (3, [(0, 0), (0, 1)])], 5),
             2, None, ("edges_none", "edge_duplicate", "edge_reversed", "edge_loop", "deg_0", "deg_1digit")),
        Case("bad_endpoints", "degree", pack([GOOD5[0], (3, [(0, 1), (-1, 2)]), GOOD5[1], (3, [(0, 1), (1, 3)]), GOOD5[2],
                                              (4, [(0, 1), ((1 << 32) + 1, 2)]), GOOD5[3]], 5), 1, None,
             ("endpoint_minus1", "endpoint_eq_n", "endpoint_ge_2_32", "status2_between_ok")),
        # ranges [0,2) [2,1) [1,3) [3,-1) [-1,3) [3,5) [5,99) [99,4) [4,6) and [6,7) on a row without vertices; 6 columns
        Case("bad_edge_ptr", "degree", pack([(3, [(0, 1), (1, 2)]), (3, [(0, 2), (0, 1)]), (3, [(1, 2), (0, 2)])] + [(3, [])] * 6 + [(0, [])],
                                             4, ptr=[0, 2, 1, 3, -1, 3, 5, 99, 4, 6, 7]), 1, None,
             ("ptr_lo_negative", "ptr_hi_lt_lo", "ptr_hi_gt_cols", "ptr_bad_row_empty")),
        Case("iter0", "degree", pack([(3, [(0, 1)]), (0, []), (1, [])], 3), 0, None, ("iter_0", "final_0_items", "final.finish_one_word")),
        Case("iter8_final_exact", "degree", pack(list(found_rows(8, 16, 8, ("final.finish_exact_3plus",))), 16), 8, None,
             ("iter_8", "final.finish_exact_3plus")),
        Case("later_blocks", "degree", pack(LATER_BLOCKS, 12), 2, None,
             ("later.opens_block", "later.flush_nothing", "later.finish_exact_1", "later.finish_exact_2", "later.finish_exact_3plus")),
        Case("final_stream", "degree", pack(list(found_rows(3, 8, 3, FINAL_STREAM)), 8), 3, None, FINAL_STREAM),
        Case("label_values", "labels", pack([([0, -1, 1, -1, 2, 3], both(path(4))), ([4, 4, 5], both(path(3))), ([6, 7, 0, 2, 1, 3], both(cycle(6))),
                                             ([-1, -1, 5], [])], 6), 2, LABELS8,
             ("label_0", "label_ffffffff", "label_top_bit", "label_leading_zero", "holes", "dup_ids", "labels_all_distinct")),
        Case("label_refusals", "labels", pack([([0, 3], [(0, 1)]), ([4, 0], [(0, 1)]), ([3, 0], [(0, 1)]), ([1, 0], [(0, 1)]), ([0], []),
                                               ([-1, 2], []), ([3, 3, 0], both(path(3))), ([4, 0], [(0, 2)]), ([0, 3], [])], 4), 1,
             [5, -1, 1 << 32, 9], ("id_eq_num_labels", "label_minus1", "label_2_32", "bad_endpoint_and_bad_id")),
        Case("label_table_empty", "labels", pack([([0, 1], [(0, 1)]), ([], []), ([-1, 0], [])], 3), 1, [], ("num_labels_0",)),
        Case("label_blocks", "labels", pack([(list(range(32)), complete(32)), (list(range(32, 48)), complete(16)), ([63], [])], 32), 1, LABELS64,
             ("lab1.opens_block", "lab1.flush_nothing", "lab1.finish_exact_1", "lab1.finish_exact_2", "lab1.finish_one_word")),
        Case("lookup_empty", "lookup", ({}, [one, "%032x" % 0, one], [0, 0, 1]), None, None, ("table_empty",)),
        Case("lookup_one", "lookup", ({one: 4}, [one, "%032x" % (9 << 64 | 8), "%032x" % (9 << 64 | 10), one], [0, 0, 0, 2]), None, None,
             ("table_one", "miss_below", "miss_above")),
        Case("lookup_17", "lookup", lookup_17(), None, None,
             ("table_not_pow2", "hit_first", "hit_last", "miss_between", "eqhi_hit_lower", "eqhi_hit_upper", "eqhi_miss_between",
              "hi_top_bit", "lo_top_bit", "status_1_in_table", "status_2_in_table", "status_3_in_table")),
        Case("lookup_16", "lookup", lookup_16(), None, None, ("table_pow2",)),
    )


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def census_of(name):
    c = case(name)
    if c.form == "lookup":
        vocab, digests, statuses = c.arrays
        return frozenset(L.lookup_census([int(x, 16) for x in vocab], [int(d, 16) for d in digests], statuses))
    return frozenset(L.census(*c.arrays, c.iterations, c.labels))


@functools.lru_cache(maxsize=None)
def law_of(name):
    """(hexdigests, statuses) of a hash case, ids of a lookup case: hashlib and a dict, nothing else."""
    c = case(name)
    if c.form == "lookup":
        vocab, digests, statuses = c.arrays
        return L.ids_from(digests, statuses, vocab)
    if c.form == "labels":
        return FL.wl_feature_rows(*c.arrays, c.labels, c.iterations)[:2]
    return L.wl_rows(*c.arrays, c.iterations)[:2]


# a compact width list for ugs_wl_feature_labels: between them the widths reach every class of wl_law.md5_census when the rows
# sit at an odd row stride (row addresses of every residue mod 4 in one launch)
MD5_WIDTHS = (0, 1, 2, 3, 55, 56, 63, 64)
MD5_ROWS = 5
