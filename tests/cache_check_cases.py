"""cache_check_cases.py -- the inputs that pin the check of a cached call of ugs_sampler.GraphCache (ugs_store.hip: ugs_store_check_k)
and of rwr_sampler.GraphCache (ugs_rwr.hip: rwr_store_check), one list for both, shared by tests/test_cache_check_law.py (CPU: census,
model of both kernels, mutants) and tests/test_gpu_cache_checks.py.  No GPU and no product import here.

A case is a list of graphs (n, local columns), the batch they collate to, the same batch with some columns altered (`bad`) and the
graph the check must name.  The law is column-for-column equality, graph by graph: the smallest graph with a column that is not the
stored one is named (`law`).  `reaches` names the classes (CLASSES, computed by `census` from the inputs alone) the case is there
for.  `failed`: graphs that fail when rwr_sampler adds them (10 n k overflows the reference's int iteration limit): they keep
their column count and store nothing, the check skips their columns; such a case is for rwr_sampler only.

The model (`Model`) restates both kernels: the binary search over the column offsets -- each kernel has its own -- the stored column
of a batch column, and the comparison in 64 bits; MUTANTS are one-line slips of it:
  compare_32_bit           the batch's endpoint is narrowed to 32 bits before it is compared
  search_lower_neighbour   the search takes `coff[mid] < e`: a graph's first column goes to the graph before it
  search_upper_neighbour   the search takes `coff[mid] <= e + 1`: a graph's last column goes to the graph behind it
  names_largest            atomicMax in place of atomicMin
  skips_last_column        `e >= E - 1` leaves
"""
import collections
import functools

import numpy as np

import rwr_cache_cases as RC
import ugs_cache_cases as UC
import ugs_workloads as wl

Case = collections.namedtuple("Case", "name graphs ei ptr bad expect reaches failed")
BLOCK = 256                                     # STORE_BLOCK and RWR_BLOCK: one lane per batch column
K, M, SEED = 4, 3, 11                           # every case is sampled at this k, m and seed
OVERFLOW_N = 60_000_000                         # 10 n k > INT_MAX at k = 4
NONE = np.zeros((2, 0), np.int64)
ALIAS = 1 << 32

CLASSES = ("E_le_256", "E_gt_256", "bad_column_in_second_workgroup", "bad_column_is_last", "bad_column_first_of_its_graph",
           "bad_column_last_of_its_graph", "columnless_graph_first", "columnless_graph_between", "columnless_graph_last",
           "bad_graph_right_after_columnless", "G_eq_1", "ptr0_nonzero", "two_bad_graphs_smaller_named", "src_plus_2_to_32",
           "dst_minus_2_to_32", "endpoints_exchanged", "rwr_failed_graph_col0_negative")


def tu(n, e, seed):
    return n, wl.tu_graph(n, e, seed)


def collate(graphs, first=0):
    cols, ptr = [], [first]
    for n, a in graphs:
        cols.append(np.asarray(a, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    return np.ascontiguousarray(np.concatenate(cols + [NONE], axis=1)), np.array(ptr, np.int64)


def offsets(graphs):
    return np.concatenate([[0], np.cumsum([a.shape[1] for _, a in graphs])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, graphs, expect, reaches, alter, first=0, failed=()):
        ei, ptr = collate(graphs, first)
        bad = ei.copy()
        alter(bad, ei, ptr, offsets(graphs))
        for a in (ei, ptr, bad):
            a.setflags(write=False)
        out.append(Case(name, tuple(graphs), ei, ptr, bad, expect, tuple(reaches), tuple(failed)))

    def loop_at(g, e):
        """column e becomes a loop at the first vertex of graph g (no graph here has a loop)"""
        def alter(bad, ei, ptr, coff):
            bad[:, e if e >= 0 else ei.shape[1] + e] = ptr[g]
        return alter

    # ---- one graph, one workgroup: the last column of all
    add("one_graph_last_column", [tu(18, 20, 1)], 0, ["G_eq_1", "E_le_256", "bad_column_is_last", "bad_column_last_of_its_graph"], loop_at(0, -1))
    # ---- eight graphs of 40 columns, ptr[0] = 5: columns 256 ... 319 belong to the second workgroup
    eight = [tu(18, 20, 10 + g) for g in range(8)]
    add("second_workgroup_last_column", eight, 7, ["E_gt_256", "bad_column_in_second_workgroup", "bad_column_is_last", "ptr0_nonzero"],
        loop_at(7, -1), first=5)
    add("second_workgroup_first_of_graph", eight, 7, ["E_gt_256", "bad_column_in_second_workgroup", "bad_column_first_of_its_graph"],
        loop_at(7, 280))
    add("last_column_of_a_middle_graph", eight[:3], 1, ["bad_column_last_of_its_graph", "E_le_256"], loop_at(1, 79))
    # ---- graphs without a column: equal entries of coff in front, in the middle (two in a row) and at the end
    holes = [(3, NONE), tu(12, 14, 20), (0, NONE), (5, NONE), tu(14, 15, 21), (2, NONE)]
    add("right_after_columnless", holes, 4, ["columnless_graph_first", "columnless_graph_between", "columnless_graph_last",
                                             "bad_graph_right_after_columnless", "bad_column_first_of_its_graph"], loop_at(4, 28), first=2)
    add("first_column_of_all_after_columnless", holes, 1, ["columnless_graph_first", "bad_graph_right_after_columnless"], loop_at(1, 0))
    # ---- two graphs differ: the smaller is named, whichever workgroup finds it
    def two(bad, ei, ptr, coff):
        bad[:, 300] = ptr[7]
        bad[:, 50] = ptr[1]
    add("two_bad_graphs", eight, 1, ["two_bad_graphs_smaller_named", "E_gt_256", "bad_column_in_second_workgroup"], two, first=1)
    # ---- endpoints 2^32 away: the same low 32 bits as the stored column
    def src_up(bad, ei, ptr, coff):
        bad[0, 95] += ALIAS
    add("src_plus_2_to_32", eight[:4], 2, ["src_plus_2_to_32"], src_up, first=3)

    def both_away(bad, ei, ptr, coff):
        bad[0, 47] += ALIAS
        bad[1, 47] -= ALIAS
    add("src_plus_dst_minus_2_to_32", eight[:4], 1, ["src_plus_2_to_32", "dst_minus_2_to_32"], both_away)

    def turned(bad, ei, ptr, coff):
        bad[:, 101] = ei[::-1, 101]
    add("endpoints_exchanged", eight[:4], 2, ["endpoints_exchanged"], turned)
    # ---- rwr only: a graph that failed when it was added keeps two columns in the batch and none in the store
    over = [tu(12, 14, 30), (OVERFLOW_N, np.array([[0, 1], [1, 0]], np.int64)), tu(13, 15, 31)]
    add("rwr_failed_graph_ahead", over, 2, ["rwr_failed_graph_col0_negative", "bad_column_first_of_its_graph"], loop_at(2, 30), failed=(1,))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def bad_columns(c):
    return np.nonzero((c.ei != c.bad).any(axis=0))[0]


def graph_of(c, e):
    """the graph that owns batch column e: the one with coff[g] <= e < coff[g + 1]"""
    return int(np.searchsorted(offsets(c.graphs), e, side="right") - 1)


def law(c, ei):
    """The smallest graph with a column that is not the added graph's column at that place, shifted by ptr[g]; None: none.  A
    failed graph is not compared."""
    coff = offsets(c.graphs)
    for g, (n, a) in enumerate(c.graphs):
        if g not in c.failed and not np.array_equal(ei[:, coff[g]:coff[g + 1]] - c.ptr[g], a):
            return g
    return None


@functools.lru_cache(maxsize=None)
def census(name):
    c = case(name)
    coff, G, E = offsets(c.graphs), len(c.graphs), c.ei.shape[1]
    cols = np.diff(coff)
    bad = bad_columns(c)
    owners = sorted({graph_of(c, e) for e in bad} - set(c.failed))
    out = set()
    hit = lambda cls, cond=True: out.add(cls) if cond else None      # noqa: E731
    hit("E_le_256", E <= BLOCK)
    hit("E_gt_256", E > BLOCK)
    hit("bad_column_in_second_workgroup", (bad >= BLOCK).any())
    hit("bad_column_is_last", E - 1 in bad)
    hit("bad_column_first_of_its_graph", any(e == coff[graph_of(c, e)] for e in bad))
    hit("bad_column_last_of_its_graph", any(e == coff[graph_of(c, e) + 1] - 1 for e in bad))
    hit("columnless_graph_first", cols[0] == 0)
    hit("columnless_graph_last", cols[-1] == 0)
    hit("columnless_graph_between", G > 2 and (cols[1:-1] == 0).any())
    g0 = owners[0]
    hit("bad_graph_right_after_columnless", g0 > 0 and cols[g0 - 1] == 0 and coff[g0] in bad)
    hit("G_eq_1", G == 1)
    hit("ptr0_nonzero", c.ptr[0] != 0)
    hit("two_bad_graphs_smaller_named", len(owners) >= 2)
    up = (c.bad[0] == c.ei[0] + ALIAS)
    down = (c.bad[1] == c.ei[1] - ALIAS)
    hit("src_plus_2_to_32", (up & ((c.bad[1] == c.ei[1]) | down)).any())
    hit("dst_minus_2_to_32", (up & down).any())
    hit("endpoints_exchanged", any(c.ei[0, e] != c.ei[1, e] and np.array_equal(c.bad[:, e], c.ei[::-1, e]) for e in bad))
    hit("rwr_failed_graph_col0_negative", any(f < g0 and cols[f] > 0 for f in c.failed))
    return frozenset(out)


# ---- the model of the two kernels ----
MUTANTS = ("compare_32_bit", "search_lower_neighbour", "search_upper_neighbour", "names_largest", "skips_last_column")


class ModelFault(Exception):
    """the model read outside the store: on the device, memory that is not the cache's"""


def store_of(c, kind):
    """(the store's columns as a flat list of local pairs, col0 per graph of the case): the dummy graph first, then the graphs in
    the order the GPU test adds them; a failed graph stores nothing and has col0 = -1"""
    dummy = UC.DUMMY[1] if kind == "ugs" else RC.DUMMY[2]
    flat = list(zip(*dummy.tolist()))
    order = (UC if kind == "ugs" else RC).adding_order(len(c.graphs), len(c.graphs))
    col0 = [-1] * len(c.graphs)
    for g in order:
        if g in c.failed:
            continue
        col0[g] = len(flat)
        flat += list(zip(*c.graphs[g][1].tolist()))
    return flat, col0


def int32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def model(c, kind, ei, mutant=None):
    """first_bad as the kernel of `kind` ("ugs": ugs_store_check_k, "rwr": rwr_store_check) leaves it, None where the host reads
    a value above every g"""
    assert mutant is None or mutant in MUTANTS
    flat, col0 = store_of(c, kind)
    coff, G, E = offsets(c.graphs).tolist(), len(c.graphs), ei.shape[1]
    src, dst, base = ei[0].tolist(), ei[1].tolist(), c.ptr.tolist()

    def le(mid, e):
        if mutant == "search_lower_neighbour":
            return coff[mid] < e
        if mutant == "search_upper_neighbour":
            return coff[mid] <= e + 1
        return coff[mid] <= e

    first_bad = None
    for e in range(E):
        if mutant == "skips_last_column" and e >= E - 1:
            continue
        if kind == "ugs":
            lo, hi = 0, G                                           # invariant: coff[lo] <= e < coff[hi]
            while hi - lo > 1:
                mid = (lo + hi) >> 1
                if le(mid, e):
                    lo = mid
                else:
                    hi = mid
        else:
            lo, hi = 0, G - 1                                       # the last g with coff[g] <= e
            while lo < hi:
                mid = (lo + hi + 1) >> 1
                if le(mid, e):
                    lo = mid
                else:
                    hi = mid - 1
            if col0[lo] < 0:
                continue
        at = col0[lo] + e - coff[lo]
        if not 0 <= at < len(flat):
            raise ModelFault((e, lo, at))
        wx, wy = flat[at]
        du, dv = src[e] - base[lo], dst[e] - base[lo]
        if mutant == "compare_32_bit":
            du, dv = int32(du), int32(dv)
        if du != wx or dv != wy:
            first_bad = lo if first_bad is None else max(first_bad, lo) if mutant == "names_largest" else min(first_bad, lo)
    return first_bad
