"""eps_cache_cases.py -- what the tests of epsilon_uniform_sampler.GraphCache share (tests/test_eps_cache_law.py on the CPU,
tests/test_gpu_eps_cache.py on the GPU): the graphs that pin the build kernel's row order, batches put together the way a collate
function would, a batch taken apart into the graphs a dataset would hold, and the rows the uncached call builds on the host
(csrc/ugs_side_eps.cpp, eps_begin) restated from oracle/eps_oracle.py."""
import random

import numpy as np

import eps_oracle
import ugs_workloads as wl


def cols_of(pairs):
    return np.array(pairs, np.int64).reshape(-1, 2).T.copy()


def _star70():
    """centre 0 with 70 columns, alternately as source and as destination: its row runs across two 64-column chunks"""
    return cols_of([(0, 1 + t % 12) if t % 2 else (1 + t % 12, 0) for t in range(70)])


def _random130():
    """130 columns over 9 vertices in random order, loops and repeats among them: every 64-column chunk holds several vertices and
    every vertex's row runs over all three chunks"""
    rng = np.random.default_rng(130)
    a = rng.integers(0, 9, size=(2, 130))
    for v in range(9):                                                  # (pinned below: test_eps_cache_law checks it)
        a[0, 7 * v] = v
    return np.ascontiguousarray(a.astype(np.int64))


# name -> (n, columns [2, E]): the graphs of the build-order test
BUILD_GRAPHS = {
    "path4": (4, cols_of([(0, 1), (1, 2), (2, 3)])),
    "triangle_dup_reversed": (3, cols_of([(0, 1), (1, 2), (2, 0), (0, 1), (2, 1)])),        # (0, 1) again, and (1, 2) turned round
    "loop_among_columns": (4, cols_of([(0, 1), (1, 1), (1, 2), (3, 1), (1, 1), (2, 3)])),   # loop columns on vertex 1
    "isolated_vertices": (7, cols_of([(1, 4), (4, 5), (5, 1)])),                            # 0, 2, 3 and 6 have empty rows
    "no_columns": (5, np.zeros((2, 0), np.int64)),
    "zero_vertices": (0, np.zeros((2, 0), np.int64)),
    "star70": (13, _star70()),
    "random130": (9, _random130()),
}


def rows_of(n, cols):
    """(rowptr [n + 1], nbr, ecs) as eps_begin lays a graph out: for every column j = (u, v), in order, row u gets (v, 2 j) and then
    row v gets (u, 2 j + 1).  The neighbour lists are checked against eps_oracle.adjacency, whose order this is."""
    nb, ec = [[] for _ in range(n)], [[] for _ in range(n)]
    for j, (u, v) in enumerate(np.asarray(cols).T.tolist()):
        nb[u].append(v)
        ec[u].append(2 * j)
        nb[v].append(u)
        ec[v].append(2 * j + 1)
    assert nb == eps_oracle.adjacency(np.asarray(cols).T.tolist(), n)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in nb], out=rowptr[1:])
    return rowptr, np.array([x for r in nb for x in r], np.int32), np.array([x for r in ec for x in r], np.int32)


def batch_of(graphs, first=0):
    """[(n, columns)] collated: (edge_index [2, E], ptr [G + 1]) with ptr[0] = first"""
    ptr = np.zeros(len(graphs) + 1, np.int64)
    ptr[0] = first
    for g, (n, _) in enumerate(graphs):
        ptr[g + 1] = ptr[g] + n
    parts = [np.asarray(a, np.int64).reshape(2, -1) + ptr[g] for g, (_, a) in enumerate(graphs)]
    ei = np.concatenate(parts, axis=1) if parts else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), ptr


def coff_of(graphs):
    """prefix sums of the graphs' column counts: coff[g] = the batch column of graph g's column 0"""
    c = np.zeros(len(graphs) + 1, np.int64)
    np.cumsum([a.shape[1] for _, a in graphs], out=c[1:])
    return c


def split(ei, ptr):
    """Each graph's own columns, local vertex ids, in batch order: [(n, columns [2, E_g])].  A column belongs to the graph whose
    vertex range holds both its endpoints (assign_columns of the uncached call); any other column is dropped."""
    ei, ptr = np.asarray(ei, np.int64).reshape(2, -1), np.asarray(ptr, np.int64)
    out = []
    for g in range(len(ptr) - 1):
        lo, hi = ptr[g], ptr[g + 1]
        keep = (ei[0] >= lo) & (ei[0] < hi) & (ei[1] >= lo) & (ei[1] < hi)
        out.append((int(hi - lo), np.ascontiguousarray(ei[:, keep] - lo)))
    return out


def regrouped(ei, ptr):
    """The batch of the same graphs collated again: every graph's own columns together, graphs in order, same ptr."""
    out = batch_of(split(ei, ptr), first=int(np.asarray(ptr)[0]))
    assert np.array_equal(out[1], ptr)
    return out


def tu(n, und, seed):
    return n, wl.tu_graph(n, und, seed)


def mixed_graphs():
    """The batch of the offsets-and-order test: TU-shaped graphs, a graph with fewer vertices than any k used (rows of -1), a graph
    without columns, and the loop and duplicate graphs of the build test."""
    return [tu(12, 15, 1), BUILD_GRAPHS["loop_among_columns"], tu(9, 12, 2), (2, cols_of([(0, 1), (1, 0)])), BUILD_GRAPHS["no_columns"],
            BUILD_GRAPHS["triangle_dup_reversed"], tu(17, 24, 3), BUILD_GRAPHS["random130"]]


def path_among_isolated():
    """One 5-path among 1695 isolated vertices (the shape of tests/test_gpu_eps_rows.py, test_epsilon_values_and_failing_rows): at
    k = 5 an attempt succeeds only if it starts on the path, 0.3 % of them, and is then accepted almost surely (its weight is far
    below any epsilon used).  So epsilon = 1.0 (10 attempts) leaves about 3 % of the rows successful and epsilon = 0.01 (1000
    attempts) about 5 % of them failed: both kinds of row at both values."""
    return 1700, cols_of([(60, 61), (61, 62), (62, 63), (63, 64)])


PATH_ROWS = 200                                                         # rows of such a call: a few rows of the rare kind at either epsilon


DUMMY = (-5, 7, cols_of([(0, 1), (1, 2), (2, 3), (3, 4), (1, 0)]))     # (dataset index, n, columns) of the graph added first


def dataset_index(g):
    """The dataset index the tests give the graph at batch position g: never the position itself"""
    return 1000 + 3 * g


def adding_order(G, seed):
    """Batch positions in the order the tests add them: not the batch's own order (for G > 1)"""
    order = list(range(G))
    random.Random(seed).shuffle(order)
    if G > 1 and order == sorted(order):
        order.reverse()
    return order
