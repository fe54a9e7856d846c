"""Graphs of more than 1000 columns for the tests of the device batch pass with its column limit raised
(ugs_sampler.set_batch_pass_max_cols): above 1000 columns the reference's LRU key hashes every (columns / 500)-th column only
(include/cache.hpp:100-107), so two different graphs can share a key and the reference then samples from the cached one.

Everything here is regenerated from ugs_workloads by seeds and shapes: the fixture tests/golden/f17_large_graph_batches.npz
(tools/make_golden_large_graphs.py, from the reference module) stores those and the reference's five output tensors only."""
import os

import numpy as np

import ugs_workloads as wl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f17_large_graph_batches.npz")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
M = 4

# name -> (vertices, undirected edges, seed of ugs_workloads.tu_graph, variant); variant 1: column 1 replaced (below)
GRAPHS = {
    "a": (477, 1347, 1, 0),      # 2694 columns: the reference's key hashes columns 0, 5, 10, ...
    "b": (477, 1347, 1, 1),      # `a` with column 1 replaced: same key, other graph
    "c": (300, 550, 2, 0),       # 1100 columns, stride 2
    "d": (400, 900, 3, 0),       # 1800 columns, stride 3
    "e": (250, 700, 4, 0),       # 1400 columns, stride 2
}
# one process, one LRU history: (graphs of the batch, k, mode, seed)
CALLS = [
    (("a", "c"), 4, "sample", 42),
    (("b",), 4, "graph", 7),                 # meets a's entry under the shared key: sampled from `a`
    (("d", "a"), 6, "global", 0),
    (("e", "c", "d"), 4, "sample", -3),
    (("b", "e"), 6, "sample", 42),
    (("a",), 6, "graph", 99991),
    (("d",), 4, "global", 5),
    (("c", "b", "a"), 6, "sample", -(2 ** 31)),
]


def replace_column_1(ei, n):
    """`ei` with column 1 replaced by another in-range pair that is no self loop; every other column, and so every column a
    stride >= 2 hashes, stays"""
    out = ei.copy()
    u, v = int(ei[0, 1]), int(ei[1, 1])
    w = (v + 7) % n
    while w == u or w == v:
        w = (w + 1) % n
    out[1, 1] = w
    return out


def graph(name):
    """(vertices, edge_index [2, E] int64 in local ids)"""
    n, e, seed, variant = GRAPHS[name]
    ei = wl.tu_graph(n, e, seed)
    return n, (replace_column_1(ei, n) if variant else ei)


def assemble(graphs):
    """PyG-style batch of [(n, edge_index local)]: (edge_index int64 [2, E], ptr int64 [G + 1])"""
    cols, ptr = [], [0]
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, dtype=np.int64)


def calls():
    """[(edge_index, ptr, m, k, mode, seed)] of the fixture's history"""
    return [assemble([graph(g) for g in names]) + (M, k, mode, seed) for names, k, mode, seed in CALLS]


def fixture():
    """the reference's outputs, call by call: [{name: array}]; asserts that the stored seeds and shapes are the ones above"""
    z = np.load(GOLDEN)
    assert [tuple(int(x) for x in row) for row in z["graphs"]] == [GRAPHS[g] for g in sorted(GRAPHS)]
    assert [tuple(int(x) for x in row) for row in z["calls"]] == [(k, ("sample", "graph", "global").index(mode), seed, len(names)) for names, k, mode, seed in CALLS]
    assert z["call_graphs"].tobytes().decode() == " ".join("".join(names) for names, _, _, _ in CALLS)
    return [{nm: z[f"c{i}/{nm}"] for nm in NAMES} for i in range(len(CALLS))]
