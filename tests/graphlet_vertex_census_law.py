"""The law of ugs_graphlet_vertex_census (include/ugs_mi355.h) in numpy: the exact k-graphlet degree vector of every vertex of a batch.
A helper for the tests, not a test.  Nothing here imports torch or the library.

  1. population: S_g = every connected k-subset of graph g -- uniform_enum_law.subsets, as in graphlet_census_law;
  2. orbit of a member: its rooted code among the rooted codes of the set's induced graph -- graphlet_orbit_law.rooted_codes, the
     minimum over the (k - 1)! orders that put the member last, by brute force; the set's class is the smallest of them;
  3. columns: the classes are the ascending keys of the connected graphs on exactly k vertices, class c owns widths[c] columns from
     base[c] on (its orbits by ascending rooted code), and a member's column is base[class] + graphlet_orbit_law.local_indices.
"""
from functools import lru_cache

import numpy as np

import graphlet_census_law as C
import graphlet_law as G
import graphlet_orbit_law as O
import uniform_enum_law as E
import uniform_law as U

CONNECTED_ORBITS = (1, 1, 3, 11, 58, 407, 4306)         # orbits of the connected graphs on exactly k vertices, k = 1 .. 7


def layout(k, columns=None, widths=None):
    """(class keys, base [W + 1]): the ascending keys of the connected graphs on k vertices (default: by brute force, k <= 6) and the
    exclusive prefix sum of their numbers of orbits (default: by brute force over each key's rooted codes)."""
    columns = _connected_keys(k) if columns is None else [int(c) for c in columns]
    widths = O.orbit_counts(columns) if widths is None else [int(w) for w in widths]
    return columns, np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(widths, np.int64))])


@lru_cache(maxsize=None)
def _connected_keys(k):
    return C.connected_keys(k)


def member_columns(code, k, at, base):
    """The column of each of the k vertices of the graph `code`, vertex i at position i."""
    rooted = O.rooted_codes(code, k)
    c = at[(k << 28) | min(rooted)]                                             # KeyError: a connected set outside the classes
    assert len(set(rooted)) == base[c + 1] - base[c]
    return [int(base[c]) + l for l in O.local_indices(rooted)]


def vertex_census(edge_index, ptr, k, columns=None, widths=None, failed=(), how="auto"):
    """gdv int64 [ptr[-1], O].  `columns`, `widths`: see layout (handed in for k = 7).  `failed`: graphs whose vertices have zero rows."""
    columns, base = layout(k, columns, widths)
    at = {key: c for c, key in enumerate(columns)}
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    out = np.zeros((int(ptr[-1]), int(base[-1])), np.int64)
    for g in range(len(ptr) - 1):
        if g in failed:
            continue
        lo = int(ptr[g])
        adj = U.graph_adjacency(ei[0], ei[1], lo, int(ptr[g + 1]) - lo)
        adj = [a & ~(1 << v) for v, a in enumerate(adj)]                        # a loop joins nothing
        for row in E.subsets(adj, k, how).tolist():
            for u, col in zip(row, member_columns(C.induced_code(adj, row), k, at, base)):
                out[lo + u, col] += 1
    return out


def column_of(k, graph, vertex, columns=None, widths=None):
    """The column of `vertex` of the k-vertex graph (n, edges)."""
    columns, base = layout(k, columns, widths)
    return member_columns(G.code_of_edges(*graph), k, {key: c for c, key in enumerate(columns)}, base)[vertex]


def orbit_sizes(k, columns=None, widths=None):
    """(size int64 [O], class int64 [O]): how many vertices of its class's representative each column's orbit holds, and the class
    column it belongs to.  Identity 5: the sum of gdv[:, c] over a graph's vertices = size[c] * census[g, class[c]]."""
    columns, base = layout(k, columns, widths)
    size, cls = np.zeros(int(base[-1]), np.int64), np.zeros(int(base[-1]), np.int64)
    for c, key in enumerate(columns):
        for l in O.local_indices(O.rooted_codes(key & ((1 << 28) - 1), k)):
            size[base[c] + l] += 1
        cls[base[c]:base[c + 1]] = c
    return size, cls


def graph_sums(gdv, ptr):
    """int64 [G, O]: gdv summed over the vertices of each graph."""
    return np.stack([gdv[int(ptr[g]):int(ptr[g + 1])].sum(axis=0) for g in range(len(ptr) - 1)]) if len(ptr) > 1 else gdv[:0]
