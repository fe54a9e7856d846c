"""The law of ugs_graphlet_census (include/ugs_mi355.h) in numpy: the exact k-graphlet histogram of every graph of a batch.  A helper
for the tests, not a test.  Nothing here imports torch or the library.

  1. population: S_g = every connected k-subset of graph g (columns with both endpoints in g's range, symmetrised, loops join
     nothing, duplicates collapse; none for n < k) -- uniform_enum_law.subsets, the definition the enumeration tests trust;
  2. class of a set: the key (k << 28) | canonical code of its induced simple graph -- graphlet_law.key_of, the minimum over all k!
     orders by brute force;
  3. columns: the ascending keys of the connected graphs on exactly k vertices; counts[g, c] = the sets of S_g with key columns[c].
"""
from collections import Counter

import numpy as np

import graphlet_law as G
import uniform_enum_law as E
import uniform_law as U

CONNECTED_ON = G.CONNECTED_ON                           # W for k = 1 .. 8


def induced_code(adj, members):
    """The adjacency code of the subgraph induced on `members` (local vertices, any order), member i at position i."""
    code = 0
    for j in range(1, len(members)):
        for i in range(j):
            if members[i] != members[j] and adj[members[i]] >> members[j] & 1:
                code |= 1 << G.bit(i, j)
    return code


def graph_census(adj, k, how="auto"):
    """Counter {key: number of sets} of one graph given by its neighbour bitmasks (uniform_law.graph_adjacency)."""
    adj = [a & ~(1 << v) for v, a in enumerate(adj)]                            # a loop joins nothing
    out = Counter()
    for row in E.subsets(adj, k, how).tolist():
        out[G.key_of(induced_code(adj, row), k)] += 1
    return out


def census_keys(edge_index, ptr, k, how="auto"):
    """[Counter {key: count} for g in batch order]."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    return [graph_census(U.graph_adjacency(ei[0], ei[1], int(ptr[g]), int(ptr[g + 1] - ptr[g])), k, how) for g in range(len(ptr) - 1)]


def connected_keys(k):
    """The columns by brute force over every code, k <= 6."""
    n = k
    codes = G.canonical_codes(np.arange(1 << (n * (n - 1) // 2)), n)
    return sorted((n << 28) | int(c) for c in set(codes.tolist()) if G.connected(int(c), n))


def census(edge_index, ptr, k, columns=None, failed=(), how="auto"):
    """counts int64 [G, W].  `columns`: the ascending keys of the connected graphs on k vertices (default: connected_keys(k), k <= 6);
    every set's key must be one of them.  `failed`: graphs whose row is zero."""
    columns = connected_keys(k) if columns is None else [int(c) for c in columns]
    at = {key: c for c, key in enumerate(columns)}
    per_graph = census_keys(edge_index, ptr, k, how)
    out = np.zeros((len(per_graph), len(columns)), np.int64)
    for g, counter in enumerate(per_graph):
        if g in failed:
            continue
        for key, n in counter.items():
            out[g, at[key]] = n                                                 # KeyError: a connected set outside the columns
    return out


def batch(graphs):
    """(edge_index [2, E], ptr [G+1]) of a list of (n, [(u, v), ...]) with local endpoints, columns in list order."""
    cols, ptr = [], [0]
    for n, es in graphs:
        cols += [(ptr[-1] + u, ptr[-1] + v) for u, v in es]
        ptr.append(ptr[-1] + n)
    ei = np.array(cols, np.int64).reshape(-1, 2).T if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


def clique(n):
    return n, [(u, v) for v in range(n) for u in range(v)]


def cycle(n):
    return n, [(u, (u + 1) % n) for u in range(n)]


def path(n):
    return n, [(u, u + 1) for u in range(n - 1)]


def star(n_leaves, centre=0):
    """K_{1, n_leaves} on n_leaves + 1 vertices with the given centre."""
    return n_leaves + 1, [(centre, u) for u in range(n_leaves + 1) if u != centre]


def bipartite(a, b):
    return a + b, [(u, a + v) for u in range(a) for v in range(b)]


def key_of_graph(n, edges):
    return G.key_of(G.code_of_edges(n, edges), n)
