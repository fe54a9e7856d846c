"""The law of ugs_graphlet_canon (include/ugs_mi355.h) in numpy: the canonical code of a graph on n <= 8 vertices is the minimum of
its adjacency code over ALL n! permutations, by brute force.  A helper for the tests, not a test.  Nothing here imports torch or the
library.

Pair (i, j), i < j, sits at bit j(j-1)/2 + i.  `canonical_code` is vectorised over the permutations of one row; `canonical_codes`
over many rows of one n (it loops over the permutations instead, for the exhaustive n <= 6 checks)."""
import itertools
from functools import lru_cache

import numpy as np

STATUS_OK, STATUS_EMPTY, STATUS_BAD = 0, 1, 2
NUM_CLASSES = (1, 3, 7, 18, 52, 208, 1252, 13598)       # C_k: graphs on at most k vertices
GRAPHS_ON = (1, 2, 4, 11, 34, 156, 1044, 12346)         # graphs on exactly n vertices (OEIS A000088)
CONNECTED_ON = (1, 1, 2, 6, 21, 112, 853, 11117)        # connected ones (OEIS A001349)


def bit(i, j):
    i, j = min(i, j), max(i, j)
    return j * (j - 1) // 2 + i


def pairs(n):
    return [(i, j) for j in range(1, n) for i in range(j)]


@lru_cache(maxsize=None)
def _perms(n):
    return np.array(list(itertools.permutations(range(n))), dtype=np.int64).reshape(-1, n)


def code_of_edges(n, edges):
    """The adjacency code in the identity order of the SIMPLE graph of `edges`: loops dropped, copies collapsed."""
    c = 0
    for u, v in edges:
        if u != v:
            c |= 1 << bit(u, v)
    return c


def edges_of_code(code, n):
    return [(i, j) for i, j in pairs(n) if code >> bit(i, j) & 1]


def matrix(code, n):
    A = np.zeros((n, n), dtype=np.int64)
    for i, j in edges_of_code(code, n):
        A[i, j] = A[j, i] = 1
    return A


def canonical_code(code, n):
    """min over all n! permutations p of sum A[p(i), p(j)] << bit(i, j)."""
    if n <= 1:
        return 0
    A, P = matrix(code, n), _perms(n)
    total = np.zeros(len(P), dtype=np.int64)
    for i, j in pairs(n):
        total |= A[P[:, i], P[:, j]] << bit(i, j)
    return int(total.min())


def canonical_codes(codes, n):
    """canonical_code of every entry of the int array `codes`, all on n vertices."""
    codes = np.asarray(codes, dtype=np.int64)
    if n <= 1:
        return np.zeros_like(codes)
    best = np.full(codes.shape, 1 << 28, dtype=np.int64)
    pr = pairs(n)
    for p in itertools.permutations(range(n)):
        total = np.zeros_like(codes)
        for i, j in pr:
            total |= ((codes >> bit(p[i], p[j])) & 1) << bit(i, j)
        np.minimum(best, total, out=best)
    return best


def relabel(code, n, perm):
    """The code of the same graph with vertex v renamed perm[v]."""
    return code_of_edges(n, [(perm[i], perm[j]) for i, j in edges_of_code(code, n)])


def connected(code, n):
    A = matrix(code, n)
    seen, todo = {0}, [0]
    while todo:
        u = todo.pop()
        for v in range(n):
            if A[u, v] and v not in seen:
                seen.add(v)
                todo.append(v)
    return len(seen) == n


_cache = {}


def key_of(code, n):
    """(n << 28) | canonical code, remembered per (n, code): the tests ask for the same symmetric graphs many times."""
    if (n, code) not in _cache:
        _cache[n, code] = (n << 28) | canonical_code(code, n)
    return _cache[n, code]


def rows_law(nodes, edge_index, edge_ptr, num_cols=None):
    """The law over a sampler's three outputs: (keys, statuses), lists of int.  Items 1 and 2: n = entries >= 0; status 1 for n = 0;
    status 2 for an edge_ptr range outside [0, num_cols] (nothing of it is read) or an endpoint outside [0, n); key -1 for both."""
    num_cols = len(edge_index[0]) if num_cols is None else int(num_cols)
    keys, stats = [], []
    for r in range(len(nodes)):
        n = sum(1 for x in nodes[r] if int(x) >= 0)
        lo, hi = int(edge_ptr[r]), int(edge_ptr[r + 1])
        if n == 0:
            st = STATUS_EMPTY
        elif lo < 0 or hi < lo or hi > num_cols:
            st = STATUS_BAD
        else:
            es = [(int(a), int(b)) for a, b in zip(edge_index[0][lo:hi], edge_index[1][lo:hi])]
            st = STATUS_OK if all(0 <= a < n and 0 <= b < n for a, b in es) else STATUS_BAD
        keys.append(key_of(code_of_edges(n, es), n) if st == STATUS_OK else -1)
        stats.append(st)
    return keys, stats


def all_keys(k):
    """The ascending keys of all graphs on at most k vertices, k <= 6 (brute force over every code)."""
    out = []
    for n in range(1, k + 1):
        out += sorted({(n << 28) | int(c) for c in canonical_codes(np.arange(1 << (n * (n - 1) // 2)), n)})
    return out


def ids_from(keys, stats, table):
    """Class ids: the rank of the key in the ascending `table`, len(table) where status != 0."""
    rank = {int(t): i for i, t in enumerate(table)}
    return [rank[k] if st == STATUS_OK else len(table) for k, st in zip(keys, stats)]
