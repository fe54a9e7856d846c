"""The law of ugs_graphlet_orbits (include/ugs_mi355.h) in numpy, by brute force, on top of tests/graphlet_law.py.  A helper for the
tests, not a test.  Nothing here imports torch or the library.

The rooted code of vertex v is the minimum of the adjacency code over the permutations p with p[n - 1] = v: `rooted_codes` takes all
n of them from ONE pass over all n! permutations, grouped by p[n - 1].  `automorphism_orbits` finds the orbits a second way that
shares nothing with it: the permutations that preserve the adjacency matrix, their images joined.  `burnside_rooted` counts rooted
graphs from the cycle types of S_n, which is where the expected numbers of orbits come from."""
import itertools
from functools import lru_cache
from math import factorial, gcd

import numpy as np

import graphlet_law as law

ABOVE = 1 << 28                                         # above every code


@lru_cache(maxsize=None)
def rooted_codes(code, n):
    """tuple of the n rooted codes: [v] = min over the permutations p with p[n - 1] = v of sum A[p(i), p(j)] << bit(i, j)."""
    if n <= 1:
        return (0,) * n
    A, P = law.matrix(code, n), law._perms(n)
    total = np.zeros(len(P), dtype=np.int64)
    for i, j in law.pairs(n):
        total |= A[P[:, i], P[:, j]] << law.bit(i, j)
    best = np.full(n, ABOVE, dtype=np.int64)
    np.minimum.at(best, P[:, n - 1], total)
    return tuple(int(x) for x in best)


def local_indices(rooted):
    """Item 3: for every vertex the number of distinct rooted codes of the graph below its own."""
    distinct = sorted(set(rooted))
    return [distinct.index(c) for c in rooted]


def rooted_codes_many(codes, n):
    """rooted_codes of every entry of the int array `codes`, all on n vertices: int64 [len(codes), n].  Loops over the
    permutations instead, as graphlet_law.canonical_codes does, for the exhaustive n <= 6 checks."""
    codes = np.asarray(codes, dtype=np.int64)
    best = np.full((len(codes), max(n, 1)), ABOVE if n > 1 else 0, dtype=np.int64)
    pr = law.pairs(n)
    for p in (itertools.permutations(range(n)) if n > 1 else ()):
        total = np.zeros_like(codes)
        for i, j in pr:
            total |= ((codes >> law.bit(p[i], p[j])) & 1) << law.bit(i, j)
        np.minimum(best[:, p[n - 1]], total, out=best[:, p[n - 1]])
    return best


def local_indices_many(rooted):
    """local_indices of every row of the int array `rooted` [R, n]."""
    rooted = np.asarray(rooted, dtype=np.int64)
    first = np.ones(rooted.shape, dtype=bool)                                   # no earlier vertex has this code
    for v in range(rooted.shape[1]):
        for w in range(v):
            first[:, v] &= rooted[:, w] != rooted[:, v]
    return (first[:, None, :] & (rooted[:, None, :] < rooted[:, :, None])).sum(axis=2)


def automorphism_orbits(code, n):
    """[v] = the smallest vertex an automorphism maps v to.  The automorphisms are all permutations p with A[p(i), p(j)] = A[i, j];
    they form a group, so the images of v under all of them are v's orbit -- the union of v ~ p(v) over every one of them."""
    A, P = law.matrix(code, n), law._perms(n)
    keeps = (A[P[:, :, None], P[:, None, :]] == A[None]).all(axis=(1, 2))
    assert keeps[0]                                      # the identity comes first
    return [int(x) for x in P[keeps].min(axis=0)]


def rows_law(nodes, edge_index, edge_ptr, num_cols=None):
    """(keys, statuses, local): keys and statuses as graphlet_law.rows_law; local[r][s] is the local orbit index of the vertex that
    slot s of row r is -- vertex j being the j-th entry >= 0 in row order (item 1) -- and -1 where the entry is < 0 or the row's
    status is not 0."""
    keys, stats = law.rows_law(nodes, edge_index, edge_ptr, num_cols)
    local = []
    for r in range(len(nodes)):
        out = [-1] * len(nodes[r])
        if stats[r] == law.STATUS_OK:
            n = sum(1 for x in nodes[r] if int(x) >= 0)
            lo, hi = int(edge_ptr[r]), int(edge_ptr[r + 1])
            es = [(int(a), int(b)) for a, b in zip(edge_index[0][lo:hi], edge_index[1][lo:hi])]
            idx = local_indices(rooted_codes(law.code_of_edges(n, es), n))
            j = 0
            for s, x in enumerate(nodes[r]):
                if int(x) >= 0:
                    out[s] = idx[j]
                    j += 1
        local.append(out)
    return keys, stats, local


def orbit_ids_from(keys, stats, local, table, base):
    """Item 4 and 5: base[rank of the key in table] + local index; base[len(table)] where there is no vertex."""
    rank = {int(t): i for i, t in enumerate(table)}
    fill = int(base[len(table)])
    return [[int(base[rank[k]]) + x if st == law.STATUS_OK and x >= 0 else fill for x in row] for k, st, row in zip(keys, stats, local)]


def orbit_counts(keys):
    """The number of orbits of every key of the list, by the brute force."""
    return [len(set(rooted_codes(int(k) & (ABOVE - 1), int(k) >> 28))) for k in keys]


def _partitions(n, largest=None):
    largest = n if largest is None else largest
    if n == 0:
        yield ()
        return
    for first in range(min(n, largest), 0, -1):
        for rest in _partitions(n - first, first):
            yield (first,) + rest


def _burnside(n, rooted):
    """Orbits of S_n on the graphs on n labelled vertices (rooted: on the pairs of a graph and one of its vertices): the mean over
    the permutations of 2^(cycles on the vertex pairs), times the number of fixed vertices if rooted, summed by cycle type."""
    total = 0
    for lam in _partitions(n):
        perms = factorial(n)
        for length in set(lam):
            m = lam.count(length)
            perms //= length ** m * factorial(m)
        pair_cycles = sum(length // 2 for length in lam) + sum(gcd(lam[a], lam[b]) for a in range(len(lam)) for b in range(a))
        total += perms * (lam.count(1) if rooted else 1) * 2 ** pair_cycles
    assert total % factorial(n) == 0
    return total // factorial(n)


def burnside_rooted(nmax):
    """(total, connected): lists over n = 1 .. nmax of the number of rooted graphs on n vertices and of the connected ones.  A rooted
    graph is the root's component, a connected rooted graph on m vertices, beside any graph on the other n - m vertices."""
    graphs = [1] + [_burnside(n, False) for n in range(1, nmax + 1)]            # [0] = the empty rest
    total = [_burnside(n, True) for n in range(1, nmax + 1)]
    conn = []
    for n in range(1, nmax + 1):
        conn.append(total[n - 1] - sum(conn[m - 1] * graphs[n - m] for m in range(1, n)))
    return total, conn
