"""The law of ugs_graphlet_labelled (include/ugs_mi355.h) in numpy, by brute force, on top of tests/graphlet_law.py.  A helper for the
tests, not a test.  Nothing here imports torch or the library.

A permutation p is label-monotone if labels[p[i]] <= labels[p[j]] for all positions i < j.  `labelled_codes` takes the labelled
canonical code -- the minimum of the adjacency code over the label-monotone subset of all n! permutations -- and the n labelled rooted
codes -- the minima over the permutations whose first n - 1 positions are monotone, grouped by p[n - 1] -- from ONE pass.
`automorphism_orbits` finds the orbits a second way that shares nothing with it: the permutations that preserve the adjacency matrix
and the labels, their images joined.  `burnside_labelled` counts the L-labelled graphs on n vertices from the cycle types of S_n,
which is where the expected numbers of distinct keys come from."""
import itertools
from functools import lru_cache
from math import factorial, gcd

import numpy as np

import graphlet_law as law

ABOVE = 1 << 28                                         # above every code
LABEL_BITS = 12
STATUS_LABEL = 3


@lru_cache(maxsize=None)
def labelled_codes(code, n, labels):
    """(labelled canonical code, tuple of the n labelled rooted codes) of the graph `code` whose vertex v has labels[v] (a tuple)."""
    if n <= 1:
        return 0, (0,) * n
    A, P = law.matrix(code, n), law._perms(n)
    total = np.zeros(len(P), dtype=np.int64)
    for i, j in law.pairs(n):
        total |= A[P[:, i], P[:, j]] << law.bit(i, j)
    lab = np.array(labels, dtype=np.int64)[P]                                   # [n!, n]: the label at every position
    steps = lab[:, 1:] >= lab[:, :-1]
    mono, mono_rest = steps.all(axis=1), steps[:, :n - 2].all(axis=1)            # all n positions; all but the last
    best = np.full(n, ABOVE, dtype=np.int64)
    np.minimum.at(best, P[mono_rest, n - 1], total[mono_rest])
    return int(total[mono].min()), tuple(int(x) for x in best)


def labelled_codes_many(codes, labels, n):
    """labelled_codes of every row: codes int [R], labels int [R, n].  Returns (canonical [R], rooted [R, n]).  Loops over the
    permutations instead, as graphlet_law.canonical_codes does, for the exhaustive checks."""
    codes, labels = np.asarray(codes, dtype=np.int64), np.asarray(labels, dtype=np.int64).reshape(len(codes), n)
    best = np.full(codes.shape, ABOVE if n > 1 else 0, dtype=np.int64)
    rooted = np.full((len(codes), max(n, 1)), ABOVE if n > 1 else 0, dtype=np.int64)
    pr = law.pairs(n)
    for p in (itertools.permutations(range(n)) if n > 1 else ()):
        total = np.zeros_like(codes)
        for i, j in pr:
            total |= ((codes >> law.bit(p[i], p[j])) & 1) << law.bit(i, j)
        rest = np.ones(codes.shape, dtype=bool)
        for i in range(n - 2):
            rest &= labels[:, p[i]] <= labels[:, p[i + 1]]
        mono = rest & (labels[:, p[n - 2]] <= labels[:, p[n - 1]])
        best = np.where(mono & (total < best), total, best)
        col = rooted[:, p[n - 1]]
        rooted[:, p[n - 1]] = np.where(rest & (total < col), total, col)
    return best, rooted


def key_number(n, canon, labels):
    """Item 4: K = n 2^124 + code 2^96 + sum of L[p] 2^(12 p), L the labels sorted ascending.  A Python int."""
    return (n << 124) + (canon << 96) + sum(int(x) << (LABEL_BITS * p) for p, x in enumerate(sorted(labels)))


def key_words(K):
    """(K >> 64, K & (2^64 - 1)) as int64 bit patterns; (-1, -1) for K = -1, a row of status != 0."""
    if K < 0:
        return (-1, -1)
    return tuple(w - (1 << 64) if w >> 63 else w for w in (K >> 64, K & ((1 << 64) - 1)))


def key_of(code, n, labels):
    return key_number(n, labelled_codes(code, n, tuple(int(x) for x in labels))[0], labels)


def key_words_many(n, canon, labels):
    """key_words of every row, with numpy's 64-bit words: int64 [R, 2]."""
    L = np.zeros((len(canon), 8), dtype=np.uint64)
    L[:, :n] = np.sort(np.asarray(labels, dtype=np.int64).reshape(len(canon), n), axis=1).astype(np.uint64)
    lo = np.zeros(len(canon), dtype=np.uint64)
    for p in range(6):                                                           # L[5] << 60 keeps its low four bits
        lo |= L[:, p] << np.uint64(LABEL_BITS * p)
    hi = (np.uint64(n) << np.uint64(60)) | (np.asarray(canon).astype(np.uint64) << np.uint64(32))
    hi |= (L[:, 5] >> np.uint64(4)) | (L[:, 6] << np.uint64(8)) | (L[:, 7] << np.uint64(20))
    return np.stack([hi, lo], axis=1).view(np.int64)


def decode(K):
    """(n, code, sorted labels) of a key number: the bit fields of item 4."""
    n = K >> 124
    return n, (K >> 96) & (ABOVE - 1), [(K >> (LABEL_BITS * p)) & 4095 for p in range(n)]


def local_indices(labels, rooted):
    """Item 7: for every vertex the number of distinct (label, labelled rooted code) pairs of the row below its own."""
    pairs = list(zip((int(x) for x in labels), rooted))
    distinct = sorted(set(pairs))
    return [distinct.index(p) for p in pairs]


def local_indices_many(labels, rooted):
    """local_indices of every row of labels [R, n] (< 4096) and rooted [R, n]."""
    val = (np.asarray(labels, dtype=np.int64) << 28) | np.asarray(rooted, dtype=np.int64)
    first = np.ones(val.shape, dtype=bool)                                      # no earlier vertex has this pair
    for v in range(val.shape[1]):
        for w in range(v):
            first[:, v] &= val[:, w] != val[:, v]
    return (first[:, None, :] & (val[:, None, :] < val[:, :, None])).sum(axis=2)


def automorphisms(code, n):
    """All permutations p with A[p(i), p(j)] = A[i, j]: int [|Aut|, n], the identity first."""
    A, P = law.matrix(code, n), law._perms(n)
    keeps = (A[P[:, :, None], P[:, None, :]] == A[None]).all(axis=(1, 2))
    assert keeps[0]
    return P[keeps]


def automorphism_orbits(code, n, labels):
    """[v] = the smallest vertex a label-preserving automorphism maps v to.  They form a group, so the images of v under all of them
    are v's orbit."""
    auts = automorphisms(code, n)
    lab = np.array(labels, dtype=np.int64)
    auts = auts[(lab[auts] == lab[None]).all(axis=1)]
    return [int(x) for x in auts.min(axis=0)]


def same_labelled_graph(code, n, labels_a, labels_b):
    """Whether an automorphism p of the graph carries labelling a onto labelling b: labels_b[p(v)] = labels_a[v] for all v."""
    auts = automorphisms(code, n)
    a, b = np.array(labels_a, dtype=np.int64), np.array(labels_b, dtype=np.int64)
    return bool((b[auts] == a[None]).all(axis=1).any())


def relabel(code, n, labels, perm):
    """The same labelled graph with vertex v renamed perm[v]: (code, labels), the labels carried along."""
    out = [0] * n
    for v in range(n):
        out[perm[v]] = int(labels[v])
    return law.relabel(code, n, perm), out


def rows_law(nodes, edge_index, edge_ptr, node_labels, num_cols=None):
    """The law over a sampler's three outputs and the label vector: (key numbers, statuses, local).  Statuses 1 and 2 as
    graphlet_law.rows_law and before the labels are looked at; then status 3 for an entry >= len(node_labels) or a label outside
    [0, 4096).  The key number is -1 where the status is not 0.  local[r][s] is the local orbit index of the vertex that slot s of
    row r is -- vertex j being the j-th entry >= 0 in row order -- and k where the entry is < 0 or the row's status is not 0."""
    num_cols = len(edge_index[0]) if num_cols is None else int(num_cols)
    keys, stats, local = [], [], []
    for r in range(len(nodes)):
        k = len(nodes[r])
        ids = [int(x) for x in nodes[r] if int(x) >= 0]
        n = len(ids)
        lo, hi = int(edge_ptr[r]), int(edge_ptr[r + 1])
        if n == 0:
            st = law.STATUS_EMPTY
        elif lo < 0 or hi < lo or hi > num_cols:
            st = law.STATUS_BAD
        else:
            es = [(int(a), int(b)) for a, b in zip(edge_index[0][lo:hi], edge_index[1][lo:hi])]
            st = law.STATUS_OK if all(0 <= a < n and 0 <= b < n for a, b in es) else law.STATUS_BAD
        if st == law.STATUS_OK and not all(x < len(node_labels) and 0 <= int(node_labels[x]) < 4096 for x in ids):
            st = STATUS_LABEL
        out = [k] * k
        if st == law.STATUS_OK:
            labels = tuple(int(node_labels[x]) for x in ids)
            canon, rooted = labelled_codes(law.code_of_edges(n, es), n, labels)
            keys.append(key_number(n, canon, labels))
            idx = local_indices(labels, rooted)
            j = 0
            for s, x in enumerate(nodes[r]):
                if int(x) >= 0:
                    out[s] = idx[j]
                    j += 1
        else:
            keys.append(-1)
        stats.append(st)
        local.append(out)
    return keys, stats, local


def _partitions(n, largest=None):
    largest = n if largest is None else largest
    if n == 0:
        yield ()
        return
    for first in range(min(n, largest), 0, -1):
        for rest in _partitions(n - first, first):
            yield (first,) + rest


def burnside_labelled(n, num_labels):
    """The number of graphs on n vertices with one of num_labels labels on every vertex, up to label-preserving isomorphism: the mean
    over S_n of the fixed points 2^(cycles on the vertex pairs) * num_labels^(cycles on the vertices), summed by cycle type."""
    total = 0
    for lam in _partitions(n):
        perms = factorial(n)
        for length in set(lam):
            m = lam.count(length)
            perms //= length ** m * factorial(m)
        pair_cycles = sum(length // 2 for length in lam) + sum(gcd(lam[a], lam[b]) for a in range(len(lam)) for b in range(a))
        total += perms * 2 ** pair_cycles * num_labels ** len(lam)
    assert total % factorial(n) == 0
    return total // factorial(n)
