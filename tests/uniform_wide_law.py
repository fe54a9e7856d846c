"""uniform_wide_law.py -- the law of tests/uniform_law.py for graphs of more than 64 vertices, and the wide key of the HIP product
(include/ugs_mi355.h, ugs_uniform_sample_batch_begin: "Representation").

Nothing of the law changes with the size of a graph: S_g is the connected k-subsets in lexicographic order of their ascending
tuples.  `sorted_tuples` enumerates them with uniform_law.esu_masks (Python ints: no 64-bit limit) and sorts the tuples;
`uniform_law.sample_batch(..., enumerate_fn=sorted_tuples)` is the sampler.  `tuple_key` is the product's sort key of a set."""
import numpy as np

import uniform_law as U


def mask_tuple(mask):
    out = []
    while mask:
        low = mask & -mask
        out.append(low.bit_length() - 1)
        mask ^= low
    return tuple(out)


def sorted_tuples(adj, k):
    """S_g as a list of ascending tuples in lexicographic order, any number of vertices."""
    return sorted(mask_tuple(x) for x in U.esu_masks(adj, k))


def field_bits(n):
    """b: the bit length of n - 1"""
    return (n - 1).bit_length()


def tuple_key(t, n):
    """The ascending tuple packed big-endian in fields of b bits: ascending keys = lexicographic tuples (needs len(t) * b <= 64)."""
    b, k = field_bits(n), len(t)
    assert k * b <= 64 and all(0 <= v < n for v in t)
    key = 0
    for i, v in enumerate(t):
        key |= v << (b * (k - 1 - i))
    return key


def takes_wide_form(n, k, limit):
    """The rule of the header: 64 < n <= limit, 1 <= k <= 8, k b <= 64."""
    return 64 < n <= limit and 1 <= k <= 8 and k * field_bits(n) <= 64


def sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42):
    return U.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed, enumerate_fn=sorted_tuples)


def batch(graphs, first=0):
    """Concatenates local edge_index arrays [(n, ei)] into a PyG batch starting at vertex `first`."""
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(np.asarray(ei, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)
