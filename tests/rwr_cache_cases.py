"""rwr_cache_cases.py -- what the tests of rwr_sampler.GraphCache share (tests/test_rwr_cache_law.py on the CPU,
tests/test_gpu_rwr_cache.py on the GPU): a batch taken apart into the graphs a dataset would hold, and put together again the
way a collate function would."""
import random

import numpy as np

import rwr_paths as P


def split(ei, ptr):
    """Each graph's kept columns, local vertex ids, in batch order: [(n, columns [2, E_g])].  A column is kept by the graph whose
    vertex range holds both its endpoints (point 1 of the law at ugs_rwr_sample_batch_begin); any other column is dropped."""
    ei, ptr = np.asarray(ei, np.int64).reshape(2, -1), np.asarray(ptr, np.int64)
    G = len(ptr) - 1
    if G == 0:
        return []
    u, v = ei
    g = np.searchsorted(ptr[1:], u, side="right")                   # the graph with ptr[g] <= u < ptr[g + 1], empty graphs skipped
    gc = np.minimum(g, G - 1)
    kept = (g < G) & (u >= ptr[gc]) & (v >= ptr[gc]) & (v < ptr[gc + 1])
    return [(int(ptr[i + 1] - ptr[i]), np.ascontiguousarray(ei[:, kept & (gc == i)] - ptr[i])) for i in range(G)]


def regrouped(ei, ptr):
    """The batch of the same graphs collated again: every graph's kept columns together, graphs in order, same ptr."""
    out = P.batch_of(split(ei, ptr), first=int(ptr[0]))
    assert np.array_equal(out[1], ptr)
    return out


DUMMY = (-5, 7, np.array([[0, 1, 2, 3, 1], [1, 2, 3, 4, 0]], np.int64))     # (dataset index, n, columns) of the graph added first


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
