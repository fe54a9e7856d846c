"""eps_graphs_law.py -- TEST INFRASTRUCTURE: the law of epsilon_uniform_sampler.sample_graphs (one seed per graph), from eps_rows.py.

The law (include/ugs_mi355.h at ugs_eps_sample_graphs_begin): graph g's block of m rows equals the one-graph call on the same
edge_index with the pointer ptr[g:g+2] and seed seeds[g] -- row i of the block is row i of that call.  eps_rows.Batch restates
such a call row by row, with batch node ids and batch column indices, so the blocks only have to be put one after the other:
no generator code of its own here."""
import numpy as np

import eps_rows


def _graph(ei, ptr, g, m, k, epsilon, seeds, large=False):
    return eps_rows.Batch(ei, np.asarray(ptr)[g:g + 2], m, k, epsilon, int(seeds[g]), large=large)


def expected(ei, ptr, m, k, mode, seeds, epsilon):
    """the five outputs of sample_graphs(ei, ptr, m, k, seeds, mode, epsilon)"""
    G = len(ptr) - 1
    assert len(seeds) == G
    per_row = []
    for g in range(G):
        b = _graph(ei, ptr, g, m, k, epsilon, seeds)
        per_row += [b.row(i, mode) for i in range(m)]
    return eps_rows.assemble(per_row, k, G, m)


def expected_rows(ei, ptr, m, k, mode, seeds, epsilon, rows):
    """{row: (nodes [k], [(a, b, column)])} for chosen batch rows of a large call (one restated graph per graph touched)"""
    graphs, out = {}, {}
    for r in rows:
        g = int(r) // m
        if g not in graphs:
            graphs[g] = _graph(ei, ptr, g, m, k, epsilon, seeds)
        out[int(r)] = graphs[g].row(int(r) - g * m, mode)
    return out
