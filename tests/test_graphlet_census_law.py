"""The numpy law of graphlets.census (tests/graphlet_census_law.py) against closed forms on small graphs, `connected_classes` against
`is_connected(table(k))` and the published counts, and the refusals of `census` that need no device.  No GPU: nothing here launches
a kernel."""
from math import comb

import numpy as np
import pytest
import torch

import graphlet_census_law as law

CONNECTED = (1, 1, 2, 6, 21, 112, 853, 11117)           # connected graphs on k vertices, k = 1 .. 8 (OEIS A001349)


def one_graph(graph, k):
    ei, ptr = law.batch([graph])
    return law.census_keys(ei, ptr, k)[0]


@pytest.mark.parametrize("n,k", [(5, 1), (5, 2), (6, 3), (7, 4), (7, 5), (8, 6), (8, 7), (9, 8)])
def test_clique_puts_every_subset_in_the_clique_column(n, k):
    assert one_graph(law.clique(n), k) == {law.key_of_graph(*law.clique(k)): comb(n, k)}


@pytest.mark.parametrize("n,k", [(5, 2), (6, 3), (7, 4), (9, 5), (9, 6), (9, 7), (10, 8)])
def test_cycle_gives_n_paths(n, k):
    assert one_graph(law.cycle(n), k) == {law.key_of_graph(*law.path(k)): n}


def test_cycle_of_k_vertices_is_one_cycle():
    assert one_graph(law.cycle(5), 5) == {law.key_of_graph(*law.cycle(5)): 1}


@pytest.mark.parametrize("leaves,k,centre", [(6, 2, 0), (6, 3, 6), (7, 4, 3), (7, 5, 0), (8, 6, 8), (8, 7, 0), (9, 8, 4)])
def test_star_gives_stars(leaves, k, centre):
    assert one_graph(law.star(leaves, centre), k) == {law.key_of_graph(*law.star(k - 1)): comb(leaves, k - 1)}


def test_population_rules():
    """n < k and a disconnected graph give nothing; loops join nothing, copies and reversed columns collapse; a column that crosses
    two graphs or lies outside every range belongs to none."""
    graphs = [(2, [(0, 1)]), (4, [(0, 1), (2, 3)]), (3, [(0, 1), (1, 0), (0, 1), (1, 1), (1, 2), (2, 2)]), (3, [(0, 1)])]
    ei, ptr = law.batch(graphs)
    ei = np.concatenate([ei, np.array([[1, 8, 40], [2, 9, 41]], np.int64)], axis=1)      # 1-2 and 8-9 cross graphs, 40-41 is outside
    got = law.census_keys(ei, ptr, 3)
    assert got == [{}, {}, {law.key_of_graph(*law.path(3)): 1}, {}]
    counts = law.census(ei, ptr, 3)
    assert counts.shape == (4, 2) and counts.sum(axis=1).tolist() == [0, 0, 1, 0]
    assert law.census(ei, ptr, 3, failed={2}).sum() == 0


def test_law_columns_and_mixed_graph():
    """A triangle with a tail at k = 3: two paths and one triangle, in the columns' order (the path's key is the smaller)."""
    cols = law.connected_keys(3)
    assert cols == sorted([law.key_of_graph(*law.path(3)), law.key_of_graph(*law.clique(3))])
    ei, ptr = law.batch([(4, [(0, 1), (1, 2), (0, 2), (2, 3)])])
    assert law.census(ei, ptr, 3).tolist() == [[2, 1]]
    assert [len(law.connected_keys(k)) for k in range(1, 6)] == list(CONNECTED[:5])


@pytest.mark.parametrize("k", range(1, 9))
def test_connected_classes(k):
    from ugs_sampler import graphlets
    ids = graphlets.connected_classes(k)
    assert ids.dtype == torch.int64 and ids.device.type == "cpu" and ids.numel() == CONNECTED[k - 1]
    keys = graphlets.table(k)
    want = torch.nonzero(graphlets.is_connected(keys) & ((keys >> 28) == k)).view(-1)
    assert torch.equal(ids, want)
    assert bool((ids[1:] > ids[:-1]).all())
    if k <= 5:
        assert keys[ids].tolist() == law.connected_keys(k)
    ids[0] = -1                                                                 # the caller's copy: the module keeps its own
    assert graphlets.connected_classes(k)[0] >= 0


def test_census_is_public():
    from ugs_sampler import graphlets
    assert "census" in graphlets.__all__ and "connected_classes" in graphlets.__all__


def test_refusals_without_a_device():
    from ugs_sampler import graphlets
    ei, ptr = torch.zeros((2, 0), dtype=torch.int64), torch.zeros((1,), dtype=torch.int64)
    for limit in (0, -1, (1 << 32) + 1):
        with pytest.raises(ValueError, match="limit"):
            graphlets.census(ei, ptr, 3, limit=limit)
    for k in (0, 9, -1):
        with pytest.raises(RuntimeError, match="1 <= k <= 8"):
            graphlets.census(ei, ptr, k)
        with pytest.raises(RuntimeError, match="1 <= k <= 8"):
            graphlets.connected_classes(k)
    with pytest.raises(TypeError):
        graphlets.census(ei, ptr, 3.0)
    with pytest.raises(TypeError):
        graphlets.census(ei.numpy(), ptr, 3)
    with pytest.raises(RuntimeError, match="int64"):
        graphlets.census(ei.to(torch.int32), ptr, 3)
