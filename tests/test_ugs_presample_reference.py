"""CPU: the reference's presample loop (fixture f16: one-graph sample_batch calls in one process, k = 4 then k = 5) is what the
oracle's one-graph calls on one LRU give -- the right-hand side of the law of ugs_sampler.sample_graphs -- and the argument
checks of sample_graphs that need no GPU."""
import numpy as np
import pytest
import torch

import oracle
from ugs_graphs_law import NAMES, fixture


def test_oracle_one_graph_loop_reproduces_the_reference_presample_loop():
    graphs, seeds, m, want = fixture()
    assert len(graphs) >= 20 and 0 in seeds and min(seeds) < 0
    assert any(n == 0 for n, _ in graphs) and any(0 < n < 4 for n, _ in graphs)
    assert any(((ei < 0) | (ei >= n)).any() for n, ei in graphs if n > 0)
    cache = oracle.Cache()
    for k in (4, 5):                                 # one LRU for both passes: the k = 5 pass meets the k = 4 pass's entries
        for i, (n, ei) in enumerate(graphs):
            got = oracle.sample_batch(ei, np.array([0, n], np.int64), m, k, "sample", seeds[i], cache)
            for name, g, w in zip(NAMES, got, want[k][i]):
                assert np.array_equal(np.asarray(g), w), (k, i, name)
    st = cache.stats()
    assert st["hits"] > st["misses"] > 0             # the second pass and the repeated graph hit
    cache.close()


def test_sample_graphs_is_exported():
    import ugs_sampler
    assert "sample_graphs" in ugs_sampler.__all__ and callable(ugs_sampler.sample_graphs)


def _two_graphs():
    ei = torch.tensor([[0, 1, 2, 3, 4, 5], [1, 2, 0, 4, 5, 3]], dtype=torch.int64)
    return ei, torch.tensor([0, 3, 6], dtype=torch.int64)


@pytest.mark.parametrize("bad", [2 ** 31, -(2 ** 31) - 1, 2 ** 40])
@pytest.mark.parametrize("form", ["list", "tensor", "array"])
def test_a_seed_outside_c_int_raises_type_error_naming_the_graph(bad, form):
    import ugs_sampler
    ei, ptr = _two_graphs()
    seeds = [7, bad]
    if form == "tensor":
        seeds = torch.tensor(seeds, dtype=torch.int64)
    elif form == "array":
        seeds = np.array(seeds, np.int64)
    with pytest.raises(TypeError, match=r"seeds\[1\]"):
        ugs_sampler.sample_graphs(ei, ptr, 4, 3, seeds)
    with pytest.raises(TypeError, match=r"seeds\[0\]"):
        ugs_sampler.sample_graphs(ei, ptr, 4, 3, [1.5, 2])


@pytest.mark.parametrize("seeds", [[1], [1, 2, 3], torch.tensor([1], dtype=torch.int64), np.arange(3)])
def test_a_wrong_number_of_seeds_raises(seeds):
    import ugs_sampler
    ei, ptr = _two_graphs()
    with pytest.raises(RuntimeError, match="one seed per graph"):
        ugs_sampler.sample_graphs(ei, ptr, 4, 3, seeds)


def test_inputs_are_checked_like_sample_batch():
    import ugs_sampler
    ei, ptr = _two_graphs()
    with pytest.raises(RuntimeError, match="int64"):
        ugs_sampler.sample_graphs(ei.to(torch.int32), ptr, 4, 3, [1, 2])
    with pytest.raises(RuntimeError, match="mode must be"):
        ugs_sampler.sample_graphs(ei, ptr, 4, 3, [1, 2], mode="local")
    with pytest.raises(RuntimeError, match="int64 tensor"):
        ugs_sampler.sample_graphs(ei, ptr, 4, 3, torch.tensor([1, 2], dtype=torch.int32))
