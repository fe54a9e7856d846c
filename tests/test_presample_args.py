"""CPU (no GPU needed): the argument handling of sample_graphs and PresampleCache(sampler=...)."""
import numpy as np
import pytest
import torch

M64 = (1 << 64) - 1


def test_seeds_are_taken_mod_2_64_from_sequences_and_tensors():
    from ugs_sampler._graphs import seed_array
    want = np.array([0, M64, 42, (1 << 63)], np.uint64)
    assert np.array_equal(seed_array([0, -1, 42 + (1 << 64), 1 << 63], 4), want)
    assert np.array_equal(seed_array(torch.tensor([0, -1, 42, -(1 << 63)], dtype=torch.int64), 4), want)
    assert np.array_equal(seed_array(np.array([0, M64, 42, 1 << 63], np.uint64), 4), want)
    with pytest.raises(RuntimeError):
        seed_array([1, 2], 3)
    with pytest.raises(RuntimeError):
        seed_array(torch.tensor([1.0, 2.0]), 2)


def test_presample_cache_names_its_sampler():
    from ugs_sampler.presample import PresampleCache
    for s in ("ugs", "uniform", "rwr"):
        c = PresampleCache(4, 3, "cpu", sampler=s)
        assert c.sampler == s and c.failed == set()
    assert PresampleCache(4, 3, "cpu").sampler == "ugs"
    with pytest.raises(ValueError):
        PresampleCache(4, 3, "cpu", sampler="epsilon")


def test_sample_graphs_is_exported():
    import rwr_sampler
    import uniform_sampler
    assert "sample_graphs" in uniform_sampler.__all__ and "sample_graphs" in rwr_sampler.__all__
