"""CPU (no GPU, no device call): epsilon_uniform_sampler.sample_graphs exists through every layer, PresampleCache names the sampler
as the configs do, and the law helper of the GPU tests (tests/eps_graphs_law.py) is itself held to eps_rows.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import eps_graphs_law as L
import eps_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAPHS = {
    # name: (n, columns)
    "house": (5, [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 4)]),
    "tailed_triangle_both_dirs": (5, [(0, 1), (1, 0), (1, 2), (2, 1), (2, 0), (0, 2), (2, 3), (3, 2), (3, 4), (4, 3)]),
    "loops_and_an_isolated_vertex": (7, [(0, 1), (1, 1), (1, 2), (2, 3), (3, 4), (4, 0), (2, 5), (5, 5), (1, 2)]),
}


def test_sample_graphs_is_exported():
    import epsilon_uniform_sampler as eps
    assert "sample_graphs" in eps.__all__ and "_sample_graphs" in eps.__all__ and "sample_batch" in eps.__all__
    assert callable(eps.sample_graphs) and callable(eps._sample_graphs)


def test_presample_cache_takes_the_configs_name_and_epsilon():
    from ugs_sampler.presample import SAMPLERS, PresampleCache
    c = PresampleCache(4, 3, "cpu", sampler="epsilon_uniform", epsilon=0.3)
    assert c.sampler == "epsilon_uniform" and c.epsilon == 0.3 and c.failed == set()
    assert PresampleCache(4, 3, "cpu", sampler="epsilon_uniform").epsilon == 0.1
    assert "epsilon_uniform" in SAMPLERS
    with pytest.raises(ValueError):
        PresampleCache(4, 3, "cpu", sampler="epsilon")
    # epsilon is a new keyword behind the existing parameters: positional calls mean what they meant
    d = PresampleCache(4, 3, "cpu", "rwr", 0.5, 100, 200)
    assert (d.sampler, d.p_restart, d.chunk_vertices, d.chunk_rows, d.epsilon) == ("rwr", 0.5, 100, 200, 0.1)


def test_the_c_entry_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ugs_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+ugs_eps_sample_graphs_begin\s*\(([^)]*)\)", code)
    assert m, "ugs_eps_sample_graphs_begin is not declared in include/ugs_mi355.h"
    args = " ".join(m.group(1).split())
    assert "const uint64_t *seeds" in args and "double epsilon" in args and "int32_t *graph_status" in args
    lib = ctypes.CDLL(os.path.join(ROOT, "ss-gnn_amd", "csrc", "libugs_mi355.so"))
    assert hasattr(lib, "ugs_eps_sample_graphs_begin")
    import ugs_sampler
    assert "ugs_eps_sample_graphs_begin" in ugs_sampler._lib.EXPORTS


def test_bad_epsilon_is_refused_before_any_work():
    import torch

    import epsilon_uniform_sampler as eps
    ei, ptr = torch.zeros((2, 0), dtype=torch.int64), torch.tensor([0, 3])
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"epsilon must be in \(0, 1\]"):
            eps.sample_graphs(ei, ptr, 2, 2, [1], epsilon=bad)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_law_on_a_one_graph_batch_is_sample_rows(name):
    n, cols = GRAPHS[name]
    ei = np.array(cols, dtype=np.int64).reshape(-1, 2).T + 4
    for k, epsilon, mode, seed in ((3, 0.3, "sample", 99), (4, 1.0, "global", (1 << 64) - 1), (2, 0.05, "sample", 0)):
        got = L.expected(ei, [4, 4 + n], 20, k, mode, [seed], epsilon)
        want = eps_rows.sample_rows(ei, [4, 4 + n], 20, k, mode, seed, epsilon)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a, b), (name, k, mode)
        rows = L.expected_rows(ei, [4, 4 + n], 20, k, mode, [seed], epsilon, [0, 7, 19])
        b = eps_rows.Batch(ei, [4, 4 + n], 20, k, epsilon, seed)
        assert rows == {r: b.row(r, mode) for r in (0, 7, 19)}


def test_law_blocks_are_keyed_by_the_graphs_seed_and_local_row():
    """two copies of one graph: the same seed gives the same block up to the offsets, whatever the position in the batch; a seed
    that differs only above bit 32 gives other rows"""
    n, cols = GRAPHS[sorted(GRAPHS)[0]]
    one = np.array(cols, dtype=np.int64).reshape(-1, 2).T
    E = one.shape[1]
    ei = np.concatenate([one, one + n], axis=1)
    ptr = [0, n, 2 * n]
    m, k = 40, 3
    lo, hi = 5, 5 + (1 << 32)
    same = L.expected(ei, ptr, m, k, "sample", [lo, lo], 0.3)
    a, b = same[2][m], same[2][2 * m]
    assert np.array_equal(same[0][:m], same[0][m:] - n) and np.array_equal(same[1][:, :a], same[1][:, a:b])
    assert np.array_equal(same[4][:a], same[4][a:b] - E) and np.array_equal(same[2][:m + 1], same[2][m:] - a)
    assert (same[0][:m] >= 0).any()
    other = L.expected(ei, ptr, m, k, "sample", [lo, hi], 0.3)
    assert np.array_equal(other[0][:m], same[0][:m])
    assert not np.array_equal(other[0][m:], same[0][m:]), "the high 32 bits of a graph's seed do not reach its rows"
