"""The numpy law of graphlets.vertex_census (tests/graphlet_vertex_census_law.py) against closed forms on small graphs, the host's table
entry (ugs_graphlet_vertex_census_entry, the code path of the device table) against tests/graphlet_orbit_law.py over every code of at
most 6 vertices, and the refusals of `vertex_census` that need no device.  No GPU: nothing here launches a kernel."""
import ctypes
from math import comb

import numpy as np
import pytest
import torch

import graphlet_census_law as census_law
import graphlet_orbit_law as orbit_law
import graphlet_vertex_census_law as law
import uniform_enum_law
import uniform_law

NONE = 0xFFFFFFFF


def one_graph(graph, k):
    ei, ptr = census_law.batch([graph])
    return law.vertex_census(ei, ptr, k)


def test_widths():
    assert [int(law.layout(k)[1][-1]) for k in range(1, 7)] == list(law.CONNECTED_ORBITS[:6])


@pytest.mark.parametrize("n,k", [(5, 1), (5, 2), (6, 3), (7, 4), (7, 5), (8, 6)])
def test_clique(n, k):
    gdv = one_graph(census_law.clique(n), k)
    want = np.zeros_like(gdv)
    want[:, law.column_of(k, census_law.clique(k), 0)] = comb(n - 1, k - 1)
    assert np.array_equal(gdv, want)


@pytest.mark.parametrize("n,k", [(5, 2), (6, 3), (7, 4), (9, 5), (9, 6)])
def test_cycle(n, k):
    """Every vertex is once at each position of a path of k: two of each two-vertex orbit, one of the middle for odd k."""
    gdv = one_graph(census_law.cycle(n), k)
    want = np.zeros_like(gdv)
    cols = [law.column_of(k, census_law.path(k), i) for i in range(k)]
    assert [cols[i] == cols[k - 1 - i] for i in range(k)] == [True] * k and len(set(cols)) == (k + 1) // 2
    for c in cols:
        want[:, c] += 1
    assert np.array_equal(gdv, want) and sorted(set(want[0].tolist()) - {0}) == ([2] if k % 2 == 0 else [1, 2])


@pytest.mark.parametrize("leaves,k,centre", [(6, 3, 6), (7, 4, 3), (7, 5, 0), (8, 6, 8)])
def test_star(leaves, k, centre):
    gdv = one_graph(census_law.star(leaves, centre), k)
    want = np.zeros_like(gdv)
    hub, leaf = law.column_of(k, census_law.star(k - 1), 0), law.column_of(k, census_law.star(k - 1), 1)
    assert hub != leaf
    want[:, leaf] = comb(leaves - 1, k - 2)
    want[centre] = 0
    want[centre, hub] = comb(leaves, k - 1)
    assert np.array_equal(gdv, want)


def test_k_one_and_two():
    n, es = 7, [(0, 1), (1, 2), (2, 0), (2, 3), (5, 5), (3, 2)]
    assert one_graph((n, es), 1).tolist() == [[1]] * 7
    assert one_graph((n, es), 2).tolist() == [[2], [2], [3], [1], [0], [0], [0]]


def test_population_rules():
    """n < k and a disconnected graph give nothing; loops join nothing, copies and reversed columns collapse; a column that crosses
    two graphs or lies outside every range belongs to none."""
    graphs = [(2, [(0, 1)]), (4, [(0, 1), (2, 3)]), (3, [(0, 1), (1, 0), (0, 1), (1, 1), (1, 2), (2, 2)]), (3, [(0, 1)])]
    ei, ptr = census_law.batch(graphs)
    ei = np.concatenate([ei, np.array([[1, 8, 40], [2, 9, 41]], np.int64)], axis=1)      # 1-2 and 8-9 cross graphs, 40-41 is outside
    gdv = law.vertex_census(ei, ptr, 3)
    end, mid = law.column_of(3, census_law.path(3), 0), law.column_of(3, census_law.path(3), 1)
    want = np.zeros((12, 3), np.int64)
    want[6, end] = want[8, end] = want[7, mid] = 1
    assert np.array_equal(gdv, want)
    assert law.vertex_census(ei, ptr, 3, failed={2}).sum() == 0
    shifted = law.vertex_census(ei + 5, ptr + 5, 3)                            # ptr[0] > 0: the rows below it are zero
    assert shifted.shape == (17, 3) and shifted[:5].sum() == 0 and np.array_equal(shifted[5:], want)


@pytest.mark.parametrize("k", [3, 4, 5])
def test_identities_on_a_random_graph(k):
    rng = np.random.default_rng(40 + k)
    n = 11
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < 0.3]
    ei, ptr = census_law.batch([census_law.cycle(6), (n, es)])
    gdv = law.vertex_census(ei, ptr, k)
    counts = census_law.census(ei, ptr, k)
    size, cls = law.orbit_sizes(k)
    assert size.sum() == k * len(law.layout(k)[0])
    assert np.array_equal(law.graph_sums(gdv, ptr), size[None, :] * counts[:, cls])
    for g in range(2):                                                          # a row sums to the sets that hold the vertex
        lo = int(ptr[g])
        adj = uniform_law.graph_adjacency(ei[0], ei[1], lo, int(ptr[g + 1]) - lo)
        rows = uniform_enum_law.subsets(adj, k)
        assert np.array_equal(gdv[lo:int(ptr[g + 1])].sum(axis=1), np.bincount(rows.reshape(-1), minlength=len(adj)))
    assert gdv.sum() == k * counts.sum() > 0


def entry_of(code, n):
    from ugs_sampler._lib import check, lib
    out = ctypes.c_uint32(0)
    check(lib.ugs_graphlet_vertex_census_entry(int(code), n, ctypes.byref(out)))
    return out.value


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_table_entry_of_every_code(n):
    codes = np.arange(1 << (n * (n - 1) // 2), dtype=np.int64)
    rooted = orbit_law.rooted_codes_many(codes, n)
    local = orbit_law.local_indices_many(rooted)
    at = {key & ((1 << 28) - 1): c for c, key in enumerate(census_law.connected_keys(n))}
    want = np.full(len(codes), NONE, np.int64)
    for i in range(len(codes)):
        c = at.get(int(rooted[i].min()))
        if c is not None:
            want[i] = c | sum(int(local[i, p]) << (10 + 3 * p) for p in range(n))
    got = np.array([entry_of(c, n) for c in codes], np.int64)
    assert np.array_equal(got, want)
    assert int((want != NONE).sum()) == (1, 1, 4, 38, 728, 26704)[n - 1]         # labelled connected graphs (OEIS A001187)


def test_table_entry_refusals():
    from ugs_sampler._lib import lib
    out = ctypes.c_uint32(0)
    assert lib.ugs_graphlet_vertex_census_entry(1 << 15, 6, ctypes.byref(out)) != 0      # a bit above n (n - 1) / 2
    assert lib.ugs_graphlet_vertex_census_entry(0, 8, ctypes.byref(out)) != 0
    assert lib.ugs_graphlet_vertex_census_entry(0, 0, ctypes.byref(out)) != 0
    assert lib.ugs_graphlet_vertex_census_entry(0, 3, None) != 0
    assert entry_of((1 << 21) - 1, 7) == 852                                    # K7: the last of the 853 classes, one orbit
    assert entry_of(0, 7) == NONE


def test_vertex_census_is_public():
    from ugs_sampler import graphlets
    assert "vertex_census" in graphlets.__all__ and "8 * N * O" in graphlets.vertex_census.__doc__


def test_refusals_without_a_device():
    from ugs_sampler import graphlets
    ei, ptr = torch.zeros((2, 0), dtype=torch.int64), torch.zeros((1,), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="1 <= k <= 7"):
        graphlets.vertex_census(ei, ptr, 8)
    for k in (0, 9, -1):
        with pytest.raises(RuntimeError, match="1 <= k <= 8"):
            graphlets.vertex_census(ei, ptr, k)
    for limit in (0, -1, (1 << 32) + 1):
        with pytest.raises(ValueError, match="limit"):
            graphlets.vertex_census(ei, ptr, 3, limit=limit)
    with pytest.raises(TypeError):
        graphlets.vertex_census(ei, ptr, 3.0)
    with pytest.raises(TypeError):
        graphlets.vertex_census(ei.numpy(), ptr, 3)
    with pytest.raises(RuntimeError, match="int64"):
        graphlets.vertex_census(ei.to(torch.int32), ptr, 3)
