"""CPU: why a graph may be served from a store (ugs_sampler.GraphCache), shown with the oracle alone, and the refusals of the cache
that need no device.

The property: the oracle on the collated batch, with a fresh LRU, equals the concatenation of the oracle's one-graph calls -- each
on the graph's own columns, ptr [0, n], a fresh LRU and the same seed (or seeds[g]) -- re-based by ptr[g] and coff[g].  So a
graph's rows depend on its own content, k, the seed and m alone: not on its place in the batch, its neighbours or the LRU's
history.  Every case's census class (degenerate, relaxation level, candidate bound) is asserted from oracle.Preproc."""
import numpy as np
import pytest
import torch

import oracle
import ugs_cache_cases as CC


def census_of(cols, n, k):
    """(degenerate, level, candidate bound) as the reference's preprocessing sees the graph"""
    if n <= 0 or n < k:
        return (True, None, None)
    p = oracle.Preproc(cols, n, k)
    info, d = p.info(), p.dump()
    p.close()
    deg = np.diff(d["indptr"])
    bound = max(0, min(n - 1, (k - 1) * int(deg.max())))
    if info["bucket_count_nonzero"] > 0:
        return (False, 0, bound)
    return (False, 1 if (d["suffix_deg"] > 0).any() else 2, bound)


batch_law = CC.batch_law


@pytest.mark.parametrize("name", [c.name for c in CC.cases()])
def test_the_batch_is_the_concatenation_of_its_graphs_one_graph_calls(name):
    c = CC.case(name)
    ei, ptr, coff = CC.collate(c)
    blocks = []
    for g, p in enumerate(c.picks):
        cols, n = c.graphs[p]
        seed = c.seed if c.seeds is None else c.seeds[g]
        blocks.append(oracle.sample_batch(cols, np.array([0, n], np.int64), c.m, c.k, c.mode, seed))      # a fresh LRU each
    want = CC.rebased(blocks, ptr, coff, c.m, c.k, c.mode)
    got = batch_law(c)
    for nm, a, b in zip(CC.NAMES, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (name, nm)
    assert got[0].shape == (len(c.picks) * c.m, c.k)


@pytest.mark.parametrize("name", [c.name for c in CC.cases()])
def test_every_case_is_in_the_class_it_is_there_for(name):
    c = CC.case(name)
    for g, p in enumerate(c.picks):
        cols, n = c.graphs[p]
        assert census_of(cols, n, c.k) == c.census[g], (name, g)
    bounds = [b for gone, _, b in c.census if not gone]
    if c.tier == "global":
        assert max(bounds) > CC.TIER_CAP[-1]
    if c.tier == "every" or name == "star70_k3":
        assert max(bounds) > CC.TIER_CAP[0]
    if name == "levels_k2":
        cols, n = c.graphs[2]
        p = oracle.Preproc(cols, n, c.k)
        prob = p.dump()["prob"]
        p.close()
        assert ((prob > 0) & (prob < 1)).any(), "no alias row with prob < 1"
    if name == "repeated_columns":
        got = batch_law(c)                                              # some row holds more than two entries for one pair of its vertices
        eptr, pairs = got[2], np.sort(got[1].T, axis=1)
        assert any(eptr[r + 1] - eptr[r] > 2 * len({tuple(x) for x in pairs[eptr[r]:eptr[r + 1]].tolist()}) for r in range(c.m, 2 * c.m))
    rows = len(c.picks) * c.m
    if name.startswith("g33_m3"):
        assert rows % 8 and rows % 32 and rows > 32


def test_the_cases_cover_what_the_list_promises():
    cs = CC.cases()
    assert {c.mode for c in cs} == {"sample", "graph", "global"}
    assert any(c.m == 1 for c in cs) and any(len(set(c.picks)) < len(c.picks) for c in cs)
    assert any(c.seeds is not None and 0 in c.seeds and min(c.seeds) < 0 for c in cs)
    levels = {lv for c in cs for gone, lv, _ in c.census if not gone}
    assert levels == {0, 1, 2} and any(gone for c in cs for gone, _, _ in c.census)
    for c in cs:
        assert all(CC.dataset_index(p) != g for g, p in enumerate(c.picks))


# ---- refusals that need no device ----
def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture()
def cache():
    import ugs_sampler
    c = ugs_sampler.GraphCache(3, "cuda:0")
    yield c
    c.close()


def test_refusals_before_any_device_work(cache):
    import ugs_sampler
    ring, n = CC.ring(6)
    before = ugs_sampler.cache_stats()
    with pytest.raises(KeyError):
        cache.sample_batch([5], t(np.array([0, n])), t(ring), 2)
    with pytest.raises(ValueError, match="graph_idx names 2 graphs, ptr holds 1"):
        cache.sample_batch([5, 6], t(np.array([0, n])), t(ring), 2)
    with pytest.raises(ValueError, match="edge_index=None needs check=False"):
        cache.sample_batch([], t(np.array([0])), None, 2)
    with pytest.raises(ValueError, match="device= must be a GPU device"):
        cache.sample_batch([], t(np.array([0])), t(CC.NONE), 2, device="cpu")
    with pytest.raises(RuntimeError, match="mode must be one of"):
        cache.sample_batch([], t(np.array([0])), t(CC.NONE), 2, "rows")
    with pytest.raises(TypeError, match=r"seeds\[1\]=4294967296 does not fit a C int"):
        cache.sample_graphs([5, 6], t(np.array([0, n, 2 * n])), None, 2, [1, 1 << 32], check=False)
    with pytest.raises(TypeError, match="seed=.* does not fit a C int"):
        cache.sample_batch([], t(np.array([0])), t(CC.NONE), 2, seed=1 << 40)
    with pytest.raises(ValueError, match=r"graph 9 has a column with an endpoint outside \[0, 6\)"):
        cache.add_many([8, 9], [(t(ring), n), (t(ring + 1), n)])
    with pytest.raises(ValueError, match=r"graph 9 has a column with an endpoint outside"):
        cache.add(9, t(np.array([[0], [-1]])), n)
    assert cache.info() == {"graphs": 0, "vertices": 0, "csr_entries": 0, "bytes": 0, "generations": 0}      # nothing of the refused call was added
    assert cache.last_launch() == ("", "")
    assert ugs_sampler.cache_stats() == before


def test_k_above_32_is_refused_with_the_existing_text():
    import ugs_sampler
    with pytest.raises(RuntimeError, match="^k > 32 is not supported by the HIP sampler$"):
        ugs_sampler.GraphCache(33, "cuda:0")
    with pytest.raises(ValueError, match="device must be a GPU device"):
        ugs_sampler.GraphCache(3, "cpu")
    with pytest.raises(ValueError, match="reserve must be two counts"):
        ugs_sampler.GraphCache(3, "cuda:0", reserve=(-1, 0))
    c = ugs_sampler.GraphCache(32, "cuda:0")
    c.close()
    with pytest.raises(RuntimeError, match="the cache is closed"):
        c.info()
