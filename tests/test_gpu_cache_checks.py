"""The check of a cached call, in ugs_sampler.GraphCache (ugs_store.hip: ugs_store_check_k) and in rwr_sampler.GraphCache (ugs_rwr.hip:
rwr_store_check), on the inputs of tests/cache_check_cases.py: columns in the second workgroup, the last column of all, the first and
last column of a graph, graphs without a column in front of, between and behind the others and right ahead of the graph that
differs, one graph, ptr[0] != 0, two graphs that differ, endpoints 2^32 away from the stored ones, exchanged endpoints, and (rwr) a
graph that failed when it was added ahead of the one that differs.

Every case first asserts by the census (CPU) that its input is what it is there for.  Then: the unaltered batch equals the CPU
oracle (ugs) or the law (rwr), the altered batch is refused and the message names the case's graph, the cache serves the unaltered
batch afterwards, and check=False gives the added graphs' result for the altered batch.  tests/test_cache_check_law.py shows on a
model of both kernels that these inputs tell each modelled slip from the law.

The altered columns are safe to send: a cached call uploads the batch's columns for the check alone and reads them by column
position, never as an index (test_cache_check_law.py asserts the two host lines)."""
import numpy as np
import pytest
import torch

import cache_check_cases as CC
import oracle
import rwr_cache_cases as RC
import rwr_law as R
import ugs_cache_cases as UC

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
CASE_NAMES = [c.name for c in CC.cases()]
REFUSED = r"graph %d of the batch differs from the graph added in its place$"


def t(a):
    return torch.from_numpy(np.array(a, dtype=np.int64, order="C"))          # (a copy: the cases' arrays are read-only)


def assert_same(got, want, what=""):
    assert len(got) >= 5, what
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def assert_reaches(c):
    census = CC.census(c.name)
    for cls in c.reaches:
        assert cls in census, f"the input no longer reaches {cls!r}: choose it again (census: {sorted(census)})"
    assert CC.law(c, c.ei) is None and CC.law(c, c.bad) == c.expect


def rwr_graphs_law(c, seeds):
    """sample_graphs as one-graph law calls; a failed graph gives m rows of -1 and no edge"""
    nodes, eidx, eptr = [], [], [np.zeros(1, np.int64)]
    coff = CC.offsets(c.graphs)
    for g in range(len(c.graphs)):
        if g in c.failed:
            one = (np.full((CC.M, CC.K), -1, np.int64), np.zeros((2, 0), np.int64), np.zeros(CC.M + 1, np.int64))
        else:
            one = R.sample_batch(c.ei[:, coff[g]:coff[g + 1]], c.ptr[g:g + 2], CC.M, CC.K, "sample", 0, 0.2, seeds=[seeds[g]])
        nodes.append(one[0]); eidx.append(one[1])
        eptr.append(one[2][1:] + eptr[-1][-1])
    ei = np.concatenate(eidx, axis=1)
    return (np.concatenate(nodes), ei, np.concatenate(eptr), np.arange(len(c.graphs) + 1, dtype=np.int64) * CC.M, np.full(ei.shape[1], -1, np.int64))


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if not CC.case(n).failed])
def test_ugs_cache_check(name):
    import ugs_sampler
    c = CC.case(name)
    assert_reaches(c)
    G = len(c.graphs)
    idx = [UC.dataset_index(g) for g in range(G)]
    want = oracle.sample_batch(c.ei, c.ptr, CC.M, CC.K, "sample", CC.SEED)
    cache = ugs_sampler.GraphCache(CC.K, "cuda:0")
    try:
        i, a, n = UC.DUMMY
        cache.add(i, t(a), n)
        order = UC.adding_order(G, G)
        cache.add_many([idx[g] for g in order], [(t(c.graphs[g][1]), c.graphs[g][0]) for g in order])
        good = lambda what: assert_same(cache.sample_batch(idx, t(c.ptr), t(c.ei), CC.M, "sample", CC.SEED), want, (name, what))   # noqa: E731
        good("unaltered")
        with pytest.raises(RuntimeError, match=REFUSED % c.expect):
            cache.sample_batch(idx, t(c.ptr), t(c.bad), CC.M, "sample", CC.SEED)
        with pytest.raises(RuntimeError, match=REFUSED % c.expect):
            cache.sample_graphs(idx, t(c.ptr), t(c.bad), CC.M, list(range(G)), device="cuda:0")
        good("after the refusal")
        assert_same(cache.sample_batch(idx, t(c.ptr), t(c.bad), CC.M, "sample", CC.SEED, check=False), want, (name, "check=False"))
    finally:
        cache.close()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rwr_cache_check(name):
    import rwr_sampler
    c = CC.case(name)
    assert_reaches(c)
    G = len(c.graphs)
    idx = [RC.dataset_index(g) for g in range(G)]
    seeds = [CC.SEED + 5 * g for g in range(G)]
    cache = rwr_sampler.GraphCache(CC.K, "cuda:0")
    try:
        i, n, a = RC.DUMMY
        assert cache.add(i, t(a), n)
        order = RC.adding_order(G, G)
        cache.add_many([idx[g] for g in order], [(t(c.graphs[g][1]), c.graphs[g][0]) for g in order])
        assert cache.failed == {idx[g] for g in c.failed}
        if c.failed:                                                 # a batch with a failed graph is served by sample_graphs alone
            want = rwr_graphs_law(c, seeds)
            call = lambda ei, **kw: cache.sample_graphs(idx, t(c.ptr), t(ei), CC.M, seeds, **kw)      # noqa: E731
            assert call(c.ei)[5].tolist() == [g in c.failed for g in range(G)]
        else:
            want = R.sample_batch(c.ei, c.ptr, CC.M, CC.K, "sample", CC.SEED, 0.2)
            call = lambda ei, **kw: cache.sample_batch(idx, t(c.ptr), t(ei), CC.M, "sample", CC.SEED, **kw)   # noqa: E731
        assert_same(call(c.ei), want, (name, "unaltered"))
        for streams in ("graph", "row"):
            with pytest.raises(RuntimeError, match=REFUSED % c.expect):
                call(c.bad, streams=streams)
        with pytest.raises(RuntimeError, match=REFUSED % c.expect):
            cache.sample_graphs(idx, t(c.ptr), t(c.bad), CC.M, seeds)
        assert_same(call(c.ei), want, (name, "after the refusal"))
        assert_same(call(c.bad, check=False), want, (name, "check=False"))
    finally:
        cache.close()
