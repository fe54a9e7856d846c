"""uniform_sampler's wide-form kernel paths (ugs_uniform.hip: uni_wadj, uni_wesu, uni_wrows / uni_wfill, uni_wenum_*, uni_wpop_*),
one input per path: the slot loop at 64, 65 and 129 higher neighbours with its r-th member in every place, 16 words per vertex with
prefix sums across every lane distance, vertex 1023 and bit 63, every level from k = 1 to k = 8 with whole-width keys, both sort
routes side by side, the lane flush of the count pass, the budget at and past max_rows, mask and wide graphs interleaved, and the
population's lane groups at 15, 16 and 17 columns and across chunks.

The inputs live in tests/uniform_wide_paths.py.  Every case first asserts by the census of the law (uniform_wide_law.census, CPU)
that its input reaches the path it is there for -- if that fails the input is wrong, not the kernel -- and then compares every
tensor of sample_batch / sample_graphs / enumerate_graphs / count_graphs with the law (uniform_wide_law, uniform_enum_law), bit for
bit; every sampling case is drawn through PopulationCache as well.  tests/test_uniform_wide_paths_law.py shows on a CPU model of the
kernels that these inputs tell each modelled slip from the law.  The vertex limit and the mask threshold are process-wide, so every
case sets them under a context manager that restores them."""
import contextlib

import numpy as np
import pytest
import torch

import uniform_enum_law as EL
import uniform_wide_law as W
import uniform_wide_paths as P

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
CASE_NAMES = [c.name for c in P.cases()]
DEV = "cuda:0"


def sampler():
    import uniform_sampler
    return uniform_sampler


@contextlib.contextmanager
def limits(max_vertices, mask_vertices):
    us = sampler()
    prev_max = us.set_max_vertices(max_vertices)
    try:
        prev_mask = us._set_mask_vertices(mask_vertices)
        try:
            yield
        finally:
            us._set_mask_vertices(prev_mask)
    finally:
        us.set_max_vertices(prev_max)


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def local_graphs(c):
    """[(columns local to the graph, n)]: what a dataset holds for each graph of the batch"""
    out = []
    for g in range(len(c.ptr) - 1):
        lo, hi = int(c.ptr[g]), int(c.ptr[g + 1])
        inside = (c.ei[0] >= lo) & (c.ei[0] < hi) & (c.ei[1] >= lo) & (c.ei[1] < hi)
        out.append((torch.from_numpy(np.ascontiguousarray(c.ei[:, inside] - lo)), hi - lo))
    return out


def through_population(c, mode, e, q, want, what):
    """The same draw from a PopulationCache that holds the batch's graphs (added under the same limits)"""
    G = len(c.ptr) - 1
    pop = sampler().PopulationCache(c.k, DEV)
    try:
        pop.add_many(range(G), local_graphs(c))
        assert pop.failed == {g for g in range(G) if c.failed[g]}, what
        if c.what == "batch":
            got = pop.sample_batch(range(G), q, e, c.m, mode, c.seed)
        else:
            got = pop.sample_graphs(range(G), q, e, c.m, list(c.seeds), mode)
            assert got[5].tolist() == list(c.failed), what
        assert_same(got[:5], want, what + ("population",))
    finally:
        pop.close()


def run_and_compare(c, mode, device=None):
    """The case through the entry it names, every tensor against the law's."""
    us = sampler()
    e, q = torch.from_numpy(c.ei), torch.from_numpy(c.ptr)
    if device is not None:
        e, q = e.to(device), q.to(device)
    G = len(c.ptr) - 1
    want = P.law_of(c.name, mode)
    what = (c.name, mode, device)
    if c.what == "count":
        counts, failed = us.count_graphs(e, q, c.k)
        assert counts.dtype == torch.int64 and counts.tolist() == want[0].tolist() and failed.tolist() == [False] * G, what
        return
    if c.what == "refused":
        with pytest.raises(RuntimeError, match="split the call"):
            us.enumerate_graphs(e, q, c.k, mode, max_rows=c.max_rows)
        got = us.enumerate_graphs(e, q, c.k, mode, max_rows=c.max_rows + 1)      # the library serves the next call
        assert got[5].tolist() == [False] * G, what
        assert_same(got[:5], EL.enumerate_graphs(c.ei, c.ptr, c.k, mode), what)
        return
    if c.what == "batch":
        got = us.sample_batch(e, q, c.m, c.k, mode=mode, seed=c.seed)
        assert len(got) == 5
    elif c.what == "graphs":
        got = us.sample_graphs(e, q, c.m, c.k, list(c.seeds), mode=mode)
        assert len(got) == 6 and got[5].tolist() == list(c.failed), what
    else:
        got = us.enumerate_graphs(e, q, c.k, mode, max_rows=c.max_rows)
        assert len(got) == 6 and got[5].tolist() == list(c.failed), what
        counts, failed = us.count_graphs(e, q, c.k)
        assert counts.tolist() == want[5].tolist() and failed.tolist() == list(c.failed), what
    if device is not None:
        assert all(t.is_cuda for t in got[:5]), what
    assert_same(got[:5], want, what)
    if c.what in ("batch", "graphs") and device is None:
        through_population(c, mode, e, q, want, what)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_path_equals_law(name):
    c = P.case(name)
    census = P.census_of(name)
    for cls in c.reaches:
        assert cls in census, f"the input no longer reaches {cls!r}: choose it again (census: {sorted(census)})"
    with limits(P.LIMIT, c.mask_vertices):
        for mode in c.modes:
            run_and_compare(c, mode)


@pytest.mark.parametrize("name", P.ON_DEVICE)
def test_path_equals_law_with_device_inputs(name):
    c = P.case(name)
    with limits(P.LIMIT, c.mask_vertices):
        run_and_compare(c, c.modes[-1], device=DEV)


def test_an_ordinary_call_after_the_paths_equals_the_law():
    """Runs behind the cases above: whatever they left in the pools and the limits, an everyday wide batch still gives the law's
    tensors, and the limits are back at their defaults."""
    import ugs_workloads as wl
    us = sampler()
    assert us.max_vertices() == 64 and us._set_mask_vertices(64) == 64
    ei, ptr = W.batch([(90, wl.tu_graph(90, 100, 1)), (20, wl.tu_graph(20, 24, 2)), (150, wl.tu_graph(150, 160, 3))], first=2)
    with limits(P.LIMIT, 64):
        for mode, seed in (("sample", 5), ("global", 6)):
            got = us.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 16, 4, mode=mode, seed=seed)
            assert_same(got, W.sample_batch(ei, ptr, 16, 4, mode, seed), mode)
