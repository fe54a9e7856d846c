"""uniform_sampler's mask-form kernel paths (ugs_uniform.hip), one input per path: the column search and sort at their edges, both
forms of the search and its deepest stack, vertex 63, the count pass's flush, root buckets on both sides of the LDS bound (alone and
as neighbours, with one-key buckets beside them), the draw kernel's blocks of 320 graphs and 312 outputs, a generator per graph,
and the rows' decoding.

The inputs live in tests/uniform_paths.py.  Every case first asserts by the census of the law (uniform_law.census, CPU) that its
input reaches the path it is there for -- if that fails the input is wrong, not the kernel -- and then compares every tensor of
sample_batch / sample_graphs / enumerate_graphs / count_graphs with the law (uniform_law, uniform_enum_law), bit for bit.
tests/test_uniform_paths_law.py shows on a CPU model of the kernels that these inputs tell each modelled slip from the law."""
import numpy as np
import pytest
import torch

import uniform_law as U
import uniform_paths as P

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
CASE_NAMES = [c.name for c in P.cases()]


def sampler():
    import uniform_sampler
    return uniform_sampler


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def run_and_compare(c, mode, device=None):
    """The case through the entry it names, every tensor against the law's."""
    e, q = torch.from_numpy(c.ei), torch.from_numpy(c.ptr)
    if device is not None:
        e, q = e.to(device), q.to(device)
    G = len(c.ptr) - 1
    want = P.law_of(c.name, mode)
    what = (c.name, mode, device)
    if c.what == "batch":
        got = sampler().sample_batch(e, q, c.m, c.k, mode=mode, seed=c.seed)
        assert len(got) == 5
    elif c.what == "graphs":
        got = sampler().sample_graphs(e, q, c.m, c.k, list(c.seeds), mode=mode)
        assert len(got) == 6 and got[5].tolist() == [False] * G, what
    elif c.what == "enumerate":
        got = sampler().enumerate_graphs(e, q, c.k, mode)
        assert len(got) == 6 and got[5].tolist() == [False] * G, what
        counts, failed = sampler().count_graphs(e, q, c.k)
        assert counts.tolist() == want[5].tolist() and failed.tolist() == [False] * G, what
    else:
        counts, failed = sampler().count_graphs(e, q, c.k)
        assert counts.dtype == torch.int64 and counts.tolist() == want[0].tolist() and failed.tolist() == [False] * G, what
        return
    if device is not None:
        assert all(t.is_cuda for t in got[:5]), what
    assert_same(got[:5], want, what)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_path_equals_law(name):
    c = P.case(name)
    census = P.census_of(name)
    for cls in c.reaches:
        assert cls in census, f"the input no longer reaches {cls!r}: choose it again (census: {sorted(census)})"
    for mode in c.modes:
        run_and_compare(c, mode)


@pytest.mark.parametrize("name", P.ON_DEVICE)
def test_path_equals_law_with_device_inputs(name):
    c = P.case(name)
    run_and_compare(c, c.modes[-1], device="cuda:0")


def test_an_ordinary_call_after_the_paths_equals_the_law():
    """Runs behind the cases above: whatever they left in the pools, an everyday batch still gives the law's tensors."""
    import ugs_workloads as wl
    ei, ptr = wl.tu_batch(18, 20, 6)
    for mode, seed in (("sample", 5), ("global", 6)):
        got = sampler().sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 16, 4, mode=mode, seed=seed)
        assert_same(got, U.sample_batch(ei, ptr, 16, 4, mode, seed), mode)
