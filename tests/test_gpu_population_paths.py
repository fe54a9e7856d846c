"""What only uniform_sampler.PopulationCache runs (ugs_uniform.hip), one input per path (tests/population_paths.py):

  rows and fill   uni_pop_pairs, uni_pop_rows, uni_pop_fill: every sampling case of the mask-form pin (tests/uniform_paths.py) drawn
                  through a population, and new cases for the lanes 10 ... 15 of a row's group, k = 16, 17, 33 and 64, rows of -1 at
                  k > 16 however they come about (n < k, no vertex, no edge, failed at add time, a distinct call past |S_g|), workgroups
                  whose rows belong to several graphs, vertex 63 as either endpoint and as a loop;
  store           uni_pop_store: graphs of 8312 and 8313 keys -- a second trip of the copy -- in a shared block and in blocks of
                  their own, beside a failed and a set-less graph, and 4000 draws that land on both sides of key 8192;
  check           pop_fingerprint / uni_pop_check: more than 256 bitmap words, a difference in the last word, 1024 vertices, bit 63
                  of a mask graph, the same words at other places, the first of several differing graphs, a failed graph ahead;
  loops           uni_pop_loops: the loop vertices of a WL population in every word of the bitmap, {0} against {64}, loop columns
                  given twice, a loop past the 256th column of its graph.

Every case first asserts by its census (CPU) that the input reaches what it is there for, then compares every tensor with the law
(uniform_law / uniform_wide_law, uniform_enum_law + uniform_distinct_law, pop_wl_law), bit for bit, or expects the refusal that
names the law's graph.  tests/test_population_paths_law.py shows on a CPU model that these inputs tell each modelled slip from the
law.  The vertex limit is process-wide: every case sets it under a context manager that restores it."""
import contextlib

import numpy as np
import pytest
import torch

import pop_wl_law as PW
import population_paths as P
import uniform_law as U
import uniform_paths as UP
import uniform_wide_law as W
import wl_law as L

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
DEV = "cuda:0"
FIRST = 40                                                          # dataset index of a batch's graph 0: never a batch position


def sampler():
    import uniform_sampler
    return uniform_sampler


@contextlib.contextmanager
def vertex_limit(n):
    us = sampler()
    prev = us.set_max_vertices(n)
    try:
        yield
    finally:
        us.set_max_vertices(prev)


def t(a):
    return torch.from_numpy(np.array(a, dtype=np.int64, order="C"))          # (a copy: the cases' arrays are read-only)


def assert_same(got, want, what=""):
    assert len(got) >= 5, what
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def local_graphs(ei, ptr):
    """[(columns local to the graph, n)]: what a dataset holds for each graph of the batch"""
    out = []
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        inside = (ei[0] >= lo) & (ei[0] < hi) & (ei[1] >= lo) & (ei[1] < hi)
        out.append((t(ei[:, inside] - lo), hi - lo))
    return out


def population_of(ei, ptr, k, **kw):
    """(a population that holds the batch's graphs, each added from its local columns; their dataset indices)"""
    G = len(ptr) - 1
    pop = sampler().PopulationCache(k, DEV, **kw)
    idx = list(range(FIRST, FIRST + G))
    pop.add_many(idx, local_graphs(ei, ptr))
    return pop, idx


# ---- rows and fill ----
@pytest.mark.parametrize("name", [c.name for c in P.draw_cases()])
def test_draws_through_the_population_equal_the_law(name):
    c = P.draw_case(name)
    census = UP.census_of(name) if c.source == "uniform_paths" else P.row_census(name)
    for cls in c.reaches:
        assert cls in census, f"the input no longer reaches {cls!r}: choose it again (census: {sorted(census)})"
    G = len(c.ptr) - 1
    e, q = t(c.ei), t(c.ptr)
    with vertex_limit(c.limit):
        pop, idx = population_of(c.ei, c.ptr, c.k)
        try:
            assert pop.failed == {idx[g] for g in range(G) if c.failed[g]}, name
            for mode in c.modes:
                want = P.draw_law(name, mode)
                for check in (True, False):
                    what = (name, mode, check)
                    if c.what == "batch":
                        got = pop.sample_batch(idx, q, e, c.m, mode, c.seed, check=check)
                        assert len(got) == 5
                    elif c.what == "graphs":
                        got = pop.sample_graphs(idx, q, e, c.m, list(c.seeds), mode, check=check)
                        assert len(got) == 6 and got[5].tolist() == list(c.failed), what
                    else:
                        got = pop.sample_distinct(idx, q, e, c.m, list(c.seeds), mode, check=check)
                        assert len(got) == 7 and got[5].tolist() == want[5].tolist() and got[6].tolist() == want[6].tolist(), what
                    assert_same(got, want, what)
        finally:
            pop.close()


# ---- the store ----
@pytest.mark.parametrize("block_keys", [None, 64], ids=["shared_block", "own_blocks"])
def test_graphs_past_one_trip_of_the_copy(block_keys):
    c = P.store_case()
    assert P.store_census() == set(P.STORE_CLASSES), "the draws no longer land on both sides of key 8192: choose another seed"
    us = sampler()
    assert us.max_vertices() == 64
    pop = us.PopulationCache(c.k, DEV) if block_keys is None else us.PopulationCache(c.k, DEV, block_keys=block_keys)
    try:
        idx = list(range(FIRST, FIRST + len(c.graphs)))
        pop.add_many(idx, [(t(e), n) for n, e in c.graphs])          # one call: the failed and the set-less graph have no storage
        assert pop.failed == {idx[c.failed_at]}
        assert pop.sizes(idx).tolist() == list(c.sizes) and c.sizes[0] == 8312 and c.sizes[2] == 8313
        assert pop.info()["keys"] == sum(s for s in c.sizes if s > 0)
        order = [idx[i] for i in c.order]
        for mode in ("sample", "global"):
            got = pop.sample_batch(order, t(c.ptr), t(c.ei), c.m, mode, c.seed)
            assert_same(got, P.store_law(mode), (block_keys, mode))
    finally:
        pop.close()


# ---- the adjacency check ----
def sample(pop, idx, c, ei, mode="sample", **kw):
    if c.what == "batch":
        return pop.sample_batch(idx, t(c.ptr), t(ei), P.CHECK_M, mode, P.CHECK_SEED, **kw)
    return pop.sample_graphs(idx, t(c.ptr), t(ei), P.CHECK_M, list(P.check_seeds(c)), mode, **kw)


@pytest.mark.parametrize("name", [c.name for c in P.check_cases()])
def test_the_check_names_the_first_graph_whose_adjacency_differs(name):
    c = P.check_case(name)
    census = P.check_census(name)
    for cls in c.reaches:
        assert cls in census, f"the input no longer reaches {cls!r}: choose it again (census: {sorted(census)})"
    assert P.adjacency_law(c, c.ei) is None and P.adjacency_law(c, c.bad) == c.expect
    G, rows = len(c.graphs), len(c.graphs) * P.CHECK_M
    with vertex_limit(c.limit):
        pop, idx = population_of(c.ei, c.ptr, c.k)
        try:
            assert pop.failed == {idx[g] for g in c.failed}
            for mode in ("sample", "global"):
                got = sample(pop, idx, c, c.ei, mode)
                assert_same(got, P.check_law(c, mode), (name, mode, "unaltered"))
                if c.what == "graphs":
                    assert got[5].tolist() == [g in c.failed for g in range(G)]
            with pytest.raises(RuntimeError, match=rf"graph {c.expect} of the batch does not have the adjacency of the graph added in its place$"):
                sample(pop, idx, c, c.bad)
            unchecked = sample(pop, idx, c, c.bad, check=False)      # unspecified, but a result
            assert unchecked[0].shape == (rows, c.k) and unchecked[2].shape == (rows + 1,) and unchecked[3].tolist() == [g * P.CHECK_M for g in range(G + 1)]
            assert unchecked[1].shape == (2, int(unchecked[2][-1])) and unchecked[4].shape == (int(unchecked[2][-1]),)
            assert_same(sample(pop, idx, c, c.ei), P.check_law(c, "sample"), (name, "after the refusal"))
        finally:
            pop.close()


# ---- the loop vertices of a WL population ----
@pytest.mark.parametrize("name", [c.name for c in P.loop_cases()])
def test_the_wl_check_names_the_first_graph_whose_loop_vertices_differ(name):
    from ugs_sampler import wl
    c = P.check_case(name)
    census = P.loop_census(name)
    for cls in c.reaches:
        assert cls in census, f"the input no longer reaches {cls!r}: choose it again (census: {sorted(census)})"
    assert P.loops_law(c, c.ei) is None and P.loops_law(c, c.bad) == c.expect and P.adjacency_law(c, c.bad) is None
    it, m, seed = P.LOOP_ITERATIONS, 4 * P.CHECK_M, P.CHECK_SEED
    rows = W.sample_batch(c.ei, c.ptr, m, c.k, "sample", seed)
    known = sorted({h for h in L.wl_rows(*rows[:3], it)[0] if h is not None})[::2]
    vocab = {h: len(known) - 1 - i for i, h in enumerate(known)}
    want_ids = PW.sample_batch_ids(c.ei, c.ptr, m, c.k, seed, vocab, it)
    with vertex_limit(c.limit):
        pop, idx = population_of(c.ei, c.ptr, c.k, wl_iterations=it)
        try:
            table = wl.WLVocab(vocab, DEV)
            for mode in ("sample", "global"):
                *five, ids = pop.sample_batch(idx, t(c.ptr), t(c.ei), m, mode, seed, wl=table)
                assert_same(five, W.sample_batch(c.ei, c.ptr, m, c.k, mode, seed), (name, mode))
                assert ids.tolist() == want_ids, (name, mode)
            with pytest.raises(RuntimeError, match=rf"graph {c.expect} of the batch does not have the loop vertices of the graph added in its place$"):
                pop.sample_batch(idx, t(c.ptr), t(c.bad), m, "sample", seed, wl=table)
            # without wl= the loop vertices are not compared: the batch has the adjacency, its rows carry its own columns
            assert_same(pop.sample_batch(idx, t(c.ptr), t(c.bad), m, "sample", seed), W.sample_batch(c.bad, c.ptr, m, c.k, "sample", seed), (name, "no wl="))
            *five, ids = pop.sample_batch(idx, t(c.ptr), t(c.bad), m, "sample", seed, wl=table, check=False)
            assert ids.tolist() == want_ids, (name, "check=False: the ids of the added graphs")
            *five, ids = pop.sample_batch(idx, t(c.ptr), t(c.ei), m, "sample", seed, wl=table)
            assert ids.tolist() == want_ids, (name, "after the refusal")
        finally:
            pop.close()


def test_the_limits_are_back_at_their_defaults():
    us = sampler()
    assert us.max_vertices() == 64 and us._set_mask_vertices(64) == 64
    ei, ptr = UP.batch_of([UP.SMALL_ROOTS, (5, UP.und(UP.path(range(5))))], first=2)
    assert_same(us.sample_batch(t(ei), t(ptr), 6, 3, mode="sample", seed=5), U.sample_batch(ei, ptr, 6, 3, "sample", 5), "an ordinary call")
