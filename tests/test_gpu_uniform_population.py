"""uniform_sampler.PopulationCache (ugs_uniform.hip: uni_pop_* / uni_wpop_*) against the reference's outputs (tests/golden/f14_*,
f18_*), the CPU laws (tests/uniform_law.py, tests/uniform_wide_law.py; sample_graphs as one-graph law calls) and, where noted, the
uncached calls: bit-exact, every tensor.  The vertex limit is process-wide, so the tests that raise it restore it."""
import ctypes
import functools
import json
import os
import random
import threading

import numpy as np
import pytest
import torch

import ugs_workloads as wl
import uniform_law as U
import uniform_population_cases as P
import uniform_wide_law as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F14 = os.path.join(HERE, "golden", "f14_uniform_reference")
F18 = os.path.join(HERE, "golden", "f18_uniform_wide_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
DEV = "cuda:0"


def us():
    import uniform_sampler
    return uniform_sampler


def scenarios(path):
    with open(path + ".json") as f:
        return [(path, s) for s in json.load(f)["scenarios"]]


def assert_same(got, want, what=""):
    assert len(got) >= 5
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        b = b.cpu().numpy() if torch.is_tensor(b) else b
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def local_graphs(ei, ptr):
    """[(n, local columns)] of a batch: what a dataset holds for each of its graphs"""
    out = []
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        inside = (ei[0] >= lo) & (ei[0] < hi) & (ei[1] >= lo) & (ei[1] < hi)
        out.append((hi - lo, ei[:, inside] - lo))
    return out


def add_all(pop, graphs, first=0, one_by_one=False):
    if one_by_one:
        for i, (n, e) in enumerate(graphs):
            pop.add(first + i, t(e), n)
    else:
        pop.add_many(range(first, first + len(graphs)), [(t(e), n) for n, e in graphs])


def graphs_law(ei, ptr, m, k, mode, seeds):
    """sample_graphs as one-graph law calls, edge_ptr re-based"""
    nodes, eidx, eptr, esrc = [], [], [np.zeros(1, np.int64)], []
    for g in range(len(ptr) - 1):
        one = W.sample_batch(ei, ptr[g:g + 2], m, k, mode, seeds[g])
        nodes.append(one[0]); eidx.append(one[1]); esrc.append(one[4])
        eptr.append(one[2][1:] + eptr[-1][-1])
    G = len(ptr) - 1
    return (np.concatenate(nodes).reshape(G * m, k) if G else np.zeros((0, k), np.int64), np.concatenate(eidx + [np.zeros((2, 0), np.int64)], axis=1),
            np.concatenate(eptr), np.arange(G + 1, dtype=np.int64) * m, np.concatenate(esrc + [np.zeros(0, np.int64)]))


def small_graph(rng, n, extra=None):
    if n <= 1:
        return n, np.zeros((2, 0), np.int64)
    return n, wl.tu_graph(n, n - 1 + (rng.randint(0, n) if extra is None else extra), rng.randrange(1 << 30))


# ---- 1. the reference's outputs ----
@pytest.mark.parametrize("path,s", scenarios(F14) + scenarios(F18), ids=lambda v: v["name"] if isinstance(v, dict) else "")
def test_equals_reference_fixture(path, s):
    z = np.load(path + ".npz")
    name = s["name"]
    ei, ptr = z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"]
    prev = us().set_max_vertices(1024)
    try:
        pop = us().PopulationCache(s["k"], DEV)
        add_all(pop, local_graphs(ei, ptr), one_by_one=True)
    finally:
        us().set_max_vertices(prev)
    got = pop.sample_batch(range(len(ptr) - 1), t(ptr), t(ei), s["m"], s["mode"], int(s["seed"]))
    assert all(x.device.type == "cpu" for x in got) and all(x.is_pinned() for x in got if x.numel() > 0)
    assert_same(got, [z[f"{name}/{nm}"] for nm in NAMES], name)
    pop.close()


# ---- 2. slot indirection: the batch's order is not the order of the adds ----
@functools.lru_cache(maxsize=None)
def four_graphs():
    rng = random.Random(21)
    return [small_graph(rng, n) for n in (9, 12, 6, 11)]


@pytest.fixture(scope="module")
def four_pop():
    a, b, c, d = four_graphs()
    pop = us().PopulationCache(3, DEV)
    pop.add_many([10, 11], [(t(a[1]), a[0]), (t(b[1]), b[0])])
    pop.add_many([12], [(t(c[1]), c[0])])
    assert pop.add(13, t(d[1]), d[0])
    yield pop
    pop.close()


@pytest.mark.parametrize("order", [(12, 10, 13), (11, 11, 10), (13,)], ids=["CAD", "BBA", "D"])
@pytest.mark.parametrize("mode", ["sample", "global"])
def test_any_batch_of_added_graphs_equals_the_law_and_the_uncached_call(four_pop, order, mode):
    ei, ptr = W.batch([four_graphs()[i - 10] for i in order], first=3)
    perm = np.random.RandomState(5).permutation(ei.shape[1])
    ei = np.ascontiguousarray(ei[:, perm])
    assert four_pop.info()["graphs"] == 4 and four_pop.failed == set()
    for seed in (0, 42, (1 << 63) + 5, -1):
        want = U.sample_batch(ei, ptr, 5, 3, mode, seed)
        got = four_pop.sample_batch(torch.tensor(order), t(ptr), t(ei), 5, mode, seed)
        assert_same(got, want, f"{order} {mode} {seed}")
        assert_same(us().sample_batch(t(ei), t(ptr), 5, 3, mode=mode, seed=seed), want, "uncached")
    seeds = [7, (1 << 64) - 1, 1 << 40][:len(order)]
    got = four_pop.sample_graphs(list(order), t(ptr), t(ei), 5, seeds, mode)
    assert_same(got, graphs_law(ei, ptr, 5, 3, mode, seeds), "sample_graphs")
    assert not got[5].any()
    unc = us().sample_graphs(t(ei), t(ptr), 5, 3, seeds, mode)
    assert all(torch.equal(x, y) for x, y in zip(got, unc))
    sizes = four_pop.sizes(order).tolist()
    assert sizes == [len(W.sorted_tuples(U.graph_adjacency(ei[0], ei[1], int(ptr[g]), int(ptr[g + 1] - ptr[g])), 3)) for g in range(len(order))]


def test_adding_an_index_again_replaces_it():
    rng = random.Random(8)
    a, b = small_graph(rng, 8), small_graph(rng, 10)
    pop = us().PopulationCache(3, DEV)
    add_all(pop, [a, b])
    pop.add(0, t(b[1]), b[0])
    ei, ptr = W.batch([b, b])
    assert_same(pop.sample_batch([0, 1], t(ptr), t(ei), 6, "sample", 1), U.sample_batch(ei, ptr, 6, 3, "sample", 1))
    assert pop.info()["graphs"] == 2
    pop.close()


# ---- 3. storage: blocks of 64 keys, a graph larger than a block, adds between samples ----
def test_blocks_are_never_moved_by_later_adds():
    rng = random.Random(33)
    first = [small_graph(rng, n, extra=2) for n in (7, 8, 9, 10, 6)] + [small_graph(rng, 16, extra=14)]
    pop = us().PopulationCache(3, DEV, block_keys=64)
    add_all(pop, first)
    sizes = pop.sizes(range(len(first))).tolist()
    assert max(sizes) > 64 and sum(s for s in sizes if s <= 64) > 64, sizes     # one graph exceeds a block, the others span several
    info = pop.info()
    assert info["blocks"] >= 3 and info["keys"] == sum(sizes) and info["bytes"] >= 8 * info["keys"]
    ei, ptr = W.batch([first[i] for i in (5, 0, 3, 4, 1, 2)], first=1)
    order = [5, 0, 3, 4, 1, 2]
    want = U.sample_batch(ei, ptr, 9, 3, "sample", 77)
    before = pop.sample_batch(order, t(ptr), t(ei), 9, "sample", 77, device=DEV)
    assert_same(before, want, "before")
    add_all(pop, [small_graph(rng, n, extra=3) for n in (12, 9, 14, 11)], first=100)
    assert pop.info()["blocks"] > info["blocks"]
    after = pop.sample_batch(order, t(ptr), t(ei), 9, "sample", 77, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert_same(after, want, "after")
    pop.close()


# ---- 4. mixed forms in one batch ----
def test_wide_and_mask_graphs_interleaved():
    rng = random.Random(44)
    graphs = [small_graph(rng, 66, extra=4), small_graph(rng, 20), small_graph(rng, 70, extra=6), small_graph(rng, 2), small_graph(rng, 9),
              (5, np.zeros((2, 0), np.int64))]
    ei, ptr = W.batch(graphs, first=2)
    ei = np.ascontiguousarray(ei[:, np.random.RandomState(1).permutation(ei.shape[1])])
    prev = us().set_max_vertices(128)
    try:
        pop = us().PopulationCache(3, DEV)
        add_all(pop, graphs)
        inside = pop.sample_batch(range(6), t(ptr), t(ei), 7, "sample", 9)
        unc = us().sample_batch(t(ei), t(ptr), 7, 3, mode="sample", seed=9)
    finally:
        us().set_max_vertices(prev)
    want = W.sample_batch(ei, ptr, 7, 3, "sample", 9)
    assert_same(inside, want, "mixed")
    assert_same(unc, want, "uncached")
    assert (want[0][:7] >= 0).all() and (want[0][14:21] >= 0).all() and (want[0][21:28] == -1).all() and (want[0][35:] == -1).all()
    assert pop.failed == set() and pop.sizes([3, 5]).tolist() == [0, 0]
    # the limit in force at add time applies: the slots keep their form after it is lowered again
    assert_same(pop.sample_batch(range(6), t(ptr), t(ei), 7, "global", 10), W.sample_batch(ei, ptr, 7, 3, "global", 10), "after restore")
    seeds = [3, 4, 5, 6, 7, 8]
    assert_same(pop.sample_graphs(range(6), t(ptr), t(ei), 4, seeds), graphs_law(ei, ptr, 4, 3, "sample", seeds), "sample_graphs")
    pop.close()


# ---- 5. the edges of the 16-lane groups ----
@pytest.fixture(scope="module")
def lane_case():
    return P.lane_group_batch()


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("mode", ["sample", "global"])
def test_lane_group_edges(lane_case, k, mode):
    """Buckets of 0, 1, 15, 16, 17, 33 and 300 columns, a bucket whose hits are lane 15's alone, duplicate columns, loops and
    columns that cross graphs; 280 rows at m = 7 (18 workgroups of 16 rows).  tests/test_uniform_population_law.py shows that every
    one-line mistake in the fill differs from the law on this batch."""
    graphs, ei, ptr = lane_case
    assert (len(ptr) - 1) * 7 == 280
    pop = us().PopulationCache(k, DEV)
    add_all(pop, graphs)
    want = U.sample_batch(ei, ptr, 7, k, mode, 42)
    assert_same(pop.sample_batch(range(40), t(ptr), t(ei), 7, mode, 42), want, "lane groups")
    assert_same(pop.sample_batch(range(40), t(ptr), t(ei), 7, mode, 42, check=False), want, "check=False")
    zero = pop.sample_batch(range(40), t(ptr), t(ei), 0, mode, 42)
    assert_same(zero, U.sample_batch(ei, ptr, 0, k, mode, 42), "m = 0")
    empty = pop.sample_batch([], torch.zeros(1, dtype=torch.int64), torch.zeros((2, 0), dtype=torch.int64), 7, mode, 42)
    assert [tuple(x.shape) for x in empty] == [(0, k), (2, 0), (1,), (1,), (0,)] and empty[2].tolist() == [0]
    six = pop.sample_graphs([], torch.zeros(1, dtype=torch.int64), torch.zeros((2, 0), dtype=torch.int64), 7, [], mode)
    assert len(six) == 6 and six[5].numel() == 0
    pop.close()


# ---- 6. values of k ----
@pytest.mark.parametrize("k,n", [(1, 10), (2, 10), (6, 14), (8, 12), (9, 12)])
def test_values_of_k(k, n):
    rng = random.Random(600 + k)
    graphs = [small_graph(rng, n, extra=3), small_graph(rng, n - 1, extra=2), small_graph(rng, max(k - 1, 1))]
    ei, ptr = W.batch(graphs, first=4)
    pop = us().PopulationCache(k, DEV)
    add_all(pop, graphs)
    for mode, seed in (("sample", 42), ("global", (1 << 64) - 3)):
        assert_same(pop.sample_batch([0, 1, 2], t(ptr), t(ei), 11, mode, seed), U.sample_batch(ei, ptr, 11, k, mode, seed), f"k={k} {mode}")
    pop.close()


# ---- 7. failures at add time ----
def test_a_graph_over_max_rows_fails_alone():
    rng = random.Random(70)
    path = (5, np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.int64))
    big = small_graph(rng, 30, extra=30)
    adj = U.graph_adjacency(big[1][0], big[1][1], 0, 30)
    assert len(U.esu_masks(adj, 4)) > 100
    pop = us().PopulationCache(4, DEV, max_rows=100)
    add_all(pop, [path, big, path])
    assert pop.failed == {1} and pop.sizes([0, 1, 2]).tolist() == [2, -1, 2]
    assert pop.add(5, t(big[1]), big[0]) is False and pop.failed == {1, 5}
    ei, ptr = W.batch([path, big, path])
    with pytest.raises(RuntimeError, match="graph 1 of the batch failed"):
        pop.sample_batch([0, 1, 2], t(ptr), t(ei), 6, "sample", 3)
    # the library stays usable: the healthy graphs alone, and the whole batch through sample_graphs
    ei2, ptr2 = W.batch([path, path])
    assert_same(pop.sample_batch([0, 2], t(ptr2), t(ei2), 6, "sample", 3), U.sample_batch(ei2, ptr2, 6, 4, "sample", 3), "healthy")
    seeds = [11, 12, 13]
    six = pop.sample_graphs([0, 1, 2], t(ptr), t(ei), 6, seeds, "global")
    assert six[5].tolist() == [False, True, False] and (six[0][6:12] == -1).all()
    keep = W.batch([path, (30, np.zeros((2, 0), np.int64)), path])                 # the failed graph as one without sets
    want = graphs_law(keep[0], keep[1], 6, 4, "global", seeds)
    src = np.where(want[4] >= 4, want[4] + big[1].shape[1], want[4])              # edge_src: positions in the batch that holds big's columns
    assert_same(six, want[:4] + (src,), "sample_graphs around the failed graph")
    pop.close()


def test_graphs_jointly_over_max_rows_are_added_in_smaller_calls():
    rng = random.Random(72)
    graphs = [small_graph(rng, 10, extra=3) for _ in range(6)]
    pop = us().PopulationCache(3, DEV, max_rows=100)
    add_all(pop, graphs)
    sizes = pop.sizes(range(6)).tolist()
    assert pop.failed == set() and max(sizes) <= 100 < sum(sizes), sizes
    ei, ptr = W.batch(graphs)
    assert_same(pop.sample_batch(range(6), t(ptr), t(ei), 5, "sample", 8), U.sample_batch(ei, ptr, 5, 3, "sample", 8), "joint")
    pop.close()


def test_a_graph_over_the_vertex_limit_fails_alone():
    rng = random.Random(71)
    big, small = small_graph(rng, 70, extra=3), small_graph(rng, 8)
    assert us().max_vertices() == 64
    pop = us().PopulationCache(3, DEV)
    add_all(pop, [small, big])
    assert pop.failed == {1} and pop.sizes([1]).tolist() == [-1]
    ei, ptr = W.batch([big, small])
    with pytest.raises(RuntimeError, match="graph 0 of the batch failed"):
        pop.sample_batch([1, 0], t(ptr), t(ei), 2)
    pop.close()


# ---- 8. the checks of a sample call ----
def test_checks_of_the_batch_against_the_population():
    rng = random.Random(80)
    graphs = [small_graph(rng, 10, extra=4), small_graph(rng, 12, extra=5), small_graph(rng, 7, extra=2)]
    pop = us().PopulationCache(3, DEV)
    add_all(pop, graphs)
    ei, ptr = W.batch(graphs, first=1)
    with pytest.raises(RuntimeError, match=r"graph 1 of the batch has 11 vertices.* 12$"):
        pop.sample_batch([0, 1, 2], t(np.array([1, 11, 22, 30])), t(ei), 4)
    # one flipped edge in graph 1: an edge's columns replaced by a pair that is no edge
    lo = int(ptr[1])
    adj = U.graph_adjacency(ei[0], ei[1], lo, 12)
    u, v = next((a, b) for a in range(12) for b in range(a + 1, 12) if not adj[a] >> b & 1)
    flipped = ei.copy()
    first = int(np.nonzero(ei[0] >= lo)[0][0])
    a, b = int(ei[0, first]), int(ei[1, first])
    same = ((ei[0] == a) & (ei[1] == b)) | ((ei[0] == b) & (ei[1] == a))
    flipped[:, same] = np.array([[lo + u], [lo + v]])
    with pytest.raises(RuntimeError, match="graph 1 of the batch does not have the adjacency"):
        pop.sample_batch([0, 1, 2], t(ptr), t(flipped), 4)
    unchecked = pop.sample_batch([0, 1, 2], t(ptr), t(flipped), 4, check=False)    # unspecified, but a result
    assert unchecked[0].shape == (12, 3) and unchecked[2][-1] == unchecked[1].shape[1]
    # permuted and duplicated columns, loops and cross-graph columns: the same adjacency
    rs = np.random.RandomState(2)
    noisy = np.concatenate([ei, ei[::-1, ::3], np.array([[1, 3, int(ptr[1])], [1, 3, int(ptr[2])]])], axis=1)
    noisy = np.ascontiguousarray(noisy[:, rs.permutation(noisy.shape[1])])
    assert_same(pop.sample_batch([0, 1, 2], t(ptr), t(noisy), 4, "sample", 6), U.sample_batch(noisy, ptr, 4, 3, "sample", 6), "noisy")
    pop.close()


# ---- 9. device input ----
def test_device_in_stays_on_the_device_and_equals_cpu_in(four_pop):
    ei, ptr = W.batch([four_graphs()[i] for i in (1, 3, 0)])
    host = four_pop.sample_batch([11, 13, 10], t(ptr), t(ei), 16, "sample", 3)
    dev = four_pop.sample_batch(torch.tensor([11, 13, 10], device=DEV), t(ptr).to(DEV), t(ei).to(DEV), 16, "sample", 3)
    assert all(x.is_cuda and x.device.index == 0 for x in dev)
    assert_same(dev, [x.numpy() for x in host], "device in")
    six = four_pop.sample_graphs([11, 13, 10], t(ptr).to(DEV), t(ei).to(DEV), 4, [1, 2, 3])
    assert all(x.is_cuda for x in six)
    assert_same(six, graphs_law(ei, ptr, 4, 3, "sample", [1, 2, 3]), "device sample_graphs")
    asked = four_pop.sample_batch([11, 13, 10], t(ptr), t(ei), 16, "sample", 3, device=DEV)
    assert all(x.is_cuda for x in asked) and all(torch.equal(x, y) for x, y in zip(asked, dev))


# ---- 10. threads and jobs ----
def test_four_threads_sample_from_one_population(four_pop):
    orders = [(10, 11), (13, 12, 10), (11,), (12, 12, 13, 11)]
    cases = []
    for i, order in enumerate(orders):
        ei, ptr = W.batch([four_graphs()[j - 10] for j in order], first=i)
        cases.append((order, ei, ptr, U.sample_batch(ei, ptr, 8, 3, "sample", 50 + i)))
    errors = []

    def work(i):
        order, ei, ptr, want = cases[i]
        try:
            for _ in range(5):
                assert_same(four_pop.sample_batch(order, t(ptr), t(ei), 8, "sample", 50 + i), want, f"thread {i}")
        except BaseException as e:                                  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_two_jobs_finished_in_the_other_order(four_pop):
    from ugs_sampler._lib import check, lib
    jobs = []
    for order, seed in (((10, 12), 1), ((13, 11, 10), 2)):
        ei, ptr = W.batch([four_graphs()[j - 10] for j in order])
        slots = np.array([four_pop._slot[j][0] for j in order], np.int64)
        e, p = t(ei), t(ptr)
        job, total = ctypes.c_void_p(), ctypes.c_int64()
        check(lib.ugs_uniform_population_sample_begin(four_pop._pop, slots.ctypes.data, e.data_ptr(), e.stride(0), e.size(1), p.data_ptr(), len(order),
                                                      6, 0, ctypes.c_uint64(seed), None, 1, None, ctypes.byref(job), ctypes.byref(total)))
        jobs.append((job, total.value, len(order), U.sample_batch(ei, ptr, 6, 3, "sample", seed)))
    for job, total, G, want in reversed(jobs):
        assert total == want[1].shape[1]
        out = [torch.empty((G * 6, 3), dtype=torch.int64), torch.empty((2, total), dtype=torch.int64), torch.empty(G * 6 + 1, dtype=torch.int64),
               torch.empty(G + 1, dtype=torch.int64), torch.empty(total, dtype=torch.int64)]
        check(lib.ugs_uniform_population_sample_finish(job, *[x.data_ptr() for x in out], 0))
        assert_same(out, want, "jobs")
    # a sampler's finish takes no other's job
    assert lib.ugs_uniform_sample_batch_finish(None, None, None, None, None, None, 0) != 0
