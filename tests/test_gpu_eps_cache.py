"""epsilon_uniform_sampler.GraphCache on the GPU: the rows the build kernel writes are those of the host build, entry by entry, and
a batch of added graphs served from them equals the CPU laws (tests/eps_rows.py, tests/eps_graphs_law.py) and the uncached call bit
for bit -- never the cache itself.

In every test a dummy graph is added first, so that no offset into the store is zero; the dataset indices differ from the batch
positions (eps_cache_cases.dataset_index); and the graphs are added in another order than the batch names them
(eps_cache_cases.adding_order).  tests/test_eps_cache_law.py shows on the CPU that the inputs used here reach what they are chosen
for."""
import ctypes as C
import random
import threading

import numpy as np
import pytest
import torch

import eps_cache_cases as CC
import eps_graphs_law
import eps_rows

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
MODES = ("sample", "global")
DEV = torch.device("cuda:0")


def eps():
    import epsilon_uniform_sampler
    return epsilon_uniform_sampler


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def assert_same(got, want, what=""):
    assert len(got) == len(want) == 5, what
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        b = b.cpu().numpy() if torch.is_tensor(b) else b
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def cache_of(graphs, *, seed=0, reserve=(0, 0), calls=1):
    """A cache that holds `graphs` [(n, columns)] under dataset_index(position): the dummy graph first, then the graphs in
    adding_order, in `calls` add_many calls.  Returns the cache and the dataset index of every position."""
    cache = eps().GraphCache("cuda:0", reserve=reserve)
    i, n, a = CC.DUMMY
    cache.add(i, t(a), n)
    order = CC.adding_order(len(graphs), seed)
    per = max(1, -(-len(order) // calls))
    for at in range(0, len(order), per):
        part = order[at:at + per]
        cache.add_many([CC.dataset_index(g) for g in part], [(t(graphs[g][1]), graphs[g][0]) for g in part])
    return cache, [CC.dataset_index(g) for g in range(len(graphs))]


def both_calls(cache, gi, ei, ptr, m, k, mode, seed, epsilon, law, what):
    """the cached and the uncached sample_batch against one law"""
    assert_same(cache.sample_batch(gi, t(ptr), t(ei), m, k, mode, seed, epsilon), law, what + ("cached",))
    assert_same(eps().sample_batch(t(ei), t(ptr), m, k, mode, seed, epsilon), law, what + ("uncached",))


# ---- 1. the build kernel's row order ----
@pytest.mark.parametrize("calls", [1, 8])
def test_the_built_rows_are_the_host_builds_entry_by_entry(calls):
    names = list(CC.BUILD_GRAPHS)
    cache, idx = cache_of([CC.BUILD_GRAPHS[nm] for nm in names], seed=len(names), calls=calls)
    try:
        for nm, i in zip(names, idx):
            n, a = CC.BUILD_GRAPHS[nm]
            rowptr, nbr, ecs = cache.graph_csr(i)
            w_rowptr, w_nbr, w_ecs = CC.rows_of(n, a)
            assert rowptr.tolist() == w_rowptr.tolist(), (nm, "rowptr")
            assert nbr.tolist() == w_nbr.tolist(), (nm, "nbr")
            assert ecs.tolist() == w_ecs.tolist(), (nm, "ecs")
        _, n, a = CC.DUMMY
        assert [x.tolist() for x in cache.graph_csr(CC.DUMMY[0])] == [x.tolist() for x in CC.rows_of(n, a)]
    finally:
        cache.close()


# ---- 2. offsets and order: any batch of added graphs, every k from one cache ----
M2, EPS2, FIRST2 = 5, 0.3, 4


@pytest.fixture(scope="module")
def mixed():
    graphs = CC.mixed_graphs()
    cache, idx = cache_of(graphs, seed=8, calls=2)
    yield cache, idx, graphs
    cache.close()


@pytest.mark.parametrize("k", [3, 6])
def test_a_batch_of_added_graphs_equals_the_law_and_the_uncached_call(mixed, k):
    cache, idx, graphs = mixed
    ei, ptr = CC.batch_of(graphs, first=FIRST2)
    seeds = [(977 * g + 5) for g in range(len(graphs))]
    seeds[0] = (1 << 64) + 12                                           # taken mod 2^64
    assert any(n < k for n, _ in graphs)                                # rows of -1
    for mode in MODES:
        law = eps_rows.sample_rows(ei, ptr, M2, k, mode, 9, EPS2)
        both_calls(cache, idx, ei, ptr, M2, k, mode, 9, EPS2, law, (k, mode))
        law = eps_graphs_law.expected(ei, ptr, M2, k, mode, seeds, EPS2)
        six = cache.sample_graphs(torch.tensor(idx), t(ptr), t(ei), M2, k, seeds, mode, EPS2)
        un = eps().sample_graphs(t(ei), t(ptr), M2, k, seeds, mode, EPS2)
        assert len(six) == 6 and six[5].dtype == torch.bool and six[5].shape == (len(graphs),) and not six[5].any() and not un[5].any()
        assert_same(six[:5], law, (k, mode, "seeds"))
        assert_same(un[:5], law, (k, mode, "seeds", "uncached"))
    assert (law[0][:, 0] >= 0).any() and (law[0][:, 0] < 0).any() and law[4].max() > CC.coff_of(graphs)[1]


def test_one_slot_twice_no_rows_and_no_graphs(mixed):
    cache, idx, graphs = mixed
    picks = [6, 1, 6, 0]                                                # one dataset index named twice
    ei, ptr = CC.batch_of([graphs[g] for g in picks], first=2)
    gi = [idx[g] for g in picks]
    law = eps_rows.sample_rows(ei, ptr, M2, 4, "global", 5, EPS2)
    both_calls(cache, gi, ei, ptr, M2, 4, "global", 5, EPS2, law, ("twice",))
    assert (law[0][2 * M2:3 * M2] >= 0).any()
    got = cache.sample_batch(gi, t(ptr), t(ei), 0, 4)
    assert_same(got, eps_rows.sample_rows(ei, ptr, 0, 4), "m = 0")
    assert got[0].shape == (0, 4) and got[2].tolist() == [0] and got[3].tolist() == [0] * 5
    none, ptr0 = np.zeros((2, 0), np.int64), np.array([3], np.int64)
    assert_same(cache.sample_batch([], t(ptr0), t(none), 4, 3), eps_rows.sample_rows(none, ptr0, 4, 3), "G = 0")
    six = cache.sample_graphs([], t(ptr0), t(none), 4, 3, [])
    assert six[5].shape == (0,)
    assert_same(six[:5], eps_rows.sample_rows(none, ptr0, 4, 3), "G = 0, seeds")


# ---- 3. rows that succeed and rows that fail, at both ends of epsilon ----
@pytest.mark.parametrize("epsilon", [1.0, 0.01])
def test_accepting_and_rejecting_rows(epsilon):
    n, a = CC.path_among_isolated()
    ei, ptr = CC.batch_of([(n, a)], first=10)
    law = {mode: eps_rows.sample_rows(ei, ptr, CC.PATH_ROWS, 5, mode, 8, epsilon) for mode in MODES}
    ok = law["sample"][0][:, 0] >= 0
    assert ok.any() and (~ok).any(), "the law must predict rows of both kinds"
    cache, idx = cache_of([(n, a)])
    try:
        for mode in MODES:
            both_calls(cache, idx, ei, ptr, CC.PATH_ROWS, 5, mode, 8, epsilon, law[mode], (epsilon, mode))
    finally:
        cache.close()


# ---- 4. k = 32: the walk's last LDS slot, through the cache ----
def test_k32_on_forty_vertices():
    g = CC.tu(40, 60, 77)
    ei, ptr = CC.batch_of([g], first=1)
    cache, idx = cache_of([g])
    try:
        for mode in MODES:
            law = eps_rows.sample_rows(ei, ptr, 6, 32, mode, 4, 0.3)
            both_calls(cache, idx, ei, ptr, 6, 32, mode, 4, 0.3, law, ("k = 32", mode))
        assert (law[0][:, 0] >= 0).any()
    finally:
        cache.close()


# ---- 5. regrowth ----
def forty_graphs():
    return [CC.tu(6 + g % 9, 7 + g % 11, 300 + g) for g in range(40)]


def test_random_batches_after_forty_adds_that_regrow():
    graphs = forty_graphs()
    cache = eps().GraphCache("cuda:0", reserve=(1, 1))
    try:
        i, n, a = CC.DUMMY
        cache.add(i, t(a), n)
        gens = [cache.info()["generations"]]
        for g in CC.adding_order(40, 40):
            cache.add(CC.dataset_index(g), t(graphs[g][1]), graphs[g][0])
            gens.append(cache.info()["generations"])
        assert gens[0] == 1 and gens[1] == 2 and gens[2] == 3 and gens[-1] >= 6 and gens == sorted(gens)   # the store doubles: the first adds all regrow
        info = cache.info()
        assert info["graphs"] == 41 and info["half_edges"] == 2 * (5 + sum(a.shape[1] for _, a in graphs))
        assert info["vertices"] == 7 + 1 + sum(n + 1 for n, _ in graphs)
        rnd = random.Random(5)
        for b in range(3):
            picks = rnd.sample(range(40), 8)
            ei, ptr = CC.batch_of([graphs[g] for g in picks], first=b)
            gi = [CC.dataset_index(g) for g in picks]
            for mode in MODES:
                want = eps().sample_batch(t(ei), t(ptr), 6, 4, mode, 70 + b, 0.2)
                assert_same(cache.sample_batch(gi, t(ptr), t(ei), 6, 4, mode, 70 + b, 0.2), want, (b, mode))
            assert (want[0][:, 0] >= 0).any()
    finally:
        cache.close()


def begin_cached(cache, gi, ei, ptr, m, k, seed, epsilon, check=1):
    from ugs_sampler import _graphs
    from ugs_sampler._lib import lib, vp
    slots = np.array([cache._slot[i][0] for i in gi], np.int64)
    job, total = vp(), C.c_int64()
    _graphs._select_device(None, jobs=True)
    rc = lib.ugs_eps_cache_sample_begin(cache._handle(), slots.ctypes.data, ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(gi), m, k,
                                        0, C.c_uint64(seed), None, C.c_double(epsilon), check, None, C.byref(job), C.byref(total))
    assert rc == 0, lib.ugs_last_error()
    assert job.value
    return job, total.value


def finish(job, total, G, m, k):
    from ugs_sampler._lib import lib
    B = G * m
    out = [np.full(s, -7, np.int64) for s in ((B, k), (2, total), (B + 1,), (G + 1,), (total,))]
    assert lib.ugs_eps_sample_batch_finish(job, *[a.ctypes.data for a in out], 0) == 0, lib.ugs_last_error()
    return out


def test_a_job_across_a_regrowth_finishes_on_its_generation():
    torch.cuda.set_device(0)
    graphs = [CC.tu(12 + g, 15 + g, 70 + g) for g in range(6)]
    cache, idx = cache_of(graphs, seed=6)
    try:
        ei, ptr = CC.batch_of([graphs[g] for g in (4, 1, 5)])
        gi = [idx[g] for g in (4, 1, 5)]
        law = eps_rows.sample_rows(ei, ptr, 9, 4, "sample", 21, 0.2)
        before = cache.info()
        job = begin_cached(cache, gi, ei, ptr, 9, 4, 21, 0.2)
        more = [CC.tu(20, 30, 200 + g) for g in range(12)]              # more than the store holds: it cannot fit without a new generation
        cache.add_many(range(2000, 2012), [(t(a), n) for n, a in more])
        after = cache.info()
        assert after["generations"] > before["generations"] and after["vertices"] > 2 * before["vertices"]
        assert_same(finish(*job, 3, 9, 4), law, "begun before the add")
        assert_same(cache.sample_batch(gi, t(ptr), t(ei), 9, 4, seed=21, epsilon=0.2), law, "after the add")
        ei2, ptr2 = CC.batch_of([more[7], graphs[2]])
        assert_same(cache.sample_batch([2007, idx[2]], t(ptr2), t(ei2), 9, 4, seed=3), eps_rows.sample_rows(ei2, ptr2, 9, 4, "sample", 3, 0.1), "old and new")
    finally:
        cache.close()


# ---- 6. the check ----
def test_the_check_names_the_graph_that_differs():
    graphs = [CC.tu(18, 20, 40 + g) for g in range(3)]
    ei, ptr = CC.batch_of(graphs)
    assert all(a.shape[1] == 40 for _, a in graphs)                     # graph 1 owns columns 40 ... 79
    cache, idx = cache_of(graphs, seed=3)
    law = eps_rows.sample_rows(ei, ptr, 8, 5, "sample", 42, 0.1)

    def good():
        assert_same(cache.sample_batch(idx, t(ptr), t(ei), 8, 5), law, "unmutated")

    try:
        good()
        changed = ei.copy()
        changed[1, 55] = ptr[1] + (ei[1, 55] - ptr[1] + 1) % 18         # one endpoint, still inside graph 1
        swapped = ei.copy()
        swapped[:, [43, 57]] = ei[:, [57, 43]]                          # same rows up to their order
        moved = ei.copy()
        moved[:, 79] = ei[:, 80]                                        # graph 1's last column now lies in graph 2: the totals stay
        assert not np.array_equal(ei[:, 43], ei[:, 57])
        for what, bad in (("changed", changed), ("swapped", swapped), ("moved", moved)):
            with pytest.raises(RuntimeError, match=r"graph 1 of the batch differs from the graph added in its place$"):
                cache.sample_batch(idx, t(ptr), t(bad), 8, 5)
            with pytest.raises(RuntimeError, match=r"graph 1 of the batch differs"):
                cache.sample_graphs(idx, t(ptr), t(bad), 8, 5, [1, 2, 3])
            good()
            # without the check nothing of the batch but ptr is read: the added graphs' result
            assert_same(cache.sample_batch(idx, t(ptr), t(bad), 8, 5, check=False), law, (what, "check=False"))
        longer = ptr.copy()
        longer[2:] += 1                                                 # a vertex count is read from ptr: refused with or without the check
        for check in (True, False):
            with pytest.raises(RuntimeError, match=r"graph 1 of the batch has 19 vertices, the graph added in its place has 18$"):
                cache.sample_batch(idx, t(longer), t(ei), 8, 5, check=check)
        with pytest.raises(RuntimeError, match=r"the batch has 119 columns, the added graphs have 120$"):
            cache.sample_batch(idx, t(ptr), t(np.delete(ei, 85, axis=1)), 8, 5)
        good()
        assert_same(cache.sample_batch(idx, t(ptr), None, 8, 5, check=False), law, "no edge_index")
        with pytest.raises(ValueError, match="check=False"):
            cache.sample_batch(idx, t(ptr), None, 8, 5)
        other = [idx[1], idx[0], idx[2]]                                # the right graphs in the wrong places
        with pytest.raises(RuntimeError, match=r"graph 0 of the batch differs"):
            cache.sample_batch(other, t(ptr), t(ei), 8, 5)
        good()
    finally:
        cache.close()


# ---- 7. adding an index again replaces it ----
def test_adding_an_index_again_replaces_the_graph():
    first, second = CC.tu(14, 18, 1), CC.tu(17, 25, 2)
    cache, idx = cache_of([first, CC.tu(11, 13, 3)], seed=2)
    try:
        held = cache.info()

        def samples(graph):
            ei, ptr = CC.batch_of([graph], first=6)
            assert_same(cache.sample_batch([idx[0]], t(ptr), t(ei), 10, 4, "global", 5), eps_rows.sample_rows(ei, ptr, 10, 4, "global", 5, 0.1), graph[0])

        samples(first)
        cache.add(idx[0], t(second[1]), second[0])
        samples(second)
        cache.add(idx[0], t(first[1]), first[0])
        samples(first)
        now = cache.info()
        assert now["graphs"] == held["graphs"] and now["half_edges"] > held["half_edges"]      # the old bytes stay until close
        ei, ptr = CC.batch_of([second], first=6)
        with pytest.raises(RuntimeError, match="graph 0 of the batch has 17 vertices, the graph added in its place has 14"):
            cache.sample_batch([idx[0]], t(ptr), t(ei), 10, 4)
    finally:
        cache.close()


# ---- 8. four threads sample while a fifth adds ----
def test_four_threads_sample_while_a_fifth_adds():
    torch.cuda.set_device(0)
    graphs = forty_graphs()[:12]
    cache = eps().GraphCache("cuda:0", reserve=(1, 1))
    i, n, a = CC.DUMMY
    cache.add(i, t(a), n)
    cache.add_many([CC.dataset_index(g) for g in range(12)], [(t(a), n) for n, a in graphs])
    work_of = []
    for tid in range(4):
        picks = random.Random(100 + tid).sample(range(12), 3)
        ei, ptr = CC.batch_of([graphs[g] for g in picks], first=tid)
        k = 3 + tid % 2
        want = eps_rows.sample_rows(ei, ptr, 4, k, "sample", 30 + tid, 0.2)
        work_of.append(([CC.dataset_index(g) for g in picks], t(ei), t(ptr), k, 30 + tid, want))
    more = [CC.tu(10 + g % 7, 14 + g, 500 + g) for g in range(20)]
    barrier, bad, done = threading.Barrier(5), [], []

    def sample(tid):
        try:
            gi, e, q, k, seed, want = work_of[tid]
            barrier.wait(timeout=60)
            for i in range(20):
                got = cache.sample_batch(gi, q, e if i % 3 else None, 4, k, seed=seed, epsilon=0.2, check=bool(i % 3))
                diff = [nm for nm, x, y in zip(NAMES, got, want) if not np.array_equal(x.cpu().numpy(), y)]
                if diff:
                    bad.append((tid, i, diff))
            done.append(tid)
        except BaseException as err:                                    # (an exception is a finding: recorded, the thread ends)
            bad.append((tid, "exception", repr(err)))

    def add():
        try:
            barrier.wait(timeout=60)
            for g, (n, a) in enumerate(more):
                cache.add(3000 + g, t(a), n)
            done.append(4)
        except BaseException as err:
            bad.append((4, "exception", repr(err)))

    try:
        ts = [threading.Thread(target=sample, args=(tid,), daemon=True) for tid in range(4)] + [threading.Thread(target=add, daemon=True)]
        for th in ts:
            th.start()
        for th in ts:
            th.join(timeout=120)
        assert not any(th.is_alive() for th in ts), "threads did not finish"
        assert not bad, f"{len(bad)} mismatches / exceptions, first: {bad[:6]}"
        assert sorted(done) == [0, 1, 2, 3, 4]
        assert cache.info()["graphs"] == 33 and cache.info()["generations"] >= 4
        ei, ptr = CC.batch_of([more[19], graphs[0]])
        assert_same(cache.sample_batch([3019, CC.dataset_index(0)], t(ptr), t(ei), 4, 3), eps_rows.sample_rows(ei, ptr, 4, 3), "added meanwhile")
    finally:
        cache.close()


# ---- 9. where the outputs go ----
def test_the_outputs_are_on_the_caches_device(mixed):
    cache, idx, graphs = mixed
    picks = [0, 2, 6]
    ei, ptr = CC.batch_of([graphs[g] for g in picks])
    gi = [idx[g] for g in picks]
    law = eps_rows.sample_rows(ei, ptr, M2, 4, "sample", 42, 0.1)
    for kw, q, e in (({}, t(ptr), t(ei)), ({}, t(ptr).cuda(), t(ei)), ({}, t(ptr).cuda(), t(ei).cuda()), (dict(device="cuda:0"), t(ptr), t(ei)),
                     (dict(device="cuda"), t(ptr), t(ei))):
        out = cache.sample_batch(gi, q, e, M2, 4, **kw)
        assert all(x.device == DEV for x in out), (kw, q.device)
        assert_same(out, law, ("placement", tuple(kw), str(q.device), str(e.device)))
    six = cache.sample_graphs(gi, t(ptr), None, M2, 4, [1, 2, 3], check=False, device="cuda:0")
    assert all(x.device == DEV for x in six[:5])
    assert_same(six[:5], eps_graphs_law.expected(ei, ptr, M2, 4, "sample", [1, 2, 3], 0.1), "seeds, no edge_index")


# ---- 10. what is refused before any launch leaves the cache as it was ----
def test_refusals_before_any_launch_have_the_uncached_texts(mixed):
    cache, idx, graphs = mixed
    ei, ptr = CC.batch_of(graphs, first=FIRST2)
    held = cache.info()
    for kw in (dict(k=3, epsilon=0.0), dict(k=3, epsilon=1.5), dict(k=33, epsilon=0.1), dict(k=0, epsilon=0.1)):
        with pytest.raises(RuntimeError) as un:
            eps().sample_batch(t(ei), t(ptr), M2, kw["k"], "sample", 42, kw["epsilon"])
        with pytest.raises(RuntimeError) as ca:
            cache.sample_batch(idx, t(ptr), t(ei), M2, kw["k"], "sample", 42, kw["epsilon"])
        assert type(ca.value) is type(un.value) and str(ca.value) == str(un.value), kw
        with pytest.raises(RuntimeError) as cg:
            cache.sample_graphs(idx, t(ptr), None, M2, kw["k"], list(range(len(idx))), epsilon=kw["epsilon"], check=False)
        assert str(cg.value) == str(un.value), kw
        assert cache.info() == held
    with pytest.raises(RuntimeError, match="^m_per_graph must be >= 0$"):
        cache.sample_batch(idx, t(ptr), t(ei), -1, 3)
    with pytest.raises(KeyError):
        cache.sample_batch([idx[0], 99], t(ptr[:3]), None, M2, 3, check=False)
    assert cache.info() == held
    law = eps_rows.sample_rows(ei, ptr, 2, 3, "sample", 42, 0.1)
    assert_same(cache.sample_batch(idx, t(ptr), t(ei), 2, 3), law, "the cache stays usable")
