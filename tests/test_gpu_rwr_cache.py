"""rwr_sampler.GraphCache on the GPU: a batch of added graphs served from the stored CSRs equals the uncached call and the CPU
laws (tests/rwr_law.py, tests/rwr_row_law.py) bit for bit.

In every test a dummy graph is added first, so that every graph's vertex offset and target offset in the store is non-zero;
the dataset indices differ from the batch positions (rwr_cache_cases.dataset_index); and the graphs are added in another order
than the batch names them (rwr_cache_cases.adding_order).  tests/test_rwr_cache_law.py shows on the CPU that the regrouped batch
a cached call takes has the law of the pinned case it comes from."""
import ctypes as C
import random
import threading

import numpy as np
import pytest
import torch

import rwr_cache_cases as CC
import rwr_law as R
import rwr_paths as P
import rwr_row_law as RR
import rwr_row_paths as Q
import ugs_workloads as wl

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
LAW = {"graph": R, "row": RR}
M64 = (1 << 64) - 1
OVERFLOW_N = 40_000_000                                             # 10 n k > INT_MAX at k = 6


def sampler():
    import rwr_sampler
    return rwr_sampler


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def assert_same(got, want, what=""):
    assert len(got) == len(want) == 5, what
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        b = b.cpu().numpy() if torch.is_tensor(b) else b
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def cache_of(graphs, k, *, seed=0, reserve=(0, 0), calls=1):
    """A cache that holds `graphs` [(n, columns)] under dataset_index(position): the dummy graph first, then the graphs in
    adding_order, in `calls` add_many calls.  Returns the cache and the dataset index of every position."""
    cache = sampler().GraphCache(k, "cuda:0", reserve=reserve)
    i, n, a = CC.DUMMY
    assert cache.add(i, t(a), n)
    order = CC.adding_order(len(graphs), seed)
    per = max(1, -(-len(order) // calls))
    for at in range(0, len(order), per):
        part = order[at:at + per]
        cache.add_many([CC.dataset_index(g) for g in part], [(t(graphs[g][1]), graphs[g][0]) for g in part])
    assert not cache.failed
    return cache, [CC.dataset_index(g) for g in range(len(graphs))]


def through_cache(cache, idx, ei, ptr, m, mode, seed, p, seeds, streams, **kw):
    """sample_graphs when there are per-graph seeds, sample_batch otherwise: the five tensors"""
    if seeds is None:
        return cache.sample_batch(idx, t(ptr), None if ei is None else t(ei), m, mode, seed, p, streams=streams, **kw)
    out = cache.sample_graphs(idx, t(ptr), None if ei is None else t(ei), m, list(seeds), mode, p, streams=streams, **kw)
    assert len(out) == 6 and not out[5].any()
    return out[:5]


# ---- 1. every pinned path of both kernels' inputs, through the cache ----
def path_case(module, name, streams):
    c = module.case(name)
    census = module.census_of(name)
    for cls in c.reaches:
        assert census[cls] > 0, f"the input no longer reaches {cls!r}: choose it again (census: {dict(census)})"
    graphs = CC.split(c.ei, c.ptr)
    ei, ptr = CC.regrouped(c.ei, c.ptr)
    cache, idx = cache_of(graphs, c.k, seed=len(graphs))
    try:
        for mode in ("sample", "global"):
            got = through_cache(cache, idx, ei, ptr, c.m, mode, c.seed, c.p, c.seeds, streams)
            assert_same(got, module.law_of(name, mode), (name, mode))      # the law of the ORIGINAL case
    finally:
        cache.close()


@pytest.mark.parametrize("name", [c.name for c in P.cases()])
def test_path_through_the_cache_equals_law(name):
    path_case(P, name, "graph")


@pytest.mark.parametrize("name", [c.name for c in Q.cases()])
def test_row_path_through_the_cache_equals_row_law(name):
    path_case(Q, name, "row")


# ---- 2. any batch of added graphs ----
K2, M2, P2 = 5, 6, 0.2


def forty_graphs():
    graphs = [P.tu(10 + g % 15, 12 + g % 15 + g % 4, 50 + g) for g in range(38)]
    return graphs + [(3, np.array([[0, 1], [1, 2]], np.int64)), (0, np.zeros((2, 0), np.int64))]      # n < k and n = 0


@pytest.fixture(scope="module")
def forty():
    graphs = forty_graphs()
    cache, idx = cache_of(graphs, K2, seed=40, reserve=(1, 1), calls=3)
    assert cache.info()["generations"] == 4                         # the dummy's add and three more: every add regrew the store
    yield cache, idx, graphs
    cache.close()


def picks_of(kind):
    rnd = random.Random(len(kind))
    if kind == "one":
        return [17], 0
    if kind == "seven_with_a_repeat":
        picks = rnd.sample(range(38), 6)
        return picks[:4] + [picks[1]] + picks[4:], 0                # one dataset index named twice
    if kind == "thirty_three":
        picks = rnd.sample(range(38), 31)
        return picks[:9] + [38] + picks[9:20] + [39] + picks[20:], 0      # the n < k graph and the n = 0 graph among them
    assert kind == "first_vertex_11"
    return rnd.sample(range(40), 5), 11


@pytest.mark.parametrize("kind", ["one", "seven_with_a_repeat", "thirty_three", "first_vertex_11"])
def test_any_batch_of_added_graphs_equals_the_uncached_call_and_the_law(forty, kind):
    cache, idx, graphs = forty
    picks, first = picks_of(kind)
    ei, ptr = P.batch_of([graphs[g] for g in picks], first=first)
    gi = [idx[g] for g in picks]
    seeds = [(977 * g + 5) & M64 for g in range(len(picks))]
    seeds[0] = M64
    for streams in ("graph", "row"):
        for mode in ("sample", "global"):
            what = (kind, streams, mode)
            law = LAW[streams].sample_batch(ei, ptr, M2, K2, mode, 9, P2)
            assert_same(cache.sample_batch(gi, t(ptr), t(ei), M2, mode, 9, P2, streams=streams), law, what)
            assert_same(sampler().sample_batch(t(ei), t(ptr), M2, K2, mode, 9, P2, streams=streams), law, what + ("uncached",))
            law = LAW[streams].sample_batch(ei, ptr, M2, K2, mode, 0, P2, seeds)
            six = cache.sample_graphs(torch.tensor(gi), t(ptr), t(ei), M2, seeds, mode, P2, streams=streams)
            un = sampler().sample_graphs(t(ei), t(ptr), M2, K2, seeds, mode, P2, streams=streams)
            assert len(six) == 6 and not six[5].any() and not un[5].any()
            assert_same(six[:5], law, what + ("seeds",))
            assert_same(un[:5], law, what + ("seeds", "uncached"))
    assert (law[0][:, 0] >= 0).any()


@pytest.mark.parametrize("streams", ["graph", "row"])
def test_no_graphs_and_no_rows(forty, streams):
    cache, idx, graphs = forty
    none, ptr0 = np.zeros((2, 0), np.int64), np.array([3], np.int64)
    assert_same(cache.sample_batch([], t(ptr0), t(none), 4, streams=streams), LAW[streams].sample_batch(none, ptr0, 4, K2), "G = 0")
    six = cache.sample_graphs([], t(ptr0), t(none), 4, [], streams=streams)
    assert six[5].shape == (0,)
    assert_same(six[:5], LAW[streams].sample_batch(none, ptr0, 4, K2), "G = 0, seeds")
    ei, ptr = P.batch_of([graphs[3], graphs[8]])
    got = cache.sample_batch([idx[3], idx[8]], t(ptr), t(ei), 0, streams=streams)
    assert_same(got, LAW[streams].sample_batch(ei, ptr, 0, K2), "m = 0")
    assert got[0].shape == (0, K2) and got[2].tolist() == [0] and got[3].tolist() == [0, 0, 0]


# ---- 3. a job begun before an add finishes on the buffers it began on ----
def begin_cached(cache, gi, ei, ptr, m, seed, rows=0, check=1):
    import ugs_sampler
    from ugs_sampler._lib import lib, vp
    slots = np.array([cache._slot[i][0] for i in gi], np.int64)
    job, total = vp(), C.c_int64()
    ugs_sampler._select_device(None, jobs=True)
    rc = lib.ugs_rwr_cache_sample_begin(cache._handle(), slots.ctypes.data, ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(gi), m,
                                        0, C.c_uint64(seed), None, C.c_double(0.2), rows, check, None, C.byref(job), C.byref(total))
    assert rc == 0, lib.ugs_last_error()
    assert job.value
    return job, total.value


def finish(job, total, G, m, k):
    from ugs_sampler._lib import lib
    B = G * m
    out = [np.full(s, -7, np.int64) for s in ((B, k), (2, total), (B + 1,), (G + 1,), (total,))]
    assert lib.ugs_rwr_sample_batch_finish(job, *[a.ctypes.data for a in out], 0) == 0, lib.ugs_last_error()
    return out


def test_a_job_across_a_regrowth_finishes_on_its_generation():
    torch.cuda.set_device(0)
    graphs = [P.tu(12 + g, 15 + g, 70 + g) for g in range(6)]
    cache, idx = cache_of(graphs, 4, seed=6)
    try:
        ei, ptr = P.batch_of([graphs[g] for g in (4, 1, 5)])
        gi = [idx[g] for g in (4, 1, 5)]
        law = R.sample_batch(ei, ptr, 9, 4, "sample", 21, 0.2)
        before = cache.info()
        job = begin_cached(cache, gi, ei, ptr, 9, 21)
        more = [P.tu(20, 30, 200 + g) for g in range(12)]           # more than the store holds: it cannot fit without a new generation
        cache.add_many(range(2000, 2012), [(t(a), n) for n, a in more])
        after = cache.info()
        assert after["generations"] > before["generations"] and after["vertices"] > 2 * before["vertices"]
        assert_same(finish(*job, 3, 9, 4), law, "begun before the add")
        assert_same(cache.sample_batch(gi, t(ptr), t(ei), 9, seed=21), law, "after the add")
        ei2, ptr2 = P.batch_of([more[7], graphs[2]])
        assert_same(cache.sample_batch([2007, idx[2]], t(ptr2), t(ei2), 9, seed=3), R.sample_batch(ei2, ptr2, 9, 4, "sample", 3, 0.2), "old and new")
    finally:
        cache.close()


# ---- 4. the check ----
def test_the_check_names_the_first_graph_that_differs():
    ei, ptr = wl.tu_batch(18, 20, 4)
    graphs = CC.split(ei, ptr)
    assert all(a.shape[1] == 40 for _, a in graphs)                 # graph 2 owns columns 80 ... 119
    cache, idx = cache_of(graphs, 5, seed=4)
    law = {st: LAW[st].sample_batch(ei, ptr, 8, 5, "sample", 42, 0.2) for st in ("graph", "row")}

    def good():
        for st in ("graph", "row"):
            assert_same(cache.sample_batch(idx, t(ptr), t(ei), 8, streams=st), law[st], ("unmutated", st))

    try:
        good()
        swapped = ei.copy()
        swapped[:, [83, 97]] = ei[:, [97, 83]]                      # same adjacency, another row order
        turned = ei.copy()
        turned[:, 101] = ei[::-1, 101]                              # one column's endpoints exchanged
        replaced = ei.copy()
        replaced[:, 119] = ptr[2]                                   # graph 2's last column replaced by a loop ...
        replaced[:, 120] = ptr[3]                                   # ... and graph 3's first one: the smaller graph is named
        assert not np.array_equal(ei[:, 83], ei[:, 97]) and ei[0, 101] != ei[1, 101]
        for what, bad in (("swapped", swapped), ("turned", turned), ("replaced", replaced)):
            for st in ("graph", "row"):
                with pytest.raises(RuntimeError, match=r"graph 2 of the batch differs from the graph added in its place$"):
                    cache.sample_batch(idx, t(ptr), t(bad), 8, streams=st)
                with pytest.raises(RuntimeError, match=r"graph 2 of the batch differs"):
                    cache.sample_graphs(idx, t(ptr), t(bad), 8, [1, 2, 3, 4], streams=st)
            good()
            # without the check nothing of the batch but ptr is read: the added graphs' result
            assert_same(cache.sample_batch(idx, t(ptr), t(bad), 8, check=False), law["graph"], (what, "check=False"))
        with pytest.raises(RuntimeError, match=r"the batch has 159 columns, the added graphs have 160$"):
            cache.sample_batch(idx, t(ptr), t(np.delete(ei, 85, axis=1)), 8)
        good()
        longer = ptr.copy()
        longer[4] += 1
        with pytest.raises(RuntimeError, match=r"graph 3 of the batch has 19 vertices, the graph added in its place has 18$"):
            cache.sample_batch(idx, t(longer), t(ei), 8)
        good()
        for st in ("graph", "row"):
            assert_same(cache.sample_batch(idx, t(ptr), None, 8, streams=st, check=False), law[st], ("no edge_index", st))
        other = [idx[1], idx[0], idx[2], idx[3]]                    # the right graphs in the wrong places
        with pytest.raises(RuntimeError, match=r"graph 0 of the batch differs"):
            cache.sample_batch(other, t(ptr), t(ei), 8)
        good()
    finally:
        cache.close()


# ---- 5. adding an index again replaces it ----
def test_adding_an_index_again_replaces_the_graph():
    first, second = P.tu(14, 18, 1), P.tu(17, 25, 2)
    cache, idx = cache_of([first, P.tu(11, 13, 3)], 4, seed=2)
    try:
        held = cache.info()

        def samples(graph):
            ei, ptr = P.batch_of([graph], first=6)
            assert_same(cache.sample_batch([idx[0]], t(ptr), t(ei), 10, "global", 5), R.sample_batch(ei, ptr, 10, 4, "global", 5, 0.2), graph[0])

        samples(first)
        assert cache.add(idx[0], t(second[1]), second[0])
        samples(second)
        assert cache.add(idx[0], t(first[1]), first[0])
        samples(first)
        now = cache.info()
        assert now["graphs"] == held["graphs"] and now["half_edges"] > held["half_edges"]      # the old bytes stay until close
        ei, ptr = P.batch_of([second], first=6)
        with pytest.raises(RuntimeError, match="graph 0 of the batch has 17 vertices, the graph added in its place has 14"):
            cache.sample_batch([idx[0]], t(ptr), t(ei), 10)
    finally:
        cache.close()


# ---- 6. a graph whose iteration limit overflows takes no storage and fails alone ----
def test_the_overflowing_graph_fails_alone_and_takes_no_storage():
    live, none = P.tu(18, 20, 7), np.zeros((2, 0), np.int64)
    cache = sampler().GraphCache(6, "cuda:0")
    try:
        i, n, a = CC.DUMMY
        assert cache.add(i, t(a), n)
        cache.add_many([31, 32], [(t(none), OVERFLOW_N), (t(live[1]), live[0])])
        assert cache.failed == {31} and not cache.add(33, t(none), OVERFLOW_N) and cache.failed == {31, 33}
        info = cache.info()
        assert info["graphs"] == 4 and info["vertices"] < 100 and info["bytes"] < 1 << 16
        ei, ptr = P.batch_of([live, (OVERFLOW_N, none)], first=2)
        m, seeds = 5, [3, 4]
        with pytest.raises(RuntimeError, match=rf"^rwr_sampler: graph 1 has {OVERFLOW_N} vertices; 10 n k must fit the reference's int iteration limit$"):
            cache.sample_batch([32, 31], t(ptr), t(ei), m)
        for streams in ("graph", "row"):
            six = cache.sample_graphs([32, 31], t(ptr), t(ei), m, seeds, "global", streams=streams)
            assert six[5].tolist() == [False, True]
            b = LAW[streams].sample_batch(ei, ptr[:2], m, 6, "global", seeds[0], 0.2)    # the law: graph 0's block is its one-graph call
            want = (np.concatenate([b[0], np.full((m, 6), -1, np.int64)]), b[1], np.concatenate([b[2], np.full(m, b[2][-1], np.int64)]),
                    np.arange(3, dtype=np.int64) * m, b[4])
            assert_same(six[:5], want, streams)
            assert (b[0][:, 0] >= 0).any()
        ei1, ptr1 = P.batch_of([live])
        assert_same(cache.sample_batch([32], t(ptr1), t(ei1), m), R.sample_batch(ei1, ptr1, m, 6), "the cache stays usable")
    finally:
        cache.close()


# ---- 7. host threads, and jobs finished in another order ----
def test_four_host_threads_sample_different_batches_from_one_cache(forty):
    cache, idx, graphs = forty
    torch.cuda.set_device(0)
    work_of = []
    for tid in range(4):
        picks = random.Random(100 + tid).sample(range(40), 3 + 4 * tid)
        ei, ptr = P.batch_of([graphs[g] for g in picks], first=tid)
        streams = ("graph", "row")[tid % 2]
        want = LAW[streams].sample_batch(ei, ptr, M2, K2, "sample", 30 + tid, P2)
        work_of.append(([idx[g] for g in picks], t(ei), t(ptr), streams, 30 + tid, want))
    barrier, bad, done = threading.Barrier(4), [], []

    def work(tid):
        try:
            gi, e, q, streams, seed, want = work_of[tid]
            barrier.wait(timeout=60)
            for i in range(25):
                got = cache.sample_batch(gi, q, e if i % 3 else None, M2, seed=seed, p_restart=P2, streams=streams, check=bool(i % 3))
                diff = [nm for nm, a, b in zip(NAMES, got, want) if not np.array_equal(a.numpy(), b)]
                if diff:
                    bad.append((tid, i, diff))
            done.append(tid)
        except BaseException as err:                                 # (an exception is a finding: recorded, the thread ends)
            bad.append((tid, "exception", repr(err)))

    ts = [threading.Thread(target=work, args=(tid,), daemon=True) for tid in range(4)]
    for th in ts:
        th.start()
    for th in ts:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ts), "threads did not finish"
    assert not bad, f"{len(bad)} mismatches / exceptions, first: {bad[:6]}"
    assert sorted(done) == [0, 1, 2, 3]


def test_two_cached_jobs_finish_in_the_other_order(forty):
    cache, idx, graphs = forty
    torch.cuda.set_device(0)
    spec = {}
    for key, picks, m, seed, rows in (("A", [5, 30, 2], 7, 11, 0), ("B", [9, 9, 1, 36, 20], 12, 12, 1)):
        ei, ptr = P.batch_of([graphs[g] for g in picks])
        spec[key] = ([idx[g] for g in picks], ei, ptr, m, seed, rows)
    jobs = {key: begin_cached(cache, gi, ei, ptr, m, seed, rows) for key, (gi, ei, ptr, m, seed, rows) in spec.items()}
    for key in ("B", "A"):
        gi, ei, ptr, m, seed, rows = spec[key]
        law = (RR if rows else R).sample_batch(ei, ptr, m, K2, "sample", seed, 0.2)
        assert_same(finish(*jobs[key], len(gi), m, K2), law, key)


# ---- 8. where the outputs go ----
def test_host_input_gives_pinned_outputs_and_device_gives_device_outputs(forty):
    cache, idx, graphs = forty
    picks = [4, 22, 13]
    ei, ptr = P.batch_of([graphs[g] for g in picks])
    gi = [idx[g] for g in picks]
    for streams in ("graph", "row"):
        law = LAW[streams].sample_batch(ei, ptr, M2, K2, "sample", 42, P2)
        host = cache.sample_batch(gi, t(ptr), t(ei), M2, p_restart=P2, streams=streams)
        assert all(x.device.type == "cpu" and x.is_pinned() for x in host)
        assert_same(host, law, "host")
        for kw, q in ((dict(device="cuda:0"), t(ptr)), (dict(device="cuda"), t(ptr)), ({}, t(ptr).cuda())):
            dev = cache.sample_batch(gi, q, t(ei), M2, p_restart=P2, streams=streams, **kw)
            assert all(x.device == torch.device("cuda:0") for x in dev)
            assert_same(dev, law, ("device", tuple(kw)))
        six = cache.sample_graphs(gi, t(ptr), None, M2, [1, 2, 3], p_restart=P2, streams=streams, check=False, device="cuda:0")
        assert all(x.device == torch.device("cuda:0") for x in six)
        assert_same(six[:5], LAW[streams].sample_batch(ei, ptr, M2, K2, "sample", 0, P2, [1, 2, 3]), "device, seeds, no edge_index")
