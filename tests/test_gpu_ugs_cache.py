"""ugs_sampler.GraphCache on the GPU: a batch of added graphs served from the store equals the CPU oracle with a fresh LRU, bit for
bit -- and, in addition, the uncached call made right after clear_cache().

In every test a dummy graph is added first, so that no base in the store is zero; the dataset indices differ from the batch
positions (ugs_cache_cases.dataset_index); and the graphs are added in another order than the batch names them
(ugs_cache_cases.adding_order).  tests/test_ugs_cache_law.py shows on the CPU why a graph may be served from a store at all."""
import ctypes as C
import random
import threading

import numpy as np
import pytest
import torch

import oracle
import ugs_cache_cases as CC
import ugs_graphs_law
import ugs_workloads as wl

pytestmark = pytest.mark.gpu
NAMES = CC.NAMES


def sampler():
    import ugs_sampler
    return ugs_sampler


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
    """A cache that holds `graphs` [(columns, n)] under dataset_index(position): the dummy graph first, then the graphs in
    adding_order, in `calls` add_many calls."""
    cache = sampler().GraphCache(k, "cuda:0", reserve=reserve)
    i, a, n = CC.DUMMY
    cache.add(i, t(a), n)
    order = CC.adding_order(len(graphs), seed)
    per = max(1, -(-len(order) // calls))
    for at in range(0, len(order), per):
        part = order[at:at + per]
        cache.add_many([CC.dataset_index(g) for g in part], [(t(graphs[g][0]), graphs[g][1]) for g in part])
    return cache


def through_cache(cache, gi, ei, ptr, m, mode, seed, seeds, **kw):
    """sample_graphs when there are per-graph seeds, sample_batch otherwise: the five tensors"""
    if seeds is None:
        return cache.sample_batch(gi, t(ptr), None if ei is None else t(ei), m, mode, seed, **kw)
    out = cache.sample_graphs(gi, t(ptr), None if ei is None else t(ei), m, list(seeds), mode, **kw)
    assert len(out) == 6 and out[5].dtype == torch.bool and out[5].shape == (len(gi),) and not out[5].any()
    return out[:5]


def uncached(ei, ptr, m, k, mode, seed, seeds):
    """the uncached call right after clear_cache()"""
    s = sampler()
    s.clear_cache()
    if seeds is None:
        return s.sample_batch(t(ei), t(ptr), m, k, mode, seed)
    return s.sample_graphs(t(ei), t(ptr), m, k, list(seeds), mode)[:5]


@pytest.fixture(scope="module")
def laws():
    return {c.name: CC.batch_law(c) for c in CC.cases()}


S_FILLS = ("ugs_fill_scan<8>", "ugs_fill<8>")          # tier S: the packed step, or the ordinary fill where it does not apply


def run_case(c, law, walks, fills=S_FILLS):
    ei, ptr, _ = CC.collate(c)
    gi = [CC.dataset_index(p) for p in c.picks]
    cache = cache_of(c.graphs, c.k, seed=len(c.graphs))
    try:
        stats = sampler().cache_stats()
        host = through_cache(cache, gi, ei, ptr, c.m, c.mode, c.seed, c.seeds)
        launch = cache.last_launch()
        assert all(x.device.type == "cpu" and x.is_pinned() for x in host)
        assert_same(host, law, (c.name, "host"))
        dev = through_cache(cache, torch.tensor(gi, dtype=torch.int64), ei, ptr, c.m, c.mode, c.seed, c.seeds, device="cuda:0")
        assert all(x.device == torch.device("cuda:0") for x in dev)
        assert_same(dev, law, (c.name, "device"))
        assert sampler().cache_stats() == stats, "a cached call touched the LRU"
        assert launch[0] in walks, (c.name, launch)
        total = int(law[2][-1])
        assert launch[1] in (fills if total > 0 else ("", "ugs_fill_scan<8>")), (c.name, launch)
    finally:
        cache.close()
    assert_same(uncached(ei, ptr, c.m, c.k, c.mode, c.seed, c.seeds), law, (c.name, "uncached"))
    sampler().clear_cache()


# ---- 1. every case: host and device outputs, the oracle and the uncached call ----
@pytest.mark.parametrize("name", [c.name for c in CC.cases() if c.tier is None])
def test_case_through_the_cache_equals_the_fresh_lru_oracle(name, laws, monkeypatch):
    monkeypatch.delenv("UGS_FORCE_TIER", raising=False)
    c = CC.case(name)
    if name == "star70_k3":                              # bound 70 and 1.3 x 70 + 16 > 64: the 448 tier, which cannot hand a walk on
        run_case(c, laws[name], ("ugs_walk_lds<64,448>",), ("ugs_fill<64>",))
    else:
        run_case(c, laws[name], CC.S_WALKS)


@pytest.mark.parametrize("tier", [None, "0", "1", "2", "3", "4", "5"])
@pytest.mark.parametrize("name", [c.name for c in CC.cases() if c.tier == "every"])
def test_dense_case_under_every_first_tier(name, tier, laws, monkeypatch):
    if tier is None:
        monkeypatch.delenv("UGS_FORCE_TIER", raising=False)
        walks, fills = CC.LDS_WALKS[1:], ("ugs_fill<64>",)          # bound > 64 and a mean above tier S's margin: a 64-lane tier
    else:
        monkeypatch.setenv("UGS_FORCE_TIER", tier)
        walks, fills = (CC.LDS_WALKS[int(tier)],), ("ugs_fill<8>" if tier == "0" else "ugs_fill<64>",)
    run_case(CC.case(name), laws[name], walks, fills)


def test_three_hubs_reach_the_global_tier(laws, monkeypatch):
    monkeypatch.delenv("UGS_FORCE_TIER", raising=False)
    c = CC.case("three_hubs_2600")
    assert c.census[0][2] > CC.TIER_CAP[-1]              # no LDS tier holds the bound: the largest one starts and hands on to the global tier
    run_case(c, laws[c.name], ("ugs_walk_lds<64,2048>",), ("ugs_fill<64>",))


# ---- 2. any batch of added graphs, from a store that regrew at every add ----
K2, M2 = 5, 6


def forty_graphs():
    graphs = [CC.tu(10 + g % 15, 12 + g % 15 + g % 4, 50 + g) for g in range(38)]
    return graphs + [(CC.both([(0, 1), (1, 2)]), 3), (CC.NONE, 0)]      # n < k and n = 0


@pytest.fixture(scope="module")
def forty():
    graphs = forty_graphs()
    stats = sampler().cache_stats()
    cache = cache_of(graphs, K2, seed=40, reserve=(1, 1), calls=3)
    assert cache.info()["generations"] == 4                             # the dummy's add and three more: every add regrew the store
    assert sampler().cache_stats() == stats, "add_many touched the LRU"
    yield cache, [CC.dataset_index(g) for g in range(len(graphs))], graphs
    cache.close()


def batch_of(graphs, first=0):
    ptr, cols = [first], []
    for a, n in graphs:
        cols.append(a + ptr[-1])
        ptr.append(ptr[-1] + n)
    return np.ascontiguousarray(np.concatenate(cols, axis=1) if cols else CC.NONE), np.array(ptr, np.int64)


def picks_of(kind):
    rnd = random.Random(len(kind))
    if kind == "one":
        return [17], 0
    if kind == "seven_with_a_repeat":
        picks = rnd.sample(range(38), 6)
        return picks[:4] + [picks[1]] + picks[4:], 0                    # one dataset index named twice
    assert kind == "thirty_three"
    picks = rnd.sample(range(38), 31)
    return picks[:9] + [38] + picks[9:20] + [39] + picks[20:], 11       # the n < k graph and the n = 0 graph among them; ptr[0] = 11


@pytest.mark.parametrize("kind", ["one", "seven_with_a_repeat", "thirty_three"])
def test_any_batch_of_added_graphs_equals_the_uncached_call_and_the_oracle(forty, kind):
    cache, idx, graphs = forty
    picks, first = picks_of(kind)
    ei, ptr = batch_of([graphs[g] for g in picks], first=first)
    gi = [idx[g] for g in picks]
    seeds = [977 * g - 5000 for g in range(len(picks))]
    seeds[0] = 0
    for mode in ("sample", "graph", "global"):
        law = oracle.sample_batch(ei, ptr, M2, K2, mode, 9)
        assert_same(cache.sample_batch(gi, t(ptr), t(ei), M2, mode, 9), law, (kind, mode))
        assert_same(uncached(ei, ptr, M2, K2, mode, 9, None), law, (kind, mode, "uncached"))
        lru = oracle.Cache()
        law = ugs_graphs_law.oracle_loop(ei, ptr, M2, K2, mode, seeds, lru)
        lru.close()
        six = cache.sample_graphs(torch.tensor(gi), t(ptr), t(ei), M2, seeds, mode)
        assert len(six) == 6 and not six[5].any()
        assert_same(six[:5], law, (kind, mode, "seeds"))
        assert_same(uncached(ei, ptr, M2, K2, mode, 0, seeds), law, (kind, mode, "seeds", "uncached"))
    assert (law[0][:, 0] >= 0).any()
    sampler().clear_cache()


def test_no_graphs_and_no_rows(forty):
    cache, idx, graphs = forty
    none, ptr0 = CC.NONE, np.array([3], np.int64)
    assert_same(cache.sample_batch([], t(ptr0), t(none), 4), oracle.sample_batch(none, ptr0, 4, K2), "G = 0")
    assert_same(sampler().sample_batch(t(none), t(ptr0), 4, K2), oracle.sample_batch(none, ptr0, 4, K2), "G = 0, uncached")
    six = cache.sample_graphs([], t(ptr0), t(none), 4, [])
    assert six[5].shape == (0,)
    assert_same(six[:5], oracle.sample_batch(none, ptr0, 4, K2), "G = 0, seeds")
    ei, ptr = batch_of([graphs[3], graphs[8]])
    got = cache.sample_batch([idx[3], idx[8]], t(ptr), t(ei), 0)
    assert_same(got, oracle.sample_batch(ei, ptr, 0, K2), "m = 0")
    assert_same(sampler().sample_batch(t(ei), t(ptr), 0, K2), oracle.sample_batch(ei, ptr, 0, K2), "m = 0, uncached")
    assert got[0].shape == (0, K2) and got[2].tolist() == [0] and got[3].tolist() == [0, 0, 0]
    sampler().clear_cache()


# ---- 3. a job begun before an add finishes on the buffers it began on; jobs finished in another order ----
def begin_cached(cache, gi, ei, ptr, m, seed, check=1):
    s = sampler()
    from ugs_sampler._lib import lib, vp
    slots = np.array([cache._slot[i][0] for i in gi], np.int64)
    job, total = vp(), C.c_int64()
    s._select_device(None, jobs=True)
    rc = lib.ugs_graph_cache_sample_begin(cache._handle(), slots.ctypes.data, ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(gi), m,
                                          0, seed, None, check, C.byref(job), C.byref(total))
    assert rc == 0, lib.ugs_last_error()
    assert job.value
    return job, total.value


def finish(job, total, G, m, k):
    from ugs_sampler._lib import lib
    B = G * m
    out = [np.full(s, -7, np.int64) for s in ((B, k), (2, total), (B + 1,), (G + 1,), (total,))]
    assert lib.ugs_sample_batch_finish(job, *[a.ctypes.data for a in out], 0) == 0, lib.ugs_last_error()
    return out


def test_a_job_across_a_regrowth_finishes_on_its_generation():
    torch.cuda.set_device(0)
    graphs = [CC.tu(12 + g, 15 + g, 70 + g) for g in range(6)]
    cache = cache_of(graphs, 4, seed=6)
    idx = [CC.dataset_index(g) for g in range(6)]
    try:
        ei, ptr = batch_of([graphs[g] for g in (4, 1, 5)])
        gi = [idx[g] for g in (4, 1, 5)]
        law = oracle.sample_batch(ei, ptr, 9, 4, "sample", 21)
        before = cache.info()
        job = begin_cached(cache, gi, ei, ptr, 9, 21)
        more = [CC.tu(20, 30, 200 + g) for g in range(12)]              # more than the store holds: it cannot fit without a new generation
        cache.add_many(range(2000, 2012), [(t(a), n) for a, n in more])
        after = cache.info()
        assert after["generations"] > before["generations"] and after["vertices"] > 2 * before["vertices"]
        assert_same(finish(*job, 3, 9, 4), law, "begun before the add")
        assert_same(cache.sample_batch(gi, t(ptr), t(ei), 9, seed=21), law, "after the add")
        ei2, ptr2 = batch_of([more[7], graphs[2]])
        assert_same(cache.sample_batch([2007, idx[2]], t(ptr2), t(ei2), 9, seed=3), oracle.sample_batch(ei2, ptr2, 9, 4, "sample", 3), "old and new")
    finally:
        cache.close()


def test_two_cached_jobs_finish_in_the_other_order(forty):
    cache, idx, graphs = forty
    torch.cuda.set_device(0)
    spec = {}
    for key, picks, m, seed in (("A", [5, 30, 2], 7, 11), ("B", [9, 9, 1, 36, 20], 12, 12)):
        ei, ptr = batch_of([graphs[g] for g in picks])
        spec[key] = ([idx[g] for g in picks], ei, ptr, m, seed)
    jobs = {key: begin_cached(cache, gi, ei, ptr, m, seed) for key, (gi, ei, ptr, m, seed) in spec.items()}
    for key in ("B", "A"):
        gi, ei, ptr, m, seed = spec[key]
        assert_same(finish(*jobs[key], len(gi), m, K2), oracle.sample_batch(ei, ptr, m, K2, "sample", seed), key)


def test_four_host_threads_sample_while_a_fifth_adds(forty):
    cache, idx, graphs = forty
    torch.cuda.set_device(0)
    work_of = []
    for tid in range(4):
        picks = random.Random(100 + tid).sample(range(40), 3 + 4 * tid)
        ei, ptr = batch_of([graphs[g] for g in picks], first=tid)
        want = oracle.sample_batch(ei, ptr, M2, K2, "sample", 30 + tid)
        work_of.append(([idx[g] for g in picks], t(ei), t(ptr), 30 + tid, want))
    extra = [CC.tu(25 + g % 10, 40 + g, 900 + g) for g in range(40)]   # more vertices than the store holds: it has to regrow on the way
    barrier, bad, done = threading.Barrier(5), [], []

    def work(tid):
        try:
            gi, e, q, seed, want = work_of[tid]
            barrier.wait(timeout=60)
            for i in range(25):
                got = cache.sample_batch(gi, q, e if i % 3 else None, M2, seed=seed, check=bool(i % 3))
                diff = [nm for nm, a, b in zip(NAMES, got, want) if not np.array_equal(a.numpy(), b)]
                if diff:
                    bad.append((tid, i, diff))
            done.append(tid)
        except BaseException as err:                                 # (an exception is a finding: recorded, the thread ends)
            bad.append((tid, "exception", repr(err)))

    def adder():
        try:
            barrier.wait(timeout=60)
            for g, (a, n) in enumerate(extra):                       # one add each: the store (reserve 1, 1) regrows while the others sample
                cache.add(5000 + g, t(a), n)
            done.append(4)
        except BaseException as err:
            bad.append((4, "exception", repr(err)))

    gens = cache.info()["generations"]
    ts = [threading.Thread(target=work, args=(tid,), daemon=True) for tid in range(4)] + [threading.Thread(target=adder, daemon=True)]
    for th in ts:
        th.start()
    for th in ts:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in ts), "threads did not finish"
    assert not bad, f"{len(bad)} mismatches / exceptions, first: {bad[:6]}"
    assert sorted(done) == [0, 1, 2, 3, 4]
    assert cache.info()["generations"] > gens
    ei, ptr = batch_of([extra[39], graphs[0]])
    assert_same(cache.sample_batch([5039, idx[0]], t(ptr), t(ei), M2, seed=4), oracle.sample_batch(ei, ptr, M2, K2, "sample", 4), "added meanwhile")


# ---- 4. the check ----
def test_the_check_names_the_first_graph_that_differs():
    ei, ptr = wl.tu_batch(18, 20, 4)
    graphs = [(np.ascontiguousarray(ei[:, 40 * g:40 * (g + 1)] - ptr[g]), 18) for g in range(4)]      # graph 2 owns columns 80 ... 119
    cache = cache_of(graphs, 5, seed=4)
    idx = [CC.dataset_index(g) for g in range(4)]
    law = oracle.sample_batch(ei, ptr, 8, 5, "sample", 42)

    def good():
        assert_same(cache.sample_batch(idx, t(ptr), t(ei), 8), law, "unmutated")

    try:
        good()
        swapped = ei.copy()
        swapped[:, [83, 97]] = ei[:, [97, 83]]                      # two columns of graph 2 exchanged
        turned = ei.copy()
        turned[:, 101] = ei[::-1, 101]                              # one column's endpoints exchanged
        replaced = ei.copy()
        replaced[:, 119] = ptr[2]                                   # graph 2's last column replaced by a loop ...
        replaced[:, 120] = ptr[3]                                   # ... and graph 3's first one: the smaller graph is named
        assert not np.array_equal(ei[:, 83], ei[:, 97]) and ei[0, 101] != ei[1, 101]
        for what, bad in (("swapped", swapped), ("turned", turned), ("replaced", replaced)):
            with pytest.raises(RuntimeError, match=r"graph 2 of the batch differs from the graph added in its place$"):
                cache.sample_batch(idx, t(ptr), t(bad), 8)
            with pytest.raises(RuntimeError, match=r"graph 2 of the batch differs"):
                cache.sample_graphs(idx, t(ptr), t(bad), 8, [1, 2, 3, 4], device="cuda:0")
            good()
            # without the check nothing of the batch but ptr is read: the added graphs' result
            assert_same(cache.sample_batch(idx, t(ptr), t(bad), 8, check=False), law, (what, "check=False"))
        with pytest.raises(RuntimeError, match=r"the batch has 159 columns, the added graphs have 160$"):
            cache.sample_batch(idx, t(ptr), t(np.delete(ei, 85, axis=1)), 8)
        good()
        longer = ptr.copy()
        longer[4] += 1
        with pytest.raises(RuntimeError, match=r"graph 3 of the batch has 19 vertices, the graph added in its place has 18$"):
            cache.sample_batch(idx, t(longer), t(ei), 8)
        good()
        assert_same(cache.sample_batch(idx, t(ptr), None, 8, check=False), law, "no edge_index")
        assert_same(cache.sample_batch(idx, t(ptr).cuda(), None, 8, check=False), law, "no edge_index, ptr on the device")
        other = [idx[1], idx[0], idx[2], idx[3]]                    # the right graphs in the wrong places
        with pytest.raises(RuntimeError, match=r"graph 0 of the batch differs"):
            cache.sample_batch(other, t(ptr), t(ei), 8)
        good()
    finally:
        cache.close()


# ---- 5. adding an index again replaces it ----
def test_adding_an_index_again_replaces_the_graph():
    first, second = CC.tu(14, 18, 1), CC.tu(17, 25, 2)
    cache = cache_of([first, CC.tu(11, 13, 3)], 4, seed=2)
    i0 = CC.dataset_index(0)
    try:
        held = cache.info()

        def samples(graph):
            ei, ptr = batch_of([graph], first=6)
            assert_same(cache.sample_batch([i0], t(ptr), t(ei), 10, "global", 5), oracle.sample_batch(ei, ptr, 10, 4, "global", 5), graph[1])

        samples(first)
        cache.add(i0, t(second[0]), second[1])
        samples(second)
        cache.add(i0, t(first[0]), first[1])
        samples(first)
        now = cache.info()
        assert now["graphs"] == held["graphs"] and now["csr_entries"] > held["csr_entries"]      # the old bytes stay until close
        ei, ptr = batch_of([second], first=6)
        with pytest.raises(RuntimeError, match="graph 0 of the batch has 17 vertices, the graph added in its place has 14"):
            cache.sample_batch([i0], t(ptr), t(ei), 10)
    finally:
        cache.close()


# ---- 6. the cache and the LRU do not know of each other ----
def test_the_cache_is_independent_of_the_lru_and_the_deviation_is_real():
    s = sampler()
    graphs = [CC.tu(20 + g, 30 + 2 * g, 300 + g) for g in range(6)]
    ei, ptr = batch_of(graphs)
    idx = [CC.dataset_index(g) for g in range(6)]
    s.clear_cache()
    s.sample_batch(t(ei), t(ptr), 16, 4, "sample", 42)                  # the LRU now holds every graph, preprocessed at k = 4
    held = s.cache_stats()
    assert held["size"] == 6
    cache = cache_of(graphs, 5, seed=9)
    try:
        assert s.cache_stats() == held, "add_many touched the LRU"
        law = oracle.sample_batch(ei, ptr, 16, 5, "sample", 42)         # a fresh LRU
        assert_same(cache.sample_batch(idx, t(ptr), t(ei), 16, "sample", 42), law, "cached, after an uncached call at k = 4")
        assert s.cache_stats() == held, "a cached call touched the LRU"
        # the uncached call at this point reuses the k = 4 preprocessing (the key ignores k: fixture f5's quirk) -- with the oracle on
        # an LRU of the same history it agrees, with the fresh-LRU oracle it does not: the deviation the cache states is real
        lru = oracle.Cache()
        oracle.sample_batch(ei, ptr, 16, 4, "sample", 42, lru)
        quirk = oracle.sample_batch(ei, ptr, 16, 5, "sample", 42, lru)
        lru.close()
        got = s.sample_batch(t(ei), t(ptr), 16, 5, "sample", 42)
        assert_same(got, quirk, "uncached, LRU with history")
        assert not np.array_equal(got[0].numpy(), law[0]), "the batch does not show the quirk: choose it again"
        assert s.cache_stats()["hits"] == held["hits"] + 6
    finally:
        cache.close()
        s.clear_cache()
