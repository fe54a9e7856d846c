"""uniform_sampler.sample_distinct and PopulationCache.sample_distinct (ugs_uniform.hip: uni_draw_distinct, and the row and fill
kernels of both calls and both forms with rows of -1 inside live graphs) against the law: the expected tensors are the law's indices
(tests/uniform_distinct_law.py) into the rows enumerate_graphs gives for the same batch, every tensor bit for bit.  The batches are
uniform_distinct_law.GPU_CASES -- graphs whose population size is known in closed form; tests/test_uniform_distinct_law.py shows that
they reach every class of the kernel's resolution and tell its one-line mutants apart.  The vertex limit is process-wide, so what
raises it restores it."""
import contextlib
import functools
import threading

import numpy as np
import pytest
import torch

import uniform_distinct_law as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src", "failed", "valid")


def us():
    import uniform_sampler
    return uniform_sampler


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@contextlib.contextmanager
def vertex_limit(n):
    prev = us().set_max_vertices(n)
    try:
        yield
    finally:
        us().set_max_vertices(prev)


def rebuild(en, sizes, seeds, m, k):
    """The seven tensors of a distinct call from the enumeration `en` of the same batch in the same mode"""
    nodes_e, eidx_e, eptr_e, sptr_e, esrc_e = en[:5]
    G = len(sizes)
    sel = np.array([sptr_e[g] + d if d >= 0 else -1 for g in range(G) for d in D.law(seeds[g], sizes[g], m)], np.int64).reshape(-1)
    live = sel >= 0
    if not live.any():
        return (np.full((G * m, k), -1, np.int64), np.zeros((2, 0), np.int64), np.zeros(G * m + 1, np.int64), np.arange(G + 1, dtype=np.int64) * m,
                np.zeros(0, np.int64), np.zeros(G, bool), np.zeros(G, np.int64))
    s = np.where(live, sel, 0)
    nodes = np.where(live[:, None], nodes_e[s], -1)
    cnt = np.where(live, eptr_e[s + 1] - eptr_e[s], 0)
    eptr = np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt)])
    src = np.repeat(eptr_e[s] - eptr[:-1], cnt) + np.arange(eptr[-1])
    valid = np.array([min(m, max(N, 0)) for N in sizes], np.int64)
    return nodes, eidx_e[:, src], eptr, np.arange(G + 1, dtype=np.int64) * m, esrc_e[src], np.zeros(G, bool), valid


def assert_same(got, want, what=""):
    assert len(got) == 7
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == b.dtype and a.shape == b.shape, (what, nm, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


@functools.lru_cache(maxsize=None)
def case(name):
    """The batch of a GPU case (vertices from 2 on, columns shuffled), its population (indices 100 ...) and its enumeration per mode"""
    k, m, ei, ptr, sizes, seeds, limit, graphs = D.case_batch(name, first=2)
    ei = np.ascontiguousarray(ei[:, np.random.RandomState(3).permutation(ei.shape[1])])
    idx = list(range(100, 100 + len(graphs)))
    with vertex_limit(limit):
        pop = us().PopulationCache(k, DEV)
        pop.add_many(idx, [(t(e), n) for n, e in graphs])
        en = {mode: [x.numpy() for x in us().enumerate_graphs(t(ei), t(ptr), k, mode)] for mode in ("sample", "global")}
    assert pop.failed == set() and not en["sample"][5].any()
    assert np.diff(en["sample"][3]).tolist() == sizes == [max(x, 0) for x in pop.sizes(idx).tolist()]     # the closed forms
    return dict(k=k, m=m, ei=ei, ptr=ptr, sizes=sizes, seeds=seeds, limit=limit, pop=pop, idx=idx, en=en)


# ---- 1. every case, both calls, both modes ----
@pytest.mark.parametrize("mode", ["sample", "global"])
@pytest.mark.parametrize("name", sorted(D.GPU_CASES))
def test_both_calls_equal_the_law_over_the_enumeration(name, mode):
    c = case(name)
    want = rebuild(c["en"][mode], c["sizes"], c["seeds"], c["m"], c["k"])
    with vertex_limit(c["limit"]):
        unc = us().sample_distinct(t(c["ei"]), t(c["ptr"]), c["m"], c["k"], c["seeds"], mode)
    got = c["pop"].sample_distinct(c["idx"], t(c["ptr"]), t(c["ei"]), c["m"], c["seeds"], mode)
    assert_same(unc, want, f"{name} uncached")
    assert_same(got, want, f"{name} cached")
    assert all(torch.equal(a, b) for a, b in zip(unc, got))
    # distinct rows inside every graph, -1 rows only behind the real ones
    nodes = got[0].numpy().reshape(len(c["sizes"]), c["m"], c["k"])
    for g, N in enumerate(c["sizes"]):
        q = min(c["m"], N)
        assert len({tuple(r) for r in nodes[g, :q]}) == q and (nodes[g, :q] >= 0).all() and (nodes[g, q:] == -1).all()
    nocheck = c["pop"].sample_distinct(c["idx"], t(c["ptr"]), t(c["ei"]), c["m"], c["seeds"], mode, check=False)
    assert all(torch.equal(a, b) for a, b in zip(nocheck, got))


# ---- 2. the full bag ----
def test_m_equal_to_every_population_gives_the_enumeration_itself():
    k, n, G = 4, 9, 5
    graphs = [D.cycle(n)] * G
    ptr = np.arange(G + 1, dtype=np.int64) * n
    ei = np.concatenate([e + ptr[g] for g, (_, e) in enumerate(graphs)], axis=1)
    en = us().enumerate_graphs(t(ei), t(ptr), k)
    assert en[3].tolist() == [n * g for g in range(G + 1)]          # equal populations: sample_ptr is g * m
    pop = us().PopulationCache(k, DEV)
    pop.add_many(range(G), [(t(e), nn) for nn, e in graphs])
    for got in (us().sample_distinct(t(ei), t(ptr), n, k, 99), pop.sample_distinct(range(G), t(ptr), t(ei), n, [5, 4, 3, 2, 1])):
        assert all(torch.equal(a, b) for a, b in zip(got[:5], en[:5]))
        assert got[6].tolist() == [n] * G and not got[5].any()
    pop.close()


# ---- 3. one integer for all seeds ----
def test_the_integer_seed_conventions():
    c = case("small_mix")
    G, s = len(c["sizes"]), (1 << 64) - 3                           # the sums wrap mod 2^64
    ei, ptr = t(c["ei"]), t(c["ptr"])
    by_place = us().sample_distinct(ei, ptr, c["m"], c["k"], s)
    assert all(torch.equal(a, b) for a, b in zip(by_place, us().sample_distinct(ei, ptr, c["m"], c["k"], [s + g for g in range(G)])))
    by_index = c["pop"].sample_distinct(c["idx"], ptr, ei, c["m"], s)
    assert all(torch.equal(a, b) for a, b in zip(by_index, us().sample_distinct(ei, ptr, c["m"], c["k"], [s + i for i in c["idx"]])))
    assert_same(by_index, rebuild(c["en"]["sample"], c["sizes"], [(s + i) & D.M64 for i in c["idx"]], c["m"], c["k"]), "s + graph_idx")
    assert not torch.equal(by_place[0], by_index[0])
    # a graph's bag follows its index, not its place in the batch: graph 104 alone
    g = 4
    lo, hi = int(c["ptr"][g]), int(c["ptr"][g + 1])
    inside = (c["ei"][0] >= lo) & (c["ei"][0] < hi)
    alone = c["pop"].sample_distinct([104], t(np.array([lo, hi])), t(c["ei"][:, inside]), c["m"], s)
    assert torch.equal(alone[0], by_index[0][g * c["m"]:(g + 1) * c["m"]])
    wrapped = [(s + i) & D.M64 for i in c["idx"]]                   # as an int64 tensor: two's complement
    seeds_t = torch.tensor([x - (1 << 64) if x >> 63 else x for x in wrapped], dtype=torch.int64)
    assert all(torch.equal(a, b) for a, b in zip(by_index, c["pop"].sample_distinct(torch.tensor(c["idx"]), ptr, ei, c["m"], seeds_t)))


# ---- 4. where the outputs live ----
def test_host_input_gives_pinned_host_tensors_and_device_input_device_tensors():
    c = case("k13_m100")
    want = rebuild(c["en"]["sample"], c["sizes"], c["seeds"], c["m"], c["k"])
    ei, ptr = t(c["ei"]), t(c["ptr"])
    for host, dev in ((us().sample_distinct(ei, ptr, c["m"], c["k"], c["seeds"]), us().sample_distinct(ei.to(DEV), ptr.to(DEV), c["m"], c["k"], c["seeds"])),
                      (c["pop"].sample_distinct(c["idx"], ptr, ei, c["m"], c["seeds"]),
                       c["pop"].sample_distinct(c["idx"], ptr.to(DEV), ei.to(DEV), c["m"], c["seeds"]))):
        assert all(x.device.type == "cpu" for x in host) and all(x.is_pinned() for x in host[:5] if x.numel() > 0)
        assert all(x.is_cuda and x.device.index == 0 for x in dev)
        assert host[6].dtype == torch.int64 and host[5].dtype == torch.bool
        assert_same(host, want, "host in")
        assert_same(dev, want, "device in")
    asked = c["pop"].sample_distinct(c["idx"], ptr, ei, c["m"], c["seeds"], device=DEV)
    assert all(x.is_cuda for x in asked)
    assert_same(asked, want, "device=")


# ---- 5. m = 0, no graphs, a graph that fails alone ----
def test_no_rows_no_graphs_and_a_failed_graph():
    c = case("small_mix")
    G, k = len(c["sizes"]), c["k"]
    ei, ptr = t(c["ei"]), t(c["ptr"])
    for zero in (us().sample_distinct(ei, ptr, 0, k, c["seeds"]), c["pop"].sample_distinct(c["idx"], ptr, ei, 0, 7)):
        assert [tuple(x.shape) for x in zero] == [(0, k), (2, 0), (1,), (G + 1,), (0,), (G,), (G,)]
        assert zero[2].tolist() == [0] and zero[3].tolist() == [0] * (G + 1) and zero[6].tolist() == [0] * G and not zero[5].any()
    none = (torch.zeros((2, 0), dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    for empty in (us().sample_distinct(*none, 5, k, []), c["pop"].sample_distinct([], none[1], none[0], 5, 3)):
        assert [tuple(x.shape) for x in empty] == [(0, k), (2, 0), (1,), (1,), (0,), (0,), (0,)]
    # 70 vertices under the limit of 64: the graph fails alone, in both calls
    assert us().max_vertices() == 64
    graphs = [D.cycle(6), D.path(70), D.cycle(5)]
    ptr3 = np.array([0, 6, 76, 81], np.int64)
    ei3 = np.concatenate([e + ptr3[g] for g, (_, e) in enumerate(graphs)], axis=1)
    pop = us().PopulationCache(3, DEV)
    pop.add_many([0, 1, 2], [(t(e), n) for n, e in graphs])
    assert pop.failed == {1}
    unc = us().sample_distinct(t(ei3), t(ptr3), 6, 3, [1, 2, 3])
    got = pop.sample_distinct([0, 1, 2], t(ptr3), t(ei3), 6, [1, 2, 3])
    assert all(torch.equal(a, b) for a, b in zip(unc, got))
    assert got[5].tolist() == [False, True, False] and got[6].tolist() == [6, 0, 5] and (got[0][6:12] == -1).all() and (got[0][17] == -1).all()
    keep = np.concatenate([ei3[:, ei3[0] < 6], ei3[:, ei3[0] >= 76]], axis=1)
    en = [x.numpy() for x in us().enumerate_graphs(t(keep), t(ptr3), 3)]     # the failed graph as one without columns: n >= k, but no sets
    want = rebuild(en, [6, 0, 5], [1, 2, 3], 6, 3)
    src = np.where(want[4] >= 12, want[4] + graphs[1][1].shape[1], want[4])   # edge_src: positions in the batch that holds the path's columns
    assert_same(got, want[:4] + (src, np.array([False, True, False]), want[6]), "around the failed graph")
    pop.close()


# ---- 6. threads ----
def test_two_threads_draw_distinct_rows_beside_one_with_replacement():
    c = case("k13_m100")
    ei, ptr, pop = t(c["ei"]), t(c["ptr"]), c["pop"]
    jobs = [lambda: pop.sample_distinct(c["idx"], ptr, ei, c["m"], [1, 2, 3]), lambda: pop.sample_distinct(c["idx"], ptr, ei, c["m"], 1 << 40),
            lambda: pop.sample_graphs(c["idx"], ptr, ei, c["m"], [1, 2, 3])]
    alone = [job() for job in jobs]
    assert not torch.equal(alone[0][0], alone[1][0]) and not torch.equal(alone[0][0], alone[2][0])
    errors = []

    def work(i):
        try:
            for _ in range(4):
                assert all(torch.equal(a, b) for a, b in zip(jobs[i](), alone[i])), f"thread {i}"
        except BaseException as e:                                  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
