"""graphlets.census on the GPU (uni_census_esu / uni_census_wesu in ugs_uniform.hip) against the numpy law of
tests/graphlet_census_law.py where the law is feasible, against closed forms, and always against the recipe the law's item 4 names --
histogram(class_ids(enumerate_graphs rows))[:, connected_classes(k)], code from before the census existed -- wherever the recipe can
run.  Columns for k = 7 and 8 come from graphlets.table, whose content tests/test_graphlet_law.py pins.

One case count_graphs has cannot exist here: a graph of more than 64 vertices with n < k needs k > 65, and the census takes k <= 8."""
import contextlib
import functools
import random
from math import comb

import numpy as np
import pytest
import torch

import graphlet_census_law as law
import graphlet_law

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def columns(k):
    from ugs_sampler import graphlets
    return graphlets.table(k)[graphlets.connected_classes(k)].tolist()


def column_of(k, graph):
    return columns(k).index(law.key_of_graph(*graph))


def census(ei, ptr, k, **kw):
    from ugs_sampler import graphlets
    kw.setdefault("device", DEV)
    counts, failed = graphlets.census(ei if torch.is_tensor(ei) else torch.from_numpy(ei), ptr if torch.is_tensor(ptr) else torch.from_numpy(ptr),
                                      k, **kw)
    assert counts.dtype == torch.int64 and counts.shape == (ptr.shape[0] - 1, len(columns(k)))
    assert failed.dtype == torch.bool and failed.device.type == "cpu" and failed.shape == (ptr.shape[0] - 1,)
    return counts, failed


def recipe(ei, ptr, k, max_rows=1 << 22):
    """Item 4 of the law: the histogram over the enumerated rows, its connected columns, and every other column zero."""
    import uniform_sampler as us
    from ugs_sampler import graphlets
    nodes, e2, eptr, sptr, _, failed = us.enumerate_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), k, max_rows=max_rows, device=DEV)
    hist = graphlets.histogram(graphlets.class_ids(nodes, e2, eptr), sptr, k)
    sub = hist[:, graphlets.connected_classes(k).to(DEV)]
    assert int(hist.sum()) == int(sub.sum()) == nodes.shape[0]
    return sub, failed


def set_counts(ei, ptr, k, limit=1 << 25):
    import uniform_sampler as us
    return us.count_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), k, limit=limit)


@contextlib.contextmanager
def limits(max_vertices=None, mask_vertices=None):
    import uniform_sampler as us
    prev_max = us.set_max_vertices(max_vertices) if max_vertices is not None else None
    try:
        prev_mask = us._set_mask_vertices(mask_vertices) if mask_vertices is not None else None
        try:
            yield
        finally:
            if prev_mask is not None:
                us._set_mask_vertices(prev_mask)
    finally:
        if prev_max is not None:
            us.set_max_vertices(prev_max)


def one_hot_check(counts, want_cols):
    """counts [G, W] on the device has a one at want_cols[g] (a list of columns per graph) and zeros elsewhere."""
    G = counts.shape[0]
    assert counts.sum(dim=1).tolist() == [len(c) for c in want_cols]
    rows = torch.tensor([g for g, c in enumerate(want_cols) for _ in c], dtype=torch.int64, device=counts.device)
    cols = torch.tensor([x for c in want_cols for x in c], dtype=torch.int64, device=counts.device)
    assert rows.numel() == 0 or bool((counts[rows, cols] == 1).all())
    assert G == len(want_cols)


# ---- 1. the mixed batch -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_batch(k):
    rng = random.Random(100 + k)
    messy = [(u, v) for u in range(10) for v in range(u + 1, 10) if rng.random() < 0.3]
    messy += [(v, u) for u, v in messy if rng.random() < 0.6] + [rng.choice(messy) for _ in range(4)] + [(3, 3), (7, 7), (3, 3)]
    rng.shuffle(messy)
    lonely = [(u, v) for u in range(8) for v in range(u + 1, 8) if rng.random() < 0.4]
    graphs = [(0, []), law.path(max(k - 1, 0)), law.path(k), (k, law.path(k - 1)[1] if k > 1 else []),
              law.path(10), law.star(9, centre=4), law.cycle(10), law.clique(9), (12, lonely), (10, messy),
              (k, law.clique(k)[1]), (11, [(u, v) for u in range(11) for v in range(u + 1, 11) if rng.random() < 0.25])]
    if k == 1:
        graphs[3] = (0, [])                                                     # one vertex is always connected
    ei, ptr = law.batch(graphs)
    n0 = int(ptr[5])                                                            # the last vertex of the path of ten
    extra = np.array([[n0 - 1, int(ptr[-1]) + 3, int(ptr[-1])], [n0, int(ptr[-1]) + 4, 2]], np.int64)    # crossing, outside, half outside
    ei = np.concatenate([ei[:, :7], extra, ei[:, 7:]], axis=1)
    return np.ascontiguousarray(ei), ptr


@functools.lru_cache(maxsize=None)
def mixed_want(k):
    ei, ptr = mixed_batch(k)
    return law.census(ei, ptr, k, columns(k))


def run_mixed(k):
    ei, ptr = mixed_batch(k)
    counts, failed = census(dev(ei), dev(ptr), k)
    assert not failed.any() and counts.device.type == "cuda"
    return counts.cpu()


@pytest.mark.parametrize("k", range(1, 9))
def test_mixed_batch(k):
    ei, ptr = mixed_batch(k)
    want = mixed_want(k)
    got = run_mixed(k)
    assert np.array_equal(got.numpy(), want)
    assert want[0].sum() == 0 and want[1].sum() == 0 and want[2].sum() == 1 and want[3].sum() == 0      # n = 0, n < k, n = k, disconnected
    sub, _ = recipe(ei, ptr, k)
    assert torch.equal(got, sub.cpu())
    sizes, bad = set_counts(ei, ptr, k)
    assert not bad.any() and torch.equal(got.sum(dim=1), sizes)
    E = ei.shape[1]
    wide = torch.zeros((2, E + 5), dtype=torch.int64, device=DEV)
    wide[:, :E] = dev(ei)
    spread = torch.zeros((2, 2 * E), dtype=torch.int64, device=DEV)
    spread[:, ::2] = dev(ei)
    for view in (wide[:, :E], spread[:, ::2]):
        assert not view.is_contiguous() or E == 0
        assert torch.equal(census(view, dev(ptr), k)[0].cpu(), got)
    host, failed = census(torch.from_numpy(ei), torch.from_numpy(ptr), k, device=None)
    assert host.device.type == "cpu" and torch.equal(host, got) and not failed.any()


# ---- 2. bit 63 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", [63, 0])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_star_of_64_vertices(k, centre):
    ei, ptr = law.batch([law.star(63, centre)])
    counts, failed = census(ei, ptr, k)
    want = torch.zeros_like(counts)
    want[0, column_of(k, law.star(k - 1))] = comb(63, k - 1)
    assert not failed.any() and torch.equal(counts, want)
    if k == 5:
        assert int(counts.sum()) == 595665


@pytest.mark.parametrize("k", range(1, 9))
def test_cycle_of_64_vertices(k):
    ei, ptr = law.batch([law.cycle(64)])
    counts, failed = census(ei, ptr, k)
    want = torch.zeros_like(counts)
    want[0, column_of(k, law.path(k))] = 64
    assert not failed.any() and torch.equal(counts, want)


def test_sparse_64_vertex_graph_against_the_recipe():
    import ugs_workloads as wl
    ei, ptr = wl.tu_graph(64, 80, 5), np.array([0, 64], np.int64)
    counts, failed = census(ei, ptr, 5)
    sub, _ = recipe(ei, ptr, 5)
    assert not failed.any() and torch.equal(counts, sub) and int(counts.sum()) > 1000 and int((counts > 0).sum()) >= 5


# ---- 3. every class -------------------------------------------------------------------------------------------------------------------
def relabelled(codes, n, rng, offset_step=None):
    """A batch with one graph of n vertices per code, every graph under its own random relabelling."""
    graphs = []
    for c in codes:
        perm = list(range(n))
        rng.shuffle(perm)
        graphs.append((n, [(perm[i], perm[j]) if rng.random() < 0.5 else (perm[j], perm[i]) for i, j in graphlet_law.edges_of_code(int(c), n)]))
    return law.batch(graphs)


@functools.lru_cache(maxsize=None)
def class_batches(n):
    cols = columns(n)
    codes = [key & ((1 << 28) - 1) for key in cols]
    return [relabelled(codes, n, random.Random(7 * n + r)) for r in range(2)]


def run_classes(n):
    return [census(ei, ptr, n)[0] for ei, ptr in class_batches(n)]


@pytest.mark.parametrize("n", [5, 6, 7])
def test_every_connected_class_is_its_own_column(n):
    W = len(columns(n))
    for counts in run_classes(n):
        assert torch.equal(counts, torch.eye(W, dtype=torch.int64, device=DEV))


@functools.lru_cache(maxsize=None)
def all_codes_six():
    n, R = 6, 1 << 15
    codes = np.arange(R, dtype=np.int64)
    pr = np.array(graphlet_law.pairs(n), np.int64)
    bits = (codes[:, None] >> (pr[:, 1] * (pr[:, 1] - 1) // 2 + pr[:, 0])[None, :]) & 1
    r, p = np.nonzero(bits)
    ei = np.stack([pr[p, 0] + n * r, pr[p, 1] + n * r])
    canon = graphlet_law.canonical_codes(codes, n)
    at = {key & ((1 << 28) - 1): c for c, key in enumerate(columns(n))}
    col = np.array([at.get(int(c), -1) for c in canon], np.int64)               # -1: not connected
    return np.ascontiguousarray(ei), np.arange(R + 1, dtype=np.int64) * n, col


def run_all_codes_six():
    ei, ptr, _ = all_codes_six()
    return census(ei, ptr, 6)[0]


def test_all_codes_of_six_vertices():
    _, _, col = all_codes_six()
    counts = run_all_codes_six()
    want = torch.zeros_like(counts)
    hit = np.nonzero(col >= 0)[0]
    assert len(hit) == 26704                                                    # labelled connected graphs on 6 vertices (OEIS A001187)
    want[dev(hit), dev(col[hit])] = 1
    assert torch.equal(counts, want)


@functools.lru_cache(maxsize=None)
def packed_eight(seed):
    """All 11 117 connected classes of n = 8, eight to a 64-vertex graph as components, the 64 vertices shuffled: 1390 graphs."""
    rng = random.Random(seed)
    cols = columns(8)
    order = list(range(len(cols)))
    rng.shuffle(order)
    graphs, want = [], []
    for lo in range(0, len(order), 8):
        part = order[lo:lo + 8]
        perm = list(range(64))
        rng.shuffle(perm)
        es = []
        for slot, c in enumerate(part):
            es += [(perm[8 * slot + i], perm[8 * slot + j]) for i, j in graphlet_law.edges_of_code(cols[c] & ((1 << 28) - 1), 8)]
        rng.shuffle(es)
        graphs.append((64, es))
        want.append(part)
    return graphs, want


def run_packed_eight(seed, check):
    graphs, want = packed_eight(seed)
    for lo in range(0, len(graphs), 700):                                       # [700, 11117] int64 is 62 MB
        ei, ptr = law.batch(graphs[lo:lo + 700])
        counts, failed = census(ei, ptr, 8)
        assert not failed.any()
        check(counts, want[lo:lo + 700])


@pytest.mark.parametrize("seed", [1, 2])
def test_every_connected_class_of_eight_vertices(seed):
    graphs, _ = packed_eight(seed)
    assert len(graphs) == 1390
    run_packed_eight(seed, one_hot_check)


# ---- 4. flush boundaries and contention -----------------------------------------------------------------------------------------------
def test_clique_of_24_at_six():
    ei, ptr = law.batch([law.clique(24)])
    counts, failed = census(ei, ptr, 6)
    want = torch.zeros_like(counts)
    want[0, column_of(6, law.clique(6))] = 134596
    assert not failed.any() and torch.equal(counts, want)
    assert torch.equal(counts, recipe(ei, ptr, 6)[0])


def test_complete_bipartite_12_12_at_six():
    ei, ptr = law.batch([law.bipartite(12, 12)])
    counts, failed = census(ei, ptr, 6)
    want = torch.zeros_like(counts)
    for a, b in ((1, 5), (2, 4), (3, 3)):
        want[0, column_of(6, law.bipartite(a, b))] = comb(12, a) * comb(12, b) * (1 if a == b else 2)
    assert int(want.sum()) == 132748
    assert not failed.any() and torch.equal(counts, want)
    assert torch.equal(counts, recipe(ei, ptr, 6)[0])


# ---- 5. past the old cap ----------------------------------------------------------------------------------------------------------------
def test_clique_of_44_at_seven():
    ei, ptr = law.batch([law.clique(44)])
    counts, failed = census(ei, ptr, 7, limit=1 << 27)
    want = torch.zeros_like(counts)
    want[0, column_of(7, law.clique(7))] = 38320568
    assert not failed.any() and torch.equal(counts, want)
    sizes, bad = set_counts(ei, ptr, 7, limit=1 << 27)
    assert not bad.any() and sizes.tolist() == [38320568]
    assert census(ei, ptr, 7)[1].tolist() == [True]                             # past the default limit of 2^25


def test_complete_bipartite_19_19_at_eight():
    ei, ptr = law.batch([law.bipartite(19, 19)])
    counts, failed = census(ei, ptr, 8, limit=1 << 27)
    want = torch.zeros_like(counts)
    for (a, b), sets in (((1, 7), 1914744), ((2, 6), 9279144), ((3, 5), 22535064), ((4, 4), 15023376)):
        assert sets == comb(19, a) * comb(19, b) * (1 if a == b else 2)
        want[0, column_of(8, law.bipartite(a, b))] = sets
    assert int(want.sum()) == 48752328
    assert not failed.any() and torch.equal(counts, want)
    sizes, bad = set_counts(ei, ptr, 8, limit=1 << 27)
    assert not bad.any() and sizes.tolist() == [48752328]


# ---- 6. limit ---------------------------------------------------------------------------------------------------------------------------
def test_limit_is_per_graph():
    ei, ptr = law.batch([law.cycle(9), law.clique(10), law.path(7), law.clique(10)])
    k, sets = 4, comb(10, 4)
    want = law.census(ei, ptr, k, columns(k))
    counts, failed = census(ei, ptr, k, limit=sets)                             # two graphs at the limit, together past it
    assert failed.tolist() == [False] * 4 and np.array_equal(counts.cpu().numpy(), want)
    counts, failed = census(ei, ptr, k, limit=sets - 1)
    assert failed.tolist() == [False, True, False, True]
    want[1] = want[3] = 0
    assert np.array_equal(counts.cpu().numpy(), want) and want[0].sum() == 9 and want[2].sum() == 4


def test_a_graph_far_past_the_limit_fails_alone():
    ei, ptr = law.batch([law.cycle(9), law.clique(30), law.path(7)])            # 593 775 sets at k = 6: the flushes stop it early
    counts, failed = census(ei, ptr, 6, limit=1000)
    assert failed.tolist() == [False, True, False]
    assert np.array_equal(counts.cpu().numpy(), law.census(*law.batch([law.cycle(9), (30, []), law.path(7)]), 6, columns(6)))


# ---- 7. size ----------------------------------------------------------------------------------------------------------------------------
def test_a_graph_of_65_vertices_fails_alone_by_default():
    import uniform_sampler as us
    assert us.max_vertices() == 64
    ei, ptr = law.batch([law.cycle(9), law.path(65), law.clique(6)])
    counts, failed = census(ei, ptr, 4)
    assert failed.tolist() == [False, True, False]
    assert np.array_equal(counts.cpu().numpy(), law.census(ei, ptr, 4, columns(4), failed={1}))
    sizes, bad = set_counts(ei, ptr, 4)
    assert bad.tolist() == failed.tolist() and sizes.tolist() == [9, -1, 15]


# ---- 8. the wide form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_wide_path_ring_and_star(k):
    graphs = [law.path(65), law.cycle(65), law.star(64, centre=64), law.clique(5)]
    if k == 8:
        graphs[2] = law.star(20, centre=20)                                     # C(64, 7) stars would take the test past a second
    ei, ptr = law.batch(graphs)
    with limits(max_vertices=1024):
        counts, failed = census(ei, ptr, k)
    want = torch.zeros_like(counts)
    want[0, column_of(k, law.path(k))] = 65 - k + 1
    want[1, column_of(k, law.path(k))] = 65
    want[2, column_of(k, law.star(k - 1))] = comb(graphs[2][0] - 1, k - 1)
    want[3, column_of(k, law.clique(k))] = comb(5, k)
    assert not failed.any() and torch.equal(counts, want)


def test_wide_three_words():
    n, es = law.cycle(130)
    es = es + [(0, 64), (10, 70), (63, 65), (64, 128), (1, 129), (127, 3), (66, 66), (10, 70)]
    ei, ptr = law.batch([law.clique(6), (n, es)])
    for k in (3, 4, 5):
        with limits(max_vertices=1024):
            counts, failed = census(ei, ptr, k)
            sub, _ = recipe(ei, ptr, k)
        assert not failed.any() and torch.equal(counts, sub)
        assert np.array_equal(counts.cpu().numpy(), law.census(ei, ptr, k, columns(k)))


def test_wide_sparse_200_vertex_graph_against_the_recipe():
    import ugs_workloads as wl
    ei, ptr = wl.tu_graph(200, 260, 11), np.array([0, 200], np.int64)
    with limits(max_vertices=1024):
        counts, failed = census(ei, ptr, 4)
        sub, _ = recipe(ei, ptr, 4)
        sizes, _ = set_counts(ei, ptr, 4)
    assert not failed.any() and torch.equal(counts, sub) and torch.equal(counts.sum(dim=1).cpu(), sizes) and int(counts.sum()) > 1000


@pytest.mark.parametrize("k", range(1, 9))
def test_wide_kernels_on_the_mixed_batch(k):
    with limits(mask_vertices=0):
        got = run_mixed(k)
    assert np.array_equal(got.numpy(), mixed_want(k))


def test_wide_kernels_on_every_class():
    with limits(mask_vertices=0):
        for n in (5, 6, 7):
            for counts in run_classes(n):
                assert torch.equal(counts, torch.eye(len(columns(n)), dtype=torch.int64, device=DEV))
        wide_six = run_all_codes_six()
    assert torch.equal(wide_six, run_all_codes_six())


def test_wide_kernels_on_every_class_of_eight_vertices():
    with limits(mask_vertices=0):
        run_packed_eight(1, one_hot_check)


# ---- 9. degenerate and bad arguments ------------------------------------------------------------------------------------------------------
def test_degenerate_and_bad_arguments():
    from ugs_sampler import graphlets
    none = torch.zeros((2, 0), dtype=torch.int64)
    counts, failed = census(none, torch.zeros((1,), dtype=torch.int64), 5)      # G = 0
    assert counts.shape == (0, 21) and failed.shape == (0,)
    counts, failed = census(none, torch.tensor([0, 3, 3, 9]), 1)                # E = 0: every vertex is a set at k = 1
    assert counts.tolist() == [[3], [0], [6]] and not failed.any()
    counts, failed = census(none, torch.tensor([0, 3, 3, 9]), 2)
    assert counts.tolist() == [[0], [0], [0]] and not failed.any()
    ei, ptr = law.batch([law.clique(5)])
    with pytest.raises(RuntimeError):
        census(ei, np.array([0, 5, 3], np.int64), 3)                            # a decreasing ptr
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="1 <= k <= 8"):
            graphlets.census(torch.from_numpy(ei), torch.from_numpy(ptr), k, device=DEV)
    for limit in (0, (1 << 32) + 1):
        with pytest.raises(ValueError, match="limit"):
            graphlets.census(torch.from_numpy(ei), torch.from_numpy(ptr), 3, limit=limit, device=DEV)
    assert census(ei, ptr, 3, limit=1 << 32)[0].tolist() == [[0, 10]]


# ---- 10. nothing else changed -------------------------------------------------------------------------------------------------------------
def test_the_other_entry_points_are_undisturbed():
    import uniform_sampler as us
    from ugs_sampler import graphlets
    ei, ptr = mixed_batch(5)
    e_t, p_t = torch.from_numpy(ei), torch.from_numpy(ptr)

    def others():
        rows = us.enumerate_graphs(e_t, p_t, 5, device=DEV)
        return (us.count_graphs(e_t, p_t, 5) + rows + (graphlets.class_ids(*rows[:3]),) + graphlets.orbit_ids(*rows[:3], return_class=True))

    before = others()
    counts, _ = census(ei, ptr, 5)
    after = others()
    assert len(before) == len(after) == 11
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert np.array_equal(counts.cpu().numpy(), mixed_want(5))
