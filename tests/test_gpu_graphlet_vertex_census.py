"""graphlets.vertex_census on the GPU (uni_vcensus_esu / uni_vcensus_wesu in ugs_uniform.hip, the table kernel in ugs_graphlet.hip)
against the numpy law of tests/graphlet_vertex_census_law.py where the law is feasible, against closed forms, against the recipe the
law's item 4 names -- vertex_orbit_counts(orbit_ids(enumerate_graphs rows)), code from before the call existed -- wherever the recipe
can run, and against graphlets.census through item 5.  The class keys and orbit counts of k = 7 are handed to the law from
graphlets.table and graphlets.orbit_base, whose content tests/test_graphlet_law.py and tests/test_graphlet_orbit_law.py pin; for
k <= 6 the law finds its own by brute force."""
import contextlib
import functools
import random
from math import comb

import numpy as np
import pytest
import torch

import graphlet_census_law as census_law
import graphlet_law
import graphlet_vertex_census_law as law

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTH = law.CONNECTED_ORBITS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def layout(k):
    """(class keys, orbits per class) from the library: what the law is handed for k = 7 and what the closed forms look columns up in."""
    from ugs_sampler import graphlets
    classes = graphlets.connected_classes(k)
    base = graphlets.orbit_base(k)
    return graphlets.table(k)[classes].tolist(), (base[classes + 1] - base[classes]).tolist()


def handed(k):
    return dict(zip(("columns", "widths"), layout(k))) if k == 7 else {}


@functools.lru_cache(maxsize=None)
def column_of(k, graph_fn, size, vertex):
    return law.column_of(k, graph_fn(size), vertex, *layout(k))


@functools.lru_cache(maxsize=None)
def orbit_sizes(k):
    """(size [O], class column [O]) of item 5 from the library's rooted codes; the law's own for k <= 5 must agree."""
    from ugs_sampler import graphlets
    keys, widths = layout(k)
    size, cls = [], []
    for c, key in enumerate(keys):
        rooted = graphlets._rooted_codes(key & ((1 << 28) - 1), k)
        size += [rooted.count(code) for code in sorted(set(rooted))]
        cls += [c] * widths[c]
    if k <= 5:
        mine = law.orbit_sizes(k)
        assert mine[0].tolist() == size and mine[1].tolist() == cls
    return torch.tensor(size, dtype=torch.int64), torch.tensor(cls, dtype=torch.int64)


def vertex_census(ei, ptr, k, **kw):
    from ugs_sampler import graphlets
    kw.setdefault("device", DEV)
    ei = ei if torch.is_tensor(ei) else torch.from_numpy(ei)
    ptr = ptr if torch.is_tensor(ptr) else torch.from_numpy(ptr)
    gdv, failed = graphlets.vertex_census(ei, ptr, k, **kw)
    assert gdv.dtype == torch.int64 and gdv.shape == (int(ptr[-1]), WIDTH[k - 1])
    assert failed.dtype == torch.bool and failed.device.type == "cpu" and failed.shape == (ptr.shape[0] - 1,)
    return gdv, failed


def recipe(ei, ptr, k, max_rows=1 << 22):
    """Item 4 of the law: the orbit ids of the enumerated rows, counted per vertex."""
    import uniform_sampler as us
    from ugs_sampler import graphlets
    nodes, e2, eptr, _, _, failed = us.enumerate_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), k, max_rows=max_rows, device=DEV)
    orbit = graphlets.orbit_ids(nodes, e2, eptr)
    gdv = graphlets.vertex_orbit_counts(nodes, orbit, int(ptr[-1]), graphlets.connected_orbits(k))
    assert int(gdv.sum()) == nodes.numel()
    return gdv, failed


def census(ei, ptr, k, **kw):
    from ugs_sampler import graphlets
    return graphlets.census(torch.from_numpy(ei), torch.from_numpy(ptr), k, device=DEV, **kw)


def check_identity_five(gdv, ei, ptr, k, **kw):
    """Per graph and column the sum over the vertices is the orbit's size times the census' count of its class; a row sums to the
    sets that hold the vertex, so all of it sums to k times the sets."""
    counts, failed = census(ei, ptr, k, **kw)
    size, cls = orbit_sizes(k)
    g_of_v = torch.repeat_interleave(torch.arange(len(ptr) - 1), torch.from_numpy(np.diff(ptr))).to(DEV)
    sums = torch.zeros((len(ptr) - 1, gdv.shape[1]), dtype=torch.int64, device=DEV).index_add_(0, g_of_v, gdv[int(ptr[0]):])
    assert torch.equal(sums, size.to(DEV)[None, :] * counts[:, cls.to(DEV)])
    return counts, failed


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


# ---- 1. the mixed batch -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_batch(k):
    """n = 0, n < k, n = k, disconnected; a path, a star with its centre in the middle, a cycle, K9; two random graphs, one with loops,
    duplicates and reversed columns; columns that cross graphs, lie outside them, or half outside."""
    rng = random.Random(200 + k)
    messy = [(u, v) for u in range(10) for v in range(u + 1, 10) if rng.random() < 0.3]
    messy += [(v, u) for u, v in messy if rng.random() < 0.6] + [rng.choice(messy) for _ in range(4)] + [(3, 3), (7, 7), (3, 3)]
    rng.shuffle(messy)
    lonely = [(u, v) for u in range(8) for v in range(u + 1, 8) if rng.random() < 0.4]
    graphs = [(0, []), census_law.path(max(k - 1, 0)), census_law.path(k), (k, census_law.path(k - 1)[1] if k > 1 else []),
              census_law.path(10), census_law.star(9, centre=4), census_law.cycle(10), census_law.clique(9), (12, lonely), (10, messy),
              (k, census_law.clique(k)[1]), (11, [(u, v) for u in range(11) for v in range(u + 1, 11) if rng.random() < 0.25])]
    if k == 1:
        graphs[3] = (0, [])                                                     # one vertex is always connected
    ei, ptr = census_law.batch(graphs)
    n0 = int(ptr[5])                                                            # the last vertex of the path of ten
    extra = np.array([[n0 - 1, int(ptr[-1]) + 3, int(ptr[-1])], [n0, int(ptr[-1]) + 4, 2]], np.int64)    # crossing, outside, half outside
    ei = np.concatenate([ei[:, :7], extra, ei[:, 7:]], axis=1)
    return np.ascontiguousarray(ei), ptr


@functools.lru_cache(maxsize=None)
def mixed_want(k):
    ei, ptr = mixed_batch(k)
    return law.vertex_census(ei, ptr, k, **handed(k))


def run_mixed(k):
    ei, ptr = mixed_batch(k)
    gdv, failed = vertex_census(dev(ei), dev(ptr), k)
    assert not failed.any() and gdv.device.type == "cuda"
    return gdv


@pytest.mark.parametrize("k", range(1, 8))
def test_mixed_batch(k):
    ei, ptr = mixed_batch(k)
    want = mixed_want(k)
    got = run_mixed(k)
    assert np.array_equal(got.cpu().numpy(), want)
    per_graph = [want[int(ptr[g]):int(ptr[g + 1])].sum() for g in range(4)]
    assert per_graph == [0, 0, k, 0]                                            # n = 0, n < k, n = k, disconnected
    assert torch.equal(got, recipe(ei, ptr, k)[0])
    check_identity_five(got, ei, ptr, k)
    E = ei.shape[1]
    wide = torch.zeros((2, E + 5), dtype=torch.int64, device=DEV)
    wide[:, :E] = dev(ei)
    spread = torch.zeros((2, 2 * E), dtype=torch.int64, device=DEV)
    spread[:, ::2] = dev(ei)
    for view in (wide[:, :E], spread[:, ::2]):
        assert not view.is_contiguous() or E == 0
        assert torch.equal(vertex_census(view, dev(ptr), k)[0], got)
    host, failed = vertex_census(torch.from_numpy(ei), torch.from_numpy(ptr), k, device=None)
    assert host.device.type == "cpu" and torch.equal(host, got.cpu()) and not failed.any()


# ---- 2. every class, every position ---------------------------------------------------------------------------------------------------
def relabelled(codes, n, rng):
    """A batch with one graph of n vertices per code, every graph under its own random relabelling."""
    graphs = []
    for c in codes:
        perm = list(range(n))
        rng.shuffle(perm)
        graphs.append((n, [(perm[i], perm[j]) if rng.random() < 0.5 else (perm[j], perm[i]) for i, j in graphlet_law.edges_of_code(int(c), n)]))
    return census_law.batch(graphs)


def one_hot_by_orbit_ids(ei, ptr, n):
    """int64 [N, O] on the device: graph g (n vertices, its columns in order) read as row g of a sampler's output, every vertex's
    orbit id from graphlets.orbit_ids, a one at its column; a row of zeros where the id is no connected orbit of n vertices."""
    from ugs_sampler import graphlets
    G = len(ptr) - 1
    assert np.array_equal(ptr, np.arange(G + 1) * n)
    eptr = np.searchsorted(ei[0] // n, np.arange(G + 1)).astype(np.int64)       # the columns come graph by graph
    nodes = torch.arange(G * n, dtype=torch.int64, device=DEV).view(G, n)
    orbit = graphlets.orbit_ids(nodes, dev(ei % n), dev(eptr)).view(-1)
    cols = graphlets.connected_orbits(n).to(DEV)
    at = torch.searchsorted(cols, orbit).clamp_(max=cols.numel() - 1)
    want = torch.zeros((G * n, cols.numel()), dtype=torch.int64, device=DEV)
    want[torch.arange(G * n, device=DEV), at] = (cols[at] == orbit).to(torch.int64)
    return want


@functools.lru_cache(maxsize=None)
def class_batch(n):
    return relabelled([key & ((1 << 28) - 1) for key in layout(n)[0]], n, random.Random(11 * n))


def check_classes(n):
    ei, ptr = class_batch(n)
    assert len(ptr) - 1 == census_law.CONNECTED_ON[n - 1]
    gdv, failed = vertex_census(ei, ptr, n)
    assert not failed.any() and int(gdv.sum()) == n * (len(ptr) - 1) and torch.equal(gdv, one_hot_by_orbit_ids(ei, ptr, n))
    assert int((gdv.sum(dim=0) > 0).sum()) == WIDTH[n - 1]                     # every column is some vertex's


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_every_connected_class_as_its_own_graph(n):
    check_classes(n)


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_wide_kernel_on_every_connected_class(n):
    with limits(mask_vertices=0):
        check_classes(n)


@functools.lru_cache(maxsize=None)
def all_codes_six():
    n, R = 6, 1 << 15
    codes = np.arange(R, dtype=np.int64)
    pr = np.array(graphlet_law.pairs(n), np.int64)
    bits = (codes[:, None] >> (pr[:, 1] * (pr[:, 1] - 1) // 2 + pr[:, 0])[None, :]) & 1
    r, p = np.nonzero(bits)
    ei = np.stack([pr[p, 0] + n * r, pr[p, 1] + n * r])
    connected = np.array([graphlet_law.connected(int(c), n) for c in codes])
    return np.ascontiguousarray(ei), np.arange(R + 1, dtype=np.int64) * n, connected


@pytest.mark.parametrize("mask_vertices", [64, 0])
def test_all_codes_of_six_vertices(mask_vertices):
    ei, ptr, connected = all_codes_six()
    assert int(connected.sum()) == 26704                                        # labelled connected graphs on 6 vertices (OEIS A001187)
    with limits(mask_vertices=mask_vertices):
        gdv, failed = vertex_census(ei, ptr, 6)
    assert not failed.any()
    assert torch.equal(gdv.sum(dim=1).view(-1, 6), dev(connected.astype(np.int64))[:, None].expand(-1, 6))
    assert int(gdv.max()) == 1
    assert torch.equal(gdv, one_hot_by_orbit_ids(ei, ptr, 6) * dev(np.repeat(connected, 6).astype(np.int64))[:, None])


# ---- 3. flushes and merged runs ---------------------------------------------------------------------------------------------------------
def test_clique_of_24_at_six():
    ei, ptr = census_law.batch([census_law.clique(24)])
    gdv, failed = vertex_census(ei, ptr, 6)
    want = torch.zeros_like(gdv)
    want[:, column_of(6, census_law.clique, 6, 0)] = 33649
    assert comb(23, 5) == 33649 and not failed.any() and torch.equal(gdv, want)


def test_complete_bipartite_12_12_at_six():
    ei, ptr = census_law.batch([census_law.bipartite(12, 12)])
    gdv, failed = vertex_census(ei, ptr, 6)
    assert not failed.any() and int(gdv.sum()) == 6 * 132748 and torch.equal(gdv, recipe(ei, ptr, 6)[0])
    assert torch.equal(gdv, gdv[:1].expand(24, -1))                             # the graph is vertex-transitive
    check_identity_five(gdv, ei, ptr, 6)


# ---- 4. past the recipe's cap -------------------------------------------------------------------------------------------------------------
def test_clique_of_44_at_seven():
    ei, ptr = census_law.batch([census_law.clique(44)])
    gdv, failed = vertex_census(ei, ptr, 7, limit=1 << 27)
    want = torch.zeros_like(gdv)
    want[:, column_of(7, census_law.clique, 7, 0)] = 6096454
    assert comb(43, 6) == 6096454 and not failed.any() and torch.equal(gdv, want)


def test_clique_of_44_fails_alone_at_the_default_limit():
    ei, ptr = census_law.batch([census_law.cycle(9), census_law.clique(44), census_law.star(8, centre=2)])
    gdv, failed = vertex_census(ei, ptr, 7)
    assert failed.tolist() == [False, True, False]
    want = law.vertex_census(*census_law.batch([census_law.cycle(9), (44, []), census_law.star(8, centre=2)]), 7, **handed(7))
    assert np.array_equal(gdv.cpu().numpy(), want) and want[:9].sum() == 63 and want[9:53].sum() == 0 and want[53:].sum() == 7 * comb(8, 6)


def test_limit_is_per_graph():
    ei, ptr = census_law.batch([census_law.cycle(9), census_law.clique(10), census_law.path(7), census_law.clique(10)])
    k, sets = 4, comb(10, 4)
    want = law.vertex_census(ei, ptr, k)
    gdv, failed = vertex_census(ei, ptr, k, limit=sets)                         # two graphs at the limit, together past it
    assert failed.tolist() == [False] * 4 and np.array_equal(gdv.cpu().numpy(), want)
    gdv, failed = vertex_census(ei, ptr, k, limit=sets - 1)
    assert failed.tolist() == [False, True, False, True]
    assert np.array_equal(gdv.cpu().numpy(), law.vertex_census(ei, ptr, k, failed={1, 3}))


def test_a_graph_far_past_the_limit_fails_alone():
    ei, ptr = census_law.batch([census_law.cycle(9), census_law.clique(30), census_law.path(7)])    # 593 775 sets at k = 6: the flushes stop it early
    gdv, failed = vertex_census(ei, ptr, 6, limit=1000)
    assert failed.tolist() == [False, True, False]
    assert np.array_equal(gdv.cpu().numpy(), law.vertex_census(*census_law.batch([census_law.cycle(9), (30, []), census_law.path(7)]), 6))


# ---- 5. bit 63 ------------------------------------------------------------------------------------------------------------------------
def star_want(gdv, k, n, centre, lo=0):
    want = torch.zeros_like(gdv)
    want[lo:lo + n, column_of(k, census_law.star, k - 1, 1)] = comb(n - 2, k - 2)
    want[lo + centre] = 0
    want[lo + centre, column_of(k, census_law.star, k - 1, 0)] = comb(n - 1, k - 1)
    return want


def path_want(gdv, k, n, ring, lo=0):
    """Vertex i of a path of n is at position p of the window that starts at i - p; a ring has every start."""
    want = torch.zeros_like(gdv)
    for p in range(k):
        col = column_of(k, census_law.path, k, p)
        first, last = (0, n - 1) if ring else (p, n - k + p)
        want[lo + first:lo + last + 1, col] += 1
    return want


@pytest.mark.parametrize("k", [3, 4, 5])
def test_star_of_64_vertices_with_centre_63(k):
    ei, ptr = census_law.batch([census_law.star(63, 63)])
    gdv, failed = vertex_census(ei, ptr, k)
    assert not failed.any() and torch.equal(gdv, star_want(gdv, k, 64, 63))


@pytest.mark.parametrize("k", range(2, 8))
def test_cycle_of_64_vertices(k):
    ei, ptr = census_law.batch([census_law.cycle(64)])
    gdv, failed = vertex_census(ei, ptr, k)
    assert not failed.any() and torch.equal(gdv, path_want(gdv, k, 64, True)) and int(gdv.sum()) == 64 * k


# ---- 6. the wide form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("k", [2, 3, 4, 7])
def test_wide_path_ring_and_star(k, n):
    graphs = [census_law.path(n), census_law.cycle(n), census_law.star(n - 1, centre=n - 1) if k < 7 else census_law.star(20, centre=20),
              census_law.clique(5)]                                             # C(129, 6) stars would take the test past a second
    ei, ptr = census_law.batch(graphs)
    with limits(max_vertices=1024):
        gdv, failed = vertex_census(ei, ptr, k)
    want = path_want(gdv, k, n, False) + path_want(gdv, k, n, True, lo=n) + star_want(gdv, k, graphs[2][0], graphs[2][0] - 1, lo=2 * n)
    if k <= 5:
        want[int(ptr[3]):, column_of(k, census_law.clique, k, 0)] = comb(4, k - 1)
    assert not failed.any() and torch.equal(gdv, want)


def test_wide_sparse_200_vertex_graph_against_the_recipe():
    import ugs_workloads as wl
    ei, ptr = wl.tu_graph(200, 260, 11), np.array([0, 200], np.int64)
    with limits(max_vertices=1024):
        gdv, failed = vertex_census(ei, ptr, 4)
        want, _ = recipe(ei, ptr, 4)
        check_identity_five(gdv, ei, ptr, 4)
    assert not failed.any() and torch.equal(gdv, want) and int(gdv.sum()) > 4000


@pytest.mark.parametrize("k", range(1, 8))
def test_wide_kernel_on_the_mixed_batch(k):
    with limits(mask_vertices=0):
        got = run_mixed(k)
    assert np.array_equal(got.cpu().numpy(), mixed_want(k))


def test_a_graph_of_65_vertices_fails_alone_by_default():
    import uniform_sampler as us
    assert us.max_vertices() == 64
    ei, ptr = census_law.batch([census_law.cycle(9), census_law.path(65), census_law.clique(6)])
    gdv, failed = vertex_census(ei, ptr, 4)
    assert failed.tolist() == [False, True, False]
    assert np.array_equal(gdv.cpu().numpy(), law.vertex_census(ei, ptr, 4, failed={1}))


# ---- 7. degenerate and bad arguments ------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    none = torch.zeros((2, 0), dtype=torch.int64)
    gdv, failed = vertex_census(none, torch.zeros((1,), dtype=torch.int64), 5)  # G = 0
    assert gdv.shape == (0, 58) and failed.shape == (0,)
    gdv, failed = vertex_census(none, torch.tensor([4]), 5)                     # G = 0 behind four vertices of no graph
    assert gdv.shape == (4, 58) and int(gdv.abs().sum()) == 0
    gdv, failed = vertex_census(none, torch.tensor([0, 3, 3, 9]), 1)            # E = 0: every vertex is a set at k = 1
    assert gdv.tolist() == [[1]] * 9 and not failed.any()
    gdv, failed = vertex_census(none, torch.tensor([0, 3, 3, 9]), 2)
    assert gdv.tolist() == [[0]] * 9 and not failed.any()


def test_rows_below_the_first_graph_are_zero():
    ei, ptr = mixed_batch(4)
    gdv, failed = vertex_census(ei + 7, ptr + 7, 4)
    assert not failed.any() and int(gdv[:7].abs().sum()) == 0 and np.array_equal(gdv[7:].cpu().numpy(), mixed_want(4))


def test_bad_arguments():
    from ugs_sampler import graphlets
    ei, ptr = census_law.batch([census_law.clique(5)])
    e_t, p_t = torch.from_numpy(ei), torch.from_numpy(ptr)
    with pytest.raises(RuntimeError):
        graphlets.vertex_census(e_t, torch.tensor([0, 5, 3]), 3, device=DEV)    # a decreasing ptr
    with pytest.raises(RuntimeError):
        graphlets.vertex_census(e_t, torch.tensor([-2, 5]), 3, device=DEV)
    with pytest.raises(RuntimeError, match="1 <= k <= 7"):
        graphlets.vertex_census(e_t, p_t, 8, device=DEV)
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="1 <= k <= 8"):
            graphlets.vertex_census(e_t, p_t, k, device=DEV)
    for limit in (0, (1 << 32) + 1):
        with pytest.raises(ValueError, match="limit"):
            graphlets.vertex_census(e_t, p_t, 3, limit=limit, device=DEV)
    with pytest.raises(RuntimeError, match="GPU"):
        graphlets.vertex_census(e_t, p_t, 3, device="cpu")
    assert vertex_census(ei, ptr, 3, limit=1 << 32)[0].tolist() == [[0, 0, 6]] * 5


# ---- 8. nothing else changed -------------------------------------------------------------------------------------------------------------
def test_the_neighbours_are_undisturbed():
    import uniform_sampler as us
    from ugs_sampler import graphlets
    ei, ptr = mixed_batch(5)
    e_t, p_t = torch.from_numpy(ei), torch.from_numpy(ptr)

    def others():
        return us.count_graphs(e_t, p_t, 5) + us.enumerate_graphs(e_t, p_t, 5, device=DEV) + graphlets.census(e_t, p_t, 5, device=DEV)

    before = others()
    gdv, _ = vertex_census(ei, ptr, 5)
    after = others()
    assert len(before) == len(after) == 10
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert np.array_equal(gdv.cpu().numpy(), mixed_want(5))
