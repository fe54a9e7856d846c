"""graphlets.census / vertex_census with form="csr" on the GPU (csr_validate, csr_census_esu, csr_vcensus_esu, csr_single and the clears
in ugs_census_csr.hip): bit for bit against the bitmap form wherever that form runs, against the numpy laws of
tests/graphlet_census_law.py and tests/graphlet_vertex_census_law.py above its size limit, against closed forms on hubs and long
cycles, and the validation pass straight through the C ABI.  The inputs shared with the bitmap form's tests are taken from their
modules."""
import functools
from math import comb

import numpy as np
import pytest
import torch

import graphlet_census_law as law
import graphlet_vertex_census_law as vlaw
import test_gpu_graphlet_census as cen
import test_gpu_graphlet_vertex_census as vcen

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dev = cen.dev


def both(ei, ptr, k, **kw):
    """(counts, gdv) of the csr form, shapes and placement checked by the bitmap tests' wrappers."""
    counts, failed = cen.census(ei, ptr, k, form="csr", **kw)
    gdv, vfailed = vcen.vertex_census(ei, ptr, k, form="csr", **kw)
    assert failed.tolist() == vfailed.tolist()
    return counts, gdv, failed


def bitmap(ei, ptr, k, **kw):
    counts, failed = cen.census(ei, ptr, k, **kw)
    gdv, vfailed = vcen.vertex_census(ei, ptr, k, **kw)
    assert not failed.any() and not vfailed.any()
    return counts, gdv


def same_as_bitmap(ei, ptr, k, **kw):
    counts, gdv, failed = both(ei, ptr, k, **kw)
    want_counts, want_gdv = bitmap(ei, ptr, k, **kw)
    assert not failed.any() and torch.equal(counts, want_counts) and torch.equal(gdv, want_gdv)
    return counts, gdv


# ---- 1. identity with the bitmap form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 8))
def test_mixed_batch_in_every_placement(k):
    ei, ptr = cen.mixed_batch(k)
    counts, gdv = same_as_bitmap(dev(ei), dev(ptr), k)
    assert counts.device.type == "cuda" and gdv.device.type == "cuda"
    assert np.array_equal(counts.cpu().numpy(), cen.mixed_want(k))
    E = ei.shape[1]
    wide = torch.zeros((2, E + 5), dtype=torch.int64, device=DEV)
    wide[:, :E] = dev(ei)
    spread = torch.zeros((2, 2 * E), dtype=torch.int64, device=DEV)
    spread[:, ::2] = dev(ei)
    for view in (wide[:, :E], spread[:, ::2]):
        assert not view.is_contiguous()
        c2, g2, _ = both(view, dev(ptr), k)
        assert torch.equal(c2, counts) and torch.equal(g2, gdv)
    c3, g3, _ = both(torch.from_numpy(ei), torch.from_numpy(ptr), k)            # host tensors, the result on `device`
    assert c3.device.type == "cuda" and torch.equal(c3, counts) and torch.equal(g3, gdv)
    c4, g4, failed = both(torch.from_numpy(ei), torch.from_numpy(ptr), k, device=None)
    assert c4.device.type == "cpu" and g4.device.type == "cpu" and not failed.any()
    assert torch.equal(c4, counts.cpu()) and torch.equal(g4, gdv.cpu())
    c5, _, _ = both(dev(ei), torch.from_numpy(ptr), k)                          # a host ptr beside a device edge_index
    assert torch.equal(c5, counts)


@pytest.mark.parametrize("n", [4, 5, 6])
def test_every_connected_class_as_its_own_graph(n):
    W = len(cen.columns(n))
    for ei, ptr in cen.class_batches(n):
        counts, _ = same_as_bitmap(ei, ptr, n)
        assert torch.equal(counts, torch.eye(W, dtype=torch.int64, device=DEV))
    ei, ptr = cen.class_batches(n)[0]
    for k in range(2, n):                                                       # the smaller sets inside every class
        same_as_bitmap(ei, ptr, k)


def test_all_codes_of_six_vertices():
    """32 768 graphs, a quarter of a million entries: every wave finds its row and its graph by search."""
    ei, ptr, _ = cen.all_codes_six()
    counts, failed = cen.census(ei, ptr, 6, form="csr")
    assert not failed.any() and torch.equal(counts, cen.run_all_codes_six())
    same_as_bitmap(ei, ptr, 4)


@pytest.mark.parametrize("graph,sets", [(law.clique(24), 134596), (law.bipartite(12, 12), 132748)])
def test_dense_graphs_at_six(graph, sets):
    ei, ptr = law.batch([graph])
    counts, gdv = same_as_bitmap(ei, ptr, 6)
    assert int(counts.sum()) == sets and int(gdv.sum()) == 6 * sets


def test_a_lane_past_4096_sets_and_the_limit_behind_it():
    """K28 at k = 7: the lane of (root, first, second extension) completes C(25, 4) = 12 650 sets, three flushes of the running total."""
    ei, ptr = law.batch([law.cycle(9), law.clique(28), law.path(8)])
    sets = comb(28, 7)
    counts, gdv, failed = both(ei, ptr, 7, limit=sets)
    assert not failed.any()
    want = torch.zeros_like(counts)
    want[0, cen.column_of(7, law.path(7))] = 9
    want[1, cen.column_of(7, law.clique(7))] = sets
    want[2, cen.column_of(7, law.path(7))] = 2
    assert torch.equal(counts, want)
    assert bool((gdv[9:37].sum(dim=1) == comb(27, 6)).all()) and int(gdv[9:37].sum()) == 7 * sets
    c2, g2, failed = both(ei, ptr, 7, limit=1000)                               # stopped at a flush, far before the end
    assert failed.tolist() == [False, True, False]
    want[1] = 0
    assert torch.equal(c2, want) and int(g2[9:37].sum()) == 0
    assert torch.equal(g2[:9], gdv[:9]) and torch.equal(g2[37:], gdv[37:])


def test_wide_graph_of_130_vertices():
    n, es = law.cycle(130)
    es = es + [(0, 64), (10, 70), (63, 65), (64, 128), (1, 129), (127, 3), (66, 66), (10, 70)]
    ei, ptr = law.batch([law.clique(6), (n, es)])
    for k in (3, 4, 5):
        counts, gdv, failed = both(ei, ptr, k)
        with cen.limits(max_vertices=1024):
            want_counts, want_gdv = bitmap(ei, ptr, k)
        assert not failed.any() and torch.equal(counts, want_counts) and torch.equal(gdv, want_gdv)
    assert cen.census(ei, ptr, 4)[1].tolist() == [False, True]                  # the size rule, which the csr form does not have


# ---- 2. above the old limit, against the numpy laws --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_graph():
    """110 blobs of 10 vertices with edge probability 0.45, one bridge from every blob to the next (the last to the first), the ids
    scattered by a permutation: 1100 vertices, 2356 edges, sparse but with every small class somewhere."""
    rng = np.random.default_rng(11)
    edges = [(10 * b + u, 10 * b + v) for b in range(110) for u in range(10) for v in range(u + 1, 10) if rng.random() < 0.45]
    edges += [(10 * b + int(rng.integers(10)), 10 * ((b + 1) % 110) + int(rng.integers(10))) for b in range(110)]
    perm = rng.permutation(1100)
    edges = [(int(perm[u]), int(perm[v])) for u, v in edges]
    assert len({(min(e), max(e)) for e in edges}) == 2356
    return 1100, edges


BLOB_SETS = {4: 16843, 5: 41487, 6: 109876}             # counted on the CPU by the law
BLOB_CLASSES = {4: 6, 5: 21, 6: 111}                     # of 6, 21, 112
BLOB_ORBITS = {4: 11, 5: 58}                             # of 11, 58


@functools.lru_cache(maxsize=None)
def blob_census_law(k):
    want = law.census(*law.batch([blob_graph()]), k)
    assert int(want.sum()) == BLOB_SETS[k] and int((want > 0).sum()) == BLOB_CLASSES[k]
    return want


@functools.lru_cache(maxsize=None)
def blob_vertex_law(k):
    want = vlaw.vertex_census(*law.batch([blob_graph()]), k)
    assert int(want.sum()) == k * BLOB_SETS[k] and int((want.sum(axis=0) > 0).sum()) == BLOB_ORBITS[k]
    return want


@pytest.mark.parametrize("k", [4, 5, 6])
def test_blob_graph_census_against_the_law(k):
    ei, ptr = law.batch([blob_graph()])
    counts, failed = cen.census(ei, ptr, k, form="csr")
    assert not failed.any() and np.array_equal(counts.cpu().numpy(), blob_census_law(k))
    assert cen.census(ei, ptr, k)[1].tolist() == [True]                         # new ground: the bitmap form refuses the graph
    ei2, ptr2 = law.batch([law.cycle(7), blob_graph()])                         # and as the second graph of a batch
    counts2, failed2 = cen.census(ei2, ptr2, k, form="csr")
    assert not failed2.any() and torch.equal(counts2[1], counts[0])
    assert np.array_equal(counts2[:1].cpu().numpy(), law.census(*law.batch([law.cycle(7)]), k))
    with cen.limits(max_vertices=1024):
        assert cen.census(ei2, ptr2, k)[1].tolist() == [False, True]


@pytest.mark.parametrize("k", [4, 5])
def test_blob_graph_vertex_census_against_the_law(k):
    ei, ptr = law.batch([blob_graph()])
    gdv, failed = vcen.vertex_census(ei, ptr, k, form="csr")
    assert not failed.any() and np.array_equal(gdv.cpu().numpy(), blob_vertex_law(k))
    assert vcen.vertex_census(ei, ptr, k)[1].tolist() == [True]
    ei2, ptr2 = law.batch([law.cycle(7), blob_graph()])
    gdv2, failed2 = vcen.vertex_census(ei2, ptr2, k, form="csr")
    assert not failed2.any() and torch.equal(gdv2[7:], gdv)
    assert np.array_equal(gdv2[:7].cpu().numpy(), vlaw.vertex_census(*law.batch([law.cycle(7)]), k))


@pytest.mark.parametrize("k", [4, 5, 6])
def test_item_five_between_the_two_csr_calls(k):
    ei, ptr = law.batch([law.clique(7), blob_graph(), law.star(9, centre=3)])
    counts, gdv, failed = both(ei, ptr, k)
    assert not failed.any()
    size, cls = vcen.orbit_sizes(k)
    sums = torch.stack([gdv[int(ptr[g]):int(ptr[g + 1])].sum(dim=0) for g in range(3)])
    assert torch.equal(sums, counts[:, cls.to(DEV)] * size.to(DEV))


# ---- 3. hubs and long cycles by closed form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", [0, 1200])
def test_star_of_1200_leaves_at_three(centre):
    ei, ptr = law.batch([law.star(1200, centre)])
    counts, gdv, failed = both(ei, ptr, 3)
    sets = comb(1200, 2)
    want = torch.zeros_like(counts)
    want[0, cen.column_of(3, law.path(3))] = sets
    assert sets == 719400 and not failed.any() and torch.equal(counts, want)
    middle, end = vcen.column_of(3, law.path, 3, 1), vcen.column_of(3, law.path, 3, 0)
    want_gdv = torch.zeros_like(gdv)
    want_gdv[:, end] = 1199
    want_gdv[centre, end] = 0
    want_gdv[centre, middle] = sets
    assert torch.equal(gdv, want_gdv)
    deg = both(ei, ptr, 2)[1]                                                   # at k = 2 the one column is the degree
    assert int(deg[centre, 0]) == 1200 and int(deg.sum()) == 2400 and int(deg.max()) == 1200 and int(deg.min()) == 1


def test_cycle_of_1500_vertices_at_five():
    ei, ptr = law.batch([law.cycle(1500)])
    counts, gdv, failed = both(ei, ptr, 5)
    want = torch.zeros_like(counts)
    want[0, cen.column_of(5, law.path(5))] = 1500
    assert not failed.any() and torch.equal(counts, want)
    want_gdv = torch.zeros_like(gdv)
    for vertex, n in ((0, 2), (1, 2), (2, 1)):                                  # end, next to the end, middle
        want_gdv[:, vcen.column_of(5, law.path, 5, vertex)] = n
    assert torch.equal(gdv, want_gdv)


@functools.lru_cache(maxsize=None)
def path_with_a_clique():
    """A path of 600 vertices and six more that form a K7 with vertex 300."""
    n, es = law.path(600)
    members = [300] + list(range(600, 606))
    return 606, es + [(u, v) for a, u in enumerate(members) for v in members[a + 1:]]


def test_path_of_600_with_a_clique_at_seven():
    graph = path_with_a_clique()
    ei, ptr = law.batch([graph])
    counts, gdv, failed = both(ei, ptr, 7)
    assert not failed.any()
    want = law.census(ei, ptr, 7, cen.columns(7))
    assert np.array_equal(counts.cpu().numpy(), want)
    # 594 paths inside the path, and 12 that end in a clique vertex: it, vertex 300 and five more to one side
    assert int(want[0, cen.column_of(7, law.clique(7))]) == 1 and int(want[0, cen.column_of(7, law.path(7))]) == 594 + 12
    assert np.array_equal(gdv.cpu().numpy(), vlaw.vertex_census(ei, ptr, 7, **vcen.handed(7)))
    with cen.limits(max_vertices=1024):
        assert cen.census(ei, ptr, 7)[1].tolist() == [True]                     # the wide rule: k * b <= 64 fails at 606 vertices


# ---- 4. limit ----------------------------------------------------------------------------------------------------------------------------------
def test_the_star_past_the_limit_fails_alone():
    ei, ptr = law.batch([law.cycle(9), law.star(1200, 7), law.clique(5)])
    counts, gdv, failed = both(ei, ptr, 3, limit=100000)
    assert failed.tolist() == [False, True, False]
    want = law.census(*law.batch([law.cycle(9), (1201, []), law.clique(5)]), 3)
    assert np.array_equal(counts.cpu().numpy(), want) and int(gdv[9:1210].sum()) == 0
    assert int(gdv[:9].sum()) == 27 and int(gdv[1210:].sum()) == 30
    counts, gdv, failed = both(ei, ptr, 3, limit=1 << 40)
    assert not failed.any() and int(counts[1].sum()) == 719400 and int(gdv[9:1210].sum()) == 3 * 719400
    counts, _, failed = both(ei, ptr, 3, limit=719400)                          # at the limit is within it
    assert not failed.any() and int(counts[1].sum()) == 719400
    assert both(ei, ptr, 3, limit=719399)[2].tolist() == [False, True, False]


# ---- 5. degenerate and bad input ------------------------------------------------------------------------------------------------------------------
def test_degenerate_batches():
    none = torch.zeros((2, 0), dtype=torch.int64)
    counts, gdv, failed = both(none, torch.zeros((1,), dtype=torch.int64), 5)   # G = 0
    assert counts.shape == (0, 21) and gdv.shape == (0, 58) and failed.shape == (0,)
    ptr = torch.tensor([0, 3, 3, 9])
    counts, gdv, failed = both(none, ptr, 1)                                    # no columns: every vertex is a set at k = 1
    assert counts.tolist() == [[3], [0], [6]] and gdv.tolist() == [[1]] * 9 and not failed.any()
    counts, gdv, failed = both(none, ptr, 2)
    assert counts.tolist() == [[0], [0], [0]] and int(gdv.sum()) == 0 and not failed.any()
    ei, ptr = law.batch([law.clique(4), law.path(3), (0, []), law.clique(6)])   # n < k: healthy with zeros
    counts, gdv, failed = both(ei, ptr, 5)
    assert not failed.any() and counts.sum(dim=1).tolist() == [0, 0, 0, 6] and int(gdv[:7].sum()) == 0
    assert both(ei, ptr, 1, limit=5)[2].tolist() == [False, False, False, True]


def test_rows_below_the_first_graph_are_zero():
    ei, ptr = law.batch([law.clique(5), law.path(4)])
    ei, ptr = ei + 3, ptr + 3
    ei = np.concatenate([ei, np.array([[0, 1, 2], [1, 2, 4]], np.int64)], axis=1)       # columns below and across ptr[0]
    for k in (1, 2, 3):
        counts, gdv, failed = both(ei, ptr, k)
        want_counts, want_gdv = bitmap(ei, ptr, k)
        assert not failed.any() and torch.equal(counts, want_counts) and torch.equal(gdv, want_gdv)
        assert int(gdv[:3].sum()) == 0 and gdv.shape[0] == 12


def test_bad_arguments_on_the_device_path():
    ei, ptr = law.batch([law.clique(5)])
    for form_call in (cen.census, vcen.vertex_census):
        with pytest.raises(RuntimeError, match="ptr must be non-decreasing"):
            form_call(ei, np.array([0, 5, 3], np.int64), 3, form="csr")
        with pytest.raises(RuntimeError):
            form_call(ei, np.array([-1, 5], np.int64), 3, form="csr")
    assert cen.census(ei, ptr, 3, form="csr", limit=1 << 62)[0].tolist() == [[0, 10]]


def csr_call(k, ptr, rowptr, col):
    """Both C entries on a hand-made CSR: (census rc, counts, vertex census rc, gdv)."""
    from ugs_sampler import _graphs, graphlets
    from ugs_sampler._lib import lib
    d = torch.device(DEV)
    _graphs._select_device(d, jobs=True)
    keys, code_col = graphlets._census_tables(d, k)
    obase, O, tab = graphlets._vertex_census_tables(d, k)
    p, r = dev(np.array(ptr, np.int64)), dev(np.array(rowptr, np.int64))
    c = dev(np.array(col, np.int32))
    G, N, M = len(ptr) - 1, len(rowptr) - 1, len(col)
    counts = torch.full((G, keys.numel()), -7, dtype=torch.int64, device=d)
    gdv = torch.full((N, O), -7, dtype=torch.int64, device=d)
    status = np.zeros(max(G, 1), np.int32)
    rc1 = lib.ugs_graphlet_census_csr(p.data_ptr(), G, r.data_ptr(), c.data_ptr(), N, M, k, 1 << 25, keys.data_ptr(), keys.numel(),
                                      code_col.data_ptr(), counts.data_ptr(), status.ctypes.data)
    rc2 = lib.ugs_graphlet_vertex_census_csr(p.data_ptr(), G, r.data_ptr(), c.data_ptr(), N, M, k, 1 << 25, obase.numel() - 1,
                                             obase.data_ptr(), O, tab.data_ptr(), gdv.data_ptr(), status.ctypes.data)
    torch.cuda.synchronize()
    return rc1, counts, rc2, gdv


PATH5 = ([0, 5], [0, 1, 3, 5, 7, 8], [1, 0, 2, 1, 3, 2, 4, 3])

BROKEN = {
    "an entry outside its graph": ([0, 3, 5], PATH5[1], PATH5[2]),
    "an entry that is no vertex": (PATH5[0], PATH5[1], [1, 0, 2, 1, 3, 2, 7, 3]),
    "a negative entry": (PATH5[0], PATH5[1], [1, 0, 2, 1, 3, 2, -4, 3]),
    "a row out of order": (PATH5[0], PATH5[1], [1, 2, 0, 1, 3, 2, 4, 3]),
    "a repeated entry": (PATH5[0], [0, 2, 4, 6, 8, 9], [1, 1, 0, 2, 1, 3, 2, 4, 3]),
    "a missing mirror": (PATH5[0], [0, 1, 2, 4, 6, 7], [1, 2, 1, 3, 2, 4, 3]),
    "a loop": (PATH5[0], [0, 2, 4, 6, 8, 9], [0, 1, 0, 2, 1, 3, 2, 4, 3]),
    "rowptr that decreases": (PATH5[0], [0, 3, 1, 5, 7, 8], PATH5[2]),
    "rowptr that starts late": (PATH5[0], [1, 1, 3, 5, 7, 8], PATH5[2]),
    "rowptr that ends early": (PATH5[0], [0, 1, 3, 5, 7, 7], PATH5[2]),
    "rowptr past the entries": (PATH5[0], [0, 1, 3, 5, 7, 99], PATH5[2]),
    "a negative rowptr": (PATH5[0], [0, -1, 3, 5, 7, 8], PATH5[2]),
    "a negative rowptr under an entry that passes its other tests": (PATH5[0], [0, -1, 3, 5, 7, 8], [0, 0, 2, 1, 3, 2, 4, 3]),
    "ptr that decreases": ([0, 4, 3, 5], PATH5[1], PATH5[2]),
    "ptr that ends elsewhere": ([0, 4], PATH5[1], PATH5[2]),
    "a negative ptr": ([-1, 5], PATH5[1], PATH5[2]),
    "a row below the first graph": ([1, 5], PATH5[1], PATH5[2]),
}


def test_a_broken_csr_through_the_c_abi_is_an_argument_error():
    """The validation pass answers UGS_E_BAD_ARG before the search reads through the CSR; a sound call afterwards is exact."""
    from ugs_sampler._lib import lib
    rc1, counts, rc2, gdv = csr_call(3, *PATH5)
    assert rc1 == 0 and rc2 == 0 and counts.tolist() == [[3, 0]] and gdv.sum(dim=1).tolist() == [1, 2, 3, 2, 1]
    for name, (ptr, rowptr, col) in BROKEN.items():
        rc1, _, rc2, _ = csr_call(3, ptr, rowptr, col)
        assert (rc1, rc2) == (-4, -4), name
        assert b"strictly ascending" in lib.ugs_last_error(), name
    rc1, counts2, rc2, gdv2 = csr_call(3, *PATH5)
    assert rc1 == 0 and rc2 == 0 and torch.equal(counts2, counts) and torch.equal(gdv2, gdv)


# ---- 6. nothing else changed ------------------------------------------------------------------------------------------------------------------------
def test_the_neighbours_are_undisturbed():
    import uniform_sampler as us
    from ugs_sampler import graphlets
    ei, ptr = cen.mixed_batch(5)
    e_t, p_t = torch.from_numpy(ei), torch.from_numpy(ptr)

    def others():
        return (graphlets.census(e_t, p_t, 5, device=DEV) + graphlets.vertex_census(e_t, p_t, 5, device=DEV) + us.count_graphs(e_t, p_t, 5)
                + us.sample_batch(e_t.to(DEV), p_t.to(DEV), 6, 5, seed=9))

    before = others()
    both(ei, ptr, 5)
    both(*law.batch([blob_graph()]), 4)
    after = others()
    assert len(before) == len(after) >= 9
    for a, b in zip(before, after):
        assert torch.equal(a, b)
