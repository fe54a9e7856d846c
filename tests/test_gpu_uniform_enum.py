"""uniform_sampler.enumerate_graphs / count_graphs on the GPU against the CPU law (tests/uniform_enum_law.py): bit-exact, every
tensor.  The vertex limit and the mask threshold are process-wide, so every test that changes them restores them."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import ugs_workloads as wl
import uniform_enum_law as EL
import uniform_law as U
import uniform_wide_law as W
import wl_law

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def sampler():
    import uniform_sampler
    return uniform_sampler


@contextlib.contextmanager
def limits(max_vertices=None, mask_vertices=None):
    us = sampler()
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


def tensors(ei, ptr, device=None):
    e, p = torch.from_numpy(np.ascontiguousarray(ei)), torch.from_numpy(np.asarray(ptr, np.int64))
    return (e.to(device), p.to(device)) if device is not None else (e, p)


def enum(ei, ptr, k, mode="sample", device=None, **kw):
    return sampler().enumerate_graphs(*tensors(ei, ptr, device), k, mode, **kw)


def count(ei, ptr, k, **kw):
    counts, failed = sampler().count_graphs(*tensors(ei, ptr), k, **kw)
    assert counts.dtype == torch.int64 and failed.dtype == torch.bool and not counts.is_cuda and not failed.is_cuda
    return counts.tolist(), failed.tolist()


def assert_same(got, want, what=""):
    assert len(got) == 6 and got[5].dtype == torch.bool and not got[5].is_cuda, what
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy()
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def check(ei, ptr, k, modes=("sample",), failed=(), what="", **kw):
    """enumerate_graphs equals the law in every mode; on a healthy batch count_graphs equals diff(sample_ptr) and the law's counts"""
    G = len(ptr) - 1
    sets = EL.graph_sets(ei, ptr, k)
    for mode in modes:
        law = EL.enumerate_graphs(ei, ptr, k, mode, failed=failed, sets=sets)
        got = enum(ei, ptr, k, mode, **kw)
        assert_same(got, law, (what, mode))
        assert got[5].tolist() == [g in failed for g in range(G)], (what, mode)
        assert (got[0].cpu().numpy() >= 0).all()
    if not failed:
        counts, cfailed = count(ei, ptr, k)
        assert counts == np.diff(law[3]).tolist() == law[5].tolist() and cfailed == [False] * G, what
    return law


def undirected(pairs):
    a = np.array(pairs, np.int64).reshape(-1, 2).T
    return np.concatenate([a, a[::-1]], axis=1)


def complete_graph(n):
    u, v = np.triu_indices(n, 1)
    return np.array([np.r_[u, v], np.r_[v, u]], np.int64)


# ---- 1. hand graphs ----
def hand_batch():
    """ptr[0] = 5.  A path of 5; a triangle with a tail (both directions, loops, duplicate columns); 4 isolated vertices; a graph of
    2 vertices (n < k at k = 3) in the middle; an empty graph; a path of 3 -- and columns that cross graph ranges or lie outside all."""
    path = undirected([(0, 1), (1, 2), (2, 3), (3, 4)])
    tailed = np.array([[0, 1, 1, 2, 2, 0, 2, 3, 3, 4, 1, 1, 0, 2, 4],
                       [1, 0, 2, 1, 0, 2, 3, 2, 4, 3, 1, 1, 1, 3, 4]], np.int64)        # loops at 1 (twice) and 4, (0,1) and (2,3) again
    two = np.array([[0], [1]], np.int64)
    last = np.array([[0, 1], [1, 2]], np.int64)                                          # one direction only
    ei, ptr = W.batch([(5, path), (5, tailed), (4, np.zeros((2, 0), np.int64)), (2, two), (0, np.zeros((2, 0), np.int64)), (3, last)], first=5)
    stray = np.array([[9, 10, 0, 30, 3, 21], [10, 9, 6, 31, 5, 24]], np.int64)            # across ranges, below ptr[0], above ptr[G]
    ei = np.concatenate([ei[:, :7], stray[:, :3], ei[:, 7:], stray[:, 3:]], axis=1)
    return np.ascontiguousarray(ei), ptr


@pytest.mark.parametrize("k", [2, 3])
def test_hand_graphs_in_all_modes(k):
    ei, ptr = hand_batch()
    law = check(ei, ptr, k, modes=("sample", "graph", "global"), what=f"hand k={k}")
    sp = law[3]
    assert sp[0] == 0 and sp[3] == sp[2] and sp[5] == sp[4]                              # isolated vertices and the empty graph: no rows
    if k == 3:
        assert sp[4] == sp[3]                                                            # n < k in the middle
        assert law[5].tolist() == [3, 4, 0, 0, 0, 1]


# ---- 2. degenerate k ----
def test_k0_gives_no_rows():
    ei, ptr = hand_batch()
    got = enum(ei, ptr, 0)
    assert tuple(got[0].shape) == (0, 0) and tuple(got[1].shape) == (2, 0) and got[2].tolist() == [0]
    assert got[3].tolist() == [0] * len(ptr) and tuple(got[4].shape) == (0,) and got[5].tolist() == [False] * (len(ptr) - 1)
    check(ei, ptr, 0, what="k=0")


def test_k1_rows_are_the_vertices_and_loops_are_edges():
    ei, ptr = hand_batch()
    law = check(ei, ptr, 1, modes=("sample", "global"), what="k=1")
    assert np.array_equal(law[0][:, 0], np.arange(ptr[0], ptr[-1])) and law[2][-1] == 3 and np.array_equal(np.diff(law[3]), np.diff(ptr))


def test_k_equal_n():
    ei, ptr = hand_batch()
    law = check(ei, ptr, 5, modes=("sample", "global"), what="k=n")
    assert law[5].tolist() == [1, 1, 0, 0, 0, 0] and np.array_equal(law[0][0], np.arange(5, 10))


# ---- 3. larger mask graphs ----
def test_bit_63():
    ei = wl.tu_graph(64, 100, 7)
    law = check(ei, [0, 64], 5, modes=("sample", "global"), what="tu64")
    assert law[5].tolist() == [4601] and (law[0] == 63).any()


@pytest.mark.parametrize("k", [4, 6])
def test_rows_cross_workgroups_and_graph_boundaries(k):
    ei, ptr = W.batch([(11, wl.csl_graph(11, 2))] * 3 + [(41, wl.csl_graph(41, 2))], first=2)
    law = check(ei, ptr, k, modes=("sample", "graph"), what=f"csl k={k}")
    if k == 4:
        assert law[5][:3].tolist() == [88] * 3                                           # boundaries at 88, 176 and, past the first workgroup, 264
    else:
        assert law[5][3] == 1312


@functools.lru_cache(maxsize=None)
def tu20():
    ei = wl.tu_graph(20, 100, 1)
    ptr = np.array([0, 20], np.int64)
    return ei, ptr, EL.graph_sets(ei, ptr, 6)


@pytest.mark.parametrize("mode", ["sample", "global"])
def test_segmented_radix_path(mode):
    """34 109 sets; the largest root bucket (10 489) is above SMALL_SORT = 8192, so its keys go through the segmented radix sort"""
    ei, ptr, sets = tu20()
    assert len(sets[0]) == 34109 and np.bincount(sets[0][:, 0]).max() == 10489
    assert_same(enum(ei, ptr, 6, mode), EL.enumerate_graphs(ei, ptr, 6, mode, sets=sets), mode)
    if mode == "sample":
        assert count(ei, ptr, 6) == ([34109], [False])


# ---- 4. wide graphs ----
WIDE = {"tu65": (65, 100, 1, 4, 922), "tu129": (129, 190, 2, 4, 2351), "tu257": (257, 300, 4, 3, 676)}


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_graphs(name):
    n, e, seed, k, sets = WIDE[name]
    ei, ptr = W.batch([(n, wl.tu_graph(n, e, seed))], first=3)
    with limits(1024):
        law = check(ei, ptr, k, modes=("sample", "global"), what=name)
    assert law[5].tolist() == [sets]


def mixed_graphs():
    return [(70, wl.tu_graph(70, 76, 5)), (12, wl.tu_graph(12, 15, 6)), (130, wl.tu_graph(130, 136, 7)), (2, np.array([[0], [1]], np.int64)),
            (30, wl.tu_graph(30, 36, 8))]


def test_wide_and_mask_graphs_interleaved():
    """[wide, mask, wide, mask with n < k, mask]: the keys lie mask graphs first, the rows in batch order"""
    ei, ptr = W.batch(mixed_graphs(), first=1)
    with limits(1024):
        law = check(ei, ptr, 4, modes=("sample", "graph"), what="mixed")
    assert (law[5] > 0).tolist() == [True, True, True, False, True]
    with limits(64):                                                                     # at the default limit the wide ones fail alone
        check(ei, ptr, 4, failed=(0, 2), what="mixed at 64")


def test_small_graphs_through_the_wide_kernels():
    ei, ptr = hand_batch()
    ei2, ptr2 = W.batch([(11, wl.csl_graph(11, 2)), (20, wl.tu_graph(20, 30, 3)), (64, wl.tu_graph(64, 70, 4))], first=4)
    for e, p, k in ((ei, ptr, 3), (ei, ptr, 1), (ei2, ptr2, 4)):
        want = enum(e, p, k, "sample")
        with limits(mask_vertices=0):
            check(e, p, k, modes=("sample", "global"), what=f"mask_vertices=0 k={k}")
            for a, b in zip(enum(e, p, k, "sample"), want):
                assert torch.equal(a, b)
        assert_same(enum(e, p, k, "sample"), EL.enumerate_graphs(e, p, k, "sample"), "restored")


# ---- 5. failures ----
def test_a_65_vertex_graph_fails_alone_at_the_default_limit():
    ei, ptr = W.batch([(8, complete_graph(8)), (65, wl.tu_graph(65, 100, 1)), (11, wl.csl_graph(11, 2))], first=2)
    with limits(64):
        check(ei, ptr, 4, modes=("sample", "global"), failed=(1,), what="65 at 64")
        assert count(ei, ptr, 4) == ([70, -1, 88], [False, True, False])
        check(ei, ptr, 66, what="n < k is no failure")                                  # fewer than k vertices: empty, not refused
    with limits(1024):
        check(ei, ptr, 4, what="65 at 1024")


def test_max_rows_and_limit():
    k8, k8ptr = complete_graph(8), np.array([0, 8], np.int64)
    check(k8, k8ptr, 4, max_rows=70, what="K8 at 70")
    two, twoptr = W.batch([(8, k8), (8, k8)])
    with pytest.raises(RuntimeError, match="split the call"):
        enum(two, twoptr, 4, max_rows=100)
    check(two, twoptr, 4, max_rows=140, what="after the refusal")
    ei, ptr = W.batch([(8, k8), (11, wl.csl_graph(11, 2))], first=1)
    law = check(ei, ptr, 4, modes=("sample", "global"), failed=(1,), max_rows=80, what="[K8, csl11] at 80")
    assert law[3].tolist() == [0, 70, 70] and law[5].tolist() == [70, 88]
    got = enum(k8, k8ptr, 4, max_rows=69)                                                # alone and over: no rows, no error
    assert got[5].tolist() == [True] and got[3].tolist() == [0, 0] and tuple(got[0].shape) == (0, 4)
    assert count(k8, k8ptr, 4, limit=70) == ([70], [False])
    assert count(k8, k8ptr, 4, limit=69) == ([-1], [True])
    assert count(ei, ptr, 4, limit=80) == ([70, -1], [False, True])
    check(ei, ptr, 4, what="after the refusals")


# ---- 6. placement and cross-checks ----
def test_placement():
    ei, ptr = W.batch([(11, wl.csl_graph(11, 2)), (8, complete_graph(8))], first=2)
    want = EL.enumerate_graphs(ei, ptr, 4)
    host = enum(ei, ptr, 4)
    assert all(t.device.type == "cpu" for t in host) and all(t.is_pinned() for t in host[:5] if t.numel() > 0)
    dev = enum(ei, ptr, 4, device="cuda:0")
    assert all(t.is_cuda for t in dev[:5]) and not dev[5].is_cuda
    placed = sampler().enumerate_graphs(*tensors(ei, ptr), 4, device="cuda:0")
    assert all(t.is_cuda for t in placed[:5])
    for got in (host, dev, placed):
        assert_same(got, want)


def test_sample_graphs_rows_are_enumeration_rows_at_the_drawn_index():
    ei, ptr = W.batch([(11, wl.csl_graph(11, 2))] * 3 + [(41, wl.csl_graph(41, 2))], first=2)
    k, m, seeds = 6, 24, [42, 0, (1 << 64) - 1, 7]
    nodes, eidx, eptr, sptr, esrc, failed = [t.cpu().numpy() for t in enum(ei, ptr, k, "global")]
    out = sampler().sample_graphs(*tensors(ei, ptr), m, k, np.array(seeds, np.uint64), mode="global")
    s_nodes, s_eidx, s_eptr, _, s_esrc, s_failed = [t.cpu().numpy() for t in out]
    assert not failed.any() and not s_failed.any()
    for g in range(4):
        gen = U.mt19937_64(seeds[g])
        for i in range(m):
            r, row = sptr[g] + U.lemire(gen, int(sptr[g + 1] - sptr[g])), g * m + i
            a, b, c, d = s_eptr[row], s_eptr[row + 1], eptr[r], eptr[r + 1]
            assert np.array_equal(s_nodes[row], nodes[r]), (g, i)
            assert np.array_equal(s_eidx[:, a:b], eidx[:, c:d]) and np.array_equal(s_esrc[a:b], esrc[c:d]), (g, i)


def test_exact_wl_histogram_of_a_csl_graph():
    from ugs_sampler import wl as wlh
    ei, ptr = wl.csl_graph(41, 2), np.array([0, 41], np.int64)
    nodes, eidx, eptr = enum(ei, ptr, 6, device="cuda:0")[:3]
    assert nodes.shape[0] == 1312
    digest, status = wlh.wl_hash(nodes, eidx, eptr)
    hexes, stats, _ = wl_law.wl_rows(nodes.cpu().numpy(), eidx.cpu().numpy(), eptr.cpu().numpy())
    assert status.cpu().tolist() == stats == [0] * 1312
    assert wlh.hexdigests(digest, status) == hexes
