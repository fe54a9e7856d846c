"""GPU: the row of the LAST vertex of a sample in the one-walk-per-wave tiers (do_walk's last pick, scan_chunk_last), every output
against the CPU oracle by exact equality in all three edge modes.  That row is scanned by comparing each neighbour with the sampled
vertices themselves instead of probing the membership table, and the last pick leaves out the upkeep nothing reads any more (the
shift of the candidate list, the stages' validity, the vertex's flag in the table).  Small graphs (a dozen to 600 vertices, a few
hundred to a few thousand rows) built so that a walk meets what that can get wrong: self loops of the last vertex and of earlier
members (the column once and twice), a sampled neighbour repeated in the last row, a last row of ~200 entries with hits in its
second and third chunk, samples that are cliques (every member a hit; more hits than the staging list holds), k = 1, 2, 3, 8, 14 and
32, walks that stop early beside complete ones, relaxed roots, several graphs, one seed per graph, every tier, walks handed on
from the 448-candidate tier, rows read through the row pointer, and many consecutive walks per wave.  Each case asserts on the
oracle's output that the sample has the property it is named for."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

MODES = ("sample", "graph", "global")
TIER_M = 1                                                                     # 448 candidates, one walk per wave


def _sym_rows(ei, n):
    """row of every vertex in the symmetrised adjacency in the sampler's order (column order): a column (u, v) is an entry of u's
    row and of v's; a self loop (u, u) is two entries of u's row"""
    rows = [[] for _ in range(n)]
    for u, v in ei.T.tolist():
        rows[u].append(v)
        rows[v].append(u)
    return rows


def _sparse(rng, lo, hi, deg):
    """random columns among the vertices lo..hi-1, about `deg` entries per row, plus a ring that keeps them connected"""
    n = hi - lo
    ring = np.stack([np.arange(lo, hi), lo + (np.arange(n) + 1) % n])
    m = n * (deg - 2) // 2
    u, v = rng.integers(lo, hi, m), rng.integers(lo, hi, m)
    keep = u != v
    return np.concatenate([ring, np.stack([u[keep], v[keep]])], axis=1).astype(np.int64)


def _clique(n, lo=0):
    u, v = np.triu_indices(n, 1)
    return np.stack([u + lo, v + lo]).astype(np.int64)


def _product(ei, ptr, m, k, mode, seed):
    import ugs_sampler
    ugs_sampler.clear_cache()
    got = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode, seed)
    ugs_sampler.clear_cache()
    return [t.numpy() for t in got]


def _launch(ei, ptr, m, k, seed):
    """(tier the plan starts in, rows its first launch handed on)"""
    import ugs_sampler
    ugs_sampler.clear_cache()
    plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), k)
    plan.walk(m, "sample", seed)
    tier, handed_on = plan.info()["tier"], plan.last_launch()["overflow_rows"]
    plan.close()
    ugs_sampler.clear_cache()
    return tier, handed_on


def _check(ei, ptr, k, rows, monkeypatch, tier=TIER_M, seed=42, modes=MODES, want_handed_on=False):
    """the product in `tier` against the oracle; returns the oracle's "sample"-mode output"""
    ei = np.ascontiguousarray(ei)
    monkeypatch.setenv("UGS_FORCE_TIER", str(tier))
    m = rows // (len(ptr) - 1)
    first = None
    for mode in modes:
        want = oracle.sample_batch(ei, ptr, m, k, mode, seed)
        got = _product(ei, ptr, m, k, mode, seed)
        assert len(got) == len(want) == 5
        for name, a, b in zip(("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src"), got, want):
            assert a.shape == np.asarray(b).shape and np.array_equal(a, np.asarray(b)), f"{name} differs (mode {mode}, k {k}, tier {tier})"
        first = first or want
    got_tier, handed_on = _launch(ei, ptr, m, k, seed)
    assert got_tier == tier, (got_tier, tier)
    assert (handed_on > 0) == want_handed_on, handed_on
    return first


def _complete(want, k):
    nodes = np.asarray(want[0])
    return nodes[(nodes >= 0).all(axis=1)]


@pytest.mark.parametrize("k", [1, 3, 8])
def test_self_loops_of_the_last_vertex_and_of_earlier_members(k, monkeypatch):
    rng = np.random.default_rng(100 + k)
    n = 240
    once, twice = np.arange(0, n, 3), np.arange(1, n, 3)                   # the column (u, u) once: two entries of u's row; twice: four
    ei = np.concatenate([_sparse(rng, 0, n, 8), np.stack([once, once]), np.stack([twice, twice]), np.stack([twice, twice])], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    rows = _sym_rows(ei, n)
    assert all(rows[u].count(u) == 2 for u in once) and all(rows[u].count(u) == 4 for u in twice)
    want = _check(ei, np.array([0, n], dtype=np.int64), k, 2000, monkeypatch)
    nodes = _complete(want, k)
    last, earlier = nodes[:, k - 1], nodes[:, : k - 1]
    assert np.isin(last, once).any() and np.isin(last, twice).any() and (last % 3 == 2).any(), "last vertex: loop once, twice, none"
    if k > 1:
        both = np.isin(last, np.concatenate([once, twice])) & np.isin(earlier, np.concatenate([once, twice])).any(axis=1)
        assert both.any(), "a sample whose last vertex and an earlier member both carry a self loop"
    # a self entry counts once: the rows of a k = 1 sample hold exactly the root's own loop entries
    if k == 1:
        e = np.diff(np.asarray(want[2]))
        assert set(e[np.isin(last, once)]) == {2} and set(e[np.isin(last, twice)]) == {4} and set(e[last % 3 == 2]) == {0}


@pytest.mark.parametrize("k", [2, 3, 8])
def test_sampled_neighbour_repeated_in_the_last_row(k, monkeypatch):
    rng = np.random.default_rng(110 + k)
    n = 240
    base = _sparse(rng, 0, n, 8)
    both = base[:, ::3]                                                    # a third of the columns again, the other way round: twice in a row
    thrice = base[:, 1::3]                                                 # and a third three times
    ei = np.concatenate([base, both[::-1], thrice, thrice], axis=1)
    rows = _sym_rows(ei, n)
    want = _check(ei, np.array([0, n], dtype=np.int64), k, 2000, monkeypatch)
    nodes = _complete(want, k)
    mult = [max(rows[r[k - 1]].count(int(x)) for x in r[: k - 1]) for r in nodes]
    assert mult.count(2) > 20 and sum(x >= 3 for x in mult) > 20, "last rows holding an earlier member twice, and three times"
    # every entry appears: a sample that is a tree apart from its repeats has exactly as many items as its members' rows hold of each other
    e = np.diff(np.asarray(want[2]))[(np.asarray(want[0]) >= 0).all(axis=1)]
    inside = [sum(rows[int(a)].count(int(b)) for a in r for b in r) for r in nodes]
    assert np.array_equal(e, inside)


@pytest.mark.parametrize("shift", [4, 6])
@pytest.mark.parametrize("k", [3, 8])
def test_last_row_of_200_entries_with_hits_in_later_chunks(k, shift, monkeypatch):
    monkeypatch.setenv("UGS_PROW_SHIFT", str(shift))                       # entries per padded row: 2^shift, one of them the header
    rng = np.random.default_rng(120 + k + shift)
    n, hub, deg = 420, 0, 200
    nb = rng.choice(np.arange(1, n), size=deg, replace=False)
    ei = np.concatenate([np.stack([np.full(deg, hub), nb]), _sparse(rng, 1, n, 4)], axis=1).astype(np.int64)   # the hub's columns first: its row is `nb` in order
    rows = _sym_rows(ei, n)
    assert rows[hub] == nb.tolist()
    want = _check(ei, np.array([0, n], dtype=np.int64), k, 3000, monkeypatch)
    nodes = _complete(want, k)
    inl = (1 << shift) - 1
    pos = {int(v): i for i, v in enumerate(nb)}
    chunks = set()
    for r in nodes[nodes[:, k - 1] == hub]:
        chunks.update(0 if pos[int(x)] < inl else 1 + (pos[int(x)] - inl) // 64 for x in r[: k - 1] if int(x) in pos)
    assert {0, 1, 2} <= chunks, f"hits of a last hub row in its block and in its second and third chunk: {sorted(chunks)}"


@pytest.mark.parametrize("doubled", [False, True])
def test_clique_samples_hit_every_member(doubled, monkeypatch):
    k = 8
    ei = _clique(12)
    if doubled:
        ei = np.concatenate([ei, ei[::-1]], axis=1)                        # every pair twice: 56 hits per sample, the staging list holds 32
    want = _check(ei, np.array([0, 12], dtype=np.int64), k, 1000, monkeypatch)
    e = np.diff(np.asarray(want[2]))
    assert (e == (2 if doubled else 1) * k * (k - 1)).all()


@pytest.mark.parametrize("k,n", [(14, 16), (32, 36)])
def test_large_cliques(k, n, monkeypatch):
    want = _check(_clique(n), np.array([0, n], dtype=np.int64), k, 300, monkeypatch)
    assert (np.diff(np.asarray(want[2])) == k * (k - 1)).all()             # more hits than the staging list holds: the row-reading fill


@pytest.mark.parametrize("k", [1, 2, 3, 8, 14, 32])
def test_every_k(k, monkeypatch):
    rng = np.random.default_rng(130 + k)
    n = 300
    ei = _sparse(rng, 0, n, 10)
    want = _check(ei, np.array([0, n], dtype=np.int64), k, 1500, monkeypatch)
    e = np.diff(np.asarray(want[2]))
    assert len(_complete(want, k)) == 1500 and (e >= 2 * (k - 1)).all()
    if k > 2:
        assert (e > 2 * (k - 1)).any(), "samples with a cycle"


def _small_components(lo):
    """components of 2, 3, 5 and 7 vertices (paths, stars and cliques): no connected 8-subgraph, so the graph's roots come from the
    relaxed list and every walk stops early, after 1 to 6 picks (or none: the edgeless graph's)"""
    cols = []
    for i, size in enumerate([2, 3, 5, 7] * 3):
        if i % 3 == 0:
            cols.append(_clique(size, lo))
        elif i % 3 == 1:
            cols.append(np.stack([np.arange(size - 1) + lo, np.arange(1, size) + lo]))
        else:
            cols.append(np.stack([np.full(size - 1, lo), np.arange(1, size) + lo]))
        lo += size
    return np.concatenate(cols, axis=1).astype(np.int64), lo


def _mixed_batch(rng, k=8):
    """six graphs in turn: small components only (relaxed roots: every row partial), a graph whose walks all complete, ...; and
    an edgeless graph (the other relaxed level) at the end"""
    cols, ptr = [], [0]
    for g in range(6):
        if g % 2 == 0:
            ei, hi = _small_components(ptr[-1])
            pre = oracle.Preproc(ei - ptr[-1], hi - ptr[-1], k)
            d = pre.dump()
            pre.close()
            assert not (d["bucket_b"] > 0).any() and (d["suffix_deg"] > 0).any(), "roots drawn from the relaxed list (level 1)"
        else:
            hi = ptr[-1] + 150
            ei = np.concatenate([_sparse(rng, ptr[-1], hi, 8), np.stack([np.arange(ptr[-1], hi, 3)] * 2)], axis=1)
        cols.append(ei)
        ptr.append(hi)
    ptr.append(ptr[-1] + 9)                                                 # no column at all: level 2
    return np.concatenate(cols, axis=1), np.array(ptr, dtype=np.int64)


def _mixed_properties(want, m):
    full = (np.asarray(want[0]) >= 0).all(axis=1).reshape(7, m)
    assert not full[[0, 2, 4, 6]].any() and full[[1, 3, 5]].all(), "relaxed graphs: partial rows only; the others: complete rows only"
    sizes = (np.asarray(want[0]) >= 0).sum(axis=1).reshape(7, m)
    assert {2, 3, 5, 7} <= set(sizes[0].tolist()) and set(sizes[6].tolist()) == {1}
    assert (np.diff(np.asarray(want[2])).reshape(7, m)[[0, 2, 4, 6]] == 0).all()


def test_walks_that_stop_early_beside_complete_ones_relaxed_roots(monkeypatch):
    ei, ptr = _mixed_batch(np.random.default_rng(140))
    want = _check(ei, ptr, 8, 7 * 400, monkeypatch)
    _mixed_properties(want, 400)


def test_many_consecutive_walks_per_wave(monkeypatch):
    """many more rows than resident waves, complete walks and walks that stop early in turn: a wave's next walk meets the table, the
    candidate list and the sample list as the last pick of the previous one left them"""
    ei, ptr = _mixed_batch(np.random.default_rng(141))
    want = _check(ei, ptr, 8, 7 * 9000, monkeypatch, modes=("sample",))
    _mixed_properties(want, 9000)


@pytest.mark.parametrize("mode", MODES)
def test_one_seed_per_graph(mode, monkeypatch):
    import ugs_sampler
    from ugs_graphs_law import oracle_loop
    rng = np.random.default_rng(160)
    ei = np.ascontiguousarray(np.concatenate([_sparse(rng, 0, 200, 8), _clique(10, 200), _sparse(rng, 210, 330, 12)], axis=1))
    ptr = np.array([0, 200, 210, 330], dtype=np.int64)
    seeds, m, k = [42, -7, 123456789], 700, 8
    monkeypatch.setenv("UGS_FORCE_TIER", str(TIER_M))
    cache = oracle.Cache()
    want = oracle_loop(ei, ptr, m, k, mode, seeds, cache)
    cache.close()
    ugs_sampler.clear_cache()
    got = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, seeds, mode)
    ugs_sampler.clear_cache()
    for name, a, b in zip(("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src"), got, want):
        assert np.array_equal(a.numpy(), np.asarray(b)), (name, mode)


@pytest.mark.parametrize("tier", [1, 2, 3, 4, 5])
def test_every_tier_with_one_walk_per_wave(tier, monkeypatch):
    rng = np.random.default_rng(170)
    n = 300
    ei = np.concatenate([_sparse(rng, 0, n, 12), np.stack([np.arange(0, n, 4), np.arange(0, n, 4)])], axis=1)
    _check(ei, np.array([0, n], dtype=np.int64), 8, 2000, monkeypatch, tier=tier)


def test_rows_read_through_the_row_pointer(monkeypatch):
    monkeypatch.setenv("UGS_NO_PROW", "1")                                 # no padded rows: the last row comes in chunks of 64 from the CSR
    rng = np.random.default_rng(180)
    n, deg = 420, 200
    nb = rng.choice(np.arange(1, n), size=deg, replace=False)
    loops = np.stack([np.arange(0, n, 4), np.arange(0, n, 4)])
    ei = np.concatenate([np.stack([np.zeros(deg, dtype=np.int64), nb]), _sparse(rng, 1, n, 6), loops], axis=1).astype(np.int64)
    want = _check(ei, np.array([0, n], dtype=np.int64), 8, 3000, monkeypatch)
    assert (_complete(want, 8)[:, 7] == 0).sum() > 20, "the hub as the last vertex"


def test_walks_handed_on_from_the_448_candidate_tier(monkeypatch):
    rng = np.random.default_rng(190)
    n = 600
    hub = np.stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])     # vertex 0 is adjacent to all: its row alone outgrows the tier
    loops = np.stack([np.arange(0, n, 4), np.arange(0, n, 4)])
    ei = np.concatenate([_sparse(rng, 0, n, 6), hub, loops], axis=1)
    want = _check(ei, np.array([0, n], dtype=np.int64), 8, 3000, monkeypatch, want_handed_on=True)
    nodes = _complete(want, 8)
    assert (nodes[:, :7] == 0).any(axis=1).sum() > 100, "walks that scan the hub's row with candidates added: handed on"
    assert (nodes[:, 7] == 0).any(), "and walks that only end on the hub: they stay"
