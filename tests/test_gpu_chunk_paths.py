"""GPU: the adjacency-chunk paths of the one-walk-per-wave 448-candidate tier (scan_prow / scan_chunk), every output against the
CPU oracle.  Small graphs (200-600 vertices, 2000 rows) built so that a walk meets: a vertex repeated two and three times inside
one chunk (duplicate columns in both orientations), a self loop, chunks with no, one and several entries pointing into the sample,
rows of exactly inl - 1, inl, inl + 1, 64, 65 and 130 entries (block only, block + tail, several tail chunks; inl = entries a
padded row's block holds), a hub row whose walk outgrows the tier so that the guarded chunks hand it on (which is also the launch
from a list of rows), k = 2 (the first scanned row is the last one: no candidates added), 3 and 8, and a two-graph batch (the
instantiation that is not specialised for one graph).  Each case asserts on the CPU that the graph has the property it is named for.

The 448-candidate tier allows 448 candidates and 448 distinct vertices seen; a walk has seen at least one vertex more than it has
candidates, so of the two guards of a chunk the table's limit is always met first in this tier: one hub case drives both tests."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

ROWS = 2000
MODES = ("sample", "global")


def _sym_rows(ei, n):
    """row of every vertex in the symmetrised adjacency, as the sampler builds it: a column (u, v) is an entry of u's row and of v's;
    a self loop (u, u) is two entries of u's row"""
    rows = [[] for _ in range(n)]
    for u, v in ei.T.tolist():
        rows[u].append(v)
        rows[v].append(u)
    return rows


def _sparse(rng, lo, hi, deg):
    """random columns among the vertices lo..hi-1, about `deg` entries per row, plus a ring that keeps the graph connected"""
    n = hi - lo
    ring = np.stack([np.arange(lo, hi), lo + (np.arange(n) + 1) % n])
    m = n * (deg - 2) // 2
    u, v = rng.integers(lo, hi, m), rng.integers(lo, hi, m)
    keep = u != v
    return np.concatenate([ring, np.stack([u[keep], v[keep]])], axis=1).astype(np.int64)


def _rows_of_exact_length(rng, n, lengths):
    """vertex i < len(lengths) gets exactly lengths[i] entries: that many distinct ordinary vertices, no other column touches it"""
    s = len(lengths)
    cols = [_sparse(rng, s, n, 6)]
    for i, d in enumerate(lengths):
        nb = rng.choice(np.arange(s, n), size=d, replace=False)
        cols.append(np.stack([np.full(d, i), nb]).astype(np.int64))
    return np.concatenate(cols, axis=1)


def _check(ei, ptr, k, monkeypatch, seed=42, want_overflow=False):
    import ugs_sampler
    monkeypatch.setenv("UGS_FORCE_TIER", "1")            # the 448-candidate tier, one walk per wave
    m = ROWS // (len(ptr) - 1)
    outs = {}
    for mode in MODES:
        ugs_sampler.clear_cache()
        got = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode, seed)
        want = oracle.sample_batch(ei, ptr, m, k, mode, seed)
        assert len(got) == len(want) >= 4
        for j, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a.numpy(), np.asarray(b)), f"output {j} differs (mode {mode}, k {k})"
        outs[mode] = want
    if want_overflow:
        ugs_sampler.clear_cache()
        plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), k)
        plan.walk(m, "sample", seed)
        info, handed_on = plan.info(), plan.last_launch()["overflow_rows"]
        plan.close()
        assert info["tier"] == 1 and handed_on > 0, (info, handed_on)
    ugs_sampler.clear_cache()
    return outs["sample"]


def _edges_per_row(want):
    eptr = np.asarray(want[2])
    return np.diff(eptr)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_repeated_vertices_and_self_loops_in_a_chunk(k, monkeypatch):
    rng = np.random.default_rng(10 + k)
    n = 240
    base = _sparse(rng, 0, n, 8)
    both = base[:, ::3]                                                    # a third of the columns again, the other way round: twice in a row
    thrice = base[:, 1::7]                                                 # and some three times
    loops = np.stack([np.arange(0, n, 5), np.arange(0, n, 5)])             # self loops
    ei = np.ascontiguousarray(np.concatenate([base, both[::-1], thrice, thrice, loops], axis=1))
    rows = _sym_rows(ei, n)
    mult = [max(np.unique(r, return_counts=True)[1]) for r in rows]
    assert sum(x == 2 for x in mult) > 20 and sum(x >= 3 for x in mult) > 20, "rows with a vertex twice, and three times"
    assert max(len(r) for r in rows) <= 62, "every row is one chunk: its repeats meet inside it"
    assert all(rows[u].count(u) == 2 for u in range(0, n, 5)), "self loops"
    _check(ei, np.array([0, n], dtype=np.int64), k, monkeypatch)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_chunks_with_no_one_and_several_hits(k, monkeypatch):
    rng = np.random.default_rng(20 + k)
    n = 200
    ei = np.ascontiguousarray(_sparse(rng, 0, n, 24))                      # dense enough for cycles inside a sample of 8
    want = _check(ei, np.array([0, n], dtype=np.int64), k, monkeypatch)
    e = _edges_per_row(want)
    # every walk's root row has no entry pointing into the sample; a sample that is a tree (2 (k - 1) entries) has exactly one hit in the
    # row of each later vertex; a sample with more entries has a row with several
    assert (e == 2 * (k - 1)).any(), "tree samples: one hit per scanned row"
    if k > 2:
        assert (e > 2 * (k - 1)).any(), "samples with a cycle: a row with several hits"


@pytest.mark.parametrize("shift", [4, 6])
@pytest.mark.parametrize("k", [3, 8])
def test_rows_at_the_block_and_chunk_boundaries(k, shift, monkeypatch):
    monkeypatch.setenv("UGS_PROW_SHIFT", str(shift))                       # entries per padded row: 2^shift, one of them the header
    inl = (1 << shift) - 1
    lengths = [inl - 1, inl, inl + 1, 64, 65, 130]
    rng = np.random.default_rng(30 + k + shift)
    n = 320
    ei = np.ascontiguousarray(_rows_of_exact_length(rng, n, lengths))
    rows = _sym_rows(ei, n)
    assert [len(rows[i]) for i in range(len(lengths))] == lengths
    want = _check(ei, np.array([0, n], dtype=np.int64), k, monkeypatch)
    nodes = np.asarray(want[0])
    for i in range(len(lengths)):                                          # each of those rows is scanned: the vertex is sampled before the last place
        assert (nodes[:, : k - 1] == i).any(), f"vertex {i} (row of {lengths[i]} entries) is never scanned with candidates added"


@pytest.mark.parametrize("k", [3, 8])
def test_hub_row_hands_the_walk_on(k, monkeypatch):
    rng = np.random.default_rng(40 + k)
    n = 600
    hub = np.stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])     # vertex 0 is adjacent to all: 599 entries, nine tail chunks
    ei = np.ascontiguousarray(np.concatenate([_sparse(rng, 0, n, 6), hub], axis=1))
    rows = _sym_rows(ei, n)
    assert len(set(rows[0])) == n - 1 and n - 1 > 448, "the hub's row alone holds more vertices than the tier's table admits"
    _check(ei, np.array([0, n], dtype=np.int64), k, monkeypatch, want_overflow=True)


@pytest.mark.parametrize("k", [2, 8])
def test_two_graph_batch(k, monkeypatch):
    rng = np.random.default_rng(50 + k)
    n0, n1 = 210, 330
    g0 = _rows_of_exact_length(rng, n0, [62, 63, 64, 130])
    g1 = _sparse(rng, 0, n1, 10) + n0
    dup = g1[:, ::4]
    ei = np.ascontiguousarray(np.concatenate([g0, g1, dup[::-1]], axis=1))
    ptr = np.array([0, n0, n0 + n1], dtype=np.int64)
    assert len(ptr) - 1 == 2
    _check(ei, ptr, k, monkeypatch)
