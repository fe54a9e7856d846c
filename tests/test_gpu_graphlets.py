"""ugs_sampler.graphlets on the GPU (ugs_graphlet.hip) against the brute-force law of tests/graphlet_law.py: keys, statuses and
class ids, never against the kernel's own search.  Ids are the rank of the LAW's key: in the law's own table of all keys for
k <= 6, and for k = 7 and 8 (2^21 and 2^28 codes: no brute-force table) in the host table, whose content tests/test_graphlet_law.py
pins by the published class counts and whose entry at that rank must be the law's key."""
import random
from collections import Counter

import numpy as np
import pytest
import torch

import graphlet_law as law

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_tables = {}


def key_table(k):
    """The ascending keys for n <= k the ids are ranks in (see the module docstring)."""
    if k not in _tables:
        if k <= 6:
            _tables[k] = law.all_keys(k)
        else:
            from ugs_sampler import graphlets
            _tables[k] = graphlets.table(k).tolist()
            assert len(_tables[k]) == law.NUM_CLASSES[k - 1] and _tables[k][:208] == key_table(6)
    return _tables[k]


def pack(entries, k):
    """(nodes [S, k], edge_index [2, E], edge_ptr [S+1]) as int64 arrays from a list of (n, [(u, v), ...]): n valid ids first."""
    nodes = np.full((len(entries), k), -1, np.int64)
    cols, ptr = [], [0]
    for r, (n, es) in enumerate(entries):
        nodes[r, :n] = 100 + np.arange(n)
        cols += list(es)
        ptr.append(len(cols))
    ei = np.array(cols, np.int64).reshape(-1, 2).T if cols else np.zeros((2, 0), np.int64)
    return nodes, np.ascontiguousarray(ei), np.array(ptr, np.int64)


def random_entry(rng, n):
    """Edges on vertices 0..n-1 of mixed density with reversed copies, duplicates and loops."""
    p = rng.choice([0.0, 0.15, 0.4, 0.7, 1.0])
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    es += [(v, u) for u, v in es if rng.random() < 0.6]
    es += [rng.choice(es) for _ in range(rng.randrange(3))] if es else []
    es += [(u, u) for u in range(n) if rng.random() < 0.1]
    rng.shuffle(es)
    return n, es


def mixed_rows(rng, k, rows=40):
    entries = [(0, []), (k, []), (rng.randrange(1, k + 1), [])]                 # all -1, no edges at full and at partial width
    while len(entries) < rows:
        n = k if rng.random() < 0.6 else rng.randrange(1, k + 1)               # rows whose valid entries are fewer than k
        entries.append(random_entry(rng, n))
    rng.shuffle(entries)
    return entries


def rows_of_codes(codes, n, k, rng=None):
    """Rows for the graphs with adjacency codes `codes` on n vertices, built with numpy.  With rng every row is relabelled by a random
    permutation, its entries get random orientations and a random order; without, the identity order.  Returns the arrays and the
    code each row then has."""
    codes = np.asarray(codes, np.int64)
    R = len(codes)
    pr = np.array(law.pairs(n), np.int64).reshape(-1, 2)
    P = len(pr)
    bits = (codes[:, None] >> (pr[:, 1] * (pr[:, 1] - 1) // 2 + pr[:, 0])[None, :]) & 1
    u, v = np.broadcast_to(pr[:, 0], (R, P)), np.broadcast_to(pr[:, 1], (R, P))
    if rng is not None:
        perm = np.argsort(rng.random((R, n)), axis=1)
        u, v = perm[:, pr[:, 0]], perm[:, pr[:, 1]]
        flip = rng.random((R, P)) < 0.5
        u, v = np.where(flip, v, u), np.where(flip, u, v)
        order = np.argsort(rng.random((R, P)), axis=1)
        u, v, bits = (np.take_along_axis(a, order, 1) for a in (u, v, bits))
    m = bits.astype(bool)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    now = ((np.int64(1) << (hi * (hi - 1) // 2 + lo)) * m).sum(axis=1) if P else np.zeros(R, np.int64)
    nodes = np.full((R, k), -1, np.int64)
    nodes[:, :n] = 100 + np.arange(n)
    return (nodes, np.stack([u[m], v[m]]).astype(np.int64), np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)), now


def on_gpu(arrays, strided=False):
    nodes, ei, ep = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)
    if strided:                                                                 # rows 0 and 2 of a [3, E + 5] buffer: row stride 2 E + 10
        buf = torch.full((3, ei.size(1) + 5), -7, dtype=torch.int64, device=DEV)
        buf[0, :ei.size(1)], buf[2, :ei.size(1)] = ei[0], ei[1]
        ei = buf[::2, :ei.size(1)]
        assert not ei.is_contiguous() or ei.size(1) == 0
    return nodes, ei, ep


def assert_keys(arrays, want_keys, want_stats, what, strided=False):
    """canonical and class_ids of the rows on the GPU against the given keys and statuses."""
    from ugs_sampler import graphlets
    args = on_gpu(arrays, strided)
    k = args[0].size(1)
    key, status = graphlets.canonical(*args)
    assert key.is_cuda and key.dtype == torch.int64 and tuple(key.shape) == (len(want_keys),)
    assert status.is_cuda and status.dtype == torch.int32 and tuple(status.shape) == (len(want_keys),)
    assert status.cpu().tolist() == list(want_stats), what
    got = key.cpu().tolist()
    bad = [r for r, (a, b) in enumerate(zip(got, want_keys)) if a != b]
    assert not bad, (what, bad[:5], [got[r] for r in bad[:3]], [want_keys[r] for r in bad[:3]])
    ids = graphlets.class_ids(*args)
    assert ids.is_cuda and ids.dtype == torch.int64
    table = key_table(k)
    got_ids = ids.cpu().tolist()
    assert got_ids == law.ids_from(want_keys, want_stats, table), what
    assert all(table[i] == key for i, key, st in zip(got_ids, want_keys, want_stats) if st == 0), what
    return got_ids


def assert_law(arrays, what, strided=False, num_cols=None):
    keys, stats = law.rows_law(*arrays, num_cols=num_cols)
    assert_keys(arrays, keys, stats, what, strided)
    return keys, stats


@pytest.mark.parametrize("k", range(1, 9))
def test_every_k(k):
    rng = random.Random(2000 + k)
    entries = mixed_rows(rng, k)
    keys, stats = assert_law(pack(entries, k), f"k={k}")
    assert_law(pack(entries, k), f"k={k} strided", strided=True)
    assert 0 in stats and 1 in stats and (k == 1 or len(set(keys)) > 2)


@pytest.mark.parametrize("rows", [1, 63, 257])
def test_launch_shapes(rows):
    rng = random.Random(rows)
    entries = mixed_rows(rng, 6, rows=max(rows, 3))[:rows]                       # 257 rows end one row into a second workgroup
    assert_law(pack(entries, 6), f"rows={rows}")
    assert_law(pack(entries, 6), f"rows={rows} strided", strided=True)


def test_statuses_do_not_disturb_neighbouring_rows():
    from ugs_sampler import graphlets
    rng = random.Random(3)
    good = [random_entry(rng, 5) for _ in range(6)]
    entries = [good[0], (3, [(0, 1), (1, 3)]), good[1], (5, [(0, 1), (-1, 2)]), good[2], (0, []), good[3],
               (2, [(0, 1), (2, 2)]), (1, [(0, 0), (0, 5)]), good[4], (4, [(0, 1), (1, 0), (10 ** 12, 1)]), good[5]]
    arrays = pack(entries, 5)
    keys, stats = assert_law(arrays, "statuses")
    assert stats == [0, 2, 0, 2, 0, 1, 0, 2, 2, 0, 2, 0]
    alone, _ = law.rows_law(*pack(good, 5))
    assert [k for k in keys if k >= 0] == alone
    ids = graphlets.class_ids(*on_gpu(arrays)).cpu().tolist()
    assert [i for i, s in zip(ids, stats) if s] == [graphlets.num_classes(5)] * 6

    # edge_ptr ranges that are no ranges of the columns: a decreasing pair, a negative start, an end past the columns
    entries = [random_entry(rng, 6) for _ in range(6)] + [(0, [])]
    nodes, ei, ep = pack(entries, 6)
    ep = ep.copy()
    ep[2] = -1                                                                   # rows 1 and 2 lose their ranges, rows 0 and 3 keep theirs
    ep[6] += 3                                                                   # row 5 ends past the columns; row 6 has no vertices: status 1
    ep[7] = ep[6]
    keys, stats = assert_law((nodes, ei, ep), "edge_ptr ranges")
    assert stats == [0, 2, 2, 0, 0, 2, 1]
    whole, _ = law.rows_law(*pack(entries, 6))
    assert [keys[r] for r in (0, 3, 4)] == [whole[r] for r in (0, 3, 4)]


def test_endpoints_that_only_a_32_bit_cast_would_put_in_range():
    """2^32, 2^32 + 1 and -2^32 read as 0, 1 and 0 once narrowed to 32 bits, and 2^63 - 1 as -1: a kernel that narrows an endpoint
    before it checks it would take three of these rows for good ones.  The law compares the 64-bit value: status 2, key -1, and
    the rows between keep their keys."""
    rng = random.Random(32)
    good = [random_entry(rng, 5) for _ in range(5)]
    wide = [1 << 32, (1 << 32) + 1, -(1 << 32), (1 << 63) - 1]
    bad = [(5, [(0, 1), (x, 2), (3, 4)]) if r % 2 == 0 else (5, [(1, 2), (4, x)]) for r, x in enumerate(wide)]
    entries = [good[0], bad[0], good[1], bad[1], good[2], bad[2], good[3], bad[3], good[4]]
    arrays = pack(entries, 5)
    assert sorted(int(x) for x in arrays[1].ravel() if not 0 <= x < 5) == sorted(wide)
    assert [int(np.int64(x).astype(np.int32)) for x in wide] == [0, 1, 0, -1]
    keys, stats = assert_law(arrays, "wide endpoints")
    assert_law(arrays, "wide endpoints, strided", strided=True)
    assert stats == [0, 2, 0, 2, 0, 2, 0, 2, 0] and [keys[r] for r in (1, 3, 5, 7)] == [-1] * 4
    alone, _ = law.rows_law(*pack(good, 5))
    assert [k for k in keys if k >= 0] == alone


def test_no_rows_and_no_edge_entries():
    from ugs_sampler import graphlets
    nodes, ei, ep = on_gpu(pack([(6, [])], 6))
    key, status = graphlets.canonical(nodes[:0], ei, ep[:1])
    assert tuple(key.shape) == (0,) and tuple(status.shape) == (0,) and tuple(graphlets.class_ids(nodes[:0], ei, ep[:1]).shape) == (0,)
    entries = [(6, []), (0, []), (3, []), (1, [])]
    keys, stats = assert_law(pack(entries, 6), "no edge entries at all")
    assert keys == [6 << 28, -1, 3 << 28, 1 << 28] and stats == [0, 1, 0, 0]
    with pytest.raises(RuntimeError, match="k <= 8"):
        graphlets.canonical(*on_gpu(pack([(9, [(0, 8)])], 9)))
    with pytest.raises(RuntimeError, match="k <= 8"):
        graphlets.class_ids(*on_gpu(pack([(9, [(0, 8)])], 9)))
    with pytest.raises(ValueError):
        graphlets.canonical(nodes, ei.cpu(), ep)
    assert_law(pack(entries, 6), "after the refusals")


def test_all_codes_of_six_vertices():
    """All 32 768 graphs on 6 labelled vertices as rows: every key is the law's, and the keys are exactly table(6)'s n = 6 part."""
    codes = np.arange(1 << 15)
    arrays, now = rows_of_codes(codes, 6, 6)
    assert np.array_equal(now, codes)
    want = ((6 << 28) | law.canonical_codes(codes, 6)).tolist()
    assert_keys(arrays, want, [0] * len(want), "all codes of n = 6")
    assert sorted(set(want)) == [k for k in key_table(6) if k >> 28 == 6]


@pytest.mark.parametrize("n", [7, 8])
def test_every_class_under_relabelling(n):
    """Every representative of the table under two random relabellings with shuffled entries: each row returns its own key.  What a
    pruning rule that is wrong for one symmetric class cannot pass.  Fifty of the rows are put to the brute-force law as well."""
    reps = np.array([k for k in key_table(n) if k >> 28 == n], np.int64)
    assert len(reps) == law.GRAPHS_ON[n - 1]
    rng = np.random.default_rng(n)
    codes = np.concatenate([reps, reps]) & ((1 << 28) - 1)
    arrays, now = rows_of_codes(codes, n, n, rng)
    assert (now != codes).sum() > len(codes) // 2
    want = np.concatenate([reps, reps]).tolist()
    for r in rng.choice(len(codes), 50, replace=False):
        assert law.key_of(int(now[r]), n) == want[r]
    assert_keys(arrays, want, [0] * len(want), f"every class of n = {n}")


def symmetric_graphs():
    c8 = [(i, (i + 1) % 8) for i in range(8)]
    allp = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    return {"K8": allp, "C8": c8, "cube": [(a, a ^ d) for a in range(8) for d in (1, 2, 4) if a < a ^ d],
            "K4,4": [(i, 4 + j) for i in range(4) for j in range(4)],
            "complement of C8": [p for p in allp if p not in c8 and p[::-1] not in c8],
            "2 x K4": [(i, j) for i, j in allp if (i < 4) == (j < 4)],
            "2 x C4": [(i, (i + 1) % 4) for i in range(4)] + [(4 + i, 4 + (i + 1) % 4) for i in range(4)], "empty": []}


def test_symmetric_graphs():
    """The graphs with the most ties: ten relabellings of each, a launch of 256 rows that are all C8 (every lane of four waves in
    the long search) and one with a single C8 among 255 paths (one long lane in a wave of short ones)."""
    rng = np.random.default_rng(8)
    graphs = symmetric_graphs()
    codes = [law.code_of_edges(8, es) for es in graphs.values()]
    arrays, now = rows_of_codes(np.repeat(codes, 10), 8, 8, rng)
    want = [law.key_of(int(c), 8) for c in now]
    assert want == [law.key_of(c, 8) for c in codes for _ in range(10)] and len(set(want)) == 8
    assert_keys(arrays, want, [0] * 80, "symmetric graphs")

    c8, p8 = law.code_of_edges(8, graphs["C8"]), law.code_of_edges(8, graphs["C8"][:-1])
    arrays, _ = rows_of_codes([c8] * 256, 8, 8, rng)
    assert_keys(arrays, [law.key_of(c8, 8)] * 256, [0] * 256, "256 x C8")
    mix = [p8] * 256
    mix[101] = c8
    arrays, _ = rows_of_codes(mix, 8, 8, rng)
    assert_keys(arrays, [law.key_of(c, 8) for c in mix], [0] * 256, "one C8 among paths")


def test_sampler_rows_histogram_and_cpu_tensors():
    import ugs_sampler
    import ugs_workloads as workloads
    from ugs_sampler import graphlets
    ei, ptr = workloads.tu_batch(18, 20, 16)
    out = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 100, 6, mode="sample", seed=11, device=DEV)
    nodes, eidx, eptr, sptr = out[:4]
    assert nodes.shape == (1600, 6)
    keys, stats = law.rows_law(nodes.cpu().numpy(), eidx.cpu().numpy(), eptr.cpu().numpy())
    want = law.ids_from(keys, stats, key_table(6))
    ids = graphlets.class_ids(nodes, eidx, eptr)
    assert ids.is_cuda and ids.cpu().tolist() == want and max(want) < graphlets.num_classes(6) and len(set(want)) > 5
    key, status = graphlets.canonical(nodes, eidx, eptr)
    assert key.cpu().tolist() == keys and status.cpu().tolist() == stats
    full = (nodes >= 0).sum(dim=1) == 6
    assert full.any() and graphlets.is_connected(key)[full].all()               # a sampled 6-subgraph is connected
    assert graphlets.is_connected(key).cpu().tolist() == [law.connected(k & ((1 << 28) - 1), k >> 28) for k in keys]

    hist = graphlets.histogram(ids, sptr, 6)
    assert hist.is_cuda and tuple(hist.shape) == (16, graphlets.num_classes(6))
    bounds = sptr.cpu().tolist()
    for g in range(16):
        count = Counter(want[bounds[g]:bounds[g + 1]])
        assert hist[g].cpu().tolist() == [count.get(c, 0) for c in range(graphlets.num_classes(6))], g

    host_ids = graphlets.class_ids(nodes.cpu(), eidx.cpu(), eptr.cpu())          # CPU tensors in, CPU tensors out
    assert not host_ids.is_cuda and host_ids.tolist() == want
    hk, hs = graphlets.canonical(nodes.cpu(), eidx.cpu(), eptr.cpu())
    assert not hk.is_cuda and not hs.is_cuda and hk.tolist() == keys and hs.tolist() == stats
