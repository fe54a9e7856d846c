"""graphlets.orbit_ids on the GPU (ugs_graphlet_orbits_kernel) against the brute-force law of tests/graphlet_orbit_law.py, never
against the kernel's own search.  For k <= 6 every expected id comes from the brute force: rooted codes over all n! permutations,
the law's own key table and the law's own orbit counts.  For n = 7 and 8 the mixed rows are brute-forced too; the exhaustive runs take
the rooted codes of a class's representative from ugs_graphlet_rooted_codes, which tests/test_graphlet_orbit_law.py pins against the
brute force and the automorphism groups, and carry them to a relabelled row by equivariance: the vertex renamed perm[v] has v's
orbit.  The key table and orbit_base for k = 7, 8 are the host's, pinned there by the Burnside counts."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

import graphlet_law as law
import graphlet_orbit_law as olaw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MASK = (1 << 28) - 1
_tables = {}


def tables(k):
    """(ascending keys for n <= k, base with k's orbit count as its last entry): the law's own for k <= 6, the host's above."""
    if k not in _tables:
        if k <= 6:
            keys = law.all_keys(k)
            base = [0] + np.cumsum(olaw.orbit_counts(keys)).tolist()
        else:
            from ugs_sampler import graphlets
            keys, base = graphlets.table(k).tolist(), graphlets.orbit_base(k).tolist()
            k6, b6 = tables(6)
            assert keys[:208] == k6 and base[:209] == b6
        assert len(base) == len(keys) + 1 == law.NUM_CLASSES[k - 1] + 1
        _tables[k] = (keys, base)
    return _tables[k]


def pack(entries, k):
    """(nodes [S, k], edge_index [2, E], edge_ptr [S+1]) from a list of (node entries of length k, [(u, v), ...])."""
    nodes = np.array([e[0] for e in entries], np.int64).reshape(len(entries), k)
    cols, ptr = [], [0]
    for _, es in entries:
        cols += list(es)
        ptr.append(len(cols))
    ei = np.array(cols, np.int64).reshape(-1, 2).T if cols else np.zeros((2, 0), np.int64)
    return nodes, np.ascontiguousarray(ei), np.array(ptr, np.int64)


def random_entry(rng, n, k, bad=False):
    """A row with n vertices in k slots: entries of -1 anywhere, the middle included, ids that repeat; edges of mixed density
    with reversed copies, duplicates and loops; with `bad`, one endpoint outside the row's vertices."""
    slots = sorted(rng.sample(range(k), n))
    ids = [rng.choice([3, 5, 5, 40, 10 ** 12]) for _ in range(n)]               # a repeated id is two vertices
    row = [-1] * k
    for s, x in zip(slots, ids):
        row[s] = x
    p = rng.choice([0.0, 0.15, 0.4, 0.7, 1.0])
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    es += [(v, u) for u, v in es if rng.random() < 0.6]
    es += [rng.choice(es) for _ in range(rng.randrange(3))] if es else []
    es += [(u, u) for u in range(n) if rng.random() < 0.1]
    if bad:
        es.append(rng.choice([(0, n), (-1, 0), (n + 3, n + 3)]))
    rng.shuffle(es)
    return row, es


def mixed_rows(rng, k, rows=40):
    entries = [random_entry(rng, 0, k), random_entry(rng, k, k), random_entry(rng, rng.randrange(1, k + 1), k, bad=True)]
    if k >= 3:                                                                   # the slot rule: -1 in the middle, vertices around it
        row, es = random_entry(rng, k - 1, k - 1)
        entries.append((row[:1] + [-1] + row[1:], es + [(0, k - 2), (k - 2, 1)]))
    while len(entries) < rows:
        n = k if rng.random() < 0.5 else rng.randrange(1, k + 1)                 # rows whose valid entries are fewer than k
        entries.append(random_entry(rng, n, k, bad=rng.random() < 0.08))
    rng.shuffle(entries)
    return entries[:rows]


def on_gpu(arrays, strided=False):
    nodes, ei, ep = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)
    if strided:                                                                 # rows 0 and 2 of a [3, E + 5] buffer: row stride 2 E + 10
        buf = torch.full((3, ei.size(1) + 5), -7, dtype=torch.int64, device=DEV)
        buf[0, :ei.size(1)], buf[2, :ei.size(1)] = ei[0], ei[1]
        ei = buf[::2, :ei.size(1)]
        assert not ei.is_contiguous() or ei.size(1) == 0
    return nodes, ei, ep


def assert_orbits(arrays, want, what, strided=False, want_ids=None):
    """orbit_ids of the rows on the GPU against the given [S][k] ids, with and without return_class."""
    from ugs_sampler import graphlets
    args = on_gpu(arrays, strided)
    S, k = args[0].shape
    got = graphlets.orbit_ids(*args)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (S, k), what
    got = got.cpu().tolist()
    bad = [r for r in range(S) if got[r] != list(want[r])]
    assert not bad, (what, bad[:5], [got[r] for r in bad[:3]], [list(want[r]) for r in bad[:3]])
    both = graphlets.orbit_ids(*args, return_class=True)
    assert isinstance(both, tuple) and len(both) == 2 and both[0].cpu().tolist() == got, what
    assert both[1].is_cuda and both[1].dtype == torch.int64 and tuple(both[1].shape) == (S,), what
    if want_ids is not None:
        assert both[1].cpu().tolist() == list(want_ids), what
    return got


def assert_law(arrays, what, strided=False, num_cols=None):
    k = arrays[0].shape[1]
    keys, stats, local = olaw.rows_law(*arrays, num_cols=num_cols)
    table, base = tables(k)
    want = olaw.orbit_ids_from(keys, stats, local, table, base)
    got = assert_orbits(arrays, want, what, strided, law.ids_from(keys, stats, table))
    fill = base[-1]
    assert all((x == fill) == (int(e) < 0 or st != 0) for row, ent, st in zip(got, arrays[0], stats) for x, e in zip(row, ent)), what
    return keys, stats, want


@pytest.mark.parametrize("k", range(1, 9))
def test_every_k(k):
    from ugs_sampler import graphlets
    rng = random.Random(3000 + k)
    entries = mixed_rows(rng, k)
    nodes, ei, ep = pack(entries, k)
    keys, stats, want = assert_law((nodes, ei, ep), f"k={k}")
    assert_law((nodes, ei, ep), f"k={k} strided", strided=True)
    assert 0 in stats and 1 in stats and 2 in stats
    assert max(max(row) for row in want) == graphlets.num_orbits(k) and (k == 1 or len({x for row in want for x in row}) > 3)
    # an edge_ptr range that is no range of the columns: rows 10 and 11 lose theirs, the rows around them keep their ids
    ep2 = ep.copy()
    ep2[11] = -1
    keys2, stats2, want2 = assert_law((nodes, ei, ep2), f"k={k} bad range")
    assert all(s == 2 or not (nodes[r] >= 0).any() for r, s in zip((10, 11), stats2[10:12]))
    assert want2[:10] == want[:10] and want2[12:] == want[12:]
    ep3 = ep.copy()
    ep3[-1] += 2                                                                 # the last row ends past the columns
    assert_law((nodes, ei, ep3), f"k={k} range past the columns")


@pytest.mark.parametrize("k", [6, 8])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 257])
def test_launch_shapes(rows, k):
    """One row (seven groups of its wave missing); a workgroup of 32 rows one short, full and one over; 257 rows."""
    rng = random.Random(100 * k + rows)
    pool = mixed_rows(rng, k, rows=12)                                           # few graphs, so that the brute force stays short
    entries = [pool[rng.randrange(12)] for _ in range(rows)]
    assert_law(pack(entries, k), f"rows={rows}")
    assert_law(pack(entries, k), f"rows={rows} strided", strided=True)


def test_slot_rule_and_repeated_ids():
    """The paw on slots 0, 2, 3, 5 of six: the ids are those of vertices 0 .. 3 in row order whatever stands in the slots."""
    paw = [(0, 1), (1, 2), (2, 0), (2, 3)]                                       # triangle 0 1 2, tail 3 at 2
    rows = [([7, -1, 7, 9, -1, 7], paw), ([7, 7, 9, 7, -1, -1], paw), ([-1, -1, 1, 2, 3, 4], paw)]
    keys, stats, want = assert_law(pack(rows, 6), "slot rule")
    assert stats == [0, 0, 0] and len(set(keys)) == 1
    a, b, c = sorted({x for x in want[1][:4]})                                   # tail (degree 1), corners (2), the corner with the tail (3)
    fill = tables(6)[1][-1]
    assert want == [[b, fill, b, c, fill, a], [b, b, c, a, fill, fill], [fill, fill, b, b, c, a]]


def test_all_codes_of_six_vertices():
    """All 32 768 graphs on 6 labelled vertices as rows, in the identity order."""
    codes = np.arange(1 << 15)
    pr = law.pairs(6)
    cols = [[(i, j) for i, j in pr if c >> law.bit(i, j) & 1] for c in codes.tolist()]
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    ei = np.array([e for c in cols for e in c], np.int64).T
    nodes = np.broadcast_to(np.arange(6, dtype=np.int64) + 50, (len(codes), 6)).copy()
    rooted = olaw.rooted_codes_many(codes, 6)
    table, base = tables(6)
    rank = np.searchsorted(np.array(table), (6 << 28) | rooted.min(axis=1))
    assert np.array_equal(np.array(table)[rank], (6 << 28) | law.canonical_codes(codes, 6))
    want = np.array(base)[rank][:, None] + olaw.local_indices_many(rooted)
    for c in (0, 1, 12345, 32767):                                               # the vectorised law is the row-by-row law
        idx = olaw.local_indices(olaw.rooted_codes(c, 6))
        assert want[c].tolist() == [base[rank[c]] + x for x in idx]
    assert_orbits((nodes, np.ascontiguousarray(ei), ptr), want.tolist(), "all codes of n = 6", want_ids=rank.tolist())


def host_rooted(code, n):
    from ugs_sampler._lib import lib
    out = (C.c_uint32 * 8)()
    assert lib.ugs_graphlet_rooted_codes(int(code), n, out) == 0
    return list(out)[:n]


def relabelled_rows(codes, n, rng):
    """Rows for the graphs with adjacency codes `codes` on n vertices, every one relabelled by a random permutation (vertex v is
    renamed perm[v]), its entries in random orientations and order.  Returns the arrays and perm [R, n]."""
    codes = np.asarray(codes, np.int64)
    R = len(codes)
    pr = np.array(law.pairs(n), np.int64).reshape(-1, 2)
    bits = ((codes[:, None] >> (pr[:, 1] * (pr[:, 1] - 1) // 2 + pr[:, 0])[None, :]) & 1).astype(bool)
    perm = np.argsort(rng.random((R, n)), axis=1)
    u, v = perm[:, pr[:, 0]], perm[:, pr[:, 1]]
    flip = rng.random(u.shape) < 0.5
    u, v = np.where(flip, v, u), np.where(flip, u, v)
    order = np.argsort(rng.random(u.shape), axis=1)
    u, v, bits = (np.take_along_axis(a, order, 1) for a in (u, v, bits))
    nodes = np.broadcast_to(100 + np.arange(n, dtype=np.int64), (R, n)).copy()
    ptr = np.concatenate([[0], np.cumsum(bits.sum(axis=1))]).astype(np.int64)
    return (nodes, np.stack([u[bits], v[bits]]).astype(np.int64), ptr), perm


def want_by_equivariance(codes, class_ids, n, perm, base):
    """The orbit ids of relabelled_rows: slot perm[v] of row r has the id of vertex v of codes[r]."""
    rooted = {}
    for c in set(int(c) for c in codes):
        rooted[c] = host_rooted(c, n)
    local = olaw.local_indices_many(np.array([rooted[int(c)] for c in codes]))
    want = np.zeros_like(local)
    np.put_along_axis(want, perm, np.array(base)[np.asarray(class_ids)][:, None] + local, axis=1)
    return want


@pytest.mark.parametrize("n", [7, 8])
def test_every_class_under_relabelling(n):
    """Every class of n vertices under two random relabellings with shuffled, randomly oriented entries: the test that a pruning or
    twin rule that is wrong for one symmetric class cannot pass.  Thirty of the rows are put to the brute-force law as well."""
    table, base = tables(n)
    first = law.NUM_CLASSES[n - 2]
    cids = np.concatenate([np.arange(first, len(table))] * 2)
    assert len(cids) == 2 * law.GRAPHS_ON[n - 1]
    codes = np.array(table)[cids] & MASK
    rng = np.random.default_rng(50 + n)
    arrays, perm = relabelled_rows(codes, n, rng)
    want = want_by_equivariance(codes, cids, n, perm, base)
    for r in rng.choice(len(codes), 30, replace=False):
        lo, hi = arrays[2][r], arrays[2][r + 1]
        now = law.code_of_edges(n, zip(arrays[1][0][lo:hi].tolist(), arrays[1][1][lo:hi].tolist()))
        assert law.key_of(now, n) == table[cids[r]]
        assert want[r].tolist() == [base[cids[r]] + x for x in olaw.local_indices(olaw.rooted_codes(now, n))]
    assert_orbits(arrays, want.tolist(), f"every class of n = {n}", want_ids=cids.tolist())


def symmetric_graphs():
    c8 = [(i, (i + 1) % 8) for i in range(8)]
    allp = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    cube = [(a, a ^ d) for a in range(8) for d in (1, 2, 4) if a < a ^ d]
    star, path = [(0, i) for i in range(1, 8)], [(i, i + 1) for i in range(7)]

    def co(es):
        return [p for p in allp if p not in es and p[::-1] not in es]
    return {"K8": allp, "empty": [], "C8": c8, "complement of C8": co(c8), "cube": cube, "complement of the cube": co(cube),
            "K1,7": star, "P8": path}


def test_symmetric_graphs():
    """K8, C8, the cube and their complements are one orbit each; K1,7 is centre and leaves; the path P8 has four orbits, symmetric
    about its middle.  Identity order first, then five relabellings of each against the brute force."""
    from ugs_sampler import graphlets
    graphs = symmetric_graphs()
    codes = [law.code_of_edges(8, es) for es in graphs.values()]
    ident = [(list(range(8)), es) for es in graphs.values()]
    got = graphlets.orbit_ids(*on_gpu(pack(ident, 8))).cpu().tolist()
    rows = dict(zip(graphs, got))
    for name in list(graphs)[:6]:
        assert len(set(rows[name])) == 1, name
    assert len({rows[name][0] for name in list(graphs)[:6]}) == 6
    star, path = rows["K1,7"], rows["P8"]
    assert len(set(star)) == 2 and len(set(star[1:])) == 1 and star[0] == max(star)          # leaves (degree 1) before the centre
    assert len(set(path)) == 4 and path == path[::-1] and path[0] == min(path)
    assert_law(pack(ident, 8), "symmetric graphs, identity order")

    rng = np.random.default_rng(8)
    table, base = tables(8)
    cids = [table.index(law.key_of(c, 8)) for c in codes for _ in range(5)]
    arrays, _ = relabelled_rows(np.repeat(codes, 5), 8, rng)
    want = np.zeros((40, 8), np.int64)
    for r in range(40):                                                          # brute force on the row's own code
        lo, hi = arrays[2][r], arrays[2][r + 1]
        now = law.code_of_edges(8, zip(arrays[1][0][lo:hi].tolist(), arrays[1][1][lo:hi].tolist()))
        want[r] = [base[cids[r]] + x for x in olaw.local_indices(olaw.rooted_codes(now, 8))]
    assert_orbits(arrays, want.tolist(), "symmetric graphs relabelled", want_ids=cids)


def test_cubes_in_one_launch_and_one_cube_among_paths():
    """256 rows that are all cubes (every lane of four waves in the long search) and one cube among 255 paths (eight long lanes in
    a wave of short ones)."""
    graphs = symmetric_graphs()
    cube, p8 = law.code_of_edges(8, graphs["cube"]), law.code_of_edges(8, graphs["P8"])
    table, base = tables(8)
    rng = np.random.default_rng(81)
    for what, codes in (("256 x cube", [cube] * 256), ("one cube among paths", [p8] * 101 + [cube] + [p8] * 154)):
        cids = [table.index(law.key_of(c, 8)) for c in codes]
        arrays, perm = relabelled_rows(codes, 8, rng)
        want = want_by_equivariance(codes, cids, 8, perm, base)
        assert_orbits(arrays, want.tolist(), what, want_ids=cids)
        assert all(len(set(row)) == (1 if c == cube else 4) for row, c in zip(want.tolist(), codes))


def test_return_class_is_class_ids_and_leaves_them_alone():
    from ugs_sampler import graphlets
    rng = random.Random(77)
    for k in (3, 6, 8):
        args = on_gpu(pack(mixed_rows(rng, k, rows=70), k))
        before_ids = graphlets.class_ids(*args).clone()
        before_key, before_status = (t.clone() for t in graphlets.canonical(*args))
        orbit, cls = graphlets.orbit_ids(*args, return_class=True)
        assert torch.equal(cls, before_ids)
        assert torch.equal(graphlets.class_ids(*args), before_ids)
        key, status = graphlets.canonical(*args)
        assert torch.equal(key, before_key) and torch.equal(status, before_status)
        tab = torch.cat([graphlets.table(k), torch.tensor([-1])]).to(DEV)
        assert torch.equal(tab[cls], key)                                        # the class the orbits were numbered in is the key's
        assert bool((orbit[status != 0] == graphlets.num_orbits(k)).all()) and bool((status != 0).any())
        base = graphlets.orbit_base(k).to(DEV)
        ok = status == 0
        inside = (orbit[ok] >= base[cls[ok]][:, None]) & (orbit[ok] < base[cls[ok] + 1][:, None]) | (args[0][ok] < 0)
        assert bool(inside.all())


def test_key_status_and_class_from_the_same_launch():
    """ugs_graphlet_orbits with all three optional outputs: what ugs_graphlet_canon writes, bit for bit, and the same orbit ids."""
    from ugs_sampler import _select_device, graphlets
    from ugs_sampler._lib import check, lib
    nodes, ei, ep = on_gpu(pack(mixed_rows(random.Random(78), 7, rows=70), 7))
    want_key, want_status = graphlets.canonical(nodes, ei, ep)
    want_cls, want_orbit = graphlets.class_ids(nodes, ei, ep), graphlets.orbit_ids(nodes, ei, ep)
    tab, base = graphlets.table(7).to(DEV), graphlets.orbit_base(7).to(DEV)
    orbit, key, cls = (torch.full(shape, -5, dtype=torch.int64, device=DEV) for shape in ((70, 7), (70,), (70,)))
    status = torch.full((70,), -5, dtype=torch.int32, device=DEV)
    _select_device(nodes.device, jobs=True)
    check(lib.ugs_graphlet_orbits(nodes.data_ptr(), ei.data_ptr(), ei.stride(0), ei.size(1), ep.data_ptr(), 70, 7, tab.data_ptr(),
                                  base.data_ptr(), tab.numel(), orbit.data_ptr(), key.data_ptr(), status.data_ptr(), cls.data_ptr()))
    assert torch.equal(key, want_key) and torch.equal(status, want_status) and torch.equal(cls, want_cls)
    assert torch.equal(orbit, want_orbit) and set(want_status.cpu().tolist()) == {0, 1, 2}


def gdv_law(n_vertices, und_edges, k):
    """{vertex: {orbit id: count}} over every connected k-subset of the graph, by the brute force."""
    nb = {v: set() for v in range(n_vertices)}
    for u, v in und_edges:
        nb[u].add(v)
        nb[v].add(u)
    table, base = tables(k)
    rank = {t: i for i, t in enumerate(table)}
    out = {v: {} for v in range(n_vertices)}
    sets = 0
    for sub in itertools.combinations(range(n_vertices), k):
        code = law.code_of_edges(k, [(i, j) for i, j in law.pairs(k) if sub[j] in nb[sub[i]]])
        if not law.connected(code, k):
            continue
        sets += 1
        first = base[rank[law.key_of(code, k)]]
        for v, x in zip(sub, olaw.local_indices(olaw.rooted_codes(code, k))):
            out[v][first + x] = out[v].get(first + x, 0) + 1
    return out, sets


def gdv_gpu(graphs, k):
    """The k-GDV of a batch of (n, undirected edges) graphs: enumerate_graphs + orbit_ids + vertex_orbit_counts."""
    import uniform_sampler
    from ugs_sampler import graphlets
    cols, ptr = [], [0]
    for n, es in graphs:
        cols += [(u + ptr[-1], v + ptr[-1]) for u, v in es] + [(v + ptr[-1], u + ptr[-1]) for u, v in es]
        ptr.append(ptr[-1] + n)
    ei = torch.tensor(cols, dtype=torch.int64).t().contiguous().to(DEV)
    out = uniform_sampler.enumerate_graphs(ei, torch.tensor(ptr, dtype=torch.int64).to(DEV), k, device=DEV)
    nodes, eidx, eptr, failed = out[0], out[1], out[2], out[5]
    assert not failed.any()
    columns = graphlets.connected_orbits(k)
    orbit = graphlets.orbit_ids(nodes, eidx, eptr)
    gdv = graphlets.vertex_orbit_counts(nodes, orbit, ptr[-1], columns)
    assert gdv.is_cuda and gdv.dtype == torch.int64 and tuple(gdv.shape) == (ptr[-1], columns.numel())
    assert int(gdv.sum()) == nodes.size(0) * k                                   # every slot of every connected k-set is counted
    return gdv.cpu().tolist(), columns.tolist(), ptr


def assert_gdv(graphs, k):
    gdv, columns, ptr = gdv_gpu(graphs, k)
    for g, (n, es) in enumerate(graphs):
        want, _ = gdv_law(n, es, k)
        for v in range(n):
            assert set(want[v]) <= set(columns)
            assert gdv[ptr[g] + v] == [want[v].get(c, 0) for c in columns], (g, v, k)
    return gdv


def test_gdv_of_the_petersen_graph():
    petersen = [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)]
    gdv = assert_gdv([(10, petersen)], 5)
    _, sets = gdv_law(10, petersen, 5)
    assert all(row == gdv[0] for row in gdv) and sum(gdv[0]) * 10 == sets * 5     # vertex-transitive: 5 * sets / 10 sets through each


@pytest.mark.parametrize("k", [3, 4])
def test_gdv_of_a_star(k):
    gdv = assert_gdv([(7, [(0, i) for i in range(1, 7)])], k)
    assert gdv[0] != gdv[1] and all(row == gdv[1] for row in gdv[1:])
    assert sum(x > 0 for x in gdv[0]) == 1 and sum(x > 0 for x in gdv[1]) == 1


@pytest.mark.parametrize("k", [4, 5])
def test_gdv_of_random_graphs(k):
    import ugs_workloads as workloads
    graphs = []
    for g, (n, e) in enumerate([(12, 14), (9, 12), (11, 11), (5, 4)]):
        ei = workloads.tu_graph(n, e, 900 + g)
        graphs.append((n, sorted({(int(min(u, v)), int(max(u, v))) for u, v in ei.T.tolist() if u != v})))
    gdv = assert_gdv(graphs, k)
    assert len({tuple(row) for row in gdv}) > 10


def test_cpu_tensors_and_no_rows():
    from ugs_sampler import graphlets
    rng = random.Random(12)
    arrays = pack(mixed_rows(rng, 5), 5)
    keys, stats, want = assert_law(arrays, "device tensors")
    host = tuple(torch.from_numpy(a) for a in arrays)
    got = graphlets.orbit_ids(*host)
    assert not got.is_cuda and got.dtype == torch.int64 and got.tolist() == want
    orbit, cls = graphlets.orbit_ids(*host, device=DEV, return_class=True)
    assert not orbit.is_cuda and not cls.is_cuda and orbit.tolist() == want
    assert cls.tolist() == law.ids_from(keys, stats, tables(5)[0])
    gdv = graphlets.vertex_orbit_counts(host[0], got, 50, graphlets.connected_orbits(5))
    assert not gdv.is_cuda and int(gdv.sum()) == sum(1 for r, row in enumerate(arrays[0]) for s, x in enumerate(row)
                                                       if 0 <= x < 50 and want[r][s] in graphlets.connected_orbits(5).tolist())

    nodes, ei, ep = on_gpu(arrays)
    none = graphlets.orbit_ids(nodes[:0], ei, ep[:1])
    assert none.is_cuda and none.dtype == torch.int64 and tuple(none.shape) == (0, 5)
    orbit, cls = graphlets.orbit_ids(nodes[:0], ei, ep[:1], return_class=True)
    assert tuple(orbit.shape) == (0, 5) and tuple(cls.shape) == (0,)
    nine = (torch.zeros((1, 9), dtype=torch.int64, device=DEV), ei, ep[:2])
    with pytest.raises(RuntimeError, match="k <= 8"):
        graphlets.orbit_ids(*nine)
    with pytest.raises(ValueError):
        graphlets.orbit_ids(nodes, ei.cpu(), ep)
    assert_law(arrays, "after the refusals")
