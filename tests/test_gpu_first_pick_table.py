"""GPU: the first-pick table of a single-graph plan (UgsWalkArgs::ord1, ugs_build_ord1) and the walks that take their first pick
from it (do_walk's launch-uniform instantiation), bit-exact against the CPU oracle.

The candidate list a root's row leaves, D1(v) -- the distinct neighbours of v that pass the suffix filter, v itself left out, in
first-occurrence order -- and the iteration order of the reference's unordered_set built from it depend on the plan and the root
alone.  The table keeps, per vertex, the position in D1 of the candidate at every iteration position r < |D1| <= 64; the walk reads
byte `rsel` of its root instead of computing the order.  Checked here: every byte of the table of small multigraphs against the
oracle's restated unordered_set (stl_order); walks through the table path against the oracle and against the same call with the
table switched off; and how a plan keeps, shares and accounts for the table."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

MODES = ("sample", "graph", "global")
TIER_M = "1"                                                                   # 448 candidates, one walk per wave
NAMES = ("nodes", "edge_index", "edge_ptr", "edge_src")


def _multigraph(rng, n, deg, isolated=10, wide=150, core=0, core_deg=0):
    """Random multigraph on n vertices with a mean of `deg` entries per row, repeats counted: random columns among the first
    n - isolated vertices (the last `isolated` have none) -- `core_deg` of a core vertex's entries inside the first `core` vertices --,
    a fifth of them again the other way round and a seventh again the same way, self loops once and twice.  On top of that
    vertex 0 is adjacent to `wide` vertices that each carry 110 self-loop columns: their rows are longer than vertex 0's, so the
    ordering ranks them all behind it and D1(0) holds all of them."""
    live = n - isolated
    rep = 1.0 + 1.0 / 5 + 1.0 / 7                                              # entries per random column, with its repeats
    mc = int(core * core_deg / 2 / rep)
    m = int((live * deg - core * core_deg) / 2 / rep)
    u, v = rng.integers(1, live, m), rng.integers(1, live, m)
    if mc:
        u, v = np.concatenate([u, rng.integers(1, core, mc)]), np.concatenate([v, rng.integers(1, core, mc)])
        mix = rng.permutation(len(u))
        u, v = u[mix], v[mix]
    base = np.stack([u, v])
    once, twice = np.arange(1, live, 9), np.arange(2, live, 11)
    cols = [base, base[::-1, ::5], base[:, 1::7], np.stack([once, once]), np.stack([twice, twice]), np.stack([twice, twice])]
    if wide:
        nb = rng.choice(np.arange(1, live), size=wide, replace=False)
        cols += [np.stack([np.zeros(wide, dtype=np.int64), nb]), np.repeat(np.stack([nb, nb]), 110, axis=1)]
    ei = np.concatenate(cols, axis=1).astype(np.int64)
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def _small_components(sizes):
    """paths, stars and cliques of the given sizes: with k above the largest no root has weight, the roots come from the relaxed list
    (level 1) and every walk stops early"""
    cols, lo = [], 0
    for i, size in enumerate(sizes):
        if i % 3 == 0:
            a, b = np.triu_indices(size, 1)
        elif i % 3 == 1:
            a, b = np.arange(size - 1), np.arange(1, size)
        else:
            a, b = np.zeros(size - 1, dtype=np.int64), np.arange(1, size)
        cols.append(np.stack([a + lo, b + lo]))
        lo += size
    return np.ascontiguousarray(np.concatenate(cols, axis=1).astype(np.int64)), lo


_D1 = {}


def _d1(key, ei, n, k):
    """(D1(v) for every v, the preprocessing dump) from the oracle's CSR and ordering; computed once per graph"""
    if key not in _D1:
        pre = oracle.Preproc(ei, n, k)
        d = pre.dump()
        pre.close()
        indptr, idx, rank = d["indptr"], d["indices"], d["index_of"]
        lists = []
        for v in range(n):
            row = idx[indptr[v]:indptr[v + 1]]
            keep = row[(rank[row] >= rank[v]) & (row != v)]
            _, first = np.unique(keep, return_index=True)
            lists.append(keep[np.sort(first)])
        _D1[key] = (lists, d)
    return _D1[key]


def _expected_bytes(d1):
    """byte r = position in D1 of the candidate at iteration position r of the unordered_set built from D1"""
    pos = {int(w): i for i, w in enumerate(d1)}
    return np.array([pos[int(w)] for w in oracle.stl_order(d1)], dtype=np.uint8)


def _plan(ei, n, k):
    import ugs_sampler
    ugs_sampler.clear_cache()
    return ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.tensor([0, n], dtype=torch.int64), k)


GRAPHS = {                                                                     # name: (seed, n, mean degree, vertices in vertex 0's D1, core, its degree)
    "n300_deg3": (1, 300, 3, 150, 0, 0),
    "n700_deg24": (2, 700, 24, 150, 0, 0),
    "n2000_deg12": (3, 2000, 12, 200, 0, 0),
    "n600_deg70": (4, 600, 70, 200, 160, 150),
}


def _graph(name):
    seed, n, deg, wide, core, core_deg = GRAPHS[name]
    return _multigraph(np.random.default_rng(seed), n, deg, wide=wide, core=core, core_deg=core_deg), n, wide


@pytest.mark.parametrize("name", list(GRAPHS))
def test_every_byte_of_the_table_against_the_oracle(name, monkeypatch):
    ei, n, wide = _graph(name)
    lists, d = _d1(name, ei, n, 3)
    c1 = np.array([len(x) for x in lists])
    # the inputs: repeated columns in both directions, self loops, isolated vertices, a root with far more than 64 candidates
    pairs = {}
    for a, b in ei.T.tolist():
        pairs[(a, b)] = pairs.get((a, b), 0) + 1
    assert any(c > 1 for c in pairs.values()) and any((b, a) in pairs for (a, b) in pairs if a != b)
    assert any(a == b for a, b in pairs) and (np.diff(d["indptr"])[n - 10:] == 0).all() and c1[0] == wide and wide > 128
    monkeypatch.setenv("UGS_FORCE_TIER", TIER_M)
    plan = _plan(ei, n, 3)
    assert plan.first_pick_table() is None, "built with the padded rows, at the first walk"
    plan.walk(4, "sample", 1)
    roots = plan.graph_roots(0, n)
    assert roots["level"] == 0                                                 # roots drawn by weight: every vertex has its 64 bytes
    tab = plan.first_pick_table()
    plan.close()
    assert tab is not None and tab["ord1"].shape == (n, 64)
    assert np.array_equal(tab["c1"], c1), "candidates the root's row leaves"
    checked = 0
    for v in range(n):
        if 1 <= c1[v] <= 64:
            want = _expected_bytes(lists[v])
            assert np.array_equal(tab["ord1"][v, :c1[v]], want), (v, c1[v])
            checked += 1
    assert checked > n // 3


def test_the_graphs_cover_every_range_of_candidate_counts():
    """a condition on the inputs of the test above: between them the graphs have roots whose D1 stays below the 13-bucket stage, ends
    in the 29-, in the 59- and, with 60..64 candidates, at the top of the table's range -- and roots beyond it"""
    c1 = []
    for name in GRAPHS:
        ei, n, _ = _graph(name)
        c1 += [len(x) for x in _d1(name, ei, n, 3)[0]]
    c1 = np.array(c1)
    for lo, hi in ((1, 12), (13, 29), (30, 59), (60, 64), (65, 448)):
        assert ((c1 >= lo) & (c1 <= hi)).sum() >= 5, (lo, hi)
    assert (c1 == 0).any()


def test_table_of_a_graph_with_relaxed_roots(monkeypatch):
    """level 1: the roots are the viable list; the table holds the bytes of exactly those vertices"""
    ei, n = _small_components([2, 3, 5, 7] * 6)
    lists, d = _d1("components", ei, n, 8)
    monkeypatch.setenv("UGS_FORCE_TIER", TIER_M)
    plan = _plan(ei, n, 8)
    plan.walk(4, "sample", 1)
    roots = plan.graph_roots(0, n)
    tab = plan.first_pick_table()
    plan.close()
    assert roots["level"] == 1 and 0 < roots["num_viable"] < n
    viable = roots["viable_v"][:roots["num_viable"]]
    assert tab is not None and max(len(lists[v]) for v in viable) >= 4
    for v in viable:
        c = len(lists[v])
        assert tab["c1"][v] == c
        if c:
            assert np.array_equal(tab["ord1"][v, :c], _expected_bytes(lists[v])), v
    rest = np.setdiff1d(np.arange(n), viable)
    assert all(len(lists[v]) == 0 for v in rest), "a vertex outside the viable list has no candidate: nothing to look up"


def _rows(ei, n, m, k, mode, seed):
    plan = _plan(ei, n, k)
    got = [t.cpu().numpy() for t in plan.sample_rows(m, mode=mode, seed=seed)]
    info, launch, tab = plan.info(), plan.last_launch(), plan.first_pick_table() is not None
    plan.close()
    return got, info, launch, tab


def _walks(ei, n, m, k, monkeypatch, modes=MODES, seed=42):
    """rows with the table, rows without it, the oracle's; returns the oracle's "sample" output"""
    monkeypatch.setenv("UGS_FORCE_TIER", TIER_M)
    first = None
    for mode in modes:
        w = oracle.sample_batch(ei, np.array([0, n], dtype=np.int64), m, k, mode, seed)
        want = [np.asarray(w[0]), np.asarray(w[1]), np.asarray(w[2]), np.asarray(w[4])]
        monkeypatch.delenv("UGS_NO_FIRST_PICK_TABLE", raising=False)
        got, info, launch, tab = _rows(ei, n, m, k, mode, seed)
        assert info["tier"] == 1 and tab and launch["kernel"].startswith("ugs_walk_lds<64,448"), (info, launch, tab)
        monkeypatch.setenv("UGS_NO_FIRST_PICK_TABLE", "1")
        off, _, launch_off, tab_off = _rows(ei, n, m, k, mode, seed)
        monkeypatch.delenv("UGS_NO_FIRST_PICK_TABLE")
        assert not tab_off and launch_off["kernel"] == launch["kernel"]
        for name, a, b, c in zip(NAMES, got, want, off):
            assert a.shape == b.shape and np.array_equal(a, b), f"{name} differs from the oracle (mode {mode}, k {k})"
            assert np.array_equal(a, c), f"{name} differs from the call without the table (mode {mode}, k {k})"
        first = first or w
    return first


def _dense():
    """n = 400, a mean of 125 entries per row (D1 of up to 78 vertices): roots on both sides of 64 candidates are drawn at every k"""
    return _multigraph(np.random.default_rng(11), 400, 125, wide=0), 400


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_walks_through_the_table_path(k, monkeypatch):
    ei, n = _dense()
    want = _walks(ei, n, 2000, k, monkeypatch)
    lists, _ = _d1("dense", ei, n, k if k > 1 else 2)                        # (the ordering does not depend on k)
    c1 = np.array([len(x) for x in lists])
    roots = np.asarray(want[0])[:, 0]
    assert (roots >= 0).all()
    cr = c1[roots]
    assert ((cr >= 1) & (cr <= 64)).sum() > 100 and (cr > 64).sum() > 100, "roots whose first pick comes from the table, and roots beyond it"
    if k > 1:
        assert (np.asarray(want[0])[:, 1] >= 0).all()


def test_walks_with_relaxed_roots(monkeypatch):
    """no connected 8-subgraph: level 1, every walk stops early -- after its first pick, or later"""
    ei, n = _small_components([2, 3, 5, 7] * 6)
    want = _walks(ei, n, 2000, 8, monkeypatch)
    sizes = (np.asarray(want[0]) >= 0).sum(axis=1)
    assert {2, 3, 5, 7} <= set(sizes.tolist()) and sizes.max() == 7


def test_walks_of_a_launch_that_shares_its_work_through_the_counter(monkeypatch):
    """more rows than 64 per CU: the dynamic work loop, whose walks take their random numbers from the lanes (the flagship's kernel)"""
    ei, n = _dense()
    monkeypatch.setenv("UGS_FORCE_TIER", TIER_M)
    plan = _plan(ei, n, 8)
    plan.walk(20000, "sample", 7)
    name = plan.last_launch()["kernel"]
    plan.close()
    assert name == "ugs_walk_lds<64,448,draws>", name
    _walks(ei, n, 20000, 8, monkeypatch, modes=("sample",), seed=7)


def test_plan_and_twin_on_two_streams_and_the_bytes_of_the_table(monkeypatch):
    ei, n = _dense()
    monkeypatch.setenv("UGS_FORCE_TIER", TIER_M)
    monkeypatch.setenv("UGS_PROW_SHIFT", "4")                                  # padded rows of 16 entries: 128 bytes per vertex
    m, k = 1500, 8
    grown = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv("UGS_NO_FIRST_PICK_TABLE", "1")
        plan = _plan(ei, n, k)
        before = plan.info()["device_bytes"]
        twin = plan.twin()                                                     # builds the owner's rows (and table) and shares them
        grown[off] = plan.info()["device_bytes"] - before
        assert (plan.first_pick_table() is None) == off and (twin.first_pick_table() is None) == off
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for p, s, seed in ((plan, s1, 5), (twin, s2, 6), (plan, s1, 6), (twin, s2, 5)):
            with torch.cuda.stream(s):
                outs.append(p.sample_rows(m, mode="sample", seed=seed))
        torch.cuda.synchronize()
        for a, b in ((0, 3), (1, 2)):
            for name, x, y in zip(NAMES, outs[a], outs[b]):
                assert torch.equal(x, y), (name, off)
        w = oracle.sample_batch(ei, np.array([0, n], dtype=np.int64), m, k, "sample", 5)
        for name, x, y in zip(NAMES, outs[0], (w[0], w[1], w[2], w[4])):
            assert np.array_equal(x.cpu().numpy(), np.asarray(y)), (name, off)
        twin.close()
        plan.close()
    assert grown[True] == n * 128 and grown[False] == n * 128 + n * 64, grown
