"""Order of a row's induced-edge items as the walk kernel stages them (stage_flush, 64-lane tiers), against the CPU oracle.

stage_flush has two branches.  Rows of at most 8 hits (a hit = one adjacency entry of a newly added vertex that points into the
sample) without a self hit rank their items one per lane inside a DPP row -- the FAST branch; rows of 9..32 hits, or with a self
hit, take the GENERAL branch (one hit per lane); rows of more than 32 hits are not staged at all and go to the row-reading fill
kernel (UNSTAGED).  Each case below is a graph built so that its complete rows reach one named branch; which one is verified on
the CPU from the oracle's rows alone: a row's hits are (entries with source != target) / 2 + (entries with source == target) of
its edge_ptr slice.  The GPU tests then ask for the oracle's outputs bit for bit, all in the 448-candidate 64-lane tier."""
import random

import numpy as np
import pytest

import scenarios as sc

FAST, GENERAL, UNSTAGED = "fast", "general", "unstaged"


def _ei(cols):
    return np.array(cols, dtype=np.int64).T.reshape(2, -1).copy()


def _tree(rng, n, off=0):
    return [(off + rng.randrange(v), off + v) if rng.random() < 0.5 else (off + v, off + rng.randrange(v)) for v in range(1, n)]


def _call(cols, ptr, m, k, mode, seed):
    return dict(fn="sample_batch", edge_index=_ei(cols), ptr=np.array(ptr, dtype=np.int64), m=m, k=k, mode=mode, seed=seed)


def _cases():
    """name -> (calls, {branch: (lowest, highest) hits its complete rows must have, and at least one row must reach each})"""
    rng = random.Random(20251)
    cases = {}
    # tree-shaped samples: every connected k-subgraph of a tree has exactly k - 1 hits (k <= 8 and k > 8: two forms of the member lookup)
    t = _tree(rng, 300)
    rng.shuffle(t)
    cases["trees"] = ([_call(t, [0, 300], 400, 8, "sample", 3), _call(t, [0, 300], 300, 5, "global", 4), _call(t, [0, 300], 300, 9, "graph", 5),
                       _call(t, [0, 300], 50, 2, "sample", 6)], {FAST: (1, 8)})
    # the boundary: graphs of exactly k vertices, so every complete row holds every edge -- a tree plus one extra edge at k = 8 (8 hits),
    # a tree at k = 9 (8 hits); a tree plus two at k = 8 and a tree plus one at k = 9 (9 hits)
    for name, k, extra, hits, branch in [("exactly_8_hits_k8", 8, 1, 8, FAST), ("exactly_8_hits_k9", 9, 0, 8, FAST),
                                         ("exactly_9_hits_k8", 8, 2, 9, GENERAL), ("exactly_9_hits_k9", 9, 1, 9, GENERAL)]:
        cols, ptr = [], [0]
        for _ in range(6):
            off = ptr[-1]
            e = _tree(rng, k, off)
            have = {frozenset(c) for c in e}
            while len(e) < k - 1 + extra:
                u, v = rng.sample(range(k), 2)
                if frozenset((off + u, off + v)) not in have:
                    have.add(frozenset((off + u, off + v)))
                    e.append((off + u, off + v))
            rng.shuffle(e)
            cols += e
            ptr.append(off + k)
        cases[name] = ([_call(cols, ptr, 40, k, mode, 11) for mode in ("sample", "graph", "global")], {branch: (hits, hits)})
    # a self loop among the hits: trees whose vertices carry self loops (a self loop is two equal adjacency entries, two hits with
    # source == target) -- at most 8 hits but a self hit: the general branch
    t = _tree(rng, 120)
    t += [(v, v) for v in range(0, 120, 5)]
    rng.shuffle(t)
    cases["self_loops"] = ([_call(t, [0, 120], 400, 4, "sample", 8)], {FAST: (3, 3), GENERAL: (5, 11)})
    # duplicate columns in both directions of an edge: a path whose edges each come as (u, v), (v, u) and (u, v) again -- three columns
    # per pair, k = 3: six hits whose columns must come out in column order inside every source
    p = []
    for v in range(1, 60):
        p += [(v - 1, v), (v, v - 1), (v - 1, v)]
    rng.shuffle(p)
    cases["duplicate_columns"] = ([_call(p, [0, 60], 300, 3, mode, 9) for mode in ("sample", "global")], {FAST: (6, 6)})
    # a dense small graph: 9..32 hits
    d = [(u, v) for u in range(14) for v in range(u + 1, 14) if rng.random() < 0.7]
    rng.shuffle(d)
    cases["dense_9_to_32_hits"] = ([_call(d, [0, 14], 300, 8, "sample", 10)], {GENERAL: (9, 28)})
    # more than 32 hits: complete graph, k = 10 -> 45 hits, not staged
    c = [(u, v) for u in range(13) for v in range(u + 1, 13)]
    rng.shuffle(c)
    cases["more_than_32_hits"] = ([_call(c, [0, 13], 200, 10, "sample", 12)], {UNSTAGED: (45, 45)})
    return cases


CASES = _cases()


def _branch_of(hits, self_hits):
    if hits > 32:
        return UNSTAGED
    return FAST if hits <= 8 and self_hits == 0 else GENERAL


def _rows_by_branch(result, k):
    """complete rows of one oracle result, as {branch: [hits, ...]}"""
    nodes, edge_index, edge_ptr = result[0], result[1], result[2]
    out = {}
    for r in range(nodes.shape[0]):
        lo, hi = int(edge_ptr[r]), int(edge_ptr[r + 1])
        if hi == lo:
            continue                                    # incomplete rows (and k = 1) carry no edges: nothing is staged
        assert (nodes[r] >= 0).all()
        s = int((edge_index[0, lo:hi] == edge_index[1, lo:hi]).sum())
        assert (hi - lo - s) % 2 == 0
        hits = (hi - lo - s) // 2 + s
        out.setdefault(_branch_of(hits, s), []).append(hits)
    return out


@pytest.fixture(scope="module")
def orc():
    from backends import OracleBackend
    return OracleBackend()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_branch_by_the_oracles_rows(name, orc):
    calls, want = CASES[name]
    seen = {}
    for call, res in zip(calls, sc.run_scenario(calls, orc)):
        assert isinstance(res, tuple) and not isinstance(res[0], str), repr(res)
        for b, h in _rows_by_branch(res, call["k"]).items():
            seen.setdefault(b, []).extend(h)
    assert set(seen) == set(want), f"{name}: rows reach {sorted(seen)}, meant {sorted(want)}"
    for b, (lo, hi) in want.items():
        assert min(seen[b]) >= lo and max(seen[b]) <= hi, f"{name}: {b} rows have {min(seen[b])}..{max(seen[b])} hits, meant {lo}..{hi}"
        assert len(seen[b]) >= 20, f"{name}: only {len(seen[b])} rows reach the {b} branch"
    if name == "trees":
        assert 7 in seen[FAST] and 8 in seen[FAST] and 1 in seen[FAST]


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(CASES))
def test_item_order_vs_oracle(name, orc, monkeypatch):
    from backends import ProductBackend
    monkeypatch.setenv("UGS_FORCE_TIER", "1")           # 64 lanes per walk, 448 candidates: the tier that stages edges
    calls, _ = CASES[name]
    got = sc.run_scenario(calls, ProductBackend())
    want = sc.run_scenario(calls, orc)
    for i, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, tuple) and isinstance(w, tuple) and not isinstance(g[0], str), f"{name}: call {i}: {g!r}"
        assert len(g) == len(w)
        for j, (a, b) in enumerate(zip(g, w)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{name}: call {i} output {j} differs"
