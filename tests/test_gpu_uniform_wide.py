"""uniform_sampler on graphs of 65 to 1024 vertices (the wide form of ugs_uniform.hip, opt-in by set_max_vertices) against the
reference's outputs (tests/golden/f18_uniform_wide_reference.*) and the CPU law (tests/uniform_wide_law.py): bit-exact, every
tensor.  The limit and the mask threshold are process-wide, so every test restores them."""
import contextlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import ugs_workloads as wl
import uniform_law as U
import uniform_wide_law as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F18 = os.path.join(HERE, "golden", "f18_uniform_wide_reference")
F14 = os.path.join(HERE, "golden", "f14_uniform_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
SIZES = [65, 127, 128, 129, 191, 192, 193, 256, 257, 512, 1000, 1024]


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


def scenarios(path):
    with open(path + ".json") as f:
        return json.load(f)["scenarios"]


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        b = b.cpu().numpy() if torch.is_tensor(b) else b
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def call(ei, ptr, m, k, mode="sample", seed=42, device=None):
    e, p = torch.from_numpy(np.ascontiguousarray(ei)), torch.from_numpy(np.asarray(ptr))
    if device is not None:
        e, p = e.to(device), p.to(device)
    return sampler().sample_batch(e, p, m, k, mode=mode, seed=seed)


# ---- 1. the reference's outputs ----
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("s", scenarios(F18), ids=lambda s: s["name"])
def test_equals_reference_fixture(s, where):
    z = np.load(F18 + ".npz")
    name = s["name"]
    with limits(1024):
        got = call(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]),
                   device="cuda:0" if where == "device" else None)
    if where == "device":
        assert all(t.is_cuda for t in got)
    else:
        assert all(t.device.type == "cpu" for t in got) and all(t.is_pinned() for t in got if t.numel() > 0)
    assert_same(got, [z[f"{name}/{nm}"] for nm in NAMES], name)


# ---- 2. random mixed batches against the law ----
def sparse_graph(rng, n, k):
    if n <= 1:
        return np.zeros((2, 0), np.int64)
    extra = rng.randint(0, max(1, n // 16)) if k >= 5 else rng.randint(0, n // 3 + 1)
    return wl.tu_graph(n, n - 1 + extra, rng.randrange(1 << 30))


def mixed_batch(rng, k, G):
    allowed = [n for n in SIZES if W.takes_wide_form(n, k, 1024)]
    sizes = [rng.choice(allowed) if rng.random() < 0.5 else rng.randint(1, 64) for _ in range(G)]
    sizes[rng.randrange(G)] = rng.choice(allowed)
    sizes += [0, max(k - 1, 0)]                                     # an empty graph and one with n < k
    rng.shuffle(sizes)
    ei, ptr = W.batch([(n, sparse_graph(rng, n, k)) for n in sizes], first=rng.randint(1, 9))
    perm = np.array(rng.sample(range(ei.shape[1]), ei.shape[1]), dtype=np.int64)   # columns in any order
    return np.ascontiguousarray(ei[:, perm]), ptr


# every k of the rule with rows to compare, every mode at small and at large k; m = 0 as cases of its own
MIXED = [(1, 7, "sample"), (2, 40, "global"), (3, 13, "graph"), (4, 25, "sample"), (5, 40, "global"), (6, 7, "graph"),
         (7, 25, "sample"), (8, 40, "global"), (8, 13, "sample"), (7, 9, "graph"), (4, 0, "sample"), (8, 0, "global")]


@pytest.mark.parametrize("case", range(len(MIXED)), ids=lambda c: "k%d_m%d_%s" % MIXED[c])
def test_equals_law_on_random_mixed_batches(case):
    k, m, mode = MIXED[case]
    rng = random.Random(1800 + case)
    ei, ptr = mixed_batch(rng, k, rng.randint(2, 5))
    assert any(W.takes_wide_form(int(n), k, 1024) for n in np.diff(ptr))
    seed = rng.getrandbits(64)
    want = W.sample_batch(ei, ptr, m, k, mode, seed)
    if m:                                                           # a wide graph of the batch has rows that are not placeholders
        wide = [g for g, n in enumerate(np.diff(ptr)) if n > 64]
        assert any((want[0][g * m:(g + 1) * m] >= 0).all() for g in wide)
    with limits(1024):
        assert_same(call(ei, ptr, m, k, mode, seed), want, f"case {case}")


@pytest.mark.parametrize("n", [129, 200, 256])
def test_k8_uses_the_whole_key(n):
    """k = 8 with b = 8: the key is 64 bits wide and a root of 128 or more sets its bit 63 (the last search level, the sort and
    the row decode at full width).  One component below vertex 20, one in the graph's last 40 vertices (n = 256: up to 255)."""
    high = n - 40
    assert high + 39 == n - 1 and (n == 129 or high >= 128)
    low_part, high_part = wl.tu_graph(20, 22, n), wl.tu_graph(40, 44, n + 1) + high
    if n == 129:                                                    # 89 ... 128 straddles the word and the bit-63 boundary
        high_part = np.concatenate([high_part, undirected([(120, 128), (127, 128)])], axis=1)
    ei, ptr = W.batch([(12, wl.tu_graph(12, 13, 3)), (n, np.concatenate([low_part, high_part], axis=1))], first=6)
    assert W.takes_wide_form(n, 8, 1024) and W.field_bits(n) == 8
    m = 96
    for mode, seed in (("sample", 42), ("global", (1 << 64) - 1)):
        want = W.sample_batch(ei, ptr, m, 8, mode, seed)
        roots = want[0][m:, 0] - ptr[1]
        assert (roots >= 0).all() and (roots < 20).any() and (want[0][m:, 7] - ptr[1] == n - 1).any()
        if n != 129:
            assert (roots >= 128).any()                             # keys with bit 63 set are drawn
        with limits(1024):
            assert_same(call(ei, ptr, m, 8, mode, seed), want, (n, mode))
            assert_same(call(ei, ptr, m, 8, mode, seed, device="cuda:0"), want, (n, mode, "device"))


@pytest.mark.parametrize("k", [1, 2])
def test_vertex_zero_of_a_wide_graph_is_drawn(k):
    """{0} at k = 1 has key 0, {0, 1} at k = 2 has key 1: a row is valid by its graph, not by its key."""
    n = 130
    ei, ptr = W.batch([(n, np.array([[0, 1], [1, 0]], np.int64))], first=3)    # k = 2: the only set is {0, 1}
    m = 64
    seed = next(s for s in range(100) if (W.sample_batch(ei, ptr, m, k, "sample", s)[0][:, 0] == 3).any())   # a seed that draws vertex 0
    with limits(1024):
        for mode in ("sample", "global"):
            assert_same(call(ei, ptr, m, k, mode, seed), W.sample_batch(ei, ptr, m, k, mode, seed), mode)


# ---- 3. word boundaries ----
def undirected(pairs):
    a = np.array(pairs, np.int64).reshape(-1, 2).T
    return np.concatenate([a, a[::-1]], axis=1)


BOUNDARY = {
    "path_across_words": (1024, undirected([(i, i + 1) for i in (61, 62, 63, 64, 125, 126, 127, 128, 957, 958, 959, 960, 961)]), 3),
    "star_hub_64": (200, undirected([(64, v) for v in (0, 1, 63, 65, 127, 128, 129, 191, 192, 199)]), 4),
    "vertex_1023": (1024, undirected([(1020, 1021), (1021, 1022), (1022, 1023), (1019, 1023), (0, 1023)]), 3),
    "last_word_only": (1000, undirected([(960 + i, 961 + i) for i in range(39)] + [(960, 999), (970, 990)]), 5),
    "hub_above_its_leaves": (300, undirected([(299, v) for v in range(0, 290, 7)] + [(150, 299), (150, 151)]), 3),
}


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_word_boundaries(name):
    n, g, k = BOUNDARY[name]
    ei, ptr = W.batch([(n, g)], first=2)
    want = W.sample_batch(ei, ptr, 50, k, "sample", 9)
    assert (want[0] >= 0).all()
    if name == "vertex_1023":
        assert (want[0] == 2 + 1023).any()
    with limits(1024):
        assert_same(call(ei, ptr, 50, k, "sample", 9), want, name)
        assert_same(call(ei, ptr, 50, k, "global", 9), W.sample_batch(ei, ptr, 50, k, "global", 9), name)


# ---- 4. a wide root bucket above the LDS sort's 8192 keys, at depth ----
def test_large_wide_root_bucket_k6():
    """tu_graph(620, 1150, 6): 620 vertices, 2300 columns, 891 625 connected 6-subsets, largest root bucket 77 054."""
    ei = wl.tu_graph(620, 1150, 6)
    ptr = np.array([0, 620], np.int64)
    tuples = W.sorted_tuples(U.graph_adjacency(ei[0], ei[1], 0, 620), 6)
    roots = np.bincount([t[0] for t in tuples])
    assert len(tuples) == 891625 and roots.max() == 77054
    enum = lambda adj, k: tuples                                    # noqa: E731  (computed once, shared by both modes)
    with limits(1024):
        for mode, seed in (("sample", 42), ("global", 7)):
            assert_same(call(ei, ptr, 64, 6, mode, seed), U.sample_batch(ei, ptr, 64, 6, mode, seed, enumerate_fn=enum), mode)


# ---- 5. the mask threshold: narrow graphs through the wide kernels ----
@pytest.mark.parametrize("s", [s for s in scenarios(F14) if 1 <= s["k"] <= 8], ids=lambda s: s["name"])
def test_f14_through_the_wide_kernels(s):
    z = np.load(F14 + ".npz")
    name = s["name"]
    with limits(mask_vertices=0):
        got = call(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]))
    assert_same(got, [z[f"{name}/{nm}"] for nm in NAMES], name)


@pytest.mark.parametrize("k,mask_vertices", [(3, 0), (6, 0), (8, 0), (5, 20), (9, 0)])
def test_narrow_batch_wide_equals_mask(k, mask_vertices):
    """k = 9 does not fit the wide rule: those graphs stay masks whatever the threshold."""
    rng = random.Random(50 + k)
    graphs = [(n, sparse_graph(rng, n, k)) for n in (1, 5, 13, 20, 21, 40, 63, 64, 33, 2)]
    ei, ptr = W.batch(graphs, first=4)
    want = call(ei, ptr, 25, k, "sample", 77)
    assert (want[0].numpy() >= 0).any()
    with limits(mask_vertices=mask_vertices):
        assert_same(call(ei, ptr, 25, k, "sample", 77), want, "sample")
        assert_same(call(ei, ptr, 25, k, "global", 78, device="cuda:0"), call(ei, ptr, 25, k, "global", 78), "global")
    assert_same(call(ei, ptr, 25, k, "sample", 77), want, "restored")


# ---- 6. limit mechanics ----
def test_setter_returns_previous_and_rejects_out_of_range():
    us = sampler()
    start = us.max_vertices()
    try:
        assert us.set_max_vertices(200) == start and us.max_vertices() == 200
        assert us.set_max_vertices(1024) == 200 and us.max_vertices() == 1024
        for bad in (63, 1025, 0, -1):
            with pytest.raises(RuntimeError):
                us.set_max_vertices(bad)
            assert us.max_vertices() == 1024
        for bad in (-1, 65):
            with pytest.raises(RuntimeError):
                us._set_mask_vertices(bad)
        assert us._set_mask_vertices(64) == 64
    finally:
        us.set_max_vertices(start)
    assert us.max_vertices() == start
    assert "set_max_vertices" in us.__all__ and "max_vertices" in us.__all__


def test_narrow_batch_does_not_depend_on_the_limit():
    ei, ptr = wl.tu_batch(18, 20, 6)
    with limits(64):
        a = call(ei, ptr, 32, 5, "sample", 3)
    with limits(1024):
        b = call(ei, ptr, 32, 5, "sample", 3)
    assert_same(a, b)
    assert_same(a, U.sample_batch(ei, ptr, 32, 5, "sample", 3))


def test_refusals_name_the_limit_and_the_rule():
    e129, p129 = W.batch([(10, wl.tu_graph(10, 12, 1)), (129, wl.tu_graph(129, 140, 2))])
    with limits(128):
        with pytest.raises(RuntimeError, match=r"graph 1 has 129 vertices.*more than 128 vertices"):
            call(e129, p129, 4, 3)
        assert_same(call(*W.batch([(128, wl.tu_graph(128, 140, 2))]), 4, 3), W.sample_batch(*W.batch([(128, wl.tu_graph(128, 140, 2))]), 4, 3))
    with limits(64):
        with pytest.raises(RuntimeError, match="graphs of more than 64 vertices"):
            call(e129, p129, 4, 3)
    e300, p300 = W.batch([(300, wl.tu_graph(300, 310, 3))])
    with limits(1024):
        with pytest.raises(RuntimeError, match=r"graph 0 has 300 vertices.*1024.*k \* b <= 64"):
            call(e300, p300, 4, 8)
        with pytest.raises(RuntimeError, match=r"k <= 8"):
            call(e300, p300, 4, 9)
        assert (call(e300, p300, 2, 301)[0].numpy() == -1).all()   # fewer than k vertices: allowed, rows of -1
        assert_same(call(e129, p129, 4, 3), W.sample_batch(e129, p129, 4, 3), "usable after the errors")


# ---- 7. sample_graphs and the presample cache ----
def complete_graph(n):
    u, v = np.triu_indices(n, 1)
    return np.array([np.r_[u, v], np.r_[v, u]], np.int64)


def test_sample_graphs_wide_members_and_lone_failures():
    k, m = 6, 16
    graphs = [(30, wl.tu_graph(30, 33, 1)), (200, wl.tu_graph(200, 215, 2)), (1025, wl.tu_graph(1025, 1030, 3)), (100, complete_graph(100)),
              (70, wl.tu_graph(70, 80, 4)), (5, wl.tu_graph(5, 5, 5))]
    ei, ptr = W.batch(graphs, first=1)
    seeds = torch.tensor([11, 12, 13, 14, 15, 16], dtype=torch.int64)
    with limits(1024):
        out = sampler().sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, seeds)
        nodes, eidx, eptr, sptr, esrc, failed = [t.cpu().numpy() for t in out]
        assert failed.tolist() == [False, False, True, True, False, False]
        for g in range(len(graphs)):
            rows = slice(g * m, (g + 1) * m)
            e0, e1 = eptr[g * m], eptr[(g + 1) * m]
            if failed[g]:
                assert (nodes[rows] == -1).all() and e0 == e1
                continue
            one = [t.numpy() for t in call(ei, ptr[g:g + 2], m, k, "sample", int(seeds[g]))]
            assert np.array_equal(nodes[rows], one[0]) and np.array_equal(eidx[:, e0:e1], one[1]), g
            assert np.array_equal(eptr[g * m:(g + 1) * m + 1] - e0, one[2]) and np.array_equal(esrc[e0:e1], one[4]), g
            if g in (1, 4):
                law = W.sample_batch(ei, ptr[g:g + 2], m, k, "sample", int(seeds[g]))
                assert np.array_equal(one[0], law[0]) and np.array_equal(one[1], law[1]) and np.array_equal(one[4], law[4])
        assert np.array_equal(sptr, np.arange(len(graphs) + 1) * m)
    with limits(64):                                                # back at the default the wide members fail alone, as before
        failed = sampler().sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, seeds)[5]
        assert failed.tolist() == [False, True, True, True, True, False]


def test_presample_cache_add_many_equals_add_loop_with_wide_members():
    """A PROTEINS-shaped list: most graphs below 64 vertices, some above, one of 620; one of 1100 fails in both."""
    from ugs_sampler.presample import PresampleCache
    rng = random.Random(7)
    sizes = [rng.randint(8, 60) for _ in range(12)] + [90, 150, 620, 1100]
    rng.shuffle(sizes)
    graphs = [wl.tu_graph(n, n + n // 8, 100 + i) for i, n in enumerate(sizes)]
    N, m, k = len(sizes), 8, 6
    seeds = [42 + i for i in range(N)]
    with limits(1024):
        loop = PresampleCache(m, k, "cuda:0", sampler="uniform")
        for i in range(N):
            loop.add(i, torch.from_numpy(graphs[i]), sizes[i], seeds[i])
        many = PresampleCache(m, k, "cuda:0", sampler="uniform")
        many.add_many(range(N), [(torch.from_numpy(g), n) for g, n in zip(graphs, sizes)], seeds)
        assert loop.failed == many.failed == {sizes.index(1100)}
        for order in (list(range(N)), [sizes.index(620), 0, sizes.index(150), sizes.index(1100)]):
            ptr = np.cumsum([0] + [sizes[i] for i in order])
            cols = np.concatenate([graphs[i] + ptr[j] for j, i in enumerate(order)], axis=1)
            x, y = (c.load(torch.tensor(order), torch.from_numpy(ptr), torch.from_numpy(cols)) for c in (loop, many))
            for u, v in zip(x, y):
                assert torch.equal(u.cpu(), v.cpu()), order
        w = sizes.index(620)
        got = loop.load(torch.tensor([w]), torch.tensor([0, 620]), torch.from_numpy(graphs[w]))
        assert_same(got, W.sample_batch(graphs[w], [0, 620], m, k, "sample", seeds[w]), "620 vertices")


# ---- 8. the environment variable, in a fresh process ----
def test_environment_variable_sets_the_initial_limit():
    code = "import uniform_sampler as u; print(u.max_vertices())"
    env = dict(os.environ, UGS_UNIFORM_MAX_VERTICES="256", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split() == ["256"]
