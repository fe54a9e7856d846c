"""CPU checks of tests/uniform_law.py, the restatement of the reference uniform_sampler's law that the GPU tests compare the
HIP product against: generator, draw rule, enumeration, and the reference's own outputs (tests/golden/f14_uniform_reference.*)."""
import json
import os
import random

import numpy as np
import pytest

import ugs_workloads as wl
import uniform_law as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f14_uniform_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def golden():
    z = np.load(GOLDEN + ".npz")
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    return [(s, z) for s in meta["scenarios"]]


def test_mt19937_64_10000th_output():
    g = U.mt19937_64()
    for _ in range(9999):
        g()
    assert g() == 9981545732273789042          # C++ [rand.predef]


class Stub:
    def __init__(self, words):
        self.words, self.i = list(words), 0

    def __call__(self):
        w = self.words[self.i % len(self.words)]
        self.i += 1
        return w


def rejecting_word(n, c):
    """A 64-bit word x with lo64(x * n) == c (n odd): rejected by the Lemire step when c < 2^64 mod n."""
    return (c * pow(n, -1, 1 << 64)) & U.M64


def libstdcxx_rule(words, n):
    """bits/uniform_int_dist.h:246-268 transcribed literally."""
    it = iter(words)
    product = next(it) * n
    low = product & U.M64
    if low < n:
        threshold = (-n) % (1 << 64) % n
        while low < threshold:
            product = next(it) * n
            low = product & U.M64
    return product >> 64


@pytest.mark.parametrize("n", [1, 3, 7, 1000003, 2147483647])
def test_lemire_matches_libstdcxx_rule_with_forced_rejections(n):
    t = (1 << 64) % n
    rng = random.Random(n)
    for trial in range(50):
        rej = [rejecting_word(n, rng.randrange(t)) for _ in range(trial % 4)] if t else []
        words = rej + [rng.getrandbits(64)]
        assert U.lemire(Stub(words), n) == libstdcxx_rule(words, n)
        assert U.lemire(Stub(words), n) == U.lemire(Stub(words[len(rej):]), n)   # rejected words are skipped


def test_blocked_draws_equal_sequential_draws_with_rejections():
    """The GPU draw kernel's cursor logic: rejections inside a block, at its last word, and in runs."""
    rng = random.Random(5)
    sizes = [rng.choice([3, 7, 2147483647, 1000003]) for _ in range(1500)]
    words = []
    for d, n in enumerate(sizes):
        t = (1 << 64) % n
        if t and d % 37 == 0:
            words += [rejecting_word(n, rng.randrange(t)) for _ in range(1 + d % 3)]
        words.append(rng.getrandbits(64))
    words += [rng.getrandbits(64) for _ in range(1000)]
    seq = Stub(words)
    want = [U.lemire(seq, n) for n in sizes]
    assert U.draws_blocked(Stub(words), sizes) == want
    assert U.draws_blocked(Stub(words), sizes, block=5) == want
    g1, g2 = U.mt19937_64(42), U.mt19937_64(42)
    assert U.draws_blocked(g1, sizes) == [U.lemire(g2, n) for n in sizes]


def random_adj(n, p, seed):
    rng = random.Random(seed)
    adj = [0] * n
    for u in range(n):
        for v in range(u + 1, n):
            if rng.random() < p:
                adj[u] |= 1 << v
                adj[v] |= 1 << u
    return adj


@pytest.mark.parametrize("n", range(1, 15))
def test_esu_enumeration_equals_combinations(n):
    for k in range(0, min(n, 7) + 2):
        for p in (0.15, 0.35, 0.7):
            adj = random_adj(n, p, n * 100 + k)
            assert U.connected_subsets_esu(adj, k) == U.connected_subsets_comb(adj, k), (n, k, p)


def test_subset_counts_of_the_issue_examples():
    ei = wl.csl_graph(41, 2)
    assert len(U.sorted_masks(U.graph_adjacency(ei[0], ei[1], 0, 41), 6)) == 1312
    ei = wl.tu_graph(64, 300, 3)
    assert len(U.esu_masks(U.graph_adjacency(ei[0], ei[1], 0, 64), 6)) == 2251320


@pytest.mark.parametrize("scen", golden(), ids=lambda s: s[0]["name"])
def test_restatement_reproduces_the_reference(scen):
    s, z = scen
    name = s["name"]
    got = U.sample_batch(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]))
    for nm, a in zip(NAMES, got):
        b = z[f"{name}/{nm}"]
        assert a.shape == b.shape and np.array_equal(a, b), (name, nm)


def test_golden_covers_the_edge_cases():
    z = np.load(GOLDEN + ".npz")
    ptr = z["edge_k4/in_ptr"]
    assert ptr[0] != 0 and np.diff(ptr).min() < 4                      # ptr[0] != 0, a graph with n < k
    assert (z["edge_k4/nodes"][20:40] == -1).all()                      # its rows
    ei = z["edge_k1/in_edge_index"]
    assert (ei[0] == ei[1]).any() and len(z["edge_k1/edge_src"]) > 0   # k = 1 emits a loop
    assert z["edge_k0/nodes"].shape == (9, 0)
