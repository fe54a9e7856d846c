"""CPU checks of tests/uniform_wide_law.py: the law on graphs of more than 64 vertices reproduces the reference's own outputs
(tests/golden/f18_uniform_wide_reference.*), the enumeration equals the literal definition, and the wide key keeps the order."""
import itertools
import json
import os
import random

import numpy as np
import pytest

import ugs_workloads as wl
import uniform_law as U
import uniform_wide_law as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f18_uniform_wide_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def scenarios():
    with open(GOLDEN + ".json") as f:
        return json.load(f)["scenarios"]


@pytest.mark.parametrize("s", scenarios(), ids=lambda s: s["name"])
def test_law_reproduces_the_reference(s):
    z = np.load(GOLDEN + ".npz")
    name = s["name"]
    got = W.sample_batch(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]))
    for nm, a in zip(NAMES, got):
        b = z[f"{name}/{nm}"]
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), (name, nm)


def test_fixture_covers_what_it_should():
    sc = scenarios()
    z = np.load(GOLDEN + ".npz")
    assert {s["seed"] for s in sc} >= {"0", "42", str((1 << 64) - 1)}
    assert {s["mode"] for s in sc} >= {"sample", "global"}
    sizes = {int(n) for s in sc for n in np.diff(z[s["name"] + "/in_ptr"])}
    assert {65, 100, 129, 136, 300, 1024, 14, 64} <= sizes
    assert any(z[s["name"] + "/in_ptr"][0] == 5 for s in sc)
    for s in sc:                                                    # no placeholder rows: every graph here has connected k-subsets
        assert (z[s["name"] + "/nodes"] >= 0).all(), s["name"]


@pytest.mark.parametrize("n", [65, 66, 67, 68, 69, 70])
def test_sorted_tuples_equals_the_literal_definition(n):
    ei = wl.tu_graph(n, n + 6, n)
    adj = U.graph_adjacency(ei[0], ei[1], 0, n)
    want = U.connected_subsets_comb(adj, 3)
    assert len(want) > n and W.sorted_tuples(adj, 3) == want


@pytest.mark.parametrize("n,k,bits", [(128, 6, 7), (129, 6, 8), (1024, 6, 10), (256, 8, 8), (65, 1, 7), (512, 7, 9)])
def test_key_order_is_tuple_order_at_the_field_width_edges(n, k, bits):
    assert W.field_bits(n) == bits and W.takes_wide_form(n, k, 1024)
    rng = random.Random(n * 10 + k)
    edge = [0, 1, 2, n // 2, n - 3, n - 2, n - 1, 63, 64, 65, 127, 128]
    tuples = {tuple(sorted(rng.sample(range(n), k))) for _ in range(400)}
    tuples |= {t for t in itertools.combinations(sorted({v for v in edge if v < n}), k)} if k <= 6 else set()
    tuples |= {tuple(range(k)), tuple(range(n - k, n))}
    tuples = sorted(tuples)
    keys = [W.tuple_key(t, n) for t in tuples]
    assert all(0 <= x < 1 << 64 for x in keys)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    if (n, k) in ((256, 8), (1024, 6)):
        assert max(keys).bit_length() == k * bits                   # the top field reaches the key's last bit: 64 of 64, 60 of 64


def test_the_rule_table():
    for k, top in ((1, 1024), (6, 1024), (7, 512), (8, 256)):
        assert W.takes_wide_form(top, k, 1024) and not W.takes_wide_form(top + 1, k, 1024)
    assert not W.takes_wide_form(64, 3, 1024) and not W.takes_wide_form(200, 3, 128) and not W.takes_wide_form(100, 9, 1024)
    assert not W.takes_wide_form(300, 8, 1024)                      # k b = 72
