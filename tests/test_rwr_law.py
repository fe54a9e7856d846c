"""CPU checks of the RWR restatement (tests/rwr_law.py): it reproduces every reference fixture (tests/golden/f15_rwr_reference.*),
the counter form of SplitMix64 equals the sequential one, and the speculate / resolve model the device runs finds the same walk
starts as the sequential walk."""
import json
import os
import random

import numpy as np
import pytest

import rwr_law as R
import ugs_workloads as wl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f15_rwr_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def scenarios():
    with open(GOLDEN + ".json") as f:
        return json.load(f)["scenarios"]


@pytest.mark.parametrize("s", scenarios(), ids=lambda s: s["name"])
def test_restatement_reproduces_fixture(s):
    z = np.load(GOLDEN + ".npz")
    name = s["name"]
    got = R.sample_batch(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]), s["p_restart"])
    for nm, a in zip(NAMES, got):
        b = z[f"{name}/{nm}"]
        assert a.shape == b.shape and np.array_equal(a, b), (name, nm)


def test_fixture_covers_the_cases():
    s = {x["name"]: x for x in scenarios()}
    assert any(x["mode"] == "graph" for x in s.values()) and any(x["mode"] == "global" for x in s.values())
    assert {0.0, 1.0} <= {x["p_restart"] for x in s.values()}
    assert s["m0_k5"]["rows"] == 0 and s["small_k4"]["failed_rows"] > 0 and int(s["seed_top_k6"]["seed"]) > (1 << 64) - 8
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    assert meta["omp_num_threads"] == 1 and meta["source_sha256"].startswith("c60c99bb")


def test_counter_form_equals_sequential():
    for seed in (0, 42, (1 << 64) - 1, (1 << 64) - 5, 0x9E3779B97F4A7C15, 123456789):
        rng = R.SplitMix64(seed)
        for i in range(1, 300):
            assert rng.next_u64() == R.draw(seed, i)


def test_splitmix_known_values():
    # SplitMix64 of Steele, Lea and Flood seeded with 0 (the generator's state starts at seed + GAMMA, one step ahead of the
    # published sequence whose first output for seed 0 is 0xe220a8397b1dcdaf)
    assert R.mix(R.GAMMA) == 0xE220A8397B1DCDAF
    assert R.draw((0 - R.GAMMA) & R.M64, 1) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("shape,k,p", [((39, 73), 6, 0.2), ((18, 20), 8, 0.2), ((30, 29), 8, 0.5), ((12, 11), 3, 0.0)])
@pytest.mark.parametrize("window", [1, 7, 64])
def test_speculate_resolve_equals_sequential(shape, k, p, window):
    rnd = random.Random(shape[0] * 7 + k + window)
    for t in range(3):
        ei = wl.tu_graph(shape[0], shape[1], rnd.randrange(1000))
        adj = R.adjacency(ei[0], ei[1], [0, shape[0]])[0]
        gseed = rnd.getrandbits(64)
        want = R.sequential_starts(adj, k, p, gseed, 12)
        assert R.chain_starts(adj, k, p, gseed, 12, window) == want


def test_speculate_resolve_with_small_components():
    # a component smaller than k: walks seeded there run all 10 n k iterations; the chain skips over them the same way
    ei = np.array([[0, 1, 2, 3, 5, 6], [1, 2, 3, 4, 6, 6]], np.int64)
    adj = R.adjacency(ei[0], ei[1], [0, 8])[0]
    for seed in (1, 42):
        want = R.sequential_starts(adj, 4, 0.2, seed, 10)
        assert R.chain_starts(adj, 4, 0.2, seed, 10, 16) == want
        lens = np.diff(want)
        assert (lens >= 1 + 10 * 8 * 4).any()                        # some walk ran to the iteration limit


def test_isolated_seed_length():
    # an isolated vertex without edges: every iteration restarts with one draw, so the walk takes exactly 1 + 10 n k draws
    adj = [[1], [0], []]
    for c in range(200):
        chosen, L = R.walk(adj, 2, 0.2, 5, c)
        if chosen == [2]:
            assert L == 1 + 10 * 3 * 2
            break
    else:
        pytest.fail("no walk seeded at the isolated vertex")
