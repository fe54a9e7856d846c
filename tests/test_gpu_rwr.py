"""rwr_sampler (HIP, ugs_rwr.hip) against the reference's outputs (tests/golden/f15_rwr_reference.*) and against the CPU
restatement of its law (tests/rwr_law.py): bit-exact, every tensor."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import rwr_law as R
import ugs_workloads as wl

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f15_rwr_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def sampler():
    import rwr_sampler
    return rwr_sampler


def scenarios():
    with open(GOLDEN + ".json") as f:
        return json.load(f)["scenarios"]


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def call(ei, ptr, m, k, mode="sample", seed=42, p=0.2, device=None):
    e, q = torch.from_numpy(np.ascontiguousarray(ei)), torch.from_numpy(np.asarray(ptr))
    if device is not None:
        e, q = e.to(device), q.to(device)
    return sampler().sample_batch(e, q, m, k, mode=mode, seed=seed, p_restart=p)


@pytest.mark.parametrize("s", scenarios(), ids=lambda s: s["name"])
def test_equals_reference_fixture(s):
    z = np.load(GOLDEN + ".npz")
    name = s["name"]
    got = call(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]), s["p_restart"])
    assert all(t.device.type == "cpu" for t in got)
    assert all(t.is_pinned() for t in got if t.numel())
    assert_same(got, [z[f"{name}/{nm}"] for nm in NAMES], name)


@pytest.mark.parametrize("s", [s for s in scenarios() if s["name"] in ("proteins_k6", "edge_k4_global", "small_k4")],
                         ids=lambda s: s["name"])
def test_device_in_device_out(s):
    z = np.load(GOLDEN + ".npz")
    name = s["name"]
    got = call(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]), s["p_restart"],
               device="cuda:0")
    assert all(t.is_cuda for t in got)
    assert_same(got, [z[f"{name}/{nm}"] for nm in NAMES], name)


def random_batch(rnd):
    """Graphs of 0..20 vertices: TU-shaped, sparse trees, or random multigraphs with loops, duplicates and isolated vertices;
    a few cross-graph columns; ptr starting anywhere."""
    graphs = []
    for _ in range(rnd.randint(1, 12)):
        kind = rnd.random()
        n = rnd.randint(0, 20)
        if n >= 2 and kind < 0.4:
            ei = wl.tu_graph(n, rnd.randint(n - 1, 2 * n), rnd.randrange(10 ** 6))
        elif n >= 1:
            cols = rnd.randint(0, 2 * n)
            ei = np.array([[rnd.randrange(n) for _ in range(cols)], [rnd.randrange(n) for _ in range(cols)]], np.int64).reshape(2, -1)
        else:
            ei = np.zeros((2, 0), np.int64)
        graphs.append((n, ei))
    first = rnd.randint(0, 5)
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1)
    if ptr[-1] > first + 1:
        extra = np.array([[rnd.randrange(first, ptr[-1]) for _ in range(3)], [rnd.randrange(first, ptr[-1]) for _ in range(3)]])
        ei = np.concatenate([ei, extra.astype(np.int64)], axis=1)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


def test_random_batches_equal_restatement():
    rnd = random.Random(2026)
    for t in range(20):
        ei, ptr = random_batch(rnd)
        m, k = rnd.randint(0, 12), rnd.choice([1, 2, 3, 4, 5, 6, 8, 10, 17])
        mode = rnd.choice(["sample", "global", "graph"])
        seed = rnd.getrandbits(64)
        p = rnd.choice([0.0, 0.1, 0.2, 0.5, 1.0])
        assert_same(call(ei, ptr, m, k, mode, seed, p), R.sample_batch(ei, ptr, m, k, mode, seed, p), (t, m, k, mode, seed, p))


def test_large_k_equals_restatement():
    ei, ptr = wl.tu_batch(80, 120, 3, dataset_seed=4)
    for k in (33, 64):
        assert_same(call(ei, ptr, 4, k, "sample", 3, 0.1), R.sample_batch(ei, ptr, 4, k, "sample", 3, 0.1), k)


def test_presample_style_calls():
    # the training loop's presampling: one graph per call, seed + i
    rnd = random.Random(5)
    for i in range(12):
        n = rnd.randint(5, 40)
        ei = wl.tu_graph(n, n + rnd.randint(0, n), i)
        ptr = np.array([0, n], np.int64)
        assert_same(call(ei, ptr, 100, 6, "sample", 42 + i), R.sample_batch(ei, ptr, 100, 6, "sample", 42 + i), i)


def test_large_single_graph():
    # one graph of 5000 vertices, m = 300: several speculation windows, CSR read from global memory
    n = 5000
    ei = wl.tu_graph(n, 6000, 11)
    ei = np.concatenate([ei, np.array([[n - 1, n - 2], [n - 1, n - 2]], np.int64)], axis=1)   # two loops
    ptr = np.array([0, n], np.int64)
    assert_same(call(ei, ptr, 300, 7, "global", 9), R.sample_batch(ei, ptr, 300, 7, "global", 9), "large")


@pytest.mark.parametrize("pairs", [20, 296])
def test_many_doomed_walks(pairs):
    # most vertices sit in components smaller than k (pairs, loops, isolated vertices): the chain meets many walks that run all
    # 10 n k iterations; with 296 pairs (n = 968, T = 38720) measuring one takes several rounds of the block's position scan
    und = [(3 * i, 3 * i + 1) for i in range(pairs)] + [(3 * i + 2, 3 * i + 2) for i in range(0, pairs, 2)]
    ei = np.array([[u for u, _ in und] + [v for _, v in und], [v for _, v in und] + [u for u, _ in und]], np.int64)
    n0 = 3 * pairs
    ei = np.concatenate([ei, wl.tu_graph(8, 7, 3) + n0], axis=1)
    ptr = np.array([0, n0 + 8], np.int64)
    got = call(ei, ptr, 40, 4, "sample", 1)
    want = R.sample_batch(ei, ptr, 40, 4, "sample", 1)
    assert_same(got, want, "doomed")
    assert (want[0][:, 0] < 0).sum() > 20


@pytest.mark.parametrize("bad", ["k0", "k65", "p_neg", "p_big", "p_nan", "m_neg", "empty_ptr", "decreasing_ptr", "overflow",
                                 "ei_dtype", "ptr_dtype"])
def test_limits_raise_and_library_stays_usable(bad):
    ei, ptr = wl.tu_batch(18, 20, 4)
    args = dict(m=8, k=5, p=0.2)
    if bad == "k0":
        args["k"] = 0
    elif bad == "k65":
        args["k"] = 65
    elif bad == "p_neg":
        args["p"] = -0.01
    elif bad == "p_big":
        args["p"] = 1.5
    elif bad == "p_nan":
        args["p"] = math.nan
    elif bad == "m_neg":
        args["m"] = -1
    elif bad == "empty_ptr":
        ptr = np.zeros(0, np.int64)
    elif bad == "decreasing_ptr":
        ptr = ptr.copy()
        ptr[2] = ptr[1] - 1
    elif bad == "overflow":
        ptr = np.array([0, 18, 18 + 40_000_000], np.int64)           # 10 n k > INT_MAX for k = 6
        args["k"] = 6
    if bad == "ei_dtype":
        with pytest.raises(RuntimeError):
            sampler().sample_batch(torch.from_numpy(ei).int(), torch.from_numpy(ptr), 8, 5)
    elif bad == "ptr_dtype":
        with pytest.raises(RuntimeError):
            sampler().sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr).int(), 8, 5)
    else:
        with pytest.raises(RuntimeError):
            call(ei, ptr, args["m"], args["k"], "sample", 42, args["p"])
    ei, ptr = wl.tu_batch(18, 20, 4)
    assert_same(call(ei, ptr, 8, 5, "sample", 42), R.sample_batch(ei, ptr, 8, 5, "sample", 42), "after " + bad)


def test_defaults_and_empty_batch():
    ei, ptr = wl.tu_batch(39, 73, 2)
    got = sampler().sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 5, 6)
    assert_same(got, R.sample_batch(ei, ptr, 5, 6, "sample", 42, 0.2), "defaults")
    got = call(np.zeros((2, 0), np.int64), np.array([3], np.int64), 5, 4)
    assert [tuple(t.shape) for t in got] == [(0, 4), (2, 0), (1,), (1,), (0,)]
    assert got[2].tolist() == [0] and got[3].tolist() == [0]
