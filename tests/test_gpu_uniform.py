"""uniform_sampler (HIP, ugs_uniform.hip) against the reference's outputs (tests/golden/f14_uniform_reference.*) and against the
CPU restatement of its law (tests/uniform_law.py): bit-exact, every tensor."""
import json
import os
import random

import numpy as np
import pytest
import torch

import ugs_workloads as wl
import uniform_law as U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f14_uniform_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def sampler():
    import uniform_sampler
    return uniform_sampler


def scenarios():
    with open(GOLDEN + ".json") as f:
        return json.load(f)["scenarios"]


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def call(ei, ptr, m, k, mode="sample", seed=42, device=None):
    e, p = torch.from_numpy(np.ascontiguousarray(ei)), torch.from_numpy(np.asarray(ptr))
    if device is not None:
        e, p = e.to(device), p.to(device)
    return sampler().sample_batch(e, p, m, k, mode=mode, seed=seed)


@pytest.mark.parametrize("s", scenarios(), ids=lambda s: s["name"])
def test_equals_reference_fixture(s):
    z = np.load(GOLDEN + ".npz")
    name = s["name"]
    got = call(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]))
    assert all(t.device.type == "cpu" for t in got)
    if torch.cuda.is_available():
        assert all(t.is_pinned() for t in got if t.numel() > 0)      # (torch does not pin empty tensors)
    assert_same(got, [z[f"{name}/{nm}"] for nm in NAMES], name)


def random_batch(rng, G):
    graphs = []
    for _ in range(G):
        n = rng.choice([1, 2, 3, 5, 8, 13, 18, 28, 40, 64]) if rng.random() < 0.8 else rng.randint(1, 64)
        extra = rng.randint(0, n // 4 + 1) if n > 30 else rng.randint(0, n)
        graphs.append((n, wl.tu_graph(n, n - 1 + extra, rng.randrange(1 << 30)) if n > 1 else np.zeros((2, 0), np.int64)))
    cols, ptr = [], [rng.randint(0, 3)]
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1)
    perm = np.array(rng.sample(range(ei.shape[1]), ei.shape[1]), dtype=np.int64)   # columns in any order
    return ei[:, perm], np.array(ptr, np.int64)


@pytest.mark.parametrize("case", range(12))
def test_equals_restatement_on_random_batches(case):
    rng = random.Random(1000 + case)
    ei, ptr = random_batch(rng, rng.randint(1, 12))
    k = 1 + case % 8
    m = [0, 1, 7, 100][case % 4]
    mode = "sample" if case % 3 else "global"
    seed = rng.getrandbits(64)
    want = U.sample_batch(ei, ptr, m, k, mode, seed)
    # a strided view: rows of a wider buffer (row stride != columns)
    wide = torch.full((2, ei.shape[1] + 7), -5, dtype=torch.int64)
    wide[:, :ei.shape[1]] = torch.from_numpy(ei)
    got = sampler().sample_batch(wide[:, :ei.shape[1]], torch.from_numpy(ptr), m, k, mode=mode, seed=seed)
    assert_same(got, want, f"case {case}")


def test_equals_restatement_on_csl_k7():
    graphs = [(41, wl.csl_graph(41, s)) for s in (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)]
    cols, ptr = [], [0]
    for n, e in graphs:
        cols.append(e + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei, ptr = np.concatenate(cols, axis=1), np.array(ptr, np.int64)
    assert_same(call(ei, ptr, 100, 7, "sample", 42), U.sample_batch(ei, ptr, 100, 7, "sample", 42), "csl k7")


def test_equals_restatement_on_large_root_buckets():
    """tu_graph(64, 300, 3), k = 6: 2 251 320 connected subsets, largest root bucket 343 139 keys -- sorted outside LDS."""
    ei = wl.tu_graph(64, 300, 3)
    ptr = np.array([0, 64], np.int64)
    masks = U.esu_masks(U.graph_adjacency(ei[0], ei[1], 0, 64), 6)
    roots = np.bincount([(x & -x).bit_length() - 1 for x in masks])
    assert len(masks) == 2251320 and roots.max() == 343139
    for mode, seed in (("sample", 42), ("global", 7)):
        assert_same(call(ei, ptr, 200, 6, mode, seed), U.sample_batch(ei, ptr, 200, 6, mode, seed), mode)


def test_device_in_equals_cpu_in_and_stays_on_device():
    ei, ptr = wl.tu_batch(18, 20, 16)
    host = call(ei, ptr, 64, 5, "sample", 3)
    dev = call(ei, ptr, 64, 5, "sample", 3, device="cuda:0")
    assert all(t.is_cuda and t.device.index == 0 for t in dev)
    assert_same(dev, [t.numpy() for t in host], "device in")


def test_seed_determinism():
    ei, ptr = wl.tu_batch(18, 20, 8)
    a, b, c = call(ei, ptr, 32, 4, seed=11), call(ei, ptr, 32, 4, seed=11), call(ei, ptr, 32, 4, seed=12)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])


def check_recovers():
    ei, ptr = wl.tu_batch(18, 20, 4)
    assert_same(call(ei, ptr, 16, 4, "sample", 5), U.sample_batch(ei, ptr, 16, 4, "sample", 5), "after an error")


def complete_graph(n):
    u, v = np.triu_indices(n, 1)
    return np.array([np.r_[u, v], np.r_[v, u]], np.int64)


@pytest.mark.parametrize("bad", ["int32", "k<0", "m<0", "decreasing", "empty_ptr", "65_vertices", "over_budget"])
def test_errors_raise_and_leave_the_library_usable(bad):
    ei, ptr = wl.tu_batch(18, 20, 2)
    e, p, m, k = torch.from_numpy(ei), torch.from_numpy(ptr), 4, 3
    if bad == "int32":
        e = e.int()
    elif bad == "k<0":
        k = -1
    elif bad == "m<0":
        m = -1
    elif bad == "decreasing":
        p = torch.tensor([0, 18, 10, 36])
    elif bad == "empty_ptr":
        p = torch.zeros(0, dtype=torch.int64)
    elif bad == "65_vertices":
        e, p = torch.from_numpy(wl.tu_graph(65, 70, 1)), torch.tensor([0, 65])
    elif bad == "over_budget":                                    # 2 x C(64, 6) = 150 M connected 6-subsets
        kg = complete_graph(64)
        e, p, k = torch.from_numpy(np.concatenate([kg, kg + 64], axis=1)), torch.tensor([0, 64, 128]), 6
    with pytest.raises(RuntimeError):
        sampler().sample_batch(e, p, m, k)
    check_recovers()


def test_small_graphs_below_k_are_fine_next_to_large_ones():
    """A 100-vertex graph is allowed when it has fewer than k vertices; here k = 101: every row is -1."""
    ei = np.concatenate([wl.tu_graph(100, 120, 1), wl.tu_graph(10, 12, 2) + 100], axis=1)
    ptr = np.array([0, 100, 110], np.int64)
    got = call(ei, ptr, 3, 101)
    assert (got[0].numpy() == -1).all() and got[1].shape == (2, 0)
