"""CPU: the oracle against the reference ITSELF on seeded random inputs.  The reference's outputs for these inputs are
stored in tests/golden/f12_oracle_vs_ref.npz (generator: oracle/make_golden_vs_ref.py, from the reference module built by
oracle/build_ref.py), so the test runs anywhere; where the reference's sources are present, the oracle is also compared
with the reference module live, and the stored outputs with the live ones."""
import os
import random

import numpy as np
import pytest

import oracle

REF_SRC = "/root/reference/src/samplers/ugs_sampler"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f12_oracle_vs_ref.npz")


@pytest.fixture(scope="module")
def ref():
    """the reference module where its sources are present, else None (the stored outputs stand in for it)"""
    if not os.path.isdir(REF_SRC):
        return None
    import torch  # noqa: F401
    import build_ref
    build_ref.build()
    return build_ref.load()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {key: z[key] for key in z.files}


def _rand_graph(rng, n, p, both):
    e = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    if both:
        e = e + [(v, u) for u, v in e]
    return np.array(e, dtype=np.int64).T.reshape(2, -1)


def handle_calls():
    """the seeded handle-API calls: (edge_index, n, k, m, mode, base_offset, seed)"""
    rng = random.Random(2024)
    for _ in range(120):
        n = rng.choice([3, 5, 8, 12, 20, 40, 80, 150])
        ei = _rand_graph(rng, n, rng.choice([0.05, 0.1, 0.2, 0.4, 0.6]), rng.random() < 0.5)
        k, m = rng.randint(1, 8), rng.choice([1, 5, 50])
        seed = rng.choice([42, 0, 7, -5, 123456789])
        mode, bo = rng.choice(["local", "flat", "global"]), rng.choice([0, 10])
        yield ei, n, k, m, mode, bo, seed


def batch_calls():
    """the seeded sample_batch calls, in order (the process-global LRU, whose key ignores k, evolves with them)"""
    rng = random.Random(99)
    for _ in range(150):
        G = rng.randint(1, 6)
        cols, ptr = [], [0]
        for _g in range(G):
            n = rng.choice([0, 1, 2, 3, 5, 8, 12, 20, 40])
            off = ptr[-1]
            e = [(u + off, v + off) for u in range(n) for v in range(u + 1, n) if rng.random() < rng.choice([0.1, 0.3, 0.7])]
            if n and rng.random() < 0.2:
                e.append((off + rng.randrange(n),) * 2)
            if rng.random() < 0.5:
                e = e + [(v, u) for u, v in e]
            cols += e
            ptr.append(off + n)
        if rng.random() < 0.3:
            rng.shuffle(cols)
        ei = np.array(cols, dtype=np.int64).T.reshape(2, -1)
        ptr = np.array(ptr, dtype=np.int64)
        m, k = rng.choice([1, 2, 7, 33]), rng.randint(1, 7)
        mode, seed = rng.choice(["sample", "graph", "global"]), rng.choice([42, 0, -5, 99991])
        yield ei, ptr, m, k, mode, seed


def run_handle_call(ref, call):
    """the reference's answer to one handle-API call: (info as float64 [num_nodes, num_edges_stored, Z, bucket_count_nonzero,
    has_graphlets], its four output tensors)"""
    import torch
    ei, n, k, m, mode, bo, seed = call
    h = ref.create_preproc(torch.from_numpy(ei), n, k)
    info = ref.get_preproc_info(h)
    info = np.array([info["num_nodes"], info["num_edges_stored"], info["Z"], info["bucket_count_nonzero"], bool(ref.has_graphlets(h))], dtype=np.float64)
    out = [x.numpy() for x in ref.sample(h, m, k, mode, bo, seed)]
    ref.destroy_preproc(h)
    return info, out


def run_batch_call(ref, call):
    import torch
    ei, ptr, m, k, mode, seed = call
    return [x.numpy() for x in ref.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode, seed)]


def _same(want, got):
    assert len(want) == len(got)
    for a, b in zip(want, got):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_handle_api_random(ref, golden):
    for i, call in enumerate(handle_calls()):
        ei, n, k, m, mode, bo, seed = call
        info = golden[f"h{i}_info"]
        want = [golden[f"h{i}_{j}"] for j in range(4)]
        if ref is not None:
            live_info, live = run_handle_call(ref, call)
            assert np.array_equal(live_info, info)
            _same(live, want)
        P = oracle.Preproc(ei, n, k)
        oi = P.info()
        assert (oi["num_nodes"], oi["num_edges_stored"], oi["Z"], oi["bucket_count_nonzero"]) == tuple(float(x) for x in info[:4])
        assert oi["has_graphlets"] == bool(info[4])
        _same(want, P.sample(m, k, mode, bo, seed))
        P.close()


def test_sample_batch_random_shared_cache(ref, golden):
    """same call sequence on both sides so the process-global LRU (key ignores k) evolves identically."""
    cache = oracle.Cache(1000)
    for i, call in enumerate(batch_calls()):
        ei, ptr, m, k, mode, seed = call
        want = [golden[f"b{i}_{j}"] for j in range(5)]
        if ref is not None:
            _same(run_batch_call(ref, call), want)
        got = oracle.sample_batch(ei, ptr, m, k, mode, seed, cache=cache)
        _same(want, got)
