"""GPU: walks built to take the table final's leader fast path (stage_final: the target is its bucket's first arrival) and its
general path at high rates, every output against the CPU oracle.  Vertex ids that collide modulo the chain's bucket counts
13 / 29 / 59 / 127 / 257 make shared buckets -- and removals of their leaders -- common; degree-40 ER graphs at k = 8 and k = 12
are the benchmark's shape with candidate lists of up to ~450."""
import numpy as np
import pytest

import scenarios as sc
import ugs_workloads as wl

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


@pytest.fixture(scope="module")
def product():
    from backends import ProductBackend
    return ProductBackend()


@pytest.fixture(scope="module")
def orc():
    from backends import OracleBackend
    return OracleBackend()


def _same(calls, product, orc, what):
    got = sc.run_scenario(calls, product)
    want = sc.run_scenario(calls, orc)
    for i, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, tuple) and isinstance(w, tuple) and not isinstance(g[0], str), f"{what}: call {i}: {g!r}"
        for j, (a, b) in enumerate(zip(g, w)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{what}: call {i} output {j} differs"


def _colliding_ids(rng, n_vertices):
    """ids congruent to a few residues modulo 13 * 29, 59 * 127 and 257: most of a walk's candidates share buckets"""
    ids = set()
    for mod in (13 * 29, 59 * 127, 257, 13 * 59):
        j = rng.integers(0, n_vertices // mod, size=400)
        ids.update((j * mod + rng.integers(0, 3, size=j.size)).tolist())
    return np.array(sorted(x for x in ids if x < n_vertices), dtype=np.int64)


@pytest.mark.parametrize("k", [8, 12])
@pytest.mark.parametrize("mode", ["sample", "global"])
def test_colliding_vertex_ids_vs_oracle(k, mode, product, orc):
    rng = np.random.default_rng(1000 + k)
    nv = 400_000
    ids = _colliding_ids(rng, nv)
    deg = 40
    src = rng.choice(ids, size=ids.size * deg // 2)
    dst = rng.choice(ids, size=src.size)
    ei = np.stack([src, dst]).astype(np.int64)
    calls = [dict(fn="sample_batch", edge_index=ei, ptr=np.array([0, nv], dtype=np.int64), m=3000, k=k, mode=mode, seed=s)
             for s in (7, 123456789)]
    _same(calls, product, orc, f"colliding ids, k={k}, {mode}")


@pytest.mark.parametrize("k", [8, 12])
def test_degree_40_er_vs_oracle(k, product, orc):
    ei, ptr = wl.er_graph(20_000, 400_000, 5)
    calls = [dict(fn="sample_batch", edge_index=ei, ptr=ptr, m=6000, k=k, mode="sample", seed=s) for s in (42, -9)]
    _same(calls, product, orc, f"degree-40 ER, k={k}")
