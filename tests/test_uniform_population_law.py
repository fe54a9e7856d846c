"""CPU: the 16-lane ordered fill of the population cache's row kernels (ugs_uniform.hip, uni_pop_fill / uni_wpop_fill), restated in
Python (tests/uniform_population_cases.py: chunks of 16 columns, one hit per lane, exclusive prefix, running offset), gives the
edges of the law (tests/uniform_law.py) -- and each one-line mistake in it does not, on the very batch the GPU test samples."""
import random

import numpy as np
import pytest

import ugs_workloads as wl
import uniform_law as U
import uniform_population_cases as P

MUTANTS = ("inclusive", "no_carry", "tail")


def same_edges(model, law):
    return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(model, (law[1], law[2], law[4])))


def test_group_fill_keeps_bucket_order_on_random_hit_patterns():
    rng = random.Random(3)
    for n in list(range(0, 40)) + [47, 48, 49, 300]:
        for density in (0.0, 0.1, 0.5, 1.0):
            hits = [rng.random() < density for _ in range(n)]
            assert P.group_fill(hits) == [q for q in range(n) if hits[q]], (n, density)


@pytest.mark.parametrize("case", range(8))
def test_model_equals_the_law_on_random_buckets(case):
    rng = random.Random(4100 + case)
    graphs = []
    for _ in range(rng.randint(1, 6)):
        n = rng.choice([1, 2, 5, 9, 17, 30])
        e = wl.tu_graph(n, n - 1 + rng.randint(0, 2 * n), rng.randrange(1 << 30)) if n > 1 else np.zeros((2, 0), np.int64)
        dup = e[:, [rng.randrange(e.shape[1]) for _ in range(rng.randint(0, 20))]] if e.shape[1] else e
        loops = np.array([[v, v] for v in range(0, n, 3)], np.int64).T.reshape(2, -1)
        graphs.append((n, np.concatenate([e, dup[::-1], loops], axis=1)))
    cols, ptr = [], [rng.randint(0, 4)]
    for n, e in graphs:
        cols.append(e + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1)
    ei = ei[:, rng.sample(range(ei.shape[1]), ei.shape[1])]
    k, m, mode = 1 + case % 4, (1, 7)[case % 2], ("sample", "global")[case // 4]
    law = U.sample_batch(ei, ptr, m, k, mode, 99 + case)
    assert same_edges(P.model_edges(ei, ptr, law[0], m, mode), law)


@pytest.mark.parametrize("k", [2, 3])
def test_model_equals_the_law_and_every_mutant_differs_on_the_gpu_tests_batch(k):
    _, ei, ptr = P.lane_group_batch()
    assert len(ptr) - 1 == 40
    sizes = [int(((ei[0] >= ptr[g]) & (ei[0] < ptr[g + 1]) & (ei[1] >= ptr[g]) & (ei[1] < ptr[g + 1])).sum()) for g in range(8)]
    assert tuple(sizes[:7]) == P.BUCKETS and sizes[7] == 48
    law = U.sample_batch(ei, ptr, 7, k, "sample", 42)
    assert same_edges(P.model_edges(ei, ptr, law[0], 7, "sample"), law)
    for mutant in MUTANTS:
        assert not same_edges(P.model_edges(ei, ptr, law[0], 7, "sample", mutant), law), mutant


def test_the_last_lane_bucket_has_its_hits_in_lane_15_only():
    n, e = P.last_lane_graph()
    law = U.sample_batch(e, np.array([0, n]), 3, 2, "global", 5)
    assert (law[0] == [0, 1]).all() and law[4].tolist() == [15, 31, 47] * 3
    assert all(c % P.LANES == P.LANES - 1 for c in law[4].tolist())
