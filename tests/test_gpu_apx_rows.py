"""GPU: the GPU variant of apx_ugs_sampler (csrc/ugs_apx_gpu.hip) equals tests/apx_gpu_rows.py row for row.

Every trial draws from its own (seed, sample, trial) stream and a sample's row is its accepted trial with the smallest index, so
the rows are a function of (graph, order, seed) that the restatement reproduces; tests/test_apx_gpu_rows.py (CPU) ties the
restatement to apx_oracle.law_k3 and through it to the reference.  Cases: k = 3, 4, 5 on house, kite and a 12-vertex graph with an
isolated vertex id and zero bucket estimates, under a lowered trial cap (UGS_APX_TRIAL_CAP) so that samples drop and the output
compacts; 4100 samples under the full cap (the second slab of 4096 samples); epsilon = 0.1.

Acceptance per trial is tiny (about 3e-6 on house and kite at k = 3, 6.5e-5 on a 6-path, less at k = 4 and 5), and the
restatement runs about 10^5 trials per second at k = 3, 10^4 at k = 4 and 3 * 10^3 at k = 5.  So the caps are sized per k, the
full-cap case uses the path, and every capped case runs with a seed under which at least one sample has an accepted trial
below the cap (found once by scanning seeds 0, 1, 2, ... with the GPU call itself; the test asserts that rows come back, so a
seed that stops producing them fails instead of comparing two empty outputs).  With k = 4 and 5 that reaches the permutation
steps a 2-vertex tail never takes (next_permutation's reversal, links and cut estimates over three or more vertices).

Out of scope: k >= 8, where one trial costs millions of draws (720 permutations x k - 1 cut estimates of up to k x 100 draws);
those k stay on the connectivity and determinism test of tests/test_gpu_apx.py."""
import numpy as np
import pytest

import apx_gpu_rows as ar

GRAPHS = {
    "house": [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 4)],
    "kite": [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (3, 4)],
    # 12 ids: 5 has no column; duplicate columns, a self loop, both directions; several vertices keep a zero estimate
    "twelve": [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 6), (6, 7), (7, 8), (8, 9), (9, 10), (10, 11), (11, 7), (3, 4),
               (4, 3), (9, 9), (1, 0)],
    "path6": [(i, i + 1) for i in range(5)],
}


def call(name, m, k, seed, epsilon, extra_cols=()):
    """one GPU call on GRAPHS[name] (columns ptr[0]:ptr[1] of an edge_index that carries `extra_cols` outside that range)"""
    import torch
    import apx_ugs_sampler
    edges = GRAPHS[name]
    cols = list(extra_cols) + edges + list(extra_cols)
    ei = torch.tensor(cols, dtype=torch.long).t().contiguous()
    ptr = torch.tensor([len(extra_cols), len(extra_cols) + len(edges)])
    s, p, pos, est = apx_ugs_sampler.sample_batch(ei, ptr, m, k, seed=seed, epsilon=epsilon, backend="gpu", return_order=True)
    assert p.tolist() == list(range(s.size(1) + 1))
    return s.t().numpy(), pos.numpy(), est.numpy(), ar.Graph(ei.numpy(), ptr.numpy())


def check_order(name, k, epsilon, pos, est):
    """the order and estimates the call used equal apx_oracle.order's wherever that order is deterministic"""
    import apx_oracle as ao
    edges = GRAPHS[name]
    n = max(max(e) for e in edges) + 1
    try:
        w_pos, w_est = ao.order(ao.adjacency(n, edges), k, epsilon)
    except AssertionError:          # a sampled neighbour fraction close to its threshold: the order is random here
        return False
    assert pos.tolist() == w_pos and est.tolist() == w_est
    return True


# (graph, k, trial cap, samples, seed, rows kept): the seed keeps `rows` of the samples (3 at k = 3, 1 at k = 4 and 5)
CAPPED = [("house", 3, 20000, 12, 16, 3), ("kite", 3, 20000, 12, 14, 3), ("twelve", 3, 20000, 12, 121, 3),
          ("path6", 3, 20000, 40, 14, None),
          ("house", 4, 8000, 8, 8, 1), ("kite", 4, 8000, 8, 8, 1), ("twelve", 4, 8000, 8, 8, 1),
          ("house", 5, 8000, 6, 775, 1), ("kite", 5, 8000, 6, 70, 1), ("twelve", 5, 8000, 6, 5, 1)]


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,k,cap,m,seed,rows", CAPPED)
def test_capped_trials_bit_exact(monkeypatch, name, k, cap, m, seed, rows):
    monkeypatch.setenv("UGS_APX_TRIAL_CAP", str(cap))
    got, pos, est, g = call(name, m, k, seed, 0.9, extra_cols=[(0, 1), (-1, 3)] if name == "twelve" else ())
    check_order(name, k, 0.9, pos, est)
    if name == "twelve":
        assert g.n == 12 and g.deg[5] == 0 and est[5] == 0.0 and ((est == 0.0) & (g.deg > 0)).any()
    want, _ = ar.sample_rows(ar.Params(g, k, 0.9, seed, pos, est, trial_cap=cap), m)
    assert len(want) > 0, f"{name} k={k} seed {seed}: no sample accepted below the cap -- the case would compare nothing"
    assert got.shape == want.shape and np.array_equal(got, want), f"{name} k={k}: got {got.tolist()}, want {want.tolist()}"
    if rows is not None:
        assert len(want) == rows
    else:
        assert 0 < len(got) < m          # samples dropped and the rest compacted


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_cap_second_slab():
    """4100 samples: the second slab of 4096 starts at sample 4096; under the full cap of 10^6 trials no sample of the 6-path
    is dropped (per-trial acceptance 6.5e-5), so row i is sample i"""
    got, pos, est, g = call("path6", 4100, 3, 5, 0.9)
    assert check_order("path6", 3, 0.9, pos, est)
    assert got.shape == (4100, 3)
    rng = np.random.default_rng(1)
    pick = [0, 1, 2, 3, 4094, 4095, 4096, 4097, 4098, 4099] + rng.integers(4, 4094, 5).tolist()
    want = ar.first_accepted(ar.Params(g, 3, 0.9, 5, pos, est), pick)
    for s in pick:
        assert want[s] is not None and tuple(got[s].tolist()) == want[s][1], f"sample {s}: got {got[s].tolist()}, want {want[s]}"


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_epsilon_0_1(monkeypatch):
    monkeypatch.setenv("UGS_APX_TRIAL_CAP", "40000")
    got, pos, est, g = call("path6", 16, 3, 9, 0.1)
    assert check_order("path6", 3, 0.1, pos, est)
    want, _ = ar.sample_rows(ar.Params(g, 3, 0.1, 9, pos, est, trial_cap=40000), 16)
    assert np.array_equal(got, want) and 0 < len(got) < 16, f"got {got.tolist()}, want {want.tolist()}"
