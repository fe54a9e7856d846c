"""CPU: tests/apx_gpu_rows.py, the restatement of the GPU variant of apx_ugs_sampler, against the reference's law.

tests/test_gpu_apx_rows.py holds the GPU rows to the restatement; here the restatement's own rows follow apx_oracle.law_k3 (the
enumerated k = 3 law of the reference's algorithm, pinned against the sequential restatement in tests/test_apx_law.py)."""
import collections

import numpy as np
import pytest

import apx_gpu_rows as ar
import apx_oracle as ao


@pytest.mark.timeout(120)
def test_restated_rows_follow_the_k3_law():
    """the restatement's rows against apx_oracle.law_k3 on the 6-path (house accepts ~3e-6 of its trials, 20 times fewer:
    a law test there costs minutes of numpy)"""
    edges = [(i, i + 1) for i in range(5)]
    adj = ao.adjacency(6, edges)
    pos, est = ao.order(adj, 3, 0.9)
    law, acc = ao.law_k3(adj, pos, est, 0.9)
    P = ar.Params(ar.Graph(np.array(edges).T, [0, len(edges)]), 3, 0.9, 7, pos, est)
    rows, trials = ar.sample_rows(P, 150)
    assert len(rows) == 150
    counts = collections.Counter(tuple(r) for r in rows.tolist())
    pval, chi2, dof = ao.chi_square_p(counts, law)
    assert pval > 1e-4, f"chi2 {chi2:.1f} on {dof} dof, p = {pval:.2e}; counts {dict(counts)}"
    # the first accepted trial index is geometric with the law's per-trial acceptance
    assert abs(np.mean(trials) * acc - 1.0) < 0.3
