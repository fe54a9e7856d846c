"""CPU: tests/eps_rows.py, the bit-exact restatement of the HIP epsilon_uniform_sampler, against the reference's law.

tests/test_gpu_eps_rows.py holds the GPU outputs to this restatement bit for bit; here the restatement's own rows are held to
oracle/eps_oracle.sample_law (the enumerated law of the reference's algorithm, pinned against the reference itself in
tests/test_eps_oracle.py), so that equality with the restatement means equality with an implementation of the reference's
law.  Known-answer checks cover the generator pieces a law test cannot see: below()'s rejection branch and unit()."""
import numpy as np
import pytest

import eps_oracle
import eps_rows
from test_eps_oracle import CASES, GRAPHS, check_rows_against_law


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("k,eps", CASES)
def test_restated_rows_follow_the_reference_law(name, k, eps):
    n, cols = GRAPHS[name]
    law, p_fail = eps_oracle.sample_law(eps_oracle.adjacency(cols, n), n, k, eps)
    adj = eps_oracle.adjacency(cols, n)
    rows = np.array([eps_rows.walk_row(adj, n, k, eps, 99, r) or [-1] * k for r in range(12000)], dtype=np.int64)
    check_rows_against_law(rows, law, p_fail, f"restatement {name} k={k} eps={eps}")


def test_whole_call_format():
    """sample_rows on a two-graph batch: pointers, failed rows, edges = expected_edges with batch column ids, both modes"""
    n, cols = GRAPHS["house"]
    ei = np.array(cols + [(u + 7, v + 7) for u, v in cols] + [(1, 8)], dtype=np.int64).T     # last column crosses graphs
    ptr = np.array([0, 5, 7, 12])
    for mode in ("sample", "global"):
        nodes, eidx, eptr, sptr, esrc = eps_rows.sample_rows(ei, ptr, 30, 3, mode, 5, 0.3)
        assert nodes.shape == (90, 3) and sptr.tolist() == [0, 30, 60, 90] and eptr[0] == 0 and eptr[-1] == eidx.shape[1] == len(esrc)
        assert (nodes[30:60] == -1).all() and (np.diff(eptr)[30:60] == 0).all()
        for r in list(range(30)) + list(range(60, 90)):
            lo = 0 if r < 30 else 7
            if nodes[r, 0] < 0:
                continue
            local = [int(x) - lo for x in nodes[r]]
            want = eps_oracle.expected_edges(cols, local, mode, lo)
            off = 0 if r < 30 else 6
            got = list(zip(eidx[0, eptr[r]:eptr[r + 1]].tolist(), eidx[1, eptr[r]:eptr[r + 1]].tolist(), esrc[eptr[r]:eptr[r + 1]].tolist()))
            assert got == [(a, b, e + off) for a, b, e in want]
        # rows of the two copies of the house are walks of their own rows, not copies of each other
        assert not np.array_equal(nodes[:30] , nodes[60:] - 7)


def test_generator_known_answers():
    assert eps_rows.mix64(0) == 0xE220A8397B1DCDAF                      # splitmix64's first output for seed 0
    # unit(): the top 53 bits of the next output, scaled by 2^-53
    g = eps_rows.CRng(1, 2, 3)
    s0 = g.s
    x = s0 ^ (s0 >> 12)
    x ^= (x << 25) & eps_rows.MASK
    x ^= x >> 27
    want = ((x * 2685821657736338717) & eps_rows.MASK) >> 11
    assert g.unit() == want / 2.0 ** 53 and 0.0 <= want / 2.0 ** 53 < 1.0


def _draws(rng, count):
    return [rng.next() >> 32 for _ in range(count)]


def test_below_rejection_branch():
    """below(n) with n = 3 * 10^9 (2^32 mod n = 1294967296, so about 30 % of first draws are rejected): a rejected draw is
    replaced by the next one, as often as needed; an accepted low half is never redrawn"""
    n = 3_000_000_000
    t = (1 << 32) % n
    rejected = accepted = 0
    for row in range(400):
        probe, g = eps_rows.CRng(7, row, 0), eps_rows.CRng(7, row, 0)
        d = _draws(probe, 8)
        i = 0
        while ((d[i] * n) & 0xFFFFFFFF) < t:
            i += 1
        assert g.below(n) == (d[i] * n) >> 32
        rejected += i > 0
        accepted += i == 0
    assert rejected > 50 and accepted > 50
    # numpy restatement agrees, and first_draw_rejected finds exactly the rows with a rejected first draw
    rows = np.arange(400)
    s = eps_rows.init_np(7, rows, 0)
    got = eps_rows.below_np(s, n, np.ones(400, bool))
    assert got.tolist() == [eps_rows.CRng(7, r, 0).below(n) for r in range(400)]
    rej = set(eps_rows.first_draw_rejected(7, rows, n).tolist())
    assert rej == {r for r in range(400) if ((_draws(eps_rows.CRng(7, r, 0), 1)[0] * n) & 0xFFFFFFFF) < t}


def test_vectorised_k1_equals_row_walks():
    """k1_rows (numpy) against the per-row walk on a graph with self loops of several multiplicities, both modes"""
    n = 11
    loops = [(3, 0), (5, 2), (3, 4), (7, 5), (3, 6), (0, 8)]      # (vertex, column)
    ei = np.zeros((2, 9), np.int64)
    for v, j in loops:
        ei[:, j] = v
    ei[:, 1] = (1, 2); ei[:, 3] = (2, 4); ei[:, 7] = (9, 10)      # other columns give no edge at k = 1
    for eps in (1.0, 0.003):
        for mode in ("sample", "global"):
            want = eps_rows.sample_rows(ei + 4, [4, 4 + n], 3000, 1, mode, 11, eps)
            nodes, eptr, eidx, esrc = eps_rows.k1_rows(n, loops, 3000, eps, 11, node_lo=4, mode=mode)
            assert np.array_equal(nodes, want[0][:, 0]) and np.array_equal(eptr, want[2])
            assert np.array_equal(eidx, want[1]) and np.array_equal(esrc, want[4])


def test_csr_adjacency_keeps_the_oracle_order():
    rng = np.random.default_rng(3)
    cols = rng.integers(0, 30, size=(200, 2))
    cols[::17, 1] = cols[::17, 0]                       # self loops
    cols[5::23] = cols[4::23][: len(cols[5::23])]       # duplicate columns
    csr = eps_rows.CsrAdj(cols, 30)
    want = eps_oracle.adjacency([tuple(c) for c in cols.tolist()], 30)
    assert [csr[u] for u in range(30)] == want
    nodes = sorted({int(x) for x in cols[:6].ravel()})
    assert csr.edges(nodes, "sample", 0) == eps_oracle.expected_edges([tuple(c) for c in cols.tolist()], nodes, "sample")
    assert csr.edges(nodes, "global", 9) == eps_oracle.expected_edges([tuple(c) for c in cols.tolist()], nodes, "global", 9)
