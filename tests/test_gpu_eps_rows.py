"""GPU: the HIP epsilon_uniform_sampler (csrc/ugs_eps.hip) equals tests/eps_rows.py bit for bit.

The kernel is deterministic in (seed, row, attempt), so every output tensor -- nodes, edge_index, edge_ptr, sample_ptr,
edge_src -- is predicted by the restatement, which tests/test_eps_rows.py ties to the reference's law.  Beyond the law tests of
tests/test_gpu_eps.py this reaches: k up to UGS_KMAX = 32 (the last LDS slot), batches with shuffled / duplicate / looping /
cross-graph / out-of-range columns and empty or too-small graphs, a row count past one sweep of the capped walk grid with
below()'s rejection branch firing, and every path of the edge_ptr scan (one block up to 16 384 rows, two launches up to
8 388 608 rows, three launches beyond)."""
import numpy as np
import pytest

import eps_rows
from test_eps_oracle import GRAPHS

pytestmark = [pytest.mark.gpu]

MODES = ("sample", "global")


@pytest.fixture(scope="module")
def eps():
    import epsilon_uniform_sampler
    return epsilon_uniform_sampler


def call(eps, ei, ptr, m, k, mode, seed, epsilon, device=None):
    import torch
    ei_t = ei if isinstance(ei, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ei))
    ptr_t = torch.from_numpy(np.asarray(ptr, dtype=np.int64))
    if device is not None:
        ei_t, ptr_t = ei_t.to(device), ptr_t.to(device)
    out = eps.sample_batch(ei_t, ptr_t, m, k, mode, seed, epsilon)
    return [t.cpu().numpy() for t in out]


def assert_same(got, want, what):
    for name, a, b in zip(("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src"), got, want):
        assert a.shape == b.shape, f"{what}: {name} shape {a.shape} != {b.shape}"
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)[:5].tolist()
            raise AssertionError(f"{what}: {name} differs at {bad}")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("k,epsilon", [(3, 0.1), (4, 0.5), (3, 0.01), (5, 1.0)])
def test_fixture_graphs_bit_exact(eps, name, k, epsilon):
    n, cols = GRAPHS[name]
    ei = np.array(cols, dtype=np.int64).T
    for mode in MODES:
        got = call(eps, ei, [0, n], 1500, k, mode, 99, epsilon)
        assert_same(got, eps_rows.sample_rows(ei, [0, n], 1500, k, mode, 99, epsilon), f"{name} k={k} eps={epsilon} {mode}")


def tu_messy_batch(seed):
    """a TU-shaped batch with every column oddity the host must sort out: ptr[0] > 0, an empty graph, graphs smaller than k,
    columns shuffled and in both directions, duplicate columns, self loops, columns crossing graphs, columns outside
    [ptr[0], ptr[G])"""
    import ugs_workloads as wl
    rng = np.random.default_rng(seed)
    sizes = [18, 0, 2, 25, 5, 1, 39, 9]
    ptr = [3]
    cols = []
    for g, n in enumerate(sizes):
        lo = ptr[-1]
        if n >= 2:
            cols.append(wl.tu_graph(n, int(n * 1.2), seed * 31 + g) + lo)
        ptr.append(lo + n)
    ei = np.concatenate(cols, axis=1)
    ei = np.concatenate([ei, ei[:, rng.integers(0, ei.shape[1], 20)]], axis=1)                 # duplicates
    loops = rng.integers(ptr[0], ptr[-1], 12)
    ei = np.concatenate([ei, np.stack([loops, loops]), np.stack([loops[:4], loops[:4]])], axis=1)   # loops, repeated
    cross = np.array([[3, 21, 50, 70], [50, 60, 3, 100]])                                         # endpoints in two graphs
    outside = np.array([[0, 1, 5, ptr[-1], ptr[-1] + 4, -1], [5, 2, 0, 8, ptr[-1] + 1, 7]])       # below ptr[0], past ptr[G]
    ei = np.concatenate([ei, cross, outside], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    return np.ascontiguousarray(ei), np.array(ptr, dtype=np.int64)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", range(1, 9))
def test_tu_batches_bit_exact(eps, k):
    import torch
    ei, ptr = tu_messy_batch(k)
    for m in (0, 1, 7, 100):
        for mode in MODES:
            want = eps_rows.sample_rows(ei, ptr, m, k, mode, 1000 + k, 0.3)
            got = call(eps, ei, ptr, m, k, mode, 1000 + k, 0.3)
            assert_same(got, want, f"k={k} m={m} {mode}")
    # a strided view: edge_index rows 0 and 2 of a [3, E + 5] buffer (row stride E + 5, unit column stride)
    E = ei.shape[1]
    buf = torch.full((3, E + 5), -7, dtype=torch.int64)
    buf[0, :E] = torch.from_numpy(ei[0])
    buf[2, :E] = torch.from_numpy(ei[1])
    view = buf[0::2, :E]
    assert view.stride() == (2 * (E + 5), 1)
    got = call(eps, view, ptr, 7, k, "global", 5, 0.1)
    assert_same(got, eps_rows.sample_rows(ei, ptr, 7, k, "global", 5, 0.1), f"k={k} strided view")
    # a view with a non-unit column stride (the wrapper copies it)
    wide = torch.from_numpy(np.repeat(ei, 2, axis=1))[:, ::2]
    got = call(eps, wide, ptr, 7, k, "sample", 5, 0.1)
    assert_same(got, eps_rows.sample_rows(ei, ptr, 7, k, "sample", 5, 0.1), f"k={k} column-strided view")


@pytest.mark.timeout(300)
def test_epsilon_values_and_failing_rows(eps):
    ei, ptr = tu_messy_batch(11)
    for epsilon in (1.0, 0.3, 0.1, 0.003):
        assert eps_rows.max_attempts(epsilon) == {1.0: 10, 0.3: 33, 0.1: 100, 0.003: 3333}[epsilon]
        for mode in MODES:
            assert_same(call(eps, ei, ptr, 60, 5, mode, 3, epsilon), eps_rows.sample_rows(ei, ptr, 60, 5, mode, 3, epsilon),
                        f"eps={epsilon} {mode}")
    # most rows fail: one 5-path among 195 isolated vertices gives an attempt about a 2.5 % chance; eps = 1 allows 10 attempts
    # (at any epsilon an attempt that completes is accepted with probability eps / (w + eps), and 10 / eps attempts make
    # a failed row rare whenever most walks complete -- failing rows come from walks that die)
    ei = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=np.int64) + 70
    for mode in MODES:
        got = call(eps, ei, [10, 210], 400, 5, mode, 8, 1.0)
        assert_same(got, eps_rows.sample_rows(ei, [10, 210], 400, 5, mode, 8, 1.0), f"failing rows {mode}")
        failed = int((got[0][:, 0] < 0).sum())
        assert 200 < failed < 400, failed


@pytest.mark.timeout(300)
def test_k32_last_lds_slot(eps):
    import torch
    import ugs_workloads as wl
    sizes = [40, 64, 31, 52]
    cols, ptr = [], [0]
    for g, n in enumerate(sizes):
        cols.append(wl.tu_graph(n, int(n * 1.5), 77 + g) + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.ascontiguousarray(np.concatenate(cols, axis=1))
    for mode in MODES:
        got = call(eps, ei, ptr, 40, 32, mode, 4, 0.3)
        want = eps_rows.sample_rows(ei, ptr, 40, 32, mode, 4, 0.3)
        assert_same(got, want, f"k=32 {mode}")
        assert (got[0][:40] >= 0).any() and (got[0][80:120] == -1).all()        # graph 2 has 31 < 32 vertices
    with pytest.raises(RuntimeError, match="k > 32"):
        eps.sample_batch(torch.from_numpy(ei), torch.tensor(ptr), 4, 33, "sample", 4, 0.3)
    assert_same(call(eps, ei, ptr, 5, 6, "sample", 4, 0.3), eps_rows.sample_rows(ei, ptr, 5, 6, "sample", 4, 0.3), "after k=33")


@pytest.mark.timeout(300)
def test_device_in_device_out(eps):
    ei, ptr = tu_messy_batch(5)
    for mode in MODES:
        host = call(eps, ei, ptr, 50, 4, mode, 12, 0.1)
        dev = call(eps, ei, ptr, 50, 4, mode, 12, 0.1, device="cuda:0")
        assert_same(dev, host, f"device {mode}")
        assert_same(host, eps_rows.sample_rows(ei, ptr, 50, 4, mode, 12, 0.1), f"host {mode}")


@pytest.mark.timeout(600)
def test_large_graph_rejection_and_grid_sweeps(eps):
    """One graph of n = 2 999 301 vertices (2^32 mod n = 2 967 565: about 0.07 % of start draws are rejected) and more rows
    than one sweep of the walk grid (capped at cus * 8 blocks of 128 rows).  Restated: every row whose first start draw is
    rejected, the rows around each sweep boundary and 2000 random rows; edge_ptr of every row against the columns inside it."""
    import torch
    n, k, seed, epsilon = 2_999_301, 4, 2024, 1.0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweep = cus * 8 * 128
    rows = 3 * sweep + 1000
    rng = np.random.default_rng(0)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n])
    chords = rng.integers(0, n, size=(2, n // 2))
    ei = np.ascontiguousarray(np.concatenate([ring, chords], axis=1) + 5)
    ptr = [5, 5 + n]
    got = call(eps, ei, ptr, rows, k, "sample", seed, epsilon)
    nodes, eidx, eptr, sptr, esrc = got
    assert nodes.shape == (rows, k) and sptr.tolist() == [0, rows] and eptr[0] == 0 and eptr[-1] == eidx.shape[1] == len(esrc)
    rejected = eps_rows.first_draw_rejected(seed, np.arange(rows), n)
    assert len(rejected) > 0
    bounds = [b + d for b in range(sweep, rows, sweep) for d in (-2, -1, 0, 1)]
    check = sorted(set(rejected.tolist()) | set(bounds) | set(rng.integers(0, rows, 2000).tolist()))
    b = eps_rows.Batch(ei, ptr, rows, k, epsilon, seed, large=True)
    for r in check:
        want_nodes, want_edges = b.row(r, "sample")
        assert nodes[r].tolist() == want_nodes, f"row {r}"
        e0, e1 = eptr[r], eptr[r + 1]
        assert list(zip(eidx[0, e0:e1].tolist(), eidx[1, e0:e1].tolist(), esrc[e0:e1].tolist())) == want_edges, f"row {r}"
    # every row: sorted distinct vertices of the graph; edge count = columns (loops included) with both endpoints in the row
    assert (nodes >= 5).all() and (nodes < 5 + n).all() and (np.diff(nodes, axis=1) > 0).all()
    lo_hi = np.sort(ei - 5, axis=0)
    key = np.unique(lo_hi[0] * n + lo_hi[1], return_counts=True)
    cnt = np.zeros(rows, dtype=np.int64)
    loc = nodes - 5
    for i in range(k):
        for j in range(i, k):                      # i == j: self loops
            q = loc[:, i] * n + loc[:, j]
            at = np.minimum(np.searchsorted(key[0], q), len(key[0]) - 1)
            cnt += np.where(key[0][at] == q, key[1][at], 0)
    assert np.array_equal(np.diff(eptr), cnt)


@pytest.mark.timeout(900)
def test_scan_paths_k1(eps):
    """k = 1 on a graph whose vertices carry 0-3 self loops, so row edge counts differ: every row of calls of 0, 1, 16 384,
    16 385 (one-block scan and the two-launch scan), 8 388 608 and 8 388 609 rows (two launches, then the three-launch scan with
    ugs_scan_block_sums) against the vectorised restatement"""
    n, lo = 1000, 2
    rng = np.random.default_rng(9)
    mult = rng.choice(4, size=n, p=[0.8, 0.1, 0.06, 0.04])
    loop_v = np.repeat(np.arange(n), mult)
    loop_v = loop_v[rng.permutation(len(loop_v))]
    other = rng.integers(0, n, size=(2, 300))
    other = other[:, other[0] != other[1]]
    ei = np.concatenate([np.stack([loop_v, loop_v]), other], axis=1)
    perm = rng.permutation(ei.shape[1])
    ei = np.ascontiguousarray(ei[:, perm] + lo)
    is_loop = ei[0] == ei[1]
    loops = [(int(ei[0, j]) - lo, j) for j in np.nonzero(is_loop)[0]]
    for rows in (0, 1, 16_384, 16_385, 8_388_608, 8_388_609):
        mode = "global" if rows % 2 else "sample"
        nodes, eidx, eptr, sptr, esrc = call(eps, ei, [lo, lo + n], rows, 1, mode, 31, 0.5)
        w_nodes, w_eptr, w_eidx, w_esrc = eps_rows.k1_rows(n, loops, rows, 0.5, 31, node_lo=lo, mode=mode)
        assert nodes.shape == (rows, 1) and np.array_equal(nodes[:, 0], w_nodes), rows
        assert sptr.tolist() == [0, rows]
        assert np.array_equal(eptr, w_eptr), f"{rows} rows: edge_ptr differs at {np.argwhere(eptr != w_eptr)[:5].tolist()}"
        assert np.array_equal(eidx, w_eidx) and np.array_equal(esrc, w_esrc), rows
        del nodes, eidx, eptr, esrc, w_nodes, w_eptr, w_eidx, w_esrc
