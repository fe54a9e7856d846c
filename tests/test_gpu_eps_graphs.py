"""GPU: epsilon_uniform_sampler.sample_graphs (one seed per graph) against its law (tests/eps_graphs_law.py: the blocks of one-graph
calls, restated by eps_rows.py) and against the loop of one-graph sample_batch calls on the GPU, bit for bit; and
PresampleCache(sampler="epsilon_uniform").add_many against the loop of add.  Nothing here is statistical."""
import random

import numpy as np
import pytest
import torch

import eps_graphs_law as L
import eps_rows
import ugs_workloads as wl

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MODES = ("sample", "global")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
# distinct; 0 and 2^64 - 1; two pairs that differ only above bit 32
SEEDS8 = [0, M64, 0x1_0000_0007, 0x2_0000_0007, 42, 1 << 63, 0xDEAD_BEEF_0000_0001, 0x0000_0001_0000_0001]


@pytest.fixture(scope="module")
def eps():
    import epsilon_uniform_sampler
    return epsilon_uniform_sampler


def graphs_call(eps, ei, ptr, m, k, mode, seeds, epsilon, device=None):
    e, p = torch.from_numpy(np.ascontiguousarray(ei)), torch.from_numpy(np.asarray(ptr, dtype=np.int64))
    if device is not None:
        e, p = e.to(device), p.to(device)
    out = eps.sample_graphs(e, p, m, k, seeds, mode=mode, epsilon=epsilon)
    G = len(ptr) - 1
    assert len(out) == 6 and out[5].dtype == torch.bool and out[5].device.type == "cpu" and out[5].shape == (G,) and not out[5].any()
    assert all(t.dtype == torch.int64 and t.device.type == ("cuda" if device else "cpu") for t in out[:5])
    return [t.cpu().numpy() for t in out[:5]]


def one_graph(eps, ei, ptr2, m, k, mode, seed, epsilon):
    out = eps.sample_batch(torch.from_numpy(np.ascontiguousarray(ei)), torch.from_numpy(np.asarray(ptr2, dtype=np.int64)), m, k, mode, seed, epsilon)
    return [t.numpy() for t in out]


def block(out, g, m):
    """graph g's block in the one-graph form: edge_ptr re-based, sample_ptr [0, m]; nothing else moves"""
    nodes, eidx, eptr, _, esrc = out
    a, b = int(eptr[g * m]), int(eptr[(g + 1) * m])
    return [nodes[g * m:(g + 1) * m], eidx[:, a:b], eptr[g * m:(g + 1) * m + 1] - a, np.array([0, m], np.int64), esrc[a:b]]


def assert_same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        b = np.asarray(b)
        assert a.shape == b.shape, f"{what}: {name} shape {a.shape} != {b.shape}"
        if not np.array_equal(a, b):
            raise AssertionError(f"{what}: {name} differs at {np.argwhere(a != b)[:5].tolist()}")


def messy_batch(seed):
    """8 graphs with every column oddity the host must sort out: ptr[0] > 0, an empty graph, graphs smaller than k, columns
    shuffled and in both directions, duplicate columns, self loops, columns crossing graphs, columns outside [ptr[0], ptr[G])"""
    rng = np.random.default_rng(seed)
    sizes = [18, 0, 2, 25, 5, 1, 39, 9]
    ptr, cols = [3], []
    for g, n in enumerate(sizes):
        lo = ptr[-1]
        if n >= 2:
            cols.append(wl.tu_graph(n, int(n * 1.2), seed * 31 + g) + lo)
        ptr.append(lo + n)
    end = ptr[-1]
    ei = np.concatenate(cols, axis=1)
    ei = np.concatenate([ei, ei[:, rng.integers(0, ei.shape[1], 20)]], axis=1)
    loops = rng.integers(ptr[0], end, 12)
    ei = np.concatenate([ei, np.stack([loops, loops]), np.stack([loops[:4], loops[:4]])], axis=1)
    cross = np.array([[3, 21, 50, 70], [50, 60, 3, 100]])
    outside = np.array([[0, 1, 5, end, end + 4, -1], [5, 2, 0, 8, end + 1, 7]])
    ei = np.concatenate([ei, cross, outside], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    return np.ascontiguousarray(ei.astype(np.int64)), np.array(ptr, dtype=np.int64)


@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_graph_boundaries_inside_waves_and_blocks(eps, k):
    """m = 1, 7, 100 put the 8 graphs' boundaries at rows that are no multiple of 64 or 128 (at m = 100 rows 100 ... 700: inside
    waves and inside the 128-lane blocks); graphs 1, 2 and 5 (and 4 at k = 8) are smaller than k"""
    ei, ptr = messy_batch(k)
    G = len(ptr) - 1
    for epsilon in (1.0, 0.3, 0.01):
        for mode in MODES:
            for m in (0, 1, 7, 100):
                what = f"k={k} m={m} eps={epsilon} {mode}"
                got = graphs_call(eps, ei, ptr, m, k, mode, SEEDS8, epsilon)
                assert_same(got, L.expected(ei, ptr, m, k, mode, SEEDS8, epsilon), what + " law")
                for g in range(G):
                    assert_same(block(got, g, m), one_graph(eps, ei, ptr[g:g + 2], m, k, mode, SEEDS8[g], epsilon), f"{what} graph {g}")
            assert (got[0][:100] >= 0).any() and (got[0][100:200] == -1).all()               # graph 1 is empty


def test_seed_forms_agree(eps):
    """a list, an int64 tensor (two's complement) and a uint64 numpy array of the same seeds mod 2^64 give the same call"""
    ei, ptr = messy_batch(2)
    want = graphs_call(eps, ei, ptr, 7, 3, "sample", SEEDS8, 0.3)
    as_i64 = torch.tensor([s if s < 1 << 63 else s - (1 << 64) for s in SEEDS8], dtype=torch.int64)
    assert_same(graphs_call(eps, ei, ptr, 7, 3, "sample", as_i64, 0.3), want, "int64 tensor")
    assert_same(graphs_call(eps, ei, ptr, 7, 3, "sample", np.array(SEEDS8, np.uint64), 0.3), want, "uint64 array")
    assert_same(graphs_call(eps, ei, ptr, 7, 3, "sample", [s + (1 << 64) for s in SEEDS8], 0.3), want, "seeds past 2^64")


def test_local_row_key(eps):
    """the generator key is (seeds[g], row inside the graph): two copies of one graph with the same seed, at batch positions 1 and
    3 behind graphs of other sizes, give the same block up to the node and column offsets; with different seeds they differ"""
    a, b, c = wl.tu_graph(13, 17, 5), wl.tu_graph(30, 40, 6), wl.tu_graph(6, 7, 7)
    sizes, graphs = [6, 30, 13, 30, 6], [c, b, a, b, c]
    ptr = np.cumsum([0] + sizes)
    col0 = np.cumsum([0] + [g.shape[1] for g in graphs])
    ei = np.concatenate([g + ptr[i] for i, g in enumerate(graphs)], axis=1).astype(np.int64)
    m, k = 77, 4
    for mode in MODES:
        got = graphs_call(eps, ei, ptr, m, k, mode, [1, 9, 2, 9, 1 + (1 << 40)], 0.3)
        x, y = block(got, 1, m), block(got, 3, m)
        assert (x[0] >= 0).any()
        assert np.array_equal(x[0] - ptr[1], y[0] - ptr[3]) and np.array_equal(x[2], y[2])
        assert np.array_equal(x[4] - col0[1], y[4] - col0[3])
        off = 0 if mode == "sample" else 1
        assert np.array_equal(x[1] - off * ptr[1], y[1] - off * ptr[3])
        u, v = block(got, 0, m), block(got, 4, m)              # same graph, seeds that differ only in bit 40
        assert not np.array_equal(u[0] - ptr[0], v[0] - ptr[4])
        assert_same(got, L.expected(ei, ptr, m, k, mode, [1, 9, 2, 9, 1 + (1 << 40)], 0.3), f"law {mode}")


def test_k32_last_lds_slot(eps):
    def pathlike(n, s):
        r = np.random.default_rng(s)
        p = np.stack([np.arange(n - 1), np.arange(1, n)])
        return np.concatenate([p, r.integers(0, n, size=(2, 3))], axis=1)
    sizes = [40, 31, 33]
    ptr = np.cumsum([0] + sizes)
    ei = np.concatenate([pathlike(n, g) + ptr[g] for g, n in enumerate(sizes)], axis=1).astype(np.int64)
    seeds = [4, M64 - 1, 1 << 33]
    for mode in MODES:
        got = graphs_call(eps, ei, ptr, 5, 32, mode, seeds, 0.3)
        assert_same(got, L.expected(ei, ptr, 5, 32, mode, seeds, 0.3), f"k=32 {mode}")
        assert (got[0][:5] >= 0).any() and (got[0][5:10] == -1).all()                       # graph 1 has 31 < 32 vertices
        for g in range(3):
            assert_same(block(got, g, 5), one_graph(eps, ei, ptr[g:g + 2], 5, 32, mode, seeds[g], 0.3), f"k=32 {mode} graph {g}")
    with pytest.raises(RuntimeError, match="k > 32"):
        eps.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), 5, 33, seeds)


def test_grid_stride_sweep(eps):
    """more rows than one sweep of the capped walk grid (cus * 8 blocks of 128 rows): 4-vertex graphs at m = 128, so that every
    block of the first sweep is one graph and the second sweep starts again at block 0 with other graphs"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sweep = cus * 8 * 128
    m, k, epsilon = 128, 3, 0.3
    G = cus * 8 + 77
    rows = G * m
    assert rows > sweep
    rng = np.random.default_rng(12)
    pairs = np.array([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])
    cols = []
    for g in range(G):                                          # 2 to 6 of the 6 possible edges: some graphs have no connected triple
        pick = pairs[rng.permutation(6)[:rng.integers(2, 7)]]
        cols.append(np.where(rng.random(len(pick))[:, None] < 0.5, pick, pick[:, ::-1]).T + 4 * g)
    ei = np.concatenate(cols, axis=1).astype(np.int64)
    ei = np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])
    ptr = np.arange(G + 1, dtype=np.int64) * 4
    seeds = rng.integers(0, 1 << 63, G, dtype=np.int64).astype(np.uint64) * np.uint64(2) + (np.arange(G) % 2).astype(np.uint64)
    nodes, eidx, eptr, sptr, esrc = got = graphs_call(eps, ei, ptr, m, k, "sample", seeds, epsilon)
    assert nodes.shape == (rows, k) and np.array_equal(sptr, np.arange(G + 1) * m) and eptr[0] == 0 and eptr[-1] == eidx.shape[1] == len(esrc)
    edges = [b + d for b in range(sweep - 256, min(sweep + 257, rows), 128) for d in (-2, -1, 0, 1)]
    check = sorted(set(edges) | {0, 1, rows - 2, rows - 1} | set(rng.integers(0, rows, 2000).tolist()))
    want = L.expected_rows(ei, ptr, m, k, "sample", seeds.tolist(), epsilon, check)
    for r in check:
        assert nodes[r].tolist() == want[r][0], f"row {r}"
        e0, e1 = eptr[r], eptr[r + 1]
        assert list(zip(eidx[0, e0:e1].tolist(), eidx[1, e0:e1].tolist(), esrc[e0:e1].tolist())) == want[r][1], f"row {r}"
    ok = nodes[:, 0] >= 0
    assert ok.any() and (~ok).any()
    for g in sorted(set(rng.integers(0, G, 14).tolist()) | {cus * 8 - 1, cus * 8}):
        assert_same(block(got, g, m), one_graph(eps, ei, ptr[g:g + 2], m, k, "sample", int(seeds[g]), epsilon), f"graph {g}")


def test_empty_calls_have_sample_batchs_shapes(eps):
    ei, ptr = messy_batch(3)
    none = torch.zeros((2, 0), dtype=torch.int64)
    for e, p, m, seeds in ((none, torch.tensor([0]), 5, []), (torch.from_numpy(ei), torch.tensor([7]), 5, []),
                           (torch.from_numpy(ei), torch.from_numpy(ptr), 0, SEEDS8), (none, torch.tensor([0, 4]), 0, [1])):
        out = eps.sample_graphs(e, p, m, 3, seeds, epsilon=0.3)
        ref = eps.sample_batch(e, p, m, 3, "sample", 1, 0.3)
        assert out[5].shape == (p.numel() - 1,) and not out[5].any()
        for name, a, b in zip(NAMES, out, ref):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), name


def test_device_in_device_out(eps):
    ei, ptr = messy_batch(5)
    for mode in MODES:
        host = graphs_call(eps, ei, ptr, 50, 4, mode, SEEDS8, 0.1)
        dev = graphs_call(eps, ei, ptr, 50, 4, mode, SEEDS8, 0.1, device="cuda:0")
        assert_same(dev, host, f"device {mode}")
        assert_same(host, L.expected(ei, ptr, 50, 4, mode, SEEDS8, 0.1), f"host {mode}")


def test_errors_come_before_any_launch(eps):
    ei, ptr = messy_batch(4)
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    for bad in (0.0, 1.0001, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match=r"epsilon must be in \(0, 1\]"):
            eps.sample_graphs(e, p, 5, 3, SEEDS8, epsilon=bad)
    with pytest.raises(RuntimeError, match="one seed per graph"):
        eps.sample_graphs(e, p, 5, 3, SEEDS8[:7])
    with pytest.raises(RuntimeError, match="one seed per graph"):
        eps.sample_graphs(e, p, 5, 3, SEEDS8 + [1])
    with pytest.raises(RuntimeError, match="int64 or uint64"):
        eps.sample_graphs(e, p, 5, 3, torch.ones(8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="edge_index must be int64"):
        eps.sample_graphs(e.to(torch.int32), p, 5, 3, SEEDS8)
    with pytest.raises(RuntimeError, match="ptr must be int64"):
        eps.sample_graphs(e, p.to(torch.int32), 5, 3, SEEDS8)
    with pytest.raises(RuntimeError, match="m_per_graph must be >= 0"):
        eps.sample_graphs(e, p, -1, 3, SEEDS8)
    with pytest.raises(RuntimeError, match="k must be >= 1"):
        eps.sample_graphs(e, p, 5, 0, SEEDS8)
    assert_same(graphs_call(eps, ei, ptr, 5, 3, "sample", SEEDS8, 0.3), L.expected(ei, ptr, 5, 3, "sample", SEEDS8, 0.3), "after the errors")


# ---- PresampleCache(sampler="epsilon_uniform") ----
def dataset(rng, N):
    """N random graphs of 1 to 40 vertices: some smaller than k = 4, one without edges, some with columns outside [0, n)"""
    sizes, graphs = [], []
    for i in range(N):
        n = rng.randint(1, 3) if rng.random() < 0.12 else rng.randint(4, 40)
        ei = wl.tu_graph(n, n - 1 + rng.randint(0, n // 3 + 1), rng.randrange(1 << 30)) if n > 1 else np.zeros((2, 0), np.int64)
        if i == 11:
            n, ei = 9, np.zeros((2, 0), np.int64)
        if rng.random() < 0.15:
            ei = np.concatenate([ei, [[0, n], [n + 2, -1]]], axis=1)
        if rng.random() < 0.3 and ei.shape[1]:                  # a loop, duplicate columns, any order
            ei = np.concatenate([ei, [[0], [0]], ei[:, :2]], axis=1)
            ei = ei[:, np.array(rng.sample(range(ei.shape[1]), ei.shape[1]))]
        sizes.append(n)
        graphs.append(np.ascontiguousarray(ei.astype(np.int64)))
    return sizes, graphs


def batch_of(order, sizes, graphs):
    ptr = np.cumsum([0] + [sizes[i] for i in order])
    cols = np.concatenate([graphs[i] + ptr[j] for j, i in enumerate(order)] + [np.zeros((2, 0), np.int64)], axis=1)
    return ptr, cols


def loads(cache, orders, sizes, graphs):
    res = []
    for order in orders:
        ptr, cols = batch_of(order, sizes, graphs)
        res.append([t.cpu().numpy() for t in cache.load(torch.tensor(order), torch.from_numpy(ptr), torch.from_numpy(cols))])
    return res


def trainer_load(per_graph, order, sizes, graphs):
    """the reference trainer's _load_from_presample_cache (gps/experiment.py:936-993) over cached one-graph results: nodes plus
    ptr[g], edge ids as cached, edge_src plus the batch columns whose source lies in an earlier graph, edge_ptr accumulated"""
    ptr, cols = batch_of(order, sizes, graphs)
    nodes, eidx, esrc, eptr, sptr = [], [], [], [0], [0]
    for g, i in enumerate(order):
        n_g, e_g, p_g, _, s_g = per_graph[i]
        before = int((cols[0] < ptr[g]).sum() - (cols[0] < ptr[0]).sum())
        nodes.append(n_g + ptr[g])
        eidx.append(e_g)
        esrc.append(s_g + before)
        eptr += (eptr[-1] + p_g[1:]).tolist()
        sptr.append(sptr[-1] + n_g.shape[0])
    return [np.concatenate(nodes), np.concatenate(eidx, axis=1), np.array(eptr), np.array(sptr), np.concatenate(esrc)]


def test_presample_cache_add_many_equals_the_add_loop(eps, monkeypatch):
    from ugs_sampler.presample import PresampleCache
    rng = random.Random(77)
    N, m, k, epsilon = 60, 10, 4, 0.3
    sizes, graphs = dataset(rng, N)
    assert min(sizes) < k and any(g.shape[1] == 0 and n >= k for g, n in zip(graphs, sizes))
    seeds = [42 + i for i in range(N)]
    seeds[5], seeds[6] = M64, 42 + (1 << 32)                   # past int64, and equal to seeds[0] below bit 32
    ts = [torch.from_numpy(g) for g in graphs]
    calls = []
    real = eps._sample_graphs
    monkeypatch.setattr(eps, "_sample_graphs", lambda *a, **kw: (calls.append(a[1].numel() - 1), real(*a, **kw))[1])
    loop = PresampleCache(m, k, "cuda:0", sampler="epsilon_uniform", epsilon=epsilon)
    for i in range(N):
        assert loop.add(i, ts[i], sizes[i], seeds[i])
    assert not calls and not loop.failed
    many = PresampleCache(m, k, "cuda:0", sampler="epsilon_uniform", epsilon=epsilon)
    many.add_many(range(N), list(zip(ts, sizes)), seeds)
    assert calls == [N] and not many.failed
    del calls[:]
    tiny = PresampleCache(m, k, "cuda:0", sampler="epsilon_uniform", epsilon=epsilon, chunk_vertices=50, chunk_rows=3 * m)
    tiny.add_many(torch.arange(N), list(zip(ts, sizes)), seeds)
    assert len(calls) >= N // 3 and sum(calls) == N and max(calls) <= 3 and not tiny.failed
    law = {i: eps_rows.sample_rows(graphs[i], [0, sizes[i]], m, k, "sample", seeds[i], epsilon) for i in range(N)}
    orders = [list(range(N)), [5, 11, 11, 40, 0, 59, 6], rng.sample(range(N), 32)]
    want = [trainer_load(law, order, sizes, graphs) for order in orders]
    for cache in (loop, many, tiny):
        for order, got, exp in zip(orders, loads(cache, orders, sizes, graphs), want):
            for name, a, b in zip(NAMES, got, exp):
                assert a.shape == b.shape and np.array_equal(a, b), (name, order[:4])
    # epsilon reaches the sampler: at 0.002 an attempt of weight w is accepted with probability 0.002 / (w + 0.002), about a half
    # for these graphs (w about 1e-3), against more than 0.99 at 0.3, so the rows cannot all agree
    other = PresampleCache(m, k, "cuda:0", sampler="epsilon_uniform", epsilon=0.002)
    other.add_many(range(N), list(zip(ts, sizes)), seeds)
    assert not np.array_equal(loads(other, orders[:1], sizes, graphs)[0][0], want[0][0])
