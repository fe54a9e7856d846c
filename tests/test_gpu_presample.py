"""uniform_sampler.sample_graphs / rwr_sampler.sample_graphs (one seed per graph) against the one-graph drop-in calls and the CPU
restatements of their laws, and PresampleCache(sampler="uniform" / "rwr").add_many against the loop of add."""
import random

import numpy as np
import pytest
import torch

import rwr_law as R
import ugs_workloads as wl
import uniform_law as U

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


def mod(name):
    if name == "uniform":
        import uniform_sampler
        return uniform_sampler
    import rwr_sampler
    return rwr_sampler


def one_graph(name, ei, ptr, m, k, mode, seed, law=False):
    """the drop-in call (or the law) for the one-graph pointer ptr[g:g+2] of the same batch, as numpy arrays"""
    if law:
        return (U if name == "uniform" else R).sample_batch(ei, ptr, m, k, mode, seed)
    out = mod(name).sample_batch(torch.from_numpy(ei), torch.from_numpy(np.asarray(ptr, np.int64)), m, k, mode=mode, seed=seed)
    return [t.cpu().numpy() for t in out]


def block(out, g, m):
    """graph g's block of a sample_graphs result, in the one-graph form (edge_ptr re-based, sample_ptr [0, m])"""
    nodes, eidx, eptr, _, esrc = [t.cpu().numpy() for t in out[:5]]
    a, b = int(eptr[g * m]), int(eptr[(g + 1) * m])
    return [nodes[g * m:(g + 1) * m], eidx[:, a:b], eptr[g * m:(g + 1) * m + 1] - a, np.array([0, m], np.int64), esrc[a:b]]


def assert_block(got, want, what):
    for nm, a, b in zip(("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src"), got, want):
        b = np.asarray(b)
        assert a.shape == b.shape and np.array_equal(a, b), (what, nm, a.shape, b.shape)


def random_batch(rng, G, max_n=64):
    """graphs like test_gpu_uniform.random_batch, plus empty graphs, loops, duplicate, cross-graph and out-of-range columns,
    ptr[0] > 0, columns in any order"""
    sizes = []
    for _ in range(G):
        r = rng.random()
        sizes.append(0 if r < 0.1 else rng.randint(1, 3) if r < 0.2 else rng.choice([5, 8, 13, 18, 28, 40, max_n])
                     if r < 0.8 else rng.randint(1, max_n))
    cols, ptr = [], [rng.randint(0, 3)]
    for n in sizes:
        if n > 1:
            extra = rng.randint(0, n // 4 + 1) if n > 30 else rng.randint(0, n)
            ei = wl.tu_graph(n, n - 1 + extra, rng.randrange(1 << 30))
            if rng.random() < 0.4:
                v = rng.randrange(n)
                ei = np.concatenate([ei, [[v], [v]], ei[:, :rng.randint(0, 3)]], axis=1)      # a loop, duplicate columns
            cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    end = ptr[-1]
    odd = [[ptr[0], end - 1], [end, ptr[0]], [end + 5, end + 6], [-1, ptr[0]], [0, 0]]      # cross-graph, out of range
    cols.append(np.array(rng.sample(odd, rng.randint(1, len(odd))), np.int64).T)
    ei = np.concatenate(cols, axis=1).astype(np.int64)
    perm = np.array(rng.sample(range(ei.shape[1]), ei.shape[1]), dtype=np.int64)
    return np.ascontiguousarray(ei[:, perm]), np.array(ptr, np.int64)


@pytest.mark.parametrize("name", ["uniform", "rwr"])
@pytest.mark.parametrize("case", range(10))
def test_sample_graphs_equals_one_graph_calls(name, case):
    rng = random.Random(7000 + case + (100 if name == "rwr" else 0))
    ei, ptr = random_batch(rng, rng.randint(1, 9))
    G = len(ptr) - 1
    k = 1 + case % 6
    m = [0, 1, 7, 400][case % 4]
    mode = "sample" if case % 3 else "global"
    seeds = [[0, M64][g % 2] if case % 5 == 0 else rng.getrandbits(64) for g in range(G)]
    if case == 3:
        seeds = torch.tensor([(s if s < 1 << 63 else s - (1 << 64)) for s in seeds], dtype=torch.int64)   # int64 tensor: mod 2^64
    dev = "cuda:0" if case % 2 else None
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    if dev:
        e, p = e.to(dev), p.to(dev)
    out = mod(name).sample_graphs(e, p, m, k, seeds, mode=mode)
    assert len(out) == 6 and out[5].dtype == torch.bool and out[5].shape == (G,)
    assert all(t.device.type == ("cuda" if dev else "cpu") for t in out)
    assert not out[5].any()
    assert np.array_equal(out[3].cpu().numpy(), np.arange(G + 1) * m)
    sd = [int(s) & M64 for s in (seeds.tolist() if torch.is_tensor(seeds) else seeds)]
    for g in range(G):
        got = block(out, g, m)
        assert_block(got, one_graph(name, ei, ptr[g:g + 2], m, k, mode, sd[g]), f"{name} case {case} graph {g}")
        if m <= 7:
            assert_block(got, one_graph(name, ei, ptr[g:g + 2], m, k, mode, sd[g], law=True), f"{name} law case {case} graph {g}")


def test_rwr_sample_graphs_uses_each_graphs_seed_and_p_restart():
    rng = random.Random(99)
    ei, ptr = random_batch(rng, 6)
    G = len(ptr) - 1
    seeds = [rng.getrandbits(64) for _ in range(G)]
    out = mod("rwr").sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), 50, 4, seeds, p_restart=0.6)
    for g in range(G):
        want = R.sample_batch(ei, ptr[g:g + 2], 50, 4, "sample", seeds[g], 0.6)
        assert_block(block(out, g, 50), want, f"graph {g}")


def clique(n):
    a, b = np.triu_indices(n, 1)
    return np.concatenate([np.stack([a, b]), np.stack([b, a])], axis=1).astype(np.int64)


def batch_of(graphs):
    ptr, cols = [0], []
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    return np.ascontiguousarray(np.concatenate(cols, axis=1)), np.array(ptr, np.int64)


def test_uniform_graphs_that_one_graph_calls_refuse_fail_alone():
    k, m = 6, 20
    graphs = [(18, wl.tu_graph(18, 22, 1)), (65, wl.tu_graph(65, 80, 2)), (30, wl.tu_graph(30, 36, 3)), (64, clique(64)),
              (12, wl.tu_graph(12, 14, 4))]
    ei, ptr = batch_of(graphs)
    seeds = [11, 12, 13, 14, 15]
    out = mod("uniform").sample_graphs(torch.from_numpy(ei).cuda(), torch.from_numpy(ptr), m, k, seeds)
    assert out[5].cpu().tolist() == [False, True, False, True, False]
    for g in range(len(graphs)):
        got = block(out, g, m)
        if g in (1, 3):
            with pytest.raises(RuntimeError):
                one_graph("uniform", ei, ptr[g:g + 2], m, k, "sample", seeds[g])
            assert (got[0] == -1).all() and got[1].shape == (2, 0) and not got[2].any()
        else:
            assert_block(got, one_graph("uniform", ei, ptr[g:g + 2], m, k, "sample", seeds[g]), f"graph {g}")


def loads(cache, orders, sizes, graphs):
    res = []
    for order in orders:
        ptr = np.cumsum([0] + [sizes[i] for i in order])
        cols = np.concatenate([graphs[i] + ptr[j] for j, i in enumerate(order)] + [np.zeros((2, 0), np.int64)], axis=1)
        res.append([t.cpu().numpy() for t in cache.load(torch.tensor(order), torch.from_numpy(ptr), torch.from_numpy(cols))])
    return res


def assert_same_cache(a, b, orders, sizes, graphs):
    assert a.failed == b.failed
    for order, x, y in zip(orders, loads(a, orders, sizes, graphs), loads(b, orders, sizes, graphs)):
        for u, v in zip(x, y):
            assert u.shape == v.shape and np.array_equal(u, v), order


def test_uniform_joint_budget_is_a_call_error_and_add_many_splits():
    from ugs_sampler.presample import PresampleCache
    k, m = 6, 8
    graphs = [clique(40)] * 9                                   # 3.8e6 sets each, 3.4e7 together: over the 2^25 budget
    ei, ptr = batch_of([(40, g) for g in graphs])
    with pytest.raises(RuntimeError, match="split"):
        mod("uniform").sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, list(range(9)))
    small = mod("uniform").sample_batch(torch.from_numpy(clique(5)), torch.tensor([0, 5]), 3, 2, seed=1)   # still usable
    assert small[0].shape == (3, 2)
    loop = PresampleCache(m, k, "cuda:0", sampler="uniform")
    for i, g in enumerate(graphs):
        loop.add(i, torch.from_numpy(g), 40, 42 + i)
    many = PresampleCache(m, k, "cuda:0", sampler="uniform")
    many.add_many(range(9), [(torch.from_numpy(g), 40) for g in graphs], [42 + i for i in range(9)])
    assert not many.failed
    assert_same_cache(loop, many, [list(range(9)), [8, 0, 0, 3]], [40] * 9, graphs)


def dataset(rng, N, max_n):
    sizes, graphs = [], []
    for i in range(N):
        n = rng.choice([0, 1, 2, 3]) if rng.random() < 0.08 else rng.randint(4, max_n)
        if i in (17, 150) and max_n <= 64:
            n = 70                                              # uniform: more than 64 vertices, fails
        ei = wl.tu_graph(n, n - 1 + rng.randint(0, n // 3 + 1), rng.randrange(1 << 30)) if n > 1 else np.zeros((2, 0), np.int64)
        if rng.random() < 0.1 and n > 0:
            ei = np.concatenate([ei, [[0, n], [n + 2, -1]]], axis=1)    # columns outside [0, n): dropped by the one-graph call
        sizes.append(n)
        graphs.append(np.ascontiguousarray(ei.astype(np.int64)))
    return sizes, graphs


def reference_load(host, m, k, order, sizes, graphs):
    """test_gpu_parity.py::test_presample_cache_assembles_batches_like_the_reference_trainer's restatement of the reference's
    _load_from_presample_cache (gps/experiment.py:936-993)"""
    ptr = np.cumsum([0] + [sizes[i] for i in order])
    cols = np.concatenate([graphs[i] + ptr[j] for j, i in enumerate(order)] + [np.zeros((2, 0), np.int64)], axis=1)
    off = [0]
    for g in range(len(order) - 1):
        off.append(off[-1] + int(((cols[0] >= ptr[g]) & (cols[0] < ptr[g + 1])).sum()))
    nodes, edges, esrc, eptr, sptr, ce, cs = [], [], [], [0], [0], 0, 0
    for g, i in enumerate(order):
        if i in host:
            n_g, e_g, p_g, _, s_g = host[i]
        else:
            n_g, e_g, p_g, s_g = np.full((m, k), -1, np.int64), np.zeros((2, 0), np.int64), np.zeros(m + 1, np.int64), np.zeros(0, np.int64)
        nodes.append(n_g + ptr[g]); edges.append(e_g); esrc.append(s_g + off[g])
        eptr += [ce + int(p_g[r + 1]) for r in range(n_g.shape[0])]
        ce += e_g.shape[1]; cs += n_g.shape[0]; sptr.append(cs)
    return [np.concatenate(nodes), np.concatenate(edges, axis=1), np.array(eptr), np.array(sptr), np.concatenate(esrc)]


@pytest.mark.parametrize("name", ["uniform", "rwr"])
def test_presample_cache_add_many_equals_the_add_loop(name):
    from ugs_sampler.presample import PresampleCache
    rng = random.Random(31 if name == "uniform" else 32)
    m, k = 12, 4 if name == "uniform" else 5
    N = 300
    sizes, graphs = dataset(rng, N, 40 if name == "uniform" else 60)
    seeds = [42 + i for i in range(N)]
    ts = [torch.from_numpy(g) for g in graphs]
    ts[40] = ts[40].to(torch.int32)                             # add refuses it (edge_index must be int64): a failure in its place
    loop = PresampleCache(m, k, "cuda:0", sampler=name)
    for i in range(N):
        loop.add(i, ts[i], sizes[i], seeds[i])
    assert loop.failed == {40} | ({17, 150} if name == "uniform" else set())
    host = {i: one_graph(name, graphs[i], [0, sizes[i]], m, k, "sample", seeds[i]) for i in range(N) if i not in loop.failed}
    many = PresampleCache(m, k, "cuda:0", sampler=name)
    many.add_many(range(N), list(zip(ts, sizes)), seeds)
    tiny = PresampleCache(m, k, "cuda:0", sampler=name, chunk_vertices=50, chunk_rows=3 * m)
    tiny.add_many(torch.arange(N), list(zip(ts, sizes)), torch.tensor(seeds))
    orders = [list(range(N)), [5, 17, 17, 40, 0, 299], [3], rng.sample(range(N), 64), [150, 2, 2, 2]]
    assert_same_cache(loop, many, orders, sizes, graphs)
    assert_same_cache(loop, tiny, orders, sizes, graphs)
    for order, got in zip(orders, loads(many, orders, sizes, graphs)):
        for a, b in zip(got, reference_load(host, m, k, order, sizes, graphs)):
            assert a.shape == b.shape and np.array_equal(a, b), order


def test_presample_cache_ugs_add_many_is_the_loop():
    from ugs_sampler.presample import PresampleCache
    rng = random.Random(5)
    sizes, graphs = dataset(rng, 20, 30)
    loop, many = PresampleCache(8, 3, "cuda:0"), PresampleCache(8, 3, "cuda:0", sampler="ugs")
    for i in range(20):
        loop.add(i, torch.from_numpy(graphs[i]), sizes[i], 7 + i)
    many.add_many(range(20), [(torch.from_numpy(g), n) for g, n in zip(graphs, sizes)], [7 + i for i in range(20)])
    assert_same_cache(loop, many, [list(range(20)), [3, 3, 1]], sizes, graphs)
