"""GPU: ugs_sampler.sample_graphs (sample_batch with one seed per graph; law in include/ugs_mi355.h at ugs_sample_graphs_begin)
against the reference fixture f16 and against the CPU oracle's one-graph loop on one LRU -- never against the product alone.
Bit-exact."""
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import oracle
import ugs_workloads as wl
from ugs_graphs_law import NAMES, block, check_random_batches, concat, fixture, oracle_loop

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        assert g.shape == np.asarray(w).shape and np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("device", [None, "cuda:0"])
def test_fixture_blocks_of_the_reference_presample_loop(device):
    """the k = 4 call, then the k = 5 call in one process after clear_cache(): every graph's block, re-based, is the reference's
    one-graph call of f16 (the second call reuses the first's preprocessing through the key that ignores k, like the fixture)"""
    import ugs_sampler
    graphs, seeds, m, want = fixture()
    ei, ptr, col0 = concat(graphs)
    ugs_sampler.clear_cache()
    for k in (4, 5):
        out = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, seeds, device=device)
        assert all(t.is_cuda == (device is not None) for t in out)
        out = [t.cpu().numpy() for t in out]
        assert np.array_equal(out[3], np.arange(len(graphs) + 1) * m) and not out[5].any()
        for g in range(len(graphs)):
            same(block(out, g, m, int(ptr[g]), int(col0[g])), want[k][g], (k, g))
    ugs_sampler.clear_cache()


def test_random_batches_against_the_oracle_loop_fresh_lru():
    check_random_batches(1000, 70, 1601)


def test_random_batches_against_the_oracle_loop_lru_of_three():
    """UGS_CACHE_SIZE=3 (fixed at first use: subprocess) on both sides: evictions and re-misses inside one call"""
    code = ("import os, sys\nos.environ['UGS_CACHE_SIZE'] = '3'\n"
            "sys.path[:0] = [os.path.join(os.getcwd(), p) for p in ('tests', 'oracle', 'ss-gnn_amd')]\n"
            "import ugs_graphs_law\nugs_graphs_law.check_random_batches(3, 50, 1602)\nprint('OK')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=800)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])


@pytest.mark.parametrize("mode", ["sample", "graph", "global"])
def test_the_same_seed_everywhere_is_sample_batch(mode):
    import ugs_sampler
    ei, ptr = wl.tu_batch(39, 73, 24)
    cache = oracle.Cache()
    for s in (42, 0, -5):
        ugs_sampler.clear_cache()
        want = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 16, 5, mode, s)
        ugs_sampler.clear_cache()
        got = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), 16, 5, [s] * 24, mode)
        same(got, [t.numpy() for t in want], (mode, s))
        same(got, oracle.sample_batch(ei, ptr, 16, 5, mode, s, cache), (mode, s, "oracle"))
    cache.close()
    ugs_sampler.clear_cache()


def _dense_case(rng, big=False):
    """test_gpu_stress.py's recipe, graphs dense enough to leave tier S"""
    cols, ptr = [], [0]
    for _ in range(rng.randint(2, 4)):
        n = rng.choice([70, 150, 400, 460]) if not big else 2600
        p = rng.choice([0.05, 0.15, 0.4]) if not big else 0.0
        off = ptr[-1]
        e = [(u + off, v + off) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
        e += [(off + v - 1, off + v) for v in range(1, n)]                                # connected
        if big:                                                                           # three hubs: most walks outgrow 2048 candidates
            e += [(off + h, off + v) for h in range(3) for v in range(3, n)]
        if rng.random() < 0.4:
            e = e + [(v, u) for u, v in e]
        if rng.random() < 0.3:
            e += [(off + rng.randrange(n),) * 2 for _ in range(3)]
        cols += e
        ptr.append(off + n)
    if rng.random() < 0.5:
        rng.shuffle(cols)
    ei = np.array(cols, dtype=np.int64).T.reshape(2, -1).copy()
    G = len(ptr) - 1
    return (ei, np.array(ptr, np.int64), rng.choice([3, 7]), rng.choice([3, 4, 6, 8, 12]), rng.choice(["sample", "graph", "global"]),
            [rng.choice([42, 0, -7]) + g for g in range(G)])


@pytest.mark.parametrize("tier", [None, "0", "1", "2", "3", "4", "5"])
def test_per_graph_seeds_under_every_first_tier(tier, monkeypatch):
    import ugs_sampler
    if tier is None:
        monkeypatch.delenv("UGS_FORCE_TIER", raising=False)
    else:
        monkeypatch.setenv("UGS_FORCE_TIER", tier)
    rng = random.Random(3000 + (int(tier) if tier else 7))
    ugs_sampler.clear_cache()
    cache = oracle.Cache()
    for it in range(10):
        ei, ptr, m, k, mode, seeds = _dense_case(rng)
        want = oracle_loop(ei, ptr, m, k, mode, seeds, cache)          # (the oracle completes every row: no case is skipped)
        got = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, seeds, mode)
        same(got, want, (tier, it, list(np.diff(ptr)), m, k, mode))
    ugs_sampler.clear_cache()
    cache.close()


def test_per_graph_seeds_in_the_global_memory_tier(monkeypatch):
    import ugs_sampler
    monkeypatch.delenv("UGS_FORCE_TIER", raising=False)
    rng = random.Random(3100)
    ugs_sampler.clear_cache()
    cache = oracle.Cache()
    for it in range(2):
        ei, ptr, m, k, mode, seeds = _dense_case(rng, big=True)
        want = oracle_loop(ei, ptr, m, 4, mode, seeds, cache)
        got = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, 4, seeds, mode)
        same(got, want, ("global tier", it, mode))
    plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 4)
    plan.walk(m)
    assert plan.last_launch()["overflow_rows"] > 0          # rows did reach the tiers behind the first
    plan.close()
    ugs_sampler.clear_cache()
    cache.close()


@pytest.mark.parametrize("packed", [True, False])
def test_packed_and_ordinary_step(packed, monkeypatch):
    import ugs_sampler
    if packed:
        monkeypatch.delenv("UGS_NO_PACKED_STEP", raising=False)
    else:
        monkeypatch.setenv("UGS_NO_PACKED_STEP", "1")
    ei, ptr = wl.tu_batch(20, 24, 64)
    seeds = [100 - 3 * g for g in range(64)]
    cache = oracle.Cache()
    for mode in ("sample", "graph", "global"):
        ugs_sampler.clear_cache()
        want = oracle_loop(ei, ptr, 32, 6, mode, seeds, cache)
        for device in (None, "cuda:0"):
            same(ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), 32, 6, seeds, mode, device=device), want, (packed, mode, device))
    cache.close()
    ugs_sampler.clear_cache()


def test_cold_batch_of_new_graphs_is_preprocessed_on_the_device():
    """a fresh process in the default mode, like the trainer's start-up (the library pauses the device pass for a while after
    batches it had to refuse, which earlier tests of this process may have sent)"""
    code = r'''
import os, sys
os.environ.pop("UGS_DEVICE_BATCH", None)
sys.path[:0] = [os.path.join(os.getcwd(), p) for p in ("tests", "oracle", "ss-gnn_amd")]
import numpy as np, torch
import oracle, ugs_sampler, ugs_workloads as wl
from ugs_graphs_law import NAMES, concat, oracle_loop
graphs = [(n, wl.tu_graph(n, n + 3, 9000 + i)) for i, n in enumerate([12 + i % 17 for i in range(120)])]
ei, ptr, _ = concat(graphs)
assert ei.shape[1] >= 2048
seeds = [5 * g - 100 for g in range(len(graphs))]
before = ugs_sampler.batch_pass_stats()
got = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), 10, 5, seeds)
after = ugs_sampler.batch_pass_stats()
assert after["device_plans"] == before["device_plans"] + 1 and after["general_path"] == before["general_path"], (before, after)
assert ugs_sampler.cache_stats()["misses"] == len(graphs)
for name, g, w in zip(NAMES, got, oracle_loop(ei, ptr, 10, 5, "sample", seeds, oracle.Cache())):
    assert np.array_equal(g.numpy(), w), name
print("OK")
'''
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])


def test_presample_cache_ugs_add_many_equals_the_add_loop_and_the_oracle():
    import ugs_sampler
    from test_gpu_presample import assert_same_cache, dataset, loads, reference_load
    from ugs_sampler.presample import PresampleCache
    rng = random.Random(33)
    m, k, N = 12, 5, 300
    sizes, graphs = dataset(rng, N, 60)
    seeds = [42 + i for i in range(N)]
    seeds[7], seeds[8], seeds[200] = 0, -(2 ** 31), 2 ** 40          # 2^40 is no C int: the one-graph call refuses it
    ts = [torch.from_numpy(g) for g in graphs]
    ts[40] = ts[40].to(torch.int32)                                  # add refuses it (edge_index must be int64)
    ugs_sampler.clear_cache()
    loop = PresampleCache(m, k, "cuda:0", sampler="ugs")
    for i in range(N):
        loop.add(i, ts[i], sizes[i], seeds[i])
    assert loop.failed == {40, 200}
    cache = oracle.Cache()
    host = {}
    for i in range(N):
        if i not in loop.failed:
            host[i] = oracle.sample_batch(graphs[i], np.array([0, sizes[i]], np.int64), m, k, "sample", seeds[i], cache)
    cache.close()
    ugs_sampler.clear_cache()
    many = PresampleCache(m, k, "cuda:0", sampler="ugs")
    many.add_many(range(N), list(zip(ts, sizes)), seeds)
    ugs_sampler.clear_cache()
    tiny = PresampleCache(m, k, "cuda:0", sampler="ugs", chunk_vertices=50, chunk_rows=3 * m)
    tiny.add_many(torch.arange(N), list(zip(ts, sizes)), seeds)
    orders = [list(range(N)), [5, 17, 17, 40, 0, 299], [3], rng.sample(range(N), 64), [200, 2, 2, 2]]
    assert_same_cache(loop, many, orders, sizes, graphs)
    assert_same_cache(loop, tiny, orders, sizes, graphs)
    for order, got in zip(orders, loads(many, orders, sizes, graphs)):
        for a, b in zip(got, reference_load(host, m, k, order, sizes, graphs)):
            assert a.shape == b.shape and np.array_equal(a, b), order
    ugs_sampler.clear_cache()


def test_two_threads_with_their_own_seed_tables():
    """both threads sample the SAME batch (one plan, one scratch) with different seed lists: each job carries its own table"""
    import ugs_sampler
    ei, ptr = wl.tu_batch(39, 73, 48)
    G, m, k = 48, 24, 6
    tables = [[42 + g for g in range(G)], [-1000 - 7 * g for g in range(G)]]
    cache = oracle.Cache()
    wants = [oracle_loop(ei, ptr, m, k, "sample", t, cache) for t in tables]
    cache.close()
    ugs_sampler.clear_cache()
    eit, ptrt = torch.from_numpy(ei), torch.from_numpy(ptr)
    errors = []

    def work(t):
        try:
            for it in range(40):
                got = ugs_sampler.sample_graphs(eit, ptrt, m, k, tables[t], device=None if it % 2 else "cuda:0")
                same(got, wants[t], (t, it))
        except BaseException as ex:  # noqa: BLE001
            errors.append((t, repr(ex)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    ugs_sampler.clear_cache()
