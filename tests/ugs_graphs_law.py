"""Shared by the sample_graphs tests: the f16 fixture (reference one-graph calls of the trainer's presample loop) and the
right-hand side of the law of ugs_sampler.sample_graphs built from the CPU oracle's one-graph calls on ONE oracle.Cache."""
import os

import numpy as np

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16_ugs_presample_reference.npz")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def fixture():
    """(graphs [(n, edge_index)], seeds, m, {k: [five arrays per graph]}) of f16"""
    z = np.load(GOLDEN)
    cp, n = z["col_ptr"], z["n"]
    graphs = [(int(n[i]), np.ascontiguousarray(z["in_edge_index"][:, cp[i]:cp[i + 1]])) for i in range(len(n))]
    m = z["k4/edge_ptr"].shape[1] - 1
    want = {}
    for k in (4, 5):
        ep = z[f"k{k}/e_ptr"]
        want[k] = [(z[f"k{k}/nodes"][i * m:(i + 1) * m], z[f"k{k}/edge_index"][:, ep[i]:ep[i + 1]], z[f"k{k}/edge_ptr"][i],
                    z[f"k{k}/sample_ptr"][i], z[f"k{k}/edge_src"][ep[i]:ep[i + 1]]) for i in range(len(n))]
    return graphs, [int(s) for s in z["seeds"]], int(m), want


def concat(graphs):
    """[(n, local edge_index)] as one batch: columns outside [0, n) become (-1, -1) (in no graph's range), as PresampleCache does"""
    cols, ptr = [], [0]
    for n, ei in graphs:
        bad = ((ei < 0) | (ei >= n)).any(axis=0)
        cols.append(np.where(bad, -1, ei + ptr[-1]))
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64), np.cumsum([0] + [g[1].shape[1] for g in graphs])


def block(out, g, m, lo=0, col0=0):
    """graph g's block of a batched "sample"-mode result in the one-graph form: edge_ptr re-based, lo subtracted from the nodes,
    col0 from edge_src"""
    nodes, eidx, eptr, _, esrc = [np.asarray(t) for t in out[:5]]
    a, b = int(eptr[g * m]), int(eptr[(g + 1) * m])
    nd = nodes[g * m:(g + 1) * m]
    return (np.where(nd >= 0, nd - lo, nd), eidx[:, a:b], eptr[g * m:(g + 1) * m + 1] - a, np.array([0, m], np.int64), esrc[a:b] - col0)


def oracle_loop(ei, ptr, m, k, mode, seeds, cache):
    """What sample_graphs must return: for g = 0, 1, ... the oracle's one-graph call on the batch's own numbering (ptr {ptr[g],
    ptr[g+1]}, seed seeds[g]) on the shared LRU `cache`, the blocks put one behind the other."""
    G = len(ptr) - 1
    parts = [oracle.sample_batch(ei, ptr[g:g + 2], m, k, mode, int(seeds[g]), cache) for g in range(G)]
    nodes = np.concatenate([p[0] for p in parts], axis=0) if G else np.zeros((0, k), np.int64)
    eidx = np.concatenate([p[1] for p in parts], axis=1) if G else np.zeros((2, 0), np.int64)
    esrc = np.concatenate([p[4] for p in parts]) if G else np.zeros(0, np.int64)
    eptr, base = [np.zeros(1, np.int64)], 0
    for p in parts:
        eptr.append(p[2][1:] + base)
        base += int(p[2][-1])
    return nodes, eidx, np.concatenate(eptr), np.arange(G + 1, dtype=np.int64) * m, esrc


SEED_POOL = [0, -1, 2 ** 31 - 1, -(2 ** 31), 42, 42, 7]


def random_batch(rng):
    """G in 1 .. a few hundred connected graphs of 0 .. 60 vertices, both directions or one, columns shuffled, stray columns between
    graphs; seeds with 0, -1, the ends of the C int range and repeats"""
    G = rng.choice([1, 2, 3, 7, 40, 130, 300])
    cols, ptr = [], [0]
    for _ in range(G):
        n = rng.choice([0, 1, 2, 3]) if rng.random() < 0.1 else rng.randint(4, 60 if G < 100 else 24)
        off = ptr[-1]
        e = [(off + rng.randrange(v), off + v) for v in range(1, n)]                       # a spanning tree: connected
        e += [(off + rng.randrange(n), off + rng.randrange(n)) for _ in range(rng.randint(0, n // 2 + 1))] if n else []
        if rng.random() < 0.7:
            e = e + [(v, u) for u, v in e]
        cols += e
        ptr.append(off + n)
    if ptr[-1] > 0:
        cols += [(rng.randrange(ptr[-1]), rng.randrange(ptr[-1])) for _ in range(rng.randint(0, 6))]   # mostly between graphs
    if rng.random() < 0.6:
        rng.shuffle(cols)
    ei = np.array(cols, dtype=np.int64).reshape(-1, 2).T.copy()
    seeds = [rng.choice(SEED_POOL) if rng.random() < 0.5 else rng.randint(-(2 ** 31), 2 ** 31 - 1) for _ in range(G)]
    return ei, np.array(ptr, np.int64), rng.choice([1, 5, 9]), rng.choice([1, 2, 3, 4, 6, 8]), rng.choice(["sample", "graph", "global"]), seeds


def check_random_batches(capacity, calls, seed):
    """`calls` random batches through ugs_sampler.sample_graphs and through the oracle's one-graph loop on one LRU of `capacity`
    entries (the product's comes from UGS_CACHE_SIZE, fixed at first use): all five tensors and the LRU's hit / miss counts equal."""
    import random

    import torch

    import ugs_sampler
    rng = random.Random(seed)
    ugs_sampler.clear_cache()
    cache = oracle.Cache(capacity)
    st0 = ugs_sampler.cache_stats()
    for it in range(calls):
        ei, ptr, m, k, mode, seeds = random_batch(rng)
        want = oracle_loop(ei, ptr, m, k, mode, seeds, cache)
        sd = seeds if it % 3 == 0 else (torch.tensor(seeds, dtype=torch.int64) if it % 3 == 1 else np.array(seeds, np.int64))
        got = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, sd, mode)
        assert len(got) == 6 and got[5].dtype == torch.bool and got[5].shape == (len(ptr) - 1,) and not got[5].any()
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(g.numpy(), w), (it, name, len(ptr) - 1, ei.shape[1], m, k, mode)
        st, ost = ugs_sampler.cache_stats(), cache.stats()
        assert (st["hits"] - st0["hits"], st["misses"] - st0["misses"]) == (ost["hits"], ost["misses"]), (it, st, st0, ost)
    ugs_sampler.clear_cache()
    cache.close()
