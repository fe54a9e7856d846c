#!/usr/bin/env python3
"""Timing of epsilon_uniform_sampler.GraphCache against the uncached epsilon_uniform_sampler.sample_batch, per shape, three arms
taken in turn inside every round, each entry the median of --iters calls (host time of the call up to the device's idle):

    uncached          ugs_eps_sample_batch_begin / finish on the batch: adjacency built on the host and uploaded, every call
    cached_check      GraphCache.sample_batch with the check (the batch's edge_index goes up and is compared)
    cached_nocheck    GraphCache.sample_batch(check=False, edge_index=None)

All three take a host batch and return device tensors (the cache's placement); the uncached arm goes through the same
ugs_sampler._graphs.run_job the package's sample_batch uses, with device="cuda:0", so that no arm pays a copy another does not.
Every call gets a new batch of --graphs graphs drawn from a pool of --pool dataset graphs, built before the timed span.

Shapes: proteins_k6 (tu_graph(39, 73), k = 6, m = 100: the reference's PROTEINS configs) and subgnn_k5 / subgnn_k8 (tu_graph graphs
of 10 ... 200 vertices with three undirected edges per vertex, m = 50: the shape of configs/ss_gnn/SubGNN, the densest graphs
this sampler sees).  The verdict per cached arm: "cached below uncached" only where the two arms' ranges over the rounds are
disjoint, "cached above uncached" likewise, "no verdict" otherwise.  Then one add_many of a 1 113-graph PROTEINS-shaped dataset.

    python tools/eps_cache_bench.py --rounds 5 --out profiles/eps_graph_cache.json
    python tools/eps_cache_bench.py --cache-call subgnn_k8 --iters 200      # cached calls alone, for a kernel trace
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
import epsilon_uniform_sampler as eps  # noqa: E402
import ugs_workloads as wl  # noqa: E402
from ugs_sampler import _graphs  # noqa: E402
from ugs_sampler._lib import lib  # noqa: E402

ARMS = ("uncached", "cached_check", "cached_nocheck")
EPSILON = 0.1


def shapes(pool):
    rnd = random.Random(7)
    sizes = [rnd.randint(10, 200) for _ in range(pool)]
    subgnn = [(torch.from_numpy(wl.tu_graph(n, 3 * n, 60000 + g)), n) for g, n in enumerate(sizes)]
    proteins = [(torch.from_numpy(wl.tu_graph(39, 73, 90000 + g)), 39) for g in range(pool)]
    return {"proteins_k6": (proteins, 100, 6, "tu_graph(39, 73), k = 6, m = 100"),
            "subgnn_k5": (subgnn, 50, 5, "tu_graph(n, 3 n), n = 10 ... 200, k = 5, m = 50"),
            "subgnn_k8": (subgnn, 50, 8, "tu_graph(n, 3 n), n = 10 ... 200, k = 8, m = 50")}


def batch(pool, picks):
    ptr, cols = [0], []
    for p in picks:
        a, n = pool[p]
        cols.append(a + ptr[-1])
        ptr.append(ptr[-1] + n)
    return picks, torch.cat(cols, dim=1).contiguous(), torch.tensor(ptr, dtype=torch.int64)


def uncached(b, m, k):
    """the package's sample_batch with a host batch in and device tensors out"""
    return _graphs.run_job(lambda bt, out: lib.ugs_eps_sample_batch_begin(*bt, 0, C.c_uint64(42), C.c_double(EPSILON), *out),
                           lib.ugs_eps_sample_batch_finish, b[1], b[2], m, k, "cuda:0")


def timed(fn, items, warmup):
    ts = []
    for i, it in enumerate(items):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(it)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def verdict(base, new):
    if max(new) < min(base):
        word = "cached below uncached"
    elif min(new) > max(base):
        word = "cached above uncached"
    else:
        word = "no verdict"
    return dict(verdict=word, uncached_range_ms=[min(base), max(base)], cached_range_ms=[min(new), max(new)],
                median_gap_ms=round(statistics.median(base) - statistics.median(new), 4))


def bench_shape(a, name, pool, m, k, what):
    rng = random.Random(len(name))
    cache = eps.GraphCache("cuda:0")
    cache.add_many(range(len(pool)), pool)
    G = a.graphs
    arms = {"uncached": lambda b: uncached(b, m, k),
            "cached_check": lambda b: cache.sample_batch(b[0], b[2], b[1], m, k, "sample", 42, EPSILON),
            "cached_nocheck": lambda b: cache.sample_batch(b[0], b[2], None, m, k, "sample", 42, EPSILON, check=False)}
    line = dict(shape=name, what=what, graphs=G, m=m, k=k, epsilon=EPSILON, pool=len(pool), iters=a.iters, warmup=a.warmup, rounds=a.rounds,
                device=torch.cuda.get_device_name(0), placement="host batch in, device tensors out")
    try:
        b0 = batch(pool, rng.sample(range(len(pool)), G))
        want = eps.sample_batch(b0[1], b0[2], m, k, "sample", 42, EPSILON)
        for arm in ARMS:
            assert all(torch.equal(x.cpu(), y) for x, y in zip(arms[arm](b0), want)), (name, arm)
        line["columns_per_batch"] = int(b0[1].shape[1])
        ms = {arm: [] for arm in ARMS}
        for _ in range(a.rounds):
            for arm in ARMS:
                items = [batch(pool, rng.sample(range(len(pool)), G)) for _ in range(a.iters + a.warmup)]
                ms[arm].append(timed(arms[arm], items, a.warmup))
        for arm in ARMS:
            line.update({f"{arm}_ms": statistics.median(ms[arm]), f"{arm}_ms_rounds": ms[arm]})
        for arm in ARMS[1:]:
            line[f"{arm}_vs_uncached"] = verdict(ms["uncached"], ms[arm])
    finally:
        cache.close()
    return line


def add_many_line(count):
    data = [(torch.from_numpy(wl.tu_graph(39, 73, 7000 + g)), 39) for g in range(count)]
    times = []
    for _ in range(3):                                                # three fresh caches: the first call also loads the kernel
        cache = eps.GraphCache("cuda:0")
        t0 = time.perf_counter()
        cache.add_many(range(len(data)), data)
        times.append(round((time.perf_counter() - t0) * 1e3, 3))
        info = cache.info()
        cache.close()
    return dict(shape="proteins_dataset_add_many", what=f"one add_many of {count} x tu_graph(39, 73) into a fresh cache, host time of the call",
                add_many_ms=times, store=info)


def cache_call(a, table):
    """--cache-call SHAPE: nothing but one add_many and cached calls of one shape (for a kernel trace of their own)"""
    pool, m, k, _ = table[a.cache_call]
    cache = eps.GraphCache("cuda:0")
    cache.add_many(range(len(pool)), pool)
    rng = random.Random(1)
    for _ in range(a.iters):
        b = batch(pool, rng.sample(range(len(pool)), a.graphs))
        cache.sample_batch(b[0], b[2], b[1], m, k, "sample", 42, EPSILON)
    torch.cuda.synchronize()
    cache.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=32, help="graphs per batch")
    ap.add_argument("--pool", type=int, default=64, help="dataset graphs the batches are drawn from")
    ap.add_argument("--no-add-many", action="store_true")
    ap.add_argument("--cache-call", default="", metavar="SHAPE", help="run --iters cached calls of this shape and nothing else")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rounds < 5 and not a.cache_call:
        ap.error("--rounds must be at least 5: the verdict compares ranges over the rounds")
    table = shapes(a.pool)
    if a.cache_call:
        return cache_call(a, table)
    lines = []
    for name, (pool, m, k, what) in table.items():
        if a.only and name not in a.only.split(","):
            continue
        lines.append(bench_shape(a, name, pool, m, k, what))
        print(json.dumps(lines[-1]), flush=True)
    if not a.only and not a.no_add_many:
        lines.append(add_many_line(1113))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
