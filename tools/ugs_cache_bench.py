#!/usr/bin/env python3
"""Timing of ugs_sampler.GraphCache against the uncached ugs_sampler.sample_batch, per shape and placement (drop-in: pinned host
tensors out; device: device="cuda:0" out), arms taken in turn inside every round, each entry the median of --iters calls:

    a  uncached_same        the same batch every call (the batch index and the plan cache serve it)
    b  uncached_permuted    a new combination of known graphs every call (the LRU knows every graph, the batch is new)
    c  uncached_all_miss    clear_cache() before every call, outside the timed span (every graph new to the LRU)
    d  cached_check / cached_nocheck    GraphCache.sample_batch on the batches of arm b, with the check and without

The batches of arms b, c and d are drawn from a pool of --pool dataset graphs of the shape, 32 at a time, built before the
timed span.  The verdict per cached arm and baseline is tools/rwr_bench.py's: ranges disjoint and medians at least twice the wider
spread apart.  c6_cocosp_b3200 runs with set_batch_pass_max_cols(8192) in force for the uncached arms.  Then one add_many of a
1 113-graph tu_graph(39, 73) dataset and of 2 000 tu_graph(477, 1347) graphs: host time of the call and info().

    python tools/ugs_cache_bench.py --rounds 5 --out profiles/ugs_graph_cache.json
    python tools/ugs_cache_bench.py --cache-call c3_proteins_b8192 --iters 200      # cached calls alone, for a kernel trace
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
import ugs_sampler  # noqa: E402
import ugs_workloads as wl  # noqa: E402

SHAPES = ("c2_mutag_b1024", "c3_proteins_b8192", "c4_qm9_b65536", "c6_cocosp_b3200")
ARMS = ("uncached_same", "uncached_permuted", "uncached_all_miss", "cached_check", "cached_nocheck")


def verdict(base, new):
    spread = max(max(base) - min(base), max(new) - min(new))
    gap = statistics.median(base) - statistics.median(new)
    return dict(cached_below_uncached=max(new) < min(base), spread_ms=round(spread, 4), median_gap_ms=round(gap, 4),
                passes=bool(max(new) < min(base) and gap >= 2 * spread))


def pool_of(name, count):
    n, e, k, G, m = wl.TU_SHAPES[name]
    return [(torch.from_numpy(wl.tu_graph(n, e, 90000 + g)), n) for g in range(count)], G, m, k


def batch(pool, picks):
    ptr, cols = [0], []
    for p in picks:
        a, n = pool[p]
        cols.append(a + ptr[-1])
        ptr.append(ptr[-1] + n)
    return picks, torch.cat(cols, dim=1).contiguous(), torch.tensor(ptr, dtype=torch.int64)


def timed(fn, items, warmup, before=None):
    """median over items[warmup:] of the host time of fn(item) up to the device's idle; `before` runs outside the timed span"""
    ts = []
    for i, it in enumerate(items):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(it)
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


def bench_shape(a, name):
    pool, G, m, k = pool_of(name, a.pool)
    rng = random.Random(len(name))
    cache = ugs_sampler.GraphCache(k, "cuda:0")
    cache.add_many(range(len(pool)), pool)
    prev = ugs_sampler.set_batch_pass_max_cols(8192) if name == "c6_cocosp_b3200" else None
    line = dict(shape=name, graphs=G, m=m, k=k, pool=a.pool, iters=a.iters, warmup=a.warmup, rounds=a.rounds, device=torch.cuda.get_device_name(0),
                batch_pass_max_cols=ugs_sampler.batch_pass_max_cols())
    same = batch(pool, list(range(G)))
    try:
        for place, dev in (("dropin", None), ("device", "cuda:0")):
            arms = {
                "uncached_same": (lambda b: ugs_sampler.sample_batch(same[1], same[2], m, k, device=dev), None),
                "uncached_permuted": (lambda b: ugs_sampler.sample_batch(b[1], b[2], m, k, device=dev), None),
                "uncached_all_miss": (lambda b: ugs_sampler.sample_batch(b[1], b[2], m, k, device=dev), ugs_sampler.clear_cache),
                "cached_check": (lambda b: cache.sample_batch(b[0], b[2], b[1], m, device=dev), None),
                "cached_nocheck": (lambda b: cache.sample_batch(b[0], b[2], None, m, check=False, device=dev), None),
            }
            b0 = batch(pool, rng.sample(range(a.pool), G))
            want = ugs_sampler.sample_batch(b0[1], b0[2], m, k, device=dev)
            for arm in ("cached_check", "cached_nocheck"):
                assert all(torch.equal(x, y) for x, y in zip(arms[arm][0](b0), want)), (name, place, arm)
            ms = {arm: [] for arm in ARMS}
            for _ in range(a.rounds):
                for arm in ARMS:
                    fn, before = arms[arm]
                    if arm == "uncached_permuted":                   # every graph known to the LRU, every batch new
                        ugs_sampler.clear_cache()
                        for at in range(0, a.pool, G):
                            part = batch(pool, list(range(at, min(at + G, a.pool))))
                            ugs_sampler.sample_batch(part[1], part[2], 1, k)
                    items = [batch(pool, rng.sample(range(a.pool), G)) for _ in range(a.iters + a.warmup)]
                    ms[arm].append(timed(fn, items, a.warmup, before))
            for arm in ARMS:
                line.update({f"{place}_{arm}_ms": statistics.median(ms[arm]), f"{place}_{arm}_ms_rounds": ms[arm]})
            for arm in ("cached_check", "cached_nocheck"):
                for base in ("uncached_same", "uncached_permuted", "uncached_all_miss"):
                    line[f"{place}_{arm}_vs_{base}"] = verdict(ms[base], ms[arm])
    finally:
        if prev is not None:
            ugs_sampler.set_batch_pass_max_cols(prev)
        cache.close()
        ugs_sampler.clear_cache()
    return line


def add_many_line(what, n, e, count, k):
    data = [(torch.from_numpy(wl.tu_graph(n, e, 7000 + g)), n) for g in range(count)]
    times = []
    for _ in range(3):                                                # three fresh caches: the first call also loads the kernels
        cache = ugs_sampler.GraphCache(k, "cuda:0")
        t0 = time.perf_counter()
        cache.add_many(range(len(data)), data)
        times.append(round((time.perf_counter() - t0) * 1e3, 3))
        info = cache.info()
        cache.close()
    return dict(shape=what, what=f"one add_many of {count} x tu_graph({n}, {e}) into a fresh cache, k = {k}, host time of the call", add_many_ms=times, store=info)


def cache_call(a):
    """--cache-call SHAPE: nothing but cached calls of one shape (for a kernel trace of their own)"""
    pool, G, m, k = pool_of(a.cache_call, a.pool)
    cache = ugs_sampler.GraphCache(k, "cuda:0")
    cache.add_many(range(len(pool)), pool)
    rng = random.Random(1)
    for _ in range(a.iters):
        b = batch(pool, rng.sample(range(a.pool), G))
        cache.sample_batch(b[0], b[2], b[1], m)
    torch.cuda.synchronize()
    cache.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pool", type=int, default=64, help="dataset graphs the permuted batches are drawn from")
    ap.add_argument("--no-add-many", action="store_true")
    ap.add_argument("--cache-call", default="", metavar="SHAPE", help="run --iters cached calls of this shape and nothing else")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.cache_call:
        return cache_call(a)
    lines = []
    for name in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        lines.append(bench_shape(a, name))
        print(json.dumps(lines[-1]), flush=True)
    if not a.only and not a.no_add_many:
        for args in (("proteins_dataset_add_many", 39, 73, 1113, 6), ("cocosp_2000_add_many", 477, 1347, 2000, 8)):
            lines.append(add_many_line(*args))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
