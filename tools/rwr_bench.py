#!/usr/bin/env python3
"""Timing of rwr_sampler.sample_batch (HIP) on the reference configs' RWR shape (PROTEINS: 32 graphs, k = 6, m = 100) and the
fixture shapes: the drop-in call (CPU tensors in, pinned CPU tensors out) and the device-resident call (cuda:0 in and out), median
of --iters calls after --warmup, one JSON line per shape (also written to --out).  The draws per walk printed beside them come
from the CPU restatement (tests/rwr_law.py).

    python tools/rwr_bench.py [--only proteins_k6] [--iters 50] [--warmup 5] [--out profiles/rwr_bench.json]
    python tools/rwr_bench.py --streams both --rounds 5 --out profiles/rwr_row_streams.json

--streams row times the streams="row" law (one generator per row); --streams both takes the two laws in turn, --rounds medians
each, and says per shape whether the row law's range lies below the per-graph law's with the medians two spreads apart.

--cache times rwr_sampler.GraphCache against the uncached call: per shape and per value of `streams` three arms in one process --
the uncached call, the cached call with check=True, the cached call with check=False -- taken in turn inside every round, drop-in
placement and device out, the same verdict per cached arm; then one add_many of a 1 113-graph PROTEINS-shaped dataset.

    python tools/rwr_bench.py --cache --rounds 5 --out profiles/rwr_graph_cache.json
    python tools/rwr_bench.py --cache-call proteins_k6 --streams row --iters 200     # the cached call alone, for a kernel trace

With --reference MODULE.so (a hand-built reference rwr_sampler, see tools/make_golden_rwr.py; run with OMP_NUM_THREADS=1) it
times that module on the CPU instead, labelled as such.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ss-gnn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import rwr_law as R  # noqa: E402
import ugs_workloads as wl  # noqa: E402


def shapes():
    return {
        "proteins_k6": (wl.tu_batch(39, 73, 32), 100, 6, "32 x tu_graph(39, 73), k = 6, m = 100 (PROTEINS rwr configs, batch 32)"),
        "mutag_k8": (wl.tu_batch(18, 20, 32), 100, 8, "32 x tu_graph(18, 20), k = 8, m = 100"),
        "tree_k8": (wl.tu_batch(30, 29, 32), 100, 8, "32 x tu_graph(30, 29) (trees), k = 8, m = 100"),
        "proteins_k6_b128_m16": (wl.tu_batch(39, 73, 128), 16, 6, "128 x tu_graph(39, 73), k = 6, m = 16"),
    }


def draws_per_walk(ei, ptr, m, k):
    adjs = R.adjacency(ei[0], ei[1], ptr)
    lens = []
    for g, adj in enumerate(adjs):
        c = 0
        for _ in range(m):
            L = R.walk_len(adj, k, 0.2, 42 + g, c)
            lens.append(L)
            c += L
    a = np.array(lens)
    return dict(mean=round(float(a.mean()), 1), p99=float(np.percentile(a, 99)), max=int(a.max()))


def median_ms(fn, iters, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def series(rwr_sampler, e, p, m, k, streams, a, sync):
    """--rounds medians per value of `streams`, the values taken in turn inside every round"""
    out = {st: [] for st in streams}
    for _ in range(a.rounds):
        for st in streams:
            out[st].append(round(median_ms(lambda: rwr_sampler.sample_batch(e, p, m, k, streams=st), a.iters, a.warmup, sync), 4))
    return out


def verdict(graph, row):
    """The issue's test of a shape: row's range below graph's range, medians at least two of the wider spread apart."""
    spread = max(max(graph) - min(graph), max(row) - min(row))
    gap = statistics.median(graph) - statistics.median(row)
    return dict(row_below_graph=max(row) < min(graph), spread_ms=round(spread, 4), median_gap_ms=round(gap, 4),
                passes=bool(max(row) < min(graph) and gap >= 2 * spread))


def graphs_of(ei, ptr):
    """the batch's graphs as a dataset holds them: (columns with local ids, vertices); every column of a tu_batch stays in its graph"""
    out = []
    for g in range(len(ptr) - 1):
        own = (ei[0] >= ptr[g]) & (ei[0] < ptr[g + 1])
        out.append((torch.from_numpy(np.ascontiguousarray(ei[:, own] - ptr[g])), int(ptr[g + 1] - ptr[g])))
    return out


def cache_of(rwr_sampler, ei, ptr, k):
    cache = rwr_sampler.GraphCache(k, "cuda:0")
    idx = list(range(len(ptr) - 1))
    cache.add_many(idx, graphs_of(ei, ptr))
    return cache, idx


def cache_arms(rwr_sampler, cache, idx, e, p, m, k, st):
    return {"uncached": lambda: rwr_sampler.sample_batch(e, p, m, k, streams=st),
            "cached_check": lambda: cache.sample_batch(idx, p, e, m, streams=st),
            "cached_nocheck": lambda: cache.sample_batch(idx, p, e, m, streams=st, check=False)}


def cache_verdict(base, new):
    v = verdict(base, new)
    v["cached_below_uncached"] = v.pop("row_below_graph")
    return v


def cache_bench(a, rwr_sampler):
    """--cache: the three arms per shape, streams value and placement; then the one-off add of a whole dataset"""
    sync = torch.cuda.synchronize
    lines = []
    for name, ((ei, ptr), m, k, what) in shapes().items():
        if a.only and name not in a.only.split(","):
            continue
        e_h, p_h = torch.from_numpy(ei), torch.from_numpy(ptr)
        e_d, p_d = e_h.cuda(), p_h.cuda()
        cache, idx = cache_of(rwr_sampler, ei, ptr, k)
        for st in ("graph", "row"):
            line = dict(shape=name, what=what, graphs=len(ptr) - 1, k=k, m=m, streams=st, iters=a.iters, rounds=a.rounds,
                        device=torch.cuda.get_device_name(0))
            for place, (e, p) in (("dropin", (e_h, p_h)), ("device", (e_d, p_d))):
                arms = cache_arms(rwr_sampler, cache, idx, e, p, m, k, st)
                want = arms["uncached"]()
                for arm in ("cached_check", "cached_nocheck"):
                    assert all(torch.equal(x, y) for x, y in zip(arms[arm](), want)), (name, st, place, arm)
                ms = {arm: [] for arm in arms}
                for _ in range(a.rounds):
                    for arm, fn in arms.items():
                        ms[arm].append(round(median_ms(fn, a.iters, a.warmup, sync), 4))
                for arm in arms:
                    line.update({f"{place}_{arm}_ms": statistics.median(ms[arm]), f"{place}_{arm}_ms_rounds": ms[arm]})
                for arm in ("cached_check", "cached_nocheck"):
                    line[f"{place}_{arm}_verdict"] = cache_verdict(ms["uncached"], ms[arm])
            print(json.dumps(line), flush=True)
            lines.append(line)
        cache.close()
    if not a.only:
        data = [(torch.from_numpy(wl.tu_graph(39, 73, 7000 + g)), 39) for g in range(1113)]
        times = []
        for _ in range(3):                                            # three fresh caches: the first call also loads the kernels
            cache = rwr_sampler.GraphCache(6, "cuda:0")
            t0 = time.perf_counter()
            cache.add_many(range(len(data)), data)
            times.append(round((time.perf_counter() - t0) * 1e3, 3))
            info = cache.info()
            cache.close()
        line = dict(shape="proteins_dataset_add_many", what="one add_many of 1113 x tu_graph(39, 73) into a fresh cache, k = 6, host time of the call",
                    add_many_ms=times, store=info)
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def cache_call(a, rwr_sampler):
    """--cache-call SHAPE: nothing but cached calls of one shape (for a kernel trace of their own)"""
    (ei, ptr), m, k, _ = shapes()[a.cache_call]
    cache, idx = cache_of(rwr_sampler, ei, ptr, k)
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    for st in (("graph", "row") if a.streams == "both" else (a.streams,)):
        for _ in range(a.iters):
            cache.sample_batch(idx, p, e, m, streams=st)
    torch.cuda.synchronize()
    cache.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", choices=("graph", "row", "both"), default="graph",
                    help="the law: one generator per graph (default), one per row, or both in turn (--rounds times)")
    ap.add_argument("--rounds", type=int, default=1, help="medians taken per value of --streams, alternating")
    ap.add_argument("--cache", action="store_true", help="GraphCache against the uncached call: three arms, both streams, both placements")
    ap.add_argument("--cache-call", default="", metavar="SHAPE", help="run --iters cached calls of this shape and nothing else")
    ap.add_argument("--reference", default="", help="time this hand-built reference module on the CPU instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    streams = ("graph", "row") if a.streams == "both" else (a.streams,)
    lines = []
    if a.reference:
        spec = importlib.util.spec_from_file_location("rwr_sampler", a.reference)
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    else:
        import rwr_sampler
    if a.cache_call:
        return cache_call(a, rwr_sampler)
    if a.cache:
        lines = cache_bench(a, rwr_sampler)
    for name, ((ei, ptr), m, k, what) in ({} if a.cache else shapes()).items():
        if a.only and name not in a.only.split(","):
            continue
        e_h, p_h = torch.from_numpy(ei), torch.from_numpy(ptr)
        line = dict(shape=name, what=what, graphs=len(ptr) - 1, k=k, m=m)
        if a.reference:
            ms = median_ms(lambda: ref.sample_batch(e_h, p_h, m, k), a.iters, a.warmup, lambda: None)
            line.update(reference_cpu_ms=round(ms, 4), omp_num_threads=os.environ.get("OMP_NUM_THREADS"),
                        what_ran="reference rwr_sampler on the CPU, one OpenMP thread")
        else:
            sync = torch.cuda.synchronize
            e_d, p_d = e_h.cuda(), p_h.cuda()
            host = series(rwr_sampler, e_h, p_h, m, k, streams, a, sync)
            dev = series(rwr_sampler, e_d, p_d, m, k, streams, a, sync)
            line.update(draws_per_walk=draws_per_walk(ei, ptr, m, k), iters=a.iters, rounds=a.rounds,
                        device=torch.cuda.get_device_name(0))
            for st in streams:
                out = rwr_sampler.sample_batch(e_h, p_h, m, k, streams=st)
                tag = "" if st == "graph" else "row_"
                line.update({tag + "failed_rows": int((out[0][:, 0] < 0).sum()), tag + "edge_entries": int(out[1].shape[1]),
                             tag + "dropin_ms": statistics.median(host[st]), tag + "device_ms": statistics.median(dev[st])})
                if a.rounds > 1:
                    line.update({tag + "dropin_ms_rounds": host[st], tag + "device_ms_rounds": dev[st]})
            if len(streams) == 2 and a.rounds > 1:
                line.update(dropin_verdict=verdict(host["graph"], host["row"]), device_verdict=verdict(dev["graph"], dev["row"]))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
