#!/usr/bin/env python3
"""Timing of rwr_sampler.sample_batch (HIP) on the reference configs' RWR shape (PROTEINS: 32 graphs, k = 6, m = 100) and the
fixture shapes: the drop-in call (CPU tensors in, pinned CPU tensors out) and the device-resident call (cuda:0 in and out), median
of --iters calls after --warmup, one JSON line per shape (also written to --out).  The draws per walk printed beside them come
from the CPU restatement (tests/rwr_law.py).

    python tools/rwr_bench.py [--only proteins_k6] [--iters 50] [--warmup 5] [--out profiles/rwr_bench.json]
    python tools/rwr_bench.py --streams both --rounds 5 --out profiles/rwr_row_streams.json

--streams row times the streams="row" law (one generator per row); --streams both takes the two laws in turn, --rounds medians
each, and says per shape whether the row law's range lies below the per-graph law's with the medians two spreads apart.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", choices=("graph", "row", "both"), default="graph",
                    help="the law: one generator per graph (default), one per row, or both in turn (--rounds times)")
    ap.add_argument("--rounds", type=int, default=1, help="medians taken per value of --streams, alternating")
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
    for name, ((ei, ptr), m, k, what) in shapes().items():
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
