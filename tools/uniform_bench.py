#!/usr/bin/env python3
"""Timing of uniform_sampler.sample_batch (HIP) on the reference configs' shapes: the drop-in call (CPU tensors in, pinned CPU
tensors out) and the device-resident call (cuda:0 in and out), median of --iters calls after --warmup, one JSON line per shape
(also written to --out).  The connected k-subset counts printed beside them come from the CPU restatement (tests/uniform_law.py).

    python tools/uniform_bench.py [--only csl_k6] [--iters 20] [--warmup 3] [--out profiles/uniform_bench.json]
"""
import argparse
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
import ugs_workloads as wl  # noqa: E402
import uniform_law as U  # noqa: E402
import uniform_sampler  # noqa: E402

CSL_SKIPS = (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)


def batch(graphs):
    cols, ptr = [], [0]
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    return np.ascontiguousarray(np.concatenate(cols, axis=1)), np.array(ptr, np.int64)


def shapes():
    csl = batch([(41, wl.csl_graph(41, s)) for s in CSL_SKIPS])
    return {
        "csl_k6": (csl, 100, 6, "CSL 10 x 41, k = 6, m = 100 (gin-k6.json, batch 10)"),
        "csl_k7": (csl, 100, 7, "CSL 10 x 41, k = 7, m = 100 (gin-k7-wl.json)"),
        "mutag_k6": (batch([(18, wl.tu_graph(18, 20, g)) for g in range(64)]), 64, 6, "64 x tu_graph(18, 20), k = 6, m = 64 (gcn-mutag.json)"),
        "mutag_max_k6": (batch([(28, wl.tu_graph(28, 31, g)) for g in range(64)]), 64, 6, "64 x tu_graph(28, 31), k = 6, m = 64"),
        "dense64_k5": (batch([(64, wl.tu_graph(64, 300, g)) for g in range(32)]), 200, 5, "32 x tu_graph(64, 300), k = 5, m = 200"),
    }


def subset_count(ei, ptr, k):
    total = 0
    for g in range(len(ptr) - 1):
        lo, n = int(ptr[g]), int(ptr[g + 1] - ptr[g])
        total += len(U.esu_masks(U.graph_adjacency(ei[0], ei[1], lo, n), k))
    return total


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sync = torch.cuda.synchronize
    lines = []
    for name, ((ei, ptr), m, k, what) in shapes().items():
        if a.only and name not in a.only.split(","):
            continue
        e_h, p_h = torch.from_numpy(ei), torch.from_numpy(ptr)
        e_d, p_d = e_h.cuda(), p_h.cuda()
        host = median_ms(lambda: uniform_sampler.sample_batch(e_h, p_h, m, k), a.iters, a.warmup, sync)
        dev = median_ms(lambda: uniform_sampler.sample_batch(e_d, p_d, m, k), a.iters, a.warmup, sync)
        out = uniform_sampler.sample_batch(e_h, p_h, m, k)
        line = dict(shape=name, what=what, graphs=len(ptr) - 1, k=k, m=m, connected_subsets=subset_count(ei, ptr, k),
                    edge_entries=int(out[1].shape[1]), dropin_ms=round(host, 4), device_ms=round(dev, 4), iters=a.iters,
                    device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
