#!/usr/bin/env python3
"""Timing of uniform_sampler.enumerate_graphs (HIP): begin (count, scan, write, sorts, rows) and finish (edge fill) apart, device
outputs, medians of --iters calls after --warmup.  Beside them, on the same inputs, sample_graphs with m = 1, whose begin pays the
same count pass, scan, write pass and sorts and then one row per graph.  One JSON line per shape, also written to --out.

    python tools/enumerate_bench.py [--only csl150_k6] [--iters 5] [--warmup 1] [--out profiles/uniform_enumerate.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
import ugs_workloads as wl  # noqa: E402
import uniform_sampler  # noqa: E402
from ugs_sampler import _graphs  # noqa: E402
from ugs_sampler._lib import check, lib, vp  # noqa: E402

CSL_SKIPS = (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)


def batch(graphs):
    cols, ptr = [], [0]
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    return np.ascontiguousarray(np.concatenate(cols, axis=1)), np.array(ptr, np.int64)


def shapes():
    return {
        "csl150_k6": (batch([(41, wl.csl_graph(41, CSL_SKIPS[i % len(CSL_SKIPS)])) for i in range(150)]), 6, "150 x csl_graph(41, s), k = 6"),
        "dense64_k6": (batch([(64, wl.tu_graph(64, 300, 3))]), 6, "tu_graph(64, 300, 3), k = 6"),
    }


def two_phase(begin, finish, ei, ptr, k, rows_of):
    """One call on device tensors, begin and finish timed apart (both return with the stream drained).  Returns (begin ms, finish ms,
    rows, edge entries)."""
    keep, p, stride, e = _graphs._edge_index_view(ei)
    G = ptr.numel() - 1
    _graphs._select_device(torch.device("cuda:0"), jobs=True)
    job, rows, total = vp(), C.c_int64(), C.c_int64()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check(begin((p, stride, e, ptr.data_ptr(), G), k, (job, rows, total)))
    t1 = time.perf_counter()
    R = rows_of(G, rows.value)
    opts = dict(dtype=torch.int64, device="cuda:0")
    out = [torch.empty((R, k), **opts), torch.empty((2, total.value), **opts), torch.empty((R + 1,), **opts), torch.empty((G + 1,), **opts),
           torch.empty((total.value,), **opts)]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    check(finish(job, *[t.data_ptr() for t in out], 1))
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t3 - t2) * 1e3, R, total.value


def medians(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    runs = [fn() for _ in range(iters)]
    return [round(statistics.median(r[i] for r in runs), 4) for i in (0, 1)] + list(runs[0][2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniform_enumerate.json"))
    a = ap.parse_args()
    lines = []
    for name, ((ei, ptr), k, what) in shapes().items():
        if a.only and name not in a.only.split(","):
            continue
        e_h, p_h = torch.from_numpy(ei), torch.from_numpy(ptr)
        G = len(ptr) - 1
        status = np.zeros(G, np.int32)
        seeds = np.arange(42, 42 + G, dtype=np.uint64)

        def enum_begin(b, kk, out):
            return lib.ugs_uniform_enumerate_begin(*b, kk, 0, 1 << 22, status.ctypes.data, C.byref(out[0]), C.byref(out[1]), C.byref(out[2]))

        def graphs_begin(b, kk, out):
            return lib.ugs_uniform_sample_graphs_begin(*b, 1, kk, 0, seeds.ctypes.data, status.ctypes.data, C.byref(out[0]), C.byref(out[2]))

        en = medians(lambda: two_phase(enum_begin, lib.ugs_uniform_enumerate_finish, e_h, p_h, k, lambda G, r: r), a.iters, a.warmup)
        sg = medians(lambda: two_phase(graphs_begin, lib.ugs_uniform_sample_batch_finish, e_h, p_h, k, lambda G, r: G), a.iters, a.warmup)

        def count_ms():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            uniform_sampler.count_graphs(e_h, p_h, k)
            return ((time.perf_counter() - t0) * 1e3, 0.0)

        ct = medians(lambda: count_ms() + (0, 0), a.iters, a.warmup)
        line = dict(shape=name, what=what, graphs=G, k=k, rows=en[2], edge_entries=en[3], enumerate_begin_ms=en[0], enumerate_finish_ms=en[1],
                    sample_graphs_m1_begin_ms=sg[0], sample_graphs_m1_finish_ms=sg[1], count_graphs_ms=ct[0], iters=a.iters, warmup=a.warmup,
                    device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
