#!/usr/bin/env python3
"""uniform_sampler.PopulationCache against uniform_sampler.sample_batch (the same build, untouched code) on the call shapes of
DESIGN.md section 10 (tools/uniform_bench.py: the five mask-form shapes and the PROTEINS-shaped wide batch).

Per shape: add_many time and the population's bytes; then host-in / pinned-out calls of sample_batch, pop.sample_batch (check=True)
and pop.sample_batch(check=False), interleaved call by call, --warmup rounds dropped, median, min and max of --iters.  The outputs of
the cached call are compared with the uncached call's once per shape.  One JSON line per shape, also written to --out.

    python tools/population_bench.py [--only csl_k6] [--iters 20] [--warmup 5] [--out profiles/uniform_population.json]
    python tools/population_bench.py --trace csl_k6 --trace-dir <dir>      # rocprofv3 --kernel-trace --stats over a child of its own
    python tools/population_bench.py --calls-only csl_k6                   # the child: add_many and 47 cached calls, nothing else
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import uniform_bench  # noqa: E402
import uniform_sampler  # noqa: E402

SHAPES = ("csl_k6", "csl_k7", "mutag_k6", "mutag_max_k6", "dense64_k5", "proteins_k6")
DEV = "cuda:0"


def shape(name):
    spec = uniform_bench.shapes()[name]
    (ei, ptr), m, k, what = spec[:4]
    limit = (spec[4] if len(spec) > 4 else {}).get("limit")
    return ei, ptr, m, k, what, limit


def local_graphs(ei, ptr):
    """the batch taken apart into what a dataset holds: (local edge_index, num_nodes) per graph (no column of these shapes crosses)"""
    first = torch.searchsorted(torch.from_numpy(ptr), torch.from_numpy(ei[0]), right=True) - 1
    e = torch.from_numpy(ei)
    return [(e[:, first == g] - int(ptr[g]), int(ptr[g + 1] - ptr[g])) for g in range(len(ptr) - 1)]


def build(ei, ptr, k):
    pop = uniform_sampler.PopulationCache(k, DEV)
    graphs = local_graphs(ei, ptr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pop.add_many(range(len(graphs)), graphs)
    return pop, (time.perf_counter() - t0) * 1e3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def measure(name, iters, warmup):
    ei, ptr, m, k, what, limit = shape(name)
    if limit:
        uniform_sampler.set_max_vertices(limit)
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    idx = list(range(len(ptr) - 1))
    pop, add_ms = build(ei, ptr, k)
    forms = {"uncached": lambda: uniform_sampler.sample_batch(e, p, m, k, "sample", 42),
             "cached": lambda: pop.sample_batch(idx, p, e, m, "sample", 42),
             "cached_unchecked": lambda: pop.sample_batch(idx, p, e, m, "sample", 42, check=False)}
    same = all(torch.equal(a, b) for a, b in zip(forms["uncached"](), forms["cached"]()))
    ts = {f: [] for f in forms}
    for r in range(warmup + iters):
        for f, fn in forms.items():                                 # interleaved: every round runs each form once
            t = timed(fn)
            if r >= warmup:
                ts[f].append(t)
    info = pop.info()
    line = dict(shape=name, what=what, graphs=len(idx), m=m, k=k, sets=info["keys"], population_bytes=info["bytes"], blocks=info["blocks"],
                add_many_ms=round(add_ms, 3), equal_to_uncached=same, iters=iters, warmup=warmup, device=torch.cuda.get_device_name(0))
    for f in forms:
        line[f] = stats(ts[f])
    line["cached_over_uncached"] = round(line["cached"]["median_ms"] / line["uncached"]["median_ms"], 3)
    pop.close()
    return line


def calls_only(name, calls=47):
    ei, ptr, m, k, _, limit = shape(name)
    if limit:
        uniform_sampler.set_max_vertices(limit)
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    idx = list(range(len(ptr) - 1))
    pop = build(ei, ptr, k)[0]
    for _ in range(calls):
        pop.sample_batch(idx, p, e, m, "sample", 42)
    torch.cuda.synchronize()


def trace(name, out_dir, calls=47):
    """Kernel times of `calls` cached calls (and the one add_many before them) from a rocprofv3 run of its own: {kernel: [calls, total us]}"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--calls-only", name]
    subprocess.run(cmd, check=True, timeout=280)
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
                lib_kernel = re.search(r"wrapped_(\w+)_config", name)        # rocPRIM's kernels: the algorithm's name is enough
                name = "rocprim " + lib_kernel.group(1) if lib_kernel else name.split("(")[0]
                calls, us = rows.get(name, [0, 0.0])
                rows[name] = [calls + int(r["Calls"]), round(us + float(r["TotalDurationNs"]) / 1e3, 1)]
    return dict(shape=name, calls=calls, kernels=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniform_population.json"))
    ap.add_argument("--trace", default="")
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--calls-only", default="")
    a = ap.parse_args()
    if a.calls_only:
        calls_only(a.calls_only)
        return
    lines = []
    if a.trace:
        lines.append(trace(a.trace, a.trace_dir or tempfile.mkdtemp(prefix="population_trace_")))
        print(json.dumps(lines[-1]), flush=True)
    else:
        for name in SHAPES:
            if a.only and name not in a.only.split(","):
                continue
            lines.append(measure(name, a.iters, a.warmup))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a" if a.trace else "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
