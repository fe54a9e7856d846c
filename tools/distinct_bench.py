#!/usr/bin/env python3
"""PopulationCache.sample_distinct (draws without replacement) against PopulationCache.sample_graphs (the
same build, unchanged code: the yardstick) on the call shapes of section 10.2's table (tools/population_bench.py).

Per shape: host-in / pinned-out calls of pop.sample_graphs and pop.sample_distinct with the same seeds array, interleaved call by
call, --warmup rounds dropped, median, min and max of --iters; the distinct call's rows are checked to be distinct per graph once.
On the CSL k = 6 shape a second line measures m = 1312 (--bag-m; the whole population wherever a graph has at most that many sets:
`full_bag_graphs` says for how many graphs of the batch that holds).  One JSON line per measurement, also written to --out.

    python tools/distinct_bench.py [--only csl_k6] [--iters 20] [--warmup 5] [--out profiles/uniform_distinct.json]
    python tools/distinct_bench.py --trace csl_k6 --trace-dir <dir>      # rocprofv3 --kernel-trace --stats over a child of its own
    python tools/distinct_bench.py --calls-only csl_k6                   # the child: add_many, 47 calls of either kind, nothing else
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import population_bench as pb  # noqa: E402
import uniform_sampler  # noqa: E402


def setup(name):
    ei, ptr, m, k, what, limit = pb.shape(name)
    if limit:
        uniform_sampler.set_max_vertices(limit)
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    idx = list(range(len(ptr) - 1))
    pop = pb.build(ei, ptr, k)[0]
    seeds = [42 + g for g in idx]
    return pop, idx, p, e, m, k, what, seeds


def measure(name, iters, warmup, m_override=None):
    pop, idx, p, e, m, k, what, seeds = setup(name)
    m = m_override or m
    forms = {"with_replacement": lambda: pop.sample_graphs(idx, p, e, m, seeds),
             "distinct": lambda: pop.sample_distinct(idx, p, e, m, seeds)}
    got = forms["distinct"]()
    nodes, valid, sizes = got[0].reshape(len(idx), m, k), got[6].tolist(), pop.sizes(idx).tolist()
    distinct = all(len({tuple(r) for r in nodes[g, :valid[g]].tolist()}) == valid[g] and bool((nodes[g, valid[g]:] == -1).all()) for g in idx)
    ts = {f: [] for f in forms}
    for r in range(warmup + iters):
        for f, fn in forms.items():                                 # interleaved: every round runs each form once
            t = pb.timed(fn)
            if r >= warmup:
                ts[f].append(t)
    line = dict(shape=name, what=what, graphs=len(idx), m=m, k=k, sets=pop.info()["keys"], population_min=min(sizes), population_max=max(sizes),
                valid_min=min(valid), valid_max=max(valid), full_bag_graphs=sum(1 for s in sizes if 0 <= s <= m), rows_distinct=distinct,
                iters=iters, warmup=warmup, device=torch.cuda.get_device_name(0))
    for f in forms:
        line[f] = pb.stats(ts[f])
    line["distinct_over_with_replacement"] = round(line["distinct"]["median_ms"] / line["with_replacement"]["median_ms"], 3)
    spread = line["with_replacement"]["max_ms"] - line["with_replacement"]["min_ms"]
    line["slower_by_more_than_the_yardsticks_spread"] = line["distinct"]["median_ms"] - line["with_replacement"]["median_ms"] > spread
    pop.close()
    return line


def calls_only(name, calls=47):
    pop, idx, p, e, m, k, _, seeds = setup(name)
    for _ in range(calls):
        pop.sample_graphs(idx, p, e, m, seeds)
        pop.sample_distinct(idx, p, e, m, seeds)
    torch.cuda.synchronize()


def trace(name, out_dir, calls=47):
    """Kernel times of `calls` calls of either kind (and the one add_many before them) from a rocprofv3 run of its own:
    {kernel: [calls, total us]}"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--calls-only", name]
    subprocess.run(cmd, check=True, timeout=280)
    rows = {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                kernel = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
                lib_kernel = re.search(r"wrapped_(\w+)_config", kernel)      # rocPRIM's kernels: the algorithm's name is enough
                kernel = "rocprim " + lib_kernel.group(1) if lib_kernel else kernel.split("(")[0]
                n, us = rows.get(kernel, [0, 0.0])
                rows[kernel] = [n + int(r["Calls"]), round(us + float(r["TotalDurationNs"]) / 1e3, 1)]
    return dict(shape=name, calls_of_either_kind=calls, kernels=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bag-m", type=int, default=1312)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniform_distinct.json"))
    ap.add_argument("--trace", default="")
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--calls-only", default="")
    a = ap.parse_args()
    if a.calls_only:
        calls_only(a.calls_only)
        return
    lines = []
    if a.trace:
        lines.append(trace(a.trace, a.trace_dir or tempfile.mkdtemp(prefix="distinct_trace_")))
        print(json.dumps(lines[-1]), flush=True)
    else:
        for name in pb.SHAPES:
            if a.only and name not in a.only.split(","):
                continue
            lines.append(measure(name, a.iters, a.warmup))
            print(json.dumps(lines[-1]), flush=True)
            if name == "csl_k6" and a.bag_m:
                lines.append(measure(name, a.iters, a.warmup, a.bag_m))
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a" if a.trace else "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
