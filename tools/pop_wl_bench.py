#!/usr/bin/env python3
"""The WL population (uniform_sampler.PopulationCache(..., wl_iterations=3)) on the call shapes of DESIGN.md section 10.2: the CSL
10 x 41, k = 6, m = 100 call and the PROTEINS-shaped call, the latter once degree-labelled and once with node-feature labels.

Per shape, host batch in and device tensors out, interleaved call by call in one process, --warmup rounds dropped, median, min and max
of --iters:
  a  pop.sample_batch, then WLVocab.ids on its output     (the two calls a trainer made before: cached sampling, then hashing)
  b  pop.sample_batch(..., wl=table)                      (the ids gathered from the cache)
  c  pop.sample_batch alone
and, once, the add_many time and the bytes held with and without wl_iterations.  The ids of (a) and (b) are compared once per
shape.  One JSON line per shape, also written to --out.

    python tools/pop_wl_bench.py [--only csl_k6] [--iters 20] [--warmup 5] [--out profiles/pop_wl.json]
    python tools/pop_wl_bench.py --trace csl_k6 --trace-dir <dir>      # rocprofv3 --kernel-trace --stats over a child of its own
    python tools/pop_wl_bench.py --calls-only csl_k6                   # the child: add_many and 47 calls of form b, nothing else
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
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import population_bench  # noqa: E402
import uniform_sampler  # noqa: E402
from ugs_sampler import wl  # noqa: E402

SHAPES = {"csl_k6": ("csl_k6", False), "proteins_k6": ("proteins_k6", False), "proteins_k6_labeled": ("proteins_k6", True)}
DEV = "cuda:0"
ITERATIONS = 3


def features(ptr):
    """PROTEINS-like node features: one of three one-hot rows per vertex, float32"""
    g = torch.Generator().manual_seed(5)
    kind = torch.randint(0, 3, (int(ptr[-1]),), generator=g)
    x = torch.nn.functional.one_hot(kind, 3).to(torch.float32)
    return [x[int(ptr[i]):int(ptr[i + 1])] for i in range(len(ptr) - 1)], x


def timed(fn):
    """the call and the device work it queued"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def build(ei, ptr, k, iterations, xs):
    pop = uniform_sampler.PopulationCache(k, DEV, wl_iterations=iterations)
    graphs = population_bench.local_graphs(ei, ptr)
    kw = {"x": xs} if xs is not None and iterations is not None else {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pop.add_many(range(len(graphs)), graphs, **kw)
    torch.cuda.synchronize()
    return pop, (time.perf_counter() - t0) * 1e3


def setup(name):
    base, labeled = SHAPES[name]
    ei, ptr, m, k, what, limit = population_bench.shape(base)
    if limit:
        uniform_sampler.set_max_vertices(limit)
    xs, x = features(ptr) if labeled else (None, None)
    return ei, ptr, m, k, what, xs, x


def measure(name, iters, warmup):
    ei, ptr, m, k, what, xs, x = setup(name)
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    idx = list(range(len(ptr) - 1))
    plain, plain_ms = build(ei, ptr, k, None, None)
    pop, add_ms = build(ei, ptr, k, ITERATIONS, xs)
    table = wl.WLVocab(wl.extend_vocab({}, *pop.wl_digests()), DEV)
    labels = None if x is None else wl.feature_labels(x.to(DEV))       # form a hashes with the labels of the batch, made once

    def form_a():
        five = pop.sample_batch(idx, p, e, m, "sample", 42, device=DEV)
        return table.ids(five[0], five[1], five[2], iterations=ITERATIONS, node_labels=labels)

    forms = {"a_sample_then_ids": form_a,
             "b_sample_wl": lambda: pop.sample_batch(idx, p, e, m, "sample", 42, device=DEV, wl=table),
             "c_sample_alone": lambda: pop.sample_batch(idx, p, e, m, "sample", 42, device=DEV)}
    ids_b = forms["b_sample_wl"]()[5]
    same = torch.equal(forms["a_sample_then_ids"](), ids_b) and bool((ids_b < len(table)).all())
    ts = {f: [] for f in forms}
    for r in range(warmup + iters):
        for f, fn in forms.items():                                 # interleaved: every round runs each form once
            t = timed(fn)
            if r >= warmup:
                ts[f].append(t)
    info, plain_info = pop.info(), plain.info()
    line = dict(shape=name, what=what, graphs=len(idx), m=m, k=k, iterations=ITERATIONS, labeled=xs is not None, sets=info["keys"],
                classes=info["wl_classes"], rows_hashed=info["wl_rows_hashed"], bytes_wl=info["bytes"], bytes_plain=plain_info["bytes"],
                add_many_wl_ms=round(add_ms, 3), add_many_plain_ms=round(plain_ms, 3), ids_equal=same, iters=iters, warmup=warmup,
                device=torch.cuda.get_device_name(0))
    for f in forms:
        line[f] = population_bench.stats(ts[f])
    line["b_minus_c_ms"] = round(line["b_sample_wl"]["median_ms"] - line["c_sample_alone"]["median_ms"], 4)
    line["a_minus_c_ms"] = round(line["a_sample_then_ids"]["median_ms"] - line["c_sample_alone"]["median_ms"], 4)
    line["c_spread_ms"] = round(line["c_sample_alone"]["max_ms"] - line["c_sample_alone"]["min_ms"], 4)
    pop.close()
    plain.close()
    return line


def calls_only(name, calls=47):
    ei, ptr, m, k, _, xs, _ = setup(name)
    e, p = torch.from_numpy(ei), torch.from_numpy(ptr)
    idx = list(range(len(ptr) - 1))
    pop = build(ei, ptr, k, ITERATIONS, xs)[0]
    table = wl.WLVocab(wl.extend_vocab({}, *pop.wl_digests()), DEV)
    for _ in range(calls):
        pop.sample_batch(idx, p, e, m, "sample", 42, device=DEV, wl=table)
    torch.cuda.synchronize()


def trace(name, out_dir, calls=47):
    """Kernel times of one add_many and `calls` calls of form b from a rocprofv3 run of its own: {kernel: [launches, total us]}.  The
    hash kernel's launches are the add's chunks; a step adds none."""
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
    return dict(shape=name, calls=calls, kernels=rows, wl_hash_kernel_launches=sum(v[0] for n, v in rows.items() if "wl_hash" in n),
                wl_ids_kernel_launches=sum(v[0] for n, v in rows.items() if "uni_pop_wl_ids" in n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pop_wl.json"))
    ap.add_argument("--trace", default="")
    ap.add_argument("--trace-dir", default="")
    ap.add_argument("--calls-only", default="")
    a = ap.parse_args()
    if a.calls_only:
        calls_only(a.calls_only)
        return
    lines = []
    if a.trace:
        lines.append(trace(a.trace, a.trace_dir or tempfile.mkdtemp(prefix="pop_wl_trace_")))
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
