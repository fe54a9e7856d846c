#!/usr/bin/env python3
"""Timing of graphlets.vertex_census (HIP) against the recipe it replaces -- enumerate_graphs, orbit_ids, vertex_orbit_counts -- and,
as floors, against graphlets.census (the same search, one merged add a set instead of k) and count_graphs (the search alone).  Host
inputs, device outputs, every call timed from a drained device to a drained device.  After --warmup calls of every side the sides
alternate call by call, so that clock and cache drift fall on all alike; medians with the 10th and 90th percentiles over --iters
calls.  The recipe's result is checked against the new call once per shape.  A shape the recipe cannot hold (more than 2^25 rows in a
call) reports its reason in the recipe's place.  The build of the k = 7 code table, once per device, is timed on its own and
reported in a line of its own.  One JSON line per shape, also written to --out.

    python tools/graphlet_vertex_census_bench.py [--only csl150_k6,k44_k7] [--iters 9] [--warmup 2] [--out profiles/graphlet_vertex_census.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
import ugs_workloads as wl  # noqa: E402
import uniform_sampler  # noqa: E402
from ugs_sampler import graphlets  # noqa: E402

CSL_SKIPS = (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)
DEV = "cuda:0"


def batch(graphs):
    cols, ptr = [], [0]
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    return np.ascontiguousarray(np.concatenate(cols, axis=1)), np.array(ptr, np.int64)


def clique(n):
    return n, np.array([[u for v in range(n) for u in range(v)], [v for v in range(n) for u in range(v)]], np.int64)


def shapes():
    """name -> (batch, k, limit, what): the shapes of tools/graphlet_census_bench.py for k <= 7"""
    proteins = wl.tu_batch(39, 73, 128)
    return {
        "csl150_k6": (batch([(41, wl.csl_graph(41, CSL_SKIPS[i % len(CSL_SKIPS)])) for i in range(150)]), 6, 1 << 25, "150 x csl_graph(41, s), k = 6"),
        "dense64_k6": (batch([(64, wl.tu_graph(64, 300, 3))]), 6, 1 << 25, "tu_graph(64, 300, 3), k = 6"),
        "proteins_k6": (proteins, 6, 1 << 25, "tu_batch(39, 73, 128), k = 6"),
        "proteins_k7": (proteins, 7, 1 << 25, "tu_batch(39, 73, 128), k = 7"),
        "k44_k7": (batch([clique(44)]), 7, 1 << 27, "K44 alone, k = 7: 38 320 568 sets, past the enumeration's 2^25 rows"),
    }


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    q = np.percentile(np.array(ms), [50, 10, 90])
    return dict(median_ms=round(float(q[0]), 4), p10_ms=round(float(q[1]), 4), p90_ms=round(float(q[2]), 4), calls=len(ms))


def table_build(k, iters):
    """The code table of k, built `iters` times from nothing: what the first call on a device pays once."""
    none = torch.zeros((2, 0), dtype=torch.int64)
    graphlets.vertex_census(none, torch.tensor([0, k]), k, device=DEV)          # the host's tables, the library's context
    ms = []
    for _ in range(iters):
        graphlets._dev_vertex_census.clear()
        ms.append(timed(lambda: graphlets._vertex_census_tables(torch.device(DEV), k))[0])
    return dict(shape=f"table_k{k}", what=f"the code table of k = {k}: {1 << (k * (k - 1) // 2)} entries of 4 bytes, built and synchronised",
                device=torch.cuda.get_device_name(0), build=summary(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graphlet_vertex_census.json"))
    a = ap.parse_args()
    lines = []
    if not a.only or "table_k7" in a.only.split(","):
        lines.append(table_build(7, 5))
        print(json.dumps(lines[-1]), flush=True)
    for name, ((ei, ptr), k, limit, what) in shapes().items():
        if a.only and name not in a.only.split(","):
            continue
        e_h, p_h = torch.from_numpy(ei), torch.from_numpy(ptr)
        N = int(ptr[-1])
        cols = graphlets.connected_orbits(k).to(DEV)

        def vertex_census():
            return graphlets.vertex_census(e_h, p_h, k, limit=limit, device=DEV)[0]

        def recipe():
            nodes, e2, eptr, _, _, _ = uniform_sampler.enumerate_graphs(e_h, p_h, k, max_rows=1 << 25, device=DEV)
            return graphlets.vertex_orbit_counts(nodes, graphlets.orbit_ids(nodes, e2, eptr), N, cols)

        def census():
            return graphlets.census(e_h, p_h, k, limit=limit, device=DEV)[0]

        def count():
            return uniform_sampler.count_graphs(e_h, p_h, k, limit=limit)[0]

        sides = {"vertex_census": vertex_census, "recipe": recipe, "census": census, "count_graphs": count}
        skipped = {}
        sets = int(count().sum())
        if sets > 1 << 25:
            skipped["recipe"] = f"{sets} sets: more than the 2^25 rows one enumeration holds"
            del sides["recipe"]
        else:
            try:
                want = recipe()
                assert torch.equal(vertex_census(), want), "vertex_census != recipe"
                del want
            except RuntimeError as err:                                         # "split the call", or out of memory
                skipped["recipe"] = str(err).splitlines()[0][:200]
                del sides["recipe"]
                torch.cuda.empty_cache()
        assert int(vertex_census().sum()) == k * sets
        ms = {s: [] for s in sides}
        for it in range(a.warmup + a.iters):
            for s, fn in sides.items():                                         # the sides alternate call by call
                t, out = timed(fn)
                del out
                if it >= a.warmup:
                    ms[s].append(t)
        line = dict(shape=name, what=what, graphs=len(ptr) - 1, vertices=N, k=k, sets=sets, columns=int(cols.numel()), warmup=a.warmup,
                    device=torch.cuda.get_device_name(0), **{s: summary(v) for s, v in ms.items()}, skipped=skipped)
        v = line["vertex_census"]["median_ms"]
        line["vertex_census_over_census"] = round(v / line["census"]["median_ms"], 3)
        line["vertex_census_over_count"] = round(v / line["count_graphs"]["median_ms"], 3)
        if "recipe" in line:
            line["recipe_over_vertex_census"] = round(line["recipe"]["median_ms"] / v, 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
