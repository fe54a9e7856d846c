#!/usr/bin/env python3
"""Timing of the CSR form of graphlets.census and graphlets.vertex_census (form="csr": ugs_census_csr.hip) -- against the bitmap form on
shapes both can run, and alone, checked against facts that need no second enumeration, on shapes only it can run.  Device tensors in,
device results out, whole synchronous calls (the csr form's include the build of the simple CSR with torch), every call timed from a
drained device to a drained device.  After --warmup calls of every side the sides alternate call by call; medians with the 10th and
90th percentiles over --iters calls.  A shape whose first call takes more than --slow seconds is timed over that one call and one
more, and says so.  One JSON line per shape, also written to --out.

    python tools/graphlet_census_csr_bench.py [--only csl150_k6,er] [--er-ks 2,3 --er-vks 2,3] [--iters 9] [--warmup 2] [--out profiles/graphlet_census_csr.json]

The checks of the large shapes: at k = 3, paths + 3 * triangles = sum over v of C(deg v, 2), the degrees from the CSR; at k = 2,
gdv[:, 0] is the degree; and at every k the column sums of gdv against the census (item 5 of the vertex census law).
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


def shared_shapes():
    """name -> (batch, k, limit, what): shapes both forms run (those of tools/graphlet_census_bench.py)"""
    proteins = wl.tu_batch(39, 73, 128)
    return {
        "csl150_k6": (batch([(41, wl.csl_graph(41, CSL_SKIPS[i % len(CSL_SKIPS)])) for i in range(150)]), 6, 1 << 25, "150 x csl_graph(41, s), k = 6"),
        "proteins_k6": (proteins, 6, 1 << 25, "tu_batch(39, 73, 128), k = 6"),
        "proteins_k7": (proteins, 7, 1 << 25, "tu_batch(39, 73, 128), k = 7"),
        "k44_k7": (batch([clique(44)]), 7, 1 << 27, "K44 alone, k = 7: 38 320 568 sets"),
    }


def csr_shapes(args):
    """name -> (make batch, ks of census, ks of vertex_census, limit, what): shapes only the csr form runs"""
    ks = lambda text: tuple(int(x) for x in text.split(",") if x)
    n, cols = args.er_vertices, args.er_columns
    return {
        "tu600_k7": (lambda: (wl.tu_graph(600, 1123, 7), np.array([0, 600], np.int64)), (7,), (7,), 1 << 40,
                     "tu_graph(600, 1123, 7): one PROTEINS-shaped graph of 600 vertices, k = 7"),
        "er": (lambda: wl.er_graph(n, cols), ks(args.er_ks), ks(args.er_vks), 1 << 40,
               f"er_graph({n}, {cols}): the ER workload of bench.py (1 000 000 vertices, 20 000 000 columns) or a smaller one, device tensors in"),
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


def alternate(sides, iters, warmup, slow):
    """sides: name -> callable.  {name: summary}, the results of the last calls.  A first call above `slow` seconds: two calls in all."""
    ms, last = {n: [] for n in sides}, {}
    first = {n: timed(fn) for n, fn in sides.items()}
    if max(t for t, _ in first.values()) > slow * 1e3:
        for n, fn in sides.items():
            ms[n] = [first[n][0], timed(fn)[0]]
            last[n] = first[n][1]
        return {n: dict(summary(v), note="a slow shape: the first call and one more") for n, v in ms.items()}, last
    for _ in range(max(warmup - 1, 0)):
        for fn in sides.values():
            fn()
    for _ in range(iters):
        for n, fn in sides.items():
            t, last[n] = timed(fn)
            ms[n].append(t)
    return {n: summary(v) for n, v in ms.items()}, last


def item_five(k, counts, gdv, ptr):
    """Item 5: gdv summed over each graph's vertices = orbit size * the census count of the orbit's class."""
    classes = graphlets.connected_classes(k)
    base = graphlets.orbit_base(k)
    keys = graphlets.table(k)[classes].tolist()
    size, cls = [], []
    for c, key in enumerate(keys):
        rooted = graphlets._rooted_codes(key & ((1 << 28) - 1), k)
        size += [rooted.count(code) for code in sorted(set(rooted))]
        cls += [c] * int(base[classes[c] + 1] - base[classes[c]])
    size, cls = torch.tensor(size, device=gdv.device), torch.tensor(cls, device=gdv.device)
    G = ptr.numel() - 1
    graph = torch.bucketize(torch.arange(gdv.shape[0], device=gdv.device), ptr.to(gdv.device)[1:], right=True).clamp_(max=max(G - 1, 0))
    sums = torch.zeros((G, gdv.shape[1]), dtype=torch.int64, device=gdv.device).index_add_(0, graph, gdv)
    return bool(torch.equal(sums, counts[:, cls] * size))


def run_shared(name, shape, args):
    (ei, ptr), k, limit, what = shape
    e_d, p_d = torch.from_numpy(ei).to(DEV), torch.from_numpy(ptr).to(DEV)
    out = dict(shape=name, what=what, k=k, graphs=int(ptr.shape[0] - 1), vertices=int(ptr[-1]), columns=int(ei.shape[1]),
               device=torch.cuda.get_device_name(0))
    for call in ("census", "vertex_census"):
        fn = getattr(graphlets, call)
        sides = {"bitmap": lambda: fn(e_d, p_d, k, limit=limit), "csr": lambda: fn(e_d, p_d, k, limit=limit, form="csr")}
        stats, last = alternate(sides, args.iters, args.warmup, args.slow)
        same = bool(torch.equal(last["bitmap"][0], last["csr"][0])) and not last["bitmap"][1].any() and not last["csr"][1].any()
        sets = int(last["csr"][0].sum()) // (k if call == "vertex_census" else 1)
        out[call] = dict(stats, sets=sets, equal=same, csr_over_bitmap=round(stats["csr"]["median_ms"] / stats["bitmap"]["median_ms"], 3),
                         csr_sets_per_s=round(sets / stats["csr"]["median_ms"] * 1e3))
    return out


def run_csr(name, shape, args):
    make, ks, vks, limit, what = shape
    ei, ptr = make()
    e_d, p_d = torch.from_numpy(np.ascontiguousarray(ei)).to(DEV), torch.from_numpy(ptr).to(DEV)
    build, (rowptr, col) = timed(lambda: graphlets._simple_csr(e_d, p_d))
    build = [build] + [timed(lambda: graphlets._simple_csr(e_d, p_d))[0] for _ in range(2)]
    deg = rowptr[1:] - rowptr[:-1]
    wedges = int((deg * (deg - 1) // 2).sum())
    out = dict(shape=name, what=what, graphs=int(ptr.shape[0] - 1), vertices=int(ptr[-1]), columns=int(ei.shape[1]), csr_entries=int(col.numel()),
               max_degree=int(deg.max()), device=torch.cuda.get_device_name(0), simple_csr=summary(build), runs={})
    del rowptr, col
    counts_of = {}
    for k in ks:
        stats, last = alternate({"csr": lambda: graphlets.census(e_d, p_d, k, limit=limit, form="csr")}, args.iters, args.warmup, args.slow)
        counts, failed = last["csr"]
        counts_of[k] = counts
        sets = int(counts.sum())
        run = dict(stats["csr"], sets=sets, failed=bool(failed.any()), sets_per_s=round(sets / stats["csr"]["median_ms"] * 1e3))
        if k == 3:                                      # columns of k = 3: the path, then the triangle
            paths, triangles = int(counts[:, 0].sum()), int(counts[:, 1].sum())
            run.update(paths=paths, triangles=triangles, wedges_from_degrees=wedges, wedge_identity=paths + 3 * triangles == wedges)
        out["runs"][f"census_k{k}"] = run
        print(json.dumps({name: {f"census_k{k}": run}}), flush=True)
    for k in vks:
        stats, last = alternate({"csr": lambda: graphlets.vertex_census(e_d, p_d, k, limit=limit, form="csr")}, args.iters, args.warmup, args.slow)
        gdv, failed = last["csr"]
        sets = int(gdv.sum()) // k
        run = dict(stats["csr"], sets=sets, failed=bool(failed.any()), sets_per_s=round(sets / stats["csr"]["median_ms"] * 1e3),
                   gdv_bytes=int(gdv.numel()) * 8)
        if k in counts_of:
            run["item_five"] = item_five(k, counts_of[k], gdv, p_d)
        if k == 2:
            run["degree_identity"] = bool(torch.equal(gdv[:, 0], deg))
        out["runs"][f"vertex_census_k{k}"] = run
        print(json.dumps({name: {f"vertex_census_k{k}": run}}), flush=True)
        del gdv
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow", type=float, default=5.0, help="seconds: a shape whose first call takes longer is timed over two calls")
    ap.add_argument("--er-vertices", type=int, default=1_000_000)
    ap.add_argument("--er-columns", type=int, default=20_000_000)
    ap.add_argument("--er-ks", default="2,3,4", help="the k of the ER shape's census calls")
    ap.add_argument("--er-vks", default="2,3,4", help="the k of the ER shape's vertex_census calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graphlet_census_csr.json"))
    args = ap.parse_args()
    only = [s for s in args.only.split(",") if s]
    lines = []
    for name, shape in shared_shapes().items():
        if not only or name in only:
            lines.append(run_shared(name, shape, args))
            print(json.dumps(lines[-1]), flush=True)
    for name, shape in csr_shapes(args).items():
        if not only or name in only:
            lines.append(run_csr(name, shape, args))
            print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
