#!/usr/bin/env python3
"""Times ugs_sampler.graphlets.orbit_ids beside class_ids, whose rows it reads and whose search it runs once per vertex instead of
once per tied first pick, on the shapes and by the method of tools/graphlet_bench.py: device-resident rows of
ugs_sampler.sample_batch (mode "sample", seed 42) for the three TU shapes and ER k = 8, and 12 800 rows that are all K8, all C8 and
all cubes.  Per shape: warm calls of class_ids and orbit_ids alternating call by call inside one process; device events around the
whole call; medians with the 10th and 90th percentiles.

class_ids' kernel is the one profiles/graphlet_ids.json measured: its medians here are put beside that file's (--baseline), which is
this run's check that the two runs measure the same thing.

End to end, the exact 6-GDV of the CSL batch (10 x csl_graph(41, skip), the batch of tools/uniform_bench.py): enumerate_graphs +
orbit_ids + vertex_orbit_counts with columns = connected_orbits(6), as one timed unit and stage by stage.

The whole-call times of the small shapes are mostly the host's way to the launch, which differs between the two calls (class_ids
allocates three outputs, orbit_ids one).  --trace adds the kernels' own times: a rocprofv3 --kernel-trace --stats run over a child
of its own per shape (--calls-only: 200 calls of each side, nothing else).

    python tools/graphlet_orbit_bench.py --trace --out profiles/graphlet_orbits.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ss-gnn_amd", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

CSL_SKIPS = (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)
WORST = {"all_K8": [(i, j) for i in range(8) for j in range(i + 1, 8)], "all_C8": [(i, (i + 1) % 8) for i in range(8)],
         "all_cubes": [(a, a ^ d) for a in range(8) for d in (1, 2, 4) if a < a ^ d]}
TRACED = ("mutag_like", "er_k8", "all_cubes", "csl_k6_population")
TRACE_CALLS = 200


def csl_batch():
    import numpy as np
    import ugs_workloads as wl_shapes
    cols, ptr = [], [0]
    for s in CSL_SKIPS:
        cols.append(wl_shapes.csl_graph(41, s) + ptr[-1])
        ptr.append(ptr[-1] + 41)
    return np.concatenate(cols, axis=1), ptr


def rows_of(name, dev):
    """(the three device tensors, a description) of one shape."""
    import numpy as np
    import torch

    import ugs_sampler
    import ugs_workloads as wl_shapes
    import uniform_sampler
    from graphlet_bench import ER, GRAPHS, SEED, SHAPES, relabelled_rows
    for shape, n, e, k, m in SHAPES:
        if shape == name:
            ei, ptr = wl_shapes.tu_batch(n, e, GRAPHS)
            out = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode="sample", seed=SEED, device=dev)
            return out[:3], {"n": n, "undirected_edges": e, "graphs": GRAPHS, "m": m}
    if name == "er_k8":
        n, cols, k, m = ER
        ei, ptr = wl_shapes.er_graph(n, cols, 0)
        out = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode="sample", seed=SEED, device=dev)
        return out[:3], {"n": n, "columns": cols, "graphs": 1, "m": m}
    if name == "csl_k6_population":
        ei, ptr = csl_batch()
        en = uniform_sampler.enumerate_graphs(torch.from_numpy(ei).to(dev), torch.tensor(ptr, dtype=torch.int64, device=dev), 6, device=dev)
        return en[:3], {"graphs": len(CSL_SKIPS), "vertices": ptr[-1]}
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in relabelled_rows(WORST[name], ER[3], 7)), {}


def calls_only(name):
    """The child of --trace: TRACE_CALLS calls of each side on one shape."""
    import torch
    from ugs_sampler import graphlets
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    three, _ = rows_of(name, dev)
    for _ in range(TRACE_CALLS):
        graphlets.class_ids(*three)
        graphlets.orbit_ids(*three)
    torch.cuda.synchronize()


def trace(name):
    """Mean kernel times in microseconds of the two graphlet kernels over the child's calls, from a rocprofv3 run of its own."""
    with tempfile.TemporaryDirectory() as out_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
               "--calls-only", name]
        subprocess.run(cmd, check=True, timeout=280, stdout=subprocess.DEVNULL)
        rows = {}
        for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    for kernel in ("ugs_graphlet_canon_kernel", "ugs_graphlet_orbits_kernel"):
                        if kernel in r["Name"]:
                            assert int(r["Calls"]) == TRACE_CALLS, (name, r["Name"], r["Calls"])
                            rows[kernel] = {"calls": int(r["Calls"]), "mean_us": round(float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3, 2)}
    assert len(rows) == 2, (name, rows)
    rows["orbits_over_canon"] = round(rows["ugs_graphlet_orbits_kernel"]["mean_us"] / rows["ugs_graphlet_canon_kernel"]["mean_us"], 2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--gdv-calls", type=int, default=30)
    ap.add_argument("--baseline", default=os.path.join(ROOT, "profiles", "graphlet_ids.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--calls-only", default=None)
    args = ap.parse_args()
    import torch

    import uniform_sampler
    from graphlet_bench import SEED, SHAPES
    from ugs_sampler import graphlets
    assert torch.cuda.is_available(), "graphlet_orbit_bench needs a GPU: nothing here is measured without one"
    if args.calls_only:
        return calls_only(args.calls_only)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with open(args.baseline) as f:
        doc = json.load(f)
    baseline = {r["shape"]: r["class_ids"] for r in doc["shapes"] + doc["worst_cases"]}

    def timed(sides, calls, warmup):
        """Medians and percentiles of device events around every side's call, the sides alternating call by call."""
        ev = {s: [] for s in sides}
        for it in range(warmup + calls):
            for s, fn in sides.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if it >= warmup:
                    ev[s].append(a.elapsed_time(b))
        out = {}
        for s in sides:
            q = statistics.quantiles(ev[s], n=10)
            out[s] = {"median_ms_events": round(statistics.median(ev[s]), 4), "p10_ms_events": round(q[0], 4), "p90_ms_events": round(q[-1], 4),
                      "min_ms_events": round(min(ev[s]), 4), "max_ms_events": round(max(ev[s]), 4)}
        return out

    def measure(name):
        three, extra = rows_of(name, dev)
        sides = {"class_ids": lambda: graphlets.class_ids(*three), "orbit_ids": lambda: graphlets.orbit_ids(*three)}
        orbit, cls = graphlets.orbit_ids(*three, return_class=True)
        k = three[0].size(1)
        assert torch.equal(orbit, sides["orbit_ids"]()) and torch.equal(cls, sides["class_ids"]()) and int(orbit.max()) <= graphlets.num_orbits(k)
        res = dict({"shape": name, "k": k, "rows": three[0].size(0), "edge_entries": three[1].size(1),
                    "orbits_seen": int(torch.unique(orbit[orbit < graphlets.num_orbits(k)]).numel()),
                    "classes_seen": int(torch.unique(cls).numel()), "calls": args.calls}, **extra)
        res.update(timed(sides, args.calls, args.warmup))
        base = baseline[name]
        res["class_ids_in_profiles_graphlet_ids"] = {x: base[x] for x in ("median_ms_events", "p10_ms_events", "p90_ms_events")}
        res["class_ids_median_over_that_file"] = round(res["class_ids"]["median_ms_events"] / base["median_ms_events"], 3)
        res["orbit_ids_over_class_ids"] = round(res["orbit_ids"]["median_ms_events"] / res["class_ids"]["median_ms_events"], 2)
        print(json.dumps(res), flush=True)
        return res

    results = [measure(name) for name in [s[0] for s in SHAPES] + ["er_k8"]]
    worst = [measure(name) for name in WORST]
    assert all(r["orbits_seen"] == 1 for r in worst)

    # the exact 6-GDV of the CSL batch, end to end and by stage
    ei, ptr = csl_batch()
    ei, ptr_t = torch.from_numpy(ei).to(dev), torch.tensor(ptr, dtype=torch.int64, device=dev)
    columns = graphlets.connected_orbits(6).to(dev)

    def gdv():
        en = uniform_sampler.enumerate_graphs(ei, ptr_t, 6, device=dev)
        return graphlets.vertex_orbit_counts(en[0], graphlets.orbit_ids(*en[:3]), ptr[-1], columns)

    en = uniform_sampler.enumerate_graphs(ei, ptr_t, 6, device=dev)
    orbit = graphlets.orbit_ids(*en[:3])
    first = gdv()
    assert int(first.sum()) == en[0].numel() and not en[5].any()
    stages = {"gdv_end_to_end": gdv, "enumerate_graphs": lambda: uniform_sampler.enumerate_graphs(ei, ptr_t, 6, device=dev),
              "class_ids": lambda: graphlets.class_ids(*en[:3]), "orbit_ids": lambda: graphlets.orbit_ids(*en[:3]),
              "vertex_orbit_counts": lambda: graphlets.vertex_orbit_counts(en[0], orbit, ptr[-1], columns)}
    gdv_res = dict({"shape": "csl_k6", "graphs": len(CSL_SKIPS), "vertices": ptr[-1], "k": 6, "rows": en[0].size(0), "edge_entries": en[1].size(1),
                    "columns": int(columns.numel()), "columns_occupied": int((first.sum(dim=0) > 0).sum()),
                    "distinct_vectors": int(torch.unique(first, dim=0).size(0)), "calls": args.gdv_calls},
                   **timed(stages, args.gdv_calls, max(3, args.gdv_calls // 10)))
    print(json.dumps(gdv_res), flush=True)

    kernels = {}
    if args.trace:
        for name in TRACED:
            kernels[name] = trace(name)
            print(json.dumps({"shape": name, "kernels": kernels[name]}), flush=True)

    doc = {"tool": "tools/graphlet_orbit_bench.py", "device": torch.cuda.get_device_name(0), "sampler": "ugs_sampler.sample_batch", "seed": SEED,
           "note": "times cover the whole call on device-resident rows, one launch for class_ids and for orbit_ids; kernel_times are the "
           "kernels alone (rocprofv3, a run of its own per shape); the effect on a training step's time is not measured here",
           "shapes": results, "worst_cases": worst, "gdv": gdv_res, "kernel_times": kernels}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
