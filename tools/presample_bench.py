#!/usr/bin/env python3
"""Presampling a whole dataset with ugs_sampler / uniform_sampler / rwr_sampler / epsilon_uniform_sampler: the reference trainer's loop of one-graph calls
(PresampleCache.add per graph, gps/experiment.py:379-440) against PresampleCache.add_many (a few sample_graphs calls).

Synthetic datasets (ugs_workloads.tu_graph, both edge directions stored):
  proteins  1113 graphs, PROTEINS-like sizes (mean 39 vertices, 1.86 undirected edges per vertex), clipped to 4..64 vertices so
            that every graph is within uniform_sampler's 64-vertex limit;
  qm9       20 000 graphs of 9..29 vertices, 1.04 undirected edges per vertex;
  cocosp    2 000 graphs of tu_graph(477, 1347), the COCO-SP shape (ugs only, at k = 8, m = 100: every graph is over the device
            batch pass's default 1000-column limit, so each is preprocessed on the host).  --large-pass times add_many a second
            time with the limit raised to 8192 (ugs_sampler.set_batch_pass_max_cols), the two settings' runs taking turns, checks
            the two caches equal and writes profiles/presample_bench_large_pass.json.
  subgnn    1 600 graphs of 10..200 vertices, 2 undirected edges per vertex: the size range of the reference's SubGNN configs
            (gin-ppi-bp, gin-hpo-metab, gin-hpo-neuro, gin-em-user: "sampler": "epsilon_uniform", k = 5, m = 100); epsilon_uniform only.
epsilon_uniform runs only when named (--sampler epsilon_uniform: proteins, qm9 and subgnn at the configs' k = 5, m = 100, epsilon 0.1,
written to profiles/eps_presample.json unless --out says otherwise).
ugs and uniform run at k = 6, m = 64 and rwr at k = 5, m = 50, seeds 42 + i; ugs starts every timed build from an empty
preprocessing LRU (clear_cache: what the trainer's start-up sees).  Timings are wall time to a synchronised device, after a
warm-up on the first 64 graphs: add_many the median of three runs, the loop one run (--loop-runs 3: the median of three); both caches are checked equal (load of every graph) before the numbers are written.

    python tools/presample_bench.py [--only qm9] [--sampler rwr] [--out profiles/presample_bench.json]
    python tools/presample_bench.py --sampler epsilon_uniform --loop-runs 3
    python tools/presample_bench.py --only qm9 --many-only        # add_many alone, e.g. under rocprofv3 --kernel-trace --stats
    python tools/presample_bench.py --large-pass                   # cocosp, add_many at limit 1000 and 8192
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
from ugs_sampler.presample import PresampleCache  # noqa: E402

CONFIGS = {"ugs": dict(k=6, m=64), "uniform": dict(k=6, m=64), "rwr": dict(k=5, m=50), "epsilon_uniform": dict(k=5, m=100)}
DATASETS = {"proteins": list(CONFIGS), "qm9": list(CONFIGS), "cocosp": ["ugs"], "subgnn": ["epsilon_uniform"]}
ON_REQUEST = ("epsilon_uniform",)      # samplers that run only when --sampler names them
COCOSP = dict(k=8, m=100)


def dataset(name):
    if name == "cocosp":
        return [(torch.from_numpy(wl.tu_graph(477, 1347, 7 * i + 1)), 477) for i in range(2000)]
    rng = np.random.default_rng({"proteins": 1113, "qm9": 20000, "subgnn": 1600}[name])
    if name == "subgnn":
        sizes = rng.integers(10, 201, 1600)
        und = 2 * sizes
    elif name == "proteins":
        sizes = np.clip(np.round(rng.gamma(2.2, 39.06 / 2.2, 1113)), 4, 64).astype(int)
        und = np.round(sizes * 1.86).astype(int)
    else:
        sizes = rng.integers(9, 30, 20000)
        und = np.round(sizes * 1.04).astype(int)
    return [(torch.from_numpy(wl.tu_graph(int(n), int(e), 7 * i + 1)), int(n)) for i, (n, e) in enumerate(zip(sizes, und))]


def sync():
    torch.cuda.synchronize()


def build_loop(cache, graphs, seeds):
    for i, ((ei, n), s) in enumerate(zip(graphs, seeds)):
        cache.add(i, ei, n, s)


def timed(fn, sampler=None):
    if sampler == "ugs":
        import ugs_sampler
        ugs_sampler.clear_cache()
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def same(a, b, G):
    assert a.failed == b.failed, "failed sets differ"
    order = list(range(G))
    ptr = torch.zeros(G + 1, dtype=torch.int64)                  # load's edge_src offsets need the batch: an empty one will do here
    for x, y in zip(a.load(order, ptr, torch.zeros((2, 0), dtype=torch.int64)), b.load(order, ptr, torch.zeros((2, 0), dtype=torch.int64))):
        assert torch.equal(x, y), "caches differ"


def large_pass(out):
    """cocosp / ugs: add_many with the batch pass's column limit at 1000 and at 8192, three fresh caches each, alternating"""
    import ugs_sampler
    dev = "cuda:0"
    graphs = dataset("cocosp")
    G = len(graphs)
    seeds = [42 + i for i in range(G)]
    ts, caches = {1000: [], 8192: []}, {}
    try:
        for lim in ts:
            ugs_sampler.set_batch_pass_max_cols(lim)
            PresampleCache(COCOSP["m"], COCOSP["k"], dev, sampler="ugs").add_many(range(64), graphs[:64], seeds[:64])      # warm-up
        for _ in range(3):
            for lim in ts:
                ugs_sampler.set_batch_pass_max_cols(lim)
                many = PresampleCache(COCOSP["m"], COCOSP["k"], dev, sampler="ugs")
                s0 = ugs_sampler.batch_pass_stats()
                ts[lim].append(timed(lambda: many.add_many(range(G), graphs, seeds), "ugs"))
                s1 = ugs_sampler.batch_pass_stats()
                caches[lim] = (many, {k: s1[k] - s0[k] for k in s1})
    finally:
        ugs_sampler.set_batch_pass_max_cols(1000)
    same(caches[1000][0], caches[8192][0], G)
    rec = dict(dataset="cocosp", sampler="ugs", graphs=G, k=COCOSP["k"], m=COCOSP["m"], caches_equal=True)
    for lim, v in ts.items():
        rec[f"limit_{lim}"] = dict(add_many_s=round(sorted(v)[1], 4), add_many_runs_s=[round(t, 4) for t in v],
                                   add_many_us_per_graph=round(1e6 * sorted(v)[1] / G, 2), batch_pass_stats_delta=caches[lim][1])
    rec["speedup_of_the_raised_limit"] = round(sorted(ts[1000])[1] / sorted(ts[8192])[1], 2)
    print(json.dumps(rec), flush=True)
    meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip,
                note="wall time to a synchronised device, empty preprocessing LRU before every run; medians of three runs per setting, alternated")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(meta=meta, results=[rec]), f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=list(DATASETS))
    ap.add_argument("--sampler", choices=list(CONFIGS))
    ap.add_argument("--many-only", action="store_true", help="time add_many alone (no loop, no check, no file)")
    ap.add_argument("--loop-runs", type=int, default=1, help="timed runs of the add loop (the median is reported)")
    ap.add_argument("--out", help="default: profiles/presample_bench.json (profiles/eps_presample.json with --sampler epsilon_uniform)")
    ap.add_argument("--large-pass", action="store_true", help="cocosp only: add_many at column limit 1000 and 8192 of the device batch pass")
    ap.add_argument("--large-pass-out", default=os.path.join(ROOT, "profiles", "presample_bench_large_pass.json"))
    a = ap.parse_args()
    if a.large_pass:
        return large_pass(a.large_pass_out)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "eps_presample.json" if a.sampler == "epsilon_uniform" else "presample_bench.json")
    dev = "cuda:0"
    results = []
    for dname in [a.only] if a.only else list(DATASETS):
        snames = [s for s in DATASETS[dname] if a.sampler == s or (a.sampler is None and s not in ON_REQUEST)]
        if not snames:
            continue
        graphs = dataset(dname)
        G = len(graphs)
        seeds = [42 + i for i in range(G)]
        nv = sum(n for _, n in graphs)
        for sname in snames:
            cfg = COCOSP if dname == "cocosp" else CONFIGS[sname]
            warm = PresampleCache(cfg["m"], cfg["k"], dev, sampler=sname)
            warm.add_many(range(64), graphs[:64], seeds[:64])
            if not a.many_only:
                build_loop(PresampleCache(cfg["m"], cfg["k"], dev, sampler=sname), graphs[:64], seeds[:64])
            ts = []
            for _ in range(3):                                  # median of three fresh caches
                many = PresampleCache(cfg["m"], cfg["k"], dev, sampler=sname)
                ts.append(timed(lambda: many.add_many(range(G), graphs, seeds), sname))
            t_many = sorted(ts)[1]
            rec = dict(dataset=dname, sampler=sname, graphs=G, vertices=nv, k=cfg["k"], m=cfg["m"], add_many_s=round(t_many, 4),
                       add_many_runs_s=[round(t, 4) for t in ts], add_many_us_per_graph=round(1e6 * t_many / G, 2), failed=len(many.failed))
            if not a.many_only:
                tl = []
                for _ in range(max(a.loop_runs, 1)):
                    loop = PresampleCache(cfg["m"], cfg["k"], dev, sampler=sname)
                    tl.append(timed(lambda: build_loop(loop, graphs, seeds), sname))
                t_loop = sorted(tl)[(len(tl) - 1) // 2]
                same(loop, many, G)
                assert t_loop - t_many > max(ts) - min(ts), "add_many is not faster than the loop by more than its own spread"
                rec.update(add_loop_s=round(t_loop, 4), add_loop_runs_s=[round(t, 4) for t in tl], add_loop_us_per_graph=round(1e6 * t_loop / G, 2),
                           speedup=round(t_loop / t_many, 2), caches_equal=True)
            print(json.dumps(rec), flush=True)
            results.append(rec)
    if not a.many_only:
        meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip,
                    note="wall time to a synchronised device; add_loop = PresampleCache.add per graph (the reference's loop), "
                         "add_many = batched sample_graphs calls")
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(meta=meta, results=results), f, indent=1)


if __name__ == "__main__":
    main()
