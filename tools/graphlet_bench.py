#!/usr/bin/env python3
"""Times ugs_sampler.graphlets.class_ids against wl.WLVocab.ids(iterations=3), the call it replaces, on the same device-resident rows.

Sampler shapes (ugs_sampler.sample_batch, mode "sample", seed 42, device outputs):
  MUTAG-like     tu_batch(18, 20, 128), k = 6, m = 100
  QM9-like       tu_batch(18, 19, 128), k = 5, m = 100
  PROTEINS-like  tu_batch(39, 73, 128), k = 6, m = 64
  ER k = 8       er_graph(100 000, 2 000 000), k = 8, m = 12 800
The WL side looks its digests up in the vocabulary of the same rows (every row known).  Per shape: the median, 10th and 90th
percentile of a warm call of each side from device events recorded on torch's current stream around the whole call, and beside
it a host clock around the call ended by a device synchronise.  The two sides alternate call by call inside one process.

Worst cases: 12 800 rows that are all K8, all C8 and all cubes (every row relabelled at random), the launches in which every lane
of every wave runs the longest searches, each as a ratio to the ER k = 8 time, with the WL call on the same rows beside it.

Host side: the time of the first ugs_graphlet_table(8) of the process (it builds n = 1 .. 8), and how many complete codes the
sequential search compares, and how many nodes it evaluates, over the 12 346 classes of n = 8 (ugs_graphlet_search_stats).

    python tools/graphlet_bench.py --out profiles/graphlet_ids.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ss-gnn_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

SHAPES = (("mutag_like", 18, 20, 6, 100), ("qm9_like", 18, 19, 5, 100), ("proteins_like", 39, 73, 6, 64))
GRAPHS, SEED, ER = 128, 42, (100_000, 2_000_000, 8, 12_800)


def relabelled_rows(edges, rows, seed):
    """`rows` copies of the 8-vertex graph `edges`, each under a random permutation, both directions of every edge, as numpy arrays."""
    import numpy as np
    rng = np.random.default_rng(seed)
    e = np.array(edges, np.int64).reshape(-1, 2)
    perm = np.argsort(rng.random((rows, 8)), axis=1)
    u, v = perm[:, e[:, 0]], perm[:, e[:, 1]]
    ei = np.stack([np.concatenate([u, v], axis=1).reshape(-1), np.concatenate([v, u], axis=1).reshape(-1)])
    nodes = np.broadcast_to(np.arange(8, dtype=np.int64), (rows, 8)).copy()
    return nodes, ei, np.arange(rows + 1, dtype=np.int64) * (2 * len(e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    import numpy as np
    import torch

    import ugs_sampler
    import ugs_workloads as wl_shapes
    from ugs_sampler import graphlets, wl
    assert torch.cuda.is_available(), "graphlet_bench needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    t0 = time.perf_counter()
    table8 = graphlets.table(8)
    table_s = time.perf_counter() - t0
    stats = [graphlets.search_stats(int(key)) for key in table8[-12346:].tolist()]
    leaves, nodes = [a for a, _ in stats], [b for _, b in stats]
    host = {"table_build_n1_to_8_seconds": round(table_s, 3), "classes": int(table8.numel()),
            "sequential_search_over_the_classes_of_n8": {
                "leaves": {"mean": round(statistics.mean(leaves), 3), "median": statistics.median(leaves), "max": max(leaves),
                           "classes_above_8": sum(x > 8 for x in leaves), "classes_with_1": sum(x == 1 for x in leaves)},
                "nodes": {"mean": round(statistics.mean(nodes), 3), "median": statistics.median(nodes), "max": max(nodes)}}}
    print(json.dumps(host), flush=True)

    def measure(name, three, extra):
        digest, status = wl.wl_hash(*three, 3)
        vocab = wl.WLVocab(wl.extend_vocab({}, digest, status), dev)
        sides = {"class_ids": lambda: graphlets.class_ids(*three), "wl_vocab_ids": lambda: vocab.ids(*three, 3)}
        ids, wl_ids = sides["class_ids"](), sides["wl_vocab_ids"]()
        k = three[0].size(1)
        assert int(ids.max()) < graphlets.num_classes(k) and int(wl_ids.max()) < len(vocab)
        # WL never splits an isomorphism class: the exact ids refine the WL ids
        pairs = torch.unique(torch.stack([ids, wl_ids]), dim=1)
        assert pairs.size(1) == torch.unique(ids).numel(), "an exact class with two WL digests"
        ev = {s: [] for s in sides}
        clock = {s: [] for s in sides}
        for it in range(args.warmup + args.calls):
            for s, fn in sides.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                h1 = time.perf_counter()
                if it >= args.warmup:
                    ev[s].append(a.elapsed_time(b))
                    clock[s].append((h1 - h0) * 1e3)
        res = dict({"shape": name, "k": k, "rows": three[0].size(0), "edge_entries": three[1].size(1),
                    "exact_classes_seen": int(torch.unique(ids).numel()), "wl_digests_seen": len(vocab), "calls": args.calls}, **extra)
        for s in sides:
            q = statistics.quantiles(ev[s], n=10)
            res[s] = {"median_ms_events": round(statistics.median(ev[s]), 4), "p10_ms_events": round(q[0], 4), "p90_ms_events": round(q[-1], 4),
                      "min_ms_events": round(min(ev[s]), 4), "max_ms_events": round(max(ev[s]), 4),
                      "median_ms_host_clock": round(statistics.median(clock[s]), 4)}
        res["wl_over_class_ids"] = round(res["wl_vocab_ids"]["median_ms_events"] / res["class_ids"]["median_ms_events"], 2)
        print(json.dumps(res), flush=True)
        return res

    results = []
    for name, n, e, k, m in SHAPES:
        ei, ptr = wl_shapes.tu_batch(n, e, GRAPHS)
        out = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode="sample", seed=SEED, device=dev)
        results.append(measure(name, out[:3], {"n": n, "undirected_edges": e, "graphs": GRAPHS, "m": m}))
    n, cols, k, m = ER
    ei, ptr = wl_shapes.er_graph(n, cols, 0)
    out = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode="sample", seed=SEED, device=dev)
    er = measure("er_k8", out[:3], {"n": n, "columns": cols, "graphs": 1, "m": m})
    results.append(er)

    allp = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    worst = []
    for name, edges in (("all_K8", allp), ("all_C8", [(i, (i + 1) % 8) for i in range(8)]),
                        ("all_cubes", [(a, a ^ d) for a in range(8) for d in (1, 2, 4) if a < a ^ d])):
        three = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in relabelled_rows(edges, m, 7))
        res = measure(name, three, {})
        assert res["exact_classes_seen"] == 1
        res["class_ids_over_er_k8"] = round(res["class_ids"]["median_ms_events"] / er["class_ids"]["median_ms_events"], 2)
        worst.append(res)
    doc = {"tool": "tools/graphlet_bench.py", "device": torch.cuda.get_device_name(0), "sampler": "ugs_sampler.sample_batch", "seed": SEED,
           "note": "times cover the whole call on device-resident rows: one launch for class_ids, two for WLVocab.ids; the effect on a "
           "training step's time is not measured here", "host": host, "shapes": results, "worst_cases": worst}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
