#!/usr/bin/env python3
"""Timing of uniform_sampler.sample_batch (HIP) on the reference configs' shapes: the drop-in call (CPU tensors in, pinned CPU
tensors out) and the device-resident call (cuda:0 in and out), median of --iters calls after --warmup, one JSON line per shape
(also written to --out).  The connected k-subset counts printed beside them come from the CPU restatement (tests/uniform_law.py).

    python tools/uniform_bench.py [--only csl_k6] [--iters 20] [--warmup 3] [--out profiles/uniform_bench.json]

The rows after dense64_k5 are about the wide form (graphs of more than 64 vertices): they set the vertex limit
or the mask threshold for their own calls and put both back.  `--only` with one of them is what a kernel trace runs.
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


def proteins_like(wide):
    """32 graphs shaped like a PROTEINS batch: sizes 8 ... 60, and (wide) five above 64, one of them the 620-vertex graph of the
    tests (2300 columns, 891 625 connected 6-subsets); without `wide` the same batch with those five left out."""
    small = [(n, wl.tu_graph(n, n + n // 8, 500 + i)) for i, n in enumerate([8 + (37 * i) % 53 for i in range(27)])]
    big = [(n, wl.tu_graph(n, n + n // 8, 600 + i)) for i, n in enumerate([70, 96, 130, 210])] + [(620, wl.tu_graph(620, 1150, 6))]
    graphs = small[:5] + big[:1] + small[5:12] + big[1:3] + small[12:20] + big[3:] + small[20:] if wide else small
    return batch(graphs)


def shapes():
    csl = batch([(41, wl.csl_graph(41, s)) for s in CSL_SKIPS])
    mutag_max = batch([(28, wl.tu_graph(28, 31, g)) for g in range(64)])
    return {
        "csl_k6": (csl, 100, 6, "CSL 10 x 41, k = 6, m = 100 (gin-k6.json, batch 10)"),
        "csl_k7": (csl, 100, 7, "CSL 10 x 41, k = 7, m = 100 (gin-k7-wl.json)"),
        "mutag_k6": (batch([(18, wl.tu_graph(18, 20, g)) for g in range(64)]), 64, 6, "64 x tu_graph(18, 20), k = 6, m = 64 (gcn-mutag.json)"),
        "mutag_max_k6": (mutag_max, 64, 6, "64 x tu_graph(28, 31), k = 6, m = 64"),
        "dense64_k5": (batch([(64, wl.tu_graph(64, 300, g)) for g in range(32)]), 200, 5, "32 x tu_graph(64, 300), k = 5, m = 200"),
        "mutag_max_k6_wide": (mutag_max, 64, 6, "64 x tu_graph(28, 31), k = 6, m = 64, through the wide kernels (mask threshold 0)", dict(mask=0)),
        "proteins_k6": (proteins_like(True), 64, 6, "PROTEINS-shaped, 32 graphs, 5 above 64 vertices (one of 620), k = 6, m = 64, limit 1024",
                        dict(limit=1024)),
        "proteins_k6_narrow": (proteins_like(False), 64, 6, "the same batch without its 5 wide graphs (27 graphs)", dict(limit=1024)),
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
    for name, ((ei, ptr), m, k, what, *opts) in shapes().items():
        if a.only and name not in a.only.split(","):
            continue
        opts = opts[0] if opts else {}
        # the limit and the threshold are process-wide: put back whatever happens to the row, so that no later row runs in the wrong form
        prev_limit = uniform_sampler.set_max_vertices(opts["limit"]) if "limit" in opts else None
        try:
            prev_mask = uniform_sampler._set_mask_vertices(opts["mask"]) if "mask" in opts else None
            try:
                e_h, p_h = torch.from_numpy(ei), torch.from_numpy(ptr)
                e_d, p_d = e_h.cuda(), p_h.cuda()
                host = median_ms(lambda: uniform_sampler.sample_batch(e_h, p_h, m, k), a.iters, a.warmup, sync)
                dev = median_ms(lambda: uniform_sampler.sample_batch(e_d, p_d, m, k), a.iters, a.warmup, sync)
                out = uniform_sampler.sample_batch(e_h, p_h, m, k)
            finally:
                if prev_mask is not None:
                    uniform_sampler._set_mask_vertices(prev_mask)
        finally:
            if prev_limit is not None:
                uniform_sampler.set_max_vertices(prev_limit)
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
