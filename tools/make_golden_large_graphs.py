#!/usr/bin/env python3
"""Generates tests/golden/f17_large_graph_batches.npz: what the reference `ugs_sampler` module returns for a history of eight
sample_batch calls on graphs of 1100 - 2700 columns, in ONE fresh process, so that the module's process-global preprocessing LRU
sees them in order.  Above 1000 columns the reference's LRU key hashes every (columns / 500)-th column only
(include/cache.hpp:100-107): graph `b` of tests/large_graphs.py differs from graph `a` in a column the key skips, shares a's key,
and is sampled from a's cached preprocessing.  m = 4, k in {4, 6}, all three modes.

Stored: the seeds and shapes of the inputs (they are regenerated from ugs_workloads by tests/large_graphs.py) and the five
output tensors of every call.  tests/test_batch_pass_limit.py replays the history on the CPU oracle,
tests/test_gpu_batch_pass_large.py on the HIP product with the device batch pass's column limit raised.

    python tools/make_golden_large_graphs.py        # needs the reference module of oracle/build_ref.py (oracle/_ref)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("ss-gnn_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import build_ref  # noqa: E402
import large_graphs as lg  # noqa: E402


def main():
    ref = build_ref.load()
    arrays = {
        "graphs": np.array([lg.GRAPHS[g] for g in sorted(lg.GRAPHS)], np.int64),                       # (n, undirected edges, seed, variant)
        "calls": np.array([(k, ("sample", "graph", "global").index(mode), seed, len(names)) for names, k, mode, seed in lg.CALLS], np.int64),
        "call_graphs": np.frombuffer(" ".join("".join(names) for names, _, _, _ in lg.CALLS).encode(), np.uint8),
        "m": np.array(lg.M, np.int64),
    }
    for i, (ei, ptr, m, k, mode, seed) in enumerate(lg.calls()):
        out = ref.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode, seed)
        for nm, t in zip(lg.NAMES, out):
            arrays[f"c{i}/{nm}"] = t.numpy().copy()
    np.savez_compressed(lg.GOLDEN, **arrays)
    print(len(lg.CALLS), "calls ->", lg.GOLDEN, os.path.getsize(lg.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
