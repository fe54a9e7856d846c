#!/usr/bin/env python3
"""Generates tests/golden/f16_ugs_presample_reference.npz (+ .json): what the reference `ugs_sampler` module returns for the
trainer's presample loop (gps/experiment.py:379-440) -- one-graph `sample_batch(edge_index, [0, n], m, k, "sample", seed)` calls
in sequence, in ONE fresh process, so that the module's process-global preprocessing LRU sees them in order.

Two passes over the same graphs: k = 4, then k = 5 (the second pass meets the first's cache entries through the key that ignores
k).  Seeds are 42 + i except for two graphs that take 0 and a negative seed.  The graphs include an empty graph, a graph with
n < k, two graphs with identical content (an LRU hit inside a pass) and a graph with out-of-range columns.

The fixture pins the right-hand side of the law of ugs_sampler.sample_graphs (include/ugs_mi355.h, ugs_sample_graphs_begin):
tests/test_ugs_presample_reference.py replays it on the CPU oracle, tests/test_gpu_ugs_graphs.py on the HIP product.

    python tools/make_golden_ugs_presample.py        # needs the reference module of oracle/build_ref.py (oracle/_ref)
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import build_ref  # noqa: E402
import ugs_workloads as wl  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "f16_ugs_presample_reference")
M = 8
KS = (4, 5)


def graphs():
    """[(n, edge_index [2, E] int64 local ids)]"""
    g = [(int(n), wl.tu_graph(int(n), int(e), 1600 + i)) for i, (n, e) in enumerate(
        [(9, 10), (12, 13), (17, 19), (23, 27), (30, 41), (14, 14), (20, 37), (26, 28), (11, 12), (39, 73), (8, 9), (16, 24),
         (21, 22), (33, 40), (18, 20), (28, 31), (13, 15), (45, 60)])]
    g.insert(2, (0, np.zeros((2, 0), np.int64)))                                        # an empty graph
    g.insert(5, (3, np.array([[0, 1, 1, 2], [1, 0, 2, 1]], np.int64)))                  # n < k for both passes
    g.insert(9, (4, np.array([[0, 1, 2, 3, 1, 0, 3, 2], [1, 2, 3, 0, 0, 3, 2, 1]], np.int64)))   # n = 4: degenerate in the k = 5 pass only
    g.insert(12, g[3])                                                                  # identical content: an LRU hit within a pass
    n, ei = g[7]
    stray = np.array([[0, n, -1, 2, n + 3], [n, 1, 0, -2, n + 4]], np.int64)           # columns with an endpoint outside [0, n)
    g.insert(15, (n, np.concatenate([ei[:, :5], stray[:, :3], ei[:, 5:], stray[:, 3:]], axis=1)))
    g.append((6, np.zeros((2, 0), np.int64)))                                           # vertices, no columns
    return g


def seeds(G):
    s = [42 + i for i in range(G)]
    s[4] = 0
    s[10] = -7
    s[G - 2] = -(2 ** 31)
    return s


def main():
    ref = build_ref.load()
    gs = graphs()
    sd = seeds(len(gs))
    arrays, meta = {}, []
    # stored concatenated over the graphs (a zip member per call would cost more than its data): graph i's columns are
    # in_edge_index[:, col_ptr[i]:col_ptr[i+1]], its rows of pass k are k{k}/nodes[i*M:(i+1)*M], its edge entries
    # k{k}/edge_index and k{k}/edge_src[e_ptr[i]:e_ptr[i+1]], its edge_ptr and sample_ptr rows i of [G, M+1] and [G, 2]
    arrays["in_edge_index"] = np.concatenate([ei for _, ei in gs], axis=1)
    arrays["col_ptr"] = np.cumsum([0] + [ei.shape[1] for _, ei in gs]).astype(np.int64)
    arrays["n"] = np.array([n for n, _ in gs], np.int64)
    arrays["seeds"] = np.array(sd, np.int64)
    for k in KS:                                            # one process, one LRU: pass k = 4, then pass k = 5
        outs = []
        for i, (n, ei) in enumerate(gs):
            out = ref.sample_batch(torch.from_numpy(np.ascontiguousarray(ei)), torch.tensor([0, n], dtype=torch.int64), M, k, "sample", sd[i])
            outs.append([t.numpy().copy() for t in out])
            meta.append(dict(k=k, graph=i, n=n, columns=int(ei.shape[1]), seed=sd[i], edges=int(out[1].shape[1])))
        arrays[f"k{k}/nodes"] = np.concatenate([o[0] for o in outs], axis=0)
        arrays[f"k{k}/edge_index"] = np.concatenate([o[1] for o in outs], axis=1)
        arrays[f"k{k}/edge_ptr"] = np.stack([o[2] for o in outs])
        arrays[f"k{k}/sample_ptr"] = np.stack([o[3] for o in outs])
        arrays[f"k{k}/edge_src"] = np.concatenate([o[4] for o in outs])
        arrays[f"k{k}/e_ptr"] = np.cumsum([0] + [o[1].shape[1] for o in outs]).astype(np.int64)
    srcs = [os.path.join(build_ref.HERE, "ref_unity.cpp")] + [os.path.join(build_ref.REF, "src", f) for f in (
        "preproc.cpp", "sampler.cpp", "ugs_sampler_batch_extension.cpp", "extension.cpp")] + [
        os.path.join(build_ref.REF, "include", f) for f in ("sampler.hpp", "cache.hpp")]
    sha = {("oracle/" if p.startswith(build_ref.HERE) else "src/samplers/ugs_sampler/") + os.path.relpath(
        p, build_ref.HERE if p.startswith(build_ref.HERE) else build_ref.REF): hashlib.sha256(open(p, "rb").read()).hexdigest() for p in srcs}
    np.savez_compressed(OUT + ".npz", **arrays)
    with open(OUT + ".json", "w") as f:
        json.dump(dict(source="reference ugs_sampler (src/samplers/ugs_sampler), one-graph sample_batch calls in one process",
                       build_command="python oracle/build_ref.py  (one g++ -O3 -std=c++17 -shared -fPIC invocation on oracle/ref_unity.cpp, "
                                     "torch / pybind11 include and library paths)",
                       source_sha256=sha, m=M, ks=list(KS), mode="sample", graphs=len(gs), calls=meta), f, indent=1)
        f.write("\n")
    print(len(gs), "graphs,", len(meta), "calls ->", OUT + ".npz", os.path.getsize(OUT + ".npz"), "bytes")


if __name__ == "__main__":
    main()
