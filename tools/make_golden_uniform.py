#!/usr/bin/env python3
"""Generates tests/golden/f14_uniform_reference.npz (+ .json): outputs of the reference `uniform_sampler` module
(AniruddhaMandal/SS-GNN src/samplers/uniform_sampler) on fixed batches, for the bit-exact parity tests
(tests/test_uniform_law.py against the CPU restatement, tests/test_gpu_uniform.py against the HIP product).

The reference module is not built by this repository: compile it by hand, outside the tree, from the reference's
uniform_sampler.cpp (one g++ line with torch / pybind11 includes, -fopenmp, and `pinned_memory(x)` re-spelled
`pinned_memory(false)` by a macro so that a machine without a GPU can allocate its outputs), then

    python tools/make_golden_uniform.py /path/to/uniform_sampler.<ext-suffix>.so --cmd "<the g++ line>" --sha256 <of uniform_sampler.cpp>

The command and the source hash are recorded in the json next to the scenarios.
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
import ugs_workloads as wl  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "f14_uniform_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def batch(graphs, first=0):
    """Concatenates local edge_index arrays [(n, ei)] into a PyG batch starting at vertex `first`."""
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(np.asarray(ei, np.int64) + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


def edge_case_batch():
    """ptr[0] = 5; a 7-vertex graph with an isolated vertex (6), a loop (2, 2) and a duplicate column (0, 1); a 3-vertex graph
    (n < k for k >= 4); a 6-vertex graph; one column across graphs 0 and 2."""
    g0 = np.array([[0, 1, 1, 2, 3, 2, 0, 4], [1, 2, 3, 2, 4, 4, 1, 5]], np.int64)
    g1 = np.array([[0, 1], [1, 2]], np.int64)
    g2 = np.array([[0, 1, 2, 3, 4, 0, 1, 2], [1, 2, 3, 4, 5, 2, 0, 0]], np.int64)
    ei, ptr = batch([(7, g0), (3, g1), (6, g2)], first=5)
    ei = np.concatenate([ei[:, :5], np.array([[6], [ptr[2] + 1]], np.int64), ei[:, 5:]], axis=1)   # cross-graph column
    return ei, ptr


def scenarios():
    csl = batch([(41, wl.csl_graph(41, s)) for s in (2, 3, 5)])
    mutag = batch([(18, wl.tu_graph(18, 20, s)) for s in range(6)] + [(28, wl.tu_graph(28, 31, 100))])
    ptc = batch([(14, wl.tu_graph(14, 14, 200 + s)) for s in range(6)] + [(26, wl.tu_graph(26, 28, 210))])
    ptc64 = batch([(14, wl.tu_graph(14, 14, 300 + s)) for s in range(3)] + [(64, wl.tu_graph(64, 71, 310))])
    edge = edge_case_batch()
    U64 = (1 << 64) - 1
    return [
        ("csl_k6", csl, 100, 6, "sample", 42),
        ("csl_k6_global", csl, 100, 6, "global", 0),
        ("mutag_k4", mutag, 32, 4, "sample", 0),
        ("mutag_k5", mutag, 32, 5, "global", 42),
        ("mutag_k6", mutag, 32, 6, "sample", U64),
        ("ptc_k4_64", ptc64, 24, 4, "sample", 42),
        ("ptc_k5_64", ptc64, 24, 5, "graph", U64),
        ("ptc_k6", ptc, 24, 6, "sample", 0),
        ("edge_k4", edge, 20, 4, "sample", 42),
        ("edge_k4_global", edge, 20, 4, "global", U64),
        ("edge_k1", edge, 30, 1, "sample", 0),
        ("edge_k1_global", edge, 5, 1, "global", 42),
        ("edge_k0", edge, 3, 0, "sample", 42),
        ("edge_k2", edge, 7, 2, "sample", U64),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("module", help="path of the hand-built reference uniform_sampler extension module")
    ap.add_argument("--cmd", default="", help="the command that built it (recorded)")
    ap.add_argument("--sha256", default="", help="sha256 of the uniform_sampler.cpp it was built from (recorded)")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("uniform_sampler", a.module)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    arrays, meta = {}, []
    for name, (ei, ptr), m, k, mode, seed in scenarios():
        out = ref.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode, seed)
        arrays[f"{name}/in_edge_index"] = ei
        arrays[f"{name}/in_ptr"] = ptr
        for t, nm in zip(out, NAMES):
            arrays[f"{name}/{nm}"] = t.numpy()
        meta.append(dict(name=name, m=m, k=k, mode=mode, seed=str(seed), graphs=int(len(ptr) - 1), rows=int(out[0].shape[0]),
                         edges=int(out[1].shape[1])))
        print(name, meta[-1])
    np.savez_compressed(OUT + ".npz", **arrays)
    with open(OUT + ".json", "w") as f:
        json.dump(dict(source="reference uniform_sampler (src/samplers/uniform_sampler/src/uniform_sampler.cpp)",
                       source_sha256=a.sha256, build_command=a.cmd, scenarios=meta), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
