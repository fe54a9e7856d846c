#!/usr/bin/env python3
"""Generates tests/golden/f15_rwr_reference.npz (+ .json): outputs of the reference `rwr_sampler` module
(AniruddhaMandal/SS-GNN src/samplers/rwr_sampler) on fixed batches, for the bit-exact parity tests
(tests/test_rwr_law.py against the CPU restatement, tests/test_gpu_rwr.py against the HIP product).

The reference module is not built by this repository: compile it by hand, outside the tree, from the reference's
rwr_sampler.cpp (one g++ line with torch / pybind11 includes, -fopenmp, and `pinned_memory(x)` re-spelled
`pinned_memory(false)` by a macro so that a machine without a GPU can allocate its outputs), then run, with ONE OpenMP thread
(the only deterministic setting of the reference: its seeds and row order depend on the thread schedule otherwise),

    OMP_NUM_THREADS=1 python tools/make_golden_rwr.py /path/to/rwr_sampler.<ext-suffix>.so --cmd "<the g++ line>" --sha256 <of rwr_sampler.cpp>

The command, the thread count and the source hash are recorded in the json next to the scenarios.
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

OUT = os.path.join(ROOT, "tests", "golden", "f15_rwr_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def batch(graphs, first=0):
    """Concatenates local edge_index arrays [(n, ei)] into a PyG batch starting at vertex `first`."""
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(np.asarray(ei, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


def edge_case_batch():
    """ptr[0] = 5; a 7-vertex graph with an isolated vertex (6), a loop (2, 2) and a duplicate column (0, 1); a 3-vertex graph
    (n < k for k >= 4); an empty graph; a 6-vertex graph; one column across graphs 0 and 3."""
    g0 = np.array([[0, 1, 1, 2, 3, 2, 0, 4], [1, 2, 3, 2, 4, 4, 1, 5]], np.int64)
    g1 = np.array([[0, 1], [1, 2]], np.int64)
    g3 = np.array([[0, 1, 2, 3, 4, 0, 1, 2], [1, 2, 3, 4, 5, 2, 0, 0]], np.int64)
    ei, ptr = batch([(7, g0), (3, g1), (0, np.zeros((2, 0))), (6, g3)], first=5)
    ei = np.concatenate([ei[:, :5], np.array([[6], [ptr[3] + 1]], np.int64), ei[:, 5:]], axis=1)   # cross-graph column
    return ei, ptr


def small_component_batch():
    """Graphs with components smaller than k, so that some walks run the full 10 n k iterations: a 12-vertex graph made of a
    9-vertex tree, a triangle-free pair with a loop (9, 10) and an isolated vertex (11); a 10-vertex graph of two 5-paths; a graph
    whose vertex 3 has only a loop."""
    t = wl.tu_graph(9, 8, 7)
    g0 = np.concatenate([t, np.array([[9, 10, 10], [10, 9, 10]], np.int64)], axis=1)
    g1 = np.array([[0, 1, 2, 3, 5, 6, 7, 8], [1, 2, 3, 4, 6, 7, 8, 9]], np.int64)
    g2 = np.concatenate([wl.tu_graph(3, 2, 1), np.array([[3], [3]], np.int64), wl.tu_graph(3, 3, 2) + 4], axis=1)
    return batch([(12, g0), (10, g1), (7, g2)])


def scenarios():
    proteins = wl.tu_batch(39, 73, 8)
    mutag = wl.tu_batch(18, 20, 8, dataset_seed=1)
    tree = wl.tu_batch(30, 29, 6, dataset_seed=2)
    edge = edge_case_batch()
    small = small_component_batch()
    U64 = (1 << 64) - 1
    return [
        ("proteins_k6", proteins, 24, 6, "sample", 42, 0.2),
        ("proteins_k5_global", proteins, 8, 5, "global", 7, 0.2),
        ("mutag_k5", mutag, 16, 5, "sample", 0, 0.2),
        ("mutag_k8", mutag, 16, 8, "graph", 42, 0.2),
        ("tree_k8", tree, 16, 8, "sample", 123, 0.2),
        ("tree_k6_p05", tree, 8, 6, "sample", 5, 0.5),
        ("edge_k4", edge, 20, 4, "sample", 42, 0.2),
        ("edge_k4_global", edge, 12, 4, "global", U64, 0.2),
        ("edge_k3_graph", edge, 12, 3, "graph", 3, 0.3),
        ("small_k4", small, 20, 4, "sample", 42, 0.2),
        ("small_k6_global", small, 10, 6, "global", 11, 0.2),
        ("p0_k5", mutag, 8, 5, "sample", 42, 0.0),
        ("p1_k3", edge, 6, 3, "sample", 42, 1.0),
        ("p1_k1", edge, 6, 1, "sample", 9, 1.0),
        ("loops_k1", edge, 10, 1, "sample", 42, 0.2),
        ("loops_k1_global", small, 5, 1, "global", 1, 0.2),
        ("m0_k5", proteins, 0, 5, "sample", 42, 0.2),
        ("seed_top_k6", proteins, 6, 6, "sample", U64 - 3, 0.2),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("module", help="path of the hand-built reference rwr_sampler extension module")
    ap.add_argument("--cmd", default="", help="the command that built it (recorded)")
    ap.add_argument("--sha256", default="", help="sha256 of the rwr_sampler.cpp it was built from (recorded)")
    a = ap.parse_args()
    threads = os.environ.get("OMP_NUM_THREADS")
    if threads != "1":
        sys.exit("run with OMP_NUM_THREADS=1: the reference is deterministic with one thread only")
    spec = importlib.util.spec_from_file_location("rwr_sampler", a.module)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    arrays, meta = {}, []
    for name, (ei, ptr), m, k, mode, seed, p in scenarios():
        out = ref.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode, seed, p)
        arrays[f"{name}/in_edge_index"] = ei
        arrays[f"{name}/in_ptr"] = ptr
        for t, nm in zip(out, NAMES):
            arrays[f"{name}/{nm}"] = t.numpy()
        rows = out[0].numpy()
        meta.append(dict(name=name, m=m, k=k, mode=mode, seed=str(seed), p_restart=p, graphs=int(len(ptr) - 1),
                         rows=int(rows.shape[0]), failed_rows=int((rows[:, 0] < 0).sum()) if rows.size else 0,
                         edges=int(out[1].shape[1])))
        print(name, meta[-1])
    np.savez_compressed(OUT + ".npz", **arrays)
    with open(OUT + ".json", "w") as f:
        json.dump(dict(source="reference rwr_sampler (src/samplers/rwr_sampler/src/rwr_sampler.cpp)", source_sha256=a.sha256,
                       build_command=a.cmd, omp_num_threads=int(threads), scenarios=meta), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
