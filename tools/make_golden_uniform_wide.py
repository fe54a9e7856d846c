#!/usr/bin/env python3
"""Generates tests/golden/f18_uniform_wide_reference.npz (+ .json): outputs of the reference `uniform_sampler` module on graphs
of more than 64 vertices, for the wide form of the HIP product (tests/test_uniform_wide_law.py, tests/test_gpu_uniform_wide.py).

Same recipe as tools/make_golden_uniform.py: the reference module is built by hand, outside the tree, and only its outputs are
stored.  The reference scans all C(n, k) combinations, so every scenario keeps C(n, k) below about 1.5e7.

    python tools/make_golden_uniform_wide.py /path/to/uniform_sampler.<ext-suffix>.so --cmd "<the g++ line>" --sha256 <of uniform_sampler.cpp>
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ugs_workloads as wl  # noqa: E402
from uniform_wide_law import batch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "f18_uniform_wide_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def one(n, e, s):
    return batch([(n, wl.tu_graph(n, e, s))])


def mixed_batch():
    """ptr[0] = 5; graphs of 14, 64, 65 and 129 vertices; a loop (3, 3) and a duplicate of column 0 in the 65-vertex graph; one
    column from the 14-vertex graph into the 129-vertex graph."""
    g65 = wl.tu_graph(65, 72, 21)
    g65 = np.concatenate([g65, np.array([[3], [3]], np.int64), g65[:, :1]], axis=1)
    ei, ptr = batch([(14, wl.tu_graph(14, 15, 20)), (64, wl.tu_graph(64, 70, 22)), (65, g65), (129, wl.tu_graph(129, 140, 23))], first=5)
    cross = np.array([[ptr[0] + 2], [ptr[3] + 100]], np.int64)
    return np.concatenate([ei[:, :9], cross, ei[:, 9:]], axis=1), ptr


def scenarios():
    U64 = (1 << 64) - 1
    mixed = mixed_batch()
    return [
        ("tu65_k4", one(65, 70, 1), 32, 4, "sample", 42),
        ("tu100_k4", one(100, 110, 2), 32, 4, "global", 0),
        ("tu129_k4", one(129, 300, 3), 32, 4, "sample", U64),
        ("tu300_k3", one(300, 330, 5), 32, 3, "global", 42),
        ("tu136_k4_dense", one(136, 1300, 10), 48, 4, "sample", 0),
        ("tu1024_k2", one(1024, 1100, 7), 32, 2, "sample", U64),
        ("tu1024_k2_global", one(1024, 1100, 7), 16, 2, "global", 42),
        ("mixed_k3", mixed, 20, 3, "sample", 42),
        ("mixed_k3_global", mixed, 20, 3, "global", U64),
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
