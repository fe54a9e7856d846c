#!/usr/bin/env python3
"""Generates tests/golden/f20_wl_feature_reference.npz (+ .json): what the reference's SS-GNN-WL path computes with
use_node_features_in_wl=True for fixed sampler outputs and feature matrices, for the bit-exact parity tests
(tests/test_wl_feature_law.py against the plain-Python law, tests/test_gpu_wl_features.py against the HIP product).

Runs on the CPU.  It loads the reference's src/gps/gps/utils/wl_vocab.py BY PATH (needs networkx, tqdm and torch) and, per scenario,
  * extracts every row with its extract_subgraph_from_batch (batch.x set: the features of the row's valid entries, in row order)
    and hashes it with its compute_wl_hash(node_features=...) (rows without valid vertices are skipped, as in _compute_wl_ids),
  * builds a vocabulary in first-seen order from the first half of the rows (build_wl_vocabulary_from_loader:156-175),
  * records the ids of _compute_wl_ids's rule (ss_gnn_wl.py:224-247: len(vocab) for rows without vertices and unknown hashes).

    python tools/make_golden_wl_features.py /path/to/reference/src/gps/gps/utils/wl_vocab.py

Inputs: rows of this repository's CPU oracle for `ugs` (k = 4, 6, 8) with one-hot float32 features of 3, 7 and 18 columns (the
widths of PROTEINS, MUTAG and PTC_MR; 18 columns are 72 bytes, two MD5 blocks), an int64 and a float64 feature matrix, and
hand-made rows.  The json records the networkx version and the sha256 of the reference source.  Only data goes into the fixture.
"""
import hashlib
import importlib.util
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ss-gnn_amd", "oracle", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))
import oracle  # noqa: E402
import ugs_workloads as wl  # noqa: E402
from make_golden_wl import deviation_rows, rows_of  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "f20_wl_feature_reference")


def one_hot(rng, n, f, dtype=np.float32):
    x = np.zeros((n, f), dtype)
    x[np.arange(n), rng.integers(0, f, n)] = 1
    return x


def hand_made(k=16):
    """Rows over 48 vertex ids: interior -1 entries, duplicate ids, n = 0, n = 1, a loop, a vertex of degree 15."""
    both = lambda es: [e for u, v in es for e in ((u, v), (v, u))]           # noqa: E731
    pad = lambda r: list(r) + [-1] * (k - len(r))                            # noqa: E731
    return rows_of([
        (pad([5, -1, 7, -1, 9]), both([(0, 1), (1, 2)])),                     # interior -1: 7 is vertex 1, 9 is vertex 2
        (pad([-1, -1, 3, 4]), both([(0, 1)])),                                # leading -1
        ([39] * k, both([(0, 1), (2, 3)])),                                   # one id k times: k vertices with one label
        (pad([11, 12, 11, 13, 12]), both([(0, 1), (1, 2), (2, 3), (3, 4)])),  # duplicates among others
        (pad([]), []),                                                        # n = 0
        (pad([47]), []),                                                      # n = 1
        (pad([0]), [(0, 0)]),                                                 # n = 1 with a loop
        (pad([1, 2, 3, 4]), both([(0, 1), (1, 2), (2, 3)]) + [(2, 2)]),       # a loop inside a path
        (list(range(20, 20 + k)), both([(0, i) for i in range(1, k)])),       # degree 15: a first message of 8 + 15 * 8 = 128 bytes
        (list(range(k)), both([(0, i) for i in range(1, k - 1)])),            # degree 14 beside it
        (pad([-1, 30, -1, 31, 32, -1, 33]), both([(0, 1), (1, 2), (2, 3), (3, 0)])),
        (pad([]), []),
        (list(range(10, 10 + k)), []),                                        # k isolated vertices
        (pad([8, 9, 10, 11, 12]), [(0, 1), (0, 1), (1, 0), (1, 2), (3, 4), (4, 3), (3, 4)]),
    ])


def scenarios():
    out = []
    rng = np.random.default_rng(20)
    for name, (n, e, g), m, k, it, seed, f in (("tu_k4_f3_it1", (17, 24, 6), 6, 4, 1, 1, 3), ("tu_k4_f7_it3", (17, 24, 6), 6, 4, 3, 2, 7),
                                               ("tu_k6_f3_it3", (39, 73, 6), 6, 6, 3, 42, 3), ("tu_k6_f7_it3", (28, 40, 6), 6, 6, 3, 5, 7),
                                               ("tu_k6_f18_it3", (26, 52, 6), 6, 6, 3, 6, 18), ("tu_k8_f3_it3", (39, 73, 5), 8, 8, 3, 7, 3),
                                               ("tu_k8_f18_it1", (28, 40, 4), 8, 8, 1, 9, 18)):
        ei, ptr = wl.tu_batch(n, e, g)
        nodes, eidx, eptr = oracle.sample_batch(ei, ptr, m, k, "sample", seed)[:3]
        what = "CPU oracle, ugs sample_batch(tu_batch(%d, %d, %d), m=%d, k=%d, mode='sample', seed=%d); x one-hot float32 [%d, %d]" % (n, e, g, m, k, seed, ptr[-1], f)
        out.append((name, what, it, nodes, eidx, eptr, one_hot(rng, int(ptr[-1]), f), False))
    ei, ptr = wl.tu_batch(22, 30, 5)
    nodes, eidx, eptr = oracle.sample_batch(ei, ptr, 6, 6, "sample", 13)[:3]
    x_i64 = rng.integers(-3, 4, (int(ptr[-1]), 9)).astype(np.int64) * (rng.random((int(ptr[-1]), 9)) < 0.3)
    out.append(("tu_k6_int64_f9_it3", "CPU oracle, ugs sample_batch(tu_batch(22, 30, 5), m=6, k=6, seed=13); x int64 [N, 9] of small values", 3,
                nodes, eidx, eptr, x_i64, False))
    x_f64 = np.round(rng.standard_normal((int(ptr[-1]), 2)), 1)
    out.append(("tu_k6_float64_f2_it1", "the same rows; x float64 [N, 2] rounded to one decimal (ties and distinct rows)", 1,
                nodes, eidx, eptr, x_f64.astype(np.float64), False))
    x_hand = one_hot(rng, 48, 7)
    out.append(("hand_made_it3", "hand-made rows, k = 16, x one-hot float32 [48, 7]", 3) + hand_made() + (x_hand, False))
    out.append(("hand_made_it1", "hand-made rows, k = 16, x one-hot float32 [48, 7]", 1) + hand_made() + (x_hand, False))
    out.append(("hand_made_distinct_it3", "hand-made rows, k = 16, x float32 [48, 1] = arange: all labels distinct", 3) + hand_made()
               + (np.arange(48, dtype=np.float32).reshape(48, 1), False))
    out.append(("bad_endpoints_it3", "rows with an endpoint outside [0, n): the documented deviation; x one-hot float32 [8, 3]", 3) + deviation_rows()
               + (one_hot(rng, 8, 3), True))
    return out


def main():
    src = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_wl_vocab", src)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    import networkx
    arrays, meta = {}, []
    for i, (name, what, it, nodes, eidx, eptr, x, deviation) in enumerate(scenarios()):
        nodes_t, eidx_t, eptr_t = (torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)) for a in (nodes, eidx, eptr))
        S = nodes_t.shape[0]
        batch = SimpleNamespace(x=torch.from_numpy(np.ascontiguousarray(x)))
        hashes = []
        for r in range(S):
            edges, n, feats = ref.extract_subgraph_from_batch(batch, r, nodes_t, eidx_t, eptr_t)
            hashes.append(None if n == 0 else ref.compute_wl_hash(edge_index=edges, num_nodes=n, node_features=feats, num_iterations=it))
        vocab = {}
        for h in hashes[:(S + 1) // 2]:
            if h is not None and h not in vocab:
                vocab[h] = len(vocab)
        ids = [len(vocab) if h is None else ref.hash_to_id(h, vocab) for h in hashes]
        arrays["s%d_nodes" % i], arrays["s%d_edge_index" % i], arrays["s%d_edge_ptr" % i] = nodes_t.numpy(), eidx_t.numpy(), eptr_t.numpy()
        arrays["s%d_x" % i] = batch.x.numpy()
        arrays["s%d_ids" % i] = np.array(ids, np.int64)
        meta.append({"name": name, "inputs": what, "k": int(nodes_t.shape[1]), "iterations": it, "rows": S, "deviation": deviation,
                     "x_dtype": str(batch.x.numpy().dtype), "x_shape": list(batch.x.shape), "hashes": hashes, "vocab": list(vocab)})
    np.savez_compressed(OUT + ".npz", **arrays)
    with open(src, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(OUT + ".json", "w") as f:
        json.dump({"source": "reference SS-GNN-WL host path with use_node_features_in_wl=True (src/gps/gps/utils/wl_vocab.py: "
                             "extract_subgraph_from_batch, compute_wl_hash with node_features, hash_to_id; id rule of "
                             "src/gps/gps/models/ss_gnn_wl.py:224-247)",
                   "source_sha256": sha, "networkx": networkx.__version__,
                   "vocab_rule": "first-seen order over the first (rows + 1) // 2 rows of the scenario; 'vocab'[i] has id i",
                   "scenarios": meta}, f, indent=1)
    print("wrote", OUT + ".npz", os.path.getsize(OUT + ".npz"), "bytes;", OUT + ".json", os.path.getsize(OUT + ".json"), "bytes;",
          sum(m["rows"] for m in meta), "rows")


if __name__ == "__main__":
    main()
