#!/usr/bin/env python3
"""Generates tests/golden/f19_wl_reference.npz (+ .json): what the reference's SS-GNN-WL path computes for fixed sampler outputs,
for the bit-exact parity tests (tests/test_wl_law.py against the plain-Python law, tests/test_gpu_wl.py against the HIP product).

Runs on the CPU.  It loads the reference's src/gps/gps/utils/wl_vocab.py BY PATH (needs networkx, tqdm and torch) and, per scenario,
  * extracts every row with its extract_subgraph_from_batch and hashes it with its compute_wl_hash (rows without valid vertices
    are skipped, as in _compute_wl_ids and build_wl_vocabulary_from_loader),
  * builds a vocabulary in first-seen order from the first half of the rows (build_wl_vocabulary_from_loader:156-175), so that
    the second half also holds unknown hashes,
  * records the ids of _compute_wl_ids's rule (ss_gnn_wl.py:224-247: len(vocab) for rows without vertices and unknown hashes).

    python tools/make_golden_wl.py /path/to/reference/src/gps/gps/utils/wl_vocab.py

Inputs: rows of this repository's CPU oracle for `ugs` (k = 4, 6, 8), the row sets of existing fixtures, and hand-made rows.
The json records the networkx version and the sha256 of the reference source.  Only data goes into the fixture.
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
for p in ("ss-gnn_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import oracle  # noqa: E402
import ugs_workloads as wl  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "f19_wl_reference")


def rows_of(entries):
    """(nodes [S, k], edge_index [2, E], edge_ptr [S+1]) from a list of (row of k ids, [(u, v), ...])."""
    nodes = np.array([r for r, _ in entries], np.int64)
    cols, ptr = [], [0]
    for _, es in entries:
        cols += list(es)
        ptr.append(len(cols))
    ei = np.array(cols, np.int64).reshape(-1, 2).T if cols else np.zeros((2, 0), np.int64)
    return nodes, np.ascontiguousarray(ei), np.array(ptr, np.int64)


def hand_made(k=8):
    def row(n, fill=7):
        return [fill + i for i in range(n)] + [-1] * (k - n)
    both = lambda es: [e for u, v in es for e in ((u, v), (v, u))]           # noqa: E731  (a sampler lists both directions)
    path = [(i, i + 1) for i in range(k - 1)]
    return rows_of([
        (row(0), []),                                                         # n = 0
        (row(1), []),                                                         # n = 1
        (row(k), []),                                                         # k isolated vertices
        (row(k), both(path)),                                                 # path
        (row(k), both([(0, i) for i in range(1, k)])),                        # star
        (row(k), both([(i, j) for i in range(k) for j in range(i + 1, k)])),  # clique
        (row(4), both([(0, 1), (1, 2), (2, 3)]) + [(2, 2)]),                  # a self-loop
        (row(5), [(0, 1), (0, 1), (1, 0), (1, 2), (3, 4), (4, 3), (3, 4)]),   # duplicate and reversed entries, one direction only
        (row(1), [(0, 0)]),                                                   # a lone vertex with a loop
        (row(k, fill=40), []),                                                # presample cache: a failed graph at a later ptr (rows of ptr[g] - 1, no edges)
        ([39] * k, []),
        (row(k), both(path) + both([(0, k - 1)])),                            # cycle
        (row(0), []),
        (row(6), both([(0, 1), (0, 2), (0, 3), (1, 4), (1, 5)])),            # degree-3 vertices: messages of 128 bytes from iteration 2 on
        (row(k), both([(0, i) for i in range(1, k)] + [(1, 2)])),             # a degree-7 vertex: a message of 256 bytes
    ])


def deviation_rows(k=4):
    """Rows with an endpoint outside [0, n): the reference answers its fallback string, the library status 2."""
    return rows_of([
        ([3, 4, 5, -1], [(0, 1), (1, 0), (1, 3)]),                            # endpoint >= n
        ([3, 4, 5, 6], [(0, 1), (-1, 2)]),                                    # negative endpoint
        ([3, 4, 5, 6], [(0, 1), (1, 2), (2, 3)]),                             # a good row between them
        ([3, 4, -1, -1], [(0, 1), (1, 0), (0, 2)]),
    ])


def scenarios():
    out = []
    for name, (n, e, g), m, k, it, seed in (("tu_k4_it1", (17, 24, 6), 6, 4, 1, 1), ("tu_k4_it3", (17, 24, 6), 6, 4, 3, 2),
                                            ("tu_k6_it3", (39, 73, 6), 6, 6, 3, 42), ("tu_k6_it1", (39, 73, 4), 8, 6, 1, 5),
                                            ("tu_k8_it3", (39, 73, 5), 8, 8, 3, 7), ("tu_k8_it1", (28, 40, 4), 8, 8, 1, 9)):
        ei, ptr = wl.tu_batch(n, e, g)
        nodes, eidx, eptr = oracle.sample_batch(ei, ptr, m, k, "sample", seed)[:3]
        out.append((name, "CPU oracle, ugs sample_batch(tu_batch(%d, %d, %d), m=%d, k=%d, mode='sample', seed=%d)" % (n, e, g, m, k, seed), it, nodes, eidx, eptr, False))
    f8 = np.load(os.path.join(GOLDEN, "f8_tu_shapes.npz"))
    out.append(("f8_c0_it3", "rows of f8_tu_shapes.npz case 0", 3, f8["c0_out0"], f8["c0_out1"], f8["c0_out2"], False))
    f6 = np.load(os.path.join(GOLDEN, "f6_degenerate_in_batch.npz"))
    for c in range(9):
        if "c%d_out0" % c in f6 and (f6["c%d_out1" % c].size == 0 or f6["c%d_out1" % c].max() < f6["c%d_out0" % c].shape[1]):
            out.append(("f6_c%d_it3" % c, "rows of f6_degenerate_in_batch.npz case %d (graphs with fewer than k vertices: rows of -1)" % c, 3,
                        f6["c%d_out0" % c], f6["c%d_out1" % c], f6["c%d_out2" % c], False))
            break
    out.append(("hand_made_it3", "hand-made rows, k = 8", 3) + hand_made() + (False,))
    out.append(("hand_made_it1", "hand-made rows, k = 8", 1) + hand_made() + (False,))
    out.append(("bad_endpoints_it3", "rows with an endpoint outside [0, n): the documented deviation", 3) + deviation_rows() + (True,))
    return out


def main():
    src = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_wl_vocab", src)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    import networkx
    arrays, meta = {}, []
    for i, (name, what, it, nodes, eidx, eptr, deviation) in enumerate(scenarios()):
        nodes_t, eidx_t, eptr_t = (torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)) for x in (nodes, eidx, eptr))
        S = nodes_t.shape[0]
        batch = SimpleNamespace(x=None)
        hashes = []
        for r in range(S):
            edges, n, _ = ref.extract_subgraph_from_batch(batch, r, nodes_t, eidx_t, eptr_t)
            hashes.append(None if n == 0 else ref.compute_wl_hash(edge_index=edges, num_nodes=n, node_features=None, num_iterations=it))
        vocab = {}
        for h in hashes[:(S + 1) // 2]:
            if h is not None and h not in vocab:
                vocab[h] = len(vocab)
        ids = [len(vocab) if h is None else ref.hash_to_id(h, vocab) for h in hashes]
        arrays["s%d_nodes" % i], arrays["s%d_edge_index" % i], arrays["s%d_edge_ptr" % i] = nodes_t.numpy(), eidx_t.numpy(), eptr_t.numpy()
        arrays["s%d_ids" % i] = np.array(ids, np.int64)
        meta.append({"name": name, "inputs": what, "k": int(nodes_t.shape[1]), "iterations": it, "rows": S, "deviation": deviation,
                     "hashes": hashes, "vocab": list(vocab)})
    np.savez_compressed(OUT + ".npz", **arrays)
    with open(src, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    with open(OUT + ".json", "w") as f:
        json.dump({"source": "reference SS-GNN-WL host path (src/gps/gps/utils/wl_vocab.py: extract_subgraph_from_batch, compute_wl_hash, "
                             "hash_to_id; id rule of src/gps/gps/models/ss_gnn_wl.py:224-247)",
                   "source_sha256": sha, "networkx": networkx.__version__,
                   "vocab_rule": "first-seen order over the first (rows + 1) // 2 rows of the scenario; 'vocab'[i] has id i",
                   "scenarios": meta}, f, indent=1)
    print("wrote", OUT + ".npz", os.path.getsize(OUT + ".npz"), "bytes;", OUT + ".json", os.path.getsize(OUT + ".json"), "bytes;",
          sum(m["rows"] for m in meta), "rows")


if __name__ == "__main__":
    main()
