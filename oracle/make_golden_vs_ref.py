#!/usr/bin/env python3
"""oracle/make_golden_vs_ref.py -- TEST INFRASTRUCTURE ONLY.

Writes, from the REFERENCE's own modules (oracle/_ref, built from the reference's sources by oracle/build_ref.py):
  * tests/golden/f12_oracle_vs_ref.npz: the reference's outputs for the seeded random calls of tests/test_oracle_vs_ref.py,
    in one fresh process and in the test's order (the reference's preprocessing LRU is process-global);
  * tests/golden/f13_eps_reference_draws.npz (`--eps`): one draw of the reference epsilon_uniform_sampler per case of
    tests/test_eps_oracle.py (its output is not reproducible: per-thread generators), as small integers.
Runs only where the reference's sources are present; the fixtures (data only) are committed so that the tests need neither
the reference nor this script.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)


def main():
    import build_ref
    import test_oracle_vs_ref as t
    build_ref.build()
    ref = build_ref.load()
    arrays = {}
    for i, call in enumerate(t.handle_calls()):
        info, out = t.run_handle_call(ref, call)
        arrays[f"h{i}_info"] = info
        for j, a in enumerate(out):
            arrays[f"h{i}_{j}"] = a
    for i, call in enumerate(t.batch_calls()):
        for j, a in enumerate(t.run_batch_call(ref, call)):
            arrays[f"b{i}_{j}"] = a
    np.savez_compressed(t.GOLDEN, **arrays)
    print(t.GOLDEN, len(arrays), "arrays", os.path.getsize(t.GOLDEN), "bytes")


def main_eps():
    import build_ref
    import test_eps_oracle as t
    build_ref.build_eps()
    os.environ["OMP_NUM_THREADS"] = "1"
    ref = build_ref.load_eps()
    arrays = {}
    for name in sorted(t.GRAPHS):
        for k, eps in t.CASES:
            key = t.golden_key(name, k, eps)
            for part, a in zip(("nodes", "edge_index", "edge_ptr", "edge_src"), t.draw(ref, name, k, eps)):
                small = np.int8 if part == "nodes" else np.int32          # vertex ids of graphs of <= 6 vertices; offsets
                assert np.array_equal(a.astype(small), a)
                arrays[f"{key}_{part}"] = a.astype(small)
    np.savez_compressed(t.GOLDEN, **arrays)
    print(t.GOLDEN, len(arrays), "arrays", os.path.getsize(t.GOLDEN), "bytes")


if __name__ == "__main__":
    main_eps() if "--eps" in sys.argv else main()
