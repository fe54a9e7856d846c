#!/usr/bin/env python3
"""Times the node-feature form of ugs_sampler.wl (WLVocab.ids(x=)) against the host loop it replaces, and holds the degree form
to the previous commit's library.  A sibling of tools/wl_bench.py: same shapes (PROTEINS-shaped c3: 8192 rows, k = 6, with one-hot
float32 features of 3 columns; COCO-SP-shaped c6: 3200 rows, k = 8, with 7 columns), iterations 3, medians of --calls calls after
warm-up, each call ended by a device synchronise.

  (a) WLVocab.ids(x=) and its parts: feature_labels, wl_hash(node_labels=), lookup.
  (b) the reference's host loop with features on one CPU core -- per row three .item() reads, x[valid ids], a networkx.Graph, one
      hashlib.md5 per vertex, weisfeiler_lehman_graph_hash and a dict lookup (src/gps/gps/utils/wl_vocab.py:21-107,
      src/gps/gps/models/ss_gnn_wl.py:210-247) -- in a child process started and finished before this process's first GPU call,
      on the CPU oracle's rows (bit-exact with the GPU sampler); the parent compares the ids.
  (c) with --parent-lib: the degree-labelled hash + lookup through the C ABI of this commit's library and of a library built
      from the parent commit, interleaved call by call in one session, and the labelled hash kernel of this commit against the
      parent's degree-labelled one on the same rows (HIP events around the single launch).  Two conditions are evaluated:
      1. this commit's degree-labelled median lies within the parent's own min-max spread of the session;
      2. the feature-labelled hash kernel is at most 1.10 x the parent's degree-labelled kernel.

    python tools/wl_features_bench.py --out profiles/wl_features_bench.json [--parent-lib /path/to/parent/libugs_mi355.so]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ss-gnn_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

SHAPES = (("c3_proteins_b8192", 3), ("c6_cocosp_b3200", 7))
ITERATIONS, SEED = 3, 42


def features(num_nodes, F):
    import numpy as np
    return np.eye(F, dtype=np.float32)[np.random.default_rng(F).integers(0, F, num_nodes)]


def baseline_child(shape, F):
    """One CPU core: rows from the CPU oracle, then the per-row host loop with features.  Prints one JSON line."""
    import networkx as nx
    import numpy as np
    import torch
    torch.set_num_threads(1)
    import oracle
    import ugs_workloads as workloads
    import wl_feature_law as law
    ei, ptr, m, k = workloads.workload(shape)
    nodes, eidx, eptr = (torch.from_numpy(np.ascontiguousarray(a)) for a in oracle.sample_batch(ei, ptr, m, k, "sample", SEED)[:3])
    x_np = features(int(ptr[-1]), F)
    x = torch.from_numpy(x_np)

    def ids_of(vocab):
        out = []
        for i in range(nodes.shape[0]):
            row = nodes[i]
            valid = row >= 0
            n = valid.sum().item()
            edges = eidx[:, eptr[i].item():eptr[i + 1].item()]
            if n == 0:
                out.append(len(vocab))
                continue
            feats = x[row[valid]]
            G = nx.Graph()
            G.add_nodes_from(range(n))
            if edges.numel() > 0:
                G.add_edges_from(edges.t().numpy())
            for u in range(n):
                G.nodes[u]["attr"] = hashlib.md5(feats[u].numpy().tobytes()).hexdigest()[:8]
            out.append(vocab.get(nx.weisfeiler_lehman_graph_hash(G, node_attr="attr", iterations=ITERATIONS), len(vocab)))
        return out

    hexes, stats, _ = law.wl_feature_rows(nodes.numpy(), eidx.numpy(), eptr.numpy(), law.labels_of(x_np), ITERATIONS)
    vocab = {}
    for h in hexes[:len(hexes) // 2]:
        if h is not None and h not in vocab:
            vocab[h] = len(vocab)
    t0 = time.perf_counter()
    ids = ids_of(vocab)
    dt = time.perf_counter() - t0
    assert ids == [vocab.get(h, len(vocab)) if st == 0 else len(vocab) for h, st in zip(hexes, stats)], "the host loop and the law disagree"
    print(json.dumps({"shape": shape, "engine": "networkx " + nx.__version__ + " + hashlib.md5", "rows": len(ids), "k": k, "seconds": dt,
                      "vocab": list(vocab), "ids": ids}))


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}


def timed(fn, calls, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return summary(ts)


def interleaved(fns, calls, warmup=5):
    """Wall time (call + synchronise) and HIP-event time of several callables, taken in turns: {name: (wall, events)}."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    wall, dev = {n: [] for n in fns}, {n: [] for n in fns}
    for _ in range(calls):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            dev[name].append(a.elapsed_time(b))
    return {n: {"wall": summary(wall[n]), "events": summary(dev[n])} for n in fns}


def bind(path):
    """The WL entry points of a library file through ctypes, on device 0 and torch's current stream."""
    import torch
    L = C.CDLL(path)
    vp = C.c_void_p
    L.ugs_set_device.argtypes = [C.c_int]
    L.ugs_set_stream.argtypes = [vp, C.c_int]
    L.ugs_wl_hash.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int, C.c_int, vp, vp]
    L.ugs_wl_lookup.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, C.c_int64, vp]
    assert L.ugs_set_device(0) == 0 and L.ugs_set_stream(torch.cuda.current_stream(0).cuda_stream, 1) == 0
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libugs_mi355.so built from the parent commit, for the A/B of the degree form")
    ap.add_argument("--baseline-child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.baseline_child:
        return baseline_child(args.baseline_child[0], int(args.baseline_child[1]))

    base = {}
    if not args.no_baseline:                           # before the first GPU call of this process, one shape after the other
        env = dict(os.environ, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
        for shape, F in SHAPES:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-child", shape, str(F)], env=env, check=True,
                                 capture_output=True, text=True).stdout
            base[shape] = json.loads(out.strip().splitlines()[-1])

    import torch
    import ugs_sampler
    import ugs_workloads as workloads
    import wl_feature_law as law
    from ugs_sampler import wl
    from ugs_sampler._lib import LIB_PATH
    dev = "cuda:0"
    results = {"device": torch.cuda.get_device_name(0), "iterations": ITERATIONS, "shapes": {}}
    for shape, F in SHAPES:
        ei, ptr, m, k = workloads.workload(shape)
        nodes, eidx, eptr = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode="sample", seed=SEED, device=dev)[:3]
        x_np = features(int(ptr[-1]), F)
        x = torch.from_numpy(x_np).to(dev)
        S = int(nodes.shape[0])
        if shape in base:
            vocab = {h: i for i, h in enumerate(base[shape]["vocab"])}
        else:
            vocab = wl.extend_vocab({}, *wl.wl_hash(nodes[:S // 2], eidx, eptr[:S // 2 + 1], ITERATIONS, x=x))
        table = wl.WLVocab(vocab, dev)
        ids = table.ids(nodes, eidx, eptr, ITERATIONS, x=x)
        if shape in base:
            assert ids.cpu().tolist() == base[shape]["ids"], "GPU ids differ from the host loop's"
        hexes, stats, _ = law.wl_feature_rows(nodes[:64].cpu().numpy(), eidx.cpu().numpy(), eptr[:65].cpu().numpy(), law.labels_of(x_np), ITERATIONS)
        assert ids[:64].cpu().tolist() == [vocab.get(h, len(vocab)) if st == 0 else len(vocab) for h, st in zip(hexes, stats)], "GPU ids differ from the law's"
        labels = wl.feature_labels(x)
        digest, status = wl.wl_hash(nodes, eidx, eptr, ITERATIONS, node_labels=labels)
        deg_table = wl.WLVocab(wl.extend_vocab({}, *wl.wl_hash(nodes[:S // 2], eidx, eptr[:S // 2 + 1], ITERATIONS)), dev)
        r = {"rows": S, "k": k, "edge_entries": int(eidx.shape[1]), "x": [int(x.shape[0]), F, "float32"], "vocab": len(vocab),
             "unknown_rows": int((ids == len(vocab)).sum()),
             "wl_ids_x": timed(lambda: table.ids(nodes, eidx, eptr, ITERATIONS, x=x), args.calls),
             "feature_labels": timed(lambda: wl.feature_labels(x), args.calls),
             "wl_hash_node_labels": timed(lambda: wl.wl_hash(nodes, eidx, eptr, ITERATIONS, node_labels=labels), args.calls),
             "lookup": timed(lambda: table.lookup(digest, status), args.calls),
             "wl_ids_degree": timed(lambda: deg_table.ids(nodes, eidx, eptr, ITERATIONS), args.calls)}
        if shape in base:
            r["host_loop"] = {"engine": base[shape]["engine"], "seconds": base[shape]["seconds"], "cpu_cores": 1}
            r["host_loop_over_wl_ids_x"] = base[shape]["seconds"] * 1e3 / r["wl_ids_x"]["median_ms"]
        if args.parent_lib:
            ugs_sampler._select_device(dev, jobs=True)
            this, parent = bind(LIB_PATH), bind(os.path.abspath(args.parent_lib))
            this.ugs_wl_hash_labeled.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_int64, C.c_void_p, C.c_void_p]
            keys, key_ids = deg_table._table()
            E, es = int(eidx.shape[1]), int(eidx.stride(0))
            outs = {n: (torch.empty((S, 2), dtype=torch.int64, device=dev), torch.empty((S,), dtype=torch.int32, device=dev),
                        torch.empty((S,), dtype=torch.int64, device=dev)) for n in ("this", "parent", "labeled")}

            def hash_of(L, name):
                d, s, _ = outs[name]
                assert L.ugs_wl_hash(nodes.data_ptr(), eidx.data_ptr(), es, E, eptr.data_ptr(), S, k, ITERATIONS, d.data_ptr(), s.data_ptr()) == 0

            def ids_of(L, name):
                d, s, o = outs[name]
                hash_of(L, name)
                assert L.ugs_wl_lookup(d.data_ptr(), s.data_ptr(), S, keys.data_ptr(), key_ids.data_ptr(), key_ids.numel(), len(deg_table), o.data_ptr()) == 0

            def labeled():
                d, s, _ = outs["labeled"]
                assert this.ugs_wl_hash_labeled(nodes.data_ptr(), eidx.data_ptr(), es, E, eptr.data_ptr(), S, k, ITERATIONS, labels.data_ptr(),
                                                labels.numel(), d.data_ptr(), s.data_ptr()) == 0

            ab = interleaved({"degree_ids_this": lambda: ids_of(this, "this"), "degree_ids_parent": lambda: ids_of(parent, "parent")}, args.calls)
            assert torch.equal(outs["this"][2], outs["parent"][2]) and torch.equal(outs["this"][0], outs["parent"][0]), "this commit and its parent disagree"
            kern = interleaved({"labeled_hash_this": labeled, "degree_hash_this": lambda: hash_of(this, "this"),
                                "degree_hash_parent": lambda: hash_of(parent, "parent")}, args.calls)
            assert torch.equal(outs["labeled"][0], digest)
            t, p = ab["degree_ids_this"]["wall"], ab["degree_ids_parent"]["wall"]
            ratio = kern["labeled_hash_this"]["events"]["median_ms"] / kern["degree_hash_parent"]["events"]["median_ms"]
            r["ab"] = dict(ab, **kern)
            r["condition_1_degree_median_within_parent_spread"] = {"this_median_ms": t["median_ms"], "parent_min_ms": p["min_ms"],
                                                                   "parent_max_ms": p["max_ms"], "holds": p["min_ms"] <= t["median_ms"] <= p["max_ms"]}
            r["condition_2_labeled_kernel_over_parent_degree_kernel"] = {"ratio": ratio, "bound": 1.10, "holds": ratio <= 1.10}
        results["shapes"][shape] = r
    line = json.dumps(results, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
