#!/usr/bin/env python3
"""Times ugs_sampler.wl.WLVocab.ids on device-resident sampler outputs against the host loop it replaces.

Shapes: the PROTEINS-shaped batch (c3: 8192 rows, k = 6) and the COCO-SP-shaped one (c6: 3200 rows, k = 8), iterations 3.
  * GPU: median of --calls calls of WLVocab.ids after warm-up, each ended by a device synchronise; beside it the `ugs` sampling
    step that produces the tensors (Plan.step on the resident plan, same protocol), so a reader sees which of the two costs more.
  * baseline: the reference's host path on the same tensors on one CPU core -- per row three .item() reads, a networkx.Graph with
    str(degree) attributes, weisfeiler_lehman_graph_hash and a dict lookup (src/gps/gps/models/ss_gnn_wl.py:210-247) -- if networkx
    can be imported, otherwise the same loop over tests/wl_law.py, labelled as such.  It runs in a child process that is started
    and finished before this process makes its first GPU call; the child gets its rows from the CPU oracle, which is bit-exact
    with the GPU sampler, and the parent checks that both hashed the same tensors (ids compared).

    python tools/wl_bench.py --out profiles/wl_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/wl_bench.py --no-baseline --calls 20   # kernel times, a run of its own
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ss-gnn_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

SHAPES = ("c3_proteins_b8192", "c6_cocosp_b3200")
ITERATIONS, SEED = 3, 42


def baseline_child(shape):
    """One CPU core: rows from the CPU oracle, then the per-row host loop.  Prints one JSON line."""
    import numpy as np
    import torch
    torch.set_num_threads(1)
    import oracle
    import ugs_workloads as workloads
    import wl_law
    ei, ptr, m, k = workloads.workload(shape)
    nodes, eidx, eptr = (torch.from_numpy(np.ascontiguousarray(a)) for a in oracle.sample_batch(ei, ptr, m, k, "sample", SEED)[:3])
    try:
        import networkx as nx
        engine = "networkx " + nx.__version__

        def row_hash(edges, n):
            G = nx.Graph()
            G.add_nodes_from(range(n))
            if edges.numel() > 0:
                G.add_edges_from(edges.t().numpy())
            for u in range(n):
                G.nodes[u]["attr"] = str(G.degree(u))
            return nx.weisfeiler_lehman_graph_hash(G, node_attr="attr", iterations=ITERATIONS)
    except ImportError:
        engine = "tests/wl_law.py (networkx is not installed)"

        def row_hash(edges, n):
            return wl_law.wl_row(list(range(n)), edges[0].tolist(), edges[1].tolist(), ITERATIONS)[0]

    def ids_of(vocab):
        out = []
        for i in range(nodes.shape[0]):
            n = (nodes[i] >= 0).sum().item()
            edges = eidx[:, eptr[i].item():eptr[i + 1].item()]
            out.append(len(vocab) if n == 0 else vocab.get(row_hash(edges, n), len(vocab)))
        return out

    hexes, stats, _ = wl_law.wl_rows(nodes.numpy(), eidx.numpy(), eptr.numpy(), ITERATIONS)
    vocab = {}
    for h in hexes[:len(hexes) // 2]:
        if h is not None and h not in vocab:
            vocab[h] = len(vocab)
    t0 = time.perf_counter()
    ids = ids_of(vocab)
    dt = time.perf_counter() - t0
    assert ids == wl_law.ids_from(hexes, stats, vocab), "the host loop and the law disagree"
    print(json.dumps({"shape": shape, "engine": engine, "rows": len(ids), "k": k, "seconds": dt, "vocab": list(vocab), "ids": ids}))


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
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.baseline_child:
        return baseline_child(args.baseline_child)

    base = {}
    if not args.no_baseline:                           # before the first GPU call of this process, one shape after the other
        env = dict(os.environ, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
        for shape in SHAPES:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-child", shape], env=env, check=True,
                                 capture_output=True, text=True).stdout
            base[shape] = json.loads(out.strip().splitlines()[-1])

    import torch
    import ugs_sampler
    import ugs_workloads as workloads
    import wl_law
    from ugs_sampler import wl
    dev = "cuda:0"
    results = {"device": torch.cuda.get_device_name(0), "iterations": ITERATIONS, "shapes": {}}
    for shape in SHAPES:
        ei, ptr, m, k = workloads.workload(shape)
        ei_t, ptr_t = torch.from_numpy(ei), torch.from_numpy(ptr)
        nodes, eidx, eptr = ugs_sampler.sample_batch(ei_t, ptr_t, m, k, mode="sample", seed=SEED, device=dev)[:3]
        if shape in base:
            vocab = {h: i for i, h in enumerate(base[shape]["vocab"])}
        else:
            vocab = wl.extend_vocab({}, *wl.wl_hash(nodes[:nodes.shape[0] // 2], eidx, eptr[:nodes.shape[0] // 2 + 1], ITERATIONS))
        table = wl.WLVocab(vocab, dev)
        ids = table.ids(nodes, eidx, eptr, ITERATIONS)
        if shape in base:
            assert ids.cpu().tolist() == base[shape]["ids"], "GPU ids differ from the host loop's"
        else:
            hexes, stats, _ = wl_law.wl_rows(nodes[:64].cpu().numpy(), eidx.cpu().numpy(), eptr[:65].cpu().numpy(), ITERATIONS)
            assert ids[:64].cpu().tolist() == wl_law.ids_from(hexes, stats, vocab), "GPU ids differ from the law's"
        plan = ugs_sampler.Plan.from_batch(ei_t, ptr_t, k, device=dev)
        seeds = iter(range(1000, 1000000))
        r = {"rows": int(nodes.shape[0]), "k": k, "edge_entries": int(eidx.shape[1]), "vocab": len(vocab),
             "unknown_rows": int((ids == len(vocab)).sum()),
             "wl_ids": timed(lambda: table.ids(nodes, eidx, eptr, ITERATIONS), args.calls),
             "wl_hash_only": timed(lambda: wl.wl_hash(nodes, eidx, eptr, ITERATIONS), args.calls),
             "ugs_plan_step": timed(lambda: plan.step(m, mode="sample", seed=next(seeds)), args.calls),
             "ugs_sample_batch_device": timed(lambda: ugs_sampler.sample_batch(ei_t, ptr_t, m, k, mode="sample", seed=next(seeds), device=dev), args.calls)}
        if shape in base:
            r["host_loop"] = {"engine": base[shape]["engine"], "seconds": base[shape]["seconds"], "cpu_cores": 1}
            r["host_loop_over_wl_ids"] = base[shape]["seconds"] * 1e3 / r["wl_ids"]["median_ms"]
        results["shapes"][shape] = r
        plan.close()
    line = json.dumps(results, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
