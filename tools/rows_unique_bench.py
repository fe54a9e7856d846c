#!/usr/bin/env python3
"""Times ugs_sampler.rows.unique_rows on device-resident rwr_sampler outputs against the torch formulation of the same result.

Shapes: 128-graph batches sampled by rwr_sampler (seed 42, p_restart 0.2, mode "sample", device outputs):
  MUTAG-like     tu_batch(18, 20, 128), k = 6, m = 100
  QM9-like       tu_batch(18, 19, 128), k = 5, m = 100
  PROTEINS-like  tu_batch(39, 73, 128), k = 6, m = 64
Per shape: the kept fraction (by="set"), and the median time of a warm call of each side -- device events recorded on torch's
current stream around the whole call (begin, the read-back of U and Eu, finish), and beside it a host clock around the call ended by
a device synchronise.  The two sides alternate call by call inside one process.  The torch side: a sort along k, torch.unique(dim=0,
return_inverse=True) on the rows prefixed with their graph id, the first row of every class by scatter_reduce(amin), and the gathers
that rebuild nodes, edge_ptr, edge_index and edge_src.  Its rows come out in torch.unique's sorted order inside a graph, not in
first-occurrence order; the bench checks that both sides keep the same rows (as sets per graph) with the same counts.

    python tools/rows_unique_bench.py --out profiles/rows_unique.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ss-gnn_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

SHAPES = (("mutag_like", 18, 20, 6, 100), ("qm9_like", 18, 19, 5, 100), ("proteins_like", 39, 73, 6, 64))
GRAPHS, SEED, P_RESTART = 128, 42, 0.2


def torch_unique_rows(nodes, ei, eptr, sptr, esrc):
    import torch
    R, k = nodes.shape
    G = sptr.numel() - 1
    dev = nodes.device
    ar = lambda n: torch.arange(n, dtype=torch.int64, device=dev)      # noqa: E731
    gid = torch.repeat_interleave(ar(G), sptr[1:] - sptr[:-1], output_size=R)
    keyed = torch.cat([gid.unsqueeze(1), nodes.sort(dim=1).values], dim=1)
    uniq, inverse = torch.unique(keyed, dim=0, return_inverse=True)     # (synchronises: U)
    U = uniq.size(0)
    count = torch.bincount(inverse, minlength=U)
    first = torch.full((U,), R, dtype=torch.int64, device=dev).scatter_reduce(0, inverse, ar(R), "amin")
    lens = (eptr[1:] - eptr[:-1]).index_select(0, first)
    eptr_u = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    eptr_u[1:] = torch.cumsum(lens, 0)
    Eu = int(eptr_u[-1])                                                # (synchronises: Eu)
    seg = torch.repeat_interleave(ar(U), lens, output_size=Eu)
    pos = eptr.index_select(0, first).index_select(0, seg) + ar(Eu) - eptr_u.index_select(0, seg)
    sptr_u = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    sptr_u[1:] = torch.cumsum(torch.bincount(uniq[:, 0], minlength=G), 0)
    return nodes.index_select(0, first), ei.index_select(1, pos), eptr_u, sptr_u, esrc.index_select(0, pos), count, inverse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    import torch

    import rwr_sampler
    import ugs_workloads as wl
    from ugs_sampler import rows
    assert torch.cuda.is_available(), "rows_unique_bench needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    results = []
    for name, n, e, k, m in SHAPES:
        ei, ptr = wl.tu_batch(n, e, GRAPHS)
        ptr_t = torch.from_numpy(ptr)
        five = rwr_sampler.sample_batch(torch.from_numpy(ei).to(dev), ptr_t, m, k, mode="sample", seed=SEED, p_restart=P_RESTART)
        ptr_d = ptr_t.to(dev)
        sides = {"unique_rows": lambda: rows.unique_rows(*five, ptr=ptr_d, by="set"), "torch": lambda: torch_unique_rows(*five)}
        ours, theirs = sides["unique_rows"](), sides["torch"]()
        form = rows.last_launch()
        # the same rows kept, with the same counts: compare per graph as sorted (sorted row, count) lists
        def canon(u):
            keyed = torch.cat([torch.repeat_interleave(torch.arange(GRAPHS, device=dev), u[3][1:] - u[3][:-1]).unsqueeze(1),
                               u[0].sort(dim=1).values, u[5].unsqueeze(1)], dim=1)
            return torch.unique(keyed, dim=0)
        assert torch.equal(canon(ours), canon(theirs)), "the two sides disagree"
        assert torch.equal(ours[3], theirs[3]) and int(ours[2][-1]) == int(theirs[2][-1])
        ev = {s: [] for s in sides}
        host = {s: [] for s in sides}
        for it in range(args.warmup + args.calls):
            for s, fn in sides.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if it >= args.warmup:
                    ev[s].append(a.elapsed_time(b))
                    host[s].append((t1 - t0) * 1e3)
        R, U = five[0].size(0), ours.nodes.size(0)
        res = {"shape": name, "n": n, "undirected_edges": e, "graphs": GRAPHS, "k": k, "m": m, "rows": R, "edge_entries": five[1].size(1),
               "kept_rows": U, "kept_fraction": round(U / R, 4), "kept_edge_entries": ours.edge_index.size(1), "dedup_form": form, "calls": args.calls}
        for s in sides:
            q = statistics.quantiles(ev[s], n=10)
            res[s] = {"median_ms_events": round(statistics.median(ev[s]), 4), "p10_ms_events": round(q[0], 4), "p90_ms_events": round(q[-1], 4),
                      "median_ms_host_clock": round(statistics.median(host[s]), 4)}
        res["torch_over_unique_rows"] = round(res["torch"]["median_ms_events"] / res["unique_rows"]["median_ms_events"], 2)
        results.append(res)
        print(json.dumps(res), flush=True)
    doc = {"tool": "tools/rows_unique_bench.py", "device": torch.cuda.get_device_name(0), "by": "set", "sampler": "rwr_sampler", "seed": SEED,
           "p_restart": P_RESTART, "note": "times cover the whole call, read-backs included; the encoder-side saving is the kept fraction and "
           "its effect on a training step's time is not measured here", "shapes": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
