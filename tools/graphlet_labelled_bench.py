#!/usr/bin/env python3
"""Times ugs_sampler.graphlets.labelled_keys beside the labelled WL call it is exact for, on the shapes and by the method of
tools/graphlet_bench.py: device-resident rows of ugs_sampler.sample_batch (mode "sample", seed 42) for the three TU shapes and
ER k = 8, and 12 800 rows that are all K8, all C8 and all cubes.  Two label settings per shape:
  two_labels   one of 2 labels on every vertex of the batch, drawn at random (seed 42);
  onehot7      compact_labels(feature_labels(x)) of a 7-class one-hot float32 x, the class of every vertex drawn at random.
Per shape and setting, warm calls alternating call by call inside one process, device events around the whole call, medians with the
10th and 90th percentiles, of
  labelled_keys                 one launch;
  labelled_keys_orbits          the same with return_orbits;
  labelled_keys_lookup          labelled_keys + WLVocab.lookup in the vocabulary of the same rows: exact ids, two launches;
  wl_vocab_ids_labelled         WLVocab.ids(..., 3, node_labels=) in the vocabulary of the same rows: the reference's ids, two launches;
  class_ids                     the unlabelled exact ids, one launch.
and the number of distinct labelled keys beside that of distinct labelled WL digests.  WL never splits a labelled class, which is
asserted: every key has one digest.  The times cover whole calls; the kernels alone are not separated here.

    python tools/graphlet_labelled_bench.py --out profiles/graphlet_labelled.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ss-gnn_amd", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

SIDES = ("labelled_keys", "labelled_keys_orbits", "labelled_keys_lookup", "wl_vocab_ids_labelled", "class_ids")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--shapes", default=None, help="comma-separated subset of the seven shapes")
    args = ap.parse_args()
    import torch

    from graphlet_bench import ER, SEED, SHAPES
    from graphlet_orbit_bench import WORST, rows_of
    from ugs_sampler import graphlets, wl
    assert torch.cuda.is_available(), "graphlet_labelled_bench needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def label_settings(num_vertices):
        """{setting: (labels for labelled_keys, labels for the WL call)}: int64 [num_vertices] on the device, one partition each."""
        gen = torch.Generator().manual_seed(SEED)
        two = torch.randint(0, 2, (num_vertices,), generator=gen, dtype=torch.int64).to(dev)
        x = torch.nn.functional.one_hot(torch.randint(0, 7, (num_vertices,), generator=gen), 7).to(torch.float32).to(dev)
        raw = wl.feature_labels(x)
        alphabet = torch.unique(wl.feature_labels(torch.eye(7, dtype=torch.float32, device=dev)))     # the seven classes' own labels
        compact = graphlets.compact_labels(raw, alphabet)
        assert alphabet.numel() == 7 and int(compact.min()) >= 0 and int(compact.max()) <= 6
        return {"two_labels": (two, two), "onehot7": (compact, raw)}

    def timed(sides):
        ev = {s: [] for s in sides}
        for it in range(args.warmup + args.calls):
            for s, fn in sides.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    ev[s].append(a.elapsed_time(b))
        out = {}
        for s in sides:
            q = statistics.quantiles(ev[s], n=10)
            out[s] = {"median_ms_events": round(statistics.median(ev[s]), 4), "p10_ms_events": round(q[0], 4), "p90_ms_events": round(q[-1], 4),
                      "min_ms_events": round(min(ev[s]), 4), "max_ms_events": round(max(ev[s]), 4)}
        return out

    def measure(name):
        three, extra = rows_of(name, dev)
        k = three[0].size(1)
        num_vertices = extra["n"] * extra["graphs"] if "n" in extra else 8
        res = dict({"shape": name, "k": k, "rows": three[0].size(0), "edge_entries": three[1].size(1), "vertices": num_vertices,
                    "calls": args.calls}, **extra)
        for setting, (labels, wl_labels) in label_settings(num_vertices).items():
            key, status = graphlets.labelled_keys(*three, labels)
            digest, wl_status = wl.wl_hash(*three, 3, node_labels=wl_labels)
            assert not bool(status.any()) and not bool(wl_status.any())
            keys_vocab = wl.WLVocab(wl.extend_vocab({}, key, status), dev)
            wl_vocab = wl.WLVocab(wl.extend_vocab({}, digest, wl_status), dev)
            sides = {"labelled_keys": lambda: graphlets.labelled_keys(*three, labels),
                     "labelled_keys_orbits": lambda: graphlets.labelled_keys(*three, labels, return_orbits=True),
                     "labelled_keys_lookup": lambda: keys_vocab.lookup(*graphlets.labelled_keys(*three, labels)),
                     "wl_vocab_ids_labelled": lambda: wl_vocab.ids(*three, 3, node_labels=wl_labels),
                     "class_ids": lambda: graphlets.class_ids(*three)}
            ids, wl_ids = sides["labelled_keys_lookup"](), sides["wl_vocab_ids_labelled"]()
            assert int(ids.max()) < len(keys_vocab) and int(wl_ids.max()) < len(wl_vocab)
            pairs = torch.unique(torch.stack([ids, wl_ids]), dim=1)
            assert pairs.size(1) == len(keys_vocab), "a labelled class with two WL digests"
            orbit = sides["labelled_keys_orbits"]()[2]
            orbit = torch.where(orbit < k, orbit, torch.full_like(orbit, -1))    # k marks a slot without a vertex
            one = dict({"distinct_labelled_keys": len(keys_vocab), "distinct_labelled_wl_digests": len(wl_vocab),
                        "distinct_unlabelled_classes": int(torch.unique(sides["class_ids"]()).numel()),
                        "mean_orbits_per_row": round(float((orbit.max(dim=1).values + 1).double().mean()), 3)}, **timed(sides))
            med = {s: one[s]["median_ms_events"] for s in SIDES}
            one["wl_over_keys_lookup"] = round(med["wl_vocab_ids_labelled"] / med["labelled_keys_lookup"], 2)
            one["labelled_keys_over_class_ids"] = round(med["labelled_keys"] / med["class_ids"], 2)
            one["orbits_over_labelled_keys"] = round(med["labelled_keys_orbits"] / med["labelled_keys"], 2)
            res[setting] = one
        print(json.dumps(res), flush=True)
        return res

    names = [s[0] for s in SHAPES] + ["er_k8"] + list(WORST)
    if args.shapes:
        names = [x for x in names if x in args.shapes.split(",")]
    results = [measure(name) for name in names]
    doc = {"tool": "tools/graphlet_labelled_bench.py", "device": torch.cuda.get_device_name(0), "sampler": "ugs_sampler.sample_batch", "seed": SEED,
           "er": {"n": ER[0], "columns": ER[1]},
           "note": "times cover the whole call on device-resident rows: one launch for labelled_keys (with or without orbits) and for "
           "class_ids, two for labelled_keys + lookup and for WLVocab.ids; the kernels alone were not separated by a kernel-level run, "
           "and the effect on a training step's time is not measured here", "shapes": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
