#!/usr/bin/env python3
"""What a drop-in call on COCO-SP-shaped graphs (c6: 32 graphs of 477 vertices and 2694 columns, k = 8, m = 100) costs with the
device batch pass's column limit at its default (1000: such a batch takes the general host path) and raised to 8192
(ugs_sampler.set_batch_pass_max_cols: slicing, strided keys, fingerprints, CSR and root records on the device).

Three legs, each with host-visible and device outputs, the two settings taking turns call by call (a drift of the box or of the
allocator cannot favour one of them), every call timed on its own:
  warm      the same batch again (whole-batch index);
  new_comb  a new combination of graphs the LRU knows (a permutation of the warm batch's graphs: the trainer's shuffled epoch
            while the dataset fits the LRU);
  all_miss  32 graphs never seen before (COCO-SP has 123 k graphs against an LRU of 1000: every training batch), clear_cache()
            outside the timed region.
A library without the setter (an older build) is measured at limit 1000 only.  Medians, min-to-max spreads and the
batch_pass_stats deltas go to profiles/large_graph_pass.json under --tag.

    python tools/large_graph_pass_probe.py --tag this_change [--calls 40] [--limits 1000,8192] [--out profiles/large_graph_pass.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ss-gnn_amd"))
import ugs_sampler  # noqa: E402
import ugs_workloads as wl  # noqa: E402

N, E_UND, K, G, M = wl.TU_SHAPES.get("c6_cocosp_b3200", (477, 1347, 8, 32, 100))
HAS_SETTER = hasattr(ugs_sampler, "set_batch_pass_max_cols")
LIMITS = (1000, 8192) if HAS_SETTER else (1000,)          # (--limits 1000: one setting alone, nothing in between its calls)


def set_limit(limit):
    if HAS_SETTER:
        ugs_sampler.set_batch_pass_max_cols(limit)


def summary(ts):
    v = sorted(ts)
    return dict(calls=len(v), median_ms=round(v[len(v) // 2] * 1e3, 4), min_ms=round(v[0] * 1e3, 4), max_ms=round(v[-1] * 1e3, 4),
                spread_ms=round((v[-1] - v[0]) * 1e3, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--calls", type=int, default=40, help="timed calls per setting and leg (after 4 untimed ones)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_graph_pass.json"))
    ap.add_argument("--limits", default=None, help="comma-separated limits taking turns (default: 1000,8192 where the setter exists)")
    a = ap.parse_args()
    global LIMITS
    if a.limits and HAS_SETTER:
        LIMITS = tuple(int(x) for x in a.limits.split(","))
    dev = torch.device("cuda:0")
    os.environ["UGS_DEVICE_BATCH"] = "1"                     # the pass wherever it applies: the default mode's pause cannot interfere
    cols = 2 * E_UND
    ei, ptr = wl.tu_batch(N, E_UND, G)
    ptr_t = torch.from_numpy(ptr)
    rng = np.random.default_rng(1)
    fresh_at = [10_000]

    def warm_batch():
        return torch.from_numpy(ei)

    def new_comb():
        perm = rng.permutation(G)
        return torch.from_numpy(np.ascontiguousarray(np.concatenate(
            [ei[:, g * cols:(g + 1) * cols] - g * N + i * N for i, g in enumerate(perm)], axis=1)))

    def all_miss():
        fresh_at[0] += G
        return torch.from_numpy(wl.tu_batch(N, E_UND, G, first_graph=fresh_at[0])[0])

    legs = {"warm": (warm_batch, False), "new_comb": (new_comb, False), "all_miss": (all_miss, True)}
    result = dict(tag=a.tag, device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, has_setter=HAS_SETTER,
                  shape=dict(n=N, columns=cols, k=K, graphs=G, m=M), legs={})
    for leg, (make, clear) in legs.items():
        for out_tag, kw in (("host", {}), ("dev", {"device": dev})):
            ts = {lim: [] for lim in LIMITS}
            stats = {lim: [0, 0] for lim in LIMITS}
            ugs_sampler.clear_cache()
            for lim in LIMITS:                               # every graph of the warm batch known, under both settings
                set_limit(lim)
                ugs_sampler.sample_batch(torch.from_numpy(ei), ptr_t, M, K, mode="sample", seed=42, **kw)
            for it in range((a.calls + 4) * len(LIMITS)):
                lim = LIMITS[it % len(LIMITS)]
                set_limit(lim)
                e = make()
                if clear:
                    ugs_sampler.clear_cache()
                torch.cuda.synchronize()
                s0 = ugs_sampler.batch_pass_stats()
                t = time.perf_counter()
                o = ugs_sampler.sample_batch(e, ptr_t, M, K, mode="sample", seed=42, **kw)
                if kw:
                    torch.cuda.synchronize()
                dt = time.perf_counter() - t
                s1 = ugs_sampler.batch_pass_stats()
                del o
                if it >= 4 * len(LIMITS):
                    ts[lim].append(dt)
                    stats[lim][0] += s1["device_plans"] - s0["device_plans"]
                    stats[lim][1] += s1["general_path"] - s0["general_path"]
            for lim in LIMITS:
                rec = summary(ts[lim])
                rec.update(device_plans=stats[lim][0], general_path=stats[lim][1])
                result["legs"].setdefault(leg, {}).setdefault(out_tag, {})[f"limit_{lim}"] = rec
                print(f"{a.tag} {leg:9s} {out_tag:4s} limit {lim}: median {rec['median_ms']:.3f} ms  min {rec['min_ms']:.3f}  max {rec['max_ms']:.3f}  "
                      f"device_plans +{rec['device_plans']} general_path +{rec['general_path']}", flush=True)
    set_limit(1000)
    ugs_sampler.clear_cache()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.tag] = result
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
