#!/usr/bin/env python3
"""Builds libugs_mi355.so (HIP kernels for gfx950 + host library behind the C ABI of include/ugs_mi355.h).
In-tree build: the .so lands next to this file and travels with the repo snapshot (it is git-ignored)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "libugs_mi355.so")
SRCS = [os.path.join(HERE, "ugs_kernels.hip"), os.path.join(HERE, "ugs_eps.hip"), os.path.join(HERE, "ugs_uniform.hip"), os.path.join(HERE, "ugs_rwr.hip"), os.path.join(HERE, "ugs_preproc.hip"), os.path.join(HERE, "ugs_collate.hip"), os.path.join(HERE, "ugs_batch.hip"), os.path.join(HERE, "ugs_host.cpp"),
        os.path.join(HERE, "ugs_jobs.cpp"), os.path.join(HERE, "ugs_side_eps.cpp"), os.path.join(HERE, "ugs_side_uniform.cpp"), os.path.join(HERE, "ugs_side_rwr.cpp"), os.path.join(HERE, "ugs_cache_common.cpp"), os.path.join(HERE, "ugs_rwr_cache.cpp"),
        os.path.join(HERE, "ugs_graph_cache.cpp"), os.path.join(HERE, "ugs_store.hip"), os.path.join(HERE, "ugs_eps_cache.cpp"),
        os.path.join(HERE, "ugs_apx.cpp"), os.path.join(HERE, "ugs_apx_gpu.hip"), os.path.join(HERE, "ugs_wl.hip"),
        os.path.join(HERE, "ugs_rows.hip"), os.path.join(HERE, "ugs_rows.cpp"),
        os.path.join(HERE, "ugs_graphlet.hip"), os.path.join(HERE, "ugs_graphlet.cpp"),
        os.path.join(HERE, "ugs_census_csr.hip"), os.path.join(HERE, "ugs_census_csr.cpp")]
HDRS = [os.path.join(HERE, "ugs_device.h"), os.path.join(HERE, "ugs_host_internal.h"), os.path.join(HERE, "ugs_apx_common.h"), os.path.join(HERE, "ugs_graphlet_common.h"), os.path.join(HERE, "ugs_census_csr.h"), os.path.join(HERE, "..", "..", "include", "ugs_mi355.h")]
DEPS = SRCS + HDRS
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(force=False, verbose=False):
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in DEPS):
        return OUT
    from concurrent.futures import ThreadPoolExecutor

    def compile_one(src):
        stem = os.path.splitext(src)[0]
        twins = sum(os.path.splitext(s)[0] == stem for s in SRCS) > 1       # ugs_rows.hip beside ugs_rows.cpp: one object each
        obj = (src if twins else stem) + ".o"
        if not force and os.path.exists(obj) and all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in [src, __file__] + HDRS):
            return obj                                       # object is newer than its source, the headers and this recipe
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
               "-x", "hip", "-c", src, "-o", obj]
        if src.endswith("ugs_kernels.hip"):
            # the walk kernel is bound by instruction issue: the ILP-first machine scheduler fills more of the wait slots behind
            # DPP and lane-mask hazards than the default occupancy-first one (C5 walk 5.45 -> 5.42 ms; same register counts)
            cmd[4:4] = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=4) as pool:          # the walk kernels take a minute: the other sources compile beside them
        objs = list(pool.map(compile_one, SRCS))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
