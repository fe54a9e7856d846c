"""rwr_row_paths.py -- the inputs that pin the paths of rwr_sampler's streams="row" kernel (ugs_rwr.hip, rwr_row_walks), shared
by the CPU tests (tests/test_rwr_row_law.py: the census) and the GPU tests (tests/test_gpu_rwr_rows.py).  The graphs are those of
tests/rwr_paths.py where they fit; every case names in `reaches` the classes of rwr_row_law.census it is there for, and both test
files assert them, so an input that stops reaching its path fails instead of losing coverage.  Seeds marked "found" come from
running the census over candidate seeds.  Every graph keeps T = 10 n k below 10^5 (the census asserts it)."""
import functools

import numpy as np

import rwr_paths as P
import rwr_row_law as RR
import ugs_workloads as wl

Case = P.Case
LANES = RR.ROW_LANES


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, batch, m, k, seed, p, reaches, seeds=None):
        out.append(Case(name, batch[0], batch[1], m, k, seed, p, seeds, tuple(reaches)))

    def of(name):
        c = P.case(name)
        return c.ei, c.ptr

    # CSR placement: the graphs of rwr_paths' placement cases at k = 4 (T = 80 120); the dynamic LDS is sized by the graph at the bound
    classes = ["csr_words == 8192", "csr_words == 8193", "lds, vbase > 0", "global, vbase > 0"]
    add("placement", of("placement"), 20, 4, 5, 0.2, classes)
    add("placement_graph_seeds", of("placement"), 20, 4, 0, 0.2, classes, seeds=(11, (1 << 64) - 1, 1 << 63, 7))
    add("placement_last_vertex", of("placement_last_vertex"), 20, 4, 3, 0.2, ["csr_words == 8193", "global", "lds, vbase > 0"])
    # KM dispatch: k = KM, k = KM - 1 and k = KM / 2 + 1 on the km_k* graphs
    for K in (8, 16, 32, 64):
        add(f"km_k{K}", of(f"km_k{K}"), 3, K, K, 0.1, [f"KM == {K}", "k == KM", "T0", "found"])
        add(f"km_k{K}_minus_1", of(f"km_k{K}"), 3, K - 1, K, 0.1, [f"KM == {K}", "found"])
    for k in (9, 17, 33):
        add(f"km_k{k}", of(f"km_k{k}"), 3, k, k, 0.1, [f"KM == {2 * (k - 1)}", "T0", "found"])
    # seed-doomed rows: first row, last row, twice in a row, live rows of the same graph around them
    around = ["doomed_row0", "doomed_row_last", "doomed_twice", "live after doomed", "doomed after live", "found"]
    add("components_k9", of("components_k9"), 8, 9, COMPONENTS_SEED, 0.0, around)
    add("doomed91", of("doomed91_s3"), 48, 5, 3, 0.2, ["doomed_row0", "doomed_row_last", "doomed_twice"])
    add("mixed20", of("mixed20_s1451"), 16, 5, MIXED_SEED, 0.2, around)
    # n < k and n = 0 between live graphs
    live = lambda s: P.tu(10, 12, s)
    add("T0", P.batch_of([live(1), (0, [[], []]), live(2), (3, [[0, 1], [1, 2]]), (0, [[], []]), live(3)], first=5), 5, 4, 2, 0.2,
        ["T0", "n == 0", "found", "lds, vbase > 0"])
    # p = 1: the shortcut (k > 1) and k = 1; p just below 1: live walks that run all T iterations; p = 0; walks of more than 64 draws
    add("p1_live", of("p1_live"), 20, 4, 9, 1.0, ["p1_shortcut"])
    add("k1_p1", of("k1_p1.0"), 2100, 1, 6, 1.0, ["L == 1", "workgroups per graph > 1"])
    add("p099_live", of("p1_live"), 20, 4, 9, 0.99, ["ran all T", "live_failed"])
    add("p0_live", of("p0_live"), 10, 5, 2, 0.0, ["found"])
    add("cap_s8", of("cap_s8_m24"), 24, 8, 8, 0.5, ["L > 64", "found"])
    add("cap_s10", of("cap_s10_m16"), 16, 8, 10, 0.5, ["L > 64", "found"])
    # rows against workgroups
    add("m1", wl.tu_batch(10, 12, 3, dataset_seed=5), 1, 4, 1, 0.2, ["idle lanes", "found"])
    add("m7_g40", of("rows_across_blocks"), 7, 4, 12, 0.2, ["found"])
    add("m300", P.batch_of([P.tu(12, 14, 5)]), 300, 5, 4, 0.2, ["workgroups per graph > 1", "short last workgroup"])
    for m in (LANES - 1, LANES, LANES + 1, 2 * LANES):
        add(f"m{m}", wl.tu_batch(10, 12, 2, dataset_seed=6), m, 4, 3, 0.2, ["found"] + (["workgroups per graph > 1"] if m > LANES else []))
    add("tree_tail", P.batch_of([P.tu(30, 29, 8), P.tu(30, 29, 9)]), 200, 8, TAIL_SEED, 0.2, ["long tail", "workgroups per graph > 1", "L > 64"])
    # nothing to do
    add("m0", wl.tu_batch(10, 12, 3, dataset_seed=5), 0, 4, 1, 0.2, [])
    add("G0", (np.zeros((2, 0), np.int64), np.array([4], np.int64)), 5, 4, 1, 0.2, [])
    # per-graph seeds, unequal
    add("graph_seeds", wl.tu_batch(12, 14, 5, dataset_seed=7), 9, 4, 0, 0.2, ["found"], seeds=(5, 5, (1 << 64) - 2, 0, 1 << 40))
    return tuple(out)


COMPONENTS_SEED = 1     # found: the first seed from 0 whose census holds the case's classes
MIXED_SEED = 354
TAIL_SEED = 0


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def census_of(name):
    c = case(name)
    return RR.census(c.ei, c.ptr, c.m, c.k, c.seed, c.p, c.seeds)


@functools.lru_cache(maxsize=None)
def law_of(name, mode):
    """rwr_row_law.sample_batch of the case: computed once, shared, never modified (the arrays are read-only)."""
    c = case(name)
    out = RR.sample_batch(c.ei, c.ptr, c.m, c.k, mode, c.seed, c.p, c.seeds)
    for a in out:
        a.setflags(write=False)
    return out
