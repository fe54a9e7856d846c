"""CPU (no GPU needed): the law of uniform_sampler.sample_distinct (tests/uniform_distinct_law.py restates it from
include/ugs_mi355.h), the model of uni_draw_distinct's parallel resolution against it, its uniformity, a census showing that the
batches the GPU test samples reach every class of the resolution and tell every one-line mutant of it apart, and the argument
refusals, which all come before any device work."""
import ctypes
import os
import random
import re
from itertools import permutations

import numpy as np
import pytest
import torch

import uniform_distinct_law as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = "no usable HIP device"
PAIRS = [(2, 1), (3, 2), (5, 2), (5, 4), (7, 3), (16, 2), (37, 1)]
Z_BOUND = 4.0


# ---- law and model ----
def test_mix_is_splitmix64s_finaliser():
    # SplitMix64 seeded with 0: its first outputs are mix(gamma), mix(2 gamma) (Steele, Lea & Flood 2014; the published test vector)
    assert D.mix(D.GAMMA) == 0xE220A8397B1DCDAF and D.mix(2 * D.GAMMA) == 0x6E789E6AA1B965F4


def test_the_model_equals_the_law_on_random_cases():
    rng = random.Random(1)
    for _ in range(4000):
        N, m, s = rng.randint(-1, 40), rng.randint(0, 45), rng.getrandbits(64)
        assert D.model(s, N, m) == D.law(s, N, m), (N, m, s)


@pytest.mark.parametrize("N,m", [(300, 299), (4097, 4096), (1312, 100), (8008, 4096), (1, 1), (1, 0), (1, 4), (9, 0), (9, 9), (9, 12), (0, 3), (-1, 3)])
def test_the_model_equals_the_law_at_the_edges(N, m):
    for s in (0, 1, 42, D.M64):
        rows = D.law(s, N, m)
        assert D.model(s, N, m) == rows, (N, m, s)
        assert len(rows) == m
        live = [r for r in rows if r >= 0]
        assert len(live) == min(m, max(N, 0)) and len(set(live)) == len(live) and all(0 <= r < N for r in live)
        assert rows[len(live):] == [-1] * (m - len(live))
        if m >= N:
            assert live == list(range(max(N, 0)))


def test_a_smaller_m_gives_a_prefix():
    for s in range(50):
        assert D.law(s, 40, 17) == D.law(s, 40, 39)[:17]


# ---- uniformity ----
def z_of(counts, total):
    exp = total / len(counts)
    chi2 = sum((c - exp) ** 2 / exp for c in counts)
    df = len(counts) - 1
    return (chi2 - df) / (2 * df) ** 0.5


@pytest.mark.parametrize("N,m", PAIRS)
def test_every_ordered_selection_is_equally_likely(N, m):
    """chi-square over all ordered outcomes, seeds 0 ... 19 999, z = (chi2 - df) / sqrt(2 df).  Measured for the law: -1.34 ... +1.52
    over the seven pairs; a 4- or 6-round Feistel permutation with cycle walking gives z = 15 at (5, 2) and 40 at (5, 5)."""
    counts = {p: 0 for p in permutations(range(N), m)}
    for s in range(20000):
        counts[tuple(D.model(s, N, m))] += 1
    z = z_of(list(counts.values()), 20000)
    print(f"(N, m) = ({N}, {m}): z = {z:+.2f}")
    assert abs(z) <= Z_BOUND


def test_graphs_that_share_an_integer_seed_are_independent():
    """one integer s means seeds s + g: the first rows of graphs 0 and 1 (seeds s and s + 1) at (5, 2), a 5 x 5 table over
    s = 0 ... 19 999, chi-square of independence with 16 degrees of freedom.  Measured with this statistic: z = +1.79."""
    table = np.zeros((5, 5))
    for s in range(20000):
        table[D.law(s, 5, 2)[0], D.law(s + 1, 5, 2)[0]] += 1
    exp = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / table.sum()
    chi2 = float(((table - exp) ** 2 / exp).sum())
    z = (chi2 - 16) / 32 ** 0.5
    print(f"independence: z = {z:+.2f}")
    assert abs(z) <= Z_BOUND


# ---- census of the GPU test's inputs ----
def gpu_inputs():
    for name in D.GPU_CASES:
        k, m, _, _, sizes, seeds, _, _ = D.case_batch(name)
        yield name, sizes, seeds, m


def test_the_gpu_cases_reach_every_class_of_the_resolution():
    reached = {}
    for name, sizes, seeds, m in gpu_inputs():
        assert m <= D.MAX_M
        for c in D.census(sizes, seeds, m):
            reached.setdefault(c, name)
    assert set(reached) == set(D.CLASSES), sorted(set(D.CLASSES) - set(reached))


@pytest.mark.parametrize("mutant", sorted(D.MUTANTS))
def test_every_mutant_differs_from_the_law_on_a_gpu_case(mutant):
    differs = [name for name, sizes, seeds, m in gpu_inputs()
               if any(D.model(s, N, m, **D.MUTANTS[mutant]) != D.law(s, N, m) for N, s in zip(sizes, seeds))]
    assert differs, mutant


def test_the_closed_forms_are_the_population_sizes():
    import uniform_law as U
    for kind, n, k in (("path", 8, 3), ("cycle", 7, 3), ("cycle", 5, 3), ("complete", 6, 3), ("path", 3, 3), ("path", 2, 3), ("cycle", 9, 4)):
        _, ei = D.BUILD[kind](n)
        adj = U.graph_adjacency(ei[0], ei[1], 0, n)
        assert len(U.esu_masks(adj, k)) == D.closed_form(kind, n, k), (kind, n, k)


# ---- arguments: every refusal comes before the library looks for a device ----
def us():
    import uniform_sampler
    return uniform_sampler


EI = torch.tensor([[0, 1, 2, 3, 4], [1, 2, 0, 4, 3]], dtype=torch.int64)
PTR = torch.tensor([0, 3, 5], dtype=torch.int64)


def expect(want, fn, *args, **kw):
    if want == DEVICE and torch.cuda.is_available():
        assert len(fn(*args, **kw)) == 7
        return
    with pytest.raises(RuntimeError, match=want):
        fn(*args, **kw)


def pop_with_graphs():
    pop = us().PopulationCache(2, "cuda:0")
    pop._slot[0], pop._slot[1] = (0, 3), (1, 2)                     # what add records on the host, without the device call
    return pop


def test_the_functions_exist_through_every_layer():
    assert "sample_distinct" in us().__all__ and callable(us().PopulationCache.sample_distinct) and us().DISTINCT_MAX_M == D.MAX_M
    hdr = open(os.path.join(ROOT, "include", "ugs_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    import ugs_sampler
    lib = ctypes.CDLL(os.path.join(ROOT, "ss-gnn_amd", "csrc", "libugs_mi355.so"))
    for name in ("ugs_uniform_distinct_begin", "ugs_uniform_population_distinct_begin"):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m and "const uint64_t *seeds" in m.group(1) and "int64_t *valid_out" in m.group(1) and "int32_t *graph_status" in m.group(1)
        assert hasattr(lib, name) and name in ugs_sampler._lib.EXPORTS
    for words in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15", "Fisher-Yates", "2^-39", "m_per_graph <= 4096"):
        assert words in hdr, words


def test_refusals_of_the_uncached_call():
    f = us().sample_distinct
    expect(DEVICE, f, EI, PTR, 2, 2, [1, 2])
    expect(DEVICE, f, EI, PTR, 4096, 2, 7)
    expect(r"sample_distinct: m_per_graph must be <= 4096 \(got 4097\)", f, EI, PTR, 4097, 2, [1, 2])
    expect(r"m_per_graph must be >= 0", f, EI, PTR, -1, 2, [1, 2])
    expect(r"m_per_graph must be >= 0", f, EI, PTR, -1, -1, [1, 2])
    expect(r"k must be >= 0", f, EI, PTR, 2, -1, [1, 2])
    expect(r"seeds must hold one seed per graph \(2\), got 1", f, EI, PTR, 2, 2, [1])
    expect(r"ptr must be non-decreasing \(graph 1\)", f, EI, torch.tensor([0, 3, 2]), 2, 2, [1, 2])
    expect(r"bad arguments to sample_distinct", f, EI, torch.tensor([], dtype=torch.int64), 2, 2, [])
    expect(r"edge_index must be int64", f, EI.to(torch.int32), PTR, 2, 2, [1, 2])
    expect(r"edge_index must have shape \[2, E\]", f, EI.t().contiguous(), PTR, 2, 2, [1, 2])
    expect(r"graph 1 has 67 vertices; graphs of more than 64 vertices", lambda: us().sample_batch(EI, torch.tensor([0, 3, 70]), 2, 2))
    expect(DEVICE, f, EI, torch.tensor([0, 3, 70]), 2, 2, [1, 2])   # in a per-graph call such a graph fails alone


def test_refusals_of_the_cached_call():
    pop = pop_with_graphs()
    f = pop.sample_distinct
    expect(r"sample_distinct: m_per_graph must be <= 4096 \(got 5000\)", f, [0, 1], PTR, EI, 5000, [1, 2])
    expect(r"m_per_graph must be >= 0", f, [0, 1], PTR, EI, -1, [1, 2])
    expect(r"seeds must hold one seed per graph \(2\), got 3", f, [0, 1], PTR, EI, 2, [1, 2, 3])
    expect(r"edge_index must be int64", f, [0, 1], PTR, EI.to(torch.int32), 2, 5)
    expect(r"graph 1 of the batch has 3 vertices.* 2$", f, [0, 1], torch.tensor([0, 3, 6]), EI, 2, 5)
    expect(r"unknown population slot 0", f, [0, 1], PTR, EI, 2, 5)  # the slots were never added to the library's population
    with pytest.raises(KeyError):
        f([0, 7], PTR, EI, 2, 5)
    with pytest.raises(ValueError, match="graph_idx"):
        f([0], PTR, EI, 2, 5)
    pop.close()


def test_the_c_abi_checks_its_own_arguments_first():
    import ugs_sampler
    lib, bad_arg, unsupported = ugs_sampler._lib.lib, ugs_sampler._lib.UGS_E_BAD_ARG, -7       # UGS_E_UNSUPPORTED
    job, total = ctypes.c_void_p(), ctypes.c_int64()
    seeds, st, valid = (ctypes.c_uint64 * 2)(1, 2), (ctypes.c_int32 * 2)(), (ctypes.c_int64 * 2)()
    args = (EI.data_ptr(), EI.stride(0), EI.size(1), PTR.data_ptr(), 2)
    out = (ctypes.byref(job), ctypes.byref(total))
    assert lib.ugs_uniform_distinct_begin(*args, 4097, 2, 0, seeds, st, valid, *out) == unsupported and b"4096" in lib.ugs_last_error()
    assert lib.ugs_uniform_distinct_begin(*args, 4, 2, 0, seeds, st, None, *out) == bad_arg and b"valid" in lib.ugs_last_error()
    assert lib.ugs_uniform_distinct_begin(*args, 4, 2, 0, None, st, valid, *out) == bad_arg
    pop = ctypes.c_void_p()
    assert lib.ugs_uniform_population_create(2, 64, ctypes.byref(pop)) == 0
    slots = (ctypes.c_int64 * 2)(0, 1)
    assert lib.ugs_uniform_population_distinct_begin(pop, slots, *args, 4097, 0, seeds, 1, st, valid, *out) == unsupported
    assert lib.ugs_uniform_population_distinct_begin(pop, slots, *args, 4, 0, seeds, 1, st, None, *out) == bad_arg
    assert lib.ugs_uniform_population_distinct_begin(pop, slots, *args, 4, 0, seeds, 1, st, valid, *out) == bad_arg and b"slot" in lib.ugs_last_error()
    assert not job.value and lib.ugs_uniform_population_destroy(pop) == 0
