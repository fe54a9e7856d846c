"""CPU checks of the RWR restatement (tests/rwr_law.py): it reproduces every reference fixture (tests/golden/f15_rwr_reference.*),
the counter form of SplitMix64 equals the sequential one, and the speculate / resolve model the device runs finds the same walk
starts as the sequential walk."""
import json
import os
import random

import numpy as np
import pytest

import rwr_law as R
import ugs_workloads as wl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f15_rwr_reference")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def scenarios():
    with open(GOLDEN + ".json") as f:
        return json.load(f)["scenarios"]


@pytest.mark.parametrize("s", scenarios(), ids=lambda s: s["name"])
def test_restatement_reproduces_fixture(s):
    z = np.load(GOLDEN + ".npz")
    name = s["name"]
    got = R.sample_batch(z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"], s["m"], s["k"], s["mode"], int(s["seed"]), s["p_restart"])
    for nm, a in zip(NAMES, got):
        b = z[f"{name}/{nm}"]
        assert a.shape == b.shape and np.array_equal(a, b), (name, nm)


def test_fixture_covers_the_cases():
    s = {x["name"]: x for x in scenarios()}
    assert any(x["mode"] == "graph" for x in s.values()) and any(x["mode"] == "global" for x in s.values())
    assert {0.0, 1.0} <= {x["p_restart"] for x in s.values()}
    assert s["m0_k5"]["rows"] == 0 and s["small_k4"]["failed_rows"] > 0 and int(s["seed_top_k6"]["seed"]) > (1 << 64) - 8
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    assert meta["omp_num_threads"] == 1 and meta["source_sha256"].startswith("c60c99bb")


def test_counter_form_equals_sequential():
    for seed in (0, 42, (1 << 64) - 1, (1 << 64) - 5, 0x9E3779B97F4A7C15, 123456789):
        rng = R.SplitMix64(seed)
        for i in range(1, 300):
            assert rng.next_u64() == R.draw(seed, i)


def test_splitmix_known_values():
    # SplitMix64 of Steele, Lea and Flood seeded with 0 (the generator's state starts at seed + GAMMA, one step ahead of the
    # published sequence whose first output for seed 0 is 0xe220a8397b1dcdaf)
    assert R.mix(R.GAMMA) == 0xE220A8397B1DCDAF
    assert R.draw((0 - R.GAMMA) & R.M64, 1) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("shape,k,p", [((39, 73), 6, 0.2), ((18, 20), 8, 0.2), ((30, 29), 8, 0.5), ((12, 11), 3, 0.0)])
@pytest.mark.parametrize("window", [1, 7, 64])
def test_speculate_resolve_equals_sequential(shape, k, p, window):
    rnd = random.Random(shape[0] * 7 + k + window)
    for t in range(3):
        ei = wl.tu_graph(shape[0], shape[1], rnd.randrange(1000))
        adj = R.adjacency(ei[0], ei[1], [0, shape[0]])[0]
        gseed = rnd.getrandbits(64)
        want = R.sequential_starts(adj, k, p, gseed, 12)
        assert R.chain_starts(adj, k, p, gseed, 12, window) == want


def test_speculate_resolve_with_small_components():
    # a component smaller than k: walks seeded there run all 10 n k iterations; the chain skips over them the same way
    ei = np.array([[0, 1, 2, 3, 5, 6], [1, 2, 3, 4, 6, 6]], np.int64)
    adj = R.adjacency(ei[0], ei[1], [0, 8])[0]
    for seed in (1, 42):
        want = R.sequential_starts(adj, 4, 0.2, seed, 10)
        assert R.chain_starts(adj, 4, 0.2, seed, 10, 16) == want
        lens = np.diff(want)
        assert (lens >= 1 + 10 * 8 * 4).any()                        # some walk ran to the iteration limit


def test_isolated_seed_length():
    # an isolated vertex without edges: every iteration restarts with one draw, so the walk takes exactly 1 + 10 n k draws
    adj = [[1], [0], []]
    for c in range(200):
        chosen, L = R.walk(adj, 2, 0.2, 5, c)
        if chosen == [2]:
            assert L == 1 + 10 * 3 * 2
            break
    else:
        pytest.fail("no walk seeded at the isolated vertex")


# ---- the census of kernel paths (rwr_law.census), the inputs that pin them (rwr_paths.py) and the device model with its mutants ----
import re

import rwr_device_model as DM
import rwr_paths as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in P.cases()]

# every class of the census that some input must reach (DESIGN.md section 11 names the path behind each)
CLASSES = [
    "T0", "lds", "global", "csr_words == 8192", "csr_words == 8193", "vbase > 0", "lds, vbase > 0", "global, vbase > 0",
    "L < 64", "L == 64", "L in (65, 66)", "L > 66", "L > W", "live_failed", "capped", "L == 65 uncapped",
    "offset W - 1", "lands on base + W", "slides", "window with capped and uncapped walks",
    "doomed_row0", "doomed_row_last", "doomed_twice", "doomed at offset W - 1", "doomed_isolated",
    "round 0", "round 1", "round >= 2", "j == 0", "j == 31, bit 0", "j == 31, bit 1",
    "lane == 255 and j == 31, bit 1", "lane == 255 and j == 31, bit 0", "lane == 0 and j == 0 and round > 0", "last_in_lane",
    "spec == 1", "spec == 2", "spec == 3", "spec == 4", "KM == 8", "KM == 16", "KM == 32", "KM == 64", "k == KM",
    "component == k - 1", "component == k", "dropped columns, NV a power of two", "every column dropped",
]


def test_census_constants_are_the_kernels():
    # the census restates these; if the kernel's move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_rwr.hip")) as f:
        hip = f.read()
    hosts = []
    for name in ("ugs_side_rwr.cpp", "ugs_rwr_cache.cpp"):          # rwr_begin and the cached begin
        with open(os.path.join(CSRC, name)) as f:
            hosts.append(f.read())
    const = lambda name: int(re.search(r"constexpr \w+ %s = (\d+);" % name, hip).group(1))
    assert const("RWR_BLOCK") == R.RWR_BLOCK and const("SPEC_CAP") == R.SPEC_CAP and const("RWR_LDS_INTS") == R.RWR_LDS_INTS
    assert "constexpr int RWR_WMAX = %d * RWR_BLOCK;" % R.SPEC_MAX in hip
    assert "if (L >= cap) return ~0ull;" in hip
    assert "(int64_t)gd.n + 1 + D + (gd.n + 3) / 4 <= RWR_LDS_INTS" in hip
    assert "for (int j = 0; j < %d; ++j, z += GAMMA) bits |=" % R.DOOM_LANE in hip and "pos += %dull * RWR_BLOCK;" % R.DOOM_LANE in hip
    assert "while (s < c.m && cc < base + (uint64_t)W)" in hip and "if (left <= n) {" in hip
    assert [int(x) for x in re.findall(r"launch_walks<(\d+)>\(c, s\);", hip)] == list(R.KM_WIDTHS)
    assert [int(x) for x in re.findall(r"hipLaunchKernelGGL\(\(rwr_fill<(\d+)>\)", hip)] == list(R.KM_WIDTHS)
    for host in hosts:
        assert "c.spec = (int32_t)std::min<int64_t>(%d, std::max<int64_t>(1, ((int64_t)m_per_graph * 16 + 255) / 256));" % R.SPEC_MAX in host
    assert [R.spec_window(m) for m in (0, 1, 16, 17, 32, 33, 48, 49, 2100)] == \
        [(1, 256), (1, 256), (1, 256), (2, 512), (2, 512), (3, 768), (3, 768), (4, 1024), (4, 1024)]


def test_step_bits_and_closed_form_equal_the_walk():
    for seed, c, p in ((5, 0, 0.2), ((1 << 64) - 3, 77, 0.5), (9, 1 << 40, 0.0), (9, 3, 1.0)):
        assert R.step_bits(seed, c + 2, 40, p) == [int(R.to_double(R.draw(seed, c + 2 + i)) >= p) for i in range(40)]
    adj = [[1], [0], [2, 2]]                                         # a pair and a looped vertex: every seed doomed for k = 3
    for c in range(30):
        for p in (0.0, 0.3, 1.0):
            x, bit = R.doomed_last_step(11, c, 90, p)
            assert x + 2 + bit == R.walk_len(adj, 3, p, 11, c)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes(name):
    census = P.census_of(name)
    for cls in P.case(name).reaches:
        assert cls in CLASSES or cls.startswith(("spec ==", "KM ==")), cls
        assert census[cls] > 0, (name, cls, dict(census))


@pytest.mark.parametrize("cls", CLASSES)
def test_census_covers_every_class(cls):
    assert sum(P.census_of(name)[cls] for name in CASE_NAMES) > 0, cls


@pytest.mark.parametrize("name", CASE_NAMES)
def test_census_chain_reproduces_sequential_starts(name):
    chains = P.census_starts_of(name)[1]
    assert chains == P.sequential_of(name)
    assert any(ch is not None for ch in chains)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_model_equals_the_law(name):
    c = P.case(name)
    got = DM.batch_starts(c.ei, c.ptr, c.m, c.k, c.seed, c.p, c.seeds)
    assert [g and g[0] for g in got] == P.sequential_of(name)
    want = P.law_of(name, "global")[0].reshape(len(c.ptr) - 1, c.m, c.k)
    for g, res in enumerate(got):
        if res is not None:
            assert res[1] == (want[g, :, 0] >= 0).tolist(), (name, g)
    census = P.census_of(name)
    assert sum(len(res[2]) for res in got if res) == census["capped"]           # lane 0 redoes exactly the capped chain walks


def model_differs(mutant, name):
    c = P.case(name)
    got = DM.batch_starts(c.ei, c.ptr, c.m, c.k, c.seed, c.p, c.seeds, mutant=mutant)
    return [g and g[0] for g in got] != P.sequential_of(name)


# the census class whose inputs can tell the mutant from the kernel: they are tried first, then every other input
KILLERS = {"left_lt": "last_in_lane", "no_lane_carry": "round 0", "no_round_carry": "round 1", "end_no_bit": "round 0",
           "isolated_no_seed": "doomed_isolated", "first_step_early": "round 0",
           "window_le": "lands on base + W", "lds_words_plus_1": "csr_words == 8193"}


@pytest.mark.parametrize("mutant", DM.MUTANTS)
def test_some_input_tells_the_mutant_from_the_law(mutant):
    assert set(KILLERS) == set(DM.MUTANTS)
    order = sorted(CASE_NAMES, key=lambda name: P.census_of(name)[KILLERS[mutant]] == 0)
    assert any(model_differs(mutant, name) for name in order), mutant


def test_every_input_of_a_doomed_class_tells_its_mutant():
    # stronger than "some input": wherever the census says the line decides the result, the mutant is wrong there
    for name in CASE_NAMES:
        census = P.census_of(name)
        if census["last_in_lane"]:
            assert model_differs("left_lt", name), name
        if census["lands on base + W"]:
            assert model_differs("window_le", name), name
        if census["j == 31, bit 1"] or census["round 0"] + census["round 1"] + census["round >= 2"] > 0 and P.case(name).p < 1.0:
            assert model_differs("end_no_bit", name), name


def test_equivalent_mutants_change_the_path_not_the_result():
    # `L > cap` for `L >= cap` and an LDS bound one word too narrow cannot be told from the kernel by any output: lane 0's redo
    # finds the same length, and the global-memory CSR holds the same rows.  What they change is which path runs, so the inputs
    # must at least put walks on that line: a chain walk that only `>=` caps, and a graph of exactly RWR_LDS_INTS words.
    fewer = 0
    for name in CASE_NAMES:
        if P.census_of(name)["L in (65, 66)"]:
            c = P.case(name)
            kernel = DM.batch_starts(c.ei, c.ptr, c.m, c.k, c.seed, c.p)[0]
            mutant = DM.batch_starts(c.ei, c.ptr, c.m, c.k, c.seed, c.p, mutant="cap_gt")[0]
            assert mutant[:2] == kernel[:2] and set(mutant[2]) <= set(kernel[2]), name
            fewer += set(mutant[2]) < set(kernel[2])
    assert fewer > 0
    assert P.census_of("placement")["csr_words == 8192"] == 1
