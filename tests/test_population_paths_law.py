"""CPU checks of what pins the kernels only uniform_sampler.PopulationCache runs (ugs_uniform.hip: uni_pop_pairs / uni_pop_rows /
uni_pop_fill, uni_pop_store, pop_fingerprint / uni_pop_check, uni_pop_loops): the census of the inputs (tests/population_paths.py)
and the device model with its mutants (tests/population_device_model.py).  Shown here by assertion: every class is reached by a case
that names it, every case reaches what it names, every model equals its law on every case, every result-changing mutant differs
from the law on a named case, and the mutants listed as equivalent change nothing.  tests/test_gpu_population_paths.py runs the same
inputs through a PopulationCache."""
import os
import re

import numpy as np
import pytest

import population_device_model as DM
import population_paths as P
import uniform_law as U
import uniform_paths as UP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
DRAW_NAMES = [c.name for c in P.draw_cases()]
NEW_DRAWS = [c.name for c in P.draw_cases() if c.source == "population"]
CHECK_NAMES = [c.name for c in P.check_cases()]
LOOP_NAMES = [c.name for c in P.loop_cases()]


def same(got, want):
    return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got[:5], want[:5]))


def rows_differ(mutant, name):
    c = P.draw_case(name)
    try:
        return any(not same(DM.rows(c, P.draw_rows(name), mode, mutant), P.draw_law(name, mode)) for mode in c.modes)
    except DM.ModelFault:
        return True


def test_model_constants_and_lines_are_the_kernels():
    # the census and the models restate these; if the kernels' move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_uniform.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "ugs_device.h")) as f:
        header = f.read()
    const = lambda name: int(re.search(r"\b%s = (\d+)[;,]" % name, hip).group(1))   # noqa: E731
    assert const("POP_LANES") == P.LANES and const("UNI_BLOCK") == P.ROW_BLOCK
    assert "hipLaunchKernelGGL(uni_pop_store, dim3((unsigned)c.G, %d), dim3(UNI_BLOCK), 0, s, c, w, dst, fp_out);" % P.STORE_Y in hip
    assert "#define UGS_UNI_WIDE_MAX_N %d\n" % (64 * P.LOOP_WORDS) in header and "constexpr int WORDS = UGS_UNI_WIDE_MAX_N / 64;" in hip
    for line in ("p.pair[q] = (uint32_t)(p.c.src[col] - lo) | ((uint32_t)(p.c.dst[col] - lo) << 16);",
                 "const int64_t row = (int64_t)blockIdx.x * POP_GROUPS + threadIdx.x / POP_LANES;", "const int l = threadIdx.x & (POP_LANES - 1);",
                 "const int64_t g = row / c.m;", "const uint64_t mask = live ? mask_of(key) : 0ull;",
                 "int j = __popcll(mask & ((1ull << (4 * l)) - 1));",
                 "for (uint32_t e = (uint32_t)(mask >> (4 * l)) & 15u; e; e &= e - 1) out[j++] = pg.lo + 4 * l + (__ffs(e) - 1);",
                 "for (int64_t q = c.cstart[g] + l; q < c.cstart[g + 1]; q += POP_LANES) {",
                 "cnt += (uint32_t)((mask >> (uv & 63)) & (mask >> ((uv >> 16) & 63)) & 1);",
                 "for (int j = l; j < c.k; j += POP_LANES) out[j] = -1;", "if (l == POP_LANES - 1) c.ecount[row] = tot;",
                 "u = uv & 63; v = (uv >> 16) & 63;", "hit = (uint32_t)((mask >> u) & (mask >> v) & 1);",
                 "const int64_t o = w + (incl - hit);", "edge_index[o] = __popcll(mask & ((1ull << u) - 1));",
                 "w += (uint32_t)__shfl((int)incl, POP_LANES - 1, POP_LANES);",
                 "const int64_t d = p.c.seeds ? row : (int64_t)p.c.nepos[g] * p.c.m + (row - g * p.c.m);",
                 # the store
                 "for (int64_t i = (int64_t)blockIdx.y * UNI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.y * UNI_BLOCK) out[i] = in[i];",
                 "if (out) {",
                 # the fingerprint and its check
                 "uint64_t x = word + 0x9E3779B97F4A7C15ull * (pos + 1);", "x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;",
                 "x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;", "return x ^ (x >> 31);",
                 "const int64_t words = gd.enumerable == 1 ? (int64_t)gd.n : (int64_t)gd.n * ((gd.n + 63) >> 6);",
                 "for (int64_t i = threadIdx.x; i < words; i += UNI_BLOCK) { const uint64_t x = bm[i]; if (x) acc += fp_mix(x, (uint64_t)i); }",
                 "if ((int)threadIdx.x < off) s_sum[threadIdx.x] += s_sum[threadIdx.x + off];",
                 "if (threadIdx.x == 0 && p.pg[g].form != 0 && fp != p.pg[g].fp)",
                 "atomicMax((unsigned long long *)&p.c.status[2], (unsigned long long)(p.c.G - g));",
                 "if (u == v) return;                                             // a loop joins nothing (the reference's BFS ignores it)",
                 "atomicOr((unsigned long long *)&wd.wadj[base + (int64_t)u * W + (v >> 6)], 1ull << (v & 63));",
                 # the loop vertices
                 "for (int64_t q = c.cstart[g] + threadIdx.x; q < c.cstart[g + 1]; q += UNI_BLOCK) {",
                 "if (u == c.dst[col] - gd.lo && u >= 0 && u < UGS_UNI_WIDE_MAX_N) atomicOr(&s_bits[u >> 6], 1ull << (u & 63));",
                 "for (int i = 0; i < WORDS; ++i) if (s_bits[i]) fp += fp_mix(s_bits[i], (uint64_t)i);",
                 "if (want && gd.enumerable && fp != want[g]) atomicMax((unsigned long long *)&c.status[3], (unsigned long long)(c.G - g));"):
        assert line in hip, line


def test_mutant_lists_are_disjoint_and_documented():
    for result_changing, equivalent in ((DM.STORE_MUTANTS, DM.STORE_EQUIVALENT), (DM.CHECK_MUTANTS, DM.CHECK_EQUIVALENT)):
        assert not set(result_changing) & set(equivalent)
    for name in DM.ROW_MUTANTS + DM.STORE_MUTANTS + DM.CHECK_MUTANTS + DM.LOOP_MUTANTS:
        assert re.search(r"^  %s\s" % name, DM.__doc__, re.M), name
    for name in DM.STORE_EQUIVALENT + DM.CHECK_EQUIVALENT:
        assert re.search(r"^  %s \(equivalent\)\s" % name, DM.__doc__, re.M), name


# ---- rows and fill ----
def test_every_sampling_case_of_the_mask_form_pin_is_drawn_through_the_population():
    assert [c.name for c in P.draw_cases() if c.source == "uniform_paths"] == [c.name for c in UP.cases() if c.what in ("batch", "graphs")]


@pytest.mark.parametrize("name", DRAW_NAMES)
def test_draw_case_reaches_its_classes(name):
    c = P.draw_case(name)
    if c.source == "uniform_paths":
        census = UP.census_of(name)
        assert all(cls in U.CLASSES and cls in census for cls in c.reaches), (name, sorted(census))
    else:
        census = P.row_census(name)
        assert census <= set(P.ROW_CLASSES)
        for cls in c.reaches:
            assert cls in P.ROW_CLASSES and cls in census, (name, cls, sorted(census))


@pytest.mark.parametrize("cls", P.ROW_CLASSES)
def test_row_census_covers_every_class(cls):
    assert any(cls in P.draw_case(name).reaches and cls in P.row_census(name) for name in NEW_DRAWS), cls


def test_what_the_mask_form_cases_bring_through_the_population_rows():
    """vertex 63 as root, member and endpoint, k = 9 and 33, stray, duplicate and loop columns, ptr[0] != 0, the draw boundaries"""
    reached = set().union(*[P.row_census(c.name) | UP.census_of(c.name) for c in P.draw_cases() if c.source == "uniform_paths"])
    for cls in ("root_63", "w0_63", "edge_at_vertex_63", "k9", "k_ge_33", "stray_cross", "duplicate_column", "loop_column", "ptr0_nonzero",
                "eq_312", "eq_313", "eq_624", "eq_625", "G_eq_320", "G_eq_321", "edge_endpoint_63_as_u", "edge_endpoint_63_as_v", "loop_at_63",
                "nepos_ne_g", "per_graph_seeds", "rows_not_multiple_of_16", "group_spans_two_graphs"):
        assert cls in reached, cls


@pytest.mark.parametrize("name", DRAW_NAMES)
def test_row_model_equals_the_law(name):
    c = P.draw_case(name)
    for mode in c.modes:
        got, want = DM.rows(c, P.draw_rows(name), mode), P.draw_law(name, mode)
        for i, (a, b) in enumerate(zip(got, want[:5])):
            assert a.shape == b.shape and np.array_equal(a, b), (name, mode, i)


def test_the_distinct_case_has_live_rows_of_more_than_16_members_ahead_of_its_rows_of_minus_one():
    c = P.draw_case("distinct_k17")
    nodes, valid = P.draw_law("distinct_k17", "sample")[0].reshape(4, c.m, c.k), P.draw_law("distinct_k17", "sample")[6]
    assert valid.tolist() == [4, 2, 0, 6] and (nodes[0, :4] >= 0).all() and (nodes[0, 4:] == -1).all() and c.k > P.LANES


# mutant -> (the class whose inputs can tell it from the kernel, the case that does)
ROWS_KILLED_BY = {"minus_one_single_trip": ("minus_one_n_lt_k_k_gt_16", "minus_one_k17_batch"), "prefix_uses_4l_plus_4": ("k_eq_16", "paths_k16"),
                  "endpoint_mask_31": ("edge_endpoint_63_as_u", "path64_k33_lanes"), "v_shift_8": ("edge_endpoint_63_as_v", "path64_k33_lanes"),
                  "last_lane_skipped": ("lane15_writes_1", "path64_k33_lanes")}


@pytest.mark.parametrize("mutant", DM.ROW_MUTANTS)
def test_a_named_input_tells_the_row_mutant_from_the_law(mutant):
    assert set(ROWS_KILLED_BY) == set(DM.ROW_MUTANTS)
    cls, name = ROWS_KILLED_BY[mutant]
    assert cls in P.row_census(name) and rows_differ(mutant, name), (mutant, cls, name)


def test_every_input_of_a_deciding_class_tells_its_row_mutant():
    for name in NEW_DRAWS:
        census = P.row_census(name)
        if any(cls.startswith("minus_one_") or cls.startswith("distinct_minus_one") for cls in census):
            assert rows_differ("minus_one_single_trip", name), name
        if any(cls.startswith("lane15_writes_") for cls in census):
            assert rows_differ("last_lane_skipped", name), name
        if census & {"edge_endpoint_63_as_u", "edge_endpoint_63_as_v", "loop_at_63"}:
            assert rows_differ("endpoint_mask_31", name), name
    # at k <= 16 a row of -1 has no second trip: the cases of the earlier pins cannot tell the single trip from the loop
    assert not any(rows_differ("minus_one_single_trip", c.name) for c in P.draw_cases() if c.source == "uniform_paths" and c.k <= P.LANES)


# ---- the store ----
def test_store_case_reaches_its_classes():
    c = P.store_case()
    assert [c.sizes[i] for i in (0, 1, 2, 3)] == [8312, -1, 8313, 0] and 0 < c.sizes[4] < 100 and c.failed_at == 1
    assert P.store_census() == set(P.STORE_CLASSES)
    assert sum(1 for g, d in P.store_draws() if d >= P.STORE_TRIP) >= 12        # m = 4000 over 8313 and 8312 keys: dozens, not one lucky draw


def test_store_model_and_its_mutants():
    c = P.store_case()
    keys = {g: [int(x) for x in U.sorted_masks(U.graph_adjacency(c.graphs[i][1][0], c.graphs[i][1][1], 0, c.graphs[i][0]), c.k)]
            for g, i in enumerate(c.order) if c.sizes[i] > 0}
    assert {g: len(v) for g, v in keys.items()} == {0: 8313, 1: c.sizes[4], 3: 8312}
    stored = {(g, mutant): DM.stored_keys(keys[g], mutant) for g in keys for mutant in (None,) + DM.STORE_MUTANTS + DM.STORE_EQUIVALENT}
    rows = lambda mutant: [stored[g, mutant][d] for g, d in P.store_draws()]      # noqa: E731
    assert all(stored[g, None] == keys[g] for g in keys)
    for mutant in DM.STORE_MUTANTS:
        assert rows(mutant) != rows(None), mutant                    # some drawn row changes
    for mutant in DM.STORE_EQUIVALENT:
        assert all(stored[g, mutant] == keys[g] for g in keys), mutant
    # the single trip is wrong exactly from key 8192 on
    assert [i for i, x in enumerate(stored[0, "single_trip"]) if x != keys[0][i]] == list(range(P.STORE_TRIP, 8313))


# ---- the adjacency check ----
@pytest.mark.parametrize("name", CHECK_NAMES)
def test_check_case_reaches_its_classes_and_its_fingerprints_differ(name):
    c = P.check_case(name)
    census = P.check_census(name)
    assert census <= set(P.CHECK_CLASSES)
    for cls in c.reaches:
        assert cls in P.CHECK_CLASSES and cls in census, (name, cls, sorted(census))
    assert P.adjacency_law(c, c.ei) is None and P.adjacency_law(c, c.bad) == c.expect
    # the expectation on the device rests on this computed inequality, not on luck
    stored, given = DM.graph_fingerprints(c, c.ei), DM.graph_fingerprints(c, c.bad)
    for g, (n, e) in enumerate(c.graphs):
        differs = P.plain_adjacency(c.bad[0], c.bad[1], int(c.ptr[g]), n) != P.plain_adjacency(e[0], e[1], 0, n)
        if P.forms(c)[g]:
            assert (stored[g] != given[g]) == differs, (name, g)
        else:
            assert stored[g] == given[g] == 0


@pytest.mark.parametrize("cls", P.CHECK_CLASSES)
def test_check_census_covers_every_class(cls):
    assert any(cls in P.check_case(name).reaches and cls in P.check_census(name) for name in CHECK_NAMES), cls


@pytest.mark.parametrize("name", CHECK_NAMES)
def test_check_model_equals_the_law(name):
    c = P.check_case(name)
    assert DM.named_graph(c, c.ei) is None and DM.named_graph(c, c.bad) == c.expect


CHECK_KILLED_BY = {"no_position": ("same_words_other_positions", "rows_exchanged_mask"), "one_trip": ("diff_word_index_ge_256", "wide130_last_word"),
                   "names_last": ("two_graphs_differ_first_named", "two_graphs_differ")}


def check_differs(mutant, name):
    c = P.check_case(name)
    return any(DM.named_graph(c, ei, mutant) != P.adjacency_law(c, ei) for ei in (c.ei, c.bad))


@pytest.mark.parametrize("mutant", DM.CHECK_MUTANTS)
def test_a_named_input_tells_the_check_mutant_from_the_law(mutant):
    assert set(CHECK_KILLED_BY) == set(DM.CHECK_MUTANTS)
    cls, name = CHECK_KILLED_BY[mutant]
    assert cls in P.check_census(name) and check_differs(mutant, name), (mutant, cls, name)


def test_every_input_of_a_deciding_class_tells_its_check_mutant():
    for name in CHECK_NAMES:
        census = P.check_census(name)
        if "same_words_other_positions" in census:
            assert check_differs("no_position", name), name
        if "diff_word_index_ge_256" in census:
            assert check_differs("one_trip", name), name
        if "two_graphs_differ_first_named" in census:
            assert check_differs("names_last", name), name


def test_equivalent_check_mutants_change_no_verdict():
    for mutant in DM.CHECK_EQUIVALENT:
        for name in CHECK_NAMES:
            assert not check_differs(mutant, name), (mutant, name)
    # xor_fold is another fingerprint all the same
    c = P.check_case("mask_flip")
    assert DM.graph_fingerprints(c, c.ei, "xor_fold") != DM.graph_fingerprints(c, c.ei)


# ---- the loop vertices ----
@pytest.mark.parametrize("name", LOOP_NAMES)
def test_loop_case_reaches_its_classes_and_the_model_equals_the_law(name):
    c = P.check_case(name)
    census = P.loop_census(name)
    assert census <= set(P.LOOP_CLASSES)
    for cls in c.reaches:
        assert cls in P.LOOP_CLASSES and cls in census, (name, cls, sorted(census))
    assert 1 <= c.k <= 32
    assert P.adjacency_law(c, c.bad) is None and DM.named_graph(c, c.bad) is None          # the adjacency is the added one
    assert P.loops_law(c, c.ei) is None and P.loops_law(c, c.bad) == c.expect
    assert DM.named_loop_graph(c, c.ei) is None and DM.named_loop_graph(c, c.bad) == c.expect


@pytest.mark.parametrize("cls", P.LOOP_CLASSES)
def test_loop_census_covers_every_class(cls):
    assert any(cls in P.check_case(name).reaches and cls in P.loop_census(name) for name in LOOP_NAMES), cls


LOOPS_KILLED_BY = {"bit_only": ("loop_sets_differ_only_in_word_index", "loop_0_stored_64_given"),
                   "no_position": ("loop_sets_differ_only_in_word_index", "loop_64_stored_0_given")}


@pytest.mark.parametrize("mutant", DM.LOOP_MUTANTS)
def test_a_named_input_tells_the_loop_mutant_from_the_law(mutant):
    assert set(LOOPS_KILLED_BY) == set(DM.LOOP_MUTANTS)
    cls, name = LOOPS_KILLED_BY[mutant]
    c = P.check_case(name)
    assert cls in P.loop_census(name) and DM.named_loop_graph(c, c.bad, mutant) != P.loops_law(c, c.bad), (mutant, cls, name)
    for other in LOOP_NAMES:
        if "loop_sets_differ_only_in_word_index" in P.loop_census(other):
            c = P.check_case(other)
            assert DM.named_loop_graph(c, c.bad, mutant) is None, (mutant, other)      # the slip accepts the batch
