"""CPU checks of rows.unique_rows' pins: the census restates the kernels' constants; every input of
tests/rows_unique_paths.py reaches the classes it is there for and every reachable class is named by some input; the device model
(tests/rows_unique_device_model.py) equals the law (tests/rows_unique_law.py) on every input, for both `by`; every mutant of the
model differs from the law on the input named for it.  No GPU and no library call."""
import os
import re
import time

import numpy as np
import pytest

import rows_unique_device_model as DM
import rows_unique_law as L
import rows_unique_paths as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in P.cases()]
GOOD = [c.name for c in P.cases() if c.refusal is None]
SMALL = [n for n in CASE_NAMES if not n.startswith("second_trip")]

# every class of the census that some input must reach
CLASSES = (
    # check
    ["second_trip", "big_past_first_trip", "offence_past_first_trip", "class0", "class1", "class2", "no_small", "no_big", "small_and_big",
     "sample_ptr0", "sample_end", "sample_decreases", "edge_ptr0", "edge_end", "edge_decreases", "ptr_decreases", "rows_over"]
    + ["vertices_over@%d" % b for b in L.ALL_BITS] + ["two_offences_lower_index_wins@%s" % w for w in ("ptr", "graph", "entry")] + ["ptr_beats_graph", "graph_beats_entry"]
    # keys
    + ["unrolled_k%d" % k for k in range(1, 9)] + ["looped"] + ["top_code@%d" % b for b in L.ALL_BITS]
    + ["straddle_hi_only@%d" % k for k in L.STRADDLE_K] + ["straddle_lo_only@%d" % k for k in L.STRADDLE_K]
    + ["field_at_64@%d" % k for k in L.FIELD_AT_64_K]
    + ["bit_127", "set_ties", "set_all_equal", "graph_behind_empty_graphs", "entry_below_graph", "entry_at_hi", "entry_minus_two", "entry_2p32_above"]
    # wave
    + ["rows_1", "rows_2", "rows_63", "rows_64", "slot0", "slot1", "slot2", "slot3", "partial_group", "all_equal", "all_distinct",
       "rep_not_first_lane", "lane63_kept_with_edges"]
    # block
    + ["pn%d_%s" % (pn, what) for pn in (128, 256, 512, 1024, 2048, 4096) for what in ("full", "half_plus_1")] + ["n4095"]
    + ["pad_meets_all_ones_key@%d" % k for k in L.FIELD_AT_64_K]
    + ["run_first", "run_last", "run_all", "run_across_threads", "kept_in_later_wave", "word_x_only", "word_y_only", "word_z_only", "word_w_only",
       "two_graphs_one_class"]
    # scan, compact, edges
    + ["one_pass", "exactly_1024", "1025", "many_passes", "rows_fewer_than_graphs"] + ["span_%d" % s for s in L.SPANS]
    + ["no_edge_src", "strided_edge_index"]
)


def test_census_constants_are_the_kernels():
    # the census restates these; if the kernels' move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_rows.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "ugs_device.h")) as f:
        dev = f.read()
    with open(os.path.join(CSRC, "ugs_rows.cpp")) as f:
        cpp = f.read()
    assert L.constants_in_source(hip, dev) == []
    assert "c.bits = std::min(31, 128 / k);" in cpp and all(L.key_bits(k) == min(31, 128 // k) for k in L.ALL_K)
    assert L.ALL_BITS == (31, 25, 21, 18, 16, 14, 12, 11, 10, 9, 8, 7, 6, 5, 4)
    assert (L.WAVE_ROWS, L.CLASS_BOUNDS, L.MAX_ROWS_PER_GRAPH) == (64, (256, 1024, 4096), 4096)
    assert (L.GRAPHS_PER_GROUP, L.SCAN_PASS, L.EDGE_LANES, L.CHECK_TRIP) == (4, 1024, 16, 1 << 20)
    assert "%#x" % DM.NONE == re.search(r"#define UGS_ROWS_NONE (0x[0-9a-f]+)ll", dev).group(1)
    # the k of the straddle and field-at-64 classes: every b with a field across bit 64 has one, and the three k whose fields end there
    assert {L.key_bits(k) for k in L.STRADDLE_K} == {b for b in L.ALL_BITS if 64 % b}
    assert all(64 // L.key_bits(k) < k for k in L.STRADDLE_K + L.FIELD_AT_64_K) and any(k >= 17 for k in L.STRADDLE_K) and 9 in L.STRADDLE_K
    assert [k for k in L.ALL_K if 64 % L.key_bits(k) == 0 and k * L.key_bits(k) == 128] == list(L.FIELD_AT_64_K)


# ---- census ----
@pytest.mark.parametrize("by", P.BYS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes(name, by):
    c = P.case(name)
    census = P.census_of(name, by)
    for cls in P.reaches_for(c, by):
        assert cls in CLASSES, cls
        assert cls in census, (name, cls, sorted(census))
    assert (c.refusal is None) == (L.refusal(c.arrays) is None)


@pytest.mark.parametrize("cls", CLASSES)
def test_census_covers_every_class(cls):
    by = "set"                                                             # (the set_* classes exist for "set" only; the others for both)
    named = [c.name for c in P.cases() if cls in c.reaches]
    assert named, "no case names %s" % cls
    assert any(cls in P.census_of(name, by) for name in named)
    if not cls.startswith("set_"):
        assert any(cls in P.census_of(name, "sequence") for name in named)


def test_classes_are_what_the_census_can_say():
    said = set().union(*(P.census_of(name, by) for name in CASE_NAMES for by in P.BYS))
    assert said <= set(CLASSES), sorted(said - set(CLASSES))
    assert len(set(CLASSES)) == len(CLASSES)


def test_unreachable_classes_stay_unreached():
    for cls in L.UNREACHABLE:
        assert cls not in CLASSES
        assert not any(cls in P.census_of(name, by) for name in CASE_NAMES for by in P.BYS), cls
    # the arithmetic behind them: k * b, and a class's list against its grid -- m graphs of at least `least` rows each need
    # R >= m * least rows, so m <= R // least, the grid
    assert all(k * L.key_bits(k) <= 128 for k in L.ALL_K)
    for name in GOOD:
        sptr = P.case(name).arrays[3]
        rows, R, G = np.diff(sptr), int(sptr[-1]), len(sptr) - 1
        for least in (65, 257, 1025):
            assert int((rows >= least).sum()) <= min(G, R // least)


def test_every_case_is_needed():
    """deleting a case leaves a class unnamed or a mutant without its input"""
    for c in P.cases():
        others = {cls for o in P.cases() if o.name != c.name for cls in o.reaches}
        assert c.kills or set(c.reaches) - others, c.name


def test_the_large_case_is_quick_for_the_law():
    c = P.case("second_trip")
    t = time.perf_counter()
    L.unique_rows(*c.arrays, "set")
    spent = time.perf_counter() - t
    print("law on second_trip: %.2f s" % spent)
    assert spent < 30.0                                                    # a few seconds; the bound only catches a law gone quadratic
    assert len(c.arrays[3]) - 1 == (1 << 20) + 40 and c.arrays[0].shape == (78, 2)
    assert P.case("second_trip_refused").refusal.endswith(r"\(index %d\)" % P.REFUSED_INDEX) and P.REFUSED_INDEX > L.CHECK_TRIP


# ---- device model ----
def same(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == "refused":
        return a[1:] == b[1:]
    return a[1] == b[1] and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def model_differs(name, by, mutant=None):
    """does the model leave anything but the law's result?  (an IndexError is an access outside an array of the call)"""
    try:
        got = DM.run(P.case(name).arrays, by, mutant)
    except IndexError:
        return True
    return not same(got, P.law_of(name, by))


@pytest.mark.parametrize("by", P.BYS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_model_equals_the_law(name, by):
    assert not model_differs(name, by)


KILLERS = {m: c.name for c in P.cases() for m in c.kills}


@pytest.mark.parametrize("mutant", sorted(DM.MUTANTS))
def test_a_named_input_tells_the_mutant_from_the_law(mutant):
    assert set(KILLERS) == set(DM.MUTANTS) and sum(len(c.kills) for c in P.cases()) == len(KILLERS)
    name = KILLERS[mutant]
    bys = ("set",) if mutant == "rank_tie_le" else P.BYS                   # the rank exists for "set" only
    for by in bys:
        assert model_differs(name, by, mutant), (mutant, name, by)


@pytest.mark.parametrize("by", P.BYS)
def test_the_straddle_mutant_is_told_apart_at_every_width(by):
    """not at one k by chance: every k that has a field across bit 64, the looped form's among them"""
    for k in L.STRADDLE_K:
        assert model_differs("keys_k%d" % k, by, "straddle_hi_dropped"), k
    for k in L.FIELD_AT_64_K:
        assert model_differs("keys_k%d" % k, by, "field_at_64_into_lo"), k
        assert model_differs("pad_all_ones_k%d" % k, by, "pad_row_zero") and model_differs("pad_all_ones_k%d" % k, by, "upper_bound_to_pn"), k


def test_equivalent_slips_equal_the_law():
    for slip in DM.EQUIVALENT:
        for name in SMALL:
            assert not model_differs(name, "set", slip), (slip, name)
    # and the routine itself does change the key: equal codes share a field
    a = DM.Call(P.case("set_ties").arrays, "set")
    b = DM.Call(P.case("set_ties").arrays, "set")
    DM.keys(a, None)
    DM.keys(b, "rank_no_tiebreak")
    assert a.keys != b.keys and len(set(a.keys)) == len(set(b.keys))


def test_mutants_leave_the_other_paths_alone():
    # a slip in one kernel form cannot show in an input that never runs it
    assert not model_differs("wave_sizes", "set", "sort_ignores_row") and not model_differs("block_runs", "set", "wave_rep_last")
    assert not model_differs("keys_k9", "set", "field_at_64_into_lo") and not model_differs("scan_1024", "set", "scan_carry_dropped")
    assert not model_differs("edge_spans", "set", "check_one_trip")


def random_inputs_of_the_gpu_test():
    """every synthetic input of tests/test_gpu_rows_unique.py that comes from law.random_case, rebuilt with its seed"""
    rc, rng = L.random_case, np.random.default_rng
    for rows in ([0], [1], [2], [63], [64], [0, 1, 2, 63, 64, 0, 17, 64, 5], [0, 0, 0]):
        yield "wave%s" % rows, rc(rng(sum(rows) + len(rows)), rows, 6)
    for rows in ([65], [100], [129], [256], [257], [1024], [1025]):
        yield "workgroup%s" % rows, rc(rng(rows[0]), rows, 6, distinct=40)
    yield "mixed", rc(rng(11), [3, 70, 0, 300, 64, 65, 1100, 1, 4096, 0, 130], 5, distinct=25)
    r = rng(2500)
    rows = r.integers(0, 4, size=2500).tolist()
    rows[1023], rows[1024], rows[2499] = 70, 64, 66
    yield "scan2500", rc(r, rows, 3, distinct=2, max_edges=2)
    for k in (1, 2, 5, 8, 9, 32):
        yield "every_k[%d]" % k, rc(rng(k), [10, 80, 0, 33], k, distinct=12)
    r = rng(6)
    yield "no_src", rc(r, [30, 90], 4, max_edges=2, edge_src=False)
    yield "strided", rc(r, [30, 90], 4, max_edges=2)
    yield "cpu", rc(rng(8), [20, 70], 6)
    yield "repeat", rc(rng(9), [64, 700, 65], 6, distinct=30)
    yield "good", rc(rng(21), [10, 70, 5], 4, distinct=9)
    for t in range(2):
        yield "threads%d" % t, rc(rng(31 + t), [64, 200, 3, 900][t:] + [50], 6, distinct=20)


def test_what_the_random_inputs_of_the_gpu_test_leave_open():
    """The two measurements behind section 18.1: the largest edge span among the random inputs of test_gpu_rows_unique.py is 4
    entries, so the edge copy never takes a second trip there; and the straddle mutant is told apart by four of them, none drawn
    for it -- at k = 3 (a row of -1 against one whose last code has no low part), k = 4 and twice at k = 6, mostly for
    by="sequence" only -- and by none at k = 5, 7 or in the looped form (k >= 9)."""
    largest, tellers = 0, []
    for name, case in random_inputs_of_the_gpu_test():
        largest = max(largest, int(np.diff(case[2]).max(initial=0)))
        if case[0].shape[1] in L.STRADDLE_K:
            for by in P.BYS:
                a, b = DM.Call(case, by), DM.Call(case, by)
                DM.check(a, None)
                DM.keys(a, None)
                DM.keys(b, "straddle_hi_dropped")
                sptr = case[3]
                merged = any(len(set(a.keys[sptr[g]:sptr[g + 1]])) != len(set(b.keys[sptr[g]:sptr[g + 1]])) for g in range(len(sptr) - 1))
                if merged:
                    tellers.append((name, by))
    assert largest == 4
    assert tellers == [("workgroup[1024]", "sequence"), ("scan2500", "set"), ("scan2500", "sequence"), ("strided", "sequence"), ("threads0", "sequence")]


def test_design_names_every_case_and_mutant():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    design = design[design.index("### 18.1 Paths pinned"):]
    for name in CASE_NAMES + sorted(DM.MUTANTS) + sorted(L.UNREACHABLE) + sorted(DM.EQUIVALENT):
        assert "`%s`" % name in design, name
