"""CPU checks of what pins the wide-form kernels of uniform_sampler (ugs_uniform.hip): the census of kernel paths
(uniform_wide_law.census), the inputs chosen by it (tests/uniform_wide_paths.py) and the device model with its mutants
(tests/uniform_wide_device_model.py).  Shown here by assertion: every census class is reached by some input, every input reaches
what it names, the model equals the law on every input -- through the plain entries and through the population's rows -- every
result-changing mutant of the model differs from the law on some input, and the equivalent mutants change nothing.
tests/test_gpu_uniform_wide_paths.py runs the same inputs through the kernels."""
import math
import os
import re

import numpy as np
import pytest

import uniform_law as U
import uniform_wide_device_model as DM
import uniform_wide_law as W
import uniform_wide_paths as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in P.cases()]
SLOW = ("K66_k3", "K66_k4_count", "K70_k3", "K34_k5_count_narrow", "cluster256_k8", "cluster256_k8_batch", "star130_k3")


def same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def model_run(c, mode, mutant=None, pop=False):
    """(the model's tensors in the law's layout, the model); a refused call gives ()"""
    model = DM.Model(c.ei, c.ptr, c.k, c.what != "batch", mutant=mutant, limit=P.LIMIT, mask_vertices=c.mask_vertices,
                     budget=c.max_rows if c.what in ("enumerate", "refused") else W.BUDGET, over=[g for g, _ in c.closed])
    if c.what == "count":
        return (np.array(model.count(), np.int64),), model
    if c.what in ("enumerate", "refused"):
        try:
            return model.enumerate(mode), model
        except DM.Refused:
            return (), model
    return model.sample(c.m, mode, c.seed, c.seeds, pop=pop), model


def model_differs(mutant, name):
    c = P.case(name)
    try:
        return any(not same(model_run(c, mode, mutant, pop)[0], P.law_of(name, mode)) for mode in c.modes
                   for pop in ((False, True) if c.what in ("batch", "graphs") else (False,)))
    except DM.ModelFault:
        return True


def test_model_constants_and_lines_are_the_kernels():
    # the census and the model restate these; if the kernel's move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_uniform.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "ugs_device.h")) as f:
        header = f.read()
    const = lambda name, text=hip: int(re.search(r"\b%s = (\d+)[;,]" % name, text).group(1))   # noqa: E731
    assert const("WIDE_LANES") == W.WIDE_LANES == DM.LANES and const("POP_LANES") == W.POP_LANES == DM.POP_LANES
    assert const("UNI_BLOCK") == W.ROW_BLOCK and const("SMALL_SORT") == W.SMALL_SORT == DM.SMALL_SORT
    assert "#define UGS_UNI_WIDE_MAX_K %d\n" % W.WIDE_MAX_K in header and DM.MAX_K == W.WIDE_MAX_K
    assert "#define UGS_UNI_BUDGET ((int64_t)1 << 25)" in header and W.BUDGET == 1 << 25
    assert "if (x.cnt - x.flushed >= %d / WIDE_LANES) {" % W.ITEM_FLUSH in hip and W.LANE_FLUSH == DM.LANE_FLUSH == W.ITEM_FLUSH // W.WIDE_LANES
    assert "const int slot = (int)(item & %d);" % (W.ROOT_ITEMS - 1) in hip and DM.ITEMS == W.ROOT_ITEMS
    for line in ("for (uint32_t r = (uint32_t)slot; r < deg && !x.stop; r += 64) {", "const bool holds = excl <= r && r < incl;",
                 "for (uint32_t i = r - excl; i > 0; --i) t &= t - 1;",
                 "const uint64_t later = x.l < l0 ? 0ull : x.l == l0 ? above_mask(f) : ~0ull;",
                 "return v >= 63 ? 0ull : (~0ull << (v + 1));",
                 "x.abv = x.l < vw ? 0ull : x.l == vw ? above_mask(v & 63) : ~0ull;",
                 "const int l0 = __ffs(bits) - 1;", "if (x.l == l0) ext &= ext - 1;",
                 "for (int i = 0; i < D; ++i) above += (uint32_t)((key >> (i * b)) & fm) > w ? 1 : 0;",
                 "return (sh + b >= 64 ? 0ull : hi << (sh + b)) | ((uint64_t)w << sh) | (key & ((1ull << sh) - 1));",
                 "0x111, 0xf, 0xf, false);   // row_shr:1", "0x112, 0xf, 0xf, false);   // row_shr:2",
                 "0x114, 0xf, 0xf, false);   // row_shr:4", "0x118, 0xf, 0xf, false);   // row_shr:8",
                 "x.out += tot;", "wide_level<D + 1, WRITE>(x, ext | (aw & ~nb & x.abv), nb | aw, key_with<D>(key, (uint32_t)w, x.b));",
                 "wide_level<2, WRITE>(x, (ext1 & later) | (aw & ~nb1 & x.abv), nb1 | aw, ((uint64_t)v << x.b) | (uint64_t)w);",
                 "if (slot == 0) wide_last<1, WRITE>(x, ext1, (uint64_t)v);",
                 "int b = 1; while (b < 16 && (1 << b) < n) ++b; return b;", "const int W = (gd.n + 63) >> 6;",
                 "wd.wpair[p] = (uint32_t)u | ((uint32_t)v << 16);",
                 "atomicOr((unsigned long long *)&wd.wadj[base + (int64_t)u * W + (v >> 6)], 1ull << (v & 63));",
                 "const int64_t d = c.seeds ? row : (int64_t)c.nepos[g] * c.m + s;",
                 "return !c.status[1] && c.gsize[g] > 0;",
                 "if ((uint32_t)((key >> (b * (k - 1 - j))) & fm) == u) return j;",
                 "const int pu = tuple_pos(key, k, b, uv & 0xFFFFu), pv = tuple_pos(key, k, b, uv >> 16);",
                 "if (c.sptr[mid + 1] <= row) lo = mid + 1; else hi = mid;",
                 "w += (uint32_t)__shfl((int)incl, POP_LANES - 1, POP_LANES);"):
        assert line in hip, line


def test_mutant_lists_are_disjoint_and_documented():
    assert not set(DM.MUTANTS) & set(DM.EQUIVALENT)
    for name in DM.MUTANTS + DM.EQUIVALENT:
        assert re.search(r"^  %s\s" % name, DM.__doc__, re.M), name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes(name):
    census = P.census_of(name)
    assert census <= set(W.WIDE_CLASSES)
    for cls in P.case(name).reaches:
        assert cls in W.WIDE_CLASSES, cls
        assert cls in census, (name, cls, sorted(census))


@pytest.mark.parametrize("cls", W.WIDE_CLASSES)
def test_census_covers_every_class(cls):
    assert any(cls in P.case(name).reaches and cls in P.census_of(name) for name in CASE_NAMES), cls


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_model_equals_the_law(name):
    c = P.case(name)
    for mode in c.modes:
        for pop in ((False, True) if c.what in ("batch", "graphs") else (False,)):
            got, model = model_run(c, mode, pop=pop)
            want = P.law_of(name, mode)
            assert len(got) == len(want), (name, mode, pop)
            for i, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and np.array_equal(a, b), (name, mode, pop, i)
            if c.what in ("graphs", "enumerate"):
                assert tuple(model.failed) == c.failed
            assert model.max_sh_b <= 56                              # key_with's `sh + b >= 64` case is never taken


def test_closed_forms_and_the_count_pass_flushes():
    """K_66 at k = 4: 720 720 sets, the largest item holds C(64, 2) = 2016, lanes flush and end with a remainder; K_34 at k = 5
    through the wide kernels: item (0, 0) holds C(32, 3) = 4960 sets, all of them counted by lane 0."""
    c = P.case("K66_k4_count")
    got, model = model_run(c, None)
    assert got[0].tolist() == [math.comb(66, 4)] == list(c.counts)
    assert max(model.icount.values()) == model.icount[0] == math.comb(64, 2) == 2016
    flushed = [v for v in model.flushes.values()]
    assert len(flushed) > 100 and any(any(rest) for _, rest in flushed)
    c = P.case("K34_k5_count_narrow")
    got, model = model_run(c, None)
    assert got[0].tolist() == [math.comb(34, 5)] and model.icount[0] == math.comb(32, 3) > W.ITEM_FLUSH
    nflush, rest = model.flushes[0]
    assert nflush >= 4960 // 256 - 1 and rest[0] > 0 and not any(rest[1:])


def test_boundary_buckets_and_budget_as_the_law_computes_them():
    n, ei = P.star130()
    roots = np.bincount([t[0] for t in W.sorted_tuples(U.graph_adjacency(ei[0], ei[1], 0, n), 3)], minlength=n)
    assert roots[0] == math.comb(129, 2) == 8256 > W.SMALL_SORT and 2 <= roots[1] <= W.SMALL_SORT
    n, ei = P.cluster256()
    roots = np.bincount([t[0] for t in W.sorted_tuples(U.graph_adjacency(ei[0], ei[1], 0, n), 8)], minlength=n)
    assert roots[128] == math.comb(16, 7) > W.SMALL_SORT > roots[129] == math.comb(15, 7) and roots[:128].sum() == 0
    at, over = P.case("enum_at_max_rows"), P.case("enum_over_max_rows")
    assert P.law_of("enum_at_max_rows", "sample")[3][-1] == at.max_rows == over.max_rows + 1
    assert model_run(over, "sample")[0] == () and len(model_run(at, "sample")[0]) == 6
    assert math.comb(100, 6) > W.BUDGET and dict(P.case("graphs_over_budget").closed) == {1: math.comb(100, 6)}


# mutant -> (the census class whose inputs can tell it from the kernel, the case that does)
KILLED_BY = {"one_trip": ("deg_ge129", "star130_k3"), "later_le": ("rth_inside_word", "hub1024_k3"), "later_no_guard": ("rth_bit63", "hub1024_k3"),
             "abv_no_own_word": ("root_lower_in_word", "hub1024_k3"), "take_clear_all": ("take_lane_above0", "hub1024_k4"),
             "excl_lt": ("deg1", "hub1024_k3"), "scan_no_shr1": ("last_shr1", "star130_k2"), "scan_no_shr2": ("last_shr2", "star130_k2"),
             "scan_no_shr4": ("last_shr4", "hub1024_k3"), "scan_no_shr8": ("last_shr8", "hub1024_k3"), "out_pc": ("last_two_lanes", "hub1024_k4"),
             "fb_le": ("key_bit63", "cluster256_k8_batch"), "wadj_W_shr6": ("W2", "K10_k5"), "wadj_and31": ("adj_bit63", "star130_k2"),
             "wrows_g_m": ("nepos_ne_g", "layout_batch"), "wrows_key_ne0": ("k1_set0", "k1_batch"), "tp_shift": ("sample", "star130_k2"),
             "wfill_swap": ("sample", "hub1024_k4_batch"), "enum_lt": ("wide_mask_wide", "layout_enum"),
             "pop_carry_lane0": ("pop_hit_lane15_then_lane0", "pop_cols_batch")}


@pytest.mark.parametrize("mutant", DM.MUTANTS)
def test_a_named_input_tells_the_mutant_from_the_law(mutant):
    assert set(KILLED_BY) == set(DM.MUTANTS)
    cls, name = KILLED_BY[mutant]
    assert cls in W.WIDE_CLASSES and cls in P.census_of(name), (mutant, cls, name)
    assert model_differs(mutant, name), (mutant, name)


def test_every_input_of_a_deciding_class_tells_its_mutant():
    # stronger than "some input": wherever the census says the line decides the result, the mutant is wrong there
    for name in [n for n in CASE_NAMES if n not in SLOW]:
        census, c = P.census_of(name), P.case(name)
        if c.what == "refused":
            continue
        if c.k >= 3 and census & {"deg1", "deg64", "deg65"}:
            assert model_differs("excl_lt", name), name
        if c.k >= 3 and "rth_bit63" in census:
            assert model_differs("later_no_guard", name), name
        for s in W.SCAN_STEPS:
            if f"last_shr{s}" in census and c.what == "enumerate":
                assert model_differs(f"scan_no_shr{s}", name), (name, s)
        if "k1_set0" in census and c.what == "batch":
            assert model_differs("wrows_key_ne0", name), name
        if "pop_hit_lane15_then_lane0" in census:
            assert model_differs("pop_carry_lane0", name), name
    # where 64 divides n the two row strides of uni_wadj agree
    assert not model_differs("wadj_W_shr6", "hub1024_k3") and model_differs("wadj_W_shr6", "K10_k5")
    # the 64-stride: a second trip exists from 65 higher neighbours on
    assert model_differs("one_trip", "star130_k2") is False and model_differs("one_trip", "star130_k3")
    # field_bits at n = 2^j: one bit more per field still fits at k = 3, and no longer at k = 8 with 256 vertices
    assert not model_differs("fb_le", "sizes_enum") and model_differs("fb_le", "cluster256_k8_batch")


def test_equivalent_mutants_change_nothing():
    for mutant in DM.EQUIVALENT:
        for name in ("hub1024_k3", "hub1024_k4", "hub1024_k4_batch", "sizes_graphs", "K10_k7", "layout_batch", "star130_k2", "k1_batch",
                     "cluster256_k8_batch"):
            assert not model_differs(mutant, name), (mutant, name)
    # take_highest does take another way through the search: the keys of an item are written in another order
    c = P.case("hub1024_k4")
    a, b = model_run(c, "sample")[1], model_run(c, "sample", "take_highest")[1]
    assert a.keys_sorted == b.keys_sorted and a.icount == b.icount
