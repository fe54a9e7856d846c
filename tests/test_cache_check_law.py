"""CPU checks of what pins the check of a cached call in ugs_sampler.GraphCache (ugs_store.hip: ugs_store_check_k) and
rwr_sampler.GraphCache (ugs_rwr.hip: rwr_store_check): the census of the inputs (tests/cache_check_cases.py), the model of both
kernels and its mutants.  Shown here by assertion: every class is reached by a case that names it, every case reaches what it names,
the model of either kernel equals the law on the unaltered and on the altered batch of every case, and every mutant differs from the
law on a named case.  tests/test_gpu_cache_checks.py sends the same batches through both caches."""
import os
import re

import numpy as np
import pytest

import cache_check_cases as CC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in CC.cases()]
KINDS = ("ugs", "rwr")


def kinds_of(c):
    return ("rwr",) if c.failed else KINDS


def differs(mutant, name):
    """the mutant names another graph than the law, on the unaltered or on the altered batch, in either kernel"""
    c = CC.case(name)
    try:
        return any(CC.model(c, kind, ei, mutant) != CC.law(c, ei) for kind in kinds_of(c) for ei in (c.ei, c.bad))
    except CC.ModelFault:
        return True


def test_model_constants_and_lines_are_the_kernels():
    with open(os.path.join(CSRC, "ugs_store.hip")) as f:
        store = f.read()
    with open(os.path.join(CSRC, "ugs_rwr.hip")) as f:
        rwr = f.read()
    assert int(re.search(r"constexpr int STORE_BLOCK = (\d+);", store).group(1)) == CC.BLOCK
    assert int(re.search(r"constexpr int RWR_BLOCK = (\d+);", rwr).group(1)) == CC.BLOCK
    for line in ("const int64_t e = (int64_t)blockIdx.x * STORE_BLOCK + threadIdx.x;", "if (e >= c.E) return;", "int64_t lo = 0, hi = c.G;",
                 "while (hi - lo > 1) {", "if (c.coff[mid] <= e) lo = mid; else hi = mid;",
                 "const int2 want = c.cols[c.col0[lo] + (e - c.coff[lo])];", "const int64_t base = c.lo[lo];",
                 "if (c.src[e] - base != (int64_t)want.x || c.dst[e] - base != (int64_t)want.y) atomicMin(c.first_bad, (int32_t)lo);",
                 "hipLaunchKernelGGL(ugs_store_check_k, dim3(blocks(c.E, STORE_BLOCK)), dim3(STORE_BLOCK), 0, s, c);"):
        assert line in store, line
    for line in ("int64_t lo = 0, hi = k.G - 1;",
                 "while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (k.coff[mid] <= e) lo = mid; else hi = mid - 1; }",
                 "if (c0 < 0) return;", "const int2 want = k.cols[c0 + e - k.coff[lo]];", "const int64_t base = k.graphs[lo].lo;",
                 "if (k.src[e] - base != (int64_t)want.x || k.dst[e] - base != (int64_t)want.y) atomicMin(k.first_bad, (int32_t)lo);",
                 "hipLaunchKernelGGL(rwr_store_check, dim3(blocks(k.E, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, k);"):
        assert line in rwr, line
    # the batch's columns of a cached call go up for the check alone
    with open(os.path.join(CSRC, "ugs_graph_cache.cpp")) as f:
        assert "const int64_t Ec = run_check ? E : 0;" in f.read()
    with open(os.path.join(CSRC, "ugs_rwr_cache.cpp")) as f:
        assert "const int64_t Ec = checked ? E : 0;" in f.read()


def test_mutants_are_documented():
    for name in CC.MUTANTS:
        assert re.search(r"^  %s\s" % name, CC.__doc__, re.M), name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes_and_the_law_names_its_graph(name):
    c = CC.case(name)
    census = CC.census(name)
    assert census <= set(CC.CLASSES)
    for cls in c.reaches:
        assert cls in CC.CLASSES and cls in census, (name, cls, sorted(census))
    assert CC.law(c, c.ei) is None and CC.law(c, c.bad) == c.expect
    assert all(a.shape[1] > 0 or g not in c.failed for g, (_, a) in enumerate(c.graphs))
    assert all(10 * n * CC.K > 2**31 - 1 for g, (n, _) in enumerate(c.graphs) if g in c.failed)
    assert not any((a[0] == a[1]).any() for _, a in c.graphs)       # no loop anywhere: a loop put in is a change


@pytest.mark.parametrize("cls", CC.CLASSES)
def test_census_covers_every_class(cls):
    assert any(cls in CC.case(name).reaches and cls in CC.census(name) for name in CASE_NAMES), cls


@pytest.mark.parametrize("name", CASE_NAMES)
def test_models_of_both_kernels_equal_the_law(name):
    c = CC.case(name)
    for kind in kinds_of(c):
        assert CC.model(c, kind, c.ei) is None, (name, kind)
        assert CC.model(c, kind, c.bad) == c.expect, (name, kind)


def test_the_aliased_columns_differ_only_above_bit_31():
    for name in ("src_plus_2_to_32", "src_plus_dst_minus_2_to_32"):
        c = CC.case(name)
        assert np.array_equal(c.ei & 0xFFFFFFFF, c.bad & 0xFFFFFFFF) and len(CC.bad_columns(c)) == 1
        assert all(CC.model(c, kind, c.bad, "compare_32_bit") is None for kind in KINDS)      # narrowed to 32 bits the batch passes


# mutant -> (the class whose inputs can tell it from the kernel, the case that does)
KILLED_BY = {"compare_32_bit": ("src_plus_2_to_32", "src_plus_2_to_32"), "search_lower_neighbour": ("bad_graph_right_after_columnless", "right_after_columnless"),
             "search_upper_neighbour": ("bad_column_last_of_its_graph", "last_column_of_a_middle_graph"),
             "names_largest": ("two_bad_graphs_smaller_named", "two_bad_graphs"), "skips_last_column": ("bad_column_is_last", "one_graph_last_column")}


@pytest.mark.parametrize("mutant", CC.MUTANTS)
def test_a_named_input_tells_the_mutant_from_the_law(mutant):
    assert set(KILLED_BY) == set(CC.MUTANTS)
    cls, name = KILLED_BY[mutant]
    assert cls in CC.census(name) and differs(mutant, name), (mutant, cls, name)


def test_every_input_of_a_deciding_class_tells_its_mutant():
    for name in CASE_NAMES:
        census = CC.census(name)
        if "bad_column_is_last" in census and "two_bad_graphs_smaller_named" not in census:
            assert differs("skips_last_column", name), name
        if "two_bad_graphs_smaller_named" in census:
            assert differs("names_largest", name), name
        if census & {"src_plus_2_to_32", "dst_minus_2_to_32"}:
            assert differs("compare_32_bit", name), name
    # each slip of the search shows in the graph it names for the altered batch, in either kernel
    c = CC.case("right_after_columnless")
    assert all(CC.model(c, kind, c.bad, "search_lower_neighbour") != c.expect for kind in KINDS)
    c = CC.case("last_column_of_a_middle_graph")
    # (a graph's last column compared with the next graph's store: that slip refuses the unaltered batch already)
    assert all(CC.model(c, kind, c.ei, "search_upper_neighbour") is not None for kind in KINDS)
