"""CPU checks of what pins the mask-form kernels of uniform_sampler (ugs_uniform.hip): the census of kernel paths
(uniform_law.census), the inputs chosen by it (tests/uniform_paths.py) and the device model with its mutants
(tests/uniform_device_model.py).  Shown here by assertion: every census class is reached by some input, every input reaches what
it names, the model equals the law on every input, every result-changing mutant of the model differs from the law on some input,
and the equivalent mutants change the path and nothing else.  tests/test_gpu_uniform_paths.py runs the same inputs through the
kernels.  That the law itself reproduces the reference's recorded outputs is tests/test_uniform_law.py's assertion."""
import math
import os
import re

import numpy as np
import pytest

import uniform_device_model as DM
import uniform_law as U
import uniform_paths as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in P.cases()]


def same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def model_run(c, mode, mutant=None, current="b"):
    """(the model's tensors in the law's layout, the model)"""
    model = DM.Model(c.ei, c.ptr, c.k, c.what != "batch", mutant=mutant, current=current)
    if c.what == "count":
        return (np.array(model.count(), np.int64),), model
    if c.what == "enumerate":
        return model.enumerate(mode), model
    return model.sample(c.m, mode, c.seed, c.seeds), model


def model_differs(mutant, name, current="b"):
    c = P.case(name)
    return any(not same(model_run(c, mode, mutant, current)[0], P.law_of(name, mode)) for mode in c.modes)


def test_model_constants_and_lines_are_the_kernels():
    # the census and the model restate these; if the kernel's move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_uniform.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "ugs_kernels.hip")) as f:
        kernels = f.read()
    const = lambda name, text=hip: int(re.search(r"\b%s = (\d+)[;,]" % name, text).group(1))   # noqa: E731
    assert const("SMALL_SORT") == DM.SMALL_SORT == U.SMALL_SORT and const("DRAW_BLOCK") == DM.DRAW_BLOCK == U.DRAW_BLOCK
    assert const("UNI_BLOCK") == U.ROW_BLOCK
    assert "constexpr int MT_N = %d, MT_M = %d;" % (DM.MT_N, DM.MT_M) in hip and U.MT_BLOCK == DM.MT_N
    assert 2 * const("kScanWide", kernels) * const("kScanPer", kernels) == U.SCAN_ONE_BLOCK
    for line in ("return v >= 63 ? 0ull : (~0ull << (v + 1));", "return ~__brevll(mask);", "if (c.ptr[mid + 1] <= u) lo = mid + 1;",
                 "while (bits < 32 && ((int64_t)1 << bits) <= c.G) ++bits;", "c.bpair[p] = (uint16_t)(u | (v << 8));",
                 "ext[2] = (ext1 & above_mask(w0)) | (adj[w0] & ~nb1 & abv);", "if (d == k - 1) {", "if (cnt - flushed >= %d) {" % U.FLUSH,
                 "ext[d + 1] = ext[d] | (adj[w] & ~nb[d] & abv);", "if (c.k <= 8) hipLaunchKernelGGL((uni_esu<8, false>)",
                 "b1 - b0 > SMALL_SORT;", "if (n <= 1 || n > SMALL_SORT) {", "if (n == 1 && dst != c.keys_a && threadIdx.x == 0)",
                 "s[i] = i < n ? c.keys_a[b0 + i] : ~0ull;", "const int base = s_ne;", "(int64_t)c.nepos[g] * c.m + s;",
                 "if (i >= MT_M && i < MT_N - 1) r = mt_step(mt[i], mt[i + 1], mt[i - MT_M]);",
                 "mt[MT_N - 1] = mt_step(mt[MT_N - 1], mt[0], mt[MT_M - 1]);", "if (pos == MT_N) { mt_twist(mt); pos = 0; }",
                 "const int u = uv & 63, v = uv >> 8;", "__popcll(mask & ((1ull << u) - 1));", "edge_src[w] = c.cval2[p];"):
        assert line in hip, line


def test_mutant_lists_are_disjoint_and_documented():
    assert not set(DM.MUTANTS) & set(DM.EQUIVALENT)
    for name in DM.MUTANTS + DM.EQUIVALENT:
        assert re.search(r"^  %s\s" % name, DM.__doc__, re.M), name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes(name):
    census = P.census_of(name)
    assert census <= set(U.CLASSES)
    for cls in P.case(name).reaches:
        assert cls in U.CLASSES, cls
        assert cls in census, (name, cls, sorted(census))


@pytest.mark.parametrize("cls", U.CLASSES)
def test_census_covers_every_class(cls):
    assert any(cls in P.case(name).reaches and cls in P.census_of(name) for name in CASE_NAMES), cls


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_model_equals_the_law(name):
    c = P.case(name)
    for mode in c.modes:
        for current in ("a", "b"):                                  # whichever buffer the segmented sort hands back
            got, _ = model_run(c, mode, current=current)
            want = P.law_of(name, mode)
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and np.array_equal(a, b), (name, mode, current, i)


def test_boundary_buckets_as_the_law_computes_them():
    """Root 0's bucket of the two star graphs holds exactly SMALL_SORT and SMALL_SORT + 1 keys, by uniform_law.esu_masks."""
    for (n, ei), total, first in ((P.G8192, 8312, 8192), (P.G8193, 8313, 8193)):
        masks = U.esu_masks(U.graph_adjacency(ei[0], ei[1], 0, n), 4)
        roots = np.bincount([(x & -x).bit_length() - 1 for x in masks], minlength=n)
        assert len(masks) == total and roots[0] == first and roots[1:].max() == 36 and (roots == 0).any() and (roots == 1).any()
        counted = U.item_counts(U.graph_adjacency(ei[0], ei[1], 0, n), 4)
        assert sum(c for (v, _), c in counted.items() if v == 0) == first
    n, ei = P.SMALL_ROOTS
    masks = U.esu_masks(U.graph_adjacency(ei[0], ei[1], 0, n), 4)
    roots = np.bincount([(x & -x).bit_length() - 1 for x in masks], minlength=n).tolist()
    assert 1 in roots and any(r >= 3 and r & (r - 1) for r in roots)   # bucket_1 and bucket_np2 beside the two large roots


def test_count_pass_flushes_and_keeps_a_remainder():
    """K_30 at k = 6: item (0, 1) holds C(28, 4) sets, the count pass flushes its running count and ends with a remainder; the
    graph's total is the closed form (nothing here lists the 593 775 sets)."""
    c = P.case("K30_k6_count")
    adj = U.graph_adjacency(c.ei[0], c.ei[1], 0, 30)
    items = U.item_counts(adj, 6)
    assert items[(0, 1)] == math.comb(28, 4) == 20475 and sum(items.values()) == math.comb(30, 6) == c.counts[0]
    got, model = model_run(c, None)
    assert got[0].tolist() == list(c.counts)
    flushes, rest = model.flushes[1]                                 # item (root 0, first extension 1)
    assert flushes >= 1 and 0 < rest < U.FLUSH
    assert model.icount[1] == 20475


# the census class whose inputs can tell the mutant from the kernel: they are tried first, then every other input
KILLERS = {"above_no_guard": "root_63", "ext2_no_above_w0": "k3", "nb_next": "k8", "d_eq_k": "k3", "key_no_complement": "bucket_2",
           "pad_zero": "bucket_np2", "small_ge": "bucket_8192", "no_copy_1": "bucket_1", "ptr_lt": "stray_cross",
           "bits_lt": "G_pow2_with_stray", "no_carry": "G_eq_321", "draw_g_m": "empties_between", "twist2_to_N": "seed_0",
           "twist3_mt_M": "seed_0", "pos_wrap_no_twist": "eq_313", "decode_v_shr6": "k1", "popc_no_minus1": "k1",
           "cval_for_cval2": "columns_shuffled"}
QUICK = [n for n in CASE_NAMES if n not in ("K18_k6", "K30_k6_count", "sort_pair")]   # the slow inputs last


def tried_in_order(mutant):
    cls = KILLERS[mutant]
    return sorted(CASE_NAMES, key=lambda n: (cls not in P.case(n).reaches, n not in QUICK))


@pytest.mark.parametrize("mutant", DM.MUTANTS)
def test_some_input_tells_the_mutant_from_the_law(mutant):
    assert set(KILLERS) == set(DM.MUTANTS) and set(KILLERS.values()) <= set(U.CLASSES)
    assert any(model_differs(mutant, name) for name in tried_in_order(mutant)), mutant


def test_every_input_of_a_boundary_class_tells_its_mutant():
    # stronger than "some input": wherever the census says the line decides the result, the mutant is wrong there
    for name in QUICK:
        census, c = P.census_of(name), P.case(name)
        if "bucket_8192" in census:
            assert model_differs("small_ge", name), name
        if "G_pow2_with_stray" in census and len(c.ptr) - 1 > 1:
            assert model_differs("bits_lt", name), name
        if census & {"G_eq_321", "G_gt_640"}:
            assert model_differs("no_carry", name), name
        if census & {"eq_313", "eq_624", "eq_625", "m_eq_313", "m_gt_624"}:
            assert model_differs("pos_wrap_no_twist", name), name
        if census & {"eq_312", "eq_313", "eq_624", "eq_625", "m_eq_312", "m_eq_313", "m_gt_624"}:   # the block's last word is drawn from
            assert model_differs("twist2_to_N", name) and model_differs("twist3_mt_M", name), name
        if "root_63" in census:
            assert model_differs("above_no_guard", name), name
    # one generator block exactly: the cursor reaches MT_N and the twist that follows is never read
    assert not model_differs("pos_wrap_no_twist", "draw_312") and not model_differs("pos_wrap_no_twist", "graphs_m312")
    # with keys.Current() == keys_a the n == 1 copy is not needed
    assert not model_differs("no_copy_1", "sort_pair_batch", current="a") and model_differs("no_copy_1", "sort_pair_batch", current="b")


def test_equivalent_mutants_change_the_path_not_the_result():
    for mutant, names in (("switch_k9", ("K12_k8", "K12_k9", "K12_k9_batch", "path64_k33")), ("seg_ge", ("sort_8192", "sort_8193", "sort_pair_batch")),
                          ("decode_u_ff", ("columns_batch", "v63_k3", "path64_k64", "k1_loops"))):
        for name in names:
            assert not model_differs(mutant, name), (mutant, name)
    # switch_k9: the input does write stack level 8, the one an 8-entry stack folds onto level 0
    c = P.case("K12_k9")
    for mutant in (None, "switch_k9"):
        model = model_run(c, "global", mutant)[1]
        assert model.depth == 8
    assert model_run(P.case("K12_k8"), "sample")[1].depth == 7
    # seg_ge / small_ge: the bucket of exactly 8192 keys is sorted in LDS alone; by both routes; by neither
    c = P.case("sort_8192")
    route = lambda mutant: model_run(c, "global", mutant)[1].routes[0]   # noqa: E731
    assert route(None) == [8192, False, True] and route("seg_ge") == [8192, True, True] and route("small_ge") == [8192, False, False]
    assert model_run(P.case("sort_8193"), "global")[1].routes[0] == [8193, True, False]
    # decode_u_ff: bits 6 and 7 of every packed pair are 0, at vertex 63 too
    model = model_run(P.case("v63_k3"), "sample")[1]
    assert any(b & 63 == 63 for b in model.bpair) and any(b >> 8 == 63 for b in model.bpair) and not any(b & 0xC0 for b in model.bpair)
