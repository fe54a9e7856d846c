"""CPU checks of the device batch pass's pins: the law (tests/batch_pass_law.py) equals the oracle's preprocessing on every graph
of every input (tests/batch_pass_paths.py) and the oracle's LRU behaviour for the keys; the census restates the kernels'
constants; every input reaches the classes it is there for; the device model (tests/batch_pass_device_model.py) equals the law;
and every mutant of the model differs from the law on a named input."""
import os
import re

import numpy as np
import pytest

import batch_pass_device_model as DM
import batch_pass_law as L
import batch_pass_paths as P
import oracle

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in P.cases()]

# every class of the census that some input must reach ("Which test pins which path")
CLASSES = [
    "fused, empty quarter", "fused, straddles quarter", "fused, partial chunk", "keep, 512 chunks", "no keep", "keep and no keep in one block",
    "no keep, large", "two kernels, G * E > 4 Mi", "span > 256", "foreign inside span", "assign, many graphs per wave", "assign, shared ptr value",
    "cross-graph column", "stray column", "cn == 0", "cn == lim", "cn == lim + 1", "n == 256", "n == 257", "n == 2048", "n == 2049",
    "ns == 63", "ns == 64", "ns == 65", "strided s == 2", "strided s == 3", "strided s == 16", "degree tie",
    "row fills a chunk", "row over chunks", "two rows share a chunk", "loop", "empty row", "last chunk partial",
    "mask search n == 64", "list search n == 65", "mask search, vertex >= 32 reached", "n == 1024", "n == 1025 host", "n > 256",
    "reaches k at the last neighbour", "second level needed", "unreachable among reachable", "k == 1", "k == 32",
    "no small stack", "demotion", "no demotion", "demoted one popped next", "leftover small", "leftover large",
    "b inexact", "scale association matters", "alias association matters", "level 0", "level 1", "level 2", "large form",
]
# classes no input reaches, with the reason (DESIGN.md section 9 repeats them)
UNREACHABLE = {
    "leftovers on both stacks": "Vose's loop runs while both stacks hold an entry, so it ends -- or never starts -- with one of them empty",
    "no large stack": "needs Z's rounded sum above the rounded b * n of the largest weight b: not proven impossible where b * n is inexact, but no input "
                      "here has it; the kernel's loop is then skipped like the oracle's",
}


def test_census_constants_are_the_kernels():
    # the census restates these; if the kernels' move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_batch.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "ugs_device.h")) as f:
        dev = f.read()
    define = lambda name: re.search(r"#define %s \(?(\d+)(ll << (\d+)\))?" % name, dev)
    assert int(define("UGS_BATCH_PASS_MAX_COLS").group(1)) == L.MAX_COLS and int(define("UGS_BATCH_PASS_COLS_CEIL").group(1)) == L.COLS_CEIL
    assert int(define("UGS_BATCH_PASS_MAX_N").group(1)) == L.MAX_N and int(define("UGS_BATCH_ROOTS_MAX_N").group(1)) == L.ROOTS_MAX_N
    assert int(define("UGS_KMAX").group(1)) == L.KMAX
    fw = define("UGS_BATCH_PASS_FUSED_WORK")
    assert int(fw.group(1)) << int(fw.group(3)) == L.FUSED_WORK == 4 << 20
    assert "constexpr int kBpBlock = %d;" % L.BLOCK in hip and "constexpr int kBpMaskChunks = %d;" % L.MASK_CHUNKS in hip
    assert "per = (((E32 + 3u) / 4u) + 63u) & ~63u;" in hip and "const bool keep = nchunk <= (uint32_t)kBpMaskChunks;" in hip
    assert "for (uint32_t base = j0; base <= j1; base += kBpBlock)" in hip and "const bool mine = j <= j1 && a.owner[j] == g;" in hip
    assert "cn / %du : 1u;" % L.KEY_DIV in hip and "for (uint32_t t0 = 0; t0 < ns; t0 += 64)" in hip
    assert "for (uint32_t e0 = 0; e0 < ne; e0 += 64)" in hip and "if (n <= 64) {" in hip
    assert "if (G * E <= ugs_batch_pass_fused_work())" in hip and 'std::getenv("UGS_BP_FUSED_WORK")' in hip
    assert "pl = (pl + ps) - 1.0;" in hip and "P[i] = P[i] * n / Z;" in hip and "for (int t = 1; t < k; ++t) b *= d;" in hip
    assert [L.key_stride(c) for c in (1000, 1001, 1499, 1500, 8192)] == [1, 2, 2, 3, 16]
    assert L.quarters(600) == [(0, 192), (192, 384), (384, 576), (576, 600)] and L.quarters(131073)[3] == (98496, 131073)


# ---- the law against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_law_equals_the_oracles_preprocessing(name):
    c = P.case(name)
    laws = P.law_of(name)
    assert any(g is not None for g in laws)
    for g, law in enumerate(laws):
        if law is None:
            continue
        pre = oracle.Preproc(np.stack([law["lu"], law["lv"]]), law["n"], c.k)
        d = pre.dump()
        pre.close()
        what = (name, g)
        assert np.array_equal(d["indptr"], law["rowptr"]) and np.array_equal(d["indices"], law["nbr"]), what
        assert np.array_equal(law["cols"][d["edge_col"]], law["nbr_col"]) if law["cn"] else len(law["nbr_col"]) == 0, what
        assert np.array_equal(d["order"], law["order"]) and np.array_equal(d["index_of"], law["rank"]), what
        assert d["suffix_deg"].tolist() == law["suffix_deg"] and d["bucket_b"].tolist() == law["b"] and d["Z"] == law["Z"], what
        if law["Z"] > 0.0:
            assert d["prob"].tolist() == law["prob"] and d["alias"].tolist() == law["alias"], what            # doubles compared exactly
        else:
            assert law["level"] in (1, 2) and len(law["viable_vi"]) > 0, what


def hit_after(first, second, k=3):
    """the oracle's LRU after graph `first`: does `second` hit?  graphs as (n, local columns)"""
    cache = oracle.Cache()
    try:
        for n, e in (first, second):
            oracle.sample_batch(e, np.array([0, n]), 1, k, "sample", 1, cache)
        return cache.stats()["hits"] == 1
    finally:
        cache.close()


@pytest.mark.parametrize("name", ["key_63_64_65", "key_strided", "cols_1000", "cols_8192"])
def test_law_keys_behave_as_the_oracles_lru(name):
    """equal law keys <=> a hit in the oracle's LRU: the graph itself, the graph with a column the stride skips replaced, with a
    column the key covers replaced, and with one more vertex"""
    for law in P.law_of(name):
        if law is None or law["cn"] < 3:
            continue
        n, e = law["n"], np.stack([law["lu"], law["lv"]])
        s = L.key_stride(law["cn"])
        variants = [(n, e), (n + 1, e)]
        for t in (1, s, ((law["cn"] - 1) // s) * s):
            x = e.copy()
            x[1, t] = (x[1, t] + 1) % n
            variants.append((n, x))
        for vn, ve in variants:
            same = L.key(vn, ve[0], ve[1]) == law["key"]
            assert same == hit_after((n, e), (vn, ve)), (name, n, law["cn"], s)
            assert not (same and law["cn"] > L.MAX_COLS and (vn, ve.tobytes()) != (n, e.tobytes())) or L.fingerprint(vn, ve[0], ve[1]) != law["fp"]
        assert (L.key(n, variants[2][1][0], variants[2][1][1]) == law["key"]) == (s > 1)


# ---- census ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes(name):
    c = P.case(name)
    census = P.census_of(name)
    for cls in c.reaches:
        assert cls in CLASSES or cls.startswith("strided s =="), cls
        assert census[cls] > 0, (name, cls, dict(census))
    assert L.hands_over(c.ei, c.ptr, c.k, c.lim) == c.hand_over
    if c.both:                                                       # the two-kernel variant of the same input reaches the two-kernel side
        assert P.census_of(name, "two")["two kernels"] == 1


@pytest.mark.parametrize("cls", CLASSES)
def test_census_covers_every_class(cls):
    assert sum(P.census_of(name)[cls] for name in CASE_NAMES) > 0, cls


def test_unreachable_classes_stay_unreached():
    for cls in UNREACHABLE:
        assert sum(P.census_of(name)[cls] for name in CASE_NAMES) == 0, cls


def test_the_floating_point_inputs_change_the_records():
    """on the inputs the census found, the other association of each formula gives other records -- so a kernel that
    re-associates cannot pass tests/test_gpu_batch_pass_paths.py"""
    for name, g, alt in (("fp_er40_k12", 0, "scale_alt"), ("fp_er40_k12", 0, "alias_alt"), ("path40_k32", 1, "b_exact")):
        c = P.case(name)
        assert L.graph_law(c.ei, c.ptr, g, c.k, **{alt: True})["prob"] != P.law_of(name)[g]["prob"], (name, alt)


# ---- device model ---------------------------------------------------------------------------------------------------------------
FIELDS = ("n", "cn", "first", "last", "key", "rowptr", "rank", "nbr", "nbr_rank", "nbr_col", "cols")
ROOT_FIELDS = ("suffix_deg", "Z", "level", "viable_vi", "viable_v", "prob", "alias", "v_self", "v_alias")


def model_differs(name, mutant=None, variant="default", lim=None):
    """does the model leave anything but the law's values on the case?  (an IndexError is a write outside the block's arrays)"""
    c = P.case(name)
    lim = c.lim if lim is None else lim
    laws = P.law_of(name)
    try:
        got = DM.batch(c.ei, c.ptr, c.k, lim, P.fused_work_of(c, variant), mutant)
    except IndexError:
        return True
    for g, (law, m) in enumerate(zip(laws, got)):
        n = int(c.ptr[g + 1] - c.ptr[g])
        if n <= 0 or n < c.k:
            want = None
        elif n > L.MAX_N or len(L.owned(c.ei, c.ptr[g], c.ptr[g + 1])) > lim:
            want = "over"
        else:
            want = law
        if want is None or isinstance(want, str):
            if m is not want and m != want:
                return True
            continue
        if m is None or isinstance(m, str):
            return True
        for f in FIELDS:
            if not np.array_equal(np.asarray(m[f]), np.asarray(law[f])):
                return True
        if "level" in m:
            for f in ROOT_FIELDS:
                if f in law and (m[f] != law[f] if f in ("Z", "level") else list(m.get(f, ())) != list(law[f])):
                    return True
    return False


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_model_equals_the_law(name):
    c = P.case(name)
    assert not model_differs(name)
    if c.both:
        assert not model_differs(name, variant="two")
    if c.fused_work == 0:
        assert not model_differs(name, variant="fused")
    if c.large_too:
        assert not model_differs(name, lim=L.COLS_CEIL)


# the input that tells each mutant from the law, and the variant it runs in
KILLERS = {
    "fused_inclusive_prefix": ("fused_small", "default"), "span_inclusive_prefix": ("span_rounds", "default"),
    "fused_off_without_earlier_waves": ("fused_straddle", "default"), "span_off_without_earlier_waves": ("span_rounds", "default"),
    "fused_no_w1_bound": ("fused_straddle", "default"), "fused_wrong_chunk": ("fused_straddle", "default"),
    "reread_one_endpoint": ("keep_and_no_keep", "default"),
    "span_last_excluded": ("span_rounds", "default"), "run_sh_not_advanced": ("span_rounds", "default"),
    "search_first_of_equal_ptr": ("assign_many", "default"), "jmax_from_lowest_lane": ("assign_many", "default"),
    "rank_tie_le": ("fused_small", "default"), "below_inclusive": ("placement", "default"), "cursor_by_one": ("placement", "default"),
    "msk_not_cleared": ("placement", "default"), "suffix_gt": ("two_hubs", "default"), "no_cnt_bound": ("path40_k32", "default"),
    "mask_32_bits": ("n64_n65", "default"), "stride_512": ("key_strided", "default"), "ns_no_round_up": ("key_strided", "default"),
    "carry_dropped": ("n256_257", "default"), "b_power": ("path40_k32", "default"), "scale_reassociated": ("fp_er40_k12", "default"),
    "alias_reassociated": ("fp_er40_k12", "default"), "demoted_not_next": ("two_hubs", "default"),
}


@pytest.mark.parametrize("mutant", DM.MUTANTS)
def test_a_named_input_tells_the_mutant_from_the_law(mutant):
    assert set(KILLERS) == set(DM.MUTANTS)
    name, variant = KILLERS[mutant]
    assert model_differs(name, mutant, variant), (mutant, name)


def test_mutants_of_one_variant_leave_the_other_alone():
    # the fused and the span compaction are separate code: a slip in one cannot show in the other's run of the same input
    assert not model_differs("span_rounds", "fused_inclusive_prefix") and not model_differs("fused_straddle", "span_inclusive_prefix")
    assert model_differs("fused_straddle", "span_inclusive_prefix", "two") and model_differs("fused_straddle", "jmax_from_lowest_lane", "two")


def test_design_names_every_case_and_mutant_killer():
    with open(os.path.join(os.path.dirname(CSRC), os.pardir, "DESIGN.md")) as f:
        design = f.read()
    for name in CASE_NAMES + [k for k, _ in KILLERS.values()]:
        assert "`%s`" % name in design, name
