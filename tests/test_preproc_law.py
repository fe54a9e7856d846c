"""CPU checks of the device preprocessing's pins: the law (tests/preproc_law.py) equals the oracle's preprocessing on every named
input (tests/preproc_paths.py) and, where the library loads without a GPU, the host path's preproc_dump; the constants the law
mirrors are the sources'; every input reaches the census classes it is there for and every class is reached; the device model
(tests/preproc_device_model.py) equals the law; every mutant of the model differs from the law on a named input."""
import os
import re

import numpy as np
import pytest

import oracle
import preproc_device_model as DM
import preproc_law as L
import preproc_paths as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in P.cases()]
BATCH_NAMES = [b.name for b in P.batches()]
DUMP_FIELDS = ("indptr", "indices", "edge_col", "order", "index_of", "suffix_deg", "bucket_b")

# every class of the census that some input must reach ("Which test pins which path of device preprocessing")
CLASSES = (
    ["bits == %d" % b for b in (1, 2, 8, 9, 16, 17, 21)] + ["sentinel n at a power of two, n == %d" % n for n in (1, 2, 256, 65536)]
    + ["skip: u < 0", "skip: v < 0", "skip: u == n", "skip: v == n", "skip: u == 2^40", "skip: low 32 bits in range", "skip: one bad endpoint, source",
       "skip: one bad endpoint, target", "every column skipped"]
    + ["E == %d" % e for e in (1, 255, 256, 257)] + ["nnz == %d" % z for z in (254, 256, 258)]
    + ["widen n + 1 == 256", "widen n + 1 == 257", "roots n == 256", "roots n == 257"]
    + ["column repeated both ways", "repeated self loop", "isolated vertex 0", "isolated vertex n - 1", "run of equal indptr", "row of >= 3000 entries"]
    + ["k == %d: %s" % (k, c) for k in (2, 3, 32) for c in P.ROOT_CLASSES]
    + ["k == 1", "k <= 0", "n < k", "level 0", "level 1", "level 2", "k > 32", "k > 32: root reaches", "k > 32: root does not reach"]
)
ASSEMBLY_CLASSES = ["device piece: identity column map", "device piece: non-identity column map", "host piece: graph held by the LRU",
                    "host piece: graph without columns", "degenerate graph"]
# classes no input can reach, with the reason (DESIGN.md section 9 repeats them)
UNREACHABLE = {
    "nnz odd": "every kept column leaves two entries, so pre_entries never sees 255 or 257 of them: its block edge is pinned at 254, 256 and 258",
}


def test_constants_are_the_sources():
    # the law and the model restate these; if the sources' move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_preproc.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "ugs_device.h")) as f:
        dev = f.read()
    with open(os.path.join(CSRC, "ugs_host.cpp")) as f:
        host = f.read()
    assert int(re.search(r"#define UGS_KMAX (\d+)", dev).group(1)) == L.KMAX
    kernels = re.findall(r"__global__ void __launch_bounds__\((\d+)\) (\w+)\(", hip)
    assert [k for _, k in kernels] == ["pre_keys", "pre_entries", "pre_widen", "pre_roots", "pre_assemble"]
    assert all(int(b) == L.BLOCK for b, _ in kernels) and hip.count("blockIdx.x * %d + threadIdx.x" % L.BLOCK) == 5
    assert "return (unsigned)((items + %d) / %d);" % (L.BLOCK - 1, L.BLOCK) in hip
    assert "int32_t got[UGS_KMAX];" in hip
    assert "while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)n) ++bits;" in hip
    assert "const bool ok = (uint64_t)u < (uint64_t)n && (uint64_t)v < (uint64_t)n;" in hip
    assert "for (int32_t h = 0; h < cnt && cnt < k; ++h) {" in hip and "p < e && cnt < k; ++p) {" in hip
    assert "if (k > UGS_KMAX) return UGS_OK;" in host                       # the guard that keeps a larger k off pre_roots
    assert "if (!forced && E < ((int64_t)1 << 21)) return UGS_OK;" in host and L.DEFAULT_MIN_COLS == 1 << 21
    assert [L.key_bits(n) for n in (1, 2, 3, 4, 255, 256, 257, 65535, 65536, (1 << 20) + 1, (1 << 30) - 2)] == [1, 2, 2, 3, 8, 9, 9, 16, 17, 21, 30]


# ---- the law against the oracle and the host path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_law_equals_the_oracles_preprocessing(name):
    c, law = P.case(name), P.law_of(name)
    pre = oracle.Preproc(c.ei, c.n, c.k)
    d, info = pre.dump(), pre.info()
    pre.close()
    for f in DUMP_FIELDS:
        assert d[f].dtype == law[f].dtype and np.array_equal(d[f], law[f]), (name, f)      # bucket_b: doubles compared exactly
    assert d["Z"] == law["Z"] and info["bucket_count_nonzero"] == law["nonzero"] and info["num_edges_stored"] == len(law["indices"]), name
    assert all(info[x] == y for x, y in L.info_of(law).items()), name
    assert (law["level"] == 0) == info["has_graphlets"], name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_law_equals_the_host_path(name):
    import torch
    import ugs_sampler
    c, law = P.case(name), P.law_of(name)
    old = os.environ.get("UGS_DEVICE_PREPROC")
    os.environ["UGS_DEVICE_PREPROC"] = "0"
    try:
        s0 = ugs_sampler.preproc_stats()
        h = ugs_sampler.create_preproc(torch.from_numpy(c.ei), c.n, c.k)
        s1 = ugs_sampler.preproc_stats()
    finally:
        if old is None:
            os.environ.pop("UGS_DEVICE_PREPROC", None)
        else:
            os.environ["UGS_DEVICE_PREPROC"] = old
    d, info = ugs_sampler.preproc_dump(h), ugs_sampler.get_preproc_info(h)
    ugs_sampler.destroy_preproc(h)
    assert {x: s1[x] - s0[x] for x in s0} == {"device_graphs": 0, "host_graphs": 1, "device_pieces": 0}, name
    for f in DUMP_FIELDS:
        assert np.array_equal(d[f], law[f]), (name, f)
    assert info == L.info_of(law), name


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_law_equals_the_oracle_on_the_assembly_graphs(name):
    b = P.batch(name)
    ei, ptr = P.batch_arrays(b)
    for g in range(len(b.graphs)):
        n, e, _ = P.local_graph(ei, ptr, g)
        if n < b.k:
            continue
        law = L.graph_law(e, n, b.k)
        pre = oracle.Preproc(e, n, b.k)
        d = pre.dump()
        pre.close()
        for f in DUMP_FIELDS:
            assert np.array_equal(d[f], law[f]), (name, g, f)


# ---- census --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes(name):
    c, census = P.case(name), P.census_of(name)
    assert c.reaches
    for cls in c.reaches:
        assert cls in CLASSES or cls.startswith("k == 5: "), cls
        assert census[cls] > 0, (name, cls, dict(census))
    assert L.takes_device_path(c.n, c.ei.shape[1], c.k) == (c.k <= L.KMAX), name


@pytest.mark.parametrize("cls", CLASSES)
def test_census_covers_every_class(cls):
    assert sum(P.census_of(name)[cls] for name in CASE_NAMES) > 0, cls


def test_unreachable_classes_stay_unreached():
    for cls in UNREACHABLE:
        assert sum(P.census_of(name)[cls] for name in CASE_NAMES) == 0, cls


def test_assembly_batches_hold_every_kind_of_piece():
    kinds = {b.name: P.batch_census(b) for b in P.batches()}
    assert kinds["assembly_in_order"] == ["device piece: identity column map", "host piece: graph held by the LRU", "host piece: graph without columns",
                                          "degenerate graph", "device piece: non-identity column map"]
    assert kinds["assembly_shuffled"] == ["device piece: non-identity column map", "host piece: graph held by the LRU", "device piece: non-identity column map"]
    assert set(ASSEMBLY_CLASSES) == set(sum(kinds.values(), []))


# ---- device model ----------------------------------------------------------------------------------------------------------------------
def model_differs(name, mutant=None):
    """does the model leave anything but the law's values on the case?  (an IndexError is a write outside an array)"""
    c, law = P.case(name), P.law_of(name)
    try:
        m = DM.preprocess(c.ei, c.n, c.k, L.degree_order, mutant)
    except IndexError:
        return True
    if any(not np.array_equal(m[f], law[f]) for f in ("indptr", "indices", "edge_col", "order", "index_of", "suffix_deg", "reach")):
        return True
    return not np.array_equal(L.bucket_b(m["suffix_deg"], m["reach"], c.k), law["bucket_b"])


def assembly_differs(name, mutant=None):
    b = P.batch(name)
    ei, ptr = P.batch_arrays(b)
    for g, kind in enumerate(P.batch_census(b)):
        if not kind.startswith("device piece"):
            continue
        n, e, cm = P.local_graph(ei, ptr, g)
        law = L.graph_law(e, n, b.k)
        m = DM.preprocess(e, n, b.k, L.degree_order)
        got = DM.assemble(m["indices"], m["edge_col"], m["index_of"], m["indptr"], None if kind.endswith(" identity column map") else cm, mutant)
        want = L.plan_arrays(law, cm)
        if any(not np.array_equal(got[f], want[f]) for f in want):
            return True
    return False


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if P.case(n).k <= L.KMAX])
def test_device_model_equals_the_law(name):
    assert not model_differs(name)


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if P.case(n).k > L.KMAX])
def test_device_model_cannot_take_k_above_its_list(name):
    assert model_differs(name)                                              # pre_roots must not see these: the guard sends them to the host stages


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_assembly_model_equals_the_law(name):
    assert not assembly_differs(name)


# the input that tells each mutant from the law
KILLERS = {
    "bits_one_too_few": "kw_n256", "range_test_on_low_32_bits": "skip_kinds", "range_test_one_endpoint": "skip_kinds",
    "unstable_within_key": "repeated_both_ways", "entries_side_swapped": "E_1", "widen_stops_at_n": "E_1", "sdeg_rank_gt": "self_loops",
    "bfs_no_suffix_filter": "roots_k3", "bfs_no_seen_test": "roots_k3", "bfs_bound_le": "roots_k32", "row_scan_not_stopped": "roots_k32",
    "assemble_rank_of_row_vertex": "assembly_in_order", "assemble_colmap_ignored": "assembly_shuffled",
}


@pytest.mark.parametrize("mutant", DM.MUTANTS)
def test_a_named_input_tells_the_mutant_from_the_law(mutant):
    assert set(KILLERS) == set(DM.MUTANTS) and len(DM.MUTANTS) >= 13
    name = KILLERS[mutant]
    assert (assembly_differs if mutant.startswith("assemble_") else model_differs)(name, mutant), (mutant, name)


def test_mutants_show_where_the_census_says_they_must():
    # the sentinel's extra bit matters only at a power of two with a skipped column; every other key width loses a vertex's row
    assert all(model_differs(n, "bits_one_too_few") for n in ("kw_n1", "kw_n2", "kw_n256", "kw_n65536"))
    # the root-stage slips show at every k the roots inputs are built for, the overruns of the list only at k == KMAX
    for k in (2, 3, 32):
        assert model_differs("roots_k%d" % k, "bfs_no_suffix_filter") and model_differs("roots_k%d" % k, "bfs_no_seen_test") and model_differs("roots_k%d" % k, "sdeg_rank_gt")
        assert model_differs("roots_k%d" % k, "bfs_bound_le") == (k == L.KMAX) and model_differs("roots_k%d" % k, "row_scan_not_stopped") == (k == L.KMAX)
    # an identity map hides a dropped column map
    assert not assembly_differs("assembly_in_order", "assemble_colmap_ignored") or "non-identity" in " ".join(P.batch_census(P.batch("assembly_in_order")))


def test_design_names_every_case_and_mutant_killer():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    for name in CASE_NAMES + BATCH_NAMES + list(KILLERS.values()):
        assert "`%s`" % name in design, name
