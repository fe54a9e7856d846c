"""CPU checks of the edge phase's restatement (tests/fill_law.py), the inputs chosen by its census (tests/fill_paths.py) and the
device model of the fill kernels with its mutants (tests/fill_device_model.py): the law reproduces the oracle's edge outputs, the
numpy form equals the plain one, every census class is reached from the oracle's rows alone at 8 and at 64 lanes, the constants
are the kernels', the model equals the law and every mutant is told from it by some input (or is listed as equivalent, with the
reason, and shown to change nothing)."""
import os
import re

import numpy as np
import pytest

import fill_device_model as DM
import fill_law as L
import fill_paths as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
REF_MODES = ("sample", "graph", "global")
# every class some input must reach, per lane width (DESIGN.md section 4.3 names the path behind each)
CLASSES = [c for c in L.ROW_CLASSES + L.ROWS_CLASSES] + [f"{kc}, {t}" for kc in ("k <= 8", "k > 8") for t in L.T_CLASSES]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_law_reproduces_the_oracle(name):
    c = P.case(name)
    assert 3 <= int(np.diff(c.ptr).min()) and int(np.diff(c.ptr).max()) <= 120 and c.m <= 64 and c.k in (1, 2, 3, 7, 8, 9, 16, 32)
    for mode in REF_MODES:
        nodes, edge_index, edge_ptr, _, edge_src = P.oracle_of(name, mode)
        assert np.array_equal(nodes, P.rows_of(name)[0])                       # the rows do not depend on the mode
        assert same(P.law_of(name, mode), (edge_ptr, edge_index, edge_src)), (name, mode)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_numpy_form_equals_the_plain_law(name):
    c = P.case(name)
    graph = L.csr(c.ei, c.ptr)
    flat = DM.flat_csr(P.adjacency_of(name))
    assert all(np.array_equal(a, b) for a, b in zip(graph, flat))
    for permuted in (False, True):
        nodes = P.rows_of(name)[int(permuted)]
        for mode in L.MODES:
            assert same(L.edge_phase_np(c.ei, c.ptr, nodes, c.m, c.k, mode, graph=graph), P.law_of(name, mode, permuted)), (name, mode)
        rb, rc = c.m + 3, c.m
        part = np.where(nodes[rb:rb + rc] >= 0, nodes[rb:rb + rc] + 1000, -1)
        for mode in L.MODES:
            assert same(L.edge_phase_np(c.ei, c.ptr, part, c.m, c.k, mode, rb, 1000, graph=graph), P.law_of(name, mode, permuted, rb, rc, 1000))


def test_law_drops_foreign_columns_and_takes_the_first_of_duplicates():
    # columns that leave the batch, join two graphs or touch ids below ptr[0] give nothing; a self loop gives two equal entries
    ei = np.array([[2, 3, 9, 4, -1, 2, 3, 1], [3, 4, 2, 5, 2, 2, 2, 2]], np.int64)
    ptr = np.array([2, 5, 7], np.int64)
    adj = L.adjacency(ei, ptr)
    assert adj[2] == [(3, 0), (2, 5), (2, 5), (3, 6)] and adj[3] == [(2, 0), (4, 1), (2, 6)] and adj[4] == [(3, 1)] and adj[5] == adj[0] == []
    assert all(np.array_equal(a, b) for a, b in zip(L.csr(ei, ptr), DM.flat_csr(adj)))
    # a row with a vertex twice (no walk produces one): the member lookup names the first position, as the kernels' does
    eptr, eidx, esrc = L.edge_phase(ei, ptr, [[3, 2, 3]], 1, 3, "sample")
    assert eidx.tolist() == [[0, 0, 1, 1, 1, 1, 2, 2], [1, 1, 0, 1, 1, 0, 1, 1]] and esrc.tolist() == [0, 6, 0, 5, 5, 6, 0, 6]
    assert same(L.edge_phase_np(ei, ptr, [[3, 2, 3]], 1, 3, "sample"), (eptr, eidx, esrc))


def test_census_constants_are_the_kernels():
    # the census and the model restate these; if the kernels' move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_kernels.hip")) as f:
        hip = f.read()
    with open(os.path.join(CSRC, "ugs_device.h")) as f:
        dev = f.read()
    with open(os.path.join(CSRC, "ugs_host.cpp")) as f:
        host = f.read()
    with open(os.path.join(CSRC, "ugs_jobs.cpp")) as f:                     # begin_common and the packed step
        jobs = f.read()
    assert hip.count("for (uint32_t cb = 0; cb < T; cb += %d * GS) {" % L.SUB_CHUNKS) == 2
    assert hip.count("for (int u = 0; u < %d; ++u) {" % L.SUB_CHUNKS) >= 4 and hip.count("if (cb + u * GS >= T) break;") == 2
    assert "if (k <= %d) {" % L.LOOKUP_REGS in hip and "j += (ps[t] <= e) ? 1 : 0;" in hip and "j += (PS[t] <= e) ? 1 : 0;" in hip
    assert "0x%Xu /* matches no vertex and no idle lane */" % DM.SV_PAD in hip and "constexpr uint32_t kEmpty = 0x%Xu;" % DM.EMPTY in hip
    assert "hipLaunchKernelGGL((ugs_fill<%d, BLOCK>)" % L.GS_WIDE in hip and "hipLaunchKernelGGL((ugs_fill<%d, BLOCK>)" % L.GS_NARROW in hip
    assert "constexpr int GS = %d, GROUPS = BLOCK / GS;\n    static_assert(GROUPS == %d," % (L.GS_NARROW, L.TILE_ROWS) in hip
    assert "const long long nw = (long long)((a.row_count + %d) / %d);" % (L.SUM_ROWS - 1, L.SUM_ROWS) in hip
    assert "for (long long t0 = 0; t0 < tile; t0 += 8 * BLOCK) {" in hip and L.TRIP_TILES == 8 * 256
    assert "hipLaunchKernelGGL((ugs_fill_scan<BLOCK>)" in hip and "constexpr int BLOCK = 256, GROUPS = %d;" % L.TILE_ROWS in hip
    assert hip.count("if (grid > (int64_t)cus * %d) grid = (int64_t)cus * %d;" % (L.GRID_PER_CU, L.GRID_PER_CU)) == 3
    assert "write = 3 * (int64_t)tot <= a.packed_cap;" in hip and "if (l >= 0 && pos < a.ld) {" in hip
    assert "#define UGS_STAGE_ITEMS %d " % L.STAGE_ITEMS in dev
    assert "!dyn && row_count <= %d && !capturing(s)" % L.FUSED_MAX_ROWS in host
    assert "j->rows <= %d && tc0.first == UGS_TIER_S" % L.FUSED_MAX_ROWS in jobs
    assert "const int64_t cap3_want = 3 * j->rows * 2 * (int64_t)k * (int64_t)(k - 1);" in jobs
    assert "cap3_want * (int64_t)sizeof(int64_t) <= ((int64_t)192 << 20)" in jobs and L.PACKED_STAGING_BYTES == 192 << 20
    assert "j->packed_ok = 3 * j->total <= cap3;" in jobs


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_case_reaches_its_classes_by_the_oracles_rows(name):
    c = P.case(name)
    for GS, reaches in ((L.GS_NARROW, c.reaches8), (L.GS_WIDE, c.reaches64)):
        census = P.census_of(name, GS)
        for cls in reaches:
            assert cls in CLASSES, cls
            assert census[cls] > 0, (name, GS, cls, dict(census))
        assert not any(census[cls] for cls in L.IMPOSSIBLE)


@pytest.mark.parametrize("GS", [L.GS_NARROW, L.GS_WIDE])
@pytest.mark.parametrize("cls", CLASSES)
def test_census_covers_every_class(cls, GS):
    assert sum(P.census_of(name, GS)[cls] for name in P.CASE_NAMES) > 0, (cls, GS)


def test_packed_batches_sit_on_both_sides_of_the_bound():
    import oracle
    for name, over in (("at_bound", 0), ("above_bound", 16)):
        ei, ptr, m, k = P.packed_batch(name)
        nodes, _, edge_ptr, _, _ = oracle.sample_batch(ei, ptr, m, k, "sample", 3)
        assert (nodes >= 0).all() and L.may_pack(len(nodes), k)
        assert 3 * int(edge_ptr[-1]) == L.packed_words(len(nodes), k) + 3 * over          # 1280 entries = the bound; 1296


def test_fused_row_counts():
    counts = P.fused_row_counts(256)
    assert {c % 8 for c in counts} == set(range(8)) and {-(-c // 8) % 4 for c in counts if c < 100} == {0, 1, 2, 3}
    assert {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65536, 65537, 65569, 131072, 131073} <= set(counts)
    assert L.fused_tiles(65536) == 2048 == L.fused_grid(65536, 256) and L.fused_tiles(65537) == 2049 and L.fused_tiles(65569) == 2050
    assert max(counts) <= P.FUSED_GRAPHS * P.FUSED_M
    assert set(P.fused_row_counts(304)) >= {65536, 65537, 8 * 304 * 32, 8 * 304 * 32 + 1}   # another CU count moves the stride's edge only


# ---- the device model -------------------------------------------------------------------------------------------------------------
def fill_configs(name):
    """(permuted, GS, mode, row_begin, row_count, extra, ld) for one case: both lane widths, every mode, a range that crosses a graph
    boundary with an offset, and capacities below the total"""
    c = P.case(name)
    out = []
    for GS in (L.GS_NARROW, L.GS_WIDE):
        for i, mode in enumerate(L.MODES):
            out.append((bool(i % 2), GS, mode, 0, None, 0, None))
        out.append((False, GS, "batch", c.m + 3, c.m, 0, None))
        out.append((True, GS, "graph", c.m + 3, c.m, 1000, None))
        out.append((False, GS, "global", c.m - 1, 2, 1000, None))
        for what, ld in P.capacities(name, GS).items():
            if what != "total":
                out.append((False, GS, "sample", 0, None, 0, ld))
    return out


def run_model(name, cfg, mutant=None):
    permuted, GS, mode, rb, rc, extra, ld = cfg
    c = P.case(name)
    law = P.law_of(name, mode, permuted, rb, rc, extra)
    nodes = P.rows_of(name)[int(permuted)]
    part = nodes[rb:] if rc is None else nodes[rb:rb + rc]
    part = np.where(part >= 0, part + extra, part)
    graph = DM.flat_csr(P.adjacency_of(name))
    out = DM.model_fill(graph, len(c.ptr) - 1, part, law[0], c.m, c.k, GS, int(law[0][-1]) if ld is None else ld, mode, rb, extra, mutant,
                        reverse=permuted)                 # (the rows in one order for the oracle's rows, in the other for the permuted ones)
    return DM.agrees(out, law)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_fill_model_equals_the_law(name):
    for cfg in fill_configs(name):
        assert run_model(name, cfg), (name, cfg)


# the case whose rows can tell the mutant from the kernel: tried first, then every other one
FILL_KILLERS = {"row_of_entry_lt": "small_k3", "sub_break_early": "small_k3", "prefix_includes_own_lane": "small_k2", "w_off_by_lanes": "small_k2",
                "capacity_le": "small_k3", "graph_mode_row": "small_k2", "batch_mode_absolute_row": "small_k2", "sv_pad_is_empty": "small_k3",
                "chunk_of_3_sub_chunks": "small_k8", "sub_break_gt": "small_k3"}


def fill_mutant_differs(mutant, names):
    return any(not run_model(name, cfg, mutant) for name in names for cfg in fill_configs(name))


@pytest.mark.parametrize("mutant", DM.FILL_MUTANTS)
def test_some_input_tells_the_fill_mutant_from_the_law(mutant):
    assert set(FILL_KILLERS) == set(DM.FILL_MUTANTS)
    first = FILL_KILLERS[mutant]
    if mutant in DM.EQUIVALENT:
        assert not fill_mutant_differs(mutant, [first, "small_k16", "k8_cliques"]), DM.EQUIVALENT[mutant]
        return
    assert fill_mutant_differs(mutant, [first]) or fill_mutant_differs(mutant, [n for n in P.CASE_NAMES if n != first]), mutant


# ---- the scan folded into the fill ---------------------------------------------------------------------------------------------
def fused_counts(rows, seed=42):
    return np.diff(P.fused_reference("sample", seed)[1])[:rows].tolist()


def scan_agrees(counts, rows, cus, packed_cap=0, lanes=8, mutant=None):
    eptr, h_total, write = DM.model_fill_scan(counts, rows, cus, packed_cap, lanes, mutant)
    want = np.concatenate([[0], np.cumsum(counts[:rows])]).tolist()
    ok = eptr == want
    if packed_cap:
        ok = ok and h_total == want[-1] and write == (3 * want[-1] <= packed_cap)
    return ok


SMALL_ROWS = [r for r in P.fused_row_counts(256) if r < 100] + [257, 300]


def test_scan_model_equals_the_law():
    counts = fused_counts(131073)
    for rows in SMALL_ROWS:
        for lanes in (8, 16):
            for cus in (1, 256):                                             # one CU: 8 blocks, the tile loop strides
                assert scan_agrees(counts, rows, cus, 0, lanes), (rows, lanes, cus)
                total = sum(counts[:rows])
                for cap in (3 * total, 3 * total - 1, 3 * total + 1):
                    assert scan_agrees(counts, rows, cus, cap, lanes), (rows, lanes, cus, cap)
    for rows in (r for r in P.fused_row_counts(256) if 100 < r <= L.FUSED_MAX_ROWS):
        assert scan_agrees(counts, rows, 256, 0), rows
        assert scan_agrees(counts, rows, 256, 3 * sum(counts[:rows])), rows


@pytest.mark.parametrize("name", sorted(P.PACKED))
def test_models_on_the_packed_batches(name):
    import oracle
    ei, ptr, m, k = P.packed_batch(name)
    nodes = oracle.sample_batch(ei, ptr, m, k, "global", 3)[0]
    law = L.edge_phase(ei, ptr, nodes, m, k, "graph")
    counts, cap = np.diff(law[0]).tolist(), L.packed_words(len(nodes), k)
    eptr, h_total, write = DM.model_fill_scan(counts, len(nodes), 256, cap)
    assert eptr == law[0].tolist() and h_total == int(law[0][-1]) and write == (name == "at_bound")
    assert not DM.model_fill_scan(counts, len(nodes), 256, cap, mutant="write_lt")[2]          # at the bound only `<=` stages
    out = DM.model_fill(DM.flat_csr(L.adjacency(ei, ptr)), len(ptr) - 1, nodes, law[0], m, k, L.GS_NARROW, int(law[0][-1]), "graph")
    assert DM.agrees(out, law)


# (rows, cus, packed, lanes) that tells the mutant from the kernel
SCAN_KILLERS = {"before_le_tile": (33, 256, False, 8), "trip_2047": (65569, 256, False, 8), "trip_2049": (65569, 256, False, 8),
                "tail_words_dropped": (44, 256, True, 8), "tile_stride_plus_1": (65537, 256, False, 8), "tile_stride_minus_1": (65569, 256, False, 8),
                "write_lt": (32, 256, True, 8), "sums_of_7_rows": (33, 256, False, 8), "wide_sums_one_wave": (33, 256, False, 16)}


@pytest.mark.parametrize("mutant", DM.SCAN_MUTANTS)
def test_some_row_count_tells_the_scan_mutant_from_the_law(mutant):
    assert set(SCAN_KILLERS) == set(DM.SCAN_MUTANTS)
    rows, cus, packed, lanes = SCAN_KILLERS[mutant]
    assert rows in P.fused_row_counts(256)                                   # the GPU test runs this count
    counts = fused_counts(131073)
    cap = 3 * sum(counts[:rows]) if packed else 0
    assert scan_agrees(counts, rows, cus, cap, lanes)
    if mutant in DM.EQUIVALENT:
        assert scan_agrees(counts, rows, cus, cap, lanes, mutant), DM.EQUIVALENT[mutant]
        assert scan_agrees(counts, 300, 1, cap and 3 * sum(counts[:300]), lanes, mutant)
    else:
        assert not scan_agrees(counts, rows, cus, cap, lanes, mutant), mutant


def test_trip_mutants_need_the_second_trip():
    # no row count up to 65 536 -- the largest fused call the suite ran before -- can see a wrong trip step or stride
    counts = fused_counts(65536)
    for mutant in ("trip_2047", "trip_2049", "tile_stride_plus_1"):
        assert scan_agrees(counts, 65536, 256, 0, 8, mutant), mutant
