"""The edge phase's kernels path by path: fill_row inside ugs_fill<8> and ugs_fill<64>, the scan folded into the fill
(ugs_fill_scan<8>) and its packed form behind sample_batch, against tests/fill_law.py -- everything compared is an integer and
compared exactly.

The inputs live in tests/fill_paths.py; tests/test_fill_law.py asserts on the CPU, from the oracle's rows alone, which path every
row takes (chunk and sub-chunk boundaries, ballots, register and LDS lookup) and shows on a model of the kernels that these
inputs tell each modelled slip from the law.  Which kernel ran is asserted through Plan.last_fill(); whether the packed step
staged or refused through ugs_sampler.step_stats()."""
import numpy as np
import pytest
import torch

import fill_law as L
import fill_paths as P

pytestmark = pytest.mark.gpu

GUARD = -7
NARROW, WIDE, SCAN = "ugs_fill<8>", "ugs_fill<64>", "ugs_fill_scan<8>"


def ugs():
    import ugs_sampler
    torch.cuda.set_device(0)
    return ugs_sampler


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()            # (a copy: the shared references are read-only)


def plan_of(ei, ptr, k, monkeypatch=None, force_wide=False):
    """A plan in its own tier, or in the 448-candidate 64-lane tier (the tier is chosen once per plan and k: a fresh cache first)."""
    u = ugs()
    u.clear_cache()
    if force_wide:
        monkeypatch.setenv("UGS_FORCE_TIER", "1")
    plan = u.Plan.from_batch(torch.from_numpy(np.array(ei)), torch.from_numpy(np.array(ptr)), k)
    if force_wide:
        assert plan.info()["tier"] == 1
    return plan


def fill_kernel(plan):
    return NARROW if plan.info()["tier"] == 0 else WIDE


def guarded(ld):
    """edge_index [2, ld] and edge_src [ld] of exactly ld entries, with guard words behind both"""
    gi = torch.full((2 * ld + 64,), GUARD, dtype=torch.int64, device="cuda")
    gs = torch.full((ld + 64,), GUARD, dtype=torch.int64, device="cuda")
    return gi, gs, (gi[:2 * ld].view(2, ld), gs[:ld])


def assert_edges(gi, gs, ld, law, what):
    """entries below ld equal the law's, the guard words behind both buffers keep their value"""
    n = min(int(law[0][-1]), ld)
    gi, gs = gi.cpu().numpy(), gs.cpu().numpy()
    assert np.array_equal(gi[:n], law[1][0, :n]) and np.array_equal(gi[ld:ld + n], law[1][1, :n]), (what, "edge_index")
    assert np.array_equal(gs[:n], law[2][:n]), (what, "edge_src")
    assert (gi[2 * ld:] == GUARD).all() and (gs[ld:] == GUARD).all(), (what, "guard words")
    if n < ld:
        assert (gi[n:ld] == GUARD).all() and (gi[ld + n:2 * ld] == GUARD).all() and (gs[n:ld] == GUARD).all(), (what, "beyond the total")


def fill_alone(plan, m, nodes, law, mode, row_begin=0, extra=0, ld=None, what=""):
    """Plan.fill on a FRESH nodes tensor (not the last walk's buffer: the staged path is out) with the law's edge_ptr"""
    ld = int(law[0][-1]) if ld is None else ld
    gi, gs, out = guarded(ld)
    plan.fill(m, dev(nodes), dev(law[0]), ld, mode, row_begin, extra, out=out)
    torch.cuda.synchronize()
    assert_edges(gi, gs, ld, law, (what, mode, row_begin, extra, ld))


def run_fill_case(name, plan, kernel):
    c = P.case(name)
    rows = len(P.rows_of(name)[0])
    for permuted in (False, True):
        nodes = P.rows_of(name)[int(permuted)]
        for mode in L.MODES:
            fill_alone(plan, c.m, nodes, P.law_of(name, mode, permuted), mode, what=(name, permuted))
            assert plan.last_fill()["kernel"] == kernel
        # a range whose rows lie in two graphs (row / m crosses a graph boundary inside the call), with a node offset
        rb, rc = c.m + 3, min(c.m, rows - c.m - 3)
        for mode in L.MODES:
            part = np.where(nodes[rb:rb + rc] >= 0, nodes[rb:rb + rc] + 1000, -1)
            fill_alone(plan, c.m, part, P.law_of(name, mode, permuted, rb, c.m, 1000), mode, rb, 1000, what=(name, permuted, "range"))
    assert plan.last_fill()["block"] == 256 and plan.last_fill()["grid"] >= 1


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_fill_alone_in_the_plans_own_tier(name):
    c = P.case(name)
    for cls in c.reaches8:
        assert P.census_of(name, L.GS_NARROW)[cls] > 0, f"the input no longer reaches {cls!r}: choose it again"
    plan = plan_of(c.ei, c.ptr, c.k)
    if name != "wide_k16":                                   # (graphs of 70 and 120 vertices: the plan may choose a 64-lane tier itself)
        assert plan.info()["tier"] == 0
    run_fill_case(name, plan, fill_kernel(plan))
    plan.close()


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_fill_alone_with_64_lanes_per_row(name, monkeypatch):
    c = P.case(name)
    for cls in c.reaches64:
        assert P.census_of(name, L.GS_WIDE)[cls] > 0, f"the input no longer reaches {cls!r}: choose it again"
    plan = plan_of(c.ei, c.ptr, c.k, monkeypatch, force_wide=True)
    run_fill_case(name, plan, WIDE)
    plan.close()


@pytest.mark.parametrize("wide", [False, True])
def test_fill_of_a_one_graph_plan(wide, monkeypatch):
    """num_graphs == 1: the kernels skip row / m (graph mode numbers by the row itself)"""
    import oracle
    ei, ptr = P.one_graph()
    m, k = 40, 5
    nodes = np.ascontiguousarray(oracle.sample_batch(ei, ptr, m, k, "global", 11)[0], dtype=np.int64)
    assert (nodes >= 0).all()
    plan = plan_of(ei, ptr, k, monkeypatch, force_wide=wide)
    assert plan.info()["num_graphs"] == 1
    for mode in L.MODES:
        fill_alone(plan, m, nodes, L.edge_phase(ei, ptr, nodes, m, k, mode), mode, what="one graph")
        part = nodes[7:31] + 5
        fill_alone(plan, m, part, L.edge_phase(ei, ptr, part, m, k, mode, 7, 5), mode, 7, 5, what="one graph, range")
        assert plan.last_fill()["kernel"] == (WIDE if wide else NARROW)
    plan.close()


def test_fill_64_above_its_grid_bound(monkeypatch):
    """More rows than ugs_fill<64>'s capped grid has groups (8 blocks per CU, 4 rows per block): the grid-stride loop's second trip.
    Every graph's rows repeated, m_per_graph grown by the same factor, so that row / m still names the row's graph."""
    c = P.case("small_k3")
    G = len(c.ptr) - 1
    reps = -(-(L.GRID_PER_CU * cus() * 4 + 1) // (G * c.m)) + 1
    nodes = np.tile(P.rows_of("small_k3")[1].reshape(G, c.m, c.k), (1, reps, 1)).reshape(-1, c.k)
    assert len(nodes) > L.GRID_PER_CU * cus() * 4
    plan = plan_of(c.ei, c.ptr, c.k, monkeypatch, force_wide=True)
    for mode in ("graph", "batch"):
        fill_alone(plan, c.m * reps, nodes, L.edge_phase_np(c.ei, c.ptr, nodes, c.m * reps, c.k, mode), mode, what="repeated rows")
        assert plan.last_fill() == {"kernel": WIDE, "grid": L.GRID_PER_CU * cus(), "block": 256}
    plan.close()


# ---- (b) capacity ---------------------------------------------------------------------------------------------------------------
CAPACITY_CASES = ("small_k3", "small_k16", "hits_k8", "hits_k9")


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", CAPACITY_CASES)
def test_capacity_of_the_row_reading_fill(name, wide, monkeypatch):
    c = P.case(name)
    caps = P.capacities(name, L.GS_WIDE if wide else L.GS_NARROW)
    assert {"total", "total - 1", "inside a row", "inside a ballot", "1"} == set(caps)
    plan = plan_of(c.ei, c.ptr, c.k, monkeypatch, force_wide=wide)
    for what, ld in caps.items():
        fill_alone(plan, c.m, P.rows_of(name)[0], P.law_of(name, "sample"), "sample", ld=ld, what=(name, what))
        assert plan.last_fill()["kernel"] == (WIDE if wide else NARROW)
    plan.close()


@pytest.mark.parametrize("name", CAPACITY_CASES)
def test_capacity_of_the_fused_step(name):
    c = P.case(name)
    plan = plan_of(c.ei, c.ptr, c.k)
    nodes_want, law = P.rows_of(name)[0], P.law_of(name, "sample")
    rows = len(nodes_want)
    for what, ld in P.capacities(name, L.GS_NARROW).items():
        gi, gs, out = guarded(ld)
        nodes = torch.full((rows, c.k), GUARD, dtype=torch.int64, device="cuda")
        eptr = torch.full((rows + 1,), GUARD, dtype=torch.int64, device="cuda")
        plan.step(c.m, "sample", c.seed, out=(nodes, eptr) + out)
        torch.cuda.synchronize()
        assert plan.last_fill()["kernel"] == SCAN
        assert np.array_equal(nodes.cpu().numpy(), nodes_want) and np.array_equal(eptr.cpu().numpy(), law[0]), (name, what)   # the true total
        assert_edges(gi, gs, ld, law, (name, what))
    plan.close()


@pytest.mark.parametrize("name", CAPACITY_CASES)
def test_capacity_of_the_staged_fill(name, monkeypatch):
    """walk-then-fill on the walk's own buffers in a one-walk-per-wave tier: rows of at most 32 hits are expanded from the walk's
    staging (ugs_fill_staged), the others are read again by ugs_fill<64>, which is the kernel the call reports"""
    c = P.case(name)
    plan = plan_of(c.ei, c.ptr, c.k, monkeypatch, force_wide=True)
    law = P.law_of(name, "sample")
    for what, ld in P.capacities(name, L.GS_WIDE).items():
        nodes, eptr, total = plan.walk(c.m, "sample", c.seed)
        assert total == int(law[0][-1]) and np.array_equal(nodes.cpu().numpy(), P.rows_of(name)[0]) and np.array_equal(eptr.cpu().numpy(), law[0])
        gi, gs, out = guarded(ld)
        plan.fill(c.m, nodes, eptr, ld, "sample", out=out)
        torch.cuda.synchronize()
        assert plan.last_fill()["kernel"] == WIDE
        assert_edges(gi, gs, ld, law, (name, what))
    plan.close()


# ---- (c) the scan folded into the fill -----------------------------------------------------------------------------------------
SEED = 42
REF_MODES = ("sample", "graph", "global")


def step_equals_reference(plan, mode, rb, rc, what):
    want = P.fused_slice(mode, SEED, rb, rc)
    total = int(want[1][-1])
    nodes, eptr, eidx, esrc = plan.step(P.FUSED_M, mode, SEED, rb, rc, edge_capacity=total + 7)
    assert torch.equal(nodes, dev(want[0])), (what, "nodes")
    assert torch.equal(eptr, dev(want[1])), (what, "edge_ptr")
    assert torch.equal(eidx[:, :total], dev(want[2])) and torch.equal(esrc[:total], dev(want[3])), (what, "edges")


def test_fused_scan_at_every_row_count(monkeypatch):
    """Plan.step at row counts chosen for the scan's paths, largest first on ONE plan -- every call finds the sum words of a larger
    call behind its own in the scratch.  The counts from 65 536 up are written for the MI355X's 256 CUs and computed from the
    device's CU count (fill_paths.fused_row_counts): the second trip of the `before` loop, the tile loop's second stride, the
    last fused count and the hand-over to the three-launch form."""
    ei, ptr = P.fused_batch()
    plan = plan_of(ei, ptr, P.FUSED_K)
    rows_all = P.FUSED_GRAPHS * P.FUSED_M
    wide_max = cus() * 3 * 16                                # rows up to which the 16-lane walk is taken
    for it, rc in enumerate(sorted(P.fused_row_counts(cus()), reverse=True)):
        mode = REF_MODES[it % 3]
        rb = 2 * P.FUSED_M - rc // 2 if rc < 100 else min(rows_all - rc, 100)                 # small ranges cross a graph boundary
        for narrow in ((False, True) if rc <= wide_max else (False,)):
            if narrow:
                monkeypatch.setenv("UGS_NO_WIDE_TIER", "1")
            else:
                monkeypatch.delenv("UGS_NO_WIDE_TIER", raising=False)
            step_equals_reference(plan, mode, rb, rc, (rc, rb, mode, narrow))
            walk = plan.last_launch()["kernel"]
            assert walk.startswith("ugs_walk_lds<16," if rc <= wide_max and not narrow else "ugs_walk_lds<8,"), (rc, walk)
            fill = plan.last_fill()
            if rc <= L.FUSED_MAX_ROWS:
                assert fill == {"kernel": SCAN, "grid": L.fused_grid(rc, cus()), "block": 256}, (rc, fill)
            else:
                assert fill["kernel"] == NARROW, (rc, fill)
    plan.close()


def test_three_launch_form_behind_the_same_call(monkeypatch):
    ei, ptr = P.fused_batch()
    plan = plan_of(ei, ptr, P.FUSED_K)
    monkeypatch.setenv("UGS_NO_FUSED_SCAN", "1")
    for it, rc in enumerate((L.TRIP_TILES * L.TILE_ROWS + 1, 33, 7)):
        step_equals_reference(plan, REF_MODES[it], 3, rc, ("unfused", rc))
        assert plan.last_fill()["kernel"] == NARROW
    monkeypatch.delenv("UGS_NO_FUSED_SCAN")
    step_equals_reference(plan, "graph", 3, 33, ("fused again", 33))
    assert plan.last_fill()["kernel"] == SCAN
    plan.close()


# ---- (d) the packed step ----------------------------------------------------------------------------------------------------------
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def sample_batch_equals_oracle(ei, ptr, m, k, mode, seed, what):
    import oracle
    u = ugs()
    want = oracle.sample_batch(ei, ptr, m, k, mode, seed)
    moved = []
    for device in (None, "cuda:0"):
        before = u.step_stats()
        got = u.sample_batch(torch.from_numpy(np.array(ei)), torch.from_numpy(np.array(ptr)), m, k, mode=mode, seed=seed, device=device)
        after = u.step_stats()
        moved.append((after["packed_staged"] - before["packed_staged"], after["packed_refused"] - before["packed_refused"]))
        for nm, a, b in zip(NAMES, got, want):
            assert a.is_cuda == (device is not None)
            a = a.cpu().numpy()
            assert a.shape == np.asarray(b).shape and np.array_equal(a, b), (what, device, nm)
    return moved


@pytest.mark.parametrize("mode", REF_MODES)
def test_packed_step_on_both_sides_of_its_bound(mode):
    """Complete graphs on exactly k vertices with both directions as columns: every row holds 2 k (k - 1) entries, 3 * total ==
    packed_cap -- the kernel stages.  One column repeated: 16 entries more, the kernel writes nothing and finish fills."""
    ugs().clear_cache()
    ei, ptr, m, k = P.packed_batch("at_bound")
    assert sample_batch_equals_oracle(ei, ptr, m, k, mode, 3, "at the bound") == [(1, 0), (1, 0)]
    ei, ptr, m, k = P.packed_batch("above_bound")
    assert sample_batch_equals_oracle(ei, ptr, m, k, mode, 3, "above the bound") == [(0, 1), (0, 1)]


def test_packed_step_at_the_staging_limit():
    """k = 7: 84 entries per row bound the staging, and 192 MB of it are reached at 99 864 rows, below the fused scan's 131 072 --
    the last row count whose step may pack and the first whose may not (begin_common's formula, fill_law.may_pack)."""
    import ugs_workloads as wl
    k = 7
    last = L.PACKED_STAGING_BYTES // (8 * L.packed_words(1, k))
    assert L.may_pack(last, k) and not L.may_pack(last + 1, k) and last + 1 < L.FUSED_MAX_ROWS
    ugs().clear_cache()
    for rows, want in ((last, (1, 0)), (last + 1, (0, 0))):
        G = next(g for g in range(2, 256) if rows % g == 0)
        ei, ptr = wl.tu_batch(12, 14, G)
        moved = sample_batch_equals_oracle(ei, ptr, rows // G, k, "sample", 5, rows)
        assert moved == [want, want], (rows, moved)
