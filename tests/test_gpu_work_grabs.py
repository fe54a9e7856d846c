"""The walk kernel's grabs from the work counter (ugs_kernels.hip, the dynamic loop of ugs_walk_lds) against the CPU oracle, bit for bit.

A wave takes UGS_WORK_GRAB = 32 rows per counter trip while more than 64 rows per wave are left and works them off as sub-chunks
of four; which wave samples a row changes no output.  tests/work_grabs.py restates the schedule; tests/test_work_grabs_law.py proves
on the CPU that every row is handed out once and what each case below reaches.  Every call runs in the 448-candidate tier
(UGS_FORCE_TIER=1); the row counts come from the device's compute-unit count.

  (i)   the mixed batch of 49 152 rows on ONE block per compute unit (Plan.set_walk_share(5)): grabs of 32 by index and from the
        counter, then 4, 2, 1 -- k = 8 in the three modes, k = 5 (self hits beside parked rows), k = 9 (nothing parked)
  (ii)  one sparse graph, k = 4, every wave resident, 2 * 32 rows per wave plus 13 from row 12 345 on: the launch-uniform
        instantiation with lane-parallel draws takes its first grab of 32; the row count is odd
  (iii) the same call with the static split: the same tensors
  (iv)  ER of degree 40 at k = 12, more than 64 rows per compute unit: the 448-candidate tier hands rows on, and the launch that
        redoes them takes its rows from the list through the second counter"""
import numpy as np
import pytest

import row_epilogue_batches as reb
import scenarios as sc
import work_grabs as wg

_results = {}


@pytest.fixture(scope="module")
def orc():
    from backends import OracleBackend
    return OracleBackend()


@pytest.fixture(scope="module")
def batch():
    return reb.mixed_batch()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _call(ei, ptr, m, k, mode="sample", seed=42):
    return dict(fn="sample_batch", edge_index=ei, ptr=ptr, m=m, k=k, mode=mode, seed=seed)


def _oracle(orc, name, call):
    """the oracle's result of one call on a fresh cache, computed once per module"""
    if name not in _results:
        (res,) = sc.run_scenario([call], orc)
        assert isinstance(res, tuple) and not isinstance(res[0], str), repr(res)
        _results[name] = res
    return _results[name]


def _same(got, want, what):
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: output {j} differs"


def _plan_rows(ei, ptr, k, m, mode, seed, share=None, row_begin=0, row_count=None):
    """(nodes, edge_index, edge_ptr, edge_src) of Plan.sample_rows and the launch record of its walk"""
    import torch
    import ugs_sampler
    ugs_sampler.clear_cache()
    plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), k)
    if share is not None:
        plan.set_walk_share(share)
    nodes, eptr, total = plan.walk(m, mode, seed, row_begin, row_count)
    launch = plan.last_launch()
    eidx, esrc = plan.fill(m, nodes, eptr, total, mode, row_begin)
    got = tuple(t.cpu().numpy() for t in (nodes, eidx, eptr, esrc))
    plan.close()
    return got, launch


# (i) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("k,mode", [(8, "sample"), (8, "graph"), (8, "global"), (5, "sample"), (9, "sample")])
def test_mixed_batch_on_one_block_per_unit(k, mode, orc, batch, cus, monkeypatch):
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr, _ = batch
    seen = wg.sizes_reached(reb.ROWS, cus)
    assert wg.is_dynamic(reb.ROWS, cus) and wg.grab_for(reb.ROWS, cus) == wg.GRAB and all(seen.get(s, 0) > 0 for s in (wg.GRAB, 4, 2, 1)), seen
    want = _oracle(orc, f"mixed_k{k}_{mode}", _call(ei, ptr, reb.M, k, mode))
    got, launch = _plan_rows(ei, ptr, k, reb.M, mode, 42, share=5)
    assert launch["kernel"] == "ugs_walk_lds<64,448>" and launch["grid"] == cus, launch           # one one-wave block per unit
    _same(got, (want[0], want[1], want[2], want[4]), f"k={k} {mode}")


# (ii), (iii) ---------------------------------------------------------------------------------------------------------------
ROW_BEGIN = 12345


def _sparse_want(cus):
    name = f"sparse_k4_{cus}"
    if name not in _results:
        import oracle
        ei, ptr = reb.sparse_graph()
        rows = wg.full_residency_rows(cus)
        P = oracle.Preproc(ei, int(ptr[1]), 4)
        _results[name] = tuple(np.asarray(x) for x in P.sample(ROW_BEGIN + rows + 7, 4, "local", 0, 7, ROW_BEGIN, ROW_BEGIN + rows))
        P.close()
    return _results[name]


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("static", [False, True])
def test_single_graph_at_full_residency(static, cus, monkeypatch):
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    if static:
        monkeypatch.setenv("UGS_STATIC_SPLIT", "1")
    rows, groups = wg.full_residency_rows(cus), cus * wg.WAVES_PER_CU
    seen = wg.sizes_reached(rows, groups)
    assert wg.is_dynamic(rows, cus) and rows % 2 == 1 and seen[wg.GRAB] == groups and seen.get(4, 0) > 0 and seen.get(2, 0) > 0, seen
    ei, ptr = reb.sparse_graph()
    got, launch = _plan_rows(ei, ptr, 4, ROW_BEGIN + rows + 7, "sample", 7, row_begin=ROW_BEGIN, row_count=rows)
    assert launch["kernel"] == ("ugs_walk_lds<64,448>" if static else "ugs_walk_lds<64,448,draws>") and launch["grid"] == groups, launch
    _same(got, _sparse_want(cus), f"{rows} rows from {ROW_BEGIN}, static={static}")


# (iv) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_rows_handed_on_take_the_second_counter(cus, monkeypatch):
    # ER of degree 40 at k = 12: the plan starts in the 448-candidate tier by itself and a few per cent of its walks outgrow it
    import oracle
    import ugs_workloads as wl
    monkeypatch.delenv("UGS_FORCE_TIER", raising=False)
    n, k = 60000, 12
    m = max(40000, cus * wg.DYNAMIC_ABOVE_PER_CU + 1)
    assert wg.is_dynamic(m, cus)
    ei, ptr = wl.er_graph(n, 1_200_000, seed=11)
    got, launch = _plan_rows(ei, ptr, k, m, "sample", 5)
    assert launch["kernel"].startswith("ugs_walk_lds<64,448") and launch["overflow_rows"] > 0, launch
    P = oracle.Preproc(ei, n, k)
    want = P.sample(m, k, "local", 0, 5)
    P.close()
    _same(got, tuple(want), "handed-on rows")
