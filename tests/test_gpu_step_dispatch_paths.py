"""GPU: every dispatch class of a growth step of the 448-candidate tier (tests/step_dispatch_paths.py; the CPU test
tests/test_step_dispatch_law.py asserts that these inputs reach every class), all four outputs against the CPU oracle, in modes
"sample" and "global".  One graph with k = 8, 2 and 3 (the launch-uniform instantiation, which reads its graph's descriptor once per
kernel), a two-graph batch and a batch with a degenerate graph (the instantiation that reads it per walk), the same single graph
read through row pointers (UGS_NO_PROW: the plan without padded rows) and with enough rows for the dynamic work loop."""
import numpy as np
import pytest
import torch

import oracle
import step_dispatch_paths as sdp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

MODES = ("sample", "global")


def _check(name, monkeypatch, m=None, seed=42):
    import ugs_sampler
    monkeypatch.setenv("UGS_FORCE_TIER", "1")                              # the 448-candidate tier, one walk per wave
    ei, ptr, k = sdp.cases()[name]
    for mode in MODES:
        ugs_sampler.clear_cache()
        if m is None:
            want = sdp.oracle_rows(name, mode, seed)
            got = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), sdp.ROWS // (len(ptr) - 1), k, mode, seed)
        else:
            want = oracle.sample_batch(ei, ptr, m, k, mode, seed)
            got = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode, seed)
        assert len(got) == len(want) >= 4
        for j, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a.numpy(), np.asarray(b)), f"{name}: output {j} differs (mode {mode}, k {k})"
    ugs_sampler.clear_cache()


@pytest.mark.parametrize("name", ["low", "mid", "high"])
def test_one_graph(name, monkeypatch):
    _check(name, monkeypatch)


@pytest.mark.parametrize("name", ["k2", "k3"])
def test_short_samples(name, monkeypatch):
    _check(name, monkeypatch)


def test_two_graph_batch(monkeypatch):
    _check("two_graphs", monkeypatch)


def test_batch_with_a_degenerate_graph(monkeypatch):
    _check("degenerate", monkeypatch)
    nodes = np.asarray(sdp.oracle_rows("degenerate")[0])
    m = sdp.ROWS // 3
    assert (nodes[m:2 * m] == -1).all() and (nodes[:m, 0] >= 0).all()


@pytest.mark.parametrize("name", ["mid", "two_graphs"])
def test_plan_without_padded_rows(name, monkeypatch):
    monkeypatch.setenv("UGS_NO_PROW", "1")
    _check(name, monkeypatch)


def test_dynamic_work_loop(monkeypatch):
    """more than 64 rows per compute unit: the launch-uniform walk in its dynamic work loop (the flagship's instantiation)"""
    import ugs_sampler
    rows = 20000
    _check("mid", monkeypatch, m=rows)
    ei, ptr, k = sdp.cases()["mid"]
    plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), k)
    plan.walk(rows, "sample", 42)
    name = plan.last_launch()["kernel"]
    plan.close()
    ugs_sampler.clear_cache()
    assert name == "ugs_walk_lds<64,448,draws>", name
