"""CPU: the switch that raises the device batch pass's column limit (ugs_set_batch_pass_max_cols; include/ugs_mi355.h) -- its
default, range and environment variable -- and the fixture of large-graph batches (tests/golden/f17_large_graph_batches.npz,
from the reference module) replayed on the CPU oracle, strided-key collision included."""
import os
import subprocess
import sys

import numpy as np
import pytest

import large_graphs as lg
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_setter_and_getter():
    import ugs_sampler
    assert "UGS_BATCH_PASS_MAX_COLS" not in os.environ
    assert ugs_sampler.batch_pass_max_cols() == 1000
    try:
        assert ugs_sampler.set_batch_pass_max_cols(8192) == 1000
        assert ugs_sampler.batch_pass_max_cols() == 8192
        assert ugs_sampler.set_batch_pass_max_cols(1200) == 8192
        assert ugs_sampler.set_batch_pass_max_cols(1000) == 1200
        assert ugs_sampler.batch_pass_max_cols() == 1000
    finally:
        ugs_sampler.set_batch_pass_max_cols(1000)


@pytest.mark.parametrize("bad", [999, 8193, 0, -1, -8192, 2 ** 40])
def test_out_of_range_is_the_argument_error_and_keeps_the_value(bad):
    import ctypes

    import ugs_sampler
    from ugs_sampler import _lib
    try:
        ugs_sampler.set_batch_pass_max_cols(4096)
        with pytest.raises(RuntimeError, match=r"1000 \.\.\. 8192"):
            ugs_sampler.set_batch_pass_max_cols(bad)
        assert ugs_sampler.batch_pass_max_cols() == 4096
        prev = ctypes.c_int64(-5)
        assert _lib.lib.ugs_set_batch_pass_max_cols(bad, ctypes.byref(prev)) == _lib.UGS_E_BAD_ARG
        assert prev.value == -5 and ugs_sampler.batch_pass_max_cols() == 4096
        assert _lib.lib.ugs_set_batch_pass_max_cols(2000, None) == 0 and ugs_sampler.batch_pass_max_cols() == 2000      # previous_out may be NULL
    finally:
        ugs_sampler.set_batch_pass_max_cols(1000)


def test_batch_pass_stats_keeps_its_two_keys():
    import ugs_sampler
    assert sorted(ugs_sampler.batch_pass_stats()) == ["device_plans", "general_path"]


@pytest.mark.parametrize("value, want", [("8192", 8192), ("1000", 1000), ("2700", 2700), ("999", 1000), ("8193", 1000), ("-4", 1000),
                                         ("lots", 1000), ("", 1000), ("4096x", 1000)])
def test_environment_variable_sets_the_initial_value(value, want):
    code = ("import os, sys\n"
            "sys.path[:0] = [os.path.join(os.getcwd(), 'ss-gnn_amd')]\n"
            "import ugs_sampler\n"
            "print('LIMIT', ugs_sampler.batch_pass_max_cols())\n"
            "print('PREV', ugs_sampler.set_batch_pass_max_cols(1500), ugs_sampler.batch_pass_max_cols())\n")
    env = dict(os.environ, UGS_BATCH_PASS_MAX_COLS=value, UGS_DEBUG="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f"LIMIT {want}\n" in out.stdout and f"PREV {want} 1500\n" in out.stdout, out.stdout
    ignored = "UGS_BATCH_PASS_MAX_COLS=" + value + " ignored" in out.stderr
    assert ignored == (value != "" and want == 1000 and value != "1000"), out.stderr[-500:]


def test_workload_table_has_the_coco_sp_shape():
    import ugs_workloads as wl
    assert wl.TU_SHAPES["c6_cocosp_b3200"] == (477, 1347, 8, 32, 100)
    ei, ptr, m, k = wl.workload("c6_cocosp_b3200")
    assert ei.shape == (2, 32 * 2694) and ptr[-1] == 32 * 477 and (m, k) == (100, 8)


def test_the_fixture_graphs_share_a_strided_key_and_differ():
    (n, a), (_, b) = lg.graph("a"), lg.graph("b")
    assert a.shape == b.shape == (2, 2694) and n == 477
    diff = np.nonzero((a != b).any(axis=0))[0]
    assert list(diff) == [1] and 1 % (2694 // 500) != 0                  # the only differing column is one the key skips
    assert 0 <= b[:, 1].min() and b[:, 1].max() < n and b[0, 1] != b[1, 1]
    ptr = np.array([0, n], np.int64)
    cache = oracle.Cache()
    on_a = oracle.sample_batch(a, ptr, 16, 6, "sample", 42, cache)
    after_a = oracle.sample_batch(b, ptr, 16, 6, "sample", 42, cache)     # hit on a's entry
    assert cache.stats()["hits"] == 1
    cache.close()
    fresh = oracle.sample_batch(b, ptr, 16, 6, "sample", 42)
    assert np.array_equal(np.asarray(after_a[0]), np.asarray(on_a[0]))
    assert not all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(after_a, fresh))


def test_oracle_reproduces_the_reference_on_large_graph_batches():
    want = lg.fixture()
    calls = lg.calls()
    assert len(calls) == 8 and {c[3] for c in calls} == {4, 6} and {c[4] for c in calls} == {"sample", "graph", "global"}
    assert all(1100 <= 2 * e <= 2700 for _, e, _, _ in lg.GRAPHS.values())
    cache = oracle.Cache()
    for i, (ei, ptr, m, k, mode, seed) in enumerate(calls):
        got = oracle.sample_batch(ei, ptr, m, k, mode, seed, cache)
        for nm, g in zip(lg.NAMES, got):
            assert np.array_equal(np.asarray(g), want[i][nm]), (i, nm)
    st = cache.stats()
    assert st["misses"] == 4 and st["hits"] == 11                         # a, c, d, e: `b` never misses -- it meets a's entry
    cache.close()
