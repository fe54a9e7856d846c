"""CPU (no GPU, no device call): uniform_sampler.enumerate_graphs / count_graphs exist through every layer, and refuse bad
arguments before any device work, with sample_batch's texts for the dtype checks."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ugs_uniform_count_graphs", "ugs_uniform_enumerate_begin", "ugs_uniform_enumerate_finish")


def batch():
    return torch.tensor([[0, 1], [1, 0]], dtype=torch.int64), torch.tensor([0, 3], dtype=torch.int64)


def test_the_functions_are_exported():
    import uniform_sampler as us
    assert "enumerate_graphs" in us.__all__ and "count_graphs" in us.__all__
    assert callable(us.enumerate_graphs) and callable(us.count_graphs)
    assert {"sample_batch", "sample_graphs", "set_max_vertices", "max_vertices"} <= set(us.__all__)
    from ugs_sampler import _graphs
    assert callable(_graphs.run_rows_job) and callable(_graphs.run_job)


def test_the_c_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ugs_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    args = {}
    for name in SYMBOLS:
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, f"{name} is not declared in include/ugs_mi355.h"
        args[name] = " ".join(m.group(1).split())
    assert "int64_t limit" in args[SYMBOLS[0]] and "int64_t *counts_out" in args[SYMBOLS[0]] and "int32_t *graph_status" in args[SYMBOLS[0]]
    assert "int64_t max_rows" in args[SYMBOLS[1]] and "int64_t *total_rows_out" in args[SYMBOLS[1]] and "ugs_job **job_out" in args[SYMBOLS[1]]
    assert "m_per_graph" not in args[SYMBOLS[1]] and "seed" not in args[SYMBOLS[1]]
    assert "ugs_job *job" in args[SYMBOLS[2]] and "int dst_is_device" in args[SYMBOLS[2]]
    lib = ctypes.CDLL(os.path.join(ROOT, "ss-gnn_amd", "csrc", "libugs_mi355.so"))
    import ugs_sampler
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in ugs_sampler._lib.EXPORTS
    # the law stands beside the sampler's
    assert hdr.index("ugs_uniform_sample_batch_finish(") < hdr.index("uniform_sampler.enumerate_graphs") < hdr.index("int ugs_uniform_set_max_vertices")


@pytest.mark.parametrize("bad", [0, -1, (1 << 25) + 1, 1 << 40])
def test_max_rows_out_of_range_is_a_value_error(bad):
    import uniform_sampler as us
    with pytest.raises(ValueError, match="max_rows"):
        us.enumerate_graphs(*batch(), 2, max_rows=bad)


@pytest.mark.parametrize("bad", [0, -5, (1 << 32) + 1])
def test_limit_out_of_range_is_a_value_error(bad):
    import uniform_sampler as us
    with pytest.raises(ValueError, match="limit"):
        us.count_graphs(*batch(), 2, limit=bad)


def test_the_c_abi_refuses_the_same_ranges():
    import ugs_sampler
    lib = ugs_sampler._lib.lib
    ei, ptr = batch()
    job, rows, total = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
    st, cnt = (ctypes.c_int32 * 1)(), (ctypes.c_int64 * 1)()
    for bad in (0, (1 << 25) + 1):
        rc = lib.ugs_uniform_enumerate_begin(ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 2, 0, bad, st, ctypes.byref(job), ctypes.byref(rows), ctypes.byref(total))
        assert rc == ugs_sampler._lib.UGS_E_BAD_ARG and b"max_rows" in lib.ugs_last_error() and not job.value
    for bad in (0, (1 << 32) + 1):
        assert lib.ugs_uniform_count_graphs(ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 2, bad, cnt, st) == ugs_sampler._lib.UGS_E_BAD_ARG
        assert b"limit" in lib.ugs_last_error()
    assert lib.ugs_uniform_enumerate_finish(None, None, None, None, None, None, 0) == ugs_sampler._lib.UGS_E_BAD_ARG


def test_dtype_refusals_have_sample_batchs_texts():
    import uniform_sampler as us
    ei, ptr = batch()
    for call in (lambda e, p: us.enumerate_graphs(e, p, 2), lambda e, p: us.count_graphs(e, p, 2), lambda e, p: us.sample_batch(e, p, 1, 2)):
        with pytest.raises(RuntimeError, match="^edge_index must be int64$"):
            call(ei.to(torch.int32), ptr)
        with pytest.raises(RuntimeError, match="^ptr must be int64$"):
            call(ei, ptr.to(torch.int32))
        with pytest.raises(RuntimeError, match=r"^edge_index must have shape \[2, E\]$"):
            call(ei.reshape(-1), ptr)
