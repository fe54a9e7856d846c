"""CPU (no GPU, no device call): uniform_sampler.PopulationCache exists through every layer, and refuses bad arguments before any
device work, with sample_batch's texts for the dtype checks."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ugs_uniform_population_create", "ugs_uniform_population_destroy", "ugs_uniform_population_add", "ugs_uniform_population_sizes",
           "ugs_uniform_population_info", "ugs_uniform_population_sample_begin", "ugs_uniform_population_sample_finish")


def batch():
    return torch.tensor([[0, 1], [1, 0]], dtype=torch.int64), torch.tensor([0, 3], dtype=torch.int64)


def make(**kw):
    import uniform_sampler as us
    return us.PopulationCache(3, "cuda:0", **kw)


def with_graph(pop, index=0, n=3, slot=0):
    """what add records on the host for a graph of n vertices, without the device call"""
    pop._slot[index] = (slot, n)
    return pop


def test_the_class_is_exported_with_its_methods():
    import uniform_sampler as us
    assert "PopulationCache" in us.__all__
    for name in ("add", "add_many", "sample_batch", "sample_graphs", "sizes", "info", "close"):
        assert callable(getattr(us.PopulationCache, name)), name
    pop = make()
    assert pop.k == 3 and pop.failed == set() and pop.info() == {"graphs": 0, "keys": 0, "bytes": 0, "blocks": 0}
    pop.close()
    pop.close()
    with pytest.raises(RuntimeError, match="closed"):
        pop.info()


def test_the_c_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ugs_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    args = {}
    for name in SYMBOLS:
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, f"{name} is not declared in include/ugs_mi355.h"
        args[name] = " ".join(m.group(1).split())
    assert "int k" in args[SYMBOLS[0]] and "int64_t block_keys" in args[SYMBOLS[0]]
    assert "int64_t max_rows" in args[SYMBOLS[2]] and "int64_t *slots_out" in args[SYMBOLS[2]] and "int32_t *graph_status" in args[SYMBOLS[2]]
    for word in ("const int64_t *slots", "int m_per_graph", "uint64_t seed", "const uint64_t *seeds", "int check", "ugs_job **job_out"):
        assert word in args[SYMBOLS[5]], word
    assert "int dst_is_device" in args[SYMBOLS[6]]
    lib = ctypes.CDLL(os.path.join(ROOT, "ss-gnn_amd", "csrc", "libugs_mi355.so"))
    import ugs_sampler
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in ugs_sampler._lib.EXPORTS
    # the law stands beside the enumeration's
    assert hdr.index("int ugs_uniform_enumerate_begin(") < hdr.index("uniform_sampler.PopulationCache") < hdr.index("int ugs_uniform_set_max_vertices")


@pytest.mark.parametrize("bad", [0, -1, (1 << 25) + 1])
def test_max_rows_out_of_range_is_a_value_error(bad):
    with pytest.raises(ValueError, match="max_rows"):
        make(max_rows=bad)


@pytest.mark.parametrize("bad", [0, -1, (1 << 28) + 1])
def test_block_keys_out_of_range_is_a_value_error(bad):
    with pytest.raises(ValueError, match="block_keys"):
        make(block_keys=bad)


def test_the_c_abi_refuses_the_same_ranges():
    import ugs_sampler
    lib, bad_arg = ugs_sampler._lib.lib, ugs_sampler._lib.UGS_E_BAD_ARG
    pop = ctypes.c_void_p()
    for bad in (0, (1 << 28) + 1):
        assert lib.ugs_uniform_population_create(3, bad, ctypes.byref(pop)) == bad_arg and b"block_keys" in lib.ugs_last_error() and not pop.value
    assert lib.ugs_uniform_population_create(-1, 64, ctypes.byref(pop)) == bad_arg
    assert lib.ugs_uniform_population_create(3, 64, ctypes.byref(pop)) == 0 and pop.value
    ei, ptr = batch()
    slots, st = (ctypes.c_int64 * 1)(), (ctypes.c_int32 * 1)()
    for bad in (0, (1 << 25) + 1):
        assert lib.ugs_uniform_population_add(pop, ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, bad, slots, st) == bad_arg
        assert b"max_rows" in lib.ugs_last_error()
    job, total = ctypes.c_void_p(), ctypes.c_int64()
    slots[0] = 5                                                    # no such slot: refused before any device work
    rc = lib.ugs_uniform_population_sample_begin(pop, slots, ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 4, 0, 42, None, 1, None,
                                                 ctypes.byref(job), ctypes.byref(total))
    assert rc == bad_arg and b"slot" in lib.ugs_last_error() and not job.value
    assert lib.ugs_uniform_population_sizes(pop, slots, 1, (ctypes.c_int64 * 1)()) == bad_arg
    assert lib.ugs_uniform_population_sample_finish(None, None, None, None, None, None, 0) == bad_arg
    assert lib.ugs_uniform_population_destroy(pop) == 0


def test_an_unknown_index_is_a_key_error():
    pop = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(KeyError):
        pop.sample_batch([7], ptr, ei, 4)
    with pytest.raises(KeyError):
        pop.sample_graphs(torch.tensor([7]), ptr, ei, 4, [1])
    with pytest.raises(KeyError):
        pop.sizes([0, 7])


def test_graph_idx_must_match_ptr_in_length():
    pop = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(ValueError, match="graph_idx"):
        pop.sample_batch([0, 0], ptr, ei, 4)
    with pytest.raises(ValueError, match="graph_idx"):
        pop.sample_graphs([], ptr, ei, 4, [])


def test_a_wrong_vertex_count_names_the_graph_and_both_counts():
    pop = with_graph(with_graph(make()), index=1, n=5, slot=1)
    ei = torch.tensor([[0, 1], [1, 0]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"graph 1 of the batch has 4 vertices.* 5$"):
        pop.sample_batch([0, 1], torch.tensor([0, 3, 7]), ei, 4)


def test_dtype_refusals_have_sample_batchs_texts():
    pop = with_graph(make())
    ei, ptr = batch()
    for call in (lambda e, p: pop.sample_batch([0], p, e, 1), lambda e, p: pop.sample_graphs([0], p, e, 1, [3])):
        with pytest.raises(RuntimeError, match="^edge_index must be int64$"):
            call(ei.to(torch.int32), ptr)
        with pytest.raises(RuntimeError, match="^ptr must be int64$"):
            call(ei, ptr.to(torch.int32))
        with pytest.raises(RuntimeError, match=r"^edge_index must have shape \[2, E\]$"):
            call(ei.reshape(-1), ptr)
    with pytest.raises(RuntimeError, match="^edge_index must be int64$"):
        pop.add(1, ei.to(torch.int32), 3)
    with pytest.raises(ValueError, match="same length"):
        pop.add_many([1, 2], [(ei, 3)])
