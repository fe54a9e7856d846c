"""CPU (no GPU, no device call): the WL population exists through every layer -- keywords, C entries, header -- and every refusal of
its arguments comes before any device work."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ugs_uniform_population_create_wl", "ugs_uniform_population_add_wl", "ugs_uniform_population_wl_digests",
           "ugs_uniform_population_wl_stats", "ugs_uniform_population_sample_wl_begin", "ugs_uniform_population_distinct_wl_begin")


def us():
    import uniform_sampler
    return uniform_sampler


def wl():
    from ugs_sampler import wl as module
    return module


def make(k=3, **kw):
    kw.setdefault("wl_iterations", 3)
    return us().PopulationCache(k, "cuda:0", **kw)


def batch():
    return torch.tensor([[0, 1], [1, 0]], dtype=torch.int64), torch.tensor([0, 3], dtype=torch.int64)


def with_graph(pop, index=0, n=3, slot=0):
    """what add records on the host for a graph of n vertices, without the device call"""
    pop._slot[index] = (slot, n)
    return pop


def test_a_wl_population_is_created_without_a_device():
    pop = make()
    assert pop.wl_iterations == 3
    assert pop.info() == {"graphs": 0, "keys": 0, "bytes": 0, "blocks": 0, "wl_classes": 0, "wl_rows_hashed": 0}
    digest, status = pop.wl_digests()
    assert tuple(digest.shape) == (0, 2) and digest.dtype == torch.int64 and tuple(status.shape) == (0,) and status.dtype == torch.int32
    pop.close()
    plain = us().PopulationCache(3, "cuda:0")
    assert plain.wl_iterations is None and plain.info() == {"graphs": 0, "keys": 0, "bytes": 0, "blocks": 0}
    with pytest.raises(RuntimeError, match="wl_iterations"):
        plain.wl_digests()


def test_the_c_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ugs_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "ss-gnn_amd", "csrc", "libugs_mi355.so"))
    import ugs_sampler
    for name in SYMBOLS:
        assert re.search(r"int\s+" + name + r"\s*\(", code), f"{name} is not declared in include/ugs_mi355.h"
        assert hasattr(lib, name) and name in ugs_sampler._lib.EXPORTS
    # the law stands beside the population's, and the existing declarations are as they were
    assert hdr.index("uniform_sampler.PopulationCache") < hdr.index("WL class indices of a population") < hdr.index("int ugs_uniform_set_max_vertices")
    assert "int ugs_uniform_population_create(int k, int64_t block_keys, ugs_uniform_population **pop_out);" in hdr


@pytest.mark.parametrize("bad", [-1, 9, 100, 2.0, True, "3"])
def test_wl_iterations_outside_0_to_8_is_a_value_error(bad):
    with pytest.raises(ValueError, match="wl_iterations"):
        make(wl_iterations=bad)


@pytest.mark.parametrize("k", [0, 33, 64])
def test_k_outside_the_wl_kernels_range_is_a_value_error(k):
    with pytest.raises(ValueError, match="1 <= k <= 32"):
        make(k=k)
    us().PopulationCache(k, "cuda:0").close()          # a plain population of that k is as before


def test_the_c_abi_refuses_the_same_ranges_and_a_plain_population():
    import ugs_sampler
    lib, bad_arg = ugs_sampler._lib.lib, ugs_sampler._lib.UGS_E_BAD_ARG
    pop = ctypes.c_void_p()
    for k, it in ((3, -1), (3, 9), (0, 3), (33, 3)):
        assert lib.ugs_uniform_population_create_wl(k, 64, it, ctypes.byref(pop)) != 0 and not pop.value
    assert lib.ugs_uniform_population_create_wl(3, 0, 3, ctypes.byref(pop)) == bad_arg and b"block_keys" in lib.ugs_last_error()
    plain = ctypes.c_void_p()
    assert lib.ugs_uniform_population_create(3, 64, ctypes.byref(plain)) == 0
    ei, ptr = batch()
    slots, st, n = (ctypes.c_int64 * 1)(), (ctypes.c_int32 * 1)(), ctypes.c_int64()
    assert lib.ugs_uniform_population_add_wl(plain, ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 100, None, 0, slots, st) == bad_arg
    assert b"without WL" in lib.ugs_last_error()
    assert lib.ugs_uniform_population_wl_digests(plain, 0, None, ctypes.byref(n)) == bad_arg
    job, total = ctypes.c_void_p(), ctypes.c_int64()
    rc = lib.ugs_uniform_population_sample_wl_begin(plain, slots, ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 4, 0, 42, None, 1, None,
                                                    None, None, 0, 0, 1, None, ctypes.byref(job), ctypes.byref(total))
    assert rc == bad_arg and b"without WL" in lib.ugs_last_error() and not job.value
    assert lib.ugs_uniform_population_destroy(plain) == 0
    assert lib.ugs_uniform_population_create_wl(3, 64, 8, ctypes.byref(pop)) == 0 and pop.value
    cls, rows = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.ugs_uniform_population_wl_stats(pop, ctypes.byref(cls), ctypes.byref(rows)) == 0 and (cls.value, rows.value) == (0, 0)
    assert lib.ugs_uniform_population_wl_digests(pop, 0, None, ctypes.byref(n)) == 0 and n.value == 0
    # labels for another number of vertices than the call's: refused before any device work
    assert lib.ugs_uniform_population_add_wl(pop, ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 100, ctypes.c_void_p(8), 2, slots, st) == bad_arg
    assert b"labels for 3 vertices" in lib.ugs_last_error()
    assert lib.ugs_uniform_population_destroy(pop) == 0


def test_wl_on_a_plain_population_is_a_runtime_error():
    pop = with_graph(us().PopulationCache(3, "cuda:0"))
    ei, ptr = batch()
    table = wl().WLVocab({}, "cuda:0")
    for call in (lambda: pop.sample_batch([0], ptr, ei, 2, wl=table), lambda: pop.sample_graphs([0], ptr, ei, 2, [1], wl=table),
                 lambda: pop.sample_distinct([0], ptr, ei, 2, [1], wl=table)):
        with pytest.raises(RuntimeError, match="wl_iterations"):
            call()
    with pytest.raises(RuntimeError, match="wl_iterations"):
        pop.add_many([1], [(ei, 3)], node_labels=[torch.zeros(3, dtype=torch.int64)])
    with pytest.raises(RuntimeError, match="wl_iterations"):
        pop.add(1, ei, 3, x=torch.zeros(3, 2))


def test_wl_takes_a_vocabulary_on_the_populations_device():
    pop = with_graph(make())
    ei, ptr = batch()
    for bad in ({}, "vocab", 3, torch.zeros(2)):
        with pytest.raises(TypeError, match="WLVocab"):
            pop.sample_batch([0], ptr, ei, 2, wl=bad)
        with pytest.raises(TypeError, match="WLVocab"):
            pop.sample_graphs([7], ptr, ei, 2, [1], wl=bad)         # (before the unknown index is looked at)
        with pytest.raises(TypeError, match="WLVocab"):
            pop.sample_distinct([0], ptr, ei, 2, [1], wl=bad)
    elsewhere = wl().WLVocab({}, "cuda:0")
    elsewhere.device = torch.device("cuda:1")                       # (a table that lives on another GPU, without needing one)
    with pytest.raises(ValueError, match="cuda:1"):
        pop.sample_batch([0], ptr, ei, 2, wl=elsewhere)


def test_label_arguments_are_checked_before_any_device_work():
    pop = make()
    ei = torch.tensor([[0, 1], [1, 0]], dtype=torch.int64)
    lab, x = torch.zeros(3, dtype=torch.int64), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="mutually exclusive"):
        pop.add_many([0], [(ei, 3)], x=[x], node_labels=[lab])
    with pytest.raises(ValueError, match="one tensor per graph"):
        pop.add_many([0, 1], [(ei, 3), (ei, 3)], node_labels=[lab])
    with pytest.raises(ValueError, match="one tensor per graph"):
        pop.add_many([0], [(ei, 3)], x=[x, x])
    with pytest.raises(ValueError, match="4 vertices for a graph of 3"):
        pop.add_many([0], [(ei, 3)], node_labels=[torch.zeros(4, dtype=torch.int64)])
    with pytest.raises(ValueError, match="2 vertices for a graph of 3"):
        pop.add_many([0], [(ei, 3)], x=[torch.zeros(2, 5)])
    with pytest.raises(ValueError, match="int64"):
        pop.add_many([0], [(ei, 3)], node_labels=[torch.zeros(3, dtype=torch.int32)])
    with pytest.raises(TypeError):
        pop.add_many([0], [(ei, 3)], x=[torch.zeros(3, 2, dtype=torch.bfloat16)])
    assert pop.info()["graphs"] == 0 and pop._wl_labeled is None


@pytest.mark.parametrize("first", [False, True])
def test_one_labelling_per_population(first):
    pop = make()
    pop._wl_labeled = first                             # what an add of that labelling records
    ei = torch.tensor([[0, 1], [1, 0]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="same labelling"):
        if first:
            pop.add_many([1], [(ei, 3)])
        else:
            pop.add_many([1], [(ei, 3)], node_labels=[torch.zeros(3, dtype=torch.int64)])
    with pytest.raises(RuntimeError, match="same labelling"):
        if first:
            pop.add(1, ei, 3)
        else:
            pop.add(1, ei, 3, x=torch.zeros(3, 2))
