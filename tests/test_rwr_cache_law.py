"""CPU (no GPU, no device call): what rwr_sampler.GraphCache stands on, and what it refuses before any device work.

The cache stores every dataset graph's own columns and serves a batch as if it were those graphs collated in batch order.  So
for every pinned input of tests/rwr_paths.py and tests/rwr_row_paths.py the batch regrouped that way -- each graph's kept
columns together, dropped columns gone -- must give the law's five tensors of the original batch, in both modes: then the GPU
tests may send the regrouped batch through the cache and compare with the law of the original case."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rwr_cache_cases as CC
import rwr_law as R
import rwr_paths as P
import rwr_row_law as RR
import rwr_row_paths as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ugs_rwr_cache_create", "ugs_rwr_cache_destroy", "ugs_rwr_cache_add", "ugs_rwr_cache_info", "ugs_rwr_cache_sample_begin")
OVERFLOW_N = 40_000_000                                             # 10 n k > INT_MAX at k = 6


def same(got, want, what):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), what


@pytest.mark.parametrize("name", [c.name for c in P.cases()])
def test_the_regrouped_batch_has_the_law_of_the_batch(name):
    c = P.case(name)
    ei, ptr = CC.regrouped(c.ei, c.ptr)
    for mode in ("sample", "global"):
        same(R.sample_batch(ei, ptr, c.m, c.k, mode, c.seed, c.p, c.seeds), P.law_of(name, mode), (name, mode))


@pytest.mark.parametrize("name", [c.name for c in Q.cases()])
def test_the_regrouped_batch_has_the_row_law_of_the_batch(name):
    c = Q.case(name)
    ei, ptr = CC.regrouped(c.ei, c.ptr)
    for mode in ("sample", "global"):
        same(RR.sample_batch(ei, ptr, c.m, c.k, mode, c.seed, c.p, c.seeds), Q.law_of(name, mode), (name, mode))


def test_some_cases_really_are_regrouped():
    dropped = [c.name for c in P.cases() + Q.cases() if sum(a.shape[1] for _, a in CC.split(c.ei, c.ptr)) < c.ei.shape[1]]
    assert {"nv1", "nv2", "nv256", "nv4096", "all_dropped"} <= set(dropped)


def test_split_keeps_order_and_drops_what_the_law_drops():
    ei = np.array([[5, 9, 6, 4, 8, 5, 7], [6, 8, 5, 5, 7, 5, 9]], np.int64)   # graphs [5, 7), [7, 7) and [7, 10)
    ptr = np.array([5, 7, 7, 10], np.int64)
    (n0, a0), (n1, a1), (n2, a2) = CC.split(ei, ptr)
    assert (n0, n1, n2) == (2, 0, 3) and a1.shape == (2, 0)
    assert a0.tolist() == [[0, 1, 0], [1, 0, 0]]                    # (5, 6), (6, 5), (5, 5) in batch order; (4, 5) leaves the batch
    assert a2.tolist() == [[2, 1, 0], [1, 0, 2]]                    # (9, 8), (8, 7), (7, 9)
    assert CC.split(np.zeros((2, 0), np.int64), np.array([4], np.int64)) == []


# ---- the class, its C entries, and the refusals that need no device ----
def make(k=3, **kw):
    import rwr_sampler
    return rwr_sampler.GraphCache(k, "cuda:0", **kw)


def with_graph(cache, index=0, n=3, slot=0, cols=2):
    """what add records on the host for a graph of n vertices and `cols` columns, without the device call"""
    cache._slot[index] = (slot, n, cols)
    return cache


def batch():
    return torch.tensor([[0, 1], [1, 0]], dtype=torch.int64), torch.tensor([0, 3], dtype=torch.int64)


def test_the_class_is_exported_with_its_methods():
    import rwr_sampler
    assert "GraphCache" in rwr_sampler.__all__
    for name in ("add", "add_many", "sample_batch", "sample_graphs", "info", "close"):
        assert callable(getattr(rwr_sampler.GraphCache, name)), name
    cache = make(reserve=(10, 20))
    assert cache.k == 3 and cache.failed == set()
    assert cache.info() == {"graphs": 0, "vertices": 0, "half_edges": 0, "bytes": 0, "generations": 0}    # create touches no device
    cache.close()
    cache.close()
    with pytest.raises(RuntimeError, match="closed"):
        cache.info()


def test_the_c_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ugs_mi355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    args = {}
    for name in SYMBOLS:
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, f"{name} is not declared in include/ugs_mi355.h"
        args[name] = " ".join(m.group(1).split())
    for word in ("int k", "int64_t reserve_vertices", "int64_t reserve_columns"):
        assert word in args[SYMBOLS[0]], word
    assert "int64_t *slots_out" in args[SYMBOLS[2]] and "int32_t *status_out" in args[SYMBOLS[2]]
    for word in ("const int64_t *slots", "int m_per_graph", "uint64_t seed", "const uint64_t *seeds", "double p_restart", "int row_streams",
                 "int check", "int32_t *graph_status", "ugs_job **job_out"):
        assert word in args[SYMBOLS[4]], word
    lib = ctypes.CDLL(os.path.join(ROOT, "ss-gnn_amd", "csrc", "libugs_mi355.so"))
    import ugs_sampler
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in ugs_sampler._lib.EXPORTS
    # the contract stands at sample_begin, and says how strict the check is
    text = hdr[hdr.index("rwr_sampler.GraphCache"):hdr.index("int ugs_rwr_cache_sample_begin(")]
    assert "THE CONTRACT" in text and "stricter" in text and "never accept" in text


def test_the_c_abi_refuses_before_any_device_work():
    import ugs_sampler
    lib, bad_arg = ugs_sampler._lib.lib, ugs_sampler._lib.UGS_E_BAD_ARG
    cache = ctypes.c_void_p()
    assert lib.ugs_rwr_cache_create(0, 0, 0, ctypes.byref(cache)) == bad_arg and not cache.value
    assert lib.ugs_rwr_cache_create(65, 0, 0, ctypes.byref(cache)) != 0 and b"k must be <= 64" in lib.ugs_last_error() and not cache.value
    assert lib.ugs_rwr_cache_create(3, -1, 0, ctypes.byref(cache)) == bad_arg and b"reserve" in lib.ugs_last_error()
    assert lib.ugs_rwr_cache_create(3, 0, 0, ctypes.byref(cache)) == 0 and cache.value
    ei, ptr = batch()
    slots, st = (ctypes.c_int64 * 1)(), (ctypes.c_int32 * 1)()
    crossing = torch.tensor([[0, 3], [1, 4]], dtype=torch.int64)    # a column outside the graph: refused on the host
    assert lib.ugs_rwr_cache_add(cache, crossing.data_ptr(), 2, 2, ptr.data_ptr(), 1, slots, st) == bad_arg
    assert b"not inside one graph" in lib.ugs_last_error()
    job, total = ctypes.c_void_p(), ctypes.c_int64()
    slots[0] = 5                                                    # no such slot
    for check in (1, 0):
        rc = lib.ugs_rwr_cache_sample_begin(cache, slots, ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 4, 0, 42, None, 0.2, 0, check, None,
                                            ctypes.byref(job), ctypes.byref(total))
        assert rc == bad_arg and b"slot" in lib.ugs_last_error() and not job.value
    rc = lib.ugs_rwr_cache_sample_begin(cache, slots, None, 0, 2, ptr.data_ptr(), 1, 4, 0, 42, None, 0.2, 0, 1, None, ctypes.byref(job),
                                        ctypes.byref(total))
    assert rc == bad_arg and b"edge_index" in lib.ugs_last_error()   # the check without the batch's columns
    rc = lib.ugs_rwr_cache_sample_begin(cache, slots, ei.data_ptr(), 2, 2, ptr.data_ptr(), 1, 4, 0, 42, None, 1.5, 0, 1, None,
                                        ctypes.byref(job), ctypes.byref(total))
    assert rc == bad_arg and b"p_restart" in lib.ugs_last_error()
    assert lib.ugs_rwr_cache_info(cache, None, None, None, None, None) == 0
    assert lib.ugs_rwr_cache_destroy(cache) == 0


def test_an_unknown_index_is_a_key_error():
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(KeyError):
        cache.sample_batch([7], ptr, ei, 4)
    with pytest.raises(KeyError):
        cache.sample_graphs(torch.tensor([7]), ptr, ei, 4, [1])
    with pytest.raises(KeyError):
        cache.sample_batch([7], ptr, None, 4, check=False)


def test_graph_idx_must_match_ptr_in_length():
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(ValueError, match="graph_idx names 2 graphs, ptr holds 1"):
        cache.sample_batch([0, 0], ptr, ei, 4)
    with pytest.raises(ValueError, match="graph_idx"):
        cache.sample_graphs([], ptr, ei, 4, [])


@pytest.mark.parametrize("device", ["cpu", "cuda:1"])
def test_a_device_that_is_not_the_caches_is_a_value_error(device):
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(ValueError, match="GPU device" if device == "cpu" else "the cache lives on cuda:0"):
        cache.sample_batch([0], ptr, ei, 4, device=device)
    with pytest.raises(ValueError, match="GPU device"):
        import rwr_sampler
        rwr_sampler.GraphCache(3, "cpu")


@pytest.mark.parametrize("streams", ["rows", None, 1])
def test_another_value_of_streams_is_a_value_error(streams):
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(ValueError, match="streams must be 'graph' or 'row'"):
        cache.sample_batch([0], ptr, ei, 4, streams=streams)
    with pytest.raises(ValueError, match="streams must be 'graph' or 'row'"):
        cache.sample_graphs([0], ptr, ei, 4, [1], streams=streams)


def test_a_wrong_vertex_count_names_the_graph_and_both_counts():
    cache = with_graph(with_graph(make()), index=1, n=5, slot=1)
    ei = torch.tensor([[0, 1, 3, 4], [1, 0, 4, 3]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"graph 1 of the batch has 4 vertices, the graph added in its place has 5$"):
        cache.sample_batch([0, 1], torch.tensor([0, 3, 7]), ei, 4)
    with pytest.raises(RuntimeError, match=r"graph 1 of the batch has 4 vertices"):
        cache.sample_batch([0, 1], torch.tensor([0, 3, 7]), None, 4, check=False)


def test_a_wrong_column_count_gives_both_counts():
    cache = with_graph(with_graph(make()), index=1, n=4, slot=1, cols=3)
    ei = torch.tensor([[0, 1, 3, 4], [1, 0, 4, 3]], dtype=torch.int64)
    for check in (True, False):
        with pytest.raises(RuntimeError, match=r"the batch has 4 columns, the added graphs have 5$"):
            cache.sample_batch([0, 1], torch.tensor([0, 3, 7]), ei, 4, check=check)


def test_sample_batch_on_a_failed_graph_raises_the_uncached_text():
    cache = with_graph(with_graph(make(k=6), n=18, cols=0), index=1, n=OVERFLOW_N, slot=1, cols=0)
    cache.failed.add(1)
    none, ptr = torch.zeros((2, 0), dtype=torch.int64), torch.tensor([0, 18, 18 + OVERFLOW_N])
    with pytest.raises(RuntimeError, match=rf"^rwr_sampler: graph 1 has {OVERFLOW_N} vertices; 10 n k must fit the reference's int iteration limit$"):
        cache.sample_batch([0, 1], ptr, none, 4)


def test_no_edge_index_needs_check_false():
    cache = with_graph(make())
    with pytest.raises(ValueError, match="check=False"):
        cache.sample_batch([0], batch()[1], None, 4)
    with pytest.raises(ValueError, match="check=False"):
        cache.sample_graphs([0], batch()[1], None, 4, [1])


def test_dtype_refusals_have_sample_batchs_texts():
    cache = with_graph(make())
    ei, ptr = batch()
    for call in (lambda e, p: cache.sample_batch([0], p, e, 1), lambda e, p: cache.sample_graphs([0], p, e, 1, [3])):
        with pytest.raises(RuntimeError, match="^edge_index must be int64$"):
            call(ei.to(torch.int32), ptr)
        with pytest.raises(RuntimeError, match="^ptr must be int64$"):
            call(ei, ptr.to(torch.int32))
        with pytest.raises(RuntimeError, match=r"^edge_index must have shape \[2, E\]$"):
            call(ei.reshape(-1), ptr)
    with pytest.raises(RuntimeError, match="^ptr must be int64$"):
        cache.sample_batch([0], ptr.to(torch.int32), None, 1, check=False)


def test_add_many_refuses_a_column_that_leaves_its_graph_and_adds_nothing():
    cache = make()
    good = torch.tensor([[0, 1], [1, 2]], dtype=torch.int64)
    for bad in (torch.tensor([[0, 1], [1, 3]]), torch.tensor([[0, -1], [1, 0]])):
        with pytest.raises(ValueError, match=r"^graph 12 has a column with an endpoint outside \[0, 3\)$"):
            cache.add_many([11, 12], [(good, 3), (bad, 3)])
        assert cache._slot == {} and cache.info()["graphs"] == 0
    with pytest.raises(ValueError, match="same length"):
        cache.add_many([1, 2], [(good, 3)])
    with pytest.raises(RuntimeError, match="^edge_index must be int64$"):
        cache.add(1, good.to(torch.int32), 3)
    with pytest.raises(ValueError, match="reserve"):
        make(reserve=(-1, 0))
