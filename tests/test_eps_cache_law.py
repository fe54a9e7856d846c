"""CPU (no GPU, no device call): what epsilon_uniform_sampler.GraphCache stands on, and what it refuses before any device work.

The cache stores every dataset graph's own columns, numbered from 0 inside the graph, and serves a batch as if it were those
graphs collated in batch order.  So for the inputs of tests/test_gpu_eps_cache.py: the batch regrouped that way is the batch
itself, with the same law (tests/eps_rows.py, tests/eps_graphs_law.py); a graph's rows drawn alone, with its columns numbered
from 0, become the batch's rows once coff[g] -- the columns of the graphs ahead of it -- is added to edge_src; and the rows the
build kernel has to produce (eps_cache_cases.rows_of) are those of oracle/eps_oracle.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import eps_cache_cases as CC
import eps_graphs_law
import eps_oracle
import eps_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ugs_eps_cache_create", "ugs_eps_cache_destroy", "ugs_eps_cache_add", "ugs_eps_cache_info", "ugs_eps_cache_graph_csr",
           "ugs_eps_cache_sample_begin")


def same(got, want, what):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), what


def inputs():
    """name -> (graphs, first vertex, m, k, epsilon): the batches the GPU tests send through the cache"""
    return {"mixed_k3": (CC.mixed_graphs(), 4, 5, 3, 0.3), "mixed_k6": (CC.mixed_graphs(), 4, 5, 6, 0.3),
            "path_among_isolated": ([CC.path_among_isolated()], 10, 40, 5, 1.0),
            "build_graphs": (list(CC.BUILD_GRAPHS.values()), 0, 3, 3, 0.5)}


@pytest.mark.parametrize("name", sorted(inputs()))
def test_the_regrouped_batch_is_the_batch_and_has_its_law(name):
    graphs, first, m, k, epsilon = inputs()[name]
    ei, ptr = CC.batch_of(graphs, first=first)
    again = CC.regrouped(ei, ptr)
    assert np.array_equal(again[0], ei) and np.array_equal(again[1], ptr)
    back = CC.split(ei, ptr)
    assert [n for n, _ in back] == [n for n, _ in graphs] and all(np.array_equal(a, b) for (_, a), (_, b) in zip(back, graphs))
    seeds = [(31 * g + 7) for g in range(len(graphs))]
    for mode in ("sample", "global"):
        same(eps_rows.sample_rows(*again, m, k, mode, 9, epsilon), eps_rows.sample_rows(ei, ptr, m, k, mode, 9, epsilon), (name, mode))
        same(eps_graphs_law.expected(*again, m, k, mode, seeds, epsilon), eps_graphs_law.expected(ei, ptr, m, k, mode, seeds, epsilon), (name, mode))


@pytest.mark.parametrize("name", sorted(inputs()))
def test_coff_turns_a_graphs_own_columns_into_the_batchs(name):
    """graph g alone at its place in the batch, its columns numbered from 0 (what the store holds), seeded with seeds[g]: its rows
    are block g of sample_graphs on the batch once coff[g] is added to edge_src"""
    graphs, first, m, k, epsilon = inputs()[name]
    ei, ptr = CC.batch_of(graphs, first=first)
    coff = CC.coff_of(graphs)
    assert coff[-1] == ei.shape[1]
    seeds = [(31 * g + 7) for g in range(len(graphs))]
    nodes, eidx, eptr, sptr, esrc = eps_graphs_law.expected(ei, ptr, m, k, "global", seeds, epsilon)
    some = False
    for g, (n, a) in enumerate(graphs):
        alone = eps_rows.sample_rows(a + ptr[g], ptr[g:g + 2], m, k, "global", seeds[g], epsilon)
        e0, e1 = eptr[g * m], eptr[(g + 1) * m]
        assert np.array_equal(alone[0], nodes[g * m:(g + 1) * m]) and np.array_equal(alone[1], eidx[:, e0:e1])
        assert np.array_equal(alone[2], eptr[g * m:(g + 1) * m + 1] - e0)
        assert np.array_equal(alone[4] + coff[g], esrc[e0:e1]), (name, g)
        some = some or (e1 > e0 and coff[g] > 0)
    assert some or len(graphs) == 1, "no graph behind the first has an edge: the offsets are not exercised"


def test_rows_of_is_the_oracles_order():
    for name, (n, a) in CC.BUILD_GRAPHS.items():
        rowptr, nbr, ecs = CC.rows_of(n, a)
        adj = eps_oracle.adjacency(a.T.tolist(), n)
        assert rowptr.tolist() == [0] + np.cumsum([len(r) for r in adj]).tolist()[:n] and rowptr[-1] == 2 * a.shape[1], name
        for u in range(n):
            row = list(zip(nbr[rowptr[u]:rowptr[u + 1]].tolist(), ecs[rowptr[u]:rowptr[u + 1]].tolist()))
            assert [v for v, _ in row] == adj[u], (name, u)
            assert [cs for _, cs in row] == sorted(cs for _, cs in row), (name, u)       # (column, side) order
            for v, cs in row:
                assert (a[0, cs >> 1], a[1, cs >> 1]) == ((v, u) if cs & 1 else (u, v)), (name, u, cs)


def test_the_build_graphs_reach_what_they_are_chosen_for():
    n, a = CC.BUILD_GRAPHS["star70"]
    assert a.shape[1] == 70 and ((a[0] == 0) ^ (a[1] == 0)).all() and (a[0, :64] == 0).any() and (a[1, :64] == 0).any()
    n, a = CC.BUILD_GRAPHS["random130"]
    assert a.shape[1] == 130 and n == 9 and (a[0] == a[1]).any()
    for lo in (0, 64):                                                  # both full chunks hold every vertex ...
        assert set(a[:, lo:lo + 64].ravel().tolist()) == set(range(9))
    for v in range(9):                                                  # ... and every vertex's row runs over more than one chunk
        assert sum(bool((a[:, lo:lo + 64] == v).any()) for lo in (0, 64, 128)) >= 2
    n, a = CC.BUILD_GRAPHS["loop_among_columns"]
    assert ((a[0] == 1) & (a[1] == 1)).sum() == 2 and ((a[0] == 1) ^ (a[1] == 1)).sum() >= 2
    n, a = CC.BUILD_GRAPHS["triangle_dup_reversed"]
    assert a[:, 0].tolist() == a[:, 3].tolist() and a[:, 1].tolist() == a[::-1, 4].tolist()
    n, a = CC.path_among_isolated()
    for epsilon in (1.0, 0.01):                                          # what test 3 of the GPU file asserts first, on its own inputs
        want = eps_rows.sample_rows(a + 10, [10, 10 + n], CC.PATH_ROWS, 5, "sample", 8, epsilon)[0]
        assert (want[:, 0] < 0).any() and (want[:, 0] >= 0).any(), epsilon


# ---- the class, its C entries, and the refusals that need no device ----
def make(**kw):
    import epsilon_uniform_sampler
    return epsilon_uniform_sampler.GraphCache("cuda:0", **kw)


def with_graph(cache, index=0, n=3, slot=0, cols=2):
    """what add records on the host for a graph of n vertices and `cols` columns, without the device call"""
    cache._slot[index] = (slot, n, cols)
    return cache


def batch():
    return torch.tensor([[0, 1], [1, 0]], dtype=torch.int64), torch.tensor([0, 3], dtype=torch.int64)


def test_the_class_is_exported_with_its_methods():
    import epsilon_uniform_sampler as eps
    assert "GraphCache" in eps.__all__
    for name in ("add", "add_many", "sample_batch", "sample_graphs", "info", "close"):
        assert callable(getattr(eps.GraphCache, name)), name
    cache = make(reserve=(10, 20))
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
    assert "int k" not in args[SYMBOLS[0]] and "int64_t reserve_vertices" in args[SYMBOLS[0]]      # one cache for every k
    assert "int64_t *slots_out" in args[SYMBOLS[2]]
    for word in ("int64_t *rowptr", "int32_t *nbr", "int32_t *ecs"):
        assert word in args[SYMBOLS[4]], word
    for word in ("const int64_t *slots", "int m_per_graph", "int k", "uint64_t seed", "const uint64_t *seeds", "double epsilon", "int check",
                 "ugs_job **job_out"):
        assert word in args[SYMBOLS[5]], word
    lib = ctypes.CDLL(os.path.join(ROOT, "ss-gnn_amd", "csrc", "libugs_mi355.so"))
    import ugs_sampler
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in ugs_sampler._lib.EXPORTS
    text = hdr[hdr.index("epsilon_uniform_sampler.GraphCache"):hdr.index("int ugs_eps_cache_sample_begin(")]
    assert "THE CONTRACT" in text and "THE ROW ORDER" in text and "never accept" in text


def test_the_c_abi_refuses_before_any_device_work():
    import ugs_sampler
    lib, bad_arg = ugs_sampler._lib.lib, ugs_sampler._lib.UGS_E_BAD_ARG
    cache = ctypes.c_void_p()
    assert lib.ugs_eps_cache_create(-1, 0, ctypes.byref(cache)) == bad_arg and b"reserve" in lib.ugs_last_error() and not cache.value
    assert lib.ugs_eps_cache_create(0, 0, ctypes.byref(cache)) == 0 and cache.value
    ei, ptr = batch()
    slots = (ctypes.c_int64 * 1)()
    crossing = torch.tensor([[0, 3], [1, 4]], dtype=torch.int64)    # a column outside the graph: refused on the host
    assert lib.ugs_eps_cache_add(cache, crossing.data_ptr(), 2, 2, ptr.data_ptr(), 1, slots) == bad_arg
    assert b"not inside one graph" in lib.ugs_last_error()
    job, total = ctypes.c_void_p(), ctypes.c_int64()

    def begin(e, stride, ncols, m, k, epsilon, check):
        return lib.ugs_eps_cache_sample_begin(cache, slots, e, stride, ncols, ptr.data_ptr(), 1, m, k, 0, 42, None, epsilon, check, None,
                                              ctypes.byref(job), ctypes.byref(total))

    slots[0] = 5                                                    # no such slot
    for check in (1, 0):
        assert begin(ei.data_ptr(), 2, 2, 4, 3, 0.1, check) == bad_arg and b"slot" in lib.ugs_last_error() and not job.value
    assert begin(None, 0, 2, 4, 3, 0.1, 1) == bad_arg and b"edge_index" in lib.ugs_last_error()     # the check without the columns
    for epsilon in (0.0, 1.5, -0.1, float("nan")):
        assert begin(ei.data_ptr(), 2, 2, 4, 3, epsilon, 1) == bad_arg and lib.ugs_last_error() == b"epsilon must be in (0, 1]"
    assert begin(ei.data_ptr(), 2, 2, -1, 3, 0.1, 1) == bad_arg and lib.ugs_last_error() == b"m_per_graph must be >= 0"
    assert begin(ei.data_ptr(), 2, 2, 4, 0, 0.1, 1) == bad_arg and lib.ugs_last_error() == b"k must be >= 1"
    assert begin(ei.data_ptr(), 2, 2, 4, 33, 0.1, 1) != 0 and lib.ugs_last_error() == b"k > 32 is not supported by the HIP sampler"
    assert not job.value
    assert lib.ugs_eps_cache_graph_csr(cache, 0, 0, 0, None, None, None, None, None) == bad_arg and b"slot" in lib.ugs_last_error()
    assert lib.ugs_eps_cache_info(cache, None, None, None, None, None) == 0
    assert lib.ugs_eps_cache_destroy(cache) == 0


def test_an_unknown_index_is_a_key_error():
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(KeyError):
        cache.sample_batch([7], ptr, ei, 4, 3)
    with pytest.raises(KeyError):
        cache.sample_graphs(torch.tensor([7]), ptr, ei, 4, 3, [1])
    with pytest.raises(KeyError):
        cache.sample_batch([7], ptr, None, 4, 3, check=False)


@pytest.mark.parametrize("epsilon", [0.0, -0.5, 1.0000001, float("nan")])
def test_a_bad_epsilon_raises_the_uncached_calls_error(epsilon):
    import epsilon_uniform_sampler as eps
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(RuntimeError, match=r"^epsilon must be in \(0, 1\]$"):
        eps.sample_batch(ei, ptr, 4, 3, "sample", 42, epsilon)
    with pytest.raises(RuntimeError, match=r"^epsilon must be in \(0, 1\]$"):
        cache.sample_batch([0], ptr, ei, 4, 3, "sample", 42, epsilon)
    with pytest.raises(RuntimeError, match=r"^epsilon must be in \(0, 1\]$"):
        cache.sample_graphs([0], ptr, None, 4, 3, [1], epsilon=epsilon, check=False)


def test_graph_idx_must_match_ptr_in_length():
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(ValueError, match="graph_idx names 2 graphs, ptr holds 1"):
        cache.sample_batch([0, 0], ptr, ei, 4, 3)
    with pytest.raises(ValueError, match="graph_idx"):
        cache.sample_graphs([], ptr, ei, 4, 3, [])


@pytest.mark.parametrize("device", ["cpu", "cuda:1"])
def test_a_device_that_is_not_the_caches_is_a_value_error(device):
    import epsilon_uniform_sampler as eps
    cache = with_graph(make())
    ei, ptr = batch()
    with pytest.raises(ValueError, match="GPU device" if device == "cpu" else "the cache lives on cuda:0"):
        cache.sample_batch([0], ptr, ei, 4, 3, device=device)
    with pytest.raises(ValueError, match="GPU device"):
        eps.GraphCache("cpu")


def test_a_wrong_vertex_count_names_the_graph_and_both_counts():
    cache = with_graph(with_graph(make()), index=1, n=5, slot=1)
    ei = torch.tensor([[0, 1, 3, 4], [1, 0, 4, 3]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"graph 1 of the batch has 4 vertices, the graph added in its place has 5$"):
        cache.sample_batch([0, 1], torch.tensor([0, 3, 7]), ei, 4, 3)
    with pytest.raises(RuntimeError, match=r"graph 1 of the batch has 4 vertices"):
        cache.sample_batch([0, 1], torch.tensor([0, 3, 7]), None, 4, 3, check=False)


def test_a_wrong_column_count_gives_both_counts():
    cache = with_graph(with_graph(make()), index=1, n=4, slot=1, cols=3)
    ei = torch.tensor([[0, 1, 3, 4], [1, 0, 4, 3]], dtype=torch.int64)
    for check in (True, False):
        with pytest.raises(RuntimeError, match=r"the batch has 4 columns, the added graphs have 5$"):
            cache.sample_batch([0, 1], torch.tensor([0, 3, 7]), ei, 4, 3, check=check)


def test_no_edge_index_needs_check_false():
    cache = with_graph(make())
    with pytest.raises(ValueError, match="check=False"):
        cache.sample_batch([0], batch()[1], None, 4, 3)
    with pytest.raises(ValueError, match="check=False"):
        cache.sample_graphs([0], batch()[1], None, 4, 3, [1])


def test_dtype_refusals_have_sample_batchs_texts():
    cache = with_graph(make())
    ei, ptr = batch()
    for call in (lambda e, p: cache.sample_batch([0], p, e, 1, 3), lambda e, p: cache.sample_graphs([0], p, e, 1, 3, [3])):
        with pytest.raises(RuntimeError, match="^edge_index must be int64$"):
            call(ei.to(torch.int32), ptr)
        with pytest.raises(RuntimeError, match="^ptr must be int64$"):
            call(ei, ptr.to(torch.int32))
        with pytest.raises(RuntimeError, match=r"^edge_index must have shape \[2, E\]$"):
            call(ei.reshape(-1), ptr)
    with pytest.raises(RuntimeError, match="^ptr must be int64$"):
        cache.sample_batch([0], ptr.to(torch.int32), None, 1, 3, check=False)


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
