"""The CSR form of graphlets.census / vertex_census (form="csr"), the part that needs no device: `_simple_csr` -- item 1 of the census
law as a data structure -- on CPU tensors against uniform_law.graph_adjacency, and the refusals that touch no device.  No GPU: nothing
here launches a kernel."""
import numpy as np
import pytest
import torch

import graphlet_census_law as law
import uniform_law as U


def messy_batch():
    """Duplicate columns, both directions of a column, loops, columns across two graphs, columns with an endpoint in no graph, an empty
    graph and a graph of one vertex."""
    graphs = [(5, [(0, 1), (1, 0), (0, 1), (2, 2), (3, 4), (4, 3), (1, 3), (1, 3)]),
              (0, []),
              (1, [(0, 0)]),
              law.star(4, centre=2),
              (6, [(5, 0), (0, 5), (4, 1), (3, 3), (2, 4)])]
    ei, ptr = law.batch(graphs)
    N = int(ptr[-1])
    extra = np.array([[4, 0, 5, N, -1, 2, N + 3], [5, 6, 7, 1, 3, -2, N + 3]], np.int64)       # crossing, crossing, crossing, outside ...
    ei = np.concatenate([ei[:, :5], extra, ei[:, 5:]], axis=1)
    return np.ascontiguousarray(ei), ptr


def rows_of(rowptr, col):
    rowptr, col = rowptr.tolist(), col.tolist()
    return [col[rowptr[v]:rowptr[v + 1]] for v in range(len(rowptr) - 1)]


def want_rows(ei, ptr):
    """Every vertex's neighbours by the law: graph_adjacency of its graph, loops dropped, global ids ascending."""
    out = [[] for _ in range(int(ptr[0]))]                                      # vertices below the first graph belong to none
    for g in range(len(ptr) - 1):
        lo, n = int(ptr[g]), int(ptr[g + 1] - ptr[g])
        adj = U.graph_adjacency(ei[0], ei[1], lo, n)
        out += [[lo + u for u in range(n) if u != v and adj[v] >> u & 1] for v in range(n)]
    return out


def check_csr(ei_t, ptr_t, ei, ptr):
    from ugs_sampler import graphlets
    rowptr, col = graphlets._simple_csr(ei_t, ptr_t)
    N = int(ptr[-1])
    assert rowptr.dtype == torch.int64 and rowptr.shape == (N + 1,) and col.dtype == torch.int32
    assert rowptr.device == ei_t.device and col.device == ei_t.device
    assert int(rowptr[0]) == 0 and int(rowptr[-1]) == col.numel()
    rows = rows_of(rowptr, col)
    assert rows == want_rows(ei, ptr)
    for v, row in enumerate(rows):
        assert all(a < b for a, b in zip(row, row[1:])) and v not in row       # strictly ascending, no loop
        assert all(v in rows[u] for u in row)                                   # symmetric
    return rows


def test_simple_csr_on_a_messy_batch():
    ei, ptr = messy_batch()
    rows = check_csr(torch.from_numpy(ei), torch.from_numpy(ptr), ei, ptr)
    assert rows[:5] == [[1], [0, 3], [], [1, 4], [3]]                           # duplicates, both directions and the loop are gone
    assert rows[5] == []                                                        # the graph of one vertex, its loop dropped
    assert rows[8] == [6, 7, 9, 10]                                             # the star's centre
    assert sum(len(r) for r in rows) == 2 * (3 + 4 + 3)


def test_simple_csr_strided_and_empty_edge_index():
    ei, ptr = messy_batch()
    E = ei.shape[1]
    spread = torch.zeros((2, 2 * E), dtype=torch.int64)
    spread[:, ::2] = torch.from_numpy(ei)
    wide = torch.zeros((2, E + 3), dtype=torch.int64)
    wide[:, :E] = torch.from_numpy(ei)
    for view in (spread[:, ::2], wide[:, :E]):
        assert not view.is_contiguous()
        check_csr(view, torch.from_numpy(ptr), ei, ptr)
    none = np.zeros((2, 0), np.int64)
    for p in (np.array([0, 3, 3, 9], np.int64), np.array([0], np.int64), np.array([2, 2], np.int64)):
        rows = check_csr(torch.from_numpy(none), torch.from_numpy(p), none, p)
        assert all(r == [] for r in rows) and len(rows) == int(p[-1])


def test_simple_csr_rows_below_the_first_graph_are_empty():
    ei, ptr = law.batch([law.clique(4)])
    ei, ptr = ei + 3, ptr + 3                                                   # ptr[0] = 3
    ei = np.concatenate([ei, np.array([[0, 1, 2], [1, 2, 4]], np.int64)], axis=1)
    from ugs_sampler import graphlets
    rows = rows_of(*graphlets._simple_csr(torch.from_numpy(ei), torch.from_numpy(ptr)))
    assert rows == [[], [], [], [4, 5, 6], [3, 5, 6], [3, 4, 6], [3, 4, 5]]


def test_simple_csr_on_a_random_batch():
    rng = np.random.default_rng(5)
    graphs = []
    for n in (1, 7, 0, 12, 3, 20):
        m = int(rng.integers(0, 3 * n + 1))
        graphs.append((n, [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(m)] if n else []))
    ei, ptr = law.batch(graphs)
    ei = ei[:, rng.permutation(ei.shape[1])]
    check_csr(torch.from_numpy(np.ascontiguousarray(ei)), torch.from_numpy(ptr), ei, ptr)


# ---- the refusals that touch no device ---------------------------------------------------------------------------------------------
def small():
    ei, ptr = law.batch([law.clique(5)])
    return torch.from_numpy(ei), torch.from_numpy(ptr)


@pytest.mark.parametrize("call", ["census", "vertex_census"])
def test_a_bad_form_is_refused_before_anything_else(call):
    from ugs_sampler import graphlets
    fn = getattr(graphlets, call)
    ei, ptr = small()
    for form in ("CSR", "wide", None, 1):
        with pytest.raises(ValueError, match="form"):
            fn(ei, ptr, 3, form=form)
        with pytest.raises(ValueError, match="form"):
            fn("no tensor", ptr, 99, limit=0, form=form)                         # before k, limit and the tensors


@pytest.mark.parametrize("call", ["census", "vertex_census"])
def test_limit_bounds_of_both_forms(call):
    from ugs_sampler import graphlets
    fn = getattr(graphlets, call)
    ei, ptr = small()
    for limit in (0, -1, (1 << 62) + 1, 1 << 63):
        with pytest.raises(ValueError, match=r"limit must be 1 \.\.\. 2\*\*62"):
            fn(ei, ptr, 3, limit=limit, form="csr")
    for limit in (0, (1 << 32) + 1, 1 << 40, 1 << 62):
        with pytest.raises(ValueError, match=r"limit must be 1 \.\.\. 2\*\*32"):
            fn(ei, ptr, 3, limit=limit, form="bitmap")
        with pytest.raises(ValueError, match=r"limit must be 1 \.\.\. 2\*\*32"):
            fn(ei, ptr, 3, limit=limit)


@pytest.mark.parametrize("call", ["census", "vertex_census"])
def test_k_bounds_of_the_csr_form(call):
    from ugs_sampler import graphlets
    fn = getattr(graphlets, call)
    ei, ptr = small()
    with pytest.raises(RuntimeError, match="1 <= k <= 7"):
        fn(ei, ptr, 8, form="csr")
    for k in (0, 9, -1):
        with pytest.raises(RuntimeError, match="1 <= k <= 8"):
            fn(ei, ptr, k, form="csr")
    with pytest.raises(TypeError):
        fn(ei, ptr, 3.0, form="csr")


def test_the_c_entries_state_their_refusals_without_a_device():
    from ugs_sampler._lib import lib
    E_BAD_ARG, E_UNSUPPORTED = -4, -7
    census = lambda N, M, k, limit: lib.ugs_graphlet_census_csr(None, 0, None, None, N, M, k, limit, None, 0, None, None, None)
    vertex = lambda N, M, k, limit: lib.ugs_graphlet_vertex_census_csr(None, 0, None, None, N, M, k, limit, 0, None, 0, None, None, None)
    for fn in (census, vertex):
        assert fn(0, 0, 8, 1) == E_UNSUPPORTED and fn(0, 0, 0, 1) == E_UNSUPPORTED and fn(0, 0, 9, 1) == E_UNSUPPORTED
        assert fn(0, 0, 3, 0) == E_BAD_ARG and fn(0, 0, 3, (1 << 62) + 1) == E_BAD_ARG
        assert fn(1 << 31, 0, 3, 1) == E_UNSUPPORTED and fn(5, 1 << 31, 3, 1) == E_UNSUPPORTED
        assert fn(5, 4, 3, 1 << 62) == E_BAD_ARG                                # the limits hold: now the pointers are missing
