"""uniform_sampler -- MI355X-native drop-in for the reference's `uniform_sampler` extension module
(AniruddhaMandal/SS-GNN src/samplers/uniform_sampler/src/uniform_sampler.cpp:86-285; signature __init__.pyi):
sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42) -> the 5-tuple
(nodes_t, edge_index_t, edge_ptr_t, sample_ptr_t, edge_src_t), int64, returned on the device of `edge_index`.

Exact uniform sampling over every connected k-subset of each graph, bit-exact with the reference: the subsets are enumerated,
ordered and drawn from (std::mt19937_64 + libstdc++'s uniform_int_distribution) in HIP kernels (ugs_uniform.hip).  The law is
stated in include/ugs_mi355.h at ugs_uniform_sample_batch_begin.  By default graphs of more than 64 vertices (with at least k
of them) raise RuntimeError, as does a batch with more connected k-subsets than the device budget.

set_max_vertices(n) -> previous raises that limit for the process, to 1024 at most: graphs of 65 to n vertices are then sampled
too (k <= 8 and k * bit_length(n_g - 1) <= 64: 1024 vertices up to k = 6, 512 at k = 7, 256 at k = 8), by the same law.  Nothing
raises it implicitly; a trainer on PROTEINS or IMDB-BINARY calls it once at start-up, or sets UGS_UNIFORM_MAX_VERTICES in the
environment.  max_vertices() reads it.

sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample") -> the 5-tuple + failed[G] (bool): one call for many
one-graph calls, graph g drawn from its own std::mt19937_64(seeds[g]) by its own workgroup (the presample loop batched; law at
ugs_uniform_sample_graphs_begin; a graph sample_batch would refuse fails alone).

enumerate_graphs(edge_index, ptr, k, mode="sample", *, max_rows=1 << 22, device=None) -> the 5-tuple + failed[G]: every connected
k-subset of every graph as a row, in the order the samplers draw from (row sample_ptr[g] + d is the row a draw d gives), with its
edges; count_graphs(edge_index, ptr, k, *, limit=1 << 25) -> (counts[G], failed[G]): |S_g| alone, without storing a set.  Law at
ugs_uniform_enumerate_begin.
"""
import ctypes as C

import numpy as np
import torch

from ugs_sampler import _graphs
from ugs_sampler._lib import check, lib

__all__ = ["sample_batch", "sample_graphs", "enumerate_graphs", "count_graphs", "set_max_vertices", "max_vertices"]


def set_max_vertices(n):
    """Largest graph (vertices) sample_batch / sample_graphs / PresampleCache enumerate, 64 ... 1024, for the whole process.
    Returns the previous value; a value out of range raises RuntimeError and changes nothing."""
    prev = C.c_int()
    check(lib.ugs_uniform_set_max_vertices(int(n), C.byref(prev)))
    return prev.value


def max_vertices():
    """The limit in force (default 64, or UGS_UNIFORM_MAX_VERTICES from the environment)"""
    return int(lib.ugs_uniform_max_vertices())


def _set_mask_vertices(n):
    """Testing and measurement aid: graphs of up to n vertices (0 ... 64, default 64) take the 64-bit mask form, smaller ones that
    fit the wide rule go through the wide kernels.  Same tensors either way.  Returns the previous value."""
    prev = C.c_int()
    check(lib.ugs_uniform_set_mask_vertices(int(n), C.byref(prev)))
    return prev.value


def sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42):
    """Sample truly uniform connected k-subgraphs from batched graphs"""
    return _graphs.run_job(lambda batch, out: lib.ugs_uniform_sample_batch_begin(*batch, 0 if mode == "sample" else 1,
                                                                                 C.c_uint64(int(seed) & _graphs.M64), *out),
                           lib.ugs_uniform_sample_batch_finish, edge_index, ptr, m_per_graph, k)


def sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample"):
    """Many one-graph calls in one: graph g's block of m rows equals sample_batch(edge_index, ptr[g:g+2], m_per_graph, k, mode,
    seeds[g]) with edge_ptr re-based (node ids are batch ids, edge_src batch column positions).  A graph whose one-graph call
    would raise (at least k vertices and more than max_vertices() allows, more connected k-subsets than the device budget) gives m rows of -1 and
    failed[g] = True instead; healthy graphs that together exceed the budget raise RuntimeError (split the call).
    Returns (nodes, edge_index, edge_ptr, sample_ptr, edge_src, failed), on the device of `edge_index`."""
    out, failed = _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode)
    return out + (failed.to(out[0].device),)


def _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", device=None):
    """sample_graphs with `failed` left on the host and the outputs on `device` (PresampleCache.add_many)"""
    return _graphs.sample_graphs(lambda batch, md, sd, st, out: lib.ugs_uniform_sample_graphs_begin(*batch, md, sd, st, *out),
                                 lib.ugs_uniform_sample_batch_finish, edge_index, ptr, m_per_graph, k, seeds, mode, device)


def enumerate_graphs(edge_index, ptr, k, mode="sample", *, max_rows=1 << 22, device=None):
    """Every connected k-subset of every graph: graph g's rows [sample_ptr[g], sample_ptr[g+1]) are its sets in lexicographic order
    of the ascending vertex tuples (batch ids, never -1), edges and edge_src as sample_batch writes them; row sample_ptr[g] + d is
    the row sample_batch / sample_graphs emit when the graph's generator draws d.  A graph the samplers refuse for its size, or
    with more than max_rows sets of its own, gives no rows and failed[g] = True; healthy graphs with more than max_rows sets
    together raise RuntimeError (split the call).  max_rows: 1 ... 2**25 (ValueError otherwise).
    Returns (nodes [R, k], edge_index [2, E], edge_ptr [R+1], sample_ptr [G+1], edge_src [E], failed [G] host bool): pinned host
    tensors for host input, else on the input's device (or `device`), on torch's current stream."""
    max_rows = int(max_rows)
    if not 1 <= max_rows <= 1 << 25:
        raise ValueError(f"max_rows must be 1 ... 2**25, got {max_rows}")
    status = []

    def begin(batch, out):
        status.append(np.zeros(max(batch[4], 1), dtype=np.int32))
        return lib.ugs_uniform_enumerate_begin(*batch, 0 if mode == "sample" else 1, max_rows, status[0].ctypes.data, *out)

    five = _graphs.run_rows_job(begin, lib.ugs_uniform_enumerate_finish, edge_index, ptr, k, device)
    return five + (torch.from_numpy(status[0][:ptr.numel() - 1] != 0),)


def count_graphs(edge_index, ptr, k, *, limit=1 << 25):
    """|S_g| of every graph without storing a set: (counts [G] host int64, failed [G] host bool).  counts[g] is exact wherever it
    is at most `limit`; a graph with more sets, or one the samplers refuse for its size, has counts[g] = -1 and failed[g] = True.
    The work per graph is bounded by `limit` (1 ... 2**32, ValueError otherwise); no key array is allocated."""
    limit = int(limit)
    if not 1 <= limit <= 1 << 32:
        raise ValueError(f"limit must be 1 ... 2**32, got {limit}")
    _graphs.check_int64(edge_index, ptr)
    keep, p, stride, e = _graphs._edge_index_view(edge_index.cpu())
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    _graphs._select_device(edge_index.device if edge_index.device.type == "cuda" else None)
    counts = np.zeros(max(G, 1), dtype=np.int64)
    status = np.zeros(max(G, 1), dtype=np.int32)
    check(lib.ugs_uniform_count_graphs(p, stride, e, pt.data_ptr(), G, int(k), limit, counts.ctypes.data, status.ctypes.data))
    return torch.from_numpy(counts[:max(G, 0)]), torch.from_numpy(status[:max(G, 0)] != 0)
