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
"""
import ctypes as C

from ugs_sampler import _graphs
from ugs_sampler._lib import check, lib

__all__ = ["sample_batch", "sample_graphs", "set_max_vertices", "max_vertices"]


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
