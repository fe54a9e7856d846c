"""epsilon_uniform_sampler -- MI355X-native drop-in for the reference's `epsilon_uniform_sampler` extension module
(AniruddhaMandal/SS-GNN src/samplers/epsilon_uniform_sampler/src/epsilon_uniform_sampler.cpp:122-377; pybind signature
:366-377): sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42, epsilon=0.1) -> the 5-tuple
(nodes_t, edge_index_t, edge_ptr_t, sample_ptr_t, edge_src_t), int64, returned on the device of `edge_index`.

Sampling runs in HIP kernels (one lane per sample, counter-based generator per (row, attempt)).  The reference is not
deterministic for this sampler (per-thread generators seeded with the OpenMP thread id, dynamic schedule, rows written in
completion order); this implementation is deterministic in (seed, row) and its parity with the reference is statistical:
same growth law, same acceptance law min(1, eps/(w+eps)), same attempt budget max(10, 10/eps), same output format.

sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", epsilon=0.1) -> the 5-tuple + failed[G] (bool, all False):
graph g's rows keyed by (seeds[g], row inside the graph) instead of (seed, batch row) -- the presample loop batched; law at
ugs_eps_sample_graphs_begin.

GraphCache(device) builds the adjacency lists of every dataset graph once, on the device (add / add_many), and keeps them there:
cache.sample_batch / cache.sample_graphs over any batch of added graphs equal the module's calls bit for bit, for every k and
epsilon, while running only the walks, the scan and the fill.  Contract at ugs_eps_cache_sample_begin.
"""
import ctypes as C

from ugs_sampler import _graphs
from ugs_sampler._lib import lib

from .graph_cache import GraphCache

__all__ = ["sample_batch", "sample_graphs", "_sample_graphs", "GraphCache"]


def sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42, epsilon=0.1):
    """Epsilon-uniform connected subgraph sampling via random walk with rejection sampling"""
    _graphs.check_int64(edge_index, ptr)          # (before epsilon, as ever)
    if not (epsilon > 0.0 and epsilon <= 1.0):
        raise RuntimeError("epsilon must be in (0, 1]")
    return _graphs.run_job(lambda batch, out: lib.ugs_eps_sample_batch_begin(*batch, 0 if mode == "sample" else 1,
                                                                             C.c_uint64(int(seed) & _graphs.M64),
                                                                             C.c_double(float(epsilon)), *out),
                           lib.ugs_eps_sample_batch_finish, edge_index, ptr, m_per_graph, k)


def sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", epsilon=0.1):
    """Many one-graph calls in one: graph g's block of m rows equals sample_batch(edge_index, ptr[g:g+2], m_per_graph, k, mode,
    seeds[g], epsilon) with edge_ptr re-based (node ids are batch ids, edge_src batch columns).  No graph fails alone: a graph
    with fewer than k vertices gives m rows of -1, and failed is all False.
    Returns (nodes, edge_index, edge_ptr, sample_ptr, edge_src, failed), the five on the device of `edge_index`, failed on the host."""
    out, failed = _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode, epsilon)
    return out + (failed,)


def _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", epsilon=0.1, device=None):
    """sample_graphs with the outputs on `device` (PresampleCache.add_many)"""
    if not (epsilon > 0.0 and epsilon <= 1.0):
        raise RuntimeError("epsilon must be in (0, 1]")
    eps = C.c_double(float(epsilon))
    return _graphs.sample_graphs(lambda batch, md, sd, st, out: lib.ugs_eps_sample_graphs_begin(*batch, md, sd, eps, st, *out),
                                 lib.ugs_eps_sample_batch_finish, edge_index, ptr, m_per_graph, k, seeds, mode, device)
