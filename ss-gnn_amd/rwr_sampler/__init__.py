"""rwr_sampler -- MI355X-native drop-in for the reference's `rwr_sampler` extension module
(AniruddhaMandal/SS-GNN src/samplers/rwr_sampler/src/rwr_sampler.cpp:73-307; signature __init__.pyi):
sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42, p_restart=0.2) -> the 5-tuple
(nodes_t, edge_index_t, edge_ptr_t, sample_ptr_t, edge_src_t), int64, returned on the device of `edge_index`.

Random walk with restart, bit-exact with the reference run with one OpenMP thread (its only deterministic setting): one
SplitMix64 stream per graph, its m walks one after the other.  The walks, rows and edges run in HIP kernels (ugs_rwr.hip); the law
is stated in include/ugs_mi355.h at ugs_rwr_sample_batch_begin.  k > 64 and graphs whose 10 n k iteration limit overflows the
reference's int raise RuntimeError.

sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", p_restart=0.2) -> the 5-tuple + failed[G] (bool): graph g
seeded with seeds[g] instead of seed + g (the presample loop batched; law at ugs_rwr_sample_graphs_begin).

Both take the keyword streams="graph" (the default: the law above, unchanged) or streams="row": one SplitMix64 per ROW, seeded
with output s of the graph's generator, so that every walk is independent -- same distribution, reproducible, a row independent of
m and of the other rows, and each row still row 0 of a one-graph, m = 1 call of the reference (law at ugs_rwr_sample_rows_begin).
"""
import ctypes as C

from ugs_sampler import _graphs
from ugs_sampler._lib import lib

__all__ = ["sample_batch", "sample_graphs"]


def _row_streams(streams):
    if streams not in ("graph", "row"):
        raise ValueError("streams must be 'graph' or 'row'")
    return streams == "row"


def sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42, p_restart=0.2, *, streams="graph"):
    """Random-Walk-with-Restart (RWR) connected induced subgraph sampler"""
    md, sd, p = 0 if mode == "sample" else 1, C.c_uint64(int(seed) & _graphs.M64), C.c_double(float(p_restart))
    if _row_streams(streams):
        begin = lambda batch, out: lib.ugs_rwr_sample_rows_begin(*batch, md, sd, None, p, None, *out)
    else:
        begin = lambda batch, out: lib.ugs_rwr_sample_batch_begin(*batch, md, sd, p, *out)
    return _graphs.run_job(begin, lib.ugs_rwr_sample_batch_finish, edge_index, ptr, m_per_graph, k)


def sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", p_restart=0.2, *, streams="graph"):
    """Many one-graph calls in one: graph g's block of m rows equals sample_batch(edge_index, ptr[g:g+2], m_per_graph, k, mode,
    seeds[g], p_restart) with edge_ptr re-based (node ids are batch ids, edge_src -1), with the same `streams`.  A graph whose
    one-graph call would raise (n >= k and 10 n k past the reference's int) gives m rows of -1 and failed[g] = True instead.
    Returns (nodes, edge_index, edge_ptr, sample_ptr, edge_src, failed), on the device of `edge_index`."""
    out, failed = _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode, p_restart, streams=streams)
    return out + (failed.to(out[0].device),)


def _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", p_restart=0.2, device=None, streams="graph"):
    """sample_graphs with `failed` left on the host and the outputs on `device` (PresampleCache.add_many)"""
    p = C.c_double(float(p_restart))
    if _row_streams(streams):
        begin = lambda batch, md, sd, st, out: lib.ugs_rwr_sample_rows_begin(*batch, md, C.c_uint64(0), sd, p, st, *out)
    else:
        begin = lambda batch, md, sd, st, out: lib.ugs_rwr_sample_graphs_begin(*batch, md, sd, p, st, *out)
    return _graphs.sample_graphs(begin, lib.ugs_rwr_sample_batch_finish, edge_index, ptr, m_per_graph, k, seeds, mode, device)
