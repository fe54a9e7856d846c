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

import torch

from ugs_sampler import _graphs
from ugs_sampler._lib import check, lib, vp

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
    if edge_index.dtype != torch.int64:
        raise RuntimeError("edge_index must be int64")
    if ptr.dtype != torch.int64:
        raise RuntimeError("ptr must be int64")
    in_dev = edge_index.device
    ei = edge_index.cpu()
    if ei.dim() != 2 or ei.size(0) != 2:
        raise RuntimeError("edge_index must have shape [2, E]")
    if ei.size(1) > 0 and ei.stride(1) != 1:
        ei = ei.contiguous()
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    m, k = int(m_per_graph), int(k)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if in_dev.type == "cuda":     # device in, device out: the job runs on torch's current stream of that device (see ugs_set_stream)
        idx = in_dev.index if in_dev.index is not None else torch.cuda.current_device()
        check(lib.ugs_set_device(idx))
        check(lib.ugs_set_stream(torch.cuda.current_stream(idx).cuda_stream, 1))
    else:
        if torch.cuda.is_available():
            check(lib.ugs_set_device(torch.cuda.current_device()))
        check(lib.ugs_set_stream(None, 0))
    job, total = vp(), C.c_int64()
    check(lib.ugs_uniform_sample_batch_begin(ei.data_ptr(), ei.stride(0) if ei.size(1) else 0, ei.size(1), pt.data_ptr(), G, m, k,
                                             0 if mode == "sample" else 1, C.c_uint64(seed), C.byref(job), C.byref(total)))
    on_dev = in_dev.type == "cuda"
    try:
        opts = dict(dtype=torch.int64, device=in_dev) if on_dev else dict(dtype=torch.int64, device="cpu", pin_memory=torch.cuda.is_available())
        B = G * m
        nodes = torch.empty((B, k), **opts)
        eidx = torch.empty((2, total.value), **opts)
        eptr = torch.empty((B + 1,), **opts)
        sptr = torch.empty((G + 1,), **opts)
        esrc = torch.empty((total.value,), **opts)
    except BaseException:
        lib.ugs_job_cancel(job)
        raise
    check(lib.ugs_uniform_sample_batch_finish(job, nodes.data_ptr(), eidx.data_ptr(), eptr.data_ptr(), sptr.data_ptr(),
                                              esrc.data_ptr(), 1 if on_dev else 0))
    return nodes, eidx, eptr, sptr, esrc


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
    return _graphs.sample_graphs(lib.ugs_uniform_sample_graphs_begin, lib.ugs_uniform_sample_batch_finish, edge_index, ptr,
                                 m_per_graph, k, seeds, mode, device)
