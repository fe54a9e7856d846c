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
"""
import ctypes as C

import torch

from ugs_sampler import _graphs
from ugs_sampler._lib import check, lib, vp

__all__ = ["sample_batch", "sample_graphs"]


def sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42, p_restart=0.2):
    """Random-Walk-with-Restart (RWR) connected induced subgraph sampler"""
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
    m, k, p = int(m_per_graph), int(k), float(p_restart)
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
    check(lib.ugs_rwr_sample_batch_begin(ei.data_ptr(), ei.stride(0) if ei.size(1) else 0, ei.size(1), pt.data_ptr(), G, m, k,
                                         0 if mode == "sample" else 1, C.c_uint64(seed), C.c_double(p), C.byref(job), C.byref(total)))
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
    check(lib.ugs_rwr_sample_batch_finish(job, nodes.data_ptr(), eidx.data_ptr(), eptr.data_ptr(), sptr.data_ptr(),
                                          esrc.data_ptr(), 1 if on_dev else 0))
    return nodes, eidx, eptr, sptr, esrc


def sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", p_restart=0.2):
    """Many one-graph calls in one: graph g's block of m rows equals sample_batch(edge_index, ptr[g:g+2], m_per_graph, k, mode,
    seeds[g], p_restart) with edge_ptr re-based (node ids are batch ids, edge_src -1).  A graph whose one-graph call would raise
    (n >= k and 10 n k past the reference's int) gives m rows of -1 and failed[g] = True instead.
    Returns (nodes, edge_index, edge_ptr, sample_ptr, edge_src, failed), on the device of `edge_index`."""
    out, failed = _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode, p_restart)
    return out + (failed.to(out[0].device),)


def _sample_graphs(edge_index, ptr, m_per_graph, k, seeds, mode="sample", p_restart=0.2, device=None):
    """sample_graphs with `failed` left on the host and the outputs on `device` (PresampleCache.add_many)"""
    p = C.c_double(float(p_restart))
    return _graphs.sample_graphs(lambda ei, rs, nc, pt, G, m, kk, md, sd, st, job, tot:
                                 lib.ugs_rwr_sample_graphs_begin(ei, rs, nc, pt, G, m, kk, md, sd, p, st, job, tot),
                                 lib.ugs_rwr_sample_batch_finish, edge_index, ptr, m_per_graph, k, seeds, mode, device)
