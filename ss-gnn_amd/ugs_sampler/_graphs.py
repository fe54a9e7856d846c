"""Shared body of uniform_sampler.sample_graphs and rwr_sampler.sample_graphs: one call over many graphs, graph g drawn from its
own seed seeds[g] (C ABI: ugs_*_sample_graphs_begin in include/ugs_mi355.h, which states the law)."""
import ctypes as C

import numpy as np
import torch

from ._lib import check, lib, vp

M64 = (1 << 64) - 1


def seed_array(seeds, G):
    """seeds (a sequence, or an int64 / uint64 tensor or array) as a contiguous uint64 numpy array of length G, values mod 2^64."""
    if torch.is_tensor(seeds):
        if seeds.dtype not in (torch.int64, torch.uint64):
            raise RuntimeError("seeds must be an int64 or uint64 tensor")
        a = seeds.detach().cpu().contiguous().view(torch.int64).numpy().view(np.uint64)     # two's complement = mod 2^64
    elif isinstance(seeds, np.ndarray) and seeds.dtype in (np.int64, np.uint64):
        a = seeds.view(np.uint64)
    else:
        a = np.array([int(s) & M64 for s in seeds], dtype=np.uint64)
    a = np.ascontiguousarray(a).reshape(-1)
    if a.shape[0] != G:
        raise RuntimeError(f"seeds must hold one seed per graph ({G}), got {a.shape[0]}")
    return a


def sample_graphs(begin, finish, edge_index, ptr, m_per_graph, k, seeds, mode, device=None):
    """Runs begin(ei, row_stride, num_cols, ptr, G, m, k, mode, seeds, graph_status, job, total) and finish.  Returns the five
    tensors on `device` (default: the device of `edge_index`) and the per-graph failures as a host bool tensor [G]."""
    if edge_index.dtype != torch.int64:
        raise RuntimeError("edge_index must be int64")
    if ptr.dtype != torch.int64:
        raise RuntimeError("ptr must be int64")
    in_dev = torch.device(device) if device is not None else edge_index.device
    ei = edge_index.cpu()
    if ei.dim() != 2 or ei.size(0) != 2:
        raise RuntimeError("edge_index must have shape [2, E]")
    if ei.size(1) > 0 and ei.stride(1) != 1:
        ei = ei.contiguous()
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    m, k = int(m_per_graph), int(k)
    sd = seed_array(seeds, max(G, 0))
    status = np.zeros(max(G, 1), dtype=np.int32)
    if in_dev.type == "cuda":     # device in, device out: the job runs on torch's current stream of that device (see ugs_set_stream)
        idx = in_dev.index if in_dev.index is not None else torch.cuda.current_device()
        check(lib.ugs_set_device(idx))
        check(lib.ugs_set_stream(torch.cuda.current_stream(idx).cuda_stream, 1))
    else:
        if torch.cuda.is_available():
            check(lib.ugs_set_device(torch.cuda.current_device()))
        check(lib.ugs_set_stream(None, 0))
    job, total = vp(), C.c_int64()
    check(begin(ei.data_ptr(), ei.stride(0) if ei.size(1) else 0, ei.size(1), pt.data_ptr(), G, m, k, 0 if mode == "sample" else 1,
                sd.ctypes.data, status.ctypes.data, C.byref(job), C.byref(total)))
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
    check(finish(job, nodes.data_ptr(), eidx.data_ptr(), eptr.data_ptr(), sptr.data_ptr(), esrc.data_ptr(), 1 if on_dev else 0))
    return (nodes, eidx, eptr, sptr, esrc), torch.from_numpy(status[:G] != 0)
