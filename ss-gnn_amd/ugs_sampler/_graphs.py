"""What the batch entry points of every sampler package share: the view of a batch (`_edge_index_view`), where the outputs go and on
which device and stream the job runs (`_out_opts`, `_select_device`), the two-phase call of uniform_sampler, rwr_sampler and
epsilon_uniform_sampler (`run_job`; `run_rows_job` where the begin reports its own row count), and their sample_graphs on top of it: one call over many graphs, graph g drawn from its own
seed seeds[g] (C ABI: ugs_*_sample_graphs_begin in include/ugs_mi355.h, which states the law)."""
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


def _edge_index_view(edge_index):
    """(tensor kept alive, data pointer, row stride in elements, number of columns) of an int64 [2, E] tensor."""
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise RuntimeError("edge_index must have shape [2, E]")
    if edge_index.size(1) > 0 and edge_index.stride(1) != 1:
        edge_index = edge_index.contiguous()
    stride = edge_index.stride(0) if edge_index.size(1) > 0 else 0
    return edge_index, edge_index.data_ptr(), stride, edge_index.size(1)


def _out_opts(device):
    if device is None:
        return dict(dtype=torch.int64, device="cpu", pin_memory=torch.cuda.is_available()), 0
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("device= must be a GPU device (or None for pinned host tensors)")
    return dict(dtype=torch.int64, device=dev), 1


def _select_device(device, jobs=False):
    """Device of the calling thread's next library calls.  For a job (`jobs`) that returns DEVICE tensors, the job also runs on
    torch's current stream of that device: the outputs come from torch's stream-ordered allocator, and only stream order keeps
    the job's writes behind kernels that may still read a recycled block."""
    if device is not None:
        idx = torch.device(device).index
        idx = idx if idx is not None else torch.cuda.current_device()
        check(lib.ugs_set_device(idx))
        if jobs:
            check(lib.ugs_set_stream(torch.cuda.current_stream(idx).cuda_stream, 1))
        else:
            check(lib.ugs_set_stream(None, 0))       # only a device job runs on the caller's stream: a stale handle must not outlive it
    else:
        if torch.cuda.is_available():
            check(lib.ugs_set_device(torch.cuda.current_device()))
        check(lib.ugs_set_stream(None, 0))


def check_int64(edge_index, ptr):
    if edge_index.dtype != torch.int64:
        raise RuntimeError("edge_index must be int64")
    if ptr.dtype != torch.int64:
        raise RuntimeError("ptr must be int64")


def run_job(begin, finish, edge_index, ptr, m_per_graph, k, device=None, host_job_device=None):
    """The two-phase call of a side sampler: begin (walks and edge counts), five tensors sized by its total, finish (fill and copy).
    `begin(batch, out)` calls the sampler's ugs_*_begin with batch = (ei, row_stride, num_cols, ptr, G, m, k), its own arguments
    behind them, and out = (job, total) last; it returns the status.  A batch on a GPU (or `device`) gives device tensors and runs on
    torch's current stream of that device; a host batch gives pinned host tensors, and its job runs on torch's current device, or on
    `host_job_device` (a call tied to storage on one device).  Returns (nodes, edge_index, edge_ptr, sample_ptr, edge_src)."""
    check_int64(edge_index, ptr)
    in_dev = torch.device(device) if device is not None else edge_index.device
    keep, p, stride, e = _edge_index_view(edge_index.cpu())
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    m, k = int(m_per_graph), int(k)
    dev = in_dev if in_dev.type == "cuda" else None
    if dev is None and host_job_device is not None:
        _select_device(host_job_device)
    else:
        _select_device(dev, jobs=True)
    job, total = vp(), C.c_int64()
    check(begin((p, stride, e, pt.data_ptr(), G, m, k), (C.byref(job), C.byref(total))))
    try:
        opts, on_dev = _out_opts(dev)
        B = G * m
        nodes = torch.empty((B, k), **opts)
        eidx = torch.empty((2, total.value), **opts)
        eptr = torch.empty((B + 1,), **opts)
        sptr = torch.empty((G + 1,), **opts)
        esrc = torch.empty((total.value,), **opts)
    except BaseException:
        lib.ugs_job_cancel(job)
        raise
    check(finish(job, nodes.data_ptr(), eidx.data_ptr(), eptr.data_ptr(), sptr.data_ptr(), esrc.data_ptr(), on_dev))
    return nodes, eidx, eptr, sptr, esrc


def run_rows_job(begin, finish, edge_index, ptr, k, device=None):
    """run_job for a begin that reports its own row count (uniform_sampler.enumerate_graphs): `begin(batch, out)` gets
    batch = (ei, row_stride, num_cols, ptr, G, k) and out = (job, rows, total); the five tensors are sized by rows and total.
    Same placement and stream rules as run_job."""
    check_int64(edge_index, ptr)
    in_dev = torch.device(device) if device is not None else edge_index.device
    keep, p, stride, e = _edge_index_view(edge_index.cpu())
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    k = int(k)
    dev = in_dev if in_dev.type == "cuda" else None
    _select_device(dev, jobs=True)
    job, rows, total = vp(), C.c_int64(), C.c_int64()
    check(begin((p, stride, e, pt.data_ptr(), G, k), (C.byref(job), C.byref(rows), C.byref(total))))
    try:
        opts, on_dev = _out_opts(dev)
        nodes = torch.empty((rows.value, k), **opts)
        eidx = torch.empty((2, total.value), **opts)
        eptr = torch.empty((rows.value + 1,), **opts)
        sptr = torch.empty((G + 1,), **opts)
        esrc = torch.empty((total.value,), **opts)
    except BaseException:
        lib.ugs_job_cancel(job)
        raise
    check(finish(job, nodes.data_ptr(), eidx.data_ptr(), eptr.data_ptr(), sptr.data_ptr(), esrc.data_ptr(), on_dev))
    return nodes, eidx, eptr, sptr, esrc


def sample_graphs(begin, finish, edge_index, ptr, m_per_graph, k, seeds, mode, device=None):
    """run_job with one seed per graph: `begin(batch, mode, seeds, graph_status, out)` calls the sampler's ugs_*_sample_graphs_begin.
    Returns the five tensors on `device` (default: the device of `edge_index`) and the per-graph failures as a host bool tensor [G]."""
    status = []

    def begin_graphs(batch, out):
        G = batch[4]
        sd = seed_array(seeds, max(G, 0))
        status.append(np.zeros(max(G, 1), dtype=np.int32))
        return begin(batch, 0 if mode == "sample" else 1, sd.ctypes.data, status[0].ctypes.data, out)

    five = run_job(begin_graphs, finish, edge_index, ptr, m_per_graph, k, device)
    return five, torch.from_numpy(status[0][:ptr.numel() - 1] != 0)
