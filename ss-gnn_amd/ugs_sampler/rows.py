"""Repeated subgraphs of a sampler's output, merged on the GPU.

Every sampler here hands the SS-GNN encoder G * m rows, and on small graphs many of them are the same subgraph drawn again.  The
encoder (`encode_subgraphs`) is a pure function of each row and pools over the k vertices whatever their order, so it needs each
distinct subgraph once:

    from ugs_sampler import rows
    u = rows.unique_rows(nodes_t, edge_index_t, edge_ptr_t, sample_ptr_t, edge_src_t, ptr=batch.ptr, by="set")
    emb = model.encode_subgraphs(x, edge_attr, u.nodes, u.edge_index, u.edge_ptr, u.edge_src)[u.inverse]   # [R, H] as before

The law is stated in include/ugs_mi355.h at ugs_rows_unique_begin: within a graph, row r is kept iff no earlier row of that graph
has its key -- its k entries in order (by="sequence") or sorted (by="set"); kept rows keep their order and are copied unchanged
with their spans of edge_index and edge_src; count[u] is how many rows have kept row u's key and inverse[r] is where the kept row
with r's key went.  Keys are exact (128 bits, no hashing).  Limits: 1 <= k <= 32, at most 4096 rows per graph, at most
2^min(31, 128 // k) - 1 vertices in a graph that has rows (65 535 at k = 8, 2 M at k = 6).
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _select_device
from ._lib import check, lib, vp
from .wl import _gpu_of

__all__ = ["unique_rows", "last_launch", "UniqueRows"]

UniqueRows = namedtuple("UniqueRows", ["nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src", "count", "inverse"])
_BY = {"sequence": 0, "set": 1}


def _check_inputs(nodes, edge_index, edge_ptr, sample_ptr, edge_src, ptr, by):
    named = ((nodes, "nodes_sampled"), (edge_index, "edge_index_sampled"), (edge_ptr, "edge_ptr"), (sample_ptr, "sample_ptr"),
             (edge_src, "edge_src"), (ptr, "ptr"))
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {t.dtype}")
    if not isinstance(by, str):
        raise TypeError("by must be 'set' or 'sequence'")
    if by not in _BY:
        raise ValueError(f"by must be 'set' or 'sequence', got {by!r}")
    if nodes.dim() != 2:
        raise ValueError("nodes_sampled must have shape [R, k]")
    R, k = nodes.shape
    if not 1 <= k <= 32:
        raise ValueError(f"1 <= k <= 32, got k = {k}")
    if R >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows")
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("edge_index_sampled must have shape [2, E]")
    Es = edge_index.size(1)
    if edge_ptr.dim() != 1 or edge_ptr.numel() != R + 1:
        raise ValueError("edge_ptr must have shape [R + 1]")
    if sample_ptr.dim() != 1 or sample_ptr.numel() < 1:
        raise ValueError("sample_ptr must have shape [G + 1]")
    if ptr.dim() != 1 or ptr.numel() != sample_ptr.numel():
        raise ValueError("ptr must have shape [G + 1], like sample_ptr")
    if edge_src.dim() != 1 or edge_src.numel() not in (0, Es):
        raise ValueError("edge_src must have shape [E], or be empty")
    five = (nodes, edge_index, edge_ptr, sample_ptr, edge_src)
    if any(t.device != nodes.device for t in five):
        raise ValueError("nodes_sampled, edge_index_sampled, edge_ptr, sample_ptr and edge_src must be on one device")
    if nodes.device.type not in ("cpu", "cuda") or ptr.device.type not in ("cpu", "cuda"):
        raise ValueError("tensors must be on the CPU or on a GPU")
    if nodes.device.type == "cpu":                       # host arrays are checked here; device arrays by the kernels
        for t, name, end, what in ((sample_ptr, "sample_ptr", R, "rows"), (edge_ptr, "edge_ptr", Es, "edge entries")):
            if int(t[0]) != 0 or int(t[-1]) != end or bool((t[1:] < t[:-1]).any()):
                raise ValueError(f"{name} must start at 0, must not decrease and must end at the number of {what} ({end})")


def unique_rows(nodes_sampled, edge_index_sampled, edge_ptr, sample_ptr, edge_src, *, ptr, by="set", device=None):
    """The distinct rows of a sampler's five tensors, per graph: a named tuple (nodes [U, k], edge_index [2, Eu], edge_ptr [U + 1],
    sample_ptr [G + 1], edge_src [Eu], count [U], inverse [R]), all int64 (module docstring; the law: include/ugs_mi355.h).

    `ptr` is the batch's ptr [G + 1] (either side): the key of a row codes its entries relative to its graph.  `edge_src` may be
    an empty tensor, and then so is the result's.  Device tensors are used in place and the results stay there, on torch's current
    stream; CPU tensors are copied to `device` (default: the current GPU) and the results come back on the CPU.  One read-back
    (U, Eu and the status of the device checks) separates the two phases.

    ValueError / TypeError before any device work: wrong dtypes, shapes or devices, `by`, k, and for host tensors a sample_ptr or
    edge_ptr that decreases or does not end at R or E.  RuntimeError naming the first offending graph or row, from the kernels'
    checks: a graph over the row or vertex limit, an entry below -1 or outside its graph, device pointer arrays that are not
    monotone or do not end at R or E.  Nothing is returned then, and the next call works as usual."""
    _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, sample_ptr, edge_src, ptr, by)
    dev, back = _gpu_of(nodes_sampled, device)
    _select_device(dev, jobs=True)
    nodes, eptr, sptr = nodes_sampled.to(dev).contiguous(), edge_ptr.to(dev).contiguous(), sample_ptr.to(dev).contiguous()
    eidx, esrc, bptr = edge_index_sampled.to(dev), edge_src.to(dev).contiguous(), ptr.to(dev).contiguous()
    R, k = nodes.shape
    G, Es = sptr.numel() - 1, eidx.size(1)
    if Es > 0 and eidx.stride(1) != 1:
        eidx = eidx.contiguous()
    in_stride = eidx.stride(0) if Es > 0 else 0
    job, U, Eu = vp(), C.c_int64(), C.c_int64()
    check(lib.ugs_rows_unique_begin(nodes.data_ptr() if R > 0 else None, k, R, eptr.data_ptr(), Es, sptr.data_ptr(), G, bptr.data_ptr(),
                                    _BY[by], C.byref(job), C.byref(U), C.byref(Eu)))
    try:
        opts = dict(dtype=torch.int64, device=dev)
        has_src = esrc.numel() > 0
        out = UniqueRows(torch.empty((U.value, k), **opts), torch.empty((2, Eu.value), **opts), torch.empty((U.value + 1,), **opts),
                         torch.empty((G + 1,), **opts), torch.empty((Eu.value if has_src else 0,), **opts), torch.empty((U.value,), **opts),
                         torch.empty((R,), **opts))
    except BaseException:
        lib.ugs_job_cancel(job)
        raise
    ptr_or_none = lambda t: t.data_ptr() if t.numel() > 0 else None      # noqa: E731
    check(lib.ugs_rows_unique_finish(job, ptr_or_none(out.nodes), ptr_or_none(eidx), in_stride, esrc.data_ptr() if has_src else None,
                                     ptr_or_none(out.edge_index), Eu.value, out.edge_ptr.data_ptr(), out.sample_ptr.data_ptr(),
                                     out.edge_src.data_ptr() if has_src and Eu.value > 0 else None, ptr_or_none(out.count), ptr_or_none(out.inverse)))
    return UniqueRows(*(t.cpu() for t in out)) if back else out


def last_launch():
    """The dedup kernel forms the calling thread's last unique_rows used: "wave" (graphs of at most 64 rows), "workgroup" (65 to
    4096 rows), "wave+workgroup", or "none" (no rows, or a refused call)."""
    buf = C.create_string_buffer(32)
    check(lib.ugs_rows_last_launch(buf, len(buf)))
    return buf.value.decode()
