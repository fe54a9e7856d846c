"""epsilon_uniform_sampler.GraphCache: the adjacency lists of every graph of a dataset built once, by a kernel, and kept on the
device; a training step over any batch of added graphs then runs only the walks, the scan and the fill (C ABI and contract:
include/ugs_mi355.h at ugs_eps_cache_sample_begin; layout, the build kernel and generations: DESIGN.md section 16; what it shares
with the other samplers' caches: ugs_sampler/_dataset_cache.py)."""
import ctypes as C

import numpy as np
import torch

from ugs_sampler import _graphs
from ugs_sampler._dataset_cache import DatasetCache
from ugs_sampler._lib import check as _check
from ugs_sampler._lib import lib

# add_many's call bound: columns and vertices per device call (the host stages 8 bytes per column, the build 4 per vertex)
CHUNK_COLUMNS = 1 << 24


class GraphCache(DatasetCache):
    """The adjacency lists of a dataset's graphs, built once and kept on `device`, for every k and epsilon.

        cache = GraphCache("cuda:0")
        cache.add_many(range(len(dataset)), [(d.edge_index, d.num_nodes) for d in dataset])             # start-up
        five = cache.sample_batch(batch.graph_idx, batch.ptr, batch.edge_index, m, k, mode, seed, eps)  # every step

    If the batch's columns are, graph by graph in batch order, the columns of the graphs added under graph_idx[g], in the order
    given and shifted by ptr[g] -- what collating those graphs produces -- cache.sample_batch equals
    epsilon_uniform_sampler.sample_batch(edge_index, ptr, m, k, mode, seed, epsilon) in all five tensors, bit for bit, and
    cache.sample_graphs equals epsilon_uniform_sampler.sample_graphs likewise in all six.

    check=True (the default) uploads the batch's edge_index and compares every column with the stored one, exactly: any other
    batch raises RuntimeError, also one that merely permutes a graph's columns.  check=False reads nothing of the batch but ptr
    (edge_index may be None): the result is that of the added graphs, whatever the batch holds.

    The outputs are tensors on the cache's device, on torch's current stream.  Adding an index again gives it a new slot (the old
    bytes stay until close).  reserve=(vertices, columns) sizes the first allocation; the storage grows by doubling, and a call
    begun before an add finishes on the buffers it started with.  Adds are exclusive among themselves; any number of threads may
    sample meanwhile."""

    SAMPLER, ENTRIES, CHUNK = "epsilon_uniform_sampler", "half_edges", CHUNK_COLUMNS
    _destroy, _info = staticmethod(lib.ugs_eps_cache_destroy), staticmethod(lib.ugs_eps_cache_info)

    def __init__(self, device, *, reserve=(0, 0)):
        super().__init__(device, reserve, lib.ugs_eps_cache_create)

    def _add(self, run, ei, ptr, slots):
        _check(lib.ugs_eps_cache_add(self._handle(), ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(run), slots.ctypes.data))

    def _job(self, graph_idx, ptr, edge_index, m_per_graph, k, mode, seed, seeds, epsilon, check, device):
        self._check_batch(ptr, edge_index, check)
        if not (epsilon > 0.0 and epsilon <= 1.0):                     # (the uncached call's check and text)
            raise RuntimeError("epsilon must be in (0, 1]")
        dev = self._own_device(device)
        gi, G = self._graphs_of(graph_idx, ptr)
        pt = ptr.detach().cpu().contiguous()
        slots = self._slots_of(gi, pt.tolist(), edge_index)
        cache = self._handle()
        md, eps = 0 if mode == "sample" else 1, C.c_double(float(epsilon))
        sd = _graphs.seed_array(seeds, max(G, 0)) if seeds is not None else None
        status = np.zeros(max(G, 1), np.int32)
        given = edge_index is not None and bool(check)                   # without the check the columns stay where they are

        def begin(batch, out):
            ei = batch[:3] if given else (None, 0, 0)
            return lib.ugs_eps_cache_sample_begin(cache, slots.ctypes.data, *ei, *batch[3:7], md, C.c_uint64(int(seed) & _graphs.M64),
                                                  sd.ctypes.data if sd is not None else None, eps, 1 if check else 0,
                                                  status.ctypes.data if sd is not None else None, *out)

        batch_ei = edge_index.detach().cpu() if given else torch.empty((2, 0), dtype=torch.int64)
        return _graphs.run_job(begin, lib.ugs_eps_sample_batch_finish, batch_ei, pt, m_per_graph, k, dev)

    def sample_batch(self, graph_idx, ptr, edge_index, m_per_graph, k, mode="sample", seed=42, epsilon=0.1, *, check=True, device=None):
        """epsilon_uniform_sampler.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed, epsilon) for a batch whose graph g is the
        graph added under graph_idx[g]; tensors on the cache's device.  Before any device work: KeyError for an index never added,
        ValueError if graph_idx and ptr disagree in length, if `device` is not the cache's and for edge_index=None without
        check=False, RuntimeError naming the graph for a wrong vertex count, for a wrong column total, and the uncached call's
        for epsilon, k and m_per_graph.  With check, after the device work: RuntimeError "graph g of the batch differs from the
        graph added in its place", g the smallest such."""
        return self._job(graph_idx, ptr, edge_index, m_per_graph, k, mode, seed, None, epsilon, check, device)

    def sample_graphs(self, graph_idx, ptr, edge_index, m_per_graph, k, seeds, mode="sample", epsilon=0.1, *, check=True, device=None):
        """epsilon_uniform_sampler.sample_graphs for such a batch: the five tensors on the cache's device and failed [G], all
        False, on the host as there; seeds are taken mod 2^64."""
        five = self._job(graph_idx, ptr, edge_index, m_per_graph, k, mode, 0, seeds, epsilon, check, device)
        return five + (torch.zeros(max(ptr.numel() - 1, 0), dtype=torch.bool),)

    def graph_csr(self, index):
        """(rowptr [n + 1], nbr, ecs) of the graph added under `index`, copied back from the device: rowptr relative to the graph,
        nbr the local neighbour, ecs = 2 * (column inside the graph) + side.  A read-only diagnostic."""
        slot, n, ncol = self._slot[int(index)]
        rowptr, nbr, ecs = np.zeros(n + 1, np.int64), np.zeros(2 * ncol, np.int32), np.zeros(2 * ncol, np.int32)
        nn, ne = C.c_int64(), C.c_int64()
        _graphs._select_device(self.dev)
        _check(lib.ugs_eps_cache_graph_csr(self._handle(), slot, n, 2 * ncol, C.byref(nn), C.byref(ne), rowptr.ctypes.data, nbr.ctypes.data,
                                           ecs.ctypes.data))
        assert (nn.value, ne.value) == (n, 2 * ncol)
        return rowptr, nbr, ecs

    def info(self):
        """graphs (indices held), vertices (entries of the row-offset array: vertices plus one per graph added), half_edges, bytes
        of the device storage and generations (allocations so far); what replaced graphs held stays counted until close"""
        return super().info()
