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

GraphCache(k, device) builds the CSR of every dataset graph once (add / add_many) and keeps it on the device: cache.sample_batch /
cache.sample_graphs over any batch of added graphs equal the module's calls bit for bit, with either `streams`, while running
only the walks, the scan and the fill.  Contract at ugs_rwr_cache_sample_begin.
"""
import ctypes as C

import numpy as np
import torch

from ugs_sampler import _graphs
from ugs_sampler._dataset_cache import DatasetCache
from ugs_sampler._lib import check as _check
from ugs_sampler._lib import lib

__all__ = ["sample_batch", "sample_graphs", "GraphCache"]


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


# add_many's call bound: columns and vertices per device call (the build's scratch is 56 bytes per column)
CHUNK_COLUMNS = 1 << 24


class GraphCache(DatasetCache):
    """The CSRs of a dataset's graphs, built once and kept on `device`, for one k.

        cache = GraphCache(k, "cuda:0")
        cache.add_many(range(len(dataset)), [(d.edge_index, d.num_nodes) for d in dataset])          # start-up
        five = cache.sample_batch(batch.graph_idx, batch.ptr, batch.edge_index, m, mode, seed)       # every step

    If the batch's columns are, graph by graph in batch order, the columns of the graphs added under graph_idx[g], each shifted
    by ptr[g] -- what collating those graphs produces -- cache.sample_batch equals rwr_sampler.sample_batch(edge_index, ptr, m, k,
    mode, seed, p_restart, streams=streams) in all five tensors and cache.sample_graphs equals rwr_sampler.sample_graphs in all six.
    check=True (the default) uploads the batch's edge_index and compares every column with the stored one, exactly: any other
    batch raises RuntimeError, also one whose columns are merely permuted.  check=False reads nothing of the batch but ptr
    (edge_index may be None): the result is that of the added graphs, whatever the batch holds.

    A graph with n >= k and 10 n k past the reference's int is recorded in `failed` and takes no storage: sample_batch on a batch
    that names it raises the uncached call's RuntimeError, sample_graphs gives it m rows of -1 and failed[g] = True.  Adding an
    index again replaces it (the old bytes stay until close).  reserve=(vertices, columns) sizes the first allocation; the storage
    grows by doubling, and a call begun before an add finishes on the buffers it started with.  Adds are exclusive; any number of
    threads may sample at once."""

    SAMPLER, ENTRIES, CHUNK = "rwr_sampler", "half_edges", CHUNK_COLUMNS
    _destroy, _info = staticmethod(lib.ugs_rwr_cache_destroy), staticmethod(lib.ugs_rwr_cache_info)

    def __init__(self, k, device, *, reserve=(0, 0)):
        self.k = int(k)
        self.failed = set()
        super().__init__(device, reserve, lib.ugs_rwr_cache_create, self.k)

    def add(self, index, edge_index, num_nodes):
        """One graph; same effect as add_many of one.  Returns False if the graph failed."""
        self.add_many([index], [(edge_index, num_nodes)])
        return int(index) not in self.failed

    def _add(self, run, ei, ptr, slots):
        status = np.zeros(len(run), np.int32)
        _check(lib.ugs_rwr_cache_add(self._handle(), ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(run), slots.ctypes.data,
                                     status.ctypes.data))
        for (i, _, _), st in zip(run, status.tolist()):
            if st:
                self.failed.add(i)
            else:
                self.failed.discard(i)

    def _job(self, graph_idx, ptr, edge_index, m_per_graph, mode, seed, seeds, p_restart, streams, check, device):
        rows = _row_streams(streams)
        self._check_batch(ptr, edge_index, check)
        dev = self._out_device(device, ptr, edge_index)
        gi, G = self._graphs_of(graph_idx, ptr)
        have = ptr.cpu().tolist()
        slots = self._slots_of(gi, have, edge_index)
        if seeds is None:
            for g, i in enumerate(gi):
                if i in self.failed:
                    raise RuntimeError(f"rwr_sampler: graph {g} has {have[g + 1] - have[g]} vertices; "
                                       "10 n k must fit the reference's int iteration limit")
        cache = self._handle()
        md, p = 0 if mode == "sample" else 1, C.c_double(float(p_restart))
        sd = _graphs.seed_array(seeds, G) if seeds is not None else None
        status = np.zeros(max(G, 1), np.int32)
        given = edge_index is not None and bool(check)                   # without the check the columns stay where they are

        def begin(batch, out):
            ei = batch[:3] if given else (None, 0, 0)
            return lib.ugs_rwr_cache_sample_begin(cache, slots.ctypes.data, *ei, *batch[3:6], md, C.c_uint64(int(seed) & _graphs.M64),
                                                  sd.ctypes.data if sd is not None else None, p, 1 if rows else 0, 1 if check else 0,
                                                  status.ctypes.data if sd is not None else None, *out)

        batch_ei = edge_index if given else torch.empty((2, 0), dtype=torch.int64)
        five = _graphs.run_job(begin, lib.ugs_rwr_sample_batch_finish, batch_ei.cpu() if given else batch_ei, ptr, m_per_graph, self.k,
                               dev, host_job_device=self.dev)
        return five, status[:G]

    def sample_batch(self, graph_idx, ptr, edge_index, m_per_graph, mode="sample", seed=42, p_restart=0.2, *, streams="graph",
                     check=True, device=None):
        """rwr_sampler.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed, p_restart, streams=streams) for a batch whose graph g
        is the graph added under graph_idx[g].  Pinned host tensors by default; with device= or a GPU ptr, tensors on the cache's
        device, on torch's current stream.  Before any device work: KeyError for an index never added, ValueError if graph_idx and
        ptr disagree in length, if the device is not the cache's, if streams is neither value and for edge_index=None without
        check=False, RuntimeError for a wrong vertex count or column count and for a failed graph.  With check, after the device
        work: RuntimeError "graph g of the batch differs from the graph added in its
        place", g the smallest such."""
        return self._job(graph_idx, ptr, edge_index, m_per_graph, mode, seed, None, p_restart, streams, check, device)[0]

    def sample_graphs(self, graph_idx, ptr, edge_index, m_per_graph, seeds, mode="sample", p_restart=0.2, *, streams="graph", check=True,
                      device=None):
        """rwr_sampler.sample_graphs for such a batch: the five tensors and failed [G] (on their device); a graph that failed when
        it was added gives m rows of -1 and failed[g] = True."""
        five, status = self._job(graph_idx, ptr, edge_index, m_per_graph, mode, 0, seeds, p_restart, streams, check, device)
        return five + (torch.from_numpy(status != 0).to(five[0].device),)

    def info(self):
        """graphs (indices held), vertices (entries of the row-start array: vertices plus one per add), half_edges, bytes of the
        device storage and generations (allocations so far); what replaced graphs held stays counted until close"""
        return super().info()
