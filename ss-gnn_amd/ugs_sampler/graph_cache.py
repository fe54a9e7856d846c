"""ugs_sampler.GraphCache: every graph of a dataset preprocessed once, at one k, and kept on the device; a training step over any
batch of added graphs then runs only the walks, the scan and the fill (C ABI and contract: include/ugs_mi355.h at
ugs_graph_cache_sample_begin; layout and generations: DESIGN.md section 15; what it shares with the other samplers' caches:
_dataset_cache.py)."""
import ctypes as C

import torch

from . import _graphs
from ._dataset_cache import DatasetCache
from ._lib import check, lib, vp

# add_many's call bound: columns and vertices per device call (a chunk is staged as one pooled plan: 32 bytes per column and per vertex)
CHUNK_COLUMNS = 1 << 20


class GraphCache(DatasetCache):
    """The preprocessing of a dataset's graphs, done once and kept on `device`, for one k.

        cache = GraphCache(k, "cuda:0")
        cache.add_many(range(len(dataset)), [(d.edge_index, d.num_nodes) for d in dataset])          # start-up
        five = cache.sample_batch(batch.graph_idx, batch.ptr, batch.edge_index, m, mode, seed)       # every step

    If the batch's columns are, graph by graph in batch order, the columns of the graphs added under graph_idx[g], in the order
    given and shifted by ptr[g] -- what collating those graphs produces -- cache.sample_batch equals ugs_sampler.sample_batch(
    edge_index, ptr, m, k, mode, seed) called right after ugs_sampler.clear_cache(), in all five tensors, bit for bit, and
    cache.sample_graphs equals ugs_sampler.sample_graphs likewise in all six.

    The deviation: the cache never reads or changes the preprocessing LRU (cache_stats() is the same before and after any add and
    any cached call), so it does not reproduce the reference's reuse of ANOTHER graph's preprocessing -- for a graph the LRU holds
    under another k (its key ignores k), and for two different graphs of more than 1000 columns that share a strided key.  Every
    graph gets the preprocessing of its own content at the cache's k.

    check=True (the default) uploads the batch's edge_index and compares every column with the stored one, exactly: any other
    batch raises RuntimeError, also one that merely permutes a graph's columns.  check=False reads nothing of the batch but ptr
    (edge_index may be None): the result is that of the added graphs, whatever the batch holds.

    Adding an index again gives it a new slot (the old bytes stay until close).  reserve=(vertices, columns) sizes the first
    allocation; the storage grows by doubling, and a call begun before an add finishes on the buffers it started with.  Adds are
    exclusive among themselves; any number of threads may sample meanwhile."""

    SAMPLER, ENTRIES, CHUNK = "ugs_sampler", "csr_entries", CHUNK_COLUMNS
    _destroy, _info = staticmethod(lib.ugs_graph_cache_destroy), staticmethod(lib.ugs_graph_cache_info)

    def __init__(self, k, device, *, reserve=(0, 0)):
        from . import _as_c_int
        self.k = _as_c_int(k, "k")
        super().__init__(device, reserve, lib.ugs_graph_cache_create, self.k)

    def _add(self, run, ei, ptr, slots):
        check(lib.ugs_graph_cache_add(self._handle(), ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(run), slots.ctypes.data))

    def _job(self, graph_idx, ptr, edge_index, m_per_graph, mode, seed, seeds, check_batch, device):
        from . import _BATCH_MODES, _as_c_int, _carve, _seed_ints
        self._check_batch(ptr, edge_index, check_batch)
        if mode not in _BATCH_MODES:
            raise RuntimeError("mode must be one of: 'sample', 'graph', 'global'")
        m = _as_c_int(m_per_graph, "m_per_graph")
        dev = self._out_device(device, ptr, edge_index)
        gi, G = self._graphs_of(graph_idx, ptr)
        pt = ptr.detach().cpu().contiguous()
        if seeds is None:
            sd, seed = None, _as_c_int(seed, "seed")
        else:
            sd, seed = _seed_ints(seeds, max(G, 0)), 0
        slots = self._slots_of(gi, pt.tolist(), edge_index)
        cache = self._handle()
        k = self.k
        if check_batch:
            keep, p, stride, e = _graphs._edge_index_view(edge_index.detach().cpu())
        else:
            keep, p, stride, e = None, None, 0, 0
        if dev is None:
            _graphs._select_device(self.dev)
        else:
            _graphs._select_device(self.dev, jobs=True)
        job, tot = vp(), C.c_int64()
        check(lib.ugs_graph_cache_sample_begin(cache, slots.ctypes.data, p, stride, e, pt.data_ptr(), G, m, _BATCH_MODES[mode], seed,
                                               sd.ctypes.data if sd is not None else None, 1 if check_batch else 0,
                                               C.byref(job), C.byref(tot)))
        try:
            opts, on_dev = _graphs._out_opts(dev)
            B = max(G, 0) * m
            nodes, edge_ptr, edge_index_t, edge_src, sample_ptr = _carve(opts, [(B, k), (B + 1,), (2, tot.value), (tot.value,), (max(G, 0) + 1,)])
        except BaseException:
            lib.ugs_job_cancel(job)
            raise
        check(lib.ugs_sample_batch_finish(job, nodes.data_ptr(), edge_index_t.data_ptr(), edge_ptr.data_ptr(), sample_ptr.data_ptr(),
                                          edge_src.data_ptr(), on_dev))
        return nodes, edge_index_t, edge_ptr, sample_ptr, edge_src

    def sample_batch(self, graph_idx, ptr, edge_index, m_per_graph, mode="sample", seed=42, *, check=True, device=None):
        """ugs_sampler.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed) on an empty LRU, for a batch whose graph g is the
        graph added under graph_idx[g].  Pinned host tensors by default; with device= or a GPU ptr, tensors on the cache's device,
        on torch's current stream.  Before any device work: KeyError for an index never added, ValueError if graph_idx and ptr
        disagree in length, if the device is not the cache's and for edge_index=None without check=False, RuntimeError naming
        the graph for a wrong vertex count and for a wrong column total.  With check, after the device work: RuntimeError
        "graph g of the batch differs from the graph added in its
        place", g the smallest such."""
        return self._job(graph_idx, ptr, edge_index, m_per_graph, mode, seed, None, check, device)

    def sample_graphs(self, graph_idx, ptr, edge_index, m_per_graph, seeds, mode="sample", *, check=True, device=None):
        """ugs_sampler.sample_graphs for such a batch: the five tensors and failed [G], all False (on their device).  `seeds` are
        C ints; one that does not fit raises TypeError naming its graph, before any work."""
        five = self._job(graph_idx, ptr, edge_index, m_per_graph, mode, 0, seeds, check, device)
        return five + (torch.zeros(max(ptr.numel() - 1, 0), dtype=torch.bool, device=five[0].device),)

    def last_launch(self):
        """(walk, fill): the names of the first-tier walk kernel and of the fill kernel of the calling thread's last cached call
        on this cache ("" where none ran).  A read-only aid, as Plan.last_launch / last_fill are."""
        w, f = C.create_string_buffer(128), C.create_string_buffer(128)
        check(lib.ugs_graph_cache_last_launch(self._handle(), w, 128, f, 128))
        return w.value.decode(), f.value.decode()

    def info(self):
        """graphs (indices held), vertices (root records: the vertices of every non-degenerate graph added), csr_entries, bytes of
        the device storage and generations (allocations so far); what replaced graphs held stays counted until close"""
        return super().info()
