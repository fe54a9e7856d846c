"""ugs_sampler.GraphCache: every graph of a dataset preprocessed once, at one k, and kept on the device; a training step over any
batch of added graphs then runs only the walks, the scan and the fill (C ABI and contract: include/ugs_mi355.h at
ugs_graph_cache_sample_begin; layout and generations: DESIGN.md section 15).  Modelled on rwr_sampler.GraphCache."""
import ctypes as C

import numpy as np
import torch

from . import _graphs
from ._lib import check, lib, vp

# add_many's call bound: columns and vertices per device call (a chunk is staged as one pooled plan: 32 bytes per column and per vertex)
CHUNK_COLUMNS = 1 << 20


class GraphCache:
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

    def __init__(self, k, device, *, reserve=(0, 0)):
        from . import _as_c_int
        self.k = _as_c_int(k, "k")
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise ValueError("device must be a GPU device")
        rv, rc = (int(x) for x in reserve)
        if rv < 0 or rc < 0:
            raise ValueError(f"reserve must be two counts >= 0, got {reserve}")
        self._slot = {}                 # graph index -> (slot, vertices, columns)
        self._cache = vp()
        check(lib.ugs_graph_cache_create(self.k, rv, rc, C.byref(self._cache)))

    def close(self):
        """Frees the storage (once the jobs still sampling from it have finished); the object cannot be used afterwards."""
        if getattr(self, "_cache", None):
            lib.ugs_graph_cache_destroy(self._cache)
            self._cache = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001  (interpreter shutdown: the library may be gone already)
            pass

    def _handle(self):
        if not self._cache:
            raise RuntimeError("the cache is closed")
        return self._cache

    def add(self, index, edge_index, num_nodes):
        """One graph; same effect as add_many of one."""
        self.add_many([index], [(edge_index, num_nodes)])

    def add_many(self, indices, graphs):
        """`graphs` holds (edge_index, num_nodes) per index, local vertex ids as a dataset stores them.  A column with an endpoint
        outside [0, num_nodes) raises ValueError naming the index, and nothing of the call is added: in a batch such a column
        could fall into a neighbouring graph, where the uncached call would keep it.  A few batched device calls."""
        indices = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
        graphs = list(graphs)
        if len(indices) != len(graphs):
            raise ValueError("indices and graphs must have the same length")
        cols = []
        for i, (ei, n) in zip(indices, graphs):
            if not torch.is_tensor(ei):
                raise RuntimeError("edge_index must be a tensor")
            _graphs.check_int64(ei, torch.empty(0, dtype=torch.int64))
            if ei.dim() != 2 or ei.size(0) != 2:
                raise RuntimeError("edge_index must have shape [2, E]")
            if int(n) < 0:
                raise ValueError("num_nodes must be >= 0")
            a = ei.detach().cpu().numpy()
            if a.size and (a.min() < 0 or a.max() >= int(n)):
                raise ValueError(f"graph {i} has a column with an endpoint outside [0, {int(n)})")
            cols.append(a)
        self._handle()
        run, ne, nv = [], 0, 0
        for i, a, (_, n) in zip(indices, cols, graphs):
            if run and (ne + a.shape[1] > CHUNK_COLUMNS or nv + int(n) > CHUNK_COLUMNS):
                self._batched(run)
                run, ne, nv = [], 0, 0
            run.append((i, a, int(n)))
            ne, nv = ne + a.shape[1], nv + int(n)
        self._batched(run)

    def _batched(self, run):
        if not run:
            return
        G = len(run)
        ptr = np.zeros(G + 1, np.int64)
        np.cumsum([g[2] for g in run], out=ptr[1:])
        ei = np.ascontiguousarray(np.concatenate([a + ptr[g] for g, (_, a, _) in enumerate(run)], axis=1))
        slots = np.zeros(G, np.int64)
        _graphs._select_device(self.dev)
        check(lib.ugs_graph_cache_add(self._handle(), ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, G, slots.ctypes.data))
        for (i, a, n), s in zip(run, slots.tolist()):
            self._slot[i] = (s, n, a.shape[1])

    def _out_device(self, device, ptr, edge_index):
        """Where the outputs go: `device`, else the device of a GPU ptr (or edge_index), else None (pinned host tensors)."""
        if device is None:
            for t in (ptr, edge_index):
                if t is not None and t.device.type == "cuda":
                    device = t.device
                    break
            else:
                return None
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("device= must be a GPU device (or None for pinned host tensors)")
        if dev.index is not None and self.dev.index is not None and dev.index != self.dev.index:
            raise ValueError(f"the cache lives on {self.dev}, not on {dev}")
        return self.dev

    def _job(self, graph_idx, ptr, edge_index, m_per_graph, mode, seed, seeds, check_batch, device):
        from . import _BATCH_MODES, _as_c_int, _carve, _seed_ints
        if not torch.is_tensor(ptr):
            raise TypeError("ptr must be a torch.Tensor")
        if edge_index is None:
            if check_batch:
                raise ValueError("edge_index=None needs check=False: the check compares the batch's columns")
        else:
            _graphs.check_int64(edge_index, ptr)
            _graphs._edge_index_view(edge_index)
        if ptr.dtype != torch.int64:
            raise RuntimeError("ptr must be int64")
        if mode not in _BATCH_MODES:
            raise RuntimeError("mode must be one of: 'sample', 'graph', 'global'")
        m = _as_c_int(m_per_graph, "m_per_graph")
        dev = self._out_device(device, ptr, edge_index)
        gi = graph_idx.cpu().flatten().tolist() if torch.is_tensor(graph_idx) else [int(i) for i in graph_idx]
        pt = ptr.detach().cpu().contiguous()
        G = pt.numel() - 1
        if len(gi) != G:
            raise ValueError(f"graph_idx names {len(gi)} graphs, ptr holds {G}")
        if seeds is None:
            sd, seed = None, _as_c_int(seed, "seed")
        else:
            sd, seed = _seed_ints(seeds, max(G, 0)), 0
        slots = np.zeros(max(G, 1), np.int64)
        have, total = pt.tolist(), 0
        for g, i in enumerate(gi):
            if i not in self._slot:
                raise KeyError(i)
            slots[g], n, ncol = self._slot[i]
            if have[g + 1] - have[g] != n:
                raise RuntimeError(f"ugs_sampler cache: graph {g} of the batch has {have[g + 1] - have[g]} vertices, "
                                   f"the graph added in its place has {n}")
            total += ncol
        if edge_index is not None and edge_index.size(1) != total:
            raise RuntimeError(f"ugs_sampler cache: the batch has {edge_index.size(1)} columns, the added graphs have {total}")
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
        "graph g of the batch differs from the graph added in its place", g the smallest such."""
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
        v = [C.c_int64() for _ in range(5)]
        check(lib.ugs_graph_cache_info(self._handle(), *[C.byref(x) for x in v]))
        return {"graphs": len(self._slot), "vertices": v[1].value, "csr_entries": v[2].value, "bytes": v[3].value, "generations": v[4].value}
