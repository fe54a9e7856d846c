"""What the three dataset caches share on the Python side -- rwr_sampler.GraphCache, ugs_sampler.GraphCache and
epsilon_uniform_sampler.GraphCache: the handle and its life, add / add_many up to the one library call, where the outputs go, the
resolution of a batch's graph indices to slots with its refusals, and info.  (The host side they share: csrc/ugs_cache_common.cpp;
DESIGN.md section 17.)"""
import ctypes as C

import numpy as np
import torch

from . import _graphs
from ._lib import check, vp


class DatasetCache:
    """Base of the GraphCache classes.  A subclass names its sampler (SAMPLER, in the refusals), the third key of info() (ENTRIES),
    its add_many call bound (CHUNK) and its library's destroy and info calls (_destroy, _info), and gives _add: the one library
    call of an add."""
    SAMPLER = ENTRIES = CHUNK = _destroy = _info = None

    def __init__(self, device, reserve, create, *args):
        """`create(*args, reserve_vertices, reserve_columns, handle)` is the library's create call."""
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise ValueError("device must be a GPU device")
        rv, rc = (int(x) for x in reserve)
        if rv < 0 or rc < 0:
            raise ValueError(f"reserve must be two counts >= 0, got {reserve}")
        self._slot = {}                 # graph index -> (slot, vertices, columns)
        self._cache = vp()
        check(create(*args, rv, rc, C.byref(self._cache)))

    def close(self):
        """Frees the storage (once the jobs still sampling from it have finished); the object cannot be used afterwards."""
        if getattr(self, "_cache", None):
            self._destroy(self._cache)
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
            if run and (ne + a.shape[1] > self.CHUNK or nv + int(n) > self.CHUNK):
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
        self._add(run, ei, ptr, slots)
        for (i, a, n), s in zip(run, slots.tolist()):
            self._slot[i] = (s, n, a.shape[1])

    def _add(self, run, ei, ptr, slots):
        """The library's add of the collated run (ei [2, E] contiguous, ptr [G + 1]); fills slots [G]."""
        raise NotImplementedError

    def _own_device(self, device):
        """`device`, if given, must be the cache's: the outputs are always there."""
        if device is not None:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise ValueError("device= must be a GPU device")
            if dev.index is not None and self.dev.index is not None and dev.index != self.dev.index:
                raise ValueError(f"the cache lives on {self.dev}, not on {dev}")
        return self.dev

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

    # The top of a cached call, in the order its refusals are tried: _check_batch, the sampler's own argument checks and its output
    # device, _graphs_of, (ugs: the seeds,) _slots_of.
    @staticmethod
    def _check_batch(ptr, edge_index, check_batch):
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

    @staticmethod
    def _graphs_of(graph_idx, ptr):
        """(the batch's graph indices as a list, G)"""
        gi = graph_idx.cpu().flatten().tolist() if torch.is_tensor(graph_idx) else [int(i) for i in graph_idx]
        G = ptr.numel() - 1
        if len(gi) != G:
            raise ValueError(f"graph_idx names {len(gi)} graphs, ptr holds {G}")
        return gi, G

    def _slots_of(self, gi, have, edge_index):
        """The slots of the batch's graphs (int64 [max(G, 1)]); `have` is ptr as a list.  KeyError for an index never added,
        RuntimeError for a graph of another size than the one added in its place and for another column total."""
        slots = np.zeros(max(len(gi), 1), np.int64)
        total = 0
        for g, i in enumerate(gi):
            if i not in self._slot:
                raise KeyError(i)
            slots[g], n, ncol = self._slot[i]
            if have[g + 1] - have[g] != n:
                raise RuntimeError(f"{self.SAMPLER} cache: graph {g} of the batch has {have[g + 1] - have[g]} vertices, "
                                   f"the graph added in its place has {n}")
            total += ncol
        if edge_index is not None and edge_index.size(1) != total:
            raise RuntimeError(f"{self.SAMPLER} cache: the batch has {edge_index.size(1)} columns, the added graphs have {total}")
        return slots

    def info(self):
        v = [C.c_int64() for _ in range(5)]
        check(self._info(self._handle(), *[C.byref(x) for x in v]))
        return {"graphs": len(self._slot), "vertices": v[1].value, self.ENTRIES: v[2].value, "bytes": v[3].value, "generations": v[4].value}
