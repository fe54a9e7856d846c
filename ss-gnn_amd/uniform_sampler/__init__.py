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

enumerate_graphs(edge_index, ptr, k, mode="sample", *, max_rows=1 << 22, device=None) -> the 5-tuple + failed[G]: every connected
k-subset of every graph as a row, in the order the samplers draw from (row sample_ptr[g] + d is the row a draw d gives), with its
edges; count_graphs(edge_index, ptr, k, *, limit=1 << 25) -> (counts[G], failed[G]): |S_g| alone, without storing a set.  Law at
ugs_uniform_enumerate_begin.

PopulationCache(k, device) keeps those populations on the device: every dataset graph is enumerated once (add / add_many), and
pop.sample_batch / pop.sample_graphs over any batch of added graphs equal the module's sample_batch / sample_graphs bit for bit
while running only column buckets, draws, rows and fill.  Law at ugs_uniform_population_create.

sample_distinct(edge_index, ptr, m_per_graph, k, seeds, mode="sample") -> the 5-tuple + failed[G] + valid[G], and
pop.sample_distinct: sampling WITHOUT replacement -- m distinct sets per graph (m <= 4096), uniform over all such selections, and the
whole population in enumerate_graphs' order when it has at most m sets; the rows past valid[g] = min(m, |S_g|) are rows of -1.  The
law (a counter-based partial Fisher-Yates shuffle, the project's own: the reference only draws with replacement) stands at
ugs_uniform_distinct_begin.
"""
import ctypes as C

import numpy as np
import torch

from ugs_sampler import _graphs
from ugs_sampler._lib import check, lib

__all__ = ["sample_batch", "sample_graphs", "sample_distinct", "enumerate_graphs", "count_graphs", "set_max_vertices", "max_vertices", "PopulationCache"]


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
    return _graphs.run_job(lambda batch, out: lib.ugs_uniform_sample_batch_begin(*batch, 0 if mode == "sample" else 1,
                                                                                 C.c_uint64(int(seed) & _graphs.M64), *out),
                           lib.ugs_uniform_sample_batch_finish, edge_index, ptr, m_per_graph, k)


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
    return _graphs.sample_graphs(lambda batch, md, sd, st, out: lib.ugs_uniform_sample_graphs_begin(*batch, md, sd, st, *out),
                                 lib.ugs_uniform_sample_batch_finish, edge_index, ptr, m_per_graph, k, seeds, mode, device)


DISTINCT_MAX_M = 4096                 # rows per graph of a distinct call (UGS_UNI_DISTINCT_MAX_M)


def _distinct_seeds(seeds, offsets):
    """The seeds of a distinct call: one per graph (as _graphs.seed_array takes them), or one integer s, graph g then getting
    s + offsets[g] mod 2^64."""
    if isinstance(seeds, (int, np.integer)) and not isinstance(seeds, bool):
        return np.array([(int(seeds) + int(o)) & _graphs.M64 for o in offsets], dtype=np.uint64)
    return _graphs.seed_array(seeds, len(offsets))


def sample_distinct(edge_index, ptr, m_per_graph, k, seeds, mode="sample"):
    """m distinct connected k-subsets per graph, uniform over all ordered selections (sampling without replacement); a graph with at
    most m sets gives all of them, in enumerate_graphs' order, and rows of -1 behind them.  Row j of graph g is row
    sample_ptr_e[g] + d of enumerate_graphs, d the j-th place of the shuffle the law at ugs_uniform_distinct_begin defines from
    (seeds[g], |S_g|); a smaller m gives a prefix.  m_per_graph <= 4096 (RuntimeError otherwise, before any device work).
    seeds: G integers (sequence or tensor, mod 2^64), or one integer s, which stands for s + g for graph g.
    Failures, devices, streams and pinned host outputs are those of sample_graphs.
    Returns (nodes, edge_index, edge_ptr, sample_ptr, edge_src, failed, valid): valid[g] = min(m, |S_g|) (0 for a failed graph), int64,
    the number of graph g's rows that are real -- always its first ones."""
    status, valid = [], []

    def begin(batch, out):
        G = max(batch[4], 0)
        sd = _distinct_seeds(seeds, range(G))
        status.append(np.zeros(max(G, 1), dtype=np.int32))
        valid.append(np.zeros(max(G, 1), dtype=np.int64))
        return lib.ugs_uniform_distinct_begin(*batch, 0 if mode == "sample" else 1, sd.ctypes.data, status[0].ctypes.data,
                                              valid[0].ctypes.data, *out)

    five = _graphs.run_job(begin, lib.ugs_uniform_sample_batch_finish, edge_index, ptr, m_per_graph, k)
    G, dev = ptr.numel() - 1, five[0].device
    return five + (torch.from_numpy(status[0][:G] != 0).to(dev), torch.from_numpy(valid[0][:G].copy()).to(dev))


def enumerate_graphs(edge_index, ptr, k, mode="sample", *, max_rows=1 << 22, device=None):
    """Every connected k-subset of every graph: graph g's rows [sample_ptr[g], sample_ptr[g+1]) are its sets in lexicographic order
    of the ascending vertex tuples (batch ids, never -1), edges and edge_src as sample_batch writes them; row sample_ptr[g] + d is
    the row sample_batch / sample_graphs emit when the graph's generator draws d.  A graph the samplers refuse for its size, or
    with more than max_rows sets of its own, gives no rows and failed[g] = True; healthy graphs with more than max_rows sets
    together raise RuntimeError (split the call).  max_rows: 1 ... 2**25 (ValueError otherwise).
    Returns (nodes [R, k], edge_index [2, E], edge_ptr [R+1], sample_ptr [G+1], edge_src [E], failed [G] host bool): pinned host
    tensors for host input, else on the input's device (or `device`), on torch's current stream."""
    max_rows = int(max_rows)
    if not 1 <= max_rows <= 1 << 25:
        raise ValueError(f"max_rows must be 1 ... 2**25, got {max_rows}")
    status = []

    def begin(batch, out):
        status.append(np.zeros(max(batch[4], 1), dtype=np.int32))
        return lib.ugs_uniform_enumerate_begin(*batch, 0 if mode == "sample" else 1, max_rows, status[0].ctypes.data, *out)

    five = _graphs.run_rows_job(begin, lib.ugs_uniform_enumerate_finish, edge_index, ptr, k, device)
    return five + (torch.from_numpy(status[0][:ptr.numel() - 1] != 0),)


def count_graphs(edge_index, ptr, k, *, limit=1 << 25):
    """|S_g| of every graph without storing a set: (counts [G] host int64, failed [G] host bool).  counts[g] is exact wherever it
    is at most `limit`; a graph with more sets, or one the samplers refuse for its size, has counts[g] = -1 and failed[g] = True.
    The work per graph is bounded by `limit` (1 ... 2**32, ValueError otherwise); no key array is allocated."""
    limit = int(limit)
    if not 1 <= limit <= 1 << 32:
        raise ValueError(f"limit must be 1 ... 2**32, got {limit}")
    _graphs.check_int64(edge_index, ptr)
    keep, p, stride, e = _graphs._edge_index_view(edge_index.cpu())
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    _graphs._select_device(edge_index.device if edge_index.device.type == "cuda" else None)
    counts = np.zeros(max(G, 1), dtype=np.int64)
    status = np.zeros(max(G, 1), dtype=np.int32)
    check(lib.ugs_uniform_count_graphs(p, stride, e, pt.data_ptr(), G, int(k), limit, counts.ctypes.data, status.ctypes.data))
    return torch.from_numpy(counts[:max(G, 0)]), torch.from_numpy(status[:max(G, 0)] != 0)


# add_many's call bound (vertices per enumeration call), as PresampleCache.add_many: the count pass keeps 768 B per vertex
CHUNK_VERTICES = 1 << 17
_JOINT_BUDGET = "split the call"       # healthy graphs that together exceed max_rows: the call is halved


class PopulationCache:
    """The connected k-subsets of a dataset's graphs, enumerated once and kept on `device`.

        pop = PopulationCache(k, "cuda:0")
        pop.add_many(range(len(dataset)), [(d.edge_index, d.num_nodes) for d in dataset])         # start-up
        five = pop.sample_batch(batch.graph_idx, batch.ptr, batch.edge_index, m, mode, seed)     # every step

    If graph g of the batch has the vertex count and the adjacency (as a set of undirected non-loop pairs) of the graph added under
    graph_idx[g], pop.sample_batch equals uniform_sampler.sample_batch(batch_edge_index, ptr, m, k, mode, seed) in all five tensors
    and pop.sample_graphs equals uniform_sampler.sample_graphs in all six: only the vertex sets come from the cache, edges and
    edge_src from the batch's own columns.  The one difference: a cached call does not refuse a batch with more than 2**25 sets.

    A graph the samplers refuse for its size (set_max_vertices at add time), or with more than max_rows (1 ... 2**25) sets of its own,
    is recorded in `failed`: sample_batch on a batch that names it raises RuntimeError, sample_graphs gives it m rows of -1 and
    failed[g] = True.  Adding an index again replaces it.  block_keys (1 ... 2**28): keys per storage block.  Adds are exclusive;
    any number of threads may sample at once."""

    def __init__(self, k, device, *, max_rows=1 << 22, block_keys=1 << 22):
        max_rows, block_keys = int(max_rows), int(block_keys)
        if not 1 <= max_rows <= 1 << 25:
            raise ValueError(f"max_rows must be 1 ... 2**25, got {max_rows}")
        if not 1 <= block_keys <= 1 << 28:
            raise ValueError(f"block_keys must be 1 ... 2**28, got {block_keys}")
        if int(k) < 0:
            raise ValueError(f"k must be >= 0, got {k}")
        self.k, self.max_rows, self.block_keys = int(k), max_rows, block_keys
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise ValueError("device must be a GPU device")
        self.failed = set()
        self._slot = {}                 # graph index -> (slot, vertices)
        self._pop = C.c_void_p()
        check(lib.ugs_uniform_population_create(self.k, block_keys, C.byref(self._pop)))

    def close(self):
        """Frees the storage (once the jobs still sampling from it have finished); the object cannot be used afterwards."""
        if getattr(self, "_pop", None):
            lib.ugs_uniform_population_destroy(self._pop)
            self._pop = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001  (interpreter shutdown: the library may be gone already)
            pass

    def _handle(self):
        if not self._pop:
            raise RuntimeError("the population is closed")
        return self._pop

    def add(self, index, edge_index, num_nodes):
        """One graph; same effect as add_many of one.  Returns False if the graph failed."""
        self.add_many([index], [(edge_index, num_nodes)])
        return int(index) not in self.failed

    def add_many(self, indices, graphs):
        """`graphs` holds (edge_index, num_nodes) per index, local vertex ids as a dataset stores them (columns with an endpoint
        outside [0, num_nodes) are dropped, as the one-graph call drops them).  A few batched device calls."""
        indices = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
        graphs = list(graphs)
        if len(indices) != len(graphs):
            raise ValueError("indices and graphs must have the same length")
        for ei, n in graphs:
            if not torch.is_tensor(ei):
                raise RuntimeError("edge_index must be a tensor")
            _graphs.check_int64(ei, torch.empty(0, dtype=torch.int64))
            if ei.dim() != 2 or ei.size(0) != 2:
                raise RuntimeError("edge_index must have shape [2, E]")
            if int(n) < 0:
                raise ValueError("num_nodes must be >= 0")
        self._handle()
        run, nv = [], 0
        for i, (ei, n) in zip(indices, graphs):
            if run and nv + int(n) > CHUNK_VERTICES:
                self._batched(run)
                run, nv = [], 0
            run.append((i, ei, int(n)))
            nv += int(n)
        self._batched(run)

    def _batched(self, run):
        if not run:
            return
        G = len(run)
        n = np.array([g[2] for g in run], np.int64)
        ptr = np.zeros(G + 1, np.int64)
        np.cumsum(n, out=ptr[1:])
        cols = [g[1].detach().cpu().numpy() for g in run]
        ncol = np.array([c.shape[1] for c in cols], np.int64)
        ei = np.concatenate(cols, axis=1)
        gid = np.repeat(np.arange(G, dtype=np.int64), ncol)
        bad = ((ei < 0) | (ei >= n[gid])).any(axis=0)
        ei = np.ascontiguousarray(np.where(bad, -1, ei + ptr[gid]))
        slots, status = np.zeros(G, np.int64), np.zeros(G, np.int32)
        _graphs._select_device(self.dev)
        try:
            check(lib.ugs_uniform_population_add(self._handle(), ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, G, self.max_rows,
                                                 slots.ctypes.data, status.ctypes.data))
        except RuntimeError as e:
            if G > 1 and _JOINT_BUDGET in str(e):
                self._batched(run[:G // 2])
                self._batched(run[G // 2:])
                return
            raise
        for (i, _, n_i), s, st in zip(run, slots.tolist(), status.tolist()):
            self._slot[i] = (s, n_i)
            if st:
                self.failed.add(i)
            else:
                self.failed.discard(i)

    def _slots(self, graph_idx, ptr=None):
        gi = graph_idx.cpu().flatten().tolist() if torch.is_tensor(graph_idx) else [int(i) for i in graph_idx]
        if ptr is not None and len(gi) != ptr.numel() - 1:
            raise ValueError(f"graph_idx names {len(gi)} graphs, ptr holds {ptr.numel() - 1}")
        out = np.zeros(max(len(gi), 1), np.int64)
        for g, i in enumerate(gi):
            if i not in self._slot:
                raise KeyError(i)
            out[g] = self._slot[i][0]
        if ptr is not None:
            have = ptr.cpu().tolist()
            for g, i in enumerate(gi):
                if have[g + 1] - have[g] != self._slot[i][1]:
                    raise RuntimeError(f"uniform_sampler population: graph {g} of the batch has {have[g + 1] - have[g]} vertices, "
                                       f"the graph added in its place has {self._slot[i][1]}")
        return gi, out

    def _job(self, graph_idx, ptr, edge_index, m_per_graph, mode, seed, seeds, check_graphs, device, distinct=False):
        _graphs.check_int64(edge_index, ptr)
        _graphs._edge_index_view(edge_index)
        gi, slots = self._slots(graph_idx, ptr)
        pop = self._handle()
        md = 0 if mode == "sample" else 1
        status = np.zeros(max(len(gi), 1), np.int32)
        if distinct:
            sd = _distinct_seeds(seeds, gi)
            valid = np.zeros(max(len(gi), 1), np.int64)
        else:
            sd = _graphs.seed_array(seeds, len(gi)) if seeds is not None else None

        def begin(batch, out):
            if distinct:
                return lib.ugs_uniform_population_distinct_begin(pop, slots.ctypes.data, *batch[:6], md, sd.ctypes.data, 1 if check_graphs else 0,
                                                                 status.ctypes.data, valid.ctypes.data, *out)
            return lib.ugs_uniform_population_sample_begin(pop, slots.ctypes.data, *batch[:6], md, C.c_uint64(int(seed) & _graphs.M64),
                                                           sd.ctypes.data if sd is not None else None, 1 if check_graphs else 0,
                                                           status.ctypes.data if sd is not None else None, *out)

        five = _graphs.run_job(begin, lib.ugs_uniform_population_sample_finish, edge_index, ptr, m_per_graph, self.k, device)
        if distinct:
            return five, status[:len(gi)], valid[:len(gi)]
        return five, status[:len(gi)]

    def sample_batch(self, graph_idx, ptr, batch_edge_index, m_per_graph, mode="sample", seed=42, *, check=True, device=None):
        """uniform_sampler.sample_batch(batch_edge_index, ptr, m_per_graph, k, mode, seed) for a batch whose graph g is the graph added
        under graph_idx[g]: pinned host tensors for host input, else on the input's device (or `device`), on torch's current stream.
        KeyError for an index never added, ValueError if graph_idx and ptr disagree in length, RuntimeError for a wrong vertex count
        (all before any device work), for a failed graph, and -- with check -- for a graph whose adjacency is not the added one's.
        check=False skips that comparison; the result for a wrong graph is then unspecified."""
        return self._job(graph_idx, ptr, batch_edge_index, m_per_graph, mode, seed, None, check, device)[0]

    def sample_graphs(self, graph_idx, ptr, batch_edge_index, m_per_graph, seeds, mode="sample", *, check=True, device=None):
        """uniform_sampler.sample_graphs for such a batch: the five tensors and failed [G] (on their device); a graph that failed when
        it was added gives m rows of -1 and failed[g] = True."""
        five, status = self._job(graph_idx, ptr, batch_edge_index, m_per_graph, mode, 0, seeds, check, device)
        return five + (torch.from_numpy(status != 0).to(five[0].device),)

    def sample_distinct(self, graph_idx, ptr, batch_edge_index, m_per_graph, seeds, mode="sample", *, check=True, device=None):
        """uniform_sampler.sample_distinct for such a batch, all seven tensors: m distinct sets per graph, or the graph's whole
        population (the full bag, served from the cache on every step) and rows of -1 behind it where it has at most m sets.
        seeds: one per graph of the batch, or one integer s, which here stands for s + graph_idx[g] -- a graph's seed follows its
        dataset index, not its place, so its bag does not depend on which batch it lands in (the uncached call, which knows no
        dataset index, takes s + g; it equals this call when given seeds = [s + i for i in graph_idx]).
        Errors, check, device and stream as sample_graphs; m_per_graph <= 4096."""
        five, status, valid = self._job(graph_idx, ptr, batch_edge_index, m_per_graph, mode, 0, seeds, check, device, distinct=True)
        dev = five[0].device
        return five + (torch.from_numpy(status != 0).to(dev), torch.from_numpy(valid.copy()).to(dev))

    def sizes(self, graph_idx):
        """|S_g| of the graphs added under graph_idx (host int64 [G]); -1 for a failed graph"""
        gi, slots = self._slots(graph_idx)
        out = np.zeros(max(len(gi), 1), np.int64)
        check(lib.ugs_uniform_population_sizes(self._handle(), slots.ctypes.data, len(gi), out.ctypes.data))
        return torch.from_numpy(out[:len(gi)])

    def info(self):
        """graphs (indices held), keys, bytes and blocks of the device storage (keys of replaced graphs stay until close)"""
        v = [C.c_int64() for _ in range(4)]
        check(lib.ugs_uniform_population_info(self._handle(), *[C.byref(x) for x in v]))
        return {"graphs": len(self._slot), "keys": v[1].value, "bytes": v[2].value, "blocks": v[3].value}
