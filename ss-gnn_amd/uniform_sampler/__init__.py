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

PopulationCache(k, device, wl_iterations=3) also hashes every member of every S_g once, when its graph is added, and the three
sample calls take wl=WLVocab: one more tensor, the rows' WL vocabulary ids, gathered from the cache -- what WLVocab.ids gives on
the call's mode-"sample" output, bit for bit, with no hashing per step.  Law at ugs_uniform_population_create_wl.
"""
import ctypes as C
import itertools
import threading

import numpy as np
import torch

from ugs_sampler import _graphs
from ugs_sampler import wl as _wl
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


_vocab_tokens = itertools.count(1)      # a WLVocab's name towards the populations' id arrays (ugs_uniform_population_sample_wl_begin)
_vocab_token_lock = threading.Lock()


def _vocab_token(table):
    with _vocab_token_lock:
        if getattr(table, "_population_token", None) is None:
            table._population_token = next(_vocab_tokens)
        return table._population_token


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
    any number of threads may sample at once.

    wl_iterations (0 ... 8, with 1 <= k <= 32; default None: a plain population) makes it a WL population: every add also hashes each
    member of each S_g (ugs_sampler.wl's digests with that many iterations) and keeps a class index beside its key.

        pop = PopulationCache(k, "cuda:0", wl_iterations=3)
        pop.add_many(indices, graphs)                              # degree labels (use_node_features_in_wl=False)
        pop.add_many(indices, graphs, x=[d.x for d in dataset])    # node-feature labels (md5 of the rows), or node_labels=[...]
        table = wl.WLVocab(vocab, "cuda:0")
        *five, wl_ids = pop.sample_batch(graph_idx, ptr, edge_index, m, mode, seed, wl=table)

    wl_ids (int64 [G m], on the outputs' device) equals table.ids(nodes, edge_index_s, edge_ptr, iterations=wl_iterations[,
    node_labels=L]) over the three tensors the same call gives in mode "sample", L holding for batch vertex ptr[g] + v the label
    given for vertex v of graph graph_idx[g] -- whatever the call's own mode, with len(vocab) for rows of -1 and for members whose
    label is outside [0, 2**32).  The labels are fixed when the graph is added: the batch's x is not read per step, and no row is
    hashed per step.  Loop columns change a digest, so a WL population records each graph's loop vertices, and with wl= and check a
    batch whose loop set differs raises like one whose adjacency differs (check=False: the ids of the added graph).  All adds of
    one population use one labelling.  Calls without wl= behave exactly as on a plain population."""

    def __init__(self, k, device, *, max_rows=1 << 22, block_keys=1 << 22, wl_iterations=None):
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
        if wl_iterations is not None:
            if isinstance(wl_iterations, bool) or not isinstance(wl_iterations, (int, np.integer)) or not 0 <= int(wl_iterations) <= 8:
                raise ValueError(f"wl_iterations must be 0 ... 8 (or None), got {wl_iterations!r}")
            if not 1 <= self.k <= 32:
                raise ValueError(f"a WL population needs 1 <= k <= 32 (the WL kernels' range), got k = {self.k}")
            wl_iterations = int(wl_iterations)
        self.wl_iterations = wl_iterations
        self._wl_labeled = None         # the labelling of the adds so far: None (no add yet), False (degrees), True (labels)
        self.failed = set()
        self._slot = {}                 # graph index -> (slot, vertices)
        self._pop = C.c_void_p()
        if wl_iterations is None:
            check(lib.ugs_uniform_population_create(self.k, block_keys, C.byref(self._pop)))
        else:
            check(lib.ugs_uniform_population_create_wl(self.k, block_keys, wl_iterations, C.byref(self._pop)))

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

    def add(self, index, edge_index, num_nodes, *, x=None, node_labels=None):
        """One graph; same effect as add_many of one.  Returns False if the graph failed."""
        self.add_many([index], [(edge_index, num_nodes)], x=None if x is None else [x], node_labels=None if node_labels is None else [node_labels])
        return int(index) not in self.failed

    def _labels_arg(self, graphs, x, node_labels):
        """The per-graph label tensors of an add (None: degree labels), checked before any device work."""
        if x is not None and node_labels is not None:
            raise ValueError("x= and node_labels= are mutually exclusive")
        given = x if x is not None else node_labels
        name = "x" if x is not None else "node_labels"
        if given is not None and self.wl_iterations is None:
            raise RuntimeError(f"{name}= needs a population created with wl_iterations")
        if given is not None:
            given = list(given)
            if len(given) != len(graphs):
                raise ValueError(f"{name} must hold one tensor per graph ({len(graphs)}), got {len(given)}")
            for t, (_, n) in zip(given, graphs):
                if not torch.is_tensor(t):
                    raise TypeError(f"{name} must hold tensors")
                if x is not None:
                    _wl._check_x(t)
                    if t.dtype != given[0].dtype or t.shape[1:] != given[0].shape[1:]:
                        raise ValueError("the feature rows of one add must share dtype and shape")
                elif t.dtype != torch.int64 or t.dim() != 1:
                    raise ValueError("node_labels must hold int64 tensors of shape [num_nodes]")
                if t.size(0) != int(n):
                    raise ValueError(f"{name}: a tensor of {t.size(0)} vertices for a graph of {int(n)}")
        if self.wl_iterations is not None and graphs and self._wl_labeled not in (None, given is not None):
            raise RuntimeError("every add of a WL population uses the same labelling: all degree-labelled, or all with x= / node_labels=")
        return given

    def add_many(self, indices, graphs, *, x=None, node_labels=None):
        """`graphs` holds (edge_index, num_nodes) per index, local vertex ids as a dataset stores them (columns with an endpoint
        outside [0, num_nodes) are dropped, as the one-graph call drops them).  A few batched device calls.
        A WL population: x= (one feature tensor [num_nodes, ...] per graph; the label of a vertex is the md5 of its row, as
        wl.feature_labels gives it) or node_labels= (one int64 tensor [num_nodes] per graph) set the start labels of the digests,
        neither means degree labels; one labelling per population (RuntimeError otherwise)."""
        indices = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
        graphs = list(graphs)
        if len(indices) != len(graphs):
            raise ValueError("indices and graphs must have the same length")
        labels = self._labels_arg(graphs, x, node_labels)
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
        for j, (i, (ei, n)) in enumerate(zip(indices, graphs)):
            if run and nv + int(n) > CHUNK_VERTICES:
                self._batched(run, x is not None)
                run, nv = [], 0
            run.append((i, ei, int(n), None if labels is None else labels[j]))
            nv += int(n)
        self._batched(run, x is not None)

    def _batched(self, run, features=False):
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
        lab = None
        if run[0][3] is not None:
            # the start labels of the call's vertices, on the device: given, or the md5 of the feature rows (one launch per call)
            _graphs._select_device(self.dev, jobs=True)
            lab = torch.cat([g[3].reshape(g[3].size(0), -1) if features else g[3] for g in run]).to(self.dev)
            lab = _wl._labels_on_device(lab) if features else lab.contiguous()
            torch.cuda.current_stream(self.dev).synchronize()     # the add runs on the library's own stream
        _graphs._select_device(self.dev)
        try:
            if self.wl_iterations is None:
                check(lib.ugs_uniform_population_add(self._handle(), ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, G, self.max_rows,
                                                     slots.ctypes.data, status.ctypes.data))
            else:
                check(lib.ugs_uniform_population_add_wl(self._handle(), ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, G, self.max_rows,
                                                        lab.data_ptr() if lab is not None and lab.numel() else None,
                                                        lab.numel() if lab is not None else 0, slots.ctypes.data, status.ctypes.data))
        except RuntimeError as e:
            if G > 1 and _JOINT_BUDGET in str(e):
                self._batched(run[:G // 2], features)
                self._batched(run[G // 2:], features)
                return
            raise
        if self.wl_iterations is not None:
            self._wl_labeled = lab is not None
        for (i, _, n_i, _), s, st in zip(run, slots.tolist(), status.tolist()):
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

    def _wl_arg(self, table):
        """The checks of wl=, before anything else of the call."""
        if table is None:
            return
        if self.wl_iterations is None:
            raise RuntimeError("wl= needs a population created with wl_iterations")
        if not isinstance(table, _wl.WLVocab):
            raise TypeError("wl= takes a ugs_sampler.wl.WLVocab")
        if table.device.type != self.dev.type or None not in (table.device.index, self.dev.index) and table.device.index != self.dev.index:
            raise ValueError(f"the population lives on {self.dev}, the vocabulary on {table.device}")

    def _job(self, graph_idx, ptr, edge_index, m_per_graph, mode, seed, seeds, check_graphs, device, distinct=False, table=None):
        self._wl_arg(table)
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

        ids = []

        def begin(batch, out):
            if table is not None:
                # the ids are written by begin, on the job's stream: torch's current one for a device batch, else the library's own
                keys, key_ids = table._table()
                if table.device != torch.device(self.dev.type, self.dev.index if self.dev.index is not None else torch.cuda.current_device()):
                    raise ValueError(f"the population lives on {self.dev}, the vocabulary on {table.device}")
                ids.append(torch.empty((max(batch[4], 0) * int(m_per_graph),), dtype=torch.int64, device=table.device))
                if not (edge_index.is_cuda or device is not None):
                    torch.cuda.current_stream(table.device).synchronize()
                voc = (keys.data_ptr() if key_ids.numel() else None, key_ids.data_ptr() if key_ids.numel() else None, key_ids.numel(),
                       len(table), C.c_uint64(_vocab_token(table)), ids[0].data_ptr() if ids[0].numel() else None)
                if distinct:
                    return lib.ugs_uniform_population_distinct_wl_begin(pop, slots.ctypes.data, *batch[:6], md, sd.ctypes.data,
                                                                        1 if check_graphs else 0, status.ctypes.data, valid.ctypes.data, *voc, *out)
                return lib.ugs_uniform_population_sample_wl_begin(pop, slots.ctypes.data, *batch[:6], md, C.c_uint64(int(seed) & _graphs.M64),
                                                                  sd.ctypes.data if sd is not None else None, 1 if check_graphs else 0,
                                                                  status.ctypes.data if sd is not None else None, *voc, *out)
            if distinct:
                return lib.ugs_uniform_population_distinct_begin(pop, slots.ctypes.data, *batch[:6], md, sd.ctypes.data, 1 if check_graphs else 0,
                                                                 status.ctypes.data, valid.ctypes.data, *out)
            return lib.ugs_uniform_population_sample_begin(pop, slots.ctypes.data, *batch[:6], md, C.c_uint64(int(seed) & _graphs.M64),
                                                           sd.ctypes.data if sd is not None else None, 1 if check_graphs else 0,
                                                           status.ctypes.data if sd is not None else None, *out)

        five = _graphs.run_job(begin, lib.ugs_uniform_population_sample_finish, edge_index, ptr, m_per_graph, self.k, device)
        if table is not None:
            five = five + (ids[0].to(five[0].device),)
        if distinct:
            return five, status[:len(gi)], valid[:len(gi)]
        return five, status[:len(gi)]

    @staticmethod
    def _with_ids(five, *more):
        """(five tensors, the call's own extras, wl_ids last) from _job's five-or-six tuple"""
        return five[:5] + more + five[5:]

    def sample_batch(self, graph_idx, ptr, batch_edge_index, m_per_graph, mode="sample", seed=42, *, check=True, device=None, wl=None):
        """uniform_sampler.sample_batch(batch_edge_index, ptr, m_per_graph, k, mode, seed) for a batch whose graph g is the graph added
        under graph_idx[g]: pinned host tensors for host input, else on the input's device (or `device`), on torch's current stream.
        KeyError for an index never added, ValueError if graph_idx and ptr disagree in length, RuntimeError for a wrong vertex count
        (all before any device work), for a failed graph, and -- with check -- for a graph whose adjacency is not the added one's.
        check=False skips that comparison; the result for a wrong graph is then unspecified.
        wl=WLVocab (a WL population): a sixth tensor, the rows' vocabulary ids (class docstring); the three calls put it last."""
        return self._job(graph_idx, ptr, batch_edge_index, m_per_graph, mode, seed, None, check, device, table=wl)[0]

    def sample_graphs(self, graph_idx, ptr, batch_edge_index, m_per_graph, seeds, mode="sample", *, check=True, device=None, wl=None):
        """uniform_sampler.sample_graphs for such a batch: the five tensors and failed [G] (on their device); a graph that failed when
        it was added gives m rows of -1 and failed[g] = True."""
        five, status = self._job(graph_idx, ptr, batch_edge_index, m_per_graph, mode, 0, seeds, check, device, table=wl)
        return self._with_ids(five, torch.from_numpy(status != 0).to(five[0].device))

    def sample_distinct(self, graph_idx, ptr, batch_edge_index, m_per_graph, seeds, mode="sample", *, check=True, device=None, wl=None):
        """uniform_sampler.sample_distinct for such a batch, all seven tensors: m distinct sets per graph, or the graph's whole
        population (the full bag, served from the cache on every step) and rows of -1 behind it where it has at most m sets.
        seeds: one per graph of the batch, or one integer s, which here stands for s + graph_idx[g] -- a graph's seed follows its
        dataset index, not its place, so its bag does not depend on which batch it lands in (the uncached call, which knows no
        dataset index, takes s + g; it equals this call when given seeds = [s + i for i in graph_idx]).
        Errors, check, device and stream as sample_graphs; m_per_graph <= 4096."""
        five, status, valid = self._job(graph_idx, ptr, batch_edge_index, m_per_graph, mode, 0, seeds, check, device, distinct=True, table=wl)
        dev = five[0].device
        return self._with_ids(five, torch.from_numpy(status != 0).to(dev), torch.from_numpy(valid.copy()).to(dev))

    def sizes(self, graph_idx):
        """|S_g| of the graphs added under graph_idx (host int64 [G]); -1 for a failed graph"""
        gi, slots = self._slots(graph_idx)
        out = np.zeros(max(len(gi), 1), np.int64)
        check(lib.ugs_uniform_population_sizes(self._handle(), slots.ctypes.data, len(gi), out.ctypes.data))
        return torch.from_numpy(out[:len(gi)])

    def wl_digests(self):
        """The distinct WL digests the population holds, ascending as 128-bit numbers, in wl.wl_hash's format: (digest int64 [C, 2],
        status int32 [C], all 0), host tensors -- what wl.extend_vocab and wl.hexdigests take."""
        if self.wl_iterations is None:
            raise RuntimeError("wl_digests needs a population created with wl_iterations")
        n = C.c_int64()
        check(lib.ugs_uniform_population_wl_digests(self._handle(), 0, None, C.byref(n)))
        while True:
            out = np.zeros((max(n.value, 1), 2), np.uint64)
            cap = n.value
            check(lib.ugs_uniform_population_wl_digests(self._handle(), cap, out.ctypes.data, C.byref(n)))
            if n.value <= cap:                     # (an add between the two calls: ask again)
                break
        return torch.from_numpy(out[:n.value].view(np.int64).copy()), torch.zeros(n.value, dtype=torch.int32)

    def info(self):
        """graphs (indices held), keys, bytes and blocks of the device storage (keys of replaced graphs stay until close);
        a WL population also reports wl_classes (distinct digests) and wl_rows_hashed (members hashed: by adds only), and its bytes
        include the class indices and the class table"""
        v = [C.c_int64() for _ in range(6)]
        check(lib.ugs_uniform_population_info(self._handle(), *[C.byref(x) for x in v[:4]]))
        out = {"graphs": len(self._slot), "keys": v[1].value, "bytes": v[2].value, "blocks": v[3].value}
        if self.wl_iterations is not None:
            check(lib.ugs_uniform_population_wl_stats(self._handle(), C.byref(v[4]), C.byref(v[5])))
            out.update(wl_classes=v[4].value, wl_rows_hashed=v[5].value)
        return out
