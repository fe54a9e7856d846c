"""Device-resident presample cache: the reference trainer's `--presample` path without its Python loops.

The reference samples every dataset graph once at start-up (gps/experiment.py:379-440: `sampler(edge_index, [0, n], m, k,
mode="sample", seed=cfg.seed + running_index)`, results cloned into a dict) and, for every mini-batch, stitches the cached
results of the batch's graphs together on the host (gps/experiment.py:936-993): nodes re-based by ptr[g], edge ids left local,
edge_src re-based by the number of batch columns that belong to earlier graphs, edge_ptr / sample_ptr accumulated -- Python loops
with `.item()` per graph and per sample.  Here the cache lives in HBM as flat tensors and a batch is assembled by a handful of
device gathers; the sizes that decide the output shapes are known on the host from build time, so nothing synchronises.

    cache = PresampleCache(m, k, device="cuda:0", sampler="rwr")   # "ugs" (default), "uniform", "rwr" or "epsilon_uniform"
                                                                   # (with epsilon=...): the config's sampler
    cache.add_many(range(len(dataset)), [(d.edge_index, d.num_nodes) for d in dataset],
                   [cfg.seed + i for i in range(len(dataset))])    # start-up, like _setup_presampling
    cache.finalize()
    nodes, edge_index, edge_ptr, sample_ptr, edge_src = cache.load(batch.graph_idx, batch.ptr, batch.edge_index)

`add(i, edge_index, num_nodes, seed)` presamples one graph with the sampler's drop-in call, exactly like one iteration of the
reference's loop; `add_many` leaves the cache exactly as the loop of `add` over its arguments would, but samples the graphs in a
few batched calls (the sampler's sample_graphs: one seed per graph).  `failed` is the set of indices whose presampling failed.

`load` returns exactly what the reference's `_load_from_presample_cache` stores on the batch -- including its treatment of
graphs whose presampling failed (m rows of -1 to which ptr[g] is ADDED like to every other row, no edges).
"""
import numpy as np
import torch

from . import _I32_MAX, _I32_MIN, sample_batch

SAMPLERS = ("ugs", "uniform", "rwr", "epsilon_uniform")
# add_many's call bounds.  Vertices: the uniform count pass keeps 12 B per (root, first extension) item and 64 items per vertex,
# 768 B per vertex, so 2^17 vertices hold about 100 MB of item arrays (a whole QM9 split would need gigabytes).  Rows: the
# outputs and per-row scratch of 2^21 rows are about 130 MB at k = 6.  A graph larger than a bound is a call of its own.
CHUNK_VERTICES = 1 << 17
CHUNK_ROWS = 1 << 21
_JOINT_BUDGET = "split the call"       # uniform_sampler: healthy graphs that together exceed the device budget


def _drop_in(sampler):
    if sampler == "ugs":
        import ugs_sampler
        return ugs_sampler
    if sampler == "uniform":
        import uniform_sampler
        return uniform_sampler
    if sampler == "epsilon_uniform":
        import epsilon_uniform_sampler
        return epsilon_uniform_sampler
    import rwr_sampler
    return rwr_sampler


class PresampleCache:
    def __init__(self, m, k, device, sampler="ugs", p_restart=0.2, chunk_vertices=CHUNK_VERTICES, chunk_rows=CHUNK_ROWS,
                 epsilon=0.1):
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
        self.m, self.k = int(m), int(k)
        self.dev = torch.device(device)
        self.sampler, self.p_restart, self.epsilon = sampler, float(p_restart), float(epsilon)
        self.chunk_vertices, self.chunk_rows = max(int(chunk_vertices), 1), max(int(chunk_rows), 1)
        self.failed = set()             # indices whose presampling failed
        self._slot = {}                 # graph index -> slot (-1: presampling failed)
        # blocks of consecutive slots: (nodes [S*m,k], edge_index [2,E], edge_ptr [S,m+1], edge_src [E], edges per slot [S]) on the device
        self._parts = []
        self._nslots = 0
        self._final = None

    def _call(self, edge_index, num_nodes, seed):
        ptr = torch.tensor([0, int(num_nodes)], dtype=torch.long)
        if self.sampler == "ugs":
            return sample_batch(edge_index.cpu(), ptr, self.m, self.k, mode="sample", seed=int(seed), device=self.dev)
        mod = _drop_in(self.sampler)
        ei = edge_index.to(self.dev)    # device in, device out
        if self.sampler == "rwr":
            return mod.sample_batch(ei, ptr, self.m, self.k, mode="sample", seed=int(seed), p_restart=self.p_restart)
        if self.sampler == "epsilon_uniform":
            return mod.sample_batch(ei, ptr, self.m, self.k, mode="sample", seed=int(seed), epsilon=self.epsilon)
        return mod.sample_batch(ei, ptr, self.m, self.k, mode="sample", seed=int(seed))

    def _fail(self, index):
        self._slot[index] = -1
        self.failed.add(index)

    def _append(self, indices, ok, nodes, eidx, eptr, esrc, n_edges):
        base = self._nslots
        j = 0
        for i, good in zip(indices, ok):
            if good:
                self._slot[i] = base + j
                self.failed.discard(i)
                j += 1
            else:
                self._fail(i)
        self._parts.append((nodes, eidx, eptr, esrc, n_edges))
        self._nslots += j
        self._final = None

    def add(self, index, edge_index, num_nodes, seed):
        """Presample one graph (reference: experiment.py:403-430); a sampler error marks the graph as failed, like the reference."""
        try:
            nodes, eidx, eptr, _, esrc = self._call(edge_index, num_nodes, seed)
        except Exception:   # noqa: BLE001  (the reference swallows every exception here)
            self._fail(int(index))
            return False
        self._append([int(index)], [True], nodes, eidx, eptr.unsqueeze(0), esrc, [int(eidx.size(1))])
        return True

    def add_many(self, indices, graphs, seeds):
        """Presample many graphs: `graphs` holds (edge_index, num_nodes) per index, `seeds` one seed per index.  Leaves the cache
        exactly as `for i, (ei, n), s in zip(indices, graphs, seeds): add(i, ei, n, s)` would, failures included."""
        indices = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
        graphs = list(graphs)
        seeds = [int(s) for s in (seeds.tolist() if torch.is_tensor(seeds) else seeds)]
        if not (len(indices) == len(graphs) == len(seeds)):
            raise ValueError("indices, graphs and seeds must have the same length")
        run, nv, rows = [], 0, 0        # graphs of the current call, in order
        for t, (ei, n) in enumerate(graphs):
            regular = torch.is_tensor(ei) and ei.dtype == torch.int64 and ei.dim() == 2 and ei.size(0) == 2 and int(n) >= 0
            if self.sampler == "ugs":   # its seeds are C ints: the one-graph call refuses any other
                regular = regular and _I32_MIN <= seeds[t] <= _I32_MAX
            if not regular:             # whatever add makes of it, in its place in the order
                self._batched(run)
                run, nv, rows = [], 0, 0
                self.add(indices[t], ei, n, seeds[t])
                continue
            n = int(n)
            if run and (nv + n > self.chunk_vertices or rows + self.m > self.chunk_rows):
                self._batched(run)
                run, nv, rows = [], 0, 0
            run.append((indices[t], ei, n, seeds[t]))
            nv += n
            rows += self.m
        self._batched(run)

    def _batched(self, run):
        """One sample_graphs call over `run` ([(index, edge_index, n, seed)]): halves a uniform call refused for the joint budget,
        and falls back to `add` per graph on any other call error."""
        if not run:
            return
        G, m, k = len(run), self.m, self.k
        n = np.array([g[2] for g in run], np.int64)
        ptr = np.zeros(G + 1, np.int64)
        np.cumsum(n, out=ptr[1:])
        cols = [g[1].detach().cpu().numpy() for g in run]
        ncol = np.array([c.shape[1] for c in cols], np.int64)
        col0 = np.zeros(G + 1, np.int64)
        np.cumsum(ncol, out=col0[1:])
        ei = np.concatenate(cols, axis=1) if G else np.zeros((2, 0), np.int64)
        # columns with an endpoint outside [0, n) become (-1, -1): dropped as in the one-graph call, never in a neighbour's range,
        # and every other column keeps its position
        gid = np.repeat(np.arange(G, dtype=np.int64), ncol)
        bad = ((ei < 0) | (ei >= n[gid])).any(axis=0)
        ei = np.where(bad, -1, ei + ptr[gid])
        mod = _drop_in(self.sampler)
        extra = {"rwr": dict(p_restart=self.p_restart), "epsilon_uniform": dict(epsilon=self.epsilon)}.get(self.sampler, {})
        try:
            (nodes, eidx, eptr, _, esrc), failed = mod._sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), m, k,
                                                                      [g[3] for g in run], "sample",
                                                                      device=self.dev, **extra)
        except (RuntimeError, TypeError) as e:
            if self.sampler == "uniform" and G > 1 and _JOINT_BUDGET in str(e):
                self._batched(run[:G // 2])
                self._batched(run[G // 2:])
            else:
                for i, e_i, n_i, s in run:
                    self.add(i, e_i, n_i, s)
            return
        # back to the one-graph form: local node ids, edge_src local to the graph's own columns (rwr's -1 stays; the other samplers'
        # edge_src are column positions >= 0, so the guard leaves them alone), edge_ptr per graph
        dev = nodes.device
        i64 = dict(dtype=torch.int64, device=dev)
        ptr_d = torch.from_numpy(ptr).to(dev)
        nodes = torch.where(nodes >= 0, nodes - ptr_d[:G].repeat_interleave(m).unsqueeze(1), nodes)
        bound = (torch.arange(G + 1, **i64) * m).clamp(max=eptr.numel() - 1)
        per_graph = eptr.index_select(0, bound).cpu()                       # edge entries before each graph: the one read-back
        cnt = (per_graph[1:] - per_graph[:-1]).to(dev)
        total = int(per_graph[-1])
        seg = torch.repeat_interleave(torch.arange(G, **i64), cnt, output_size=total)
        esrc = torch.where(esrc >= 0, esrc - torch.from_numpy(col0[:G]).to(dev).index_select(0, seg), esrc)
        eptr = eptr.index_select(0, ((torch.arange(G, **i64) * m).unsqueeze(1) + torch.arange(m + 1, **i64)).reshape(-1)).reshape(G, m + 1)
        eptr = eptr - eptr[:, :1]
        ok = ~failed
        if not bool(ok.all()):                                            # failed graphs have rows of -1 and no edges
            keep = torch.nonzero(ok).flatten().to(dev)
            nodes = nodes.reshape(G, m, k).index_select(0, keep).reshape(keep.numel() * m, k)
            eptr = eptr.index_select(0, keep)
        n_edges = (per_graph[1:] - per_graph[:-1])[ok].tolist()
        self._append([g[0] for g in run], ok.tolist(), nodes, eidx, eptr, esrc, n_edges)

    def finalize(self):
        m, k, dev = self.m, self.k, self.dev
        i64 = dict(dtype=torch.int64, device=dev)
        # slot S is the placeholder of failed graphs: m rows of -1, no edges
        self.nodes = torch.cat([p[0] for p in self._parts] + [torch.full((m, k), -1, **i64)], dim=0)                     # [(S+1)*m, k]
        self.eptr_local = torch.cat([p[2] for p in self._parts] + [torch.zeros(1, m + 1, **i64)], dim=0)                # [S+1, m+1]
        self.n_edges_host = [c for p in self._parts for c in p[4]] + [0]                                                 # host, no sync later
        self.eidx = torch.cat([p[1] for p in self._parts] + [torch.empty((2, 0), **i64)], dim=1)                         # [2, Etot]
        self.esrc = torch.cat([p[3] for p in self._parts] + [torch.empty((0,), **i64)], dim=0)
        base = [0]
        for n in self.n_edges_host[:-1]:
            base.append(base[-1] + n)
        self.edge_base_host = base                                                                                       # first cached edge of every slot
        self.edge_base = torch.tensor(base, **i64)
        self.n_edges = torch.tensor(self.n_edges_host, **i64)
        self._parts = None
        self._final = True

    def load(self, graph_indices, ptr, batch_edge_index):
        """(nodes_sampled [G*m,k], edge_index_sampled [2,Es], edge_ptr [G*m+1], sample_ptr [G+1], edge_src_global [Es]) of a batch made
        of the cached graphs `graph_indices` (a sequence or tensor of dataset indices, in batch order), as device tensors."""
        if self._final is None:
            self.finalize()
        m, k, dev = self.m, self.k, self.dev
        gi = graph_indices.cpu().flatten().tolist() if torch.is_tensor(graph_indices) else list(graph_indices)
        G = len(gi)
        fail = len(self.n_edges_host) - 1
        slots_h = [self._slot.get(int(i), -1) for i in gi]
        slots_h = [fail if s < 0 else s for s in slots_h]
        total = sum(self.n_edges_host[s] for s in slots_h)                        # known on the host: output shapes need no round trip
        i64 = dict(dtype=torch.int64, device=dev)
        slots = torch.tensor(slots_h, **i64)
        ptr_d = ptr.to(dev, dtype=torch.int64)
        # nodes: the slot's m rows + ptr[g] (the reference adds the offset to every entry, -1 padding included: experiment.py:966)
        rows = (slots * m).repeat_interleave(m) + torch.arange(m, **i64).repeat(G)
        nodes = self.nodes.index_select(0, rows) + ptr_d[:G].repeat_interleave(m).unsqueeze(1)
        # edge_ptr: every graph's local offsets shifted by the edge entries of the graphs before it
        cnt = self.n_edges.index_select(0, slots)
        shift = torch.cumsum(cnt, 0) - cnt
        edge_ptr = torch.empty(G * m + 1, **i64)
        edge_ptr[0] = 0
        edge_ptr[1:] = (self.eptr_local.index_select(0, slots)[:, 1:] + shift.unsqueeze(1)).reshape(-1)
        sample_ptr = torch.arange(G + 1, **i64) * m
        # edges: segment gather of the cached entries; ids stay local (the model adds the sample offsets itself, experiment.py:968-971)
        seg = torch.repeat_interleave(torch.arange(G, **i64), cnt, output_size=total)
        src_pos = self.edge_base.index_select(0, slots).index_select(0, seg) + (torch.arange(total, **i64) - shift.index_select(0, seg))
        edge_index = self.eidx.index_select(1, src_pos)
        # edge_src: + number of batch columns whose source vertex belongs to an earlier graph (experiment.py:937-942, 973-974)
        src = batch_edge_index[0].to(dev)
        owner = torch.bucketize(src, ptr_d[1:], right=True)
        inside = ((owner < G) & (src >= ptr_d[0])).to(torch.float64)
        per_graph = torch.bincount(owner.clamp(max=max(G - 1, 0)), weights=inside, minlength=max(G, 1)).to(torch.int64)
        orig_off = torch.cumsum(per_graph, 0) - per_graph
        edge_src = self.esrc.index_select(0, src_pos) + orig_off.index_select(0, seg)
        return nodes, edge_index, edge_ptr, sample_ptr, edge_src
