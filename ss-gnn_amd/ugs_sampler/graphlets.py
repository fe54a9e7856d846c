"""Exact graphlet class ids of sampled subgraphs, computed on the GPU.

`ugs_sampler.wl` reproduces the digest the reference's SS-GNN-WL model uses as a stand-in for a sample's isomorphism class.  For
k <= 8 the class itself is small: a graph on n <= 8 vertices is 28 adjacency bits, and there are 1, 2, 4, 11, 34, 156, 1044 and
12 346 graphs on 1 .. 8 vertices.  So the complete vocabulary is a fixed table -- no build pass over a dataset, no unknown id, the
same ids for every dataset and every run -- and WL's merged classes (3 of the 112 connected graphs on 6 vertices, 17 of 853 on 7)
stay apart:

    vocab_size = graphlets.num_classes(k)                                        # the frozen embedding's size, 208 for k = 6
    wl_ids = graphlets.class_ids(nodes, edge_index, edge_ptr)                    # every forward pass, one launch

The law is stated at ugs_graphlet_canon in include/ugs_mi355.h.  A row's key is (n << 28) | canonical code, the canonical code being
the smallest adjacency code over all n! orders of the row's vertices; its class id is the key's rank among all keys with n <= 8, so
the id of a graph does not depend on k and the ids of a k-sampler fill [0, num_classes(k)).  Row status: 0 = classified; 1 = the row
has no entry >= 0; 2 = an edge endpoint outside the row's vertices or an edge_ptr range outside the columns.  A row of status 1 or 2
has key -1 and the id num_classes(k), the len(vocab) convention of `wl.WLVocab.ids`.  The graph is simple: loops are dropped, which
is the one difference from WL's reading of the same row.  Limits: 1 <= k <= 8.

With `uniform_sampler.enumerate_graphs` the ids give a graph's exact graphlet histogram:

    nodes, edge_index, edge_ptr, sample_ptr, _, _ = uniform_sampler.enumerate_graphs(batch.edge_index, batch.ptr, k, device=dev)
    hist = graphlets.histogram(graphlets.class_ids(nodes, edge_index, edge_ptr), sample_ptr, k)     # int64 [G, num_classes(k)]

`census` gives the non-zero columns of that histogram in one call that stores no rows -- the sets are classified where the search
finds them -- so a graph may hold up to 2**32 sets where an enumeration stops at 2**25 rows, and the memory of the call does not
grow with the population.  The law is stated at ugs_graphlet_census in the same header:

    counts, failed = graphlets.census(batch.edge_index, batch.ptr, k, device=dev)      # int64 [G, len(connected_classes(k))]
    assert torch.equal(counts, hist[:, graphlets.connected_classes(k).to(dev)])

`orbit_ids` says where each of a row's vertices sits inside that class: its orbit under the class's automorphism group (centre or
leaf of a star, end or middle of a path).  The law is stated at ugs_graphlet_orbits in the same header.  The ROOTED CODE of a vertex
is the smallest adjacency code over the orders that put it last; two vertices of a row lie in one orbit exactly when their rooted
codes are equal.  A class's orbits are numbered by ascending rooted code and the orbit id is orbit_base[class id] + that number, so
like the class id it does not depend on k and the ids of a k-sampler fill [0, num_orbits(k)); num_orbits(k) marks a slot < 0 and
every slot of a row of status 1 or 2.  The numbering is this library's own (`orbit_info` decodes it), not ORCA's.  A fixed
embedding of num_orbits(k) + 1 rows is an exact structural feature of every slot, and over the enumerated population the ids count
the graphlet degree vector of every vertex -- how often it occupies each orbit of each connected k-graphlet:

    orbit = graphlets.orbit_ids(nodes, edge_index, edge_ptr)                                        # int64 [S, k]
    gdv = graphlets.vertex_orbit_counts(nodes, orbit, batch.num_nodes, graphlets.connected_orbits(k))

`vertex_census` gives that degree vector in one call that stores no rows, as `census` gives the histogram: every set adds to the rows
of its k members where the search finds it, up to 2**32 sets a graph, k <= 7.  The law is stated at ugs_graphlet_vertex_census in
the same header:

    gdv, failed = graphlets.vertex_census(batch.edge_index, batch.ptr, k, device=dev)   # int64 [N, len(connected_orbits(k))]

Both censuses take form="csr" for graphs above the uniform sampler's size rule -- the 1 M-vertex graph of the headline workload, a
PROTEINS graph of 600 vertices at k = 7: the same results from a search over adjacency lists, k <= 7, up to 2**62 sets a graph:

    counts, failed = graphlets.census(edge_index, ptr, 4, limit=1 << 40, form="csr")   # edge_index on the GPU is used where it is

`labelled_keys` is the exact class of a row as a NODE-LABELLED graph (the reference's use_node_features_in_wl): two rows of one shape
with different atoms are different classes.  The law is stated at ugs_graphlet_labelled in the same header.  The orders are restricted
to those that put the labels in non-decreasing order by position, the labelled canonical code is the smallest adjacency code over
them, and the key is the 128-bit number n * 2^124 + code * 2^96 + sum of L[p] * 2^(12 p), L the row's labels sorted ascending, in
the [S, 2] int64 form of `wl.wl_hash`'s digests.  There is no fixed table of labelled classes; the vocabulary is built from the data
by the functions that take digests, and a frozen embedding reads exact ids through the path it uses for WL ids:

    labels = graphlets.compact_labels(wl.feature_labels(data.x), alphabet)        # or atom numbers: int64 [N] in [0, 4096)
    for batch in loader:                                                         # once over the dataset
        key, status = graphlets.labelled_keys(nodes, edge_index, edge_ptr, labels)
        wl.extend_vocab(vocab, key, status)
    table = wl.WLVocab(vocab, dev)
    ids = table.lookup(*graphlets.labelled_keys(nodes, edge_index, edge_ptr, labels))        # every step: two launches

Status 3: an entry >= len(node_labels) or a label outside [0, 4096); such a row has key (-1, -1).  With return_orbits the same launch
numbers the orbits of the label-preserving automorphism group inside every row.
"""
import ctypes as C

import numpy as np
import torch

from . import _graphs, _select_device
from ._lib import check, lib
from .wl import _check_inputs, _check_labels, _placed

__all__ = ["canonical", "class_ids", "num_classes", "table", "decode", "is_connected", "histogram", "search_stats",
           "orbit_ids", "num_orbits", "orbit_base", "orbit_info", "connected_orbits", "vertex_orbit_counts",
           "labelled_keys", "decode_labelled", "compact_labels", "LABEL_BITS", "census", "connected_classes",
           "vertex_census"]

KMAX = 8
LABEL_BITS = 12                                         # a label's width in a labelled key: labels lie in [0, 4096)
_NUM_CLASSES = (1, 3, 7, 18, 52, 208, 1252, 13598)     # graphs on at most k vertices, k = 1 .. 8
_host_tables = {}                                       # n -> numpy int64 keys of the graphs on exactly n vertices
_dev_tables = {}                                        # (device index, k) -> the table for n <= k on that GPU
_NUM_ORBITS = (1, 3, 9, 29, 119, 663, 5759, 85023)      # orbits of the graphs on at most k vertices, k = 1 .. 8
_host_orbit_counts = {}                                 # n -> numpy int64 orbit counts of the graphs on exactly n vertices, in table order
_dev_bases = {}                                         # (device index, k) -> orbit_base(k) on that GPU
_host_connected = {}                                    # k -> connected_classes(k)
_dev_census = {}                                        # (device index, k) -> census' column keys and code -> column table on that GPU
_dev_vertex_census = {}                                 # (device index, k) -> vertex_census' orbit bases, width and code table on that GPU


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("k must be an int")
    if not 1 <= k <= KMAX:                              # the library states the limit
        check(lib.ugs_graphlet_canon(None, None, 0, 0, None, 0, k, None, 0, None, None, None))


def num_classes(k):
    """The number of graphs on at most k vertices, 1 <= k <= 8: 1, 3, 7, 18, 52, 208, 1252, 13598.  The ids of `class_ids` on
    [S, k] rows are below it, and it is the id of a row without a class."""
    _check_k(k)
    return _NUM_CLASSES[k - 1]


def _table_n(n):
    if n not in _host_tables:
        count = C.c_int64(0)
        check(lib.ugs_graphlet_table(n, None, 0, C.byref(count)))
        keys = np.empty((count.value,), dtype=np.int64)
        check(lib.ugs_graphlet_table(n, keys.ctypes.data, keys.size, C.byref(count)))
        _host_tables[n] = keys
    return _host_tables[n]


def table(k):
    """The keys of all graphs on at most k vertices, ascending: int64 [num_classes(k)] on the host; table(k)[id] is the key of
    class `id`.  Built by the library on first use (all of k = 8 takes a fraction of a second) and kept."""
    _check_k(k)
    return torch.from_numpy(np.concatenate([_table_n(n) for n in range(1, k + 1)]))


def _device_table(dev, k):
    key = (dev.index, k)
    if key not in _dev_tables:
        _dev_tables[key] = table(k).to(dev)
    return _dev_tables[key]


def _canon_on_device(nodes, edge_index, edge_ptr, with_ids):
    """(key int64 [S], status int32 [S], ids int64 [S] or None) on the tensors' GPU; the library's device and stream are selected."""
    dev = nodes.device
    S, k = nodes.shape
    tab = _device_table(dev, k) if with_ids and 1 <= k <= KMAX else None
    key = torch.empty((S,), dtype=torch.int64, device=dev)
    status = torch.empty((S,), dtype=torch.int32, device=dev)
    ids = torch.empty((S,), dtype=torch.int64, device=dev) if with_ids else None
    nodes, edge_ptr = nodes.contiguous(), edge_ptr.contiguous()
    E = edge_index.size(1)
    if E > 0 and edge_index.stride(1) != 1:
        edge_index = edge_index.contiguous()
    stride = edge_index.stride(0) if E > 0 else 0
    if S > 0 or not 1 <= k <= KMAX:                     # the library states the limit
        check(lib.ugs_graphlet_canon(nodes.data_ptr(), edge_index.data_ptr() if E > 0 else None, stride, E, edge_ptr.data_ptr(), S, k,
                                     tab.data_ptr() if tab is not None else None, tab.numel() if tab is not None else 0,
                                     key.data_ptr(), status.data_ptr(), ids.data_ptr() if with_ids else None))
    return key, status, ids


def canonical(nodes_sampled, edge_index_sampled, edge_ptr, *, device=None):
    """Key and status of every sampled subgraph: (key int64 [S], status int32 [S]).

    The inputs are the first three outputs of any sampler's sample_batch / sample_graphs in mode "sample" (or of
    PresampleCache.load, or of uniform_sampler.enumerate_graphs).  key[i] = (n << 28) | canonical code of row i, -1 where
    status != 0; two rows have the same key exactly when their subgraphs are isomorphic.  Device tensors are used in place (a
    strided edge_index too) and the results stay there, on torch's current stream; CPU tensors are copied to `device` (default: the
    current GPU) and the results come back on the CPU.  One launch, no synchronisation with the host."""
    _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, 0)
    nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, device)
    _select_device(dev, jobs=True)
    key, status, _ = _canon_on_device(nodes, edge_index, eptr, False)
    return (key.cpu(), status.cpu()) if back else (key, status)


def class_ids(nodes_sampled, edge_index_sampled, edge_ptr, *, device=None):
    """The graphlet class id of every sampled subgraph: int64 [S] with values in [0, num_classes(k)), and num_classes(k) for a row
    of status 1 or 2 (module docstring).  What `wl.WLVocab.ids` answers with a vocabulary, without one: table(k)[id] is the row's
    key.  Placement as `canonical`; the key table (at most 13 598 int64) is uploaded once per device and k.  One launch."""
    _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, 0)
    nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, device)
    _select_device(dev, jobs=True)
    _, _, ids = _canon_on_device(nodes, edge_index, eptr, True)
    return ids.cpu() if back else ids


def decode(key):
    """(n, [(i, j), ...]) of a key: the vertex count and the edges i < j of the class's canonical representative."""
    key = int(key)
    n = key >> 28
    if not 1 <= n <= KMAX or (key & ((1 << 28) - 1)) >> (n * (n - 1) // 2):
        raise ValueError(f"{key} is no graphlet key")
    return n, [(i, j) for j in range(1, n) for i in range(j) if key >> (j * (j - 1) // 2 + i) & 1]


def is_connected(keys):
    """bool tensor, on the device of `keys` (int64, any shape): whether the graph of each key is connected; False for -1.
    Plain torch bit operations, no synchronisation."""
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64:
        raise TypeError("keys must be an int64 torch.Tensor")
    ok = keys >= 0
    k = torch.where(ok, keys, torch.zeros_like(keys))
    n = k >> 28
    nb = [torch.zeros_like(k) for _ in range(KMAX)]     # neighbour masks
    for j in range(1, KMAX):
        for i in range(j):
            bit = (k >> (j * (j - 1) // 2 + i)) & 1
            nb[i] = nb[i] | (bit << j)
            nb[j] = nb[j] | (bit << i)
    reach = torch.ones_like(k)
    for _ in range(KMAX - 1):
        step = reach
        for v in range(KMAX):
            step = step | (nb[v] * ((reach >> v) & 1))
        reach = step
    return ok & (n >= 1) & (reach == (torch.ones_like(k) << n) - 1)


def histogram(class_ids, sample_ptr, k):
    """The graphlet counts of every graph: int64 [G, num_classes(k)], row g counting the ids of rows sample_ptr[g] ..
    sample_ptr[g+1]-1.  Rows with the id num_classes(k) are not counted.  Over `uniform_sampler.enumerate_graphs` rows this is
    the graph's exact k-graphlet histogram.  A torch scatter on the tensors' device, no synchronisation."""
    for t, name in ((class_ids, "class_ids"), (sample_ptr, "sample_ptr")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {t.dtype}")
    if class_ids.dim() != 1:
        raise ValueError("class_ids must have shape [S]")
    if sample_ptr.dim() != 1 or sample_ptr.numel() < 1:
        raise ValueError("sample_ptr must have shape [G + 1]")
    if class_ids.device != sample_ptr.device:
        raise ValueError("class_ids and sample_ptr must be on one device")
    classes = num_classes(k)
    G, S = sample_ptr.numel() - 1, class_ids.numel()
    graph = torch.searchsorted(sample_ptr[1:].contiguous(), torch.arange(S, dtype=torch.int64, device=class_ids.device), right=True)
    counted = (class_ids >= 0) & (class_ids < classes) & (graph < G)
    slot = torch.where(counted, graph * classes + class_ids, torch.zeros_like(class_ids))
    out = torch.zeros((G * classes,), dtype=torch.int64, device=class_ids.device)
    out.scatter_add_(0, slot, counted.to(torch.int64))
    return out.view(G, classes)


def search_stats(key_or_code, n=None):
    """(leaves, nodes): the complete codes the canonical search compares for a graph and the search nodes it evaluates, its measures
    of cost; (1, n - 1) for a graph without symmetry.  Takes a key, or a raw adjacency code with n.  Host only."""
    code = int(key_or_code)
    if n is None:
        n, code = code >> 28, code & ((1 << 28) - 1)
    leaves, nodes = C.c_uint32(0), C.c_uint32(0)
    check(lib.ugs_graphlet_search_stats(code, n, C.byref(leaves), C.byref(nodes)))
    return leaves.value, nodes.value


def _orbit_counts_n(n):
    if n not in _host_orbit_counts:
        count = C.c_int64(0)
        check(lib.ugs_graphlet_orbit_counts(n, None, 0, C.byref(count)))
        counts = np.empty((count.value,), dtype=np.int64)
        check(lib.ugs_graphlet_orbit_counts(n, counts.ctypes.data, counts.size, C.byref(count)))
        _host_orbit_counts[n] = counts
    return _host_orbit_counts[n]


def num_orbits(k):
    """The number of vertex orbits of the graphs on at most k vertices, 1 <= k <= 8: 1, 3, 9, 29, 119, 663, 5759, 85023.  The ids
    of `orbit_ids` on [S, k] rows are below it, and it is the id of a slot without a vertex."""
    _check_k(k)
    return _NUM_ORBITS[k - 1]


def orbit_base(k):
    """int64 [num_classes(k) + 1] on the host: orbit_base(k)[c] is the first orbit id of class c, the orbits of class c being
    orbit_base(k)[c] .. orbit_base(k)[c + 1] - 1, and the last entry is num_orbits(k).  Built by the library on first use (all of
    k = 8 takes a fraction of a second) and kept."""
    _check_k(k)
    counts = np.concatenate([_orbit_counts_n(n) for n in range(1, k + 1)])
    return torch.from_numpy(np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)]))


def _rooted_codes(code, n):
    out = (C.c_uint32 * KMAX)()
    check(lib.ugs_graphlet_rooted_codes(code, n, out))
    return list(out)[:n]


def orbit_info(orbit_id):
    """(class id, class key, rooted code, orbit size, degree) of an orbit id: the class the orbit belongs to, the rooted code that
    its vertices share, how many of the class's vertices it holds and the degree each of them has.  Vertex v of the class's
    canonical representative `decode(key)` lies in it exactly when its rooted code is that one.  Host only."""
    if isinstance(orbit_id, bool) or not isinstance(orbit_id, int):
        raise TypeError("orbit_id must be an int")
    if not 0 <= orbit_id < _NUM_ORBITS[-1]:
        raise ValueError(f"{orbit_id} is no orbit id")
    base = orbit_base(KMAX).numpy()
    cid = int(np.searchsorted(base, orbit_id, side="right")) - 1
    key = int(table(KMAX)[cid])
    n = key >> 28
    rooted = _rooted_codes(key & ((1 << 28) - 1), n)
    code = sorted(set(rooted))[orbit_id - int(base[cid])]
    return cid, key, code, rooted.count(code), bin(code >> ((n - 1) * (n - 2) // 2)).count("1")


def connected_orbits(k):
    """The ids of the orbits of the connected graphs on exactly k vertices, ascending: int64 on the host, 1, 1, 3, 11, 58, 407, 4306
    and 72 489 of them for k = 1 .. 8.  The columns of a k-GDV (`vertex_orbit_counts`); connected_orbits(2) .. (5) together are
    the 73 orbits of the graphlets on at most 5 vertices."""
    _check_k(k)
    base, keys = orbit_base(k), table(k)
    first = num_classes(k - 1) if k > 1 else 0
    ids = [torch.arange(int(base[c]), int(base[c + 1]), dtype=torch.int64)
           for c in (first + torch.nonzero(is_connected(keys[first:])).view(-1)).tolist()]
    return torch.cat(ids)


def _device_base(dev, k):
    key = (dev.index, k)
    if key not in _dev_bases:
        _dev_bases[key] = orbit_base(k).to(dev)
    return _dev_bases[key]


def orbit_ids(nodes_sampled, edge_index_sampled, edge_ptr, *, device=None, return_class=False):
    """The orbit id of every slot of every sampled subgraph: int64 [S, k] with values in [0, num_orbits(k)), and num_orbits(k) where
    the entry is < 0 and in every slot of a row of status 1 or 2 (module docstring).  Slot s answers for the vertex that entry s
    of the row is: the j-th entry >= 0 in row order is vertex j of the row's edges.  With return_class, (orbit, class_ids) from
    the same launch, class_ids as `class_ids` returns them.  Placement as `canonical`; the key table and `orbit_base(k)` are
    uploaded once per device and k.  One launch, no synchronisation with the host."""
    _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, 0)
    nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, device)
    _select_device(dev, jobs=True)
    S, k = nodes.shape
    known = 1 <= k <= KMAX
    tab, base = (_device_table(dev, k), _device_base(dev, k)) if known else (None, None)
    orbit = torch.empty((S, k), dtype=torch.int64, device=dev)
    ids = torch.empty((S,), dtype=torch.int64, device=dev) if return_class else None
    nodes, eptr = nodes.contiguous(), eptr.contiguous()
    E = edge_index.size(1)
    if E > 0 and edge_index.stride(1) != 1:
        edge_index = edge_index.contiguous()
    stride = edge_index.stride(0) if E > 0 else 0
    if S > 0 or not known:                              # the library states the limit
        check(lib.ugs_graphlet_orbits(nodes.data_ptr(), edge_index.data_ptr() if E > 0 else None, stride, E, eptr.data_ptr(), S, k,
                                      tab.data_ptr() if known else None, base.data_ptr() if known else None,
                                      tab.numel() if known else 0, orbit.data_ptr(), None, None,
                                      ids.data_ptr() if return_class else None))
    if back:
        orbit, ids = orbit.cpu(), ids.cpu() if return_class else None
    return (orbit, ids) if return_class else orbit


def vertex_orbit_counts(nodes, orbit, num_vertices, columns):
    """How often every vertex occupies every orbit: int64 [num_vertices, len(columns)], entry [v, c] counting the slots with node id
    v and orbit id columns[c].  `nodes` and `orbit` are int64 of one shape on one device (a sampler's nodes [S, k] and
    `orbit_ids` of them); `columns` is an int64 vector of ASCENDING, DISTINCT orbit ids (it is not checked: that would wait for the
    device) and is moved to that device if it is elsewhere.  A slot whose node id is outside [0, num_vertices) or whose orbit id is
    not in `columns` is not counted.  Over `uniform_sampler.enumerate_graphs(..., k)` rows with columns = connected_orbits(k) this is
    the exact k-graphlet degree vector of every vertex of the batch.  There is no default for `columns`: all num_orbits(8) = 85 023
    columns are no sensible width.  A torch searchsorted and one scatter_add_ on the tensors' device, no synchronisation."""
    for t, name in ((nodes, "nodes"), (orbit, "orbit"), (columns, "columns")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {t.dtype}")
    if isinstance(num_vertices, bool) or not isinstance(num_vertices, int):
        raise TypeError("num_vertices must be an int")
    if num_vertices < 0:
        raise ValueError("num_vertices must be >= 0")
    if nodes.shape != orbit.shape:
        raise ValueError("nodes and orbit must have one shape")
    if nodes.device != orbit.device:
        raise ValueError("nodes and orbit must be on one device")
    if columns.dim() != 1:
        raise ValueError("columns must have shape [C]")
    dev, width = nodes.device, columns.numel()
    out = torch.zeros((num_vertices * width,), dtype=torch.int64, device=dev)
    if width > 0 and num_vertices > 0:
        columns = columns.to(dev).contiguous()
        v, o = nodes.reshape(-1), orbit.reshape(-1)
        col = torch.searchsorted(columns, o).clamp_(max=width - 1)
        counted = (columns[col] == o) & (v >= 0) & (v < num_vertices)
        out.scatter_add_(0, torch.where(counted, v * width + col, torch.zeros_like(v)), counted.to(torch.int64))
    return out.view(num_vertices, width)


def labelled_keys(nodes_sampled, edge_index_sampled, edge_ptr, node_labels, *, device=None, return_orbits=False):
    """Key and status of every sampled subgraph as a node-labelled graph: (key int64 [S, 2], status int32 [S]), and with
    return_orbits (key, status, orbit_local int64 [S, k]) from the same launch.

    node_labels is int64 [N] on the device of the sampler tensors, with values in [0, 4096) (`compact_labels` makes them); the
    label of a row's vertex is node_labels[entry].  key[i] holds the high and the low word of the 128-bit key of the module
    docstring as int64 bit patterns, (-1, -1) where status != 0: two rows have the same key exactly when an isomorphism of their
    subgraphs maps labels to equal labels.  The form is that of `wl.wl_hash`'s digests: `wl.hexdigests`, `wl.extend_vocab`,
    `wl.WLVocab` and `WLVocab.lookup` take it as it is, and `decode_labelled` reads it back.  Status 0, 1 and 2 as `canonical`;
    3 = an entry >= N or a label outside [0, 4096), checked after 1 and 2.

    orbit_local[i, s] numbers the orbit, under the label-preserving automorphism group of row i, of the vertex that slot s is:
    0, 1, ... by ascending (label, labelled rooted code), and k where the entry is < 0 or status != 0.  With all labels equal it is
    `orbit_ids` minus orbit_base[class id].  Placement as `canonical`.  One launch, no synchronisation with the host."""
    _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, 0)
    if node_labels is None:
        raise TypeError("node_labels must be a torch.Tensor")
    _check_labels(nodes_sampled, None, node_labels)
    nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, device)
    _select_device(dev, jobs=True)
    labels = node_labels.to(dev).contiguous()
    S, k = nodes.shape
    N = labels.numel()
    key = torch.empty((S, 2), dtype=torch.int64, device=dev)
    status = torch.empty((S,), dtype=torch.int32, device=dev)
    orbit = torch.empty((S, k), dtype=torch.int64, device=dev) if return_orbits else None
    nodes, eptr = nodes.contiguous(), eptr.contiguous()
    E = edge_index.size(1)
    if E > 0 and edge_index.stride(1) != 1:
        edge_index = edge_index.contiguous()
    stride = edge_index.stride(0) if E > 0 else 0
    if S > 0 or not 1 <= k <= KMAX:                     # the library states the limit
        check(lib.ugs_graphlet_labelled(nodes.data_ptr(), edge_index.data_ptr() if E > 0 else None, stride, E, eptr.data_ptr(), S, k,
                                        labels.data_ptr() if N > 0 else None, N, key.data_ptr(), status.data_ptr(),
                                        orbit.data_ptr() if return_orbits and S > 0 else None))
    if back:
        key, status, orbit = key.cpu(), status.cpu(), orbit.cpu() if return_orbits else None
    return (key, status, orbit) if return_orbits else (key, status)


def connected_classes(k):
    """The class ids of the connected graphs on exactly k vertices, ascending: int64 on the host, 1, 1, 2, 6, 21, 112, 853 and
    11 117 of them for k = 1 .. 8.  The columns of `census`, and the only columns of a `histogram` over `enumerate_graphs` rows
    that can be non-zero; the class-level sibling of `connected_orbits`."""
    _check_k(k)
    if k not in _host_connected:
        first = num_classes(k - 1) if k > 1 else 0
        _host_connected[k] = first + torch.nonzero(is_connected(table(k)[first:])).view(-1)
    return _host_connected[k].clone()


def _census_tables(dev, k):
    """(keys of the columns int64 [W], code -> column table or None) on `dev`; the library's device and stream are selected.  The
    table of k <= 7 is built by one launch over all 2^(k (k-1) / 2) codes, once per device and k."""
    at = (dev.index, k)
    if at not in _dev_census:
        keys = table(k)[connected_classes(k)].to(dev)
        code_col = None
        if k < KMAX:
            code_col = torch.empty((1 << (k * (k - 1) // 2),), dtype=torch.int16, device=dev)     # uint16 bit patterns
            check(lib.ugs_graphlet_census_table(k, keys.data_ptr(), keys.numel(), code_col.data_ptr()))
            torch.cuda.current_stream(dev).synchronize()                                           # later calls may run on other streams
        _dev_census[at] = (keys, code_col)
    return _dev_census[at]


_FORMS = ("bitmap", "csr")


def _check_form(form):
    if form not in _FORMS:
        raise ValueError(f"form must be one of {_FORMS}, got {form!r}")


def _check_limit(limit, form):
    limit = int(limit)
    top = 62 if form == "csr" else 32
    if not 1 <= limit <= 1 << top:
        raise ValueError(f"limit must be 1 ... 2**{top}, got {limit}")
    return limit


def _simple_csr(edge_index, ptr):
    """The simple graph of a batch as a CSR: (rowptr int64 [N + 1], col int32 [M]) on the device of `edge_index`, N = ptr[-1].  Item 1
    of the census law as a data structure: only columns with both endpoints inside one graph's range are kept (an endpoint outside
    [0, N) lies in no graph: such a column is dropped, as the bitmap form drops it), the adjacency is symmetrised, loops are dropped,
    duplicates collapse, and every row is strictly ascending.  Torch ops only -- bucketize by ptr, keys u * N + v, unique,
    searchsorted -- so it runs on CPU tensors as well.  ptr is taken as it is; the library checks it."""
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise RuntimeError("edge_index must have shape [2, E]")
    dev = edge_index.device
    ptr = ptr.to(dev).contiguous()
    G = ptr.numel() - 1
    N = max(int(ptr[-1]), 0) if G >= 0 else 0
    u, v = edge_index[0].contiguous(), edge_index[1].contiguous()
    gu = torch.bucketize(u, ptr, right=True)            # ptr[gu - 1] <= u < ptr[gu]: graph gu - 1, for 1 <= gu <= G
    gv = torch.bucketize(v, ptr, right=True)
    keep = (gu >= 1) & (gu <= G) & (gu == gv) & (u != v) & (u >= 0) & (u < N) & (v >= 0) & (v < N)
    u, v = u[keep], v[keep]
    keys = torch.unique(torch.cat([u * N + v, v * N + u]))                      # sorted: by row, then ascending inside the row
    rowptr = torch.searchsorted(keys, torch.arange(N + 1, dtype=torch.int64, device=dev) * N)
    col = (keys % max(N, 1)).to(torch.int32)
    return rowptr, col


def _csr_inputs(edge_index, ptr, device, k, limit):
    """(rowptr, col, ptr, G, N, dev, back) of a csr-form call: the CSR and ptr on the GPU the call runs on.  Device tensors are used
    where they are; CPU tensors go up once.  The form's limits are refused here: N before the CSR is built (its keys u * N + v need
    N < 2**31), the entries behind it."""
    for t, name in ((edge_index, "edge_index"), (ptr, "ptr")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    _graphs.check_int64(edge_index, ptr)
    if ptr.dim() != 1 or ptr.numel() < 1:
        raise RuntimeError("ptr must hold at least one entry")
    back = device is None and edge_index.device.type != "cuda"
    dev = torch.device(device) if device is not None else edge_index.device if not back else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("device= must be a GPU device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    ptr = ptr.to(dev).contiguous()
    if int(ptr[-1]) >= 1 << 31:
        _refuse_csr(k, limit, int(ptr[-1]), 0)
    rowptr, col = _simple_csr(edge_index.to(dev), ptr)
    if col.numel() >= 1 << 31:
        _refuse_csr(k, limit, rowptr.numel() - 1, col.numel())
    G = ptr.numel() - 1
    return rowptr, col, ptr, G, rowptr.numel() - 1, dev, back


def _refuse_csr(k, limit, N=0, M=0):
    """The refusals of the csr form that touch no device, stated by the library."""
    check(lib.ugs_graphlet_census_csr(None, 0, None, None, N, M, k, limit, None, 0, None, None, None))


def census(edge_index, ptr, k, *, limit=1 << 25, device=None, form="bitmap"):
    """The exact k-graphlet histogram of every graph of a batch: (counts int64 [G, W], failed host bool [G]), W =
    len(connected_classes(k)), counts[g, c] the number of connected k-subsets of graph g whose class id is connected_classes(k)[c].

    What histogram(class_ids(rows), sample_ptr, k)[:, connected_classes(k)] gives over `uniform_sampler.enumerate_graphs` rows, bit
    for bit, without the rows: every set is classified where the search finds it and nothing is stored per set, so the call's memory
    does not grow with the population and a graph may hold up to `limit` sets, 1 ... 2**32 (ValueError otherwise), the bound of
    `count_graphs`, not the 2**25 rows of an enumeration.  The law is stated at ugs_graphlet_census in include/ugs_mi355.h.  A graph
    the samplers refuse for its size (`uniform_sampler.set_max_vertices` raises that limit for the census too) or with more than
    `limit` sets has failed[g] = True and a row of zeros, and leaves the other graphs exact; there is no joint budget.  Arguments and
    their errors are those of `count_graphs`.  counts is on the device of `edge_index`, or on `device`; for CPU tensors without
    `device` the work runs on the current GPU and counts comes back on the CPU.  One synchronous call on torch's current stream.
    For k <= 7 a set's class is one table load and the call is several times faster than the recipe; at k = 8 it is a canonical search
    per set, slower than the recipe wherever the recipe can hold the rows.

    form="csr" gives the same result for graphs of ANY size: the search runs over sorted adjacency lists (`_simple_csr`) instead of
    bitmap rows, so no graph fails for its size and `set_max_vertices` plays no part.  k = 1 ... 7 (k = 8 is refused before any device
    work); `limit` may be 1 ... 2**62; N = ptr[-1] < 2**31 and at most 2**31 - 1 adjacency entries.  A GPU `edge_index` or `ptr` is used
    where it is, CPU tensors are uploaded once.  On graphs the default form accepts, the default is the faster one: the form is for the
    graphs it refuses.  The law is stated at ugs_graphlet_census_csr in the same header.  A `form` other than
    "bitmap" and "csr" is a ValueError, before anything else."""
    _check_form(form)
    _check_k(k)
    limit = _check_limit(limit, form)
    if form == "csr":
        if k == KMAX:                                   # the library states the refusal, before any device work
            _refuse_csr(k, limit)
        rowptr, col, pt, G, N, dev, back = _csr_inputs(edge_index, ptr, device, k, limit)
        _graphs._select_device(dev, jobs=True)
        keys, code_col = _census_tables(dev, k)
        counts = torch.empty((G, keys.numel()), dtype=torch.int64, device=dev)
        status = np.zeros(max(G, 1), dtype=np.int32)
        check(lib.ugs_graphlet_census_csr(pt.data_ptr(), G, rowptr.data_ptr(), col.data_ptr() if col.numel() > 0 else None, N, col.numel(), k,
                                          limit, keys.data_ptr(), keys.numel(), code_col.data_ptr(), counts.data_ptr() if G > 0 else None,
                                          status.ctypes.data))
        return counts.cpu() if back else counts, torch.from_numpy(status[:G] != 0)
    for t, name in ((edge_index, "edge_index"), (ptr, "ptr")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    _graphs.check_int64(edge_index, ptr)
    back = device is None and edge_index.device.type != "cuda"
    dev = torch.device(device) if device is not None else edge_index.device if not back else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("device= must be a GPU device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    keep, p, stride, e = _graphs._edge_index_view(edge_index.cpu())
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    _graphs._select_device(dev, jobs=True)
    keys, code_col = _census_tables(dev, k)
    counts = torch.empty((max(G, 0), keys.numel()), dtype=torch.int64, device=dev)
    status = np.zeros(max(G, 1), dtype=np.int32)
    check(lib.ugs_graphlet_census(p, stride, e, pt.data_ptr(), G, k, limit, keys.data_ptr(), keys.numel(),
                                  code_col.data_ptr() if code_col is not None else None, counts.data_ptr() if G > 0 else None,
                                  status.ctypes.data))
    return counts.cpu() if back else counts, torch.from_numpy(status[:max(G, 0)] != 0)


def _vertex_census_tables(dev, k):
    """(orbit bases of the connected classes int64 [W + 1], code -> (class column, orbit of every position) table) on `dev`, k <= 7; the
    library's device and stream are selected.  The table is built by one launch over all 2^(k (k-1) / 2) codes, once per device and k."""
    at = (dev.index, k)
    if at not in _dev_vertex_census:
        classes = connected_classes(k)
        first = num_classes(k - 1) if k > 1 else 0
        sizes = _orbit_counts_n(k)[(classes - first).numpy()]
        obase = torch.from_numpy(np.concatenate([np.zeros(1, np.int64), np.cumsum(sizes)])).to(dev)
        keys = table(k)[classes].to(dev)
        tab = torch.empty((1 << (k * (k - 1) // 2),), dtype=torch.int32, device=dev)               # uint32 bit patterns
        check(lib.ugs_graphlet_vertex_census_table(k, keys.data_ptr(), keys.numel(), tab.data_ptr()))
        torch.cuda.current_stream(dev).synchronize()                                               # later calls may run on other streams
        _dev_vertex_census[at] = (obase, int(sizes.sum()), tab)
    return _dev_vertex_census[at]


def vertex_census(edge_index, ptr, k, *, limit=1 << 25, device=None, form="bitmap"):
    """The exact k-graphlet degree vector of every vertex of a batch: (gdv int64 [N, O], failed host bool [G]), N = ptr[-1], O =
    len(connected_orbits(k)) = 1, 1, 3, 11, 58, 407, 4306 for k = 1 .. 7; gdv[v, c] is the number of connected k-subsets of v's graph
    that contain v and in which v's orbit id is connected_orbits(k)[c].

    What vertex_orbit_counts(nodes, orbit_ids(rows), N, connected_orbits(k)) gives over `uniform_sampler.enumerate_graphs` rows, bit
    for bit, without the rows: every set adds to the rows of its k members where the search finds it, so a graph may hold up to
    `limit` sets, 1 ... 2**32 (ValueError otherwise), and beside the result the call's memory does not grow with the population.  The
    result is 8 * N * O bytes -- 34 KiB per vertex at k = 7, 3.2 KiB at k = 6 -- allocated with torch; there is no cap of the call's
    own.  The law is stated at ugs_graphlet_vertex_census in include/ugs_mi355.h; summed over a graph's vertices a column is the
    orbit's size times `census`' count of its class.  A graph the samplers refuse for its size or with more than `limit` sets has
    failed[g] = True and rows of zeros for all its vertices, and leaves every other vertex exact; rows of vertices below ptr[0] are
    zero.  k = 8 is refused (72 489 columns a vertex and a canonical search a set are no sensible call), before any device is touched.
    Arguments, their errors, placement (gdv on the device of `edge_index`, or on `device`; CPU tensors in and gdv back on the CPU)
    and `uniform_sampler.set_max_vertices` are as for `census`.  One synchronous call on torch's current stream (DESIGN.md section
    19.4).

    form="csr": the same result for graphs of any size, as `census` describes it -- no size refusal, `limit` 1 ... 2**62, device
    tensors used where they are (ugs_graphlet_vertex_census_csr in the same header)."""
    _check_form(form)
    _check_k(k)
    if k == KMAX:                                       # the library states the refusal, before any device work
        if form == "csr":
            _refuse_csr(k, 1)
        check(lib.ugs_graphlet_vertex_census(None, 0, 0, None, 0, k, 1, 0, None, 0, None, None, None))
    limit = _check_limit(limit, form)
    if form == "csr":
        rowptr, col, pt, G, N, dev, back = _csr_inputs(edge_index, ptr, device, k, limit)
        _graphs._select_device(dev, jobs=True)
        obase, O, tab = _vertex_census_tables(dev, k)
        gdv = torch.empty((N, O), dtype=torch.int64, device=dev)
        status = np.zeros(max(G, 1), dtype=np.int32)
        check(lib.ugs_graphlet_vertex_census_csr(pt.data_ptr(), G, rowptr.data_ptr(), col.data_ptr() if col.numel() > 0 else None, N,
                                                 col.numel(), k, limit, obase.numel() - 1, obase.data_ptr(), O, tab.data_ptr(),
                                                 gdv.data_ptr() if N > 0 else None, status.ctypes.data))
        return gdv.cpu() if back else gdv, torch.from_numpy(status[:G] != 0)
    for t, name in ((edge_index, "edge_index"), (ptr, "ptr")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    _graphs.check_int64(edge_index, ptr)
    back = device is None and edge_index.device.type != "cuda"
    dev = torch.device(device) if device is not None else edge_index.device if not back else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("device= must be a GPU device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    keep, p, stride, e = _graphs._edge_index_view(edge_index.cpu())
    pt = ptr.cpu().contiguous()
    G = pt.numel() - 1
    N = max(int(pt[-1]), 0) if G >= 0 else 0            # (the library refuses a ptr that is not sound)
    _graphs._select_device(dev, jobs=True)
    obase, O, tab = _vertex_census_tables(dev, k)
    gdv = torch.empty((N, O), dtype=torch.int64, device=dev)
    status = np.zeros(max(G, 1), dtype=np.int32)
    check(lib.ugs_graphlet_vertex_census(p, stride, e, pt.data_ptr(), G, k, limit, obase.numel() - 1, obase.data_ptr(), O,
                                         tab.data_ptr(), gdv.data_ptr() if N > 0 else None, status.ctypes.data))
    return gdv.cpu() if back else gdv, torch.from_numpy(status[:max(G, 0)] != 0)


def decode_labelled(key):
    """(n, code, labels) of labelled keys: `key` is int64 [..., 2] (high word, low word); n and code are int64 [...], the vertex
    count and the labelled canonical code -- bit j (j - 1) / 2 + i is the pair i < j of the representative -- and labels is int64
    [..., 8], the label of the representative's vertex p, ascending, -1 behind n.  A key of (-1, -1), a row of status != 0, gives
    n = 0, code = -1 and labels of -1.  Torch bit operations on the key's device, no synchronisation."""
    if not isinstance(key, torch.Tensor) or key.dtype != torch.int64:
        raise TypeError("key must be an int64 torch.Tensor")
    if key.dim() < 1 or key.size(-1) != 2:
        raise ValueError("key must have shape [..., 2]")
    hi, lo = key[..., 0], key[..., 1]
    none = (hi == -1) & (lo == -1)
    mask = (1 << LABEL_BITS) - 1
    n = torch.where(none, torch.zeros_like(hi), (hi >> 60) & 15)
    code = torch.where(none, torch.full_like(hi, -1), (hi >> 32) & ((1 << 28) - 1))
    fields = [(lo >> (LABEL_BITS * p)) & mask for p in range(5)]
    fields += [((lo >> 60) & 15) | ((hi & 255) << 4), (hi >> 8) & mask, (hi >> 20) & mask]
    labels = torch.stack(fields, dim=-1)
    behind = torch.arange(KMAX, dtype=torch.int64, device=key.device) >= n.unsqueeze(-1)
    return n, code, torch.where(behind, torch.full_like(labels, -1), labels)


def compact_labels(raw, alphabet):
    """Maps arbitrary int64 labels onto [0, len(alphabet)): the index of raw's value in `alphabet`, -1 for a value that is not in it
    (a row with such a vertex gets status 3).  `raw` is an int64 tensor of any shape -- `wl.feature_labels(x)`, atom numbers --
    and `alphabet` an int64 vector of ASCENDING, DISTINCT values of at most 4096 entries (the order is not checked: that would
    wait for the device), moved to raw's device if it is elsewhere; torch.unique(all the dataset's raw labels) is one.  A torch
    searchsorted on raw's device, no synchronisation."""
    for t, name in ((raw, "raw"), (alphabet, "alphabet")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {t.dtype}")
    if alphabet.dim() != 1:
        raise ValueError("alphabet must have shape [A]")
    A = alphabet.numel()
    if A > 1 << LABEL_BITS:
        raise ValueError(f"a labelled key holds {LABEL_BITS} bits per label: at most {1 << LABEL_BITS} labels, got {A}")
    if A == 0:
        return torch.full_like(raw, -1)
    alphabet = alphabet.to(raw.device).contiguous()
    at = torch.searchsorted(alphabet, raw.contiguous()).clamp_(max=A - 1)
    return torch.where(alphabet[at] == raw, at, torch.full_like(at, -1))
