"""Weisfeiler-Lehman graph hashes and vocabulary ids of sampled subgraphs, computed on the GPU.

The reference's SS-GNN-WL model turns every sampled subgraph into a vocabulary id on the host, one sample at a time
(src/gps/gps/models/ss_gnn_wl.py:210-247, `_compute_wl_ids`; vocabulary: src/gps/gps/utils/wl_vocab.py:21-67, 110-183): it slices
the sample's row out of `nodes_sampled`, `edge_index_sampled` and `edge_ptr` (three `.item()` synchronisations), builds a
`networkx.Graph`, calls `weisfeiler_lehman_graph_hash(G, node_attr='attr', iterations=3)` with str(degree) as the attribute and
looks the hex string up in a dict.  Here the same digests -- networkx 3.4.2's, bit for bit -- come from one kernel launch over the
sampler's three output tensors, and the lookup from a second one; nothing synchronises with the host:

    vocab = {}                                                   # once per dataset (build_wl_vocabulary_from_loader)
    for nodes, edge_index, edge_ptr in sampled_batches:
        extend_vocab(vocab, *wl_hash(nodes, edge_index, edge_ptr, iterations=3))
    table = WLVocab(vocab, device="cuda:0")
    wl_ids = table.ids(nodes, edge_index, edge_ptr, iterations=3)   # every forward pass (_compute_wl_ids)

The law is stated at ugs_wl_hash in include/ugs_mi355.h.  Row status: 0 = hashed; 1 = the row has no entry >= 0 (the reference
answers the unknown id); 2 = an edge endpoint outside the row's vertices -- the one deviation: the reference hashes a fallback
string "deg_.._edges_.." there, this module answers the unknown id; no sampler of this library produces such a row in mode
"sample".  Limits: 1 <= k <= 32, 0 <= iterations <= 8.

Node-feature labels (`use_node_features_in_wl=True`, the reference's real-data configs): `x=batch.x` makes the start label of a
vertex the first 8 hex characters of the md5 of its feature row's bytes instead of its degree, as compute_wl_hash does with
node_features (one more launch: the md5 of every row of x, once per vertex of the batch):

    wl_ids = table.ids(nodes, edge_index, edge_ptr, iterations=3, x=batch.x)

`feature_labels(x)` returns those labels (int64 [N], values below 2^32) and `node_labels=` takes them, or any other 32-bit
categorical labels, so that a caller hashes a batch's features once for several calls.  Vertex j of a row is its j-th entry >= 0
(`subgraph_nodes[valid_mask]`).  Row status 3: an entry that is no row of x / node_labels, or a label outside [0, 2^32) -- the
reference raises IndexError there; this module answers no digest and the unknown id, other rows are not disturbed.  Edge
attributes and weisfeiler_lehman_subgraph_hashes are out of scope.
"""
import re

import numpy as np
import torch

from . import _select_device
from ._lib import check, lib

__all__ = ["wl_hash", "feature_labels", "hexdigests", "WLVocab", "extend_vocab"]

_HEX32 = re.compile(r"[0-9a-f]{32}\Z")


def _check_inputs(nodes, edge_index, edge_ptr, iterations):
    for t, name in ((nodes, "nodes_sampled"), (edge_index, "edge_index_sampled"), (edge_ptr, "edge_ptr")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {t.dtype}")
    if isinstance(iterations, bool) or not isinstance(iterations, int):
        raise TypeError("iterations must be an int")
    if nodes.dim() != 2:
        raise ValueError("nodes_sampled must have shape [S, k]")
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("edge_index_sampled must have shape [2, E]")
    if edge_ptr.dim() != 1 or edge_ptr.numel() != nodes.size(0) + 1:
        raise ValueError("edge_ptr must have shape [S + 1]")
    if not (nodes.device == edge_index.device == edge_ptr.device):
        raise ValueError("nodes_sampled, edge_index_sampled and edge_ptr must be on one device")
    if nodes.device.type not in ("cpu", "cuda"):
        raise ValueError("tensors must be on the CPU or on a GPU")


# dtypes numpy represents: the reference hashes x[i].numpy().tobytes(), which fails for any other one (bfloat16, ...)
_FEATURE_DTYPES = (torch.float16, torch.float32, torch.float64, torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8, torch.bool)


def _check_x(x):
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype not in _FEATURE_DTYPES:
        raise TypeError(f"x must have a dtype numpy represents (float16/32/64, int8/16/32/64, uint8, bool), got {x.dtype}")
    if x.dim() < 1:
        raise ValueError("x must have shape [N, ...]")
    if x.device.type not in ("cpu", "cuda"):
        raise ValueError("x must be on the CPU or on a GPU")


def _check_labels(nodes, x, node_labels):
    """Validation of the two label keywords against the sampler tensors, before any device work."""
    if x is not None and node_labels is not None:
        raise ValueError("x= and node_labels= are mutually exclusive")
    if x is not None:
        _check_x(x)
    if node_labels is not None:
        if not isinstance(node_labels, torch.Tensor):
            raise TypeError("node_labels must be a torch.Tensor")
        if node_labels.dtype != torch.int64:
            raise TypeError(f"node_labels must be int64, got {node_labels.dtype}")
        if node_labels.dim() != 1:
            raise ValueError("node_labels must have shape [N]")
    given = x if x is not None else node_labels
    if given is not None and given.device != nodes.device:
        raise ValueError(f"the sampler tensors are on {nodes.device}, the labels on {given.device}")


def _labels_on_device(x):
    """label32 of every row of the GPU tensor x: int64 [N]; the library's device and stream are already selected."""
    N = x.size(0)
    rows = x.reshape(N, int(np.prod(x.shape[1:], dtype=np.int64)))
    row_bytes = rows.size(1) * rows.element_size()
    if not (rows.stride(1) == 1 or rows.size(1) <= 1) or (N > 1 and rows.stride(0) < rows.size(1)):
        rows = rows.contiguous()                       # the logical C order of a row's elements
    stride_bytes = rows.stride(0) * rows.element_size() if N > 1 else row_bytes
    labels = torch.empty((N,), dtype=torch.int64, device=x.device)
    if N > 0 or row_bytes >= 1 << 29:                  # the library states the limit
        check(lib.ugs_wl_feature_labels(rows.data_ptr() if row_bytes > 0 and N > 0 else None, row_bytes, max(stride_bytes, row_bytes), N, labels.data_ptr()))
    return labels


def _gpu_of(t, device):
    """The GPU that works on tensor t (its own, or `device` for a CPU tensor), and whether results go back to the CPU."""
    if t.device.type == "cuda":
        if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, t.device.index):
            raise ValueError(f"the tensors are on {t.device}, device={device} names another GPU")
        return t.device, False
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("device= must be a GPU device: the hashes are computed there")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev, True


def feature_labels(x, *, device=None):
    """The node-feature start labels of the reference's compute_wl_hash: int64 [N] with
    labels[i] = int(hashlib.md5(x[i].numpy().tobytes()).hexdigest()[:8], 16), computed on the GPU in one launch.

    x has shape [N, ...] (a 1-D x is N rows of one element) and a dtype numpy represents; a row's bytes are its elements in C
    order in x's own dtype, whatever x's strides.  The result is on x's device: a CPU x is copied to `device` (default: the
    current GPU) and the labels come back on the CPU.  For `wl_hash(..., node_labels=)` and `WLVocab.ids(..., node_labels=)`."""
    _check_x(x)
    dev, back = _gpu_of(x, device)
    _select_device(dev, jobs=True)
    labels = _labels_on_device(x.to(dev))
    return labels.cpu() if back else labels


def _hash_on_device(nodes, edge_index, edge_ptr, iterations, x=None, node_labels=None):
    """(digest int64 [S, 2], status int32 [S]) on the tensors' GPU; the library's device and stream are already selected."""
    dev = nodes.device
    S, k = nodes.shape
    digest = torch.empty((S, 2), dtype=torch.int64, device=dev)
    status = torch.empty((S,), dtype=torch.int32, device=dev)
    nodes, edge_ptr = nodes.contiguous(), edge_ptr.contiguous()
    E = edge_index.size(1)
    if E > 0 and edge_index.stride(1) != 1:
        edge_index = edge_index.contiguous()
    stride = edge_index.stride(0) if E > 0 else 0
    if x is not None:
        node_labels = _labels_on_device(x)
    if node_labels is not None:
        node_labels = node_labels.contiguous()
        N = node_labels.numel()
        if S > 0 or not 1 <= k <= 32 or not 0 <= iterations <= 8:
            check(lib.ugs_wl_hash_labeled(nodes.data_ptr(), edge_index.data_ptr() if E > 0 else None, stride, E, edge_ptr.data_ptr(), S, k, iterations,
                                          node_labels.data_ptr() if N > 0 else None, N, digest.data_ptr(), status.data_ptr()))
    elif S > 0 or not 1 <= k <= 32 or not 0 <= iterations <= 8:     # the library states the limits
        check(lib.ugs_wl_hash(nodes.data_ptr(), edge_index.data_ptr() if E > 0 else None, stride, E, edge_ptr.data_ptr(), S, k, iterations,
                              digest.data_ptr(), status.data_ptr()))
    return digest, status


def _placed(nodes, edge_index, edge_ptr, device):
    """The three tensors on the GPU that does the work (copies of CPU tensors), and whether results go back to the CPU."""
    dev, back = _gpu_of(nodes, device)
    if not back:
        return nodes, edge_index, edge_ptr, dev, False
    return nodes.to(dev), edge_index.to(dev), edge_ptr.to(dev), dev, True


def wl_hash(nodes_sampled, edge_index_sampled, edge_ptr, iterations=3, *, device=None, x=None, node_labels=None):
    """WL graph hash of every sampled subgraph: (digest int64 [S, 2], status int32 [S]).

    The inputs are the first three outputs of any sampler's sample_batch / sample_graphs in mode "sample" (or of
    PresampleCache.load).  digest[i] holds bytes 0-7 and 8-15 of row i's BLAKE2b-128 digest as big-endian numbers (as int64 bit
    patterns; zero where status != 0): `hexdigests` turns them into networkx's strings.  Device tensors are used in place and
    the results stay there, on torch's current stream; CPU tensors are copied to `device` (default: the current GPU) and the
    results come back on the CPU.

    Without `x` and `node_labels` the start labels are the degrees (use_node_features_in_wl=False).  `x=batch.x` [N, ...] gives
    the node-feature form: the label of a vertex is the md5 of its feature row (`feature_labels`, one more launch);
    `node_labels=` int64 [N] supplies the labels directly.  Either lives on the device of the sampler tensors; the two exclude
    each other.  A row with an entry >= N or a label outside [0, 2^32) gets status 3 (module docstring)."""
    _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, iterations)
    _check_labels(nodes_sampled, x, node_labels)
    nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, device)
    _select_device(dev, jobs=True)
    digest, status = _hash_on_device(nodes, edge_index, eptr, iterations, None if x is None else x.to(dev),
                                     None if node_labels is None else node_labels.to(dev))
    return (digest.cpu(), status.cpu()) if back else (digest, status)


def hexdigests(digest, status):
    """networkx's hex strings of `wl_hash` results, None where status != 0 (no vertices, a bad endpoint, or with labels status 3:
    an id or label out of range): for a host-side consumer or a pickled vocabulary."""
    d = digest.detach().cpu().numpy().astype(np.int64, copy=False).view(np.uint64).reshape(-1, 2)
    s = status.detach().cpu().numpy().reshape(-1)
    if d.shape[0] != s.shape[0]:
        raise ValueError("digest [S, 2] and status [S] must describe the same rows")
    return ["%016x%016x" % (int(hi), int(lo)) if st == 0 else None for (hi, lo), st in zip(d, s)]


def extend_vocab(vocab, digest, status):
    """Adds the unseen hashes of one batch to `vocab` (hex string -> id) in row order, with ids len(vocab), len(vocab) + 1, ...:
    one batch's worth of build_wl_vocabulary_from_loader (wl_vocab.py:156-175).  Rows without valid vertices are skipped as the
    reference does, and so are rows of status 2 and 3 (module docstring).  Returns `vocab`."""
    for h in hexdigests(digest, status):
        if h is not None and h not in vocab:
            vocab[h] = len(vocab)
    return vocab


class WLVocab:
    """A WL vocabulary (hex string -> id, e.g. the reference's pickled dict) as a sorted table on the GPU.

    Keys that are not 32 lowercase hex characters -- the reference's fallback strings -- stay on the host and never match a
    digest; they still count towards len(), which is the unknown id, and come back from to_dict()."""

    def __init__(self, vocab, device):
        self._vocab = dict(vocab)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("device must be a GPU device: the table lives there")
        self.host_only = {key: i for key, i in self._vocab.items() if not (isinstance(key, str) and _HEX32.match(key))}
        rows = sorted((int(key, 16), int(i)) for key, i in self._vocab.items() if key not in self.host_only)
        # the table, ascending as 128-bit numbers: keys [V, 2] uint64 (high word, low word), ids [V]
        self.keys = np.array([[v >> 64, v & 0xFFFFFFFFFFFFFFFF] for v, _ in rows], dtype=np.uint64).reshape(-1, 2)
        self.key_ids = np.array([i for _, i in rows], dtype=np.int64)
        self._dev_table = None
        if torch.cuda.is_available():
            self._table()

    def _table(self):
        """The table on the GPU, uploaded once (at construction where a GPU is present)."""
        if self._dev_table is None:
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            self._dev_table = (torch.from_numpy(self.keys.view(np.int64)).to(self.device), torch.from_numpy(self.key_ids).to(self.device))
        return self._dev_table

    def __len__(self):
        return len(self._vocab)

    def to_dict(self):
        return dict(self._vocab)

    def lookup(self, digest, status):
        """ids int64 [S] of `wl_hash` results that live on the table's GPU: the id of each digest, len(self) where it is unknown
        or status != 0 -- rows of status 2 and 3 too (hash_to_id, wl_vocab.py:205-216)."""
        keys, key_ids = self._table()
        if digest.device != self.device or status.device != self.device:
            raise ValueError(f"digest and status must be on {self.device}")
        if digest.dtype != torch.int64 or status.dtype != torch.int32:
            raise TypeError("digest must be int64 and status int32")
        if digest.dim() != 2 or digest.size(1) != 2 or status.dim() != 1 or status.numel() != digest.size(0):
            raise ValueError("digest [S, 2] and status [S] expected")
        _select_device(self.device, jobs=True)
        digest, status = digest.contiguous(), status.contiguous()
        S, V = status.numel(), key_ids.numel()
        out = torch.empty((S,), dtype=torch.int64, device=self.device)
        check(lib.ugs_wl_lookup(digest.data_ptr(), status.data_ptr(), S, keys.data_ptr() if V else None,
                                key_ids.data_ptr() if V else None, V, len(self), out.data_ptr()))
        return out

    def ids(self, nodes_sampled, edge_index_sampled, edge_ptr, iterations=3, *, x=None, node_labels=None):
        """What the reference's _compute_wl_ids returns: int64 [S] on the device of nodes_sampled, len(self) for unknown hashes
        and for rows without valid vertices.  Without `x` and `node_labels` that is use_node_features_in_wl=False; `x=batch.x`
        or `node_labels=feature_labels(batch.x)` is use_node_features_in_wl=True (see `wl_hash`; rows of status 3 get
        len(self)).  Two launches on torch's current stream, three with `x=`, no synchronisation with the host (CPU tensors:
        copied to the table's GPU, the ids come back on the CPU)."""
        _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, iterations)
        _check_labels(nodes_sampled, x, node_labels)
        self._table()
        nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, self.device)
        if dev != self.device:
            raise ValueError(f"the tensors are on {dev}, the vocabulary on {self.device}")
        _select_device(dev, jobs=True)
        digest, status = _hash_on_device(nodes, edge_index, eptr, iterations, None if x is None else x.to(dev),
                                         None if node_labels is None else node_labels.to(dev))
        out = self.lookup(digest, status)
        return out.cpu() if back else out
