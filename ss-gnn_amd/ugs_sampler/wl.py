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
"sample".  Limits: 1 <= k <= 32, 0 <= iterations <= 8.  Node-feature labels (`use_node_features_in_wl=True`: md5 of the feature
bytes), edge attributes and weisfeiler_lehman_subgraph_hashes are out of scope.
"""
import re

import numpy as np
import torch

from . import _select_device
from ._lib import check, lib

__all__ = ["wl_hash", "hexdigests", "WLVocab", "extend_vocab"]

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


def _hash_on_device(nodes, edge_index, edge_ptr, iterations):
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
    if S > 0 or not 1 <= k <= 32 or not 0 <= iterations <= 8:       # the library states the limits
        check(lib.ugs_wl_hash(nodes.data_ptr(), edge_index.data_ptr() if E > 0 else None, stride, E, edge_ptr.data_ptr(), S, k, iterations,
                              digest.data_ptr(), status.data_ptr()))
    return digest, status


def _placed(nodes, edge_index, edge_ptr, device):
    """The three tensors on the GPU that does the work (copies of CPU tensors), and whether results go back to the CPU."""
    if nodes.device.type == "cuda":
        if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, nodes.device.index):
            raise ValueError(f"the tensors are on {nodes.device}, device={device} names another GPU")
        return nodes, edge_index, edge_ptr, nodes.device, False
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("device= must be a GPU device: the hashes are computed there")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return nodes.to(dev), edge_index.to(dev), edge_ptr.to(dev), dev, True


def wl_hash(nodes_sampled, edge_index_sampled, edge_ptr, iterations=3, *, device=None):
    """WL graph hash of every sampled subgraph: (digest int64 [S, 2], status int32 [S]).

    The inputs are the first three outputs of any sampler's sample_batch / sample_graphs in mode "sample" (or of
    PresampleCache.load).  digest[i] holds bytes 0-7 and 8-15 of row i's BLAKE2b-128 digest as big-endian numbers (as int64 bit
    patterns; zero where status != 0): `hexdigests` turns them into networkx's strings.  Device tensors are used in place and
    the results stay there, on torch's current stream; CPU tensors are copied to `device` (default: the current GPU) and the
    results come back on the CPU.  Node-feature labels are not supported (module docstring)."""
    _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, iterations)
    nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, device)
    _select_device(dev, jobs=True)
    digest, status = _hash_on_device(nodes, edge_index, eptr, iterations)
    return (digest.cpu(), status.cpu()) if back else (digest, status)


def hexdigests(digest, status):
    """networkx's hex strings of `wl_hash` results, None where status != 0: for a host-side consumer or a pickled vocabulary."""
    d = digest.detach().cpu().numpy().astype(np.int64, copy=False).view(np.uint64).reshape(-1, 2)
    s = status.detach().cpu().numpy().reshape(-1)
    if d.shape[0] != s.shape[0]:
        raise ValueError("digest [S, 2] and status [S] must describe the same rows")
    return ["%016x%016x" % (int(hi), int(lo)) if st == 0 else None for (hi, lo), st in zip(d, s)]


def extend_vocab(vocab, digest, status):
    """Adds the unseen hashes of one batch to `vocab` (hex string -> id) in row order, with ids len(vocab), len(vocab) + 1, ...:
    one batch's worth of build_wl_vocabulary_from_loader (wl_vocab.py:156-175).  Rows without valid vertices are skipped as the
    reference does, and so are rows of status 2 (module docstring).  Returns `vocab`."""
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
        or status != 0 (hash_to_id, wl_vocab.py:205-216)."""
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

    def ids(self, nodes_sampled, edge_index_sampled, edge_ptr, iterations=3):
        """What the reference's _compute_wl_ids returns with use_node_features_in_wl=False: int64 [S] on the device of
        nodes_sampled, len(self) for unknown hashes and for rows without valid vertices.  Two launches on torch's current
        stream, no synchronisation with the host (CPU tensors: copied to the table's GPU, the ids come back on the CPU)."""
        _check_inputs(nodes_sampled, edge_index_sampled, edge_ptr, iterations)
        self._table()
        nodes, edge_index, eptr, dev, back = _placed(nodes_sampled, edge_index_sampled, edge_ptr, self.device)
        if dev != self.device:
            raise ValueError(f"the tensors are on {dev}, the vocabulary on {self.device}")
        _select_device(dev, jobs=True)
        digest, status = _hash_on_device(nodes, edge_index, eptr, iterations)
        out = self.lookup(digest, status)
        return out.cpu() if back else out
