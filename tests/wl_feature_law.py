"""The law of ugs_wl_hash_labeled and ugs_wl_feature_labels (include/ugs_mi355.h) in plain Python: the reference's compute_wl_hash
with node_features on the rows its extract_subgraph_from_batch cuts out (src/gps/gps/utils/wl_vocab.py:21-107), restated on
neighbour masks with hashlib.md5 and hashlib.blake2b.  A helper for the tests, not a test.  Nothing here imports networkx, torch or
the library; the pieces shared with the degree form come from wl_law.

Besides the digest it reports the length of every vertex message and of the final string, so that tests can pick the rows that
sit on a BLAKE2b block boundary."""
import hashlib
from collections import Counter

from wl_law import STATUS_BAD_ENDPOINT, STATUS_EMPTY, STATUS_OK, _h, bad_range, final_text, row_masks

STATUS_BAD_LABEL = 3


def label32(row_bytes):
    """The first four bytes of the MD5 of a feature row's bytes as a big-endian number."""
    return int(hashlib.md5(bytes(row_bytes)).hexdigest()[:8], 16)


def labels_of(x):
    """label32 of every row of a numpy array x [N, ...]: the bytes of a row are its elements in C order in x's own dtype."""
    return [label32(x[i].tobytes()) for i in range(x.shape[0])]


def wl_from_labels(n, masks, start, iterations=3):
    """(hexdigest, message lengths [iteration][vertex], length of the final string) of the graph on vertices 0..n-1 whose start
    labels are the strings `start`.  A loop makes a vertex its own neighbour and nothing else."""
    nbrs = [[v for v in range(n) if masks[u] >> v & 1] for u in range(n)]
    label = list(start)
    items, msg_lens = [], []
    for _ in range(iterations):
        msgs = [label[u] + "".join(sorted(label[v] for v in nbrs[u])) for u in range(n)]
        msg_lens.append([len(m) for m in msgs])
        label = [_h(m) for m in msgs]
        items.extend(sorted(Counter(label).items()))
    text = final_text(items)
    assert text == str(tuple(items))
    return _h(text), msg_lens, len(text)


def wl_feature_row(nodes_row, src, dst, labels, iterations=3):
    """(hexdigest or None, status, message lengths, final length) of one sampled row: vertex j is the row's j-th entry >= 0 and
    starts with "%08x" % labels[entry].  Status 1: no entry >= 0; 2: an endpoint outside [0, n); 3: an entry that is no index of
    `labels`, or a label outside [0, 2^32) -- in that order of precedence."""
    n, masks, status = row_masks(nodes_row, src, dst)
    if status != STATUS_OK:
        return None, status, [], 0
    ids = [int(v) for v in nodes_row if int(v) >= 0]
    if any(v >= len(labels) or not 0 <= int(labels[v]) < 1 << 32 for v in ids):
        return None, STATUS_BAD_LABEL, [], 0
    hx, lens, flen = wl_from_labels(n, masks, ["%08x" % int(labels[v]) for v in ids], iterations)
    return hx, STATUS_OK, lens, flen


def wl_feature_rows(nodes, edge_index, edge_ptr, labels, iterations=3, num_cols=None):
    """The law over a sampler's three outputs and the labels by vertex id (a list of ints, e.g. labels_of(x)).
    Returns (hexdigests: list of str or None, statuses: list of int, reports: list of (message lengths, final length)).
    Rule 4 of ugs_wl_hash as in wl_law.wl_rows: an edge_ptr range that is no range of [0, num_cols] gives status 2 whatever the
    row's ids and labels, status 1 where the row has no vertex."""
    num_cols = len(edge_index[0]) if num_cols is None else int(num_cols)
    hexes, stats, reports = [], [], []
    for i in range(len(nodes)):
        lo, hi = int(edge_ptr[i]), int(edge_ptr[i + 1])
        if bad_range(lo, hi, num_cols):
            empty = not any(int(x) >= 0 for x in nodes[i])
            hx, st, lens, flen = None, STATUS_EMPTY if empty else STATUS_BAD_ENDPOINT, [], 0
        else:
            hx, st, lens, flen = wl_feature_row(nodes[i], edge_index[0][lo:hi], edge_index[1][lo:hi], labels, iterations)
        hexes.append(hx)
        stats.append(st)
        reports.append((lens, flen))
    return hexes, stats, reports


__all__ = ["STATUS_OK", "STATUS_EMPTY", "STATUS_BAD_ENDPOINT", "STATUS_BAD_LABEL", "label32", "labels_of", "wl_from_labels", "wl_feature_row",
           "wl_feature_rows"]
