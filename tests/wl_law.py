"""The law of ugs_wl_hash (include/ugs_mi355.h) in plain Python: networkx 3.4.2's weisfeiler_lehman_graph_hash with the degree as
node attribute, as the reference calls it (src/gps/gps/utils/wl_vocab.py:21-67), restated on neighbour masks with hashlib.blake2b.
A helper for the tests, not a test.  Nothing here imports networkx, torch or the library.

Besides the digest it reports the length of every vertex message and of the final string, so that tests can pick the rows that
sit on a BLAKE2b block boundary."""
import hashlib
from collections import Counter

STATUS_OK, STATUS_EMPTY, STATUS_BAD_ENDPOINT = 0, 1, 2


def _h(s):
    return hashlib.blake2b(s.encode("ascii"), digest_size=16).hexdigest()


def row_masks(nodes_row, src, dst):
    """(n, masks, status) of one sample: n = entries >= 0 of the row, masks[u] = bit v set for every neighbour v of u (bit u itself
    for a self-loop).  Status 1: no valid vertex.  Status 2: an endpoint outside [0, n)."""
    n = sum(1 for x in nodes_row if int(x) >= 0)
    if n == 0:
        return 0, [], STATUS_EMPTY
    masks = [0] * n
    for a, b in zip(src, dst):
        a, b = int(a), int(b)
        if not (0 <= a < n and 0 <= b < n):
            return n, [], STATUS_BAD_ENDPOINT
        masks[a] |= 1 << b
        masks[b] |= 1 << a
    return n, masks, STATUS_OK


def final_text(items):
    """str(tuple(items)) for items = [(hexdigest, count), ...], written out: what Python prints, byte for byte."""
    if not items:
        return "()"
    body = ", ".join("('%s', %d)" % (h, c) for h, c in items)
    return "(" + body + (",)" if len(items) == 1 else ")")


def wl_from_masks(n, masks, iterations=3):
    """(hexdigest, message lengths [iteration][vertex], length of the final string) of the graph on vertices 0..n-1."""
    nbrs = [[v for v in range(n) if masks[u] >> v & 1] for u in range(n)]
    label = [str(len(nbrs[u]) + (masks[u] >> u & 1)) for u in range(n)]      # a loop counts 2 towards the degree
    items, msg_lens = [], []
    for _ in range(iterations):
        msgs = [label[u] + "".join(sorted(label[v] for v in nbrs[u])) for u in range(n)]
        msg_lens.append([len(m) for m in msgs])
        label = [_h(m) for m in msgs]
        items.extend(sorted(Counter(label).items()))
    text = final_text(items)
    assert text == str(tuple(items))
    return _h(text), msg_lens, len(text)


def wl_row(nodes_row, src, dst, iterations=3):
    """(hexdigest or None, status, message lengths, final length) of one sampled row with its edge entries."""
    n, masks, status = row_masks(nodes_row, src, dst)
    if status != STATUS_OK:
        return None, status, [], 0
    hx, lens, flen = wl_from_masks(n, masks, iterations)
    return hx, STATUS_OK, lens, flen


def wl_rows(nodes, edge_index, edge_ptr, iterations=3):
    """The law over a sampler's three outputs (array-likes: nodes [S, k], edge_index [2, E], edge_ptr [S+1]).
    Returns (hexdigests: list of str or None, statuses: list of int, reports: list of (message lengths, final length))."""
    hexes, stats, reports = [], [], []
    for i in range(len(nodes)):
        lo, hi = int(edge_ptr[i]), int(edge_ptr[i + 1])
        hx, st, lens, flen = wl_row(nodes[i], edge_index[0][lo:hi], edge_index[1][lo:hi], iterations)
        hexes.append(hx)
        stats.append(st)
        reports.append((lens, flen))
    return hexes, stats, reports


def digest_words(hx):
    """A hexdigest as the two int64 words of the library's digest tensor: bytes 0-7 and 8-15, big-endian, as signed bit patterns."""
    def signed(x):
        return x - (1 << 64) if x >= 1 << 63 else x
    return signed(int(hx[:16], 16)), signed(int(hx[16:], 16))


def ids_from(hexes, stats, vocab):
    """The ids of the reference's _compute_wl_ids (src/gps/gps/models/ss_gnn_wl.py:210-247): len(vocab) for unknown hashes and for
    rows without valid vertices; a row with a bad endpoint is unknown too (the reference's fallback string is in no hash vocabulary)."""
    return [vocab.get(h, len(vocab)) if st == STATUS_OK else len(vocab) for h, st in zip(hexes, stats)]
