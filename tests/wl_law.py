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


def bad_range(lo, hi, num_cols):
    """Law rule 4: [lo, hi) is no range of [0, num_cols]."""
    return lo < 0 or hi < lo or hi > num_cols


def wl_rows(nodes, edge_index, edge_ptr, iterations=3, num_cols=None):
    """The law over a sampler's three outputs (array-likes: nodes [S, k], edge_index [2, E], edge_ptr [S+1]).
    Returns (hexdigests: list of str or None, statuses: list of int, reports: list of (message lengths, final length)).
    Rule 4: a row whose edge_ptr range is no range of [0, num_cols] (default: the width of edge_index) has status 2 and no digest,
    and none of its entries is looked at; a row without vertices keeps status 1 (rule 3 comes first)."""
    num_cols = len(edge_index[0]) if num_cols is None else int(num_cols)
    hexes, stats, reports = [], [], []
    for i in range(len(nodes)):
        lo, hi = int(edge_ptr[i]), int(edge_ptr[i + 1])
        if bad_range(lo, hi, num_cols):
            empty = not any(int(x) >= 0 for x in nodes[i])
            hx, st, lens, flen = None, STATUS_EMPTY if empty else STATUS_BAD_ENDPOINT, [], 0
        else:
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


# ---- the census of ugs_wl.hip's paths ("Paths pinned") ----
# Which paths of the three kernels an input reaches, computed from the law alone: hashlib, the texts the law hashes, and the launch
# geometry (256 threads, 8, 16 or 32 lanes per row, 64 lanes per wave).  tests/wl_paths.py chooses its inputs by it.

WL_BLOCK, WAVE = 256, 64
STREAMS = ("deg1", "lab1", "later", "final")       # vertex messages of iteration 1 in degree / label mode, later ones, the final string
STREAM_CLASSES = ("word_complete", "word_straddle", "block_straddle", "opens_block", "flush_nothing", "flush_stores",
                  "flush_opens_block", "finish_exact_1", "finish_exact_2", "finish_exact_3plus", "finish_one_word", "finish_partial_word")
_SHORT = "a message of iteration 1 in degree mode has at most 33 labels of at most 2 bytes: 66 bytes, never a second block"
_EIGHT = "every piece is 8 hex characters, so a piece starts and ends on a word"
IMPOSSIBLE = {
    "deg1.block_straddle": _SHORT, "deg1.opens_block": _SHORT, "deg1.flush_opens_block": _SHORT, "deg1.finish_exact_1": _SHORT,
    "deg1.finish_exact_2": _SHORT, "deg1.finish_exact_3plus": _SHORT,
    "lab1.word_complete": _EIGHT, "lab1.word_straddle": _EIGHT, "lab1.block_straddle": _EIGHT, "lab1.flush_stores": _EIGHT,
    "lab1.flush_opens_block": _EIGHT, "lab1.finish_partial_word": _EIGHT,
    "lab1.finish_exact_3plus": "at most 33 labels of 8 bytes (32 neighbours, a loop among them, and the vertex): 264 bytes < 384",
    "later.word_complete": _EIGHT, "later.word_straddle": _EIGHT, "later.block_straddle": _EIGHT, "later.flush_stores": _EIGHT,
    "later.flush_opens_block": _EIGHT, "later.finish_partial_word": _EIGHT,
    "later.finish_one_word": "the vertex's own label alone is 32 bytes",
    "final.finish_exact_1": "N >= 2 items of 39 or 40 bytes print as 41 N .. 42 N bytes: 123-126 for 3, 164-168 for 4, never 128",
    "final.finish_exact_2": "246-252 bytes for 6 items, 287-294 for 7, never 256 (the first exact multiple is 1152 = 9 blocks, 28 items)",
}
CLASSES = (
    # group
    "group_8", "group_16", "group_32", "k_8", "k_9", "k_16", "k_17", "k_32", "n_1", "n_lt_k", "n_eq_k", "last_group_of_wave",
    "rows_plus1_g32", "rows_plus1_g16", "rows_plus1_g8", "rows_fill_block", "row_empty",
    # edges
    "edges_none", "edges_second_trip", "edge_duplicate", "edge_reversed", "edge_loop", "endpoint_minus1", "endpoint_eq_n",
    "endpoint_ge_2_32", "ptr_lo_negative", "ptr_hi_lt_lo", "ptr_hi_gt_cols", "ptr_bad_row_empty", "status2_between_ok",
    # degree labels
    "deg_0", "deg_1digit", "deg_2digit", "deg_33", "loop_counts_twice", "string_order_differs",
    # label mode
    "label_0", "label_ffffffff", "label_top_bit", "label_leading_zero", "holes", "dup_ids", "id_eq_num_labels", "label_minus1",
    "label_2_32", "bad_endpoint_and_bad_id", "num_labels_0",
    # order, Counter items, final string, iterations
    "labels_all_equal", "labels_all_distinct", "labels_ties_and_distinct", "count_1", "count_2digit", "count_32",
    "final_0_items", "final_1_item", "final_many", "iter_0", "iter_1", "iter_8",
) + tuple("%s.%s" % (s, c) for s in STREAMS for c in STREAM_CLASSES)


def lanes_of(k):
    """Lanes per row: the kernel's group width."""
    return 8 if k <= 8 else 16 if k <= 16 else 32


def stream_classes(lengths):
    """The piece-stream classes of one message produced in pieces of the given byte lengths (1..8 each), then flushed and
    finished: how the pieces fall on the 8-byte words and 128-byte blocks of BLAKE2b."""
    out, pos = set(), 0
    for n in lengths:
        assert 1 <= n <= 8
        off, widx = pos % 8, pos // 8 % 16
        if off + n >= 8:                               # the piece completes a word, which is stored
            if off + n == 8 and n < 8:
                out.add("word_complete")
            if off + n > 8:
                out.add("block_straddle" if widx == 15 else "word_straddle")
            if widx == 0 and pos >= 128:               # word 0 of a new block: the block before is compressed first
                out.add("opens_block")
        pos += n
    if pos % 8 == 0:
        out.add("flush_nothing")
    else:
        out.add("flush_stores")
        if pos // 8 % 16 == 0 and pos >= 128:
            out.add("flush_opens_block")
    if pos and pos % 128 == 0:
        out.add("finish_exact_%s" % {1: "1", 2: "2"}.get(pos // 128, "3plus"))
    if pos and (pos - 1) % 128 < 8:
        out.add("finish_one_word")
    if pos % 8:
        out.add("finish_partial_word")
    return out


def final_pieces(items):
    """The final string in the pieces it is produced in: per item its opening, four quarters of the label, "', <count>)"; the tail."""
    out = []
    for j, (h, c) in enumerate(items):
        out += ["(('" if j == 0 else ", ('", h[:8], h[8:16], h[16:24], h[24:], "', %d)" % c]
    return out + ["()" if not items else ",)" if len(items) == 1 else ")"]


def wl_trace(n, masks, start, iterations):
    """What the law hashes on the way: (labels[t][u] for t = 0..iterations, messages as lists of pieces [t-1][u], items)."""
    nbrs = [[v for v in range(n) if masks[u] >> v & 1] for u in range(n)]
    labels, msgs, items = [list(start)], [], []
    for _ in range(iterations):
        cur = labels[-1]
        pieces = [[cur[u]] + sorted(cur[v] for v in nbrs[u]) for u in range(n)]
        msgs.append(pieces)
        labels.append([_h("".join(p)) for p in pieces])
        items.extend(sorted(Counter(labels[-1]).items()))
    return labels, msgs, items


def census(nodes, edge_index, edge_ptr, iterations, labels=None, num_labels=None):
    """The set of CLASSES the input reaches; `labels` (ints by vertex id, the first `num_labels` of them) selects label mode."""
    import wl_feature_law as FL                        # imports this module
    out = set()
    S, k = len(nodes), len(nodes[0])
    labeled = labels is not None
    ncols = len(edge_index[0])
    if labeled:
        labs = [int(x) for x in labels][:len(labels) if num_labels is None else num_labels]
        hexes, stats, _ = FL.wl_feature_rows(nodes, edge_index, edge_ptr, labs, iterations)
        if not labs:
            out.add("num_labels_0")
    else:
        hexes, stats, _ = wl_rows(nodes, edge_index, edge_ptr, iterations)
    W = lanes_of(k)
    per_block, per_wave = WL_BLOCK // W, WAVE // W
    out.add("group_%d" % W)
    if k in (8, 9, 16, 17, 32):
        out.add("k_%d" % k)
    if S > per_block and S % per_block == 1:
        out.add("rows_plus1_g%d" % W)
    if S and S % per_block == 0:
        out.add("rows_fill_block")
    if iterations in (0, 1, 8):
        out.add("iter_%d" % iterations)
    for i in range(S):
        row = [int(x) for x in nodes[i]]
        ids = [x for x in row if x >= 0]
        n, st = len(ids), stats[i]
        lo, hi = int(edge_ptr[i]), int(edge_ptr[i + 1])
        bad = bad_range(lo, hi, ncols)
        if st == STATUS_EMPTY:
            out.add("row_empty")
            if bad:
                out.add("ptr_bad_row_empty")
            continue
        src, dst = [], []
        if bad:
            out |= {name for name, holds in (("ptr_lo_negative", lo < 0), ("ptr_hi_lt_lo", hi < lo), ("ptr_hi_gt_cols", hi > ncols)) if holds}
        else:
            src, dst = [int(x) for x in edge_index[0][lo:hi]], [int(x) for x in edge_index[1][lo:hi]]
        ends = src + dst
        out |= {name for name, holds in (("endpoint_minus1", -1 in ends), ("endpoint_eq_n", n in ends),
                                         ("endpoint_ge_2_32", any(x >= 1 << 32 for x in ends))) if holds}
        if labeled:
            if any(x < 0 for x in row[:max(j for j, x in enumerate(row) if x >= 0)]):
                out.add("holes")
            if len(set(ids)) < n:
                out.add("dup_ids")
            vals = [labs[x] for x in ids if x < len(labs)]
            wrong = {name for name, holds in (("id_eq_num_labels", len(labs) in ids), ("label_minus1", -1 in vals),
                                              ("label_2_32", 1 << 32 in vals)) if holds}
            assert st in (STATUS_BAD_ENDPOINT, FL.STATUS_BAD_LABEL) or not wrong
            out |= wrong if st == FL.STATUS_BAD_LABEL else {"bad_endpoint_and_bad_id"} if wrong else set()
        if st == STATUS_BAD_ENDPOINT and 0 < i < S - 1 and stats[i - 1] == stats[i + 1] == STATUS_OK and (i - 1) // per_block == (i + 1) // per_block:
            out.add("status2_between_ok")
        if st != STATUS_OK:
            continue
        out.add("n_1" if n == 1 else "n_eq_k" if n == k else "n_lt_k")
        if n == k:
            out.add("n_eq_k")
        if i % per_block % per_wave == per_wave - 1:
            out.add("last_group_of_wave")
        pairs = list(zip(src, dst))
        out |= {name for name, holds in (("edges_none", not pairs), ("edges_second_trip", len(pairs) > W),
                                         ("edge_duplicate", len(set(pairs)) < len(pairs)),
                                         ("edge_reversed", any(a != b and (b, a) in pairs for a, b in pairs)),
                                         ("edge_loop", any(a == b for a, b in pairs))) if holds}
        _, masks, _ = row_masks(row, src, dst)
        if labeled:
            start = ["%08x" % labs[x] for x in ids]
            out |= {name for name, holds in (("label_0", 0 in vals), ("label_ffffffff", 0xffffffff in vals),
                                             ("label_top_bit", any(x >> 31 for x in vals)),
                                             ("label_leading_zero", any(0 < x < 1 << 28 for x in vals))) if holds}
        else:
            degs = [bin(masks[u]).count("1") + (masks[u] >> u & 1) for u in range(n)]
            start = [str(d) for d in degs]
            out |= {name for name, holds in (("deg_0", 0 in degs), ("deg_1digit", any(0 < d < 10 for d in degs)),
                                             ("deg_2digit", any(d >= 10 for d in degs)), ("deg_33", 33 in degs),
                                             ("loop_counts_twice", any(masks[u] >> u & 1 for u in range(n)))) if holds}
            if iterations and any(sorted(p[1:]) != sorted(p[1:], key=int) for p in wl_trace(n, masks, start, 1)[1][0]):
                out.add("string_order_differs")
        labs_t, msgs, items = wl_trace(n, masks, start, iterations)
        assert _h(final_text(items)) == hexes[i]
        for cur in labs_t:                             # every label set the kernel ranks
            if n >= 2:
                d = len(set(cur))
                out.add("labels_all_equal" if d == 1 else "labels_all_distinct" if d == n else "labels_ties_and_distinct")
        out |= {name for name, holds in (("count_1", any(c == 1 for _, c in items)), ("count_2digit", any(c >= 10 for _, c in items)),
                                         ("count_32", any(c == 32 for _, c in items))) if holds}
        out.add("final_0_items" if not items else "final_1_item" if len(items) == 1 else "final_many")
        for t, per_vertex in enumerate(msgs):
            stream = "later" if t else "lab1" if labeled else "deg1"
            for pieces in per_vertex:
                lengths = [len(p) for p in pieces] if t == 0 else [8] * (4 * len(pieces))
                out |= {"%s.%s" % (stream, c) for c in stream_classes(lengths)}
        pieces = final_pieces(items)
        assert "".join(pieces) == final_text(items)
        out |= {"final.%s" % c for c in stream_classes([len(p) for p in pieces])}
    assert out <= set(CLASSES), sorted(out - set(CLASSES))
    return out


LOOKUP_CLASSES = ("table_empty", "table_one", "table_pow2", "table_not_pow2", "hit_first", "hit_last", "miss_below", "miss_above",
                  "miss_between", "eqhi_hit_lower", "eqhi_hit_upper", "eqhi_miss_between", "hi_top_bit", "lo_top_bit",
                  "status_1_in_table", "status_2_in_table", "status_3_in_table")
M64 = (1 << 64) - 1


def lookup_census(keys, digests, statuses):
    """The set of LOOKUP_CLASSES reached by looking the rows' digests up in the table: keys and digests are 128-bit numbers
    (int(hexdigest, 16)), keys in any order; a row's digest counts whatever its status."""
    keys = sorted(keys)
    V, out = len(keys), set()
    out.add("table_empty" if V == 0 else "table_one" if V == 1 else "table_pow2" if V & (V - 1) == 0 else "table_not_pow2")
    for d, st in zip(digests, statuses):
        if st != STATUS_OK:
            if d in keys:
                out.add("status_%d_in_table" % st)
            continue
        same_hi = [x for x in keys if x >> 64 == d >> 64]
        if d in keys:
            out |= {name for name, holds in (("hit_first", d == keys[0]), ("hit_last", d == keys[-1]),
                                             ("eqhi_hit_lower", any(x > d for x in same_hi)),
                                             ("eqhi_hit_upper", any(x < d for x in same_hi))) if holds}
        elif V:
            out.add("miss_below" if d < keys[0] else "miss_above" if d > keys[-1] else "miss_between")
            if any(x < d for x in same_hi) and any(x > d for x in same_hi):
                out.add("eqhi_miss_between")
        # unsigned order: the digest's top bit is set and the table holds keys on both sides of the sign
        if d >> 127 and len({x >> 127 for x in keys}) == 2:
            out.add("hi_top_bit")
        if d >> 63 & 1 and len({x >> 63 & 1 for x in same_hi}) == 2:
            out.add("lo_top_bit")
    return out


MD5_CLASSES = ("len_0", "tail_0", "tail_1", "tail_2", "tail_3", "pad_same_block", "pad_extra_block", "mod64_55", "mod64_56",
               "mod64_63", "mod64_0", "read_words", "read_bytes", "both_reads_one_launch")


def md5_census(row_bytes, address_mods):
    """The set of MD5_CLASSES reached by one launch of ugs_wl_feature_labels over rows of `row_bytes` bytes whose addresses
    have the given residues mod 4."""
    out = {"tail_%d" % (row_bytes % 4), "pad_same_block" if row_bytes % 64 <= 55 else "pad_extra_block"}
    if row_bytes == 0:
        out.add("len_0")
    if row_bytes % 64 in (55, 56, 63, 0):
        out.add("mod64_%d" % (row_bytes % 64))
    mods = {a % 4 for a in address_mods}
    out |= {name for name, holds in (("read_words", 0 in mods), ("read_bytes", bool(mods - {0})),
                                     ("both_reads_one_launch", 0 in mods and len(mods) > 1)) if holds}
    return out
