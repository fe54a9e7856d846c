"""The law of ugs_sampler.rows.unique_rows (include/ugs_mi355.h at ugs_rows_unique_begin) in plain numpy, with one dict of tuples
per graph, and the input generators its tests share.  No GPU and no library call here.

Below the generators: the kernels' constants restated (tests/test_rows_unique_paths_law.py compares them with the source text),
the refusals of the device check as the law has them (`refusal`), and `census`, which says from an input and the law's result
which paths of csrc/ugs_rows.hip the input reaches."""
import re

import numpy as np

MAX_ROWS_PER_GRAPH = 4096


def key_bits(k):
    return min(31, 128 // k)


def row_key(row, by):
    """The key of a row: its entries in order ("sequence") or sorted ascending ("set"); -1 is a value like any other."""
    t = tuple(int(v) for v in row)
    return t if by == "sequence" else tuple(sorted(t))


def check_limits(nodes, sample_ptr, ptr):
    """What the kernels refuse: the first offending graph or row, as the text of the refusal's name, or None."""
    R, k = nodes.shape
    b = key_bits(k)
    for g in range(len(sample_ptr) - 1):
        rows = int(sample_ptr[g + 1] - sample_ptr[g])
        if rows > 0 and rows > MAX_ROWS_PER_GRAPH:
            return f"graph {g}"
        if rows > 0 and int(ptr[g + 1] - ptr[g]) + 1 > (1 << b):
            return f"graph {g}"
    for g in range(len(sample_ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        for r in range(int(sample_ptr[g]), int(sample_ptr[g + 1])):
            for v in nodes[r]:
                if v != -1 and not lo <= v < hi:
                    return f"row {r}"
    return None


def unique_rows(nodes, edge_index, edge_ptr, sample_ptr, edge_src, ptr, by="set"):
    """The seven arrays of the law, int64: (nodes_u [U, k], edge_index_u [2, Eu], edge_ptr_u [U + 1], sample_ptr_u [G + 1],
    edge_src_u [Eu] (empty where edge_src is), count [U], inverse [R])."""
    assert by in ("set", "sequence")
    nodes = np.asarray(nodes, dtype=np.int64)
    edge_index = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    edge_ptr = np.asarray(edge_ptr, dtype=np.int64)
    sample_ptr = np.asarray(sample_ptr, dtype=np.int64)
    edge_src = np.asarray(edge_src, dtype=np.int64)
    R, k = nodes.shape
    G = len(sample_ptr) - 1
    assert check_limits(nodes, sample_ptr, ptr) is None
    kept, count, inverse = [], [], np.zeros(R, dtype=np.int64)
    sample_ptr_u = np.zeros(G + 1, dtype=np.int64)
    for g in range(G):
        seen = {}                                           # key -> position in the result
        for r in range(int(sample_ptr[g]), int(sample_ptr[g + 1])):
            key = row_key(nodes[r], by)
            if key not in seen:
                seen[key] = len(kept)
                kept.append(r)
                count.append(0)
            count[seen[key]] += 1
            inverse[r] = seen[key]
        sample_ptr_u[g + 1] = len(kept)
    U = len(kept)
    nodes_u = nodes[kept].reshape(U, k) if U else np.zeros((0, k), dtype=np.int64)
    spans = [np.arange(int(edge_ptr[r]), int(edge_ptr[r + 1])) for r in kept]
    cols = np.concatenate(spans).astype(np.int64) if spans else np.zeros(0, dtype=np.int64)
    edge_ptr_u = np.zeros(U + 1, dtype=np.int64)
    if U:
        edge_ptr_u[1:] = np.cumsum([len(s) for s in spans])
    edge_index_u = edge_index[:, cols]
    edge_src_u = edge_src[cols] if edge_src.size else np.zeros(0, dtype=np.int64)
    return (np.ascontiguousarray(nodes_u), np.ascontiguousarray(edge_index_u), edge_ptr_u, sample_ptr_u, np.ascontiguousarray(edge_src_u),
            np.asarray(count, dtype=np.int64), inverse)


# ---- generators ----
def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def with_edges(nodes, rng, max_edges=4, edge_src=True):
    """edge_index, edge_ptr and edge_src for rows `nodes`: every row gets 0..max_edges entries with values that tell its row and
    position, so that a span copied to the wrong place, or from the wrong row, shows."""
    R = nodes.shape[0]
    lens = rng.integers(0, max_edges + 1, size=R) if R else np.zeros(0, dtype=np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Es = int(edge_ptr[-1])
    row_of = np.repeat(np.arange(R), lens).astype(np.int64)
    pos = np.arange(Es, dtype=np.int64) - edge_ptr[row_of] if Es else np.zeros(0, dtype=np.int64)
    edge_index = np.stack([row_of * 1000 + pos, -(row_of * 1000 + pos) - 7]).astype(np.int64).reshape(2, Es)
    src = (row_of * 31 + pos * 3 + 5).astype(np.int64) if edge_src else np.zeros(0, dtype=np.int64)
    return edge_index, edge_ptr, src


def random_case(rng, rows_per_graph, k, graph_sizes=None, distinct=6, minus_one=0.1, max_edges=4, edge_src=True):
    """A batch with rows_per_graph[g] rows in graph g, drawn from `distinct` base rows per graph and permuted at random, so that
    rows repeat as sets and, less often, as sequences; some entries are -1 and some rows are all -1."""
    G = len(rows_per_graph)
    sizes = list(graph_sizes) if graph_sizes is not None else [int(rng.integers(max(k, 2), 3 * k + 2)) for _ in range(G)]
    b = key_bits(k)
    sizes = [min(n, (1 << b) - 1) for n in sizes]
    ptr = ptr_of(sizes)
    rows = []
    for g, cnt in enumerate(rows_per_graph):
        n = sizes[g]
        base = rng.integers(0, n, size=(max(distinct, 1), k)) + ptr[g]
        base[rng.random(base.shape) < minus_one] = -1
        if distinct > 1:
            base[0, :] = -1
        for _ in range(cnt):
            row = base[int(rng.integers(0, base.shape[0]))].copy()
            if rng.random() < 0.6:
                rng.shuffle(row)
            rows.append(row)
    nodes = np.array(rows, dtype=np.int64).reshape(len(rows), k)
    sample_ptr = ptr_of(rows_per_graph)
    edge_index, edge_ptr, src = with_edges(nodes, rng, max_edges, edge_src)
    return nodes, edge_index, edge_ptr, sample_ptr, src, ptr


def kept_fraction(nodes, sample_ptr, by):
    total = 0
    for g in range(len(sample_ptr) - 1):
        total += len({row_key(nodes[r], by) for r in range(int(sample_ptr[g]), int(sample_ptr[g + 1]))})
    return total / max(nodes.shape[0], 1)


# ---- the kernels' constants (csrc/ugs_rows.hip, csrc/ugs_device.h), restated once ----
WAVE_ROWS = 64                      # a graph of at most this many rows is the wave form's
CLASS_BOUNDS = (256, 1024, 4096)    # the workgroup form's three classes: pairs in LDS, four rows a thread
GRAPHS_PER_GROUP = 4                # wave form: graphs a workgroup
SCAN_PASS = 1024                    # graphs per pass of the scan across graphs
EDGE_LANES = 16                     # lanes a kept row in the edge copy, and entries a trip
CHECK_BLOCK, CHECK_GRID = 256, 4096
CHECK_TRIP = CHECK_BLOCK * CHECK_GRID   # 2^20 indices per trip of the check
KEY_WORD = 32                       # the key is compared as four words of this many bits
ALL_K = tuple(range(1, 33))
ALL_BITS = tuple(sorted({key_bits(k) for k in ALL_K}, reverse=True))
SPANS = (0, 1, 15, 16, 17, 33)      # edge spans of kept rows that have a class: around one and two trips of 16
# one k for every b that has a field across bit 64, and the k whose fields end at bit 64
STRADDLE_K = (3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 17, 19, 22)
FIELD_AT_64_K = (8, 16, 32)

# classes that no input reaches, with the reason; census still names them should they ever appear
UNREACHABLE = {
    "block_second_grid_trip": "rows_block strides its class's list by gridDim.x, but the host sizes the grid of the class above L rows as "
                              "min(G, R // (L + 1)), and at most that many graphs have more than L rows: the list is never longer than the grid",
    "key_over_128_bits": "b = min(31, 128 // k), so k * b <= 128 for every k: or_shl never shifts a field past bit 127",
}


def _as_case(case):
    nodes, ei, eptr, sptr, esrc, ptr = case
    return (np.asarray(nodes, dtype=np.int64), np.asarray(ei, dtype=np.int64).reshape(2, -1), np.asarray(eptr, dtype=np.int64),
            np.asarray(sptr, dtype=np.int64), np.asarray(esrc, dtype=np.int64), np.asarray(ptr, dtype=np.int64))


def offences(case):
    """Everything the device check and the key kernel refuse in `case`, as three sorted lists of (status value, class name): the
    pointer arrays' word (4 * index + 0 sample_ptr, 1 edge_ptr, 2 ptr), the graphs' word (2 * graph + 0 rows, 1 vertices) and the
    entries' word (the row).  Entries are looked at only where the pointer arrays stand, as a row has no graph otherwise."""
    nodes, ei, eptr, sptr, esrc, ptr = _as_case(case)
    R, k = nodes.shape
    G, Es, b = len(sptr) - 1, ei.shape[1], key_bits(k)
    po = []
    if sptr[0] != 0:
        po.append((0, "sample_ptr0"))
    if sptr[G] != R:
        po.append((4 * G, "sample_end"))
    if eptr[0] != 0:
        po.append((1, "edge_ptr0"))
    if eptr[R] != Es:
        po.append((4 * R + 1, "edge_end"))
    po += [(4 * int(i) + 1, "edge_decreases") for i in np.nonzero(eptr[:-1] > eptr[1:])[0]]
    po += [(4 * int(i), "sample_decreases") for i in np.nonzero(sptr[:-1] > sptr[1:])[0]]
    po += [(4 * int(i) + 2, "ptr_decreases") for i in np.nonzero(ptr[:-1] > ptr[1:])[0]]
    rows, verts = np.diff(sptr), np.diff(ptr)
    over = (rows > 0) & (rows > MAX_ROWS_PER_GRAPH)
    overv = (rows > 0) & ~over & (verts + 1 > (1 << b))
    go = [(2 * int(g), "rows_over") for g in np.nonzero(over)[0]] + [(2 * int(g) + 1, "vertices_over@%d" % b) for g in np.nonzero(overv)[0]]
    eo = []
    if not po and R > 0:
        g_of = np.repeat(np.arange(G), rows)
        lo, hi = ptr[g_of][:, None], ptr[g_of + 1][:, None]
        for name, hit in (("entry_minus_two", nodes == -2), ("entry_below_graph", (nodes >= 0) & (nodes < lo)), ("entry_at_hi", nodes == hi),
                          ("entry_2p32_above", ((nodes < lo) | (nodes >= hi)) & (nodes >= 0) & (((nodes - lo) & 0xffffffff) < hi - lo)),
                          ("entry_outside", (nodes != -1) & ((nodes < lo) | (nodes >= hi)))):
            eo += [(int(r), name) for r in np.nonzero(hit.any(axis=1))[0]]
    return sorted(po), sorted(go), sorted(eo)


def refusal(case):
    """None, or (word, status value) of the refusal: pointer arrays before graphs before entries, the lowest value of the word."""
    po, go, eo = offences(case)
    for word, found in (("ptr", po), ("graph", go), ("entry", eo)):
        if found:
            return word, found[0][0]
    return None


def refusal_pattern(word, value, k):
    """The message of a refusal as a regular expression (csrc/ugs_rows.cpp, rows_refusal)."""
    if word == "ptr":
        name, what = (("sample_ptr", "rows"), ("edge_ptr", "edge entries"), ("ptr", "vertices"))[value & 3]
        return r"unique_rows: %s must start at 0, must not decrease and must end at the number of %s \(index %d\)" % (name, what, value >> 2)
    if word == "graph":
        if value & 1 == 0:
            return "unique_rows: graph %d has more than %d rows" % (value >> 1, MAX_ROWS_PER_GRAPH)
        return "unique_rows: graph %d has more than %d vertices, the most a %d-bit key field holds" % (value >> 1, (1 << key_bits(k)) - 1, key_bits(k))
    return "unique_rows: row %d has an entry below -1 or outside its graph" % value


def form_of(sample_ptr):
    """What rows.last_launch() reports after a call that was not refused."""
    rows = np.diff(np.asarray(sample_ptr, dtype=np.int64))
    small, big = bool(((rows >= 1) & (rows <= WAVE_ROWS)).any()), bool((rows > WAVE_ROWS).any())
    return "wave+workgroup" if small and big else "workgroup" if big else "wave" if small else "none"


def row_fields(row, lo, by):
    """The k codes of a row in key order, lowest field first: v - lo + 1, 0 for -1; sorted ascending for "set"."""
    codes = [0 if v == -1 else int(v) - int(lo) + 1 for v in row]
    return tuple(sorted(codes)) if by == "set" else tuple(codes)


def key_of(fields, b):
    """The 128-bit key as one integer: field i at bit i * b."""
    key = 0
    for i, c in enumerate(fields):
        key |= c << (i * b)
    return key


def _two_differ_only_in(fields, pick):
    """Do two of the rows `fields` agree in everything but pick(field tuple) -> (rest, part)?"""
    seen = {}
    for f in fields:
        rest, part = pick(f)
        seen.setdefault(rest, set()).add(part)
    return any(len(v) > 1 for v in seen.values())


def census(case, by, strided=False):
    """The set of class names `case` reaches in csrc/ugs_rows.hip, from the input and the law's result alone.  A refused input
    reaches the classes of its offences and nothing behind the check.  `strided`: the caller hands edge_index over as a view whose
    columns are not adjacent (the arrays cannot say so)."""
    case = _as_case(case)
    nodes, ei, eptr, sptr, esrc, ptr = case
    R, k = nodes.shape
    G, b = len(sptr) - 1, key_bits(k)
    out = set()
    if max(R, G) + 1 > CHECK_TRIP:
        out.add("second_trip")
    if k * b > 128:
        out.add("key_over_128_bits")
    po, go, eo = offences(case)
    if po or go or eo:
        out |= {name for _, name in po + go + eo if name != "entry_outside"}
        first = po or go or eo
        if len({v for v, _ in first}) > 1:
            out.add("two_offences_lower_index_wins@" + ("ptr" if po else "graph" if go else "entry"))
        if first[0][0] >> (2 if po else 1 if go else 0) >= CHECK_TRIP:
            out.add("offence_past_first_trip")
        if po and go:
            out.add("ptr_beats_graph")
        if not po and go and eo:
            out.add("graph_beats_entry")
        return out
    rows = np.diff(sptr)
    small, big = (rows >= 1) & (rows <= WAVE_ROWS), rows > WAVE_ROWS
    cls = np.where(rows <= CLASS_BOUNDS[0], 0, np.where(rows <= CLASS_BOUNDS[1], 1, 2))
    if (big & (np.arange(G) >= CHECK_TRIP)).any():
        out.add("big_past_first_trip")
    for c in range(3):
        many = int((big & (cls == c)).sum())
        if many:
            out.add("class%d" % c)
        if many > 1:
            out.add("two_graphs_one_class")
        if many > min(G, R // (((WAVE_ROWS,) + CLASS_BOUNDS)[c] + 1)):          # the class's grid, as the host sizes it
            out.add("block_second_grid_trip")
    if R > 0:
        out.add("no_small" if not small.any() else "no_big" if not big.any() else "small_and_big")
        out.add("unrolled_k%d" % k if k <= 8 else "looped")
    if 1 <= G <= SCAN_PASS:
        out.add("one_pass")
    if G == SCAN_PASS:
        out.add("exactly_1024")
    if G == SCAN_PASS + 1:
        out.add("1025")
    if G > 2 * SCAN_PASS:
        out.add("many_passes")
    if R < G:
        out.add("rows_fewer_than_graphs")
    if strided:
        out.add("strided_edge_index")
    res = unique_rows(nodes, ei, eptr, sptr, esrc, ptr, by)
    inverse = res[6]
    kept_rows = np.unique(inverse, return_index=True)[1] if R else np.zeros(0, dtype=np.int64)
    rep = kept_rows[inverse] if R else inverse
    spans = set((eptr[kept_rows + 1] - eptr[kept_rows]).tolist())
    out |= {"span_%d" % s for s in SPANS if s in spans}
    if esrc.size == 0 and res[1].shape[1] > 0:
        out.add("no_edge_src")
    with_rows = np.nonzero(rows > 0)[0]
    if G and len(with_rows) and rows[0] == 0 and rows[G - 1] == 0:
        before = any(g >= 2 and rows[g - 1] == 0 and rows[g - 2] == 0 for g in with_rows)
        behind = any(g <= G - 3 and rows[g + 1] == 0 and rows[g + 2] == 0 for g in with_rows)
        if before and behind:
            out.add("graph_behind_empty_graphs")
    f64 = 64 // b                                      # the field that holds bit 64
    low = 64 - f64 * b                                  # how many of its bits lie below bit 64; 0: it starts there
    for g in with_rows:
        g = int(g)
        r0, n, lo, nv = int(sptr[g]), int(rows[g]), int(ptr[g]), int(ptr[g + 1] - ptr[g])
        block = nodes[r0:r0 + n]
        fields = [row_fields(row, lo, by) for row in block]
        keys = [key_of(f, b) for f in fields]
        top = (1 << b) - 1
        if nv == top and (block == lo + nv - 1).any():
            out.add("top_code@%d" % b)
        if k * b == 128 and any(f[k - 1] == top for f in fields):
            out.add("bit_127")
        if by == "set":
            if any(len(set(f)) < k and len(set(f)) > 1 for f in fields):
                out.add("set_ties")
            if k > 1 and any(len(set(f)) == 1 and f[0] != 0 for f in fields):
                out.add("set_all_equal")
        if f64 < k and low:
            if _two_differ_only_in(fields, lambda f: ((f[:f64], f[f64] & ((1 << low) - 1), f[f64 + 1:]), f[f64] >> low)):
                out.add("straddle_hi_only@%d" % k)
            if _two_differ_only_in(fields, lambda f: ((f[:f64], f[f64] >> low, f[f64 + 1:]), f[f64] & ((1 << low) - 1))):
                out.add("straddle_lo_only@%d" % k)
        if f64 < k and not low:
            if (_two_differ_only_in(fields, lambda f: ((f[:f64], f[f64 + 1:]), f[f64]))
                    and _two_differ_only_in(fields, lambda f: ((f[:f64 - 1], f[f64:]), f[f64 - 1]))):
                out.add("field_at_64@%d" % k)
        distinct = len(set(keys))
        rep_g = rep[r0:r0 + n] - r0
        if n <= WAVE_ROWS:
            out.add("slot%d" % (g % GRAPHS_PER_GROUP))
            if n in (1, 2, 63, 64):
                out.add("rows_%d" % n)
            if G % GRAPHS_PER_GROUP and g >= G - G % GRAPHS_PER_GROUP:
                out.add("partial_group")
            if n > 1 and distinct == 1:
                out.add("all_equal")
            if n > 1 and distinct == n:
                out.add("all_distinct")
            if any(0 < p < l for l, p in enumerate(rep_g)):
                out.add("rep_not_first_lane")
            if n == 64 and rep_g[63] == 63 and eptr[r0 + 64] > eptr[r0 + 63]:
                out.add("lane63_kept_with_edges")
            continue
        pn = 128
        while pn < n:
            pn *= 2
        if n == pn:
            out.add("pn%d_full" % pn)
        if n == pn // 2 + 1:
            out.add("pn%d_half_plus_1" % pn)
        if n == 4095:
            out.add("n4095")
        if n < pn and k * b == 128 and keys.count((1 << 128) - 1) > 1:
            out.add("pad_meets_all_ones_key@%d" % k)
        order = sorted(set(keys))
        if distinct == 1:
            out.add("run_all")
        else:
            if keys.count(order[0]) > 1:
                out.add("run_first")
            if keys.count(order[-1]) > 1:
                out.add("run_last")
        if any(p // 4 != l // 4 for l, p in enumerate(rep_g)):
            out.add("run_across_threads")
        if n > 256 and any(p == l and l >= 256 for l, p in enumerate(rep_g)):
            out.add("kept_in_later_wave")
        for w, name in enumerate("xyzw"):
            mask = ((1 << KEY_WORD) - 1) << (KEY_WORD * w)
            if _two_differ_only_in(keys, lambda key: (key & ~mask, key & mask)):
                out.add("word_%s_only" % name)
    return out


def constants_in_source(hip, dev):
    """Are the constants above the ones in the text of ugs_rows.hip and ugs_device.h?  A list of what is not."""
    want = [
        (dev, r"#define UGS_ROWS_MAX_PER_GRAPH %d\b" % MAX_ROWS_PER_GRAPH),
        (hip, r"else if \(rows > %d\) \{" % WAVE_ROWS), (hip, r"if \(n > %d\) return;" % WAVE_ROWS), (hip, r"if \(n <= %d \|\| n > P\) continue;" % WAVE_ROWS),
        (hip, r"const int cls = rows <= %d \? 0 : rows <= %d \? 1 : 2;" % CLASS_BOUNDS[:2]),
        (hip, r"rows_block<%d>.*dim3\(%d\).*c, 0\);" % (CLASS_BOUNDS[0], CLASS_BOUNDS[0] // 4)),
        (hip, r"rows_block<%d>.*dim3\(%d\).*c, 1\);" % (CLASS_BOUNDS[1], CLASS_BOUNDS[1] // 4)),
        (hip, r"rows_block<%d>.*dim3\(%d\).*c, 2\);" % (CLASS_BOUNDS[2], CLASS_BOUNDS[2] // 4)),
        (hip, r"c\.R / %d\), g1 = .*c\.R / %d\), g2 = .*c\.R / %d\);" % (WAVE_ROWS + 1, CLASS_BOUNDS[0] + 1, CLASS_BOUNDS[1] + 1)),
        (hip, r"int pn = 128;"), (hip, r"constexpr int NT = P / 4;"),
        (hip, r"const int64_t g = \(int64_t\)blockIdx\.x \* %d \+ \(threadIdx\.x >> 6\);" % GRAPHS_PER_GROUP),
        (hip, r"dim3\(\(unsigned\)\(\(c\.G \+ %d\) / %d\)\), dim3\(256\), 0, s, c\);" % (GRAPHS_PER_GROUP - 1, GRAPHS_PER_GROUP)),
        (hip, r"for \(int64_t base = 0; base < c\.G; base \+= %d\)" % SCAN_PASS), (hip, r"block_scan2\(u, e, %d, wt" % SCAN_PASS),
        (hip, r"\* 256 \+ threadIdx\.x\) >> 4;"), (hip, r"const int lane = threadIdx\.x & %d;" % (EDGE_LANES - 1)),
        (hip, r"for \(int64_t e = lane; e < len; e \+= %d\)" % EDGE_LANES), (hip, r"\(c\.R \* %d \+ 255\) / 256" % EDGE_LANES),
        (hip, r"i \+= \(int64_t\)gridDim\.x \* %d\)" % CHECK_BLOCK), (hip, r"\(top \+ 255\) / 256, %d\)\), dim3\(%d\)" % (CHECK_GRID, CHECK_BLOCK)),
        (hip, r"make_uint4\(\(u32\)klo, \(u32\)\(klo >> %d\), \(u32\)khi, \(u32\)\(khi >> %d\)\)" % (KEY_WORD, KEY_WORD)),
        (hip, r"default: launch_keys<0>"), (hip, r"case 8: launch_keys<8>"),
    ]
    return [pattern for text, pattern in want if not re.search(pattern, text)]
