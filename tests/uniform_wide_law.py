"""uniform_wide_law.py -- the law of tests/uniform_law.py for graphs of more than 64 vertices, and the wide key of the HIP product
(include/ugs_mi355.h, ugs_uniform_sample_batch_begin: "Representation").

Nothing of the law changes with the size of a graph: S_g is the connected k-subsets in lexicographic order of their ascending
tuples.  `sorted_tuples` enumerates them with uniform_law.esu_masks (Python ints: no 64-bit limit) and sorts the tuples;
`uniform_law.sample_batch(..., enumerate_fn=sorted_tuples)` is the sampler.  `tuple_key` is the product's sort key of a set.
`census` names the wide-form kernel paths of ugs_uniform.hip that a call reaches (WIDE_CLASSES), from these quantities alone;
tests/uniform_wide_paths.py chooses its inputs by it."""
import numpy as np

import uniform_law as U


def mask_tuple(mask):
    out = []
    while mask:
        low = mask & -mask
        out.append(low.bit_length() - 1)
        mask ^= low
    return tuple(out)


def sorted_tuples(adj, k):
    """S_g as a list of ascending tuples in lexicographic order, any number of vertices."""
    return sorted(mask_tuple(x) for x in U.esu_masks(adj, k))


def field_bits(n):
    """b: the bit length of n - 1"""
    return (n - 1).bit_length()


def tuple_key(t, n):
    """The ascending tuple packed big-endian in fields of b bits: ascending keys = lexicographic tuples (needs len(t) * b <= 64)."""
    b, k = field_bits(n), len(t)
    assert k * b <= 64 and all(0 <= v < n for v in t)
    key = 0
    for i, v in enumerate(t):
        key |= v << (b * (k - 1 - i))
    return key


def takes_wide_form(n, k, limit):
    """The rule of the header: 64 < n <= limit, 1 <= k <= 8, k b <= 64."""
    return 64 < n <= limit and 1 <= k <= 8 and k * field_bits(n) <= 64


def sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42):
    return U.sample_batch(edge_index, ptr, m_per_graph, k, mode, seed, enumerate_fn=sorted_tuples)


def batch(graphs, first=0):
    """Concatenates local edge_index arrays [(n, ei)] into a PyG batch starting at vertex `first`."""
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(np.asarray(ei, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols, axis=1) if cols else np.zeros((2, 0), np.int64)
    return np.ascontiguousarray(ei), np.array(ptr, np.int64)


# ---- which wide-form kernel path an input reaches (ugs_uniform.hip: uni_wadj, uni_wesu, uni_wrows / uni_wfill, uni_wenum_*,
#      uni_wpop_*), from the law's own quantities.  The search below is the law's (uniform_law.esu_masks: lowest vertex first), walked
#      once more to look at what the kernels split it by: words of 64 vertices (one per lane of a 16-lane group), 64 items per root,
#      a flush per lane.  Nothing here calls the library. ----
WIDE_LANES, ROOT_ITEMS, LANE_FLUSH, ITEM_FLUSH, WIDE_MAX_K, BUDGET, SMALL_SORT, ROW_BLOCK, POP_LANES = 16, 64, 4096 // 16, 4096, 8, 1 << 25, 8192, 256, 16
SCAN_STEPS = (1, 2, 4, 8)

WIDE_CLASSES = (
    # form and layout
    "wide_only", "mask_before_wide", "mask_after_wide", "wide_mask_wide", "empty_before_wide", "small_before_wide", "ptr0_nonzero",
    "W2", "W_np2", "W16", "n128", "n129", "n256", "n257", "n512", "n513", "n1024",
    # uni_wadj
    "adj_loop", "adj_duplicate", "adj_reversed", "adj_bit63", "adj_last_word", "adj_v1023",
    # uni_wesu: roots
    "deg0", "deg1", "deg64", "deg65", "deg_ge129", "root_bit63", "root_ext_later_word", "root_lower_in_word",
    # the r-th member of the slot loop
    "rth_above_lowest_lane", "rth_inside_word", "rth_bit63",
    # levels
    "k1", "k2", "k3", "k4", "k5", "k6", "k7", "k8", "key_bit63",
    # group_take and key_with
    "take_lane_above0", "ext_gains_below_taken", "key_insert_middle", "key_insert_after_root",
    # row_scan: the final level's members (last_*) and a root's higher neighbours (root_*); shrS: non-empty lanes on both sides of
    # lane S, and two non-empty lanes a < b with (b - a) & S: the pairs for which lane b's prefix needs the row_shr:S step
    "last_two_lanes", "last_shr1", "last_shr2", "last_shr4", "last_shr8", "root_two_lanes", "root_shr1", "root_shr2", "root_shr4", "root_shr8",
    # count pass and budget
    "lane_flush_remainder", "item_gt_4096", "enum_at_max_rows", "enum_over_max_rows", "graph_over_budget_alone",
    # sort
    "bucket_0", "bucket_1", "bucket_2", "bucket_np2", "small_and_large_buckets",
    # rows and fill
    "k1_set0", "rows_cross_256", "row_without_edges", "row_with_loop", "sample", "global", "nepos_ne_g", "per_graph_seeds",
    # population rows
    "pop_cols_0", "pop_cols_15", "pop_cols_16", "pop_cols_17", "pop_chunks_several", "pop_hit_lane15_then_lane0",
)


def words(x, W=WIDE_LANES):
    """The 64-bit words of a vertex set, word l = what lane l holds"""
    return [(x >> (64 * l)) & U.M64 for l in range(W)]


def scan_classes(prefix, pcs, hit):
    lanes = [l for l, c in enumerate(pcs) if c]
    hit(prefix + "_two_lanes", len(lanes) >= 2)
    for s in SCAN_STEPS:
        pairs = [(a, b) for i, a in enumerate(lanes) for b in lanes[i + 1:]]
        hit(f"{prefix}_shr{s}", any((b - a) & s for a, b in pairs) and any(a < s <= b for a, b in pairs))


def search_census(adj, n, k, hit):
    """Walks the search of one wide graph as uni_wesu splits it; returns {(root, slot): sets} and names the classes it meets."""
    full = (1 << n) - 1
    pc = lambda x: bin(x).count("1")                                  # noqa: E731
    items = {}
    state = {"cnt": None, "flushed": None}

    def key_classes(sub, w):
        above, D = sum(1 for u in sub if u > w), len(sub)
        hit("key_insert_middle", D >= 3 and 0 < above < D - 1)
        hit("key_insert_after_root", D >= 2 and above == D - 1)

    def last(sub, ext):
        pcs = [pc(x) for x in words(ext)]
        scan_classes("last", pcs, hit)
        if len(sub) >= 2 and ext and max(sub) > (ext & -ext).bit_length() - 1:   # a member that key_with does not append
            e = ext
            while e:
                w = (e & -e).bit_length() - 1
                e &= e - 1
                if w > max(sub):
                    break
                key_classes(sub, w)
        cnt, flushed = state["cnt"], state["flushed"]
        for l, c in enumerate(pcs):
            cnt[l] += c
            if cnt[l] - flushed[l] >= LANE_FLUSH:
                flushed[l] = cnt[l]
        return sum(pcs)

    def level(sub, ext, nb, above):
        if len(sub) == k - 1:
            return last(sub, ext)
        total = 0
        while ext:
            w = (ext & -ext).bit_length() - 1
            hit("take_lane_above0", w >= 64 and sum(1 for x in words(ext) if x) >= 2)
            ext &= ext - 1
            new = adj[w] & ~nb & above
            hit("ext_gains_below_taken", new & ((1 << w) - 1) != 0)
            key_classes(sub, w)
            total += level(sub + [w], ext | new, nb | adj[w], above)
        return total

    for v in range(n):
        above = full & ~((2 << v) - 1)
        ext1, nb1, vw = adj[v] & above, adj[v] | (1 << v), v >> 6
        deg = pc(ext1)
        if k == 1:
            items[(v, 0)] = 1
            continue
        hit("root_bit63", v & 63 == 63 and deg > 0)
        hit("root_ext_later_word", deg > 0 and all(x == 0 for x in words(ext1)[:vw + 1]))
        hit("root_lower_in_word", deg > 0 and words(adj[v])[vw] & ((1 << (v & 63)) - 1) != 0)
        scan_classes("root", [pc(x) for x in words(ext1)], hit)
        if k == 2:
            state["cnt"], state["flushed"] = [0] * WIDE_LANES, [0] * WIDE_LANES
            c = last([v], ext1)
            if c:
                items[(v, 0)] = c
            continue
        for name, cond in (("deg0", deg == 0), ("deg1", deg == 1), ("deg64", deg == 64), ("deg65", deg == 65), ("deg_ge129", deg >= 129)):
            hit(name, cond)
        members = mask_tuple(ext1)
        lowest_lane = members[0] >> 6 if members else 0
        for slot in range(min(deg, ROOT_ITEMS)):
            state["cnt"], state["flushed"] = [0] * WIDE_LANES, [0] * WIDE_LANES
            total = 0
            for r in range(slot, deg, ROOT_ITEMS):
                w = members[r]
                hit("rth_above_lowest_lane", w >> 6 > lowest_lane)
                hit("rth_inside_word", r > 0 and members[r - 1] >> 6 == w >> 6)
                hit("rth_bit63", w & 63 == 63)
                later = ext1 & ~((2 << w) - 1)
                total += level([v, w], later | (adj[w] & ~nb1 & above), nb1 | adj[w], above)
            if total:
                items[(v, slot)] = total
            hit("item_gt_4096", total > ITEM_FLUSH)
            hit("lane_flush_remainder", any(f and c > f for c, f in zip(state["cnt"], state["flushed"])))
    return items


def census(ei, ptr, m, k, seeds_or_seed, per_graph, what="sample", mode=None, limit=1024, mask_vertices=64, max_rows=None, closed=None):
    """The set of WIDE_CLASSES a call reaches.  `what`: "sample" (sample_batch, or sample_graphs when per_graph), "enumerate" or
    "count"; `limit` / `mask_vertices`: the process-wide settings the call runs under; `max_rows`: enumerate's; `closed`: {graph:
    its number of sets} for graphs too large to walk (they are over the budget: nothing of them is searched here)."""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    src, dst = ei[0], ei[1]
    G, closed = len(ptr) - 1, dict(closed or {})
    out = set()
    hit = lambda name, cond=True: out.add(name) if cond else None    # noqa: E731
    sizes = np.diff(ptr).tolist()
    wanted = [k >= 1 and n >= k for n in sizes]
    fits = lambda n: 1 <= k <= WIDE_MAX_K and k * field_bits(n) <= 64   # noqa: E731
    form = [0 if not wanted[g] else 2 if (n > 64 and n <= limit and fits(n)) or (mask_vertices < n <= 64 and fits(n)) else 1 if n <= 64 else 0
            for g, n in enumerate(sizes)]
    wide = [g for g in range(G) if form[g] == 2]
    if not wide:
        return out
    budget = max_rows if what == "enumerate" else BUDGET
    # form and layout
    hit("wide_only", 1 not in form)
    hit("mask_before_wide", any(form[a] == 1 for a in range(wide[-1])))
    hit("mask_after_wide", any(form[a] == 1 for a in range(wide[0] + 1, G)))
    hit("wide_mask_wide", any(form[a] == 1 for a in range(wide[0], wide[-1])))
    hit("empty_before_wide", any(g > 0 and sizes[g - 1] == 0 for g in wide))
    hit("small_before_wide", any(g > 0 and 0 < sizes[g - 1] < k for g in wide))
    hit("ptr0_nonzero", int(ptr[0]) != 0)
    for g in wide:
        n, Wg = sizes[g], (sizes[g] + 63) >> 6
        hit("W2", Wg == 2)
        hit("W_np2", Wg & (Wg - 1) != 0)
        hit("W16", Wg == 16)
        for s in (128, 129, 256, 257, 512, 513, 1024):
            hit(f"n{s}", n == s)
    hit(f"k{k}")
    # columns of the wide graphs
    cols = {}
    for g in wide:
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        inside = (src >= lo) & (src < hi) & (dst >= lo) & (dst < hi)
        cu, cv = (src[inside] - lo).tolist(), (dst[inside] - lo).tolist()
        cols[g] = list(zip(cu, cv))
        pairs, Wg = set(cols[g]), (sizes[g] + 63) >> 6
        hit("adj_loop", any(u == v for u, v in pairs))
        hit("adj_duplicate", len(pairs) < len(cols[g]))
        hit("adj_reversed", any(u != v and (v, u) in pairs for u, v in pairs))
        hit("adj_bit63", any(u != v and (u & 63 == 63 or v & 63 == 63) for u, v in pairs))
        hit("adj_last_word", any(u != v and (u >> 6 == Wg - 1 or v >> 6 == Wg - 1) for u, v in pairs))
        hit("adj_v1023", any(u != v and 1023 in (u, v) for u, v in pairs))
    # search
    adjs = {g: U.graph_adjacency(src, dst, int(ptr[g]), sizes[g]) for g in wide if g not in closed}
    items = {g: search_census(adjs[g], sizes[g], k, hit) for g in adjs}
    gcount = {g: closed[g] if g in closed else sum(items[g].values()) for g in wide}
    for g in adjs:
        if k == 8 and field_bits(sizes[g]) == 8:
            hit("key_bit63", any(v >= 128 for v, _ in items[g]))
    over = [g for g in wide if gcount[g] > budget]
    hit("graph_over_budget_alone", bool(over) and per_graph and what == "sample")
    mask_total = 0
    if what == "enumerate":
        for g in range(G):
            if form[g] == 1:
                c = len(U.esu_masks(U.graph_adjacency(src, dst, int(ptr[g]), sizes[g]), k))
                mask_total += c if c <= budget else 0
        total = mask_total + sum(gcount[g] for g in wide if g not in over)
        hit("enum_at_max_rows", total == max_rows and len(wide) - len(over) >= 2)
        hit("enum_over_max_rows", total == max_rows + 1 and len(wide) - len(over) >= 2)
        if total > max_rows:
            return out
    if what == "count":
        return out
    # sort: one bucket per wide root
    buckets = []
    for g in adjs:
        if g in over:
            continue
        per_root = [0] * sizes[g]
        for (v, _), c in items[g].items():
            per_root[v] += c
        buckets += per_root
    for c in buckets:
        hit("bucket_0", c == 0)
        hit("bucket_1", c == 1)
        hit("bucket_2", c == 2)
        hit("bucket_np2", c >= 3 and c & (c - 1) != 0)
    hit("small_and_large_buckets", any(c > SMALL_SORT for c in buckets) and any(2 <= c <= SMALL_SORT for c in buckets))
    # rows of the wide graphs: (graph, row index in the call, tuple)
    sets = {g: sorted_tuples(adjs[g], k) for g in adjs if g not in over and gcount[g] > 0}
    rows = []
    if what == "enumerate":
        base = 0
        for g in range(G):
            if g in sets:
                rows += [(g, base + i, t) for i, t in enumerate(sets[g])]
                base += len(sets[g])
            elif form[g] == 1:
                c = len(U.esu_masks(U.graph_adjacency(src, dst, int(ptr[g]), sizes[g]), k))
                base += c if c <= budget else 0
    else:
        mask_sizes = {g: len(U.esu_masks(U.graph_adjacency(src, dst, int(ptr[g]), sizes[g]), k)) for g in range(G) if form[g] == 1}
        size_of = lambda g: len(sets[g]) if g in sets else mask_sizes.get(g, 0)   # noqa: E731
        nonempty = [g for g in range(G) if size_of(g) > 0]
        if per_graph:
            hit("per_graph_seeds", m > 0 and bool(sets))
            for g in sets:
                gen = U.mt19937_64(int(seeds_or_seed[g]) & U.M64)
                rows += [(g, g * m + s, sets[g][U.lemire(gen, len(sets[g]))]) for s in range(m)]
        else:
            hit("nepos_ne_g", m > 0 and any(nonempty.index(g) != g for g in sets))
            gen = U.mt19937_64(int(seeds_or_seed) & U.M64)
            for g in nonempty:
                for s in range(m):
                    d = U.lemire(gen, size_of(g))
                    if g in sets:
                        rows.append((g, g * m + s, sets[g][d]))
        # population rows: every sampling case is also drawn through PopulationCache
        for g in sets:
            nc = len(cols[g])
            if m > 0:
                for c in (0, 15, 16, 17):
                    hit(f"pop_cols_{c}", nc == c)
                hit("pop_chunks_several", nc > 2 * POP_LANES)
    hit("rows_cross_256", any(r >= ROW_BLOCK for _, r, _ in rows))
    if rows and mode is not None:
        hit("sample", mode == "sample")
        hit("global", mode != "sample")
    by_pair = {}
    for g in {g for g, _, _ in rows}:
        by_pair[g] = {}
        for q, uv in enumerate(cols[g]):
            by_pair[g].setdefault(uv, []).append(q)
    for g, t in {(g, t) for g, _, t in rows}:
        hits = {q for u in t for v in t for q in by_pair[g].get((u, v), ())}     # the bucket positions of the row's edges
        hit("k1_set0", t == (0,))
        hit("row_without_edges", not hits)
        hit("row_with_loop", any((u, u) in by_pair[g] for u in t))
        if what != "enumerate":
            hit("pop_hit_lane15_then_lane0", any(q % POP_LANES == POP_LANES - 1 and q + 1 in hits for q in hits))
    return out
