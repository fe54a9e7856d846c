"""uniform_law.py -- CPU restatement of the reference's `uniform_sampler.sample_batch` (AniruddhaMandal/SS-GNN
src/samplers/uniform_sampler/src/uniform_sampler.cpp:86-285), for the tests.

The law (include/ugs_mi355.h, ugs_uniform_sample_batch_begin, states it in full):
  * per graph g, the columns with both endpoints in [ptr[g], ptr[g+1]) form its adjacency (:121-136);
  * S_g = every k-subset of g's local vertices whose induced subgraph is connected, in lexicographic order of the ascending
    vertex tuples (the combination DFS, :47-80);
  * one std::mt19937_64(seed) for the call (:144); per graph with S_g non-empty, m draws
    std::uniform_int_distribution<int>(0, |S_g|-1) (:189), i.e. libstdc++'s Lemire step with a 128-bit product;
    graphs with S_g empty draw nothing and give m rows of -1;
  * a row's edges: every batch column, in column order, with both endpoints in the graph's range and in the subset;
    mode "sample" numbers them by position in the row, any other mode keeps batch ids (:193-236).

Pure Python + numpy: `mt19937_64`, `lemire`, two enumerations (`connected_subsets_comb`, the literal definition, and
`connected_subsets_esu` / `sorted_masks`, extension-set search + sort, fast enough for 64-vertex graphs with ~1e5 subsets) and
`sample_batch`, the output assembly.  `census` names the kernel paths of ugs_uniform.hip that a call reaches (CLASSES), from these
quantities alone; tests/uniform_paths.py chooses its inputs by it.
"""
import itertools

import numpy as np

M64 = (1 << 64) - 1


class mt19937_64:
    """std::mt19937_64 (C++ [rand.predef]: the 10000th output for the default seed 5489 is 9981545732273789042)."""
    N, M = 312, 156
    A = 0xB5026F5AA96619E9
    UM, LM = 0xFFFFFFFF80000000, 0x7FFFFFFF

    def __init__(self, seed=5489):
        mt = [seed & M64]
        for i in range(1, self.N):
            mt.append((6364136223846793005 * (mt[-1] ^ (mt[-1] >> 62)) + i) & M64)
        self.mt, self.i = mt, self.N

    def _twist(self):
        mt, N, M = self.mt, self.N, self.M
        for i in range(N):
            y = (mt[i] & self.UM) | (mt[(i + 1) % N] & self.LM)
            mt[i] = mt[(i + M) % N] ^ (y >> 1) ^ (self.A if y & 1 else 0)
        self.i = 0

    def __call__(self):
        if self.i >= self.N:
            self._twist()
        y = self.mt[self.i]
        self.i += 1
        y ^= (y >> 29) & 0x5555555555555555
        y ^= (y << 17) & 0x71D67FFFEDA60000
        y ^= (y << 37) & 0xFFF7EEE000000000
        y ^= y >> 43
        return y & M64


def lemire(gen, n):
    """std::uniform_int_distribution<int>(0, n-1)(gen) for a 64-bit generator, libstdc++ 11
    (bits/uniform_int_dist.h:246-268, 302-307): p = x*n; if lo64(p) < n: t = (2^64 - n) mod n, redraw while lo64(p) < t."""
    p = gen() * n
    if (p & M64) < n:
        t = ((1 << 64) - n) % n
        while (p & M64) < t:
            p = gen() * n
    return p >> 64


def graph_adjacency(src, dst, lo, n):
    """Neighbour bitmasks (Python ints) of the graph [lo, lo+n): columns with both endpoints inside, symmetrised."""
    adj = [0] * n
    inside = (src >= lo) & (src < lo + n) & (dst >= lo) & (dst < lo + n)
    for u, v in zip((src[inside] - lo).tolist(), (dst[inside] - lo).tolist()):
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    return adj


def _connected(sub, adj):
    seen, todo = 1 << sub[0], [sub[0]]
    want = 0
    for v in sub:
        want |= 1 << v
    while todo:
        u = todo.pop()
        new = adj[u] & want & ~seen
        seen |= new
        while new:
            w = (new & -new).bit_length() - 1
            new &= new - 1
            todo.append(w)
    return seen == want


def connected_subsets_comb(adj, k):
    """The reference's definition, literally: every k-combination in lexicographic order, kept if connected."""
    n = len(adj)
    if k <= 0:
        return []
    return [c for c in itertools.combinations(range(n), k) if _connected(c, adj)]


def esu_masks(adj, k):
    """Every connected k-subset as a bitmask, each once, by extension-set search rooted at its minimum vertex
    (Wernicke 2006): grow sub by w from the extension set; the new extension set adds w's neighbours above the root that
    are neither in nor adjacent to the current set."""
    n = len(adj)
    out = []
    if k <= 0 or k > n:
        return out
    for v in range(n):
        above = ((1 << n) - 1) & ~((2 << v) - 1)
        if k == 1:
            out.append(1 << v)
            continue
        stack = [(1 << v, adj[v] & above, adj[v] | (1 << v))]
        while stack:
            sub, ext, nb = stack.pop()
            size = bin(sub).count("1")
            while ext:
                w = (ext & -ext).bit_length() - 1
                ext &= ext - 1
                if size + 1 == k:
                    out.append(sub | (1 << w))
                else:
                    stack.append((sub | (1 << w), ext | (adj[w] & ~nb & above), nb | adj[w]))
    return out


def _brev64(a):
    """Bit reversal of a uint64 array."""
    a = a.astype(np.uint64)
    for sh, mk in ((1, 0x5555555555555555), (2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF),
                   (16, 0x0000FFFF0000FFFF), (32, 0x00000000FFFFFFFF)):
        s, m = np.uint64(sh), np.uint64(mk)
        a = ((a >> s) & m) | ((a & m) << s)
    return a


def sorted_masks(adj, k):
    """S_g as a uint64 mask array in lexicographic order of the ascending tuples.  For sets of one size that order is the
    DESCENDING order of the bit-reversed mask: the first vertex where two sets differ is the highest bit of the reversed
    masks where they differ, and the set holding it comes first."""
    if len(adj) > 64:
        raise ValueError("masks hold at most 64 vertices")
    masks = np.array(esu_masks(adj, k), dtype=np.uint64)
    return masks[np.argsort(~_brev64(masks), kind="stable")]


def mask_tuple(mask):
    mask = int(mask)
    return tuple(i for i in range(mask.bit_length()) if mask >> i & 1)


def connected_subsets_esu(adj, k):
    return [mask_tuple(x) for x in sorted_masks(adj, k)]


def sample_batch(edge_index, ptr, m_per_graph, k, mode="sample", seed=42, enumerate_fn=None):
    """The five int64 arrays (nodes [G*m, k], edge_index [2, E], edge_ptr [G*m+1], sample_ptr [G+1], edge_src [E])."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, dtype=np.int64)
    src, dst = ei[0], ei[1]
    G, m = len(ptr) - 1, int(m_per_graph)
    enum = enumerate_fn or (lambda adj, kk: sorted_masks(adj, kk) if len(adj) <= 64 else connected_subsets_comb(adj, kk))
    gen = mt19937_64(seed & M64)
    nodes = np.full((max(G, 0) * m, k), -1, dtype=np.int64)
    eu, ev, es, eptr = [], [], [], [0]
    cols = np.arange(src.shape[0], dtype=np.int64)
    for g in range(G):
        lo, n = int(ptr[g]), int(ptr[g + 1] - ptr[g])
        subsets = enum(graph_adjacency(src, dst, lo, n), k) if n >= k else []
        inside = (src >= lo) & (src < lo + n) & (dst >= lo) & (dst < lo + n)
        cu, cv, cc = (src[inside] - lo).tolist(), (dst[inside] - lo).tolist(), cols[inside].tolist()
        for s in range(m):
            row = g * m + s
            if len(subsets):
                sub = subsets[lemire(gen, len(subsets))]
                sub = sub if isinstance(sub, tuple) else mask_tuple(sub)
                pos = {v: i for i, v in enumerate(sub)}
                nodes[row] = [lo + v for v in sub]
                for u, v, c in zip(cu, cv, cc):
                    if u in pos and v in pos:
                        eu.append(pos[u] if mode == "sample" else lo + u)
                        ev.append(pos[v] if mode == "sample" else lo + v)
                        es.append(c)
            eptr.append(len(es))
    return (nodes, np.array([eu, ev], dtype=np.int64).reshape(2, -1), np.array(eptr, dtype=np.int64),
            np.arange(max(G, 0) + 1, dtype=np.int64) * m, np.array(es, dtype=np.int64))


def draws_blocked(outputs, sizes, block=312):
    """The draw kernel's cursor logic (ugs_uniform.hip, uni_draw), restated: `outputs` yields the generator's words in blocks of
    `block`; within a block every pending draw d takes word pos + (d - d0), assuming each draw consumes one word; the first draw
    whose Lemire step rejects (lo64(x * N) < 2^64 mod N) ends the round: the draws before it stand, its word is consumed and it is
    retried in the next round.  Must equal [lemire(gen, N) for N in sizes]."""
    words, pos, res, d0 = [outputs() for _ in range(block)], 0, [], 0
    while d0 < len(sizes):
        todo = min(len(sizes) - d0, block - pos)
        first = todo
        for i in range(todo):
            n, x = sizes[d0 + i], words[pos + i]
            lo = (x * n) & M64
            if lo < n and lo < ((1 << 64) - n) % n:
                first = i
                break
            res.append((x * n) >> 64)
        d0 += first
        pos += first + (1 if first < todo else 0)
        if pos == block:
            words, pos = [outputs() for _ in range(block)], 0
    return res


# ---- which kernel path an input reaches (ugs_uniform.hip), from the law's own quantities -------------------------------------------
SMALL_SORT, DRAW_BLOCK, MT_BLOCK, SCAN_ONE_BLOCK, ROW_BLOCK, FLUSH = 8192, 320, 312, 16384, 256, 4096

CLASSES = (
    # columns
    "stray_cross", "stray_below", "stray_above", "stray_negative", "empty_graph_first", "empty_graph_middle", "empty_graph_last",
    "ptr0_nonzero", "G_pow2_with_stray", "loop_column", "duplicate_column", "columns_shuffled",
    # search
    "k1", "k2", "k3", "k8", "k9", "k_ge_33", "k_eq_n_64", "root_63", "w0_63", "item_ge_4096", "graph_n_lt_k",
    # scan
    "items_le_16384", "items_gt_16384",
    # sort
    "bucket_0", "bucket_1", "bucket_2", "bucket_np2", "bucket_pow2", "bucket_8192", "bucket_8193", "small_and_large_in_one_call",
    # draws, one generator
    "G_le_320", "G_eq_320", "G_eq_321", "G_gt_640", "empties_between", "eq_312", "eq_313", "eq_624", "eq_625", "m0", "size_1",
    "seed_0", "seed_all_ones",
    # draws, per-graph seeds
    "m_eq_312", "m_eq_313", "m_gt_624", "graph_without_sets",
    # rows and fill
    "rows_cross_256", "row_without_edges", "edge_at_vertex_63", "loop_in_subset", "sample", "global",
)


def item_counts(adj, k):
    """{(root v, first extension w): number of connected k-subsets of that item}: the search of esu_masks, counting at the last
    level (popcount of the extension set) instead of listing, so that K_30 at k = 6 costs C(30, 5) steps and not C(30, 6)."""
    n = len(adj)
    out = {}
    if k <= 0 or k > n:
        return out
    for v in range(n):
        above = ((1 << n) - 1) & ~((2 << v) - 1)
        if k == 1:
            out[(v, 0)] = 1
            continue
        ext1, nb1 = adj[v] & above, adj[v] | (1 << v)
        e1 = ext1
        while e1:
            w0 = (e1 & -e1).bit_length() - 1
            e1 &= e1 - 1
            cnt = 0
            stack = [(2, e1 | (adj[w0] & ~nb1 & above), nb1 | adj[w0])]
            while stack:
                size, ext, nb = stack.pop()
                if size == k:
                    cnt += 1
                elif size == k - 1:
                    cnt += bin(ext).count("1")
                else:
                    while ext:
                        w = (ext & -ext).bit_length() - 1
                        ext &= ext - 1
                        stack.append((size + 1, ext | (adj[w] & ~nb & above), nb | adj[w]))
            if cnt:
                out[(v, w0)] = cnt
    return out


def census(ei, ptr, m, k, seeds_or_seed, per_graph, what="sample", mode=None):
    """The set of path classes (CLASSES) that the call reaches in ugs_uniform.hip, from the input and the law alone: bucket sizes,
    item counts, draw totals, the drawn rows.  `what`: "sample" (sample_batch, or sample_graphs when per_graph), "enumerate" (a row
    per set) or "count" (no sort, no draw, no row).  `seeds_or_seed`: the call's seed, or one seed per graph when per_graph."""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    src, dst = ei[0], ei[1]
    G, E = len(ptr) - 1, ei.shape[1]
    out = set()
    hit = lambda name, cond=True: out.add(name) if cond else None    # noqa: E731
    # columns
    first, last = int(ptr[0]), int(ptr[-1])
    sizes = np.diff(ptr)
    gof = lambda x: np.where((x >= first) & (x < last), np.searchsorted(ptr, x, "right") - 1, -1)   # noqa: E731
    # searchsorted over repeated ptr values returns the last graph starting there, i.e. the non-empty one
    gu, gv = gof(src), gof(dst)
    key = np.where((gu == gv) & (gu >= 0), gu, G)
    stray = key == G
    hit("stray_cross", ((gu >= 0) & (gv >= 0) & (gu != gv)).any())
    hit("stray_below", (((src < first) & (src >= 0)) | ((dst < first) & (dst >= 0))).any())
    hit("stray_above", ((src >= last) | (dst >= last)).any())
    hit("stray_negative", ((src < 0) | (dst < 0)).any())
    if G > 0:
        empty = sizes == 0
        hit("empty_graph_first", empty[0])
        hit("empty_graph_last", empty[-1])
        hit("empty_graph_middle", G > 2 and empty[1:-1].any())
    hit("ptr0_nonzero", first != 0)
    hit("G_pow2_with_stray", G in (1, 2, 4, 256) and stray.any())
    hit("loop_column", ((src == dst) & ~stray).any())
    inside = np.stack([src[~stray], dst[~stray]], axis=1)
    hit("duplicate_column", len(np.unique(inside, axis=0)) < len(inside))
    hit("columns_shuffled", (np.diff(key[~stray]) < 0).any())
    # search: the graphs that are enumerated hold at least k vertices (k >= 1)
    adjs = [graph_adjacency(src, dst, int(ptr[g]), int(sizes[g])) for g in range(G)]
    live = [g for g in range(G) if k >= 1 and sizes[g] >= k]
    for name, cond in (("k1", k == 1), ("k2", k == 2), ("k3", k == 3), ("k8", k == 8), ("k9", k == 9), ("k_ge_33", k >= 33)):
        hit(name, cond and bool(live))
    hit("k_eq_n_64", k == 64 and bool(live))
    hit("graph_n_lt_k", any(sizes[g] < k for g in range(G)))
    items = {g: item_counts(adjs[g], k) for g in live}
    for g in live:
        if k >= 2 and sizes[g] == 64:
            hit("root_63", adjs[g][63] != 0)
            hit("w0_63", any(w0 == 63 for _, w0 in items[g]) or any(adjs[g][v] >> 63 & 1 for v in range(63)))
        hit("item_ge_4096", any(c >= FLUSH for c in items[g].values()))
    nv = int(sum(sizes[g] for g in live))
    if live:
        hit("items_le_16384", nv * 64 <= SCAN_ONE_BLOCK)
        hit("items_gt_16384", nv * 64 > SCAN_ONE_BLOCK)
    gsize = {g: sum(items[g].values()) for g in live}
    if what == "count":
        return out
    # sort: one bucket per root
    buckets = []
    for g in live:
        per_root = [0] * int(sizes[g])
        for (v, _), c in items[g].items():
            per_root[v] += c
        buckets += per_root
    for n in buckets:
        hit("bucket_0", n == 0)
        hit("bucket_1", n == 1)
        hit("bucket_2", n == 2)
        hit("bucket_np2", n >= 3 and n & (n - 1) != 0)
        hit("bucket_pow2", n >= 4 and n & (n - 1) == 0)
        hit("bucket_8192", n == SMALL_SORT)
        hit("bucket_8193", n == SMALL_SORT + 1)
    hit("small_and_large_in_one_call", any(n > SMALL_SORT for n in buckets) and any(2 <= n <= SMALL_SORT for n in buckets) and 1 in buckets)
    # the sets, and the rows the call emits: (graph, mask)
    sets = {g: sorted_masks(adjs[g], k) for g in live if gsize[g] > 0}
    nonempty = sorted(sets)
    rows = []
    if what == "enumerate":
        rows = [(g, int(x)) for g in nonempty for x in sets[g]]
    elif per_graph:
        seeds = [int(s) & M64 for s in seeds_or_seed]
        hit("m_eq_312", m == MT_BLOCK and bool(nonempty))
        hit("m_eq_313", m == MT_BLOCK + 1 and bool(nonempty))
        hit("m_gt_624", m > 2 * MT_BLOCK and bool(nonempty))
        hit("graph_without_sets", m > 0 and len(nonempty) < G)
        for g in nonempty:
            gen = mt19937_64(seeds[g])
            rows += [(g, int(sets[g][lemire(gen, len(sets[g]))])) for _ in range(m)]
    else:
        seed = int(seeds_or_seed) & M64
        hit("G_le_320", G <= DRAW_BLOCK)
        hit("G_eq_320", G == DRAW_BLOCK)
        hit("G_eq_321", G == DRAW_BLOCK + 1)
        hit("G_gt_640", G > 2 * DRAW_BLOCK)
        hit("empties_between", any(i != g for i, g in enumerate(nonempty)))
        total = len(nonempty) * m
        for t in (312, 313, 624, 625):
            hit(f"eq_{t}", total == t)
        hit("m0", m == 0 and G > 0)
        hit("size_1", m > 0 and any(len(sets[g]) == 1 for g in nonempty))
        hit("seed_0", seed == 0 and total > 0)
        hit("seed_all_ones", seed == M64 and total > 0)
        gen = mt19937_64(seed)
        for g in nonempty:
            rows += [(g, int(sets[g][lemire(gen, len(sets[g]))])) for _ in range(m)]
    # rows and fill
    n_rows = len(rows) if what == "enumerate" else G * m
    hit("rows_cross_256", n_rows > ROW_BLOCK)
    if rows and mode is not None:
        hit("sample", mode == "sample")
        hit("global", mode != "sample")
    cols = {}
    for g in {g for g, _ in rows}:
        sel = key == g
        cols[g] = list(zip((src[sel] - ptr[g]).tolist(), (dst[sel] - ptr[g]).tolist()))
    for g, mask in set(rows):
        inside = [(u, v) for u, v in cols[g] if mask >> u & mask >> v & 1]
        hit("row_without_edges", not inside)
        hit("edge_at_vertex_63", any(u == 63 or v == 63 for u, v in inside))
        hit("loop_in_subset", any(u == v for u, v in inside))
    return out
