"""uniform_wide_device_model.py -- CPU model of what the wide-form kernels of ugs_uniform.hip compute, lane by lane where a lane can be
wrong: uni_wadj's bitmap and pair packing, uni_wesu (the slot loop and its r-th member, `later`, `abv`, group_take, key_with,
wide_level, wide_last with row_scan, the count pass's per-lane flush), the per-root sort, uni_wrows / uni_wfill, enum_graph with
uni_wenum_rows / uni_wenum_fill, and uni_wpop_rows / uni_wpop_fill with their chunks of 16 columns.  `uniform_wide_law` states what
must come out; this states how the kernels get there.  A vertex set is one Python int whose 64-bit word l is what lane l holds: the
set algebra of the kernel is the same in every lane, so it is done on the whole int, and everything that treats lanes differently
(abv, later, ballot + ffs, the DPP scan, the per-lane counters and output pointers) is done per word.

What is modelled elsewhere and taken from the law here: the column buckets, the sort of a bucket (np.sort), the generator and the
draws, and the mask graphs of a mixed batch (tests/uniform_device_model.py); their keys ~brev(mask) still lie in front of the wide
graphs' keys in one array, as in the kernel, so a row that reads the wrong place reads what the kernel would.  Not modelled: the
bounded work of a call past its budget (it depends on the order in which groups reach the counter); a graph or a call past the
budget is emptied or refused from its full count, as uni_cap and uni_joint do.

`mutant=` swaps one line for a plausible slip.  tests/test_uniform_wide_paths_law.py asserts that the model equals the law on every
input of tests/uniform_wide_paths.py and that every mutant of MUTANTS differs on at least one.  A mutant that reads or writes outside
its arrays raises ModelFault, which counts as differing.

MUTANTS that change results:
  one_trip           the slot loop without `r += 64`: a root's 65th and later higher neighbours are never a first extension
  later_le           `later` with `x.l <= l0 ? 0`: the members of ext1 behind w in w's own word are lost
  later_no_guard     `later` from `~0ull << (f + 1)` without the `f >= 63` case: the shift count 64 is taken mod 64, w comes back
  abv_no_own_word    `abv` without `x.l == vw`: every vertex of the root's word counts as above the root
  take_clear_all     group_take clearing the lowest bit in every lane: the other words lose a member each
  excl_lt            `excl < r` for `excl <= r`: the first member of a word is held by no lane, ffs(0) - 1 names word -1
  scan_no_shr1       row_scan without row_shr:1
  scan_no_shr2       row_scan without row_shr:2
  scan_no_shr4       row_scan without row_shr:4
  scan_no_shr8       row_scan without row_shr:8
  out_pc             wide_last: `x.out += pc` for `tot`: every lane advances by its own count
  fb_le              field_bits with `(1 << b) <= n`: at n = 2^j one bit more per field, past 64 bits where k (j + 1) > 64
  wadj_W_shr6        uni_wadj with `W = n >> 6`: the rows of the bitmap overlap unless 64 divides n
  wadj_and31         uni_wadj with `v & 31`
  wrows_g_m          uni_wrows drawing at `g * m + s` for `nepos[g] * m + s`
  wrows_key_ne0      uni_wrows valid by `key != 0`: the set {0} at k = 1 becomes a row of -1
  tp_shift           tuple_pos with shift `b * j`: the positions run backwards
  wfill_swap         uni_wfill with the two 16-bit halves of wpair swapped
  enum_lt            enum_graph with `sptr[mid + 1] < row`: a graph's first row is given to the graph before
  pop_carry_lane0    uni_wpop_fill: the chunk carry from lane 0 for lane 15
EQUIVALENT (they change which path runs, never a result):
  take_highest       group_take taking the highest non-empty lane: the search may take the members of an extension set in any order
                     (each set is still found once, from its smallest vertex), and the root buckets are sorted afterwards
  key_ge             key_with counting `>=`: w is never a member of the set it is added to, so no field equals it
  key_fields_D1      key_with counting over D + 1 fields: the field above the root is 0 and w is at least 1
  key_no_sh64        key_with without its `sh + b >= 64` case: the root is the smallest vertex and keeps the top field, so at most
                     D - 1 fields exceed w and sh + b <= D b <= 56; the model asserts it at every call
"""
import numpy as np

import uniform_law as U
import uniform_wide_law as W

M64 = U.M64
LANES, ITEMS, LANE_FLUSH, MAX_K, SMALL_SORT, POP_LANES = 16, 64, 4096 // 16, 8, 8192, 16
MUTANTS = ("one_trip", "later_le", "later_no_guard", "abv_no_own_word", "take_clear_all", "excl_lt", "scan_no_shr1", "scan_no_shr2",
           "scan_no_shr4", "scan_no_shr8", "out_pc", "fb_le", "wadj_W_shr6", "wadj_and31", "wrows_g_m", "wrows_key_ne0", "tp_shift",
           "wfill_swap", "enum_lt", "pop_carry_lane0")
EQUIVALENT = ("take_highest", "key_ge", "key_fields_D1", "key_no_sh64")
UNWRITTEN = -(1 << 40)                                               # an output word no lane wrote


class ModelFault(Exception):
    """the mutant reads or writes outside its arrays"""


class Refused(Exception):
    """the call's healthy graphs together are past the budget: "split the call" """


def brev(x):
    return int(f"{x:064b}"[::-1], 2)


def pc(x):
    return bin(x).count("1")


def ffs(x):
    return (x & -x).bit_length() - 1                                 # __ffsll(x) - 1; -1 for 0


class Model:
    def __init__(self, ei, ptr, k, per_graph=False, mutant=None, limit=1024, mask_vertices=64, budget=W.BUDGET, over=()):
        assert mutant is None or mutant in MUTANTS + EQUIVALENT, mutant
        ei = np.asarray(ei, np.int64).reshape(2, -1)
        self.src, self.dst = ei[0], ei[1]
        self.ptr = np.asarray(ptr, np.int64).tolist()
        self.G, self.k, self.per_graph, self.mutant, self.budget, self.over = len(self.ptr) - 1, int(k), per_graph, mutant, budget, set(over)
        self.limit, self.mask_vertices = limit, mask_vertices
        self.flushes, self.max_sh_b, self.prepared, self._index = {}, 0, False, {}

    # ---- the host's graph records, the column buckets (from the law), uni_wadj ----
    def field_bits(self, n):
        b = 1
        while b < 16 and (((1 << b) <= n) if self.mutant == "fb_le" else ((1 << b) < n)):
            b += 1
        return b

    def columns(self):
        k, mut = self.k, self.mutant
        self.graphs, self.cols, nv = [], [], 0
        for g in range(self.G):
            lo, n = self.ptr[g], self.ptr[g + 1] - self.ptr[g]
            wanted, fits = k >= 1 and n >= k, k <= MAX_K and k * W.field_bits(n) <= 64
            over = wanted and n > 64 and (n > self.limit or not fits)
            form = 0 if not wanted or over else 2 if n > 64 or (n > self.mask_vertices and fits) else 1
            self.graphs.append([lo, n, 0, form])
            inside = (self.src >= lo) & (self.src < lo + n) & (self.dst >= lo) & (self.dst < lo + n)
            self.cols.append(np.nonzero(inside)[0].tolist())         # the graph's bucket: its columns in column order
        for want in (1, 2):                                          # the enumerated vertices: the mask graphs' first
            for gd in self.graphs:
                if gd[3] == want:
                    gd[2] = nv
                    nv += gd[1]
            if want == 1:
                self.nv_mask = nv
        self.nv = nv
        self.vgraph = {}
        self.wpair, self.rows = {}, {}
        for g, (lo, n, vbase, form) in enumerate(self.graphs):
            if form != 2:
                continue
            for v in range(n):
                self.vgraph[vbase + v] = g
            Wg = (n >> 6) if mut == "wadj_W_shr6" else (n + 63) >> 6
            sh = 31 if mut == "wadj_and31" else 63
            wadj = [0] * (n * ((n + 63) >> 6))
            pairs = []
            for col in self.cols[g]:
                u, v = int(self.src[col]) - lo, int(self.dst[col]) - lo
                pairs.append(u | (v << 16))
                if u == v:
                    continue
                wadj[u * Wg + (v >> 6)] |= 1 << (v & sh)
                wadj[v * Wg + (u >> 6)] |= 1 << (u & sh)
            self.wpair[g] = pairs
            Wr = (n + 63) >> 6                                       # uni_wesu reads rows of (n + 63) >> 6 words
            self.rows[g] = [sum(wadj[w * Wr + l] << (64 * l) for l in range(Wr)) for w in range(n)]

    # ---- uni_wesu ----
    def row_scan(self, x):
        for s in (1, 2, 4, 8):
            if self.mutant != f"scan_no_shr{s}":
                x = [x[l] + (x[l - s] if l >= s else 0) for l in range(LANES)]
        return x

    def above_word(self, f, guard=True):
        if f >= 63 and guard:
            return 0
        return (M64 << ((f + 1) % 64)) & M64

    def lanes_from(self, l0, own, strict=False):
        """a set whose word l is 0 below lane l0, `own` at l0 (0 there too if strict), all ones above"""
        out = 0
        for l in range(LANES):
            word = 0 if l < l0 or (strict and l == l0) else own if l == l0 else M64
            out |= word << (64 * l)
        return out

    def take(self, ext):
        """group_take: (the vertex, what is left of ext); (-1, ext) for the empty set"""
        ws = W.words(ext)
        lanes = [l for l in range(LANES) if ws[l]]
        if not lanes:
            return -1, ext
        l0 = lanes[-1] if self.mutant == "take_highest" else lanes[0]
        f = ffs(ws[l0])
        if self.mutant == "take_clear_all":
            ext = sum((x & (x - 1)) << (64 * l) for l, x in enumerate(ws))
        else:
            ext &= ~(1 << (l0 * 64 + f))
        return l0 * 64 + f, ext

    def key_with(self, D, key, w, b):
        mut, fm = self.mutant, (1 << b) - 1
        fields = [(key >> (i * b)) & fm for i in range(D + 1 if mut == "key_fields_D1" else D)]
        if mut is None:
            assert w not in fields[:D] and (key >> (D * b)) == 0 and w >= 1      # what makes key_ge and key_fields_D1 equivalent
        above = sum(1 for f in fields if (f >= w if mut == "key_ge" else f > w))
        sh = above * b
        self.max_sh_b = max(self.max_sh_b, sh + b)
        if mut in (None, "key_no_sh64"):
            assert above <= D - 1 and sh + b <= D * b <= 56, (D, b, sh)          # the `sh + b >= 64` case is never taken
        hi = key >> sh
        return ((0 if sh + b >= 64 and mut != "key_no_sh64" else hi << (sh + b)) | (w << sh) | (key & ((1 << sh) - 1))) & M64

    def last(self, D, x, ext, key):
        ws = W.words(ext)
        pcs = [pc(a) for a in ws]
        if x["write"]:
            incl = self.row_scan(pcs)
            tot = incl[LANES - 1]
            for l in range(LANES):
                o, e = x["out"][l] + incl[l] - pcs[l], ws[l]
                while e:
                    if not 0 <= o < len(self.keys_a):
                        raise ModelFault("a key outside keys_a")
                    self.keys_a[o] = self.key_with(D, key, l * 64 + ffs(e), x["b"])
                    o += 1
                    e &= e - 1
                x["out"][l] += pcs[l] if self.mutant == "out_pc" else tot
        else:
            cnt, flushed = x["cnt"], x["flushed"]
            for l in range(LANES):
                cnt[l] += pcs[l]
                if cnt[l] - flushed[l] >= LANE_FLUSH:
                    flushed[l] = cnt[l]
                    x["nflush"] += 1

    def level(self, D, x, ext, nb, key):
        if D == self.k - 1:
            return self.last(D, x, ext, key)
        if D < MAX_K - 1:
            while True:
                w, ext = self.take(ext)
                if w < 0:
                    break
                if w >= x["n"]:
                    raise ModelFault("a bitmap row outside the graph")
                aw = x["rows"][w]
                self.level(D + 1, x, ext | (aw & ~nb & x["abv"]), nb | aw, self.key_with(D, key, w, x["b"]))

    def wesu_root(self, vi, write):
        """uni_wesu<WRITE> of the 64 items of root vi: COUNT fills icount, WRITE stores the keys at ioff[item]"""
        mut, k = self.mutant, self.k
        g = self.vgraph[vi]
        lo, n, vbase, _ = self.graphs[g]
        v = vi - vbase
        vw, rows, b = v >> 6, self.rows[g], self.field_bits(n)
        abv = self.lanes_from(vw, M64 if mut == "abv_no_own_word" else self.above_word(v & 63))
        av = rows[v]
        ext1, nb1 = av & abv, av | (1 << v)
        pcs = [pc(a) for a in W.words(ext1)]
        incl = self.row_scan(pcs)
        excl, deg = [i - p for i, p in zip(incl, pcs)], incl[LANES - 1]
        for slot in range(ITEMS):
            item = vi * 64 + slot
            if k >= 3 and slot >= deg:
                break                                                # (the slot loop of this and every later item runs no trip)
            if write and not self.icount[item]:
                continue                                             # (an item without room writes nothing: it has no sets)
            x = {"write": write, "n": n, "rows": rows, "b": b, "abv": abv, "cnt": [0] * LANES, "flushed": [0] * LANES, "nflush": 0,
                 "out": [self.ioff[item]] * LANES if write else None}
            if k == 1:
                if slot == 0:
                    if write:
                        self.keys_a[x["out"][0]] = v
                    else:
                        x["cnt"][0] = 1
            elif k == 2:
                if slot == 0:
                    self.last(1, x, ext1, v)
            else:
                r = slot
                while r < deg:
                    holds = [l for l in range(LANES) if ((excl[l] < r) if mut == "excl_lt" else (excl[l] <= r)) and r < incl[l]]
                    if not holds:
                        raise ModelFault("no lane holds the r-th member: ffs(0) - 1 = -1 names a word in front of the bitmap")
                    l0, t = holds[0], W.words(ext1)[holds[0]]
                    for _ in range(r - excl[l0]):
                        t &= t - 1
                    f = ffs(t)
                    w = l0 * 64 + f
                    if not 0 <= w < n:
                        raise ModelFault("a bitmap row outside the graph")
                    aw = rows[w]
                    later = self.lanes_from(l0, self.above_word(f, guard=mut != "later_no_guard"), strict=mut == "later_le")
                    self.level(2, x, (ext1 & later) | (aw & ~nb1 & abv), nb1 | aw, ((v << b) | w) & M64)
                    if mut == "one_trip":
                        break
                    r += 64
            if not write:
                self.icount[item] = self.row_scan(x["cnt"])[LANES - 1]
                if x["nflush"]:
                    self.flushes[item] = (x["nflush"], [c - f for c, f in zip(x["cnt"], x["flushed"])])
            if k <= 2:
                break

    def count(self):
        """The count pass of the wide graphs (the mask graphs' counts from the law): per-graph totals; over the budget: -1"""
        self.columns()
        self.icount = {}
        gcount = [0] * self.G
        for g, (lo, n, vbase, form) in enumerate(self.graphs):
            if form == 1:
                self.mask_sets = getattr(self, "mask_sets", {})
                self.mask_sets[g] = U.sorted_masks(U.graph_adjacency(self.src, self.dst, lo, n), self.k)
                gcount[g] = len(self.mask_sets[g])
            elif form == 2 and g in self.over:
                gcount[g] = self.budget + 1                          # stated with the case: past the budget, never walked here
            elif form == 2:
                for v in range(n):
                    for slot in range(ITEMS):
                        self.icount[(vbase + v) * 64 + slot] = 0
                    self.wesu_root(vbase + v, False)
                gcount[g] = sum(self.icount[(vbase + v) * 64 + s] for v in range(n) for s in range(ITEMS))
        self.gcount = gcount
        return gcount

    # ---- uni_cap, scan, write pass, the per-root sort, gstart / gsize ----
    def prepare(self):
        if self.prepared:
            return
        self.prepared = True
        self.count()
        self.failed = [self.graphs[g][3] != 0 and self.gcount[g] > self.budget for g in range(self.G)]
        total = sum(c for g, c in enumerate(self.gcount) if not self.failed[g])
        if total > self.budget:
            raise Refused(total)
        flat, self.gstart, self.gsize = [], [0] * self.G, [0] * self.G
        for g, (lo, n, vbase, form) in enumerate(self.graphs):       # the mask graphs' keys first
            if form == 1 and not self.failed[g]:
                self.gstart[g], self.gsize[g] = len(flat), len(self.mask_sets[g])
                flat += [~brev(int(x)) & M64 for x in self.mask_sets[g]]
        wide = [g for g in range(self.G) if self.graphs[g][3] == 2 and not self.failed[g]]
        self.ioff, off = {}, 0
        for g in wide:
            lo, n, vbase, _ = self.graphs[g]
            for item in range(vbase * 64, (vbase + n) * 64 + 1):
                self.ioff[item] = off
                off += self.icount.get(item, 0) if item < (vbase + n) * 64 else 0
        self.keys_a = [0] * off
        for g in wide:
            lo, n, vbase, _ = self.graphs[g]
            for v in range(n):
                self.wesu_root(vbase + v, True)
        base = len(flat)
        self.buckets = []
        for g in wide:
            lo, n, vbase, _ = self.graphs[g]
            for v in range(n):
                b0, b1 = self.ioff[(vbase + v) * 64], self.ioff[(vbase + v) * 64 + 64]
                self.keys_a[b0:b1] = sorted(self.keys_a[b0:b1])
                self.buckets.append(b1 - b0)
            self.gstart[g] = base + self.ioff[vbase * 64]
            self.gsize[g] = self.ioff[(vbase + n) * 64] - self.ioff[vbase * 64]
        self.keys_sorted = flat + self.keys_a

    def key_at(self, i):
        return self.keys_sorted[i] if 0 <= i < len(self.keys_sorted) else 0    # behind the keys: what a fresh blob holds

    # ---- rows and fill ----
    def pair_index(self, g):
        if g not in self._index:
            self._index[g] = {}
            for q, uv in enumerate(self.wpair[g]):
                self._index[g].setdefault(uv, []).append(q)
        return self._index[g]

    def wide_row(self, g, key, mode, fill_swap, pop):
        """(nodes, [(eu, ev, column)] in the order of the output) of a wide graph's row, as uni_wrows + uni_wfill, uni_wenum_* or
        (pop) uni_wpop_rows + uni_wpop_fill write it"""
        lo, n, _, _ = self.graphs[g]
        k = self.k
        b = W.field_bits(n) if pop else self.field_bits(n)           # the population keeps the host's b
        fm = (1 << b) - 1
        nodes = [lo + ((key >> (b * (k - 1 - j))) & fm) for j in range(k)]
        # tuple_pos of every 16-bit value that has a position (the first field that holds it), then the columns whose two halves
        # both have one: the same hits as the kernels' walk over the whole bucket, found through an index of the bucket's pairs
        pos = {}
        for j in range(k):
            pos.setdefault((key >> (b * (j if self.mutant == "tp_shift" else k - 1 - j))) & fm & M64, j)
        index = self.pair_index(g)
        hits = [None] * len(self.wpair[g])
        for lo16 in pos:
            for hi16 in pos:
                for q in index.get(lo16 | (hi16 << 16), ()):
                    u, v = (hi16, lo16) if fill_swap else (lo16, hi16)
                    hits[q] = (pos[u], pos[v]) if mode == "sample" else (lo + u, lo + v)
        cols = self.cols[g]
        if not pop:
            return nodes, [(h[0], h[1], cols[q]) for q, h in enumerate(hits) if h is not None]
        # uni_wpop_rows: lane l counts the columns l, l + 16, ...; uni_wpop_fill: chunk after chunk at the row-wide exclusive prefix
        cnt = [sum(1 for q in range(l, len(hits), POP_LANES) if hits[q] is not None) for l in range(POP_LANES)]
        out = [None] * self.row_scan(cnt)[POP_LANES - 1]
        w = 0
        for base in range(0, len(hits), POP_LANES):
            hit = [1 if base + l < len(hits) and hits[base + l] is not None else 0 for l in range(POP_LANES)]
            incl = self.row_scan(hit)
            for l in range(POP_LANES):
                if hit[l]:
                    o = w + incl[l] - 1
                    if not 0 <= o < len(out):
                        raise ModelFault("an edge outside the row's room")
                    out[o] = hits[base + l] + (cols[base + l],)
            w += incl[0] if self.mutant == "pop_carry_lane0" else incl[POP_LANES - 1]
        return nodes, [e if e is not None else (UNWRITTEN, UNWRITTEN, UNWRITTEN) for e in out]

    def mask_row(self, g, key, mode):
        lo = self.graphs[g][0]
        mask = brev(~key & M64)
        members = [i for i in range(64) if mask >> i & 1]
        pos = {v: i for i, v in enumerate(members)}
        edges = []
        for col in self.cols[g]:
            u, v = int(self.src[col]) - lo, int(self.dst[col]) - lo
            if u in pos and v in pos:
                edges.append((pos[u], pos[v], col) if mode == "sample" else (lo + u, lo + v, col))
        return [lo + v for v in members[:self.k]] + [-1] * (self.k - len(members)), edges

    def assemble(self, rows):
        k = self.k
        nodes = np.array([r[0] for r in rows], np.int64).reshape(len(rows), k)
        eptr = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])]).astype(np.int64)
        edges = np.array([e for r in rows for e in r[1]], np.int64).reshape(-1, 3)
        return nodes, np.ascontiguousarray(edges[:, :2].T), eptr, np.ascontiguousarray(edges[:, 2])

    def sample(self, m, mode, seed=None, seeds=None, pop=False):
        self.prepare()
        G, mut = self.G, self.mutant
        draws = [0] * (G * m)
        nonempty = [g for g in range(G) if self.gsize[g] > 0]
        nepos = {g: i for i, g in enumerate(nonempty)}
        if seeds is None:
            gen = U.mt19937_64(int(seed) & M64)
            for i, g in enumerate(nonempty):
                for s in range(m):
                    draws[i * m + s] = U.lemire(gen, self.gsize[g])
        else:
            for g in nonempty:
                gen = U.mt19937_64(int(seeds[g]) & M64)
                for s in range(m):
                    draws[g * m + s] = U.lemire(gen, self.gsize[g])
        rows = []
        for row in range(G * m):
            g, s = row // m, row % m
            form = self.graphs[g][3]
            if self.gsize[g] <= 0:
                rows.append(([-1] * self.k, []))
                continue
            if form == 1:
                d = row if seeds is not None else nepos[g] * m + s
                rows.append(self.mask_row(g, self.keys_sorted[self.gstart[g] + draws[d]], mode))
                continue
            d = row if seeds is not None else (g if mut == "wrows_g_m" and not pop else nepos[g]) * m + s
            key = self.key_at(self.gstart[g] + draws[d])
            if mut == "wrows_key_ne0" and not pop and key == 0:
                rows.append(([-1] * self.k, []))
                continue
            rows.append(self.wide_row(g, key, mode, mut == "wfill_swap" and not pop, pop))
        nodes, eidx, eptr, esrc = self.assemble(rows)
        return nodes, eidx, eptr, np.arange(G + 1, dtype=np.int64) * m, esrc

    def enumerate(self, mode):
        self.prepare()
        G = self.G
        sptr = np.concatenate([[0], np.cumsum(self.gsize)]).astype(np.int64).tolist()
        rows = []
        for row in range(sptr[-1]):
            lo, hi = 0, G - 1
            while lo < hi:
                mid = (lo + hi) >> 1
                if (sptr[mid + 1] < row) if self.mutant == "enum_lt" else (sptr[mid + 1] <= row):
                    lo = mid + 1
                else:
                    hi = mid
            g = lo
            key = self.key_at(self.gstart[g] + row - sptr[g])
            form = self.graphs[g][3]
            if form == 2:
                rows.append(self.wide_row(g, key, mode, False, False))
            elif form == 1:
                rows.append(self.mask_row(g, key, mode))
            else:
                rows.append(([UNWRITTEN] * self.k, []))              # neither kernel takes the row
        nodes, eidx, eptr, esrc = self.assemble(rows)
        counts = [-1 if f else c for f, c in zip(self.failed, self.gcount)]
        return nodes, eidx, eptr, np.array(sptr, np.int64), esrc, np.array(counts, np.int64)
