"""uniform_device_model.py -- CPU model of what the mask-form kernels of ugs_uniform.hip compute, line for line where a line can be
wrong: uni_colgraph's search for a column's graph, the column sort's bit count, uni_bucket, uni_adj's pair packing, the uni_esu
stack (count and write pass, with the count pass's flushes), key_of / mask_of, uni_segments and uni_sort_small with the bitonic
network and its padding, uni_graph_sizes, uni_draw's 320-wide compaction with its carry, the three-part twist, the draw cursor,
uni_draw_graphs, and the decoding in uni_rows / uni_fill / uni_enum_rows / uni_enum_fill.  `uniform_law` states what must come out;
this states how the kernels get there.

`mutant=` swaps one line for a plausible slip.  tests/test_uniform_paths_law.py asserts that the model equals the law on every
input of tests/uniform_paths.py and that every mutant differs on at least one: the evidence that those inputs discriminate,
obtained without running a wrong kernel.  What the model cannot know is modelled as the value a fresh blob holds, 0: an entry no
kernel wrote (keys_b behind a small bucket that nobody copied, bpair of a column uni_adj skipped, the LDS word behind mt[]).
`current=` says which buffer the segmented sort hands back (keys.Current()): "a" (keys_a, uni_sort_small sorts in place) or "b"
(uni_sort_small writes every small bucket into the other buffer); the tests run the unmutated model with both.

MUTANTS that change results:
  above_no_guard     above_mask without `v >= 63`: `~0ull << 64` shifts by 64 mod 64 = 0, every vertex is "above" vertex 63
  ext2_no_above_w0   `ext[2] = ext1 | ...` without `& above_mask(w0)`: the root's earlier extensions come back, sets repeat
  nb_next            `adj[w] & ~nb[d + 1]` for `~nb[d]`: the level above's stale neighbourhood (0 where none was written yet)
  d_eq_k             `d == k` for `d == k - 1`: one level too deep, sets of k + 1 vertices
  key_no_complement  key_of / mask_of without the complement: the buckets come out in descending tuple order
  pad_zero           the bitonic network padded with 0: the padding sorts to the front of a bucket that is no power of two
  small_ge           uni_sort_small alone with `n >= SMALL_SORT`: a bucket of exactly 8192 keys is sorted by neither route
  no_copy_1          the n == 1 copy dropped: with keys.Current() == keys_b a one-key bucket never reaches the sorted array
  ptr_lt             uni_colgraph: `ptr[mid + 1] < u`: a column whose u is a graph's first vertex is searched into the graph before
  bits_lt            column sort bits from `(1 << bits) < G`: at G = 2^b the key G of stray columns sorts as 0, into graph 0's bucket
  no_carry           uni_draw: the compaction's base not carried across blocks of 320 graphs
  draw_g_m           uni_rows: draws indexed g * m instead of nepos[g] * m
  twist2_to_N        mt_twist part two run to `i < MT_N`: lane 311 reads mt[312] and part three then starts from its result
  twist3_mt_M        mt_twist part three reading mt[MT_M] for mt[MT_M - 1]
  pos_wrap_no_twist  the cursor past a full block goes back to 0 without the twist: the block's outputs are drawn from again
  decode_v_shr6      uni_rows / uni_fill: `v = uv >> 6` (the shift count taken mod 64, as the hardware does)
  popc_no_minus1     `__popcll(mask & (1ull << u))` without `- 1`: every endpoint at position 1
  cval_for_cval2     `edge_src[w] = c.cval[p]`: the bucket position for the column
EQUIVALENT (they change which path runs, never a result):
  switch_k9          the template switch at `k <= 9` with 8-entry stacks, index 8 aliasing index 0: levels 0 and 1 of the stacks
                     are never used (d starts at 2), so the alias overwrites nothing that is read
  seg_ge             uni_segments alone with `>=`: a bucket of exactly 8192 keys is sorted by both routes, to the same order
  decode_u_ff        `u = uv & 0xFF`: u < 64 and v sits at bit 8, so bits 6 and 7 are always 0
"""
import numpy as np

import uniform_law as U

M64 = U.M64
SMALL_SORT, DRAW_BLOCK, MT_N, MT_M = 8192, 320, 312, 156
MUTANTS = ("above_no_guard", "ext2_no_above_w0", "nb_next", "d_eq_k", "key_no_complement", "pad_zero", "small_ge", "no_copy_1",
           "ptr_lt", "bits_lt", "no_carry", "draw_g_m", "twist2_to_N", "twist3_mt_M", "pos_wrap_no_twist", "decode_v_shr6",
           "popc_no_minus1", "cval_for_cval2")
EQUIVALENT = ("switch_k9", "seg_ge", "decode_u_ff")


def brev(x):
    return int(f"{x:064b}"[::-1], 2)


def popcount(a):
    a = a.astype(np.uint64)
    out = np.zeros(a.shape, np.int64)
    for i in range(8):
        out += _POP8[((a >> np.uint64(8 * i)) & np.uint64(0xFF)).astype(np.int64)]
    return out


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


class Model:
    def __init__(self, ei, ptr, k, per_graph=False, mutant=None, current="b"):
        assert mutant is None or mutant in MUTANTS + EQUIVALENT, mutant
        ei = np.asarray(ei, np.int64).reshape(2, -1)
        self.src, self.dst = ei[0].tolist(), ei[1].tolist()
        self.ptr = np.asarray(ptr, np.int64).tolist()
        self.G, self.E, self.k, self.per_graph, self.mutant, self.current = len(self.ptr) - 1, ei.shape[1], int(k), per_graph, mutant, current
        self.flushes = {}                                            # item -> (flushes, remainder) of the count pass
        self.depth = 0                                               # deepest stack index written
        self.prepared = False

    # ---- uni_colgraph, the column sort, uni_bucket, uni_adj ----
    def columns(self):
        G, ptr, mut = self.G, self.ptr, self.mutant
        ckey = []
        for u, v in zip(self.src, self.dst):
            lo, hi = 0, G
            while lo < hi:
                mid = (lo + hi) >> 1
                if (ptr[mid + 1] < u) if mut == "ptr_lt" else (ptr[mid + 1] <= u):
                    lo = mid + 1
                else:
                    hi = mid
            key = G
            if lo < G and ptr[lo] <= u < ptr[lo + 1] and ptr[lo] <= v < ptr[lo + 1]:
                key = lo
            ckey.append(key)
        bits = 1
        while bits < 32 and (((1 << bits) < G) if mut == "bits_lt" else ((1 << bits) <= G)):
            bits += 1
        ckey = np.array(ckey, np.int64)
        order = np.argsort(ckey & ((1 << bits) - 1), kind="stable")   # the radix sort sees the low `bits` bits only
        self.ckey2, self.cval2 = ckey[order].tolist(), order.tolist()
        self.cstart = []
        for g in range(G + 1):
            lo, hi = 0, self.E
            while lo < hi:
                mid = (lo + hi) >> 1
                if self.ckey2[mid] < g:
                    lo = mid + 1
                else:
                    hi = mid
            self.cstart.append(lo)
        # the host's graph records: a graph is enumerated when it holds at least k vertices
        self.graphs, nv = [], 0
        for g in range(G):
            n = ptr[g + 1] - ptr[g]
            en = self.k >= 1 and n >= self.k
            assert n <= 64 or not en, "the mask form holds at most 64 vertices"
            self.graphs.append((ptr[g], n, nv if en else 0, en))
            nv += n if en else 0
        self.nv = nv
        self.vgraph = [g for g, (_, n, _, en) in enumerate(self.graphs) if en for _ in range(n)]
        self.adj, self.bpair = [0] * nv, [0] * self.E
        for p in range(self.E):
            g = self.ckey2[p]
            if g >= G:
                continue
            lo, n, vbase, en = self.graphs[g]
            if not en:
                continue
            col = self.cval2[p]
            u, v = self.src[col] - lo, self.dst[col] - lo
            self.bpair[p] = (u | (v << 8)) & 0xFFFF
            if u == v:
                continue
            self.adj[vbase + u] |= 1 << v
            self.adj[vbase + v] |= 1 << u

    # ---- uni_esu ----
    def above_mask(self, v):
        if v >= 63 and self.mutant != "above_no_guard":
            return 0
        return (M64 << ((v + 1) % 64)) & M64

    def key_of(self, mask):
        return brev(mask) if self.mutant == "key_no_complement" else ~brev(mask) & M64

    def mask_of(self, key):
        return brev(key) if self.mutant == "key_no_complement" else brev(~key & M64)

    def esu(self, item, write):
        """uni_esu<KM, WRITE> of one item: its count, and the keys in the order the write pass stores them."""
        k, mut = self.k, self.mutant
        KM = 8 if (k <= 9 if mut == "switch_k9" else k <= 8) else 64
        ix = (lambda d: d % KM) if mut in ("switch_k9", "d_eq_k") else (lambda d: d)
        vi, w0 = item >> 6, item & 63
        lo, n, vbase, _ = self.graphs[self.vgraph[vi]]
        v = vi - vbase
        adj = self.adj[vbase:vbase + n] + [0] * (64 - n)
        out, cnt, flushed, nflush = [], 0, 0, 0
        if k == 1:
            if w0 == 0:
                out.append(self.key_of(1 << v))
                cnt = 1
            return cnt, out
        abv = self.above_mask(v)
        ext1 = adj[v] & abv
        if not (ext1 >> w0) & 1:
            return 0, out
        nb1 = adj[v] | (1 << v)
        ext, nb, sub = [0] * KM, [0] * KM, [0] * KM
        d = 2
        sub[2] = (1 << v) | (1 << w0)
        ext[2] = ((ext1 if mut == "ext2_no_above_w0" else ext1 & self.above_mask(w0)) | (adj[w0] & ~nb1 & abv))
        nb[2] = nb1 | adj[w0]
        if k == 2:
            out.append(self.key_of(sub[2]))
            cnt, d = 1, 1
        last = k if mut == "d_eq_k" else k - 1
        while d >= 2:
            if d == last:
                if write:
                    e = ext[ix(d)]
                    while e:
                        out.append(self.key_of(sub[ix(d)] | (e & -e)))
                        e &= e - 1
                    cnt = len(out)
                else:
                    cnt += bin(ext[ix(d)]).count("1")
                    if cnt - flushed >= 4096:
                        flushed, nflush = cnt, nflush + 1
                d -= 1
                continue
            if not ext[ix(d)]:
                d -= 1
                continue
            e = ext[ix(d)]
            w = (e & -e).bit_length() - 1
            ext[ix(d)] = e & (e - 1)
            self.depth = max(self.depth, d + 1)
            sub[ix(d + 1)] = sub[ix(d)] | (1 << w)
            ext[ix(d + 1)] = ext[ix(d)] | (adj[w] & ~(nb[ix(d + 1)] if mut == "nb_next" else nb[ix(d)]) & abv)
            nb[ix(d + 1)] = nb[ix(d)] | adj[w]
            d += 1
        if not write and nflush:
            self.flushes[item] = (nflush, cnt - flushed)
        return cnt, out

    def count(self):
        """The count pass: icount per item and the per-graph totals (count_graphs stops here)."""
        self.columns()
        self.icount = [self.esu(item, False)[0] for item in range(self.nv * 64)]
        gcount = [0] * self.G
        for item, c in enumerate(self.icount):
            gcount[self.vgraph[item >> 6]] += c
        return gcount

    # ---- scan, write pass, uni_segments + segmented sort, uni_sort_small, uni_graph_sizes ----
    def bitonic(self, keys):
        n, mut = len(keys), self.mutant
        p = 2
        while p < n:
            p <<= 1
        s = np.full(p, 0 if mut == "pad_zero" else M64, np.uint64)
        s[:n] = keys
        i = np.arange(p)
        size = 2
        while size <= p:
            stride = size >> 1
            while stride > 0:
                j = i ^ stride
                sel = j > i
                ii, jj = i[sel], j[sel]
                up = (ii & size) == 0
                a, b = s[ii], s[jj]
                swap = (a > b) == up
                s[ii], s[jj] = np.where(swap, b, a), np.where(swap, a, b)
                stride >>= 1
            size <<= 1
        return s[:n]

    def prepare(self):
        if self.prepared:
            return
        self.prepared = True
        self.count()
        mut = self.mutant
        self.ioff = np.concatenate([[0], np.cumsum(np.array(self.icount, np.int64))]).astype(np.int64).tolist()
        total = self.ioff[-1]
        keys_a = np.zeros(total, np.uint64)
        for item in range(self.nv * 64):
            if self.icount[item] or mut in ("d_eq_k",):
                cnt, out = self.esu(item, True)
                room = min(len(out), total - self.ioff[item])       # (a mutant that writes more than it counted runs into the next item)
                keys_a[self.ioff[item]:self.ioff[item] + room] = np.array(out[:room], np.uint64)
        keys_b = np.zeros(total, np.uint64)
        dst = keys_a if self.current == "a" else keys_b
        self.routes = []                                             # per root: (n, sorted as a segment, sorted in LDS)
        for vi in range(self.nv):
            b0, b1 = self.ioff[vi * 64], self.ioff[vi * 64 + 64]
            large = (b1 - b0 >= SMALL_SORT) if mut == "seg_ge" else (b1 - b0 > SMALL_SORT)
            if large:
                dst[b0:b1] = np.sort(keys_a[b0:b1])
            self.routes.append([b1 - b0, large, False])
        for vi in range(self.nv):
            b0 = self.ioff[vi * 64]
            n = self.ioff[vi * 64 + 64] - b0
            if n <= 1 or ((n >= SMALL_SORT) if mut == "small_ge" else (n > SMALL_SORT)):
                if n == 1 and dst is not keys_a and mut != "no_copy_1":
                    dst[b0] = keys_a[b0]
                continue
            self.routes[vi][2] = True
            dst[b0:b0 + n] = self.bitonic(keys_a[b0:b0 + n])
        self.keys_sorted = dst
        self.gstart, self.gsize = [0] * self.G, [0] * self.G
        for g, (_, n, vbase, en) in enumerate(self.graphs):
            if en:
                self.gstart[g] = self.ioff[vbase * 64]
                self.gsize[g] = self.ioff[(vbase + n) * 64] - self.gstart[g]

    # ---- the generator and the draws ----
    @staticmethod
    def mt_step(x, xnext, far):
        y = (x & 0xFFFFFFFF80000000) | (xnext & 0x7FFFFFFF)
        return far ^ (y >> 1) ^ (0xB5026F5AA96619E9 if y & 1 else 0)

    def mt_twist(self, mt):
        mut, step = self.mutant, self.mt_step
        cell = lambda i: mt[i] if i < MT_N else 0                    # noqa: E731  (the LDS word behind mt[])
        r = [step(mt[i], mt[i + 1], mt[i + MT_M]) for i in range(MT_M)]
        mt[:MT_M] = r
        end2 = MT_N if mut == "twist2_to_N" else MT_N - 1
        r = [step(mt[i], cell(i + 1), mt[i - MT_M]) for i in range(MT_M, end2)]
        mt[MT_M:end2] = r
        mt[MT_N - 1] = step(mt[MT_N - 1], mt[0], mt[MT_M] if mut == "twist3_mt_M" else mt[MT_M - 1])

    def mt_seed(self, seed):
        x = seed & M64
        mt = [x]
        for i in range(1, MT_N):
            x = (6364136223846793005 * (x ^ (x >> 62)) + i) & M64
            mt.append(x)
        self.mt_twist(mt)
        return mt

    @staticmethod
    def mt_temper(y):
        y ^= (y >> 29) & 0x5555555555555555
        y ^= (y << 17) & 0x71D67FFFEDA60000 & M64
        y ^= (y << 37) & 0xFFF7EEE000000000 & M64
        return (y ^ (y >> 43)) & M64

    def mt_draws(self, mt, total, size_of, out, base):
        pos, d0 = 0, 0
        while d0 < total:
            todo = min(total - d0, MT_N - pos)
            first, r = DRAW_BLOCK, []
            for tid in range(todo):
                N = size_of(d0 + tid)
                x = self.mt_temper(mt[pos + tid])
                lo = (x * N) & M64
                if lo < N and lo < ((1 << 64) - N) % N and first == DRAW_BLOCK:
                    first = tid
                r.append((x * N) >> 64)
            for tid in range(min(todo, first)):
                out[base + d0 + tid] = r[tid]
            taken = first if first < todo else todo
            d0 += taken
            pos += taken + (1 if first < todo else 0)
            if pos == MT_N:
                if self.mutant != "pos_wrap_no_twist":
                    self.mt_twist(mt)
                pos = 0

    def draw(self, m, seed):
        """uni_draw: nepos, ne_list by the block-wide compaction, then the call's draws from one generator."""
        G = self.G
        self.nepos, self.ne_list, self.draws = [0] * G, [0] * G, [0] * (G * m)
        s_ne = 0
        for g0 in range(0, G, DRAW_BLOCK):
            flag = [1 if g0 + t < G and self.gsize[g0 + t] > 0 else 0 for t in range(DRAW_BLOCK)]
            scan = np.cumsum(flag).tolist()                          # the Hillis-Steele scan's result
            base = 0 if self.mutant == "no_carry" else s_ne
            for t in range(DRAW_BLOCK):
                g = g0 + t
                if g < G:
                    pos = base + scan[t] - flag[t]
                    self.nepos[g] = pos if flag[t] else -1
                    if flag[t]:
                        self.ne_list[pos] = g
            s_ne = base + scan[-1]
        total = s_ne * m
        if total == 0:
            return
        self.mt_draws(self.mt_seed(seed), total, lambda d: self.gsize[self.ne_list[d // m]], self.draws, 0)

    def draw_graphs(self, m, seeds):
        """uni_draw_graphs: workgroup g, its own generator, draws[g * m ...]"""
        self.draws = [0] * (self.G * m)
        if m == 0:
            return
        for g in range(self.G):
            N = self.gsize[g]
            if N == 0:
                continue
            self.mt_draws(self.mt_seed(int(seeds[g])), m, lambda d: N, self.draws, g * m)

    # ---- rows and fill (uni_rows / uni_fill and uni_enum_rows / uni_enum_fill decode alike) ----
    def rows_and_fill(self, row_graph, row_mask, mode):
        """nodes, edge_index, edge_ptr, edge_src of rows given as (graph, mask); mask 0: a row of -1."""
        k, mut = self.k, self.mutant
        R = len(row_graph)
        nodes = np.full((R, k), -1, np.int64)
        ecount = np.zeros(R, np.int64)
        per_row = [None] * R
        by_graph = {}
        for row, (g, mask) in enumerate(zip(row_graph, row_mask)):
            if mask:
                by_graph.setdefault(g, []).append(row)
                members = [i for i in range(64) if mask >> i & 1]
                nodes[row, :min(k, len(members))] = [self.graphs[g][0] + v for v in members[:k]]
        bpair, cval2 = np.array(self.bpair, np.int64), np.array(self.cval2, np.int64)
        for g, rws in by_graph.items():
            lo = self.graphs[g][0]
            ps = np.arange(self.cstart[g], self.cstart[g + 1])
            uv = bpair[ps]
            u = uv & (0xFF if mut == "decode_u_ff" else 63)
            v = ((uv >> 6) & 63) if mut == "decode_v_shr6" else uv >> 8
            masks = np.array([row_mask[r] for r in rws], np.uint64)[:, None]
            us, vs = u.astype(np.uint64)[None, :], v.astype(np.uint64)[None, :]
            one = np.uint64(1)
            hit = ((masks >> us) & (masks >> vs) & one).astype(bool)
            if mode == "sample":
                bit_u, bit_v = one << us, one << vs
                if mut != "popc_no_minus1":
                    bit_u, bit_v = bit_u - one, bit_v - one
                eu, ev = popcount(masks & bit_u), popcount(masks & bit_v)
            else:
                eu, ev = np.broadcast_to(lo + u, hit.shape), np.broadcast_to(lo + v, hit.shape)
            es = np.broadcast_to(ps if mut == "cval_for_cval2" else cval2[ps], hit.shape)
            for i, r in enumerate(rws):
                h = hit[i]
                ecount[r] = h.sum()
                per_row[r] = (eu[i][h], ev[i][h], es[i][h])
        eptr = np.concatenate([[0], np.cumsum(ecount)]).astype(np.int64)
        parts = [x for x in per_row if x is not None]
        cat = lambda j: np.concatenate([x[j] for x in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)   # noqa: E731
        return nodes, np.stack([cat(0), cat(1)]), eptr, cat(2)

    # ---- the four calls ----
    def sample(self, m, mode, seed=None, seeds=None):
        self.prepare()
        if seeds is None:
            self.draw(m, seed)
        else:
            self.draw_graphs(m, seeds)
        row_graph, row_mask = [], []
        for row in range(self.G * m):
            g, s = row // m, row % m
            mask = 0
            if self.gsize[g] > 0:
                d = row if seeds is not None else (g if self.mutant == "draw_g_m" else self.nepos[g]) * m + s
                mask = self.mask_of(int(self.keys_sorted[self.gstart[g] + self.draws[d]]))
            row_graph.append(g)
            row_mask.append(mask)
        nodes, eidx, eptr, esrc = self.rows_and_fill(row_graph, row_mask, mode)
        return nodes, eidx, eptr, np.arange(self.G + 1, dtype=np.int64) * m, esrc

    def enumerate(self, mode):
        self.prepare()
        sptr = np.concatenate([[0], np.cumsum(self.gsize)]).astype(np.int64)
        rows = np.arange(sptr[-1])
        row_graph = np.searchsorted(sptr[1:], rows, "right").tolist()  # enum_graph: the first g with sptr[g + 1] > row
        row_mask = [self.mask_of(int(self.keys_sorted[self.gstart[g] + (r - sptr[g])])) for r, g in zip(rows.tolist(), row_graph)]
        nodes, eidx, eptr, esrc = self.rows_and_fill(row_graph, row_mask, mode)
        return nodes, eidx, eptr, sptr, esrc, np.array(self.gsize, np.int64)
