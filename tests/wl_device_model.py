"""wl_device_model.py -- how ugs_wl_hash_kernel and ugs_wl_lookup_kernel (ugs_wl.hip) compute a row, restated in plain Python: lane
groups and the wave's ballot, neighbour masks by OR, 128-bit labels as two 64-bit words, ranks with ties broken by vertex, the
piece stream with its 16 staging words and the deferred compression, and BLAKE2b's F written out from RFC 7693.  Nothing here calls
the library or hashlib.blake2b: tests/test_wl_paths_law.py checks F against hashlib and the model against the law
(tests/wl_law.py, tests/wl_feature_law.py) on the inputs of tests/wl_paths.py.  A helper for the tests, not a test.

`mutant=` switches on one plausible kernel mistake; the inputs of wl_paths.py must tell each from the law:
  compress_at_word15     a block is compressed as soon as its word 15 is stored: a message of 128 bytes ends with an empty block
  t_not_rounded          the counter of a block compressed in mid-message is the stream position, not rounded down to the block
  carry_dropped          the bytes of a piece that straddles a word are lost beyond the word
  finish_no_zero_fill    the last block keeps the words of the block (or message) before behind the message's end
  rank_no_tiebreak       equal labels get the same rank: order[] and cnt[] slots are overwritten, others keep stale values
  cmp_signed             label words compared as signed values
  degree_numeric         the start labels of degree mode ordered as numbers, "2" < "10"
  loop_once              a loop counts 1 towards the degree
  single_item_no_comma   a single Counter item printed without the comma behind it
  hex_quarters_swapped   the four 32-bit quarters of a label printed last first
  slot_is_vertex         label mode takes slot j for vertex j, not the j-th valid slot
  ballot_wave            the valid lanes counted from the group's first lane to the end of the wave
  first_trip_only        only the first trip of the edge loop: entries behind the group's width are dropped
  ptr_unchecked          no edge_ptr check: a bad range is clamped the way Python slices
  endpoint_cast32        the endpoints' range check after a cast to 32 bits
  lookup_ignore_lo       the binary search compares high words only
  lookup_signed          the binary search compares as signed values
  lookup_ignore_status   the lookup answers the table's id whatever the row's status
UNREACHABLE mutants change the result only on labels no input can produce, and are told apart on crafted labels (Model.rank):
  cmp_ignore_lo          the low word ignored in the label comparison: only digests that agree in their first 64 bits differ"""

M64 = (1 << 64) - 1
MUTANTS = ("compress_at_word15", "t_not_rounded", "carry_dropped", "finish_no_zero_fill", "rank_no_tiebreak", "cmp_signed",
           "degree_numeric", "loop_once", "single_item_no_comma", "hex_quarters_swapped", "slot_is_vertex", "ballot_wave",
           "first_trip_only", "ptr_unchecked", "endpoint_cast32")
LOOKUP_MUTANTS = ("lookup_ignore_lo", "lookup_signed", "lookup_ignore_status")
UNREACHABLE = ("cmp_ignore_lo",)
WL_BLOCK, WAVE = 256, 64

# ---- BLAKE2b's compression function F, RFC 7693 section 3.2 ----
IV = (0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
      0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179)
SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
         (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4), (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
         (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13), (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
         (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11), (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
         (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5), (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))
_MIX = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def _rotr(x, r):
    return (x >> r | x << (64 - r)) & M64


def compress(h, m, t, last):
    """F(h, m, t, f): the new chaining value; t < 2^64 bytes."""
    v = list(h) + list(IV)
    v[12] ^= t
    if last:
        v[14] ^= M64
    for r in range(12):
        s = SIGMA[r % 10]
        for i, (a, b, c, d) in enumerate(_MIX):
            v[a] = (v[a] + v[b] + m[s[2 * i]]) & M64
            v[d] = _rotr(v[d] ^ v[a], 32)
            v[c] = (v[c] + v[d]) & M64
            v[b] = _rotr(v[b] ^ v[c], 24)
            v[a] = (v[a] + v[b] + m[s[2 * i + 1]]) & M64
            v[d] = _rotr(v[d] ^ v[a], 16)
            v[c] = (v[c] + v[d]) & M64
            v[b] = _rotr(v[b] ^ v[c], 63)
    return [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]


PIECE, FLUSH, FINISH = 0, 1, 2


class Stream:
    """One unkeyed BLAKE2b-128 stream the kernel's way (wl_stream_step): `stg` are the lane's 16 staging words, which keep what
    the message before left in them."""

    def __init__(self, stg, mutant=None):
        self.h = [IV[0] ^ 0x01010010] + list(IV[1:])
        self.acc, self.pos, self.stg, self.mutant = 0, 0, stg, mutant

    def step(self, what, v=0, n=0):
        mutant, pos = self.mutant, self.pos
        off, widx = pos & 7, (pos >> 3) & 15
        store, word = False, self.acc
        early = mutant == "compress_at_word15"
        if what == PIECE:
            word |= (v << (8 * off)) & M64
            store = off + n >= 8
        elif what == FLUSH:
            store = off != 0
        else:
            used = (((pos - 1) & 127) >> 3) + 1 if pos else 0          # words of the last block that hold message bytes
            if early:
                used = ((pos & 127) + 7) >> 3                          # the full block has gone already
            if mutant != "finish_no_zero_fill":
                for j in range(used, 16):
                    self.stg[j] = 0
        if what == FINISH or (store and widx == 0 and pos >= 128 and not early):
            t = pos if what == FINISH or mutant == "t_not_rounded" else pos & ~127
            self.h = compress(self.h, self.stg, t, what == FINISH)
        if store:
            self.stg[widx] = word
            self.acc = v >> (8 * (8 - off)) if what == PIECE and off != 0 and mutant != "carry_dropped" else 0
            if early and widx == 15:
                self.h = compress(self.h, self.stg, (pos & ~127) + 128, False)
        else:
            self.acc = word
        if what == PIECE:
            self.pos += n

    def text(self, s):
        """A piece given as its characters, first one lowest."""
        self.step(PIECE, int.from_bytes(s.encode("ascii"), "little"), len(s))

    def label(self):
        """Digest bytes 0-7 and 8-15 as big-endian numbers: bswap64 of h[0] and h[1]."""
        return tuple(int.from_bytes(self.h[i].to_bytes(8, "little"), "big") for i in (0, 1))


def _popc(x):
    return bin(x).count("1")


def _signed(x):
    return x - (1 << 64) if x >> 63 else x


def _cast32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


def _decimal(hi):
    """The decimal start label packed into the top bytes of the high word, as its characters."""
    return chr(hi >> 56) + (chr(hi >> 48 & 0xff) if hi >> 48 & 0xff else "")


def _hex_word(hi, lo, p, mutant=None):
    """32-bit quarter p = 0..3 of the label, most significant first, as 8 hex characters."""
    if mutant == "hex_quarters_swapped":
        p = 3 - p
    w = hi if p < 2 else lo
    return "%08x" % ((w if p & 1 else w >> 32) & 0xffffffff)


class Model:
    """One launch of ugs_wl_hash_kernel over nodes [S, k], edge_index [2, E] (row 1 at edge_index[1]), edge_ptr [S + 1]."""

    def __init__(self, nodes, edge_index, edge_ptr, iterations, labels=None, num_labels=None, num_cols=None, mutant=None):
        self.nodes = [[int(x) for x in row] for row in nodes]
        self.src, self.dst = [int(x) for x in edge_index[0]], [int(x) for x in edge_index[1]]
        self.ptr = [int(x) for x in edge_ptr]
        self.T, self.mutant = iterations, mutant
        self.labeled = labels is not None
        self.labels = [int(x) for x in labels] if self.labeled else []
        self.num_labels = len(self.labels) if num_labels is None else num_labels
        self.num_cols = len(self.src) if num_cols is None else num_cols
        self.k = len(self.nodes[0])
        self.wshift = 3 if self.k <= 8 else 4 if self.k <= 16 else 5

    def less_eq(self, a, b, t):
        """(a < b, a == b) for labels (hi, lo) of ranking step t."""
        mutant = self.mutant
        if mutant == "degree_numeric" and t == 0 and not self.labeled:
            a, b = (int(_decimal(a[0])), 0), (int(_decimal(b[0])), 0)
        if mutant == "cmp_signed":
            a, b = tuple(map(_signed, a)), tuple(map(_signed, b))
        if mutant == "cmp_ignore_lo":
            return a[0] < b[0], a[0] == b[0]
        return a[0] < b[0] or (a[0] == b[0] and a[1] < b[1]), a == b

    def rank(self, lab, order, cnt, t):
        """order[rank] = vertex and cnt[rank] = multiplicity at the first of equal labels, written lane after lane."""
        n = len(lab)
        for u in range(n):
            rank = eq_before = eq_all = 0
            for v in range(n):
                less, eq = self.less_eq(lab[v], lab[u], t)
                tie = eq and v < u and self.mutant != "rank_no_tiebreak"
                rank += 1 if less or tie else 0
                eq_before += 1 if eq and v < u else 0
                eq_all += 1 if eq else 0
            order[rank] = u
            cnt[rank] = eq_all if eq_before == 0 else 0

    def row(self, i):
        """(hexdigest or None, status) of row i."""
        mutant, k, T = self.mutant, self.k, self.T
        W = 1 << self.wshift
        per_block, per_wave = WL_BLOCK >> self.wshift, WAVE >> self.wshift
        g = i % per_block
        first = i - g % per_wave                       # the row of the wave's first group
        gshift = (g % per_wave) * W
        ballot = 0
        for r in range(first, min(first + per_wave, len(self.nodes))):
            for u in range(k):
                if self.nodes[r][u] >= 0:
                    ballot |= 1 << ((r - first) * W + u)
        gmask = (1 << W) - 1
        mine = (ballot >> gshift) & gmask
        n = _popc(mine)
        if mutant == "ballot_wave":
            n = min(_popc(ballot >> gshift), W)
        mask, bad = [0] * W, False
        if n > 0:
            lo, hi = self.ptr[i], self.ptr[i + 1]
            if mutant == "ptr_unchecked":
                lo, hi, _ = slice(lo, hi).indices(self.num_cols)
            if lo < 0 or hi < lo or hi > self.num_cols:
                bad = True
            else:
                for u in range(W):
                    for e in range(lo + u, hi, W):
                        if mutant == "first_trip_only" and e >= lo + W:
                            break
                        x, y = self.src[e], self.dst[e]
                        if mutant == "endpoint_cast32":
                            x, y = _cast32(x), _cast32(y)
                        if x < 0 or x >= n or y < 0 or y >= n:
                            bad = True
                        else:
                            mask[x] |= 1 << y
                            mask[y] |= 1 << x
        lab = [(0, 0)] * W
        norange = False
        if self.labeled:
            for u in range(k):
                if mine >> u & 1:
                    idv = self.nodes[i][u]
                    l = self.labels[idv] if idv < self.num_labels else -1
                    if l < 0 or l > 0xffffffff:
                        norange = True
                    else:
                        j = u if mutant == "slot_is_vertex" else _popc(mine & ((1 << u) - 1))
                        lab[j] = (l << 32, 0)
        st = 1 if n == 0 else 2 if bad else 3 if norange else 0
        if st:
            return None, st
        if not self.labeled:
            for u in range(n):
                d = str(_popc(mask[u]) + (mask[u] >> u & 1 if mutant != "loop_once" else 0))
                lab[u] = (ord(d[0]) << 56 | (ord(d[1]) << 48 if len(d) == 2 else 0), 0)
        lab = lab[:n]
        order, cnt = [0] * W, [0] * W
        stg = [[0] * 16 for _ in range(n)]             # a lane's staging words outlive its messages
        fs = Stream([0] * 16, mutant)
        nitems = 0
        for t in range(T + 1):
            self.rank(lab, order, cnt, t)
            items = n if t >= 1 else 0
            for r in range(items + (1 if t == T else 0)):
                if r == items:
                    fs.text("()" if nitems == 0 else (")" if mutant == "single_item_no_comma" else ",)") if nitems == 1 else ")")
                    fs.step(FLUSH)
                    fs.step(FINISH)
                    continue
                if cnt[r] == 0:
                    continue
                hi, lo = lab[order[r]]
                fs.text("(('" if nitems == 0 else ", ('")
                for p in range(4):
                    fs.text(_hex_word(hi, lo, p, mutant))
                fs.text("', %d)" % cnt[r])
                nitems += 1
            if t == T:
                break
            new = []
            for u in range(n):
                s = Stream(stg[u], mutant)
                for li in range(n + 1):
                    w = u if li == 0 else order[li - 1]
                    if li > 0 and not mask[u] >> w & 1:
                        continue
                    hi, lo = lab[w]
                    if t == 0 and not self.labeled:
                        s.text(_decimal(hi))
                    elif t == 0:
                        s.text(_hex_word(hi, lo, 0))
                    else:
                        for p in range(4):
                            s.text(_hex_word(hi, lo, p, mutant))
                s.step(FLUSH)
                s.step(FINISH)
                new.append(s.label())
            lab = new
        return "%016x%016x" % fs.label(), 0

    def rows(self):
        """(hexdigests, statuses) of the launch."""
        got = [self.row(i) for i in range(len(self.nodes))]
        return [h for h, _ in got], [s for _, s in got]


def lookup(keys, ids, digests, statuses, unknown, mutant=None):
    """ugs_wl_lookup_kernel: keys [(hi, lo), ...] ascending as 128-bit values, digests [(hi, lo), ...]: the rows' ids."""
    conv = _signed if mutant == "lookup_signed" else (lambda x: x)
    out = []
    for (hi, lo), st in zip(digests, statuses):
        got = unknown
        if st == 0 or mutant == "lookup_ignore_status":
            a, b = 0, len(keys)
            while a < b:
                mid = a + ((b - a) >> 1)
                kh, kl = keys[mid]
                if conv(kh) < conv(hi) or (kh == hi and conv(kl) < conv(lo) and mutant != "lookup_ignore_lo"):
                    a = mid + 1
                else:
                    b = mid
            if a < len(keys) and keys[a] == (hi, lo):
                got = ids[a]
        out.append(got)
    return out
