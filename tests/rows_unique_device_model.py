"""rows_unique_device_model.py -- csrc/ugs_rows.hip restated the way the device computes it, in plain Python and numpy, with the
single-line slips (`MUTANTS`) that tests/test_rows_unique_paths_law.py tells from the law on named inputs.  No GPU, no library call.

`run(case, by, mutant)` goes through the seven kernels in launch order over a model of the call's blob:

  check    the grid of min(ceil((max(R, G) + 1) / 256), 4096) workgroups of 256 striding over the indices in trips; status words
           by minimum; the lists of graphs of 65..256, 257..1024 and 1025..4096 rows; the count of graphs of 1..64 rows
  keys     per row: its graph by the kernel's binary search, its codes, and the key as two 64-bit words built by or_shl, a field
           across bit 64 in two parts; the unrolled form (k <= 8) holds the codes, the looped form computes them again per compare
  wave     64 lanes: every lane compares its key with lane j's for j < n, the lowest equal lane is the representative; rank by
           the ballot's bits below the lane; inclusive scan of the kept rows' edge entries; the total read from lane 63
  block    pairs (x, y, z, w, row) padded to pn with (all ones, 2^32 - 1); the bitonic network, every stage as the kernel indexes it;
           lower and upper bound of a pair's key by binary search over the sorted pairs; the scatter back by row into the x and y
           arrays; four rows a thread; block_scan2 with a wave's inclusive scan and the totals of the earlier waves
  scan     1024 graphs a pass, the totals of the passes before carried on
  compact  one lane a row, as rows_compact; edges: 16 lanes a kept row, 16 entries a trip

and returns ("refused", word, value) or ("ok", form, the seven arrays).  What no kernel wrote keeps the blob's start values (a
row its own representative, zeros elsewhere) and -7 in the outputs, so that a skipped graph or entry shows.  An index outside an
array raises IndexError, as numpy's own negative indices would not: the caller counts that as told apart.

Shifts are mathematical and the key is cut to 128 bits; where a slip shifts by 64 or more the model says so at the mutant.

Slips that cannot change any output, and so are no mutants:
  - comparing the key words as signed numbers in pair_gt: the sort order changes, consistently in the network and in both binary
    searches, and only equality of keys and the order of rows within a run (by row number, below 2^31) reach an output;
  - the wave total taken from lane n - 1 instead of lane 63: lanes n .. 63 add 0 to the inclusive scan;
  - `rank_no_tiebreak` (the rank of a code counts smaller codes only): equal codes land on one field and OR to themselves, the
    fields behind stay 0, and the key still determines the multiset -- a code's multiplicity is the distance to the next
    non-zero field, the leading zeros are the multiplicity of -1 -- so equal sets keep equal keys and different sets different
    ones.  It is kept as `EQUIVALENT`, and the CPU test asserts that it equals the law on every case;
  - the edge copy's trip taken as 8 with 16 lanes: lanes 8 .. 15 write again what lanes 0 .. 7 reach a trip later.
"""
import numpy as np

import rows_unique_law as L

M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1
NONE = 0x7f7f7f7f7f7f7f7f
STALE = -7

MUTANTS = {
    # keys
    "straddle_hi_dropped": "or_shl without `hi |= v >> (64 - s)`: the high part of a field across bit 64 is lost",
    "field_at_64_into_lo": "or_shl tests `s <= 64`: at s == 64 the hardware shifts by s & 63 = 0, the field is ORed onto field 0 as well",
    "code_without_plus_one": "rows_code returns d, not d + 1: a graph's first vertex codes like -1",
    "below_lo_unchecked": "rows_code without `d < 0`: an entry below its graph passes, ptr[g] - 1 with the code of -1",
    "cast32_before_check": "rows_code narrows d to 32 bits before `d >= n`: ptr[g] + 2^32 passes as the first vertex",
    "rank_tie_le": "`j <= i` in the rank's tie-break: every rank one too high, the highest field shifted past bit 127 where (k + 1) b > 128",
    "graph_search_first_of_equal": "`sample_ptr[mid] >= r` in the search for the row's graph: the first row of a graph goes to the graph before",
    # wave
    "wave_rep_last": "the representative is the last equal lane, not the first",
    # block
    "pad_row_zero": "padding pairs carry row 0, not 2^32 - 1: they sort in front of the rows whose key is all ones",
    "pad_key_zero": "padding pairs carry key 0: they sort to the front and push rows out of the first n positions",
    "upper_bound_to_pn": "the upper bound searched up to pn: a run of the all-ones key counts the padding",
    "sort_ignores_row": "pair_gt without the row as last word: the network is not stable, a run's first pair need not be its lowest row",
    "cmp_skips_x": "pair_gt without the x word (bits 0..31)", "cmp_skips_y": "pair_gt without the y word (bits 32..63)",
    "cmp_skips_z": "pair_gt without the z word (bits 64..95)", "cmp_skips_w": "pair_gt without the w word (bits 96..127)",
    "block_scan_without_earlier_waves": "block_scan2 in rows_block leaves out the totals of the waves before the thread's own",
    # scan
    "scan_carry_dropped": "rows_scan writes a pass's offsets without the totals of the passes before",
    # edges
    "edges_one_trip": "rows_edges copies `if (lane < len)` once, no loop: at most 16 entries a row",
    "edges_stride_8": "rows_edges takes the lane as `threadIdx.x & 7` with the trip still 16: entries 8..15 of every trip stay unwritten",
    # check
    "check_one_trip": "rows_check without its grid-stride loop: indices from 2^20 on are never looked at",
    "class_bound_le_256": "`rows < 256` for the first class: a graph of exactly 256 rows is listed for the 1024-pair kernel, whose grid is R / 257",
    "class_bound_le_1024": "`rows < 1024` for the second class: a graph of exactly 1024 rows is listed for the 4096-pair kernel, whose grid is R / 1025",
    "small_bound_lt_64": "`rows >= 64` for the workgroup form's lists: a graph of 64 rows is listed there and not counted for the wave form",
    "status_max_instead_of_min": "the status words keep the highest offender, not the lowest",
}
EQUIVALENT = {"rank_no_tiebreak": "the key still determines the multiset (module docstring)"}


def at(a, i):
    if not 0 <= i < len(a):
        raise IndexError("%d outside [0, %d)" % (i, len(a)))
    return a[i]


def put(a, i, v):
    if not 0 <= i < len(a):
        raise IndexError("%d outside [0, %d)" % (i, len(a)))
    a[i] = v


class Call:
    """The inputs and the blob of one call."""
    def __init__(self, case, by):
        self.nodes, self.ei, self.eptr, self.sptr, self.esrc, self.ptr = L._as_case(case)
        self.R, self.k = self.nodes.shape
        self.G, self.Es = len(self.sptr) - 1, self.ei.shape[1]
        self.by, self.bits = by == "set", L.key_bits(self.k)
        R, G = self.R, self.G
        self.keys = [(0, 0, 0, 0)] * R
        self.rowg = np.zeros(R, np.int64)
        self.rep = np.arange(R, dtype=np.int64)
        self.lrank, self.cnt, self.eoff = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
        self.ug, self.eg = np.zeros(G, np.int64), np.zeros(G, np.int64)
        self.ubase, self.ebase = np.zeros(G + 1, np.int64), np.zeros(G + 1, np.int64)
        self.big, self.small = [[], [], []], 0
        self.status = {"ptr": [], "graph": [], "entry": []}


def status_of(c, word, mut):
    found = c.status[word]
    if not found:
        return NONE
    return max(found) if mut == "status_max_instead_of_min" else min(found)


# ---- rows_check ----
def check(c, mut):
    top = max(c.R, c.G)
    grid = min((top + 1 + 255) // 256, L.CHECK_GRID)
    stride = grid * L.CHECK_BLOCK
    sptr, eptr, ptr = c.sptr, c.eptr, c.ptr
    for base in range(0, top + 1, stride):
        if base > 0 and mut == "check_one_trip":
            break
        i = np.arange(base, min(base + stride, top + 1))
        if base == 0:
            if sptr[0] != 0:
                c.status["ptr"].append(0)
            if sptr[c.G] != c.R:
                c.status["ptr"].append(4 * c.G)
            if eptr[0] != 0:
                c.status["ptr"].append(1)
            if eptr[c.R] != c.Es:
                c.status["ptr"].append(4 * c.R + 1)
        m = i[i < c.R]
        c.status["ptr"] += (4 * m[eptr[m] > eptr[m + 1]] + 1).tolist()
        g = i[i < c.G]
        a, b, lo, hi = sptr[g], sptr[g + 1], ptr[g], ptr[g + 1]
        c.status["ptr"] += (4 * g[a > b]).tolist() + (4 * g[lo > hi] + 2).tolist()
        rows = b - a
        over = (rows > 0) & (rows > L.MAX_ROWS_PER_GRAPH)
        overv = (rows > 0) & ~over & (hi - lo + 1 > (1 << c.bits))
        c.status["graph"] += (2 * g[over]).tolist() + (2 * g[overv] + 1).tolist()
        rest = (rows > 0) & ~over & ~overv
        isbig = rest & ((rows >= 64) if mut == "small_bound_lt_64" else (rows > 64))
        in0 = (rows < 256) if mut == "class_bound_le_256" else (rows <= 256)
        in1 = (rows < 1024) if mut == "class_bound_le_1024" else (rows <= 1024)
        cls = np.where(in0, 0, np.where(in1, 1, 2))
        for k in range(3):
            c.big[k] += g[isbig & (cls == k)].tolist()
        c.small += int((rest & ~isbig).sum())


# ---- rows_keys ----
def or_shl(lo, hi, code, s, mut):
    v = code
    if s < 64 or (s == 64 and mut == "field_at_64_into_lo"):
        lo |= (v << (s & 63)) & M64
        if s > 0 and mut != "straddle_hi_dropped":
            hi |= v >> ((64 - s) & 63)
    else:
        hi |= (v << (s - 64)) & M64
    return lo, hi


def rows_code(v, lo, n, mut):
    """(code, bad)"""
    if v == -1:
        return 0, False
    d = v - lo
    if mut == "cast32_before_check":
        d &= M32
    below = d < 0 and mut != "below_lo_unchecked"
    if v < -1 or below or d >= n:
        return 0, True
    return ((d if mut == "code_without_plus_one" else d + 1) & M32), False


def graph_of_row(c, r, mut):
    a, b = 1, c.G
    while a < b:
        mid = a + ((b - a) >> 1)
        v = int(at(c.sptr, mid))
        if (v >= r) if mut == "graph_search_first_of_equal" else (v > r):
            b = mid
        else:
            a = mid + 1
    return a - 1


def rank_of(ci, i, cj, j, mut):
    return 1 if cj < ci or (cj == ci and mut != "rank_no_tiebreak" and ((j <= i) if mut == "rank_tie_le" else (j < i))) else 0


def keys(c, mut):
    k, bits = c.k, c.bits
    for r in range(c.R):
        g = graph_of_row(c, r, mut)
        lo = int(at(c.ptr, g))
        n = int(at(c.ptr, g + 1)) - lo
        row = [int(v) for v in c.nodes[r]]
        bad, klo, khi = False, 0, 0
        if k <= 8:                                   # the unrolled form: codes held
            code = []
            for i in range(k):
                ci, b = rows_code(row[i], lo, n, mut)
                bad |= b
                code.append(ci)
            for i in range(k):
                pos = i
                if c.by:
                    pos = sum(rank_of(code[i], i, code[j], j, mut) for j in range(k))
                klo, khi = or_shl(klo, khi, code[i], pos * bits, mut)
        else:                                        # the looped form: the row read again for every compare
            for i in range(k):
                ci, b = rows_code(row[i], lo, n, mut)
                bad |= b
                pos = i
                if c.by:
                    pos = 0
                    for j in range(k):
                        cj, _ = rows_code(row[j], lo, n, mut)
                        pos += rank_of(ci, i, cj, j, mut)
                klo, khi = or_shl(klo, khi, ci, pos * bits, mut)
        if bad:
            c.status["entry"].append(r)
        c.keys[r] = (klo & M32, klo >> 32, khi & M32, khi >> 32)
        c.rowg[r] = g


# ---- rows_wave ----
def wave_graph(c, g, mut):
    r0 = int(c.sptr[g])
    n = int(c.sptr[g + 1]) - r0
    if n > 64:
        return
    if n == 0:
        c.ug[g] = c.eg[g] = 0
        return
    key = [at(c.keys, r0 + l) if l < n else (0, 0, 0, 0) for l in range(64)]
    elen = [int(c.eptr[r0 + l + 1] - c.eptr[r0 + l]) if l < n else 0 for l in range(64)]
    rep, cnt = [-1] * 64, [0] * 64
    for lane in range(64):
        for j in range(n):
            if key[j] == key[lane]:
                if rep[lane] < 0 or mut == "wave_rep_last":
                    rep[lane] = j
                cnt[lane] += 1
    kept = [l < n and rep[l] == l for l in range(64)]
    mask = sum(1 << l for l in range(64) if kept[l])
    e = [elen[l] if kept[l] else 0 for l in range(64)]
    incl = list(np.cumsum(e))
    for l in range(n):
        r = r0 + l
        put(c.rep, r, r0 + rep[l])
        if kept[l]:
            c.lrank[r] = bin(mask & ((1 << l) - 1)).count("1")
            c.cnt[r] = cnt[l]
            c.eoff[r] = incl[l] - e[l]
    c.ug[g] = bin(mask).count("1")
    c.eg[g] = incl[63]


def wave(c, mut):
    c.ug[:] = 0                                      # what the lanes 0 of the empty graphs write; the others follow one by one
    c.eg[:] = 0
    rows = c.sptr[1:] - c.sptr[:-1]
    for g in np.nonzero(rows != 0)[0]:               # wave g % 4 of workgroup g // 4; the last workgroup may be partly filled
        wave_graph(c, int(g), mut)


# ---- rows_block ----
SKIP = {"cmp_skips_x": 0, "cmp_skips_y": 1, "cmp_skips_z": 2, "cmp_skips_w": 3}


def words_of(mut, with_row):
    order = [w for w in (3, 2, 1, 0) if SKIP.get(mut) != w]
    return order + [4] if with_row and mut != "sort_ignores_row" else order


def pair_gt(a, b, order):
    """a > b over the words in `order`, highest first; a and b are sequences (x, y, z, w, row)"""
    for w in order:
        if a[w] != b[w]:
            return a[w] > b[w]
    return False


def pair_gt_many(a, b, order):
    res = np.zeros(len(a[0]), bool)
    open_ = np.ones(len(a[0]), bool)
    for w in order:
        ne = open_ & (a[w] != b[w])
        res[ne] = a[w][ne] > b[w][ne]
        open_ &= ~ne
    return res


def block_graph(c, g, P, mut):
    NT = P // 4
    r0 = int(c.sptr[g])
    n = int(c.sptr[g + 1]) - r0
    if n <= 64 or n > P:
        return
    pn = 128
    while pn < n:
        pn <<= 1
    lds = np.zeros((5, P), np.int64)                 # kx, ky, kz, kw, kr
    for p in range(pn):
        key = (0, 0, 0, 0) if mut == "pad_key_zero" else (M32, M32, M32, M32)
        if p < n:
            key = at(c.keys, r0 + p)
        lds[0:4, p] = key
        lds[4, p] = p if p < n else (0 if mut == "pad_row_zero" else M32)
    sort_order = words_of(mut, True)
    t = np.arange(pn >> 1)
    size = 2
    while size <= pn:
        stride = size >> 1
        while stride > 0:
            i = 2 * t - (t & (stride - 1))
            j = i + stride
            up = (i & size) == 0
            a, b = lds[:, i], lds[:, j]
            swap = pair_gt_many(a, b, sort_order) == up
            lds[:, i[swap]], lds[:, j[swap]] = b[:, swap], a[:, swap]
            stride >>= 1
        size <<= 1
    find_order = words_of(mut, False)
    end = pn if mut == "upper_bound_to_pn" else n
    mine = []
    for p in range(n):                               # p = tid + it * NT over the threads and their four turns
        me = lds[:, p]
        lo, hi = 0, p
        while lo < hi:
            mid = (lo + hi) >> 1
            if pair_gt(me, lds[:, mid], find_order):
                lo = mid + 1
            else:
                hi = mid
        first = lo
        lo, hi = p + 1, end
        while lo < hi:
            mid = (lo + hi) >> 1
            if pair_gt(lds[:, mid], me, find_order):
                hi = mid
            else:
                lo = mid + 1
        mine.append((int(lds[4, p]), int(lds[4, first]), lo - first))
    for my_row, my_rep, my_cnt in mine:
        if my_row != M32:
            put(lds[0], my_row, my_rep)
            put(lds[1], my_row, my_cnt)
    kx, ky = lds[0], lds[1]
    kept = np.zeros(4 * NT, bool)
    length = np.zeros(4 * NT, np.int64)
    for lr in range(min(n, 4 * NT)):
        if kx[lr] == lr:
            kept[lr] = True
            length[lr] = c.eptr[r0 + lr + 1] - c.eptr[r0 + lr]
    kc, ke = kept.reshape(NT, 4).sum(axis=1), length.reshape(NT, 4).sum(axis=1)
    ia, ib = np.cumsum(kc.reshape(-1, 64), axis=1), np.cumsum(ke.reshape(-1, 64), axis=1)     # a wave's inclusive scans
    wt = np.stack([ia[:, 63], ib[:, 63]])
    for tid in range(NT):
        w, lane = tid >> 6, tid & 63
        ba, bb = (0, 0) if mut == "block_scan_without_earlier_waves" else (int(wt[0, :w].sum()), int(wt[1, :w].sum()))
        ec, ee = ba + int(ia[w, lane]) - int(kc[tid]), bb + int(ib[w, lane]) - int(ke[tid])
        for it in range(4):
            lr = 4 * tid + it
            if lr < n:
                r = r0 + lr
                put(c.rep, r, r0 + int(kx[lr]))
                if kept[lr]:
                    c.lrank[r], c.cnt[r], c.eoff[r] = ec, int(ky[lr]), ee
                    ec += 1
                    ee += int(length[lr])
    c.ug[g], c.eg[g] = int(wt[0].sum()), int(wt[1].sum())


def block(c, mut):
    for cls, (P, least) in enumerate(zip(L.CLASS_BOUNDS, (65, 257, 1025))):
        grid = min(c.G, c.R // least)                # as the host sizes it; not launched at 0
        many = len(c.big[cls])
        for bid in range(grid):
            for idx in range(bid, many, grid):
                block_graph(c, c.big[cls][idx], P, mut)


# ---- rows_scan ----
def scan(c, mut):
    cu = ce = 0
    for base in range(0, c.G, L.SCAN_PASS):
        u, e = c.ug[base:base + L.SCAN_PASS], c.eg[base:base + L.SCAN_PASS]
        keep = mut != "scan_carry_dropped"
        c.ubase[base:base + len(u)] = (cu if keep else 0) + np.cumsum(u) - u
        c.ebase[base:base + len(e)] = (ce if keep else 0) + np.cumsum(e) - e
        cu += int(u.sum())
        ce += int(e.sum())
    c.ubase[c.G], c.ebase[c.G] = cu, ce
    return cu, ce


# ---- rows_compact, rows_edges ----
def compact(c, U, Eu, mut):
    k = c.k
    nodes_u = np.full((U, k), STALE, np.int64)
    edge_ptr_u, count, inverse = np.full(U + 1, STALE, np.int64), np.full(U, STALE, np.int64), np.full(c.R, STALE, np.int64)
    sample_ptr_u = c.ubase.copy()                    # lanes 0 .. G
    edge_ptr_u[U] = Eu
    for i in range(c.R):
        g = int(c.rowg[i])
        rp = int(c.rep[i])
        u = int(at(c.ubase, g)) + int(at(c.lrank, rp))
        inverse[i] = u
        if rp != i:
            continue
        put(count, u, c.cnt[i])
        put(edge_ptr_u, u, int(c.ebase[g]) + int(c.eoff[i]))
        put(nodes_u, u, c.nodes[i])
    edge_index_u = np.full((2, Eu), STALE, np.int64)
    edge_src_u = np.full(Eu if c.esrc.size else 0, STALE, np.int64)
    if Eu > 0 and c.R > 0:
        lanes = 8 if mut == "edges_stride_8" else L.EDGE_LANES
        for r in range(c.R):
            if c.rep[r] != r:
                continue
            frm, length = int(c.eptr[r]), int(c.eptr[r + 1] - c.eptr[r])
            to = int(c.ebase[c.rowg[r]]) + int(c.eoff[r])
            for lane in range(lanes):
                e = lane
                while e < length:
                    put(edge_index_u[0], to + e, at(c.ei[0], frm + e))
                    put(edge_index_u[1], to + e, at(c.ei[1], frm + e))
                    if c.esrc.size:
                        put(edge_src_u, to + e, at(c.esrc, frm + e))
                    e += L.EDGE_LANES
                    if mut == "edges_one_trip":
                        break
    return nodes_u, edge_index_u, edge_ptr_u, sample_ptr_u, edge_src_u, count, inverse


def run(case, by, mut=None):
    assert mut is None or mut in MUTANTS or mut in EQUIVALENT, mut
    c = Call(case, by)
    check(c, mut)
    for word in ("ptr", "graph"):
        if status_of(c, word, mut) != NONE:
            return "refused", word, status_of(c, word, mut)
    keys(c, mut)
    if status_of(c, "entry", mut) != NONE:
        return "refused", "entry", status_of(c, "entry", mut)
    if c.G > 0:
        wave(c, mut)
    block(c, mut)
    U, Eu = scan(c, mut)
    nbig = sum(len(b) for b in c.big)
    form = ("wave+workgroup" if c.small else "workgroup") if nbig else "wave" if c.small else "none"
    return "ok", form, compact(c, U, Eu, mut)
