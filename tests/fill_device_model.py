"""fill_device_model.py -- what the row-reading fill and the scan folded into it do on the device (fill_row, ugs_fill and
ugs_fill_scan in ss-gnn_amd/csrc/ugs_kernels.hip, and the 8-row sums of ugs_walk_lds), lane by lane in Python, with one-line
mutants.  tests/test_fill_law.py requires the unmutated model to equal the law (tests/fill_law.py) on every input of
tests/fill_paths.py and every mutant to differ on at least one: the inputs the GPU tests run can see those slips."""
import numpy as np

import fill_law as L

EMPTY = 0xFFFFFFFF          # kEmpty: what an idle lane holds in place of a neighbour
SV_PAD, PS_PAD = 0xFFFFFFFE, 0xFFFFFFFF   # register sentinels of the k <= 8 form: match no vertex and no idle lane / below no entry
GUARD = -7

FILL_MUTANTS = ("row_of_entry_lt", "sub_break_gt", "sub_break_early", "prefix_includes_own_lane", "w_off_by_lanes", "capacity_le",
                "graph_mode_row", "batch_mode_absolute_row", "sv_pad_is_empty", "chunk_of_3_sub_chunks")
SCAN_MUTANTS = ("before_le_tile", "trip_2047", "trip_2049", "tail_words_dropped", "tile_stride_plus_1", "tile_stride_minus_1",
                "write_lt", "sums_of_7_rows", "wide_sums_one_wave")
# mutants no output can tell from the kernel, with the reason (test_fill_law.py asserts that they change nothing)
EQUIVALENT = {
    "sub_break_gt": "a sub-chunk that begins exactly at T has no active lane: its ballot is 0, nothing is written and w_off stays -- "
                    "the break only saves the ballot",
    "tile_stride_minus_1": "a stride one short of the grid still reaches every tile; some tiles are computed twice, by two blocks that "
                           "write the same words",
}


def flat_csr(adj):
    """The law's adjacency lists as the arrays the kernel reads: rowptr, (neighbour, column) per entry"""
    rowptr, nbr, col = [0], [], []
    for entries in adj:
        nbr += [w for w, _ in entries]
        col += [c for _, c in entries]
        rowptr.append(len(nbr))
    return rowptr, nbr, col


class Out:
    """edge_index [2, ld] and edge_src [ld] as the flat buffers the kernel is handed, with guard words behind both"""

    def __init__(self, ld, guard=8):
        self.ld = ld
        self.ei = [GUARD] * (2 * ld + guard)
        self.es = [GUARD] * (ld + guard)

    def store(self, buf, idx, val):
        if 0 <= idx < len(buf):          # (a store past the guard words would be a fault on the device: the guards already tell)
            buf[idx] = val

    def guards_intact(self):
        return all(x == GUARD for x in self.ei[2 * self.ld:]) and all(x == GUARD for x in self.es[self.ld:])

    def edges(self, total):
        n = min(total, self.ld)
        return self.ei[:n], self.ei[self.ld:self.ld + n], self.es[:n]


def model_fill_row(graph, row, k, GS, e0, out, mode, i, row_abs, row_rel, extra=0, mutant=None):
    """fill_row<GS> for one complete row: returns w_off behind the row's last hit."""
    rowptr, nbr, col = graph
    ld = out.ld
    SV = [int(v) - extra for v in row]                     # (the kernel holds graph-local ids: the same numbers less the graph's first)
    R0 = [rowptr[u] for u in SV]
    PS = [0]
    for u in SV:
        PS.append(PS[-1] + rowptr[u + 1] - rowptr[u])      # PS[j] = entries of rows < j
    T = PS[k]
    regs = k <= L.LOOKUP_REGS
    if regs:
        pad = EMPTY if mutant == "sv_pad_is_empty" else SV_PAD
        sv = [SV[t] if t < k else pad for t in range(8)]
        ps = [PS[t] if t < k else PS_PAD for t in range(8)] + [PS_PAD]
    subs = 3 if mutant == "chunk_of_3_sub_chunks" else L.SUB_CHUNKS
    w_off = e0
    for cb in range(0, T, L.SUB_CHUNKS * GS):
        wv = [[EMPTY] * GS for _ in range(4)]
        jj = [[0] * GS for _ in range(4)]
        ec = [[0] * GS for _ in range(4)]
        for u in range(4):
            for lane in range(GS):
                e = cb + u * GS + lane
                if e < T:
                    below = (lambda p: p < e) if mutant == "row_of_entry_lt" else (lambda p: p <= e)
                    if regs:
                        j = sum(below(ps[t]) for t in range(1, 8))
                        base_e = ps[j]
                    else:
                        j = sum(below(PS[t]) for t in range(1, k))
                        base_e = PS[j]
                    at = R0[j] + (e - base_e)
                    jj[u][lane] = j
                    wv[u][lane], ec[u][lane] = (nbr[at], col[at]) if 0 <= at < len(nbr) else (EMPTY, 0)
        for u in range(subs):
            start = cb + u * GS
            if mutant == "sub_break_gt":
                if start > T:
                    break
            elif mutant == "sub_break_early":
                if start + 1 >= T:
                    break
            elif start >= T:
                break
            ls = []
            for lane in range(GS):
                w = wv[u][lane]
                l = -1
                if regs:
                    for t in range(7, -1, -1):
                        l = t if sv[t] == w else l
                elif w != EMPTY:
                    for t in range(k):
                        if SV[t] == w:
                            l = t
                            break
                ls.append(l)
            mk = [l >= 0 for l in ls]
            for lane in range(GS):
                pos = w_off + sum(mk[:lane + 1] if mutant == "prefix_includes_own_lane" else mk[:lane])
                l = ls[lane]
                if l >= 0 and (pos <= ld if mutant == "capacity_le" else pos < ld):
                    j = jj[u][lane]
                    if mode == "sample":
                        uf, vf = j, l
                    elif mode == "graph":
                        base = row_abs if mutant == "graph_mode_row" else i
                        uf, vf = base * k + j, base * k + l
                    elif mode == "batch":
                        base = row_abs if mutant == "batch_mode_absolute_row" else row_rel
                        uf, vf = base * k + j, base * k + l
                    else:
                        uf, vf = SV[j] + extra, (SV[l] if l < k else GUARD) + extra   # (l >= k: only a mutant gets there)
                    out.store(out.ei, pos, uf)
                    out.store(out.ei, ld + pos, vf)
                    out.store(out.es, pos, ec[u][lane])
            w_off += min(GS, T - start) if mutant == "w_off_by_lanes" else sum(mk)
    return w_off


def model_fill(graph, num_graphs, nodes, edge_ptr, m, k, GS, ld, mode, row_begin=0, extra=0, mutant=None, reverse=False):
    """ugs_fill<GS> over rows whose edge_ptr is given (and the rows' loop of ugs_fill_scan<8>): the Out it leaves.  The device runs
    the rows in no particular order; `reverse` takes them last to first, so that a row writing into its neighbour's entries shows."""
    out = Out(ld)
    rows = list(enumerate(np.asarray(nodes).reshape(-1, k)))
    for row_rel, row in (rows[::-1] if reverse else rows):
        e0, e1 = int(edge_ptr[row_rel]), int(edge_ptr[row_rel + 1])
        if e1 == e0:
            continue                                       # incomplete or edgeless row
        row_abs = row_begin + row_rel
        i = row_abs if num_graphs == 1 else row_abs - (row_abs // m) * m
        model_fill_row(graph, row, k, GS, e0, out, mode, i, row_abs, row_rel, extra, mutant)
    return out


def agrees(out, law):
    """The model's buffers against the law's (edge_ptr, edge_index, edge_src): entries below ld equal, guard words untouched."""
    n = min(int(law[0][-1]), out.ld)
    u, v, s = out.edges(n)
    return out.guards_intact() and u == law[1][0, :n].tolist() and v == law[1][1, :n].tolist() and s == law[2][:n].tolist()


# ---- the scan folded into the fill ---------------------------------------------------------------------------------------------
def model_walk_sums(counts, lanes=8, grid=None, mutant=None):
    """The 8-row sums ugs_walk_lds leaves beside the counts (wsum), block by block: 256 threads are 32 rows of 8 lanes (a wave
    holds 8 rows and writes their sum) or 16 rows of 16 lanes (a wave holds 4 rows, two waves make a sum)."""
    total = len(counts)
    groups = 256 // lanes
    grid = max(1, -(-total // groups)) if grid is None else grid
    ngroups = grid * groups
    span = 7 if mutant == "sums_of_7_rows" else L.SUM_ROWS
    wsum = [GUARD] * (-(-total // L.SUM_ROWS))
    for block in range(grid):
        for it0 in range(block * groups, total, ngroups):
            ne = [counts[it0 + g] if it0 + g < total else 0 for g in range(groups)]
            rpw = 64 // lanes
            wave = [sum(ne[w * rpw:w * rpw + rpw][:span]) for w in range(4)]
            if lanes == 8:
                for w in range(4):
                    w0 = it0 + w * 8
                    if w0 < total:
                        wsum[w0 >> 3] = wave[w]
            else:
                for t in range(groups // 8):
                    r0 = it0 + t * 8
                    if r0 < total:
                        wsum[r0 >> 3] = wave[2 * t] + (0 if mutant == "wide_sums_one_wave" else wave[2 * t + 1])
    return wsum


def model_fill_scan(counts, rows, cus, packed_cap=0, lanes=8, mutant=None, stale=12345):
    """ugs_fill_scan<8> without the rows' fill: (edge_ptr [rows + 1], total handed to the host or None, write) from the per-row
    counts.  `stale`: what the scratch holds behind the call's sum words (an earlier, larger call's)."""
    BLOCK, GROUPS = 256, L.TILE_ROWS
    wsum = model_walk_sums(counts[:rows], lanes, mutant=mutant) + [stale] * 8
    nw = -(-rows // L.SUM_ROWS)
    W4 = np.array(wsum[:len(wsum) // 4 * 4], np.int64).reshape(-1, 4).sum(1)           # the sum words as sixteen-byte loads see them
    span = lambda t0, end: int(W4[t0:max(t0, min(t0 + 8 * BLOCK, end))].sum())         # one trip: 8 loads x 256 threads, those below `end`
    ntiles = -(-rows // GROUPS)
    grid = max(1, min(ntiles, L.GRID_PER_CU * cus))
    stride = grid + (1 if mutant == "tile_stride_plus_1" else -1 if mutant == "tile_stride_minus_1" and grid > 1 else 0)
    trip = {"trip_2047": 2047, "trip_2049": 2049}.get(mutant, 8 * BLOCK)
    edge_ptr = [GUARD] * (rows + 1)
    h_total, write_any = None, True
    for block in range(grid):
        write = True
        tile = block
        while tile < ntiles:
            before = 0
            end = tile + 1 if mutant == "before_le_tile" else tile
            for t0 in range(0, tile, trip):                 # a trip: threads 0 .. 8 * 256 - 1 load one sixteen-byte word each
                before += span(t0, end)
            if packed_cap and tile == block:
                n4 = nw >> 2
                tot = before
                for t0 in range(tile, n4, trip):
                    tot += span(t0, n4)
                if mutant != "tail_words_dropped":
                    tot += sum(wsum[4 * n4 + x] for x in range(BLOCK) if x < nw - 4 * n4)
                write = 3 * tot < packed_cap if mutant == "write_lt" else 3 * tot <= packed_cap
                if block == 0:
                    h_total, write_any = tot, write
            c = [counts[tile * GROUPS + g] if tile * GROUPS + g < rows else 0 for g in range(GROUPS)]
            for g in range(GROUPS):
                row_rel = tile * GROUPS + g
                if row_rel < rows:
                    e0 = before + sum(c[:g])
                    edge_ptr[row_rel] = e0
                    if row_rel == rows - 1:
                        edge_ptr[rows] = e0 + c[g]
            tile += stride
    return edge_ptr, h_total, write_any
