"""batch_pass_device_model.py -- the device batch pass's kernels (csrc/ugs_batch.hip) restated in Python the way the DEVICE
computes them: four waves with their quarters, count then place, kept ballots or not; the 256-column rounds with run_sh;
ugs_bp_assign's owner search and per-wave aggregation; the key chain in rounds of 64; the row-pointer scan with its carry; the
chunked placement with MSK / CUR; ugs_bp_roots' two searches and its alias loop with the prefetched s_below / l_below.  Each
mutant is one modelled slip in one of those lines; tests/test_batch_pass_law.py shows that the unmutated model equals the law
(tests/batch_pass_law.py) on every input of tests/batch_pass_paths.py and that every mutant differs from it on a named one.

A mutant that leaves the arrays' bounds raises IndexError, which the tests count as told apart (on the device it is a write
outside the block's LDS arrays).

Mutants that cannot change any output, and are therefore not listed: the two entries of a loop swapped in its row (both are
(x, column)); `nchunk <= 512` as `<` (kept ballots and re-read columns give the same ballots -- the census makes sure both sides
of the bound run); `n <= 64` as `<` in ugs_bp_roots (the two searches visit the same vertices in the same order)."""
import numpy as np

import batch_pass_law as L

MUTANTS = (
    "fused_inclusive_prefix", "span_inclusive_prefix", "fused_off_without_earlier_waves", "span_off_without_earlier_waves", "fused_no_w1_bound",
    "fused_wrong_chunk", "reread_one_endpoint", "span_last_excluded", "run_sh_not_advanced", "search_first_of_equal_ptr", "jmax_from_lowest_lane",
    "rank_tie_le", "below_inclusive", "cursor_by_one", "msk_not_cleared", "suffix_gt", "no_cnt_bound", "mask_32_bits",
    "stride_512", "ns_no_round_up", "carry_dropped", "b_power", "scale_reassociated", "alias_reassociated", "demoted_not_next",
)
M64 = L.M64


def popc_below(mk, lane, inclusive=False):
    return bin(mk & ((1 << (lane + inclusive)) - 1)).count("1")


# ---- ugs_bp_assign ------------------------------------------------------------------------------------------------------------
def assign(ei, ptr, mutant=None):
    """owner[E], cnt[G], first[G], last[G] (first as the kernel keeps it: 0xFFFFFFFF - jminc)"""
    G, E = len(ptr) - 1, ei.shape[1]
    owner = np.full(E, -1, np.int64)
    cnt, jminc, jmax = [0] * G, [0] * G, [0] * G
    ptr = [int(x) for x in ptr]
    for w0 in range(0, E, 64):
        g_of = [-1] * 64
        for lane in range(min(64, E - w0)):
            u, v = int(ei[0, w0 + lane]), int(ei[1, w0 + lane])
            if ptr[0] <= u < ptr[G]:
                lo, hi = 0, G
                while hi - lo > 1:
                    mid = (lo + hi) >> 1
                    if ptr[mid] <= u:
                        lo = mid
                    else:
                        hi = mid
                while mutant == "search_first_of_equal_ptr" and lo > 0 and ptr[lo - 1] == ptr[lo]:
                    lo -= 1
                if ptr[lo] <= u < ptr[lo + 1] and ptr[lo] <= v < ptr[lo + 1]:
                    g_of[lane] = lo
            owner[w0 + lane] = g_of[lane]
        todo = [l for l in range(64) if g_of[l] >= 0]
        while todo:
            l0 = todo[0]
            same = [l for l in range(64) if g_of[l] == g_of[l0]]
            g0 = g_of[l0]
            cnt[g0] += len(same)
            jminc[g0] = max(jminc[g0], 0xFFFFFFFF - (w0 + l0))
            jmax[g0] = max(jmax[g0], w0 + (same[0] if mutant == "jmax_from_lowest_lane" else same[-1]))
            todo = [l for l in todo if l not in same]
    return owner, cnt, [0xFFFFFFFF - x for x in jminc], jmax


# ---- ugs_bp_build, step 1: the graph's columns in column order ---------------------------------------------------------------
def ballots(mine):
    """per chunk of 64 lanes the ballot of a boolean array whose length is a multiple of 64"""
    return [int(x) for x in np.packbits(mine.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()]


def compact_fused(ei, lo, n, lim, mutant=None):
    """(batch columns of the graph in the order the block leaves them in LC, or None above the limit)"""
    E = ei.shape[1]
    per = (((E + 3) // 4) + 63) & ~63
    su, sv = ei[0] - lo, ei[1] - lo
    inside = (su >= 0) & (su < n) & (sv >= 0) & (sv < n)
    waves = []
    for wv in range(4):
        w0 = wv * per
        w1 = min(w0 + per, E)
        nchunk = (w1 - w0 + 63) // 64 if w1 > w0 else 0
        pad = np.zeros(nchunk * 64, bool)
        if nchunk:
            if mutant == "fused_no_w1_bound" and w0 + nchunk * 64 > w1:   # (w1 is below a chunk's end only where it is E)
                raise IndexError("columns read past the last one")
            pad[:w1 - w0] = inside[w0:w1]
        mks = ballots(pad) if nchunk else []
        waves.append((w0, w1, nchunk, mks))
    wsum = [sum(bin(m).count("1") for m in mks) for _, _, _, mks in waves]
    tot = sum(wsum)
    if tot > lim:
        return None
    LC = [None] * tot
    for wv, (w0, w1, nchunk, mks) in enumerate(waves):
        keep = nchunk <= L.MASK_CHUNKS
        off = 0 if mutant == "fused_off_without_earlier_waves" else sum(wsum[:wv])
        for c in range(nchunk):
            if keep:
                mk = mks[(c + 1) % nchunk if mutant == "fused_wrong_chunk" else c]
            else:
                mk = mks[c]                                          # the columns read again: the same ballot
                if mutant == "reread_one_endpoint":                  # ... unless the second test of `mine` forgets v
                    j = np.arange(w0 + c * 64, min(w0 + c * 64 + 64, w1))
                    pad = np.zeros(64, bool)
                    pad[:len(j)] = (su[j] >= 0) & (su[j] < n)
                    mk = ballots(pad)[0]
            if not mk:
                continue
            for lane in range(64):
                if (mk >> lane) & 1:
                    LC[off + popc_below(mk, lane, mutant == "fused_inclusive_prefix")] = w0 + c * 64 + lane
            off += bin(mk).count("1")
    return LC


def compact_span(owner, g, j0, j1, cn, mutant=None):
    LC = [None] * cn
    run = 0
    for base in range(j0, j1 + 1, L.BLOCK):
        mine = [False] * L.BLOCK
        for tid in range(L.BLOCK):
            j = base + tid
            inside = j < j1 if mutant == "span_last_excluded" else j <= j1
            mine[tid] = inside and j < len(owner) and owner[j] == g
        wsum = [sum(mine[w * 64:w * 64 + 64]) for w in range(4)]
        for tid in range(L.BLOCK):
            if mine[tid]:
                wv, lane = tid >> 6, tid & 63
                off = run + (0 if mutant == "span_off_without_earlier_waves" else sum(wsum[:wv]))
                below = sum(mine[wv * 64:wv * 64 + lane + (mutant == "span_inclusive_prefix")])
                LC[off + below] = base + tid
        if mutant != "run_sh_not_advanced":
            run += sum(wsum)
    return LC


# ---- step 2: the key chain ------------------------------------------------------------------------------------------------------
def key_chain(n, lu, lv, large, mutant=None):
    cn = len(lu)
    h = ((L.FNV_BASIS ^ n) * L.FNV_PRIME) & M64
    h = ((h ^ cn) * L.FNV_PRIME) & M64
    st = (cn // (512 if mutant == "stride_512" else L.KEY_DIV)) if large and cn > L.MAX_COLS else 1
    ns = ((cn // st if mutant == "ns_no_round_up" else (cn + st - 1) // st)) if large else cn
    for t0 in range(0, ns, 64):
        regs = [((t0 + lane) * st if t0 + lane < ns else 0) for lane in range(64)]
        for i in range(min(64, ns - t0)):
            h = ((h ^ int(lu[regs[i]])) * L.FNV_PRIME) & M64
            h = ((h ^ int(lv[regs[i]])) * L.FNV_PRIME) & M64
    return h


# ---- steps 3 - 6: degrees, scan with carry, rank, chunked placement ------------------------------------------------------------
def scan_rowptr(deg, mutant=None):
    n = len(deg)
    RP, carry = [0] * (n + 1), 0
    for base in range(0, n, L.BLOCK):
        d = [int(deg[base + t]) if base + t < n else 0 for t in range(L.BLOCK)]
        wsum = [sum(d[w * 64:w * 64 + 64]) for w in range(4)]
        for t in range(L.BLOCK):
            if base + t < n:
                wv, lane = t >> 6, t & 63
                RP[base + t] = carry + sum(wsum[:wv]) + sum(d[wv * 64:wv * 64 + lane])
        if mutant != "carry_dropped":
            carry += sum(wsum)
    RP[n] = carry
    return RP


def ranks(deg, mutant=None):
    d = np.asarray(deg)
    n = len(d)
    x = np.arange(n)
    less = d[None, :] < d[:, None]
    tie = (d[None, :] == d[:, None]) & ((x[None, :] <= x[:, None]) if mutant == "rank_tie_le" else (x[None, :] < x[:, None]))
    return (less | tie).sum(axis=1)


def place(n, lu, lv, cols, RP, RNK, mutant=None):
    ne = 2 * len(lu)
    adj, adjf = [None] * ne, [None] * ne
    CUR, MSK = list(RP[:n]), [0] * n
    for e0 in range(0, ne, 64):
        lanes = range(min(64, ne - e0))
        row, other = [0] * 64, [0] * 64
        for lane in lanes:
            t, side = (e0 + lane) >> 1, (e0 + lane) & 1
            row[lane], other[lane] = (int(lv[t]), int(lu[t])) if side else (int(lu[t]), int(lv[t]))
            MSK[row[lane]] |= 1 << lane
        mates = [MSK[row[lane]] for lane in lanes]
        cur = [CUR[row[lane]] for lane in lanes]
        for lane in lanes:
            below = popc_below(mates[lane], lane, mutant == "below_inclusive")
            pp = cur[lane] + below
            adj[pp] = (other[lane], int(RNK[other[lane]]))
            adjf[pp] = (other[lane], int(cols[(e0 + lane) >> 1]))
            if below == 0:
                CUR[row[lane]] = cur[lane] + (1 if mutant == "cursor_by_one" else bin(mates[lane]).count("1"))
                if mutant != "msk_not_cleared":
                    MSK[row[lane]] = 0
    never = (-1, -1)                                                 # (an entry no lane wrote: whatever the arrays held)
    return [a or never for a in adj], [a or never for a in adjf]


# ---- ugs_bp_roots --------------------------------------------------------------------------------------------------------------
def roots(n, RP, NBR, RNK, k, mutant=None):
    ORD = [0] * n
    for x in range(n):
        ORD[RNK[x]] = x
    P, SDEG = [0.0] * n, [0] * n
    for vi in range(n):                                              # thread vi % 256, round vi / 256: independent
        v = ORD[vi]
        c = sum(1 for p in range(RP[v], RP[v + 1]) if (RNK[NBR[p]] > vi if mutant == "suffix_gt" else RNK[NBR[p]] >= vi))
        SDEG[vi] = c
        Lst = [v] + [None] * (L.KMAX - 1)
        cnt = 1
        reached = 1 << v
        h = 0
        while h < cnt and cnt < k:
            u = Lst[h]
            p = RP[u]
            while p < RP[u + 1] and (mutant == "no_cnt_bound" or cnt < k):
                w = NBR[p]
                p += 1
                if RNK[w] < vi:
                    continue
                if n <= 64:
                    bit = 1 << (w & 31) if mutant == "mask_32_bits" else 1 << w      # (a 32-bit shift takes its count modulo 32)
                    if reached & bit:
                        continue
                    reached |= bit
                elif w in Lst[:cnt]:
                    continue
                Lst[cnt] = w                                         # IndexError past UGS_KMAX entries
                cnt += 1
            h += 1
        b = 0.0
        if cnt >= k:
            d = float(max(c, 1))
            b = float(int(d) ** (k - 1)) if mutant == "b_power" else L.weight(d, k)
        P[vi] = b
    Z = 0.0
    for x in P:
        Z += x
    nz = sum(1 for x in P if x > 0.0)
    out = {"suffix_deg": SDEG, "Z": Z, "level": 0, "viable_vi": [], "viable_v": []}
    ALI = [0] * n
    if Z > 0.0:
        P = [x * (n / Z) for x in P] if mutant == "scale_reassociated" else [x * n / Z for x in P]
        LO = [i for i in range(n) if P[i] < 1.0]
        HI = [i for i in range(n) if not P[i] < 1.0]
        nl, nh = len(LO), len(HI)
        LO += [0] * n
        if nl > 0 and nh > 0:
            l, s = HI[nh - 1], LO[nl - 1]
            pl, ps = P[l], P[s]
            while nl > 0 and nh > 0:
                nl -= 1
                s_below = LO[nl - 1] if nl > 0 else 0
                l_below = HI[nh - 2] if nh > 1 else 0
                ps_below, pl_below = P[s_below], P[l_below]
                ALI[s] = l
                pl = pl + (ps - 1.0) if mutant == "alias_reassociated" else (pl + ps) - 1.0
                if pl < 1.0:
                    P[l] = pl
                    nh -= 1
                    LO[nl] = l
                    nl += 1
                    if mutant == "demoted_not_next":
                        s, ps = s_below, ps_below
                    else:
                        s, ps = l, pl
                    l, pl = l_below, pl_below
                else:
                    s, ps = s_below, ps_below
        for i in HI[:nh] + LO[:nl]:
            P[i] = 1.0
    if nz > 0:
        out.update(prob=P, alias=ALI, v_self=ORD, v_alias=[ORD[a] for a in ALI])
    else:
        via = [vi for vi in range(n) if SDEG[vi] > 0]
        out["level"] = 1
        if not via:
            out["level"], via = 2, list(range(n))
        out["viable_vi"], out["viable_v"] = via, [ORD[vi] for vi in via]
    return out


# ---- one graph / one batch through the model -----------------------------------------------------------------------------------
def build_graph(ei, ptr, g, k, lim, fused, assigned, mutant=None, with_roots=True):
    """None for a degenerate graph, "over" above a limit, else what the block of graph g leaves (as batch_pass_law.graph_law)"""
    lo, n = int(ptr[g]), int(ptr[g + 1] - ptr[g])
    if n <= 0 or n < k:
        return None
    if fused:
        if n > L.MAX_N:
            return "over"
        LC = compact_fused(ei, lo, n, lim, mutant)
        if LC is None:
            return "over"
    else:
        owner, cnt, first, last = assigned
        if n > L.MAX_N or cnt[g] > lim:
            return "over"
        LC = compact_span(owner, g, first[g], last[g], cnt[g], mutant) if cnt[g] else []
    if any(j is None for j in LC):
        raise IndexError("a slot of LC was never written")
    cols = np.array(LC, np.int64)
    lu, lv = ei[0, cols] - lo, ei[1, cols] - lo
    if len(cols) and (lu.min() < 0 or lv.min() < 0 or max(lu.max(), lv.max()) >= n):
        raise IndexError("a foreign column among the graph's")
    cn = len(cols)
    out = {"n": n, "cn": cn, "cols": cols, "first": int(cols[0]) if cn else None, "last": int(cols[-1]) if cn else None}
    out["key"] = key_chain(n, lu, lv, lim > L.MAX_COLS, mutant)
    deg = np.zeros(n, np.int64)
    np.add.at(deg, lu, 1)
    np.add.at(deg, lv, 1)
    RP = scan_rowptr(deg, mutant)
    RNK = ranks(deg, mutant)
    if RNK.max(initial=0) >= n:
        raise IndexError("a rank outside the graph")
    adj, adjf = place(n, lu, lv, cols, RP, RNK, mutant)
    out.update(rowptr=np.array(RP), rank=RNK, nbr=np.array([a[0] for a in adj], np.int64), nbr_rank=np.array([a[1] for a in adj], np.int64),
               nbr_col=np.array([a[1] for a in adjf], np.int64))
    if with_roots and n <= L.ROOTS_MAX_N:
        out.update(roots(n, RP, [a[0] for a in adj], [int(x) for x in RNK], k, mutant))
    return out


def batch(ei, ptr, k, lim=L.MAX_COLS, fused_work=L.FUSED_WORK, mutant=None, graphs=None, with_roots=True):
    G, E = len(ptr) - 1, ei.shape[1]
    fused = G * E <= fused_work
    assigned = None if fused else assign(ei, ptr, mutant)
    return [build_graph(ei, ptr, g, k, lim, fused, assigned, mutant, with_roots) for g in (range(G) if graphs is None else graphs)]
