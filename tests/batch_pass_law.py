"""batch_pass_law.py -- what the device batch pass (csrc/ugs_batch.hip: ugs_bp_assign, ugs_bp_build, ugs_bp_roots) must leave for
every graph of a batch, in plain Python and numpy, from (edge_index, ptr, k, max_cols) alone; and the census of the kernels' paths
an input reaches.  No torch, no library: tests/test_batch_pass_law.py holds this file against the oracle's preprocessing
(reference src/ugs_sampler_batch_extension.cpp:41-75 slicing, include/cache.hpp:81-109 key, src/preproc.cpp:32-256, include/
sampler.hpp:44-69 Vose's table, src/sampler.cpp:121-150 relaxation levels).  Python floats are IEEE doubles and every operation
below is written in the reference's order, so doubles compare bit for bit."""
import collections

import numpy as np

# the kernels' constants (tests/test_batch_pass_law.py reads them from ugs_batch.hip and ugs_device.h)
WAVE, BLOCK, MASK_CHUNKS = 64, 256, 512
MAX_COLS, COLS_CEIL, MAX_N, ROOTS_MAX_N = 1000, 8192, 2048, 1024
KEY_DIV, FUSED_WORK, KMAX = 500, 4 << 20, 32
M64 = (1 << 64) - 1
FNV_BASIS, FNV_PRIME = 14695981039346656037, 1099511628211


# ---- key and fingerprint ----------------------------------------------------------------------------------------------------
def key_stride(cn):
    return cn // KEY_DIV if cn > MAX_COLS else 1


def key(n, lu, lv):
    """FNV-1a over (n, columns, renumbered columns 0, s, 2s, ...)"""
    cn = len(lu)
    h = ((FNV_BASIS ^ n) * FNV_PRIME) & M64
    h = ((h ^ cn) * FNV_PRIME) & M64
    for t in range(0, cn, key_stride(cn)):
        h = ((h ^ int(lu[t])) * FNV_PRIME) & M64
        h = ((h ^ int(lv[t])) * FNV_PRIME) & M64
    return h


def fp_mix(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    return x ^ (x >> 33)


def fingerprint(n, lu, lv):
    """ugs_fp_seed / ugs_fp_add (ugs_device.h) restated: two 64-bit sums over (t, u, v)"""
    cn = len(lu)
    a = fp_mix((n * 0x9e3779b97f4a7c15 + cn) & M64)
    b = fp_mix((cn * 0xc2b2ae3d27d4eb4f + n) & M64)
    for t in range(cn):
        ht = fp_mix((t + 0x9e3779b97f4a7c15) & M64)
        p = ((int(lu[t]) << 32) & M64) | (int(lv[t]) & 0xffffffff)
        a = (a + fp_mix(p ^ ht)) & M64
        b = (b + fp_mix((p * 0xc2b2ae3d27d4eb4f + ((ht >> 7) | (ht << 57) & M64)) & M64)) & M64
    return a, b


# ---- slicing and CSR --------------------------------------------------------------------------------------------------------
def owned(ei, lo, hi):
    """batch columns with both endpoints in [lo, hi), in column order"""
    return np.nonzero((ei[0] >= lo) & (ei[0] < hi) & (ei[1] >= lo) & (ei[1] < hi))[0]


def owners(ei, ptr):
    """per column the graph that owns it, or -1 (ptr non-decreasing: the node ranges are disjoint)"""
    out = np.full(ei.shape[1], -1, np.int64)
    for g in range(len(ptr) - 1):
        out[owned(ei, ptr[g], ptr[g + 1])] = g
    return out


def csr(n, lu, lv, cols):
    """degrees, row pointer, rank by ascending (degree, id), and the rows in column order: u's row then v's row per column"""
    deg = np.zeros(n, np.int64)
    np.add.at(deg, lu, 1)
    np.add.at(deg, lv, 1)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    order = np.lexsort((np.arange(n), deg))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    cur = rowptr[:-1].copy()
    nbr, col = np.zeros(rowptr[-1], np.int64), np.zeros(rowptr[-1], np.int64)
    for t in range(len(lu)):
        u, v = int(lu[t]), int(lv[t])
        nbr[cur[u]], col[cur[u]] = v, cols[t]
        cur[u] += 1
        nbr[cur[v]], col[cur[v]] = u, cols[t]
        cur[v] += 1
    return deg, rowptr, rank, order, nbr, col


# ---- roots --------------------------------------------------------------------------------------------------------------------
def reach(rows, rank, v, vi, k):
    """the bounded search of root v (order position vi) inside its suffix graph: (vertices reached, capped at k; the position in
    the visit list whose row supplied the last one; whether that was the row's last entry; whether the search tested a
    neighbour w on which a reached-set mask indexed by w modulo 32 answers otherwise than the set itself)"""
    L, head_of_last, at_row_end = [v], 0, False
    low32, slip32 = 1 << v, False                                     # the mask a 32-bit `1 << w` would keep (the root's bit is set in 64)
    h = 0
    while h < len(L) and len(L) < k:
        row = rows[L[h]]
        for i, w in enumerate(row):
            if rank[w] < vi:
                continue
            slip32 |= (w in L) != bool(low32 >> (w & 31) & 1)
            if w in L:
                continue
            L.append(w)
            low32 |= 1 << (w & 31)
            head_of_last, at_row_end = h, i == len(row) - 1
            if len(L) >= k:
                break
        h += 1
    return len(L), head_of_last, at_row_end, slip32


def weight(d, k):
    b = 1.0
    for _ in range(1, k):
        b *= d
    return b


def vose(P, alt=False, trace=None):
    """Vose's table with two LIFO stacks filled in ascending index (reference include/sampler.hpp:44-69).  alt: the other
    association of the update, pl + (ps - 1.0).  trace: a Counter for the census."""
    n = len(P)
    P = list(P)
    prob, alias = [0.0] * n, [0] * n
    small = [i for i in range(n) if P[i] < 1.0]
    large = [i for i in range(n) if not P[i] < 1.0]
    if trace is not None:
        trace["no small stack"] += not small
        trace["no large stack"] += not large
    demoted = False
    while small and large:
        s, l = small.pop(), large[-1]
        if trace is not None:
            trace["demoted one popped next"] += demoted
            trace["alias association matters"] += (P[l] + P[s]) - 1.0 != P[l] + (P[s] - 1.0)
        prob[s], alias[s] = P[s], l
        P[l] = P[l] + (P[s] - 1.0) if alt else (P[l] + P[s]) - 1.0
        demoted = P[l] < 1.0
        if demoted:
            small.append(large.pop())
        if trace is not None:
            trace["demotion" if demoted else "no demotion"] += 1
    if trace is not None:
        trace["leftover large"] += bool(large)
        trace["leftover small"] += bool(small)
        trace["leftovers on both stacks"] += bool(small) and bool(large)
    for i in large + small:
        prob[i] = 1.0
    return prob, alias


def roots(n, rowptr, nbr, rank, order, k, trace=None, scale_alt=False, alias_alt=False, b_exact=False):
    """suffix degrees, bounded reachability, b, Z, the scaled weights, the table, the relaxation level and its viable list.
    The three `alt` arguments give the other association of each floating-point formula (census and mutants only)."""
    rows = [nbr[rowptr[x]:rowptr[x + 1]].tolist() for x in range(n)]
    rank = rank.tolist()
    sdeg, cnt, b = [0] * n, [0] * n, [0.0] * n
    for vi in range(n):
        v = int(order[vi])
        sdeg[vi] = sum(1 for w in rows[v] if rank[w] >= vi)
        cnt[vi], head, at_end, slip32 = reach(rows, rank, v, vi, k)
        if trace is not None:
            trace["mask search, vertex >= 32 reached"] += n <= 64 and slip32
        if cnt[vi] >= k:
            d = max(sdeg[vi], 1)
            b[vi] = float(d ** (k - 1)) if b_exact else weight(float(d), k)
            if trace is not None:
                trace["b inexact"] += d ** (k - 1) >= 1 << 53 and weight(float(d), k) != float(d ** (k - 1))
                trace["second level needed"] += head > 0
                trace["reaches k at the last neighbour"] += at_end and k > 1
    Z = 0.0
    for x in b:
        Z += x
    out = {"suffix_deg": sdeg, "reached": cnt, "b": b, "Z": Z, "level": 0, "viable_vi": [], "viable_v": []}
    if Z > 0.0:
        P = [x * (n / Z) for x in b] if scale_alt else [x * n / Z for x in b]
        if trace is not None:
            trace["scale association matters"] += sum(x * n / Z != x * (n / Z) for x in b)
            trace["unreachable among reachable"] += 0.0 in b
        out["scaled"] = P
        out["prob"], out["alias"] = vose(P, alias_alt, trace)
        out["v_self"] = [int(order[i]) for i in range(n)]
        out["v_alias"] = [int(order[a]) for a in out["alias"]]
    else:
        via = [vi for vi in range(n) if sdeg[vi] > 0]
        out["level"] = 1
        if not via:
            out["level"], via = 2, list(range(n))
        out["viable_vi"], out["viable_v"] = via, [int(order[vi]) for vi in via]
    return out


# ---- the law of one graph, and of a batch -----------------------------------------------------------------------------------
def graph_law(ei, ptr, g, k, with_roots=True, trace=None, **alt):
    """None for a degenerate graph (n <= 0 or n < k), else everything the pass leaves for graph g"""
    lo, hi = int(ptr[g]), int(ptr[g + 1])
    n = hi - lo
    if n <= 0 or n < k:
        return None
    cols = owned(ei, lo, hi)
    lu, lv = ei[0, cols] - lo, ei[1, cols] - lo
    cn = len(cols)
    L = {"n": n, "cn": cn, "cols": cols, "lu": lu, "lv": lv, "first": int(cols[0]) if cn else None, "last": int(cols[-1]) if cn else None}
    L["key"] = key(n, lu, lv)
    L["fp"] = fingerprint(n, lu, lv) if cn > MAX_COLS else None
    L["deg"], L["rowptr"], L["rank"], L["order"], L["nbr"], L["nbr_col"] = csr(n, lu, lv, cols)
    L["nbr_rank"] = L["rank"][L["nbr"]]
    if with_roots:
        L.update(roots(n, L["rowptr"], L["nbr"], L["rank"], L["order"], k, trace, **alt))
    return L


def hands_over(ei, ptr, k, lim):
    """the pass gives the call to the general path: a non-degenerate graph above the limit in force or above 2048 vertices"""
    for g in range(len(ptr) - 1):
        n = int(ptr[g + 1] - ptr[g])
        if n > 0 and n >= k and (n > MAX_N or len(owned(ei, ptr[g], ptr[g + 1])) > lim):
            return True
    return False


# ---- census ------------------------------------------------------------------------------------------------------------------
def quarters(E):
    per = (((E + 3) // 4) + 63) & ~63
    return [(w * per, min(w * per + per, E)) for w in range(BLOCK // WAVE)]


def census(ei, ptr, k, lim=MAX_COLS, fused_work=FUSED_WORK, with_roots=True):
    """Counter: the classes of kernel paths the batch reaches ("Which test pins which path")"""
    c = collections.Counter()
    G, E = len(ptr) - 1, ei.shape[1]
    own = owners(ei, ptr)
    live = [g for g in range(G) if ptr[g + 1] - ptr[g] > 0 and ptr[g + 1] - ptr[g] >= k]
    fused = G * E <= fused_work
    large = lim > MAX_COLS
    c["large form"] += large
    c["cross-graph column"] += int(((own < 0) & (ei[0] >= ptr[0]) & (ei[0] < ptr[G]) & (ei[1] >= ptr[0]) & (ei[1] < ptr[G])).sum())
    c["stray column"] += int(((ei[0] < ptr[0]) | (ei[0] >= ptr[G]) | (ei[1] < ptr[0]) | (ei[1] >= ptr[G])).sum())
    if fused:
        qs = quarters(E)
        keeps = []
        for w0, w1 in qs:
            nchunk = (w1 - w0 + 63) // 64 if w1 > w0 else 0
            mine = [g for g in live if ((own[w0:w1] == g).any() if w1 > w0 else False)]
            keep = nchunk <= MASK_CHUNKS
            c["fused, empty quarter"] += nchunk == 0
            c["fused, partial chunk"] += nchunk > 0 and (w1 - w0) % 64 != 0 and any(own[j] in live for j in range(w0 + (nchunk - 1) * 64, w1))
            if mine:
                keeps.append(keep)
                c["keep, 512 chunks"] += keep and nchunk == MASK_CHUNKS
                c["no keep"] += not keep
                c["no keep, large"] += not keep and large
        c["keep and no keep in one block"] += True in keeps and False in keeps
        for g in live:
            c["fused, straddles quarter"] += sum(1 for w0, w1 in qs if w1 > w0 and (own[w0:w1] == g).any()) >= 2
    else:
        c["two kernels"] += 1
        c["two kernels, G * E > 4 Mi"] += G * E > FUSED_WORK
        for g in live:
            js = np.nonzero(own == g)[0]
            if len(js):
                c["span > 256"] += js[-1] - js[0] >= BLOCK
                c["foreign inside span"] += js[-1] - js[0] + 1 > len(js)
        for w0 in range(0, E, WAVE):
            o = own[w0:w0 + WAVE]
            c["assign, many graphs per wave"] += len(set(o[o >= 0].tolist())) >= 3
        for g in range(1, G):
            c["assign, shared ptr value"] += ptr[g] == ptr[g - 1] and ptr[g + 1] > ptr[g] and (own == g).any()
    tr = collections.Counter()
    for g in live:
        n = int(ptr[g + 1] - ptr[g])
        cn = int((own == g).sum())
        for x in (256, 257, 2048, 2049):
            c["n == %d" % x] += n == x
        c["cn == 0"] += cn == 0
        c["cn == lim"] += cn == lim
        c["cn == lim + 1"] += cn == lim + 1
        if n > MAX_N or cn > lim:
            continue
        s = key_stride(cn)
        ns = (cn + s - 1) // s
        for x in (63, 64, 65):
            c["ns == %d" % x] += ns == x
        if s > 1:
            c["strided s == %d" % s] += 1
        L = graph_law(ei, ptr, g, k, with_roots=False)
        deg = L["deg"]
        c["degree tie"] += len(set(deg.tolist())) < n
        c["empty row"] += int((deg == 0).sum())
        c["loop"] += int((L["lu"] == L["lv"]).sum())
        c["last chunk partial"] += (2 * cn) % 64 != 0
        rows_of = np.empty(2 * cn, np.int64)                         # endpoint e = 2t + side sits in row u (side 0) or v (side 1)
        rows_of[0::2], rows_of[1::2] = L["lu"], L["lv"]
        prev = set()
        for e0 in range(0, 2 * cn, 64):
            cnts = collections.Counter(rows_of[e0:e0 + 64].tolist())
            c["row fills a chunk"] += 64 in cnts.values()
            c["two rows share a chunk"] += sum(1 for x in cnts.values() if x >= 2) >= 2
            c["row over chunks"] += bool(prev & set(cnts))
            prev = set(cnts)
        c["n == 1025 host"] += n == 1025
        if with_roots and n <= ROOTS_MAX_N:
            c["mask search n == 64"] += n == 64
            c["list search n == 65"] += n == 65
            c["n == 1024"] += n == 1024
            c["n > 256"] += n > 256
            c["k == 1"] += k == 1
            c["k == 32"] += k == 32
            R = roots(n, L["rowptr"], L["nbr"], L["rank"], L["order"], k, tr)
            c["level %d" % R["level"]] += 1
    c.update(tr)
    return c
