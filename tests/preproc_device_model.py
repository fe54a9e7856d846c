"""preproc_device_model.py -- the five kernels of csrc/ugs_preproc.hip and the host lines between them (ugs_devpre_csr's `bits`,
the buffers the host hands in zeroed), restated as the device does them: 32-bit keys and values, one key per endpoint with the
sentinel key n for a skipped column, degrees that include the sentinel's, a stable sort over the low `bits` bits only, the row
pointer as the exclusive sum of n + 2 degrees, entries from the sorted values, the row pointer widened to 64 bits word by word,
and per root a breadth-first search on a private list of KMAX slots.  A write outside an array raises IndexError.

`mutant` names a one-line slip; tests/test_preproc_law.py shows that every one of them leaves something else than the law
(tests/preproc_law.py) on an input of tests/preproc_paths.py that it names.

The root stage visits only roots with a non-empty row one by one (for the others the kernel's loops do not run: cnt stays 1,
sdeg 0), so that graphs of a million isolated vertices stay cheap here."""
import numpy as np

from preproc_law import KMAX, key_bits

MUTANTS = (
    "bits_one_too_few", "range_test_on_low_32_bits", "range_test_one_endpoint", "unstable_within_key", "entries_side_swapped",
    "widen_stops_at_n", "sdeg_rank_gt", "bfs_no_suffix_filter", "bfs_no_seen_test", "bfs_bound_le", "row_scan_not_stopped",
    "assemble_rank_of_row_vertex", "assemble_colmap_ignored",
)
U32 = 0xFFFFFFFF


def i32(x):
    return np.asarray(x, np.int64).astype(np.uint32).astype(np.int32)          # (int32_t) of a 64-bit value


def stage_csr(ei, n, mutant=None):
    """ugs_devpre_csr: (h_rowptr int64[n + 1], nnz, nbr int32[nnz], col int32[nnz])"""
    src, dst = np.asarray(ei[0], np.int64), np.asarray(ei[1], np.int64)
    E = len(src)
    # pre_keys
    if mutant == "range_test_on_low_32_bits":
        ok = ((src & U32) < n) & ((dst & U32) < n)
    elif mutant == "range_test_one_endpoint":
        ok = src.astype(np.uint64) < np.uint64(n)
    else:
        ok = (src.astype(np.uint64) < np.uint64(n)) & (dst.astype(np.uint64) < np.uint64(n))
    keys = np.empty(2 * E, np.uint32)
    keys[0::2] = np.where(ok, src & U32, n)
    keys[1::2] = np.where(ok, dst & U32, n)
    vals = np.arange(2 * E, dtype=np.uint32)                                     # (2j, 2j + 1)
    deg = np.zeros(n + 2, np.uint32)
    if len(keys) and int(keys.max()) >= n + 2:
        raise IndexError("atomicAdd outside deg[n + 2]")
    np.add.at(deg, keys, 1)
    # host: bits; device: exclusive sum over n + 2 words, stable radix sort over bits [0, bits)
    bits = key_bits(n) - (1 if mutant == "bits_one_too_few" else 0)
    rowptr = np.zeros(n + 2, np.uint32)
    np.cumsum(deg[:-1], out=rowptr[1:])
    low = keys & np.uint32((1 << bits) - 1) if bits < 32 else keys
    if mutant == "unstable_within_key":
        perm = np.lexsort((-vals.astype(np.int64), low))                         # equal keys in descending value order
    else:
        perm = np.argsort(low, kind="stable")
    sorted_vals = vals[perm]
    nnz = int(rowptr[n])
    # pre_widen into the host's zeroed int64[n + 1]
    count = n if mutant == "widen_stops_at_n" else n + 1
    h_rowptr = np.zeros(n + 1, np.int64)
    h_rowptr[:count] = rowptr[:count]
    # pre_entries
    t = sorted_vals[:nnz].astype(np.int64)
    j = t >> 1
    side = (t & 1) == 1
    if mutant == "entries_side_swapped":
        side = ~side
    nbr = i32(np.where(side, src[j], dst[j]))
    return h_rowptr, nnz, nbr, j.astype(np.int32), rowptr


def stage_roots(rowptr, nbr, order, rank, n, k, mutant=None):
    """pre_roots: (sdeg int32[n], reach uint8[n]); rowptr is the device's 32-bit one"""
    if k > KMAX:
        raise IndexError("pre_roots is not to be launched with k > UGS_KMAX")
    sdeg, reach = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    reach[:] = 1 if 1 >= k else 0                                                # empty row: cnt stays 1
    rowptr = rowptr.astype(np.int64)
    for vi in np.flatnonzero(np.diff(rowptr[:n + 1])[order] > 0).tolist():
        v = int(order[vi])
        row = nbr[rowptr[v]:rowptr[v + 1]]
        sdeg[vi] = int(np.count_nonzero(rank[row] > vi if mutant == "sdeg_rank_gt" else rank[row] >= vi))
        got = [0] * KMAX
        cnt, h = 1, 0
        got[0] = v
        while h < cnt and (cnt <= k if mutant == "bfs_bound_le" else cnt < k):
            u = got[h]
            p, e = int(rowptr[u]), int(rowptr[u + 1])
            while p < e and (mutant == "row_scan_not_stopped" or (cnt <= k if mutant == "bfs_bound_le" else cnt < k)):
                w = int(nbr[p])
                p += 1
                if mutant != "bfs_no_suffix_filter" and rank[w] < vi:
                    continue
                if mutant != "bfs_no_seen_test" and w in got[:cnt]:
                    continue
                got[cnt] = w                                                     # IndexError past KMAX slots
                cnt += 1
            h += 1
        reach[vi] = 1 if cnt >= k else 0
    return sdeg, reach


def preprocess(ei, n, k, order_of, mutant=None):
    """preprocess_on_device: stage 1, the host's degree order (order_of(indptr) -> order, rank), stage 2, download"""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    h_rowptr, nnz, nbr, col, rowptr = stage_csr(ei, n, mutant)
    order, rank = order_of(h_rowptr)
    sdeg, reach = stage_roots(rowptr, nbr, order, rank, n, k, mutant)
    return {"indptr": h_rowptr, "indices": nbr, "edge_col": col, "order": order, "index_of": rank, "suffix_deg": sdeg, "reach": reach.astype(bool)}


def assemble(nbr, col, rank, rowptr, colmap=None, mutant=None):
    """pre_assemble: adj = (nbr, nbr_rank), adjf = (nbr_f, nbr_col); colmap as ugs_devpre_assemble gets it (None: identity, dropped)"""
    if mutant == "assemble_rank_of_row_vertex":
        nbr_rank = rank[np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))]
    else:
        nbr_rank = rank[nbr]
    if colmap is None or mutant == "assemble_colmap_ignored":
        nbr_col = col.copy()
    else:
        nbr_col = i32(np.asarray(colmap, np.int64)[col])
    return {"rowptr": rowptr, "nbr": nbr, "nbr_rank": nbr_rank.astype(np.int32), "nbr_f": nbr, "nbr_col": nbr_col}
