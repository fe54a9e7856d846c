"""uniform_enum_law.py -- CPU restatement of uniform_sampler.enumerate_graphs / count_graphs (include/ugs_mi355.h,
ugs_uniform_enumerate_begin): every connected k-subset of every graph as a row, in the order the samplers draw from.

Built on the enumerations the sampler tests already trust: uniform_law.connected_subsets_comb (the reference's definition,
literally), uniform_law.sorted_masks (graphs of at most 64 vertices) and uniform_wide_law.sorted_tuples (any size).  A helper for
the tests, not a test; numpy only.

  * S_g = the connected k-subsets of graph g in lexicographic order of the ascending tuples; empty for k = 0 or n < k;
  * sample_ptr = the exclusive scan of |S_g| in batch order, 0 for a failed graph; row sample_ptr[g] + i = ptr[g] + the i-th set;
  * a row's edges: the batch columns with both endpoints in g's range and in the set, in column order (loops and duplicates
    included), edge_src = the column; mode "sample" numbers the endpoints by position in the row, any other mode keeps batch ids.
"""
import numpy as np

import uniform_law as U
import uniform_wide_law as W


def subsets(adj, k, how="auto"):
    """S_g as an int64 array [|S_g|, k] of ascending local vertices.  how: "comb" (the definition), "masks", "tuples", or "auto"
    (masks up to 64 vertices, tuples above)."""
    n = len(adj)
    if k <= 0 or n < k:
        return np.zeros((0, max(k, 0)), np.int64)
    if how == "auto":
        how = "masks" if n <= 64 else "tuples"
    if how == "comb":
        rows = U.connected_subsets_comb(adj, k)
    elif how == "masks":
        rows = [U.mask_tuple(x) for x in U.sorted_masks(adj, k)]
    else:
        rows = W.sorted_tuples(adj, k)
    return np.array(rows, np.int64).reshape(-1, k)


def graph_sets(edge_index, ptr, k, how="auto"):
    """[S_g for g in batch order] (local vertices), whatever the graph's size."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    return [subsets(U.graph_adjacency(ei[0], ei[1], int(ptr[g]), int(ptr[g + 1] - ptr[g])), k, how) for g in range(len(ptr) - 1)]


def enumerate_graphs(edge_index, ptr, k, mode="sample", failed=(), how="auto", sets=None):
    """(nodes [R, k], edge_index [2, E], edge_ptr [R+1], sample_ptr [G+1], edge_src [E], counts [G]), all int64.  `failed`: the
    graphs that contribute no rows (their count is still reported); `sets`: graph_sets(...) computed before, to share it."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    src, dst = ei[0], ei[1]
    G = len(ptr) - 1
    sets = graph_sets(ei, ptr, k, how) if sets is None else sets
    counts = np.array([len(s) for s in sets], np.int64).reshape(G)
    sizes = np.where(np.isin(np.arange(G), list(failed)), 0, counts) if G else counts
    sptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cols = np.arange(src.shape[0], dtype=np.int64)
    nodes, eu, ev, es, ecount = [], [], [], [], []
    for g in range(G):
        if sizes[g] == 0:
            continue
        lo, n, S = int(ptr[g]), int(ptr[g + 1] - ptr[g]), sets[g]
        inside = (src >= lo) & (src < lo + n) & (dst >= lo) & (dst < lo + n)
        cu, cv, cc = src[inside] - lo, dst[inside] - lo, cols[inside]
        # the columns (u, v) grouped by u n + v, each group in column order; a row's edges are the groups of its k^2 ordered pairs
        # (S[a], S[b]), a = b for loops, gathered and put back into column order
        key = cu * n + cv
        by_key = np.argsort(key, kind="stable")
        skey = key[by_key]
        r_parts, c_parts, a_parts, b_parts = [], [], [], []
        for a in range(k):
            for b in range(k):
                q = S[:, a] * n + S[:, b]
                first, last = np.searchsorted(skey, q, "left"), np.searchsorted(skey, q, "right")
                cnt = last - first
                r = np.repeat(np.arange(len(S)), cnt)
                within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                r_parts.append(r)
                c_parts.append(by_key[np.repeat(first, cnt) + within])               # index into the graph's columns, in column order
                a_parts.append(np.full(len(r), a))
                b_parts.append(np.full(len(r), b))
        r, c, pa, pb = (np.concatenate(x).astype(np.int64) for x in (r_parts, c_parts, a_parts, b_parts))
        o = np.lexsort((c, r))                                               # by row, then by column
        r, c, pa, pb = r[o], c[o], pa[o], pb[o]
        nodes.append(S + lo)
        eu.append(pa if mode == "sample" else lo + cu[c])
        ev.append(pb if mode == "sample" else lo + cv[c])
        es.append(cc[c])
        ecount.append(np.bincount(r, minlength=len(S)))
    cat = lambda parts, shape: np.concatenate(parts).astype(np.int64) if parts else np.zeros(shape, np.int64)   # noqa: E731
    eptr = np.concatenate([[0], np.cumsum(cat(ecount, (0,)))]).astype(np.int64)
    return (cat(nodes, (0, max(k, 0))), np.stack([cat(eu, (0,)), cat(ev, (0,))]), eptr, sptr, cat(es, (0,)), counts)


def draw_indices(sizes, m, seed):
    """The index into S_g of every draw of uniform_sampler.sample_batch(.., m, .., seed): one mt19937_64 for the call, m draws per
    graph with S_g non-empty, in batch order.  Returns {g: [m indices]}."""
    gen = U.mt19937_64(int(seed) & U.M64)
    return {g: [U.lemire(gen, int(n)) for _ in range(m)] for g, n in enumerate(sizes) if n > 0}
