"""rwr_row_law.py -- CPU statement of rwr_sampler's streams="row" law (include/ugs_mi355.h, ugs_rwr_sample_rows_begin), on top of
tests/rwr_law.py, for the tests.

The law is rwr_law's with one change: the generator.  Let sg be the graph's seed (seed + g, or seeds[g]).  Row s of graph g owns a
SplitMix64 seeded with row_seed(sg, s) = mix(sg + (s + 1) * GAMMA) -- output s (0-based) of the graph's own generator in counter
form, `rwr_law.draw(sg, s)`; the per-graph law uses the draws 1, 2, ... only.  The row's walk is `rwr_law.walk` after c = 0 draws
of that stream.  Adjacency, n < k, the walk, rows, edges and sample_ptr are rwr_law's.

`census` walks every row and counts which paths of the device kernel (ugs_rwr.hip, rwr_row_walks) the input reaches; it restates
the kernel's constants below, and tests/test_rwr_row_law.py reads them back from the source.
"""
import collections

import numpy as np

import rwr_law as R

ROW_LANES = 64          # ugs_rwr.hip `constexpr int RWR_ROW_LANES`: lanes of rwr_row_walks' workgroup = rows of one graph it serves

Row = collections.namedtuple("Row", "g s draws doomed live_failed found")


def row_seed(sg, s):
    return R.mix((sg + (s + 1) * R.GAMMA) & R.M64)


def graph_seed(g, seed, seeds):
    return (seed + g) & R.M64 if seeds is None else int(seeds[g]) & R.M64


def sample_batch(ei, ptr, m, k, mode="sample", seed=42, p_restart=0.2, seeds=None, shortcuts=True):
    """The five outputs of the row law as numpy int64 arrays.  shortcuts=False walks out the rows the law fixes without walking
    (a doomed seed; p_restart == 1 with k > 1); the result is the same."""
    return _run(ei, ptr, m, k, mode, seed, p_restart, seeds, shortcuts)[0]


def _run(ei, ptr, m, k, mode, seed, p, seeds, shortcuts):
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    G = len(ptr) - 1
    adjs = R.adjacency(ei[0], ei[1], ptr)
    nodes = np.full((G * m, k), -1, np.int64)
    eptr, edges, rows = [0], [], []
    for g in range(G):
        adj, lo = adjs[g], int(ptr[g])
        n = len(adj)
        size = R.component_sizes(adj) if n >= k else None
        sg = graph_seed(g, seed, seeds)
        for s in range(m):
            chosen = []
            if n >= k:
                rs = row_seed(sg, s)
                seed_node = R.draw(rs, 1) % n
                doomed = size[seed_node] < k
                if shortcuts and (doomed or (p >= 1.0 and k > 1)):
                    draws = 1 if doomed else 0
                else:
                    chosen, draws = R.walk(adj, k, p, rs, 0)
                    assert chosen[0] == seed_node
                found = len(chosen) >= k
                assert not (doomed and found)
                rows.append(Row(g, s, draws, doomed, not doomed and not found, found))
            if len(chosen) >= k:
                nodes[g * m + s] = [lo + v for v in chosen]
                pos = {v: j for j, v in enumerate(chosen)}
                for u in chosen:
                    for v in adj[u]:
                        if v in pos:
                            edges.append((pos[u], pos[v]) if mode == "sample" else (lo + u, lo + v))
            eptr.append(len(edges))
    E = len(edges)
    edge_index = np.array(edges, np.int64).T.reshape(2, E) if E else np.zeros((2, 0), np.int64)
    out = (nodes, np.ascontiguousarray(edge_index), np.array(eptr, np.int64), np.arange(G + 1, dtype=np.int64) * m,
           np.full(E, -1, np.int64))
    return out, rows


def census_rows(ei, ptr, m, k, seed, p_restart, seeds=None):
    """(census, rows): a Counter of the kernel's path classes, and one Row (g, s, draws consumed, doomed, live_failed, found) per
    row of a graph with n >= k, every walk run to its end (no shortcuts), so that `draws` is what the law's walk consumes."""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    G = len(ptr) - 1
    adjs = R.adjacency(ei[0], ei[1], ptr)
    rows = _run(ei, ptr, m, k, "sample", seed, p_restart, seeds, False)[1]
    cnt = collections.Counter()
    cnt[f"KM == {min(w for w in R.KM_WIDTHS if k <= w)}"] += 1
    cnt["k == KM"] += k in R.KM_WIDTHS
    wgs = (m + ROW_LANES - 1) // ROW_LANES                          # ugs_rwr.hip ugs_rwr_row_streams: `c.row_wgs`
    cnt["workgroups per graph > 1"] += wgs > 1
    cnt["short last workgroup"] += m % ROW_LANES != 0 and wgs > 1
    cnt["idle lanes"] += m % ROW_LANES != 0
    for g, adj in enumerate(adjs):
        n = len(adj)
        if n < k:
            cnt["T0"] += 1
            cnt["n == 0"] += n == 0
            continue
        assert 10 * n * k < 10 ** 5, "keep T below 10^5: no lane may run long"
        words = n + 1 + sum(len(a) for a in adj) + (n + 3) // 4
        place = "lds" if words <= R.RWR_LDS_INTS else "global"
        cnt[place] += 1
        if words in (R.RWR_LDS_INTS, R.RWR_LDS_INTS + 1):
            cnt[f"csr_words == {words}"] += 1
        if ptr[g] > ptr[0]:
            cnt[place + ", vbase > 0"] += 1
        mine = [r for r in rows if r.g == g]
        if p_restart >= 1.0 and k > 1:
            cnt["p1_shortcut"] += 1
        for i, r in enumerate(mine):
            cnt["doomed"] += r.doomed
            cnt["doomed_row0"] += r.doomed and r.s == 0
            cnt["doomed_row_last"] += r.doomed and r.s == m - 1
            cnt["doomed_twice"] += r.doomed and i > 0 and mine[i - 1].doomed
            cnt["live after doomed"] += (not r.doomed) and i > 0 and mine[i - 1].doomed
            cnt["doomed after live"] += r.doomed and i > 0 and not mine[i - 1].doomed
            cnt["live_failed"] += r.live_failed
            cnt["ran all T"] += r.live_failed and r.draws >= 1 + 10 * n * k
            cnt["found"] += r.found
            cnt["L > 64"] += (not r.doomed) and r.draws > 64
            cnt["L == 1"] += (not r.doomed) and r.draws == 1
        live = [r.draws for r in mine if not r.doomed]
        if len(live) > ROW_LANES and max(live) > 8 * (sum(live) / len(live)):
            cnt["long tail"] += 1                                   # a walk far longer than the mean in a full wave
    return +cnt, rows


def census(ei, ptr, m, k, seed, p_restart, seeds=None):
    return census_rows(ei, ptr, m, k, seed, p_restart, seeds)[0]
