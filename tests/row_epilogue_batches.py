"""Inputs of tests/test_gpu_row_epilogue_batches.py and the classification of the oracle's rows they are chosen by.

The walk kernel's dynamic work loop hands a wave its rows in chunks; with more than 8 rows per resident wave the first chunk of
every wave is four consecutive rows, wave i taking rows 4i .. 4i + 3.  A part with 256 compute units keeps at most 20 waves per
unit resident in the 448-candidate tier and 12 in the 704-candidate tier, so a call of 49 152 rows (> 8 * 5120) starts every wave
with a chunk of four, and at least its first 4 * 3072 = 12 288 rows -- the first quarter -- are handed out as aligned blocks of four.
Rows of such a block share one batched epilogue (ugs_kernels.hip, Parked); what a row is decides whether it is parked for it:

  fast      complete, 1..8 hits, no self hit        parked, ranked by the batch
  self      complete, at most 8 hits, a self hit    epilogue on the spot (told by its edge-entry count: odd one out of 2 per hit)
  general   complete, 9..32 hits                    epilogue on the spot
  unstaged  complete, more than 32 hits             epilogue on the spot, the row is listed for the row-reading fill
  degenerate  graph of fewer than k vertices        rows of -1, written before the walk starts
  incomplete  growth failed                         -1 padded, no edges, epilogue on the spot
  handed_on   the walk outgrows 448 candidates      no epilogue in this tier at all

(a hit = one adjacency entry of a newly added vertex that points into the sample; by the oracle's rows: the row's entries with
source != target, halved, plus its entries with source == target.)  A handed-on walk cannot be told from its row -- the next tier
finishes it like any other -- but from its graph: every connected 8-subgraph of a star holds the centre, whose row is scanned while
the sample still grows and adds every leaf to the candidates; 600 leaves are more than the tier's 448."""
import random

import numpy as np

ROWS, M, K = 49152, 6, 8
QUARTER = ROWS // 4
FAST, SELF, GENERAL, UNSTAGED, DEGENERATE, INCOMPLETE, HANDED_ON = "fast", "self", "general", "unstaged", "degenerate", "incomplete", "handed_on"
OTHERS = (SELF, GENERAL, UNSTAGED, DEGENERATE, INCOMPLETE, HANDED_ON)
STAR_LEAVES = 600


def _tree(rng, n, off):
    return [(off + rng.randrange(v), off + v) if rng.random() < 0.5 else (off + v, off + rng.randrange(v)) for v in range(1, n)]


def _graph(rng, kind, off):
    """(columns, vertices) of one graph of `kind`, numbered from `off`"""
    if kind == "tree":
        n = rng.randint(9, 40)
        return _tree(rng, n, off), n
    if kind == "tree_plus_one":                      # K vertices, K edges: every complete row holds all of them -- exactly 8 hits
        e = _tree(rng, K, off)
        have = {frozenset(c) for c in e}
        while len(e) < K:
            u, v = rng.sample(range(K), 2)
            if frozenset((off + u, off + v)) not in have:
                have.add(frozenset((off + u, off + v)))
                e.append((off + u, off + v))
        return e, K
    if kind == "self_loops":                         # a tree of which every third vertex carries a self loop
        n = rng.randint(9, 24)
        return _tree(rng, n, off) + [(off + v, off + v) for v in range(rng.randrange(3), n, 3)], n
    if kind == "dense":                              # 14 vertices: 9..28 hits at k = 8
        return [(off + u, off + v) for u in range(14) for v in range(u + 1, 14) if rng.random() < 0.7], 14
    if kind == "complete_twice":                     # every edge of K9 listed twice: 56 hits at k = 8
        e = [(off + u, off + v) for u in range(9) for v in range(u + 1, 9)]
        return e + e, 9
    if kind == "small":                              # fewer than k vertices
        n = rng.randint(2, 5)
        return _tree(rng, n, off), n
    if kind == "two_components":                     # 5 + 5 vertices: no component holds 8
        return _tree(rng, 5, off) + _tree(rng, 5, off + 5), 10
    if kind == "star":
        return [(off, off + v) for v in range(1, STAR_LEAVES + 1)], STAR_LEAVES + 1
    raise KeyError(kind)


KIND_WEIGHTS = [("tree", 0.37), ("tree_plus_one", 0.08), ("self_loops", 0.11), ("dense", 0.11), ("complete_twice", 0.11), ("small", 0.11),
                ("two_components", 0.11)]
STAR_EVERY = 16        # pairs of graphs (2p, 2p + 1): every 16th pair is (star, tree) or (tree, star) in turn -- a star costs the oracle most


def mixed_batch(graphs=ROWS // M, seed=20261):
    """(edge_index, ptr, kinds): `graphs` graphs of kinds drawn by KIND_WEIGHTS, the stars at fixed places beside a tree (m = 6: the
    aligned block that spans graphs 2p and 2p + 1 holds two rows of each); columns shuffled inside each graph"""
    rng = random.Random(seed)
    names, weights = [n for n, _ in KIND_WEIGHTS], [w for _, w in KIND_WEIGHTS]
    cols, ptr, kinds = [], [0], []
    for g in range(graphs):
        kind = rng.choices(names, weights)[0]
        if (g // 2) % STAR_EVERY == 0:
            kind = "star" if g % 2 == (g // (2 * STAR_EVERY)) % 2 else "tree"
        e, n = _graph(rng, kind, ptr[-1])
        rng.shuffle(e)
        cols += e
        ptr.append(ptr[-1] + n)
        kinds.append(kind)
    return np.array(cols, dtype=np.int64).T.reshape(2, -1).copy(), np.array(ptr, dtype=np.int64), kinds


def sparse_graph(n=300, extra=12, seed=20262):
    """one tree-like graph: a random tree and a few more edges, each listed once"""
    rng = random.Random(seed)
    e = _tree(rng, n, 0) + [tuple(rng.sample(range(n), 2)) for _ in range(extra)]
    rng.shuffle(e)
    return np.array(e, dtype=np.int64).T.reshape(2, -1).copy(), np.array([0, n], dtype=np.int64)


def classify_rows(result, ptr, kinds, m, k, rows):
    """kind of each of the first `rows` rows of one oracle result of the mixed batch"""
    nodes, edge_index, edge_ptr = result[0], result[1], result[2]
    out = []
    for r in range(rows):
        g = r // m
        nd = nodes[r]
        lo, hi = int(edge_ptr[r]), int(edge_ptr[r + 1])
        if (nd < 0).all():
            assert hi == lo
            out.append(DEGENERATE)
        elif (nd < 0).any():
            assert hi == lo
            out.append(INCOMPLETE)
        elif kinds[g] == "star":
            assert int(ptr[g]) in nd.tolist() and hi - lo == 2 * (k - 1)        # the centre and k - 1 leaves
            out.append(HANDED_ON)
        else:
            s = int((edge_index[0, lo:hi] == edge_index[1, lo:hi]).sum())
            assert (hi - lo - s) % 2 == 0
            hits = (hi - lo - s) // 2 + s
            assert hits >= k - 1
            out.append(UNSTAGED if hits > 32 else (GENERAL if hits > 8 else (SELF if s else FAST)))
    return out


def census(row_kinds, m):
    """{name: aligned four-row blocks of that description}"""
    seen = {"four_fast": 0, "two_graphs": 0}
    for x in OTHERS:
        for p in range(4):
            seen[f"{x}_at_{p}_beside_fast"] = 0
    for b in range(len(row_kinds) // 4):
        blk = row_kinds[4 * b:4 * b + 4]
        if all(x == FAST for x in blk):
            seen["four_fast"] += 1
        if (4 * b) // m != (4 * b + 3) // m:
            seen["two_graphs"] += 1
        if FAST in blk:
            for p, x in enumerate(blk):
                if x != FAST:
                    seen[f"{x}_at_{p}_beside_fast"] += 1
    return seen
