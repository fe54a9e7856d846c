"""Inputs and the CPU model shared by tests/test_uniform_population_law.py (CPU) and tests/test_gpu_uniform_population.py (GPU):
the batch that walks the 16-lane fill of uni_pop_fill over its edges, and a Python restatement of that fill.

The fill gives every row a group of 16 lanes.  The graph's column bucket (its columns in batch column order) is taken in chunks of
16; in a chunk lane l looks at column base + l (none past the bucket's end), a hit being a column with both endpoints in the row's
subset; lane l writes its hit at w + (hits of the lanes below it in the chunk), and w then advances by the chunk's hits."""
import random

import numpy as np

import ugs_workloads as wl

LANES = 16
BUCKETS = (0, 1, 15, 16, 17, 33, 300)          # columns per bucket of the first graphs of lane_group_batch


def group_fill(hits, mutant=None):
    """Bucket positions of a row's edges in the order the 16-lane fill writes them.  hits[q]: column q of the bucket is an edge of
    the row.  mutant: None (the kernel), or one wrong line: "inclusive" (a lane writes at the inclusive prefix), "no_carry" (w is
    not advanced from chunk to chunk), "tail" (the last chunk's mask stops one column early)."""
    n = len(hits)
    end = n - 1 if mutant == "tail" else n
    out, w = {}, 0
    for base in range(0, n, LANES):
        lane = [1 if base + l < end and hits[base + l] else 0 for l in range(LANES)]
        incl = np.cumsum(lane).tolist()
        for l in range(LANES):
            if lane[l]:
                out[w + (incl[l] if mutant == "inclusive" else incl[l] - lane[l])] = base + l
        if mutant != "no_carry":
            w += incl[LANES - 1]
    return [out.get(i, -1) for i in range(max(out) + 1 if out else 0)]


def model_edges(edge_index, ptr, nodes, m, mode, mutant=None):
    """(edge_index [2, E], edge_ptr [rows + 1], edge_src [E]) of the rows `nodes` ([G * m, k] batch ids, -1 rows empty), every row
    filled by group_fill over its graph's bucket.  A slot the fill leaves unwritten holds -1."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    src, dst = ei[0], ei[1]
    eu, ev, es, eptr = [], [], [], [0]
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        bucket = np.nonzero((src >= lo) & (src < hi) & (dst >= lo) & (dst < hi))[0]
        for s in range(m):
            row = nodes[g * m + s]
            if row[0] >= 0:
                pos = {int(v): i for i, v in enumerate(row)}
                hits = [int(src[c]) in pos and int(dst[c]) in pos for c in bucket]
                for q in group_fill(hits, mutant):
                    c = int(bucket[q]) if q >= 0 else -1
                    u, v = (int(src[c]), int(dst[c])) if q >= 0 else (-1, -1)
                    eu.append(-1 if q < 0 else pos[u] if mode == "sample" else u)
                    ev.append(-1 if q < 0 else pos[v] if mode == "sample" else v)
                    es.append(c)
            eptr.append(len(es))
    return np.array([eu, ev], np.int64).reshape(2, -1), np.array(eptr, np.int64), np.array(es, np.int64)


def _bucket_graph(rng, cols):
    """(n, local columns [2, cols]): a connected graph whose bucket has exactly `cols` columns -- a path's edges first, then
    duplicates (either direction) and loops."""
    if cols == 0:
        return 3, np.zeros((2, 0), np.int64)
    n = min(cols + 1, 40)
    base = [(i, i + 1) for i in range(n - 1)]
    out = list(base)
    while len(out) < cols:
        r = rng.random()
        u, v = rng.choice(base)
        out.append((u, u) if r < 0.15 else (v, u) if r < 0.6 else (u, v) if r < 0.8 else tuple(rng.sample(range(n), 2)))
    return n, np.array(out, np.int64).T.reshape(2, -1)


def last_lane_graph():
    """4 vertices, 48 columns: the only edge {0, 1} sits at bucket positions 15, 31 and 47 (lane 15 of every chunk), every other
    column is a loop at 2 or 3.  k = 2: S = {{0, 1}}, so every row's hits are the last lane's alone."""
    cols = [(2, 2) if q % 2 else (3, 3) for q in range(48)]
    cols[15], cols[31], cols[47] = (0, 1), (1, 0), (0, 1)
    return 4, np.array(cols, np.int64).T.reshape(2, -1)


def lane_group_batch(G=40, seed=7):
    """([(n, local columns)] per graph, batch edge_index, ptr): the BUCKETS graphs, last_lane_graph, then random small graphs up to G;
    the batch's columns interleave the graphs (each graph's own order kept), with columns that cross graphs in between."""
    rng = random.Random(seed)
    graphs = [_bucket_graph(rng, c) for c in BUCKETS] + [last_lane_graph()]
    while len(graphs) < G:
        n = rng.randint(2, 20)
        graphs.append((n, wl.tu_graph(n, n - 1 + rng.randint(0, n), rng.randrange(1 << 30))))
    ptr = np.concatenate([[5], 5 + np.cumsum([n for n, _ in graphs])]).astype(np.int64)
    queues = [list((e + ptr[g]).T.tolist()) for g, (_, e) in enumerate(graphs)]
    cols = []
    while any(queues):
        for g, q in enumerate(queues):
            for _ in range(min(len(q), rng.randint(1, 5))):
                cols.append(q.pop(0))
            if rng.random() < 0.1:                                  # a column from this graph into the next: no graph's
                cols.append([int(ptr[g]), int(ptr[(g + 1) % G])])
    return graphs, np.ascontiguousarray(np.array(cols, np.int64).T.reshape(2, -1)), ptr
