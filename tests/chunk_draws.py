"""Inputs of tests/test_gpu_chunk_draws.py and the models its CPU tests (tests/test_chunk_draws.py) check them with.

The walk kernel's launch-uniform instantiation (one graph, one seed, rows by index: a single-graph call in the 448-candidate tier)
draws the random numbers of a whole work chunk at once (ugs_kernels.hip, chunk_draws): lane 16 r + j of the wave computes output
j + 1 of the generator of the chunk's row r, the chain s1 -> s2 -> ... running along the DPP row -- in every iteration a lane applies
the xorshift step to its left neighbour's value and lane j = 0 to the row's seed, so after t iterations lanes j < t are final.  With
k + 1 <= 16 numbers per row the walks then read their numbers out of those lanes; above that they run the sequential generator.

Restated here: the sequential generator (reference include/sampler.hpp:26-36, oracle/ugs_oracle.c), the lane pass as a numpy uint64
model, the chunk sizes of the dynamic work loop (chunk_for in ugs_walk_lds), and the graphs of the GPU cases."""
import random

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15
MULT = 2685821657736338717
LANES_PER_ROW, ROWS_PER_CHUNK = 16, 4

# the part the GPU tests run on: 256 compute units, 20 resident one-wave blocks each in the 448-candidate tier
CUS, WAVES_PER_CU = 256, 20
DYNAMIC_ABOVE = 64 * CUS           # rows: the host takes the dynamic work loop above 64 rows per compute unit


# ---------------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------------
def row_state(seed64, i):
    """the generator's first state for row i of a call with the 64-bit seed `seed64`, and whether the zero rule applied"""
    s = (seed64 + i * GOLDEN) & M64
    return (s or 1), s == 0


def sequential(seed64, i, count):
    """the first `count` outputs of row i's generator, one after the other (Python integers)"""
    s, _ = row_state(seed64, i)
    out = []
    for _ in range(count):
        s ^= s >> 12
        s ^= (s << 25) & M64
        s ^= s >> 27
        out.append((s * MULT) & M64)
    return out


def zero_state_seed(i):
    """the 64-bit seed for which row i starts from state 0"""
    return (-i * GOLDEN) & M64


def lane_pass(seed64, row0, iterations):
    """the lane pass as the kernel runs it: a [4, 16] uint64 array, entry [r, j] = lane 16 r + j after `iterations` iterations and
    the closing multiply.  The DPP shift is a shift of each 16-element row by one; lane 0 takes the row's seed instead."""
    with np.errstate(over="ignore"):
        rows = np.arange(ROWS_PER_CHUNK, dtype=np.uint64) + np.uint64(row0 & M64)
        s0 = np.uint64(seed64) + rows * np.uint64(GOLDEN)
        s0 = np.where(s0 == 0, np.uint64(1), s0)
        x = np.repeat(s0[:, None], LANES_PER_ROW, axis=1)                     # what the lanes hold before the first iteration is never used
        for _ in range(iterations):
            p = np.empty_like(x)
            p[:, 1:] = x[:, :-1]                                             # row_shr:1
            p[:, 0] = s0                                                     # ... and the lane without a left neighbour keeps `old`
            p ^= p >> np.uint64(12)
            p ^= p << np.uint64(25)
            p ^= p >> np.uint64(27)
            x = p
        return x * np.uint64(MULT)


# ---------------------------------------------------------------------------------------------------------------------------
# the dynamic work loop's chunks
# ---------------------------------------------------------------------------------------------------------------------------
def chunk_for(left, groups):
    return 4 if left > 8 * groups else (2 if left > 2 * groups else 1)


def chunk_sizes(rows):
    """(first chunk, the sizes the later chunks pass through, whether a chunk can be cut short by the row count) of a launch of `rows`
    rows, or None when the host takes the static split.  Every wave takes its first chunk by index; the later ones come from a counter
    and shrink with what is left, so a launch passes through every size below its first one on the way down."""
    if rows <= DYNAMIC_ABOVE:
        return None
    groups = min(rows, CUS * WAVES_PER_CU)
    first = chunk_for(rows, groups)
    left = rows - groups * first
    later = sorted({chunk_for(x, groups) for x in range(1, max(left, 0) + 1)}, reverse=True)
    cut_short = rows % 2 == 1 and (first > 1 or 2 in later)               # an odd row count ends inside a chunk of two or four
    return first, later, cut_short


# ---------------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------------
RING_N = 70000


def ring_with_chords(n=RING_N, chords=3, seed=20263):
    """a ring and `chords` random chords per vertex, each column listed once: n >= 65 536, the root reduction's division road"""
    rng = random.Random(seed)
    e = [(v, (v + 1) % n) for v in range(n)]
    for v in range(n):
        for _ in range(chords):
            w = rng.randrange(n)
            if w != v:
                e.append((v, w))
    rng.shuffle(e)
    return np.array(e, dtype=np.int64).T.reshape(2, -1).copy(), np.array([0, n], dtype=np.int64)


def pairs_graph(pairs=10):
    """disjoint pairs, both directions: at k = 3 no vertex is a viable root, so the plan relaxes to level 1 (uniform over the
    vertices with a neighbour later in the order: one of each pair) -- one root number, the first pick reads draw 1, and growth fails behind it"""
    e = [(2 * i, 2 * i + 1) for i in range(pairs)]
    e += [(v, u) for u, v in e]
    return np.array(e, dtype=np.int64).T.reshape(2, -1).copy(), np.array([0, 2 * pairs], dtype=np.int64)


def root_level(ei, n, k):
    """relaxation level of the plan of one graph, by the oracle's preprocessing (reference src/sampler.cpp:116-150)"""
    import oracle
    P = oracle.Preproc(ei, n, k)
    d = P.dump()
    P.close()
    if (d["bucket_b"] > 0.0).any():
        return 0
    return 1 if (d["suffix_deg"] > 0).any() else 2
