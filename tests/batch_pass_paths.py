"""batch_pass_paths.py -- the inputs that pin the device batch pass's kernel paths (csrc/ugs_batch.hip), shared by the CPU tests
(tests/test_batch_pass_law.py: law against the oracle, census, device model, mutants) and the GPU tests
(tests/test_gpu_batch_pass_paths.py).  Every case names in `reaches` the census classes (batch_pass_law.census) it is there for.
The shapes are derived from the kernels' constants -- quarters of ((E + 3) / 4 rounded up to 64) columns, 512 kept ballots per
wave, rounds of 256 columns, chunks of 64 endpoints -- and both test files assert the classes again, so an input that stops
reaching its path fails instead of losing coverage.

Case: ei, ptr, k; lim = the column limit in force (1000: the pass as it always was; above: the large form); fused_work = None
(the kernel's threshold) or the value of UGS_BP_FUSED_WORK; hand_over: the pass must give the call to the general path;
both = the case also runs in the two-kernel variant; large_too = it also runs with the limit at 8192 (same law)."""
import collections
import functools
import random

import numpy as np

import batch_pass_law as L

Case = collections.namedtuple("Case", "name ei ptr k lim fused_work hand_over both large_too cold_too reaches")
STRAY = 1 << 40


def batch_of(graphs, first=0):
    """(ei, ptr) of graphs given as (n, columns local to the graph)"""
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(np.asarray(ei, np.int64).reshape(2, -1) + ptr[-1])
        ptr.append(ptr[-1] + n)
    return np.ascontiguousarray(np.concatenate(cols, axis=1)), np.array(ptr, np.int64)


def arr(pairs):
    return np.array(pairs, np.int64).reshape(-1, 2).T


def both_ways(pairs):
    return arr(list(pairs) + [(v, u) for u, v in pairs])


def er(n, p, seed):
    r = random.Random(seed)
    return n, both_ways([(u, v) for u in range(n) for v in range(u + 1, n) if r.random() < p])


def path(n, chords=0, seed=0, upto=None):
    """a path over the first `upto` vertices (all of them by default) plus random chords over all n"""
    r = random.Random(seed)
    return n, arr([(i, i + 1) for i in range((upto or n) - 1)] + [(r.randrange(n), r.randrange(n)) for _ in range(chords)])


def cycle(n):
    return n, both_ways([(i, (i + 1) % n) for i in range(n)])


def star(leaves):
    return leaves + 1, arr([(0, i + 1) for i in range(leaves)])


def random_cols(n, cols, seed):
    """a path over a shuffled vertex order, then random pairs (loops and repeats allowed), exactly `cols` columns, shuffled"""
    nr = np.random.default_rng(seed)
    order = nr.permutation(n)
    e = np.concatenate([np.stack([order[:-1], order[1:]])[:, :cols], nr.integers(0, n, size=(2, max(cols - (n - 1), 0)))], axis=1)
    return n, np.ascontiguousarray(e[:, nr.permutation(cols)].astype(np.int64))


def scattered(E, graphs, positions, seed):
    """E columns: graph i's columns (local ids) at the batch positions positions[i] (ascending), every other column stray --
    cross-graph pairs, -1, ptr[G], 2^40 in turn"""
    ptr = np.cumsum([0] + [n for n, _ in graphs]).astype(np.int64)
    r = random.Random(seed)
    G, total = len(graphs), int(ptr[-1])
    ei = np.empty((2, E), np.int64)
    kind = np.arange(E) % 4
    a, b = np.array([r.randrange(G) for _ in range(1024)]), np.array([r.randrange(1, G) for _ in range(1024)])
    ga, gb = a[np.arange(E) % 1024], (a[np.arange(E) % 1024] + b[np.arange(E) % 1024]) % G            # two different graphs
    ei[0], ei[1] = ptr[ga], ptr[gb + 1] - 1
    ei[0][kind == 1] = -1
    ei[1][kind == 2] = total
    ei[0][kind == 3] = STRAY
    for (n, cols), pos, lo in zip(graphs, positions, ptr):
        assert len(pos) == cols.shape[1]
        ei[:, pos] = cols + lo
    return np.ascontiguousarray(ei), ptr


def spread(E, count, shift):
    """`count` ascending positions over [0, E) touching the first and last column of every wave quarter"""
    qs = L.quarters(E)
    edge = sorted({w0 + shift for w0, w1 in qs} | {w1 - 1 - shift for w0, w1 in qs})
    rest = np.linspace(shift + 7, E - 9 - shift, count - len(edge)).astype(np.int64).tolist()
    out = sorted(set(edge) | set(rest))
    assert len(out) == count, (len(out), count)
    return np.array(out)


def many_small(seed=99):
    """the 900-graph batch of tests/test_gpu_batch_pass.py: G * E above 4 Mi"""
    rng = random.Random(seed)
    cols, ptr = [], [0]
    for g in range(900):
        n = rng.choice([0, 2, 4, 5, 6, 7, 9])
        e = [(u + ptr[-1], v + ptr[-1]) for u in range(n) for v in range(u + 1, n) if rng.random() < 0.5]
        cols += e + [(v, u) for u, v in e]
        ptr.append(ptr[-1] + n)
    cols += [(rng.randrange(ptr[-1]), rng.randrange(ptr[-1])) for _ in range(50)]
    rng.shuffle(cols)
    return arr(cols).copy(), np.array(ptr, np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, batch, k, reaches, lim=1000, fused_work=None, hand_over=False, both=True, large_too=False, cold_too=False):
        ei, ptr = batch
        out.append(Case(name, np.ascontiguousarray(ei), np.asarray(ptr, np.int64), k, lim, fused_work, hand_over, both, large_too, cold_too, tuple(reaches)))

    # ---- fused compaction ----
    add("fused_small", batch_of([er(9, 0.4, 1), er(7, 0.5, 2), cycle(5)]), 3, ["fused, empty quarter", "degree tie"])
    r = random.Random(600)
    A, B = er(30, 0.4, 3), er(12, 0.5, 4)
    a_cols = A[1][:, [r.randrange(A[1].shape[1]) for _ in range(301)]]
    b_cols = B[1][:, [r.randrange(B[1].shape[1]) for _ in range(34)]]
    add("fused_straddle", scattered(600, [(30, a_cols), (12, b_cols), (6, np.zeros((2, 0), np.int64))],
                                    [np.arange(150, 451), np.array(list(range(10)) + list(range(576, 600))), np.zeros(0, np.int64)], 5),
        4, ["fused, straddles quarter", "fused, partial chunk", "cross-graph column", "cn == 0"])
    four = [er(9, 0.5, 10 + i) for i in range(4)]
    for E, name, reaches in ((131072, "keep_512", ["keep, 512 chunks"]), (131073, "keep_and_no_keep", ["no keep", "keep and no keep in one block"])):
        graphs, pos = [], []
        for i, (n, e) in enumerate(four):
            cnt = 40 + i
            graphs.append((n, e[:, np.arange(cnt) % e.shape[1]]))
            pos.append(spread(E, cnt, i))
        add(name, scattered(E, graphs, pos, E), 4, reaches + ["fused, straddles quarter", "cross-graph column"])
    add("no_keep_large", batch_of([random_cols(300, 7790 + g, 700 + g) for g in range(17)]), 5, ["no keep, large", "fused, straddles quarter", "strided s == 15"],
        lim=8192)
    # ---- two kernels ----
    add("two_kernels_900", many_small(), 4, ["two kernels, G * E > 4 Mi", "span > 256", "foreign inside span", "cross-graph column"], both=False)
    sh = batch_of([er(20, 0.5, 20), er(24, 0.5, 21), er(18, 0.6, 22)])
    sh = (sh[0][:, np.random.default_rng(7).permutation(sh[0].shape[1])], sh[1])
    add("span_rounds", sh, 5, ["span > 256", "foreign inside span"], fused_work=0, both=False)
    r = random.Random(40)
    graphs = []
    for g in range(40):
        if g % 5 == 2:
            graphs.append((0, np.zeros((2, 0), np.int64)))                    # empty: shares its ptr value with the next graph
        elif g % 7 == 3:
            graphs.append((2, arr([(0, 1)])))                                # n < k between live ones
        else:
            n = r.choice([3, 4, 5])
            graphs.append((n, arr([(r.randrange(n), r.randrange(n)) for _ in range(r.choice([1, 2, 3]))])))
    ei, ptr = batch_of(graphs, first=5)
    stray = arr([(int(ptr[3]), int(ptr[9])), (-1, 6), (int(ptr[-1]), 7), (STRAY, 8), (4, 6), (int(ptr[20]), int(ptr[21]))])
    ei = np.concatenate([ei[:, :30], stray[:, :3], ei[:, 30:], stray[:, 3:]], axis=1)
    add("assign_many", (ei, ptr), 3, ["assign, many graphs per wave", "assign, shared ptr value", "cross-graph column", "stray column"], fused_work=0, both=False)
    # ---- column bounds ----
    edgeless = (6, np.zeros((2, 0), np.int64))
    add("cols_1000", batch_of([er(8, 0.5, 30), random_cols(60, 1000, 31), edgeless]), 4, ["cn == 0", "cn == lim"])
    add("cols_1001_hands_over", batch_of([er(8, 0.5, 30), random_cols(60, 1001, 32)]), 4, ["cn == lim + 1"], hand_over=True)
    add("cols_8192", batch_of([random_cols(500, 8192, 33), edgeless, er(8, 0.5, 30)]), 4, ["cn == 0", "cn == lim", "strided s == 16"], lim=8192)
    add("cols_8193_hands_over", batch_of([er(8, 0.5, 30), random_cols(500, 8193, 34)]), 4, ["cn == lim + 1"], lim=8192, hand_over=True)
    # ---- vertex bounds ----
    add("n256_257", batch_of([path(256, 40, 40), path(257, 40, 41)]), 4, ["n == 256", "n == 257"], large_too=True)
    add("n2048", batch_of([path(2048, 300, 42, upto=600), er(8, 0.5, 30)]), 4, ["n == 2048", "empty row"], large_too=True)
    add("n2049_hands_over", batch_of([er(8, 0.5, 30), path(2049, 300, 43, upto=600)]), 4, ["n == 2049"], hand_over=True)
    # ---- key chain ----
    add("key_63_64_65", batch_of([random_cols(20, c, 50 + c) for c in (63, 64, 65)]), 4, ["ns == 63", "ns == 64", "ns == 65"], large_too=True)
    add("key_strided", batch_of([random_cols(200, 1001, 60), random_cols(210, 1499, 61), random_cols(220, 1500, 62), random_cols(230, 8192, 63)]), 5,
        ["strided s == 2", "strided s == 3", "strided s == 16"], lim=8192)
    # ---- CSR placement: 40 loops on vertex 41 (endpoints 0 .. 79: chunk 0 is one row), a star of 40 leaves, one pair 70 times, an
    #      isolated vertex (44) ----
    st = arr([(0, i + 1) if i < 20 else (i + 1, 0) for i in range(40)])     # the hub on even lanes, then on odd ones: bits left in MSK would count
    place = np.concatenate([arr([(41, 41)] * 40), st, arr([(42, 43)] * 70)], axis=1)
    add("placement", batch_of([er(6, 0.6, 70), (45, place)]), 3,
        ["row fills a chunk", "row over chunks", "two rows share a chunk", "loop", "empty row", "last chunk partial"], large_too=True)
    # ---- ugs_bp_roots: the searches ----
    add("path40_k32", batch_of([path(40), er(40, 0.3, 0)]), 32, ["k == 32", "reaches k at the last neighbour", "second level needed", "unreachable among reachable", "b inexact"],
        large_too=True, cold_too=True)
    add("n64_n65", batch_of([er(64, 0.08, 80), er(65, 0.08, 81)]), 6, ["mask search n == 64", "list search n == 65", "mask search, vertex >= 32 reached", "second level needed"],
        large_too=True, cold_too=True)
    add("n300", batch_of([path(300, 60, 82)]), 7, ["n > 256", "second level needed"], large_too=True, cold_too=True)
    add("n1024_1025", batch_of([path(1024, 100, 83, upto=800), path(1025, 100, 84, upto=800)]), 4, ["n == 1024", "n == 1025 host"], large_too=True, cold_too=True)
    # ---- alias loop ----
    add("star_k1", batch_of([star(12), er(10, 0.4, 85)]), 1, ["k == 1", "no small stack"], cold_too=True)
    hubs = both_ways([(0, i) for i in range(2, 12)] + [(1, i) for i in range(7, 20)] + [(0, 1)])
    hubs = np.concatenate([hubs, arr([(5, 5), (1, 1)])], axis=1)                                   # loops on reachable roots
    add("two_hubs", batch_of([(20, hubs), star(9)]), 3, ["demotion", "no demotion", "demoted one popped next", "loop"], large_too=True, cold_too=True)
    # ---- floating point: inputs on which another association of the same formula gives another double (found by the census) ----
    add("fp_er40_k12", batch_of([er(40, 0.3, 0), er(40, 0.3, 3)]), 12, ["scale association matters", "alias association matters", "leftover small", "leftover large"],
        large_too=True, cold_too=True)
    # ---- levels ----
    add("pairs_k3", batch_of([(20, both_ways([(2 * i, 2 * i + 1) for i in range(10)])), er(8, 0.5, 30)]), 3, ["level 1", "level 0"], large_too=True, cold_too=True)
    add("edgeless_k2", batch_of([(7, np.zeros((2, 0), np.int64)), er(8, 0.5, 30)]), 2, ["level 2", "cn == 0"], large_too=True, cold_too=True)
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def fused_work_of(c, variant="default"):
    """the threshold a variant of the case runs under: "default" is the case's own, "two" forces the two-kernel variant, "fused" is the kernel's threshold"""
    if variant == "two":
        return 0
    if variant == "fused":
        return L.FUSED_WORK
    return L.FUSED_WORK if c.fused_work is None else c.fused_work


@functools.lru_cache(maxsize=None)
def census_of(name, variant="default", lim=None):
    c = case(name)
    return L.census(c.ei, c.ptr, c.k, c.lim if lim is None else lim, fused_work_of(c, variant))


@functools.lru_cache(maxsize=None)
def law_of(name):
    """per graph the law (None for a degenerate graph); for a hand-over case only the graphs inside the limits"""
    c = case(name)
    out = []
    for g in range(len(c.ptr) - 1):
        n = int(c.ptr[g + 1] - c.ptr[g])
        skip = n > L.MAX_N or len(L.owned(c.ei, c.ptr[g], c.ptr[g + 1])) > L.COLS_CEIL + 1
        out.append(None if skip else L.graph_law(c.ei, c.ptr, g, c.k))
    return out
