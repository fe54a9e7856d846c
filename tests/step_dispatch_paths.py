"""step_dispatch_paths.py -- inputs and census for what a growth step of the 448-candidate walk tier does BETWEEN its stage routines
(ss-gnn_amd/csrc/ugs_kernels.hip, select_lds and the upkeep behind the pick in do_walk): which final serves the step, which stages are
brought up to date in front of it, and what the pick leaves valid.

A step with c candidates runs the final of stage fs = order_stage_law.final_stage(c) in the variant for ceil(c / 64) elements per lane:
the leaf is a function of c alone, and the leaves change at the thresholds THRESHOLDS.  In front of it the step materialises the stages
nvalid .. fs - 1 (`need`, a bit per stage); behind the pick of position q every stage whose candidates do not all precede q is
dropped: nvalid = min(nvalid, number of chain values <= q).  The last pick of a complete sample keeps nothing up to date.

`replay` follows every row of the oracle through its growth steps -- the candidate list D is rebuilt from the oracle's own adjacency
and vertex order (Preproc.dump), the picks are the row's vertices in growth order -- and `census` names each step's classes.  The
GPU test runs the same inputs through the sampler; the CPU test asserts that the inputs cover every class of CLASSES.
"""
import numpy as np

import oracle
import order_stage_law as L

CAP = 448
NST = 5                                           # stages the tier ever materialises: 13, 29, 59, 127, 257
ROWS = 2000
# c at which the leaf of a step changes: the chain values (the final's stage) and the variants' elements per lane (64 j)
THRESHOLDS = [13, 29, 59, 64, 127, 128, 192, 256, 257, 320, 384]
# every c whose step the GPU test must have run: both sides of every threshold, and one value in the last leaf
C_VALUES = [13, 14, 29, 30, 59, 60, 64, 65, 127, 128, 129, 192, 193, 256, 257, 258, 320, 321, 384, 385]
CLASSES = ([f"c={c}" for c in C_VALUES] + ["c>385"] + ["need=none"] + [f"need=stage{i}" for i in range(NST)]
           + ["need=run2", "need=run5", "keep=to0", "keep=same"])


def leaf_of(c):
    """(lowest c, highest c) of the leaf that serves a step with c candidates"""
    lo = max([0] + [t for t in THRESHOLDS if t < c]) + 1
    hi = min([t for t in THRESHOLDS if t >= c] + [CAP])
    return lo, hi


def _sparse(rng, lo, hi, deg):
    n = hi - lo
    ring = np.stack([np.arange(lo, hi), lo + (np.arange(n) + 1) % n])
    m = n * (deg - 2) // 2
    u, v = rng.integers(lo, hi, m), rng.integers(lo, hi, m)
    keep = u != v
    return np.concatenate([ring, np.stack([u[keep], v[keep]])], axis=1).astype(np.int64)


def rows_of_exact_length(rng, n, lengths, deg=6):
    """vertex i < len(lengths) gets exactly lengths[i] entries: that many distinct ordinary vertices, no other column touches it
    (the construction of tests/test_gpu_chunk_paths.py)"""
    s = len(lengths)
    cols = [_sparse(rng, s, n, deg)]
    for i, d in enumerate(lengths):
        nb = rng.choice(np.arange(s, n), size=d, replace=False)
        cols.append(np.stack([np.full(d, i), nb]).astype(np.int64))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def sym_rows(ei, n):
    rows = [[] for _ in range(n)]
    for u, v in ei.T.tolist():
        rows[u].append(v)
        rows[v].append(u)
    return rows


def replay(ei, ptr, m, k, nodes):
    """Growth steps of every oracle row: a list of (row, step, c, need, nvalid_before_keep, keep or None for the last pick).
    `nodes` is the oracle's nodes output for (ei, ptr, m, k); a row that is not complete is followed as far as it goes."""
    ei, ptr, nodes = np.asarray(ei), np.asarray(ptr), np.asarray(nodes)
    steps = []
    for g in range(len(ptr) - 1):
        lo, n = int(ptr[g]), int(ptr[g + 1] - ptr[g])
        rows = nodes[g * m:(g + 1) * m]
        if n < k or n <= 0:
            assert (rows == -1).all(), "a degenerate graph's rows are -1"
            continue
        sel = (ei[0] >= lo) & (ei[0] < lo + n)
        pre = oracle.Preproc(ei[:, sel] - lo, n, k)
        d = pre.dump()
        pre.close()
        indptr, indices, index_of = d["indptr"], d["indices"], d["index_of"]
        for r, row in enumerate(rows):
            sample = [int(x) - lo for x in row if x >= 0]
            root_vi = int(index_of[sample[0]])
            seen, D, nvalid = {sample[0]}, [], 0
            for s in range(len(sample)):
                v = sample[s]
                if s == k - 1:
                    break                                                    # the last vertex's row adds no candidates
                for w in indices[indptr[v]:indptr[v + 1]].tolist():
                    if w not in seen and index_of[w] >= root_vi:
                        seen.add(w)
                        D.append(w)
                c = len(D)
                if c == 0 or c > CAP or s + 1 >= len(sample):
                    assert c == 0 or c > CAP or s + 1 < len(sample) or len(sample) == k, "a row ends early only without candidates"
                    break
                fs = L.final_stage(c)
                need = ((1 << fs) - 1) & ~((1 << nvalid) - 1)
                nvalid = max(nvalid, fs)
                q = D.index(sample[s + 1])                                   # the oracle's pick is a candidate: the replay follows the oracle
                keep = None
                if s + 2 < k:
                    keep = sum(1 for b in L.CHAIN[:NST] if b <= q)
                steps.append((g * m + r, s, c, need, nvalid, keep))
                if keep is not None:
                    nvalid = min(nvalid, keep)
                D.pop(q)
    return steps


def census(steps):
    """class name -> number of steps"""
    out = {name: 0 for name in CLASSES}
    for _, _, c, need, nvalid, keep in steps:
        if c in C_VALUES:
            out[f"c={c}"] += 1
        elif 385 < c <= CAP:
            out["c>385"] += 1
        if need == 0:
            out["need=none"] += 1
        else:
            bits = [i for i in range(NST) if need >> i & 1]
            assert bits == list(range(bits[0], bits[-1] + 1)), "stages nvalid .. fs - 1: a run"
            if len(bits) == 1:
                out[f"need=stage{bits[0]}"] += 1
            if len(bits) == 2:
                out["need=run2"] += 1
            if len(bits) == NST:
                out["need=run5"] += 1
        if keep is not None and nvalid > 0:
            if keep == 0:
                out["keep=to0"] += 1
            if keep >= nvalid:
                out["keep=same"] += 1
    return out


# ---- the inputs: name -> (edge_index, ptr, k).  Rows of exact lengths put a walk's first step at a chosen c (a root's candidates are
#      its neighbours behind it in the vertex order; the census says what came of it), the ordinary vertices' degree spreads the rest.
def _spread(seed, n, lengths, deg):
    return rows_of_exact_length(np.random.default_rng(seed), n, lengths, deg)


def cases():
    out = {}
    # one graph, k = 8: three densities, so that c wanders over the whole range of the tier
    out["low"] = (_spread(1, 700, [13, 14, 15, 29, 30, 31, 59, 60, 61, 64, 65, 66], 8), np.array([0, 700], np.int64), 8)
    out["mid"] = (_spread(2, 700, [127, 128, 129, 130, 192, 193, 194, 200, 256, 257], 30), np.array([0, 700], np.int64), 8)
    out["high"] = (_spread(3, 700, [258, 259, 300, 320, 321, 322, 384, 385, 386, 400, 420, 440], 60), np.array([0, 700], np.int64), 8)
    out["k2"] = (_spread(4, 400, [13, 29, 59, 64, 65, 128, 129, 257, 258, 385], 12), np.array([0, 400], np.int64), 2)
    out["k3"] = (_spread(5, 400, [14, 30, 60, 127, 193, 256, 321, 384], 20), np.array([0, 400], np.int64), 3)
    # two graphs: the instantiation that is not specialised for one graph
    rng = np.random.default_rng(6)
    g0 = rows_of_exact_length(rng, 300, [64, 65, 128, 200], 16)
    g1 = _sparse(rng, 0, 400, 40) + 300
    out["two_graphs"] = (np.ascontiguousarray(np.concatenate([g0, g1], axis=1)), np.array([0, 300, 700], np.int64), 8)
    # a batch with a degenerate graph (fewer vertices than k) between two ordinary ones
    rng = np.random.default_rng(7)
    a = _sparse(rng, 0, 250, 24)
    b = np.array([[250, 251, 252], [251, 252, 250]], np.int64)               # three vertices: no sample of eight
    c = _sparse(rng, 0, 300, 12) + 253
    out["degenerate"] = (np.ascontiguousarray(np.concatenate([a, b, c], axis=1)), np.array([0, 250, 253, 553], np.int64), 8)
    return out


_oracle_rows = {}


def oracle_rows(name, mode="sample", seed=42):
    """the oracle's four outputs for a case, computed once per process"""
    key = (name, mode, seed)
    if key not in _oracle_rows:
        ei, ptr, k = cases()[name]
        _oracle_rows[key] = oracle.sample_batch(ei, ptr, ROWS // (len(ptr) - 1), k, mode, seed)
    return _oracle_rows[key]
