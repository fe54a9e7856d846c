"""The law of uniform_sampler.sample_distinct (include/ugs_mi355.h at ugs_uniform_distinct_begin) restated in plain Python, a model of
how uni_draw_distinct (ugs_uniform.hip) resolves it in parallel, and the batches the GPU test samples, with a census of the classes
of that resolution they reach.  Nothing here calls the library.

law(s, N, m)    the sequential definition: a partial Fisher-Yates shuffle over a dict that stands for the identity array
model(s, N, m)  the kernel's way: every step's target on its own, the keys (t_j << 32) | j sorted behind padding, the value that
                earlier steps left at a target read off the sorted keys (pred, w).  Keyword arguments switch on one-line mutants.
"""
import bisect
from math import comb

import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
MAX_M = 4096


def mix(z):
    """SplitMix64's finaliser"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def target(s0, N, j, n_minus_j=True):
    """t_j; s0 = mix(seed)"""
    return j + ((mix(s0 + (j + 1) * GAMMA) * (N - j if n_minus_j else N)) >> 64)


def law(s, N, m):
    """Graph rows 0 ... m-1 as population indices, -1 for a row of -1"""
    if N <= 0:
        return [-1] * m
    if m >= N:
        return list(range(N)) + [-1] * (m - N)
    a, s0, rows = {}, mix(s), []
    for j in range(m):
        t = target(s0, N, j)
        aj, at = a.get(j, j), a.get(t, t)
        a[j], a[t] = at, aj
        rows.append(at)
    return rows


def model(s, N, m, *, pred_last=False, follow_w=True, pad_first=False, n_minus_j=True):
    """uni_draw_distinct.  Mutants: pred_last (pred takes the last step with that target instead of the last earlier one), follow_w =
    False (w not followed), pad_first (padding keys that sort first), n_minus_j = False (N - j read as N)."""
    if N <= m:
        return [j if j < N else -1 for j in range(m)]
    P = 1
    while P < m:
        P <<= 1
    s0 = mix(s)
    t = [target(s0, N, j, n_minus_j) for j in range(m)]
    keys = sorted([(t[j] << 32) | j for j in range(m)] + [0 if pad_first else M64] * (P - m))[:m]     # the search sees m keys

    def pred(tt, j):
        pos = bisect.bisect_left(keys, ((tt + 1) << 32) if pred_last else ((tt << 32) | j))
        if pos == 0:
            return -1
        below = keys[pos - 1]
        return below & 0xFFFFFFFF if below >> 32 == tt and (not pred_last or below & 0xFFFFFFFF != j) else -1

    rows = []
    for j in range(m):
        x = pred(t[j], j)
        if x < 0:
            rows.append(t[j])
            continue
        while follow_w:
            y = pred(x, x)
            if y < 0 or y >= x:                                     # (y >= x: only a mutant's pred; the law's chain decreases)
                break
            x = y
        rows.append(x)
    return rows


MUTANTS = {"pred_last": dict(pred_last=True), "w_not_followed": dict(follow_w=False), "padding_first": dict(pad_first=True),
           "N_for_N_minus_j": dict(n_minus_j=False)}

# ---- the classes of the resolution ----
CLASSES = ("self_swap", "shared_target_ge_m", "own_place_targeted", "chain_ge_2", "pred_with_chain", "pred_with_chain_ge_2", "sort_padding",
           "full_width", "q_1", "m_eq_N_minus_1", "m_eq_N", "m_gt_N", "N_eq_1", "dead_between_live")


def census(sizes, seeds, m):
    """The classes one call reaches: sizes[g] = N_g (<= 0: nothing to draw from), seeds[g], m rows per graph."""
    out = set()
    hit = lambda name, cond=True: out.add(name) if cond else None    # noqa: E731
    live = [N > 0 for N in sizes]
    hit("dead_between_live", any(not live[g] and any(live[:g]) and any(live[g + 1:]) for g in range(len(sizes))))
    for N, s in zip(sizes, seeds):
        if N <= 0 or m == 0:
            continue
        hit("q_1", min(m, N) == 1)
        hit("m_eq_N_minus_1", m == N - 1)
        hit("m_eq_N", m == N)
        hit("m_gt_N", m > N)
        hit("N_eq_1", N == 1)
        if m >= N:
            continue
        hit("sort_padding", m & (m - 1) != 0)
        hit("full_width", m == MAX_M and N > MAX_M)
        s0 = mix(s)
        t = [target(s0, N, j) for j in range(m)]
        hit("self_swap", any(t[j] == j for j in range(m)))
        big = [x for x in t if x >= m]
        hit("shared_target_ge_m", len(set(big)) < len(big))
        last = {}                                                   # target -> the last step so far that took it
        chain = [0] * m                                             # hops of w from step i
        for j in range(m):
            if j in last:                                           # pred(j, j)
                chain[j] = chain[last[j]] + 1
                hit("own_place_targeted")
                hit("chain_ge_2", chain[j] >= 2)
            if t[j] in last:                                        # pred(t_j, j)
                hit("pred_with_chain", chain[last[t[j]]] >= 1)
                hit("pred_with_chain_ge_2", chain[last[t[j]]] >= 2)
            last[t[j]] = j
    return out


# ---- graphs whose population size is known in closed form (connected k-subsets) ----
def path(n):
    i = np.arange(max(n - 1, 0), dtype=np.int64)
    return n, np.stack([np.concatenate([i, i + 1]), np.concatenate([i + 1, i])])


def cycle(n):
    i = np.arange(n, dtype=np.int64)
    return n, np.stack([np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i])])


def complete(n):
    u, v = np.triu_indices(n, 1)
    return n, np.stack([np.concatenate([u, v]), np.concatenate([v, u])]).astype(np.int64)


def closed_form(kind, n, k):
    if n < k or k < 1:
        return 0
    return {"path": n - k + 1, "cycle": n if k < n else 1, "complete": comb(n, k)}[kind]


BUILD = {"path": path, "cycle": cycle, "complete": complete}

# The batches of tests/test_gpu_uniform_distinct.py: name -> (k, m, [(kind, n)], seeds, vertex limit).  The seeds are fixed numbers;
# test_uniform_distinct_law.py asserts, from the law alone, that together they reach every class above and tell every mutant apart.
GPU_CASES = {
    # N = 6, 7, 0 (n < k), 1, 10, 7, 0, 5 at m = 6: m = N, m = N - 1, a dead graph between live ones, N = 1, m > N, m < N
    "small_mix": (3, 6, [("path", 8), ("cycle", 7), ("path", 2), ("path", 3), ("cycle", 10), ("path", 9), ("path", 0), ("cycle", 5)],
                  [11, 12, 13, 14, 15, 16, 17, 18], 64),
    "one_row": (3, 1, [("cycle", 5), ("path", 3), ("complete", 6)], [1, 2, 3], 64),
    # the CSL-like call: N = 1 716 and m = 100 (a sort of 128 keys with padding), a small graph beside it
    "k13_m100": (6, 100, [("complete", 13), ("cycle", 12), ("complete", 13)], [5, 6, (1 << 64) - 1], 64),
    # nearly everything drawn: long chains.  path(300) is wide (N = 298, m = N - 1), K_13 has 286 < m, path(100) is wide with 98 < m,
    # cycle(40) takes the mask form with 40 < m: rows of -1 inside live graphs of both forms
    "near_full": (3, 297, [("path", 300), ("complete", 13), ("path", 100), ("cycle", 40), ("path", 320)], [21, 22, 23, 24, 25], 1024),
    # the limit: 4 096 of 8 008
    "full_width": (6, 4096, [("complete", 16), ("cycle", 9)], [31, 32], 64),
}


def case_batch(name, first=0):
    """(k, m, ei, ptr, sizes, seeds, vertex limit, graphs [(n, local columns)]) of a GPU case"""
    k, m, kinds, seeds, limit = GPU_CASES[name]
    graphs = [BUILD[kind](n) for kind, n in kinds]
    cols, ptr = [], [first]
    for n, ei in graphs:
        cols.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.ascontiguousarray(np.concatenate(cols, axis=1))
    sizes = [closed_form(kind, n, k) for kind, n in kinds]
    return k, m, ei, np.array(ptr, np.int64), sizes, list(seeds), limit, graphs
