"""apx_gpu_rows.py -- TEST INFRASTRUCTURE: the rows of the GPU variant of apx_ugs_sampler (csrc/ugs_apx_gpu.hip), restated.

The GPU variant runs the reference's APX-UGS trial (root draw, APX-RAND-GROW with EstimateCuts, APX-PROB over the
permutations of the grown set, acceptance) with one counter-keyed stream per (sample, trial) -- TrialRng: a splitmix64 key,
xorshift64*, below(n) = high half of a 32 x 32-bit product, 53-bit unit() -- and a sample's row is its accepted trial with the
smallest index below the trial cap (samples without one are dropped).  This module restates that with numpy, vectorised over
trials: every lane is one (sample, trial) pair, each with its own stream and an `alive` mask for the trial's early exits; a
stream advances only where its lane draws.

Inputs: the graph as csr_of_columns (ugs_apx_common.h) builds it from the columns ptr[0]:ptr[1] -- vertex ids 0 .. max id,
rows sorted without repeats, a self loop kept once in its own row, columns with a negative endpoint ignored -- and the
APX-DD order (pos, est) the call used (return_order=True; apx_oracle.order restates it where it is deterministic).  Z and
the inclusive sums `cum` of est are summed sequentially in vertex order like the host does; (h, ell) of the two EstimateCuts
callers come from apx_oracle.cut_params."""
import math
from itertools import permutations

import numpy as np

import apx_oracle

U = np.uint64
GOLDEN = 0x9E3779B97F4A7C15
TRIAL_CAP = 1_000_000


class Graph:
    def __init__(self, edge_index, ptr):
        ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
        c0, c1 = max(int(ptr[0]), 0), min(int(ptr[1]), ei.shape[1])
        cols = [(int(a), int(b)) for a, b in ei[:, c0:c1].T.tolist() if a >= 0 and b >= 0] if c1 > c0 else []
        self.n = max((max(a, b) for a, b in cols), default=-1) + 1
        rows = [set() for _ in range(self.n)]
        for a, b in cols:
            rows[a].add(b)
            rows[b].add(a)
        self.rows = [sorted(r) for r in rows]
        self.deg = np.array([len(r) for r in self.rows], dtype=np.int64)
        self.off = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.deg, out=self.off[1:])
        self.nbr = np.array([w for r in self.rows for w in r] or [0], dtype=np.int64)
        self.adj = np.zeros((max(self.n, 1), max(self.n, 1)), dtype=bool)
        for v, r in enumerate(self.rows):
            self.adj[v, r] = True


class Params:
    """the constants of one call (ugs_apx_gpu_sample_batch)"""

    def __init__(self, g, k, epsilon, seed, pos, est, trial_cap=TRIAL_CAP):
        self.g, self.k, self.seed, self.trial_cap = g, int(k), int(seed) & ((1 << 64) - 1), int(trial_cap)
        self.pos = np.asarray(pos, dtype=np.int64)
        self.est = np.asarray(est, dtype=np.float64)
        Z, cum = 0.0, []
        for x in self.est.tolist():          # sequential, like the host: not np.sum / fsum
            Z += x
            cum.append(Z)
        self.Z, self.cum = Z, np.array(cum, dtype=np.float64)
        k, C1, C2 = self.k, 2, 2
        beta = epsilon / 2.0
        alpha = math.pow(beta, 1.0 / (k - 1)) / (6.0 * k * k * k)
        gamma = epsilon * math.pow(3.0, -k) * math.pow(k, -C2)
        rho = gamma
        self.h_grow, self.ell_grow = apx_oracle.cut_params(k, alpha, beta, gamma / math.pow(k, 4.0))
        self.h_prob, self.ell_prob = apx_oracle.cut_params(k, alpha, beta / math.pow(k, 6.0), rho / (k * k))
        self.accept_scale = (beta / Z) * math.pow(k, -C1) if Z > 0 else 0.0
        self.perms = [list(p) for p in permutations(range(k - 1))][:720]     # next_permutation order from the sorted set


class Lanes:
    """TrialRng of every (sample, trial) lane"""

    def __init__(self, seed, sample, trial):
        with np.errstate(over="ignore"):
            z = U(seed) + U(GOLDEN) * (sample.astype(U) * U(0x100000001B3) + trial.astype(U) + U(1))
            z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        z ^= z >> U(31)
        z[z == 0] = U(0x2545F4914F6CDD1D)
        self.s = z

    def next(self, live):
        x = self.s ^ (self.s >> U(12))
        x ^= x << U(25)
        x ^= x >> U(27)
        self.s = np.where(live, x, self.s)
        with np.errstate(over="ignore"):
            return x * U(2685821657736338717)

    def below(self, n, live):
        return (((self.next(live) >> U(32)) * np.asarray(n).astype(U)) >> U(32)).astype(np.int64)

    def unit(self, live):
        return (self.next(live) >> U(11)).astype(np.float64) * 2.0 ** -53


def _cut_estimates(P, rs, live, pv, S, nu, h, ell):
    """EstimateCuts of S[:, :nu] for every lane: (cuts [L, nu], total [L]); draws only where `live`"""
    g = P.g
    L = len(pv)
    cuts = np.zeros((L, nu))
    total = np.zeros(L)
    for i in range(nu):
        u = S[:, i]
        d = g.deg[u]
        draw = live & (d > 0)
        hits = np.zeros(L, dtype=np.int64)
        if draw.any():
            base = g.off[u]
            for _ in range(h):
                w = g.nbr[np.where(draw, base + rs.below(d, draw), 0)]
                out = draw & (pv < P.pos[w])
                for t in range(nu):
                    out &= S[:, t] != w
                hits += out
        c = np.where(draw & (hits.astype(np.float64) >= ell), (d * hits).astype(np.float64) / float(h), 0.0)
        cuts[:, i] = c
        total = total + c
    return cuts, total


def run_trials(P, sample, trial):
    """(accepted [L] bool, S [L, k] graphlets in growth order) of the given (sample, trial) lanes"""
    g, k = P.g, P.k
    L = len(sample)
    rs = Lanes(P.seed, np.asarray(sample), np.asarray(trial))
    live = np.ones(L, dtype=bool)
    r = rs.unit(live) * P.Z
    v = np.minimum(np.searchsorted(P.cum, r, side="left"), g.n - 1)     # first vertex whose running sum reaches r
    live &= P.est[v] > 0.0
    pv = P.pos[v]
    S = np.zeros((L, k), dtype=np.int64)
    S[:, 0] = v
    dmax = int(g.deg.max()) if g.n else 0
    for i in range(1, k):                                                # APX-RAND-GROW
        cuts, total = _cut_estimates(P, rs, live, pv, S, i, P.h_grow, P.ell_grow)
        live &= total > 0.0
        rr = rs.unit(live) * total
        frm = S[:, 0].copy()
        run = np.zeros(L)
        found = np.zeros(L, dtype=bool)
        for j in range(i):
            run = run + cuts[:, j]
            hit = ~found & (rr <= run)
            frm[hit] = S[hit, j]
            found |= hit
        okm = np.zeros((L, max(dmax, 1)), dtype=bool)
        wm = np.zeros((L, max(dmax, 1)), dtype=np.int64)
        for p in range(dmax):
            valid = p < g.deg[frm]
            w = g.nbr[np.where(valid, g.off[frm] + p, 0)]
            ok = valid & (pv < P.pos[w])
            for t in range(i):
                ok &= S[:, t] != w
            okm[:, p], wm[:, p] = ok, w
        nok = okm.sum(axis=1)
        live &= nok > 0
        pick = rs.below(nok, live)
        rank = np.cumsum(okm, axis=1) - 1
        sel = okm & (rank == pick[:, None])
        S[:, i] = np.where(live, wm[np.arange(L), np.argmax(sel, axis=1)], 0)
    # APX-PROB: the non-root vertices sorted, their permutations in lexicographic order (at most 720)
    rest = np.sort(S[:, 1:], axis=1)
    p_hat = np.zeros(L)
    for perm_idx in P.perms:
        perm = np.concatenate([S[:, :1], rest[:, perm_idx]], axis=1)
        p = np.ones(L)
        going = live.copy()
        for i in range(k - 1):
            links = np.zeros(L, dtype=np.int64)
            for t in range(i + 1):
                links += g.adj[perm[:, t], perm[:, i + 1]]
            _, ci = _cut_estimates(P, rs, going, pv, perm, i + 1, P.h_prob, P.ell_prob)
            pos_ci = ci > 0.0
            p = np.where(going & pos_ci, p * (links.astype(np.float64) / np.where(pos_ci, ci, 1.0)), np.where(going, 0.0, p))
            going &= pos_ci
        p_hat = p_hat + np.where(live, p, 0.0)
    live &= p_hat > 0.0
    with np.errstate(divide="ignore"):
        accept = np.minimum(P.accept_scale / (P.est[v] * np.where(live, p_hat, 1.0)), 1.0)
    accepted = live & (rs.unit(live) < accept)
    return accepted, S


def first_accepted(P, samples, lanes=1 << 15):
    """{sample: (trial, graphlet tuple) or None}: the smallest accepted trial index below the cap of every sample"""
    samples = [int(s) for s in samples]
    out = {s: None for s in samples}
    nxt = {s: 0 for s in samples}
    pending = list(samples)
    while pending:
        per = max(1, lanes // len(pending))
        sm, tr = [], []
        for s in pending:
            t1 = min(nxt[s] + per, P.trial_cap)
            sm.append(np.full(t1 - nxt[s], s, dtype=np.int64))
            tr.append(np.arange(nxt[s], t1, dtype=np.int64))
            nxt[s] = t1
        sm, tr = np.concatenate(sm), np.concatenate(tr)
        acc, S = run_trials(P, sm, tr)
        for s in pending:
            hit = np.nonzero(acc & (sm == s))[0]
            if len(hit):
                i = hit[np.argmin(tr[hit])]
                out[s] = (int(tr[i]), tuple(int(x) for x in S[i]))
        pending = [s for s in pending if out[s] is None and nxt[s] < P.trial_cap]
    return out


def sample_rows(P, m):
    """the rows [S, k] of a whole call of m samples (dropped samples removed), and the trial behind each"""
    got = first_accepted(P, range(m))
    keep = [got[s] for s in range(m) if got[s] is not None]
    return np.array([g[1] for g in keep], dtype=np.int64).reshape(len(keep), P.k), [g[0] for g in keep]
