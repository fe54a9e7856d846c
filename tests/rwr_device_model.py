"""rwr_device_model.py -- CPU model of what rwr_resolve (ugs_rwr.hip) runs for one graph, line for line where a line can be
wrong: per-offset speculation capped at SPEC_CAP with the kernel's check position, lane 0's redo of capped walks on the chain,
and the lane-composed length of doomed walks (32-position bit words, counts and exit state for both entry states, lane 0 chaining
`left` and `state` across lanes and rounds).  `rwr_law.chain_starts` models speculate / resolve without either.

`mutant=` swaps one line for a plausible slip.  tests/test_rwr_law.py asserts that the model equals the law on every input of
tests/rwr_paths.py and that every mutant differs on at least one: the evidence that those inputs discriminate, obtained without
running a wrong kernel.

MUTANTS that change results:
  left_lt            rwr_doomed_len: `left < n` in place of `left <= n`; when left == n the lane scan never counts down to the
                     T-th step and ds.end keeps what it held (modelled: the previous doomed walk's end, 0 at first)
  no_lane_carry      `state = ds.ex[state][t]` dropped: every lane entered in the state the round began with
  no_round_carry     the exit state forgotten when `pos` moves on by a round: every round entered as if a step started there
  end_no_bit         `ds.end = pos + 32 t + j` without `+ bit`
  isolated_no_seed   `return (uint64_t)w.T` for a doomed seed without edges: the seed draw not counted
  first_step_early   `pos = c + 1`: the seed draw taken for the first step's
  window_le          rwr_resolve: `cc <= base + W` in place of `<`; the chain reads sl[W], which no lane wrote (modelled: 0, and
                     L == 0 sends the block into rwr_doomed_len)
  lds_words_plus_1   the LDS bound one word too wide: a graph of RWR_LDS_INTS + 1 words goes to LDS and the last word, with the
                     doomed bytes of its last vertices, falls outside csr[]; modelled as reading the doomed byte of vertex n - 1
                     one word further, i.e. byte n + 3 of the batch's doomed bytes (0 past the batch)
EQUIVALENT (they change which path runs, never a result):
  cap_gt             `L > cap`: fewer walks are handed to lane 0, which finds the same lengths
  lds_words_minus_1  the LDS bound one word too narrow: a graph of exactly RWR_LDS_INTS words walks from global memory
"""
import numpy as np

import rwr_law as R

MUTANTS = ("left_lt", "no_lane_carry", "no_round_carry", "end_no_bit", "isolated_no_seed", "first_step_early", "window_le",
           "lds_words_plus_1")
EQUIVALENT = ("cap_gt", "lds_words_minus_1")
CAPPED = R.M64                                                      # rwr_walk's ~0ull


def spec_walk(adj, doomed, k, p, graph_seed, c, cap=None, cap_gt=False):
    """rwr_walk: (L, found).  L == 0: the seed is doomed; L == CAPPED: `cap` draws taken without ending."""
    n = len(adj)
    i = c + 1
    seed_node = R.draw(graph_seed, i) % n
    if doomed[seed_node]:
        return 0, False
    cur, seen = seed_node, {seed_node}
    it, limit = 0, n * k * 10
    while len(seen) < k and it < limit:
        if cap is not None and (i - c > cap if cap_gt else i - c >= cap):
            return CAPPED, False
        it += 1
        i += 1
        if R.to_double(R.draw(graph_seed, i)) < p or not adj[cur]:
            cur = seed_node
        else:
            i += 1
            cur = adj[cur][R.draw(graph_seed, i) % len(adj[cur])]
        seen.add(cur)
    return i - c, len(seen) >= k


class Graph:
    """One graph's run of rwr_resolve: `starts(m)` gives c_0 .. c_m (c_m: the draws the m walks consumed) and the rows' success."""

    def __init__(self, adj, k, p, graph_seed, doomed=None, mutant=None):
        assert mutant is None or mutant in MUTANTS + EQUIVALENT, mutant
        self.adj, self.k, self.p, self.sg, self.mutant = adj, k, p, graph_seed & R.M64, mutant
        self.n, self.T = len(adj), 10 * len(adj) * k
        self.doomed = [z < k for z in R.component_sizes(adj)] if doomed is None else doomed
        self.end = 0                                                # ds.end
        self.redone = []                                            # chain walks that lane 0 ran again
        self.memo = {}

    def speculate(self, c):
        if c not in self.memo:
            self.memo[c] = spec_walk(self.adj, self.doomed, self.k, self.p, self.sg, c, R.SPEC_CAP, self.mutant == "cap_gt")
        return self.memo[c]

    def doomed_len(self, c):
        """rwr_doomed_len"""
        seed_node = R.draw(self.sg, c + 1) % self.n
        if not self.adj[seed_node]:
            return self.T if self.mutant == "isolated_no_seed" else 1 + self.T
        pos, left, state = c + (1 if self.mutant == "first_step_early" else 2), self.T, 0
        while True:
            bits = np.array(R.step_bits(self.sg, pos, R.DOOM_ROUND, self.p), np.int64).reshape(R.RWR_BLOCK, R.DOOM_LANE)
            # every lane: its 32 positions composed for both entry states
            st = np.array([[0] * R.RWR_BLOCK, [1] * R.RWR_BLOCK], np.int64)
            cnt = np.zeros((2, R.RWR_BLOCK), np.int64)
            for j in range(R.DOOM_LANE):
                begins = st == 0
                cnt += begins
                st = np.where(begins, bits[None, :, j], 0)
            ex = st
            # lane 0 chains the lanes
            done = False
            for t in range(R.RWR_BLOCK):
                n = int(cnt[state][t])
                if (left < n) if self.mutant == "left_lt" else (left <= n):
                    s = state
                    for j in range(R.DOOM_LANE):
                        if s != 0:
                            s = 0
                            continue
                        bit = int(bits[t][j])
                        left -= 1
                        if left == 0:
                            self.end = pos + R.DOOM_LANE * t + j + (0 if self.mutant == "end_no_bit" else bit)
                            break
                        s = bit
                    done = True
                    break
                left -= n
                if self.mutant != "no_lane_carry":
                    state = int(ex[state][t])
            if done:
                return (self.end - c) & R.M64
            pos += R.DOOM_ROUND
            if self.mutant == "no_round_carry":
                state = 0

    def starts(self, m):
        _, W = R.spec_window(m)
        sl_past = 0                                                 # sl[W]: no lane writes it
        out, ok_rows = [], []
        base = cc = 0
        s = 0
        while s < m:
            while True:
                pend = False
                while s < m and (cc <= base + W if self.mutant == "window_le" else cc < base + W):
                    o = cc - base
                    L, ok = self.speculate(cc) if o < W else (sl_past, False)
                    if L == CAPPED:
                        self.redone.append(cc)
                        L, ok = spec_walk(self.adj, self.doomed, self.k, self.p, self.sg, cc)
                    if L == 0:
                        pend = True
                        break
                    out.append(cc)
                    ok_rows.append(ok)
                    s += 1
                    cc = (cc + L) & R.M64
                if not pend:
                    break
                L = self.doomed_len(cc)
                out.append(cc)
                ok_rows.append(False)
                s += 1
                cc = (cc + L) & R.M64
            base = cc
        return out + [cc], ok_rows


def batch_starts(ei, ptr, m, k, seed, p, seeds=None, mutant=None):
    """Per graph with n >= k: (starts c_0 .. c_m, success per row, chain walks lane 0 redid) of the model."""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    adjs = R.adjacency(ei[0], ei[1], ptr)
    sizes = [R.component_sizes(adj) for adj in adjs]
    flat = [z < k for size in sizes for z in size]                  # the batch's doomed bytes, graph after graph
    out, vbase = [], 0
    for g, adj in enumerate(adjs):
        n = len(adj)
        if n >= k:
            doomed = flat[vbase:vbase + n]
            words = n + 1 + sum(len(a) for a in adj) + (n + 3) // 4
            if mutant == "lds_words_plus_1" and words == R.RWR_LDS_INTS + 1:
                doomed[n - 1] = flat[vbase + n + 3] if vbase + n + 3 < len(flat) else False
            gseed = (seed + g) & R.M64 if seeds is None else int(seeds[g]) & R.M64
            gr = Graph(adj, k, p, gseed, doomed, mutant)
            st, ok = gr.starts(m)
            out.append((st, ok, gr.redone))
        else:
            out.append(None)
        vbase += n
    return out
