"""eps_rows.py -- TEST INFRASTRUCTURE: the rows of the HIP epsilon_uniform_sampler (csrc/ugs_eps.hip), restated bit for bit.

The kernel draws every number of row `row`, attempt `attempt` from a counter-keyed stream (CRng): a splitmix64 key of
(seed, row, attempt), xorshift64* steps, a multiply-shift integer draw with rejection and a 53-bit unit draw.  What it does
with those numbers is the reference's algorithm as oracle/eps_oracle.py documents it (start vertex, frontier growth over
adjacency lists in column order, weight, acceptance min(1, eps / (w + eps)) against a unit draw with <=, max(10, int(10/eps))
attempts, sorted nodes, edges = the graph's batch columns inside the sample in column order).  This module restates the
generator and runs that algorithm on eps_oracle.adjacency lists, so every output tensor of a call can be predicted:

  * sample_rows(...)        the five outputs of a whole call (small calls: one Python walk per row);
  * Batch(...).row(r)       one row, for checking chosen rows of a large call (rows are independent);
  * k1_rows(...)            k = 1 vectorised with numpy (wrapping uint64 arithmetic, masked attempt loop), for calls of
                            millions of rows.

The kernel is built with -ffp-contract=off; the weight is updated with the same double operations in the same order
(w *= 1.0/n once, then w *= (1.0/fsz) * (1.0/cnt) after each push), which Python floats reproduce exactly."""
import numpy as np

import eps_oracle

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    """splitmix64 finaliser"""
    z = (z + GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


class CRng:
    """the kernel's per-(row, attempt) stream"""

    def __init__(self, seed, row, attempt):
        s = mix64((mix64(seed ^ mix64(row)) + attempt) & MASK)
        self.s = s if s else GOLDEN

    def next(self):
        x = self.s
        x ^= x >> 12
        x ^= (x << 25) & MASK
        x ^= x >> 27
        self.s = x
        return (x * 2685821657736338717) & MASK

    def below(self, n):
        """integer in [0, n): high half of (32-bit draw) * n, redrawn while the low half is below 2^32 mod n"""
        m = (self.next() >> 32) * n
        lo = m & 0xFFFFFFFF
        if lo < n:
            t = (1 << 32) % n
            while lo < t:
                m = (self.next() >> 32) * n
                lo = m & 0xFFFFFFFF
        return m >> 32

    def unit(self):
        return (self.next() >> 11) * 2.0 ** -53


def max_attempts(epsilon):
    """max(10, int(10 / eps)) as the host computes it in C++ -- whose int conversion is only defined below 2^31"""
    a = 10.0 / epsilon
    assert a < 2.0 ** 31, "epsilon below 10 / 2^31: the attempt budget does not fit the host's int"
    return max(10, int(a))


def walk_row(adj, n, k, epsilon, seed, row):
    """sorted local node ids of row `row` of a graph with adjacency lists `adj` (indexable by local id), or None (failed row)"""
    if n < k:
        return None
    for attempt in range(max_attempts(epsilon)):
        rng = CRng(seed, row, attempt)
        start = rng.below(n)
        nodes, front = [start], [start]
        weight = 1.0
        weight *= 1.0 / n
        tries = 0
        dead = False
        while len(nodes) < k and tries < k * 100:
            tries += 1
            if not front:
                dead = True
                break
            fi = rng.below(len(front))
            cands = [v for v in adj[front[fi]] if v not in nodes]
            if not cands:
                del front[fi]
                continue
            v = cands[rng.below(len(cands))]
            nodes.append(v)
            front.append(v)
            weight *= (1.0 / len(front)) * (1.0 / len(cands))
        if dead or len(nodes) < k:
            continue
        if rng.unit() <= min(1.0, epsilon / (weight + epsilon)):
            return sorted(nodes)
    return None


class CsrAdj:
    """eps_oracle.adjacency order (for every column (u, v): adj[u] gets v, then adj[v] gets u) as a CSR, for large graphs"""

    def __init__(self, cols, n, ids=None):
        cols = np.asarray(cols, dtype=np.int64).reshape(-1, 2)
        ids = np.arange(len(cols), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
        keep = (cols[:, 0] >= 0) & (cols[:, 0] < n) & (cols[:, 1] >= 0) & (cols[:, 1] < n)
        cols, ids = cols[keep], ids[keep]
        key = np.stack([cols[:, 0], cols[:, 1]], axis=1).ravel()
        val = np.stack([cols[:, 1], cols[:, 0]], axis=1).ravel()
        order = np.argsort(key, kind="stable")
        self.nbr = val[order]
        self.col = np.repeat(ids, 2)[order]         # the column behind every entry
        self.side = np.tile(np.array([0, 1], np.int8), len(ids))[order]     # 1: the entry is the column's destination
        self.off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(key, minlength=n), out=self.off[1:])

    def __getitem__(self, u):
        return self.nbr[self.off[u]:self.off[u + 1]].tolist()

    def edges(self, nodes_sorted, mode, node_offset):
        """expected_edges of a sample, from the rows of its vertices instead of a scan of every column"""
        pos = {v: i for i, v in enumerate(nodes_sorted)}
        seen = {}
        for u in nodes_sorted:
            a, b = self.off[u], self.off[u + 1]
            for v, j, side in zip(self.nbr[a:b].tolist(), self.col[a:b].tolist(), self.side[a:b].tolist()):
                if v in pos and j not in seen:
                    seen[j] = (v, u) if side else (u, v)
        rows = []
        for j in sorted(seen):
            u, v = seen[j]
            rows.append((pos[u], pos[v], j) if mode == "sample" else (node_offset + u, node_offset + v, j))
        return rows


class Batch:
    """one call's inputs: `edge_index` [2, E] (batch ids), `ptr` [G + 1]; graph g owns the columns with both endpoints in
    [ptr[g], ptr[g+1]), in column order"""

    def __init__(self, edge_index, ptr, m, k, epsilon, seed, large=False):
        ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
        self.ptr = [int(x) for x in np.asarray(ptr).ravel()]
        self.G = len(self.ptr) - 1
        self.m, self.k, self.epsilon, self.seed = int(m), int(k), float(epsilon), int(seed) & MASK
        self.cols, self.adj, self.n = [], [], []
        for g in range(self.G):
            lo, hi = self.ptr[g], self.ptr[g + 1]
            n = max(hi - lo, 0)
            js = np.nonzero((ei[0] >= lo) & (ei[0] < hi) & (ei[1] >= lo) & (ei[1] < hi))[0]
            self.n.append(n)
            if large:
                self.cols.append(None)
                self.adj.append(CsrAdj((ei[:, js] - lo).T, n, js))
            else:
                self.cols.append((js, [(int(ei[0, j]) - lo, int(ei[1, j]) - lo) for j in js]))
                self.adj.append(eps_oracle.adjacency(self.cols[-1][1], n))

    @property
    def rows(self):
        return self.G * self.m

    def row(self, r, mode):
        """(nodes [k] batch ids or -1, list of (a, b, column)) of row r"""
        g = r // self.m
        lo, n = self.ptr[g], self.n[g]
        got = walk_row(self.adj[g], n, self.k, self.epsilon, self.seed, r) if n >= self.k else None
        if got is None:
            return [-1] * self.k, []
        if self.cols[g] is None:
            return [lo + v for v in got], self.adj[g].edges(got, mode, lo)
        js, loc = self.cols[g]
        return [lo + v for v in got], [(a, b, int(js[e])) for a, b, e in eps_oracle.expected_edges(loc, got, mode, lo)]


def assemble(per_row, k, G, m):
    """the five output arrays from [(nodes, edges)] of consecutive rows"""
    B = len(per_row)
    nodes = np.array([r[0] for r in per_row], dtype=np.int64).reshape(B, k)
    eptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum([len(r[1]) for r in per_row], out=eptr[1:])
    flat = [e for r in per_row for e in r[1]]
    eidx = np.array([[e[0] for e in flat], [e[1] for e in flat]], dtype=np.int64).reshape(2, len(flat))
    esrc = np.array([e[2] for e in flat], dtype=np.int64)
    sptr = np.arange(G + 1, dtype=np.int64) * m
    return nodes, eidx, eptr, sptr, esrc


def sample_rows(edge_index, ptr, m, k, mode="sample", seed=42, epsilon=0.1):
    """the five outputs of epsilon_uniform_sampler.sample_batch, restated row by row"""
    b = Batch(edge_index, ptr, m, k, epsilon, seed)
    return assemble([b.row(r, mode) for r in range(b.rows)], b.k, b.G, b.m)


# ---------------------------------------------------------------------------------------------------------------------
# numpy: wrapping uint64 arithmetic over many rows at once
# ---------------------------------------------------------------------------------------------------------------------
U = np.uint64


def mix64_np(z):
    with np.errstate(over="ignore"):
        z = z + U(GOLDEN)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def init_np(seed, rows, attempt):
    with np.errstate(over="ignore"):
        s = mix64_np(mix64_np(U(seed) ^ mix64_np(rows.astype(U))) + U(attempt))
    s[s == 0] = U(GOLDEN)
    return s


def next_np(s, live):
    """advance the streams where `live`; returns the outputs (meaningful where live)"""
    x = s ^ (s >> U(12))
    x ^= x << U(25)
    x ^= x >> U(27)
    s[live] = x[live]
    with np.errstate(over="ignore"):
        return x * U(2685821657736338717)


def below_np(s, n, live):
    """CRng.below(n) for every live stream (n: one value or one per stream, each < 2^32)"""
    n = np.broadcast_to(np.asarray(n, dtype=U), s.shape)
    out = np.zeros(s.shape, dtype=U)
    t = (U(1 << 32) % np.maximum(n, U(1))).astype(U)
    need = live.copy()
    while need.any():                   # (lo < t implies lo < n: the kernel's outer test only saves the modulo)
        m = (next_np(s, need) >> U(32)) * n
        out[need] = (m >> U(32))[need]
        need &= (m & U(0xFFFFFFFF)) < t
    return out


def first_draw_rejected(seed, rows, n):
    """rows whose first start draw (attempt 0) falls into below()'s rejection branch"""
    rows = np.asarray(rows, dtype=np.int64)
    s = init_np(seed, rows, 0)
    m = (next_np(s, np.ones(len(rows), bool)) >> U(32)) * U(n)
    return rows[(m & U(0xFFFFFFFF)) < U((1 << 32) % n)]


def k1_rows(n, loops, rows, epsilon, seed, node_lo=0, mode="sample", chunk=1 << 21):
    """k = 1 on ONE graph of n vertices (ptr = [node_lo, node_lo + n]); `loops` = its self-loop columns as (local vertex,
    column) in column order -- at k = 1 no other column can lie inside a sample.  Returns (nodes [rows], edge_ptr [rows+1], edge_index [2, E], edge_src [E]) of the call, vectorised."""
    nodes = np.full(rows, -1, dtype=np.int64)
    acc = min(1.0, epsilon / ((1.0 * (1.0 / n)) + epsilon))
    for r0 in range(0, rows, chunk):
        r = np.arange(r0, min(rows, r0 + chunk), dtype=np.int64)
        got = np.full(len(r), -1, dtype=np.int64)
        todo = np.ones(len(r), bool)
        for attempt in range(max_attempts(epsilon)):
            if not todo.any():
                break
            s = init_np(seed, r, attempt)
            v = below_np(s, n, todo)
            u = (next_np(s, todo) >> U(11)).astype(np.float64) * 2.0 ** -53
            ok = todo & (u <= acc)
            got[ok] = v[ok].astype(np.int64)
            todo &= ~ok
        nodes[r0:r0 + len(r)] = got
    loops = np.asarray(loops, dtype=np.int64).reshape(-1, 2)
    per_vertex = np.bincount(loops[:, 0], minlength=n) if len(loops) else np.zeros(n, np.int64)
    cnt = np.where(nodes >= 0, per_vertex[np.maximum(nodes, 0)], 0)
    eptr = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(cnt, out=eptr[1:])
    # a row's edges: its vertex's loops in column order
    vorder = np.argsort(loops[:, 0], kind="stable") if len(loops) else np.zeros(0, np.int64)
    voff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(per_vertex, out=voff[1:])
    E = int(eptr[-1])
    rowid = np.repeat(np.arange(rows), cnt)
    within = np.arange(E) - eptr[rowid]
    esrc = loops[vorder, 1][voff[nodes[rowid]] + within] if E else np.zeros(0, np.int64)
    if mode == "sample":
        eidx = np.zeros((2, E), dtype=np.int64)
    else:
        eidx = np.stack([nodes[rowid] + node_lo, nodes[rowid] + node_lo]) if E else np.zeros((2, 0), np.int64)
    return np.where(nodes >= 0, nodes + node_lo, -1), eptr, eidx, esrc
