"""rwr_law.py -- CPU restatement of the reference's `rwr_sampler.sample_batch` (AniruddhaMandal/SS-GNN
src/samplers/rwr_sampler/src/rwr_sampler.cpp:73-296) with one OpenMP thread, for the tests.

The law (include/ugs_mi355.h, ugs_rwr_sample_batch_begin, states it in full):
  * adjacency (:31-71): columns in column order; a column belongs to the graph g with ptr[g] <= u, v < ptr[g+1] (none: dropped);
    adj[u].append(v) then adj[v].append(u), so a loop puts u into adj[u] twice and duplicate columns stay;
  * one SplitMix64 per graph seeded with seed + g (thread 0, :130): draw i (1-based) is mix(seed + g + (i+1)*GAMMA);
    next_int(b) = u64 % b, next_double = (u64 >> 11) * 2^-53;
  * graphs with n < k (n = 0 included) give m rows of -1 and draw nothing;
  * per sample (:162-190): seed_node = next_int(n); while |chosen| < k and it < 10*n*k: draw r; r < p or adj[cur] empty ->
    cur = seed_node (one draw), else cur = adj[cur][next_int(deg)] (a second draw); new vertices are appended to chosen.
    A walk that ends with fewer than k vertices gives a row of -1 and no edges; the stream goes on;
  * edges (:215-247): for u in chosen order, for v in adj[u] order with v chosen: (u, v); mode "sample" numbers them by
    position in chosen, any other mode gives batch ids; edge_src is -1.

`walk` also returns the draws a walk consumed: since the draws are a function of their index, the walk that starts after c
draws is a function of c alone (`walk_len`), which the speculate / resolve model (`chain_starts`) rests on.

`census` walks the chain of every graph as `sample_batch` does and counts which paths of the device pipeline (ugs_rwr.hip) the
input reaches: CSR placement, the speculation cap, window edges, and where the T-th step of a doomed walk falls among the lanes and
rounds of rwr_doomed_len.  It restates the kernel's constants below; tests/test_rwr_law.py reads them back from the sources.
"""
import collections

import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


# the device pipeline's constants, restated (tests/test_rwr_law.py::test_census_constants_are_the_kernels compares them with the sources)
RWR_BLOCK = 256        # ugs_rwr.hip `constexpr int RWR_BLOCK`: lanes of rwr_resolve's workgroup
SPEC_CAP = 64          # ugs_rwr.hip `constexpr uint64_t SPEC_CAP`: rwr_walk's `if (L >= cap) return ~0ull` during speculation
RWR_LDS_INTS = 8192    # ugs_rwr.hip `constexpr int RWR_LDS_INTS`: rwr_resolve's `n + 1 + D + (n + 3) / 4 <= RWR_LDS_INTS`
DOOM_LANE = 32         # ugs_rwr.hip rwr_doomed_len: `for (int j = 0; j < 32; ...)`, positions classified per lane
DOOM_ROUND = DOOM_LANE * RWR_BLOCK   # ugs_rwr.hip rwr_doomed_len: `pos += 32ull * RWR_BLOCK`, positions per round
SPEC_MAX = 4           # ugs_rwr.hip `RWR_WMAX = 4 * RWR_BLOCK` and ugs_side_rwr.cpp rwr_begin `c.spec = min(4, ...)`
KM_WIDTHS = (8, 16, 32, 64)   # ugs_rwr.hip ugs_rwr_begin / ugs_rwr_fill: launch_walks<8|16|32|64> by `c.k <= KM`


def spec_window(m):
    """(spec, W) of a call with m rows per graph: ugs_side_rwr.cpp rwr_begin `c.spec = min(4, max(1, (m * 16 + 255) / 256))`,
    ugs_rwr.hip rwr_resolve `W = c.spec * RWR_BLOCK`."""
    spec = min(SPEC_MAX, max(1, (16 * m + 255) // 256))
    return spec, RWR_BLOCK * spec


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class SplitMix64:
    """The reference's generator (:17-28), sequential form."""

    def __init__(self, seed):
        self.state = (seed + GAMMA) & M64

    def next_u64(self):
        self.state = (self.state + GAMMA) & M64
        return mix(self.state)


def draw(graph_seed, i):
    """Counter form: the i-th (1-based) output of SplitMix64(graph_seed)."""
    return mix((graph_seed + (i + 1) * GAMMA) & M64)


def to_double(u):
    return (u >> 11) * (1.0 / 9007199254740992.0)


def adjacency(src, dst, ptr):
    """Per graph, per local vertex, the neighbour list in (column, side) order."""
    G = len(ptr) - 1
    adjs = [[[] for _ in range(max(int(ptr[g + 1] - ptr[g]), 0))] for g in range(G)]
    for u, v in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        for g in range(G):
            lo, hi = int(ptr[g]), int(ptr[g + 1])
            if lo <= u < hi and lo <= v < hi:
                adjs[g][u - lo].append(v - lo)
                adjs[g][v - lo].append(u - lo)
                break
    return adjs


def walk(adj, k, p, graph_seed, c):
    """The walk that starts after c draws of the graph's stream: (chosen local vertices, draws consumed)."""
    n = len(adj)
    i = c
    i += 1
    seed_node = draw(graph_seed, i) % n
    cur, chosen, seen = seed_node, [seed_node], {seed_node}
    it, limit = 0, n * k * 10
    while len(chosen) < k and it < limit:
        it += 1
        i += 1
        r = to_double(draw(graph_seed, i))
        if r < p or not adj[cur]:
            cur = seed_node
        else:
            i += 1
            cur = adj[cur][draw(graph_seed, i) % len(adj[cur])]
        if cur not in seen:
            seen.add(cur)
            chosen.append(cur)
    return chosen, i - c


def walk_len(adj, k, p, graph_seed, c):
    return walk(adj, k, p, graph_seed, c)[1]


def sequential_starts(adj, k, p, graph_seed, m):
    """The m walk starts of a graph as the reference reaches them, one walk after the other on one SplitMix64."""
    rng, starts, consumed = SplitMix64(graph_seed), [], 0
    n = len(adj)
    for _ in range(m):
        starts.append(consumed)
        seed_node = rng.next_u64() % n
        consumed += 1
        cur, seen, it = seed_node, {seed_node}, 0
        while len(seen) < k and it < n * k * 10:
            it += 1
            r = to_double(rng.next_u64())
            consumed += 1
            if r < p or not adj[cur]:
                cur = seed_node
            else:
                cur = adj[cur][rng.next_u64() % len(adj[cur])]
                consumed += 1
            seen.add(cur)
    return starts


def chain_starts(adj, k, p, graph_seed, m, window):
    """Model of the device's speculate / resolve step: L(c) for every offset c of a window, then the chain c0 = 0,
    c_{s+1} = c_s + L(c_s) inside it; the next window begins where the chain left the last one."""
    starts, base = [], 0
    while len(starts) < m:
        lens = [walk_len(adj, k, p, graph_seed, base + o) for o in range(window)]   # independent of each other
        c = base
        while len(starts) < m and c < base + window:
            starts.append(c)
            c += lens[c - base]
        base = c
    return starts


def sample_batch(ei, ptr, m, k, mode="sample", seed=42, p_restart=0.2, seeds=None):
    """The reference's five outputs as numpy int64 arrays (one OpenMP thread).  seeds: graph g's generator is seeds[g] in place
    of seed + g (rwr_sampler.sample_graphs: the one-graph calls of the presample loop, batched)."""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    G = len(ptr) - 1
    adjs = adjacency(ei[0], ei[1], ptr)
    nodes = np.full((G * m, k), -1, np.int64)
    eptr, edges = [0], []
    for g in range(G):
        adj, lo = adjs[g], int(ptr[g])
        n = len(adj)
        gseed = (seed + g) & M64 if seeds is None else int(seeds[g]) & M64
        c = 0
        for s in range(m):
            row = g * m + s
            if n == 0 or n < k:
                eptr.append(len(edges))
                continue
            chosen, L = walk(adj, k, p_restart, gseed, c)
            c += L
            if len(chosen) < k:
                eptr.append(len(edges))
                continue
            nodes[row] = [lo + v for v in chosen]
            pos = {v: j for j, v in enumerate(chosen)}
            for u in chosen:
                for v in adj[u]:
                    if v in pos:
                        edges.append((pos[u], pos[v]) if mode == "sample" else (lo + u, lo + v))
            eptr.append(len(edges))
    E = len(edges)
    edge_index = np.array(edges, np.int64).T.reshape(2, E) if E else np.zeros((2, 0), np.int64)
    return (nodes, np.ascontiguousarray(edge_index), np.array(eptr, np.int64), np.arange(G + 1, dtype=np.int64) * m,
            np.full(E, -1, np.int64))


def step_bits(graph_seed, first, count, p):
    """[r(i) >= p for the draws i = first .. first + count - 1] as a list of 0 / 1 (numpy, wrapping uint64)."""
    i = np.full(count, (first + 1) & M64, np.uint64) + np.arange(count, dtype=np.uint64)   # (i + 1) mod 2^64
    z = np.full(count, graph_seed & M64, np.uint64) + i * np.uint64(GAMMA)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    r = (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return (r >= p).astype(np.uint8).tolist()


def doomed_last_step(graph_seed, c, T, p):
    """Closed form of a doomed walk whose seed has edges: its T iterations never stop early, and each takes one draw when r < p
    and two when not, whatever the vertex.  Returns (x, bit): the T-th step's first draw is draw c + 2 + x, bit its r >= p flag;
    the walk consumes x + 2 + bit draws."""
    bits = step_bits(graph_seed, c + 2, 2 * T, p)
    x = 0
    for _ in range(T - 1):
        x += 1 + bits[x]
    return x, bits[x]


def component_sizes(adj):
    """Size of each vertex's connected component."""
    n = len(adj)
    size, seen = [0] * n, [False] * n
    for r in range(n):
        if seen[r]:
            continue
        comp, stack = [r], [r]
        seen[r] = True
        while stack:
            for v in adj[stack.pop()]:
                if not seen[v]:
                    seen[v] = True
                    comp.append(v)
                    stack.append(v)
        for v in comp:
            size[v] = len(comp)
    return size


def walk_capped(adj, k, p, graph_seed, c):
    """`walk`, and whether speculation gives up on it: rwr_walk tests `L >= SPEC_CAP` at the top of every iteration, so a walk of
    64 draws stands, one of 65 stands only when its last step took it from 63, and 66 or more never stand."""
    n = len(adj)
    i = c + 1
    seed_node = draw(graph_seed, i) % n
    cur, seen, capped = seed_node, {seed_node}, False
    it, limit = 0, n * k * 10
    while len(seen) < k and it < limit:
        capped |= i - c >= SPEC_CAP
        it += 1
        i += 1
        if to_double(draw(graph_seed, i)) < p or not adj[cur]:
            cur = seed_node
        else:
            i += 1
            cur = adj[cur][draw(graph_seed, i) % len(adj[cur])]
        seen.add(cur)
    return len(seen), i - c, capped


def census(ei, ptr, m, k, seed, p_restart, seeds=None):
    """Which paths of ugs_rwr.hip the call reaches: a Counter of the classes named in DESIGN.md section 11.  Walks every graph's
    chain as `sample_batch` does.  The length of a doomed walk whose seed has edges comes from the closed form and is checked
    against `walk_len` here whenever T <= 5000."""
    return census_starts(ei, ptr, m, k, seed, p_restart, seeds)[0]


def census_starts(ei, ptr, m, k, seed, p_restart, seeds=None):
    """(census, per graph with n >= k the chain c_0 .. c_m it walked: the m starts and the draws all m walks consumed; else None)"""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    G = len(ptr) - 1
    adjs = adjacency(ei[0], ei[1], ptr)
    cnt = collections.Counter()
    spec, W = spec_window(m)
    chains = [None] * G
    cnt[f"spec == {spec}"] += 1
    cnt[f"KM == {min(w for w in KM_WIDTHS if k <= w)}"] += 1
    if k in KM_WIDTHS:
        cnt["k == KM"] += 1
    NV = int(ptr[-1] - ptr[0])
    kept = sum(len(a) for adj in adjs for a in adj) // 2
    if kept < ei.shape[1]:
        cnt["dropped columns"] += 1
        if NV & (NV - 1) == 0:
            cnt["dropped columns, NV a power of two"] += 1      # the dropped key NV needs one more sort bit than NV - 1
        if kept == 0:
            cnt["every column dropped"] += 1
    for g in range(G):
        adj = adjs[g]
        n = len(adj)
        if n < k:
            cnt["T0"] += 1
            continue
        D = sum(len(a) for a in adj)
        words = n + 1 + D + (n + 3) // 4
        place = "lds" if words <= RWR_LDS_INTS else "global"
        cnt[place] += 1
        if words in (RWR_LDS_INTS, RWR_LDS_INTS + 1):
            cnt[f"csr_words == {words}"] += 1
        if ptr[g] > ptr[0]:
            cnt["vbase > 0"] += 1
            cnt[place + ", vbase > 0"] += 1
        size = component_sizes(adj)
        for z in set(size):
            if z in (k - 1, k):
                cnt["component == k - 1" if z == k - 1 else "component == k"] += 1
        T = 10 * n * k
        gseed = (seed + g) & M64 if seeds is None else int(seeds[g]) & M64
        base = c = 0
        kinds, prev_doomed = set(), False
        chains[g] = [0]
        for s in range(m):
            if c >= base + W:                                       # rwr_resolve: `base = cc`, the window slides
                cnt["slides"] += 1
                cnt["window with capped and uncapped walks"] += len(kinds) == 2
                base, kinds = c, set()
            at_edge = c - base == W - 1
            cnt["offset W - 1"] += at_edge
            seed_node = draw(gseed, c + 1) % n
            if size[seed_node] >= k:
                found, L, capped = walk_capped(adj, k, p_restart, gseed, c)
                cnt["L < 64" if L < 64 else "L == 64" if L == 64 else "L in (65, 66)" if L <= 66 else "L > 66"] += 1
                cnt["L > W"] += L > W
                cnt["capped"] += capped
                cnt["L == 65 uncapped"] += L == 65 and not capped
                cnt["live_failed"] += found < k
                kinds.add(capped)
                prev_doomed = False
            else:
                cnt["doomed_row0"] += s == 0
                cnt["doomed_row_last"] += s == m - 1
                cnt["doomed_twice"] += prev_doomed
                cnt["doomed at offset W - 1"] += at_edge
                prev_doomed = True
                if not adj[seed_node]:
                    cnt["doomed_isolated"] += 1
                    L = 1 + T
                else:
                    x, bit = doomed_last_step(gseed, c, T, p_restart)
                    L = x + 2 + bit
                    if T <= 5000:
                        assert L == walk_len(adj, k, p_restart, gseed, c), (g, s, c, L)
                    rnd, lane, j = x // DOOM_ROUND, x % DOOM_ROUND // DOOM_LANE, x % DOOM_LANE
                    cnt["round 0" if rnd == 0 else "round 1" if rnd == 1 else "round >= 2"] += 1
                    cnt["j == 0"] += j == 0
                    if j == DOOM_LANE - 1:
                        cnt[f"j == 31, bit {bit}"] += 1
                        if lane == RWR_BLOCK - 1:
                            cnt[f"lane == 255 and j == 31, bit {bit}"] += 1
                    cnt["lane == 0 and j == 0 and round > 0"] += lane == 0 and j == 0 and rnd > 0
                    cnt["last_in_lane"] += j + 1 + bit >= DOOM_LANE      # no later step starts in the lane: `left == n`
            c += L
            chains[g].append(c)
            cnt["lands on base + W"] += s + 1 < m and c == base + W
        cnt["window with capped and uncapped walks"] += len(kinds) == 2
    return +cnt, chains                                             # (without the zero entries)
