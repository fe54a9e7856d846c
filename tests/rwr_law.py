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
"""
import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


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


def sample_batch(ei, ptr, m, k, mode="sample", seed=42, p_restart=0.2):
    """The reference's five outputs as numpy int64 arrays (one OpenMP thread)."""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    ptr = np.asarray(ptr, np.int64)
    G = len(ptr) - 1
    adjs = adjacency(ei[0], ei[1], ptr)
    nodes = np.full((G * m, k), -1, np.int64)
    eptr, edges = [0], []
    for g in range(G):
        adj, lo = adjs[g], int(ptr[g])
        n = len(adj)
        gseed = (seed + g) & M64
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
