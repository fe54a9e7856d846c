"""The host side of graphlets.orbit_ids (ugs_graphlet_rooted_codes, ugs_graphlet_orbit_counts: the search the kernel runs, with a forced
first pick) against the brute-force law of tests/graphlet_orbit_law.py, the brute-forced automorphism groups and the Burnside counts
of rooted graphs.  No GPU: nothing here launches a kernel."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import graphlet_law as law
import graphlet_orbit_law as olaw

UGS_E_BAD_ARG, UGS_E_UNSUPPORTED = -4, -7
NUM_ORBITS = (1, 3, 9, 29, 119, 663, 5759, 85023)
MASK = (1 << 28) - 1


def host_rooted(code, n):
    from ugs_sampler._lib import lib
    out = (C.c_uint32 * 8)(*([7] * 8))
    assert lib.ugs_graphlet_rooted_codes(int(code), n, out) == 0
    assert list(out)[n:] == [0xffffffff] * (8 - n)
    return list(out)[:n]


def host_counts(n):
    from ugs_sampler._lib import lib
    count = C.c_int64(-1)
    assert lib.ugs_graphlet_orbit_counts(n, None, 0, C.byref(count)) == 0
    counts = np.full((count.value,), -1, dtype=np.int64)
    assert lib.ugs_graphlet_orbit_counts(n, counts.ctypes.data, counts.size, C.byref(count)) == 0 and count.value == counts.size
    return counts


def class_codes(n):
    from ugs_sampler import graphlets
    keys = graphlets.table(n)
    return [int(k) & MASK for k in keys.tolist() if k >> 28 == n]


def check_class(code, n):
    """The three facts of item 2 for one graph: the host's rooted codes are the brute-force minima, equal codes are exactly the
    orbits of the brute-forced automorphism group, and the smallest is the canonical code."""
    want = list(olaw.rooted_codes(code, n))
    got = host_rooted(code, n)
    assert got == want, (n, code)
    orbit = olaw.automorphism_orbits(code, n)
    assert all((got[u] == got[v]) == (orbit[u] == orbit[v]) for u in range(n) for v in range(u)), (n, code)
    assert min(got) == law.key_of(code, n) & MASK, (n, code)
    return got


@pytest.mark.parametrize("n", range(1, 8))
def test_rooted_codes_of_every_class(n):
    codes = class_codes(n)
    assert len(codes) == law.GRAPHS_ON[n - 1]
    orbits = [len(set(check_class(c, n))) for c in codes]
    assert orbits == host_counts(n).tolist()
    if n > 1:                                                                    # orbits come in order of degree first
        for c in codes[::7]:
            got = host_rooted(c, n)
            deg = law.matrix(c, n).sum(axis=1).tolist()
            assert all(got[u] < got[v] for u in range(n) for v in range(n) if deg[u] < deg[v])


def eight_vertex_cases():
    c8 = [(i, (i + 1) % 8) for i in range(8)]
    allp = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    cube = [(a, a ^ d) for a in range(8) for d in (1, 2, 4) if a < a ^ d]
    named = {"cube": cube, "complement of the cube": [p for p in allp if p not in cube], "C8": c8,
             "2 x C4": [(i, (i + 1) % 4) for i in range(4)] + [(4 + i, 4 + (i + 1) % 4) for i in range(4)],
             "K4,4": [(i, 4 + j) for i in range(4) for j in range(4)], "2 x K4": [(i, j) for i, j in allp if (i < 4) == (j < 4)],
             "K8": allp, "empty": []}
    cases = {name: law.code_of_edges(8, [(min(p), max(p)) for p in es]) for name, es in named.items()}
    codes = class_codes(8)
    trees = [c for c in codes if bin(c).count("1") == 7 and law.connected(c, 8)]
    assert len(trees) == 23
    cases.update({f"tree {i}": c for i, c in enumerate(trees)})
    cases.update({f"class {c:#x}": c for c in random.Random(88).sample(codes, 100)})
    return cases


def test_rooted_codes_at_eight_vertices():
    cases = eight_vertex_cases()
    counts = {name: len(set(check_class(code, 8))) for name, code in cases.items()}
    assert [counts[x] for x in ("cube", "complement of the cube", "C8", "2 x C4", "K4,4", "2 x K4", "K8", "empty")] == [1] * 8
    assert len(set(counts.values())) > 4


def test_orbit_counts_are_the_burnside_counts_of_rooted_graphs():
    from ugs_sampler import graphlets
    total, conn = olaw.burnside_rooted(8)
    assert total[:5] == [1, 2, 6, 20, 90] and conn[:5] == [1, 1, 3, 11, 58]      # the published start of both series
    for n in range(1, 9):
        counts, codes = host_counts(n), class_codes(n)
        assert len(counts) == len(codes) and counts.min() >= 1 and counts.max() <= n
        assert int(counts.sum()) == total[n - 1]
        assert sum(int(x) for x, c in zip(counts, codes) if law.connected(c, n)) == conn[n - 1]
        assert graphlets.num_orbits(n) == sum(total[:n]) == NUM_ORBITS[n - 1]
        assert graphlets.connected_orbits(n).numel() == conn[n - 1]
    assert sum(graphlets.connected_orbits(k).numel() for k in range(2, 6)) == 73


def test_orbit_base_info_and_connected_orbits():
    from ugs_sampler import graphlets
    for k in range(1, 9):
        base = graphlets.orbit_base(k)
        counts = np.concatenate([host_counts(n) for n in range(1, k + 1)])
        assert base.dtype == torch.int64 and not base.is_cuda and tuple(base.shape) == (graphlets.num_classes(k) + 1,)
        assert base.tolist() == [0] + np.cumsum(counts).tolist() and int(base[-1]) == graphlets.num_orbits(k)
    assert graphlets.orbit_base(8)[:209].tolist() == graphlets.orbit_base(6).tolist()        # the id does not depend on k
    base6, keys6 = graphlets.orbit_base(6).tolist(), graphlets.table(6).tolist()
    assert [b - a for a, b in zip(base6, base6[1:])] == olaw.orbit_counts(keys6)             # the law's own counts, k <= 6

    base, keys = graphlets.orbit_base(8).tolist(), graphlets.table(8).tolist()
    rng = random.Random(5)
    for oid in list(range(663)) + rng.sample(range(663, 85023), 300):
        cid, key, rooted, size, degree = graphlets.orbit_info(oid)
        n, code = key >> 28, key & MASK
        assert base[cid] <= oid < base[cid + 1] and keys[cid] == key
        all_rooted = host_rooted(code, n)
        assert sorted(set(all_rooted))[oid - base[cid]] == rooted and all_rooted.count(rooted) == size
        degs = {int(law.matrix(code, n)[v].sum()) for v in range(n) if all_rooted[v] == rooted}
        assert degs == {degree}
    sizes = {}
    for oid in range(663):                                                       # the orbits of a class partition its vertices
        cid, key, _, size, _ = graphlets.orbit_info(oid)
        sizes[cid] = sizes.get(cid, 0) + size
    assert [sizes[c] for c in range(208)] == [k >> 28 for k in keys[:208]]
    # the path on three vertices: its ends before its middle
    path = keys.index((3 << 28) | law.key_of(law.code_of_edges(3, [(0, 1), (1, 2)]), 3) & MASK)
    assert [graphlets.orbit_info(base[path] + i)[3:] for i in range(2)] == [(2, 1), (1, 2)] and base[path + 1] - base[path] == 2

    for k in range(1, 8):
        ids = graphlets.connected_orbits(k)
        assert ids.dtype == torch.int64 and not ids.is_cuda and bool(torch.all(ids[1:] > ids[:-1]))
        conn = graphlets.is_connected(graphlets.table(k)).tolist()
        want = [o for c in range(len(conn)) if conn[c] and keys[c] >> 28 == k for o in range(base[c], base[c + 1])]
        assert ids.tolist() == want
    with pytest.raises(ValueError):
        graphlets.orbit_info(85023)
    with pytest.raises(ValueError):
        graphlets.orbit_info(-1)
    with pytest.raises(TypeError):
        graphlets.orbit_info(1.0)


@pytest.mark.parametrize("n", range(1, 7))
def test_rooted_codes_do_not_depend_on_the_labelling(n):
    rng = random.Random(60 + n)
    for code in class_codes(n):
        want = host_rooted(code, n)
        for _ in range(20):
            perm = list(range(n))
            rng.shuffle(perm)
            got = host_rooted(law.relabel(code, n, perm), n)
            assert [got[perm[v]] for v in range(n)] == want, (n, code, perm)


def test_refusals():
    from ugs_sampler import graphlets
    from ugs_sampler._lib import lib
    count, out = C.c_int64(0), (C.c_uint32 * 8)()
    for k in (0, 9, -1):
        assert lib.ugs_graphlet_orbits(None, None, 0, 0, None, 0, k, None, None, 0, None, None, None, None) == UGS_E_UNSUPPORTED
        assert b"1 <= k <= 8" in lib.ugs_last_error()
        assert lib.ugs_graphlet_orbit_counts(k, None, 0, C.byref(count)) == UGS_E_UNSUPPORTED
        assert lib.ugs_graphlet_rooted_codes(0, k, out) == UGS_E_UNSUPPORTED
        for fn in (graphlets.num_orbits, graphlets.orbit_base, graphlets.connected_orbits):
            with pytest.raises(RuntimeError, match="k <= 8"):
                fn(k)
    assert lib.ugs_graphlet_orbits(None, None, 0, 0, None, 0, 8, None, None, 0, None, None, None, None) == 0         # rows = 0: a no-op
    assert lib.ugs_graphlet_orbits(None, None, 0, 0, None, 0, 8, None, None, -1, None, None, None, None) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_orbits(None, None, 0, 0, None, 1, 8, None, None, 0, None, None, None, None) == UGS_E_BAD_ARG  # null pointers
    assert lib.ugs_graphlet_rooted_codes(8, 3, out) == UGS_E_BAD_ARG                                 # bit 3 at n = 3
    assert lib.ugs_graphlet_rooted_codes(7, 3, None) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_orbit_counts(3, None, 0, None) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_orbit_counts(3, None, 0, C.byref(count)) == 0 and count.value == 4       # too small: the count only
    nodes, ei, ep = torch.zeros((2, 6), dtype=torch.int64), torch.zeros((2, 0), dtype=torch.int64), torch.zeros((3,), dtype=torch.int64)
    with pytest.raises(TypeError):                                               # what class_ids raises for the same faults
        graphlets.orbit_ids(nodes.to(torch.int32), ei, ep)
    with pytest.raises(TypeError):
        graphlets.orbit_ids(nodes.numpy(), ei, ep)
    with pytest.raises(ValueError):
        graphlets.orbit_ids(nodes, ei, ep[:-1])
    with pytest.raises(ValueError):
        graphlets.orbit_ids(nodes, ei.t(), ep)
    with pytest.raises(ValueError):
        graphlets.orbit_ids(nodes[0], ei, ep)
    with pytest.raises(TypeError):
        graphlets.num_orbits(6.0)
    cols = torch.tensor([0, 1], dtype=torch.int64)
    with pytest.raises(TypeError):
        graphlets.vertex_orbit_counts(nodes.to(torch.int32), nodes, 3, cols)
    with pytest.raises(TypeError):
        graphlets.vertex_orbit_counts(nodes, nodes, 3, [0, 1])
    with pytest.raises(ValueError):
        graphlets.vertex_orbit_counts(nodes, nodes[:1], 3, cols)
    with pytest.raises(ValueError):
        graphlets.vertex_orbit_counts(nodes, nodes, -1, cols)


def test_vertex_orbit_counts_on_the_cpu():
    from ugs_sampler import graphlets
    rng = random.Random(9)
    columns = [2, 3, 5, 11, 12, 28]
    nodes = [[rng.choice([-1, 0, 1, 2, 3, 4, 5, 6, 9]) for _ in range(4)] for _ in range(60)]
    orbit = [[rng.choice(columns + [0, 4, 29, 13]) for _ in range(4)] for _ in range(60)]
    want = [[0] * len(columns) for _ in range(7)]
    for r in range(60):
        for v, o in zip(nodes[r], orbit[r]):
            if 0 <= v < 7 and o in columns:
                want[v][columns.index(o)] += 1
    got = graphlets.vertex_orbit_counts(torch.tensor(nodes), torch.tensor(orbit), 7, torch.tensor(columns))
    assert got.dtype == torch.int64 and got.tolist() == want and sum(map(sum, want)) > 50
    assert tuple(graphlets.vertex_orbit_counts(torch.tensor(nodes), torch.tensor(orbit), 7, torch.tensor([], dtype=torch.int64)).shape) == (7, 0)
    assert tuple(graphlets.vertex_orbit_counts(torch.tensor(nodes), torch.tensor(orbit), 0, torch.tensor(columns)).shape) == (0, 6)
    none = torch.zeros((0, 4), dtype=torch.int64)
    assert graphlets.vertex_orbit_counts(none, none, 3, torch.tensor(columns)).tolist() == [[0] * 6] * 3
