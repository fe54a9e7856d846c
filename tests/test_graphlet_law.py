"""The host side of ugs_sampler.graphlets (ugs_graphlet_table, ugs_graphlet_canon_code: the same search the kernel runs) against the
brute-force law of tests/graphlet_law.py and the published graph counts.  No GPU: nothing here launches a kernel."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import graphlet_law as law
import wl_law

UGS_E_BAD_ARG, UGS_E_UNSUPPORTED = -4, -7


def host_table(n):
    from ugs_sampler._lib import lib
    count = C.c_int64(-1)
    assert lib.ugs_graphlet_table(n, None, 0, C.byref(count)) == 0
    keys = np.empty((count.value,), dtype=np.int64)
    assert lib.ugs_graphlet_table(n, keys.ctypes.data, keys.size, C.byref(count)) == 0 and count.value == keys.size
    return keys


def host_canon(code, n):
    from ugs_sampler._lib import lib
    out = C.c_uint32(0xffffffff)
    assert lib.ugs_graphlet_canon_code(int(code), n, C.byref(out)) == 0
    return out.value


def random_code(rng, n):
    p = rng.choice([0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0])
    return sum(1 << b for b in range(n * (n - 1) // 2) if rng.random() < p)


@pytest.mark.parametrize("n", range(1, 9))
def test_class_counts_and_table_shape(n):
    keys = host_table(n)
    assert len(keys) == law.GRAPHS_ON[n - 1]
    assert np.all(np.diff(keys) > 0) and np.all(keys >> 28 == n)                 # ascending, distinct, all on n vertices
    codes = keys & ((1 << 28) - 1)
    assert all(host_canon(c, n) == c for c in codes)                             # every key is a fixed point
    assert sum(law.connected(int(c), n) for c in codes) == law.CONNECTED_ON[n - 1]


@pytest.mark.parametrize("n,count", [(1, 5), (2, 20), (3, 300), (4, 300), (5, 300), (6, 300), (7, 100), (8, 30)])
def test_host_canonicaliser_against_the_law(n, count):
    rng = random.Random(40 + n)
    codes = [random_code(rng, n) for _ in range(count)]
    if n <= 6:
        want = law.canonical_codes(codes, n).tolist()
    else:
        want = [law.canonical_code(c, n) for c in codes]
    assert [host_canon(c, n) for c in codes] == want
    assert len(set(want)) > 1 or n == 1


def test_orbits_at_six_vertices():
    """Over all 2^15 codes the image of the canonicaliser is exactly table(6), code by code the law's minimum."""
    codes = np.arange(1 << 15)
    want = law.canonical_codes(codes, 6)
    got = np.array([host_canon(c, 6) for c in codes])
    assert np.array_equal(got, want)
    assert sorted(set((6 << 28) | got)) == host_table(6).tolist()


def test_wl_merges_classes_at_six_vertices():
    """The claim the module rests on: 3 rounds of degree-labelled WL give the 112 connected graphs on 6 vertices 109 digests."""
    digests = set()
    reps = [int(c) for c in host_table(6) & ((1 << 28) - 1) if law.connected(int(c), 6)]
    assert len(reps) == 112
    for c in reps:
        masks = [0] * 6
        for i, j in law.edges_of_code(c, 6):
            masks[i] |= 1 << j
            masks[j] |= 1 << i
        digests.add(wl_law.wl_from_masks(6, masks, 3)[0])
    assert len(digests) == 109


def test_python_tables_and_helpers():
    from ugs_sampler import graphlets
    for k in range(1, 9):
        assert graphlets.num_classes(k) == law.NUM_CLASSES[k - 1] == len(graphlets.table(k))
    t6 = graphlets.table(6)
    assert t6.dtype == torch.int64 and t6.tolist() == law.all_keys(6)
    assert graphlets.table(8)[:208].tolist() == t6.tolist()                      # the id of a graph does not depend on k
    for key in t6.tolist():
        n, edges = graphlets.decode(key)
        assert (n << 28) | law.code_of_edges(n, edges) == key
    keys = torch.cat([graphlets.table(7), torch.tensor([-1])])
    want = [law.connected(int(k) & ((1 << 28) - 1), int(k) >> 28) for k in keys[:-1].tolist()] + [False]
    assert graphlets.is_connected(keys).tolist() == want
    ids = torch.tensor([0, 2, 2, 7, 1, 7, 6, 5, 0], dtype=torch.int64)           # 7 = num_classes(3): not counted
    hist = graphlets.histogram(ids, torch.tensor([0, 3, 3, 9]), 3)
    assert hist.tolist() == [[1, 0, 2, 0, 0, 0, 0], [0] * 7, [1, 1, 0, 0, 0, 1, 1]]
    cube = law.code_of_edges(8, [(a, a ^ d) for a in range(8) for d in (1, 2, 4)])
    assert graphlets.search_stats(cube, 8)[0] == 48 and graphlets.search_stats((8 << 28) | ((1 << 28) - 1)) == (1, 7)


def test_refusals():
    from ugs_sampler import graphlets
    from ugs_sampler._lib import lib
    count, out = C.c_int64(0), C.c_uint32(0)
    for k in (0, 9, -1):
        assert lib.ugs_graphlet_canon(None, None, 0, 0, None, 0, k, None, 0, None, None, None) == UGS_E_UNSUPPORTED
        assert b"1 <= k <= 8" in lib.ugs_last_error()
        assert lib.ugs_graphlet_table(k, None, 0, C.byref(count)) == UGS_E_UNSUPPORTED
        assert lib.ugs_graphlet_canon_code(0, k, C.byref(out)) == UGS_E_UNSUPPORTED
        with pytest.raises(RuntimeError, match="k <= 8"):
            graphlets.num_classes(k)
        with pytest.raises(RuntimeError, match="k <= 8"):
            graphlets.table(k)
    assert lib.ugs_graphlet_canon(None, None, 0, 0, None, 0, 8, None, 0, None, None, None) == 0      # rows = 0: a no-op
    assert lib.ugs_graphlet_canon_code(8, 3, C.byref(out)) == UGS_E_BAD_ARG                          # bit 3 at n = 3
    assert lib.ugs_graphlet_table(3, None, 0, None) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_table(3, None, 0, C.byref(count)) == 0 and count.value == 4              # too small: the count only
    nodes, ei, ep = torch.zeros((2, 6), dtype=torch.int64), torch.zeros((2, 0), dtype=torch.int64), torch.zeros((3,), dtype=torch.int64)
    for fn in (graphlets.canonical, graphlets.class_ids):                        # what wl._check_inputs raises for the same faults
        with pytest.raises(TypeError):
            fn(nodes.to(torch.int32), ei, ep)
        with pytest.raises(TypeError):
            fn(nodes.numpy(), ei, ep)
        with pytest.raises(ValueError):
            fn(nodes, ei, ep[:-1])
        with pytest.raises(ValueError):
            fn(nodes, ei.t(), ep)
        with pytest.raises(ValueError):
            fn(nodes[0], ei, ep)
    with pytest.raises(TypeError):
        graphlets.num_classes(6.0)
    with pytest.raises(TypeError):
        graphlets.histogram(torch.zeros(3, dtype=torch.int32), ep, 3)
    with pytest.raises(ValueError):
        graphlets.decode(-1)
