"""CPU: the law of uniform_sampler.enumerate_graphs (tests/uniform_enum_law.py) tied to the reference through the fixtures the sampler
tests already use: every row the reference drew (golden/f14_uniform_reference, golden/f18_uniform_wide_reference) is the law's
enumeration row at the index its generator drew, edges included; and the law's counts on the graphs the GPU tests use."""
import json
import os

import numpy as np
import pytest

import ugs_workloads as wl
import uniform_enum_law as EL
import uniform_law as U
from uniform_sampler import count_graphs, enumerate_graphs  # noqa: F401  (the calls whose law this file pins)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = [os.path.join(HERE, "golden", f) for f in ("f14_uniform_reference", "f18_uniform_wide_reference")]
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def scenarios():
    out = []
    for path in FIXTURES:
        with open(path + ".json") as f:
            out += [(path, s) for s in json.load(f)["scenarios"]]
    return out


@pytest.mark.parametrize("path,s", scenarios(), ids=lambda v: v["name"] if isinstance(v, dict) else "")
def test_reference_rows_are_enumeration_rows_at_the_drawn_index(path, s):
    z = np.load(path + ".npz")
    name, m, k, mode = s["name"], s["m"], s["k"], s["mode"]
    ei, ptr = z[f"{name}/in_edge_index"], z[f"{name}/in_ptr"]
    gold = [z[f"{name}/{nm}"] for nm in NAMES]
    nodes, eidx, eptr, sptr, esrc, counts = EL.enumerate_graphs(ei, ptr, k, mode)
    G = len(ptr) - 1
    assert nodes.shape == (sptr[-1], k) and np.array_equal(np.diff(sptr), counts) and (nodes >= 0).all()
    assert np.array_equal(gold[3], np.arange(G + 1) * m)
    draws = EL.draw_indices(counts, m, int(s["seed"]))
    for g in range(G):
        for i in range(m):
            row = g * m + i
            a, b = gold[2][row], gold[2][row + 1]
            if g not in draws:                                          # S_g empty: the reference pads, the enumeration has no row
                assert (gold[0][row] == -1).all() and a == b and sptr[g] == sptr[g + 1]
                continue
            r = sptr[g] + draws[g][i]
            c, d = eptr[r], eptr[r + 1]
            assert np.array_equal(gold[0][row], nodes[r]), (name, row)
            assert np.array_equal(gold[1][:, a:b], eidx[:, c:d]) and np.array_equal(gold[4][a:b], esrc[c:d]), (name, row)


def complete_graph(n):
    u, v = np.triu_indices(n, 1)
    return np.array([np.r_[u, v], np.r_[v, u]], np.int64)


@pytest.mark.parametrize("name,n,ei,k,want", [("csl41", 41, wl.csl_graph(41, 2), 6, 1312), ("K8", 8, complete_graph(8), 4, 70),
                                              ("tu20", 20, wl.tu_graph(20, 100, 1), 6, 34109)], ids=lambda v: v if isinstance(v, str) else "")
def test_law_counts(name, n, ei, k, want):
    out = EL.enumerate_graphs(ei, [0, n], k)
    assert out[5].tolist() == [want] and out[0].shape == (want, k) and out[3].tolist() == [0, want]
    assert len(U.esu_masks(U.graph_adjacency(ei[0], ei[1], 0, n), k)) == want
    rows = [tuple(r) for r in out[0].tolist()]
    assert rows == sorted(set(rows)) and all(list(r) == sorted(r) for r in rows[:50])


def test_three_enumerations_agree_on_a_small_batch():
    """the definition (all combinations), the mask form and the tuple form give the same tensors; a failed graph gives no rows"""
    graphs = [(7, wl.tu_graph(7, 9, 1)), (2, np.zeros((2, 0), np.int64)), (9, wl.tu_graph(9, 14, 2)), (0, np.zeros((2, 0), np.int64))]
    cols, ptr = [], [3]
    for n, g in graphs:
        cols.append(g + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = np.concatenate(cols + [np.array([[4, 4, 12], [4, 11, 30]])], axis=1)      # a loop, a crossing column, one outside every range
    for k in (0, 1, 3, 4):
        for mode in ("sample", "global"):
            want = EL.enumerate_graphs(ei, ptr, k, mode, how="comb")
            for how in ("masks", "tuples"):
                for a, b in zip(want, EL.enumerate_graphs(ei, ptr, k, mode, how=how)):
                    assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), (k, mode, how)
    full, part = EL.enumerate_graphs(ei, ptr, 3), EL.enumerate_graphs(ei, ptr, 3, failed=[0])
    n0 = full[3][1]
    assert part[3].tolist() == [0, 0] + (full[3][2:] - n0).tolist() and np.array_equal(part[0], full[0][n0:])
    assert np.array_equal(part[5], full[5]) and np.array_equal(part[4], full[4][full[2][n0]:])
