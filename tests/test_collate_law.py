"""The CPU Collator (pack, _unpack_torch) held to the collation law of tests/collate_law.py on every case the GPU test runs, so
that the case maker, the law and the torch path agree before a GPU is involved; and the wire layout's alignment guarantee."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import collate_law as law
import collate_run as run

CASES = law.all_cases()
WIRE = {"n32": torch.int32, "n64": torch.int64, "u8": torch.uint8, "i32": torch.int32, "i64": torch.int64, "s32": torch.int32, "s64": torch.int64}


def test_the_law_on_a_hand_made_batch():
    a = (np.array([[5, 6], [-1, -1]]), np.array([[0, 1, 9], [1, 0, 9]]), np.array([0, 2, 2]), np.array([7, 8, 9]))     # one junk entry of slack
    b = (np.zeros((0, 2), np.int64), np.zeros((2, 0), np.int64), np.array([0]), np.zeros(0, np.int64))
    c = (np.array([[3, 4]]), np.array([[1], [0]]), np.array([0, 1]), np.array([2]))
    nodes, eidx, eptr, esrc = law.expected([a, b, c])
    assert nodes.tolist() == [[5, 6], [-1, -1], [3, 4]] and eptr.tolist() == [0, 2, 2, 3]
    assert eidx.tolist() == [[0, 1, 1], [1, 0, 0]] and esrc.tolist() == [7, 8, 2]


def test_the_case_maker_keeps_its_promises():
    rng = np.random.default_rng(5)
    c = law.make_case(rng, 3, (4, 0, 6), 5, (30, 0, 2000), 2 ** 40 + 8, 1000, 2 ** 31 - 1, "sample", failed_share=0.5, failed_at=[(2, -1)])
    assert c.row_off == [0, 4, 4, 10] and c.totals == [30, 0, 2000] and c.total_rows == 10
    for (n, ei, ep, es), rows, t in zip(c.locals, (4, 0, 6), (30, 0, 2000)):
        assert n.shape == (rows, 5) and ei.shape == (2, t) and ep.shape == (rows + 1,) and es.shape == (t,)
        assert ep[0] == 0 and ep[-1] == t and np.all(np.diff(ep) >= 0)
        failed = np.all(n == -1, axis=1)
        assert failed.sum() == (rows + 1) // 2 and not (n[~failed] < 0).any() and np.all(np.diff(ep)[failed] == 0)
        if t:
            assert ei.min() == 0 and ei.max() == 4 and es.min() == 0 and es.max() == 2 ** 31 - 2 and n.max() == 2 ** 40 + 7
    assert np.all(c.locals[2][0][-1] == -1)
    padded = c.padded(2005)
    assert padded[0][1].shape == (2, 2005) and np.all(padded[0][1][:, 30:] == -9) and np.all(padded[2][3][2000:] == -9)
    for got, want in zip(law.expected(padded), c.expected()):                       # the law reads the first t_r entries only
        assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        law.make_case(rng, 1, (0,), 3, (4,), 10, 10, 10, "global")


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_collator_obeys_the_law(name):
    case, cap, junk = CASES[name]
    cap = run.edge_cap_of(case, cap)
    packers, msgs = run.pack_all(case, "cpu", cap, junk)
    dst = run.collator(case, 0, "cpu", cap)
    run.deliver(dst, msgs)
    run.assert_law(run.unpack_numpy(dst), case.expected(), name)
    assert not dst.overflowed() and not any(p.overflowed() for p in packers)
    assert int(dst.max_total.item()) == max(case.totals)
    if name.startswith("width:") and name.count("-") == 2:                         # the case selects the wire types it is named after
        assert [dst.nd, dst.ed, dst.sd] == [WIRE[w] for w in name.split(":")[1].split("-")]
    if name == "width:all-bounds-at-2^31":
        assert [dst.nd, dst.ed, dst.sd] == [torch.int64] * 3
    if name == "width:sample-k256":
        assert dst.ed == torch.int32


def test_cpu_collator_steady_state():
    """one destination and one packer per rank over steps whose totals grow and shrink: every step equals its own law"""
    steps = law.steady_state_steps(11)
    cap = max(max(s.totals) for s in steps)
    assert cap == 2049
    packers, dst = None, run.collator(steps[0], 0, "cpu", cap)
    for i, s in enumerate(steps):
        packers, msgs = run.pack_all(s, "cpu", cap, packers=packers)
        run.deliver(dst, msgs)
        run.assert_law(run.unpack_numpy(dst), s.expected(), f"step {i}")
    assert int(dst.max_total.item()) == 2049 and not dst.overflowed()


def test_cpu_collator_overflow():
    """the truncated rank is the middle one: reported; nodes and edge_ptr follow the law, rank 0's entries are intact"""
    case = overflow_case()
    packers, msgs = run.pack_all(case, "cpu", 1500)
    assert [p.overflowed() for p in packers] == [False, True, False]
    dst = run.collator(case, 0, "cpu", 1500)
    run.deliver(dst, msgs)
    check_overflow_result(dst, run.unpack_numpy(dst), case)


def overflow_case():
    case = law.make_case(np.random.default_rng(12), 3, (5, 7, 4), 4, (1200, 1700, 800), 3000, 3000, 9000, "global", failed_share=0.2)
    assert case.totals[1] > 1500 > 1024 and max(case.totals[0], case.totals[2]) <= 1500
    return case


def check_overflow_result(dst, got, case):
    nodes, eidx, eptr, esrc = case.expected()
    assert dst.overflowed() and int(dst.max_total.item()) == 1700
    with pytest.raises(RuntimeError):
        dst.check()
    assert np.array_equal(got[0], nodes) and np.array_equal(got[2], eptr) and int(eptr[-1]) == 3700
    assert np.array_equal(got[1][:, :1200], eidx[:, :1200]) and np.array_equal(got[3][:1200], esrc[:1200])


def test_world_above_64_is_refused():
    with pytest.raises(RuntimeError):
        run.ud.Collator(130, 3, "global", 10, 10, 10, 4, "cpu", world=65, rank=0)
    run.ud.Collator(128, 3, "global", 10, 10, 10, 4, "cpu", world=64, rank=63)


@pytest.mark.parametrize("nb,eb,sb", list(itertools.product((4, 8), (1, 4, 8), (4, 8))))
def test_layout_sections_are_aligned_and_disjoint(nb, eb, sb):
    from ugs_sampler._lib import lib
    for k, rows_cap, edge_cap in itertools.product((1, 3, 200), (0, 1, 3, 1025), (0, 1, 3, 1025)):
        so, mb = (C.c_int64 * 4)(), C.c_int64()
        assert lib.ugs_collate_layout(k, nb, eb, sb, rows_cap, edge_cap, so, C.byref(mb)) == 0
        sizes = [rows_cap * k * nb, (rows_cap + 1) * 4, 2 * edge_cap * eb, edge_cap * sb]
        assert all(o % 16 == 0 for o in so) and mb.value % 16 == 0
        assert so[0] >= 16                                                          # the header: two int64
        ends = [o + s for o, s in zip(so, sizes)]
        assert all(ends[i] <= so[i + 1] for i in range(3)) and ends[3] <= mb.value
        assert mb.value - ends[3] < 16 and all(so[i + 1] - ends[i] < 16 for i in range(3))    # padding only: no section is oversized
