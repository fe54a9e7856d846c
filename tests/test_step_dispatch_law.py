"""CPU: the inputs of tests/test_gpu_step_dispatch_paths.py cover every class of a growth step's dispatch (tests/step_dispatch_paths.py):
each c next to a threshold of the final's decision tree, every `need` mask the tier can ask for by kind, and both outcomes of the
upkeep behind the pick.  Everything is read from the oracle's rows alone: the replay follows them step by step and fails if a pick
is not a candidate of its step."""
import numpy as np
import pytest

import step_dispatch_paths as sdp
import order_stage_law as L


@pytest.fixture(scope="module")
def steps():
    out = {}
    for name, (ei, ptr, k) in sdp.cases().items():
        want = sdp.oracle_rows(name)
        out[name] = sdp.replay(ei, ptr, sdp.ROWS // (len(ptr) - 1), k, want[0])
    return out


def test_leaves_and_thresholds():
    assert sdp.NST == sum(1 for b in L.CHAIN if b < sdp.CAP) and L.CHAIN[sdp.NST] >= sdp.CAP
    assert sorted(set(L.CHAIN[:sdp.NST]) | {64 * j for j in range(1, sdp.CAP // 64)}) == sdp.THRESHOLDS
    for t in sdp.THRESHOLDS:                                       # a threshold is the last c of its leaf
        assert sdp.leaf_of(t)[1] == t and sdp.leaf_of(t + 1)[0] == t + 1
        assert t in sdp.C_VALUES and t + 1 in sdp.C_VALUES
    for c in range(1, sdp.CAP + 1):                                # one stage and one number of elements per lane inside a leaf
        lo, hi = sdp.leaf_of(c)
        assert lo <= c <= hi
        assert L.final_stage(lo) == L.final_stage(hi) and (lo + 63) // 64 == (hi + 63) // 64
    assert sdp.leaf_of(sdp.CAP) == (385, sdp.CAP)


def test_shapes(steps):
    cs = sdp.cases()
    assert {cs[n][2] for n in cs} >= {2, 3, 8}
    assert any(len(cs[n][1]) - 1 == 2 for n in cs), "a two-graph batch"
    ei, ptr, k = cs["degenerate"]
    assert any(0 < ptr[g + 1] - ptr[g] < k for g in range(len(ptr) - 1)), "a graph too small for a sample"
    for n in ("low", "mid", "high"):
        assert len(cs[n][1]) == 2 and 200 <= cs[n][1][1] <= 700 and cs[n][2] == 8
    assert all(len(s) > 0 for s in steps.values())


def test_every_class_occurs(steps):
    total = {name: 0 for name in sdp.CLASSES}
    for name, st in steps.items():
        for cls, cnt in sdp.census(st).items():
            total[cls] += cnt
    missing = [cls for cls, cnt in total.items() if cnt == 0]
    assert not missing, f"classes no row of the inputs reaches: {missing}"


@pytest.mark.parametrize("name", ["k2", "k3"])
def test_short_samples_take_the_last_pick_at_once(name, steps):
    k = sdp.cases()[name][2]
    st = steps[name]
    assert all(s[1] <= k - 2 for s in st)
    assert all(s[5] is None for s in st if s[1] == k - 2), "the last pick keeps nothing up to date"
    if k == 3:
        assert any(s[5] is not None for s in st)


def test_exact_rows(steps):
    ei, ptr, k = sdp.cases()["high"]
    rows = sdp.sym_rows(ei, int(ptr[1]))
    assert [len(rows[i]) for i in range(12)] == [258, 259, 300, 320, 321, 322, 384, 385, 386, 400, 420, 440]
    assert max(s[2] for s in steps["high"]) > 385
    assert np.asarray(sdp.oracle_rows("high")[0]).shape == (sdp.ROWS, k)
