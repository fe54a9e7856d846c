"""The grab schedule of the walk kernel's dynamic work loop, by its plain-Python restatement (tests/work_grabs.py): whatever the order
in which the waves come back to the counter, every row is handed out exactly once, in sub-chunks of at most four, and the launch
drains through grabs of two and one.  The last test states, from the same model, what each case of tests/test_gpu_work_grabs.py
reaches on a part of a given compute-unit count."""
import random

import pytest

import work_grabs as wg


def _cases(n, seed):
    rng = random.Random(seed)
    out = [(1, 1), (2, 1), (3, 2), (7, 5120), (5121, 5120), (2 * wg.GRAB * 7 + 1, 7), (2 * wg.GRAB * 7, 7)]
    while len(out) < n:
        groups = rng.choice([1, 2, 3, 5, 16, 61, 256])
        per = rng.choice([0.3, 1.5, 2.0, 7.9, 8.1, 2 * wg.GRAB - 0.5, 2 * wg.GRAB + 0.5, 3 * wg.GRAB, 5 * wg.GRAB + 3])
        out.append((max(1, int(groups * per) + rng.randrange(-3, 4)), groups))
    return out


CASES = _cases(300, 20264)


def test_ladder():
    g = 10
    assert wg.grab_for(2 * wg.GRAB * g + 1, g) == wg.GRAB and wg.grab_for(2 * wg.GRAB * g, g) == 4
    assert wg.grab_for(8 * g + 1, g) == 4 and wg.grab_for(8 * g, g) == 2
    assert wg.grab_for(2 * g + 1, g) == 2 and wg.grab_for(2 * g, g) == 1 and wg.grab_for(1, g) == 1
    assert wg.GRAB % wg.CHUNK == 0 and 2 * wg.GRAB > 8                    # the ladder's steps are in order


def test_every_row_exactly_once_in_sub_chunks_of_at_most_four():
    rng = random.Random(20265)
    for total, groups in CASES:
        for pick in (None, rng, rng):
            grabs = wg.schedule(total, groups, pick)
            rows = sorted(r for _, lo, hi, _, _ in grabs for r in range(lo, hi))
            assert rows == list(range(total)), (total, groups)
            for wave, lo, hi, size, dyn in grabs:
                assert 0 <= wave < groups and lo < hi <= lo + size and size in (wg.GRAB, 4, 2, 1)
                subs = wg.sub_chunks(lo, hi)
                assert all(0 < b - a <= wg.CHUNK for a, b in subs) and subs[0][0] == lo and subs[-1][1] == hi
                assert all(subs[i][1] == subs[i + 1][0] for i in range(len(subs) - 1))
                assert all(b - a == wg.CHUNK for a, b in subs[:-1])          # only a grab's last sub-chunk is short


def test_a_waves_grabs_never_grow_and_the_launch_drains_through_two_and_one():
    rng = random.Random(20266)
    for total, groups in CASES:
        for pick in (None, rng):
            grabs = wg.schedule(total, groups, pick)
            per_wave = {}
            for wave, lo, hi, size, _ in grabs:
                per_wave.setdefault(wave, []).append((lo, size))
            for seq in per_wave.values():
                assert all(a[0] < b[0] and a[1] >= b[1] for a, b in zip(seq, seq[1:])), (total, groups)
            # a wave asks by its own position, which is at or behind the counter: a grab that starts at row `lo` is never SMALLER
            # than the ladder's answer for what is truly left, and the rows of the last two per group are handed out one by one
            # or two by two at the most
            for _, lo, hi, size, dyn in grabs:
                if dyn:
                    assert size >= wg.grab_for(total - lo, groups)
            first = wg.grab_for(total, groups)
            if total > first * groups + 2 * groups and first > 2:
                sizes = {size for _, _, _, size, dyn in grabs if dyn}
                assert 2 in sizes or 1 in sizes, (total, groups, sizes)


def test_in_turn_the_launch_ends_with_grabs_of_two_and_one():
    # waves that come back in turn (walks of equal cost): the counter is asked for every size below the first on the way down
    for total, groups in CASES:
        first = wg.grab_for(total, groups)
        seen = wg.sizes_reached(total, groups)
        left = total - first * groups
        want = {wg.grab_for(x, groups) for x in range(1, left + 1)} if left > 0 else set()
        assert want <= set(seen) | {first}, (total, groups, seen)
        if left > 2 * groups:
            assert seen.get(1, 0) + seen.get(2, 0) > 0
        last = max(wg.schedule(total, groups), key=lambda g: g[2])
        if last[4]:                                                        # the last row came from the counter: in a grab of two at the most
            assert last[3] <= 2, (total, groups, last)
        if groups == 1 and total > first + 2:                              # one wave: its position IS the counter
            sizes = [size for _, _, _, size, dyn in wg.schedule(total, 1) if dyn]
            assert sizes[-1] == 1 and 2 in sizes and sizes == sorted(sizes, reverse=True), (total, sizes)


@pytest.mark.parametrize("cus", [256, 304, 64, 20])
def test_what_the_gpu_cases_reach(cus):
    # (i) the mixed batch of 49 152 rows on one block per compute unit (set_walk_share(5): 5 % of 20 blocks)
    rows, groups = 49152, cus
    assert wg.is_dynamic(rows, cus)
    seen = wg.sizes_reached(rows, groups)
    assert wg.grab_for(rows, groups) == wg.GRAB and all(seen.get(s, 0) > 0 for s in (wg.GRAB, 4, 2, 1)), seen
    assert any(dyn and size == wg.GRAB for _, _, _, size, dyn in wg.schedule(rows, groups))   # G-row grabs from the counter too
    # (ii) full residency, just over 2 * GRAB rows per wave plus 13
    rows, groups = wg.full_residency_rows(cus), cus * wg.WAVES_PER_CU
    assert wg.is_dynamic(rows, cus) and wg.grab_for(rows, groups) == wg.GRAB
    seen = wg.sizes_reached(rows, groups)
    assert seen[wg.GRAB] == groups and all(seen.get(s, 0) > 0 for s in (4, 2)), seen
    assert rows % 2 == 1                  # an odd end: a grab of two or more that holds the last row is cut inside its sub-chunk
    # (iv) more than 64 rows per compute unit: the launch that redoes the handed-on rows takes the second counter
    assert wg.is_dynamic(max(40000, cus * wg.DYNAMIC_ABOVE_PER_CU + 1), cus)
