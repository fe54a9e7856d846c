"""The streams="row" law of rwr_sampler (tests/rwr_row_law.py; stated in include/ugs_mi355.h at ugs_rwr_sample_rows_begin) on the
CPU: every row is row 0 of a one-graph, m = 1 call of the per-graph law (tests/rwr_law.py, which f15_rwr_reference pins to the
reference), a row does not depend on m, the rows written without walking are what walking gives, the distribution is the
per-graph law's, and the inputs of tests/rwr_row_paths.py reach the kernel paths they are named for."""
import collections
import os
import re

import numpy as np
import pytest

import rwr_law as R
import rwr_row_law as RR
import rwr_row_paths as Q

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ss-gnn_amd", "csrc")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
CASE_NAMES = [c.name for c in Q.cases()]


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), (what, nm)


def row_of(out, row):
    """(nodes row, its edge entries) of a five-tuple"""
    lo, hi = int(out[2][row]), int(out[2][row + 1])
    return out[0][row], out[1][:, lo:hi], out[4][lo:hi]


@pytest.mark.parametrize("name", ["T0", "graph_seeds", "components_k9", "km_k9", "p099_live"])
@pytest.mark.parametrize("mode", ["sample", "global"])
def test_each_row_is_row_0_of_the_one_graph_call_at_its_row_seed(name, mode):
    c = Q.case(name)
    G = len(c.ptr) - 1
    assert G >= 2 or name in ("components_k9", "p099_live")
    got = Q.law_of(name, mode)
    assert got[2].shape == (G * c.m + 1,) and np.array_equal(got[3], np.arange(G + 1) * c.m)
    for g in range(G):
        sg = RR.graph_seed(g, c.seed, c.seeds)
        for s in range(c.m):
            one = R.sample_batch(c.ei, c.ptr[g:g + 2], 1, c.k, mode, RR.row_seed(sg, s), c.p)
            for a, b in zip(row_of(got, g * c.m + s), row_of(one, 0)):
                assert np.array_equal(a, b), (name, mode, g, s)


def test_the_first_rows_of_a_longer_call_are_the_shorter_call():
    c = Q.case("graph_seeds")
    for seeds in (None, c.seeds):
        short = RR.sample_batch(c.ei, c.ptr, 37, c.k, "sample", 9, c.p, seeds)
        long = RR.sample_batch(c.ei, c.ptr, 100, c.k, "sample", 9, c.p, seeds)
        for g in range(len(c.ptr) - 1):
            for s in range(37):
                for a, b in zip(row_of(short, g * 37 + s), row_of(long, g * 100 + s)):
                    assert np.array_equal(a, b), (g, s)


def test_row_seed_is_the_generators_unused_draw_0():
    for sg in (0, 42, (1 << 64) - 1, 1 << 63):
        assert RR.row_seed(sg, 0) == R.mix(R.SplitMix64(sg).state) == R.draw(sg, 0)      # the state before the first output, mixed
        assert all(RR.row_seed(sg, s) == R.draw(sg, s) for s in range(50))
        assert RR.row_seed(sg, 1) != R.draw((sg + R.GAMMA) & R.M64, 1)
    for name in ("mixed20_s1451", "cap_s8_m24", "rows_across_blocks", "placement_graph_seeds"):
        import rwr_paths as P
        c = P.case(name)
        for g, chain in enumerate(P.census_starts_of(name)[1]):
            if chain is None:
                continue
            sg = P.graph_seed(c, g)
            assert RR.row_seed(sg, 0) not in {R.draw(sg, i) for i in range(1, min(chain[-1], 20000) + 1)}, (name, g)


@pytest.mark.parametrize("name", ["components_k9", "doomed91", "mixed20", "p1_live", "T0"])
def test_rows_written_without_walking_are_what_walking_gives(name):
    c = Q.case(name)
    walked = RR.sample_batch(c.ei, c.ptr, c.m, c.k, "sample", c.seed, c.p, c.seeds, shortcuts=False)
    assert_same(Q.law_of(name, "sample"), walked, name)
    census = Q.census_of(name)
    assert census["doomed"] > 0 or census["p1_shortcut"] > 0 or name == "T0"


CHI2_999 = {36: 67.985, 47: 82.720}      # 0.999 quantiles of chi-square


def test_distribution_is_the_per_graph_laws_and_neighbouring_rows_are_independent():
    """7-vertex graph, k = 3, m = 40 000, seed 7, p = 0.2: a two-sample chi-square between the per-graph law's rows and the row
    law's rows over the ordered rows (48 cells), and a chi-square of independence between the seed vertices of rows s and s + 1."""
    ei = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (6, 5)], np.int64).T
    ptr, m = np.array([0, 7], np.int64), 40000
    a = collections.Counter(map(tuple, R.sample_batch(ei, ptr, m, 3, "sample", 7, 0.2)[0].tolist()))
    rows = RR.sample_batch(ei, ptr, m, 3, "sample", 7, 0.2)[0]
    b = collections.Counter(map(tuple, rows.tolist()))
    cells = sorted(set(a) | set(b))
    assert len(cells) == 48 and min(min(a[c], b[c]) for c in cells) >= 300
    chi2 = sum((a[c] - b[c]) ** 2 / (a[c] + b[c]) for c in cells)
    print(f"two-sample chi2 = {chi2:.1f}, df = {len(cells) - 1}")
    assert chi2 < CHI2_999[len(cells) - 1]
    first = rows[:, 0]
    table = np.zeros((7, 7))
    np.add.at(table, (first[:-1], first[1:]), 1)
    expected = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / table.sum()
    ind = float(((table - expected) ** 2 / expected).sum())
    print(f"independence chi2 = {ind:.1f}, df = 36")
    assert ind < CHI2_999[36]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_reach_their_classes(name):
    c, census = Q.case(name), Q.census_of(name)
    for cls in c.reaches:
        assert census[cls] > 0, f"the input no longer reaches {cls!r}: choose it again (census: {dict(census)})"


def test_census_counts_draws_and_classes():
    c = Q.case("mixed20")
    census, rows = RR.census_rows(c.ei, c.ptr, c.m, c.k, c.seed, c.p)
    assert len(rows) == c.m and [r.s for r in rows] == list(range(c.m))
    adj = R.adjacency(c.ei[0], c.ei[1], c.ptr)[0]
    for r in rows:
        chosen, L = R.walk(adj, c.k, c.p, RR.row_seed(c.seed, r.s), 0)
        assert r.draws == L and r.found == (len(chosen) >= c.k) and r.doomed + r.live_failed + r.found == 1
    assert census["doomed"] == sum(r.doomed for r in rows) and census["KM == 8"] == 1


def test_census_constants_are_the_kernels():
    with open(os.path.join(CSRC, "ugs_rwr.hip")) as f:
        hip = f.read()
    const = lambda name: int(re.search(r"constexpr \w+ %s = (\d+);" % name, hip).group(1))
    assert const("RWR_ROW_LANES") == RR.ROW_LANES
    assert "c.row_wgs = (int32_t)(((int64_t)c.m + RWR_ROW_LANES - 1) / RWR_ROW_LANES);" in hip
    assert "* RWR_ROW_LANES + tid;" in hip
    assert "if (rwr_csr_words(gd.n, D) <= c.row_lds_ints) {" in hip
    assert "return (int64_t)n + 1 + D + (n + 3) / 4; }" in hip
    assert "words <= RWR_LDS_INTS && words > c.row_lds_ints" in hip
    assert [int(x) for x in re.findall(r"launch_row_walks<(\d+)>\(c, s\);", hip)] == list(R.KM_WIDTHS)
