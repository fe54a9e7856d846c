"""CPU: the rules behind the walk kernel's order stages (tests/order_stage_law.py), held against a literal simulation of
libstdc++'s bucket list and against the oracle's restatement (itself checked against the real container by
tests/test_oracle_stl_order.py): the stage chain, the leader fast path of the table final (stage_final) and the in-place edit
of the lowest stage a removal invalidates."""
import random

import pytest

import oracle
import order_stage_law as L


def _distinct(rng, n, hi):
    seen, out = set(), []
    while len(out) < n:
        x = rng.randrange(hi)
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def _colliding(rng, n):
    """ids that pile up in few buckets of 13 / 29 / 59 / 127 / 257: multiples of their product plus a small residue"""
    base = 13 * 29 * 59 * 127
    return _distinct(rng, n, 40) if n < 30 else list(dict.fromkeys(rng.randrange(64) * base + rng.choice([0, 1, 2, 3, 7])
                                                                     + rng.randrange(8) * 257 for _ in range(8 * n)))[:n]


def _sequences():
    rng = random.Random(7)
    for c in [1, 2, 12, 13, 14, 28, 29, 30, 59, 60, 64, 65, 100, 127, 128, 129, 200, 257, 258, 300, 448, 541]:
        yield c, _distinct(rng, c + 1, 1_000_000)
        yield c, _distinct(rng, c + 1, 3 * c + 5)
        col = _colliding(rng, c + 1)
        if len(col) == c + 1:
            yield c, col


def test_literal_list_matches_oracle_restatement():
    rng = random.Random(3)
    for n in [0, 1, 13, 14, 29, 30, 60, 128, 258, 542, 1200]:
        for hi in [n + 1, 4 * n + 3, 1 << 30]:
            s = [rng.randrange(hi) for _ in range(n)]
            assert L.stl_order_literal(s) == oracle.stl_order(s).tolist()


def test_stage_chain_gives_the_container_order():
    for c, D in _sequences():
        fs = L.final_stage(c)
        O = L.stage_orders(D, fs)
        got = [D[p] for p in L.final_order(D, c, O)]
        assert got == L.stl_order_literal(D[:c]), c


@pytest.mark.parametrize("GS", [64, 8])
def test_leader_fast_path_of_table_final(GS):
    """rank r of a final holds its bucket's leader exactly when no bucket-mate comes after it (off == 0), and the table
    final's slot arithmetic -- leader position picked beside the bucket and the offset -- names the container's element"""
    rng = random.Random(11 + GS)
    n_leader = n_all = 0
    for c, D in _sequences():
        fs = L.final_stage(c)
        O = L.stage_orders(D, fs)
        order = L.final_order(D, c, O)
        B = L.CHAIN[fs]
        arrival = {p: a for a, p in enumerate(L.stage_input(D, O[fs - 1] if fs else None, fs, c))}
        NJ = max(1, (c + GS - 1) // GS) if GS == 64 else rng.choice([1, 3, 5, 7, 9])
        for rsel in range(c):
            p, off, hp = L.table_final_pick(D, c, O, rsel, NJ, GS)
            assert p == order[rsel]
            mates_after = sum(1 for x in order[rsel + 1:] if D[x] % B == D[p] % B)
            assert off == mates_after
            lead = min((x for x in order if D[x] % B == D[p] % B), key=lambda x: arrival[x])
            assert hp == lead
            assert (off == 0) == (p == lead)
            n_leader += off == 0
            n_all += 1
    assert 0 < n_leader < n_all


def test_edit_rule_equals_recompute():
    rng = random.Random(5)
    accepted = fallback = 0
    for c, D in _sequences():
        fs = L.final_stage(c)
        if fs == 0:
            continue
        O = L.stage_orders(D, fs)
        for i in range(fs):                       # stage i < fs was materialised in this step: c > B_i
            lo = L.CHAIN[i - 1] if i else 0
            qs = list(range(lo, L.CHAIN[i]))
            for q in rng.sample(qs, min(len(qs), 12)) + [lo, L.CHAIN[i] - 1]:
                got = L.edit_stage(D, O[i], i, q)
                Dn = D[:q] + D[q + 1:]
                want = L.group_order(L.stage_input(Dn, O[i - 1] if i else None, i, L.CHAIN[i]), Dn, L.CHAIN[i])
                if got is None:
                    fallback += 1
                    # the fallback case: D[q] is its shared bucket's first arrival
                    B = L.CHAIN[i]
                    r = O[i].index(q)
                    assert r > 0 and D[O[i][r - 1]] % B == D[q] % B
                    continue
                accepted += 1
                assert got == want, (c, i, q)
                # and it is the container's order of the first B_i candidates left
                assert [Dn[p] for p in got] == L.stl_order_literal(Dn[:L.CHAIN[i]])
    assert accepted > 0 and fallback > 0


def test_census_of_c5_shaped_walks():
    """small census (tools/order_census.py runs the large one): a table final hits a leader in roughly 0.63-0.80 of the
    cases, and the edit accepts most of the removals it is offered"""
    s = L.census(walks=60, seed=2)
    assert s["finals_table"] > 3.0
    assert 0.6 < s["leader_share_of_table_finals"] < 0.85
    assert 0.5 < s["accept_share_of_edits"] <= 1.0
