"""The walk kernel's batched row epilogue (ugs_kernels.hip, Parked): the rows of a four-row work chunk are finished together, one
DPP row of the wave per row, against the CPU oracle.

Only a call with more than 8 rows per resident wave starts its waves with chunks of four (see row_epilogue_batches.py), which no
other path test reaches: every call here has 49 152 rows unless it says otherwise.  The CPU tests prove from the oracle's rows alone
that the aligned four-row blocks of the first quarter hold what they are meant to hold: blocks of four parked rows, every kind of
row that is NOT parked at each of the four places beside a parked one, and blocks that span two graphs (m = 6: two node offsets in
one batch).  The GPU tests ask for the oracle's outputs bit for bit."""
import numpy as np
import pytest

import row_epilogue_batches as reb
import scenarios as sc

_results = {}


@pytest.fixture(scope="module")
def orc():
    from backends import OracleBackend
    return OracleBackend()


@pytest.fixture(scope="module")
def batch():
    return reb.mixed_batch()


def _call(ei, ptr, m, k, mode="sample", seed=42):
    return dict(fn="sample_batch", edge_index=ei, ptr=ptr, m=m, k=k, mode=mode, seed=seed)


def _oracle(orc, name, call):
    """the oracle's result of one call on a fresh cache, computed once per module"""
    if name not in _results:
        (res,) = sc.run_scenario([call], orc)
        assert isinstance(res, tuple) and not isinstance(res[0], str), repr(res)
        _results[name] = res
    return _results[name]


def _same(got, want, what):
    assert isinstance(got, tuple) and not isinstance(got[0], str), f"{what}: {got!r}"
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: output {j} differs"


def _product(call):
    from backends import ProductBackend
    (res,) = sc.run_scenario([call], ProductBackend())
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the inputs reach what they are meant to reach
# ---------------------------------------------------------------------------------------------------------------------------
def _census(orc, batch, k):
    ei, ptr, kinds = batch
    res = _oracle(orc, f"mixed_k{k}_sample", _call(ei, ptr, reb.M, k))
    assert res[0].shape == (reb.ROWS, k)
    return reb.census(reb.classify_rows(res, ptr, kinds, reb.M, k, reb.QUARTER), reb.M)


def test_blocks_of_the_first_quarter_at_k8_by_the_oracles_rows(orc, batch):
    # at k = 8 a connected sample has 7 hits and a self loop adds two: no row has a self hit within 8 hits (k = 5 below has) -- the
    # one kind of row that differs from a parked one only in the test that keeps it out of the batch
    seen = _census(orc, batch, 8)
    want = ["four_fast", "two_graphs"] + [f"{x}_at_{p}_beside_fast" for x in reb.OTHERS if x != reb.SELF for p in range(4)]
    for name in want:
        assert seen[name] >= 20, f"only {seen[name]} aligned blocks of the first quarter are {name}: {seen}"
    assert all(seen[f"{reb.SELF}_at_{p}_beside_fast"] == 0 for p in range(4))
    assert set(seen) == set(want) | {f"{reb.SELF}_at_{p}_beside_fast" for p in range(4)}


def test_blocks_of_the_first_quarter_at_k5_by_the_oracles_rows(orc, batch):
    seen = _census(orc, batch, 5)
    for name in ["four_fast", "two_graphs"] + [f"{reb.SELF}_at_{p}_beside_fast" for p in range(4)]:
        assert seen[name] >= 20, f"only {seen[name]} aligned blocks of the first quarter are {name}: {seen}"


def test_the_single_graph_call_has_parked_rows_only(orc):
    ei, ptr = reb.sparse_graph()
    res = _oracle(orc, "sparse_k8", _call(ei, ptr, reb.ROWS, 8, seed=7))
    kinds = reb.classify_rows(res, ptr, ["sparse"], reb.ROWS, 8, reb.QUARTER)
    assert kinds.count(reb.FAST) >= reb.QUARTER * 9 // 10 and set(kinds) <= {reb.FAST, reb.GENERAL}


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("k,mode", [(8, "sample"), (8, "graph"), (8, "global"), (5, "sample"), (2, "sample"), (9, "sample"), (1, "sample")])
def test_mixed_batch_vs_oracle(k, mode, orc, batch, monkeypatch):
    # k = 9: the rows are not parked (k > 8), the same loop with the epilogue on the spot; k = 1: rows without edges
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr, _ = batch
    call = _call(ei, ptr, reb.M, k, mode)
    _same(_product(call), _oracle(orc, f"mixed_k{k}_{mode}", call), f"k={k} {mode}")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_mixed_batch_in_the_704_candidate_tier(orc, batch, monkeypatch):
    monkeypatch.setenv("UGS_FORCE_TIER", "2")
    ei, ptr, _ = batch
    call = _call(ei, ptr, reb.M, 8)
    _same(_product(call), _oracle(orc, "mixed_k8_sample", call), "tier 2")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_mixed_batch_with_a_static_split(orc, batch, monkeypatch):
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    monkeypatch.setenv("UGS_STATIC_SPLIT", "1")                            # rows by index: no chunks, every epilogue on the spot
    ei, ptr, _ = batch
    call = _call(ei, ptr, reb.M, 8)
    _same(_product(call), _oracle(orc, "mixed_k8_sample", call), "static split")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_chunks_of_two_and_one(orc, batch, monkeypatch):
    # 20 000 rows: more than 64 per compute unit, fewer than 8 per resident wave -- the first chunk is two rows, the later ones one
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr, _ = batch
    g = 4000
    ei5 = np.ascontiguousarray(ei[:, (ei[0] < ptr[g]) & (ei[1] < ptr[g])])
    call = _call(ei5, ptr[:g + 1].copy(), 5, 8)
    _same(_product(call), _oracle(orc, "mixed_20000", call), "20000 rows")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_per_graph_seeds(batch, monkeypatch):
    import oracle
    import torch
    import ugs_sampler
    from ugs_graphs_law import oracle_loop
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr, _ = batch
    seeds = [(g * 2654435761) % (2 ** 31) - (g % 3) * 1000 for g in range(len(ptr) - 1)]
    cache = oracle.Cache()
    want = oracle_loop(ei, ptr, reb.M, 8, "graph", seeds, cache)
    cache.close()
    ugs_sampler.clear_cache()
    got = ugs_sampler.sample_graphs(torch.from_numpy(ei), torch.from_numpy(ptr), reb.M, 8, seeds, "graph")
    assert not bool(got[5].any())
    _same(tuple(t.numpy() for t in got[:5]), want, "sample_graphs")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("no_prow", [False, True])
def test_single_graph_call_vs_oracle(no_prow, orc, monkeypatch):
    # one graph, one seed, padded rows: the launch-uniform instantiation of the walk; without padded rows: the row-pointer one
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    if no_prow:
        monkeypatch.setenv("UGS_NO_PROW", "1")
    ei, ptr = reb.sparse_graph()
    call = _call(ei, ptr, reb.ROWS, 8, seed=7)
    _same(_product(call), _oracle(orc, "sparse_k8", call), f"single graph, no_prow={no_prow}")
