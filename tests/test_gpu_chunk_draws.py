"""The walk kernel's lane-parallel draws (ugs_kernels.hip, chunk_draws) against the CPU oracle, bit for bit.

Every call is a single-graph call in the 448-candidate tier (UGS_FORCE_TIER=1) with more than 64 rows per compute unit: the
launch-uniform instantiation of the walk in its dynamic work loop, the only place the pass runs.  tests/chunk_draws.py states the
lane layout and the chunk sizes each row count reaches; tests/test_chunk_draws.py checks both on the CPU.

Which instantiation a launch took cannot be told from its outputs -- the walk as it was gives the same rows -- so every case also
makes the same launch on a plan of its own and reads the launch record: "ugs_walk_lds<64,448,draws>" when the numbers come from
the lanes, "ugs_walk_lds<64,448>" when the walks run the generator (k + 1 > 16, the static split).

The zero state: the API takes the seed as a C int and sign-extends it, so seed = 0 makes seed + i * 0x9e37... = 0 for row i = 0 --
lane row 0 of the first wave's first chunk starts from state 0 and must take the `state 0 -> 1` rule, its three neighbours not."""
import numpy as np
import pytest

import chunk_draws as cd
import row_epilogue_batches as reb
import scenarios as sc

_results = {}


@pytest.fixture(scope="module")
def orc():
    from backends import OracleBackend
    return OracleBackend()


@pytest.fixture(scope="module")
def sparse():
    return reb.sparse_graph()


def _call(ei, ptr, m, k, mode="sample", seed=7):
    return dict(fn="sample_batch", edge_index=ei, ptr=ptr, m=m, k=k, mode=mode, seed=seed)


def _oracle(orc, name, call):
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


DRAWS, PLAIN = "ugs_walk_lds<64,448,draws>", "ugs_walk_lds<64,448>"


def _kernel(ei, ptr, rows, k, seed):
    """the launch record of the same walk on a plan of its own (the environment decides tier and split as for the call)"""
    import torch
    import ugs_sampler
    plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), k)
    plan.walk(rows, "sample", seed)
    name = plan.last_launch()["kernel"]
    plan.close()
    return name


def _check(orc, name, call, what, kernel=None):
    assert cd.chunk_sizes(call["m"]) is not None                               # the dynamic work loop
    _same(_product(call), _oracle(orc, name, call), what)
    want = kernel or (DRAWS if call["k"] + 1 <= cd.LANES_PER_ROW else PLAIN)
    assert _kernel(call["edge_index"], call["ptr"], call["m"], call["k"], call["seed"]) == want, what


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["sample", "graph", "global"])
def test_chunks_of_four_from_the_start(mode, orc, sparse, monkeypatch):
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = sparse
    assert cd.chunk_sizes(49152)[0] == 4
    _check(orc, f"sparse_49152_k8_{mode}", _call(ei, ptr, 49152, 8, mode), f"49152 rows {mode}")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("rows", [49153, 16385])
def test_drain_and_cut_short_chunks(rows, orc, sparse, monkeypatch):
    # 49 153: four from the start, the drain's two and one, an odd end; 16 385: just above the dynamic threshold, two from the start
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = sparse
    assert cd.chunk_sizes(rows)[2]
    _check(orc, f"sparse_{rows}_k8", _call(ei, ptr, rows, 8), f"{rows} rows")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_the_zero_state(orc, sparse, monkeypatch):
    # seed 0: row 0 starts from state 0 (its generator draws what state 1 draws), rows 1.. of the same chunk do not
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = sparse
    assert cd.row_state(0, 0) == (1, True) and not any(cd.row_state(0, i)[1] for i in (1, 2, 3))
    assert cd.sequential(0, 0, 9) == cd.sequential(1, 0, 9)
    _check(orc, "sparse_49152_k8_seed0", _call(ei, ptr, 49152, 8, seed=0), "seed 0")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_static_split_keeps_the_walk_as_it_was(orc, sparse, monkeypatch):
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    monkeypatch.setenv("UGS_STATIC_SPLIT", "1")
    ei, ptr = sparse
    _check(orc, "sparse_49152_k8_sample", _call(ei, ptr, 49152, 8, "sample"), "static split", kernel=PLAIN)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_rows_that_do_not_start_at_zero(sparse, monkeypatch):
    # the generator is seeded by the row's index in the job, the lanes are counted from the launch's first row
    import oracle
    import torch
    import ugs_sampler
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = sparse
    m, lo, n, k = 70001, 12345, 49152, 8
    ugs_sampler.clear_cache()
    plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), k)
    got = tuple(t.cpu().numpy() for t in plan.sample_rows(m, mode="sample", seed=7, row_begin=lo, row_count=n))
    assert plan.last_launch()["kernel"] == DRAWS
    plan.close()
    P = oracle.Preproc(ei, int(ptr[1]), k)
    want = P.sample(m, k, "local", 0, 7, lo, lo + n)
    P.close()
    _same(got, tuple(want), "row_begin 12345")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", [1, 2, 9, 15, 16])
def test_k_sweep(k, orc, sparse, monkeypatch):
    # 1: the root's numbers only, no pick; 2: one pick; 9: rows are not parked; 15: sixteen numbers, the last lane of each DPP row;
    # 16: seventeen numbers, the walks run the generator themselves in the same launch shape
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = sparse
    _check(orc, f"sparse_49152_k{k}", _call(ei, ptr, 49152, k), f"k={k}")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_root_reduction_above_65536_vertices(orc, monkeypatch):
    # (the sparse graph of the other tests has 300 vertices: the exact 32-bit road)
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = cd.ring_with_chords()
    assert int(ptr[1]) >= 65536
    _check(orc, "ring_16385_k8", _call(ei, ptr, 16385, 8, seed=5), "ring of 70000")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_relaxed_root_level(orc, monkeypatch):
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = cd.pairs_graph()
    assert cd.root_level(ei, int(ptr[1]), 3) == 1                             # one root number, picks from draw 1
    _check(orc, "pairs_16385_k3", _call(ei, ptr, 16385, 3, seed=11), "pairs, k=3")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_seed_read_through_the_captured_step(orc, sparse, monkeypatch):
    # the captured HIP graph reads its seed from device memory: the pass reads it where the walks did
    import torch
    import ugs_sampler
    monkeypatch.setenv("UGS_FORCE_TIER", "1")
    ei, ptr = sparse
    want = _oracle(orc, "sparse_49152_k8_sample", _call(ei, ptr, 49152, 8, "sample"))
    ugs_sampler.clear_cache()
    plan = ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 8)
    step = plan.graph_step(49152, "sample")
    for seed in (3, 7):                                                        # the second replay: the seed the oracle's result has
        got = step.launch(seed).result()
    got = tuple(t.cpu().numpy() for t in got)
    # (the capture launches on scratch of its own, whose launch record is not exposed; the launcher decides by the launch's shape
    # -- one graph, dynamic loop, k -- which an ordinary walk of the same rows on this plan shares)
    plan.walk(49152, "sample", 7)
    assert plan.last_launch()["kernel"] == DRAWS
    step.close()
    plan.close()
    nodes, eidx, eptr, esrc = got
    assert np.array_equal(nodes, want[0]) and np.array_equal(eidx, want[1]) and np.array_equal(eptr, want[2])
    assert np.array_equal(esrc, want[-1])
