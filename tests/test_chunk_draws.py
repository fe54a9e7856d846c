"""CPU side of the walk kernel's lane-parallel draws (ugs_kernels.hip, chunk_draws; tests/chunk_draws.py states the layout):
the lane pass restated in numpy uint64 against the sequential generator, and a census of what the GPU cases of
tests/test_gpu_chunk_draws.py reach -- chunk sizes from their row counts, root levels from the oracle's preprocessing."""
import numpy as np
import pytest

import chunk_draws as cd
import row_epilogue_batches as reb

ZERO_ROW = 12345
SEEDS = [0, 1, 42, 7, (-5) & cd.M64, cd.M64, 0x0123456789ABCDEF, cd.zero_state_seed(ZERO_ROW), cd.zero_state_seed(ZERO_ROW + 2)]


def test_the_zero_state_seed_hits_state_zero():
    s = cd.zero_state_seed(ZERO_ROW)
    assert cd.row_state(s, ZERO_ROW) == (1, True)
    assert not cd.row_state(s, ZERO_ROW - 1)[1] and not cd.row_state(s, ZERO_ROW + 1)[1]
    assert cd.sequential(s, ZERO_ROW, 3) == cd.sequential(1, 0, 3)            # the row draws what state 1 draws


def test_seed_zero_is_the_zero_state_the_api_reaches():
    # the GPU case: a C-int seed is sign-extended, so seed 0 starts row 0 -- and no other row of a call -- from state 0
    assert cd.row_state(0, 0) == (1, True)
    assert not any(cd.row_state(0, i)[1] for i in range(1, 49152))
    assert [int(v) for v in cd.lane_pass(0, 0, 9)[0, :9]] == cd.sequential(1, 0, 9)


@pytest.mark.parametrize("seed", SEEDS)
def test_lane_pass_equals_the_sequential_generator(seed):
    # row0 chosen so that the zero-state row is each of the chunk's four rows in turn; 16 iterations: every lane is final
    for row0 in (0, 1, 4097, ZERO_ROW - 3, ZERO_ROW - 2, ZERO_ROW - 1, ZERO_ROW, (1 << 40) + 3):
        x = cd.lane_pass(seed, row0, 16)
        for r in range(4):
            assert [int(v) for v in x[r]] == cd.sequential(seed, row0 + r, 16), (seed, row0, r)


@pytest.mark.parametrize("iterations", [1, 2, 3, 9, 10, 15, 16])
def test_after_t_iterations_the_first_t_lanes_are_final(iterations):
    for seed in (42, cd.M64, cd.zero_state_seed(ZERO_ROW)):
        x = cd.lane_pass(seed, ZERO_ROW - 1, iterations)
        more = cd.lane_pass(seed, ZERO_ROW - 1, iterations + 1)
        for r in range(4):
            want = cd.sequential(seed, ZERO_ROW - 1 + r, iterations)
            assert [int(v) for v in x[r, :iterations]] == want
            assert [int(v) for v in more[r, :iterations]] == want                 # ... and stay final


def test_rows_past_the_call_compute_values_without_fault():
    # a chunk cut short still runs four rows of lanes: plain wrapping arithmetic, whatever the row index
    x = cd.lane_pass(cd.M64, cd.M64 - 1, 9)
    assert [int(v) for v in x[3, :9]] == cd.sequential(cd.M64, cd.M64 + 2, 9)


# ---------------------------------------------------------------------------------------------------------------------------
# census of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------------
def test_chunk_sizes_of_the_gpu_cases():
    assert cd.chunk_sizes(49152) == (4, [2, 1], False)          # chunks of four from the start, then the drain
    assert cd.chunk_sizes(49153) == (4, [2, 1], True)           # ... and an odd row count: a chunk is cut short
    assert cd.chunk_sizes(16385) == (2, [1], True)              # just above the dynamic threshold: two from the start
    assert cd.chunk_sizes(16384) is None                        # the static split: not what these tests are about
    for rows in (49152, 49153, 16385):
        assert rows > cd.DYNAMIC_ABOVE


def test_root_levels_and_reduction_roads_of_the_gpu_cases():
    ei, ptr = reb.sparse_graph()
    assert int(ptr[1]) < 65536
    for k in (1, 2, 8, 9, 15, 16):
        assert cd.root_level(ei, int(ptr[1]), k) == 0
    ei, ptr = cd.ring_with_chords()
    assert int(ptr[1]) >= 65536 and cd.root_level(ei, int(ptr[1]), 8) == 0
    ei, ptr = cd.pairs_graph()
    assert cd.root_level(ei, int(ptr[1]), 3) == 1


def test_the_relaxed_case_draws_one_root_number_and_one_pick():
    # by the oracle's rows: every row of the pairs graph at k = 3 is a pair (root, its one neighbour) and a failed growth step
    import oracle
    ei, ptr = cd.pairs_graph()
    P = oracle.Preproc(ei, int(ptr[1]), 3)
    nodes = P.sample(2000, 3, "local", 0, 11)[0]
    P.close()
    assert (nodes[:, 2] == -1).all() and (nodes[:, :2] >= 0).all()
    assert (nodes[:, 0] // 2 == nodes[:, 1] // 2).all() and (nodes[:, 0] != nodes[:, 1]).all()
    assert len(set(nodes[:, 0].tolist())) == 10                  # the viable list: of each pair the vertex with a later neighbour


def test_the_ring_rows_are_complete():
    import oracle
    ei, ptr = cd.ring_with_chords()
    P = oracle.Preproc(ei, int(ptr[1]), 8)
    nodes = P.sample(16385, 8, "local", 0, 5, 0, 512)[0]
    P.close()
    assert nodes.shape == (512, 8) and (nodes >= 0).all()
    assert int(nodes[:, 0].max()) >= 65536                       # roots from the whole range: the quotient estimate is exercised
