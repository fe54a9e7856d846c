"""CPU: the two views of tests/pop_wl_law.py agree -- the ids of the rows a call gives (uniform law, then WL law) are the ids of the
members those rows draw (what the population stores) -- and the properties the GPU test leans on hold in the law itself: loops and
labels change digests, column order and duplicates do not, the ids do not depend on the batch's composition."""
import numpy as np

import pop_wl_law as PW
import uniform_distinct_law as D
import uniform_law as U
import uniform_wide_law as W
import wl_law as L

TRIANGLE = np.array([[0, 1, 2], [1, 2, 0]], np.int64)
PATH5 = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.int64)
STAR = np.array([[0] * 5, [1, 2, 3, 4, 5]], np.int64)


def vocab_of(digests):
    return {h: i for i, h in enumerate(digests)}


def test_rows_view_equals_cache_view():
    graphs = [(5, PATH5), (6, STAR), (3, TRIANGLE), (2, np.zeros((2, 0), np.int64))]
    ei, ptr = W.batch(graphs, first=2)
    for k, it in ((3, 3), (2, 1), (3, 0)):
        members = [PW.member_digests(ei, ptr, g, k, it) for g in range(4)]
        vocab = vocab_of(PW.population_digests([(ei, ptr)], k, it)[::2])            # half of the classes are unknown
        nodes = W.sample_batch(ei, ptr, 7, k, "sample", 5)[0]
        ids = PW.sample_batch_ids(ei, ptr, 7, k, 5, vocab, it)
        for row, got in enumerate(ids):
            g = row // 7
            if nodes[row][0] < 0:
                assert got == len(vocab) and not members[g]
                continue
            sets = W.sorted_tuples(U.graph_adjacency(ei[0], ei[1], int(ptr[g]), int(ptr[g + 1] - ptr[g])), k)
            d = sets.index(tuple(int(v - ptr[g]) for v in nodes[row]))
            assert got == vocab.get(members[g][d], len(vocab))
        # distinct with m above |S_g|: the whole multiset in enumeration order, unknown ids behind it
        got, valid = PW.distinct_ids(ei, ptr, 12, k, [1, 2, 3, 4], vocab, it)
        for g in range(4):
            assert valid[g] == min(12, len(members[g]))
            assert got[12 * g:12 * g + valid[g]] == [vocab.get(h, len(vocab)) for h in members[g][:valid[g]]]
            assert got[12 * g + valid[g]:12 * (g + 1)] == [len(vocab)] * (12 - valid[g])
        assert D.law(9, 3, 12) == [0, 1, 2] + [-1] * 9


def test_loops_change_digests_and_column_order_does_not():
    ptr = np.array([0, 3])
    plain = PW.member_digests(TRIANGLE, ptr, 0, 3, 3)
    noisy = np.concatenate([TRIANGLE[:, ::-1], TRIANGLE[::-1], TRIANGLE[:, :1]], axis=1)
    assert PW.member_digests(noisy, ptr, 0, 3, 3) == plain
    looped = np.concatenate([noisy, np.array([[1], [1]])], axis=1)
    assert PW.member_digests(looped, ptr, 0, 3, 3) != plain
    lab = [5, 5, 7]
    assert PW.member_digests(looped, ptr, 0, 3, 3, lab) != PW.member_digests(noisy, ptr, 0, 3, 3, lab) != plain
    assert PW.member_digests(noisy, ptr, 0, 3, 3, [5, 5, 1 << 32]) == [None]
    assert PW.member_digests(noisy, ptr, 0, 2, 3, [5, 5, 1 << 32]).count(None) == 2


def test_ids_do_not_depend_on_the_batch_composition():
    graphs = [(5, PATH5), (6, STAR)]
    labels = {0: [1, 2, 3, 2, 1], 1: [9, 4, 4, 4, 4, 4]}
    both = W.batch(graphs)
    vocab = vocab_of(PW.population_digests([both], 3, 2, [PW.batch_labels([0, 1], both[1], labels)]))
    a = PW.sample_graphs_ids(*both, 4, 3, [11, 12], vocab, 2, [0, 1], labels)
    swapped = W.batch(graphs[::-1], first=3)
    b = PW.sample_graphs_ids(*swapped, 4, 3, [12, 11], vocab, 2, [1, 0], labels)
    assert a[:4] == b[4:] and a[4:] == b[:4] and len(vocab) not in a
    assert PW.sample_graphs_ids(*both, 4, 3, [11, 12], vocab, 2, [0, 1], labels, failed={1})[4:] == [len(vocab)] * 4
    assert L.ids_from([None], [L.STATUS_EMPTY], vocab) == [len(vocab)]
