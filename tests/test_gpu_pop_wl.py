"""The WL population (uniform_sampler.PopulationCache(..., wl_iterations=), ugs_uniform.hip: uni_pop_wl_ids / uni_pop_loops): the ids
of pop.sample_*(..., wl=table) against the law (tests/pop_wl_law.py) and against WLVocab.ids over the uncached uniform_sampler call
on the same batch -- every id of every call, bit for bit.  The vertex limits are process-wide: the tests that change them restore
them."""
import random
import threading

import numpy as np
import pytest
import torch

import pop_wl_law as PW
import uniform_wide_law as W
import wl_feature_law as FL
import wl_law as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def us():
    import uniform_sampler
    return uniform_sampler


def wl():
    from ugs_sampler import wl as module
    return module


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def path(n):
    return n, np.array([list(range(n - 1)), list(range(1, n))], np.int64).reshape(2, -1)


def complete(n):
    return n, np.array([(u, v) for u in range(n) for v in range(n) if u != v], np.int64).T.reshape(2, -1)


def star(leaves, extra=()):
    return leaves + 1, np.array([(0, v) for v in range(1, leaves + 1)] + list(extra), np.int64).T


# a path, K4, K8, K12 (vertices of degree 3, 7, 11: messages of exactly 128, 256, 384 bytes from the second iteration on), a star with
# 11 leaves (labels "11" and "1"), the same with two leaves joined ("11", "2", "1": "11" sorts before "2"), and a path of 3
SMALL = [path(13), complete(4), complete(8), complete(12), star(11), star(11, [(3, 4)]), path(3)]


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), (what, nm)


def add_all(pop, graphs, first=0, **kw):
    pop.add_many(range(first, first + len(graphs)), [(t(e), n) for n, e in graphs], **kw)


def vocab_of(hexes, keep=2):
    """every keep-th distinct digest, ids in shuffled order: the others are unknown"""
    known = sorted({h for h in hexes if h is not None})[::keep]
    ids = list(range(len(known)))
    random.Random(len(known)).shuffle(ids)
    return dict(zip(known, ids))


def shuffled_batch(graphs, first, seed):
    ei, ptr = W.batch(graphs, first=first)
    return np.ascontiguousarray(ei[:, np.random.RandomState(seed).permutation(ei.shape[1])]), ptr


def check_three_calls(pop, order, by_index, k, it, m, labels=None, first=0, seed=42, vocab=None, kinds=("batch", "graphs", "distinct")):
    """All three calls over the batch of the graphs `order`: tensors, ids against the law, ids against WLVocab.ids over the uncached
    call.  Returns the ids of sample_batch."""
    ei, ptr = shuffled_batch([by_index[i] for i in order], first, seed & 0xFFFF)
    lab = PW.batch_labels(order, ptr, labels)
    lab_t = None if lab is None else torch.tensor(lab, dtype=torch.int64)
    rows = W.sample_batch(ei, ptr, m, k, "sample", seed)
    if vocab is None:
        hexes = (L.wl_rows(*rows[:3], it) if lab is None else FL.wl_feature_rows(*rows[:3], lab, it))[0]
        vocab = vocab_of(hexes)
    table = wl().WLVocab(vocab, DEV)
    unknown, out = len(vocab), None
    args = (list(order), t(ptr), t(ei), m)
    if "batch" in kinds:
        want = PW.ids_of_rows(*rows[:3], vocab, it, lab)
        for mode in ("sample", "global"):
            *five, ids = pop.sample_batch(*args, mode, seed, wl=table)
            assert_same(five, W.sample_batch(ei, ptr, m, k, mode, seed), f"sample_batch {mode}")
            assert ids.dtype == torch.int64 and ids.device == five[0].device and ids.tolist() == want, f"sample_batch {mode}: ids against the law"
        unc = us().sample_batch(t(ei), t(ptr), m, k, "sample", seed)
        assert want == table.ids(*unc[:3], iterations=it, node_labels=lab_t).tolist(), "sample_batch: ids against WLVocab.ids"
        out = want
    seeds = [(seed * 7 + 13 * g) & ((1 << 64) - 1) for g in range(len(order))]
    if "graphs" in kinds:
        *six, ids = pop.sample_graphs(*args, seeds, "global", wl=table)
        unc = us().sample_graphs(t(ei), t(ptr), m, k, seeds, "sample")
        assert len(six) == 6 and torch.equal(six[5], unc[5]) and torch.equal(six[0], us().sample_graphs(t(ei), t(ptr), m, k, seeds, "global")[0])
        failed = {g for g in range(len(order)) if bool(unc[5][g])}
        assert ids.tolist() == PW.sample_graphs_ids(ei, ptr, m, k, seeds, vocab, it, order, labels, failed), "sample_graphs: ids against the law"
        assert ids.tolist() == table.ids(*unc[:3], iterations=it, node_labels=lab_t).tolist(), "sample_graphs: ids against WLVocab.ids"
    if "distinct" in kinds:
        *seven, ids = pop.sample_distinct(*args, seeds, "sample", wl=table)
        unc = us().sample_distinct(t(ei), t(ptr), m, k, seeds, "sample")
        assert len(seven) == 7 and all(torch.equal(a, b) for a, b in zip(seven, unc))
        want, valid = PW.distinct_ids(ei, ptr, m, k, seeds, vocab, it, order, labels)
        assert seven[6].tolist() == valid
        assert ids.tolist() == want, "sample_distinct: ids against the law"
        assert ids.tolist() == table.ids(*unc[:3], iterations=it, node_labels=lab_t).tolist(), "sample_distinct: ids against WLVocab.ids"
        for g, v in enumerate(valid):
            assert ids[g * m + v:(g + 1) * m].tolist() == [unknown] * (m - v)
    return out


# ---- 1. the mask form: every k, every iteration count ----
@pytest.mark.parametrize("k,it", [(1, 3), (2, 3), (3, 3), (4, 3), (8, 3), (12, 3), (4, 0), (4, 1), (8, 8), (3, 8)])
def test_mask_form(k, it):
    pop = us().PopulationCache(k, DEV, wl_iterations=it)
    add_all(pop, SMALL)
    order = [3, 0, 6, 1, 5, 2, 4]                       # the path of 3 has no member from k = 4 on: rows of -1 in the middle
    ids = check_three_calls(pop, order, SMALL, k, it, 40, first=2, seed=100 + k)      # 280 rows: two workgroups of the id kernel
    assert len(set(ids)) > 1 or k <= 2                  # (one vertex, one edge: a single class)
    sizes = pop.sizes(range(len(SMALL)))
    assert pop.info()["wl_rows_hashed"] == int(sizes.clamp(min=0).sum())
    pop.close()


def test_k_32_and_the_refusal_above():
    pop = us().PopulationCache(32, DEV, wl_iterations=3)
    add_all(pop, [path(33), path(32)])
    assert pop.sizes([0, 1]).tolist() == [2, 1] and pop.info()["wl_rows_hashed"] == 3
    check_three_calls(pop, [1, 0], [path(33), path(32)], 32, 3, 6, first=1, seed=9)
    pop.close()
    with pytest.raises(ValueError, match="1 <= k <= 32"):
        us().PopulationCache(33, DEV, wl_iterations=3)


# ---- 2. the wide form ----
@pytest.mark.parametrize("k,it", [(3, 3), (8, 3), (2, 1)])
def test_wide_form_of_the_small_graphs(k, it):
    prev = us()._set_mask_vertices(0)
    try:
        pop = us().PopulationCache(k, DEV, wl_iterations=it)
        add_all(pop, SMALL)
        check_three_calls(pop, [3, 0, 6, 1, 5, 2, 4], SMALL, k, it, 24, first=1, seed=31 + k)
        pop.close()
    finally:
        us()._set_mask_vertices(prev)


def test_wide_form_of_a_path_of_65():
    graphs = [path(65), complete(4)]
    prev = us().set_max_vertices(128)
    try:
        pop = us().PopulationCache(3, DEV, wl_iterations=3)
        add_all(pop, graphs)
        assert pop.sizes([0, 1]).tolist() == [63, 4]
        check_three_calls(pop, [0, 1, 0], graphs, 3, 3, 70, seed=65)
        pop.close()
    finally:
        us().set_max_vertices(prev)


# ---- 3. loops and columns ----
TRIANGLE = np.array([[0, 1, 2], [1, 2, 0]], np.int64)
LOOPED = np.concatenate([TRIANGLE, [[1], [1]], TRIANGLE[:, :1], TRIANGLE[::-1, 1:2]], axis=1)     # a loop on 1, a duplicate, a reversed duplicate


@pytest.mark.parametrize("labels", [None, {0: [7, 7, 9], 1: [1, 2, 3, 4, 5]}], ids=["degrees", "labels"])
def test_loops_and_columns(labels):
    graphs = [(3, LOOPED), path(5)]
    kw = {} if labels is None else {"node_labels": [torch.tensor(labels[i]) for i in range(2)]}
    for k in (2, 3):
        pop = us().PopulationCache(k, DEV, wl_iterations=3)
        add_all(pop, graphs, **kw)
        with_loop = check_three_calls(pop, [1, 0], graphs, k, 3, 9, labels, first=4, seed=5)
        # the loop-free triangle under the same index: the same sets, another loop set
        bare = [(3, TRIANGLE), path(5)]
        ei, ptr = shuffled_batch([bare[1], bare[0]], 4, 5)
        rows = W.sample_batch(*shuffled_batch([graphs[1], graphs[0]], 4, 5), 9, k, "sample", 5)
        lab = PW.batch_labels([1, 0], ptr, labels)
        vocab = vocab_of((L.wl_rows(*rows[:3], 3) if lab is None else FL.wl_feature_rows(*rows[:3], lab, 3))[0])
        table = wl().WLVocab(vocab, DEV)
        for call in (lambda **kw2: pop.sample_batch([1, 0], t(ptr), t(ei), 9, "sample", 5, wl=table, **kw2),
                     lambda **kw2: pop.sample_graphs([1, 0], t(ptr), t(ei), 9, [1, 2], wl=table, **kw2),
                     lambda **kw2: pop.sample_distinct([1, 0], t(ptr), t(ei), 9, [1, 2], wl=table, **kw2)):
            with pytest.raises(RuntimeError, match="graph 1 of the batch does not have the loop vertices"):
                call()
            call(check=False)
        *five, ids = pop.sample_batch([1, 0], t(ptr), t(ei), 9, "sample", 5, wl=table, check=False)
        assert ids.tolist() == with_loop, "check=False: the ids of the added graph"
        assert_same(five, W.sample_batch(ei, ptr, 9, k, "sample", 5), "the tensors follow the batch's own columns")
        assert_same(pop.sample_batch([1, 0], t(ptr), t(ei), 9, "sample", 5), W.sample_batch(ei, ptr, 9, k, "sample", 5), "without wl= no loop check")
        # and the other way round: a population of the bare triangle refuses the looped batch
        pop2 = us().PopulationCache(k, DEV, wl_iterations=3)
        add_all(pop2, bare, **kw)
        ei2, ptr2 = shuffled_batch(graphs, 0, 6)
        with pytest.raises(RuntimeError, match="graph 0 of the batch does not have the loop vertices"):
            pop2.sample_batch([0, 1], t(ptr2), t(ei2), 3, wl=table)
        pop.close()
        pop2.close()


# ---- 4. rows of -1 ----
def test_rows_of_minus_one():
    empty, big = (0, np.zeros((2, 0), np.int64)), path(70)
    graphs = [complete(4), path(2), empty, path(6), big]
    pop = us().PopulationCache(3, DEV, wl_iterations=3)
    add_all(pop, graphs)
    assert pop.failed == {4} and pop.sizes(range(5)).tolist() == [4, 0, 0, 4, -1]
    # a graph with n < k and an empty graph between healthy ones
    ids = check_three_calls(pop, [0, 1, 2, 3], graphs, 3, 3, 6, first=3, seed=17, kinds=("batch", "distinct"))
    assert set(ids[6:18]) == {max(ids)}                 # the unknown id, len(vocab), is the largest an id can be
    # a graph refused for its size: m unknown ids and failed[g] (sample_graphs), the whole bag of the others (sample_distinct, m > |S_g|)
    check_three_calls(pop, [3, 4, 0], graphs, 3, 3, 6, first=0, seed=18, kinds=("graphs",))
    ei, ptr = W.batch([graphs[3], graphs[4], graphs[0]])
    members = PW.member_digests(ei, ptr, 0, 3, 3) + PW.member_digests(ei, ptr, 2, 3, 3)
    vocab = {h: i for i, h in enumerate(sorted(set(members)))}
    table = wl().WLVocab(vocab, DEV)
    *six, ids = pop.sample_graphs([3, 4, 0], t(ptr), t(ei), 5, [1, 2, 3], wl=table)
    assert six[5].tolist() == [False, True, False] and ids[5:10].tolist() == [len(vocab)] * 5 and len(vocab) not in ids[:5].tolist() + ids[10:].tolist()
    *seven, ids = pop.sample_distinct([3, 4, 0], t(ptr), t(ei), 7, [1, 2, 3], wl=table)
    assert seven[6].tolist() == [4, 0, 4]
    assert ids.tolist() == [vocab[h] for h in members[:4]] + [len(vocab)] * 10 + [vocab[h] for h in members[4:]] + [len(vocab)] * 3
    pop.close()


# ---- 5. the labelled form ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
def test_feature_labels(dtype):
    graphs = [path(6), complete(4), star(5)]
    rs = np.random.RandomState(3)
    xs = [torch.from_numpy(rs.randint(0, 3, size=(n, 2))).to(dtype) for n, _ in graphs]
    xs[0][4] = xs[0][1]                                 # two vertices with equal rows
    labels = {i: FL.labels_of(x.numpy()) for i, x in enumerate(xs)}
    assert labels[0][4] == labels[0][1]
    pop = us().PopulationCache(3, DEV, wl_iterations=3)
    add_all(pop, graphs, x=xs)
    check_three_calls(pop, [2, 0, 1, 0], graphs, 3, 3, 12, labels, first=1, seed=77)
    # the same labels given directly make the same classes
    pop2 = us().PopulationCache(3, DEV, wl_iterations=3)
    add_all(pop2, graphs, node_labels=[torch.tensor(labels[i]) for i in range(3)])
    assert torch.equal(pop.wl_digests()[0], pop2.wl_digests()[0])
    with pytest.raises(RuntimeError, match="same labelling"):
        pop.add(9, t(graphs[0][1]), 6)
    pop.close()
    pop2.close()


def test_a_label_of_2_to_the_32_gives_no_digest_to_the_members_that_hold_it():
    graphs = [path(6), complete(4)]
    labels = {0: [3, 1 << 32, 3, 4, 5, 3], 1: [0, (1 << 32) - 1, 2, 2]}
    for k in (1, 3):
        pop = us().PopulationCache(k, DEV, wl_iterations=3)
        add_all(pop, graphs, node_labels=[torch.tensor(labels[i]) for i in range(2)])
        ei, ptr = W.batch(graphs)
        known = PW.population_digests([(ei, ptr)], k, 3, [PW.batch_labels([0, 1], ptr, labels)])
        got = pop.wl_digests()
        assert wl().hexdigests(*got) == known
        vocab = {h: i for i, h in enumerate(known)}
        check_three_calls(pop, [1, 0], graphs, k, 3, 16, labels, first=0, seed=4, vocab=vocab)
        # exactly the members with vertex 1 of the path are unknown
        *seven, ids = pop.sample_distinct([0], t(ptr[:2]), t(graphs[0][1]), 10, [5], wl=wl().WLVocab(vocab, DEV))
        sets = W.sorted_tuples([0b10, 0b101, 0b1010, 0b10100, 0b101000, 0b10000], k)
        assert [i == len(vocab) for i in ids[:len(sets)].tolist()] == [1 in s for s in sets]
        pop.close()


# ---- 6. the class table grows, an index is added again ----
def test_class_table_growth_and_re_adding():
    first, later = [path(5), complete(4)], [(3, LOOPED), path(5)]
    pop = us().PopulationCache(3, DEV, wl_iterations=3)
    add_all(pop, first)
    vocab = wl().extend_vocab({}, *pop.wl_digests())
    assert len(vocab) == pop.info()["wl_classes"] == 2 and list(vocab) == sorted(vocab)
    table = wl().WLVocab(vocab, DEV)
    ei, ptr = W.batch(first)
    *_, before = pop.sample_batch([0, 1], t(ptr), t(ei), 20, "sample", 3, wl=table)
    assert len(vocab) not in before.tolist()
    bytes_before = pop.info()["bytes"]
    add_all(pop, later, first=2)                        # the triangle with a loop is a new class
    assert pop.info()["wl_classes"] == 3 and pop.info()["bytes"] > bytes_before
    *_, again = pop.sample_batch([0, 1], t(ptr), t(ei), 20, "sample", 3, wl=table)
    assert torch.equal(before, again)
    ei2, ptr2 = W.batch([first[0], later[0], first[1]])
    *_, mixed = pop.sample_batch([0, 2, 1], t(ptr2), t(ei2), 20, "sample", 3, wl=table)
    want = PW.sample_batch_ids(ei2, ptr2, 20, 3, 3, vocab, 3)
    assert mixed.tolist() == want and len(vocab) in want[20:40] and len(vocab) not in want[:20] + want[40:]
    full = wl().extend_vocab(dict(vocab), *pop.wl_digests())
    assert len(full) == 3
    *_, known = pop.sample_batch([0, 2, 1], t(ptr2), t(ei2), 20, "sample", 3, wl=wl().WLVocab(full, DEV))
    assert known.tolist() == PW.sample_batch_ids(ei2, ptr2, 20, 3, 3, full, 3) and len(full) not in known.tolist()
    # index 0 again, with another graph: its ids follow the new graph
    pop.add(0, t(later[0][1]), later[0][0])
    ei3, ptr3 = W.batch([later[0], first[1]])
    *five, ids = pop.sample_batch([0, 1], t(ptr3), t(ei3), 20, "sample", 8, wl=wl().WLVocab(full, DEV))
    assert_same(five, W.sample_batch(ei3, ptr3, 20, 3, "sample", 8))
    assert ids.tolist() == PW.sample_batch_ids(ei3, ptr3, 20, 3, 8, full, 3)
    pop.close()


# ---- 7. no hashing per step; without wl= a WL population is a plain one ----
def test_nothing_is_hashed_per_step_and_calls_without_wl_are_unchanged():
    graphs = SMALL[:3] + [path(2)]
    pop, plain = us().PopulationCache(3, DEV, wl_iterations=3), us().PopulationCache(3, DEV)
    add_all(pop, graphs)
    add_all(plain, graphs)
    hashed = pop.info()["wl_rows_hashed"]
    assert hashed == int(pop.sizes(range(4)).sum()) == 11 + 4 + 56
    table = wl().WLVocab(wl().extend_vocab({}, *pop.wl_digests()), DEV)
    ei, ptr = shuffled_batch([graphs[i] for i in (2, 3, 0, 1)], 1, 3)
    args = ([2, 3, 0, 1], t(ptr).to(DEV), t(ei).to(DEV), 8)
    for step in range(7):
        pop.sample_batch(*args, "sample", step, wl=table)
        pop.sample_graphs(*args, [step, 1, 2, 3], wl=table)
        pop.sample_distinct(*args, step, wl=table)
    assert pop.info()["wl_rows_hashed"] == hashed
    for a, b in ((pop.sample_batch(*args, "global", 5), plain.sample_batch(*args, "global", 5)),
                 (pop.sample_graphs(*args, [9, 8, 7, 6]), plain.sample_graphs(*args, [9, 8, 7, 6])),
                 (pop.sample_distinct(*args, 4), plain.sample_distinct(*args, 4))):
        assert len(a) == len(b) and all(torch.equal(x, y) and x.is_cuda for x, y in zip(a, b))
    *five, ids = pop.sample_batch(*args, "sample", 5, wl=table)
    assert ids.is_cuda and ids.tolist() == PW.sample_batch_ids(ei, ptr, 8, 3, 5, table.to_dict(), 3)
    assert pop.info()["bytes"] > plain.info()["bytes"] and "wl_classes" not in plain.info()
    pop.close()
    plain.close()


# ---- 8. threads ----
def test_two_threads_sample_while_a_third_adds():
    graphs = SMALL[:4]
    pop = us().PopulationCache(3, DEV, wl_iterations=3, block_keys=64)
    add_all(pop, graphs)
    digests = wl().hexdigests(*pop.wl_digests())
    vocabs = [{h: i for i, h in enumerate(digests)}, {h: 5 - i for i, h in enumerate(digests[1:])}]
    cases = []
    for i, order in enumerate([(3, 0, 1), (2, 2, 0, 1)]):
        ei, ptr = shuffled_batch([graphs[j] for j in order], i, i)
        cases.append((list(order), ei, ptr, wl().WLVocab(vocabs[i], DEV), [PW.sample_batch_ids(ei, ptr, 50, 3, 60 + 2 * r + i, vocabs[i], 3) for r in range(4)]))
    errors = []

    def sample(i):
        order, ei, ptr, table, want = cases[i]
        try:
            for r in range(4):
                *five, ids = pop.sample_batch(order, t(ptr), t(ei), 50, "sample", 60 + 2 * r + i, wl=table)
                assert ids.tolist() == want[r], f"thread {i} round {r}"
                assert_same(five, W.sample_batch(ei, ptr, 50, 3, "sample", 60 + 2 * r + i), f"thread {i}")
        except BaseException as e:                                  # noqa: BLE001
            errors.append((i, repr(e)))

    def add():
        try:
            add_all(pop, [star(6), (3, LOOPED), path(9)], first=10)     # the triangle with a loop brings a new class
        except BaseException as e:                                  # noqa: BLE001
            errors.append(("add", repr(e)))

    threads = [threading.Thread(target=sample, args=(0,)), threading.Thread(target=sample, args=(1,)), threading.Thread(target=add)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert pop.info()["graphs"] == 7 and pop.info()["wl_classes"] > len(digests)
    # after the add: the old tables still answer the old classes, the new graphs' classes are unknown to them
    order, ei, ptr, table, want = cases[0]
    *_, ids = pop.sample_batch(order, t(ptr), t(ei), 50, "sample", 60, wl=table)
    assert ids.tolist() == want[0]
    pop.close()
