"""The host side of graphlets.labelled_keys (ugs_graphlet_labelled_code: the searches the kernel runs, started from the partition by
label) against the brute-force law of tests/graphlet_labelled_law.py, the brute-forced label-preserving automorphism groups and the
Burnside counts of labelled graphs; then the law against itself, and the Python surface that needs no device.  No GPU: nothing here
launches a kernel."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

import graphlet_law as law
import graphlet_labelled_law as llaw

UGS_E_BAD_ARG, UGS_E_UNSUPPORTED = -4, -7
MASK = (1 << 28) - 1


def host_labelled(code, n, labels, rooted=True):
    """((high word, low word), rooted codes or None) from the library."""
    from ugs_sampler._lib import lib
    lab = (C.c_int32 * 8)(*(list(int(x) for x in labels) + [-7] * (8 - n)))     # entries from n on are not read
    key = (C.c_int64 * 2)(5, 5)
    out = (C.c_uint32 * 8)(*([7] * 8))
    assert lib.ugs_graphlet_labelled_code(int(code), n, lab, key, out if rooted else None) == 0
    if not rooted:
        assert list(out) == [7] * 8
        return (key[0], key[1]), None
    assert list(out)[n:] == [0xffffffff] * (8 - n)
    return (key[0], key[1]), list(out)[:n]


def class_codes(n):
    from ugs_sampler import graphlets
    return [int(k) & MASK for k in graphlets.table(n).tolist() if k >> 28 == n]


def exhaustive(n, num_labels):
    """Every graph on n labelled vertices times every labelling with num_labels labels: (codes [R], labels [R, n])."""
    graphs = np.arange(1 << (n * (n - 1) // 2), dtype=np.int64)
    labellings = np.array(list(itertools.product(range(num_labels), repeat=n)), dtype=np.int64).reshape(-1, n)
    return np.repeat(graphs, len(labellings)), np.tile(labellings, (len(graphs), 1))


@pytest.mark.parametrize("n,num_labels", [(1, 3), (2, 3), (3, 3), (4, 3), (5, 2)])
def test_every_graph_and_every_labelling(n, num_labels):
    codes, labels = exhaustive(n, num_labels)
    assert (n != 4 or len(codes) == 5184) and (n != 5 or len(codes) == 32768)
    canon, rooted = llaw.labelled_codes_many(codes, labels, n)
    words = llaw.key_words_many(n, canon, labels)
    for r in range(len(codes)):
        key, got = host_labelled(codes[r], n, labels[r])
        assert key == tuple(words[r].tolist()) and got == rooted[r].tolist(), (n, int(codes[r]), labels[r].tolist())
    for r in range(0, len(codes), max(1, len(codes) // 50)):                     # the vectorised law is the graph-by-graph law
        lab = tuple(labels[r].tolist())
        assert llaw.labelled_codes(int(codes[r]), n, lab) == (int(canon[r]), tuple(rooted[r].tolist()))
        assert llaw.key_words(llaw.key_of(int(codes[r]), n, lab)) == tuple(words[r].tolist())
    distinct = len({tuple(w) for w in words.tolist()})
    assert distinct == llaw.burnside_labelled(n, num_labels)
    if num_labels == 2:
        assert distinct == (2, 6, 20, 90, 544)[n - 1]                            # the published series of 2-coloured graphs


def test_burnside_counts():
    assert [llaw.burnside_labelled(n, 1) for n in range(1, 9)] == list(law.GRAPHS_ON)
    assert [llaw.burnside_labelled(n, 2) for n in range(1, 6)] == [2, 6, 20, 90, 544]
    assert [llaw.burnside_labelled(n, 3) for n in range(1, 4)] == [3, 12, 56]     # 3, 6 pairs x 2, by hand for n = 3


@pytest.mark.parametrize("n", range(1, 9))
def test_constant_labels_give_the_unlabelled_codes(n):
    from ugs_sampler._lib import lib
    codes = class_codes(n)
    assert len(codes) == law.GRAPHS_ON[n - 1]
    rng = random.Random(40 + n)
    if n == 8:
        codes = rng.sample(codes, 300)
    for c in codes:
        c = law.relabel(c, n, rng.sample(range(n), n))                           # not the representative itself
        label = rng.choice([0, 1, 77, 4095])
        (hi, lo), rooted = host_labelled(c, n, [label] * n)
        canon, plain = C.c_uint32(0), (C.c_uint32 * 8)()
        assert lib.ugs_graphlet_canon_code(c, n, C.byref(canon)) == 0 and lib.ugs_graphlet_rooted_codes(c, n, plain) == 0
        assert rooted == list(plain)[:n] and min(rooted) == canon.value
        assert llaw.key_words(llaw.key_number(n, canon.value, [label] * n)) == (hi, lo)


def random_labelled(rng, n):
    p = rng.choice([0.15, 0.3, 0.5, 0.7, 0.9])
    code = law.code_of_edges(n, [(i, j) for i, j in law.pairs(n) if rng.random() < p])
    if rng.random() < 0.3:                                                       # symmetric shapes: ties for the search to permute
        code = law.code_of_edges(n, rng.choice([[(i, (i + 1) % n) for i in range(n)], [(0, i) for i in range(1, n)],
                                                [(i, j) for i, j in law.pairs(n)], [(i, i + 1) for i in range(n - 1)],
                                                [(i, j) for i, j in law.pairs(n) if (i < n // 2) != (j < n // 2)]]))
    count = rng.choice([1, 2, 2, 3, n])
    labels = [rng.randrange(count) * rng.choice([1, 1365]) for _ in range(n)] if count < n else rng.sample(range(4096), n)
    return code, labels


@pytest.mark.parametrize("n,cases", [(6, 100), (7, 100), (8, 40)])
def test_the_law_itself_and_the_host_on_random_labelled_graphs(n, cases):
    rng = random.Random(600 + n)
    differ = same = split = 0
    for _ in range(cases):
        code, labels = random_labelled(rng, n)
        canon, rooted = llaw.labelled_codes(code, n, tuple(labels))
        K = llaw.key_number(n, canon, labels)
        assert llaw.decode(K) == (n, canon, sorted(labels))
        key, got = host_labelled(code, n, labels)
        assert key == llaw.key_words(K) and got == list(rooted), (n, code, labels)
        # invariance: the same labelled graph under a renaming of its vertices that carries the labels along
        perm = rng.sample(range(n), n)
        code2, labels2 = llaw.relabel(code, n, labels, perm)
        canon2, rooted2 = llaw.labelled_codes(code2, n, tuple(labels2))
        assert canon2 == canon and [rooted2[perm[v]] for v in range(n)] == list(rooted)
        assert host_labelled(code2, n, labels2, rooted=False)[0] == key
        # the representative the key decodes to is the same labelled graph
        assert llaw.key_of(canon, n, sorted(labels)) == K
        # a label exchange: the same key exactly when an automorphism of the graph undoes it
        u, v = rng.sample(range(n), 2)
        swapped = list(labels)
        swapped[u], swapped[v] = labels[v], labels[u]
        again = llaw.same_labelled_graph(code, n, labels, swapped)
        assert (llaw.key_of(code, n, swapped) == K) == again, (n, code, labels, u, v)
        assert (host_labelled(code, n, swapped, rooted=False)[0] == key) == again
        differ, same = differ + (not again), same + (again and labels[u] != labels[v])
        # item 6: equal (label, rooted code) exactly inside an orbit of the label-preserving automorphisms
        orbit = llaw.automorphism_orbits(code, n, labels)
        pairs = list(zip(labels, rooted))
        assert all((pairs[a] == pairs[b]) == (orbit[a] == orbit[b]) for a in range(n) for b in range(a)), (n, code, labels)
        assert min(r for r, l in zip(rooted, labels) if l == max(labels)) == canon
        idx = llaw.local_indices(labels, rooted)
        assert idx == llaw.local_indices_many([labels], [rooted])[0].tolist() and sorted(set(idx)) == list(range(len(set(orbit))))
        split += len(set(orbit)) > len(set(llaw.automorphism_orbits(code, n, [0] * n)))
    assert differ > cases // 4 and split > cases // 10 and (n == 8 or same > 0)


def test_decode_labelled_round_trips():
    from ugs_sampler import graphlets
    assert graphlets.LABEL_BITS == llaw.LABEL_BITS == 12
    rng = random.Random(9)
    rows, want = [], []
    for _ in range(300):
        n = rng.randrange(1, 9)
        code = rng.getrandbits(n * (n - 1) // 2) if n > 1 else 0
        labels = sorted(rng.choice([0, 1, 4095, rng.randrange(4096)]) for _ in range(n))
        rows.append(llaw.key_words(llaw.key_number(n, code, labels)))
        want.append((n, code, labels + [-1] * (8 - n)))
    rows.append((-1, -1))
    want.append((0, -1, [-1] * 8))
    key = torch.tensor(rows, dtype=torch.int64)
    assert bool((key[:, 0] < 0).any()) and bool((key[:, 0] > 0).any())            # n = 8 is negative as int64
    n, code, labels = graphlets.decode_labelled(key)
    assert n.dtype == code.dtype == labels.dtype == torch.int64 and tuple(labels.shape) == (301, 8)
    assert list(zip(n.tolist(), code.tolist(), labels.tolist())) == want
    n2, code2, labels2 = graphlets.decode_labelled(key.view(7, 43, 2))
    assert tuple(n2.shape) == (7, 43) and tuple(labels2.shape) == (7, 43, 8) and torch.equal(labels2.view(301, 8), labels)
    for c, nn, lab in ((0b101, 3, [7, 7, 9]), (law.code_of_edges(8, [(i, j) for i, j in law.pairs(8)]), 8, [4095] * 8)):
        words, _ = host_labelled(c, nn, lab, rooted=False)                       # the library's key through the decoder
        got = graphlets.decode_labelled(torch.tensor(words, dtype=torch.int64))
        assert (int(got[0]), int(got[1]), got[2].tolist()[:nn]) == (nn, llaw.labelled_codes(c, nn, tuple(lab))[0], sorted(lab))
    with pytest.raises(TypeError):
        graphlets.decode_labelled(key.to(torch.int32))
    with pytest.raises(ValueError):
        graphlets.decode_labelled(key.view(-1))


def test_compact_labels():
    from ugs_sampler import graphlets
    alphabet = torch.tensor([-5, 1, 6, 7, 8, 16, 2 ** 40], dtype=torch.int64)
    raw = torch.tensor([[6, 1, 2 ** 40], [-5, 0, 9], [2 ** 41, -6, 16]], dtype=torch.int64)
    got = graphlets.compact_labels(raw, alphabet)
    assert got.dtype == torch.int64 and got.tolist() == [[2, 1, 6], [0, -1, -1], [-1, -1, 5]]
    assert graphlets.compact_labels(raw[:0], alphabet).shape == (0, 3)
    assert graphlets.compact_labels(raw, alphabet[:0]).tolist() == [[-1] * 3] * 3
    full = torch.arange(4096, dtype=torch.int64) * 3
    assert graphlets.compact_labels(torch.tensor([0, 3, 4, 12285]), full).tolist() == [0, 1, -1, 4095]
    with pytest.raises(ValueError, match="4096"):
        graphlets.compact_labels(raw, torch.arange(4097, dtype=torch.int64))
    with pytest.raises(TypeError):
        graphlets.compact_labels(raw.to(torch.int32), alphabet)
    with pytest.raises(TypeError):
        graphlets.compact_labels(raw, alphabet.tolist())
    with pytest.raises(ValueError):
        graphlets.compact_labels(raw, alphabet.view(1, -1))


def test_refusals():
    from ugs_sampler import graphlets
    from ugs_sampler._lib import lib
    lab, key, out = (C.c_int32 * 8)(), (C.c_int64 * 2)(5, 5), (C.c_uint32 * 8)()
    assert lib.ugs_graphlet_labelled_code(0, 0, lab, key, out) == UGS_E_UNSUPPORTED
    assert lib.ugs_graphlet_labelled_code(0, 9, lab, key, out) == UGS_E_UNSUPPORTED
    assert lib.ugs_graphlet_labelled_code(0, 3, None, key, out) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_labelled_code(0, 3, lab, None, out) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_labelled_code(8, 3, lab, key, out) == UGS_E_BAD_ARG           # a bit above n (n - 1) / 2
    for bad in (-1, 4096):
        lab[2] = bad
        assert lib.ugs_graphlet_labelled_code(0, 3, lab, key, out) == UGS_E_BAD_ARG
        assert lib.ugs_graphlet_labelled_code(0, 2, lab, key, out) == 0                   # entries from n on are not read
    assert lib.ugs_graphlet_labelled(None, None, 0, 0, None, 0, 9, None, 0, None, None, None) == UGS_E_UNSUPPORTED
    assert lib.ugs_graphlet_labelled(None, None, 0, 0, None, 0, 0, None, 0, None, None, None) == UGS_E_UNSUPPORTED
    assert lib.ugs_graphlet_labelled(None, None, 0, 0, None, -1, 3, None, 0, None, None, None) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_labelled(None, None, 0, 0, None, 0, 3, None, -1, None, None, None) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_labelled(None, None, 0, 0, None, 0, 3, None, 5, None, None, None) == UGS_E_BAD_ARG
    assert lib.ugs_graphlet_labelled(None, None, 0, 0, None, 0, 3, None, 0, None, None, None) == 0      # no rows: a no-op

    nodes, ei, ep = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 0), dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    labels = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError):
        graphlets.labelled_keys(nodes, ei, ep, None)
    with pytest.raises(TypeError):
        graphlets.labelled_keys(nodes, ei, ep, labels.to(torch.int32))
    with pytest.raises(TypeError):
        graphlets.labelled_keys(nodes, ei, ep, labels.tolist())
    with pytest.raises(ValueError):
        graphlets.labelled_keys(nodes, ei, ep, labels.view(2, 2))
    with pytest.raises(ValueError):
        graphlets.labelled_keys(nodes, ei, ep[:2], labels)
    with pytest.raises(TypeError):
        graphlets.labelled_keys(nodes.to(torch.int32), ei, ep, labels)


def test_the_vocabulary_functions_take_the_keys():
    """hexdigests, extend_vocab and WLVocab's table on keys of every n, n = 8 included, whose high word is negative as int64."""
    from ugs_sampler import wl
    rng = random.Random(31)
    numbers = []
    for n in range(1, 9):
        for _ in range(6):
            code, labels = random_labelled(rng, n)
            numbers.append(llaw.key_of(code, n, labels))
    numbers += numbers[:5]                                                       # repeats get no new id
    key = torch.tensor([llaw.key_words(K) for K in numbers], dtype=torch.int64)
    status = torch.zeros(len(numbers), dtype=torch.int32)
    status[3] = 3
    hexes = wl.hexdigests(key, status)
    assert hexes[3] is None and all(h == "%032x" % K for h, K in zip(hexes, numbers) if h is not None)
    vocab = wl.extend_vocab({}, key, status)
    seen = []
    for i, K in enumerate(numbers):
        if i != 3 and K not in seen:
            seen.append(K)
    assert vocab == {"%032x" % K: i for i, K in enumerate(seen)}
    table = wl.WLVocab(vocab, "cuda:0")
    assert len(table) == len(seen) and not table.host_only
    order = sorted(range(len(seen)), key=lambda i: seen[i])
    assert table.key_ids.tolist() == order
    assert [(int(h) << 64) | int(l) for h, l in table.keys] == [seen[i] for i in order]
    assert any(K >> 127 for K in seen)
