"""graphlets.labelled_keys on the GPU (ugs_graphlet_labelled_kernel, both forms) against the brute-force law of
tests/graphlet_labelled_law.py, never against the kernel's own search: keys and rooted codes over the label-monotone subset of all n!
permutations.  The exhaustive and the symmetric runs brute-force each labelled graph once and carry the result to a relabelled row
by equivariance -- the key does not change and the vertex renamed perm[v] has v's orbit -- which tests/test_graphlet_labelled_law.py
checks of the law itself.  The constant-label runs compare with `canonical` and `orbit_ids`, pinned by their own tests."""
import random

import numpy as np
import pytest
import torch

import graphlet_law as law
import graphlet_labelled_law as llaw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MASK = (1 << 28) - 1
N_LABELS = 64                                            # the label vector of the mixed rows
NO_LABEL, WIDE_LABEL = 60, 61                            # ids whose labels are -1 and 4096
GOOD_IDS = [3, 5, 5, 40, 41, 17, 0, 59]
BAD_IDS = [N_LABELS, 10 ** 12, NO_LABEL, WIDE_LABEL]


def mixed_labels(rng):
    labels = [rng.choice([0, 1, 1, 2, 4095]) for _ in range(N_LABELS)]
    labels[NO_LABEL], labels[WIDE_LABEL] = -1, 4096
    return np.array(labels, np.int64)


def pack(entries, k):
    """(nodes [S, k], edge_index [2, E], edge_ptr [S+1]) from a list of (node entries of length k, [(u, v), ...])."""
    nodes = np.array([e[0] for e in entries], np.int64).reshape(len(entries), k)
    cols, ptr = [], [0]
    for _, es in entries:
        cols += list(es)
        ptr.append(len(cols))
    ei = np.array(cols, np.int64).reshape(-1, 2).T if cols else np.zeros((2, 0), np.int64)
    return nodes, np.ascontiguousarray(ei), np.array(ptr, np.int64)


def random_entry(rng, n, k, bad=False, bad_label=False):
    """A row with n vertices in k slots: entries of -1 anywhere, the middle included, ids that repeat; edges of mixed density with
    reversed copies, duplicates and loops; with `bad`, one endpoint outside the row's vertices; with `bad_label`, one entry past the
    label vector or with a label of -1 or 4096."""
    slots = sorted(rng.sample(range(k), n))
    ids = [rng.choice(GOOD_IDS) for _ in range(n)]                               # a repeated id is two vertices with one label
    if bad_label and n:
        ids[rng.randrange(n)] = rng.choice(BAD_IDS)
    row = [-1] * k
    for s, x in zip(slots, ids):
        row[s] = x
    p = rng.choice([0.0, 0.15, 0.4, 0.7, 1.0])
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    es += [(v, u) for u, v in es if rng.random() < 0.6]
    es += [rng.choice(es) for _ in range(rng.randrange(3))] if es else []
    es += [(u, u) for u in range(n) if rng.random() < 0.1]
    if bad:
        es.append(rng.choice([(0, n), (-1, 0), (n + 3, n + 3)]))
    rng.shuffle(es)
    return row, es


def mixed_rows(rng, k, rows=40):
    entries = [random_entry(rng, 0, k), random_entry(rng, k, k), random_entry(rng, rng.randrange(1, k + 1), k, bad=True),
               random_entry(rng, k, k, bad=True, bad_label=True)]                # status 2 whatever its labels
    entries += [random_entry(rng, rng.randrange(1, k + 1), k, bad_label=True) for _ in range(4)]
    for x in BAD_IDS:                                                            # each kind of bad label, in the last vertex's slot
        row, es = random_entry(rng, k, k)
        entries.append((row[:-1] + [x], es))
    if k >= 3:                                                                   # the slot rule: -1 in the middle, vertices around it
        row, es = random_entry(rng, k - 1, k - 1)
        entries.append((row[:1] + [-1] + row[1:], es + [(0, k - 2), (k - 2, 1)]))
    while len(entries) < rows:
        n = k if rng.random() < 0.5 else rng.randrange(1, k + 1)                 # rows whose valid entries are fewer than k
        entries.append(random_entry(rng, n, k, bad=rng.random() < 0.08, bad_label=rng.random() < 0.08))
    rng.shuffle(entries)
    return entries[:rows]


def on_gpu(arrays, strided=False):
    nodes, ei, ep = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)
    if strided:                                                                 # rows 0 and 2 of a [3, E + 5] buffer: row stride 2 E + 10
        buf = torch.full((3, ei.size(1) + 5), -7, dtype=torch.int64, device=DEV)
        buf[0, :ei.size(1)], buf[2, :ei.size(1)] = ei[0], ei[1]
        ei = buf[::2, :ei.size(1)]
        assert not ei.is_contiguous() or ei.size(1) == 0
    return nodes, ei, ep


def assert_rows(arrays, labels, want_words, want_status, want_local, what, strided=False):
    """labelled_keys of the rows on the GPU, without and with the orbits, against the given words [S][2], statuses and [S][k]."""
    from ugs_sampler import graphlets
    args = on_gpu(arrays, strided) + (torch.from_numpy(np.ascontiguousarray(labels)).to(DEV),)
    S, k = args[0].shape
    key, status = graphlets.labelled_keys(*args)
    assert key.is_cuda and key.dtype == torch.int64 and tuple(key.shape) == (S, 2), what
    assert status.is_cuda and status.dtype == torch.int32 and tuple(status.shape) == (S,), what
    got_key, got_status = key.cpu().tolist(), status.cpu().tolist()
    bad = [r for r in range(S) if got_status[r] != want_status[r] or got_key[r] != list(want_words[r])]
    assert not bad, (what, bad[:5], [(got_status[r], got_key[r]) for r in bad[:3]], [(want_status[r], list(want_words[r])) for r in bad[:3]])
    three = graphlets.labelled_keys(*args, return_orbits=True)
    assert isinstance(three, tuple) and len(three) == 3, what
    assert torch.equal(three[0], key) and torch.equal(three[1], status), what    # the orbit form writes the same keys
    orbit = three[2]
    assert orbit.is_cuda and orbit.dtype == torch.int64 and tuple(orbit.shape) == (S, k), what
    got = orbit.cpu().tolist()
    bad = [r for r in range(S) if got[r] != list(want_local[r])]
    assert not bad, (what, bad[:5], [got[r] for r in bad[:3]], [list(want_local[r]) for r in bad[:3]])
    return key, status, orbit


def assert_law(arrays, labels, what, strided=False, num_cols=None):
    keys, stats, local = llaw.rows_law(*arrays, labels, num_cols=num_cols)
    assert_rows(arrays, labels, [llaw.key_words(K) for K in keys], stats, local, what, strided)
    k = arrays[0].shape[1]
    assert all((x == k) == (int(e) < 0 or st != 0) for row, ent, st in zip(local, arrays[0], stats) for x, e in zip(row, ent)), what
    return keys, stats, local


@pytest.mark.parametrize("k", range(1, 9))
def test_every_k(k):
    rng = random.Random(7000 + k)
    labels = mixed_labels(rng)
    nodes, ei, ep = pack(mixed_rows(rng, k), k)
    keys, stats, local = assert_law((nodes, ei, ep), labels, f"k={k}")
    assert_law((nodes, ei, ep), labels, f"k={k} strided", strided=True)
    assert {0, 1, 2, 3} <= set(stats) and (k == 1 or len(set(keys)) > 5)
    seen = {int(x) for row, st in zip(nodes, stats) if st == 3 for x in row}     # every kind of bad label made a status 3
    assert seen >= set(BAD_IDS)
    # an edge_ptr range that is no range of the columns: rows 10 and 11 lose theirs, the rows around them keep their results
    ep2 = ep.copy()
    ep2[11] = -1
    keys2, stats2, local2 = assert_law((nodes, ei, ep2), labels, f"k={k} bad range")
    assert all(s == 2 or not (nodes[r] >= 0).any() for r, s in zip((10, 11), stats2[10:12]))
    assert keys2[:10] == keys[:10] and keys2[12:] == keys[12:] and local2[:10] == local[:10] and local2[12:] == local[12:]
    ep3 = ep.copy()
    ep3[-1] += 2                                                                 # the last row ends past the columns
    assert_law((nodes, ei, ep3), labels, f"k={k} range past the columns")


@pytest.mark.parametrize("k", [6, 8])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 257])
def test_launch_shapes(rows, k):
    """One row (seven groups of its wave missing); a workgroup of 32 rows one short, full and one over; 257 rows."""
    rng = random.Random(100 * k + rows + 5)
    labels = mixed_labels(rng)
    pool = mixed_rows(rng, k, rows=12)                                           # few graphs, so that the brute force stays short
    entries = [pool[rng.randrange(12)] for _ in range(rows)]
    assert_law(pack(entries, k), labels, f"rows={rows}")
    assert_law(pack(entries, k), labels, f"rows={rows} strided", strided=True)


def test_slot_rule_and_repeated_ids():
    """The paw on slots 0, 2, 3, 5 of six: the answers are those of vertices 0 .. 3 in row order whatever stands in the slots, and a
    repeated id is two vertices with one label."""
    paw = [(0, 1), (1, 2), (2, 0), (2, 3)]                                       # triangle 0 1 2, tail 3 at 2
    labels = np.array([0, 5, 5, 9, 2], np.int64)
    rows = [([1, -1, 1, 3, -1, 1], paw), ([2, 2, 3, 1, -1, -1], paw), ([-1, -1, 1, 2, 3, 1], paw), ([1, -1, 1, 3, -1, 4], paw)]
    keys, stats, local = assert_law(pack(rows, 6), labels, "slot rule")
    assert stats == [0] * 4 and len(set(keys[:3])) == 1 and keys[3] != keys[0]
    # labels 5 5 9 5: tail (5), the two plain corners (5), the corner with the tail (9)
    assert local[:3] == [[1, 6, 1, 2, 6, 0], [1, 1, 2, 0, 6, 6], [6, 6, 1, 1, 2, 0]]
    assert local[3] == [1, 6, 1, 2, 6, 0]                                        # labels 5 5 9 2: the tail's label comes first


def relabelled_rows(codes, n, rng):
    """Rows for the graphs with adjacency codes `codes` on n vertices, every one relabelled by a random permutation (vertex v is
    renamed perm[v]), its entries in random orientations and order.  Row r's entries are the ids r n .. r n + n - 1.  Returns the
    arrays and perm [R, n]."""
    codes = np.asarray(codes, np.int64)
    R = len(codes)
    pr = np.array(law.pairs(n), np.int64).reshape(-1, 2)
    bits = ((codes[:, None] >> (pr[:, 1] * (pr[:, 1] - 1) // 2 + pr[:, 0])[None, :]) & 1).astype(bool)
    perm = np.argsort(rng.random((R, n)), axis=1)
    u, v = perm[:, pr[:, 0]], perm[:, pr[:, 1]]
    flip = rng.random(u.shape) < 0.5
    u, v = np.where(flip, v, u), np.where(flip, u, v)
    order = np.argsort(rng.random(u.shape), axis=1)
    u, v, bits = (np.take_along_axis(a, order, 1) for a in (u, v, bits))
    nodes = np.arange(R * n, dtype=np.int64).reshape(R, n)
    ptr = np.concatenate([[0], np.cumsum(bits.sum(axis=1))]).astype(np.int64)
    return (nodes, np.stack([u[bits], v[bits]]).astype(np.int64), ptr), perm


def assert_relabelled(codes, labels, n, canon, rooted, rng, what, spot=20):
    """The graphs `codes` with vertex labels `labels` [R, n], whose law is (canon [R], rooted [R, n]), as relabelled rows."""
    codes, labels = np.asarray(codes, np.int64), np.asarray(labels, np.int64).reshape(len(codes), n)
    arrays, perm = relabelled_rows(codes, n, rng)
    node_labels = np.zeros(len(codes) * n, np.int64)
    np.put_along_axis(node_labels.reshape(len(codes), n), perm, labels, axis=1)  # slot perm[v] is vertex v
    local = llaw.local_indices_many(labels, rooted)
    want_local = np.zeros_like(local)
    np.put_along_axis(want_local, perm, local, axis=1)
    words = llaw.key_words_many(n, canon, labels)
    for r in rng.choice(len(codes), min(spot, len(codes)), replace=False):       # the row's own brute force
        lo, hi = arrays[2][r], arrays[2][r + 1]
        now = law.code_of_edges(n, zip(arrays[1][0][lo:hi].tolist(), arrays[1][1][lo:hi].tolist()))
        lab = tuple(node_labels[r * n:(r + 1) * n].tolist())
        c, rt = llaw.labelled_codes(now, n, lab)
        assert llaw.key_words(llaw.key_number(n, c, lab)) == tuple(words[r].tolist())
        assert llaw.local_indices(lab, rt) == want_local[r].tolist()
    return assert_rows(arrays, node_labels, words.tolist(), [0] * len(codes), want_local.tolist(), what)


@pytest.mark.parametrize("n,num_labels", [(1, 3), (2, 3), (3, 3), (4, 3), (5, 2)])
def test_every_graph_and_every_labelling(n, num_labels):
    """The exhaustive sets of the host test as rows under a random relabelling with shuffled, randomly oriented entries."""
    import itertools
    graphs = np.arange(1 << (n * (n - 1) // 2), dtype=np.int64)
    labellings = np.array(list(itertools.product(range(num_labels), repeat=n)), dtype=np.int64).reshape(-1, n)
    codes, labels = np.repeat(graphs, len(labellings)), np.tile(labellings, (len(graphs), 1))
    canon, rooted = llaw.labelled_codes_many(codes, labels, n)
    key, _, _ = assert_relabelled(codes, labels * 1365, n, canon, rooted, np.random.default_rng(20 + n), f"exhaustive n = {n}")
    assert len(set(map(tuple, key.cpu().tolist()))) == llaw.burnside_labelled(n, num_labels)


@pytest.mark.parametrize("n", [7, 8])
def test_every_class_with_constant_labels(n):
    """Every class of n vertices under a random relabelling, all labels equal: the code of `canonical`, the local index of
    `orbit_ids`."""
    from ugs_sampler import graphlets
    table = graphlets.table(n)
    first = law.NUM_CLASSES[n - 2]
    codes = (table[first:] & MASK).numpy()
    assert len(codes) == law.GRAPHS_ON[n - 1]
    arrays, _ = relabelled_rows(codes, n, np.random.default_rng(70 + n))
    args = on_gpu(arrays)
    node_labels = torch.full((len(codes) * n,), 1365, dtype=torch.int64, device=DEV)
    key, status, orbit = graphlets.labelled_keys(*args, node_labels, return_orbits=True)
    plain_key, plain_status = graphlets.canonical(*args)
    assert torch.equal(plain_key.cpu(), table[first:]) and not bool(status.any()) and not bool(plain_status.any())
    got_n, got_code, got_labels = graphlets.decode_labelled(key)
    assert torch.equal((got_n << 28) | got_code, plain_key) and bool((got_labels[:, :n] == 1365).all())
    assert bool((got_labels[:, n:] == -1).all())
    ids, cls = graphlets.orbit_ids(*args, return_class=True)
    assert torch.equal(orbit, ids - graphlets.orbit_base(n).to(DEV)[cls][:, None])
    assert torch.equal(graphlets.labelled_keys(*args, node_labels)[0], key)


def symmetric_graphs():
    c8 = [(i, (i + 1) % 8) for i in range(8)]
    allp = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    cube = [(a, a ^ d) for a in range(8) for d in (1, 2, 4) if a < a ^ d]
    k44 = [(i, 4 + j) for i in range(4) for j in range(4)]
    star, path = [(0, i) for i in range(1, 8)], [(i, i + 1) for i in range(7)]
    return {"K8": allp, "C8": c8, "cube": cube, "K4,4": k44, "K1,7": star, "P8": path}


def test_symmetric_graphs_with_three_labellings():
    """K8, C8, the cube, K4,4, K1,7 and P8 with constant labels, two labels and all labels distinct, in the identity order against
    the brute force and then five relabellings of each."""
    graphs = symmetric_graphs()
    rng = random.Random(18)
    distinct = rng.sample(range(4096), 8)
    labellings = {"constant": [9] * 8, "two": [4, 4, 4, 7, 4, 7, 7, 4], "distinct": distinct}
    entries, node_labels, codes, labs = [], [], [], []
    for es in graphs.values():
        for lab in labellings.values():
            entries.append((list(range(len(node_labels), len(node_labels) + 8)), es))
            node_labels += lab
            codes.append(law.code_of_edges(8, es))
            labs.append(lab)
    arrays, node_labels = pack(entries, 8), np.array(node_labels, np.int64)
    keys, stats, local = assert_law(arrays, node_labels, "symmetric graphs, identity order")
    assert stats == [0] * 18 and len(set(keys)) == 18
    rank = {x: i for i, x in enumerate(sorted(distinct))}
    for g, es in enumerate(graphs.values()):
        n, code, sorted_labels = llaw.decode(keys[3 * g + 2])                    # all labels distinct: one monotone order
        assert code == law.code_of_edges(8, [(rank[distinct[u]], rank[distinct[v]]) for u, v in es])
        assert local[3 * g + 2] == [rank[x] for x in distinct] and sorted_labels == sorted(distinct)
        assert llaw.decode(keys[3 * g])[1] == law.key_of(codes[3 * g], 8) & MASK  # constant labels: the canonical code
    assert [len(set(local[3 * g])) for g in range(6)] == [1, 1, 1, 1, 2, 4]
    assert [len(set(local[3 * g + 1])) for g in range(6)] == [2] + [len(set(llaw.automorphism_orbits(codes[3 * g], 8, labs[1])))
                                                                    for g in range(1, 6)]
    canon_rooted = [llaw.labelled_codes(c, 8, tuple(lab)) for c, lab in zip(codes, labs)]
    assert_relabelled(np.repeat(codes, 5), np.repeat(labs, 5, axis=0), 8, np.repeat([c for c, _ in canon_rooted], 5),
                      np.repeat([r for _, r in canon_rooted], 5, axis=0), np.random.default_rng(8), "symmetric graphs relabelled")


def test_cubes_in_one_launch_and_one_cube_among_paths():
    """256 rows that are all cubes with two labels (every searching lane of four waves in the long search) and one such cube among
    255 paths (long lanes in a wave of short ones)."""
    graphs = symmetric_graphs()
    cube, p8 = law.code_of_edges(8, graphs["cube"]), law.code_of_edges(8, graphs["P8"])
    lab_cube, lab_path = (3, 3, 3, 3, 8, 8, 8, 8), (3, 8, 3, 8, 3, 8, 3, 8)       # a face of the cube against the opposite one
    law_of = {cube: llaw.labelled_codes(cube, 8, lab_cube), p8: llaw.labelled_codes(p8, 8, lab_path)}
    assert len(set(llaw.automorphism_orbits(cube, 8, lab_cube))) == 2
    rng = np.random.default_rng(81)
    for what, codes in (("256 x cube", [cube] * 256), ("one cube among paths", [p8] * 101 + [cube] + [p8] * 154)):
        labs = [lab_cube if c == cube else lab_path for c in codes]
        _, _, orbit = assert_relabelled(codes, labs, 8, [law_of[c][0] for c in codes], [law_of[c][1] for c in codes], rng, what, spot=3)
        assert all(len(set(row)) == (2 if c == cube else 8) for row, c in zip(orbit.cpu().tolist(), codes))


def test_no_labels_no_rows_and_cpu_tensors():
    from ugs_sampler import graphlets
    rng = random.Random(12)
    labels = mixed_labels(rng)
    arrays = pack(mixed_rows(rng, 5), 5)
    keys, stats, local = assert_law(arrays, labels, "device tensors")
    words = [list(llaw.key_words(K)) for K in keys]
    # N = 0: a null label pointer; every row with a vertex that is not status 2 is status 3
    keys0, stats0, local0 = assert_law(arrays, labels[:0], "no labels")
    assert stats0 == [3 if s == 0 else s for s in stats] and set(keys0) == {-1}
    host = tuple(torch.from_numpy(a) for a in arrays) + (torch.from_numpy(labels),)
    key, status = graphlets.labelled_keys(*host)
    assert not key.is_cuda and not status.is_cuda and key.dtype == torch.int64 and status.dtype == torch.int32
    assert key.tolist() == words and status.tolist() == stats
    key, status, orbit = graphlets.labelled_keys(*host, device=DEV, return_orbits=True)
    assert not key.is_cuda and not status.is_cuda and not orbit.is_cuda
    assert key.tolist() == words and status.tolist() == stats and orbit.tolist() == local

    nodes, ei, ep = on_gpu(arrays)
    dev_labels = torch.from_numpy(labels).to(DEV)
    key, status = graphlets.labelled_keys(nodes[:0], ei, ep[:1], dev_labels)
    assert key.is_cuda and tuple(key.shape) == (0, 2) and status.dtype == torch.int32 and tuple(status.shape) == (0,)
    key, status, orbit = graphlets.labelled_keys(nodes[:0], ei, ep[:1], dev_labels, return_orbits=True)
    assert tuple(key.shape) == (0, 2) and tuple(orbit.shape) == (0, 5) and orbit.dtype == torch.int64
    nine = (torch.zeros((1, 9), dtype=torch.int64, device=DEV), ei, ep[:2], dev_labels)
    with pytest.raises(RuntimeError, match="k <= 8"):
        graphlets.labelled_keys(*nine)
    with pytest.raises(ValueError):
        graphlets.labelled_keys(nodes, ei, ep, dev_labels.cpu())
    with pytest.raises(ValueError):
        graphlets.labelled_keys(nodes, ei.cpu(), ep, dev_labels)
    assert_law(arrays, labels, "after the refusals")


def test_vocabulary_ids_on_the_device():
    """WLVocab.lookup of the keys: the id of every row is the rank of its key among the law's keys, len(vocab) without one."""
    from ugs_sampler import graphlets, wl
    rng = random.Random(66)
    labels = mixed_labels(rng)
    arrays = pack(mixed_rows(rng, 8, rows=60), 8)
    keys, stats, _ = llaw.rows_law(*arrays, labels)
    known = sorted({K for K in keys if K >= 0})
    assert any(K >> 127 for K in known)                                          # n = 8: a negative high word
    held_out = known[len(known) // 2]                                            # one class the vocabulary has not seen
    vocab = {"%032x" % K: i for i, K in enumerate(K for K in known if K != held_out)}
    want = [vocab.get("%032x" % K, len(vocab)) if K >= 0 else len(vocab) for K in keys]
    args = on_gpu(arrays) + (torch.from_numpy(labels).to(DEV),)
    key, status = graphlets.labelled_keys(*args)
    ids = wl.WLVocab(vocab, DEV).lookup(key, status)
    assert ids.is_cuda and ids.tolist() == want and len(vocab) in want and 0 in want
    grown = wl.extend_vocab({}, key, status)                                     # the dataset pass of the docstring
    assert sorted(int(h, 16) for h in grown) == known
    assert wl.WLVocab(grown, DEV).lookup(key, status).tolist() == [grown.get("%032x" % K, len(grown)) if K >= 0 else len(grown) for K in keys]


def test_the_unlabelled_outputs_are_left_alone():
    from ugs_sampler import graphlets
    rng = random.Random(77)
    labels = torch.from_numpy(mixed_labels(rng)).to(DEV)
    for k in (3, 6, 8):
        args = on_gpu(pack(mixed_rows(rng, k, rows=70), k))
        before = (graphlets.class_ids(*args).clone(), *(t.clone() for t in graphlets.canonical(*args)), graphlets.orbit_ids(*args).clone())
        key, status, orbit = graphlets.labelled_keys(*args, labels, return_orbits=True)
        graphlets.labelled_keys(*args, labels)
        after = (graphlets.class_ids(*args), *graphlets.canonical(*args), graphlets.orbit_ids(*args))
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        ok = status == 0
        n, code, _ = graphlets.decode_labelled(key)
        assert torch.equal(n[ok], before[1][ok] >> 28) and bool((before[2][ok] == 0).all())     # the same vertices, another class
        assert bool(((status == 3) == ((before[2] == 0) & ~ok)).all()) and bool((orbit[~ok] == k).all())
