"""The node-feature WL law (tests/wl_feature_law.py, stated at ugs_wl_hash_labeled in include/ugs_mi355.h) against the
reference's recorded results (tests/golden/f20_wl_feature_reference, made by tools/make_golden_wl_features.py) and against the
reference's path through networkx itself.  No GPU and no library call."""
import hashlib
import json
import os
import random
import re

import numpy as np
import pytest

import wl_feature_law as law

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f20_wl_feature_reference")
HEX32 = re.compile(r"[0-9a-f]{32}\Z")


def fixture():
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    return meta, np.load(GOLDEN + ".npz")


def test_fixture_covers_the_stated_scenarios():
    meta, z = fixture()
    sc = meta["scenarios"]
    assert {s["k"] for s in sc} >= {4, 6, 8, 16} and {s["iterations"] for s in sc} >= {1, 3}
    assert {tuple(s["x_shape"][1:]) for s in sc if s["x_dtype"] == "float32"} >= {(3,), (7,), (18,)}
    assert {s["x_dtype"] for s in sc} >= {"float32", "float64", "int64"}
    assert os.path.getsize(GOLDEN + ".npz") + os.path.getsize(GOLDEN + ".json") < 100_000
    i = next(i for i, s in enumerate(sc) if s["name"] == "hand_made_it1")
    nodes = z["s%d_nodes" % i]
    assert any((row[:-1] < 0).any() and row[np.argmax(row < 0):].max() >= 0 for row in nodes if (row >= 0).any())      # an interior -1
    assert any(len(set(row.tolist())) == 1 and row[0] >= 0 for row in nodes)                                            # one id k times
    counts = (nodes >= 0).sum(axis=1)
    assert 0 in counts and 1 in counts
    _, _, reports = law.wl_feature_rows(nodes, z["s%d_edge_index" % i], z["s%d_edge_ptr" % i], law.labels_of(z["s%d_x" % i]), 1)
    assert 128 in {x for lens, _ in reports for per_it in lens for x in per_it}                                         # degree 15 at k = 16


def test_law_equals_the_reference_row_for_row():
    meta, z = fixture()
    for i, s in enumerate(meta["scenarios"]):
        x = z["s%d_x" % i]
        assert str(x.dtype) == s["x_dtype"] and list(x.shape) == s["x_shape"]
        hexes, stats, _ = law.wl_feature_rows(z["s%d_nodes" % i], z["s%d_edge_index" % i], z["s%d_edge_ptr" % i], law.labels_of(x), s["iterations"])
        for r, (want, got, st) in enumerate(zip(s["hashes"], hexes, stats)):
            if want is None:
                assert st == law.STATUS_EMPTY and got is None, (s["name"], r)
            elif HEX32.match(want):
                assert st == law.STATUS_OK and got == want, (s["name"], r)
            else:                                   # the reference's fallback string: the documented deviation
                assert s["deviation"] and st == law.STATUS_BAD_ENDPOINT and got is None, (s["name"], r)
        if not s["deviation"]:
            vocab = {h: j for j, h in enumerate(s["vocab"])}
            want_ids = [vocab.get(h, len(vocab)) if st == law.STATUS_OK else len(vocab) for h, st in zip(hexes, stats)]
            assert want_ids == z["s%d_ids" % i].tolist(), s["name"]
    assert any(s["deviation"] for s in meta["scenarios"])


def test_label32_is_the_head_of_the_md5_hexdigest():
    assert law.label32(b"") == 0xd41d8cd9
    assert law.label32(b"abc") == 0x90015098                                   # RFC 1321, appendix A.5
    x = np.eye(3, dtype=np.float32)
    assert law.labels_of(x) == [int(hashlib.md5(x[i].tobytes()).hexdigest()[:8], 16) for i in range(3)]
    assert sorted("%08x" % v for v in (0, 9, 10, 0xffffffff, 0xa0000000)) == ["%08x" % v for v in sorted((0, 9, 10, 0xffffffff, 0xa0000000))]


def test_statuses_and_their_precedence():
    labels = [1, 2, 3, 1 << 32, -1]
    row = law.wl_feature_row
    assert row([-1, -1, -1], [], [], labels)[1] == law.STATUS_EMPTY
    assert row([0, 1, -1], [0], [2], labels)[1] == law.STATUS_BAD_ENDPOINT
    assert row([0, 5, -1], [0], [2], labels)[1] == law.STATUS_BAD_ENDPOINT      # both faults: 2, not 3
    assert row([0, 5, -1], [0], [1], labels)[1] == law.STATUS_BAD_LABEL         # an id equal to the number of label rows
    assert row([0, 10 ** 12], [], [], labels)[1] == law.STATUS_BAD_LABEL
    assert row([0, 3], [], [], labels)[1] == law.STATUS_BAD_LABEL               # a label of 2^32
    assert row([4, 0], [], [], labels)[1] == law.STATUS_BAD_LABEL               # a negative label
    hx, st, lens, flen = row([2, -1, 0], [0], [1], labels, 1)
    assert st == law.STATUS_OK and lens == [[16, 16]] and HEX32.match(hx)
    assert row([2, -1, 0], [], [], labels, 0)[0] == law._h("()")


def random_case(rng):
    k = rng.randrange(1, 33)
    N = rng.randrange(1, 12)
    n = rng.randrange(1, k + 1)
    slots = sorted(rng.sample(range(k), n))
    row = [-1] * k
    for s in slots:
        row[s] = rng.randrange(N)                                              # duplicate ids happen
    p = rng.choice([0.0, 0.2, 0.5, 1.0])
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    es += [(v, u) for u, v in es if rng.random() < 0.5]
    es += [(u, u) for u in range(n) if rng.random() < 0.15]
    rng.shuffle(es)
    return row, es, N


def test_law_equals_the_reference_path_through_networkx_on_random_rows():
    nx = pytest.importorskip("networkx")
    pinned = fixture()[0]["networkx"]
    if nx.__version__ != pinned:
        pytest.skip(f"networkx {nx.__version__} is installed, the law is pinned to {pinned}")
    rng = random.Random(20)
    nprng = np.random.default_rng(20)
    interior = 0
    for trial in range(300):
        row, es, N = random_case(rng)
        it = (0, 1, 3, 4)[trial % 4]
        dtype, F = ((np.float32, 3), (np.float64, 2), (np.int64, 9), (np.uint8, 13), (np.float32, 18))[trial % 5]
        x = (nprng.integers(0, 2, (N, F)) * nprng.integers(1, 3, (N, 1))).astype(dtype)
        valid = [v for v in row if v >= 0]                                     # subgraph_nodes[valid_mask], wl_vocab.py:91-103
        interior += any(v < 0 for v in row[:max(i for i, v in enumerate(row) if v >= 0)])
        G = nx.Graph()
        G.add_nodes_from(range(len(valid)))
        G.add_edges_from(es)
        for j, v in enumerate(valid):
            G.nodes[j]["attr"] = hashlib.md5(x[v].tobytes()).hexdigest()[:8]   # wl_vocab.py:48-50
        want = nx.weisfeiler_lehman_graph_hash(G, node_attr="attr", iterations=it)
        got, st, _, _ = law.wl_feature_row(row, [a for a, _ in es], [b for _, b in es], law.labels_of(x), it)
        assert st == 0 and got == want, (trial, row, it)
    assert interior >= 50
