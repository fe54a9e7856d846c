"""The WL-hash law (tests/wl_law.py, stated at ugs_wl_hash in include/ugs_mi355.h) against the reference's recorded results
(tests/golden/f19_wl_reference, made by tools/make_golden_wl.py) and against networkx itself, plus the host-side pieces of
ugs_sampler.wl.  No GPU and no library call."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import wl_law

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f19_wl_reference")
HEX32 = re.compile(r"[0-9a-f]{32}\Z")


def fixture():
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    return meta, np.load(GOLDEN + ".npz")


def test_law_equals_the_reference_row_for_row():
    meta, z = fixture()
    assert {s["k"] for s in meta["scenarios"]} >= {4, 6, 8} and {s["iterations"] for s in meta["scenarios"]} >= {1, 3}
    for i, s in enumerate(meta["scenarios"]):
        hexes, stats, _ = wl_law.wl_rows(z["s%d_nodes" % i], z["s%d_edge_index" % i], z["s%d_edge_ptr" % i], s["iterations"])
        for r, (want, got, st) in enumerate(zip(s["hashes"], hexes, stats)):
            if want is None:
                assert st == wl_law.STATUS_EMPTY and got is None, (s["name"], r)
            elif HEX32.match(want):
                assert st == wl_law.STATUS_OK and got == want, (s["name"], r)
            else:                                   # the reference's fallback string: the documented deviation
                assert s["deviation"] and st == wl_law.STATUS_BAD_ENDPOINT and got is None, (s["name"], r)
        if not s["deviation"]:
            vocab = {h: j for j, h in enumerate(s["vocab"])}
            assert wl_law.ids_from(hexes, stats, vocab) == z["s%d_ids" % i].tolist(), s["name"]
    assert any(s["deviation"] for s in meta["scenarios"])


def random_graph(rng, n):
    """(n, [(u, v), ...]) with loops, duplicate and reversed entries; dense ones reach degrees >= 10."""
    p = rng.choice([0.0, 0.1, 0.3, 0.6, 1.0])
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    es += [(v, u) for u, v in es if rng.random() < 0.5]
    es += [rng.choice(es) for _ in range(rng.randrange(3))] if es else []
    es += [(u, u) for u in range(n) if rng.random() < 0.15]
    rng.shuffle(es)
    return n, es


def test_law_equals_networkx_on_random_graphs():
    nx = pytest.importorskip("networkx")
    pinned = fixture()[0]["networkx"]
    if nx.__version__ != pinned:
        pytest.skip(f"networkx {nx.__version__} is installed, the law is pinned to {pinned}")
    rng = random.Random(19)
    big_degree = 0
    for trial in range(240):
        n, es = random_graph(rng, rng.randrange(1, 33) if trial % 3 else 32)
        it = (0, 1, 3, 8)[trial % 4]
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(es)
        for u in range(n):
            G.nodes[u]["attr"] = str(G.degree(u))
        big_degree += max(d for _, d in G.degree()) >= 10
        want = nx.weisfeiler_lehman_graph_hash(G, node_attr="attr", iterations=it)
        got, st, _, _ = wl_law.wl_row(list(range(n)), [a for a, _ in es], [b for _, b in es], it)
        assert st == 0 and got == want, (trial, n, it)
    assert big_degree >= 20


def test_text_of_the_empty_and_the_one_item_tuple():
    assert wl_law.final_text([]) == "()" == str(tuple([]))
    one = [("0123456789abcdef0123456789abcdef", 2)]
    assert wl_law.final_text(one) == "(('0123456789abcdef0123456789abcdef', 2),)" == str(tuple(one))
    two = one + [("f" * 32, 11)]
    assert wl_law.final_text(two) == str(tuple(two))
    hx, st, lens, flen = wl_law.wl_row([5, -1, -1], [], [], 0)
    assert st == 0 and flen == 2 and lens == [] and hx == wl_law._h("()")
    hx, st, lens, flen = wl_law.wl_row([5, 6, -1], [0, 1], [1, 0], 1)            # two vertices with one label: a single item
    assert st == 0 and flen == len("(('', 2),)") + 32 and lens == [[2, 2]]


def tensors(hexes, stats):
    words = [wl_law.digest_words(h) if h else (0, 0) for h in hexes]
    return torch.tensor(words, dtype=torch.int64).reshape(-1, 2), torch.tensor(stats, dtype=torch.int32)


def test_hexdigests_and_extend_vocab_id_order():
    from ugs_sampler.wl import extend_vocab, hexdigests
    a, b, c = "00" * 16, "ff" * 15 + "fe", "80" + "0" * 29 + "1"       # high bit set: the int64 words are negative
    hexes = [b, None, a, b, None, c, a]
    stats = [0, 1, 0, 0, 2, 0, 0]
    d, s = tensors(hexes, stats)
    assert hexdigests(d, s) == hexes
    vocab = {"x" * 32: 0}
    assert extend_vocab(vocab, d, s) is vocab
    assert vocab == {"x" * 32: 0, b: 1, a: 2, c: 3}
    assert extend_vocab(vocab, d, s) == {"x" * 32: 0, b: 1, a: 2, c: 3}      # nothing new, nothing renumbered
    meta, z = fixture()                                # the reference's first-seen rule on a fixture scenario
    s0 = next(s for s in meta["scenarios"] if s["name"] == "tu_k8_it3")
    half = (s0["rows"] + 1) // 2
    d, s = tensors(s0["hashes"][:half], [0 if h else 1 for h in s0["hashes"][:half]])
    assert list(extend_vocab({}, d, s)) == s0["vocab"]


def test_vocab_keeps_keys_that_are_no_digests_on_the_host():
    from ugs_sampler.wl import WLVocab
    a, b, c = "0" * 31 + "1", "f" * 32, "8" + "0" * 31
    src = {"deg_4_edges_2": 0, b: 1, a: 2, "A" * 32: 3, c: 4, "abc": 5}
    v = WLVocab(src, "cuda:0")
    assert len(v) == 6 and v.to_dict() == src and v.to_dict() is not src
    assert v.host_only == {"deg_4_edges_2": 0, "A" * 32: 3, "abc": 5}
    assert v.keys.dtype == np.uint64 and v.keys.tolist() == [[0, 1], [8 << 60, 0], [2 ** 64 - 1, 2 ** 64 - 1]]      # ascending, unsigned
    assert v.key_ids.tolist() == [2, 4, 1]
    empty = WLVocab({}, "cuda:0")
    assert len(empty) == 0 and empty.keys.shape == (0, 2)
    with pytest.raises(ValueError):
        WLVocab({}, "cpu")
