"""ugs_sampler.wl on the GPU (ugs_wl.hip) against the plain-Python law (tests/wl_law.py) and the reference's recorded results
(tests/golden/f19_wl_reference): digests, statuses and vocabulary ids, never against itself."""
import json
import os
import random

import numpy as np
import pytest
import torch

import wl_law

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f19_wl_reference")
DEV = "cuda:0"


def pack(entries, k):
    """(nodes [S, k], edge_index [2, E], edge_ptr [S+1]) as int64 arrays from a list of (n, [(u, v), ...]): n valid ids first."""
    nodes = np.full((len(entries), k), -1, np.int64)
    cols, ptr = [], [0]
    for r, (n, es) in enumerate(entries):
        nodes[r, :n] = 100 + np.arange(n)
        cols += list(es)
        ptr.append(len(cols))
    ei = np.array(cols, np.int64).reshape(-1, 2).T if cols else np.zeros((2, 0), np.int64)
    return nodes, np.ascontiguousarray(ei), np.array(ptr, np.int64)


def random_entry(rng, n):
    """Edges on vertices 0..n-1 of mixed density with reversed copies, duplicates and loops."""
    p = rng.choice([0.0, 0.15, 0.4, 0.7, 1.0])
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    es += [(v, u) for u, v in es if rng.random() < 0.6]
    es += [rng.choice(es) for _ in range(rng.randrange(3))] if es else []
    es += [(u, u) for u in range(n) if rng.random() < 0.1]
    rng.shuffle(es)
    return n, es


def mixed_rows(rng, k, rows=40):
    entries = [(0, []), (k, []), (rng.randrange(1, k + 1), [])]                 # all -1, no edges at full and at partial width
    while len(entries) < rows:
        n = k if rng.random() < 0.6 else rng.randrange(1, k + 1)               # rows whose valid entries are fewer than k
        entries.append(random_entry(rng, n))
    rng.shuffle(entries)
    return entries


def on_gpu(arrays, strided=False):
    nodes, ei, ep = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)
    if strided:                                                                 # rows 0 and 2 of a [3, E + 5] buffer: row stride 2 E + 10
        buf = torch.full((3, ei.size(1) + 5), -7, dtype=torch.int64, device=DEV)
        buf[0, :ei.size(1)], buf[2, :ei.size(1)] = ei[0], ei[1]
        ei = buf[::2, :ei.size(1)]
        assert not ei.is_contiguous() or ei.size(1) == 0
    return nodes, ei, ep


def assert_law(arrays, iterations, what, strided=False):
    from ugs_sampler import wl
    hexes, stats, _ = wl_law.wl_rows(*arrays, iterations)
    digest, status = wl.wl_hash(*on_gpu(arrays, strided), iterations)
    assert digest.is_cuda and digest.dtype == torch.int64 and tuple(digest.shape) == (len(hexes), 2)
    assert status.is_cuda and status.dtype == torch.int32 and tuple(status.shape) == (len(hexes),)
    assert status.cpu().tolist() == stats, what
    got = wl.hexdigests(digest, status)
    bad = [r for r, (a, b) in enumerate(zip(got, hexes)) if a != b]
    assert not bad, (what, bad[:5], [got[r] for r in bad[:2]], [hexes[r] for r in bad[:2]])
    assert not digest.cpu()[torch.tensor(stats) != 0].any(), what
    return hexes, stats


@pytest.mark.parametrize("k", range(1, 33))
def test_every_k(k):
    rng = random.Random(1000 + k)
    hexes, stats = assert_law(pack(mixed_rows(rng, k), k), 3, f"k={k}")
    assert 0 in stats and 1 in stats


def test_messages_of_exactly_one_and_two_blocks():
    """A vertex of degree 3 sends 32 + 3 * 32 = 128 bytes from iteration 2 on, one of degree 7 sends 256: the last block is the
    full block with the final flag.  The rows are chosen by the law's own length report."""
    both = lambda es: [e for u, v in es for e in ((u, v), (v, u))]                # noqa: E731
    entries = [(6, both([(0, 1), (0, 2), (0, 3), (1, 4), (1, 5)])),
               (8, both([(0, i) for i in range(1, 8)] + [(1, 2)])),
               (8, both([(0, i) for i in range(1, 8)]) + [(0, 0)]),               # degree 9 by a loop: 8 neighbour labels, 288 bytes
               (4, both([(0, 1), (0, 2), (0, 3)])),
               (12, both([(0, i) for i in range(1, 12)]))]                        # degree 11: 384 bytes, three full blocks
    for k, it in ((12, 3), (12, 2), (32, 3)):
        arrays = pack(entries, k)
        _, _, reports = wl_law.wl_rows(*arrays, it)
        lens = {x for msg_lens, _ in reports for per_it in msg_lens for x in per_it}
        assert {128, 256, 384} <= lens
        assert_law(arrays, it, f"block messages k={k} it={it}")


def boundary_entry(rng):
    """Sparse to dense graphs on 2..32 vertices: many distinct labels, so the final string runs over many blocks."""
    n = rng.randrange(2, 33)
    p = rng.choice([0.5, 1.0, 2.0, 4.0, 40.0]) / max(n - 1, 1)
    es = [(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < p]
    return n, es + [(v, u) for u, v in es]


def test_final_strings_at_block_boundaries():
    """Rows whose final string is an exact multiple of 128 bytes, and one byte either side, found in a fixed seed's stream of
    graphs hashed with 3 and with 8 iterations alternately (an item is 39 or 40 bytes: exact multiples are rare at 3)."""
    rng = random.Random(75)
    found = {}
    for i in range(800):
        n, es = entry = boundary_entry(rng)
        it = (3, 8)[i % 2]
        _, _, _, flen = wl_law.wl_row(list(range(n)), [a for a, _ in es], [b for _, b in es], it)
        if flen % 128 in (127, 0, 1) and len(found.setdefault((it, flen % 128), [])) < 3:
            found[it, flen % 128].append(entry)
    for residue in (127, 0, 1):
        assert any(r == residue for _, r in found), (residue, sorted(found))
    for it in (3, 8):
        entries = [e for (j, _), v in sorted(found.items()) if j == it for e in v]
        arrays = pack(entries, 32)
        _, _, reports = wl_law.wl_rows(*arrays, it)
        assert {flen % 128 for _, flen in reports} == {r for j, r in found if j == it} and entries
        assert_law(arrays, it, f"final string boundaries, iterations={it}")


@pytest.mark.parametrize("iterations", [0, 1, 2, 8])
def test_iterations(iterations):
    rng = random.Random(5)
    assert_law(pack(mixed_rows(rng, 7, rows=24), 7), iterations, f"iterations={iterations}")
    assert_law(pack(mixed_rows(rng, 20, rows=12), 20), iterations, f"iterations={iterations}, k=20")


@pytest.mark.parametrize("rows", [1, 7, 257])
def test_launch_shapes_and_row_stride(rows):
    rng = random.Random(rows)
    for k in (6, 11, 19):                              # 32, 16 and 8 rows per workgroup: 257 rows end one row into a new workgroup
        entries = mixed_rows(rng, k, rows=max(rows, 3))[:rows]
        assert_law(pack(entries, k), 3, f"rows={rows} k={k}")
        assert_law(pack(entries, k), 3, f"rows={rows} k={k} strided", strided=True)


def test_statuses_do_not_disturb_neighbouring_rows():
    rng = random.Random(3)
    good = [random_entry(rng, 5) for _ in range(6)]
    entries = [good[0], (3, [(0, 1), (1, 3)]), good[1], (5, [(0, 1), (-1, 2)]), good[2], (0, []), good[3],
               (2, [(0, 1), (2, 2)]), (1, [(0, 0), (0, 5)]), good[4], (4, [(0, 1), (1, 0), (10 ** 12, 1)]), good[5]]
    arrays = pack(entries, 5)
    hexes, stats = assert_law(arrays, 3, "statuses")
    assert stats == [0, 2, 0, 2, 0, 1, 0, 2, 2, 0, 2, 0]
    alone, _, _ = wl_law.wl_rows(*pack(good, 5), 3)
    assert [h for h in hexes if h] == alone


def test_end_to_end_ids_after_sample_batch():
    import ugs_sampler
    import ugs_workloads as workloads
    from ugs_sampler import wl
    ei, ptr = workloads.tu_batch(39, 73, 8)
    out = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 40, 6, mode="sample", seed=11, device=DEV)
    nodes, eidx, eptr = out[:3]
    assert nodes.shape == (320, 6)
    hexes, stats, _ = wl_law.wl_rows(nodes.cpu().numpy(), eidx.cpu().numpy(), eptr.cpu().numpy(), 3)
    vocab = {}
    for h in hexes[:100]:                              # a vocabulary that misses some of the batch's classes
        if h is not None and h not in vocab:
            vocab[h] = len(vocab)
    want = wl_law.ids_from(hexes, stats, vocab)
    assert len(vocab) in want and len(set(want)) > 3
    table = wl.WLVocab(vocab, DEV)
    ids = table.ids(nodes, eidx, eptr, 3)
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.cpu().tolist() == want
    host = table.ids(nodes.cpu(), eidx.cpu(), eptr.cpu(), 3)                   # CPU tensors in, CPU tensor out
    assert not host.is_cuda and host.tolist() == want
    d, s = wl.wl_hash(nodes.cpu(), eidx.cpu(), eptr.cpu(), 3)
    assert not d.is_cuda and not s.is_cuda and wl.hexdigests(d, s) == hexes
    grown = wl.extend_vocab({}, *wl.wl_hash(nodes[:100], eidx, eptr[:101], 3))
    assert grown == vocab


def test_presample_cache_batch_with_a_failed_graph():
    import ugs_workloads as workloads
    from ugs_sampler import wl
    from ugs_sampler.presample import PresampleCache
    m, k = 8, 6
    graphs = [workloads.tu_graph(20, 30, s) for s in range(4)]
    cache = PresampleCache(m, k, DEV)
    for i, g in enumerate(graphs):
        t = torch.from_numpy(g)
        cache.add(i, t.to(torch.int32) if i == 2 else t, 20, 42 + i)           # add refuses graph 2: its rows are the failed form
    assert cache.failed == {2}
    order = [2, 0, 2, 1, 3]
    ptr = np.arange(len(order) + 1) * 20
    cols = np.concatenate([graphs[i] + ptr[j] for j, i in enumerate(order)], axis=1)
    nodes, eidx, eptr = cache.load(torch.tensor(order), torch.from_numpy(ptr), torch.from_numpy(cols))[:3]
    hexes, stats, _ = wl_law.wl_rows(nodes.cpu().numpy(), eidx.cpu().numpy(), eptr.cpu().numpy(), 3)
    assert stats[:m] == [1] * m and stats[2 * m:3 * m] == [0] * m              # -1 rows at ptr 0; rows of ptr[g] - 1 later: k isolated vertices
    vocab = {h: i for i, h in enumerate(sorted({h for h in hexes if h}))}
    ids = wl.WLVocab(vocab, DEV).ids(nodes, eidx, eptr, 3)
    assert ids.cpu().tolist() == wl_law.ids_from(hexes, stats, vocab)


def test_lookup_tables():
    from ugs_sampler import wl
    rng = random.Random(9)
    arrays = pack(mixed_rows(rng, 6, rows=60), 6)
    hexes, stats, _ = wl_law.wl_rows(*arrays, 3)
    known = sorted({h for h in hexes if h})
    args = on_gpu(arrays)
    for name, vocab in (("empty", {}), ("all hits", {h: 5 + 2 * i for i, h in enumerate(known)}),
                        ("all misses", {"%032x" % (int(h, 16) ^ 1): i for i, h in enumerate(known)}),
                        ("fallback key", dict({"deg_10_edges_5": 0}, **{h: i + 1 for i, h in enumerate(known[::2])})),
                        ("one entry", {known[len(known) // 2]: 0}), ("first", {known[0]: 0}), ("last", {known[-1]: 0})):
        got = wl.WLVocab(vocab, DEV).ids(*args, 3).cpu().tolist()
        assert got == wl_law.ids_from(hexes, stats, vocab), name
    assert set(wl.WLVocab({}, DEV).ids(*args, 3).cpu().tolist()) == {0}


def test_fixture_digests_vocabulary_and_ids():
    from ugs_sampler import wl
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    z = np.load(GOLDEN + ".npz")
    for i, s in enumerate(meta["scenarios"]):
        args = on_gpu([z["s%d_nodes" % i], z["s%d_edge_index" % i], z["s%d_edge_ptr" % i]])
        digest, status = wl.wl_hash(*args, s["iterations"])
        got = wl.hexdigests(digest, status)
        if s["deviation"]:
            for h, want, st in zip(got, s["hashes"], status.cpu().tolist()):
                assert (st == 2 and h is None) if want.startswith("deg_") else (st == 0 and h == want), s["name"]
            continue
        assert got == s["hashes"], s["name"]
        assert status.cpu().tolist() == [0 if h else 1 for h in s["hashes"]], s["name"]
        half = (s["rows"] + 1) // 2
        vocab = wl.extend_vocab({}, digest[:half], status[:half])
        assert list(vocab) == s["vocab"] and list(vocab.values()) == list(range(len(vocab))), s["name"]
        assert wl.WLVocab(vocab, DEV).ids(*args, s["iterations"]).cpu().tolist() == z["s%d_ids" % i].tolist(), s["name"]


def test_limits_and_argument_errors_leave_the_library_usable():
    from ugs_sampler import wl
    rng = random.Random(2)
    good = pack(mixed_rows(rng, 6, rows=8), 6)
    wide = on_gpu(pack([(33, [(0, 32)])], 33))
    with pytest.raises(RuntimeError, match="k <= 32"):
        wl.wl_hash(*wide, 3)
    assert_law(good, 3, "after k = 33")
    with pytest.raises(RuntimeError, match="iterations <= 8"):
        wl.wl_hash(*on_gpu(good), 9)
    with pytest.raises(RuntimeError, match="iterations"):
        wl.wl_hash(*on_gpu(good), -1)
    assert_law(good, 3, "after iterations = 9")
    nodes, ei, ep = on_gpu(good)
    with pytest.raises(TypeError):
        wl.wl_hash(nodes.to(torch.int32), ei, ep)
    with pytest.raises(TypeError):
        wl.wl_hash(nodes.cpu().numpy(), ei, ep)
    with pytest.raises(TypeError):
        wl.wl_hash(nodes, ei, ep, 3.0)
    with pytest.raises(ValueError):
        wl.wl_hash(nodes, ei, ep[:-1])
    with pytest.raises(ValueError):
        wl.wl_hash(nodes, ei.t(), ep)
    with pytest.raises(ValueError):
        wl.wl_hash(nodes[0], ei, ep)
    with pytest.raises(ValueError):
        wl.wl_hash(nodes, ei.cpu(), ep)
    empty = wl.wl_hash(nodes[:0], ei[:, :0], ep[:1], 3)
    assert tuple(empty[0].shape) == (0, 2) and tuple(empty[1].shape) == (0,)
    assert_law(good, 3, "after the argument errors")
