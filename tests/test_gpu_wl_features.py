"""The node-feature form of ugs_sampler.wl on the GPU (ugs_wl.hip: ugs_wl_feature_labels_kernel, label mode of ugs_wl_hash_kernel)
against hashlib, the plain-Python law (tests/wl_feature_law.py) and the reference's recorded results
(tests/golden/f20_wl_feature_reference): labels, digests, statuses and vocabulary ids, never against the library itself."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

import wl_feature_law as law
from test_gpu_wl import mixed_rows, on_gpu, pack, random_entry

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f20_wl_feature_reference")
DEV = "cuda:0"


def md5_labels(a):
    """hashlib's labels of a numpy array [N, ...], rows in C order."""
    return [int(hashlib.md5(np.ascontiguousarray(a[i]).tobytes()).hexdigest()[:8], 16) for i in range(a.shape[0])]


def check_labels(t, what):
    """feature_labels of the GPU tensor t against hashlib on its CPU copy."""
    from ugs_sampler import wl
    got = wl.feature_labels(t)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (t.size(0),), what
    assert got.cpu().tolist() == md5_labels(t.cpu().numpy()), what


# ---- MD5 labels against hashlib ----

@pytest.mark.parametrize("N", [0, 1, 63, 65, 257])
def test_md5_of_byte_rows_of_every_padding_case(N):
    rng = np.random.default_rng(N)
    for F in (0, 1, 3, 4, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 200):
        check_labels(torch.from_numpy(rng.integers(0, 256, (N, F), dtype=np.uint8)).to(DEV), f"uint8 N={N} F={F}")


def test_md5_of_the_empty_row():
    from ugs_sampler import wl
    assert wl.feature_labels(torch.empty((3, 0), dtype=torch.float32, device=DEV)).cpu().tolist() == [0xd41d8cd9] * 3


def test_md5_of_every_dtype():
    rng = np.random.default_rng(7)
    for F in (1, 3, 7, 13, 14, 15, 16, 18, 29, 30, 32):
        check_labels(torch.from_numpy(rng.standard_normal((65, F)).astype(np.float32)).to(DEV), f"float32 F={F}")
    for F in (1, 3, 27, 29):                           # odd widths: rows start at 2 mod 4
        check_labels(torch.from_numpy(rng.standard_normal((65, F)).astype(np.float16)).to(DEV), f"float16 F={F}")
    check_labels(torch.from_numpy(rng.standard_normal((65, 9))).to(DEV), "float64")
    check_labels(torch.from_numpy(rng.integers(-2 ** 62, 2 ** 62, (65, 9))).to(DEV), "int64")
    check_labels(torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (65, 5)).astype(np.int32)).to(DEV), "int32")
    check_labels(torch.from_numpy(rng.integers(-2 ** 15, 2 ** 15, (65, 5)).astype(np.int16)).to(DEV), "int16")
    check_labels(torch.from_numpy(rng.integers(-128, 128, (65, 5)).astype(np.int8)).to(DEV), "int8")
    check_labels(torch.from_numpy(rng.integers(0, 2, (65, 11)).astype(np.bool_)).to(DEV), "bool")
    check_labels(torch.from_numpy(np.eye(20, 3, dtype=np.float32)[rng.integers(0, 3, 65)]).to(DEV), "one-hot")
    check_labels(torch.from_numpy(rng.standard_normal(65).astype(np.float32)).to(DEV), "1-D: rows of one element")
    check_labels(torch.from_numpy(rng.standard_normal((65, 2, 3)).astype(np.float32)).to(DEV), "3-D")


def test_md5_of_views():
    rng = np.random.default_rng(8)
    base = torch.from_numpy(rng.standard_normal((40, 12)).astype(np.float32)).to(DEV)
    check_labels(base.t(), "transposed")
    check_labels(base[:, ::2], "every second column")
    check_labels(base[:, 2:9], "a block of columns: rows contiguous, row stride wider than the row")
    check_labels(base[::3], "every third row")
    check_labels(base[:, 0], "1-D strided")
    check_labels(base[:, :1].expand(40, 5), "expanded: stride 0")
    check_labels(base.reshape(40, 3, 4).permute(0, 2, 1), "3-D permuted")
    u8 = torch.from_numpy(rng.integers(0, 256, (66, 13), dtype=np.uint8)).to(DEV)
    assert u8[1:].is_contiguous() and u8[1:].data_ptr() % 2 == 1
    check_labels(u8[1:], "uint8 rows from an odd byte offset")
    check_labels(u8[:, 1:12], "uint8 column block at offset 1")
    f16 = torch.from_numpy(rng.standard_normal((66, 13)).astype(np.float16)).to(DEV)
    assert f16[1:].is_contiguous() and f16[1:].data_ptr() % 4 == 2
    check_labels(f16[1:], "float16 rows from a 2-mod-4 offset")


def test_feature_labels_of_cpu_tensors_come_back_on_the_cpu():
    from ugs_sampler import wl
    x = torch.eye(5, 3)
    got = wl.feature_labels(x, device=DEV)
    assert not got.is_cuda and got.tolist() == md5_labels(x.numpy())
    assert wl.feature_labels(x).tolist() == got.tolist()


# ---- the hash law with features ----

def pack_ids(entries, k, rng, N, holes=True):
    """`pack` with vertex ids below N (duplicates happen) and, with `holes`, the valid entries spread over the k slots."""
    nodes, ei, ep = pack(entries, k)
    for r, (n, _) in enumerate(entries):
        slots = sorted(rng.sample(range(k), n)) if holes and rng.random() < 0.5 else list(range(n))
        nodes[r] = -1
        nodes[r, slots] = [rng.randrange(N) for _ in range(n)]
    return nodes, ei, ep


def assert_feature_law(arrays, x, iterations, what, strided=False, labels=None):
    """wl_hash(x=) on the GPU against the law; x a numpy array (or `labels` a list of ints given as node_labels=)."""
    from ugs_sampler import wl
    lab = law.labels_of(x) if labels is None else labels
    hexes, stats, _ = law.wl_feature_rows(*arrays, lab, iterations)
    kw = {"x": torch.from_numpy(x).to(DEV)} if labels is None else {"node_labels": torch.tensor(labels, dtype=torch.int64, device=DEV)}
    digest, status = wl.wl_hash(*on_gpu(arrays, strided), iterations, **kw)
    assert digest.is_cuda and digest.dtype == torch.int64 and tuple(digest.shape) == (len(hexes), 2)
    assert status.is_cuda and status.dtype == torch.int32 and tuple(status.shape) == (len(hexes),)
    assert status.cpu().tolist() == stats, what
    got = wl.hexdigests(digest, status)
    bad = [r for r, (a, b) in enumerate(zip(got, hexes)) if a != b]
    assert not bad, (what, bad[:5], [got[r] for r in bad[:2]], [hexes[r] for r in bad[:2]])
    assert not digest.cpu()[torch.tensor(stats) != 0].any(), what
    return hexes, stats


def three_rows(N):
    return np.eye(3, dtype=np.float32)[np.arange(N) % 3]                      # three distinct rows: ties everywhere


def distinct_rows(N):
    return np.arange(N, dtype=np.float32).reshape(N, 1) * 0.5                 # all rows distinct


@pytest.mark.parametrize("k", range(1, 33))
def test_every_k(k):
    rng = random.Random(2000 + k)
    arrays = pack_ids(mixed_rows(rng, k), k, rng, 50)
    hexes, stats = assert_feature_law(arrays, three_rows(50), 3, f"k={k}, three labels")
    assert 0 in stats and 1 in stats
    assert_feature_law(arrays, distinct_rows(50), 3, f"k={k}, distinct labels")


@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 8])
def test_iterations(iterations):
    rng = random.Random(6)
    for k, rows in ((7, 24), (20, 12)):
        arrays = pack_ids(mixed_rows(rng, k, rows=rows), k, rng, 40)
        assert_feature_law(arrays, three_rows(40), iterations, f"iterations={iterations} k={k}")
        assert_feature_law(arrays, distinct_rows(40), iterations, f"iterations={iterations} k={k} distinct")


@pytest.mark.parametrize("rows", [1, 7, 257])
def test_launch_shapes_and_row_stride(rows):
    rng = random.Random(rows)
    for k in (6, 11, 19):
        entries = mixed_rows(rng, k, rows=max(rows, 3))[:rows]
        arrays = pack_ids(entries, k, rng, 30)
        assert_feature_law(arrays, three_rows(30), 3, f"rows={rows} k={k}")
        assert_feature_law(arrays, distinct_rows(30), 3, f"rows={rows} k={k} strided", strided=True)


def test_first_messages_of_exactly_one_and_two_blocks():
    """In iteration 1 a vertex of degree d sends 8 + 8 d bytes: 128 at degree 15, 256 at degree 31.  Degrees 14, 16 and 30 sit
    beside them.  The rows are chosen by the law's own length report."""
    both = lambda es: [e for u, v in es for e in ((u, v), (v, u))]                # noqa: E731
    star = lambda n, d: (n, both([(0, i) for i in range(1, d + 1)]))             # noqa: E731
    rng = random.Random(4)
    for k, entries, want in ((16, [star(16, 15), star(16, 14), star(15, 14), star(16, 13)], {120, 128}),
                             (32, [star(32, 31), star(32, 30), star(32, 16), star(32, 15), star(32, 14), (32, both([(0, i) for i in range(1, 16)]) + [(0, 0)])],
                              {120, 128, 136, 248, 256})):
        arrays = pack_ids(entries, k, rng, 64, holes=False)
        for x in (three_rows(64), distinct_rows(64)):
            for it in (1, 3):
                _, _, reports = law.wl_feature_rows(*arrays, law.labels_of(x), it)
                assert want <= {v for lens, _ in reports for v in lens[0]}
                assert_feature_law(arrays, x, it, f"first-message blocks k={k} it={it}")


def test_compaction_and_duplicates():
    both = lambda es: [e for u, v in es for e in ((u, v), (v, u))]                # noqa: E731
    for k in (5, 8, 17):
        pad = lambda r: list(r) + [-1] * (k - len(r))                             # noqa: E731
        nodes = np.array([pad([5, -1, 7, -1, 9]), [39] * k, pad([-1, -1, 3, -1, 4]), pad([-1, 2]), pad([6, 6, 1, 6]), pad([-1, -1, -1, -1, 11])], np.int64)
        edges = [both([(0, 1), (1, 2)]), both([(0, 1), (2, 3), (3, 4)]), both([(0, 1)]), [(0, 0)], both([(0, 1), (1, 2), (2, 3)]), []]
        cols = [e for es in edges for e in es]
        arrays = (nodes, np.ascontiguousarray(np.array(cols, np.int64).T), np.cumsum([0] + [len(es) for es in edges]).astype(np.int64))
        hexes, stats = assert_feature_law(arrays, distinct_rows(40), 3, f"compaction k={k}")
        assert stats == [0] * 6
        same = (np.array([pad([5, 7, 9])], np.int64), arrays[1][:, :4], np.array([0, 4], np.int64))      # the first row without its holes
        assert law.wl_feature_rows(*same, law.labels_of(distinct_rows(40)), 3)[0][0] == hexes[0]


def test_statuses_do_not_disturb_neighbouring_rows():
    rng = random.Random(3)
    N = 20
    good = [random_entry(rng, 5) for _ in range(6)]
    entries = [good[0], (3, [(0, 1), (1, 2)]), good[1], (3, [(0, 1), (1, 3)]), good[2], (0, []), good[3], (2, [(0, 1)]), good[4], (4, [(0, 1), (9, 1)]), good[5]]
    arrays = pack_ids(entries, 5, rng, N, holes=False)
    arrays[0][1, 1] = N                                # an id equal to N: status 3
    arrays[0][3, 0] = N + 5                            # a bad endpoint and a bad id: status 2
    arrays[0][7, 1] = 10 ** 12                         # status 3
    arrays[0][9, 2] = N                                # a bad endpoint and a bad id again
    hexes, stats = assert_feature_law(arrays, three_rows(N), 3, "statuses")
    assert stats == [0, 3, 0, 2, 0, 1, 0, 3, 0, 2, 0]
    keep = [r for r, s in enumerate(stats) if s == 0]
    alone = (arrays[0][keep], ) + pack(good, 5)[1:]
    assert law.wl_feature_rows(*alone, law.labels_of(three_rows(N)), 3)[0] == [h for h in hexes if h]


def test_node_labels_given_directly():
    from ugs_sampler import wl
    rng = random.Random(12)
    labels = [0, 9, 10, 0xffffffff, 0xa0000000, 0x0a000000, -1, 1 << 32, 7, 7]
    entries = [random_entry(rng, 6) for _ in range(30)]
    nodes, ei, ep = pack(entries, 6)
    for r in range(30):
        nodes[r] = [rng.choice([0, 1, 2, 3, 4, 5, 8, 9]) for _ in range(6)]
        if r % 5 == 0:
            nodes[r, rng.randrange(6)] = 6 if r % 10 else 7                       # a label of -1 or of 2^32
    hexes, stats = assert_feature_law((nodes, ei, ep), None, 3, "node_labels", labels=labels)
    assert stats.count(3) >= 3 and stats.count(0) >= 20
    bad = [r for r in range(30) if 6 in nodes[r] or 7 in nodes[r]]
    assert [r for r, s in enumerate(stats) if s == 3] == bad
    x = np.eye(4, dtype=np.float32)[np.arange(10) % 4]                            # feature_labels(x) as node_labels equals x=
    args = on_gpu((nodes, ei, ep))
    xt = torch.from_numpy(x).to(DEV)
    d1, s1 = wl.wl_hash(*args, 3, x=xt)
    d2, s2 = wl.wl_hash(*args, 3, node_labels=wl.feature_labels(xt))
    want, wstats, _ = law.wl_feature_rows(nodes, ei, ep, law.labels_of(x), 3)
    assert wl.hexdigests(d1, s1) == want == wl.hexdigests(d2, s2) and s1.cpu().tolist() == wstats == s2.cpu().tolist()
    d0, s0 = wl.wl_hash(*args, 3, node_labels=torch.empty((0,), dtype=torch.int64, device=DEV))      # no label rows at all
    assert s0.cpu().tolist() == [3] * 30 and not d0.cpu().any()


def test_fixture_digests_vocabulary_and_ids():
    from ugs_sampler import wl
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    z = np.load(GOLDEN + ".npz")
    for i, s in enumerate(meta["scenarios"]):
        args = on_gpu([z["s%d_nodes" % i], z["s%d_edge_index" % i], z["s%d_edge_ptr" % i]])
        x = torch.from_numpy(z["s%d_x" % i]).to(DEV)
        digest, status = wl.wl_hash(*args, s["iterations"], x=x)
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
        assert wl.WLVocab(vocab, DEV).ids(*args, s["iterations"], x=x).cpu().tolist() == z["s%d_ids" % i].tolist(), s["name"]


def ids_from(hexes, stats, vocab):
    return [vocab.get(h, len(vocab)) if st == 0 else len(vocab) for h, st in zip(hexes, stats)]


def test_end_to_end_ids_after_sample_batch():
    import ugs_sampler
    import ugs_workloads as workloads
    from ugs_sampler import wl
    ei, ptr = workloads.tu_batch(39, 73, 8)
    out = ugs_sampler.sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), 40, 6, mode="sample", seed=11, device=DEV)
    nodes, eidx, eptr = out[:3]
    assert nodes.shape == (320, 6)
    x = np.eye(3, dtype=np.float32)[np.random.default_rng(5).integers(0, 3, int(ptr[-1]))]
    hexes, stats, _ = law.wl_feature_rows(nodes.cpu().numpy(), eidx.cpu().numpy(), eptr.cpu().numpy(), law.labels_of(x), 3)
    vocab = {}
    for h in hexes[:100]:                              # a vocabulary that misses some of the batch's classes
        if h is not None and h not in vocab:
            vocab[h] = len(vocab)
    want = ids_from(hexes, stats, vocab)
    assert len(vocab) in want and len(set(want)) > 3
    table = wl.WLVocab(vocab, DEV)
    xt = torch.from_numpy(x).to(DEV)
    ids = table.ids(nodes, eidx, eptr, 3, x=xt)
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.cpu().tolist() == want
    assert table.ids(nodes, eidx, eptr, 3, node_labels=wl.feature_labels(xt)).cpu().tolist() == want
    assert table.ids(nodes, eidx, eptr, 3).cpu().tolist() != want                  # the degree form is another function
    host = table.ids(nodes.cpu(), eidx.cpu(), eptr.cpu(), 3, x=torch.from_numpy(x))      # CPU tensors in, CPU tensor out
    assert not host.is_cuda and host.tolist() == want
    d, s = wl.wl_hash(nodes.cpu(), eidx.cpu(), eptr.cpu(), 3, x=torch.from_numpy(x))
    assert not d.is_cuda and not s.is_cuda and wl.hexdigests(d, s) == hexes
    with pytest.raises(ValueError):
        wl.wl_hash(nodes, eidx, eptr, 3, x=torch.from_numpy(x))                   # sampler tensors on the GPU, x on the CPU
    grown = wl.extend_vocab({}, *wl.wl_hash(nodes[:100], eidx, eptr[:101], 3, x=xt))
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
    x = np.eye(7, dtype=np.float32)[np.random.default_rng(6).integers(0, 7, 100)]
    hexes, stats, _ = law.wl_feature_rows(nodes.cpu().numpy(), eidx.cpu().numpy(), eptr.cpu().numpy(), law.labels_of(x), 3)
    assert stats[:m] == [1] * m and stats[2 * m:3 * m] == [0] * m
    vocab = {h: i for i, h in enumerate(sorted({h for h in hexes if h}))}
    ids = wl.WLVocab(vocab, DEV).ids(nodes, eidx, eptr, 3, x=torch.from_numpy(x).to(DEV))
    assert ids.cpu().tolist() == ids_from(hexes, stats, vocab)


def test_limits_and_errors_leave_the_library_usable():
    from ugs_sampler import wl
    from ugs_sampler._lib import lib
    rng = random.Random(2)
    good = pack_ids(mixed_rows(rng, 6, rows=8), 6, rng, 12)
    x = three_rows(12)
    xt = torch.from_numpy(x).to(DEV)
    wide = on_gpu(pack([(33, [(0, 32)])], 33))
    with pytest.raises(RuntimeError, match="k <= 32"):
        wl.wl_hash(*wide, 3, x=torch.zeros((200, 3), device=DEV))
    assert_feature_law(good, x, 3, "after k = 33")
    with pytest.raises(RuntimeError, match="iterations <= 8"):
        wl.wl_hash(*on_gpu(good), 9, x=xt)
    assert_feature_law(good, x, 3, "after iterations = 9")
    out = torch.zeros((4,), dtype=torch.int64, device=DEV)
    rc = lib.ugs_wl_feature_labels(ctypes.c_void_p(xt.data_ptr()), 1 << 29, 1 << 29, 1, ctypes.c_void_p(out.data_ptr()))      # refused before any launch
    assert rc != 0 and b"2^29" in lib.ugs_last_error()
    assert lib.ugs_wl_feature_labels(ctypes.c_void_p(xt.data_ptr()), 12, 8, 4, ctypes.c_void_p(out.data_ptr())) != 0          # stride below the row
    assert lib.ugs_wl_feature_labels(ctypes.c_void_p(xt.data_ptr()), -1, 12, 4, ctypes.c_void_p(out.data_ptr())) != 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0] * 4
    nodes, ei, ep = on_gpu(good)
    empty = wl.wl_hash(nodes[:0], ei[:, :0], ep[:1], 3, x=xt)
    assert tuple(empty[0].shape) == (0, 2) and tuple(empty[1].shape) == (0,)
    assert_feature_law(good, x, 3, "after the refused calls")
