"""The kernels of ugs_wl.hip on the inputs that pin their paths (tests/wl_paths.py), against the law (tests/wl_law.py,
tests/wl_feature_law.py, hashlib, a dict): every case names the census classes it is there for, and they are asserted again here,
so an input that stops reaching its path fails instead of losing coverage.  tests/test_wl_paths_law.py shows on the CPU that the
cases cover the census and tell the device model's mutants from the law.  Also here: the C entries' own refusals, called through
ctypes -- each is refused on the host before any launch."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import wl_law as L
import wl_paths as P
from test_gpu_wl import on_gpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HASH_NAMES = [c.name for c in P.cases() if c.form != "lookup"]
LOOKUP_NAMES = [c.name for c in P.cases() if c.form == "lookup"]
CANARY64, CANARY32 = 0x5a5a5a5a5a5a5a5a, 0x5a5a5a5a


def reaches_again(name):
    census = P.census_of(name)
    for cls in P.case(name).reaches:
        assert cls in census, (name, cls)


def label_kw(c):
    return {} if c.labels is None else {"node_labels": torch.tensor(c.labels, dtype=torch.int64, device=DEV)}


def digest_tensors(hexes, statuses):
    d = torch.tensor([L.digest_words(h) for h in hexes], dtype=torch.int64).reshape(-1, 2).to(DEV)
    return d, torch.tensor(statuses, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("name", HASH_NAMES)
def test_hash_case(name):
    from ugs_sampler import wl
    c = P.case(name)
    reaches_again(name)
    hexes, stats = P.law_of(name)
    for strided in (False, True):
        digest, status = wl.wl_hash(*on_gpu(c.arrays, strided), c.iterations, **label_kw(c))
        assert status.cpu().tolist() == stats, (name, strided)
        got = wl.hexdigests(digest, status)
        bad = [r for r, (a, b) in enumerate(zip(got, hexes)) if a != b]
        assert not bad, (name, strided, bad[:5], [got[r] for r in bad[:2]], [hexes[r] for r in bad[:2]])
        assert not digest.cpu()[torch.tensor(stats) != 0].any(), (name, strided)
    # the ids of real digests: a vocabulary of every second hashed row
    known = [h for h in hexes if h][::2]
    vocab = {h: 3 + 2 * i for i, h in enumerate(dict.fromkeys(known))}
    ids = wl.WLVocab(vocab, DEV).ids(*on_gpu(c.arrays), c.iterations, **label_kw(c))
    assert ids.cpu().tolist() == L.ids_from(hexes, stats, vocab), name


def test_rows_beside_a_bad_edge_ptr_range_hash_as_they_do_alone():
    from ugs_sampler import wl
    c = P.case("bad_edge_ptr")
    nodes, ei, ep = c.arrays
    hexes, stats = P.law_of(c.name)
    good = [r for r, s in enumerate(stats) if s == 0]
    assert good == [0, 2, 5, 8] and [stats[r] for r in (1, 3, 4, 6, 7)] == [2] * 5 and stats[9] == 1
    cols = np.concatenate([ei[:, ep[r]:ep[r + 1]] for r in good], axis=1)
    alone = (nodes[good], cols, np.array([0, 2, 4, 6, 8], np.int64))
    assert L.wl_rows(*alone, c.iterations)[0] == [hexes[r] for r in good]
    d1, s1 = wl.wl_hash(*on_gpu(alone), c.iterations)
    d2, s2 = wl.wl_hash(*on_gpu(c.arrays), c.iterations)
    assert s1.cpu().tolist() == [0] * 4 and wl.hexdigests(d1, s1) == [hexes[r] for r in good]
    assert torch.equal(d2[torch.tensor(good, device=DEV)], d1)
    # label mode takes the same guard: the rows' ids 0, 1, 2 with the labels of the label_values case
    import wl_feature_law as FL
    ids = np.where(nodes >= 0, nodes - 100, -1)
    fh, fs, _ = FL.wl_feature_rows(ids, ei, ep, P.LABELS8, c.iterations)
    d3, s3 = wl.wl_hash(*on_gpu((ids, ei, ep)), c.iterations, node_labels=torch.tensor(P.LABELS8, dtype=torch.int64, device=DEV))
    assert fs == stats and s3.cpu().tolist() == fs and wl.hexdigests(d3, s3) == fh


@pytest.mark.parametrize("name", LOOKUP_NAMES)
def test_lookup_case(name):
    from ugs_sampler import wl
    reaches_again(name)
    vocab, digests, statuses = P.case(name).arrays
    table = wl.WLVocab(vocab, DEV)
    assert len(table) == len(vocab)
    ids = table.lookup(*digest_tensors(digests, statuses))
    assert ids.dtype == torch.int64 and ids.cpu().tolist() == P.law_of(name), name


def test_md5_compact_widths_at_an_odd_row_stride():
    from ugs_sampler import wl
    rng = np.random.default_rng(5)
    reached = set()
    for F in P.MD5_WIDTHS:
        stride = F + 1 if F % 2 == 0 else F + 2
        host = rng.integers(0, 256, (P.MD5_ROWS, stride), dtype=np.uint8)
        x = torch.from_numpy(host).to(DEV)[:, :F]
        assert x.stride(0) == stride or F == 0
        got = wl.feature_labels(x)
        reached |= L.md5_census(F, [x.data_ptr() + i * stride for i in range(P.MD5_ROWS)])
        assert got.cpu().tolist() == [int(hashlib.md5(host[i, :F].tobytes()).hexdigest()[:8], 16) for i in range(P.MD5_ROWS)], F
    assert reached == set(L.MD5_CLASSES)


class Buffers:
    """Device buffers of one good call of the hash entries, outputs prefilled with a canary."""

    def __init__(self, name):
        c = P.case(name)
        self.case = c
        self.nodes, self.ei, self.ep = on_gpu(c.arrays)
        self.S, self.k = self.nodes.shape
        self.E = self.ei.size(1)
        self.labels = torch.tensor(c.labels if c.labels is not None else [0], dtype=torch.int64, device=DEV)
        self.digest = torch.full((self.S, 2), CANARY64, dtype=torch.int64, device=DEV)
        self.status = torch.full((self.S,), CANARY32, dtype=torch.int32, device=DEV)

    def args(self, labeled, **change):
        a = dict(nodes=self.nodes.data_ptr(), ei=self.ei.data_ptr(), stride=self.ei.stride(0), cols=self.E, ep=self.ep.data_ptr(),
                 rows=self.S, k=self.k, it=self.case.iterations, labels=self.labels.data_ptr(), nl=self.labels.numel(),
                 digest=self.digest.data_ptr(), status=self.status.data_ptr())
        a.update(change)
        p = lambda x: ctypes.c_void_p(x)               # noqa: E731: None is the null pointer
        head = (p(a["nodes"]), p(a["ei"]), a["stride"], a["cols"], p(a["ep"]), a["rows"], a["k"], a["it"])
        tail = (p(a["digest"]), p(a["status"]))
        return head + ((p(a["labels"]), a["nl"]) if labeled else ()) + tail

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.digest == CANARY64).all()) and bool((self.status == CANARY32).all())


@pytest.mark.parametrize("labeled", [False, True])
def test_hash_entries_refuse_on_the_host(labeled):
    from ugs_sampler import wl
    from ugs_sampler._lib import lib
    name = "label_values" if labeled else "edge_forms"
    b = Buffers(name)
    wl.wl_hash(b.nodes, b.ei, b.ep, b.case.iterations)                 # selects the device and torch's stream for this thread
    fn = lib.ugs_wl_hash_labeled if labeled else lib.ugs_wl_hash
    refusals = [(dict(nodes=None), b"null pointer"), (dict(ep=None), b"null pointer"), (dict(digest=None), b"null pointer"),
                (dict(status=None), b"null pointer"), (dict(ei=None), b"null pointer"), (dict(stride=b.E - 1), b"row_stride >= num_cols"),
                (dict(rows=-1), b"rows >= 0")]
    if labeled:
        refusals += [(dict(nl=-1), b"num_labels >= 0"), (dict(labels=None), b"null pointer")]
    assert b.E > 0 and b.labels.numel() > 0
    for change, message in refusals:
        rc = fn(*b.args(labeled, **change))
        assert rc != 0 and message in lib.ugs_last_error(), (change, rc, lib.ugs_last_error())
        assert b.untouched(), change
        assert fn(*b.args(labeled)) == 0, change                       # the library goes on working
        torch.cuda.synchronize()
        assert (wl.hexdigests(b.digest, b.status), b.status.cpu().tolist()) == P.law_of(name), change
        b.digest.fill_(CANARY64)
        b.status.fill_(CANARY32)


def test_lookup_entry_refuses_on_the_host():
    from ugs_sampler import wl
    from ugs_sampler._lib import lib
    name = "lookup_17"
    vocab, digests, statuses = P.case(name).arrays
    table = wl.WLVocab(vocab, DEV)
    digest, status = digest_tensors(digests, statuses)
    assert table.lookup(digest, status).cpu().tolist() == P.law_of(name)     # selects the device and the stream
    keys, key_ids = table._table()
    out = torch.full((len(statuses),), CANARY64, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def call(keys=keys, key_ids=key_ids, vocab_size=len(vocab), rows=len(statuses)):
        return lib.ugs_wl_lookup(p(digest), p(status), rows, p(keys), p(key_ids), vocab_size, len(vocab), p(out))

    for change, message in ((dict(vocab_size=-1), b"vocab_size >= 0"), (dict(keys=None), b"null pointer"), (dict(key_ids=None), b"null pointer"),
                            (dict(rows=-1), b"rows >= 0")):
        rc = call(**change)
        assert rc != 0 and message in lib.ugs_last_error(), (change, rc, lib.ugs_last_error())
        torch.cuda.synchronize()
        assert bool((out == CANARY64).all()), change
        assert call() == 0, change
        torch.cuda.synchronize()
        assert out.cpu().tolist() == P.law_of(name), change
        out.fill_(CANARY64)
