"""GPU: ugs_sampler.rows.unique_rows against its law (tests/rows_unique_law.py; include/ugs_mi355.h at ugs_rows_unique_begin).
All seven outputs must equal the law bit for bit; `last_launch()` is asserted wherever a kernel form is named.  The refusals on the
device are validation paths that return a status word: none of them is written to fault, and a good call follows each."""
import threading

import numpy as np
import pytest
import torch

import rows_unique_law as law
import ugs_workloads as wl
from ugs_sampler import rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src", "count", "inverse")


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _same(got, want, what=""):
    for name, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy()
        assert a.dtype == np.int64 and a.shape == b.shape, f"{what}{name}: shape {a.shape} against the law's {b.shape}"
        assert np.array_equal(a, b), f"{what}{name} differs from the law"


def _check(case, by, form=None, what=""):
    nodes, ei, eptr, sptr, esrc, ptr = case
    want = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, by)
    five = _dev((nodes, ei, eptr, sptr, esrc))
    got = rows.unique_rows(*five, ptr=torch.from_numpy(ptr), by=by)
    assert all(t.is_cuda for t in got)
    if form is not None:
        assert rows.last_launch() == form
    _same(got, want, what)
    return got, want


def _digits_case(indices, k, base):
    """One graph of `base` vertices whose row i holds the base-`base` digits of indices[i]: distinct indices, distinct sequences."""
    idx = np.asarray(indices, dtype=np.int64)
    nodes = np.stack([(idx // base ** j) % base for j in range(k)], axis=1).astype(np.int64)
    ei, eptr, esrc = law.with_edges(nodes, np.random.default_rng(len(idx)), 3)
    return nodes, ei, eptr, np.array([0, len(idx)], dtype=np.int64), esrc, np.array([0, base], dtype=np.int64)


# ---- wave form ----
@pytest.mark.parametrize("by", ["set", "sequence"])
@pytest.mark.parametrize("rows_per_graph", [[0], [1], [2], [63], [64], [0, 1, 2, 63, 64, 0, 17, 64, 5], [0, 0, 0]])
def test_wave_form(rows_per_graph, by):
    rng = np.random.default_rng(sum(rows_per_graph) + len(rows_per_graph))
    _check(law.random_case(rng, rows_per_graph, 6), by, "wave" if sum(rows_per_graph) else "none")


# ---- workgroup form ----
@pytest.mark.parametrize("by", ["set", "sequence"])
@pytest.mark.parametrize("rows_per_graph", [[65], [100], [129], [256], [257], [1024], [1025]])
def test_workgroup_form(rows_per_graph, by):
    rng = np.random.default_rng(rows_per_graph[0])
    _check(law.random_case(rng, rows_per_graph, 6, distinct=40), by, "workgroup")


@pytest.mark.parametrize("by", ["set", "sequence"])
@pytest.mark.parametrize("kind", ["half", "equal", "distinct"])
def test_workgroup_form_4096_rows(kind, by):
    rng = np.random.default_rng(4096)
    idx = {"half": rng.permutation(np.arange(4096) % 2048), "equal": np.full(4096, 1234), "distinct": rng.permutation(4096)}[kind]
    got, want = _check(_digits_case(idx, 6, 8), by, "workgroup")
    if by == "sequence":
        assert got.nodes.size(0) == {"half": 2048, "equal": 1, "distinct": 4096}[kind]


@pytest.mark.parametrize("by", ["set", "sequence"])
def test_mixed_batch(by):
    rng = np.random.default_rng(11)
    _check(law.random_case(rng, [3, 70, 0, 300, 64, 65, 1100, 1, 4096, 0, 130], 5, distinct=25), by, "wave+workgroup")


@pytest.mark.parametrize("by", ["set", "sequence"])
def test_more_graphs_than_one_pass_of_the_scan_across_graphs(by):
    """2500 graphs: the scan across graphs takes 1024 a pass and carries the totals on; most graphs have 0 to 3 rows."""
    rng = np.random.default_rng(2500)
    rows_per_graph = rng.integers(0, 4, size=2500).tolist()
    rows_per_graph[1023], rows_per_graph[1024], rows_per_graph[2499] = 70, 64, 66
    _check(law.random_case(rng, rows_per_graph, 3, distinct=2, max_edges=2), by, "wave+workgroup")


# ---- keys ----
@pytest.mark.parametrize("by", ["set", "sequence"])
@pytest.mark.parametrize("k", [1, 2, 5, 8, 9, 32])
def test_every_k(k, by):
    rng = np.random.default_rng(k)
    _check(law.random_case(rng, [10, 80, 0, 33], k, distinct=12), by, "wave+workgroup")


def _top_bit_case(k, n, lo=5):
    """A graph of n vertices behind one of `lo`: rows that use its last vertex in every position, in some, and -1."""
    top = lo + n - 1
    pool = [[top] * k, [top] * (k - 1) + [lo], [lo] + [top] * (k - 1), [top] * (k - 1) + [-1], [-1] * k, [top - 1] * k, [top] * k,
            [lo] * k, [lo + 1] + [top] * (k - 1)]
    rng = np.random.default_rng(n)
    rows70 = [pool[i] for i in rng.integers(0, len(pool), size=70)]
    nodes = np.array([[0, 1, 2, 3, 4, 0, 1, 2][:k]] * 2 + pool + rows70, dtype=np.int64)
    last = nodes[2 + len(pool):]                                          # graph 2 repeats graph 1's rows one graph further
    last[last >= 0] += n
    ei, eptr, esrc = law.with_edges(nodes, rng, 3)
    return nodes, ei, eptr, np.array([0, 2, 2 + len(pool), len(nodes)], dtype=np.int64), esrc, np.array([0, lo, lo + n, lo + 2 * n], dtype=np.int64)


@pytest.mark.parametrize("by", ["set", "sequence"])
def test_k8_graph_of_65535_vertices_sets_every_top_bit(by):
    case = _top_bit_case(8, 65535)
    ptr = case[5]
    assert case[0].max() == 5 + 2 * 65535 - 1
    _check(case, by, "wave+workgroup")
    # one vertex more and the graph's codes need 17 bits: refused by name
    ptr2 = ptr.copy()
    ptr2[2:] += 1
    five = _dev(case[:5])
    with pytest.raises(RuntimeError, match="graph 1 has more than 65535 vertices"):
        rows.unique_rows(*five, ptr=torch.from_numpy(ptr2), by=by)
    assert rows.last_launch() == "none"
    _check(case, by, "wave+workgroup", "after the refusal: ")


@pytest.mark.parametrize("by", ["set", "sequence"])
def test_k6_at_21_bits(by):
    _check(_top_bit_case(6, (1 << 21) - 1), by, "wave+workgroup")


@pytest.mark.parametrize("by", ["set", "sequence"])
@pytest.mark.parametrize("k", [5, 8, 9])
def test_rows_that_differ_in_one_field(k, by):
    base = np.arange(k, dtype=np.int64)
    first, last = base.copy(), base.copy()
    first[0], last[-1] = k, k + 1                                        # (as sets these differ in the extreme coded fields too)
    nodes = np.stack([base, last, first, base, last, first])
    ei, eptr, esrc = law.with_edges(nodes, np.random.default_rng(k), 2)
    got, _ = _check((nodes, ei, eptr, np.array([0, 6]), esrc, np.array([0, k + 2])), by, "wave")
    assert got.nodes.size(0) == 3 and got.count.tolist() == [2, 2, 2] and got.inverse.tolist() == [0, 1, 2, 0, 1, 2]


# ---- semantics ----
def test_permuted_rows_merge_as_sets_only_and_the_first_is_kept_unsorted():
    nodes = np.array([[12, 10, 11], [10, 11, 12], [11, 12, 10], [10, 10, 11], [12, 10, 11]], dtype=np.int64)
    ei, eptr, esrc = law.with_edges(nodes, np.random.default_rng(3), 3)
    case = (nodes, ei, eptr, np.array([0, 5]), esrc, np.array([10, 14]))
    s, _ = _check(case, "set", "wave")
    q, _ = _check(case, "sequence", "wave")
    assert s.nodes.tolist() == [[12, 10, 11], [10, 10, 11]] and s.count.tolist() == [4, 1] and s.inverse.tolist() == [0, 0, 0, 1, 0]
    assert q.nodes.tolist() == [[12, 10, 11], [10, 11, 12], [11, 12, 10], [10, 10, 11]] and q.count.tolist() == [2, 1, 1, 1]


def test_equal_sets_in_different_graphs_do_not_merge():
    nodes = np.array([[0, 1], [1, 0], [4, 5], [5, 4], [4, 5]], dtype=np.int64)          # local ids (0, 1) in both graphs
    ei, eptr, esrc = law.with_edges(nodes, np.random.default_rng(4), 2)
    got, _ = _check((nodes, ei, eptr, np.array([0, 2, 5]), esrc, np.array([0, 4, 8])), "set", "wave")
    assert got.nodes.tolist() == [[0, 1], [4, 5]] and got.sample_ptr.tolist() == [0, 1, 2] and got.count.tolist() == [2, 3]


def test_placeholder_rows_merge_and_partly_empty_rows_are_told_apart():
    nodes = np.array([[-1, -1, -1], [-1, -1, -1], [-1, 2, -1], [2, -1, -1], [-1, -1, 3], [-1, -1, -1]], dtype=np.int64)
    ei, eptr, esrc = law.with_edges(nodes, np.random.default_rng(5), 0)
    got, _ = _check((nodes, ei, eptr, np.array([0, 6]), esrc, np.array([0, 4])), "set", "wave")
    assert got.nodes.tolist() == [[-1, -1, -1], [-1, 2, -1], [-1, -1, 3]] and got.count.tolist() == [3, 2, 1]
    assert got.edge_index.shape == (2, 0) and got.edge_ptr.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("by", ["set", "sequence"])
def test_rows_without_edges_empty_edge_src_and_strided_edge_index(by):
    rng = np.random.default_rng(6)
    case = law.random_case(rng, [30, 90], 4, max_edges=2, edge_src=False)
    got, want = _check(case, by, "wave+workgroup")
    assert got.edge_src.shape == (0,)
    nodes, ei, eptr, sptr, esrc, ptr = law.random_case(rng, [30, 90], 4, max_edges=2)
    want = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, by)
    Es = ei.shape[1]
    wide = torch.full((2, 2 * Es + 3), -99, dtype=torch.int64, device=DEV)
    wide[:, 0:2 * Es:2] = torch.from_numpy(ei).to(DEV)
    n_d, p_d, s_d, src_d = _dev((nodes, eptr, sptr, esrc))
    _same(rows.unique_rows(n_d, wide[:, 0:2 * Es:2], p_d, s_d, src_d, ptr=torch.from_numpy(ptr).to(DEV), by=by), want, "column stride 2: ")
    wide[:, :Es] = torch.from_numpy(ei).to(DEV)
    _same(rows.unique_rows(n_d, wide[:, :Es], p_d, s_d, src_d, ptr=torch.from_numpy(ptr), by=by), want, "row stride > E: ")


def test_cpu_tensors_in_give_cpu_results():
    rng = np.random.default_rng(8)
    nodes, ei, eptr, sptr, esrc, ptr = law.random_case(rng, [20, 70], 6)
    want = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, "set")
    got = rows.unique_rows(*[torch.from_numpy(a) for a in (nodes, ei, eptr, sptr, esrc)], ptr=torch.from_numpy(ptr), by="set", device=DEV)
    assert all(t.device.type == "cpu" for t in got)
    _same(got, want)


def test_repeated_calls_are_bit_identical():
    rng = np.random.default_rng(9)
    case = law.random_case(rng, [64, 700, 65], 6, distinct=30)
    five = _dev(case[:5])
    a = rows.unique_rows(*five, ptr=torch.from_numpy(case[5]))
    for _ in range(3):
        b = rows.unique_rows(*five, ptr=torch.from_numpy(case[5]))
        assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- end to end: every sampler's five tensors, and the presample cache's ----
def _sampled(name, mode, n, e, k, m):
    ei, ptr = wl.tu_batch(n, e, 16)
    ei_t, ptr_t = torch.from_numpy(ei), torch.from_numpy(ptr)
    if name == "ugs":
        import ugs_sampler
        return ugs_sampler.sample_batch(ei_t, ptr_t, m, k, mode=mode, seed=42, device=DEV), ptr
    if name == "rwr":
        import rwr_sampler
        return rwr_sampler.sample_batch(ei_t.to(DEV), ptr_t, m, k, mode=mode, seed=42, p_restart=0.2), ptr
    if name == "uniform":
        import uniform_sampler
        return uniform_sampler.sample_batch(ei_t.to(DEV), ptr_t, m, k, mode=mode, seed=42), ptr
    import epsilon_uniform_sampler
    return epsilon_uniform_sampler.sample_batch(ei_t.to(DEV), ptr_t, m, k, mode=mode, seed=42), ptr


def _end_to_end(five, ptr, by="set"):
    assert all(t.is_cuda for t in five)
    want = law.unique_rows(*[t.cpu().numpy() for t in five], ptr, by)
    got = rows.unique_rows(*five, ptr=torch.from_numpy(ptr), by=by)
    _same(got, want)
    assert torch.equal(got.nodes[got.inverse].sort(dim=1).values, five[0].sort(dim=1).values)
    return got


@pytest.mark.parametrize("mode", ["sample", "global"])
@pytest.mark.parametrize("shape", [(18, 20, 6, 0.680), (18, 19, 5, 0.550)])
def test_end_to_end_rwr_and_its_kept_fraction(shape, mode):
    n, e, k, kept = shape
    five, ptr = _sampled("rwr", mode, n, e, k, 100)
    got = _end_to_end(five, ptr)
    assert rows.last_launch() == "workgroup"
    fraction = got.nodes.size(0) / five[0].size(0)
    print(f"kept by set: {fraction:.6f}")
    assert f"{fraction:.3f}" == f"{kept:.3f}"


@pytest.mark.parametrize("mode", ["sample", "global"])
@pytest.mark.parametrize("name", ["ugs", "uniform", "epsilon_uniform"])
def test_end_to_end_other_samplers(name, mode):
    five, ptr = _sampled(name, mode, 18, 20, 6, 64)
    _end_to_end(five, ptr)
    assert rows.last_launch() == "wave"


def test_end_to_end_presample_cache_with_a_failed_graph():
    """The failed graph stands first in the batch: load gives it rows of -1 + ptr[g], which are placeholder rows (-1) only there."""
    from ugs_sampler.presample import PresampleCache
    ei, ptr = wl.tu_batch(18, 20, 16)
    cache = PresampleCache(100, 6, DEV, sampler="rwr")
    for g in range(16):
        cols = ei[:, (ei[0] >= ptr[g]) & (ei[0] < ptr[g + 1])] - ptr[g]
        t = torch.from_numpy(np.ascontiguousarray(cols))
        assert cache.add(g, t.to(torch.int32) if g == 0 else t, 18, 42 + g) == (g != 0)
    assert cache.failed == {0}
    five = cache.load(list(range(16)), torch.from_numpy(ptr), torch.from_numpy(ei))
    got = _end_to_end(five, ptr)
    assert got.sample_ptr[1].item() == 1 and got.count[0].item() == 100 and got.nodes[0].tolist() == [-1] * 6


# ---- refusals on the device: status words, no faults; the outputs' neighbours stay intact and the next call is good ----
def _good_case():
    return law.random_case(np.random.default_rng(21), [10, 70, 5], 4, distinct=9)


def _bad(kind):
    nodes, ei, eptr, sptr, esrc, ptr = [a.copy() for a in _good_case()]
    if kind == "outside":
        nodes[37, 2] = ptr[2]                                              # row 37 is graph 1's; the entry is graph 2's first vertex
        return (nodes, ei, eptr, sptr, esrc, ptr), "row 37 has an entry"
    if kind == "minus_two":
        nodes[3, 0] = -2
        return (nodes, ei, eptr, sptr, esrc, ptr), "row 3 has an entry"
    if kind == "edge_ptr":
        eptr[40] = eptr[41] + 2                                            # decreases from index 40 to 41
        return (nodes, ei, eptr, sptr, esrc, ptr), r"edge_ptr must start at 0, must not decrease.*index 40"
    rng = np.random.default_rng(22)                                        # 4097 rows in graph 1
    nodes = np.concatenate([nodes[:10], rng.integers(ptr[1], ptr[2], size=(4097, 4)), nodes[80:]]).astype(np.int64)
    ei, eptr, esrc = law.with_edges(nodes, rng, 1)
    return (nodes, ei, eptr, np.array([0, 10, 4107, 4112]), esrc, ptr), "graph 1 has more than 4096 rows"


CANARY = 0x5A5A5A5A5A5A5A5A
PAD = 32


def _abi_call(case, by):
    """The call through the C ABI with outputs the test owns: one block filled with a canary, out of which the seven outputs are
    carved with PAD words between them.  Returns (status, message, outputs or None, the block is a canary wherever no output is)."""
    import ctypes as C

    import ugs_sampler
    from ugs_sampler._lib import lib, vp
    nodes, ei, eptr, sptr, esrc = _dev(case[:5])
    ptr = torch.from_numpy(case[5]).to(DEV)
    R, k = nodes.shape
    G, Es = sptr.numel() - 1, ei.size(1)
    block = torch.full((R * k + 3 * Es + 3 * R + G + 2 + 8 * PAD,), CANARY, dtype=torch.int64, device=DEV)
    ugs_sampler._select_device(torch.device(DEV), jobs=True)
    job, U, Eu = vp(), C.c_int64(), C.c_int64()
    rc = lib.ugs_rows_unique_begin(nodes.data_ptr(), k, R, eptr.data_ptr(), Es, sptr.data_ptr(), G, ptr.data_ptr(), 1 if by == "set" else 0,
                                   C.byref(job), C.byref(U), C.byref(Eu))
    if rc != 0:
        torch.cuda.synchronize()
        return rc, (lib.ugs_last_error() or b"").decode(), None, bool((block == CANARY).all())
    u, e = U.value, Eu.value
    sizes = [u * k, 2 * e, u + 1, G + 1, e, u, R]
    outs, at = [], PAD
    for n in sizes:
        outs.append(block[at:at + n])
        at += n + PAD
    rc = lib.ugs_rows_unique_finish(job, outs[0].data_ptr(), ei.data_ptr(), ei.stride(0), esrc.data_ptr(), outs[1].data_ptr(), e, outs[2].data_ptr(),
                                    outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(), outs[6].data_ptr())
    torch.cuda.synchronize()
    mask = torch.ones_like(block, dtype=torch.bool)
    at = PAD
    for n in sizes:
        mask[at:at + n] = False
        at += n + PAD
    intact = bool((block[mask] == CANARY).all())
    return rc, "", (outs[0].view(u, k), outs[1].view(2, e), outs[2], outs[3], outs[4], outs[5], outs[6]), intact


@pytest.mark.parametrize("kind", ["outside", "minus_two", "edge_ptr", "rows"])
def test_device_refusals_leave_the_library_usable(kind):
    case, text = _bad(kind)
    five = _dev(case[:5])
    with pytest.raises(RuntimeError, match=text):
        rows.unique_rows(*five, ptr=torch.from_numpy(case[5]).to(DEV), by="set")
    torch.cuda.synchronize()
    assert rows.last_launch() == "none"
    for t, a in zip(five, case[:5]):
        assert np.array_equal(t.cpu().numpy(), a), "a refused call changed its inputs"
    # the same through the C ABI, with the test's own output block: a status, a message, no job, and the block untouched
    import re
    rc, msg, outs, intact = _abi_call(case, "set")
    assert rc < 0 and re.search(text, msg) and outs is None and intact
    # a good call right after: the law's result, and nothing written outside the outputs
    good = _good_case()
    rc, _, outs, intact = _abi_call(good, "set")
    assert rc == 0 and intact
    _same(outs, law.unique_rows(*good, "set"), "after the refusal (C ABI): ")
    _check(good, "set", "wave+workgroup", "after the refusal: ")


def test_sample_ptr_on_the_device_that_does_not_end_at_the_rows():
    nodes, ei, eptr, sptr, esrc, ptr = [a.copy() for a in _good_case()]
    sptr[-1] -= 1
    with pytest.raises(RuntimeError, match="sample_ptr must start at 0"):
        rows.unique_rows(*_dev((nodes, ei, eptr, sptr, esrc)), ptr=torch.from_numpy(ptr))
    _check(_good_case(), "sequence", "wave+workgroup", "after the refusal: ")


# ---- two host threads ----
def test_two_host_threads():
    cases = [law.random_case(np.random.default_rng(31 + t), [64, 200, 3, 900][t:] + [50], 6, distinct=20) for t in range(2)]
    wants = [law.unique_rows(*c, "set") for c in cases]
    errors = []

    def work(t):
        try:
            torch.cuda.set_device(0)
            five = _dev(cases[t][:5])
            for _ in range(8):
                _same(rows.unique_rows(*five, ptr=torch.from_numpy(cases[t][5]), by="set"), wants[t], f"thread {t}: ")
                assert rows.last_launch() == "wave+workgroup"
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---- the job: no sampler's finish takes it, and ugs_job_cancel gives it up ----
def test_job_is_refused_by_the_samplers_finishes_and_can_be_cancelled():
    import ctypes as C

    import ugs_sampler
    from ugs_sampler._lib import UGS_E_BAD_ARG, lib, vp
    case = _good_case()
    nodes, ei, eptr, sptr, esrc = _dev(case[:5])
    ptr = torch.from_numpy(case[5]).to(DEV)
    R, k = nodes.shape
    for _ in range(3):
        ugs_sampler._select_device(torch.device(DEV), jobs=True)
        job, U, Eu = vp(), C.c_int64(), C.c_int64()
        assert lib.ugs_rows_unique_begin(nodes.data_ptr(), k, R, eptr.data_ptr(), ei.size(1), sptr.data_ptr(), sptr.numel() - 1, ptr.data_ptr(), 1,
                                         C.byref(job), C.byref(U), C.byref(Eu)) == 0
        out = torch.full((R * k + R + 8,), 7, dtype=torch.int64, device=DEV)
        for finish in (lib.ugs_sample_batch_finish, lib.ugs_rwr_sample_batch_finish, lib.ugs_uniform_sample_batch_finish, lib.ugs_eps_sample_batch_finish):
            assert finish(job, out.data_ptr(), None, out.data_ptr(), None, None, 1) == UGS_E_BAD_ARG
        assert lib.ugs_sample_finish(job, out.data_ptr(), None, out.data_ptr(), None, 1) == UGS_E_BAD_ARG
        assert lib.ugs_job_cancel(job) == 0
        torch.cuda.synchronize()
        assert bool((out == 7).all())
    assert lib.ugs_rows_unique_finish(None, *([None] * 2), 0, *([None] * 2), 0, *([None] * 5)) == UGS_E_BAD_ARG
    _check(case, "set", "wave+workgroup", "after the cancelled jobs: ")
