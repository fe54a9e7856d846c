"""rwr_sampler with streams="row" (ugs_rwr.hip, rwr_row_walks) against its law (tests/rwr_row_law.py), bit for bit, all five or
six tensors: one input per kernel path (tests/rwr_row_paths.py; tests/test_rwr_row_law.py asserts on the CPU that each reaches its
path), the two entry forms, both output placements, the prefix property, host threads and overlapping jobs."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import rwr_law as R
import rwr_row_law as RR
import rwr_row_paths as Q

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
M64 = (1 << 64) - 1


def sampler():
    import rwr_sampler
    return rwr_sampler


def assert_same(got, want, what=""):
    assert len(got) == len(want) == 5, what
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        b = b.cpu().numpy() if torch.is_tensor(b) else b
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def run(c, mode, m=None, device=None, **kw):
    """The case through rwr_sampler: sample_graphs when it carries per-graph seeds, sample_batch otherwise."""
    e, q = torch.from_numpy(c.ei), torch.from_numpy(c.ptr)
    if device is not None:
        e, q = e.to(device), q.to(device)
    m = c.m if m is None else m
    kw.setdefault("streams", "row")
    if c.seeds is None:
        return sampler().sample_batch(e, q, m, c.k, mode=mode, seed=c.seed, p_restart=c.p, **kw)
    out = sampler().sample_graphs(e, q, m, c.k, list(c.seeds), mode=mode, p_restart=c.p, **kw)
    assert len(out) == 6 and out[5].dtype == torch.bool and not out[5].any() and out[5].device == out[0].device
    return out[:5]


@pytest.mark.parametrize("name", [c.name for c in Q.cases()])
def test_path_equals_row_law(name):
    c = Q.case(name)
    census = Q.census_of(name)
    for cls in c.reaches:
        assert census[cls] > 0, f"the input no longer reaches {cls!r}: choose it again (census: {dict(census)})"
    for mode in ("sample", "global"):
        assert_same(run(c, mode), Q.law_of(name, mode), (name, mode))


@pytest.mark.parametrize("name", ["mixed20", "graph_seeds", "T0", "m300"])
def test_host_input_gives_pinned_outputs_and_device_input_device_outputs(name):
    c = Q.case(name)
    host = run(c, "sample")
    assert all(t.device.type == "cpu" and t.is_pinned() for t in host)
    dev = run(c, "sample", device="cuda:0")
    assert all(t.device == torch.device("cuda:0") for t in dev)
    assert_same(dev, Q.law_of(name, "sample"), name)
    assert_same(host, Q.law_of(name, "sample"), name)


@pytest.mark.parametrize("name", ["graph_seeds", "tree_tail", "mixed20"])
def test_the_first_rows_of_a_longer_call_are_the_shorter_call(name):
    c = Q.case(name)
    G, m, m2 = len(c.ptr) - 1, c.m, 2 * c.m + 37
    short, long = [t.numpy() for t in run(c, "global")], [t.numpy() for t in run(c, "global", m=m2)]
    assert_same(short, Q.law_of(name, "global"), name)
    for g in range(G):
        assert np.array_equal(long[0][g * m2:g * m2 + m], short[0][g * m:(g + 1) * m]), g
        lo, hi, lo2, hi2 = short[2][g * m], short[2][(g + 1) * m], long[2][g * m2], long[2][g * m2 + m]
        assert np.array_equal(long[1][:, lo2:hi2], short[1][:, lo:hi]), g
        assert np.array_equal(long[2][g * m2:g * m2 + m + 1] - lo2, short[2][g * m:(g + 1) * m + 1] - lo), g


@pytest.mark.parametrize("name", ["mixed20", "graph_seeds", "cap_s8"])
def test_streams_graph_is_the_call_without_the_keyword(name):
    c = Q.case(name)
    e, q = torch.from_numpy(c.ei), torch.from_numpy(c.ptr)
    if c.seeds is None:
        plain = sampler().sample_batch(e, q, c.m, c.k, mode="sample", seed=c.seed, p_restart=c.p)
        want = R.sample_batch(c.ei, c.ptr, c.m, c.k, "sample", c.seed, c.p)
    else:
        plain = sampler().sample_graphs(e, q, c.m, c.k, list(c.seeds), mode="sample", p_restart=c.p)[:5]
        want = R.sample_batch(c.ei, c.ptr, c.m, c.k, "sample", 0, c.p, c.seeds)
    assert_same(run(c, "sample", streams="graph"), plain, name)
    assert_same(plain, want, name)
    assert not np.array_equal(plain[0].numpy(), Q.law_of(name, "sample")[0])      # and the two laws give different rows


@pytest.mark.parametrize("streams", ["rows", "", None, "Row", 1])
def test_another_value_of_streams_raises_before_any_device_work(streams):
    c = Q.case("mixed20")
    e, q = torch.from_numpy(c.ei), torch.from_numpy(c.ptr).int()     # (a ptr of the wrong dtype would raise RuntimeError later)
    with pytest.raises(ValueError, match="streams must be 'graph' or 'row'"):
        sampler().sample_batch(e, q, c.m, c.k, streams=streams)
    with pytest.raises(ValueError, match="streams must be 'graph' or 'row'"):
        sampler().sample_graphs(e, q, c.m, c.k, [1], streams=streams)
    with pytest.raises(TypeError):
        sampler().sample_batch(e, q, c.m, c.k, "sample", 42, 0.2, "row")          # keyword-only


def overflowing_batch():
    """Three graphs of the km_k64 kind around an edgeless graph of 3 400 000 vertices (by ptr alone): 10 n k > INT_MAX at k = 64."""
    import rwr_paths as P
    graphs = [P.tu(71, 284, 1), (3_400_000, np.zeros((2, 0), np.int64)), P.tu(64, 256, 2), P.tu(70, 280, 3)]
    return P.batch_of(graphs, first=2)


def test_an_overflowing_graph_fails_alone_with_graph_seeds_and_fails_the_batch_call():
    ei, ptr = overflowing_batch()
    m, k, seeds = 5, 64, [3, (1 << 64) - 1, 3, 77]
    e, q = torch.from_numpy(ei), torch.from_numpy(ptr)
    out = sampler().sample_graphs(e, q, m, k, seeds, mode="global", p_restart=0.1, streams="row")
    assert out[5].tolist() == [False, True, False, False]
    # the law: graph g's block is the one-graph call with seed seeds[g]; the refused graph's block is m rows of -1
    blocks = [RR.sample_batch(ei, ptr[g:g + 2], m, k, "global", seeds[g], 0.1) if g != 1 else None for g in range(4)]
    nodes = np.concatenate([np.full((m, k), -1, np.int64) if b is None else b[0] for b in blocks])
    edges = np.concatenate([b[1] for b in blocks if b is not None], axis=1)
    eptr = [0]
    for b in blocks:
        eptr += [eptr[-1]] * m if b is None else (b[2][1:] + eptr[-1]).tolist()
    want = (nodes, edges, np.array(eptr, np.int64), np.arange(5, dtype=np.int64) * m, np.full(edges.shape[1], -1, np.int64))
    assert_same(out[:5], want, "fails alone")
    assert (nodes[:m, 0] >= 0).any() and (nodes[2 * m:, 0] >= 0).any()
    with pytest.raises(RuntimeError, match=r"graph 1 has 3400000 vertices; 10 n k must fit"):
        sampler().sample_batch(e, q, m, k, streams="row")
    with pytest.raises(RuntimeError, match="k must be <= 64"):
        sampler().sample_batch(e, q, m, 65, streams="row")
    c = Q.case("mixed20")                                           # the library stays usable
    assert_same(run(c, "sample"), Q.law_of("mixed20", "sample"), "after the refusals")


def test_two_host_threads_one_per_streams_value_on_the_same_batch():
    c = Q.case("tree_tail")
    want = {"row": Q.law_of("tree_tail", "sample"), "graph": R.sample_batch(c.ei, c.ptr, c.m, c.k, "sample", c.seed, c.p)}
    e, q = torch.from_numpy(c.ei), torch.from_numpy(c.ptr)
    torch.cuda.set_device(0)
    barrier, bad, done = threading.Barrier(2), [], []

    def work(streams):
        try:
            barrier.wait(timeout=60)
            for i in range(12):
                got = sampler().sample_batch(e, q, c.m, c.k, seed=c.seed, p_restart=c.p, streams=streams)
                diff = [nm for nm, a, b in zip(NAMES, got, want[streams]) if not np.array_equal(a.numpy(), b)]
                if diff:
                    bad.append((streams, i, diff))
            done.append(streams)
        except BaseException as err:                                 # (an exception is a finding: recorded, the thread ends)
            bad.append((streams, "exception", repr(err)))

    ts = [threading.Thread(target=work, args=(s,), daemon=True) for s in ("graph", "row")]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "threads did not finish"
    assert not bad, f"{len(bad)} mismatches / exceptions, first: {bad[:6]}"
    assert sorted(done) == ["graph", "row"]


def test_two_row_jobs_finish_in_reverse_order():
    """Two row-mode jobs open at once through the C ABI (batch form and per-graph-seed form), finished second first."""
    import ugs_sampler
    from ugs_sampler._lib import lib, vp
    a, b = Q.case("m300"), Q.case("graph_seeds")
    ugs_sampler._select_device(None, jobs=True)
    jobs = {}
    for c in (a, b):
        ei, ptr = np.ascontiguousarray(c.ei), np.ascontiguousarray(c.ptr)
        G = len(ptr) - 1
        seeds = None if c.seeds is None else np.array([int(s) & M64 for s in c.seeds], np.uint64)
        status = None if c.seeds is None else np.full(G, -7, np.int32)
        job, total = vp(), C.c_int64()
        rc = lib.ugs_rwr_sample_rows_begin(ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, G, c.m, c.k, 0, C.c_uint64(c.seed),
                                           None if seeds is None else seeds.ctypes.data, C.c_double(c.p),
                                           None if status is None else status.ctypes.data, C.byref(job), C.byref(total))
        assert rc == 0, lib.ugs_last_error()
        assert status is None or not status.any()
        jobs[c.name] = (job, total.value, G, (ei, ptr, seeds, status))
    for c in (b, a):
        job, total, G, _ = jobs[c.name]
        B = G * c.m
        out = [np.full(s, -7, np.int64) for s in ((B, c.k), (2, total), (B + 1,), (G + 1,), (total,))]
        assert lib.ugs_rwr_sample_batch_finish(job, *[x.ctypes.data for x in out], 0) == 0, lib.ugs_last_error()
        assert_same(out, Q.law_of(c.name, "sample"), c.name)
    # the two forms of the entry point check graph_status against seeds
    ei, ptr = np.ascontiguousarray(a.ei), np.ascontiguousarray(a.ptr)
    job, total, status = vp(), C.c_int64(), np.zeros(1, np.int32)
    head = (ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, 1, 2, a.k, 0)
    assert lib.ugs_rwr_sample_rows_begin(*head, C.c_uint64(1), None, C.c_double(0.2), status.ctypes.data, C.byref(job), C.byref(total)) != 0
    one = np.array([1], np.uint64)
    assert lib.ugs_rwr_sample_rows_begin(*head, C.c_uint64(1), one.ctypes.data, C.c_double(0.2), None, C.byref(job), C.byref(total)) != 0
