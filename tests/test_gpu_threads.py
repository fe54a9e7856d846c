"""GPU: the library called from several host threads at once.  ctypes releases the GIL, so the
threads really run side by side in the host library: they share the preprocessing LRU, the cached device plans and their
scratch, the pool and the job streams.  Every test computes its expected tensors first, on the main thread, from a plain
reference (the CPU oracle, tests/uniform_law.py, or tests/eps_rows.py, the bit-exact restatement of the epsilon_uniform_sampler
kernels); then 4 to 8 threads start together behind a barrier, draw their calls from
their own random.Random and compare every result bit for bit.  Mismatches and exceptions are collected, and the main thread
asserts that there are none and that every thread finished."""
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("sample", "graph", "global")
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")


def _torch_all(arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))) for a in arrays)


def _differs(got, want, names=NAMES):
    """Names of the tensors of `got` that are not bit for bit those of `want` (CPU tensors)."""
    import torch
    return [nm for nm, g, w in zip(names, got, want) if not torch.equal(g.cpu() if g.is_cuda else g, w)]


def _run_threads(work, n, join_timeout=150.0):
    """Runs work(tid, bad) on n threads released together; `bad` collects mismatches.  Asserts none, no exception, all done."""
    barrier = threading.Barrier(n)
    bad, done = [], []

    def body(tid):
        try:
            barrier.wait(timeout=60)
            work(tid, bad)
            done.append(tid)
        except BaseException as e:          # (an exception is a finding: recorded, the thread ends)
            bad.append((tid, "exception", repr(e)))

    ts = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=join_timeout)
    alive = [i for i, t in enumerate(ts) if t.is_alive()]
    assert not alive, f"threads {alive} did not finish within {join_timeout} s"
    assert not bad, f"{len(bad)} mismatches / exceptions, first: {bad[:6]}"
    assert sorted(done) == list(range(n))


def _small_batches():
    """Batches of small graphs that take the packed step (the shapes of test_drop_in_call_with_the_step_run_in_begin)."""
    import ugs_workloads as wl
    return [(wl.tu_batch(18, 20, 64), 4), (wl.tu_batch(39, 73, 32), 6)]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "two_phase"])
def test_shared_small_batches_drop_in_call(packed, monkeypatch):
    """Six threads call sample_batch on the same two batches (one cached plan each, shared scratch) with m drawn from
    {8, 33, 77} -- the row count changes from call to call, so the plan's scratch is regrown under the other threads -- every
    mode and several seeds.  The packed step runs walk and fill in begin: the fill scans the counts and 8-row sums the walk
    left in the plan's scratch, which another thread's walk must not overwrite in between."""
    import oracle
    import torch
    import ugs_sampler
    if not packed:
        monkeypatch.setenv("UGS_NO_PACKED_STEP", "1")
    torch.cuda.set_device(0)
    ugs_sampler.clear_cache()
    batches = _small_batches()
    ms, seeds = (8, 33, 77), range(4)
    inputs = [(torch.from_numpy(ei), torch.from_numpy(ptr), k) for (ei, ptr), k in batches]
    want = {(b, m, mode, s): _torch_all(oracle.sample_batch(ei, ptr, m, k, mode, s))
            for b, ((ei, ptr), k) in enumerate(batches) for m in ms for mode in MODES for s in seeds}

    def work(tid, bad):
        r = random.Random(1000 + tid)
        for i in range(160):
            b, m, mode, s = r.randrange(len(inputs)), r.choice(ms), r.choice(MODES), r.choice(seeds)
            ei_t, ptr_t, k = inputs[b]
            got = ugs_sampler.sample_batch(ei_t, ptr_t, m, k, mode=mode, seed=s)
            diff = _differs(got, want[(b, m, mode, s)])
            if diff:
                bad.append((tid, i, b, m, mode, s, diff))

    _run_threads(work, 6)


@pytest.mark.parametrize("form", ["shared_plan_default_stream", "twin_per_stream"])
def test_plan_step_from_threads(form):
    """Plan.step from four threads.  shared_plan_default_stream: every thread holds its own Plan.from_batch over the SAME batch,
    so all four share one cached plan and its scratch, and all step on torch's default stream: the fused fill of one thread's step
    must scan its own walk's counts, not those of a walk another thread launched in between.  twin_per_stream: the documented pattern for two steps in flight -- each thread steps through its own
    plan.twin() (private scratch) on its own torch.cuda.Stream.  The edge capacity is 2 * rows * k * (k - 1), which bounds the
    entries of these simple graphs; all four outputs are compared with the oracle."""
    import oracle
    import torch
    import ugs_sampler
    torch.cuda.set_device(0)
    ugs_sampler.clear_cache()
    (ei, ptr), k = _small_batches()[0]
    G = len(ptr) - 1
    ms, seeds = (8, 33, 77), range(4)
    want = {}
    for m in ms:
        for mode in MODES:
            for s in seeds:
                w = oracle.sample_batch(ei, ptr, m, k, mode, s)
                want[(m, mode, s)] = _torch_all((w[0], w[2], w[1], w[4]))
    n = 4
    base = [ugs_sampler.Plan.from_batch(torch.from_numpy(ei), torch.from_numpy(ptr), k) for _ in range(n)]
    plans = [p.twin() for p in base] if form == "twin_per_stream" else base
    streams = [torch.cuda.Stream() for _ in range(n)] if form == "twin_per_stream" else None

    def work(tid, bad):
        r = random.Random(2000 + tid)
        plan = plans[tid]
        stream = streams[tid] if streams else torch.cuda.default_stream()
        for i in range(150):
            m, mode, s = r.choice(ms), r.choice(MODES), r.choice(seeds)
            rows = G * m
            with torch.cuda.stream(stream):
                nodes, eptr, eidx, esrc = plan.step(m, mode, s, edge_capacity=2 * rows * k * (k - 1))
                stream.synchronize()
                tot = int(eptr[-1].item())
                got = (nodes, eptr, eidx[:, :tot], esrc[:tot])
                diff = _differs(got, want[(m, mode, s)], ("nodes", "edge_ptr", "edge_index", "edge_src"))
            if diff:
                bad.append((tid, i, m, mode, s, diff))

    try:
        _run_threads(work, n)
    finally:
        for p in plans + (base if plans is not base else []):
            p.close()


@pytest.mark.parametrize("device_batch", ["1", "0"], ids=["device_batch_pass", "general_path"])
def test_device_outputs_on_per_thread_streams(device_batch, monkeypatch):
    """Four threads, each with its own torch.cuda.Stream, call sample_batch(..., device="cuda:0") inside
    `with torch.cuda.stream(own)`: the job runs on that stream and its outputs come from torch's stream-ordered allocator.  Each
    thread synchronises only its own stream before it compares.  UGS_DEVICE_BATCH=1 slices the batches with the device batch
    pass, =0 with the host's general path."""
    import oracle
    import torch
    import ugs_sampler
    monkeypatch.setenv("UGS_DEVICE_BATCH", device_batch)
    torch.cuda.set_device(0)
    ugs_sampler.clear_cache()
    before = ugs_sampler.batch_pass_stats()
    batches = _small_batches()
    ms, seeds = (8, 33, 77), range(3)
    inputs = [(torch.from_numpy(ei), torch.from_numpy(ptr), k) for (ei, ptr), k in batches]
    want = {(b, m, mode, s): _torch_all(oracle.sample_batch(ei, ptr, m, k, mode, s))
            for b, ((ei, ptr), k) in enumerate(batches) for m in ms for mode in MODES for s in seeds}
    n = 4
    streams = [torch.cuda.Stream() for _ in range(n)]

    def work(tid, bad):
        r = random.Random(3000 + tid)
        own = streams[tid]
        for i in range(100):
            b, m, mode, s = r.randrange(len(inputs)), r.choice(ms), r.choice(MODES), r.choice(seeds)
            ei_t, ptr_t, k = inputs[b]
            with torch.cuda.stream(own):
                got = ugs_sampler.sample_batch(ei_t, ptr_t, m, k, mode=mode, seed=s, device="cuda:0")
            own.synchronize()
            if not all(t.is_cuda for t in got):
                bad.append((tid, i, "host tensor"))
                continue
            diff = _differs([t.cpu() for t in got], want[(b, m, mode, s)])
            if diff:
                bad.append((tid, i, b, m, mode, s, diff))

    _run_threads(work, n)
    after = ugs_sampler.batch_pass_stats()       # (device_plans counts plans the pass built; general_path only its refusals)
    if device_batch == "1":
        assert after["device_plans"] > before["device_plans"], (before, after)
    else:
        assert after == before, (before, after)


def test_mixed_entry_points_at_once(monkeypatch):
    """One thread per entry point, all at once: sample_batch on small graphs (packed step), the handle API
    (create_preproc + sample), uniform_sampler, epsilon_uniform_sampler, the streamed call (_STREAM_MIN_ROWS lowered, many
    chunks), and two threads whose calls must fail -- k = 33 for ugs_sampler, a 65-vertex graph for uniform_sampler.  Each
    failing thread must read its OWN error text (ugs_last_error is thread-local) while the others keep matching their references."""
    import epsilon_uniform_sampler
    import eps_rows
    import oracle
    import torch
    import ugs_sampler
    import ugs_workloads as wl
    import uniform_law as U
    import uniform_sampler
    torch.cuda.set_device(0)
    ugs_sampler.clear_cache()
    # the streamed call for batches of at least 3000 rows, in chunks of 500 rows; every other ugs_sampler call here stays below
    monkeypatch.setattr(ugs_sampler, "_STREAM_MIN_ROWS", 3000)
    monkeypatch.setenv("UGS_STREAM_CHUNK_ROWS", "500")
    streamed_calls = [0]
    real_streamed = ugs_sampler._sample_batch_streamed

    def counting_streamed(*a):
        out = real_streamed(*a)
        if out is not None:
            streamed_calls[0] += 1
        return out
    monkeypatch.setattr(ugs_sampler, "_sample_batch_streamed", counting_streamed)

    seeds = range(3)
    # packed: 16 graphs x m <= 77 = at most 1232 rows
    pk_ei, pk_ptr = wl.tu_batch(39, 73, 16)
    pk_in = (torch.from_numpy(pk_ei), torch.from_numpy(pk_ptr))
    pk_want = {(m, mode, s): _torch_all(oracle.sample_batch(pk_ei, pk_ptr, m, 6, mode, s)) for m in (8, 77) for mode in MODES for s in seeds}
    # handle API: one graph, 200 rows
    h_ei = wl.tu_graph(30, 45, 5)
    h_handle = ugs_sampler.create_preproc(torch.from_numpy(h_ei), 30, 5)
    P = oracle.Preproc(h_ei, 30, 5)
    h_want = {(em, s): _torch_all(P.sample(200, 5, em, 0, s)) for em in ("local", "flat") for s in seeds}
    P.close()
    # uniform_sampler: the CPU restatement of its law
    u_ei, u_ptr = wl.tu_batch(14, 18, 6)
    u_in = (torch.from_numpy(u_ei), torch.from_numpy(u_ptr))
    u_want = {(mode, s): _torch_all(U.sample_batch(u_ei, u_ptr, 40, 4, mode, s)) for mode in ("sample", "global") for s in seeds}
    # epsilon_uniform_sampler: the restatement of its kernels, which the single-threaded result equals too
    e_ei, e_ptr = wl.tu_batch(16, 22, 6)
    e_in = (torch.from_numpy(e_ei), torch.from_numpy(e_ptr))
    e_want = {s: _torch_all(eps_rows.sample_rows(e_ei, e_ptr, 50, 4, "sample", s, 0.2)) for s in seeds}
    for s in seeds[:2]:
        assert all(torch.equal(a, b) for a, b in zip(epsilon_uniform_sampler.sample_batch(*e_in, 50, 4, "sample", s, 0.2), e_want[s]))
    # streamed: 8 graphs x 400 rows = 3200 rows, 7 chunks; the expected totals are primed so that every call streams
    st_ei, st_ptr = wl.tu_batch(25, 40, 8)
    st_in = (torch.from_numpy(st_ei), torch.from_numpy(st_ptr))
    st_want = {s: _torch_all(oracle.sample_batch(st_ei, st_ptr, 400, 5, "sample", s)) for s in seeds}
    monkeypatch.setitem(ugs_sampler._stream_totals, (st_ei.shape[1], len(st_ptr) - 1, 400, 5, "sample"), max(int(w[2][-1]) for w in st_want.values()))
    # failing calls
    big_ei, big_ptr = torch.from_numpy(wl.tu_graph(65, 70, 1)), torch.tensor([0, 65])

    def packed(r):
        m, mode, s = r.choice((8, 77)), r.choice(MODES), r.choice(seeds)
        return ugs_sampler.sample_batch(*pk_in, m, 6, mode=mode, seed=s), pk_want[(m, mode, s)]

    def handle(r):
        em, s = r.choice(("local", "flat")), r.choice(seeds)
        return ugs_sampler.sample(h_handle, 200, 5, em, 0, s), h_want[(em, s)]

    def uniform(r):
        mode, s = r.choice(("sample", "global")), r.choice(seeds)
        return uniform_sampler.sample_batch(*u_in, 40, 4, mode=mode, seed=s), u_want[(mode, s)]

    def eps(r):
        s = r.choice(seeds)
        return epsilon_uniform_sampler.sample_batch(*e_in, 50, 4, "sample", s, 0.2), e_want[s]

    def streamed(r):
        s = r.choice(seeds)
        return ugs_sampler.sample_batch(*st_in, 400, 5, mode="sample", seed=s), st_want[s]

    def k33(r):
        ugs_sampler.sample_batch(*pk_in, 8, 33, mode="sample", seed=r.randrange(9))

    def v65(r):
        uniform_sampler.sample_batch(big_ei, big_ptr, 5, 3, mode="sample", seed=r.randrange(9))

    ok_kinds = [packed, handle, uniform, eps, streamed]
    fail_kinds = [(k33, "k > 32 is not supported"), (v65, "graphs of more than 64 vertices")]
    calls = {packed: 150, handle: 150, uniform: 100, eps: 100, streamed: 60, k33: 300, v65: 300}

    def work(tid, bad):
        r = random.Random(4000 + tid)
        if tid < len(ok_kinds):
            fn = ok_kinds[tid]
            for i in range(calls[fn]):
                got, want = fn(r)
                diff = _differs(got, want, NAMES if len(want) == 5 else ("nodes", "edge_index", "edge_ptr", "edge_src"))
                if diff:
                    bad.append((fn.__name__, i, diff))
        else:
            fn, text = fail_kinds[tid - len(ok_kinds)]
            for i in range(calls[fn]):
                try:
                    fn(r)
                    bad.append((fn.__name__, i, "no error"))
                except RuntimeError as e:
                    if text not in str(e):
                        bad.append((fn.__name__, i, str(e)))

    try:
        _run_threads(work, len(ok_kinds) + len(fail_kinds))
    finally:
        ugs_sampler.destroy_preproc(h_handle)
    assert streamed_calls[0] == calls[streamed], streamed_calls
    # the library stays usable on this thread too
    got = ugs_sampler.sample_batch(*pk_in, 8, 6, mode="sample", seed=0)
    assert not _differs(got, pk_want[(8, "sample", 0)])


def test_lru_churn_under_threads():
    """UGS_CACHE_SIZE=2 (read once per process: a subprocess) and six distinct batches of small graphs, sampled by four threads:
    graphs are evicted and preprocessed again all the time, also while another thread's job still holds a plan built over them.
    Every graph has far fewer than 1000 columns, so its LRU key covers its whole content, and the whole process uses one k: a
    cache hit then returns the preprocessing a miss would build, so every call's rows are the oracle's with a fresh cache,
    whatever the interleaving of the threads."""
    code = r'''
import os, sys, random, threading
os.environ["UGS_CACHE_SIZE"] = "2"
sys.path[:0] = [os.path.join(os.getcwd(), p) for p in ("tests", "oracle", "ss-gnn_amd")]
import numpy as np, torch
import oracle, ugs_sampler, ugs_workloads as wl
torch.cuda.set_device(0)
k = 5
batches = [wl.tu_batch(n, e, G, dataset_seed=d) for n, e, G, d in
           ((12, 15, 6, 1), (18, 20, 4, 2), (25, 40, 3, 3), (12, 15, 5, 4), (30, 45, 4, 5), (18, 22, 6, 6))]
for ei, ptr in batches:
    assert all(((ei[0] >= ptr[g]) & (ei[0] < ptr[g + 1])).sum() <= 1000 for g in range(len(ptr) - 1))
inputs = [(torch.from_numpy(ei), torch.from_numpy(ptr)) for ei, ptr in batches]
modes, seeds, m = ("sample", "graph", "global"), range(3), 24
want = {(b, mode, s): tuple(torch.from_numpy(np.asarray(a, dtype=np.int64)) for a in oracle.sample_batch(ei, ptr, m, k, mode, s))
        for b, (ei, ptr) in enumerate(batches) for mode in modes for s in seeds}
bar, bad, done = threading.Barrier(4), [], []
def work(tid):
    try:
        bar.wait(timeout=60)
        r = random.Random(5000 + tid)
        for i in range(150):
            b, mode, s = r.randrange(len(batches)), r.choice(modes), r.choice(seeds)
            got = ugs_sampler.sample_batch(*inputs[b], m, k, mode=mode, seed=s)
            if not all(torch.equal(g, w) for g, w in zip(got, want[(b, mode, s)])):
                bad.append((tid, i, b, mode, s))
        done.append(tid)
    except BaseException as e:
        bad.append((tid, repr(e)))
ts = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(4)]
for t in ts: t.start()
for t in ts: t.join(timeout=150)
assert not any(t.is_alive() for t in ts), "threads did not finish"
assert not bad and sorted(done) == [0, 1, 2, 3], bad[:6]
st = ugs_sampler.cache_stats()
assert st["size"] <= 2 and st["misses"] > 2 * len(batches), st
print("OK", st)
'''
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=240)
    assert out.returncode == 0 and "OK" in out.stdout, (out.returncode, out.stdout[-1000:], out.stderr[-3000:])
