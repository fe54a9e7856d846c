"""rwr_sampler's kernel paths (ugs_rwr.hip), one input per path: CSR in LDS / in global memory at the bound, the speculation cap
and lane 0's redo, the window's edges, the block-wide closed form of doomed walks at its lane and round boundaries, the four KM
instantiations, the union-find threshold, the sort width, rows across blocks, host threads and overlapping jobs.

The inputs live in tests/rwr_paths.py.  Every case first asserts by the census of the law (rwr_law.census, CPU) that its input
reaches the path it is there for -- if that fails the input is wrong, not the kernel -- and then compares all five tensors with
tests/rwr_law.py, bit for bit.  tests/test_rwr_law.py shows on a CPU model of rwr_resolve that these inputs tell each modelled
slip in those lines from the law."""
import ctypes as C
import random
import threading

import numpy as np
import pytest
import torch

import rwr_law as R
import rwr_paths as P

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
GRAPH_MODE_TOO = ("cap_s8_m24", "km_k9", "nv256", "mixed20_s1451", "placement")
M64 = (1 << 64) - 1


def sampler():
    import rwr_sampler
    return rwr_sampler


def assert_same(got, want, what=""):
    for nm, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy() if torch.is_tensor(a) else a
        assert a.dtype == np.int64 and a.shape == b.shape, (what, nm, a.shape, b.shape)
        assert np.array_equal(a, b), (what, nm)


def run(c, mode, m=None, k=None):
    """The case through rwr_sampler: sample_graphs when it carries per-graph seeds, sample_batch otherwise."""
    e, q = torch.from_numpy(c.ei), torch.from_numpy(c.ptr)
    m, k = c.m if m is None else m, c.k if k is None else k
    if c.seeds is None:
        return sampler().sample_batch(e, q, m, k, mode=mode, seed=c.seed, p_restart=c.p)
    out = sampler().sample_graphs(e, q, m, k, list(c.seeds), mode=mode, p_restart=c.p)
    assert len(out) == 6 and not out[5].any()
    return out[:5]


@pytest.mark.parametrize("name", [c.name for c in P.cases()])
def test_path_equals_law(name):
    c = P.case(name)
    census = P.census_of(name)
    for cls in c.reaches:
        assert census[cls] > 0, f"the input no longer reaches {cls!r}: choose it again (census: {dict(census)})"
    for mode in ("sample", "global") + (("graph",) if name in GRAPH_MODE_TOO else ()):
        assert_same(run(c, mode), P.law_of(name, mode), (name, mode))
    if name.startswith("components_"):
        first = P.law_of(name, "sample")[0][:, 0]
        assert (first >= 0).any() and (first < 0).any()             # rows seeded in the k-path and rows seeded below it


def test_rwr_from_host_threads_beside_the_packed_sampler():
    """Four threads call rwr_sampler (sample_batch and sample_graphs in turn) on four inputs that take different paths -- all
    walks doomed, CSR in global memory, KM = 64, m = 0 -- while a fifth runs packed ugs_sampler.sample_batch calls; every thread
    interleaves a refused call (k = 65).  The expected tensors come from the laws, computed first on this thread."""
    import oracle
    import ugs_sampler
    import ugs_workloads as wl
    torch.cuda.set_device(0)
    ugs_sampler.clear_cache()
    inputs = []
    for name, m in (("doomed91_s3", None), ("placement", None), ("km_k33", None), ("rows_across_blocks", 0)):
        c = P.case(name)
        m = c.m if m is None else m
        want = P.law_of(name, "sample") if m == c.m else R.sample_batch(c.ei, c.ptr, m, c.k, "sample", c.seed, c.p)
        seeds = [(c.seed + g) & M64 for g in range(len(c.ptr) - 1)]  # sample_graphs with the seeds sample_batch gives the graphs
        inputs.append((torch.from_numpy(c.ei), torch.from_numpy(c.ptr), m, c.k, c.seed, c.p, seeds, [torch.from_numpy(np.array(a)) for a in want]))
    pk_ei, pk_ptr = wl.tu_batch(18, 20, 16)
    pk_in = (torch.from_numpy(pk_ei), torch.from_numpy(pk_ptr))
    pk_want = {s: [torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))) for a in oracle.sample_batch(pk_ei, pk_ptr, 8, 4, "sample", s)]
               for s in range(3)}
    barrier, bad, done = threading.Barrier(5), [], []

    def refused(tid, i, e, q):
        try:
            sampler().sample_batch(e, q, 2, 65)
            bad.append((tid, i, "k = 65 was not refused"))
        except RuntimeError as err:
            if "k must be <= 64" not in str(err):
                bad.append((tid, i, str(err)))

    def work(tid):
        try:
            barrier.wait(timeout=60)
            r = random.Random(6000 + tid)
            for i in range(40):
                if tid < 4:
                    e, q, m, k, seed, p, seeds, want = inputs[tid]
                    if i % 2:
                        got = sampler().sample_graphs(e, q, m, k, seeds, p_restart=p)[:5]
                    else:
                        got = sampler().sample_batch(e, q, m, k, seed=seed, p_restart=p)
                else:
                    e, q = pk_in
                    s = r.randrange(3)
                    got, want = ugs_sampler.sample_batch(e, q, 8, 4, mode="sample", seed=s), pk_want[s]
                diff = [nm for nm, a, b in zip(NAMES, got, want) if not torch.equal(a, b)]
                if diff:
                    bad.append((tid, i, diff))
                if i % 8 == 3:
                    refused(tid, i, e, q)
            done.append(tid)
        except BaseException as err:                                 # (an exception is a finding: recorded, the thread ends)
            bad.append((tid, "exception", repr(err)))

    ts = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(5)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "threads did not finish"
    assert not bad, f"{len(bad)} mismatches / exceptions, first: {bad[:6]}"
    assert sorted(done) == list(range(5))


# ---- overlapping jobs through the C ABI (the helpers follow tests/test_gpu_job_kinds.py) ----
def begin(kind, ei, ptr, m, k, seed):
    import ugs_sampler
    from ugs_sampler._lib import lib, vp
    head = (ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(ptr) - 1, m, k, 0, C.c_uint64(seed))
    job, total = vp(), C.c_int64()
    ugs_sampler._select_device(None, jobs=True)
    if kind == "uniform":
        rc = lib.ugs_uniform_sample_batch_begin(*head, C.byref(job), C.byref(total))
    else:
        rc = lib.ugs_rwr_sample_batch_begin(*head, C.c_double(0.2), C.byref(job), C.byref(total))
    assert rc == 0, lib.ugs_last_error()
    assert job.value
    return job, total.value


def finish(fn, job, total, G, m, k):
    from ugs_sampler._lib import lib
    B = G * m
    out = [np.full(s, -7, np.int64) for s in ((B, k), (2, total), (B + 1,), (G + 1,), (total,))]
    assert fn(job, *[a.ctypes.data for a in out], 0) == 0, lib.ugs_last_error()
    return out


def test_overlapping_jobs_finish_in_another_order():
    """Two rwr jobs of different sizes (two blobs of the pool) and a uniform job open at once; B, C and A finish in that order,
    with a fourth job begun and cancelled in between.  Each result is its package's own sample_batch, and the rwr ones the law's."""
    import uniform_sampler
    import ugs_workloads as wl
    from ugs_sampler._lib import lib
    spec = {"A": ("rwr", wl.tu_batch(18, 20, 2), 2, 3, 42), "B": ("rwr", wl.tu_batch(39, 73, 5, dataset_seed=2), 7, 6, 5),
            "C": ("uniform", wl.tu_batch(14, 18, 3, dataset_seed=1), 4, 4, 9), "D": ("rwr", wl.tu_batch(12, 14, 4, dataset_seed=3), 5, 4, 1)}
    spec = {key: (kind, np.ascontiguousarray(ei, dtype=np.int64), np.ascontiguousarray(ptr, dtype=np.int64), m, k, seed)
            for key, (kind, (ei, ptr), m, k, seed) in spec.items()}
    package = {"rwr": sampler(), "uniform": uniform_sampler}
    want = {key: [t.numpy().copy() for t in package[kind].sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, mode="sample", seed=seed)]
            for key, (kind, ei, ptr, m, k, seed) in spec.items()}
    for key in ("A", "B"):
        _, ei, ptr, m, k, seed = spec[key]
        assert_same(want[key], R.sample_batch(ei, ptr, m, k, "sample", seed, 0.2), key)
    fns = {"rwr": lib.ugs_rwr_sample_batch_finish, "uniform": lib.ugs_uniform_sample_batch_finish}
    jobs = {key: begin(spec[key][0], *spec[key][1:]) for key in ("A", "B", "C")}

    def done(key):
        kind, _, ptr, m, k, _ = spec[key]
        got = finish(fns[kind], *jobs[key], len(ptr) - 1, m, k)
        for a, b in zip(got, want[key]):
            assert a.shape == b.shape and np.array_equal(a, b), key

    done("B")
    jobs["D"] = begin(spec["D"][0], *spec["D"][1:])
    done("C")
    assert lib.ugs_job_cancel(jobs["D"][0]) == 0
    done("A")
    _, ei, ptr, m, k, seed = spec["D"]                               # the pool is as it was: the cancelled job's call again
    assert_same(sampler().sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), m, k, seed=seed), want["D"], "D")
