"""A job knows which sampler's begin made it: the *_finish of epsilon_uniform, uniform and rwr refuse each other's jobs (the job
survives and its own finish then completes it), the generic ugs_sample_batch_finish takes a job of any kind, and a cancelled job
leaves nothing behind.  All through the C ABI (ugs_sampler._lib.lib), host outputs, compared with the packages' sample_batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import ugs_sampler
import ugs_workloads as wl
from ugs_sampler._lib import UGS_E_BAD_ARG, lib, vp

pytestmark = pytest.mark.gpu

M, K, SEED = 2, 3, 42
KINDS = ("eps", "uniform", "rwr")
FINISH = {"eps": lib.ugs_eps_sample_batch_finish, "uniform": lib.ugs_uniform_sample_batch_finish, "rwr": lib.ugs_rwr_sample_batch_finish}
REFUSAL = {"eps": "not an epsilon job", "uniform": "not a uniform_sampler job", "rwr": "not an rwr_sampler job"}


def batch():
    ei, ptr = wl.tu_batch(18, 20, 2)
    return np.ascontiguousarray(ei, dtype=np.int64), np.ascontiguousarray(ptr, dtype=np.int64)


def package(kind):
    import epsilon_uniform_sampler
    import rwr_sampler
    import uniform_sampler
    return {"eps": epsilon_uniform_sampler, "uniform": uniform_sampler, "rwr": rwr_sampler}[kind]


def expected(kind):
    ei, ptr = batch()
    return [t.numpy().copy() for t in package(kind).sample_batch(torch.from_numpy(ei), torch.from_numpy(ptr), M, K, mode="sample", seed=SEED)]


def begin(kind):
    """(job, total) of the sampler's begin on the batch, as its sample_batch calls it (mode "sample", default epsilon / p_restart)"""
    ei, ptr = batch()
    head = (ei.ctypes.data, ei.shape[1], ei.shape[1], ptr.ctypes.data, len(ptr) - 1, M, K, 0, C.c_uint64(SEED))
    job, total = vp(), C.c_int64()
    ugs_sampler._select_device(None, jobs=True)
    if kind == "eps":
        rc = lib.ugs_eps_sample_batch_begin(*head, C.c_double(0.1), C.byref(job), C.byref(total))
    elif kind == "uniform":
        rc = lib.ugs_uniform_sample_batch_begin(*head, C.byref(job), C.byref(total))
    else:
        rc = lib.ugs_rwr_sample_batch_begin(*head, C.c_double(0.2), C.byref(job), C.byref(total))
    assert rc == 0, lib.ugs_last_error()
    assert job.value
    return job, total.value


def outputs(total):
    G, B = 2, 2 * M
    return [np.full(s, -7, np.int64) for s in ((B, K), (2, total), (B + 1,), (G + 1,), (total,))]


def finish(fn, job, out):
    return fn(job, *[a.ctypes.data for a in out], 0)


def assert_same(got, want, what):
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b), what


@pytest.mark.parametrize("kind", KINDS)
def test_the_other_samplers_finish_refuses_the_job_and_its_own_completes_it(kind):
    want = expected(kind)
    job, total = begin(kind)
    out = outputs(total)
    for other in KINDS:
        if other == kind:
            continue
        assert finish(FINISH[other], job, out) == UGS_E_BAD_ARG
        assert lib.ugs_last_error().decode() == REFUSAL[other]
        assert all((a == -7).all() for a in out), "a refused finish wrote to the outputs"
    assert finish(FINISH[kind], job, out) == 0, lib.ugs_last_error()
    assert_same(out, want, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_the_generic_finish_takes_a_job_of_any_kind(kind):
    want = expected(kind)
    job, total = begin(kind)
    out = outputs(total)
    assert finish(lib.ugs_sample_batch_finish, job, out) == 0, lib.ugs_last_error()
    assert_same(out, want, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_a_cancelled_job_leaves_the_sampler_as_it_was(kind):
    want = expected(kind)
    job, _ = begin(kind)
    assert lib.ugs_job_cancel(job) == 0
    assert_same(expected(kind), want, kind + " after a cancelled job")
