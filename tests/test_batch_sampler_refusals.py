"""CPU (no GPU needed): what uniform_sampler, rwr_sampler and epsilon_uniform_sampler refuse, and with which words.  The three
refuse different things on purpose -- uniform takes k = 0, rwr takes k up to 64 and eps up to 32, eps clamps a decreasing ptr
where the others reject it -- and every argument check of the library runs before it looks for a device.  So without a GPU a
refused call raises its own message and an accepted one raises "no usable HIP device"; with a GPU the accepted call returns."""
import pytest
import torch

import epsilon_uniform_sampler
import rwr_sampler
import uniform_sampler

SAMPLERS = {"uniform": uniform_sampler, "rwr": rwr_sampler, "eps": epsilon_uniform_sampler}
DEVICE = "no usable HIP device"
EI = [[0, 1, 2, 3, 4], [1, 2, 0, 4, 3]]
PTR = [0, 3, 5]

M_NEG = r"m_per_graph must be >= 0"
K_GE1 = r"k must be >= 1"
K_GT32 = r"k > 32 is not supported by the HIP sampler"
BAD_ARGS = r"bad arguments to sample_batch"
PTR_DECR = r"ptr must be non-decreasing \(graph 1\)"
EI_DTYPE = r"edge_index must be int64"
EI_SHAPE = r"edge_index must have shape \[2, E\]"
SEEDS_LEN = r"seeds must hold one seed per graph \(2\), got 1"
EPSILON = r"epsilon must be in \(0, 1\]"


def i64(x):
    return torch.tensor(x, dtype=torch.int64)


def call(sampler, fn="sample_batch", ei=None, ptr=PTR, m=2, k=2, seeds=(1, 2), **kw):
    mod = SAMPLERS[sampler]
    ei = i64(EI) if ei is None else ei
    if fn == "sample_batch":
        return mod.sample_batch(ei, i64(ptr), m, k, **kw)
    return mod.sample_graphs(ei, i64(ptr), m, k, list(seeds), **kw)


def expect(want, *args, **kw):
    """`want`: the refusal's text, or DEVICE for a call the library accepts"""
    if want == DEVICE and torch.cuda.is_available():
        out = call(*args, **kw)
        assert len(out) in (5, 6) and all(t.dtype in (torch.int64, torch.bool) for t in out)
        return
    with pytest.raises(RuntimeError, match=want):
        call(*args, **kw)


# (case, arguments of call(), expected of uniform / rwr / eps)
TABLE = [
    ("valid", {}, DEVICE, DEVICE, DEVICE),
    ("m=-1", dict(m=-1), M_NEG, M_NEG, M_NEG),
    ("k=0", dict(k=0), DEVICE, K_GE1, K_GE1),
    ("k=-1", dict(k=-1), r"k must be >= 0", K_GE1, K_GE1),
    ("k=33", dict(k=33), DEVICE, DEVICE, K_GT32),
    ("k=65", dict(k=65), DEVICE, r"rwr_sampler: k must be <= 64", K_GT32),
    ("ptr_empty", dict(ptr=[]), BAD_ARGS, BAD_ARGS, BAD_ARGS),
    ("ptr_decreasing", dict(ptr=[0, 3, 2]), PTR_DECR, PTR_DECR, DEVICE),
    ("ei_int32", dict(ei=torch.tensor(EI, dtype=torch.int32)), EI_DTYPE, EI_DTYPE, EI_DTYPE),
    ("ei_E_by_2", dict(ei=i64(EI).t().contiguous()), EI_SHAPE, EI_SHAPE, EI_SHAPE),
    ("graphs_valid", dict(fn="sample_graphs"), DEVICE, DEVICE, DEVICE),
    ("graphs_one_seed", dict(fn="sample_graphs", seeds=(1,)), SEEDS_LEN, SEEDS_LEN, SEEDS_LEN),
    ("graphs_ptr_decreasing", dict(fn="sample_graphs", ptr=[0, 3, 2]), PTR_DECR, PTR_DECR, DEVICE),
]


@pytest.mark.parametrize("sampler", ["uniform", "rwr", "eps"])
@pytest.mark.parametrize("case", [row[0] for row in TABLE])
def test_refusal_table(case, sampler):
    row = next(r for r in TABLE if r[0] == case)
    expect(row[2 + ["uniform", "rwr", "eps"].index(sampler)], sampler, **row[1])


def test_uniform_refuses_a_graph_of_more_than_64_vertices_for_the_call():
    assert uniform_sampler.max_vertices() == 64
    expect(r"graph 1 has 67 vertices; graphs of more than 64 vertices", "uniform", ptr=[0, 3, 70])


def test_uniform_sample_graphs_lets_that_graph_fail_alone():
    assert uniform_sampler.max_vertices() == 64
    expect(DEVICE, "uniform", fn="sample_graphs", ptr=[0, 3, 70])


def test_rwr_refuses_p_restart_nan():
    expect(r"p_restart in \[0,1\]", "rwr", p_restart=float("nan"))


def test_rwr_refuses_an_iteration_limit_past_int():
    expect(r"graph 1 has 40000000 vertices; 10 n k must fit", "rwr", ptr=[0, 3, 40000003], k=6)


def test_eps_refuses_epsilon_zero():
    expect(EPSILON, "eps", epsilon=0.0)
    expect(EPSILON, "eps", fn="sample_graphs", epsilon=0.0)


# two faults in one call: which one is reported (recorded from the code before the job path was unified, not chosen)
def test_eps_sample_batch_checks_dtype_before_epsilon():
    expect(EI_DTYPE, "eps", ei=torch.tensor(EI, dtype=torch.int32), epsilon=0.0)


def test_eps_sample_graphs_checks_epsilon_before_dtype():
    expect(EPSILON, "eps", fn="sample_graphs", ei=torch.tensor(EI, dtype=torch.int32), epsilon=0.0)


@pytest.mark.parametrize("sampler", ["uniform", "rwr"])
def test_m_is_checked_before_k(sampler):
    expect(M_NEG, sampler, m=-1, k=-1)
