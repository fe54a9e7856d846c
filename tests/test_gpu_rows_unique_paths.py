"""GPU: every named input of tests/rows_unique_paths.py through ugs_sampler.rows.unique_rows, for both `by` (DESIGN.md section
18.1).  All seven outputs must equal the law (tests/rows_unique_law.py) bit for bit and `last_launch()` the form the census
predicts; the classes a case is there for are asserted again, so an input that drifts off its path fails here too.  Every refusal
is a validation path that returns a status word: the call raises with its message, reports "none", leaves its inputs as they
were, and the same good input right after gives the law's result."""
import numpy as np
import pytest
import torch

import rows_unique_law as law
import rows_unique_paths as P
from ugs_sampler import rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src", "count", "inverse")
GOOD = [c.name for c in P.cases() if c.refusal is None]
REFUSED = [c.name for c in P.cases() if c.refusal is not None]
AFTER = "block_runs"                                                       # the good input that follows every refusal


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _call(c, by):
    nodes, ei, eptr, sptr, esrc, ptr = _dev(c.arrays)
    if c.strided:                                                          # every second column of a buffer twice as wide
        Es = ei.size(1)
        wide = torch.full((2, 2 * Es + 3), -99, dtype=torch.int64, device=DEV)
        wide[:, 0:2 * Es:2] = ei
        ei = wide[:, 0:2 * Es:2]
        assert ei.stride(1) == 2
    return (nodes, ei, eptr, sptr, esrc, ptr), lambda: rows.unique_rows(nodes, ei, eptr, sptr, esrc, ptr=ptr, by=by)


def _same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        a = a.cpu().numpy()
        assert a.dtype == np.int64 and a.shape == b.shape, f"{what}: {name} has shape {a.shape} against the law's {b.shape}"
        assert np.array_equal(a, b), f"{what}: {name} differs from the law"


def _good(name, by, what=""):
    c = P.case(name)
    kind, form, want = P.law_of(name, by)
    assert kind == "ok"
    _, call = _call(c, by)
    got = call()
    assert all(t.is_cuda for t in got)
    assert rows.last_launch() == form, f"{what}{name}"
    _same(got, want, f"{what}{name}, by={by}")


@pytest.mark.parametrize("by", P.BYS)
@pytest.mark.parametrize("name", GOOD)
def test_case_equals_the_law(name, by):
    c = P.case(name)
    census = P.census_of(name, by)
    for cls in P.reaches_for(c, by):
        assert cls in census, (name, cls)
    _good(name, by)


@pytest.mark.parametrize("by", P.BYS)
@pytest.mark.parametrize("name", REFUSED)
def test_refusal_names_the_offender_and_the_next_call_is_good(name, by):
    c = P.case(name)
    census = P.census_of(name, by)
    for cls in c.reaches:
        assert cls in census, (name, cls)
    word, value = law.refusal(c.arrays)
    assert c.refusal == law.refusal_pattern(word, value, c.arrays[0].shape[1])
    given, call = _call(c, by)
    with pytest.raises(RuntimeError, match=c.refusal):
        call()
    torch.cuda.synchronize()
    assert rows.last_launch() == "none"
    for t, a in zip(given, c.arrays):
        assert np.array_equal(t.cpu().numpy(), a), "a refused call changed its inputs"
    _good(AFTER, by, "after the refusal: ")
