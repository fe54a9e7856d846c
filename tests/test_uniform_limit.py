"""CPU: the switch that raises uniform_sampler's vertex limit (ugs_uniform_set_max_vertices; include/ugs_mi355.h) -- its range,
its initial value from the environment, and the mask threshold beside it.  No sampling call is made here."""
import os
import subprocess
import sys

import pytest


def test_setters_keep_their_range_and_return_the_previous_value():
    import uniform_sampler as us
    start = us.max_vertices()
    try:
        assert us.set_max_vertices(512) == start and us.max_vertices() == 512
        for bad in (63, 1025, -5):
            with pytest.raises(RuntimeError, match="64 ... 1024"):
                us.set_max_vertices(bad)
            assert us.max_vertices() == 512
    finally:
        us.set_max_vertices(start)
    assert us._set_mask_vertices(10) == 64 and us._set_mask_vertices(64) == 10
    with pytest.raises(RuntimeError, match="0 ... 64"):
        us._set_mask_vertices(65)
    assert us._set_mask_vertices(64) == 64


@pytest.mark.parametrize("bad", ["63", "1025", "abc", "128x"])
def test_invalid_environment_value_is_ignored_and_reported_under_debug(bad):
    """The library alone (ctypes, no torch): the child is cheap."""
    from ugs_sampler._lib import LIB_PATH
    code = "import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).ugs_uniform_max_vertices())"
    env = dict(os.environ, UGS_UNIFORM_MAX_VERTICES=bad, UGS_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code, LIB_PATH], env=env, capture_output=True, text=True, check=True)
    assert r.stdout.split() == ["64"]
    assert "UGS_UNIFORM_MAX_VERTICES=" + bad + " ignored" in r.stderr
    env["UGS_DEBUG"] = "0"
    r = subprocess.run([sys.executable, "-c", code, LIB_PATH], env=env, capture_output=True, text=True, check=True)
    assert r.stdout.split() == ["64"] and "UGS_UNIFORM_MAX_VERTICES" not in r.stderr
