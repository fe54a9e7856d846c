"""GPU: the device batch pass's kernel paths (csrc/ugs_batch.hip), one input per path: the fused compaction with empty quarters,
columns over several quarters, kept ballots at their bound and beyond it; the two-kernel variant with spans over several rounds,
waves of many graphs and shared ptr values; the column and vertex bounds with their hand-over to the general path; the key
chain and the strided key; the chunked CSR placement; both searches and the alias loop of ugs_bp_roots with inputs on which
another association of its floating-point formulas gives other doubles.

The inputs live in tests/batch_pass_paths.py.  Every case first asserts by the census of the law (batch_pass_law.census, CPU)
that its input reaches the path it is there for -- if that fails the input is wrong, not the kernel -- then reads the rows the
build kernel wrote (Plan.graph_csr) and the records ugs_bp_roots wrote (Plan.graph_roots) back and compares them with
tests/batch_pass_law.py exactly, and sample_batch with the oracle.  tests/test_batch_pass_law.py shows on a CPU model of the
kernels that these inputs tell each modelled slip from the law."""
import os

import numpy as np
import pytest
import torch

import batch_pass_law as L
import batch_pass_paths as P
import oracle

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
ENV = ("UGS_DEVICE_BATCH", "UGS_BP_FUSED_WORK", "UGS_DEVICE_COLD")
M = 9


class Setting:
    """the column limit and the pass's environment variables for a block of calls, restored on exit; the product's caches are
    cleared on entry and exit"""

    def __init__(self, lim, batch="1", fused_work=None, cold=None):
        self.lim, self.env = lim, dict(zip(ENV, (batch, None if fused_work is None else str(fused_work), cold)))

    def __enter__(self):
        import ugs_sampler
        self.prev_env = {v: os.environ.get(v) for v in ENV}
        self.prev_lim = ugs_sampler.batch_pass_max_cols()
        ugs_sampler.set_batch_pass_max_cols(self.lim)
        self.put(self.env)
        ugs_sampler.clear_cache()
        return self

    @staticmethod
    def put(env):
        for v, x in env.items():
            if x is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = x

    def __exit__(self, *exc):
        import ugs_sampler
        ugs_sampler.set_batch_pass_max_cols(self.prev_lim)
        self.put(self.prev_env)
        ugs_sampler.clear_cache()


def stats():
    import ugs_sampler
    s = ugs_sampler.batch_pass_stats()
    return s["device_plans"], s["general_path"]


def variants(c):
    """(limit, UGS_BP_FUSED_WORK, UGS_DEVICE_COLD) of every run of the case"""
    out = [(c.lim, c.fused_work, "1")]
    if c.both:
        out.append((c.lim, 0, "1"))
    if c.fused_work == 0:
        out.append((c.lim, None, "1"))                               # the same input through the fused kernel
    if c.large_too:
        out.append((L.COLS_CEIL, c.fused_work, "1"))
        if c.both:
            out.append((L.COLS_CEIL, 0, "1"))
    if c.cold_too:
        out.append((c.lim, c.fused_work, "0"))
    return out


def check_graph(plan, g, law, what):
    csr = plan.graph_csr(g)
    if law is None:
        assert csr["num_nodes"] == 0 and csr["num_entries"] == 0, what
        return
    n = law["n"]
    assert csr["num_nodes"] == n and csr["num_entries"] == 2 * law["cn"], what
    assert np.array_equal(csr["rowptr"], law["rowptr"]), what
    for got, want in (("nbr", "nbr"), ("nbr_f", "nbr"), ("nbr_rank", "nbr_rank"), ("nbr_col", "nbr_col")):
        assert np.array_equal(csr[got], law[want]), (what, got)
    got = plan.graph_roots(g, n)
    assert got["level"] == law["level"] and got["num_nodes"] == n, (what, got["level"], law["level"])
    if law["level"] == 0:
        assert got["prob"].tolist() == law["prob"], (what, "prob")                                  # doubles bit for bit
        for name in ("alias", "v_self", "v_alias"):
            assert got[name].tolist() == law[name], (what, name)
    else:
        nv = len(law["viable_vi"])
        assert got["num_viable"] == nv and got["viable_vi"][:nv].tolist() == law["viable_vi"] and got["viable_v"][:nv].tolist() == law["viable_v"], what


@pytest.mark.parametrize("name", [c.name for c in P.cases()])
def test_path_equals_law(name):
    import ugs_sampler
    c = P.case(name)
    census = P.census_of(name)
    for cls in c.reaches:
        assert census[cls] > 0, f"the input no longer reaches {cls!r}: choose it again (census: {dict(census)})"
    laws = P.law_of(name)
    te, tp = torch.from_numpy(c.ei), torch.from_numpy(c.ptr)
    want = {mode: oracle.sample_batch(c.ei, c.ptr, M, c.k, mode, 42) for mode in ("sample", "global")}
    for lim, fused_work, cold in variants(c):
        what = (name, lim, fused_work, cold)
        two = P.census_of(name, "two" if fused_work == 0 else "fused", lim)["two kernels"]
        assert two == (fused_work == 0 or name == "two_kernels_900"), what                       # the variant the run is meant to take
        with Setting(lim, "1", fused_work, cold):
            d0, g0 = stats()
            plan = ugs_sampler.Plan.from_batch(te, tp, c.k)
            try:
                assert stats() == ((d0, g0 + 1) if c.hand_over else (d0 + 1, g0)), what
                for g, law in enumerate(laws):
                    if law is not None or c.ptr[g + 1] - c.ptr[g] <= L.MAX_N:
                        check_graph(plan, g, law, what + (g,))
            finally:
                plan.close()
            for mode in ("sample", "global"):
                ugs_sampler.clear_cache()
                got = ugs_sampler.sample_batch(te, tp, M, c.k, mode, 42)
                for nm, a, b in zip(NAMES, got, want[mode]):
                    assert np.array_equal(a.numpy(), np.asarray(b)), (what, mode, nm)


@pytest.mark.parametrize("name", ["key_63_64_65", "key_strided", "cols_1000", "cols_8192"])
def test_keys_hit_what_the_general_path_cached(name):
    """the general path (UGS_DEVICE_BATCH=0) puts the case's graphs into the LRU under the host's keys; the same graphs at other
    positions of a new batch then go through the pass, whose keys -- and, above 1000 columns, fingerprint words -- must find every
    one of them: as many hits as graphs, no miss, one device-built plan, rows equal to the oracle's"""
    import ugs_sampler
    c = P.case(name)
    G = len(c.ptr) - 1
    graphs = []
    for g, law in enumerate(P.law_of(name)):
        n = int(c.ptr[g + 1] - c.ptr[g])
        graphs.append((n, np.stack([law["lu"], law["lv"]]) if law is not None else np.zeros((2, 0), np.int64)))
    live = sum(1 for law in P.law_of(name) if law is not None)
    ei2, ptr2 = P.batch_of(graphs[::-1], first=3)
    assert live >= 2 and not np.array_equal(ptr2, c.ptr)
    cache = oracle.Cache()
    with Setting(c.lim, "0") as st:
        try:
            want = oracle.sample_batch(c.ei, c.ptr, M, c.k, "sample", 42, cache)
            got = ugs_sampler.sample_batch(torch.from_numpy(c.ei), torch.from_numpy(c.ptr), M, c.k, "sample", 42)
            assert all(np.array_equal(a.numpy(), np.asarray(b)) for a, b in zip(got, want))
            st.put({"UGS_DEVICE_BATCH": "1"})
            s0, (d0, g0) = ugs_sampler.cache_stats(), stats()
            want = oracle.sample_batch(ei2, ptr2, M, c.k, "global", 7, cache)
            got = ugs_sampler.sample_batch(torch.from_numpy(ei2), torch.from_numpy(ptr2), M, c.k, "global", 7)
            s1 = ugs_sampler.cache_stats()
            assert (s1["hits"] - s0["hits"], s1["misses"] - s0["misses"]) == (live, 0), (s0, s1)
            assert stats() == (d0 + 1, g0)
            for nm, a, b in zip(NAMES, got, want):
                assert np.array_equal(a.numpy(), np.asarray(b)), (name, nm)
            assert cache.stats()["hits"] == live
        finally:
            cache.close()
    assert G >= live
