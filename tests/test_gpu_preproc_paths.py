"""GPU: the device preprocessing kernels (csrc/ugs_preproc.hip) path by path, one named input per path: the key width with the
sentinel key at powers of two, every kind of skipped column, the block edges of every launch, the row order of repeated columns
and loops, the bounded breadth-first search at k - 1 / k / k + 1 reachable vertices, the relaxation levels, k above the
kernel's list (which the host stages must take), and the plan assembly from a graph's device CSR.

The inputs live in tests/preproc_paths.py.  Every case first asserts by the census of the law (preproc_law.census, CPU) that
its input reaches the path it is there for -- if that fails the input is wrong, not the kernel -- then forces the device path,
asserts by preproc_stats() that this graph went through it (or, for k > 32, through the host stages), and compares preproc_dump
and get_preproc_info with tests/preproc_law.py and the oracle exactly.  The assembly cases read the plan's rows (Plan.graph_csr)
and root records (Plan.graph_roots) back.  tests/test_preproc_law.py shows on a CPU model of the kernels that these inputs tell
each modelled slip from the law."""
import os

import numpy as np
import pytest
import torch

import oracle
import preproc_law as L
import preproc_paths as P

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "edge_index", "edge_ptr", "sample_ptr", "edge_src")
ENV = ("UGS_DEVICE_PREPROC", "UGS_DEVICE_BATCH")
M = 9


class Setting:
    """UGS_DEVICE_PREPROC / UGS_DEVICE_BATCH for a block of calls, restored on exit; the product's caches are cleared on entry and exit"""

    def __init__(self, preproc="1", batch=None):
        self.env = dict(zip(ENV, (preproc, batch)))

    def __enter__(self):
        import ugs_sampler
        self.prev = {v: os.environ.get(v) for v in ENV}
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
        self.put(self.prev)
        ugs_sampler.clear_cache()


def stats():
    import ugs_sampler
    s = ugs_sampler.preproc_stats()
    return np.array([s["device_graphs"], s["host_graphs"], s["device_pieces"]])


def oracle_dump(ei, n, k):
    pre = oracle.Preproc(ei, n, k)
    d, info = pre.dump(), pre.info()
    pre.close()
    return d, info


@pytest.mark.parametrize("name", [c.name for c in P.cases()])
def test_path_equals_law_and_oracle(name):
    import ugs_sampler
    c, law, census = P.case(name), P.law_of(name), P.census_of(name)
    for cls in c.reaches:
        assert census[cls] > 0, f"the input no longer reaches {cls!r}: choose it again (census: {dict(census)})"
    want, winfo = oracle_dump(c.ei, c.n, c.k)
    with Setting("1"):
        s0 = stats()
        h = ugs_sampler.create_preproc(torch.from_numpy(c.ei), c.n, c.k)
        s1 = stats()
        d, info, has = ugs_sampler.preproc_dump(h), ugs_sampler.get_preproc_info(h), ugs_sampler.has_graphlets(h)
        ugs_sampler.destroy_preproc(h)
    # exactly this graph, through the kernels -- or, above the kernel's list, through the host stages
    assert (s1 - s0).tolist() == ([1, 0, 0] if c.k <= L.KMAX else [0, 1, 0]), (name, s0, s1)
    for f in ("indptr", "indices", "edge_col", "order", "index_of", "suffix_deg", "bucket_b"):
        assert d[f].dtype == law[f].dtype and np.array_equal(d[f], law[f]), (name, f, "law")
    for f in want:
        assert np.array_equal(d[f], want[f]), (name, f, "oracle")           # incl. Z and the alias table's doubles
    assert info == L.info_of(law) == {x: winfo[x] for x in info} and has == winfo["has_graphlets"] == (law["level"] == 0), name


def check_graph(plan, g, n, e, k, colmap, what):
    """graph g of the plan against the law of (n, e, k) and the oracle's root records"""
    csr = plan.graph_csr(g)
    if n <= 0 or (colmap is not None and n < k):
        assert csr["num_nodes"] == 0 and csr["num_entries"] == 0, what
        return
    law = L.graph_law(e, n, k)
    want = L.plan_arrays(law, colmap)
    assert csr["num_nodes"] == n and csr["num_entries"] == len(law["indices"]), what
    for f in want:
        assert np.array_equal(csr[f], want[f]), (what, f)
    d, _ = oracle_dump(e, n, k)
    got = plan.graph_roots(g, n)
    assert got["level"] == law["level"] and got["num_nodes"] == n, (what, got["level"], law["level"])
    if law["level"] == 0:
        assert np.array_equal(got["prob"], d["prob"]) and np.array_equal(got["alias"], d["alias"]), (what, "alias table")   # doubles bit for bit
        assert np.array_equal(got["v_self"], d["order"]) and np.array_equal(got["v_alias"], d["order"][d["alias"]]), (what, "root vertices")
    else:
        nv = len(law["viable_vi"])
        assert got["num_viable"] == nv and np.array_equal(got["viable_vi"][:nv], law["viable_vi"]) and np.array_equal(got["viable_v"][:nv], law["viable_v"]), what


@pytest.mark.parametrize("name", ["roots_k3", "kw_n256", "repeated_both_ways", "loops_only", "all_skipped", "n_lt_k", "nnz_258"])
def test_plan_from_a_device_preprocessed_handle(name):
    """the first plan of a fresh device-preprocessed handle is a split plan without a column map: its rows are written by
    pre_assemble from the CSR the graph left in HBM.  The handle keeps that plan: asking again hands out the same arrays and
    writes nothing."""
    import ugs_sampler
    c = P.case(name)
    with Setting("1"):
        s0 = stats()
        h = ugs_sampler.create_preproc(torch.from_numpy(c.ei), c.n, c.k)
        try:
            assert (stats() - s0).tolist() == [1, 0, 0], name
            plan = ugs_sampler.Plan.from_handle(h, c.k)
            try:
                assert (stats() - s0).tolist() == [1, 0, 1], name
                check_graph(plan, 0, c.n, c.ei, c.k, None, (name, "first plan"))
                again = ugs_sampler.Plan.from_handle(h, c.k)
                try:
                    assert (stats() - s0).tolist() == [1, 0, 1], name
                    check_graph(again, 0, c.n, c.ei, c.k, None, (name, "second plan"))
                finally:
                    again.close()
            finally:
                plan.close()
        finally:
            ugs_sampler.destroy_preproc(h)


@pytest.mark.parametrize("name", [b.name for b in P.batches()])
def test_plan_assembled_piece_by_piece(name):
    """a batch through the general path with the device preprocessing forced: fresh graphs are pieces written by pre_assemble (with
    the column map, or without it where it is the identity), a graph the LRU holds from a host-path call and a graph without
    columns are copied from the host into the same split plan, a graph without vertices has no piece.  A second batch of the same
    graphs finds every device copy taken: nothing is written by the kernel, the rows are the same."""
    import ugs_sampler
    b = P.batch(name)
    ei, ptr = P.batch_arrays(b)
    kinds = P.batch_census(b)
    n_dev = sum(k.startswith("device piece") for k in kinds)
    n_empty = kinds.count("host piece: graph without columns")
    assert n_dev >= 2 and "host piece: graph held by the LRU" in kinds
    te, tp = torch.from_numpy(ei), torch.from_numpy(ptr)

    def check(plan, ei, ptr, what):
        for g in range(len(ptr) - 1):
            n, e, cm = P.local_graph(ei, ptr, g)
            check_graph(plan, g, n, e, b.k, cm, what + (g,))

    with Setting("0", "0") as st:
        for g in b.cached:                                                   # into the LRU by the host stages, its columns in the batch's order
            n, e, _ = P.local_graph(ei, ptr, g)
            s0 = stats()
            ugs_sampler.Plan.from_batch(torch.from_numpy(np.ascontiguousarray(e)), torch.tensor([0, n]), b.k).close()
            assert (stats() - s0).tolist() == [0, 1, 0], name
        st.put({"UGS_DEVICE_PREPROC": "1"})
        s0 = stats()
        plan = ugs_sampler.Plan.from_batch(te, tp, b.k)
        try:
            assert (stats() - s0).tolist() == [n_dev, n_empty, n_dev], (name, kinds)
            check(plan, ei, ptr, (name, "first"))
        finally:
            plan.close()
        # the same columns as another batch (a graph without vertices in front): another plan, every graph's own columns unchanged
        ptr2 = np.concatenate([[0], ptr]).astype(np.int64)
        s0 = stats()
        plan = ugs_sampler.Plan.from_batch(te, torch.from_numpy(ptr2), b.k)
        try:
            assert (stats() - s0).tolist() == [0, 0, 0], name                 # every graph an LRU hit, every device copy taken
            check(plan, ei, ptr2, (name, "second"))
        finally:
            plan.close()
        for mode in ("sample", "global"):
            ugs_sampler.clear_cache()                                        # every graph with a column fresh again: all through the kernels
            s0 = stats()
            got = ugs_sampler.sample_batch(te, tp, M, b.k, mode, 42)
            fresh = n_dev + len(b.cached)
            assert (stats() - s0).tolist() == [fresh, n_empty, fresh], (name, mode)
            want = oracle.sample_batch(ei, ptr, M, b.k, mode, 42)
            for nm, a, w in zip(NAMES, got, want):
                assert np.array_equal(a.numpy(), np.asarray(w)), (name, mode, nm)
