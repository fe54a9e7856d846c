"""CPU: the law of rows.unique_rows as tests/rows_unique_law.py states it -- its invariants on random inputs, agreement with
torch.unique on sorted rows for the number of kept rows, and every refusal the Python side makes before any device work."""
import numpy as np
import pytest
import torch

import rows_unique_law as law
from ugs_sampler import rows

CASES = [([5, 0, 17, 1, 64, 9], 6), ([100, 3], 5), ([0, 0], 3), ([40], 1), ([12, 30], 9), ([7, 7, 7], 32), ([130], 2)]


def _keys(nodes, by):
    return [law.row_key(r, by) for r in nodes]


@pytest.mark.parametrize("by", ["set", "sequence"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_invariants(case, by):
    rows_per_graph, k = CASES[case]
    rng = np.random.default_rng(100 + case)
    nodes, ei, eptr, sptr, esrc, ptr = law.random_case(rng, rows_per_graph, k)
    nu, eiu, epu, spu, esu, count, inverse = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, by)
    R, U = nodes.shape[0], nu.shape[0]
    assert count.sum() == R and count.min(initial=1) >= 1
    assert spu[0] == 0 and spu[-1] == U and (np.diff(spu) >= 0).all()
    # kept rows: first of their key in their graph, in order, unchanged
    graph_of = np.repeat(np.arange(len(rows_per_graph)), rows_per_graph)
    seen, kept = set(), []
    for r in range(R):
        key = (graph_of[r], law.row_key(nodes[r], by))
        if key not in seen:
            seen.add(key)
            kept.append(r)
    assert U == len(kept)
    assert np.array_equal(inverse[kept], np.arange(U))
    assert np.array_equal(nu, nodes[kept].reshape(U, k))
    assert _keys(nu[inverse], by) == _keys(nodes, by)
    assert np.array_equal(np.bincount(inverse, minlength=U), count)
    # rows of different graphs never merge
    assert all(spu[graph_of[r]] <= inverse[r] < spu[graph_of[r] + 1] for r in range(R))
    # edge spans are copied whole
    assert epu[0] == 0 and epu[-1] == eiu.shape[1] == esu.shape[0]
    for u, r in enumerate(kept):
        assert np.array_equal(eiu[:, epu[u]:epu[u + 1]], ei[:, eptr[r]:eptr[r + 1]])
        assert np.array_equal(esu[epu[u]:epu[u + 1]], esrc[eptr[r]:eptr[r + 1]])
    # idempotent
    again = law.unique_rows(nu, eiu, epu, spu, esu, ptr, by)
    for a, b in zip(again[:5], (nu, eiu, epu, spu, esu)):
        assert np.array_equal(a, b)
    assert (again[5] == 1).all() and np.array_equal(again[6], np.arange(U))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_kept_rows_agree_with_torch_unique(case):
    rows_per_graph, k = CASES[case]
    rng = np.random.default_rng(200 + case)
    nodes, ei, eptr, sptr, esrc, ptr = law.random_case(rng, rows_per_graph, k)
    for by in ("set", "sequence"):
        spu = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, by)[3]
        t = torch.from_numpy(nodes)
        if by == "set":
            t = t.sort(dim=1).values
        for g in range(len(rows_per_graph)):
            block = t[int(sptr[g]):int(sptr[g + 1])]
            want = torch.unique(block, dim=0).size(0) if block.size(0) else 0
            assert spu[g + 1] - spu[g] == want
        assert law.kept_fraction(nodes, sptr, by) == pytest.approx(spu[-1] / max(nodes.shape[0], 1))


def test_empty_edge_src_gives_empty_edge_src():
    rng = np.random.default_rng(7)
    nodes, ei, eptr, sptr, esrc, ptr = law.random_case(rng, [9, 4], 4, edge_src=False)
    out = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, "set")
    assert out[4].shape == (0,) and out[1].shape[1] == out[2][-1]


def test_set_merges_permutations_and_sequence_does_not():
    nodes = np.array([[3, 1, 2], [1, 2, 3], [3, 1, 2], [-1, -1, -1], [-1, -1, -1], [-1, 1, -1]], dtype=np.int64)
    ei, eptr, esrc = law.with_edges(nodes, np.random.default_rng(1))
    sptr, ptr = np.array([0, 6]), np.array([0, 5])
    s = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, "set")
    q = law.unique_rows(nodes, ei, eptr, sptr, esrc, ptr, "sequence")
    assert s[0].tolist() == [[3, 1, 2], [-1, -1, -1], [-1, 1, -1]] and s[5].tolist() == [3, 2, 1] and s[6].tolist() == [0, 0, 0, 1, 1, 2]
    assert q[0].tolist() == [[3, 1, 2], [1, 2, 3], [-1, -1, -1], [-1, 1, -1]] and q[5].tolist() == [2, 1, 2, 1]


# ---- the refusals of the Python side: before any device work, so they need no GPU ----
def _good():
    rng = np.random.default_rng(5)
    nodes, ei, eptr, sptr, esrc, ptr = law.random_case(rng, [6, 3], 4)
    return [torch.from_numpy(a) for a in (nodes, ei, eptr, sptr, esrc)], torch.from_numpy(ptr)


def _call(five, ptr, **kw):
    return rows.unique_rows(*five, ptr=ptr, **kw)


@pytest.mark.parametrize("which", range(6))
def test_refuses_wrong_dtype_and_non_tensors(which):
    five, ptr = _good()
    args = five + [ptr]
    bad = list(args)
    bad[which] = args[which].to(torch.int32)
    with pytest.raises(TypeError, match="int64"):
        _call(bad[:5], bad[5])
    bad[which] = args[which].numpy()
    with pytest.raises(TypeError, match="torch.Tensor"):
        _call(bad[:5], bad[5])


def test_refuses_wrong_shapes():
    five, ptr = _good()
    nodes, ei, eptr, sptr, esrc = five
    for bad, text in (([nodes.reshape(-1), ei, eptr, sptr, esrc], r"\[R, k\]"), ([nodes, ei.reshape(-1), eptr, sptr, esrc], r"\[2, E\]"),
                      ([nodes, ei[:1], eptr, sptr, esrc], r"\[2, E\]"), ([nodes, ei, eptr[:-1], sptr, esrc], r"\[R \+ 1\]"),
                      ([nodes, ei, eptr, sptr.reshape(1, -1), esrc], r"\[G \+ 1\]"), ([nodes, ei, eptr, sptr, esrc[:-1]], r"\[E\]"),
                      ([nodes, ei, eptr, sptr, esrc.reshape(1, -1)], r"\[E\]")):
        with pytest.raises(ValueError, match=text):
            _call(bad, ptr)
    with pytest.raises(ValueError, match="ptr must have shape"):
        _call(five, ptr[:-1])
    with pytest.raises(ValueError, match="ptr must have shape"):
        _call(five, ptr.reshape(1, -1))


def test_refuses_tensors_on_different_devices():
    five, ptr = _good()
    five[2] = five[2].to("meta")
    with pytest.raises(ValueError, match="one device"):
        _call(five, ptr)
    five, ptr = _good()
    with pytest.raises(ValueError, match="CPU or on a GPU"):
        _call([t.to("meta") for t in five], ptr)


def test_refuses_by_outside_the_two_names():
    five, ptr = _good()
    with pytest.raises(ValueError, match="by must be"):
        _call(five, ptr, by="multiset")
    with pytest.raises(TypeError, match="by must be"):
        _call(five, ptr, by=1)


@pytest.mark.parametrize("k", [0, 33])
def test_refuses_k_out_of_range(k):
    nodes = torch.zeros((2, k), dtype=torch.int64)
    z = torch.zeros((0,), dtype=torch.int64)
    with pytest.raises(ValueError, match="1 <= k <= 32"):
        rows.unique_rows(nodes, torch.zeros((2, 0), dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.tensor([0, 2]), z, ptr=torch.tensor([0, 4]))


def test_refuses_bad_host_pointer_arrays():
    five, ptr = _good()
    nodes, ei, eptr, sptr, esrc = five
    dec = sptr.clone()
    dec[1] = sptr[2] + 1
    short = sptr.clone()
    short[-1] -= 1
    for bad in (dec, short, sptr + 1):
        with pytest.raises(ValueError, match="sample_ptr must start at 0"):
            _call([nodes, ei, eptr, bad, esrc], ptr)
    dec = eptr.clone()
    dec[2] = eptr[-1] + 3
    short = eptr.clone()
    short[-1] += 1
    for bad in (dec, short):
        with pytest.raises(ValueError, match="edge_ptr must start at 0"):
            _call([nodes, ei, bad, sptr, esrc], ptr)
