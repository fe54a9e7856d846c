"""The allocation rule of the three dataset caches (rwr_sampler, ugs_sampler and epsilon_uniform_sampler GraphCache), pinned through
info() after every add: what is used, how many bytes the device storage takes and how many allocations there were.

The rule: a store is a few arrays in capacity groups.  An add that needs more entries of any group than the
generation holds makes a new generation in which every group gets room(need, have, reserve) = have if need <= have, else
max(need, 2 * have, reserve) entries, at least 1.  The expectation comes from a model of that rule written here; only the two
figures of the ugs cache that depend on its preprocessing (csr_entries, bytes) are a table recorded from the library."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 3
RESERVES = [(0, 0), (1, 1), (10, 20)]


def und(n, pairs):
    """(n, columns [2, 2 len(pairs)]): every edge in both directions, as a dataset stores an undirected graph"""
    a = np.array([[u, v] for u, v in pairs] + [[v, u] for u, v in pairs], np.int64).reshape(-1, 2).T
    return n, np.ascontiguousarray(a)


def path(n):
    return und(n, [(i, i + 1) for i in range(n - 1)])


def cycle(n):
    return und(n, [(i, (i + 1) % n) for i in range(n)])


def clique(n):
    return und(n, [(i, j) for i in range(n) for j in range(i + 1, n)])


# one add of a 3-vertex path, then three add_many calls; every graph has at most 8 vertices
ADDS = [
    [path(3)],
    [cycle(5), und(6, [(0, i) for i in range(1, 6)]), und(4, [])],          # the last: a graph without columns
    [und(1, []), clique(4)],                                               # the first: one vertex (degenerate for ugs at k = 3)
    [path(8), clique(3), cycle(7), path(2), clique(5)],                    # path(2): degenerate for ugs at k = 3, with columns
]


def room(need, have, reserve):
    return have if need <= have else max(need, 2 * have, reserve)


class Store:
    """The model: `elem` bytes per entry of each group (summed over the group's arrays), `reserve` entries per group."""

    def __init__(self, elem, reserve):
        self.elem, self.reserve = elem, reserve
        self.used, self.cap, self.generations = [0] * len(elem), None, 0

    def add(self, entries):
        need = [u + e for u, e in zip(self.used, entries)]
        if self.cap is None or any(n > c for n, c in zip(need, self.cap)):
            have = self.cap or [0] * len(need)
            self.cap = [max(room(n, h, r), 1) for n, h, r in zip(need, have, self.reserve)]
            self.generations += 1
        self.used = need

    def bytes(self):
        return sum(c * e for c, e in zip(self.cap, self.elem))


def sizes(graphs):
    return sum(n for n, _ in graphs), sum(a.shape[1] for _, a in graphs)


def run_adds(cache):
    """info() after each of the ADDS; dataset indices 100, 101, ..."""
    out, at = [], 100
    try:
        for graphs in ADDS:
            idx = list(range(at, at + len(graphs)))
            at += len(graphs)
            pairs = [(torch.from_numpy(a), n) for n, a in graphs]
            if len(graphs) == 1:
                cache.add(idx[0], *pairs[0])
            else:
                cache.add_many(idx, pairs)
            out.append(cache.info())
    finally:
        cache.close()
    return out


@pytest.mark.parametrize("reserve", RESERVES)
def test_rwr_cache_grows_by_the_room_rule(reserve):
    import rwr_sampler
    rv, rc = reserve
    # rs (4 bytes) and doomed (1): vertices + 1 per add; tg (4): 2 per column; cols (8): 1 per column
    model, graphs, want = Store([5, 4, 8], [rv, 2 * rc, rc]), 0, []
    for add in ADDS:
        nv, e = sizes(add)
        model.add([nv + 1, 2 * e, e])
        graphs += len(add)
        want.append({"graphs": graphs, "vertices": model.used[0], "half_edges": model.used[1], "bytes": model.bytes(),
                     "generations": model.generations})
    got = run_adds(rwr_sampler.GraphCache(K, "cuda:0", reserve=reserve))
    assert got == want


@pytest.mark.parametrize("reserve", RESERVES)
def test_eps_cache_grows_by_the_room_rule(reserve):
    import epsilon_uniform_sampler
    rv, rc = reserve
    # rowptr (8 bytes): vertices + 1 per graph; nbr (4) and ecs (4): 2 per column; cols (8): 1 per column
    model, graphs, want = Store([8, 8, 8], [rv, 2 * rc, rc]), 0, []
    for add in ADDS:
        nv, e = sizes(add)
        model.add([nv + len(add), 2 * e, e])
        graphs += len(add)
        want.append({"graphs": graphs, "vertices": model.used[0], "half_edges": model.used[1], "bytes": model.bytes(),
                     "generations": model.generations})
    got = run_adds(epsilon_uniform_sampler.GraphCache("cuda:0", reserve=reserve))
    assert got == want


# (csr_entries, bytes) of the ugs cache after each of the ADDS, per reserve: they depend on the preprocessing (CSR entries and
# viable lists), so they are recorded -- from the library of commit bdf0694, before the three caches shared their store
UGS_RECORDED = {
    (0, 0): [(8, 272), (48, 1600), (72, 3168), (180, 6304)],
    (1, 1): [(8, 272), (48, 1600), (72, 3168), (180, 6304)],
    (10, 20): [(8, 1144), (48, 2304), (72, 2976), (180, 6336)],
}


@pytest.mark.parametrize("reserve", RESERVES)
def test_ugs_cache_grows_by_the_room_rule(reserve):
    import ugs_sampler
    rv, rc = reserve
    recorded = UGS_RECORDED[reserve]
    # rowptr (8 bytes): vertices + 1 per graph; adj and adjf (8 + 8): the CSR entries; root records (24): vertices; cols (8): columns --
    # all of them of the live graphs only (n >= k), but for the columns.  The viable lists (8 bytes, reserve 0; three entries in all
    # here) are left to the recorded bytes: every add here outgrows one of the model's groups, so they never decide an allocation.
    model, graphs, entries, want = Store([8, 16, 24, 8], [rv + rv // 4, 2 * rc, rv, rc]), 0, 0, []
    for add, (csr_entries, nbytes) in zip(ADDS, recorded):
        live = [(n, a) for n, a in add if n >= K]
        model.add([sizes(live)[0] + len(live), csr_entries - entries, sizes(live)[0], sizes(add)[1]])
        graphs, entries = graphs + len(add), csr_entries
        want.append({"graphs": graphs, "vertices": model.used[2], "csr_entries": csr_entries, "bytes": nbytes, "generations": model.generations})
    got = run_adds(ugs_sampler.GraphCache(K, "cuda:0", reserve=reserve))
    assert len(recorded) == len(ADDS) and got == want
