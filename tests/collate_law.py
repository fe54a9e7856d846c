"""The law of the collation step (csrc/ugs_collate.hip, header) in plain numpy, and a maker of synthetic per-rank results.

The law: the collated batch is the ranks' local results put one behind the other in rank order.  Nothing here reads the wire
format, the Collator or the library; the case maker uses no sampler (the collation kernels are value-agnostic), so it reaches
sizes and values a sampling run of a few seconds cannot: totals past one and several edge blocks, ids at and past 2^31, local ids
128..255, rows of -1."""
import math

import numpy as np

I64 = np.int64
# values forced into every section whose bound admits them: the edges of the 1-, 4- and 8-byte wire forms
LANDMARKS = (127, 128, 255, 256, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32)


def expected(locals_):
    """(nodes [B, k], edge_index [2, T], edge_ptr [B + 1], edge_src [T]) of the whole batch from the ranks'
    (nodes [rows_r, k], edge_index [2, >= t_r], edge_ptr [rows_r + 1], edge_src [>= t_r]); t_r = edge_ptr[-1] of rank r."""
    nodes, eidx, eptr, esrc, base = [], [], [], [], 0
    for n, ei, ep, es in locals_:
        t = int(ep[-1])
        assert ep[0] == 0 and len(ep) == n.shape[0] + 1 and ei.shape[1] >= t and es.shape[0] >= t
        nodes.append(n)
        eptr.append(ep[:-1] + base)
        eidx.append(ei[:, :t])
        esrc.append(es[:t])
        base += t
    eptr.append(np.array([base], I64))
    return (np.vstack(nodes).astype(I64), np.concatenate(eidx, axis=1).astype(I64), np.concatenate(eptr).astype(I64),
            np.concatenate(esrc).astype(I64))


def _values(rng, n, bound):
    """n values uniform in [0, bound), with bound - 1, 0 and every landmark below the bound forced in (as many as n admits)."""
    v = rng.integers(0, bound, size=n, dtype=I64)
    forced = [bound - 1, 0] + [x for x in LANDMARKS if 0 < x < bound - 1]
    slots = rng.permutation(n)[:len(forced)]
    v[slots] = np.array(forced[:len(slots)], I64)
    return v


class Case:
    """Synthetic locals of one step and the job geometry they belong to."""

    def __init__(self, locals_, k, mode, node_bound, edge_id_bound, col_bound):
        self.locals, self.k, self.mode = locals_, int(k), mode
        self.node_bound, self.edge_id_bound, self.col_bound = int(node_bound), int(edge_id_bound), int(col_bound)
        self.world = len(locals_)
        self.rows = [int(l[0].shape[0]) for l in locals_]
        self.totals = [int(l[2][-1]) for l in locals_]
        self.row_off = [0]
        for r in self.rows:
            self.row_off.append(self.row_off[-1] + r)
        self.total_rows = self.row_off[-1]

    def expected(self):
        return expected(self.locals)

    def padded(self, cap, junk=-9):
        """the same locals with edge_index / edge_src filled up to `cap` entries with junk: capacity slack beyond a rank's total"""
        out = []
        for n, ei, ep, es in self.locals:
            t = int(ep[-1])
            pad = max(cap - t, 0)
            out.append((n, np.concatenate([ei[:, :t], np.full((2, pad), junk, I64)], axis=1), ep, np.concatenate([es[:t], np.full(pad, junk, I64)])))
        return out


def make_case(rng, world, rows, k, totals, node_bound, edge_id_bound, col_bound, mode, failed_share=0.0, failed_at=()):
    """Synthetic locals of `world` ranks.  rows[r] rows and totals[r] edge entries on rank r, the entries spread over the rank's
    rows by a random non-decreasing edge_ptr from 0 to totals[r] (rows of zero entries included).  nodes / edge_index / edge_src
    are uniform below their bounds with the extremes forced in; in mode "sample" edge_index holds local ids in [0, k), k - 1 among
    them.  ceil(failed_share * rows[r]) random rows of every rank, and the rows `failed_at` = [(rank, row), ...] (row -1: the
    rank's last), are failed: nodes of -1 and no entries."""
    assert len(rows) == world and len(totals) == world
    ebound = k if mode == "sample" else edge_id_bound
    locals_ = []
    for r in range(world):
        n_rows, t = int(rows[r]), int(totals[r])
        failed = {row % n_rows for rk, row in failed_at if rk == r}
        want = min(n_rows, math.ceil(failed_share * n_rows))
        rest = [i for i in range(n_rows) if i not in failed]
        failed |= set(rng.permutation(rest)[:max(want - len(failed), 0)].tolist())
        live = np.array([i for i in range(n_rows) if i not in failed], dtype=I64)
        if t and not len(live):
            raise ValueError(f"rank {r}: {t} edge entries but no row to hold them")
        counts = np.zeros(n_rows, I64)
        if len(live):
            cuts = np.sort(rng.integers(0, t + 1, size=len(live) - 1, dtype=I64))
            counts[live] = np.diff(np.concatenate([[0], cuts, [t]]))
        eptr = np.concatenate([[0], np.cumsum(counts)]).astype(I64)
        nodes = np.full((n_rows, k), -1, I64)
        if len(live):
            nodes[live] = _values(rng, len(live) * k, node_bound).reshape(len(live), k)
        eidx = _values(rng, 2 * t, ebound).reshape(2, t)
        esrc = _values(rng, t, col_bound)
        assert eptr[-1] == t and np.all(np.diff(eptr) >= 0) and np.all(counts[sorted(failed)] == 0)
        locals_.append((nodes, eidx, eptr, esrc))
    return Case(locals_, k, mode, node_bound, edge_id_bound, col_bound)


# ---- the cases both the CPU and the GPU collation tests run (name -> (case, edge_cap or None for the largest total, slack junk)) ----
B31, BIG = 2 ** 31, 2 ** 40 + 8
EDGE_WIDTHS = {"u8": ("sample", 1000), "i32": ("global", B31 - 1), "i64": ("global", BIG)}          # edge_index wire -> (mode, edge_id_bound)


def _has(arr, v):
    return bool((np.asarray(arr) == v).any())


def rows_block_cases():
    """world 2, rows_cap * k at 255, 256, 257, 511, 513: the last block of the rows kernel partly filled, full, one entry into
    the next; uneven ranges, so the ranks end at different places of their blocks (on a block edge where k admits one)"""
    out = {}
    for k, rows in ((1, (255, 128)), (1, (256, 77)), (1, (256, 257)), (1, (257, 256)), (1, (511, 256)), (1, (513, 512)),
                    (3, (85, 40)), (3, (171, 85)), (7, (73, 20))):
        rng = np.random.default_rng(1000 + 10 * k + rows[0])
        c = make_case(rng, 2, rows, k, (rows[0] // 2 + 300, rows[1] // 3 + 1), 5000, 5000, 7000, "global", failed_share=0.05)
        assert max(rows) * k in (255, 256, 257, 511, 513) and rows[0] != rows[1]
        out[f"k{k}-rows{rows[0]}+{rows[1]}"] = (c, None, None)
    return out


EDGE_TOTALS = ((255, 0, 1), (256, 1023, 257), (1025, 1024, 2047), (2049, 4097, 256))


def edges_block_cases():
    """world 3, per-rank totals at the edges of the edges kernel's blocks (1024 entries, four steps of 256); edge_cap equal to the
    largest total and 5 above it with junk in the slack; every edge_index wire width"""
    assert {t for tr in EDGE_TOTALS for t in tr} == {0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4097}
    out = {}
    for wi, (wname, (mode, ebound)) in enumerate(EDGE_WIDTHS.items()):
        for ti, totals in enumerate(EDGE_TOTALS):
            for slack in (0, 5):
                rng = np.random.default_rng(2000 + 100 * wi + 10 * ti + slack)
                c = make_case(rng, 3, (7, 5, 9), 6, totals, 90000, ebound, 123457, mode)
                out[f"{wname}-{'-'.join(map(str, totals))}-cap+{slack}"] = (c, max(totals) + slack, -9 if slack else None)
    return out


def width_cases():
    """nodes {int32, int64} x edge_index {uint8, int32, int64} x edge_src {int32, int64}: int32 from a bound just below 2^31, int64
    from 2^40 + 8 (2^31 - 1, 2^31, 2^40 + 7 present); uint8 is mode "sample" at k = 200 with 3 rows per rank (local ids 128..199);
    one failed row per rank at either node width.  Then all three bounds AT 2^31 (the 8-byte forms at their threshold, 2^31 - 1
    present), and k = 256 in mode "sample" (the int32 wire for local ids)."""
    out = {}
    for ni, (nname, nbound) in enumerate((("n32", B31 - 1), ("n64", BIG))):
        for wi, (wname, (mode, ebound)) in enumerate(EDGE_WIDTHS.items()):
            for si, (sname, sbound) in enumerate((("s32", B31 - 1), ("s64", BIG))):
                rng = np.random.default_rng(3000 + 100 * ni + 10 * wi + si)
                k = 200 if wname == "u8" else 5
                c = make_case(rng, 2, (3, 3), k, (300, 45), nbound, ebound, sbound, mode, failed_share=0.3)
                n, ei, _, es = c.expected()
                assert _has(n, -1) and _has(n, nbound - 1) and _has(es, sbound - 1) and _has(n, 0) and _has(es, 0) and _has(ei, 0)
                if wname == "u8":
                    assert _has(ei, 199) and _has(ei, 128) and _has(ei, 127) and ei.max() == 199
                else:
                    assert _has(ei, ebound - 1)
                for arr, b in ((n, nbound), (ei, ebound), (es, sbound)):
                    if b == BIG:
                        assert _has(arr, 2 ** 31 - 1) and _has(arr, 2 ** 31) and _has(arr, 2 ** 40 + 7)
                    elif b == B31 - 1:
                        assert _has(arr, 2 ** 31 - 2)
                out[f"{nname}-{wname}-{sname}"] = (c, None, None)
    rng = np.random.default_rng(3500)
    c = make_case(rng, 2, (3, 3), 5, (300, 45), B31, B31, B31, "global", failed_share=0.3)
    assert all(_has(a, 2 ** 31 - 1) for a in c.expected()[:2]) and _has(c.expected()[3], 2 ** 31 - 1)
    out["all-bounds-at-2^31"] = (c, None, None)
    c = make_case(rng, 2, (3, 2), 256, (300, 45), 70000, 70000, 70000, "sample")
    assert _has(c.expected()[1], 255) and _has(c.expected()[1], 128)
    out["sample-k256"] = (c, None, None)
    return out


def failed_row_cases():
    """whole rows of -1 with zero entries: the first row of a rank, the last row of a rank, the last row of the batch"""
    rng = np.random.default_rng(4000)
    c = make_case(rng, 3, (4, 3, 5), 4, (40, 300, 1100), 3000, 3000, 9000, "global", failed_share=0.25, failed_at=[(0, 0), (1, -1), (2, -1)])
    n, _, ep, _ = c.expected()
    for row in (0, 4 + 3 - 1, 12 - 1):
        assert np.all(n[row] == -1) and ep[row + 1] == ep[row]
    return {"first-last-of-rank-last-of-batch": (c, None, None)}


def layout_cases():
    """world 1; world 64 (the bound of the offset sum and of row_off[]) with 1 to 3 rows and a few entries on every rank; world 5
    with zero-row ranks at the front, in the middle, at the end; a rank with rows but no entries between two with entries"""
    out = {}
    rng = np.random.default_rng(5000)
    out["world1"] = (make_case(rng, 1, (6,), 4, (1300,), 3000, 3000, 9000, "global", failed_share=0.2), None, None)
    rows = [1 + int(x) for x in rng.integers(0, 3, size=64)]
    totals = [1 + int(x) for x in rng.integers(0, 9, size=64)]
    assert set(rows) == {1, 2, 3}
    out["world64"] = (make_case(rng, 64, rows, 3, totals, 3000, 3000, 9000, "global"), None, None)
    for empty in ((0,), (2,), (4,), (0, 4), (1, 2, 3)):
        rows = [0 if r in empty else 3 + r for r in range(5)]
        totals = [0 if r in empty else 200 * r + 17 for r in range(5)]
        out["world5-empty-" + "".join(map(str, empty))] = (make_case(rng, 5, rows, 4, totals, 3000, 3000, 9000, "global", failed_share=0.2), None, None)
    c = make_case(rng, 3, (4, 5, 3), 4, (37, 0, 41), 3000, 3000, 9000, "global")
    assert c.rows[1] > 0 and c.totals == [37, 0, 41]
    out["rows-without-entries-in-the-middle"] = (c, None, None)
    return out


def no_edge_cases():
    """k = 1: a subgraph of one vertex has no edges, edge_cap = 0, the edges kernel is not launched"""
    rng = np.random.default_rng(6000)
    c = make_case(rng, 2, (5, 4), 1, (0, 0), 3000, 3000, 9000, "sample", failed_share=0.2)
    assert _has(c.expected()[0], -1) and _has(c.expected()[0], 2999)
    return {"k1-cap0": (c, 0, None)}


def empty_batch_cases():
    """no rows at all: nodes [0, k], edge_ptr == [0]"""
    out = {}
    for world in (1, 3):
        for cap in (0, 7):
            c = make_case(np.random.default_rng(7000), world, (0,) * world, 4, (0,) * world, 3000, 3000, 9000, "global")
            assert c.total_rows == 0 and c.expected()[0].shape == (0, 4) and c.expected()[2].tolist() == [0]
            out[f"world{world}-cap{cap}"] = (c, cap, None)
    return out


def all_cases():
    out = {}
    for group in (rows_block_cases, edges_block_cases, width_cases, failed_row_cases, layout_cases, no_edge_cases, empty_batch_cases):
        for name, v in group().items():
            out[f"{group.__name__[:-6]}:{name}"] = v
    return out


STEADY_ROWS = (6, 4, 5)
STEADY_TOTALS = ((1500, 0, 900), (3, 3, 3), (0, 0, 0), (2049, 1, 1024), (10, 2000, 0))


def steady_state_steps(seed):
    """five steps of one job (fixed rows and bounds) whose totals grow and shrink, fresh values every step"""
    rng = np.random.default_rng(seed)
    return [make_case(rng, 3, STEADY_ROWS, 4, t, 3000, 3000, 9000, "global", failed_share=0.2) for t in STEADY_TOTALS]
