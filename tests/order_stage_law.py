"""order_stage_law.py -- CPU restatement of how the walk kernel reproduces libstdc++'s std::unordered_set<int> iteration
order (ss-gnn_amd/csrc/ugs_kernels.hip, file header, stage_mat / stage_final), for the tests and the census tool.

The container grown from empty by single inserts rehashes through the bucket chain 13 -> 29 -> 59 -> ...; both an insert and
a rehash put an element that opens a bucket at the FRONT of the list and any other element at the front of its bucket's block.
So with arrival order a_0, a_1, ... the iteration order is: blocks by DESCENDING first arrival, members of a block by
DESCENDING arrival (the first arrival is the last entry of its block).  The kernel's stage i holds the order O_i of the
first B_i candidates of D (the distinct candidates in first-insertion order) as positions in D; its arrival sequence is
O_{i-1} ++ D[B_{i-1}:B_i].  The final stage (the first B_fs >= c) names the element at rank rsel without materialising.

Here: `StlSet` (a literal simulation of the libstdc++ singly linked list with per-bucket "before" pointers), `group_order`
(the stage rule), `stage_orders` / `final_order`, `table_final_pick` (stage_final's arithmetic, slot by slot, with the
leader fast path), `edit_stage` (the in-place edit of the lowest invalidated stage) and `census` (C5-shaped walks).
"""
import random

CHAIN = [13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273]


class StlSet:
    """libstdc++ _Hashtable<int, ..., unique keys> node list: _M_before_begin, _M_buckets[b] = node BEFORE bucket b's first
    node, _M_insert_bucket_begin and _M_rehash_aux(true_type) as written (max load factor 1, buckets along CHAIN)."""

    def __init__(self):
        self.nb = 1
        self.buckets = [None]
        self.nxt = {"BB": None}       # node -> next node ("BB" = before-begin)
        self.n = 0

    def _insert_bucket_begin(self, b, node):
        if self.buckets[b] is not None:
            before = self.buckets[b]
            self.nxt[node] = self.nxt[before]
            self.nxt[before] = node
        else:
            self.nxt[node] = self.nxt["BB"]
            self.nxt["BB"] = node
            if self.nxt[node] is not None:
                self.buckets[self.nxt[node] % self.nb] = node
            self.buckets[b] = "BB"

    def _rehash(self, nb):
        p = self.nxt["BB"]
        self.nxt["BB"] = None
        buckets = [None] * nb
        bbegin_bkt = 0
        while p is not None:
            nx = self.nxt[p]
            b = p % nb
            if buckets[b] is None:
                self.nxt[p] = self.nxt["BB"]
                self.nxt["BB"] = p
                buckets[b] = "BB"
                if self.nxt[p] is not None:
                    buckets[bbegin_bkt] = p
                bbegin_bkt = b
            else:
                self.nxt[p] = self.nxt[buckets[b]]
                self.nxt[buckets[b]] = p
            p = nx
        self.nb, self.buckets = nb, buckets

    def insert(self, x):
        if x in self.nxt:
            return
        if self.n + 1 > self.nb:
            self._rehash(next(b for b in CHAIN if b >= self.n + 1))
        self._insert_bucket_begin(x % self.nb, x)
        self.n += 1

    def order(self):
        out, p = [], self.nxt["BB"]
        while p is not None:
            out.append(p)
            p = self.nxt[p]
        return out


def stl_order_literal(seq):
    s = StlSet()
    for x in seq:
        s.insert(x)
    return s.order()


def group_order(tags, keys, B):
    """Stage rule: `tags` in arrival order, `keys[t]` their keys -> tags in iteration order for B buckets."""
    first, members = {}, {}
    for a, t in enumerate(tags):
        b = keys[t] % B
        first.setdefault(b, a)
        members.setdefault(b, []).append(t)
    return [t for b in sorted(members, key=lambda b: -first[b]) for t in reversed(members[b])]


def stage_input(D, O_prev, i, hi):
    nold = CHAIN[i - 1] if i else 0
    return (list(O_prev) if i else []) + list(range(nold, hi))


def stage_orders(D, n):
    """O_0 .. O_{n-1} as lists of positions in D (needs len(D) >= B_{n-1})."""
    O = []
    for i in range(n):
        O.append(group_order(stage_input(D, O[i - 1] if i else None, i, CHAIN[i]), D, CHAIN[i]))
    return O


def final_stage(c):
    return next(i for i, b in enumerate(CHAIN) if b >= c)


def final_order(D, c, O):
    fs = final_stage(c)
    return group_order(stage_input(D, O[fs - 1] if fs else None, fs, c), D, CHAIN[fs])


def table_final_pick(D, c, O, rsel, NJ, GS=64):
    """stage_final<GS, NJ> restated slot by slot: lane l holds arrivals t = l*NJ + j; the lane holding arrival c-1 enters its
    slots past c into an extra bucket B (laid out first).  Returns (position in D, off, leader position of the hit bucket)."""
    fs = final_stage(c)
    B = CHAIN[fs]
    tags = stage_input(D, O[fs - 1] if fs else None, fs, c)
    L = c
    past = NJ - 1 - (L - 1) % NJ
    n = L + past
    bk = [D[tags[t]] % B if t < L else B for t in range(n)]
    first, size = {}, {}
    for t in range(n):
        first.setdefault(bk[t], t)
        size[bk[t]] = size.get(bk[t], 0) + 1
    gs = [size[bk[t]] if first[bk[t]] == t else 0 for t in range(n)]
    run = 0
    target1 = rsel + past + 1
    hit = None
    for t in range(n - 1, -1, -1):          # descending arrival = the kernel's lanes from high to low, slots from NJ-1 to 0
        run += gs[t]
        e = (run - target1) & 0xFFFFFFFF
        if e < gs[t]:
            hit = (t, e)
    t_lead, off = hit
    hp = tags[t_lead]
    if off == 0:
        return hp, off, hp
    mates = [t for t in range(L) if bk[t] == bk[t_lead]]      # ascending arrival: exactly `off` members below the answer
    return tags[mates[off]], off, hp


def edit_stage(D, O_i, i, q):
    """In-place edit of stage i (B_{i-1} <= q < B_i, len(D) > B_i) for the removal of D[q]: the new order as positions in
    D-without-q, or None when D[q] is the first arrival of a bucket of two or more members (recompute)."""
    B = CHAIN[i]
    assert (CHAIN[i - 1] if i else 0) <= q < B < len(D)
    bq = D[q] % B
    r = O_i.index(q)
    last_of_block = r + 1 == len(O_i) or D[O_i[r + 1]] % B != bq
    shared = r > 0 and D[O_i[r - 1]] % B == bq
    if last_of_block and shared:
        return None
    out = [p for p in O_i if p != q]
    xn = D[B]                                                   # joins at the end: the largest arrival
    bn = xn % B
    at = next((k for k, p in enumerate(out) if D[p] % B == bn), 0)
    out.insert(at, B)
    return [p - 1 if p > q else p for p in out]


def census(walks=300, k=8, degree=40.0, n=1_000_000, seed=1, cap=448):
    """C5-shaped walks (random neighbour ids of an ER graph with n vertices and mean degree `degree`, one walk per wave):
    how many table finals (65 .. cap candidates) hit a bucket leader (off == 0), and how many stage recomputations the
    in-place edit would take over.  Returns a dict of counts per walk."""
    rng = random.Random(seed)
    nrng = random.Random(seed + 1)

    def nbrs(v):
        d = 0
        # Poisson(degree) by inversion of exponential gaps (no numpy: the census stays pure Python)
        t = nrng.expovariate(1.0)
        while t < degree:
            d += 1
            t += nrng.expovariate(1.0)
        return [nrng.randrange(n) for _ in range(d)]

    st = dict(walks=0, steps=0, finals_reg=0, finals_table=0, finals_table_leader=0, recomputes=0, recomputes_saved=0,
              edits_tried=0, edits_accepted=0, edits_last_step=0)
    for _ in range(walks):
        st["walks"] += 1
        root = rng.randrange(n)
        seen = {root}
        D = []
        for x in nbrs(root):
            if x not in seen:
                seen.add(x)
                D.append(x)
        O = []
        nvalid = nvalid_b = 0
        valid_b = []        # stage orders under the edit rule (only their count matters for the census)
        for step in range(k - 1):
            c = len(D)
            if c == 0 or c > cap:
                break
            st["steps"] += 1
            rsel = rng.randrange(c)
            fs = final_stage(c)
            O = stage_orders(D, fs)
            st["recomputes"] += max(0, fs - nvalid)
            st["recomputes_saved"] += max(0, fs - nvalid) - max(0, fs - nvalid_b)
            nvalid, nvalid_b = max(nvalid, fs), max(nvalid_b, fs)
            order = final_order(D, c, O)
            q = order[rsel]
            if c > 64:
                st["finals_table"] += 1
                NJ = (c + 63) // 64
                p, off, _ = table_final_pick(D, c, O, rsel, NJ)
                assert p == q
                st["finals_table_leader"] += off == 0
            else:
                st["finals_reg"] += 1
            keep = sum(1 for b in CHAIN[:fs] if b <= q)
            # the edit rule: the lowest invalidated stage i = keep, if it is still valid (i < nvalid_b, which implies c > B_i)
            i = keep
            accepted = False
            if i < min(nvalid_b, fs):
                st["edits_tried"] += 1
                if step == k - 2:
                    st["edits_last_step"] += 1
                accepted = edit_stage(D, O[i], i, q) is not None
                st["edits_accepted"] += accepted
            nvalid = min(keep, nvalid)
            nvalid_b = min(keep + 1 if accepted else keep, nvalid_b)
            w = D.pop(q)
            for x in nbrs(w):
                if x not in seen:
                    seen.add(x)
                    D.append(x)
    per = {key: v / st["walks"] for key, v in st.items() if key != "walks"}
    per["walks"] = st["walks"]
    per["leader_share_of_table_finals"] = st["finals_table_leader"] / max(1, st["finals_table"])
    per["accept_share_of_edits"] = st["edits_accepted"] / max(1, st["edits_tried"])
    per["saved_share_of_recomputes"] = st["recomputes_saved"] / max(1, st["recomputes"])
    return per
