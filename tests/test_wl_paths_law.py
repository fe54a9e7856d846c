"""CPU checks of what pins the kernels of ugs_wl.hip: the census of their paths (wl_law.census, lookup_census, md5_census), the
inputs chosen by it (tests/wl_paths.py) and the device model with its mutants (tests/wl_device_model.py).  Shown here by
assertion: every input reaches what it names, every census class that can exist is reached by an input that names it and the
others are impossible for the reason given, the model equals the law on every input, and every mutant of the model differs from
the law on the input named for it.  tests/test_gpu_wl_paths.py runs the same inputs through the kernels.  That the law itself
reproduces networkx's and the reference's results is the assertion of tests/test_wl_law.py and tests/test_wl_feature_law.py."""
import hashlib
import os
import re

import pytest

import wl_device_model as DM
import wl_law as L
import wl_paths as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ss-gnn_amd", "csrc")
CASE_NAMES = [c.name for c in P.cases()]
HASH_NAMES = [c.name for c in P.cases() if c.form != "lookup"]
POSSIBLE = [c for c in L.CLASSES if c not in L.IMPOSSIBLE] + list(L.LOOKUP_CLASSES)


def words(hx):
    return int(hx, 16) >> 64, int(hx, 16) & L.M64


def model_run(name, mutant=None):
    """The model's (hexdigests, statuses) of a hash case, ids of a lookup case."""
    c = P.case(name)
    if c.form == "lookup":
        vocab, digests, statuses = c.arrays
        table = sorted((int(key, 16), i) for key, i in vocab.items())
        return DM.lookup([(v >> 64, v & L.M64) for v, _ in table], [i for _, i in table], [words(d) for d in digests], statuses,
                         len(vocab), mutant)
    return DM.Model(*c.arrays, c.iterations, c.labels, mutant=mutant).rows()


def blake2b_by_model(msg, piece):
    s = DM.Stream([0x5a5a5a5a5a5a5a5a] * 16)           # staging words that hold something else
    for at in range(0, len(msg), piece):
        part = msg[at:at + piece]
        s.step(DM.PIECE, int.from_bytes(part, "little"), len(part))
    s.step(DM.FLUSH)
    s.step(DM.FINISH)
    return "%016x%016x" % s.label()


def test_model_constants_and_lines_are_the_kernels():
    # the census and the model restate these; if the kernel's move, this fails and the inputs have to be chosen again
    with open(os.path.join(CSRC, "ugs_wl.hip")) as f:
        hip = f.read()
    assert "#define UGS_WL_BLOCK %d" % L.WL_BLOCK in hip and DM.WL_BLOCK == L.WL_BLOCK and DM.WAVE == L.WAVE == 64
    for line in ("a.wshift = k <= 8 ? 3 : k <= 16 ? 4 : 5;", "const int gshift = (tid & 63) - u;",
                 "const int n = __popcll((ballot >> gshift) & gmask);", "if (lo < 0 || hi < lo || hi > a.num_cols) {",
                 "for (int64_t e = lo + u; e < hi; e += W) {", "if (x < 0 || x >= n || y < 0 || y >= n) {",
                 "out = (u64)l > 0xffffffffull;", "const int j = __popcll((ballot >> gshift) & ((1ull << u) - 1ull));",
                 "const int st = !row_ok ? -1 : n == 0 ? 1 : bad_sh[g] ? 2 : norange ? 3 : 0;",
                 "const u64 d = dec2((unsigned)__popc(mymask) + ((mymask >> u) & 1u), &len);",
                 "const bool less = h2 < hi || (h2 == hi && l2 < lo);", "rank += (less || (eq && v < u)) ? 1 : 0;",
                 "cnt_sh[base + rank] = (unsigned char)(eq_before == 0 ? eq_all : 0);", "store = off + n >= 8u;",
                 "if (what == WL_FINISH || (store && widx == 0u && s.pos >= 128u)) {",
                 "blake2b_compress(s.h, m, what == WL_FINISH ? (u64)s.pos : (u64)(s.pos & ~127u), what == WL_FINISH);",
                 "for (unsigned j = used; j < 16u; ++j) stg[j * ld] = 0;",
                 "s.acc = (what == WL_PIECE && off != 0u) ? v >> (8u * (8u - off)) : 0;",
                 "else if (nitems == 1u) { v = (u64)',' | ((u64)')' << 8); len = 2; }",
                 "return (unsigned)((p & 1) ? w : (w >> 32));", "if (a.status[i] == 0) {",
                 "if (kh < hi || (kh == hi && kl < lo)) lo_i = mid + 1; else hi_i = mid;",
                 "const bool aligned = (reinterpret_cast<uintptr_t>(p) & 3u) == 0u;", "const unsigned nblk = (len + 72u) >> 6;"):
        assert line in hip, line


def test_mutants_are_documented_and_named():
    every = DM.MUTANTS + DM.LOOKUP_MUTANTS
    assert not set(every) & set(DM.UNREACHABLE) and set(P.KILLS) == set(every)
    for name in every + DM.UNREACHABLE:
        assert re.search(r"^  %s\s" % name, DM.__doc__, re.M), name
    assert set(P.KILLS.values()) <= set(CASE_NAMES)


@pytest.mark.parametrize("size", [0, 1, 127, 128, 129, 255, 256, 257])
def test_model_blake2b_is_hashlibs(size):
    msg = bytes((7 * j + size) % 251 for j in range(size))
    for piece in (8, 5, 1):                            # whole words, straddling pieces, bytes
        assert blake2b_by_model(msg, piece) == hashlib.blake2b(msg, digest_size=16).hexdigest(), (size, piece)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_reaches_its_classes(name):
    c = P.case(name)
    census = P.census_of(name)
    every = set(L.LOOKUP_CLASSES) if c.form == "lookup" else set(L.CLASSES)
    assert census <= every and c.reaches
    for cls in c.reaches:
        assert cls in every, cls
        assert cls in census, (name, cls, sorted(census))


@pytest.mark.parametrize("cls", POSSIBLE)
def test_census_covers_every_class(cls):
    assert any(cls in P.case(name).reaches and cls in P.census_of(name) for name in CASE_NAMES), cls


def test_every_case_is_needed():
    """Deleting a case loses a class that only it names, or the input a mutant is killed on."""
    for name in CASE_NAMES:
        others = {cls for c in P.cases() if c.name != name for cls in c.reaches}
        assert set(P.case(name).reaches) - others or name in P.KILLS.values(), name


def test_impossible_classes_are_impossible():
    assert set(L.IMPOSSIBLE) <= set(L.CLASSES) and len(L.CLASSES) == len(set(L.CLASSES))
    for name in HASH_NAMES:
        assert not P.census_of(name) & set(L.IMPOSSIBLE), name
    # the reasons, worked out: the longest message of iteration 1 in degree mode ...
    deg1 = L.stream_classes([2] * 33)
    assert sum([2] * 33) < 128 and not deg1 & {"block_straddle", "opens_block", "flush_opens_block"}
    # ... pieces of 8 bytes only, up to 33 of them in label mode's iteration 1 and 4 * (1 .. 33) later ...
    eight = set().union(*(L.stream_classes([8] * j) for j in range(1, 4 * 33 + 1)))
    assert not eight & {"word_complete", "word_straddle", "block_straddle", "flush_stores", "flush_opens_block", "finish_partial_word"}
    assert all("finish_exact_3plus" not in L.stream_classes([8] * j) for j in range(1, 34))
    assert all("finish_one_word" not in L.stream_classes([8] * 4 * j) for j in range(1, 34))
    # ... and the final string: 2 bytes, 42 or 43 for one item, 41 a + 42 b for a + b >= 2 items (39 or 40 bytes each)
    h = "0" * 32
    assert [len(L.final_text(items)) for items in ([], [(h, 1)], [(h, 10)], [(h, 1)] * 2, [(h, 10)] * 2, [(h, 1)] * 3)] == [2, 42, 43, 82, 84, 123]
    lengths = {2, 42, 43} | {41 * a + 42 * b for a in range(300) for b in range(300) if a + b >= 2}
    assert 128 not in lengths and 256 not in lengths and min(x for x in lengths if x % 128 == 0) == 1152
    for cls, why in L.IMPOSSIBLE.items():
        assert cls.split(".")[0] in L.STREAMS and cls.split(".")[1] in L.STREAM_CLASSES and why


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_model_equals_the_law(name):
    got, want = model_run(name), P.law_of(name)
    if P.case(name).form == "lookup":
        assert got == want
    else:
        assert got[1] == want[1] and got[0] == want[0]


@pytest.mark.parametrize("mutant", DM.MUTANTS + DM.LOOKUP_MUTANTS)
def test_mutant_differs_on_its_case(mutant):
    name = P.KILLS[mutant]
    got, want = model_run(name, mutant), P.law_of(name)
    assert (got if P.case(name).form == "lookup" else tuple(got)) != want, (mutant, name)


def test_unreachable_mutant_differs_only_on_crafted_labels():
    """cmp_ignore_lo: no input produces two labels that agree in their high word and differ in the low one (start labels have a
    zero low word, later ones are BLAKE2b digests), so every case agrees with the law; the model's ranking, given such labels,
    does not."""
    for name in HASH_NAMES:
        got = model_run(name, "cmp_ignore_lo")
        assert tuple(got) == P.law_of(name), name
    lab = [(5, 9), (5, 1 << 63), (4, 7), (5, 9), (1 << 63, 0), (5, 3)]
    want = sorted(range(len(lab)), key=lambda u: (lab[u][0] << 64 | lab[u][1], u))
    ranked = {}
    for mutant in (None, "cmp_ignore_lo", "cmp_signed", "rank_no_tiebreak"):
        order, cnt = [0] * 8, [0] * 8
        DM.Model([[0]], [[], []], [0, 0], 1, mutant=mutant).rank(lab, order, cnt, 1)
        ranked[mutant] = (order[:len(lab)], cnt[:len(lab)])
    assert ranked[None] == (want, [1, 1, 2, 0, 1, 1])
    assert all(ranked[m] != ranked[None] for m in ("cmp_ignore_lo", "cmp_signed", "rank_no_tiebreak"))


def test_rule_4_in_both_laws():
    """An edge_ptr range that is no range of [0, num_cols]: status 2 and no digest, status 1 on a row without vertices; the rows
    beside it are what they are alone; num_cols may be narrower than edge_index."""
    import wl_feature_law as FL
    nodes, ei, ep = P.case("bad_edge_ptr").arrays
    hexes, stats = P.law_of("bad_edge_ptr")
    assert stats == [0, 2, 0, 2, 2, 0, 2, 2, 0, 1] and [h is None for h in hexes] == [s != 0 for s in stats]
    assert hexes[0] == L.wl_row(nodes[0], ei[0][0:2], ei[1][0:2], 1)[0] and hexes[8] == L.wl_row(nodes[8], ei[0][4:6], ei[1][4:6], 1)[0]
    assert L.wl_rows(nodes, ei, ep, 1, num_cols=4)[1] == [0, 2, 0, 2, 2, 2, 2, 2, 2, 1]
    ids = [[x - 100 if x >= 0 else -1 for x in row] for row in nodes.tolist()]
    fh, fs, _ = FL.wl_feature_rows(ids, ei, ep, P.LABELS8, 1)
    assert fs == stats and fh[2] == FL.wl_feature_row(ids[2], ei[0][1:3], ei[1][1:3], P.LABELS8, 1)[0]
    assert FL.wl_feature_rows(ids, ei, ep, [], 1)[1] == [3, 2, 3, 2, 2, 3, 2, 2, 3, 1]      # a bad range is 2 whatever the labels
    assert DM.Model(ids, ei, ep, 1, P.LABELS8).rows() == (fh, fs)


def test_compact_md5_widths_reach_every_class():
    reached = set()
    for F in P.MD5_WIDTHS:
        stride = F + 1 if F % 2 == 0 else F + 2            # the odd row stride of the GPU test
        assert stride % 2 == 1
        got = L.md5_census(F, [i * stride for i in range(P.MD5_ROWS)])
        assert got <= set(L.MD5_CLASSES)
        assert {"read_words", "read_bytes", "both_reads_one_launch"} <= got, F
        reached |= got
    assert reached == set(L.MD5_CLASSES)
