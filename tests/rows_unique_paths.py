"""rows_unique_paths.py -- the inputs that pin the paths of csrc/ugs_rows.hip, shared by the CPU tests
(tests/test_rows_unique_paths_law.py: census, device model, mutants) and the GPU tests (tests/test_gpu_rows_unique_paths.py).

A case is (name, arrays, reaches, kills, refusal, strided): `arrays` the six int64 numpy arrays (nodes [R, k], edge_index [2, E],
edge_ptr [R + 1], sample_ptr [G + 1], edge_src [E] or empty, ptr [G + 1]); `reaches` the classes of rows_unique_law.census it is
there for, for both `by` unless the class says otherwise (`set_*`); `kills` the mutants of tests/rows_unique_device_model.py that
it tells from the law; `refusal` the message the call must raise, as a regular expression, or None; `strided` whether the GPU
test hands edge_index over as a view with a column stride of 2.  Both test files assert `reaches` again, so an input that drifts
off its path fails instead of losing coverage.

Shapes are the smallest at which the path exists.  Graphs of up to 2^31 - 1 vertices cost nothing, only the ids are large.  Every
refusal is a validation path that returns a status word: the pointer arrays of a refused case are read by index i only, and no
entry of any case is used as an index by the kernels.  `second_trip` (2^20 + 40 graphs) and its refused twin are the only large
cases in graphs; `block_sizes` (eleven graphs, one for every padded size of the workgroup form, 14 917 rows) is the largest in rows;
everything else has at most 4099 rows."""
import collections
import functools

import numpy as np

import rows_unique_law as L

Case = collections.namedtuple("Case", "name arrays reaches kills refusal strided")
BYS = ("set", "sequence")


def edges_for(nodes, lens, edge_src=True):
    """edge_index, edge_ptr and edge_src with spans of the given lengths; the values tell row and position, as law.with_edges'."""
    lens = np.asarray(lens, dtype=np.int64)
    R = nodes.shape[0]
    assert len(lens) == R
    edge_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Es = int(edge_ptr[-1])
    row_of = np.repeat(np.arange(R), lens).astype(np.int64)
    pos = np.arange(Es, dtype=np.int64) - edge_ptr[row_of]
    edge_index = np.stack([row_of * 1000 + pos, -(row_of * 1000 + pos) - 7]).astype(np.int64).reshape(2, Es)
    src = (row_of * 31 + pos * 3 + 5).astype(np.int64) if edge_src else np.zeros(0, dtype=np.int64)
    return edge_index, edge_ptr, src


def make(rows_of_graphs, sizes, k, lens=None, edge_src=True, first=0):
    """The six arrays from the rows of every graph (lists of k entries) and the graphs' vertex counts; spans 0, 1, 2, 0, 1, 2, ...
    unless `lens` gives them; `first` is ptr[0]."""
    rows = [r for g in rows_of_graphs for r in g]
    nodes = np.array(rows, dtype=np.int64).reshape(len(rows), k)
    ptr = L.ptr_of(sizes) + first
    sptr = L.ptr_of([len(g) for g in rows_of_graphs])
    ei, eptr, esrc = edges_for(nodes, np.arange(len(rows)) % 3 if lens is None else lens, edge_src)
    return nodes, ei, eptr, sptr, esrc, ptr


def from_codes(codes, lo):
    """entries from key codes: 0 is -1, c is vertex lo + c - 1"""
    return [-1 if c == 0 else lo + c - 1 for c in codes]


# ---- keys: one case per k, a graph of exactly 2^b - 1 vertices behind one of 5 ----
KEY_KS = (1, 2) + tuple(sorted(L.STRADDLE_K + L.FIELD_AT_64_K))


def keys_case(k):
    """Rows whose codes ascend, so that "set" and "sequence" give them the same key, plus one permuted copy.  The field across
    bit 64 (or the fields on both sides of it) takes the values that differ only in its high part, or only in its low part; the
    fields above it hold the top code 2^b - 1."""
    b = L.key_bits(k)
    top, lo = (1 << b) - 1, 5
    f = 64 // b
    low = 64 - f * b
    rows, reaches = [], ["unrolled_k%d" % k if k <= 8 else "looped", "top_code@%d" % b]
    if f >= k:                                       # k = 1, 2: no field reaches bit 64
        rows = [[0] * k, [1] * k, [top] * k, [1] * (k - 1) + [top], [0] * (k - 1) + [1], [1] * k, [0] * k]
    elif low:                                        # a field across bit 64, `low` of its bits below
        x2 = (1 << low) | 1
        rows = [[1] * f + [x] + [top] * (k - f - 1) for x in (1, x2, x2 ^ 1, 1, x2)]
        reaches += ["straddle_hi_only@%d" % k, "straddle_lo_only@%d" % k]
    else:
        rows = [[1] * (f - 1) + [a, c] + [top] * (k - f - 1) for a, c in ((2, 3), (2, 2), (1, 3), (2, 3))]
        rows += [[1] + [3] * f + [top] * (k - f - 1), [2] + [3] * f + [top] * (k - f - 1), [1] + [3] * f + [top] * (k - f - 1)]
        reaches += ["field_at_64@%d" % k, "bit_127"]
    rows.append([1] * (k - 1) + [top])               # the graph's last vertex, whatever field the others end in
    rows.append(rows[1][::-1])                       # merges with row 1 as a set only (k > 1)
    rows.append([0] + rows[1][1:])                   # -1 against the first vertex in field 0
    graph1 = [from_codes(r, lo) for r in rows]
    graph0 = [[(i * 2) % 5 for i in range(k)]]
    return make([graph0, graph1], [5, top], k), tuple(reaches)


# ---- the check's status codes: a small good input with one thing wrong ----
def good_small():
    rows0 = [[0, 1, 2], [2, 1, 0], [0, 1, 2]]
    rows2 = [[7, 8, 9], [9, -1, 7], [7, 8, 9], [8, 8, 8]]
    return make([rows0, [], rows2], [4, 3, 5], 3, lens=[2, 1, 2, 3, 0, 2, 2])


def status_case(kind):
    nodes, ei, eptr, sptr, esrc, ptr = [a.copy() for a in good_small()]        # sptr [0, 3, 3, 7], eptr [0, 2, 3, 5, 8, 8, 10, 12], ptr [0, 4, 7, 12]
    if kind == "sample_ptr0":
        sptr[0] = 1
    elif kind == "sample_end":
        sptr[3] = 6
    elif kind == "sample_decreases":
        sptr[1] = 4                                  # index 1: 4 > 3
    elif kind == "edge_ptr0":
        eptr[0] = 1
    elif kind == "edge_end":
        eptr[7] = 11
    elif kind == "edge_decreases":
        eptr[4] = 9                                  # index 4: 9 > 8
    elif kind == "ptr_decreases":
        ptr[1] = 8                                   # index 1: 8 > 7; graph 0 keeps its rows inside [0, 8)
    elif kind == "two_offences":
        sptr[1] = 4                                  # 4 * 1 + 0
        eptr[4] = 9                                  # 4 * 4 + 1: the higher value loses
        ptr[1] = 8                                   # 4 * 1 + 2
    elif kind == "ptr_graph_entry":
        eptr[4] = 9
        ptr[3] = ptr[2] + (1 << 31)                  # graph 2: 2^31 vertices at 31 bits
        nodes[0, 0] = -2
    elif kind == "graph_entry":
        ptr[3] = ptr[2] + (1 << 31)
        nodes[0, 0] = -2
    elif kind == "two_graphs_over":
        ptr[1:] += 1 << 31                           # graph 0 over the vertex limit, and graph 2 behind it
        ptr[3] += 1 << 31
        nodes[3:][nodes[3:] >= 0] += 1 << 31
    elif kind == "two_entries":
        nodes[1, 1] = 4                              # graph 0 ends at 4: row 1
        nodes[5, 0] = -2                             # row 5
    else:
        raise KeyError(kind)
    return nodes, ei, eptr, sptr, esrc, ptr


def entry_case(kind):
    nodes, ei, eptr, sptr, esrc, ptr = [a.copy() for a in good_small()]
    nodes[4, 2] = {"entry_below_graph": ptr[2] - 1, "entry_at_hi": ptr[3], "entry_minus_two": -2, "entry_2p32_above": ptr[2] + (1 << 32)}[kind]
    return nodes, ei, eptr, sptr, esrc, ptr


def over_case(b):
    """One row in a graph of 2^b vertices, one more than a b-bit field holds, behind a graph that is exactly at the limit."""
    k = max(k for k in L.ALL_K if L.key_bits(k) == b)
    top = (1 << b) - 1
    return make([[[0] * k], [[top + 1] * k]], [top, top + 1], k)


def rows_over_case():
    rows1 = [[4 + (i % 3), 4 + (i // 3) % 3] for i in range(4097)]
    return make([[[0, 1]], rows1, [[7, 8]]], [4, 3, 2], 2, lens=[1] * 4099)


# ---- wave form ----
def wave_sizes():
    """Six graphs, two in the last workgroup: 1, 2, 63 (runs whose first row is not the graph's first), 64 distinct rows with
    edges on the last, 64 equal rows, 3."""
    sizes = [4, 4, 20, 64, 4, 4]
    ptr = L.ptr_of(sizes)
    graphs = [[[1, 2]], [[5, 4], [4, 5]],
              [[ptr[2] + (i * 7) % 20, ptr[2] + ((i * 7) % 20 + (i % 2)) % 20] for i in range(63)],
              [[ptr[3] + i, ptr[3] + i] for i in range(64)],
              [[ptr[4] + 1, ptr[4] + 3]] * 64, [[ptr[5], -1], [-1, ptr[5]], [-1, -1]]]
    R = sum(len(g) for g in graphs)
    lens = np.arange(R) % 4
    lens[66 + 63] = 3                                # graph 3's row 63
    return make(graphs, sizes, 2, lens=lens)


# ---- workgroup form ----
def digits_graph(n, lo, distinct):
    """n rows over 64 vertices from lo: row j holds the two base-64 digits of (j * 37) % distinct"""
    return [[lo + ((j * 37) % distinct) % 64, lo + ((j * 37) % distinct) // 64] for j in range(n)]


def block_one(n):
    return make([digits_graph(n, 0, n // 2 + 3)], [64], 2)


BLOCK_NS = (65, 128, 129, 257, 512, 513, 1025, 2048, 2049, 4096, 4095)


def block_sizes():
    return make([digits_graph(n, 64 * g, n // 2 + 3 if g % 2 else n) for g, n in enumerate(BLOCK_NS)], [64] * len(BLOCK_NS), 2)


def pad_all_ones(k):
    """70 rows in 128 pairs: the row whose key is all ones three times (first, in the middle, last); the others vary two
    fields below the top code (at most 14: b = 4 has room for no more)."""
    b = L.key_bits(k)
    top = (1 << b) - 1
    other = [[top] * (k - 2) + [1 + j % 14, 1 + j // 14] for j in range(67)]
    rows = [[top] * k] + other[:34] + [[top] * k] + other[34:] + [[top] * k]
    return make([[from_codes(r, 3) for r in rows]], [top], k, first=3)


def block_runs():
    """Two graphs of one class.  70 rows: the lowest key (-1, -1) four times, the highest three times with its first row at 66,
    every other row twice, a thread apart.  65 rows, all equal."""
    mid = [[10 + j, 3] for j in range(30)]
    g0 = [[-1, -1]] + mid + [[-1, -1]] + mid + [[-1, -1], [40, 4], [41, 4], [42, 4], [49, 49], [-1, -1], [49, 49], [49, 49]]
    g1 = [[50 + 7, 50 + 2]] * 65
    assert len(g0) == 70 and g0[66] == [49, 49]
    return make([g0, g1], [50, 10], 2)


def block_words():
    """k = 4, 31-bit fields at bits 0, 31, 62, 93.  Codes (1, 2, 4, 8) and one row each that differs from it in one 32-bit word
    only: field 0; bits 1.. of field 1; bits 2.. of field 2; bits 3.. of field 3.  60 more rows that differ in field 3."""
    rows = [[1, 2, 4, 8], [2, 2, 4, 8], [1, 4, 4, 8], [1, 2, 8, 8], [1, 2, 4, 16]] + [[1, 2, 4, 24 + 8 * j] for j in range(60)]
    rows += rows[:5]
    return make([[from_codes(r, 2) for r in rows]], [1000], 4, first=2)


# ---- scan across graphs ----
def scan_case(G):
    graphs = [[[2 * g, 2 * g + 1]] * (1 + g % 3) if g % 128 == 0 or g >= G - 2 else [] for g in range(G)]
    return make(graphs, [2] * G, 2)


# ---- sets ----
def set_ties():
    rows = [[1, 1, 2, 17], [1, 1, 2, 33], [2, 1, 17, 1], [1, 2, 2, 17], [5, 5, 5, 5], [1, 2, 1, 2], [2, 2, 1, 1], [33, 2, 1, 1]]
    return make([[from_codes(r, 9) for r in rows]], [40], 4, first=9)


def behind_empty():
    return make([[], [], [[4, 5], [5, 4], [4, 4]], [], [], [[10, 11], [10, 11]], [], []], [2, 2, 2, 2, 2, 2, 2, 2], 2)


# ---- edges ----
def edge_spans(edge_src=True):
    rows = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [5, 6], [2, 3], [6, 7], [0, 1]]
    return make([rows], [8], 2, lens=[0, 1, 15, 16, 17, 33, 40, 2, 20], edge_src=edge_src)


# ---- the second trip of the check ----
BIG_G = (1 << 20) + 40
BIG_ROWS = {7: 2, (1 << 20) - 1: 1, (1 << 20) + 3: 70, (1 << 20) + 20: 3, (1 << 20) + 38: 2}


def second_trip(refused=False):
    """2^20 + 40 graphs of 5 vertices, all empty but five; one of 70 rows and one of 3 behind index 2^20.  The refused twin has
    sample_ptr one too high at index 2^20 + 10, inside a run of empty graphs: it decreases there and nowhere else."""
    rows = np.zeros(BIG_G, dtype=np.int64)
    for g, n in BIG_ROWS.items():
        rows[g] = n
    sptr = L.ptr_of(rows)
    ptr = 5 * np.arange(BIG_G + 1, dtype=np.int64)
    g_of = np.repeat(np.arange(BIG_G), rows)
    j = np.arange(len(g_of))
    nodes = np.stack([5 * g_of + j % 5, 5 * g_of + (j // 5) % 3], axis=1).astype(np.int64)
    ei, eptr, esrc = edges_for(nodes, j % 3)
    if refused:
        sptr[(1 << 20) + 10] += 1
    return nodes, ei, eptr, sptr, esrc, ptr


REFUSED_INDEX = (1 << 20) + 10


def _pat(arrays):
    word, value = L.refusal(arrays)
    return L.refusal_pattern(word, value, arrays[0].shape[1])


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, arrays, reaches, kills=(), refused=False, strided=False):
        out.append(Case(name, arrays, tuple(reaches), tuple(kills), _pat(arrays) if refused else None, strided))

    for k in KEY_KS:
        arrays, reaches = keys_case(k)
        kills = {3: ("straddle_hi_dropped",), 8: ("field_at_64_into_lo",), 2: ("code_without_plus_one",)}.get(k, ())
        add("keys_k%d" % k, arrays, reaches, kills)
    add("set_ties", set_ties(), ("set_ties", "set_all_equal"), ("rank_tie_le",))
    add("behind_empty", behind_empty(), ("graph_behind_empty_graphs",), ("graph_search_first_of_equal",))
    for kind in ("entry_below_graph", "entry_at_hi", "entry_minus_two", "entry_2p32_above"):
        kills = {"entry_below_graph": ("below_lo_unchecked",), "entry_2p32_above": ("cast32_before_check",)}.get(kind, ())
        add(kind, entry_case(kind), (kind,), kills, refused=True)
    for kind in ("sample_ptr0", "sample_end", "sample_decreases", "edge_ptr0", "edge_end", "edge_decreases", "ptr_decreases"):
        add(kind, status_case(kind), (kind,), refused=True)
    add("two_offences", status_case("two_offences"), ("two_offences_lower_index_wins@ptr",), ("status_max_instead_of_min",), refused=True)
    add("two_graphs_over", status_case("two_graphs_over"), ("two_offences_lower_index_wins@graph",), refused=True)
    add("two_entries", status_case("two_entries"), ("two_offences_lower_index_wins@entry",), refused=True)
    add("ptr_graph_entry", status_case("ptr_graph_entry"), ("ptr_beats_graph",), refused=True)
    add("graph_entry", status_case("graph_entry"), ("graph_beats_entry",), refused=True)
    add("rows_over", rows_over_case(), ("rows_over",), refused=True)
    for b in L.ALL_BITS:
        add("over_b%d" % b, over_case(b), ("vertices_over@%d" % b,), refused=True)
    add("wave_sizes", wave_sizes(), ("rows_1", "rows_2", "rows_63", "rows_64", "slot0", "slot1", "slot2", "slot3", "partial_group", "all_equal",
                                     "all_distinct", "rep_not_first_lane", "lane63_kept_with_edges", "no_big"), ("wave_rep_last", "small_bound_lt_64"))
    add("block_256", block_one(256), ("pn256_full", "class0", "no_small"), ("class_bound_le_256",))
    add("block_1024", block_one(1024), ("pn1024_full", "class1", "kept_in_later_wave"), ("class_bound_le_1024", "block_scan_without_earlier_waves"))
    add("block_sizes", block_sizes(), ("pn128_full", "pn128_half_plus_1", "pn256_half_plus_1", "pn512_full", "pn512_half_plus_1", "pn1024_half_plus_1",
                                       "pn2048_full", "pn2048_half_plus_1", "pn4096_full", "pn4096_half_plus_1", "n4095", "class2", "two_graphs_one_class"),
        ("pad_key_zero",))
    for k in L.FIELD_AT_64_K:
        add("pad_all_ones_k%d" % k, pad_all_ones(k), ("pad_meets_all_ones_key@%d" % k, "run_last"),
            ("pad_row_zero", "upper_bound_to_pn") if k == 8 else ())
    add("block_runs", block_runs(), ("run_first", "run_last", "run_all", "run_across_threads"), ("sort_ignores_row",))
    add("block_words", block_words(), ("word_x_only", "word_y_only", "word_z_only", "word_w_only"),
        ("cmp_skips_x", "cmp_skips_y", "cmp_skips_z", "cmp_skips_w"))
    add("scan_1024", scan_case(1024), ("one_pass", "exactly_1024"))
    add("scan_1025", scan_case(1025), ("1025",), ("scan_carry_dropped",))
    add("edge_spans", edge_spans(), ("span_0", "span_1", "span_15", "span_16", "span_17", "span_33"), ("edges_one_trip", "edges_stride_8"))
    add("edge_spans_bare", edge_spans(edge_src=False), ("no_edge_src", "strided_edge_index"), strided=True)
    add("second_trip", second_trip(), ("second_trip", "big_past_first_trip", "many_passes", "rows_fewer_than_graphs", "small_and_big"), ("check_one_trip",))
    add("second_trip_refused", second_trip(refused=True), ("second_trip", "offence_past_first_trip"), refused=True)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def law_of(name, by):
    """("refused", word, value) or ("ok", form, the seven arrays): the law's side of rows_unique_device_model.run"""
    c = case(name)
    r = L.refusal(c.arrays)
    if r is not None:
        return ("refused",) + r
    return "ok", L.form_of(c.arrays[3]), L.unique_rows(*c.arrays, by)


@functools.lru_cache(maxsize=None)
def census_of(name, by):
    c = case(name)
    return frozenset(L.census(c.arrays, by, c.strided))


def reaches_for(c, by):
    """the classes of `reaches` that hold for this `by`"""
    return [cls for cls in c.reaches if by == "set" or not cls.startswith("set_")]
