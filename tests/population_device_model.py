"""population_device_model.py -- what uniform_sampler.PopulationCache alone runs (ugs_uniform.hip), restated in plain Python, with
one-line mutants.  For tests/test_population_paths_law.py; nothing here calls the library.

rows(c, draws, mode, mutant)      uni_pop_pairs, uni_pop_rows and uni_pop_fill over the rows the law draws: lane l of a row's 16 writes
                                  the members among the vertices 4 l ... 4 l + 3 at the popcount prefix of the lanes below, a row of -1
                                  is written by the loop `j = l; j < k; j += 16`, a lane counts the columns l, l + 16, ... of the
                                  graph's bucket, and the fill is uniform_population_cases.group_fill.
  minus_one_single_trip           the row of -1 is written by `if (l < k) out[l] = -1`
  prefix_uses_4l_plus_4           the popcount prefix includes the lane's own four vertices
  endpoint_mask_31                an endpoint is read with `& 31`
  v_shift_8                       the second endpoint is read at `uv >> 8`
  last_lane_skipped               lane 15 writes no member

stored_keys(keys, mutant)         uni_pop_store: workgroup (g, y) of 32 copies the keys y 256 + t, then every 8192nd behind them.
  single_trip                     no second trip
  grid_y_ignored                  every workgroup starts at key t
  stride_256 (equivalent)         the trip stride is 256: every key is still copied, by several workgroups, each time the same value

named_graph(c, ei, mutant)        pop_fingerprint and uni_pop_check: the graph the check of a batch names.
  no_position                     fp_mix(x, 0)
  one_trip                        a lane reads word t only
  names_last                      atomicMin in place of atomicMax: the largest differing graph
  xor_fold (equivalent)           the partial sums are folded with ^: another fingerprint, the same verdicts on every input here
  no_form_skip (equivalent)       a graph that is not enumerated is compared too: both fingerprints are 0

named_loop_graph(c, ei, mutant)   uni_pop_loops.
  bit_only                        every loop vertex marks bit u & 63 of word 0
  no_position                     fp_mix(x, 0)
"""
import numpy as np

import population_paths as P
import uniform_population_cases as UPC

M64 = (1 << 64) - 1
UNWRITTEN = -(1 << 40)                                              # what a slot nobody wrote holds

ROW_MUTANTS = ("minus_one_single_trip", "prefix_uses_4l_plus_4", "endpoint_mask_31", "v_shift_8", "last_lane_skipped")
STORE_MUTANTS, STORE_EQUIVALENT = ("single_trip", "grid_y_ignored"), ("stride_256",)
CHECK_MUTANTS, CHECK_EQUIVALENT = ("no_position", "one_trip", "names_last"), ("xor_fold", "no_form_skip")
LOOP_MUTANTS = ("bit_only", "no_position")


class ModelFault(Exception):
    """the model wrote outside a row: on the device, another row's memory"""


def popcount(x):
    return bin(x).count("1")


# ---- rows and fill ----
def rows(c, draws, mode, mutant=None):
    """(nodes, edge_index, edge_ptr, sample_ptr, edge_src) in the law's layout from the law's draws [(graph, mask)]"""
    assert mutant is None or mutant in ROW_MUTANTS
    G, m, k = len(c.ptr) - 1, c.m, c.k
    emask = 31 if mutant == "endpoint_mask_31" else 63
    vshift = 8 if mutant == "v_shift_8" else 16
    pairs = {}
    for g in {g for g, _ in draws}:                                  # uni_pop_pairs
        pairs[g] = [(q, (u & 0xFFFFFFFF) | ((v << 16) & 0xFFFFFFFF)) for q, u, v in P.bucket(c, g)]
    nodes = np.full((G * m, k), UNWRITTEN, np.int64)
    eu, ev, es, eptr = [], [], [], [0]
    for row, (g, mask) in enumerate(draws):
        lo = int(c.ptr[g])
        out = nodes[row]
        hits = []
        if mask:
            for l in range(P.LANES - 1 if mutant == "last_lane_skipped" else P.LANES):
                j = popcount(mask & ((1 << (4 * l + (4 if mutant == "prefix_uses_4l_plus_4" else 0))) - 1))
                e = (mask >> (4 * l)) & 15
                while e:
                    if j >= k:
                        raise ModelFault((row, l, j))
                    out[j] = lo + 4 * l + ((e & -e).bit_length() - 1)
                    j += 1
                    e &= e - 1
            for q, uv in pairs[g]:
                u, v = uv & emask, (uv >> vshift) & emask
                hits.append((mask >> u) & (mask >> v) & 1)
        else:
            for l in range(P.LANES):
                if mutant == "minus_one_single_trip":
                    if l < k:
                        out[l] = -1
                else:
                    for j in range(l, k, P.LANES):
                        out[j] = -1
        for at in UPC.group_fill(hits):                              # uni_pop_fill: bucket positions in the order they are written
            q, uv = pairs[g][at]
            u, v = uv & emask, (uv >> vshift) & emask
            eu.append(popcount(mask & ((1 << u) - 1)) if mode == "sample" else lo + u)
            ev.append(popcount(mask & ((1 << v) - 1)) if mode == "sample" else lo + v)
            es.append(q)
        eptr.append(len(es))
    return (nodes, np.array([eu, ev], np.int64).reshape(2, -1), np.array(eptr, np.int64), np.arange(G + 1, dtype=np.int64) * m,
            np.array(es, np.int64))


# ---- the copy of a graph's keys ----
def stored_keys(keys, mutant=None):
    """What uni_pop_store leaves in the population for one graph's sorted keys"""
    assert mutant is None or mutant in STORE_MUTANTS + STORE_EQUIVALENT
    n = len(keys)
    out = [UNWRITTEN] * n
    stride = P.ROW_BLOCK if mutant == "stride_256" else P.STORE_Y * P.ROW_BLOCK
    for y in range(P.STORE_Y):
        for t in range(P.ROW_BLOCK):
            i = t if mutant == "grid_y_ignored" else y * P.ROW_BLOCK + t
            while i < n:
                out[i] = keys[i]
                if mutant == "single_trip":
                    break
                i += stride
    return out


# ---- fingerprints ----
def fp_mix(word, pos):
    x = (word + 0x9E3779B97F4A7C15 * (pos + 1)) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def fingerprint(words, mutant=None):
    """pop_fingerprint: lane t sums fp_mix over the non-zero words t, t + 256, ..., the 256 partial sums are added mod 2^64"""
    part = [0] * P.ROW_BLOCK
    for t in range(P.ROW_BLOCK):
        for i in range(t, len(words), P.ROW_BLOCK):
            if words[i]:
                part[t] = (part[t] + fp_mix(words[i], 0 if mutant == "no_position" else i)) & M64
            if mutant == "one_trip":
                break
    total = 0
    for x in part:
        total = total ^ x if mutant == "xor_fold" else (total + x) & M64
    return total


def graph_fingerprints(c, ei, mutant=None):
    """per graph of the batch `ei`: the fingerprint of its bitmap in the form the graph was added in (0 for form 0)"""
    fm = P.forms(c)
    return [fingerprint(P.bitmap_words(n, P.graph_cols(c, ei, g), fm[g]), mutant) if fm[g] else 0 for g, (n, _) in enumerate(c.graphs)]


def named_graph(c, ei, mutant=None):
    """uni_pop_check over the batch `ei` against the fingerprints of the added graphs: the graph named, None where status[2] stays 0"""
    assert mutant is None or mutant in CHECK_MUTANTS + CHECK_EQUIVALENT
    G, fm = len(c.graphs), P.forms(c)
    stored = [fingerprint(P.bitmap_words(n, e, fm[g]), mutant) if fm[g] else 0 for g, (n, e) in enumerate(c.graphs)]
    given = graph_fingerprints(c, ei, mutant)
    status = None
    for g in range(G):
        if (fm[g] != 0 or mutant == "no_form_skip") and given[g] != stored[g]:
            status = G - g if status is None else min(status, G - g) if mutant == "names_last" else max(status, G - g)
    return None if status is None else G - status


def loop_fingerprint(n, cols, mutant=None):
    """uni_pop_loops: the loop vertices as a bitmap of 16 words, reduced like an adjacency bitmap"""
    bits = [0] * P.LOOP_WORDS
    for u, v in zip(*np.asarray(cols).tolist()):
        if u == v and 0 <= u < 64 * P.LOOP_WORDS:
            bits[0 if mutant == "bit_only" else u >> 6] |= 1 << (u & 63)
    return sum(fp_mix(x, 0 if mutant == "no_position" else i) for i, x in enumerate(bits) if x) & M64


def named_loop_graph(c, ei, mutant=None):
    assert mutant is None or mutant in LOOP_MUTANTS
    G, fm = len(c.graphs), P.forms(c)
    status = 0
    for g, (n, e) in enumerate(c.graphs):
        if fm[g] and loop_fingerprint(n, P.graph_cols(c, ei, g), mutant) != loop_fingerprint(n, e, mutant):
            status = max(status, G - g)
    return G - status if status else None
