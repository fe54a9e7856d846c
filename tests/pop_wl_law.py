"""The law of the WL population (include/ugs_mi355.h at ugs_uniform_population_create_wl) in plain Python, composed from the laws
the suite already has: the rows of uniform_law / uniform_wide_law (pinned to the reference by the f14 and f18 fixtures) hashed by
wl_law / wl_feature_law (pinned by f19 and f20).  A helper for the tests, not a test; nothing here calls the library.

wl_ids of a call = the vocabulary ids of the WL digests of the rows the SAME call gives in mode "sample", with the labels that were
given when the graphs were added.  Two views of it:
  rows    ids_of_rows over the law's mode-"sample" tensors (sample_batch_ids, sample_graphs_ids);
  cache   member_digests: the digest of every member of S_g in enumeration order, which is what the population stores; a row
          that draws member d has member_digests(...)[d] (distinct_ids, and tests/test_pop_wl_law.py shows the two views agree)."""
import numpy as np

import uniform_distinct_law as D
import uniform_law as U
import uniform_wide_law as W
import wl_feature_law as FL
import wl_law as L


def ids_of_rows(nodes, edge_index, edge_ptr, vocab, iterations, labels=None):
    """hash_to_id over the rows: len(vocab) for a row of -1, an unknown digest, or (labels) a label outside [0, 2^32)"""
    if labels is None:
        hexes, stats, _ = L.wl_rows(nodes, edge_index, edge_ptr, iterations)
    else:
        hexes, stats, _ = FL.wl_feature_rows(nodes, edge_index, edge_ptr, labels, iterations)
    return L.ids_from(hexes, stats, vocab)


def batch_labels(graph_idx, ptr, labels_by_index):
    """L of the law: for batch vertex ptr[g] + v the label given for vertex v of graph graph_idx[g] (0 below ptr[0]); None for the
    degree form"""
    if labels_by_index is None:
        return None
    out = [0] * int(ptr[-1])
    for g, i in enumerate(graph_idx):
        lab = [int(x) for x in labels_by_index[i]]
        assert len(lab) == int(ptr[g + 1] - ptr[g])
        out[int(ptr[g]):int(ptr[g + 1])] = lab
    return out


def sample_batch_ids(ei, ptr, m, k, seed, vocab, iterations, graph_idx=None, labels_by_index=None):
    nodes, eidx, eptr, _, _ = W.sample_batch(ei, ptr, m, k, "sample", seed)
    return ids_of_rows(nodes, eidx, eptr, vocab, iterations, batch_labels(graph_idx, ptr, labels_by_index))


def sample_graphs_ids(ei, ptr, m, k, seeds, vocab, iterations, graph_idx=None, labels_by_index=None, failed=()):
    """sample_graphs as one-graph law calls; a graph named in `failed` gives m unknown ids"""
    lab = batch_labels(graph_idx, ptr, labels_by_index)
    out = []
    for g in range(len(ptr) - 1):
        if g in failed:
            out += [len(vocab)] * m
            continue
        nodes, eidx, eptr, _, _ = W.sample_batch(ei, ptr[g:g + 2], m, k, "sample", seeds[g])
        out += ids_of_rows(nodes, eidx, eptr, vocab, iterations, lab)
    return out


def member_digests(ei, ptr, g, k, iterations, labels=None):
    """What the cache keeps for graph g of the batch: (hexdigest or None) of every member of S_g in enumeration order, each hashed as
    the row the sampler writes for it in mode "sample" -- its columns in batch order, loops and duplicates included"""
    ei = np.asarray(ei, np.int64).reshape(2, -1)
    lo, n = int(ptr[g]), int(ptr[g + 1] - ptr[g])
    if n < k or k < 1:
        return []
    inside = (ei[0] >= lo) & (ei[0] < lo + n) & (ei[1] >= lo) & (ei[1] < lo + n)
    cu, cv = (ei[0][inside] - lo).tolist(), (ei[1][inside] - lo).tolist()
    out = []
    for sub in W.sorted_tuples(U.graph_adjacency(ei[0], ei[1], lo, n), k):
        pos = {v: i for i, v in enumerate(sub)}
        pairs = [(pos[u], pos[v]) for u, v in zip(cu, cv) if u in pos and v in pos]
        row, src, dst = [lo + v for v in sub], [p[0] for p in pairs], [p[1] for p in pairs]
        hx = L.wl_row(row, src, dst, iterations)[0] if labels is None else FL.wl_feature_row(row, src, dst, labels, iterations)[0]
        out.append(hx)
    return out


def distinct_ids(ei, ptr, m, k, seeds, vocab, iterations, graph_idx=None, labels_by_index=None):
    """(ids [G m], valid [G]) of sample_distinct: row j of graph g draws member uniform_distinct_law.law(seeds[g], |S_g|, m)[j]"""
    lab = batch_labels(graph_idx, ptr, labels_by_index)
    ids, valid = [], []
    for g in range(len(ptr) - 1):
        dig = member_digests(ei, ptr, g, k, iterations, lab)
        valid.append(min(m, len(dig)))
        for d in D.law(int(seeds[g]) & D.M64, len(dig), m):
            ids.append(vocab.get(dig[d], len(vocab)) if d >= 0 and dig[d] is not None else len(vocab))
    return ids, valid


def population_digests(batches, k, iterations, labels_of_batch=None):
    """The distinct digests a population holds after adding the graphs of `batches` [(ei, ptr)], ascending (hex order is numeric order)"""
    seen = set()
    for b, (ei, ptr) in enumerate(batches):
        for g in range(len(ptr) - 1):
            seen.update(h for h in member_digests(ei, ptr, g, k, iterations, None if labels_of_batch is None else labels_of_batch[b]) if h is not None)
    return sorted(seen)
