// ugs_graphlet_common.h -- the canonical-code search of ugs_sampler.graphlets, shared by the device kernel (ugs_graphlet.hip) and the
// host canonicaliser and table builder (ugs_graphlet.cpp).  The law is stated at ugs_graphlet_canon in include/ugs_mi355.h.
//
// A graph on n <= 8 vertices is one 64-bit word: byte v holds the neighbour mask of vertex v (symmetric, no loops).  The code of a
// permutation puts pair (i, j), i < j, at bit j(j-1)/2 + i, so position j owns the j bits ("column j") above all columns below it,
// and the minimum over all n! permutations is found column by column from the top:
//   * the vertices not yet placed form an ORDERED PARTITION into cells (byte i of `cells` = vertex mask of cell i); cell i fills the
//     positions after those of cells 0 .. i-1, and vertices of one cell have the same adjacency to every vertex already placed;
//   * position j is taken by a vertex w of the LAST cell.  Its column is smallest when, inside every cell, w's neighbours take the
//     low positions: column(w) = sum over cells of (2^|N(w) & cell| - 1) << first position of the cell.  Column j outweighs all
//     lower columns together, so only the candidates with the smallest column can lead to the minimum; every cell then splits into
//     (neighbours of w, the rest), which is the refinement by adjacency to the placed vertices, iterated level by level;
//   * of tied candidates that are TWINS (equal open or closed neighbourhoods: exchanging them is an automorphism that fixes all
//     else) only the first is followed;
//   * a node whose columns so far exceed the same columns of the best code found is left (the bound by the bits already fixed).
// What is left to permute are the ties: one path for a graph without symmetry, |Aut| paths at most after the twin rule -- 48 for
// the cube, 16 for C8 and its complement, 1 for K8 -- against 40 320 permutations.
#ifndef UGS_GRAPHLET_COMMON_H
#define UGS_GRAPHLET_COMMON_H

#include <stdint.h>

#define UGS_GL_KMAX 8
#define UGS_GL_HD __host__ __device__ __forceinline__

namespace ugs_gl {

UGS_GL_HD int tri(int j) { return (j * (j - 1)) >> 1; }              // first bit of column j
UGS_GL_HD int popc8(uint32_t x) { return __builtin_popcount(x); }

// Neighbour bytes of the graph whose code is `code` in the identity order.
UGS_GL_HD uint64_t adj_of_code(uint32_t code, int n) {
    uint64_t adj = 0;
    for (int j = 1; j < n; ++j)
        for (int i = 0; i < j; ++i)
            if ((code >> (tri(j) + i)) & 1u) adj |= (1ull << (8 * i + j)) | (1ull << (8 * j + i));
    return adj;
}

// The candidates of the last cell that give the smallest column, twins removed, and that column.
UGS_GL_HD void eval_node(uint64_t adj, uint64_t cells, uint32_t &tied_out, uint32_t &col_out) {
    const int last = (63 - __builtin_clzll(cells)) >> 3;
    uint32_t best = 0xffffffffu, tied = 0;
    for (uint32_t rem = (uint32_t)(cells >> (8 * last)) & 0xffu; rem; rem &= rem - 1u) {
        const int w = __builtin_ctz(rem);
        const uint32_t nw = (uint32_t)(adj >> (8 * w)) & 0xffu;
        uint32_t c = 0;
        int pos = 0;
        for (int i = 0; i <= last; ++i) {
            const uint32_t cell = (uint32_t)(cells >> (8 * i)) & 0xffu;
            c |= ((1u << popc8(cell & nw)) - 1u) << pos;
            pos += popc8(cell);
        }
        if (c < best) { best = c; tied = 1u << w; }
        else if (c == best) tied |= 1u << w;
    }
    if (tied & (tied - 1u)) {
        uint32_t keep = 0;
        for (uint32_t rem = tied; rem; rem &= rem - 1u) {
            const int w = __builtin_ctz(rem);
            const uint32_t nw = (uint32_t)(adj >> (8 * w)) & 0xffu;
            bool twin = false;
            for (uint32_t r2 = keep; r2; r2 &= r2 - 1u) {
                const int u = __builtin_ctz(r2);
                const uint32_t nu = (uint32_t)(adj >> (8 * u)) & 0xffu;
                twin = twin || ((nu ^ nw) & ~((1u << u) | (1u << w))) == 0;
            }
            if (!twin) keep |= 1u << w;
        }
        tied = keep;
    }
    tied_out = tied;
    col_out = best;
}

// The cells after w took the last position: every cell without w, split into w's neighbours and the rest.
UGS_GL_HD uint64_t split_cells(uint64_t adj, uint64_t cells, int w) {
    const uint32_t nw = (uint32_t)(adj >> (8 * w)) & 0xffu;
    uint64_t out = 0;
    int o = 0;
    for (int i = 0; i < UGS_GL_KMAX; ++i) {
        const uint32_t cell = (uint32_t)(cells >> (8 * i)) & 0xffu & ~(1u << w);
        const uint32_t a = cell & nw, b = cell & ~nw;
        if (a) { out |= (uint64_t)a << o; o += 8; }
        if (b) { out |= (uint64_t)b << o; o += 8; }
    }
    return out;
}

// The smallest code below one node of the search: `cells` are the cells at level j0 >= 1 (positions 0 .. j0 still open) and `cur`
// holds the columns above j0.  `st` keeps one 64-bit word per level (st.put(level, word), st.get(level)): registers cannot be
// indexed by the level, so the device hands in LDS.  stats, if given, is increased by the two measures of the search the documents
// quote: [0] the complete codes compared, [1] the nodes evaluated (eval_node calls).
template <class Stack>
UGS_GL_HD uint32_t search(uint64_t adj, uint64_t cells, int j0, uint32_t cur, Stack &st, uint32_t *stats = nullptr) {
    uint32_t leaves = 0, nodes = 0;
    uint32_t best = 1u << 28;                          // above every code
    uint64_t todo = 0;                                 // byte j: the candidates of level j not yet followed
    int j = j0;
    bool fresh = true;
    for (;;) {
        if (fresh) {
            uint32_t tied, col;
            eval_node(adj, cells, tied, col);
            ++nodes;
            const int lo = tri(j), hi = lo + j;
            cur = ((cur >> hi) << hi) | (col << lo);
            if ((cur >> lo) > (best >> lo)) tied = 0;                       // the fixed bits already lose
            else if (j == 1) { ++leaves; if (cur < best) best = cur; tied = 0; }
            st.put(j, cells);
            todo = (todo & ~(0xffull << (8 * j))) | ((uint64_t)tied << (8 * j));
            fresh = false;
        }
        const uint32_t t = (uint32_t)(todo >> (8 * j)) & 0xffu;
        if (!t) {
            if (++j > j0) break;
            continue;
        }
        const int w = __builtin_ctz(t);
        todo &= ~(1ull << (8 * j + w));
        cells = split_cells(adj, st.get(j), w);
        --j;
        fresh = true;
    }
    if (stats) { stats[0] += leaves; stats[1] += nodes; }
    return best;
}

// The canonical code of the graph `adj` on n vertices, 1 <= n <= 8: the search from its root, one cell and nothing placed.
template <class Stack>
UGS_GL_HD uint32_t canon(uint64_t adj, int n, Stack &st, uint32_t *stats = nullptr) {
    if (n <= 1) {
        if (stats) { stats[0] += 1; stats[1] += 1; }
        return 0;
    }
    return search(adj, (1ull << n) - 1ull, n - 1, 0u, st, stats);
}

// The ROOTED code of vertex u (ugs_graphlet_orbits in include/ugs_mi355.h): the smallest code over the orders that put u in the last
// position.  u is forced as the first pick, tied at the root or not and with no twin rule there: its column is 2^deg - 1 over the one
// cell, the search below it is the one above.  Two vertices have equal rooted codes exactly when an automorphism maps one to the
// other, and the minimum over u is canon().
template <class Stack>
UGS_GL_HD uint32_t rooted(uint64_t adj, int n, int u, Stack &st) {
    if (n <= 1) return 0;
    const uint32_t col = (1u << popc8((uint32_t)(adj >> (8 * u)) & 0xffu)) - 1u;
    if (n == 2) return col;                            // the root is the last level with a column
    return search(adj, split_cells(adj, (1ull << n) - 1ull, u), n - 2, col << tri(n - 1), st);
}

// ---- the vertex census's table entry (ugs_graphlet_vertex_census in include/ugs_mi355.h) -----------------------------------------
// One 32-bit word says everything a completed set needs about the graph whose adjacency bits in the identity order are `code`, n <= 7:
// bits 0 .. 9 the column of its class among `keys` (the ascending keys of the connected graphs on n vertices, at most 853 of them), and
// for every position p < n, bits 10 + 3 p .. 12 + 3 p the LOCAL ORBIT INDEX of position p: the number of distinct rooted codes of the
// graph below p's, at most 6.  31 bits in all, so VERTEX_NONE -- a graph that is not connected -- is no entry.
constexpr uint32_t VERTEX_NONE = 0xFFFFFFFFu;
constexpr int VERTEX_COL_BITS = 10, VERTEX_ORB_BITS = 3;

UGS_GL_HD uint32_t vertex_col(uint32_t entry) { return entry & ((1u << VERTEX_COL_BITS) - 1u); }
UGS_GL_HD uint32_t vertex_local(uint32_t entry, int p) { return (entry >> (VERTEX_COL_BITS + VERTEX_ORB_BITS * p)) & ((1u << VERTEX_ORB_BITS) - 1u); }

template <class Stack>
UGS_GL_HD uint32_t vertex_entry(uint32_t code, int n, const int64_t *keys, int64_t num_keys, Stack &st) {
    const uint64_t adj = adj_of_code(code, n);
    const int64_t key = ((int64_t)n << 28) | (int64_t)canon(adj, n, st);
    int64_t lo = 0, hi = num_keys;                     // first key >= key
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo >= num_keys || keys[lo] != key || lo >> VERTEX_COL_BITS) return VERTEX_NONE;
    uint32_t entry = (uint32_t)lo;
    uint32_t r[UGS_GL_KMAX];
    for (int p = 0; p < n; ++p) r[p] = rooted(adj, n, p, st);
    for (int p = 0; p < n; ++p) {
        int below = 0;                                 // distinct rooted codes below r[p]: each counted at its first vertex
        for (int q = 0; q < n; ++q) {
            bool first = r[q] < r[p];
            for (int i = 0; i < q; ++i) first = first && r[i] != r[q];
            below += first;
        }
        entry |= (uint32_t)below << (VERTEX_COL_BITS + VERTEX_ORB_BITS * p);
    }
    return entry;
}

// Whether the graph `adj` on n vertices is connected.
UGS_GL_HD bool connected(uint64_t adj, int n) {
    uint32_t reach = 1u;
    for (int round = 1; round < n; ++round)
        for (int v = 0; v < n; ++v)
            if ((reach >> v) & 1u) reach |= (uint32_t)(adj >> (8 * v)) & 0xffu;
    return reach == (1u << n) - 1u;
}

// ---- node-labelled graphs (ugs_graphlet_labelled in include/ugs_mi355.h) ----------------------------------------------------------
// The orders are restricted to those that put the labels in non-decreasing order by position.  That is the search above started
// from the partition by label instead of from one cell: cell i holds the vertices of the i-th smallest label, so the last cell --
// the largest label -- fills the top positions, and refinement only ever splits a cell.  The twin rule holds as it stands: tied
// candidates share a cell, hence a label.

// The root partition of the labels of vertices 0 .. n-1: one cell per distinct label, ascending, compact.
UGS_GL_HD uint64_t label_cells(const int *labels, int n) {
    uint64_t cells = 0;
    for (int v = 0; v < n; ++v) {
        int below = 0;                                 // distinct labels below v's: its cell
        for (int w = 0; w < n; ++w) {
            bool first = labels[w] < labels[v];
            for (int x = 0; x < w; ++x) first = first && labels[x] != labels[w];
            below += first;
        }
        cells |= 1ull << (8 * below + v);
    }
    return cells;
}

// The labelled canonical code of the graph `adj` on n vertices whose root partition is `cells`.
template <class Stack>
UGS_GL_HD uint32_t canon_cells(uint64_t adj, uint64_t cells, int n, Stack &st) {
    if (n <= 1) return 0;
    return search(adj, cells, n - 1, 0u, st);
}

// The labelled ROOTED code of vertex u: the smallest code over the orders that put u last and the other n - 1 vertices in
// non-decreasing label order.  u leaves its cell wherever that is (split_cells drops a cell that becomes empty); its column is
// taken over the cells that remain.
template <class Stack>
UGS_GL_HD uint32_t rooted_cells(uint64_t adj, uint64_t cells, int n, int u, Stack &st) {
    if (n <= 1) return 0;
    const uint32_t nu = (uint32_t)(adj >> (8 * u)) & 0xffu;
    uint32_t col = 0;
    int pos = 0;
    for (int i = 0; i < UGS_GL_KMAX; ++i) {
        const uint32_t cell = (uint32_t)(cells >> (8 * i)) & 0xffu & ~(1u << u);
        col |= ((1u << popc8(cell & nu)) - 1u) << pos;
        pos += popc8(cell);
    }
    if (n == 2) return col;                            // the root is the last level with a column
    return search(adj, split_cells(adj, cells, u), n - 2, col << tri(n - 1), st);
}

}  // namespace ugs_gl

#endif /* UGS_GRAPHLET_COMMON_H */
