// ugs_graphlet.hip -- exact graphlet keys and class ids of sampled rows, on the device.  The law is stated at
// ugs_graphlet_canon in include/ugs_mi355.h; the search is ugs_graphlet_common.h, the same code the host table is built with.
//
// ugs_graphlet_canon_kernel: eight lanes per row (one per vertex), eight rows per wave64; groups never span a wave.
//   row     lane u reads entry u of the row (k = 8: a wave reads 512 consecutive bytes); n is the popcount of the group's ballot.  The
//           lanes stride over the row's edge entries and OR them into 64-bit words (byte v = neighbour mask of v) that three
//           xor-shuffles fold: range check, deduplication, reversed copies and dropped loops at once;
//   search  every lane evaluates the root of ugs_gl's search (eight candidates, one cell).  Lane u then owns the subtree below the
//           first pick u, if u is one of the tied candidates the twin rule keeps, and runs ugs_gl::search there: refinement by
//           adjacency to the vertices already placed, twins in fixed order, ties permuted, bounded by the bits already fixed.  Three
//           xor-shuffles take the minimum over the group.  The subtrees of one row run side by side and do not share their bounds: a
//           lane may follow a branch that a sequential search would have cut, but never longer than its own subtree.  The per-level
//           cell words live in LDS, [level][thread]: registers cannot be indexed by the level and the layout puts a wave's accesses
//           on consecutive addresses (0 bytes of scratch);
//   id      lane 0 of the group: binary search of the key in the ascending table (at most 13 598 entries: 14 probes, the table
//           stays in L2).
// There is one path.  What the split over first picks buys, and what the most symmetric rows cost: DESIGN.md section 19.
//
// ugs_graphlet_orbits_kernel (law: ugs_graphlet_orbits in the same header): the same geometry and reading,
// every lane u < n searching below its own vertex as the forced first pick; described at the kernel.
//
// ugs_graphlet_labelled_kernel (law: ugs_graphlet_labelled in the same header): node-labelled keys, and the
// orbits of the label-preserving automorphisms, by the same searches started from the partition by label; described at the kernel.
//
// ugs_graphlet_census_table_kernel (ugs_graphlet_census in the same header): the column of every raw code of
// n <= 7 vertices, the table the census kernels of ugs_uniform.hip classify a set with; described at the kernel.
//
// ugs_graphlet_vertex_census_table_kernel (ugs_graphlet_vertex_census in the same header): the column and the
// orbit of every position of every raw code of n <= 7 vertices, the table of the vertex census kernels; described at the kernel.
#include "ugs_device.h"
#include "ugs_graphlet_common.h"
#include "../../include/ugs_mi355.h"

#define UGS_GL_BLOCK 256
#define UGS_GL_LANES 8             // lanes per row: one per vertex, UGS_GL_KMAX

namespace {

struct GlArgs {
    const int64_t *nodes;        // [rows, k]
    const int64_t *edge_index;   // [2, num_cols], row stride `stride`
    int64_t stride, num_cols;
    const int64_t *edge_ptr;     // [rows + 1]
    int64_t rows;
    int k;
    const int64_t *table;        // ascending keys of all graphs on at most k vertices, or NULL
    int64_t table_len;
    int64_t *key;                // [rows]
    int32_t *status;             // [rows]
    int64_t *cls;                // [rows], or NULL
};

struct LdsStack {
    uint64_t *base;              // this thread's column of [UGS_GL_KMAX][UGS_GL_BLOCK]
    __device__ __forceinline__ void put(int level, uint64_t v) { base[level * UGS_GL_BLOCK] = v; }
    __device__ __forceinline__ uint64_t get(int level) const { return base[level * UGS_GL_BLOCK]; }
};

__global__ __launch_bounds__(UGS_GL_BLOCK) void ugs_graphlet_canon_kernel(GlArgs a) {
    __shared__ uint64_t cells_sh[UGS_GL_KMAX * UGS_GL_BLOCK];
    const int tid = (int)threadIdx.x;
    const int u = tid & (UGS_GL_LANES - 1);                      // vertex, and first pick, of this lane
    const int64_t row = (int64_t)blockIdx.x * (UGS_GL_BLOCK / UGS_GL_LANES) + (tid >> 3);
    if (row >= a.rows) return;                                   // whole groups leave; no barrier below: a lane's LDS column is its own

    const int64_t id = u < a.k ? a.nodes[row * a.k + u] : -1;
    const int gshift = (tid & 63) & ~(UGS_GL_LANES - 1);         // the group's first lane inside the wave
    const int n = __popc((unsigned)(__ballot(id >= 0) >> gshift) & 0xffu);
    int bad = 0;
    uint64_t adj = 0;
    if (n > 0) {
        const int64_t lo = a.edge_ptr[row], hi = a.edge_ptr[row + 1];
        if (lo < 0 || hi < lo || hi > a.num_cols) {
            bad = 1;                                             // not a range of edge_index: nothing is read
        } else {
            for (int64_t e = lo + u; e < hi; e += UGS_GL_LANES) {
                const int64_t x = a.edge_index[e], y = a.edge_index[a.stride + e];
                if (x < 0 || x >= n || y < 0 || y >= n) bad = 1;
                else if (x != y) adj |= (1ull << (8 * (int)x + (int)y)) | (1ull << (8 * (int)y + (int)x));
            }
        }
    }
    for (int d = 1; d < UGS_GL_LANES; d <<= 1) {                 // the group's lanes are all here: n and the row are theirs alike
        adj |= __shfl_xor(adj, d);
        bad |= __shfl_xor(bad, d);
    }
    const int status = n == 0 ? 1 : bad ? 2 : 0;
    uint32_t code = 1u << 28;                                    // above every code
    if (status == 0) {
        if (n == 1) {
            code = 0;
        } else {
            const uint64_t root = (1ull << n) - 1ull;            // one cell: nothing placed
            uint32_t tied, col;
            ugs_gl::eval_node(adj, root, tied, col);
            if (n == 2) {
                code = col;                                      // the root is the last level with a column
            } else if ((tied >> u) & 1u) {
                LdsStack st{cells_sh + tid};
                code = ugs_gl::search(adj, ugs_gl::split_cells(adj, root, u), n - 2, col << ugs_gl::tri(n - 1), st);
            }
        }
        for (int d = 1; d < UGS_GL_LANES; d <<= 1) code = min(code, (uint32_t)__shfl_xor((int)code, d));
    }
    if (u != 0) return;
    const int64_t key = status == 0 ? ((int64_t)n << 28) | (int64_t)code : -1;
    a.key[row] = key;
    a.status[row] = status;
    if (a.cls) {
        int64_t cid = a.table_len;                               // the id of a refused row: len(vocab)
        if (status == 0) {
            int64_t lo_i = 0, hi_i = a.table_len;                // first table key >= key
            while (lo_i < hi_i) {
                const int64_t mid = lo_i + ((hi_i - lo_i) >> 1);
                if (a.table[mid] < key) lo_i = mid + 1; else hi_i = mid;
            }
            if (lo_i < a.table_len && a.table[lo_i] == key) cid = lo_i;
        }
        a.cls[row] = cid;
    }
}

struct GlOrbitArgs {
    GlArgs g;                    // rows, table and the optional key / status / class outputs (each may be NULL here)
    const int64_t *base;         // [table_len + 1]: first orbit id of every class, then O_k
    int64_t *orbit;              // [rows, k]
};

// ugs_graphlet_orbits_kernel: the geometry, the row and edge reading and the three folds of the kernel above.
//   search  lane u < n runs ugs_gl::rooted for vertex u: the search below the FORCED first pick u, tied at the root or not and with
//           no twin rule there.  Lanes u >= n hold 2^28, above every code;
//   group   eight shuffles hand every lane the group's values.  Their minimum is the canonical code; a lane is a first occurrence
//           if no lane before it holds its value; the local index is the number of first occurrences with a smaller value;
//   id      lane 0 finds the class as above and reads base[class]; a shuffle hands it to the group;
//   store   lane s is slot s: its vertex index j is the popcount of the group's ballot below s, lane j's local index comes by a
//           shuffle, and a wave writes 8 k consecutive int64.
__global__ __launch_bounds__(UGS_GL_BLOCK) void ugs_graphlet_orbits_kernel(GlOrbitArgs oa) {
    __shared__ uint64_t cells_sh[UGS_GL_KMAX * UGS_GL_BLOCK];
    const GlArgs &a = oa.g;
    const int tid = (int)threadIdx.x;
    const int u = tid & (UGS_GL_LANES - 1);                      // slot, vertex and first pick of this lane
    const int64_t row = (int64_t)blockIdx.x * (UGS_GL_BLOCK / UGS_GL_LANES) + (tid >> 3);
    if (row >= a.rows) return;                                   // whole groups leave; no barrier below: a lane's LDS column is its own

    const int64_t id = u < a.k ? a.nodes[row * a.k + u] : -1;
    const int gshift = (tid & 63) & ~(UGS_GL_LANES - 1);         // the group's first lane inside the wave
    const unsigned present = (unsigned)(__ballot(id >= 0) >> gshift) & 0xffu;
    const int n = __popc(present);
    int bad = 0;
    uint64_t adj = 0;
    if (n > 0) {
        const int64_t lo = a.edge_ptr[row], hi = a.edge_ptr[row + 1];
        if (lo < 0 || hi < lo || hi > a.num_cols) {
            bad = 1;                                             // not a range of edge_index: nothing is read
        } else {
            for (int64_t e = lo + u; e < hi; e += UGS_GL_LANES) {
                const int64_t x = a.edge_index[e], y = a.edge_index[a.stride + e];
                if (x < 0 || x >= n || y < 0 || y >= n) bad = 1;
                else if (x != y) adj |= (1ull << (8 * (int)x + (int)y)) | (1ull << (8 * (int)y + (int)x));
            }
        }
    }
    for (int d = 1; d < UGS_GL_LANES; d <<= 1) {
        adj |= __shfl_xor(adj, d);
        bad |= __shfl_xor(bad, d);
    }
    const int status = n == 0 ? 1 : bad ? 2 : 0;

    uint32_t val = 1u << 28;                                     // above every code
    if (status == 0 && u < n) {
        LdsStack st{cells_sh + tid};
        val = ugs_gl::rooted(adj, n, u, st);
    }

    uint32_t vals[UGS_GL_LANES];
    uint32_t code = 1u << 28;
    bool first = true;
#pragma unroll
    for (int w = 0; w < UGS_GL_LANES; ++w) {
        vals[w] = (uint32_t)__shfl((int)val, w, UGS_GL_LANES);
        code = min(code, vals[w]);
        first = first && !(w < u && vals[w] == val);
    }
    const unsigned firsts = (unsigned)(__ballot(first) >> gshift) & 0xffu;
    int local = 0;
#pragma unroll
    for (int w = 0; w < UGS_GL_LANES; ++w) local += (int)((firsts >> w) & 1u) & (int)(vals[w] < val);

    const int64_t fill = oa.base[a.table_len];                   // O_k
    const int64_t key = status == 0 ? ((int64_t)n << 28) | (int64_t)code : -1;
    int64_t first_id = fill;
    if (u == 0) {
        int64_t cid = a.table_len;                               // the id of a refused row: len(vocab)
        if (status == 0) {
            int64_t lo_i = 0, hi_i = a.table_len;                // first table key >= key
            while (lo_i < hi_i) {
                const int64_t mid = lo_i + ((hi_i - lo_i) >> 1);
                if (a.table[mid] < key) lo_i = mid + 1; else hi_i = mid;
            }
            if (lo_i < a.table_len && a.table[lo_i] == key) cid = lo_i;
        }
        first_id = oa.base[cid];
        if (a.key) a.key[row] = key;
        if (a.status) a.status[row] = status;
        if (a.cls) a.cls[row] = cid;
    }
    first_id = __shfl(first_id, 0, UGS_GL_LANES);
    const int j = __popc(present & ((1u << u) - 1u));            // the vertex that slot u is, if its entry is >= 0
    const int local_j = __shfl(local, j, UGS_GL_LANES);
    if (u < a.k) oa.orbit[row * a.k + u] = (status == 0 && id >= 0) ? first_id + local_j : fill;
}

struct GlLabelArgs {
    const int64_t *nodes;        // [rows, k]
    const int64_t *edge_index;   // [2, num_cols], row stride `stride`
    int64_t stride, num_cols;
    const int64_t *edge_ptr;     // [rows + 1]
    int64_t rows;
    int k;
    const int64_t *labels;       // [num_labels]
    int64_t num_labels;
    int64_t *key;                // [rows, 2]
    int32_t *status;             // [rows]
    int64_t *orbit;              // [rows, k]; the ORBITS form only
};

// ugs_graphlet_labelled_kernel (law: ugs_graphlet_labelled in the header): the geometry, the row and edge
// reading and the folds of the kernels above.  ORBITS = false writes key and status, ORBITS = true the orbit slots as well.
//   labels  lane s is slot s: it gathers labels[entry], the bounds check before the load, and its vertex is the popcount of the
//           group's ballot below s.  Eight shuffles hand every lane the group's labels.  A slot's cell is the number of distinct
//           smaller labels, its sorted position the number of smaller labels plus that of equal ones in lower slots.  Each slot
//           sets its vertex's bit in its cell's byte and its label's 12 bits at its position; three xor-shuffles OR them into the
//           root partition (ugs_gl::label_cells' word) and the key's 96 label bits;
//   keys    every lane evaluates the root over those cells; lane u owns the subtree below first pick u if the root keeps u: only
//           vertices of the largest label are candidates, so with more than one label fewer lanes search.  Minimum over the group;
//   orbits  lane u < n runs ugs_gl::rooted_cells for vertex u and holds (cell << 28) | rooted code, which orders as (label, code).
//           Eight shuffles hand every lane the group's values; first occurrences, local index and the slot rule as in
//           ugs_graphlet_orbits_kernel.  The canonical code is the smallest rooted code of the last cell;
//   store   lanes 0 and 1 write the two key words, lane 0 the status, lane s orbit slot s.
template <bool ORBITS>
__global__ __launch_bounds__(UGS_GL_BLOCK) void ugs_graphlet_labelled_kernel(GlLabelArgs a) {
    __shared__ uint64_t cells_sh[UGS_GL_KMAX * UGS_GL_BLOCK];
    const int tid = (int)threadIdx.x;
    const int u = tid & (UGS_GL_LANES - 1);                      // slot, vertex and first pick of this lane
    const int64_t row = (int64_t)blockIdx.x * (UGS_GL_BLOCK / UGS_GL_LANES) + (tid >> 3);
    if (row >= a.rows) return;                                   // whole groups leave; no barrier below: a lane's LDS column is its own

    const int64_t id = u < a.k ? a.nodes[row * a.k + u] : -1;
    const int gshift = (tid & 63) & ~(UGS_GL_LANES - 1);         // the group's first lane inside the wave
    const unsigned present = (unsigned)(__ballot(id >= 0) >> gshift) & 0xffu;
    const int n = __popc(present);
    int lab = -1, bad = 0, badlab = 0;
    if (id >= 0) {
        if (id >= a.num_labels) {
            badlab = 1;                                          // no label of that index: nothing is read
        } else {
            const int64_t l = a.labels[id];
            if (l < 0 || l >= 4096) badlab = 1; else lab = (int)l;
        }
    }
    uint64_t adj = 0;
    if (n > 0) {
        const int64_t lo = a.edge_ptr[row], hi = a.edge_ptr[row + 1];
        if (lo < 0 || hi < lo || hi > a.num_cols) {
            bad = 1;                                             // not a range of edge_index: nothing is read
        } else {
            for (int64_t e = lo + u; e < hi; e += UGS_GL_LANES) {
                const int64_t x = a.edge_index[e], y = a.edge_index[a.stride + e];
                if (x < 0 || x >= n || y < 0 || y >= n) bad = 1;
                else if (x != y) adj |= (1ull << (8 * (int)x + (int)y)) | (1ull << (8 * (int)y + (int)x));
            }
        }
    }

    // the root partition and the sorted labels; a slot without a label (lab = -1) takes no part
    int cell = 0, pos = 0;
    {
        int labs[UGS_GL_LANES];
#pragma unroll
        for (int w = 0; w < UGS_GL_LANES; ++w) labs[w] = __shfl(lab, w, UGS_GL_LANES);
#pragma unroll
        for (int w = 0; w < UGS_GL_LANES; ++w) {
            bool first = labs[w] >= 0;                           // no lower slot holds this label
#pragma unroll
            for (int x = 0; x < w; ++x) first = first && labs[x] != labs[w];
            const bool below = labs[w] >= 0 && labs[w] < lab;
            cell += (int)(first && below);
            pos += (int)below + (int)(w < u && labs[w] == lab);
        }
    }
    const int j = __popc(present & ((1u << u) - 1u));            // the vertex that slot u is, if its entry is >= 0
    uint64_t cells = 0, lab_lo = 0, lab_hi = 0;                  // the labels' bits 0 .. 63 and 64 .. 95 of the key
    if (lab >= 0) {
        cells = 1ull << (8 * cell + j);
        const int at = 12 * pos;
        if (at < 64) lab_lo = (uint64_t)lab << at;               // position 5 straddles the words: its high 8 bits fall off here
        if (at + 12 > 64) lab_hi = at >= 64 ? (uint64_t)lab << (at - 64) : (uint64_t)lab >> (64 - at);
    }
    for (int d = 1; d < UGS_GL_LANES; d <<= 1) {                 // the group's lanes are all here: n and the row are theirs alike
        adj |= __shfl_xor(adj, d);
        bad |= __shfl_xor(bad, d);
        badlab |= __shfl_xor(badlab, d);
        cells |= __shfl_xor(cells, d);
        lab_lo |= __shfl_xor(lab_lo, d);
        lab_hi |= __shfl_xor(lab_hi, d);
    }
    const int status = n == 0 ? 1 : bad ? 2 : badlab ? 3 : 0;

    uint32_t code = 1u << 28;                                    // above every code
    int local = 0;
    if (!ORBITS) {
        if (status == 0) {
            if (n == 1) {
                code = 0;
            } else {
                uint32_t tied, col;
                ugs_gl::eval_node(adj, cells, tied, col);
                if (n == 2) {
                    code = col;                                  // the root is the last level with a column
                } else if ((tied >> u) & 1u) {
                    LdsStack st{cells_sh + tid};
                    code = ugs_gl::search(adj, ugs_gl::split_cells(adj, cells, u), n - 2, col << ugs_gl::tri(n - 1), st);
                }
            }
            for (int d = 1; d < UGS_GL_LANES; d <<= 1) code = min(code, (uint32_t)__shfl_xor((int)code, d));
        }
    } else {
        uint32_t val = 0xffffffffu;                              // above every (cell, code) pair, and of no cell
        uint32_t last = 0;
        if (status == 0) {
            last = (uint32_t)(63 - __builtin_clzll(cells)) >> 3;
            if (u < n) {
                LdsStack st{cells_sh + tid};
                uint32_t mine = 0;
#pragma unroll
                for (int i = 1; i < UGS_GL_KMAX; ++i) mine = ((cells >> (8 * i + u)) & 1ull) ? (uint32_t)i : mine;
                val = (mine << 28) | ugs_gl::rooted_cells(adj, cells, n, u, st);
            }
        }
        uint32_t vals[UGS_GL_LANES];
        bool first = true;
#pragma unroll
        for (int w = 0; w < UGS_GL_LANES; ++w) {
            vals[w] = (uint32_t)__shfl((int)val, w, UGS_GL_LANES);
            if ((vals[w] >> 28) == last) code = min(code, vals[w] & ((1u << 28) - 1u));
            first = first && !(w < u && vals[w] == val);
        }
        const unsigned firsts = (unsigned)(__ballot(first) >> gshift) & 0xffu;
#pragma unroll
        for (int w = 0; w < UGS_GL_LANES; ++w) local += (int)((firsts >> w) & 1u) & (int)(vals[w] < val);
    }

    if (u < 2) {
        const int64_t hi = (int64_t)(((uint64_t)n << 60) | ((uint64_t)code << 32) | lab_hi);
        a.key[row * 2 + u] = status != 0 ? -1 : u == 0 ? hi : (int64_t)lab_lo;
    }
    if (u == 0) a.status[row] = status;
    if (ORBITS) {
        const int local_j = __shfl(local, j, UGS_GL_LANES);
        if (u < a.k) a.orbit[row * a.k + u] = (status == 0 && id >= 0) ? (int64_t)local_j : (int64_t)a.k;
    }
}

// ugs_graphlet_census_table_kernel (ugs_graphlet_census in the header): one lane per raw adjacency code of n
// vertices.  It runs the whole canonical search alone -- the table is built once per device and n, 2^21 codes at most -- and a binary
// search among the ascending keys of the connected graphs on n vertices gives the code's column, 0xFFFF for a graph that is not one.
__global__ __launch_bounds__(UGS_GL_BLOCK) void ugs_graphlet_census_table_kernel(int n, const int64_t *keys, int64_t num_keys, uint16_t *out) {
    __shared__ uint64_t cells_sh[UGS_GL_KMAX * UGS_GL_BLOCK];
    const int tid = (int)threadIdx.x;
    const uint32_t code = blockIdx.x * UGS_GL_BLOCK + (uint32_t)tid;
    if (code >> ugs_gl::tri(n)) return;                          // no barrier below: a lane's LDS column is its own
    LdsStack st{cells_sh + tid};
    const int64_t key = ((int64_t)n << 28) | (int64_t)ugs_gl::canon(ugs_gl::adj_of_code(code, n), n, st);
    int64_t lo_i = 0, hi_i = num_keys;                           // first key >= key
    while (lo_i < hi_i) {
        const int64_t mid = lo_i + ((hi_i - lo_i) >> 1);
        if (keys[mid] < key) lo_i = mid + 1; else hi_i = mid;
    }
    out[code] = lo_i < num_keys && keys[lo_i] == key ? (uint16_t)lo_i : (uint16_t)0xFFFFu;
}

// ugs_graphlet_vertex_census_table_kernel (ugs_graphlet_vertex_census in the header): one lane per raw
// adjacency code of n vertices, as above, and besides the column the local orbit index of every position: ugs_gl::vertex_entry, the
// code path of the host's ugs_graphlet_vertex_census_entry.  n + 1 searches a lane, once per device and n.
__global__ __launch_bounds__(UGS_GL_BLOCK) void ugs_graphlet_vertex_census_table_kernel(int n, const int64_t *keys, int64_t num_keys, uint32_t *out) {
    __shared__ uint64_t cells_sh[UGS_GL_KMAX * UGS_GL_BLOCK];
    const int tid = (int)threadIdx.x;
    const uint32_t code = blockIdx.x * UGS_GL_BLOCK + (uint32_t)tid;
    if (code >> ugs_gl::tri(n)) return;                          // no barrier below: a lane's LDS column is its own
    LdsStack st{cells_sh + tid};
    out[code] = ugs_gl::vertex_entry(code, n, keys, num_keys, st);
}

}  // namespace

extern "C" int ugs_graphlet_vertex_census_table(int n, const int64_t *d_keys, int64_t num_keys, uint32_t *d_table_out) {
    if (n < 1 || n >= UGS_GL_KMAX) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_vertex_census_table: 1 <= n <= 7");
    if (!d_keys || !d_table_out || num_keys < 1 || num_keys > (1 << ugs_gl::VERTEX_COL_BITS))
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_vertex_census_table: keys (1 ... 1024 of them) and the output are needed");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    const uint32_t codes = 1u << ugs_gl::tri(n);
    hipLaunchKernelGGL(ugs_graphlet_vertex_census_table_kernel, dim3((codes + UGS_GL_BLOCK - 1) / UGS_GL_BLOCK), dim3(UGS_GL_BLOCK), 0, s,
                       n, d_keys, num_keys, d_table_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}

extern "C" int ugs_graphlet_census_table(int n, const int64_t *d_keys, int64_t num_keys, uint16_t *d_code_col_out) {
    if (n < 1 || n >= UGS_GL_KMAX) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_census_table: 1 <= n <= 7");
    if (!d_keys || !d_code_col_out || num_keys < 1 || num_keys >= 0xFFFF)
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_census_table: keys (1 ... 65534 of them) and the output are needed");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    const uint32_t codes = 1u << ugs_gl::tri(n);
    hipLaunchKernelGGL(ugs_graphlet_census_table_kernel, dim3((codes + UGS_GL_BLOCK - 1) / UGS_GL_BLOCK), dim3(UGS_GL_BLOCK), 0, s, n,
                       d_keys, num_keys, d_code_col_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}

extern "C" int ugs_graphlet_labelled(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                                     const int64_t *d_edge_ptr, int64_t rows, int k, const int64_t *d_labels, int64_t num_labels,
                                     int64_t *d_key_out, int32_t *d_status_out, int64_t *d_orbit_out) {
    if (k < 1 || k > UGS_GL_KMAX) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_labelled: 1 <= k <= 8");
    if (rows < 0 || num_cols < 0 || (num_cols > 0 && row_stride < num_cols))
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_labelled: rows >= 0, num_cols >= 0, row_stride >= num_cols");
    if (num_labels < 0 || (num_labels > 0 && !d_labels)) return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_labelled: num_labels >= 0, and labels for num_labels > 0");
    if (rows == 0) return UGS_OK;
    if (!d_nodes || !d_edge_ptr || !d_key_out || !d_status_out || (num_cols > 0 && !d_edge_index))
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_labelled: null pointer");
    const int64_t per_block = UGS_GL_BLOCK / UGS_GL_LANES;
    const int64_t blocks = (rows + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_labelled: too many rows for one launch");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    GlLabelArgs a{};
    a.nodes = d_nodes; a.edge_index = d_edge_index; a.stride = row_stride; a.num_cols = num_cols; a.edge_ptr = d_edge_ptr;
    a.rows = rows; a.k = k; a.labels = d_labels; a.num_labels = num_labels;
    a.key = d_key_out; a.status = d_status_out; a.orbit = d_orbit_out;
    if (d_orbit_out) hipLaunchKernelGGL(ugs_graphlet_labelled_kernel<true>, dim3((unsigned)blocks), dim3(UGS_GL_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(ugs_graphlet_labelled_kernel<false>, dim3((unsigned)blocks), dim3(UGS_GL_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}

extern "C" int ugs_graphlet_orbits(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                                   const int64_t *d_edge_ptr, int64_t rows, int k, const int64_t *d_table, const int64_t *d_base,
                                   int64_t table_len, int64_t *d_orbit_out, int64_t *d_key_out, int32_t *d_status_out,
                                   int64_t *d_class_out) {
    if (k < 1 || k > UGS_GL_KMAX) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_orbits: 1 <= k <= 8");
    if (rows < 0 || num_cols < 0 || (num_cols > 0 && row_stride < num_cols))
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_orbits: rows >= 0, num_cols >= 0, row_stride >= num_cols");
    if (table_len < 0) return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_orbits: table_len >= 0");
    if (rows == 0) return UGS_OK;
    if (!d_nodes || !d_edge_ptr || !d_orbit_out || !d_base || (table_len > 0 && !d_table) || (num_cols > 0 && !d_edge_index))
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_orbits: null pointer");
    const int64_t per_block = UGS_GL_BLOCK / UGS_GL_LANES;
    const int64_t blocks = (rows + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_orbits: too many rows for one launch");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    GlOrbitArgs oa{};
    GlArgs &a = oa.g;
    a.nodes = d_nodes; a.edge_index = d_edge_index; a.stride = row_stride; a.num_cols = num_cols; a.edge_ptr = d_edge_ptr;
    a.rows = rows; a.k = k; a.table = d_table; a.table_len = table_len;
    a.key = d_key_out; a.status = d_status_out; a.cls = d_class_out;
    oa.base = d_base; oa.orbit = d_orbit_out;
    hipLaunchKernelGGL(ugs_graphlet_orbits_kernel, dim3((unsigned)blocks), dim3(UGS_GL_BLOCK), 0, s, oa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}

extern "C" int ugs_graphlet_canon(const int64_t *d_nodes, const int64_t *d_edge_index, int64_t row_stride, int64_t num_cols,
                                  const int64_t *d_edge_ptr, int64_t rows, int k, const int64_t *d_table, int64_t table_len,
                                  int64_t *d_key_out, int32_t *d_status_out, int64_t *d_class_out) {
    if (k < 1 || k > UGS_GL_KMAX) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_canon: 1 <= k <= 8");
    if (rows < 0 || num_cols < 0 || (num_cols > 0 && row_stride < num_cols))
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_canon: rows >= 0, num_cols >= 0, row_stride >= num_cols");
    if (table_len < 0 || (d_class_out && !d_table && table_len > 0)) return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_canon: a class output needs the key table");
    if (rows == 0) return UGS_OK;
    if (!d_nodes || !d_edge_ptr || !d_key_out || !d_status_out || (num_cols > 0 && !d_edge_index))
        return ugs_internal_fail(UGS_E_BAD_ARG, "graphlet_canon: null pointer");
    const int64_t per_block = UGS_GL_BLOCK / UGS_GL_LANES;
    const int64_t blocks = (rows + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return ugs_internal_fail(UGS_E_UNSUPPORTED, "graphlet_canon: too many rows for one launch");
    hipStream_t s = nullptr;
    if (int rc = ugs_internal_ctx(nullptr, &s)) return rc;
    GlArgs a{};
    a.nodes = d_nodes; a.edge_index = d_edge_index; a.stride = row_stride; a.num_cols = num_cols; a.edge_ptr = d_edge_ptr;
    a.rows = rows; a.k = k; a.table = d_table; a.table_len = d_table ? table_len : 0;
    a.key = d_key_out; a.status = d_status_out; a.cls = d_class_out;
    hipLaunchKernelGGL(ugs_graphlet_canon_kernel, dim3((unsigned)blocks), dim3(UGS_GL_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ugs_internal_fail(UGS_E_HIP, hipGetErrorString(e));
    return UGS_OK;
}
