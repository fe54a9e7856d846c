// ugs_census_csr.hip -- the graphlet census and vertex census of graphs of any size, searched over adjacency lists (ugs_graphlet_census_csr
// and ugs_graphlet_vertex_census_csr in include/ugs_mi355.h, which states the law).
//
// The search is the extension-set search of uni_census_esu (ugs_uniform.hip) without the extension set.  The placed vertices p0 ...
// p(d-1) are ids, p0 the root.  Their extension list is a concatenation, for i = 0 ... d-1, of the entries u of p_i's row with u > root
// that are adjacent to none of p0 ... p(i-1) and are none of the placed vertices: every vertex above the root that touches the placed
// set stands in it once, in the row of its first placed neighbour.  A position in the list is a cursor (row i, offset t into col); a
// child starts behind its parent's cursor and sees the rest of the parent's list plus the row of the vertex it placed -- ESU's
// ext' = (ext after w) + (neighbours of w above the root that touch nothing placed before), so every connected set is met once.
// A candidate's column against the placed vertices -- the bits its raw code needs -- is d membership tests, each a binary search in a
// sorted row; bit i is known (the candidate stands in p_i's row), the bits below i decide validity and are tested first.
//
//   csr_validate        one lane per vertex / entry / graph: the preconditions of the CSR, before any search reads through it
//   csr_census_esu      one wave per item -- a CSR entry e: root v = its row, first extension w0 = col[e] > v; the lanes split the list of
//                       {v, w0} -- and 1 ... 32 consecutive entries a wave; W counters in LDS, flushed to the graph's row
//   csr_vcensus_esu     the same search; every set adds to the rows of its k members in gdv
//   csr_single          k = 1: every vertex is a set
//   csr_*_clear         behind the pass, in a call where some graph went past the budget: such a graph has zeros
// The levels are an unrolled recursion (one inlined copy per depth, the arrays indexed by unrolled loops only): no indexed stack.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ugs_census_csr.h"
#include "ugs_graphlet_common.h"

namespace {

constexpr int CSR_BLOCK = 64;                     // one wave per item
constexpr int CSR_AUX_BLOCK = 256;
constexpr int CSR_ROWS = UGS_GL_KMAX - 2;         // k <= 7: six vertices at most are placed before the leaf

// first position in col[lo, hi) whose entry is >= x
__device__ __forceinline__ uint32_t csr_lower(const int32_t *col, uint32_t lo, uint32_t hi, int32_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool csr_has(const int32_t *col, uint32_t lo, uint32_t hi, int32_t x) {
    const uint32_t at = csr_lower(col, lo, hi, x);
    return at < hi && col[at] == x;
}

// the last index i in [0, n) with a[i] <= x, for a non-decreasing a [n + 1] with a[0] <= x < a[n]; in [0, n) whatever a holds
__device__ __forceinline__ int64_t csr_owner(const int64_t *a, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid + 1] > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(CSR_AUX_BLOCK) void csr_validate(UgsCsrCall c) {
    const int64_t i = (int64_t)blockIdx.x * CSR_AUX_BLOCK + threadIdx.x;
    bool bad = false;
    if (i <= c.G) {
        if (i == 0 && c.ptr[0] < 0) bad = true;
        if (i == c.G && c.ptr[i] != c.N) bad = true;
        if (i < c.G && c.ptr[i] > c.ptr[i + 1]) bad = true;
    }
    if (i <= c.N) {
        const int64_t a = c.rowptr[i];
        if (a < 0 || a > c.M || (i == 0 && a != 0) || (i == c.N && a != c.M)) bad = true;
        if (i < c.N && a > c.rowptr[i + 1]) bad = true;
    }
    if (i < c.M && c.N > 0 && c.G > 0) {
        const int64_t u = (int64_t)c.col[i];
        const int64_t r = csr_owner(c.rowptr, c.N, i);                  // the entry's row, if rowptr is sound
        const int64_t a = c.rowptr[r], b = c.rowptr[r + 1];
        const int64_t g = csr_owner(c.ptr, c.G, r);
        const int64_t lo = c.ptr[g], hi = c.ptr[g + 1];
        if (!(0 <= a && a <= i && i < b && b <= c.M) || !(lo <= r && r < hi)) {  // (a >= 0: col[i - 1] below is read only for i > a)
            bad = true;
        } else if (u < 0 || u >= c.N || u < lo || u >= hi || u == r || (i > a && (int64_t)c.col[i - 1] >= u)) {
            bad = true;
        } else {
            const int64_t ua = c.rowptr[u], ub = c.rowptr[u + 1];
            if (ua < 0 || ub < ua || ub > c.M || !csr_has(c.col, (uint32_t)ua, (uint32_t)ub, (int32_t)r)) bad = true;   // the mirror
        }
    } else if (i < c.M) {
        bad = true;                                                     // entries without a vertex or a graph to own them
    }
    if (bad) *c.flag = 1;
}

// ---- the search ------------------------------------------------------------------------------------------------------------------------
struct CsrWalk {
    const int32_t *col;
    const int64_t *rowptr;
    int32_t root;
    int32_t p[CSR_ROWS];                          // the placed vertices, by position
    uint32_t lo[CSR_ROWS], hi[CSR_ROWS];          // their rows: col[lo, hi), entered at the first entry above the root (row 0: whole)
    uint64_t cnt, flushed;                        // this lane's sets, and how many of them it has added to the graph's running total
    unsigned long long *ctr;
    unsigned long long budget;
    uint32_t stop;                                // 1: the graph is past the limit (a number, not a flag: it lives in a VGPR)
};

// where a lane's completed sets go.  emit<D>: the set of the D placed vertices and u, whose raw code is `code`; end_leaf<D>: the placed
// vertices are about to change; done: the lane has finished.

// the census: one 16-bit table load, equal columns in a row merged into one add to the workgroup's counters in LDS
struct CsrCensusSink {
    const uint16_t *code_col;
    uint32_t W;
    unsigned long long *hist;
    uint32_t run_col, run;
    __device__ __forceinline__ void flush() {
        if (run && run_col < W) atomicAdd(&hist[run_col], (unsigned long long)run);
        run = 0;
    }
    template <int D>
    __device__ __forceinline__ void emit(const CsrWalk &, uint32_t code, int32_t) {
        const uint32_t c = code_col[code];
        if (c != run_col) { flush(); run_col = c; }
        ++run;
    }
    template <int D>
    __device__ __forceinline__ void end_leaf(const CsrWalk &) {}
    __device__ __forceinline__ void done() { flush(); }
};

// the vertex census: one 32-bit table load (ugs_gl::vertex_entry), one add for the member, and for the D placed vertices one add of the
// run's length per run of equal entries
struct CsrVertexSink {
    const uint32_t *table;
    const int64_t *obase;
    unsigned long long *gdv;
    int64_t O;
    uint32_t W;
    uint32_t run_entry, run;
    int64_t ob;
    template <int D>
    __device__ __forceinline__ void flush(const CsrWalk &x) {
        if (run && ugs_gl::vertex_col(run_entry) < W) {
#pragma unroll
            for (int q = 0; q < D; ++q)
                atomicAdd(&gdv[(int64_t)x.p[q] * O + ob + ugs_gl::vertex_local(run_entry, q)], (unsigned long long)run);
        }
        run = 0;
    }
    template <int D>
    __device__ __forceinline__ void emit(const CsrWalk &x, uint32_t code, int32_t u) {
        const uint32_t entry = table[code];
        const bool known = ugs_gl::vertex_col(entry) < W;               // (a set the search completes is connected: its entry has a column)
        if (entry != run_entry) {
            flush<D>(x);
            run_entry = entry;
            ob = known ? obase[ugs_gl::vertex_col(entry)] : 0;
        }
        ++run;
        if (known) atomicAdd(&gdv[(int64_t)u * O + ob + ugs_gl::vertex_local(entry, D)], 1ull);
    }
    template <int D>
    __device__ __forceinline__ void end_leaf(const CsrWalk &x) { flush<D>(x); }
    __device__ __forceinline__ void done() {}
};

// Picking a level's row by its number is arithmetic, not compares: a compare's result is a lane mask in two SGPRs, and the masks of
// five inlined levels do not fit the scalar file.  csr_is(i, j): all ones where i == j, for 0 <= i, j < 2^31; csr_pick: a where m.
__device__ __forceinline__ uint32_t csr_is(int i, int j) { return 0u - ((((uint32_t)i ^ (uint32_t)j) - 1u) >> 31); }
__device__ __forceinline__ uint32_t csr_pick(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }

template <int K, int D, class Sink>
__device__ __forceinline__ void csr_walk(CsrWalk &x, Sink &s, int ci, uint32_t ct, uint32_t code);

// the candidate col[t] of row i against the D placed vertices: a leaf's set, or the next level.  `skip` (all ones): there is no
// candidate (the walk is between two rows; t is any valid position) -- a value, not a branch around the call, to keep the levels'
// control flow flat.  The flags of this function are numbers (all ones or zero; csr_neg: the sign of a difference of two values
// below 2^31), for the reason csr_is gives: what is left to lane masks is one loop, one branch and the leaf.
__device__ __forceinline__ uint32_t csr_neg(uint32_t x) { return 0u - (x >> 31); }

template <int K, int D, class Sink>
__device__ __forceinline__ void csr_visit(CsrWalk &x, Sink &s, int i, uint32_t t, uint32_t code, uint32_t skip) {
    const int32_t u = x.col[t];
    // the D membership tests run side by side: one loop, their loads in flight together (a finished search rereads the candidate).
    // Row i is searched like the others (u stands in it, so bit i comes out set): leaving it out would take a compare with i per row.
    // Above the leaf the same loop finds where u's own row is entered, its first entry above the root, should u be placed.
    uint32_t l[D], h[D], adj = 0, rl = 0, rh = 0, rend = 0;
    if constexpr (D < K - 1) { rl = (uint32_t)x.rowptr[u]; rend = rh = (uint32_t)x.rowptr[(int64_t)u + 1]; }
    uint32_t bad = skip;                                                // ... or u is one of the placed vertices
#pragma unroll
    for (int j = 0; j < D; ++j) { l[j] = x.lo[j]; h[j] = x.hi[j]; bad |= csr_is(u, x.p[j]); }
    uint32_t more = ~bad;
    while (more != 0u) {
        more = 0u;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const uint32_t open = csr_neg(l[j] - h[j]);                 // l < h
            const uint32_t mid = l[j] + ((h[j] - l[j]) >> 1);
            const uint32_t at = (uint32_t)x.col[csr_pick(open, mid, t)];
            const uint32_t below = open & csr_neg(at - (uint32_t)u), above = open & csr_neg((uint32_t)u - at), hit = open & ~below & ~above;
            adj |= (hit & 1u) << j;
            l[j] = csr_pick(below, mid + 1u, l[j]);
            h[j] = csr_pick(hit, l[j], csr_pick(above, mid, h[j]));
            more |= open;
        }
        if constexpr (D < K - 1) {
            const uint32_t open = csr_neg(rl - rh);
            const uint32_t mid = rl + ((rh - rl) >> 1);
            const uint32_t at = (uint32_t)x.col[csr_pick(open, mid, t)];
            const uint32_t below = open & ~csr_neg((uint32_t)x.root - at);     // at <= root
            rh = csr_pick(open & ~below, mid, rh);
            rl = csr_pick(below, mid + 1u, rl);
            more |= open;
        }
    }
    if ((bad | (adj & ((1u << i) - 1u))) != 0u) return;                 // an earlier row holds it: it stands there, not here
    code |= adj << ugs_gl::tri(D);
    if constexpr (D == K - 1) {
        s.template emit<D>(x, code, u);
        ++x.cnt;
        if (x.cnt - x.flushed >= 4096) {                                // bounded work for a graph over the limit, as in cen_last
            const unsigned long long add = x.cnt - x.flushed;
            x.flushed = x.cnt;
            if (atomicAdd(x.ctr, add) + add > x.budget) x.stop = 1u;
        }
    } else {
        x.p[D] = u;
        x.lo[D] = rl;
        x.hi[D] = rend;
        csr_walk<K, D + 1, Sink>(x, s, i, t + 1, code);
    }
}

// the extension list of the D placed vertices from the cursor (row ci, offset ct) on
template <int K, int D, class Sink>
__device__ __forceinline__ void csr_walk(CsrWalk &x, Sink &s, int ci, uint32_t ct, uint32_t code) {
    int i = ci;
    uint32_t t = ct, end = 0;
#pragma unroll
    for (int j = 0; j < D; ++j) end = csr_pick(csr_is(i, j), x.hi[j], end);
    while (i + (int)(x.stop << 3) < D) {                                // (a graph past the limit: every level's list is done)
        const uint32_t roll = csr_neg(end - t - 1u);                    // t = end (t never passes it): the row is done, the next one is
        i += (int)(roll & 1u);                                          // entered above the root
#pragma unroll
        for (int j = 1; j < D; ++j) { const uint32_t m = roll & csr_is(i, j); t = csr_pick(m, x.lo[j], t); end = csr_pick(m, x.hi[j], end); }
        const uint32_t at = csr_pick(roll, ct - 1u, t);                 // (ct - 1: the position this level was entered from)
        t += ~roll & 1u;                                                // before the visit: nothing of `roll` lives across the levels below
        csr_visit<K, D, Sink>(x, s, i, at, code, roll);
    }
    if constexpr (D == K - 1) s.template end_leaf<D>(x);
}

// the item of entry e of row v: root v, first extension w0 = col[e]; false (for the whole wave) where w0 <= v
__device__ __forceinline__ bool csr_item(const UgsCsrCall &c, uint32_t e, int64_t v, CsrWalk &x) {
    const int32_t w0 = c.col[e];
    if ((int64_t)w0 <= v) return false;
    x.root = (int32_t)v;
    x.p[0] = (int32_t)v; x.lo[0] = (uint32_t)c.rowptr[v]; x.hi[0] = (uint32_t)c.rowptr[v + 1];
    x.p[1] = w0; x.hi[1] = (uint32_t)c.rowptr[(int64_t)w0 + 1];
    x.lo[1] = csr_lower(c.col, (uint32_t)c.rowptr[w0], x.hi[1], (int32_t)v + 1);
    return true;
}

// lane j of the item's wave: k = 2, the item is the set (lane 0); k >= 3, every 64th candidate of the list of {v, w0}
template <int K, class Sink>
__device__ __forceinline__ void csr_lane(CsrWalk &x, Sink &s, uint32_t e, int j) {
    if (*(volatile unsigned long long *)x.ctr > x.budget) return;       // a graph already past the limit starts nothing more
    if constexpr (K == 2) {
        if (j == 0) { s.template emit<1>(x, 1u, x.p[1]); s.template end_leaf<1>(x); ++x.cnt; }
    } else {
        const uint32_t n0 = x.hi[0] - (e + 1u), n = n0 + (x.hi[1] - x.lo[1]);         // two disjoint pieces of col: n <= M < 2^31
        for (uint32_t t = (uint32_t)j; t < n && x.stop == 0u; t += CSR_BLOCK) {
            const bool first = t < n0;
            csr_visit<K, 2, Sink>(x, s, first ? 0 : 1, first ? e + 1u + t : x.lo[1] + (t - n0), 1u, 0u);
        }
        if constexpr (K == 3) s.template end_leaf<2>(x);
    }
}

// A workgroup's items: the `chunk` consecutive entries from blockIdx.x * chunk on, one after the other -- rows ascend with the
// entries, graphs with the rows, so the row and the graph are searched for once and then stepped.  What a workgroup has gathered for a
// graph -- the lanes' set counts, and whatever the sink's `turn` hands over -- goes to the graph once, when the graph changes and at
// the end: a graph of many entries is not one address that every item adds to.
// (The loop's own state -- entry, row, graph and their ends, all below 2^31 -- is kept in VGPRs, csr_in_vgpr: it is the same in every
// lane, and left to itself the compiler holds it, and everything csr_item derives from it, in SGPRs, which the search needs for its
// lane masks.)
__device__ __forceinline__ uint32_t csr_in_vgpr(uint32_t x) { asm volatile("" : "+v"(x)); return x; }

// The lanes' sets not yet added to the graph's running total, as one add a wave: with the loop's state in VGPRs the compiler no longer
// sees that all lanes add to one address, and 64 adds a workgroup to a large graph's one counter are what the chunks are there to avoid.
__device__ __forceinline__ void csr_count_out(CsrWalk &x, int j) {
    unsigned long long sum = x.cnt - x.flushed;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        sum += ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(sum >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)sum, o);
    if (j == 0 && sum) atomicAdd(x.ctr, sum);
    x.flushed = x.cnt;
}

template <int K, class Sink, class Turn>
__device__ __forceinline__ void csr_chunk(const UgsCsrCall &c, uint32_t chunk, Sink &s, Turn turn) {
    const int j = (int)threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * chunk;
    const int64_t v0 = csr_owner(c.rowptr, c.N, e0), g0 = csr_owner(c.ptr, c.G, v0);
    const uint32_t e1 = csr_in_vgpr((uint32_t)(e0 + chunk < c.M ? e0 + chunk : c.M));
    uint32_t v = csr_in_vgpr((uint32_t)v0), g = csr_in_vgpr((uint32_t)g0);
    uint32_t vend = (uint32_t)c.rowptr[(int64_t)v + 1], gend = (uint32_t)c.ptr[(int64_t)g + 1];
    CsrWalk x;
    x.col = c.col; x.rowptr = c.rowptr;
#pragma unroll
    for (int i = 0; i < CSR_ROWS; ++i) { x.p[i] = 0; x.lo[i] = 0; x.hi[i] = 0; }
    x.cnt = 0; x.flushed = 0; x.stop = 0u;
    x.ctr = &c.gcount[g]; x.budget = c.budget;
    for (uint32_t e = csr_in_vgpr((uint32_t)e0); e < e1; ++e) {
        while (e >= vend) { ++v; vend = (uint32_t)c.rowptr[(int64_t)v + 1]; }
        if (v >= gend) {
            s.done();
            csr_count_out(x, j);
            turn((int64_t)g);
            g = csr_in_vgpr((uint32_t)csr_owner(c.ptr, c.G, (int64_t)v));
            gend = (uint32_t)c.ptr[(int64_t)g + 1];
            x.cnt = 0; x.flushed = 0; x.stop = 0u;
            x.ctr = &c.gcount[g];
        }
        if (csr_item(c, e, (int64_t)v, x)) csr_lane<K>(x, s, e, j);
    }
    s.done();
    csr_count_out(x, j);
    turn((int64_t)g);
}

template <int K>
__global__ __launch_bounds__(CSR_BLOCK) void csr_census_esu(UgsCsrCall c, UgsCensus z, uint32_t chunk) {
    extern __shared__ unsigned long long csr_sh[];                      // W counters
    const uint32_t W = (uint32_t)z.W, j = threadIdx.x;
    for (uint32_t i = j; i < W; i += CSR_BLOCK) csr_sh[i] = 0;
    __syncthreads();
    CsrCensusSink s;
    s.code_col = z.code_col; s.W = W; s.hist = csr_sh; s.run_col = 0xFFFFu; s.run = 0;
    csr_chunk<K>(c, chunk, s, [&](int64_t g) {                          // the workgroup's counters to graph g's row, and zero again
        __syncthreads();
        unsigned long long *dst = z.counts + g * (int64_t)W;
        for (uint32_t i = j; i < W; i += CSR_BLOCK) {
            const unsigned long long n = csr_sh[i];
            if (n) { atomicAdd(&dst[i], n); csr_sh[i] = 0; }
        }
        __syncthreads();
    });
}

template <int K>
__global__ __launch_bounds__(CSR_BLOCK) void csr_vcensus_esu(UgsCsrCall c, UgsVertexCensus z, uint32_t chunk) {
    CsrVertexSink s;
    s.table = z.table; s.obase = z.obase; s.gdv = z.gdv; s.O = z.O; s.W = (uint32_t)z.W;
    s.run_entry = ugs_gl::VERTEX_NONE; s.run = 0; s.ob = 0;
    csr_chunk<K>(c, chunk, s, [](int64_t) {});
}

// k = 1: every vertex is a set.  Lane i: graph i's count (and its census cell), vertex i's cell of gdv; `counts` or `gdv` is null.
__global__ __launch_bounds__(CSR_AUX_BLOCK) void csr_single(UgsCsrCall c, const uint16_t *code_col, unsigned long long *counts, int64_t W,
                                                            const uint32_t *table, const int64_t *obase, unsigned long long *gdv, int64_t O) {
    const int64_t i = (int64_t)blockIdx.x * CSR_AUX_BLOCK + threadIdx.x;
    if (i < c.G) {
        const unsigned long long n = (unsigned long long)(c.ptr[i + 1] - c.ptr[i]);
        c.gcount[i] = n;
        if (counts) {
            const uint32_t col = code_col[0];
            if ((int64_t)col < W) counts[i * W + col] = n;
        }
    }
    if (gdv && i >= c.ptr[0] && i < c.N) {
        const uint32_t entry = table[0];
        if ((int64_t)ugs_gl::vertex_col(entry) < W) gdv[i * O + obase[ugs_gl::vertex_col(entry)] + ugs_gl::vertex_local(entry, 0)] = 1ull;
    }
}

// behind the pass: the row of a graph past the budget is zero
__global__ __launch_bounds__(CSR_AUX_BLOCK) void csr_census_clear(UgsCsrCall c, UgsCensus z) {
    const int64_t i = (int64_t)blockIdx.x * CSR_AUX_BLOCK + threadIdx.x;
    if (i < c.G * z.W && c.gcount[i / z.W] > c.budget) z.counts[i] = 0;
}

// ... and the rows of all its vertices.  blockIdx.x: the graph; the workgroups of one graph share its cells.
__global__ __launch_bounds__(CSR_AUX_BLOCK) void csr_vcensus_clear(UgsCsrCall c, UgsVertexCensus z) {
    const int64_t g = (int64_t)blockIdx.x;
    if (c.gcount[g] <= c.budget) return;
    const int64_t lo = c.ptr[g], cells = (c.ptr[g + 1] - lo) * z.O;
    unsigned long long *rows = z.gdv + lo * z.O;
    for (int64_t i = (int64_t)blockIdx.y * CSR_AUX_BLOCK + threadIdx.x; i < cells; i += (int64_t)gridDim.y * CSR_AUX_BLOCK) rows[i] = 0;
}

inline unsigned csr_blocks(int64_t n) { return (unsigned)((n + CSR_AUX_BLOCK - 1) / CSR_AUX_BLOCK); }

// entries a workgroup: one while the call has fewer than 2^16 of them -- a small batch wants every wave it can get -- then as many
// as keep 2^16 workgroups, 32 at the most (a 1 M-vertex graph of 40 M entries: 1.25 M workgroups)
inline uint32_t csr_chunk_of(int64_t M) { return (uint32_t)std::min<int64_t>(std::max<int64_t>(M >> 16, 1), 32); }

}  // namespace

hipError_t ugs_census_csr_validate(const UgsCsrCall &c, hipStream_t s) {
    const int64_t lanes = std::max(std::max(c.G, c.N) + 1, c.M);
    hipLaunchKernelGGL(csr_validate, dim3(csr_blocks(lanes)), dim3(CSR_AUX_BLOCK), 0, s, c);
    return hipGetLastError();
}

hipError_t ugs_census_csr_census(const UgsCsrCall &c, const UgsCensus &z, hipStream_t s) {
    if (c.G <= 0) return hipSuccess;
    if (c.k == 1) {
        hipLaunchKernelGGL(csr_single, dim3(csr_blocks(c.G)), dim3(CSR_AUX_BLOCK), 0, s, c, z.code_col, z.counts, z.W,
                           (const uint32_t *)nullptr, (const int64_t *)nullptr, (unsigned long long *)nullptr, (int64_t)0);
    } else if (c.M > 0) {
        const uint32_t chunk = csr_chunk_of(c.M);
        const dim3 grid((unsigned)((c.M + chunk - 1) / chunk)), block(CSR_BLOCK);
        const size_t lds = (size_t)z.W * sizeof(unsigned long long);
        switch (c.k) {
        case 2: hipLaunchKernelGGL(csr_census_esu<2>, grid, block, lds, s, c, z, chunk); break;
        case 3: hipLaunchKernelGGL(csr_census_esu<3>, grid, block, lds, s, c, z, chunk); break;
        case 4: hipLaunchKernelGGL(csr_census_esu<4>, grid, block, lds, s, c, z, chunk); break;
        case 5: hipLaunchKernelGGL(csr_census_esu<5>, grid, block, lds, s, c, z, chunk); break;
        case 6: hipLaunchKernelGGL(csr_census_esu<6>, grid, block, lds, s, c, z, chunk); break;
        case 7: hipLaunchKernelGGL(csr_census_esu<7>, grid, block, lds, s, c, z, chunk); break;
        default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

hipError_t ugs_census_csr_census_clear(const UgsCsrCall &c, const UgsCensus &z, hipStream_t s) {
    if (c.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(csr_census_clear, dim3(csr_blocks(c.G * z.W)), dim3(CSR_AUX_BLOCK), 0, s, c, z);
    return hipGetLastError();
}

hipError_t ugs_census_csr_vertex(const UgsCsrCall &c, const UgsVertexCensus &z, hipStream_t s) {
    if (c.G <= 0) return hipSuccess;
    if (c.k == 1) {
        hipLaunchKernelGGL(csr_single, dim3(csr_blocks(std::max(c.G, c.N))), dim3(CSR_AUX_BLOCK), 0, s, c, (const uint16_t *)nullptr,
                           (unsigned long long *)nullptr, z.W, z.table, z.obase, z.gdv, z.O);
    } else if (c.M > 0) {
        const uint32_t chunk = csr_chunk_of(c.M);
        const dim3 grid((unsigned)((c.M + chunk - 1) / chunk)), block(CSR_BLOCK);
        switch (c.k) {
        case 2: hipLaunchKernelGGL(csr_vcensus_esu<2>, grid, block, 0, s, c, z, chunk); break;
        case 3: hipLaunchKernelGGL(csr_vcensus_esu<3>, grid, block, 0, s, c, z, chunk); break;
        case 4: hipLaunchKernelGGL(csr_vcensus_esu<4>, grid, block, 0, s, c, z, chunk); break;
        case 5: hipLaunchKernelGGL(csr_vcensus_esu<5>, grid, block, 0, s, c, z, chunk); break;
        case 6: hipLaunchKernelGGL(csr_vcensus_esu<6>, grid, block, 0, s, c, z, chunk); break;
        case 7: hipLaunchKernelGGL(csr_vcensus_esu<7>, grid, block, 0, s, c, z, chunk); break;
        default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

hipError_t ugs_census_csr_vertex_clear(const UgsCsrCall &c, const UgsVertexCensus &z, hipStream_t s) {
    if (c.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(csr_vcensus_clear, dim3((unsigned)std::min<int64_t>(c.G, 0x7fffffff), 32), dim3(CSR_AUX_BLOCK), 0, s, c, z);
    return hipGetLastError();
}
