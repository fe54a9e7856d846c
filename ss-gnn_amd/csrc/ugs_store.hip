// ugs_store.hip -- the three kernels of ugs_sampler.GraphCache (host side: ugs_graph_cache.cpp; layout: ugs_device.h; DESIGN.md
// section 15).  The walk, scan and fill kernels of a cached call are those of ugs_kernels.hip, unchanged: they reach a graph only
// through its descriptor, so a descriptor whose bases point into the store serves them.  What is left for this file is plain
// memory-bound work -- copy with an offset (append), compare (check), add (rebase) -- one element per lane, vector loads and stores.
#include "ugs_device.h"

namespace {

constexpr int STORE_BLOCK = 256;

inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// Lane i moves entry i of every array of the chunk that has one.  The chunk's rowptr holds offsets into the chunk's adj; in the
// store they are absolute, so adj_base is added.  Everything else is position-independent: ranks, local columns, order positions.
__global__ __launch_bounds__(STORE_BLOCK) void ugs_store_append_k(const UgsStoreAppend a) {
    const int64_t i = (int64_t)blockIdx.x * STORE_BLOCK + threadIdx.x;
    if (i < a.n_rowptr) a.s_rowptr[a.row_base + i] = a.rowptr[i] + a.adj_base;
    if (i < a.nnz) { a.s_adj[a.adj_base + i] = a.adj[i]; a.s_adjf[a.adj_base + i] = a.adjf[i]; }
    if (i < a.n_roots) a.s_roots[a.root_base + i] = a.roots[i];
    if (i < a.n_viable) a.s_viable[a.via_base + i] = a.viable[i];
    if (i < a.n_cols) a.s_cols[a.col_base + i] = make_int2((int32_t)a.col_u[i], (int32_t)a.col_v[i]);
}

// One lane per batch column.  g = the graph with coff[g] <= e < coff[g+1] (graphs without columns have empty ranges and are never
// found); the comparison is made in 64 bits, so an endpoint far outside the graph cannot alias a stored 32-bit id.
__global__ __launch_bounds__(STORE_BLOCK) void ugs_store_check_k(const UgsStoreCheck c) {
    const int64_t e = (int64_t)blockIdx.x * STORE_BLOCK + threadIdx.x;
    if (e >= c.E) return;
    int64_t lo = 0, hi = c.G;                            // invariant: coff[lo] <= e < coff[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (c.coff[mid] <= e) lo = mid; else hi = mid;
    }
    const int2 want = c.cols[c.col0[lo] + (e - c.coff[lo])];
    const int64_t base = c.lo[lo];
    if (c.src[e] - base != (int64_t)want.x || c.dst[e] - base != (int64_t)want.y) atomicMin(c.first_bad, (int32_t)lo);
}

// Eight lanes per row, as the 8-lane fill writes them: a row has at most a few dozen entries.
__global__ __launch_bounds__(STORE_BLOCK) void ugs_store_rebase_src_k(const int64_t *__restrict__ edge_ptr, int64_t *__restrict__ edge_src,
                                                                      const int64_t *__restrict__ coff, int64_t rows, int32_t m) {
    const int64_t t = (int64_t)blockIdx.x * STORE_BLOCK + threadIdx.x;
    const int64_t r = t >> 3;
    if (r >= rows) return;
    const int64_t add = coff[r / m];
    if (add == 0) return;
    const int64_t e1 = edge_ptr[r + 1];
    for (int64_t e = edge_ptr[r] + (t & 7); e < e1; e += 8) edge_src[e] += add;
}

}  // namespace

hipError_t ugs_store_append(const UgsStoreAppend &a, hipStream_t s) {
    int64_t n = a.n_rowptr;
    for (int64_t x : {a.nnz, a.n_roots, a.n_viable, a.n_cols}) n = x > n ? x : n;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ugs_store_append_k, dim3(blocks(n, STORE_BLOCK)), dim3(STORE_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t ugs_store_check(const UgsStoreCheck &c, hipStream_t s) {
    if (c.E <= 0 || c.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(ugs_store_check_k, dim3(blocks(c.E, STORE_BLOCK)), dim3(STORE_BLOCK), 0, s, c);
    return hipGetLastError();
}

hipError_t ugs_store_rebase_src(const int64_t *edge_ptr, int64_t *edge_src, const int64_t *coff, int64_t rows, int32_t m, hipStream_t s) {
    if (rows <= 0 || m <= 0) return hipSuccess;
    hipLaunchKernelGGL(ugs_store_rebase_src_k, dim3(blocks(rows * 8, STORE_BLOCK)), dim3(STORE_BLOCK), 0, s, edge_ptr, edge_src, coff, rows, m);
    return hipGetLastError();
}
