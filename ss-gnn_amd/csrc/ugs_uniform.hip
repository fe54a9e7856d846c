// ugs_uniform.hip -- gfx950 pipeline of the exact uniform connected k-subgraph sampler (reference uniform_sampler).
//
// Contract: src/samplers/uniform_sampler/src/uniform_sampler.cpp (law stated in include/ugs_mi355.h at
// ugs_uniform_sample_batch_begin): S_g = the connected k-subsets of graph g in lexicographic order of their ascending
// vertex tuples (:47-80), m draws std::uniform_int_distribution<int>(0, |S_g|-1) from ONE std::mt19937_64(seed) per
// graph with S_g non-empty (:144, :189), edges = the batch columns inside the row's subset, in column order (:193-236).
//
// ugs_uniform_sample_graphs_begin (c.seeds != nullptr) gives every graph its own generator and its own budget: the count pass
// adds into the graph's counter and stops counting a graph once it is past the budget, uni_cap empties the items of such graphs
// before the scan, uni_joint flags a call whose healthy graphs together are past it, and uni_draw_graphs replaces uni_draw.
//
// Pipeline (one stream, no host round trip until the edge total):
//   uni_colgraph + radix sort   stable bucket of the batch's columns by graph (key = graph id, ties keep column order)
//   uni_bucket                  per-graph bucket starts; uni_adj: 64-bit neighbour mask per vertex, local (u, v) per column
//   uni_esu<COUNT> + scan       connected k-subsets counted per item (graph, root v, first extension w), exclusive scan
//   uni_esu<WRITE>              the subsets as sort keys ~brev(mask) at their item's offset
//   uni_sort_small / segmented  per-root buckets sorted ascending by key (bitonic in LDS; large buckets: rocPRIM)
//   uni_draw                    one workgroup: mt19937_64 + libstdc++'s Lemire step, draws in blocks of 312
//   uni_draw_graphs             (per-graph seeds) the same, one workgroup and one generator per graph
//   uni_rows + scan             rows (node ids) and per-row edge counts -> edge_ptr
//   uni_fill (finish)           edge_index / edge_src
#include "ugs_device.h"

#include <hipcub/hipcub.hpp>

namespace {

constexpr int UNI_BLOCK = 256;
constexpr int SMALL_SORT = 8192;          // root buckets up to this many keys are sorted in LDS (64 KiB)
constexpr int DRAW_BLOCK = 320;           // >= 312: one lane per generator output of a block
constexpr int MT_N = 312, MT_M = 156;

__device__ __forceinline__ uint64_t above_mask(int v) { return v >= 63 ? 0ull : (~0ull << (v + 1)); }
__device__ __forceinline__ uint64_t key_of(uint64_t mask) { return ~__brevll(mask); }
__device__ __forceinline__ uint64_t mask_of(uint64_t key) { return __brevll(~key); }

__global__ void uni_colgraph(UgsUniCall c) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int64_t u = c.src[e], v = c.dst[e];
    // graph whose range holds u: the last g with ptr[g] <= u (empty graphs have ptr[g] == ptr[g+1] and hold nothing)
    int64_t lo = 0, hi = c.G;                                       // search in [lo, hi)
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (c.ptr[mid + 1] <= u) lo = mid + 1; else hi = mid; }
    uint32_t key = (uint32_t)c.G;                                   // G: the column belongs to no graph
    if (lo < c.G && c.ptr[lo] <= u && u < c.ptr[lo + 1] && c.ptr[lo] <= v && v < c.ptr[lo + 1]) key = (uint32_t)lo;
    c.ckey[e] = key;
    c.cval[e] = (int32_t)e;
}

__global__ void uni_bucket(UgsUniCall c) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > c.G) return;
    int64_t lo = 0, hi = c.E;                                       // first sorted position with key >= g
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)c.ckey2[mid] < g) lo = mid + 1; else hi = mid; }
    c.cstart[g] = lo;
}

__global__ void uni_adj(UgsUniCall c) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.E) return;
    const uint32_t g = c.ckey2[p];
    if (g >= (uint32_t)c.G) return;
    const UgsUniGraph gd = c.graphs[g];
    if (!gd.enumerable) return;
    const int64_t col = c.cval2[p];
    const int u = (int)(c.src[col] - gd.lo), v = (int)(c.dst[col] - gd.lo);
    c.bpair[p] = (uint16_t)(u | (v << 8));
    if (u == v) return;                                             // a loop joins nothing (the reference's BFS ignores it)
    atomicOr((unsigned long long *)&c.adj[gd.vbase + u], 1ull << v);
    atomicOr((unsigned long long *)&c.adj[gd.vbase + v], 1ull << u);
}

// Extension-set search (Wernicke 2006) of item (root v, first extension w): every connected k-set whose minimum is v and whose
// first vertex taken from v's extension set is w, each exactly once.  Stack of (ext, closed neighbourhood, set) per level.
// COUNT: icount[item] = number of sets (the pass gives up once the call's running total exceeds the budget; with per-graph
// seeds, once the graph's running total does);
// WRITE: the sets' keys at ioff[item] (nothing for the items of a graph past its budget: uni_cap gave them no room).
template <int KM, bool WRITE>
__global__ __launch_bounds__(UNI_BLOCK) void uni_esu(UgsUniCall c) {
    const int64_t item = (int64_t)blockIdx.x * UNI_BLOCK + threadIdx.x;
    if (item >= c.nv * 64) return;
    if (WRITE && c.status[1]) return;                               // over budget: nothing is written, begin reports it
    const int64_t vi = item >> 6;
    const int w0 = (int)(item & 63);
    const int32_t gi = c.vgraph[vi];
    if (WRITE && c.seeds && c.gcount[gi] > c.budget) return;
    const UgsUniGraph gd = c.graphs[gi];
    // running total that bounds the work: the call's, or the graph's with per-graph seeds
    unsigned long long *const ctr = (unsigned long long *)(c.seeds ? &c.gcount[gi] : &c.status[0]);
    const int v = (int)(vi - gd.vbase);
    const uint64_t *adj = c.adj + gd.vbase;
    const int k = c.k;
    uint64_t *out = WRITE ? c.keys_a + c.ioff[item] : nullptr;
    uint64_t cnt = 0, flushed = 0;
    if (k == 1) {
        if (w0 == 0) { if (WRITE) out[0] = key_of(1ull << v); cnt = 1; }
    } else {
        const uint64_t abv = above_mask(v);
        const uint64_t ext1 = adj[v] & abv;
        if ((ext1 >> w0) & 1) {
            const uint64_t nb1 = adj[v] | (1ull << v);
            uint64_t ext[KM], nb[KM], sub[KM];
            int d = 2;                                              // |set| at the stack top
            sub[2] = (1ull << v) | (1ull << w0);
            ext[2] = (ext1 & above_mask(w0)) | (adj[w0] & ~nb1 & abv);
            nb[2] = nb1 | adj[w0];
            if (k == 2) { if (WRITE) out[0] = key_of(sub[2]); cnt = 1; d = 1; }
            while (d >= 2) {
                if (d == k - 1) {                                   // the last vertex: every member of ext completes a set
                    if (WRITE) {
                        for (uint64_t e = ext[d]; e; e &= e - 1) out[cnt++] = key_of(sub[d] | (e & (0ull - e)));
                    } else {
                        cnt += (uint64_t)__popcll(ext[d]);
                        if (cnt - flushed >= 4096) {                // bounded work for calls (graphs) over the budget
                            const unsigned long long now = atomicAdd(ctr, (unsigned long long)(cnt - flushed)) + (cnt - flushed);
                            flushed = cnt;
                            if (now > (unsigned long long)c.budget) { if (!c.seeds) c.status[1] = 1; break; }
                        }
                    }
                    --d;
                    continue;
                }
                if (!ext[d]) { --d; continue; }
                const uint64_t e = ext[d];
                const int w = __ffsll((unsigned long long)e) - 1;
                ext[d] = e & (e - 1);
                sub[d + 1] = sub[d] | (1ull << w);
                ext[d + 1] = ext[d] | (adj[w] & ~nb[d] & abv);
                nb[d + 1] = nb[d] | adj[w];
                ++d;
            }
        }
    }
    if (!WRITE) {
        c.icount[item] = (uint32_t)(cnt < 0xFFFFFFFFull ? cnt : 0xFFFFFFFFull);
        if (cnt > flushed) {
            const unsigned long long now = atomicAdd(ctr, (unsigned long long)(cnt - flushed)) + (cnt - flushed);
            if (now > (unsigned long long)c.budget && !c.seeds) c.status[1] = 1;
        }
    }
}

// per-graph seeds, between the count pass and its scan: the items of a graph past the budget hold no sets (it fails alone)
__global__ void uni_cap(UgsUniCall c) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= c.nv * 64) return;
    if (c.gcount[c.vgraph[item >> 6]] > c.budget) c.icount[item] = 0;
}

// per-graph seeds, after the scan: the healthy graphs' sets together; past the budget the call fails as a whole
__global__ void uni_joint(UgsUniCall c) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t total = c.ioff[c.nv * 64];
    c.status[0] = total;
    c.status[1] = total > c.budget ? 1 : 0;
}

// per root bucket: large ones become segments of the radix sort, the others are empty segments there
__global__ void uni_segments(UgsUniCall c) {
    const int64_t vi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vi >= c.nv) return;
    const int64_t b0 = c.ioff[vi * 64], b1 = c.ioff[vi * 64 + 64];
    const bool large = !c.status[1] && b1 - b0 > SMALL_SORT;
    c.seg_lo[vi] = large ? (int32_t)b0 : 0;
    c.seg_hi[vi] = large ? (int32_t)b1 : 0;
}

// one workgroup per root bucket of at most SMALL_SORT keys: bitonic sort in LDS (padded to a power of two with ~0)
__global__ __launch_bounds__(UNI_BLOCK) void uni_sort_small(UgsUniCall c, uint64_t *dst) {
    __shared__ uint64_t s[SMALL_SORT];
    if (c.status[1]) return;
    const int64_t vi = blockIdx.x;
    const int64_t b0 = c.ioff[vi * 64], n = c.ioff[vi * 64 + 64] - b0;
    if (n <= 1 || n > SMALL_SORT) {
        if (n == 1 && dst != c.keys_a && threadIdx.x == 0) dst[b0] = c.keys_a[b0];
        return;
    }
    int p = 2;
    while (p < n) p <<= 1;
    for (int i = threadIdx.x; i < p; i += UNI_BLOCK) s[i] = i < n ? c.keys_a[b0 + i] : ~0ull;
    __syncthreads();
    for (int size = 2; size <= p; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < p; i += UNI_BLOCK) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool up = (i & size) == 0;
                    const uint64_t a = s[i], b = s[j];
                    if ((a > b) == up) { s[i] = b; s[j] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < n; i += UNI_BLOCK) dst[b0 + i] = s[i];
}

__global__ void uni_graph_sizes(UgsUniCall c) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= c.G) return;
    const UgsUniGraph gd = c.graphs[g];
    int64_t st = 0, sz = 0;
    if (gd.enumerable && !c.status[1]) { st = c.ioff[gd.vbase * 64]; sz = c.ioff[(gd.vbase + gd.n) * 64] - st; }
    c.gstart[g] = st;
    c.gsize[g] = sz;
}

// mt19937_64 state update of one block of 312 outputs, in three dependent parts: i < 156 reads only old words; 156 <= i < 311
// reads the new words i - 156 and old words i, i + 1 (read before anyone writes); i = 311 reads the new word 0.
__device__ __forceinline__ uint64_t mt_step(uint64_t x, uint64_t xnext, uint64_t far) {
    const uint64_t y = (x & 0xFFFFFFFF80000000ull) | (xnext & 0x7FFFFFFFull);
    return far ^ (y >> 1) ^ ((y & 1) ? 0xB5026F5AA96619E9ull : 0ull);
}
__device__ void mt_twist(uint64_t *mt) {
    const int i = threadIdx.x;
    uint64_t r = 0;
    if (i < MT_M) r = mt_step(mt[i], mt[i + 1], mt[i + MT_M]);
    __syncthreads();
    if (i < MT_M) mt[i] = r;
    __syncthreads();
    if (i >= MT_M && i < MT_N - 1) r = mt_step(mt[i], mt[i + 1], mt[i - MT_M]);
    __syncthreads();
    if (i >= MT_M && i < MT_N - 1) mt[i] = r;
    __syncthreads();
    if (i == 0) mt[MT_N - 1] = mt_step(mt[MT_N - 1], mt[0], mt[MT_M - 1]);
    __syncthreads();
}
__device__ __forceinline__ uint64_t mt_temper(uint64_t y) {
    y ^= (y >> 29) & 0x5555555555555555ull;
    y ^= (y << 17) & 0x71D67FFFEDA60000ull;
    y ^= (y << 37) & 0xFFF7EEE000000000ull;
    return y ^ (y >> 43);
}

// std::mt19937_64(seed) ([rand.eng.mers]) and its first twist: the first block of 312 outputs, untempered, in mt
__device__ void mt_seed(uint64_t *mt, uint64_t seed) {
    if (threadIdx.x == 0) {
        uint64_t x = seed;
        mt[0] = x;
        for (int i = 1; i < MT_N; ++i) { x = 6364136223846793005ull * (x ^ (x >> 62)) + (uint64_t)i; mt[i] = x; }
    }
    __syncthreads();
    mt_twist(mt);
}

// `total` draws from the seeded generator in mt, draw d uniform over [0, size_of(d)), into out[d].  Lanes take the next outputs
// of the generator block, one per draw, assuming each draw consumes exactly one output; a ballot finds the first draw whose Lemire
// step rejects (lo64(x * N) < t, t = 2^64 mod N).  The draws before it stand, the rejected output is consumed, and that draw is
// retried on the next output (the same rule: libstdc++'s `lo64 < N` test only skips computing t).  A rejection has probability
// t / 2^64 <= N / 2^64 < 2^-32 per draw, so no test input reaches that branch; tests/uniform_law.py (draws_blocked) checks the
// same cursor logic with a stub generator.  Called by all DRAW_BLOCK lanes of a workgroup.
template <class SizeOf>
__device__ void mt_draws(uint64_t *mt, int64_t total, SizeOf size_of, int32_t *out, int32_t *s_wave, int *s_first) {
    const int tid = threadIdx.x;
    int pos = 0;                                                    // next unused output of the block
    int64_t d0 = 0;                                                 // next draw
    while (d0 < total) {
        const int avail = MT_N - pos;
        const int64_t todo = total - d0 < avail ? total - d0 : avail;
        bool reject = false;
        int32_t r = 0;
        if (tid < todo) {
            const int64_t d = d0 + tid;
            const uint64_t N = size_of(d);
            const uint64_t x = mt_temper(mt[pos + tid]);
            const uint64_t lo = x * N;
            if (lo < N) reject = lo < (0ull - N) % N;
            r = (int32_t)__umul64hi(x, N);
        }
        const unsigned long long bal = __ballot(reject);
        if ((tid & 63) == 0) s_wave[tid >> 6] = bal ? (tid & ~63) + __ffsll(bal) - 1 : DRAW_BLOCK;
        __syncthreads();
        if (tid == 0) { int f = DRAW_BLOCK; for (int wv = 0; wv < DRAW_BLOCK / 64; ++wv) f = min(f, s_wave[wv]); *s_first = f; }
        __syncthreads();
        const int first = *s_first;
        if (tid < todo && tid < first) out[d0 + tid] = r;
        const int taken = first < todo ? first : (int)todo;
        d0 += taken;
        pos += taken + (first < todo ? 1 : 0);                      // a rejected output is consumed, its draw retried
        __syncthreads();
        if (pos == MT_N) { mt_twist(mt); pos = 0; }
    }
}

// The call's draws, in order: m per graph with S_g non-empty, all from ONE std::mt19937_64(seed) -- one workgroup.
__global__ __launch_bounds__(DRAW_BLOCK) void uni_draw(UgsUniCall c) {
    __shared__ uint64_t mt[MT_N];
    __shared__ int32_t s_flag[DRAW_BLOCK];
    __shared__ int32_t s_wave[DRAW_BLOCK / 64];
    __shared__ int s_first, s_ne;   // first rejecting lane of a round; graphs with S_g non-empty
    const int tid = threadIdx.x;
    if (c.status[1]) return;
    // graphs with S_g non-empty, in order (block-wide compaction)
    if (tid == 0) s_ne = 0;
    __syncthreads();
    for (int64_t g0 = 0; g0 < c.G; g0 += DRAW_BLOCK) {
        const int64_t g = g0 + tid;
        const int f = g < c.G && c.gsize[g] > 0 ? 1 : 0;
        s_flag[tid] = f;
        __syncthreads();
        for (int off = 1; off < DRAW_BLOCK; off <<= 1) {           // inclusive scan (Hillis-Steele)
            const int t = tid >= off ? s_flag[tid - off] : 0;
            __syncthreads();
            s_flag[tid] += t;
            __syncthreads();
        }
        const int base = s_ne;
        if (g < c.G) {
            const int pos = base + s_flag[tid] - f;
            c.nepos[g] = f ? pos : -1;
            if (f) c.ne_list[pos] = (int32_t)g;
        }
        __syncthreads();
        if (tid == DRAW_BLOCK - 1) s_ne = base + s_flag[DRAW_BLOCK - 1];
        __syncthreads();
    }
    const int64_t total = (int64_t)s_ne * c.m;
    if (total == 0) return;
    mt_seed(mt, c.seed);
    mt_draws(mt, total, [&](int64_t d) { return (uint64_t)c.gsize[c.ne_list[d / c.m]]; }, c.draws, s_wave, &s_first);
}

// Per-graph seeds: workgroup g draws graph g's m draws from its own std::mt19937_64(seeds[g]) into draws[g * m ..].  Graphs
// with S_g empty (n < k, not enumerable, past the budget) leave at once: they consume no draws.
__global__ __launch_bounds__(DRAW_BLOCK) void uni_draw_graphs(UgsUniCall c) {
    __shared__ uint64_t mt[MT_N];
    __shared__ int32_t s_wave[DRAW_BLOCK / 64];
    __shared__ int s_first;
    const int64_t g = blockIdx.x;
    if (c.status[1] || c.m == 0) return;
    const uint64_t N = (uint64_t)c.gsize[g];
    if (N == 0) return;
    mt_seed(mt, c.seeds[g]);
    mt_draws(mt, (int64_t)c.m, [&](int64_t) { return N; }, c.draws + g * (int64_t)c.m, s_wave, &s_first);
}

// row b = g * m + s: the drawn subset's vertices ascending (or -1) and its edge count over the graph's column bucket
__global__ void uni_rows(UgsUniCall c) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t g = row / c.m, s = row - g * c.m;
    int64_t *out = c.nodes + row * c.k;
    uint64_t mask = 0;
    if (!c.status[1] && c.gsize[g] > 0) {
        const int64_t d = c.seeds ? row : (int64_t)c.nepos[g] * c.m + s;   // per-graph seeds: graph g's draws at g * m
        mask = mask_of(c.keys_sorted[c.gstart[g] + c.draws[d]]);
    }
    c.rowmask[row] = mask;
    uint32_t cnt = 0;
    if (mask) {
        const int64_t lo = c.graphs[g].lo;
        int j = 0;
        for (uint64_t e = mask; e; e &= e - 1) out[j++] = lo + (__ffsll((unsigned long long)e) - 1);
        for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
            const uint32_t uv = c.bpair[p];
            cnt += ((mask >> (uv & 63)) & (mask >> (uv >> 8)) & 1) ? 1u : 0u;
        }
    } else {
        for (int j = 0; j < c.k; ++j) out[j] = -1;
    }
    c.ecount[row] = cnt;
}

__global__ void uni_fill(UgsUniCall c, int64_t *edge_index, int64_t *edge_src, int64_t ld) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const uint64_t mask = c.rowmask[row];
    if (!mask) return;
    const int64_t g = row / c.m;
    const int64_t lo = c.graphs[g].lo;
    int64_t w = c.edge_ptr[row];
    for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
        const uint32_t uv = c.bpair[p];
        const int u = uv & 63, v = uv >> 8;
        if (!((mask >> u) & (mask >> v) & 1)) continue;
        if (c.mode == 0) {                                          // position in the row = vertices of the subset below it
            edge_index[w] = __popcll(mask & ((1ull << u) - 1));
            edge_index[ld + w] = __popcll(mask & ((1ull << v) - 1));
        } else {
            edge_index[w] = lo + u;
            edge_index[ld + w] = lo + v;
        }
        edge_src[w] = c.cval2[p];
        ++w;
    }
}

inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

}  // namespace

size_t ugs_uniform_cub_bytes(int64_t E, int64_t nv, int64_t budget) {
    size_t a = 0, b = 0;
    if (E > 0) (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr,
                                                       (int32_t *)nullptr, (int)E, 0, 32);
    if (nv > 0) {
        hipcub::DoubleBuffer<uint64_t> keys(nullptr, nullptr);
        (void)hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, b, keys, (int)budget, (int)nv, (const int32_t *)nullptr,
                                                         (const int32_t *)nullptr, 0, 64);
    }
    return a > b ? a : b;
}

hipError_t ugs_uniform_begin(UgsUniCall &c, hipStream_t s) {
    hipError_t e = hipMemsetAsync(c.status, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) <= c.G) ++bits;                   // keys 0..G
    if (c.E > 0) {
        hipLaunchKernelGGL(uni_colgraph, dim3(blocks(c.E, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        size_t tb = c.cub_bytes;
        e = hipcub::DeviceRadixSort::SortPairs(c.cub_tmp, tb, c.ckey, c.ckey2, c.cval, c.cval2, (int)c.E, 0, bits, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(uni_bucket, dim3(blocks(c.G + 1, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
    c.keys_sorted = c.keys_a;
    if (c.nv > 0) {
        if ((e = hipMemsetAsync(c.adj, 0, (size_t)c.nv * sizeof(uint64_t), s)) != hipSuccess) return e;
        if (c.E > 0) hipLaunchKernelGGL(uni_adj, dim3(blocks(c.E, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        const int64_t items = c.nv * 64;
        if (c.seeds && (e = hipMemsetAsync(c.gcount, 0, (size_t)c.G * sizeof(int64_t), s)) != hipSuccess) return e;
        if (c.k <= 8) hipLaunchKernelGGL((uni_esu<8, false>), dim3(blocks(items, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        else hipLaunchKernelGGL((uni_esu<64, false>), dim3(blocks(items, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        if (c.seeds) hipLaunchKernelGGL(uni_cap, dim3(blocks(items, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        if ((e = ugs_launch_scan(c.icount, items, c.ioff, c.scan_tmp, s)) != hipSuccess) return e;
        if (c.seeds) hipLaunchKernelGGL(uni_joint, dim3(1), dim3(64), 0, s, c);
        if (c.k <= 8) hipLaunchKernelGGL((uni_esu<8, true>), dim3(blocks(items, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        else hipLaunchKernelGGL((uni_esu<64, true>), dim3(blocks(items, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        // root buckets larger than LDS: rocPRIM's segmented radix sort (the others are empty segments there)
        hipLaunchKernelGGL(uni_segments, dim3(blocks(c.nv, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        hipcub::DoubleBuffer<uint64_t> keys(c.keys_a, c.keys_b);
        size_t tb = c.cub_bytes;
        e = hipcub::DeviceSegmentedRadixSort::SortKeys(c.cub_tmp, tb, keys, (int)c.budget, (int)c.nv, c.seg_lo, c.seg_hi, 0, 64, s);
        if (e != hipSuccess) return e;
        c.keys_sorted = keys.Current();
        hipLaunchKernelGGL(uni_sort_small, dim3((unsigned)c.nv), dim3(UNI_BLOCK), 0, s, c, keys.Current());
    }
    if (c.G > 0) {
        hipLaunchKernelGGL(uni_graph_sizes, dim3(blocks(c.G, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        if (c.seeds) hipLaunchKernelGGL(uni_draw_graphs, dim3((unsigned)c.G), dim3(DRAW_BLOCK), 0, s, c);
        else hipLaunchKernelGGL(uni_draw, dim3(1), dim3(DRAW_BLOCK), 0, s, c);
    }
    if (c.rows > 0) hipLaunchKernelGGL(uni_rows, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return ugs_launch_scan(c.ecount, c.rows, c.edge_ptr, c.scan_tmp, s);
}

hipError_t ugs_uniform_fill(const UgsUniCall &c, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
    if (c.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(uni_fill, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, edge_index, edge_src, ld);
    return hipGetLastError();
}
