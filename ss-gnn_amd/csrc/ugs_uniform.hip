// ugs_uniform.hip -- gfx950 pipeline of the exact uniform connected k-subgraph sampler (reference uniform_sampler).
//
// Contract: src/samplers/uniform_sampler/src/uniform_sampler.cpp (law stated in include/ugs_mi355.h at
// ugs_uniform_sample_batch_begin): S_g = the connected k-subsets of graph g in lexicographic order of their ascending
// vertex tuples (:47-80), m draws std::uniform_int_distribution<int>(0, |S_g|-1) from ONE std::mt19937_64(seed) per
// graph with S_g non-empty (:144, :189), edges = the batch columns inside the row's subset, in column order (:193-236).
//
// ugs_uniform_sample_graphs_begin gives every graph its own budget (c.per_graph) and its own generator (c.seeds): the count pass
// adds into the graph's counter and stops counting a graph once it is past the budget, uni_cap empties the items of such graphs
// before the scan, uni_joint flags a call whose healthy graphs together are past it, and uni_draw_graphs replaces uni_draw.
// ugs_uniform_count_graphs and ugs_uniform_enumerate_begin take the per-graph budget without any generator: the first stops behind
// the count pass, the second replaces draws, uni_rows and uni_fill by uni_enum_rows / uni_enum_fill (wide: uni_wenum_*), one row
// per key of the sorted array.
//
// Pipeline (one stream, no host round trip until the edge total):
//   uni_colgraph + radix sort   stable bucket of the batch's columns by graph (key = graph id, ties keep column order)
//   uni_bucket                  per-graph bucket starts; uni_adj: 64-bit neighbour mask per vertex, local (u, v) per column
//   uni_esu<COUNT> + scan       connected k-subsets counted per item (graph, root v, first extension w), exclusive scan
//   uni_esu<WRITE>              the subsets as sort keys ~brev(mask) at their item's offset
//   uni_sort_small / segmented  per-root buckets sorted ascending by key (bitonic in LDS; large buckets: rocPRIM)
//   uni_draw                    one workgroup: mt19937_64 + libstdc++'s Lemire step, draws in blocks of 312
//   uni_draw_graphs             (per-graph seeds) the same, one workgroup and one generator per graph
//   uni_draw_distinct           (ugs_uniform_distinct_begin) m distinct draws per graph, or all of S_g and -1 behind it: a
//                               counter-based partial Fisher-Yates shuffle resolved through a key sort in LDS
//   uni_rows + scan             rows (node ids) and per-row edge counts -> edge_ptr
//   uni_fill (finish)           edge_index / edge_src
//
// Wide graphs (UgsUniWide: more than 64 vertices, up to the limit of ugs_uniform_set_max_vertices) keep every stage's place and
// the shared ones (scan, sorts, sizes, draws) as they are; their keys are packed ascending tuples, which sort into the same order:
//   uni_wadj                    bitmap of W = ceil(n / 64) words per vertex, local (u, v) per column in 16 + 16 bits
//   uni_wesu<COUNT / WRITE>     the same search, one 16-lane group (a DPP row) per item, lane l holding word l of every set
//   uni_wrows / uni_wfill       the tuple decoded from the key; the mask form's kernels see these graphs as empty
// A call without wide graphs launches none of these.
//
// Population cache (ugs_uniform_population_*): uni_prepare runs once per dataset graph and uni_pop_store keeps its sorted keys, with
// a fingerprint of its adjacency; a sample call served from them runs only
//   uni_colgraph + radix sort, uni_bucket, uni_pop_pairs     column buckets and the local endpoints of every sorted column
//   uni_adj / uni_wadj + uni_pop_check                        (check only) the batch's adjacency against the stored fingerprints
//   uni_draw / uni_draw_graphs                                from the sizes the host staged
//   uni_pop_rows / uni_wpop_rows + scan, uni_pop_fill / uni_wpop_fill (finish)    a 16-lane group per row
//
// Graphlet census (ugs_graphlet_census): column buckets and adjacency as above, then in the count pass's place
//   uni_census_esu / uni_census_wesu    the same search with the raw adjacency code of the placed vertices carried down the levels;
//                                       every completed set is classified (k <= 7: one load from a code -> column table; k = 8:
//                                       ugs_gl::canon and a search among the connected keys) and counted, runs merged per lane, into
//                                       the workgroup's LDS counters (k <= 7) or the graph's row (k = 8); nothing is stored per set
//   uni_census_clear                    the row of a graph past the limit
//
// Graphlet vertex census (ugs_graphlet_vertex_census): the same, per vertex
//   uni_vcensus_esu / uni_vcensus_wesu  the census's search for k <= 7 with the ids of the placed vertices carried down beside the raw
//                                       code; one load from a code -> (column, orbit of every position) table a set, and k integer
//                                       atomic adds into the rows of its members, the k - 1 placed ones merged over runs of siblings
//   uni_vcensus_clear                   the rows of the vertices of a graph past the limit
#include "ugs_device.h"
#include "ugs_graphlet_common.h"

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
    if (gd.enumerable != 1) return;                                 // wide graphs: uni_wadj
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
    if (WRITE && c.per_graph && c.gcount[gi] > c.budget) return;
    const UgsUniGraph gd = c.graphs[gi];
    // running total that bounds the work: the call's, or the graph's with per-graph budgets
    unsigned long long *const ctr = (unsigned long long *)(c.per_graph ? &c.gcount[gi] : &c.status[0]);
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
                            if (now > (unsigned long long)c.budget) { if (!c.per_graph) c.status[1] = 1; break; }
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
            if (now > (unsigned long long)c.budget && !c.per_graph) c.status[1] = 1;
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

// ---- distinct draws (ugs_uniform_distinct_begin; the law stands in include/ugs_mi355.h): graph g's rows are the first m places of
//      a Fisher-Yates shuffle of 0 ... N - 1, step j swapping a[j] with a[t_j], t_j = j + hi64(mix(mix(seed) + (j + 1) gamma) (N - j)).
//      The targets are counter-based, so every lane computes its own; what is serial in the law is only "a[t_j] as earlier steps left
//      it", and that is read off the sorted keys (t_j << 32) | j:
//        pred(t, j) = the greatest step i < j with t_i == t: the entry just below (t << 32) | j, if its t matches;
//        place t >= j is touched before step j only by such steps, and step i leaves there what stood at place i before it:
//        w(i) = pred(i, i) exists ? w(pred(i, i)) : i  (a strictly decreasing chain, nearly always empty);
//        row j = pred(t_j, j) exists ? w(pred(t_j, j)) : t_j.
//      The entry below a key is found by binary search over the m sorted keys (log2 m LDS reads), so the keys are the only array:
//      8 P bytes of LDS, P = m rounded up to a power of two, 32 KiB at the limit of 4096 rows. ----
__device__ __forceinline__ uint64_t sm_mix(uint64_t z) {                           // SplitMix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t distinct_target(uint64_t s0, uint64_t N, uint32_t j) {   // t_j, s0 = mix(seed); j < N < 2^32
    return j + (uint32_t)__umul64hi(sm_mix(s0 + (uint64_t)(j + 1) * 0x9E3779B97F4A7C15ull), N - j);
}
// pred(t, j) over the ascending keys[0 ... m), or -1
__device__ __forceinline__ int distinct_pred(const uint64_t *keys, int m, uint32_t t, uint32_t j) {
    const uint64_t key = ((uint64_t)t << 32) | j;
    int lo = 0, hi = m;                                             // first position whose key is >= key
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    if (lo == 0) return -1;
    const uint64_t below = keys[lo - 1];
    return (uint32_t)(below >> 32) == t ? (int)(uint32_t)below : -1;
}

// One workgroup per graph writes draws[g * m + j], j < m: q = min(m, N) distinct indices into S_g, then -1.  m >= N (N <= 0
// included) is the whole population in its order and needs no key; otherwise P = m rounded up to a power of two keys are sorted
// (bitonic, pair form: lane q of a stage with stride s holds places i = 2 q - (q & (s - 1)) and i + s; the padding sorts last).
// Dynamic LDS: 8 P bytes (the host passes it), m <= UGS_UNI_DISTINCT_MAX_M.
__global__ __launch_bounds__(UNI_BLOCK) void uni_draw_distinct(UgsUniCall c) {
    extern __shared__ uint64_t s_keys[];
    const int64_t g = blockIdx.x;
    const int m = c.m, tid = threadIdx.x;
    if (m == 0) return;
    int32_t *out = c.draws + g * (int64_t)m;
    const int64_t N = c.status[1] ? 0 : c.gsize[g];
    if (N <= m) {
        for (int j = tid; j < m; j += UNI_BLOCK) out[j] = j < N ? j : -1;
        return;
    }
    int P = 1;
    while (P < m) P <<= 1;
    const uint64_t s0 = sm_mix(c.seeds[g]);
    for (int j = tid; j < P; j += UNI_BLOCK) s_keys[j] = j < m ? ((uint64_t)distinct_target(s0, (uint64_t)N, (uint32_t)j) << 32) | (uint32_t)j : ~0ull;
    __syncthreads();
    for (int width = 2; width <= P; width <<= 1)
        for (int stride = width >> 1; stride > 0; stride >>= 1) {
            for (int q = tid; q < (P >> 1); q += UNI_BLOCK) {
                const int i = 2 * q - (q & (stride - 1)), l = i + stride;
                const uint64_t a = s_keys[i], b = s_keys[l];
                if ((a > b) == ((i & width) == 0)) { s_keys[i] = b; s_keys[l] = a; }
            }
            __syncthreads();
        }
    for (int j = tid; j < m; j += UNI_BLOCK) {
        const uint32_t t = distinct_target(s0, (uint64_t)N, (uint32_t)j);
        int x = distinct_pred(s_keys, m, t, (uint32_t)j);
        uint32_t r = t;
        if (x >= 0) {                                               // w(x): what stood at place x before step x
            for (;;) {
                const int y = distinct_pred(s_keys, m, (uint32_t)x, (uint32_t)x);
                if (y < 0) break;
                x = y;
            }
            r = (uint32_t)x;
        }
        out[j] = (int32_t)r;
    }
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
        const int32_t draw = c.draws[d];                            // negative (a distinct call past |S_g|): a row of -1
        if (draw >= 0) mask = mask_of(c.keys_sorted[c.gstart[g] + draw]);
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

// ---- wide graphs: a vertex set is W <= 16 words, one per lane of a 16-lane group (one DPP row; four items per wave) ----
constexpr int WIDE_LANES = 16;
constexpr int WIDE_GROUPS = UNI_BLOCK / WIDE_LANES;

__device__ __forceinline__ int field_bits(int n) { int b = 1; while (b < 16 && (1 << b) < n) ++b; return b; }   // bit length of n - 1, at least 1

// inclusive sum over the lanes of a row at and below this one
__device__ __forceinline__ uint32_t row_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);   // row_shr:8
    return x;
}

__global__ void uni_wadj(UgsUniCall c, UgsUniWide wd) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.E) return;
    const uint32_t g = c.ckey2[p];
    if (g >= (uint32_t)c.G) return;
    const int64_t base = wd.wbase[g];
    if (base < 0) return;
    const UgsUniGraph gd = c.graphs[g];
    const int64_t col = c.cval2[p];
    const int u = (int)(c.src[col] - gd.lo), v = (int)(c.dst[col] - gd.lo);   // both inside [0, n): uni_colgraph checked the range
    wd.wpair[p] = (uint32_t)u | ((uint32_t)v << 16);
    if (u == v) return;
    const int W = (gd.n + 63) >> 6;
    atomicOr((unsigned long long *)&wd.wadj[base + (int64_t)u * W + (v >> 6)], 1ull << (v & 63));
    atomicOr((unsigned long long *)&wd.wadj[base + (int64_t)v * W + (u >> 6)], 1ull << (u & 63));
}

// what one group carries through the search of its item
struct WGroup {
    const uint64_t *adj;          // the graph's bitmap rows
    int W, l, gshift, b, k;       // words per row, this lane's word, first lane of the group in the wave, field width, set size
    uint64_t abv;                 // this lane's word of the vertices above the root
    uint64_t *out;                // WRITE: the item's next key
    uint32_t cnt, flushed;        // COUNT: this lane's sets, and how many of them it has added to the running total
    unsigned long long *ctr;      // the running total that bounds the work (the call's, or the graph's with per-graph seeds)
    int64_t budget;
    int64_t *status;              // the call's over-budget flag, nullptr with per-graph seeds
    bool stop;                    // the running total is past the budget: leave (group-uniform)
};

__device__ __forceinline__ uint32_t group_ballot(const WGroup &x, bool p) { return (uint32_t)(__ballot(p) >> x.gshift) & 0xFFFFu; }

// the lowest vertex of the set `ext` (one word per lane), removed from it; -1: the set is empty.  Group-uniform.
__device__ __forceinline__ int group_take(const WGroup &x, uint64_t &ext) {
    const uint32_t bits = group_ballot(x, ext != 0);
    if (!bits) return -1;
    const int l0 = __ffs(bits) - 1;
    const int f = __shfl(__ffsll((unsigned long long)ext) - 1, l0, WIDE_LANES);
    if (x.l == l0) ext &= ext - 1;
    return l0 * 64 + f;
}

// the ascending tuple `key` of D fields with vertex w put in its place
template <int D>
__device__ __forceinline__ uint64_t key_with(uint64_t key, uint32_t w, int b) {
    const uint64_t fm = (1ull << b) - 1;
    int above = 0;                                                  // fields greater than w: the lowest ones
#pragma unroll
    for (int i = 0; i < D; ++i) above += (uint32_t)((key >> (i * b)) & fm) > w ? 1 : 0;
    const int sh = above * b;                                       // <= D b <= 56
    const uint64_t hi = key >> sh;
    return (sh + b >= 64 ? 0ull : hi << (sh + b)) | ((uint64_t)w << sh) | (key & ((1ull << sh) - 1));
}

// the set has D = k - 1 vertices: every member of ext completes one
template <int D, bool WRITE>
__device__ __forceinline__ void wide_last(WGroup &x, uint64_t ext, uint64_t key) {
    const uint32_t pc = (uint32_t)__popcll(ext);
    if (WRITE) {
        const uint32_t incl = row_scan(pc);
        const uint32_t tot = (uint32_t)__shfl((int)incl, WIDE_LANES - 1, WIDE_LANES);
        uint64_t *o = x.out + (incl - pc);
        for (uint64_t e = ext; e; e &= e - 1) *o++ = key_with<D>(key, (uint32_t)(x.l * 64 + __ffsll((unsigned long long)e) - 1), x.b);
        x.out += tot;
    } else {
        x.cnt += pc;
        bool over = false;
        if (x.cnt - x.flushed >= 4096 / WIDE_LANES) {               // the group flushes at least every 4096 sets
            const unsigned long long add = x.cnt - x.flushed;
            over = atomicAdd(x.ctr, add) + add > (unsigned long long)x.budget;
            x.flushed = x.cnt;
            if (over && x.status) x.status[1] = 1;
        }
        if (group_ballot(x, over)) x.stop = true;
    }
}

// the set has D vertices (ascending in key), ext its extension set, nb its closed neighbourhood
template <int D, bool WRITE>
__device__ __forceinline__ void wide_level(WGroup &x, uint64_t ext, uint64_t nb, uint64_t key) {
    if (D == x.k - 1) { wide_last<D, WRITE>(x, ext, key); return; }
    if constexpr (D < UGS_UNI_WIDE_MAX_K - 1) {
        while (!x.stop) {
            const int w = group_take(x, ext);
            if (w < 0) break;
            const uint64_t aw = x.l < x.W ? x.adj[(int64_t)w * x.W + x.l] : 0ull;
            wide_level<D + 1, WRITE>(x, ext | (aw & ~nb & x.abv), nb | aw, key_with<D>(key, (uint32_t)w, x.b));
        }
    }
}

// uni_esu for the items of the wide roots: item (root v, j) = the sets with minimum v whose first vertex taken from v's extension
// set is its (j + 64 i)-th member, i = 0, 1, ...  Counts, offsets, budget and bounded work as in uni_esu.
template <bool WRITE>
__global__ __launch_bounds__(UNI_BLOCK) void uni_wesu(UgsUniCall c, UgsUniWide wd) {
    const int64_t item = wd.nv_mask * 64 + (int64_t)blockIdx.x * WIDE_GROUPS + (threadIdx.x / WIDE_LANES);
    if (item >= c.nv * 64) return;
    if (WRITE && c.status[1]) return;
    const int64_t vi = item >> 6;
    const int slot = (int)(item & 63);
    const int32_t gi = c.vgraph[vi];
    if (WRITE && c.per_graph && c.gcount[gi] > c.budget) return;
    const UgsUniGraph gd = c.graphs[gi];
    const int v = (int)(vi - gd.vbase), vw = v >> 6;
    WGroup x;
    x.adj = wd.wadj + wd.wbase[gi];
    x.W = (gd.n + 63) >> 6; x.l = threadIdx.x & (WIDE_LANES - 1); x.gshift = threadIdx.x & 63 & ~(WIDE_LANES - 1);
    x.b = field_bits(gd.n); x.k = c.k;
    x.abv = x.l < vw ? 0ull : x.l == vw ? above_mask(v & 63) : ~0ull;
    x.out = WRITE ? c.keys_a + c.ioff[item] : nullptr;
    x.cnt = 0; x.flushed = 0;
    x.ctr = (unsigned long long *)(c.per_graph ? &c.gcount[gi] : &c.status[0]);
    x.budget = c.budget; x.status = c.per_graph ? nullptr : c.status; x.stop = false;
    const uint64_t av = x.l < x.W ? x.adj[(int64_t)v * x.W + x.l] : 0ull;
    const uint64_t ext1 = av & x.abv;
    const uint64_t nb1 = av | (x.l == vw ? 1ull << (v & 63) : 0ull);
    if (x.k == 1) {
        if (slot == 0 && x.l == 0) { if (WRITE) x.out[0] = (uint64_t)v; else x.cnt = 1; }
    } else if (x.k == 2) {
        if (slot == 0) wide_last<1, WRITE>(x, ext1, (uint64_t)v);
    } else {
        const uint32_t pc = (uint32_t)__popcll(ext1), incl = row_scan(pc), excl = incl - pc;
        const uint32_t deg = (uint32_t)__shfl((int)incl, WIDE_LANES - 1, WIDE_LANES);
        for (uint32_t r = (uint32_t)slot; r < deg && !x.stop; r += 64) {
            const bool holds = excl <= r && r < incl;               // this lane's word holds the r-th member
            int f = 0;
            if (holds) {
                uint64_t t = ext1;
                for (uint32_t i = r - excl; i > 0; --i) t &= t - 1;
                f = __ffsll((unsigned long long)t) - 1;
            }
            const int l0 = __ffs(group_ballot(x, holds)) - 1;
            f = __shfl(f, l0, WIDE_LANES);
            const int w = l0 * 64 + f;
            const uint64_t aw = x.l < x.W ? x.adj[(int64_t)w * x.W + x.l] : 0ull;
            const uint64_t later = x.l < l0 ? 0ull : x.l == l0 ? above_mask(f) : ~0ull;   // the members of ext1 after w
            wide_level<2, WRITE>(x, (ext1 & later) | (aw & ~nb1 & x.abv), nb1 | aw, ((uint64_t)v << x.b) | (uint64_t)w);
        }
    }
    if (!WRITE) {
        const uint32_t tot = row_scan(x.cnt), rest = row_scan(x.cnt - x.flushed);
        if (x.l == WIDE_LANES - 1) {
            c.icount[item] = tot;
            if (rest) {
                const unsigned long long now = atomicAdd(x.ctr, (unsigned long long)rest) + rest;
                if (now > (unsigned long long)c.budget && !c.per_graph) c.status[1] = 1;
            }
        }
    }
}

// what uni_rows sees: the wide graphs hold nothing (it writes their rows as -1, uni_wrows writes them again)
__global__ void uni_wsizes(UgsUniCall c, UgsUniWide wd) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= c.G) return;
    wd.gsize_mask[g] = wd.wbase[g] >= 0 ? 0 : c.gsize[g];
}

// position of local vertex u in the tuple `key` of k fields; -1: not a member
__device__ __forceinline__ int tuple_pos(uint64_t key, int k, int b, uint32_t u) {
    const uint64_t fm = (1ull << b) - 1;
    for (int j = 0; j < k; ++j) if ((uint32_t)((key >> (b * (k - 1 - j))) & fm) == u) return j;
    return -1;
}

__device__ __forceinline__ bool wide_row_valid(const UgsUniCall &c, int64_t g) { return !c.status[1] && c.gsize[g] > 0; }

// uni_rows for the rows of the wide graphs (a row is valid by its graph, not by its key: {0} at k = 1 has key 0)
__global__ void uni_wrows(UgsUniCall c, UgsUniWide wd) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t g = row / c.m, s = row - g * c.m;
    if (wd.wbase[g] < 0 || !wide_row_valid(c, g)) return;           // uni_rows has written the row of -1
    const UgsUniGraph gd = c.graphs[g];
    const int k = c.k, b = field_bits(gd.n);
    const int64_t d = c.seeds ? row : (int64_t)c.nepos[g] * c.m + s;
    const int32_t draw = c.draws[d];
    if (draw < 0) { wd.rowkey[row] = UGS_UNI_NO_KEY; return; }      // (a distinct call past |S_g|) uni_rows has written the row of -1
    const uint64_t key = c.keys_sorted[c.gstart[g] + draw];
    wd.rowkey[row] = key;
    int64_t *out = c.nodes + row * k;
    for (int j = 0; j < k; ++j) out[j] = gd.lo + (int64_t)((key >> (b * (k - 1 - j))) & ((1ull << b) - 1));
    uint32_t cnt = 0;
    for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
        const uint32_t uv = wd.wpair[p];
        cnt += tuple_pos(key, k, b, uv & 0xFFFFu) >= 0 && tuple_pos(key, k, b, uv >> 16) >= 0 ? 1u : 0u;
    }
    c.ecount[row] = cnt;
}

__global__ void uni_wfill(UgsUniCall c, UgsUniWide wd, int64_t *edge_index, int64_t *edge_src, int64_t ld) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t g = row / c.m;
    if (wd.wbase[g] < 0 || !wide_row_valid(c, g)) return;
    const UgsUniGraph gd = c.graphs[g];
    const int k = c.k, b = field_bits(gd.n);
    const uint64_t key = wd.rowkey[row];
    if (key == UGS_UNI_NO_KEY) return;                              // a row of -1 inside a live graph
    int64_t w = c.edge_ptr[row];
    for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
        const uint32_t uv = wd.wpair[p];
        const int pu = tuple_pos(key, k, b, uv & 0xFFFFu), pv = tuple_pos(key, k, b, uv >> 16);
        if (pu < 0 || pv < 0) continue;
        edge_index[w] = c.mode == 0 ? pu : gd.lo + (int64_t)(uv & 0xFFFFu);
        edge_index[ld + w] = c.mode == 0 ? pv : gd.lo + (int64_t)(uv >> 16);
        edge_src[w] = c.cval2[p];
        ++w;
    }
}

// ---- enumeration (ugs_uniform_enumerate_begin): the whole sorted key array as rows.  Row r belongs to the graph g with
//      sptr[g] <= r < sptr[g + 1], sptr = the exclusive scan of gsize in BATCH graph order (the call's sample_ptr), and is the
//      (r - sptr[g])-th key of that graph: keys_sorted[gstart[g] + r - sptr[g]].  gstart follows the enumerated vertices (mask graphs
//      first, wide graphs behind them), so it is not monotonic in g when the two kinds interleave; sptr is.  The key is read again by
//      the fill, so no per-row mask or key is kept. ----
__device__ __forceinline__ int64_t enum_graph(const UgsUniCall &c, int64_t row) {
    int64_t lo = 0, hi = c.G - 1;                                   // the first g with sptr[g + 1] > row (row < sptr[G])
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (c.sptr[mid + 1] <= row) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ __forceinline__ uint64_t enum_key(const UgsUniCall &c, int64_t g, int64_t row) { return c.keys_sorted[c.gstart[g] + (row - c.sptr[g])]; }

__global__ void uni_enum_rows(UgsUniCall c) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t g = enum_graph(c, row);
    const UgsUniGraph gd = c.graphs[g];
    if (gd.enumerable != 1) return;                                 // a wide graph's row: uni_wenum_rows
    const uint64_t mask = mask_of(enum_key(c, g, row));
    int64_t *out = c.nodes + row * c.k;
    int j = 0;
    for (uint64_t e = mask; e && j < c.k; e &= e - 1) out[j++] = gd.lo + (__ffsll((unsigned long long)e) - 1);
    uint32_t cnt = 0;
    for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
        const uint32_t uv = c.bpair[p];
        cnt += ((mask >> (uv & 63)) & (mask >> (uv >> 8)) & 1) ? 1u : 0u;
    }
    c.ecount[row] = cnt;
}

__global__ void uni_enum_fill(UgsUniCall c, int64_t *edge_index, int64_t *edge_src, int64_t ld) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t g = enum_graph(c, row);
    const UgsUniGraph gd = c.graphs[g];
    if (gd.enumerable != 1) return;
    const uint64_t mask = mask_of(enum_key(c, g, row));
    int64_t w = c.edge_ptr[row];
    for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
        const uint32_t uv = c.bpair[p];
        const int u = uv & 63, v = uv >> 8;
        if (!((mask >> u) & (mask >> v) & 1)) continue;
        if (c.mode == 0) {
            edge_index[w] = __popcll(mask & ((1ull << u) - 1));
            edge_index[ld + w] = __popcll(mask & ((1ull << v) - 1));
        } else {
            edge_index[w] = gd.lo + u;
            edge_index[ld + w] = gd.lo + v;
        }
        edge_src[w] = c.cval2[p];
        ++w;
    }
}

__global__ void uni_wenum_rows(UgsUniCall c, UgsUniWide wd) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t g = enum_graph(c, row);
    const UgsUniGraph gd = c.graphs[g];
    if (gd.enumerable != 2) return;
    const int k = c.k, b = field_bits(gd.n);
    const uint64_t key = enum_key(c, g, row);
    int64_t *out = c.nodes + row * k;
    for (int j = 0; j < k; ++j) out[j] = gd.lo + (int64_t)((key >> (b * (k - 1 - j))) & ((1ull << b) - 1));
    uint32_t cnt = 0;
    for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
        const uint32_t uv = wd.wpair[p];
        cnt += tuple_pos(key, k, b, uv & 0xFFFFu) >= 0 && tuple_pos(key, k, b, uv >> 16) >= 0 ? 1u : 0u;
    }
    c.ecount[row] = cnt;
}

__global__ void uni_wenum_fill(UgsUniCall c, UgsUniWide wd, int64_t *edge_index, int64_t *edge_src, int64_t ld) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t g = enum_graph(c, row);
    const UgsUniGraph gd = c.graphs[g];
    if (gd.enumerable != 2) return;
    const int k = c.k, b = field_bits(gd.n);
    const uint64_t key = enum_key(c, g, row);
    int64_t w = c.edge_ptr[row];
    for (int64_t p = c.cstart[g]; p < c.cstart[g + 1]; ++p) {
        const uint32_t uv = wd.wpair[p];
        const int pu = tuple_pos(key, k, b, uv & 0xFFFFu), pv = tuple_pos(key, k, b, uv >> 16);
        if (pu < 0 || pv < 0) continue;
        edge_index[w] = c.mode == 0 ? pu : gd.lo + (int64_t)(uv & 0xFFFFu);
        edge_index[ld + w] = c.mode == 0 ? pv : gd.lo + (int64_t)(uv >> 16);
        edge_src[w] = c.cval2[p];
        ++w;
    }
}

// ---- population cache (ugs_uniform_population_*): the keys of a graph are enumerated once, by uni_prepare, and kept; a sample call
//      served from them runs column buckets, draws, rows and fill only.  Rows and fill give every row a 16-lane group (one DPP row,
//      as uni_wesu does): lane l takes the columns l, l + 16, ... of the graph's bucket, the row's edge count is the row-wide sum, and
//      the fill keeps bucket order by writing each lane's hit at the row-wide exclusive prefix, chunk of 16 columns after chunk. ----
constexpr int POP_LANES = 16;
constexpr int POP_GROUPS = UNI_BLOCK / POP_LANES;

__device__ __forceinline__ uint64_t fp_mix(uint64_t word, uint64_t pos) {          // SplitMix64's finaliser over (word, position)
    uint64_t x = word + 0x9E3779B97F4A7C15ull * (pos + 1);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// fingerprint of graph g's adjacency bitmap (ugs_device.h), by all UNI_BLOCK lanes of a workgroup; 0 for a graph without one
__device__ uint64_t pop_fingerprint(const UgsUniCall &c, const UgsUniWide &w, int64_t g, uint64_t *s_sum) {
    const UgsUniGraph gd = c.graphs[g];
    uint64_t acc = 0;
    if (gd.enumerable) {
        const int64_t words = gd.enumerable == 1 ? (int64_t)gd.n : (int64_t)gd.n * ((gd.n + 63) >> 6);
        const uint64_t *bm = gd.enumerable == 1 ? c.adj + gd.vbase : w.wadj + w.wbase[g];
        for (int64_t i = threadIdx.x; i < words; i += UNI_BLOCK) { const uint64_t x = bm[i]; if (x) acc += fp_mix(x, (uint64_t)i); }
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int off = UNI_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
        __syncthreads();
    }
    return s_sum[0];
}

// add: workgroups (g, 0 ... gridDim.y - 1) copy graph g's sorted keys into the population's storage; workgroup (g, 0) writes its fingerprint
__global__ __launch_bounds__(UNI_BLOCK) void uni_pop_store(UgsUniCall c, UgsUniWide w, uint64_t *const *dst, uint64_t *fp_out) {
    __shared__ uint64_t s_sum[UNI_BLOCK];
    const int64_t g = blockIdx.x;
    uint64_t *const out = dst[g];
    if (out) {
        const uint64_t *in = c.keys_sorted + c.gstart[g];
        const int64_t n = c.gsize[g];
        for (int64_t i = (int64_t)blockIdx.y * UNI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.y * UNI_BLOCK) out[i] = in[i];
    }
    if (blockIdx.y == 0) {
        const uint64_t fp = pop_fingerprint(c, w, g, s_sum);
        if (threadIdx.x == 0) fp_out[g] = fp;
    }
}

__global__ void uni_pop_pairs(UgsPopCall p) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= p.c.E) return;
    const uint32_t g = p.c.ckey2[q];
    if (g >= (uint32_t)p.c.G) return;
    const int64_t col = p.c.cval2[q], lo = p.pg[g].lo;
    p.pair[q] = (uint32_t)(p.c.src[col] - lo) | ((uint32_t)(p.c.dst[col] - lo) << 16);   // both inside [0, n), n <= 1024 (uni_colgraph)
}

// check: one workgroup per graph compares the batch's adjacency with the fingerprint stored at add time
__global__ __launch_bounds__(UNI_BLOCK) void uni_pop_check(UgsPopCall p) {
    __shared__ uint64_t s_sum[UNI_BLOCK];
    const int64_t g = blockIdx.x;
    const uint64_t fp = pop_fingerprint(p.c, p.w, g, s_sum);
    if (threadIdx.x == 0 && p.pg[g].form != 0 && fp != p.pg[g].fp)
        atomicMax((unsigned long long *)&p.c.status[2], (unsigned long long)(p.c.G - g));
}

// the drawn key of a row, or false: the graph has nothing to draw from, or the draw is negative (a distinct call past |S_g|) -- a row of -1
__device__ __forceinline__ bool pop_key(const UgsPopCall &p, const UgsPopGraph &pg, int64_t row, int64_t g, uint64_t &key) {
    if (p.c.gsize[g] <= 0) return false;
    const int64_t d = p.c.seeds ? row : (int64_t)p.c.nepos[g] * p.c.m + (row - g * p.c.m);
    const int32_t draw = p.c.draws[d];
    if (draw < 0) return false;
    key = pg.keys[draw];
    return true;
}

// rows of the mask form and the rows of -1: lane l writes the members among the vertices 4 l ... 4 l + 3
__global__ __launch_bounds__(UNI_BLOCK) void uni_pop_rows(UgsPopCall p) {
    const UgsUniCall &c = p.c;
    const int64_t row = (int64_t)blockIdx.x * POP_GROUPS + threadIdx.x / POP_LANES;
    if (row >= c.rows) return;
    const int l = threadIdx.x & (POP_LANES - 1);
    const int64_t g = row / c.m;
    const UgsPopGraph pg = p.pg[g];
    uint64_t key = 0;
    const bool live = pop_key(p, pg, row, g, key);
    if (live && pg.form == 2) return;                               // uni_wpop_rows
    const uint64_t mask = live ? mask_of(key) : 0ull;
    // (a wide graph with keys hands its rows' keys to uni_wpop_fill: its row of -1 is marked, 0 being a key)
    if (l == 0) p.rowkey[row] = !live && pg.form == 2 && c.gsize[g] > 0 ? UGS_UNI_NO_KEY : mask;
    int64_t *out = c.nodes + row * c.k;
    uint32_t cnt = 0;
    if (mask) {
        int j = __popcll(mask & ((1ull << (4 * l)) - 1));
        for (uint32_t e = (uint32_t)(mask >> (4 * l)) & 15u; e; e &= e - 1) out[j++] = pg.lo + 4 * l + (__ffs(e) - 1);
        for (int64_t q = c.cstart[g] + l; q < c.cstart[g + 1]; q += POP_LANES) {
            const uint32_t uv = p.pair[q];
            cnt += (uint32_t)((mask >> (uv & 63)) & (mask >> ((uv >> 16) & 63)) & 1);
        }
    } else {
        for (int j = l; j < c.k; j += POP_LANES) out[j] = -1;
    }
    const uint32_t tot = row_scan(cnt);
    if (l == POP_LANES - 1) c.ecount[row] = tot;
}

__global__ __launch_bounds__(UNI_BLOCK) void uni_pop_fill(UgsPopCall p, int64_t *edge_index, int64_t *edge_src, int64_t ld) {
    const UgsUniCall &c = p.c;
    const int64_t row = (int64_t)blockIdx.x * POP_GROUPS + threadIdx.x / POP_LANES;
    if (row >= c.rows) return;
    const int l = threadIdx.x & (POP_LANES - 1);
    const int64_t g = row / c.m;
    const UgsPopGraph pg = p.pg[g];
    if (pg.form == 2 && c.gsize[g] > 0) return;                     // uni_wpop_fill
    const uint64_t mask = p.rowkey[row];
    if (!mask) return;
    int64_t w = c.edge_ptr[row];
    const int64_t end = c.cstart[g + 1];
    for (int64_t base = c.cstart[g]; base < end; base += POP_LANES) {   // (the trip count is the group's)
        const int64_t q = base + l;
        uint32_t hit = 0;
        int u = 0, v = 0;
        if (q < end) {
            const uint32_t uv = p.pair[q];
            u = uv & 63; v = (uv >> 16) & 63;
            hit = (uint32_t)((mask >> u) & (mask >> v) & 1);
        }
        const uint32_t incl = row_scan(hit);
        if (hit) {
            const int64_t o = w + (incl - hit);                     // hits of the lanes below: bucket order
            if (c.mode == 0) {
                edge_index[o] = __popcll(mask & ((1ull << u) - 1));
                edge_index[ld + o] = __popcll(mask & ((1ull << v) - 1));
            } else {
                edge_index[o] = pg.lo + u;
                edge_index[ld + o] = pg.lo + v;
            }
            edge_src[o] = c.cval2[q];
        }
        w += (uint32_t)__shfl((int)incl, POP_LANES - 1, POP_LANES);
    }
}

// rows of the wide graphs that have keys: lane j < k writes field j
__global__ __launch_bounds__(UNI_BLOCK) void uni_wpop_rows(UgsPopCall p) {
    const UgsUniCall &c = p.c;
    const int64_t row = (int64_t)blockIdx.x * POP_GROUPS + threadIdx.x / POP_LANES;
    if (row >= c.rows) return;
    const int l = threadIdx.x & (POP_LANES - 1);
    const int64_t g = row / c.m;
    const UgsPopGraph pg = p.pg[g];
    uint64_t key = 0;
    if (pg.form != 2 || !pop_key(p, pg, row, g, key)) return;       // uni_pop_rows has the row
    if (l == 0) p.rowkey[row] = key;
    const int k = c.k, b = pg.b;
    if (l < k) c.nodes[row * k + l] = pg.lo + (int64_t)((key >> (b * (k - 1 - l))) & ((1ull << b) - 1));
    uint32_t cnt = 0;
    for (int64_t q = c.cstart[g] + l; q < c.cstart[g + 1]; q += POP_LANES) {
        const uint32_t uv = p.pair[q];
        cnt += tuple_pos(key, k, b, uv & 0xFFFFu) >= 0 && tuple_pos(key, k, b, uv >> 16) >= 0 ? 1u : 0u;
    }
    const uint32_t tot = row_scan(cnt);
    if (l == POP_LANES - 1) c.ecount[row] = tot;
}

__global__ __launch_bounds__(UNI_BLOCK) void uni_wpop_fill(UgsPopCall p, int64_t *edge_index, int64_t *edge_src, int64_t ld) {
    const UgsUniCall &c = p.c;
    const int64_t row = (int64_t)blockIdx.x * POP_GROUPS + threadIdx.x / POP_LANES;
    if (row >= c.rows) return;
    const int l = threadIdx.x & (POP_LANES - 1);
    const int64_t g = row / c.m;
    const UgsPopGraph pg = p.pg[g];
    if (pg.form != 2 || c.gsize[g] <= 0) return;
    const int k = c.k, b = pg.b;
    const uint64_t key = p.rowkey[row];
    if (key == UGS_UNI_NO_KEY) return;                              // a row of -1 inside a live graph (the whole group leaves)
    int64_t w = c.edge_ptr[row];
    const int64_t end = c.cstart[g + 1];
    for (int64_t base = c.cstart[g]; base < end; base += POP_LANES) {
        const int64_t q = base + l;
        uint32_t hit = 0, uv = 0;
        int pu = -1, pv = -1;
        if (q < end) {
            uv = p.pair[q];
            pu = tuple_pos(key, k, b, uv & 0xFFFFu); pv = tuple_pos(key, k, b, uv >> 16);
            hit = pu >= 0 && pv >= 0 ? 1u : 0u;
        }
        const uint32_t incl = row_scan(hit);
        if (hit) {
            const int64_t o = w + (incl - hit);
            edge_index[o] = c.mode == 0 ? (int64_t)pu : pg.lo + (int64_t)(uv & 0xFFFFu);
            edge_index[ld + o] = c.mode == 0 ? (int64_t)pv : pg.lo + (int64_t)(uv >> 16);
            edge_src[o] = c.cval2[q];
        }
        w += (uint32_t)__shfl((int)incl, POP_LANES - 1, POP_LANES);
    }
}

// ---- WL class indices of a population (ugs_uniform_population_*_wl_begin): a stored key has one int32 class index beside it, the
//      class of its WL digest, hashed once at add time; a step turns a row's draw into a vocabulary id with two loads. ----
// ids_out[row] = id_of_class[cls of the row's drawn key]; unknown_id for a row of -1 (pop_key says so) or a key without a digest
__global__ __launch_bounds__(UNI_BLOCK) void uni_pop_wl_ids(UgsPopCall p, UgsPopWl q) {
    const int64_t row = (int64_t)blockIdx.x * UNI_BLOCK + threadIdx.x;
    if (row >= p.c.rows) return;
    const int64_t g = row / p.c.m;
    int64_t id = q.unknown_id;
    if (p.c.gsize[g] > 0) {                                         // the draw index, as pop_key reads it
        const int64_t d = p.c.seeds ? row : (int64_t)p.c.nepos[g] * p.c.m + (row - g * p.c.m);
        const int32_t draw = p.c.draws[d];
        if (draw >= 0) {
            const int32_t cls = q.cls[g][draw];
            if (cls >= 0) id = q.id_of_class[cls];
        }
    }
    q.ids_out[row] = id;
}

// The loop vertices of graph g (a loop changes a WL digest, never S_g): one workgroup per graph marks them in a bitmap of
// UGS_UNI_WIDE_MAX_N bits in LDS from the graph's column bucket and reduces it like an adjacency bitmap (fp_mix over the non-zero
// words).  out: the fingerprint is stored (add); want: it is compared with the stored one, status[3] = G - (first graph that differs).
__global__ __launch_bounds__(UNI_BLOCK) void uni_pop_loops(UgsUniCall c, const uint64_t *want, uint64_t *out) {
    constexpr int WORDS = UGS_UNI_WIDE_MAX_N / 64;
    __shared__ unsigned long long s_bits[WORDS];
    const int64_t g = blockIdx.x;
    const UgsUniGraph gd = c.graphs[g];
    if (threadIdx.x < WORDS) s_bits[threadIdx.x] = 0ull;
    __syncthreads();
    if (gd.enumerable)                                              // (n <= UGS_UNI_WIDE_MAX_N; uni_colgraph kept both endpoints inside [0, n))
        for (int64_t q = c.cstart[g] + threadIdx.x; q < c.cstart[g + 1]; q += UNI_BLOCK) {
            const int64_t col = c.cval2[q];
            const int64_t u = c.src[col] - gd.lo;
            if (u == c.dst[col] - gd.lo && u >= 0 && u < UGS_UNI_WIDE_MAX_N) atomicOr(&s_bits[u >> 6], 1ull << (u & 63));
        }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t fp = 0;
    for (int i = 0; i < WORDS; ++i) if (s_bits[i]) fp += fp_mix(s_bits[i], (uint64_t)i);
    if (out) out[g] = fp;
    if (want && gd.enumerable && fp != want[g]) atomicMax((unsigned long long *)&c.status[3], (unsigned long long)(c.G - g));
}

// ---- graphlet census (ugs_graphlet_census): the count pass's search, every completed set classified where it is found ----
// The raw code of a set is the adjacency code (ugs_graphlet_canon's bit layout) of its vertices in the order the search placed them:
// the vertex placed at position j contributes column j, its adjacency to positions 0 .. j-1.  The search keeps the adjacency rows of
// the placed vertices (row[i]; the wide form: this lane's word of them), and since adjacency is symmetric bit w of row[i] is the
// adjacency of ANY vertex w to position i: a level adds one column to the code, and at k - 1 placed vertices every member of ext
// adds only its own.  KFIX = 0: k <= 7 at run time, a set's column is code_col[raw code]; KFIX = 8: k = 8, the canonical search per
// set (one leaf depth, so one inlined copy of it) and a binary search among the connected keys.
constexpr int CEN_ROWS = UGS_GL_KMAX - 1;
constexpr int CEN_MEMO_BITS = 9, CEN_MEMO = 1 << CEN_MEMO_BITS;   // k = 8: classified codes a workgroup remembers (4 KiB of LDS)
constexpr int CEN_MASK_BLOCK = 64;            // the mask form: one wave per item (root, first extension), lane = second extension vertex

struct CenStack {                             // ugs_gl's per-level words of one thread, in LDS as [level][thread]
    uint64_t *base;
    int stride;
    __device__ __forceinline__ void put(int level, uint64_t v) { base[level * stride] = v; }
    __device__ __forceinline__ uint64_t get(int level) const { return base[level * stride]; }
};

// where a lane's classified sets go.  Equal columns in a row are merged into one add (a clique puts every set in one column).
template <int KFIX>
struct CenSink {
    const uint16_t *code_col;
    const int64_t *keys;
    uint32_t W;
    unsigned long long *hist;                 // KFIX = 0: the workgroup's W counters in LDS; KFIX = 8: the graph's row of counts
    CenStack st;
    uint32_t run_col, run;                    // the column of the last sets and how many of them are not yet added
    uint32_t last_code, last_col;             // KFIX = 8: the last raw code classified (~0: none) and its column
    unsigned long long *memo;                 // KFIX = 8: the workgroup's CEN_MEMO classified codes in LDS, behind the search's words
};

template <int KFIX>
__device__ __forceinline__ void cen_flush(CenSink<KFIX> &s) {
    if (s.run && s.run_col < s.W) atomicAdd(&s.hist[s.run_col], (unsigned long long)s.run);
    s.run = 0;
}

template <int KFIX>
__device__ __forceinline__ void cen_emit(CenSink<KFIX> &s, uint32_t code) {
    uint32_t col;
    if constexpr (KFIX == 0) {
        col = s.code_col[code];
    } else if (code == s.last_code) {                              // siblings at a leaf often attach alike (always in a clique or a
        col = s.last_col;                                           // complete bipartite graph): the search runs once per distinct code
    } else {
        // the workgroup's memo, direct-mapped: an entry is (code << 32) | column in one 64-bit word, so whatever lane wrote it last it
        // is whole, and it answers only for the code it names.  A column depends on the code alone, not on the graph.
        volatile unsigned long long *slot = s.memo + ((code * 0x9E3779B1u) >> (32 - CEN_MEMO_BITS));
        const unsigned long long seen = *slot;
        if ((uint32_t)(seen >> 32) == code) {
            col = (uint32_t)seen;
        } else {
            const int64_t key = ((int64_t)KFIX << 28) | (int64_t)ugs_gl::canon(ugs_gl::adj_of_code(code, KFIX), KFIX, s.st);
            uint32_t lo = 0, hi = s.W;                              // first column key >= key
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s.keys[mid] < key) lo = mid + 1; else hi = mid; }
            col = lo < s.W && s.keys[lo] == key ? lo : 0xFFFFu;
            *slot = ((unsigned long long)code << 32) | col;
        }
        s.last_code = code; s.last_col = col;
    }
    if (col != s.run_col) { cen_flush(s); s.run_col = col; }
    ++s.run;
}

// column of a vertex against the D placed ones: `bit` is the vertex (the wide form: its bit in this lane's word)
template <int D>
__device__ __forceinline__ uint32_t cen_column(const uint64_t (&row)[CEN_ROWS], int bit) {
    uint32_t col = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) col |= (uint32_t)((row[i] >> bit) & 1ull) << i;
    return col;
}

struct CenMask {
    const uint64_t *adj;          // the graph's neighbour masks
    uint64_t abv;                 // the vertices above the root
    int k;
    uint64_t row[CEN_ROWS];       // neighbour masks of the placed vertices, by position
    uint64_t cnt, flushed;        // this lane's sets, and how many of them it has added to the graph's running total
    unsigned long long *ctr;
    unsigned long long budget;
    bool stop;                    // the graph is past the limit
};

// D = k - 1 vertices are placed: every member of ext completes a set
template <int D, int KFIX>
__device__ __forceinline__ void cen_last(CenMask &x, CenSink<KFIX> &s, uint64_t ext, uint32_t code) {
    for (uint64_t e = ext; e; e &= e - 1)
        cen_emit(s, code | (cen_column<D>(x.row, __ffsll((unsigned long long)e) - 1) << ugs_gl::tri(D)));
    x.cnt += (uint64_t)__popcll(ext);
    if (x.cnt - x.flushed >= 4096) {                                // bounded work for a graph over the limit, as in uni_esu
        cen_flush(s);
        const unsigned long long add = x.cnt - x.flushed;
        x.flushed = x.cnt;
        if (atomicAdd(x.ctr, add) + add > x.budget) x.stop = true;
    }
}

template <int D, int KFIX>
__device__ __forceinline__ void cen_level(CenMask &x, CenSink<KFIX> &s, uint64_t ext, uint64_t nb, uint32_t code) {
    if constexpr (KFIX != 0 && D == KFIX - 1) {
        cen_last<D, KFIX>(x, s, ext, code);
    } else {
        if constexpr (KFIX == 0) {
            if (D == x.k - 1) { cen_last<D, KFIX>(x, s, ext, code); return; }
        }
        if constexpr (D < CEN_ROWS) {
            while (ext && !x.stop) {
                const int w = __ffsll((unsigned long long)ext) - 1;
                ext &= ext - 1;
                const uint64_t aw = x.adj[w];
                const uint32_t col = cen_column<D>(x.row, w);
                x.row[D] = aw;
                cen_level<D + 1, KFIX>(x, s, ext | (aw & ~nb & x.abv), nb | aw, code | (col << ugs_gl::tri(D)));
            }
        }
    }
}

// One workgroup (one wave) per item (root v, first extension w0) of uni_esu; lane j owns the sets whose next vertex, the first taken
// from the extension set of {v, w0}, is vertex j.  (k <= 3 has no such level: lane 0 does the item.)  A clique's sets crowd into the
// items of its lowest roots; this split gives them 64 times the lanes of the count pass's.  A workgroup whose w0 is no extension of
// v leaves at once.
template <int KFIX>
__global__ __launch_bounds__(CEN_MASK_BLOCK) void uni_census_esu(UgsUniCall c, UgsCensus z) {
    extern __shared__ unsigned long long cen_sh[];                  // KFIX = 0: W counters; KFIX = 8: the search's [8][64] words, the memo
    const int64_t vi = (int64_t)(blockIdx.x >> 6);
    const int w0 = (int)(blockIdx.x & 63), j = (int)threadIdx.x;
    const int32_t gi = c.vgraph[vi];
    const UgsUniGraph gd = c.graphs[gi];
    const int v = (int)(vi - gd.vbase);
    const int k = KFIX != 0 ? KFIX : c.k;
    CenMask x;
    x.adj = c.adj + gd.vbase; x.abv = above_mask(v); x.k = k;
    const uint64_t av = x.adj[v];
    const uint64_t ext1 = av & x.abv;
    if (k == 1 ? w0 != 0 : !((ext1 >> w0) & 1)) return;            // the whole workgroup: no barrier is left behind
    const uint32_t W = (uint32_t)z.W;
    CenSink<KFIX> s;
    s.memo = cen_sh + UGS_GL_KMAX * CEN_MASK_BLOCK;
    if (KFIX == 0) {
        for (uint32_t i = (uint32_t)j; i < W; i += CEN_MASK_BLOCK) cen_sh[i] = 0;
    } else {
        for (int i = j; i < CEN_MEMO; i += CEN_MASK_BLOCK) s.memo[i] = ~0ull;      // no code has 32 bits
    }
    __syncthreads();
    s.code_col = z.code_col; s.keys = z.keys; s.W = W;
    s.hist = KFIX == 0 ? cen_sh : z.counts + (int64_t)gi * (int64_t)W;
    s.st.base = (uint64_t *)cen_sh + j; s.st.stride = CEN_MASK_BLOCK;
    s.run_col = 0xFFFFu; s.run = 0; s.last_code = ~0u; s.last_col = 0xFFFFu;
    x.cnt = 0; x.flushed = 0; x.stop = false;
    x.ctr = (unsigned long long *)&c.gcount[gi]; x.budget = (unsigned long long)c.budget;
#pragma unroll
    for (int i = 0; i < CEN_ROWS; ++i) x.row[i] = 0;
    if (*(volatile unsigned long long *)x.ctr <= x.budget) {        // a graph already past the limit starts nothing more
        if constexpr (KFIX == 0) {
            if (k <= 2 && j == 0) { cen_emit(s, k == 1 ? 0u : 1u); x.cnt = 1; }
        }
        if (k >= 3) {
            const uint64_t aw = x.adj[w0];
            const uint64_t nb1 = av | (1ull << v);
            const uint64_t ext2 = (ext1 & above_mask(w0)) | (aw & ~nb1 & x.abv), nb2 = nb1 | aw;
            x.row[0] = av; x.row[1] = aw;
            if constexpr (KFIX == 0) {
                if (k == 3 && j == 0) cen_level<2, KFIX>(x, s, ext2, nb2, 1u);
            }
            if (k >= 4 && ((ext2 >> j) & 1)) {
                const uint64_t aj = x.adj[j];
                const uint32_t col = cen_column<2>(x.row, j);
                x.row[2] = aj;
                cen_level<3, KFIX>(x, s, (ext2 & above_mask(j)) | (aj & ~nb2 & x.abv), nb2 | aj, 1u | (col << ugs_gl::tri(2)));
            }
        }
    }
    cen_flush(s);
    if (x.cnt > x.flushed) atomicAdd(x.ctr, (unsigned long long)(x.cnt - x.flushed));
    if (KFIX == 0) {
        __syncthreads();
        unsigned long long *dst = z.counts + (int64_t)gi * (int64_t)W;
        for (uint32_t i = (uint32_t)j; i < W; i += CEN_MASK_BLOCK) {
            const unsigned long long n = cen_sh[i];
            if (n) atomicAdd(&dst[i], n);
        }
    }
}

struct CenWide {
    WGroup g;                     // as the count pass carries it (out, status and b are not used)
    uint64_t row[CEN_ROWS];       // this lane's word of the placed vertices' bitmap rows, by position
};

template <int D, int KFIX>
__device__ __forceinline__ void wcen_last(CenWide &x, CenSink<KFIX> &s, uint64_t ext, uint32_t code) {
    for (uint64_t e = ext; e; e &= e - 1)                           // every lane: the members in its own word
        cen_emit(s, code | (cen_column<D>(x.row, __ffsll((unsigned long long)e) - 1) << ugs_gl::tri(D)));
    x.g.cnt += (uint32_t)__popcll(ext);
    bool over = false;
    if (x.g.cnt - x.g.flushed >= 4096 / WIDE_LANES) {               // the group flushes at least every 4096 sets
        cen_flush(s);
        const unsigned long long add = x.g.cnt - x.g.flushed;
        over = atomicAdd(x.g.ctr, add) + add > (unsigned long long)x.g.budget;
        x.g.flushed = x.g.cnt;
    }
    if (group_ballot(x.g, over)) x.g.stop = true;
}

template <int D, int KFIX>
__device__ __forceinline__ void wcen_level(CenWide &x, CenSink<KFIX> &s, uint64_t ext, uint64_t nb, uint32_t code) {
    if constexpr (KFIX != 0 && D == KFIX - 1) {
        wcen_last<D, KFIX>(x, s, ext, code);
    } else {
        if constexpr (KFIX == 0) {
            if (D == x.g.k - 1) { wcen_last<D, KFIX>(x, s, ext, code); return; }
        }
        if constexpr (D < CEN_ROWS) {
            while (!x.g.stop) {
                const int w = group_take(x.g, ext);
                if (w < 0) break;
                const uint64_t aw = x.g.l < x.g.W ? x.g.adj[(int64_t)w * x.g.W + x.g.l] : 0ull;
                const uint32_t col = (uint32_t)__shfl((int)cen_column<D>(x.row, w & 63), w >> 6, WIDE_LANES);   // the lane that holds w's word
                x.row[D] = aw;
                wcen_level<D + 1, KFIX>(x, s, ext | (aw & ~nb & x.g.abv), nb | aw, code | (col << ugs_gl::tri(D)));
            }
        }
    }
}

// uni_wesu's items and groups; the 16 items of a workgroup share their root, so the workgroup counts into one set of LDS counters.
template <int KFIX>
__global__ __launch_bounds__(UNI_BLOCK) void uni_census_wesu(UgsUniCall c, UgsUniWide wd, UgsCensus z) {
    extern __shared__ unsigned long long cen_sh[];                  // KFIX = 0: W counters; KFIX = 8: the search's [8][256] words, the memo
    const int64_t item = wd.nv_mask * 64 + (int64_t)blockIdx.x * WIDE_GROUPS + (threadIdx.x / WIDE_LANES);   // < nv * 64: the grid is exact
    const int64_t vi = item >> 6;
    const int slot = (int)(item & 63);
    const int32_t gi = c.vgraph[vi];
    const UgsUniGraph gd = c.graphs[gi];
    const uint32_t W = (uint32_t)z.W;
    CenSink<KFIX> s;
    s.memo = cen_sh + UGS_GL_KMAX * UNI_BLOCK;
    if (KFIX == 0) {
        for (uint32_t i = threadIdx.x; i < W; i += UNI_BLOCK) cen_sh[i] = 0;
    } else {
        for (int i = (int)threadIdx.x; i < CEN_MEMO; i += UNI_BLOCK) s.memo[i] = ~0ull;    // no code has 32 bits
    }
    __syncthreads();
    s.code_col = z.code_col; s.keys = z.keys; s.W = W;
    s.hist = KFIX == 0 ? cen_sh : z.counts + (int64_t)gi * (int64_t)W;
    s.st.base = (uint64_t *)cen_sh + threadIdx.x; s.st.stride = UNI_BLOCK;
    s.run_col = 0xFFFFu; s.run = 0; s.last_code = ~0u; s.last_col = 0xFFFFu;
    const int v = (int)(vi - gd.vbase), vw = v >> 6;
    CenWide x;
    x.g.adj = wd.wadj + wd.wbase[gi];
    x.g.W = (gd.n + 63) >> 6; x.g.l = threadIdx.x & (WIDE_LANES - 1); x.g.gshift = threadIdx.x & 63 & ~(WIDE_LANES - 1);
    x.g.b = 0; x.g.k = c.k;
    x.g.abv = x.g.l < vw ? 0ull : x.g.l == vw ? above_mask(v & 63) : ~0ull;
    x.g.out = nullptr; x.g.cnt = 0; x.g.flushed = 0;
    x.g.ctr = (unsigned long long *)&c.gcount[gi];
    x.g.budget = c.budget; x.g.status = nullptr; x.g.stop = false;
#pragma unroll
    for (int i = 0; i < CEN_ROWS; ++i) x.row[i] = 0;
    // a graph already past the limit starts nothing more; the lanes of a group must agree, whenever each of them read the total
    if (!group_ballot(x.g, *(volatile unsigned long long *)x.g.ctr > (unsigned long long)c.budget)) {
        const uint64_t av = x.g.l < x.g.W ? x.g.adj[(int64_t)v * x.g.W + x.g.l] : 0ull;
        const uint64_t ext1 = av & x.g.abv;
        const uint64_t nb1 = av | (x.g.l == vw ? 1ull << (v & 63) : 0ull);
        x.row[0] = av;
        if constexpr (KFIX == 0) {
            if (x.g.k == 1) {
                if (slot == 0 && x.g.l == 0) { cen_emit(s, 0u); x.g.cnt = 1; }
            } else if (x.g.k == 2) {
                if (slot == 0) wcen_last<1, KFIX>(x, s, ext1, 0u);
            }
        }
        if (x.g.k >= 3) {
            const uint32_t pc = (uint32_t)__popcll(ext1), incl = row_scan(pc), excl = incl - pc;
            const uint32_t deg = (uint32_t)__shfl((int)incl, WIDE_LANES - 1, WIDE_LANES);
            for (uint32_t r = (uint32_t)slot; r < deg && !x.g.stop; r += 64) {
                const bool holds = excl <= r && r < incl;           // this lane's word holds the r-th member
                int f = 0;
                if (holds) {
                    uint64_t t = ext1;
                    for (uint32_t i = r - excl; i > 0; --i) t &= t - 1;
                    f = __ffsll((unsigned long long)t) - 1;
                }
                const int l0 = __ffs(group_ballot(x.g, holds)) - 1;
                f = __shfl(f, l0, WIDE_LANES);
                const int w = l0 * 64 + f;
                const uint64_t aw = x.g.l < x.g.W ? x.g.adj[(int64_t)w * x.g.W + x.g.l] : 0ull;
                const uint64_t later = x.g.l < l0 ? 0ull : x.g.l == l0 ? above_mask(f) : ~0ull;   // the members of ext1 after w
                x.row[1] = aw;
                wcen_level<2, KFIX>(x, s, (ext1 & later) | (aw & ~nb1 & x.g.abv), nb1 | aw, 1u);
            }
        }
    }
    cen_flush(s);
    const uint32_t rest = row_scan(x.g.cnt - x.g.flushed);
    if (x.g.l == WIDE_LANES - 1 && rest) atomicAdd(x.g.ctr, (unsigned long long)rest);
    if (KFIX == 0) {
        __syncthreads();
        unsigned long long *dst = z.counts + (int64_t)gi * (int64_t)W;
        for (uint32_t i = threadIdx.x; i < W; i += UNI_BLOCK) {
            const unsigned long long n = cen_sh[i];
            if (n) atomicAdd(&dst[i], n);
        }
    }
}

// behind the census pass: a graph past the limit has a row of zeros
__global__ void uni_census_clear(UgsUniCall c, UgsCensus z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.G * z.W) return;
    if (c.gcount[i / z.W] > c.budget) z.counts[i] = 0;
}

// ---- graphlet vertex census (ugs_graphlet_vertex_census): the census's search, every completed set counted once per member ----
// Besides the raw code the search carries the ids of the placed vertices, local to their graph, FB bits a position in one 64-bit word
// (`ids`; the mask form: 6 bits, the wide form: 10 -- a wide graph has at most UGS_UNI_WIDE_MAX_N = 1024 vertices -- and at most six
// positions are placed before a leaf of k <= 7).  Like `code` it is a value handed down the unrolled levels: no indexed stack.  At
// k - 1 placed vertices every member of ext completes a set; one table load (ugs_gl::vertex_entry) gives the set's column and the
// local orbit index of each of its k positions.  The member's cell gets one add.  The k - 1 placed vertices are the same for all
// members of ext, so members with equal entries in a row are merged: one add of the run's length per placed position.
struct VcSink {
    const uint32_t *table;
    const int64_t *obase;
    unsigned long long *rows;     // the graph's first row of gdv
    int64_t O;
    uint32_t W;
};

// the run's length to the cells of the D placed vertices
template <int D, int FB>
__device__ __forceinline__ void vc_flush(const VcSink &s, uint32_t entry, int64_t ob, uint32_t run, uint64_t ids) {
    if (!run || ugs_gl::vertex_col(entry) >= s.W) return;           // (a set the search completes is connected: its entry has a column)
#pragma unroll
    for (int p = 0; p < D; ++p)
        atomicAdd(&s.rows[(int64_t)((ids >> (FB * p)) & ((1ull << FB) - 1)) * s.O + ob + ugs_gl::vertex_local(entry, p)], (unsigned long long)run);
}

// the members `ext` of one word (their ids are first + bit) against the D placed vertices
template <int D, int FB>
__device__ __forceinline__ void vc_members(const VcSink &s, const uint64_t (&row)[CEN_ROWS], uint64_t ext, int first, uint32_t code, uint64_t ids) {
    uint32_t run_entry = ugs_gl::VERTEX_NONE, run = 0;
    int64_t ob = 0;
    for (uint64_t e = ext; e; e &= e - 1) {
        const int bit = __ffsll((unsigned long long)e) - 1;
        const uint32_t entry = s.table[code | (cen_column<D>(row, bit) << ugs_gl::tri(D))];
        if (entry != run_entry) {
            vc_flush<D, FB>(s, run_entry, ob, run, ids);
            run_entry = entry; run = 0;
            ob = ugs_gl::vertex_col(entry) < s.W ? s.obase[ugs_gl::vertex_col(entry)] : 0;
        }
        ++run;
        if (ugs_gl::vertex_col(entry) < s.W)
            atomicAdd(&s.rows[(int64_t)(first + bit) * s.O + ob + ugs_gl::vertex_local(entry, D)], 1ull);
    }
    vc_flush<D, FB>(s, run_entry, ob, run, ids);
}

constexpr int VC_MASK_FB = 6, VC_WIDE_FB = 10;

template <int D>
__device__ __forceinline__ void vc_last(CenMask &x, const VcSink &s, uint64_t ext, uint32_t code, uint64_t ids) {
    vc_members<D, VC_MASK_FB>(s, x.row, ext, 0, code, ids);
    x.cnt += (uint64_t)__popcll(ext);
    if (x.cnt - x.flushed >= 4096) {                                // bounded work for a graph over the limit, as in uni_esu
        const unsigned long long add = x.cnt - x.flushed;
        x.flushed = x.cnt;
        if (atomicAdd(x.ctr, add) + add > x.budget) x.stop = true;
    }
}

template <int D>
__device__ __forceinline__ void vc_level(CenMask &x, const VcSink &s, uint64_t ext, uint64_t nb, uint32_t code, uint64_t ids) {
    if (D == x.k - 1) { vc_last<D>(x, s, ext, code, ids); return; }
    if constexpr (D < CEN_ROWS - 1) {                               // k <= 7: six vertices at most are placed before the leaf
        while (ext && !x.stop) {
            const int w = __ffsll((unsigned long long)ext) - 1;
            ext &= ext - 1;
            const uint64_t aw = x.adj[w];
            const uint32_t col = cen_column<D>(x.row, w);
            x.row[D] = aw;
            vc_level<D + 1>(x, s, ext | (aw & ~nb & x.abv), nb | aw, code | (col << ugs_gl::tri(D)), ids | ((uint64_t)w << (VC_MASK_FB * D)));
        }
    }
}

// uni_census_esu<0>'s items and lanes: one wave per item (root v, first extension w0), lane j the second extension vertex.  No LDS:
// the counts go to the k rows of each set.
__global__ __launch_bounds__(CEN_MASK_BLOCK) void uni_vcensus_esu(UgsUniCall c, UgsVertexCensus z) {
    const int64_t vi = (int64_t)(blockIdx.x >> 6);
    const int w0 = (int)(blockIdx.x & 63), j = (int)threadIdx.x;
    const int32_t gi = c.vgraph[vi];
    const UgsUniGraph gd = c.graphs[gi];
    const int v = (int)(vi - gd.vbase);
    const int k = c.k;
    CenMask x;
    x.adj = c.adj + gd.vbase; x.abv = above_mask(v); x.k = k;
    const uint64_t av = x.adj[v];
    const uint64_t ext1 = av & x.abv;
    if (k == 1 ? w0 != 0 : !((ext1 >> w0) & 1)) return;
    VcSink s;
    s.table = z.table; s.obase = z.obase; s.O = z.O; s.W = (uint32_t)z.W;
    s.rows = z.gdv + gd.lo * z.O;
    x.cnt = 0; x.flushed = 0; x.stop = false;
    x.ctr = (unsigned long long *)&c.gcount[gi]; x.budget = (unsigned long long)c.budget;
#pragma unroll
    for (int i = 0; i < CEN_ROWS; ++i) x.row[i] = 0;
    if (*(volatile unsigned long long *)x.ctr <= x.budget) {        // a graph already past the limit starts nothing more
        x.row[0] = av;
        if (k == 1 && j == 0) vc_last<0>(x, s, 1ull << v, 0u, 0ull);
        if (k == 2 && j == 0) vc_last<1>(x, s, 1ull << w0, 0u, (uint64_t)v);
        if (k >= 3) {
            const uint64_t aw = x.adj[w0];
            const uint64_t nb1 = av | (1ull << v);
            const uint64_t ext2 = (ext1 & above_mask(w0)) | (aw & ~nb1 & x.abv), nb2 = nb1 | aw;
            const uint64_t ids2 = (uint64_t)v | ((uint64_t)w0 << VC_MASK_FB);
            x.row[1] = aw;
            if (k == 3 && j == 0) vc_last<2>(x, s, ext2, 1u, ids2);
            if (k >= 4 && ((ext2 >> j) & 1)) {
                const uint64_t aj = x.adj[j];
                const uint32_t col = cen_column<2>(x.row, j);
                x.row[2] = aj;
                vc_level<3>(x, s, (ext2 & above_mask(j)) | (aj & ~nb2 & x.abv), nb2 | aj, 1u | (col << ugs_gl::tri(2)),
                            ids2 | ((uint64_t)j << (VC_MASK_FB * 2)));
            }
        }
    }
    if (x.cnt > x.flushed) atomicAdd(x.ctr, (unsigned long long)(x.cnt - x.flushed));
}

template <int D>
__device__ __forceinline__ void wvc_last(CenWide &x, const VcSink &s, uint64_t ext, uint32_t code, uint64_t ids) {
    vc_members<D, VC_WIDE_FB>(s, x.row, ext, x.g.l * 64, code, ids);   // every lane: the members in its own word
    x.g.cnt += (uint32_t)__popcll(ext);
    bool over = false;
    if (x.g.cnt - x.g.flushed >= 4096 / WIDE_LANES) {               // the group flushes at least every 4096 sets
        const unsigned long long add = x.g.cnt - x.g.flushed;
        over = atomicAdd(x.g.ctr, add) + add > (unsigned long long)x.g.budget;
        x.g.flushed = x.g.cnt;
    }
    if (group_ballot(x.g, over)) x.g.stop = true;
}

template <int D>
__device__ __forceinline__ void wvc_level(CenWide &x, const VcSink &s, uint64_t ext, uint64_t nb, uint32_t code, uint64_t ids) {
    if (D == x.g.k - 1) { wvc_last<D>(x, s, ext, code, ids); return; }
    if constexpr (D < CEN_ROWS - 1) {
        while (!x.g.stop) {
            const int w = group_take(x.g, ext);
            if (w < 0) break;
            const uint64_t aw = x.g.l < x.g.W ? x.g.adj[(int64_t)w * x.g.W + x.g.l] : 0ull;
            const uint32_t col = (uint32_t)__shfl((int)cen_column<D>(x.row, w & 63), w >> 6, WIDE_LANES);   // the lane that holds w's word
            x.row[D] = aw;
            wvc_level<D + 1>(x, s, ext | (aw & ~nb & x.g.abv), nb | aw, code | (col << ugs_gl::tri(D)), ids | ((uint64_t)w << (VC_WIDE_FB * D)));
        }
    }
}

// uni_census_wesu<0>'s items and groups, without its LDS counters
__global__ __launch_bounds__(UNI_BLOCK) void uni_vcensus_wesu(UgsUniCall c, UgsUniWide wd, UgsVertexCensus z) {
    const int64_t item = wd.nv_mask * 64 + (int64_t)blockIdx.x * WIDE_GROUPS + (threadIdx.x / WIDE_LANES);   // < nv * 64: the grid is exact
    const int64_t vi = item >> 6;
    const int slot = (int)(item & 63);
    const int32_t gi = c.vgraph[vi];
    const UgsUniGraph gd = c.graphs[gi];
    VcSink s;
    s.table = z.table; s.obase = z.obase; s.O = z.O; s.W = (uint32_t)z.W;
    s.rows = z.gdv + gd.lo * z.O;
    const int v = (int)(vi - gd.vbase), vw = v >> 6;
    CenWide x;
    x.g.adj = wd.wadj + wd.wbase[gi];
    x.g.W = (gd.n + 63) >> 6; x.g.l = threadIdx.x & (WIDE_LANES - 1); x.g.gshift = threadIdx.x & 63 & ~(WIDE_LANES - 1);
    x.g.b = 0; x.g.k = c.k;
    x.g.abv = x.g.l < vw ? 0ull : x.g.l == vw ? above_mask(v & 63) : ~0ull;
    x.g.out = nullptr; x.g.cnt = 0; x.g.flushed = 0;
    x.g.ctr = (unsigned long long *)&c.gcount[gi];
    x.g.budget = c.budget; x.g.status = nullptr; x.g.stop = false;
#pragma unroll
    for (int i = 0; i < CEN_ROWS; ++i) x.row[i] = 0;
    // a graph already past the limit starts nothing more; the lanes of a group must agree, whenever each of them read the total
    if (!group_ballot(x.g, *(volatile unsigned long long *)x.g.ctr > (unsigned long long)c.budget)) {
        const uint64_t av = x.g.l < x.g.W ? x.g.adj[(int64_t)v * x.g.W + x.g.l] : 0ull;
        const uint64_t ext1 = av & x.g.abv;
        const uint64_t nb1 = av | (x.g.l == vw ? 1ull << (v & 63) : 0ull);
        x.row[0] = av;
        if (x.g.k == 1) {
            if (slot == 0) wvc_last<0>(x, s, x.g.l == vw ? 1ull << (v & 63) : 0ull, 0u, 0ull);
        } else if (x.g.k == 2) {
            if (slot == 0) wvc_last<1>(x, s, ext1, 0u, (uint64_t)v);
        } else {
            const uint32_t pc = (uint32_t)__popcll(ext1), incl = row_scan(pc), excl = incl - pc;
            const uint32_t deg = (uint32_t)__shfl((int)incl, WIDE_LANES - 1, WIDE_LANES);
            for (uint32_t r = (uint32_t)slot; r < deg && !x.g.stop; r += 64) {
                const bool holds = excl <= r && r < incl;           // this lane's word holds the r-th member
                int f = 0;
                if (holds) {
                    uint64_t t = ext1;
                    for (uint32_t i = r - excl; i > 0; --i) t &= t - 1;
                    f = __ffsll((unsigned long long)t) - 1;
                }
                const int l0 = __ffs(group_ballot(x.g, holds)) - 1;
                f = __shfl(f, l0, WIDE_LANES);
                const int w = l0 * 64 + f;
                const uint64_t aw = x.g.l < x.g.W ? x.g.adj[(int64_t)w * x.g.W + x.g.l] : 0ull;
                const uint64_t later = x.g.l < l0 ? 0ull : x.g.l == l0 ? above_mask(f) : ~0ull;   // the members of ext1 after w
                x.row[1] = aw;
                wvc_level<2>(x, s, (ext1 & later) | (aw & ~nb1 & x.g.abv), nb1 | aw, 1u, (uint64_t)v | ((uint64_t)w << VC_WIDE_FB));
            }
        }
    }
    const uint32_t rest = row_scan(x.g.cnt - x.g.flushed);
    if (x.g.l == WIDE_LANES - 1 && rest) atomicAdd(x.g.ctr, (unsigned long long)rest);
}

// behind the vertex census pass: the vertices of a graph past the limit have rows of zeros.  One workgroup per graph.
__global__ __launch_bounds__(UNI_BLOCK) void uni_vcensus_clear(UgsUniCall c, UgsVertexCensus z) {
    const int64_t g = (int64_t)blockIdx.x;
    if (c.gcount[g] <= c.budget) return;
    const UgsUniGraph gd = c.graphs[g];
    unsigned long long *rows = z.gdv + gd.lo * z.O;
    const int64_t cells = (int64_t)gd.n * z.O;
    for (int64_t i = threadIdx.x; i < cells; i += UNI_BLOCK) rows[i] = 0;
}

inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// uni_draw_distinct over every graph of the call; the sort's width, and with it the LDS, follows m, not the limit
inline void launch_draw_distinct(const UgsUniCall &c, hipStream_t s) {
    if (c.m <= 0 || c.m > UGS_UNI_DISTINCT_MAX_M) return;          // (the begins refuse a larger m before any device work)
    size_t P = 1;
    while (P < (size_t)c.m) P <<= 1;
    hipLaunchKernelGGL(uni_draw_distinct, dim3((unsigned)c.G), dim3(UNI_BLOCK), P * sizeof(uint64_t), s, c);
}

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

// The stages every entry shares, up to the per-graph sizes: column buckets, adjacency, the count pass and -- unless `count_only` --
// scan, write pass, sorts, gstart / gsize.  count_only stops behind the count pass: it touches neither ioff nor a key array.
// With `cen` or `vcen` (count_only) the census pass, or the vertex census pass, takes the count pass's place.
static hipError_t uni_prepare(UgsUniCall &c, const UgsUniWide &w, bool count_only, hipStream_t s, const UgsCensus *cen = nullptr,
                              const UgsVertexCensus *vcen = nullptr) {
    const int64_t nv_wide = c.nv - w.nv_mask;                                  // 0: the call runs the mask form's launches only
    UgsUniCall cm = c;                                                         // the mask form's view: its own roots
    cm.nv = w.nv_mask;
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
        if (nv_wide > 0) {
            if ((e = hipMemsetAsync(w.wadj, 0, (size_t)w.adj_words * sizeof(uint64_t), s)) != hipSuccess) return e;
            if (c.E > 0) hipLaunchKernelGGL(uni_wadj, dim3(blocks(c.E, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, w);
        }
        const int64_t items = c.nv * 64, mitems = cm.nv * 64, witems = nv_wide * 64;
        if (c.per_graph && (e = hipMemsetAsync(c.gcount, 0, (size_t)c.G * sizeof(int64_t), s)) != hipSuccess) return e;
        if (cen) {                                                             // k <= 7: LDS counters; k = 8: the canonical search's words and the memo
            const bool table = cen->code_col != nullptr;
            const size_t words = table ? (size_t)cen->W : (size_t)UGS_GL_KMAX;
            if (mitems > 0x7fffffffll) return hipErrorInvalidConfiguration;    // one workgroup per item of the mask roots
            if (mitems > 0) {
                const size_t lds = (table ? words : words * CEN_MASK_BLOCK + CEN_MEMO) * sizeof(uint64_t);
                if (table) hipLaunchKernelGGL((uni_census_esu<0>), dim3((unsigned)mitems), dim3(CEN_MASK_BLOCK), lds, s, cm, *cen);
                else hipLaunchKernelGGL((uni_census_esu<UGS_GL_KMAX>), dim3((unsigned)mitems), dim3(CEN_MASK_BLOCK), lds, s, cm, *cen);
            }
            if (witems > 0) {
                const size_t lds = (table ? words : words * UNI_BLOCK + CEN_MEMO) * sizeof(uint64_t);
                if (table) hipLaunchKernelGGL((uni_census_wesu<0>), dim3(blocks(witems, WIDE_GROUPS)), dim3(UNI_BLOCK), lds, s, c, w, *cen);
                else hipLaunchKernelGGL((uni_census_wesu<UGS_GL_KMAX>), dim3(blocks(witems, WIDE_GROUPS)), dim3(UNI_BLOCK), lds, s, c, w, *cen);
            }
            return hipGetLastError();
        }
        if (vcen) {
            if (mitems > 0x7fffffffll) return hipErrorInvalidConfiguration;    // one workgroup per item of the mask roots
            if (mitems > 0) hipLaunchKernelGGL(uni_vcensus_esu, dim3((unsigned)mitems), dim3(CEN_MASK_BLOCK), 0, s, cm, *vcen);
            if (witems > 0) hipLaunchKernelGGL(uni_vcensus_wesu, dim3(blocks(witems, WIDE_GROUPS)), dim3(UNI_BLOCK), 0, s, c, w, *vcen);
            return hipGetLastError();
        }
        if (mitems > 0) {
            if (c.k <= 8) hipLaunchKernelGGL((uni_esu<8, false>), dim3(blocks(mitems, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, cm);
            else hipLaunchKernelGGL((uni_esu<64, false>), dim3(blocks(mitems, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, cm);
        }
        if (witems > 0) hipLaunchKernelGGL((uni_wesu<false>), dim3(blocks(witems, WIDE_GROUPS)), dim3(UNI_BLOCK), 0, s, c, w);
        if (count_only) return hipGetLastError();
        if (c.per_graph) hipLaunchKernelGGL(uni_cap, dim3(blocks(items, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        if ((e = ugs_launch_scan(c.icount, items, c.ioff, c.scan_tmp, s)) != hipSuccess) return e;
        if (c.per_graph) hipLaunchKernelGGL(uni_joint, dim3(1), dim3(64), 0, s, c);
        if (mitems > 0) {
            if (c.k <= 8) hipLaunchKernelGGL((uni_esu<8, true>), dim3(blocks(mitems, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, cm);
            else hipLaunchKernelGGL((uni_esu<64, true>), dim3(blocks(mitems, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, cm);
        }
        if (witems > 0) hipLaunchKernelGGL((uni_wesu<true>), dim3(blocks(witems, WIDE_GROUPS)), dim3(UNI_BLOCK), 0, s, c, w);
        // root buckets larger than LDS: rocPRIM's segmented radix sort (the others are empty segments there)
        hipLaunchKernelGGL(uni_segments, dim3(blocks(c.nv, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
        hipcub::DoubleBuffer<uint64_t> keys(c.keys_a, c.keys_b);
        size_t tb = c.cub_bytes;
        e = hipcub::DeviceSegmentedRadixSort::SortKeys(c.cub_tmp, tb, keys, (int)c.budget, (int)c.nv, c.seg_lo, c.seg_hi, 0, 64, s);
        if (e != hipSuccess) return e;
        c.keys_sorted = keys.Current();
        hipLaunchKernelGGL(uni_sort_small, dim3((unsigned)c.nv), dim3(UNI_BLOCK), 0, s, c, keys.Current());
    }
    if (c.G > 0 && !count_only) hipLaunchKernelGGL(uni_graph_sizes, dim3(blocks(c.G, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
    return hipGetLastError();
}

hipError_t ugs_uniform_begin(UgsUniCall &c, const UgsUniWide &w, hipStream_t s) {
    const int64_t nv_wide = c.nv - w.nv_mask;
    hipError_t e = uni_prepare(c, w, false, s);
    if (e != hipSuccess) return e;
    UgsUniCall cm = c;                                                         // the mask form's view: its own graphs' sizes
    cm.nv = w.nv_mask;
    if (nv_wide > 0) cm.gsize = w.gsize_mask;
    if (c.G > 0) {
        if (nv_wide > 0) hipLaunchKernelGGL(uni_wsizes, dim3(blocks(c.G, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, w);
        if (c.seeds && c.distinct) launch_draw_distinct(c, s);
        else if (c.seeds) hipLaunchKernelGGL(uni_draw_graphs, dim3((unsigned)c.G), dim3(DRAW_BLOCK), 0, s, c);
        else hipLaunchKernelGGL(uni_draw, dim3(1), dim3(DRAW_BLOCK), 0, s, c);
    }
    if (c.rows > 0) hipLaunchKernelGGL(uni_rows, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, cm);
    if (c.rows > 0 && nv_wide > 0) hipLaunchKernelGGL(uni_wrows, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return ugs_launch_scan(c.ecount, c.rows, c.edge_ptr, c.scan_tmp, s);
}

hipError_t ugs_uniform_fill(const UgsUniCall &c, const UgsUniWide &w, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
    if (c.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(uni_fill, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, edge_index, edge_src, ld);
    if (c.nv > w.nv_mask) hipLaunchKernelGGL(uni_wfill, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, w, edge_index, edge_src, ld);
    return hipGetLastError();
}

hipError_t ugs_uniform_count(UgsUniCall &c, const UgsUniWide &w, hipStream_t s) { return uni_prepare(c, w, true, s); }

hipError_t ugs_uniform_enum_keys(UgsUniCall &c, const UgsUniWide &w, hipStream_t s) { return uni_prepare(c, w, false, s); }

// k = 8 goes without the table (code_col == nullptr), every smaller k with it: the host entry checks that
hipError_t ugs_uniform_census(UgsUniCall &c, const UgsUniWide &w, const UgsCensus &z, hipStream_t s) {
    const int64_t cells = c.G * z.W;
    hipError_t e = cells > 0 ? hipMemsetAsync(z.counts, 0, (size_t)cells * sizeof(uint64_t), s) : hipSuccess;
    if (e != hipSuccess) return e;
    if ((e = uni_prepare(c, w, true, s, &z)) != hipSuccess) return e;
    if (c.nv > 0 && cells > 0) hipLaunchKernelGGL(uni_census_clear, dim3(blocks(cells, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, z);
    return hipGetLastError();
}

// k <= 7 and the table: the host entry checks that
hipError_t ugs_uniform_vertex_census(UgsUniCall &c, const UgsUniWide &w, const UgsVertexCensus &z, hipStream_t s) {
    const int64_t cells = z.N * z.O;
    hipError_t e = cells > 0 ? hipMemsetAsync(z.gdv, 0, (size_t)cells * sizeof(uint64_t), s) : hipSuccess;
    if (e != hipSuccess) return e;
    if ((e = uni_prepare(c, w, true, s, nullptr, &z)) != hipSuccess) return e;
    if (c.nv > 0 && c.G > 0) hipLaunchKernelGGL(uni_vcensus_clear, dim3((unsigned)c.G), dim3(UNI_BLOCK), 0, s, c, z);
    return hipGetLastError();
}

hipError_t ugs_uniform_enum_rows(const UgsUniCall &c, const UgsUniWide &w, hipStream_t s) {
    if (c.rows > 0 && w.nv_mask > 0) hipLaunchKernelGGL(uni_enum_rows, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
    if (c.rows > 0 && c.nv > w.nv_mask) hipLaunchKernelGGL(uni_wenum_rows, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, w);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return ugs_launch_scan(c.ecount, c.rows, c.edge_ptr, c.scan_tmp, s);
}

hipError_t ugs_uniform_enum_fill(const UgsUniCall &c, const UgsUniWide &w, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
    if (c.rows <= 0) return hipSuccess;
    if (w.nv_mask > 0) hipLaunchKernelGGL(uni_enum_fill, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, edge_index, edge_src, ld);
    if (c.nv > w.nv_mask) hipLaunchKernelGGL(uni_wenum_fill, dim3(blocks(c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, w, edge_index, edge_src, ld);
    return hipGetLastError();
}

// ---- population cache ----
hipError_t ugs_uniform_pop_store(const UgsUniCall &c, const UgsUniWide &w, uint64_t *const *dst, uint64_t *fp_out, hipStream_t s) {
    if (c.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(uni_pop_store, dim3((unsigned)c.G, 32), dim3(UNI_BLOCK), 0, s, c, w, dst, fp_out);
    return hipGetLastError();
}

hipError_t ugs_uniform_pop_begin(UgsPopCall &p, hipStream_t s) {
    UgsUniCall &c = p.c;
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
    if (c.E > 0) hipLaunchKernelGGL(uni_pop_pairs, dim3(blocks(c.E, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, p);
    if (p.check && c.G > 0) {                                                  // the batch's adjacency, as uni_prepare builds it
        if (c.nv > 0) {
            if ((e = hipMemsetAsync(c.adj, 0, (size_t)c.nv * sizeof(uint64_t), s)) != hipSuccess) return e;
            if (c.E > 0) hipLaunchKernelGGL(uni_adj, dim3(blocks(c.E, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c);
            if (c.nv > p.w.nv_mask) {
                if ((e = hipMemsetAsync(p.w.wadj, 0, (size_t)p.w.adj_words * sizeof(uint64_t), s)) != hipSuccess) return e;
                if (c.E > 0) hipLaunchKernelGGL(uni_wadj, dim3(blocks(c.E, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, c, p.w);
            }
        }
        hipLaunchKernelGGL(uni_pop_check, dim3((unsigned)c.G), dim3(UNI_BLOCK), 0, s, p);
    }
    if (c.G > 0) {
        if (c.seeds && c.distinct) launch_draw_distinct(c, s);
        else if (c.seeds) hipLaunchKernelGGL(uni_draw_graphs, dim3((unsigned)c.G), dim3(DRAW_BLOCK), 0, s, c);
        else hipLaunchKernelGGL(uni_draw, dim3(1), dim3(DRAW_BLOCK), 0, s, c);
    }
    if (c.rows > 0) hipLaunchKernelGGL(uni_pop_rows, dim3(blocks(c.rows, POP_GROUPS)), dim3(UNI_BLOCK), 0, s, p);
    if (c.rows > 0 && p.any_wide) hipLaunchKernelGGL(uni_wpop_rows, dim3(blocks(c.rows, POP_GROUPS)), dim3(UNI_BLOCK), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return ugs_launch_scan(c.ecount, c.rows, c.edge_ptr, c.scan_tmp, s);
}

hipError_t ugs_uniform_pop_fill(const UgsPopCall &p, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
    if (p.c.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(uni_pop_fill, dim3(blocks(p.c.rows, POP_GROUPS)), dim3(UNI_BLOCK), 0, s, p, edge_index, edge_src, ld);
    if (p.any_wide) hipLaunchKernelGGL(uni_wpop_fill, dim3(blocks(p.c.rows, POP_GROUPS)), dim3(UNI_BLOCK), 0, s, p, edge_index, edge_src, ld);
    return hipGetLastError();
}

// ---- WL class indices of a population ----
hipError_t ugs_uniform_pop_loops(const UgsUniCall &c, const uint64_t *want, uint64_t *out, hipStream_t s) {
    if (c.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(uni_pop_loops, dim3((unsigned)c.G), dim3(UNI_BLOCK), 0, s, c, want, out);
    return hipGetLastError();
}

hipError_t ugs_uniform_pop_wl(const UgsPopCall &p, const UgsPopWl &q, hipStream_t s) {
    if (p.check && p.c.G > 0) hipLaunchKernelGGL(uni_pop_loops, dim3((unsigned)p.c.G), dim3(UNI_BLOCK), 0, s, p.c, q.lfp, (uint64_t *)nullptr);
    if (p.c.rows > 0) hipLaunchKernelGGL(uni_pop_wl_ids, dim3(blocks(p.c.rows, UNI_BLOCK)), dim3(UNI_BLOCK), 0, s, p, q);
    return hipGetLastError();
}
