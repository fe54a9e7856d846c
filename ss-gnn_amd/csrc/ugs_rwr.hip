// ugs_rwr.hip -- gfx950 pipeline of the random-walk-with-restart sampler (reference rwr_sampler).
//
// Contract: src/samplers/rwr_sampler/src/rwr_sampler.cpp with one OpenMP thread (law stated in include/ugs_mi355.h at
// ugs_rwr_sample_batch_begin): one SplitMix64 per graph seeded with seed + g, its m walks drawn one after the other from it.
// ugs_rwr_sample_graphs_begin seeds graph g with seeds[g] instead; global_view is the one place that reads either.
//
// The draws are counter-based: draw i (1-based) of graph g is mix(seed + g + (i + 1) * GAMMA).  So the walk that starts after
// c draws is a function of c alone, and so is L(c), the draws it consumes.  The real starts are the chain c0 = 0,
// c_{s+1} = c_s + L(c_s).  One workgroup per graph evaluates L at every offset of a window in parallel (speculate), follows the
// chain through the window in LDS (resolve) and slides the window to where the chain left it.
//
// Pipeline (one stream, no host round trip until the edge total):
//   rwr_init                    union-find parents
//   rwr_halfedges + radix sort  half-edges 2e + side keyed by source vertex, stable: each CSR row in (column, side) order;
//                               columns inside a graph also join their endpoints' components
//   rwr_compress                component roots and sizes
//   rwr_rowstart                CSR row starts; doomed[v]: v's component has fewer than k vertices
//   rwr_resolve                 one workgroup per graph: speculate / resolve windows -> rstart[row] (-1: a row of -1)
//   rwr_rows + scan             the chosen walks again: rows (node ids) and per-row edge counts -> edge_ptr
//   rwr_fill (finish)           edge_index / edge_src
// streams = "row" (ugs_rwr_sample_rows_begin: one generator per row, seeded with output s of the graph's) runs rwr_init ...
// rwr_rowstart as above, then rwr_row_walks in place of rwr_resolve + rwr_rows -- every walk is independent, there is no chain
// to follow and no doomed walk to measure -- then the same scan and rwr_fill.
// rwr_sampler.GraphCache runs rwr_init ... rwr_rowstart once per dataset graph (ugs_rwr_build) and
// rwr_store_append copies the result into a store laid out as one batch of all added graphs; a cached call then runs only
// rwr_store_check and the walks, scan and fill (ugs_rwr_walks, ugs_rwr_fill) with rs / hval2 / doomed pointing into the store.
//
// Doomed walks (seed in a component smaller than k) always run all 10 n k iterations.  Speculation stops them after the seed
// draw; when the chain reaches one, its length comes from the RNG alone (rwr_doomed_len): without edges every iteration takes one
// draw, otherwise one draw when r < p and two when not, whatever the vertex.
#include "ugs_device.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace {

constexpr int RWR_BLOCK = 256;
constexpr int RWR_WMAX = 4 * RWR_BLOCK;         // largest speculation window (spec <= 4)
constexpr int RWR_LDS_INTS = 8192;              // graphs whose CSR (+ doomed bytes) fits in 32 KiB walk from LDS
constexpr uint64_t SPEC_CAP = 64;              // speculation gives up on a walk at this many draws (lane 0 redoes it if needed)
constexpr uint64_t GAMMA = 0x9e3779b97f4a7c15ull;
constexpr int RWR_ROW_LANES = 64;               // rwr_row_walks: a workgroup is one wave, one row of its graph per lane

// LDS words of a graph of n vertices and D half-edges: row starts, targets, doomed bytes
__host__ __device__ __forceinline__ int64_t rwr_csr_words(int32_t n, int64_t D) { return (int64_t)n + 1 + D + (n + 3) / 4; }

__device__ __forceinline__ uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double to_double(uint64_t u) { return (double)(u >> 11) * (1.0 / 9007199254740992.0); }

// the walk's distinct vertices in registers (KM >= k); every loop is unrolled so that no index is dynamic
template <int KM>
struct Chosen {
    int32_t v[KM];
    int cnt;
    __device__ __forceinline__ bool has(int32_t x) const {
        bool h = false;
#pragma unroll
        for (int j = 0; j < KM; ++j) h |= (j < cnt) & (v[j] == x);
        return h;
    }
    __device__ __forceinline__ int find(int32_t x) const {
        int at = -1;
#pragma unroll
        for (int j = KM - 1; j >= 0; --j) if (j < cnt && v[j] == x) at = j;
        return at;
    }
    __device__ __forceinline__ void add(int32_t x) {
#pragma unroll
        for (int j = 0; j < KM; ++j) if (j == cnt) v[j] = x;
        ++cnt;
    }
};

// one graph's CSR, in LDS or in global memory: row v = tg[rs[v] .. rs[v+1]), local vertex ids
struct RwrView {
    const int32_t *rs, *tg;
    const uint8_t *doomed;
    uint64_t sg;          // the graph's generator: seed + g, or seeds[g] in a per-graph-seed call
    double p;
    int32_t n, k, T;
};

__device__ __forceinline__ RwrView global_view(const UgsRwrCall &c, int64_t g, const UgsRwrGraph &gd) {
    RwrView w;
    w.rs = c.rs + gd.vbase; w.tg = c.hval2; w.doomed = c.doomed + gd.vbase;
    w.sg = c.seeds ? c.seeds[g] : c.seed + (uint64_t)g; w.p = c.p; w.n = gd.n; w.k = c.k; w.T = gd.T;
    return w;
}

// One row's generator in a streams = "row" call (law at ugs_rwr_sample_rows_begin): output s (0-based) of the graph's own
// generator, the one output -- draw 0 -- that the per-graph law never uses.  The row's walk is the walk after c = 0 draws of it.
__device__ __forceinline__ RwrView row_view(RwrView w, int32_t s) { w.sg = mix(w.sg + ((uint64_t)s + 1) * GAMMA); return w; }

// The seed draw of the walk that starts after c draws: chosen = {seed}; z is left at the state of that draw.
template <int KM>
__device__ __forceinline__ int32_t rwr_walk_seed(const RwrView &w, uint64_t c, Chosen<KM> &ch, uint64_t &z) {
    z = w.sg + (c + 2) * GAMMA;                                     // state of draw c + 1
    const int32_t seed = (int32_t)(mix(z) % (uint64_t)w.n);
    ch.cnt = 0;
    ch.add(seed);
    return seed;
}

// One iteration of the walk's loop (reference :166-189); returns the draws it took, 1 or 2.
template <int KM>
__device__ __forceinline__ uint32_t rwr_walk_step(const RwrView &w, int32_t seed, int32_t &cur, Chosen<KM> &ch, uint64_t &z) {
    uint32_t L = 1;
    z += GAMMA;
    const double r = to_double(mix(z));
    const int32_t b = w.rs[cur], e = w.rs[cur + 1];
    if (r < w.p || b == e) {
        cur = seed;
    } else {
        z += GAMMA; ++L;
        cur = w.tg[b + (int32_t)(mix(z) % (uint64_t)(uint32_t)(e - b))];
    }
    if (!ch.has(cur)) ch.add(cur);
    return L;
}

// The walk that starts after c draws (reference :162-190).  Returns the draws it consumed, or 0 when its seed is doomed (the
// caller knows it fails and takes its length from rwr_doomed_len), or ~0 once it has taken `cap` draws without ending.
// ch holds the chosen vertices; ch.cnt == k: success.
template <int KM>
__device__ uint64_t rwr_walk(const RwrView &w, uint64_t c, Chosen<KM> &ch, uint64_t cap = ~0ull) {
    uint64_t z;
    const int32_t seed = rwr_walk_seed<KM>(w, c, ch, z);
    if (w.doomed[seed]) return 0;
    uint64_t L = 1;
    int32_t cur = seed;
    for (int32_t it = 0; ch.cnt < w.k && it < w.T; ++it) {
        if (L >= cap) return ~0ull;
        L += rwr_walk_step<KM>(w, seed, cur, ch, z);
    }
    return L;
}

struct DoomScratch {
    uint32_t bits[RWR_BLOCK];                  // bit j of lane t: the step draw at position pos + 32 t + j has r >= p
    uint8_t cnt[2][RWR_BLOCK], ex[2][RWR_BLOCK];   // per entry state: steps started in the lane's 32 positions, exit state
    uint64_t end;
    int32_t done;
};

// Length of the doomed walk after c draws (all lanes of the block call it; the result is uniform).  Its T = 10 n k iterations
// never stop early.  Without edges at the seed each takes one draw.  Otherwise a step at position x takes x, and x + 1 too when
// r(x) >= p: the lanes classify 8192 positions per round, each lane composes its 32 positions for both entry states (a step
// starts here / this is a neighbour draw), and lane 0 chains the 256 lanes until the T-th step.
__device__ uint64_t rwr_doomed_len(const RwrView &w, uint64_t c, DoomScratch &ds) {
    const int32_t seed = (int32_t)(mix(w.sg + (c + 2) * GAMMA) % (uint64_t)w.n);
    if (w.rs[seed] == w.rs[seed + 1]) return 1 + (uint64_t)w.T;
    const int tid = threadIdx.x;
    uint64_t pos = c + 2;                                           // draw index of the first step
    int64_t left = w.T;                                             // lane 0 only
    int state = 0;                                                  // lane 0 only: 0 = a step starts at pos
    while (true) {
        uint64_t z = w.sg + (pos + 32ull * tid + 1) * GAMMA;
        uint32_t bits = 0;
        for (int j = 0; j < 32; ++j, z += GAMMA) bits |= (to_double(mix(z)) < w.p ? 0u : 1u) << j;
        for (int e = 0; e < 2; ++e) {
            int st = e, n = 0;
            for (int j = 0; j < 32; ++j) {
                if (st == 0) { ++n; st = (bits >> j) & 1; }
                else st = 0;
            }
            ds.cnt[e][tid] = (uint8_t)n;
            ds.ex[e][tid] = (uint8_t)st;
        }
        ds.bits[tid] = bits;
        __syncthreads();
        if (tid == 0) {
            ds.done = 0;
            for (int t = 0; t < RWR_BLOCK; ++t) {
                const int n = ds.cnt[state][t];
                if (left <= n) {                                    // the T-th step starts in lane t's positions
                    const uint32_t b = ds.bits[t];
                    int st = state;
                    for (int j = 0; j < 32; ++j) {
                        if (st != 0) { st = 0; continue; }
                        const int bit = (b >> j) & 1;
                        if (--left == 0) { ds.end = pos + 32ull * t + j + bit; break; }   // its last draw
                        st = bit;
                    }
                    ds.done = 1;
                    break;
                }
                left -= n;
                state = ds.ex[state][t];
            }
        }
        __syncthreads();
        if (ds.done) {
            const uint64_t end = ds.end;
            __syncthreads();
            return end - c;
        }
        pos += 32ull * RWR_BLOCK;
    }
}

__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x) {
    int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) { x = p; p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return x;
}

__global__ void rwr_init(UgsRwrCall c) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= c.NV) return;
    c.parent[x] = (int32_t)x;
    c.csize[x] = 0;
}

__global__ void rwr_halfedges(UgsRwrCall c) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int64_t u = c.src[e], v = c.dst[e];
    // graph whose range holds u: the last g with ptr[g] <= u (empty graphs have ptr[g] == ptr[g+1] and hold nothing)
    int64_t lo = 0, hi = c.G;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (c.ptr[mid + 1] <= u) lo = mid + 1; else hi = mid; }
    if (!(lo < c.G && c.ptr[lo] <= u && u < c.ptr[lo + 1] && c.ptr[lo] <= v && v < c.ptr[lo + 1])) {
        c.hkey[2 * e] = c.hkey[2 * e + 1] = (uint32_t)c.NV;          // dropped: sorts behind every vertex
        c.hval[2 * e] = c.hval[2 * e + 1] = 0;
        return;
    }
    const int64_t base = c.ptr[0], glo = c.ptr[lo];
    int32_t a = (int32_t)(u - base), b = (int32_t)(v - base);
    c.hkey[2 * e] = (uint32_t)a;     c.hval[2 * e] = (int32_t)(v - glo);      // adj[u].push_back(v) first (:64)
    c.hkey[2 * e + 1] = (uint32_t)b; c.hval[2 * e + 1] = (int32_t)(u - glo);  // then adj[v].push_back(u) (:65)
    while (true) {                                                  // link the larger root under the smaller one
        a = uf_find(c.parent, a);
        b = uf_find(c.parent, b);
        if (a == b) break;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        if (atomicCAS(&c.parent[a], a, b) == a) break;
    }
}

__global__ void rwr_compress(UgsRwrCall c) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= c.NV) return;
    const int32_t r = uf_find(c.parent, (int32_t)x);
    c.parent[x] = r;
    atomicAdd(&c.csize[r], 1);
}

__global__ void rwr_rowstart(UgsRwrCall c) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > c.NV) return;
    int64_t lo = 0, hi = 2 * c.E;                                   // first sorted half-edge with key >= x
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)c.hkey2[mid] < x) lo = mid + 1; else hi = mid; }
    c.rs[x] = (int32_t)lo;
    if (x < c.NV) c.doomed[x] = c.csize[c.parent[x]] < c.k ? 1 : 0;
}

// One workgroup per graph: rstart[g * m + s] for its m rows.
template <int KM>
__global__ __launch_bounds__(RWR_BLOCK) void rwr_resolve(UgsRwrCall c) {
    __shared__ int32_t csr[RWR_LDS_INTS];
    __shared__ uint32_t sl[RWR_WMAX];          // L of the window's offsets (0: doomed seed)
    __shared__ uint8_t sf[RWR_WMAX];           // bit 0: the walk found k vertices; bit 1: speculation gave up on it (SPEC_CAP)
    __shared__ DoomScratch ds;
    __shared__ uint64_t sh_c;
    __shared__ int32_t sh_s, sh_pend;
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x;
    const UgsRwrGraph gd = c.graphs[g];
    int64_t *rstart = c.rstart + g * (int64_t)c.m;
    if (gd.T == 0) {                                                // n < k: m rows of -1, no draws (:136-159)
        for (int s = tid; s < c.m; s += RWR_BLOCK) rstart[s] = -1;
        return;
    }
    RwrView w = global_view(c, g, gd);
    const int32_t rs0 = c.rs[gd.vbase], D = c.rs[gd.vbase + gd.n] - rs0;
    if ((int64_t)gd.n + 1 + D + (gd.n + 3) / 4 <= RWR_LDS_INTS) {
        int32_t *lrs = csr, *ltg = csr + gd.n + 1;
        uint8_t *ldm = reinterpret_cast<uint8_t *>(ltg + D);
        for (int v = tid; v <= gd.n; v += RWR_BLOCK) lrs[v] = c.rs[gd.vbase + v] - rs0;
        for (int q = tid; q < D; q += RWR_BLOCK) ltg[q] = c.hval2[rs0 + q];
        for (int v = tid; v < gd.n; v += RWR_BLOCK) ldm[v] = c.doomed[gd.vbase + v];
        __syncthreads();
        w.rs = lrs; w.tg = ltg; w.doomed = ldm;
    }
    const int W = c.spec * RWR_BLOCK;
    uint64_t base = 0, cc = 0;
    int s = 0;
    while (s < c.m) {
        // speculate: every offset of the window, independently
        for (int o = tid; o < W; o += RWR_BLOCK) {
            Chosen<KM> ch;
            const uint64_t L = rwr_walk<KM>(w, base + o, ch, SPEC_CAP);
            sl[o] = (uint32_t)L;
            sf[o] = L == ~0ull ? 2 : ch.cnt >= w.k ? 1 : 0;
        }
        __syncthreads();
        // resolve: follow the chain through the window; a doomed start is measured by the whole block
        while (true) {
            if (tid == 0) {
                int pend = 0;
                while (s < c.m && cc < base + (uint64_t)W) {
                    const int o = (int)(cc - base);
                    uint64_t L = sl[o];
                    bool ok = sf[o] & 1;
                    if (sf[o] & 2) {                                // a long walk on the chain: lane 0 runs it to its end
                        Chosen<KM> ch;
                        L = rwr_walk<KM>(w, cc, ch);
                        ok = ch.cnt >= w.k;
                    }
                    if (L == 0) { pend = 1; break; }
                    rstart[s++] = ok ? (int64_t)cc : -1;
                    cc += L;
                }
                sh_c = cc; sh_s = s; sh_pend = pend;
            }
            __syncthreads();
            cc = sh_c; s = sh_s;
            const int pend = sh_pend;
            __syncthreads();
            if (!pend) break;
            const uint64_t L = rwr_doomed_len(w, cc, ds);
            if (tid == 0) rstart[s] = -1;
            ++s;
            cc += L;
        }
        base = cc;                                                  // slide: the next window starts where the chain is
    }
}

// a row of -1 without edges
__device__ __forceinline__ void rwr_row_failed(const UgsRwrCall &c, int64_t row) {
    int64_t *out = c.nodes + row * c.k;
    for (int j = 0; j < c.k; ++j) out[j] = -1;
    c.ecount[row] = 0;
}

// the row of a walk that found its k vertices: their ids and the row's edge count (:204-245)
template <int KM>
__device__ __forceinline__ void rwr_row_found(const UgsRwrCall &c, const RwrView &w, const UgsRwrGraph &gd, int64_t row, const Chosen<KM> &ch) {
    int64_t *out = c.nodes + row * c.k;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (j < c.k) {
            const int32_t u = ch.v[j];
            out[j] = gd.lo + u;
            for (int32_t q = w.rs[u]; q < w.rs[u + 1]; ++q) cnt += ch.has(w.tg[q]) ? 1u : 0u;
        }
    }
    c.ecount[row] = cnt;
}

// row = g * m + s: the walk at rstart[row] again, its vertices and its edge count
template <int KM>
__global__ __launch_bounds__(RWR_BLOCK) void rwr_rows(UgsRwrCall c) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows) return;
    const int64_t st = c.rstart[row];
    if (st < 0) { rwr_row_failed(c, row); return; }
    const int64_t g = row / c.m;
    const UgsRwrGraph gd = c.graphs[g];
    const RwrView w = global_view(c, g, gd);
    Chosen<KM> ch;
    (void)rwr_walk<KM>(w, (uint64_t)st, ch);
    rwr_row_found<KM>(c, w, gd, row, ch);
}

// streams = "row" (law at ugs_rwr_sample_rows_begin): every row owns a generator, so every walk is independent and this kernel
// stands in for rwr_resolve + rwr_rows.  A workgroup is one wave and serves RWR_ROW_LANES rows of ONE graph, one row per lane;
// it stages the graph's CSR and doomed bytes in LDS once (dynamic: the launch is sized to the largest graph under the
// RWR_LDS_INTS rule; larger graphs walk from global memory).  Walk lengths are long-tailed: every iteration of the loop is one
// step of each lane's walk, so the lanes run the same instructions whatever row they are in, and a wave lasts as long as its
// longest walk.  (Letting a finished lane take another row of the workgroup from a counter in LDS was measured and lost: the
// calls are bound by their longest walk, and a second row on its lane lengthens that)
// Rows the law fixes without walking are written without walking: n < k (T == 0), p_restart == 1 with k > 1 (every step
// restarts: no second vertex), and a seed in a component of fewer than k vertices -- nothing depends on such a walk's length here.
// rstart[row]: 0, or -1 for a row of -1 (all rwr_fill asks).
template <int KM>
__global__ __launch_bounds__(RWR_ROW_LANES) void rwr_row_walks(UgsRwrCall c) {
    extern __shared__ __attribute__((aligned(16))) int32_t row_csr[];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x / c.row_wgs;
    const int64_t s = (int64_t)(blockIdx.x % c.row_wgs) * RWR_ROW_LANES + tid;
    const int64_t row = g * (int64_t)c.m + s;
    const UgsRwrGraph gd = c.graphs[g];
    if (gd.T == 0 || (c.p >= 1.0 && c.k > 1)) {
        if (s < c.m) { rwr_row_failed(c, row); c.rstart[row] = -1; }
        return;
    }
    RwrView w = global_view(c, g, gd);
    const int32_t rs0 = c.rs[gd.vbase], D = c.rs[gd.vbase + gd.n] - rs0;
    if (rwr_csr_words(gd.n, D) <= c.row_lds_ints) {
        int32_t *lrs = row_csr, *ltg = row_csr + gd.n + 1;
        uint8_t *ldm = reinterpret_cast<uint8_t *>(ltg + D);
        for (int v = tid; v <= gd.n; v += RWR_ROW_LANES) lrs[v] = c.rs[gd.vbase + v] - rs0;
        for (int q = tid; q < D; q += RWR_ROW_LANES) ltg[q] = c.hval2[rs0 + q];
        for (int v = tid; v < gd.n; v += RWR_ROW_LANES) ldm[v] = c.doomed[gd.vbase + v];
        __syncthreads();
        w.rs = lrs; w.tg = ltg; w.doomed = ldm;
    }
    if (s >= c.m) return;
    Chosen<KM> ch;
    uint64_t z;
    const int32_t seed = rwr_walk_seed<KM>(row_view(w, (int32_t)s), 0, ch, z);     // the row's seed draw, on its own generator
    bool found = false;
    if (!w.doomed[seed]) {
        int32_t cur = seed;
        for (int32_t it = 0; ch.cnt < w.k && it < w.T; ++it) (void)rwr_walk_step<KM>(w, seed, cur, ch, z);
        found = ch.cnt >= w.k;
    }
    if (found) rwr_row_found<KM>(c, w, gd, row, ch);
    else rwr_row_failed(c, row);
    c.rstart[row] = found ? 0 : -1;
}

template <int KM>
__global__ __launch_bounds__(RWR_BLOCK) void rwr_fill(UgsRwrCall c, int64_t *edge_index, int64_t *edge_src, int64_t ld) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= c.rows || c.rstart[row] < 0) return;
    const int64_t g = row / c.m;
    const UgsRwrGraph gd = c.graphs[g];
    const RwrView w = global_view(c, g, gd);
    const int64_t *nd = c.nodes + row * c.k;
    Chosen<KM> ch;
    ch.cnt = c.k;
#pragma unroll
    for (int j = 0; j < KM; ++j) ch.v[j] = j < c.k ? (int32_t)(nd[j] - gd.lo) : -1;
    int64_t o = c.edge_ptr[row];
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (j < c.k) {
            const int32_t u = ch.v[j];
            for (int32_t q = w.rs[u]; q < w.rs[u + 1]; ++q) {
                const int32_t v = w.tg[q];
                const int at = ch.find(v);
                if (at < 0) continue;
                if (c.mode == 0) { edge_index[o] = j; edge_index[ld + o] = at; }
                else { edge_index[o] = gd.lo + u; edge_index[ld + o] = gd.lo + v; }
                edge_src[o] = -1;
                ++o;
            }
        }
    }
}

// ---- rwr_sampler.GraphCache: the CSRs of a dataset's graphs, built once by the stages above ----
// Appends the batch that rwr_init ... rwr_rowstart have just built to the store, behind everything it holds: row starts made
// absolute offsets into the store's targets (the walk, row and fill kernels read a graph only through rs + vbase, the targets
// and doomed + vbase, so they serve a store laid out as one batch of all added graphs), targets, doomed bytes, and every column
// narrowed to a pair of local vertex ids, in the order given (what rwr_store_check compares a batch with).  The host has made
// room, and has seen that every column lies inside one graph: no half-edge was dropped, the sorted targets are all 2E.
__global__ __launch_bounds__(RWR_BLOCK) void rwr_store_append(UgsRwrCall c, UgsRwrStore st) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x <= c.NV) st.rs[st.rs_base + x] = c.rs[x] + (int32_t)st.tg_base;
    if (x < c.NV) st.doomed[st.rs_base + x] = c.doomed[x];
    if (x < 2 * c.E) st.tg[st.tg_base + x] = c.hval2[x];
    if (x < c.E) {
        const int64_t u = c.src[x], v = c.dst[x];
        int64_t lo = 0, hi = c.G;                                   // the graph that holds u, as rwr_halfedges finds it
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (c.ptr[mid + 1] <= u) lo = mid + 1; else hi = mid; }
        const int64_t glo = c.ptr[lo < c.G ? lo : c.G];
        st.cols[st.col_base + x] = make_int2((int32_t)(u - glo), (int32_t)(v - glo));
    }
}

// The check of a cached call: batch column e belongs to the graph g with coff[g] <= e < coff[g + 1] and must be, shifted by
// ptr[g], the column stored at col0[g] + e - coff[g].  first_bad: the smallest g with a column that is not (host: set to a
// value above every g).  col0[g] < 0: a graph without stored columns (it failed when it was added; it is never walked).
__global__ __launch_bounds__(RWR_BLOCK) void rwr_store_check(UgsRwrCheck k) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= k.E) return;
    int64_t lo = 0, hi = k.G - 1;                                   // the last g with coff[g] <= e (coff[0] = 0, coff[G] = E > e)
    while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (k.coff[mid] <= e) lo = mid; else hi = mid - 1; }
    const int64_t c0 = k.col0[lo];
    if (c0 < 0) return;
    const int2 want = k.cols[c0 + e - k.coff[lo]];
    const int64_t base = k.graphs[lo].lo;
    if (k.src[e] - base != (int64_t)want.x || k.dst[e] - base != (int64_t)want.y) atomicMin(k.first_bad, (int32_t)lo);
}

inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

template <int KM>
void launch_walks(const UgsRwrCall &c, hipStream_t s) {
    hipLaunchKernelGGL((rwr_resolve<KM>), dim3((unsigned)c.G), dim3(RWR_BLOCK), 0, s, c);
    hipLaunchKernelGGL((rwr_rows<KM>), dim3(blocks(c.rows, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, c);
}

template <int KM>
void launch_row_walks(const UgsRwrCall &c, hipStream_t s) {
    const size_t lds = (size_t)c.row_lds_ints * sizeof(int32_t);
    hipLaunchKernelGGL((rwr_row_walks<KM>), dim3((unsigned)(c.G * c.row_wgs)), dim3(RWR_ROW_LANES), lds, s, c);
}

}  // namespace

void ugs_rwr_row_streams(UgsRwrCall &c, const UgsRwrGraph *graphs, const int64_t *half_edges) {
    c.row_streams = 1;
    c.row_wgs = (int32_t)(((int64_t)c.m + RWR_ROW_LANES - 1) / RWR_ROW_LANES);
    c.row_lds_ints = 0;
    const bool walks = !(c.p >= 1.0 && c.k > 1);
    for (int64_t g = 0; walks && g < c.G; ++g) {
        const int64_t words = rwr_csr_words(graphs[g].n, half_edges[g]);
        if (graphs[g].T > 0 && words <= RWR_LDS_INTS && words > c.row_lds_ints) c.row_lds_ints = (int32_t)words;
    }
}

size_t ugs_rwr_cub_bytes(int64_t E) {
    size_t a = 0;
    if (E > 0) (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr,
                                                       (int32_t *)nullptr, (int)(2 * E), 0, 32);
    return a;
}

hipError_t ugs_rwr_build(const UgsRwrCall &c, hipStream_t s) {
    hipError_t e;
    if (c.NV > 0) hipLaunchKernelGGL(rwr_init, dim3(blocks(c.NV, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, c);
    if (c.E > 0) {
        int bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) <= c.NV) ++bits;                 // keys 0..NV
        hipLaunchKernelGGL(rwr_halfedges, dim3(blocks(c.E, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, c);
        size_t tb = c.cub_bytes;
        e = hipcub::DeviceRadixSort::SortPairs(c.cub_tmp, tb, c.hkey, c.hkey2, c.hval, c.hval2, (int)(2 * c.E), 0, bits, s);
        if (e != hipSuccess) return e;
    }
    if (c.NV > 0) hipLaunchKernelGGL(rwr_compress, dim3(blocks(c.NV, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, c);
    hipLaunchKernelGGL(rwr_rowstart, dim3(blocks(c.NV + 1, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, c);
    return hipSuccess;
}

hipError_t ugs_rwr_walks(const UgsRwrCall &c, hipStream_t s) {
    hipError_t e;
    if (c.rows > 0 && c.row_streams) {
        if (c.G * c.row_wgs > (int64_t)INT32_MAX) return hipErrorInvalidValue;
        if (c.k <= 8) launch_row_walks<8>(c, s);
        else if (c.k <= 16) launch_row_walks<16>(c, s);
        else if (c.k <= 32) launch_row_walks<32>(c, s);
        else launch_row_walks<64>(c, s);
    } else if (c.rows > 0) {
        if (c.k <= 8) launch_walks<8>(c, s);
        else if (c.k <= 16) launch_walks<16>(c, s);
        else if (c.k <= 32) launch_walks<32>(c, s);
        else launch_walks<64>(c, s);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return ugs_launch_scan(c.ecount, c.rows, c.edge_ptr, c.scan_tmp, s);
}

hipError_t ugs_rwr_begin(const UgsRwrCall &c, hipStream_t s) {
    if (hipError_t e = ugs_rwr_build(c, s); e != hipSuccess) return e;
    return ugs_rwr_walks(c, s);
}

hipError_t ugs_rwr_store_append(const UgsRwrCall &c, const UgsRwrStore &st, hipStream_t s) {
    const int64_t n = std::max<int64_t>(c.NV + 1, 2 * c.E);
    hipLaunchKernelGGL(rwr_store_append, dim3(blocks(n, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, c, st);
    return hipGetLastError();
}

hipError_t ugs_rwr_store_check(const UgsRwrCheck &k, hipStream_t s) {
    if (k.E <= 0 || k.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(rwr_store_check, dim3(blocks(k.E, RWR_BLOCK)), dim3(RWR_BLOCK), 0, s, k);
    return hipGetLastError();
}

hipError_t ugs_rwr_fill(const UgsRwrCall &c, int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
    if (c.rows <= 0) return hipSuccess;
    const dim3 grid(blocks(c.rows, RWR_BLOCK)), block(RWR_BLOCK);
    if (c.k <= 8) hipLaunchKernelGGL((rwr_fill<8>), grid, block, 0, s, c, edge_index, edge_src, ld);
    else if (c.k <= 16) hipLaunchKernelGGL((rwr_fill<16>), grid, block, 0, s, c, edge_index, edge_src, ld);
    else if (c.k <= 32) hipLaunchKernelGGL((rwr_fill<32>), grid, block, 0, s, c, edge_index, edge_src, ld);
    else hipLaunchKernelGGL((rwr_fill<64>), grid, block, 0, s, c, edge_index, edge_src, ld);
    return hipGetLastError();
}
