// ugs_rows.hip -- ugs_sampler.rows.unique_rows on the device (gfx950): repeated subgraphs of a sampler's output merged per graph.
// The law is stated in include/ugs_mi355.h at ugs_rows_unique_begin; the host side is ugs_rows.cpp; DESIGN.md section 18.
//
// A call is five launches at begin and two at finish:
//   rows_check    every pointer array (monotone, ends where it must) and every graph's limits; lists the graphs of more than 64 rows
//   rows_keys     one lane per row: the row's graph, its entries validated and coded, the exact 128-bit key
//   rows_wave     graphs of at most 64 rows, one wave each: broadcast compares
//   rows_block    graphs of 65..4096 rows, one workgroup each: bitonic sort of (key, row) in LDS, runs by binary search
//   rows_scan     kept rows and their edge entries scanned across the graphs; totals and status words for the host
//   rows_compact  nodes_u, edge_ptr_u, sample_ptr_u, count, inverse
//   rows_edges    the kept rows' spans of edge_index and edge_src, 16 lanes a row
// Every kernel behind rows_check reads the status words first and does nothing unless the pointer arrays and the graphs passed, so
// no index is ever taken from a value that was not checked.  Nothing here depends on the launch shape: the only atomics are minima
// (status) and the appends to the lists of large graphs, whose order no result depends on.
#include "ugs_device.h"

#include <algorithm>

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;

__device__ inline bool rows_go(const UgsRowsCall &c) { return c.status[UGS_ROWS_ST_PTR] == UGS_ROWS_NONE && c.status[UGS_ROWS_ST_GRAPH] == UGS_ROWS_NONE; }
__device__ inline bool rows_go_all(const UgsRowsCall &c) { return rows_go(c) && c.status[UGS_ROWS_ST_ENTRY] == UGS_ROWS_NONE; }
__device__ inline void rows_bad(int64_t *word, int64_t v) { atomicMin(reinterpret_cast<long long *>(word), (long long)v); }

// ---- the check: nothing read here is used as an index ----
__global__ __launch_bounds__(256) void rows_check(UgsRowsCall c) {
    const int64_t top = c.R > c.G ? c.R : c.G;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= top; i += (int64_t)gridDim.x * 256) {
        if (i == 0) {
            if (c.sample_ptr[0] != 0) rows_bad(c.status + UGS_ROWS_ST_PTR, 0);
            if (c.sample_ptr[c.G] != c.R) rows_bad(c.status + UGS_ROWS_ST_PTR, 4 * c.G + 0);
            if (c.edge_ptr[0] != 0) rows_bad(c.status + UGS_ROWS_ST_PTR, 1);
            if (c.edge_ptr[c.R] != c.Es) rows_bad(c.status + UGS_ROWS_ST_PTR, 4 * c.R + 1);
        }
        if (i < c.R && c.edge_ptr[i] > c.edge_ptr[i + 1]) rows_bad(c.status + UGS_ROWS_ST_PTR, 4 * i + 1);
        bool small = false;                                            // a graph of 1..64 rows: the wave form's
        if (i < c.G) {
            const int64_t a = c.sample_ptr[i], b = c.sample_ptr[i + 1], lo = c.ptr[i], hi = c.ptr[i + 1];
            if (a > b) rows_bad(c.status + UGS_ROWS_ST_PTR, 4 * i + 0);
            if (lo > hi) rows_bad(c.status + UGS_ROWS_ST_PTR, 4 * i + 2);
            const int64_t rows = b - a;
            if (rows > 0) {
                if (rows > UGS_ROWS_MAX_PER_GRAPH) rows_bad(c.status + UGS_ROWS_ST_GRAPH, 2 * i + 0);
                else if (hi - lo + 1 > ((int64_t)1 << c.bits)) rows_bad(c.status + UGS_ROWS_ST_GRAPH, 2 * i + 1);
                else if (rows > 64) {
                    const int cls = rows <= 256 ? 0 : rows <= 1024 ? 1 : 2;
                    const int slot = atomicAdd(c.nbig + cls, 1);          // (at most G appends in all: i < G passes here once)
                    c.big[(int64_t)cls * c.G + slot] = (int32_t)i;
                } else small = true;
            }
        }
        const u64 sm = __ballot(small);                                // counted once per wave, by the first lane that has one
        if (small && (int)(threadIdx.x & 63) == __ffsll((unsigned long long)sm) - 1) atomicAdd(c.nbig + 3, __popcll(sm));
    }
}

// ---- keys ----
__device__ inline void or_shl(u64 &lo, u64 &hi, u32 code, int s) {      // (lo, hi) |= code << s, 0 <= s, s + bits <= 128
    const u64 v = code;
    if (s < 64) { lo |= v << s; if (s > 0) hi |= v >> (64 - s); }
    else hi |= v << (s - 64);
}

__device__ inline u32 rows_code(int64_t v, int64_t lo, int64_t n, bool &bad) {
    if (v == -1) return 0;
    const int64_t d = v - lo;
    if (v < -1 || d < 0 || d >= n) { bad = true; return 0; }
    return (u32)(d + 1);                                               // < 2^bits: the graph passed rows_check
}

// K > 0: the row's K codes in registers, every index a compile-time constant.  K == 0 (k > 8): the looped form, which reads the
// row again for every compare instead of holding it.
template <int K>
__global__ __launch_bounds__(256) void rows_keys(UgsRowsCall c) {
    if (!rows_go(c)) return;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= c.R) return;
    int64_t a = 1, b = c.G;                                            // first j in [1, G] with sample_ptr[j] > r: it exists, sample_ptr[G] = R
    while (a < b) { const int64_t mid = a + ((b - a) >> 1); if (c.sample_ptr[mid] > r) b = mid; else a = mid + 1; }
    const int64_t g = a - 1;                                           // sample_ptr[g] <= r < sample_ptr[g + 1]
    const int64_t lo = c.ptr[g], n = c.ptr[g + 1] - lo;
    const int64_t *row = c.nodes + r * c.k;
    const int bits = c.bits;
    bool bad = false;
    u64 klo = 0, khi = 0;
    if (K > 0) {
        u32 code[K > 0 ? K : 1];
#pragma unroll
        for (int i = 0; i < K; ++i) code[i] = rows_code(row[i], lo, n, bad);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            int pos = i;
            if (c.by) {
                pos = 0;
#pragma unroll
                for (int j = 0; j < K; ++j) pos += (code[j] < code[i] || (code[j] == code[i] && j < i)) ? 1 : 0;
            }
            or_shl(klo, khi, code[i], pos * bits);
        }
    } else {
        const int k = c.k;
        for (int i = 0; i < k; ++i) {
            const u32 ci = rows_code(row[i], lo, n, bad);
            int pos = i;
            if (c.by) {
                pos = 0;
                bool ignore = false;
                for (int j = 0; j < k; ++j) { const u32 cj = rows_code(row[j], lo, n, ignore); pos += (cj < ci || (cj == ci && j < i)) ? 1 : 0; }
            }
            or_shl(klo, khi, ci, pos * bits);
        }
    }
    if (bad) rows_bad(c.status + UGS_ROWS_ST_ENTRY, r);
    c.keys[r] = make_uint4((u32)klo, (u32)(klo >> 32), (u32)khi, (u32)(khi >> 32));
    c.rowg[r] = (int32_t)g;
}

// ---- dedup, wave form: graphs of at most 64 rows, one wave a graph, four graphs a workgroup ----
__device__ inline int64_t wave_scan_incl(int64_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int64_t t = __shfl_up(x, d, 64); if (lane >= d) x += t; }
    return x;
}

__global__ __launch_bounds__(256) void rows_wave(UgsRowsCall c) {
    if (!rows_go_all(c)) return;
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= c.G) return;
    const int64_t r0 = c.sample_ptr[g];
    const int n = (int)(c.sample_ptr[g + 1] - r0);                     // (at most 4096: the graph passed rows_check)
    if (n > 64) return;                                                // the workgroup form's
    if (n == 0) { if (lane == 0) { c.ug[g] = 0; c.eg[g] = 0; } return; }
    const bool live = lane < n;
    const int64_t r = r0 + lane;
    uint4 key = make_uint4(0, 0, 0, 0);
    int64_t elen = 0;
    if (live) { key = c.keys[r]; elen = c.edge_ptr[r + 1] - c.edge_ptr[r]; }
    int rep = -1, cnt = 0;
    for (int j = 0; j < n; ++j) {                                      // n is the same for the whole wave
        const u32 x = __shfl(key.x, j, 64), y = __shfl(key.y, j, 64), z = __shfl(key.z, j, 64), w = __shfl(key.w, j, 64);
        const bool eq = x == key.x && y == key.y && z == key.z && w == key.w;
        if (eq) { if (rep < 0) rep = j; ++cnt; }
    }
    const bool kept = live && rep == lane;
    const u64 mask = __ballot(kept);
    const int rank = __popcll(mask & (((u64)1 << lane) - 1));
    const int64_t e = kept ? elen : 0;
    const int64_t incl = wave_scan_incl(e, lane);
    const int64_t total = __shfl(incl, 63, 64);
    if (live) {
        c.rep[r] = (int32_t)(r0 + rep);
        if (kept) { c.lrank[r] = rank; c.cnt[r] = cnt; c.eoff[r] = incl - e; }
    }
    if (lane == 0) { c.ug[g] = __popcll(mask); c.eg[g] = total; }
}

// ---- exclusive scan of two values across a workgroup of NT threads (NT a multiple of 64, at most 1024); two barriers ----
__device__ inline void block_scan2(int64_t a, int64_t b, int nt, int64_t (*wt)[16], int64_t &ea, int64_t &eb, int64_t &ta, int64_t &tb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = nt >> 6;
    const int64_t ia = wave_scan_incl(a, lane), ib = wave_scan_incl(b, lane);
    __syncthreads();                                                   // (the previous use of wt is over)
    if (lane == 63) { wt[0][w] = ia; wt[1][w] = ib; }
    __syncthreads();
    int64_t ba = 0, bb = 0; ta = 0; tb = 0;
    for (int i = 0; i < nw; ++i) { const int64_t x = wt[0][i], y = wt[1][i]; if (i < w) { ba += x; bb += y; } ta += x; tb += y; }
    ea = ba + ia - a; eb = bb + ib - b;
}

// ---- dedup, workgroup form: graphs of 65..P rows, one workgroup of P / 4 threads a graph ----
__device__ inline bool pair_gt(u32 ax, u32 ay, u32 az, u32 aw, u32 ar, u32 bx, u32 by, u32 bz, u32 bw, u32 br) {
    if (aw != bw) return aw > bw;
    if (az != bz) return az > bz;
    if (ay != by) return ay > by;
    if (ax != bx) return ax > bx;
    return ar > br;
}

template <int P>
__global__ __launch_bounds__(P / 4) void rows_block(UgsRowsCall c, int cls) {
    constexpr int NT = P / 4;
    __shared__ u32 kx[P], ky[P], kz[P], kw[P], kr[P];                  // 20 bytes a pair
    __shared__ int64_t wt[2][16];
    if (!rows_go_all(c)) return;
    const int tid = threadIdx.x;
    const int many = c.nbig[cls];
    for (int idx = blockIdx.x; idx < many; idx += gridDim.x) {
        const int64_t g = c.big[(int64_t)cls * c.G + idx];
        const int64_t r0 = c.sample_ptr[g];
        const int n = (int)(c.sample_ptr[g + 1] - r0);
        if (n <= 64 || n > P) continue;                                // (the list holds no such graph; the same for every thread)
        int pn = 128;
        while (pn < n) pn <<= 1;
        // the pairs, padded to a power of two with a pair no row has: every key bit set and a row number above every row's, so that
        // it sorts behind a row whose key has every bit set too (k = 8 at 16 bits uses all 128)
        for (int p = tid; p < pn; p += NT) {
            uint4 key = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (p < n) key = c.keys[r0 + p];
            kx[p] = key.x; ky[p] = key.y; kz[p] = key.z; kw[p] = key.w; kr[p] = p < n ? (u32)p : ~0u;
        }
        __syncthreads();
        for (int size = 2; size <= pn; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (pn >> 1); t += NT) {
                    const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const bool up = (i & size) == 0;
                    const u32 ax = kx[i], ay = ky[i], az = kz[i], aw = kw[i], ar = kr[i];
                    const u32 bx = kx[j], by = ky[j], bz = kz[j], bw = kw[j], br = kr[j];
                    if (pair_gt(ax, ay, az, aw, ar, bx, by, bz, bw, br) == up) {
                        kx[i] = bx; ky[i] = by; kz[i] = bz; kw[i] = bw; kr[i] = br;
                        kx[j] = ax; ky[j] = ay; kz[j] = az; kw[j] = aw; kr[j] = ar;
                    }
                }
                __syncthreads();
            }
        // positions 0 .. n-1 now hold the rows, by (key, row).  The run of a key: lower and upper bound by binary search; its first
        // pair is the lowest row of the run, the representative.
        u32 my_row[4], my_rep[4], my_cnt[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int p = tid + it * NT;
            my_row[it] = ~0u; my_rep[it] = 0; my_cnt[it] = 0;
            if (p < n) {
                const u32 x = kx[p], y = ky[p], z = kz[p], w = kw[p];
                int lo = 0, hi = p;                                    // first q with key_q >= key: in [0, p]
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (pair_gt(x, y, z, w, 0, kx[mid], ky[mid], kz[mid], kw[mid], 0)) lo = mid + 1; else hi = mid; }
                const int first = lo;
                lo = p + 1; hi = n;                                    // first q with key_q > key: in (p, n]
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (pair_gt(kx[mid], ky[mid], kz[mid], kw[mid], 0, x, y, z, w, 0)) hi = mid; else lo = mid + 1; }
                my_row[it] = kr[p]; my_rep[it] = kr[first]; my_cnt[it] = (u32)(lo - first);
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) if (my_row[it] != ~0u) { kx[my_row[it]] = my_rep[it]; ky[my_row[it]] = my_cnt[it]; }   // by row now (my_row < n)
        __syncthreads();
        // kept flags and kept edge entries scanned in row order: thread t has rows 4t .. 4t+3
        int64_t kc = 0, ke = 0, len[4];
        bool kept[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int lr = 4 * tid + it;
            kept[it] = lr < n && kx[lr] == (u32)lr;
            len[it] = 0;
            if (kept[it]) { len[it] = c.edge_ptr[r0 + lr + 1] - c.edge_ptr[r0 + lr]; ++kc; ke += len[it]; }
        }
        int64_t ec, ee, tc, te;
        block_scan2(kc, ke, NT, wt, ec, ee, tc, te);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int lr = 4 * tid + it;
            if (lr < n) {
                const int64_t r = r0 + lr;
                c.rep[r] = (int32_t)(r0 + kx[lr]);
                if (kept[it]) { c.lrank[r] = (int32_t)ec; c.cnt[r] = (int32_t)ky[lr]; c.eoff[r] = ee; ++ec; ee += len[it]; }
            }
        }
        if (tid == 0) { c.ug[g] = tc; c.eg[g] = te; }
        __syncthreads();                                               // the next graph overwrites the pairs
    }
}

// ---- the scan across graphs, one workgroup; the totals and the status words go where the host reads them ----
__global__ __launch_bounds__(1024) void rows_scan(UgsRowsCall c) {
    __shared__ int64_t wt[2][16];
    const bool go = rows_go_all(c);
    int64_t cu = 0, ce = 0;
    if (go) {
        for (int64_t base = 0; base < c.G; base += 1024) {
            const int64_t g = base + threadIdx.x;
            const int64_t u = g < c.G ? c.ug[g] : 0, e = g < c.G ? c.eg[g] : 0;
            int64_t eu, ee, tu, te;
            block_scan2(u, e, 1024, wt, eu, ee, tu, te);
            if (g < c.G) { c.ubase[g] = cu + eu; c.ebase[g] = ce + ee; }
            cu += tu; ce += te;
        }
    }
    if (threadIdx.x == 0) {
        if (go) { c.ubase[c.G] = cu; c.ebase[c.G] = ce; }
        c.back->U = cu; c.back->Eu = ce;
        for (int i = 0; i < UGS_ROWS_ST_WORDS - 1; ++i) c.back->st[i] = c.status[i];
        c.back->big = (int64_t)c.nbig[0] + c.nbig[1] + c.nbig[2];
        c.back->small = c.nbig[3];
    }
}

// ---- compaction ----
__global__ __launch_bounds__(256) void rows_compact(UgsRowsCall c, UgsRowsOut o, int64_t U, int64_t Eu) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= c.G) o.sample_ptr_u[i] = c.ubase[i];
    if (i == 0) o.edge_ptr_u[U] = Eu;
    if (i >= c.R) return;
    const int64_t g = c.rowg[i];
    const int64_t rp = c.rep[i];
    const int64_t u = c.ubase[g] + c.lrank[rp];
    o.inverse[i] = u;
    if (rp != i) return;
    o.count[u] = c.cnt[i];
    o.edge_ptr_u[u] = c.ebase[g] + c.eoff[i];
    const int64_t *src = c.nodes + i * c.k;
    int64_t *dst = o.nodes_u + u * c.k;
    for (int j = 0; j < c.k; ++j) dst[j] = src[j];
}

__global__ __launch_bounds__(256) void rows_edges(UgsRowsCall c, UgsRowsOut o) {
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int lane = threadIdx.x & 15;
    if (r >= c.R || c.rep[r] != r) return;
    const int64_t from = c.edge_ptr[r], len = c.edge_ptr[r + 1] - from;
    const int64_t to = c.ebase[c.rowg[r]] + c.eoff[r];
    for (int64_t e = lane; e < len; e += 16) {
        o.edge_index_u[to + e] = o.edge_index_in[from + e];
        o.edge_index_u[o.ld + to + e] = o.edge_index_in[o.in_stride + from + e];
        if (o.edge_src_u) o.edge_src_u[to + e] = o.edge_src_in[from + e];
    }
}

template <int K>
void launch_keys(const UgsRowsCall &c, hipStream_t s) {
    hipLaunchKernelGGL(rows_keys<K>, dim3((unsigned)((c.R + 255) / 256)), dim3(256), 0, s, c);
}

}  // namespace

hipError_t ugs_rows_dedup(const UgsRowsCall &c, hipStream_t s) {
    hipError_t e = hipMemsetAsync(c.status, 0x7f, UGS_ROWS_ST_WORDS * sizeof(int64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(c.nbig, 0, 4 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    const int64_t top = (c.R > c.G ? c.R : c.G) + 1;
    hipLaunchKernelGGL(rows_check, dim3((unsigned)std::min<int64_t>((top + 255) / 256, 4096)), dim3(256), 0, s, c);
    if (c.R > 0) {
        switch (c.k) {
        case 1: launch_keys<1>(c, s); break;
        case 2: launch_keys<2>(c, s); break;
        case 3: launch_keys<3>(c, s); break;
        case 4: launch_keys<4>(c, s); break;
        case 5: launch_keys<5>(c, s); break;
        case 6: launch_keys<6>(c, s); break;
        case 7: launch_keys<7>(c, s); break;
        case 8: launch_keys<8>(c, s); break;
        default: launch_keys<0>(c, s); break;
        }
    }
    if (c.G > 0) hipLaunchKernelGGL(rows_wave, dim3((unsigned)((c.G + 3) / 4)), dim3(256), 0, s, c);
    // the workgroup form, by padded size: a class of graphs of more than `least` rows has at most R / least members
    const int64_t g0 = std::min<int64_t>(c.G, c.R / 65), g1 = std::min<int64_t>(c.G, c.R / 257), g2 = std::min<int64_t>(c.G, c.R / 1025);
    if (g0 > 0) hipLaunchKernelGGL(rows_block<256>, dim3((unsigned)g0), dim3(64), 0, s, c, 0);
    if (g1 > 0) hipLaunchKernelGGL(rows_block<1024>, dim3((unsigned)g1), dim3(256), 0, s, c, 1);
    if (g2 > 0) hipLaunchKernelGGL(rows_block<4096>, dim3((unsigned)g2), dim3(1024), 0, s, c, 2);
    hipLaunchKernelGGL(rows_scan, dim3(1), dim3(1024), 0, s, c);
    return hipGetLastError();
}

hipError_t ugs_rows_compact(const UgsRowsCall &c, const UgsRowsOut &o, int64_t U, int64_t Eu, hipStream_t s) {
    const int64_t top = std::max<int64_t>(c.R, c.G + 1);
    hipLaunchKernelGGL(rows_compact, dim3((unsigned)((top + 255) / 256)), dim3(256), 0, s, c, o, U, Eu);
    if (Eu > 0 && c.R > 0) hipLaunchKernelGGL(rows_edges, dim3((unsigned)((c.R * 16 + 255) / 256)), dim3(256), 0, s, c, o);
    return hipGetLastError();
}
