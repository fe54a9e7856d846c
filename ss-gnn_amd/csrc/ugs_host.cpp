// ugs_host.cpp -- host side of libugs_mi355.so: graph preprocessing, handle registry, the batch LRU, device plans and
// the C ABI of include/ugs_mi355.h.  Sampling itself runs only in the gfx950 kernels of ugs_kernels.hip; there is no
// CPU sampling path in this library.
//
// Behavioural contract (what must come out bit-identical): the reference `ugs_sampler`
// (AniruddhaMandal/SS-GNN src/samplers/ugs_sampler): preprocessing src/preproc.cpp:32-256 + include/sampler.hpp:39-69,
// handle registry src/preproc.cpp:262-314, LRU + graph hash include/cache.hpp:15-109, batch wrapper
// src/ugs_sampler_batch_extension.cpp:41-299.  The data structures here are flat arrays laid out for the GPU
// (see ugs_device.h), not the reference's.
#include "../../include/ugs_mi355.h"
#include "ugs_device.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <chrono>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <thread>
#include <vector>

struct ugs_plan;
namespace { void plan_unref(ugs_plan *p); void arena_release(int dev, int64_t roots_off, int64_t n_roots, int64_t via_off, int64_t n_via); void pin_slot_put(char *p); }

namespace {

thread_local std::string t_err;
int fail(int code, const std::string &msg) { t_err = msg; return code; }
}  // namespace
// the other translation units of the library report through the same thread-local message (ugs_device.h)
int ugs_internal_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
namespace {
int fail_hip(hipError_t e, const char *what) { return fail(UGS_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail_hip(e_, #expr); } while (0)

struct Lap {   // UGS_DEBUG=1: wall-clock of the host stages of a large preprocessing / plan build
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double operator()() { auto n = std::chrono::steady_clock::now(); double d = std::chrono::duration<double>(n - t).count(); t = n; return d; }
};

bool debug_on() { static const bool on = [] { const char *e = std::getenv("UGS_DEBUG"); return e && std::string(e) == "1"; }(); return on; }
bool env_is_one(const char *name) { const char *e = std::getenv(name); return e && e[0] == '1'; }     // read at every call: tests and A/Bs toggle these

// ---------------------------------------------------------------------------------------------------------------
// per-graph preprocessing result (host copy; the device plan is assembled from these)
// ---------------------------------------------------------------------------------------------------------------
struct Graph {
    int64_t n = 0, nnz = 0;
    int k_built = 0;
    std::vector<int64_t> rowptr;      // n+1, 0-based
    std::vector<int32_t> nbr, col;    // CSR neighbours and source column of each entry
    std::vector<int32_t> order, rank; // order[vi] = vertex, rank[vertex] = vi
    std::vector<int32_t> sdeg;        // suffix degree per order position
    std::vector<uint8_t> reach;       // scratch: root reaches k vertices inside its suffix graph
    std::vector<double> weight;       // bucket weight per order position
    std::vector<double> prob;         // alias table (only if Z > 0)
    std::vector<int32_t> alias;
    double Z = 0.0;
    int nonzero = 0;
    int level = 0;                    // relaxation level of the root draw
    std::vector<int32_t> viable;      // order positions for levels 1, 2
    int64_t n_viable = 0;             // their number (a graph preprocessed by the device batch pass has only this)
    // A graph the device batch pass preprocessed (cold path, ugs_bp_roots) exists on the host as a STUB: n, nnz, level, Z, the degree
    // statistics and its root records in a device's arena -- no arrays.  The general path, which has the graph's columns at hand
    // whenever it meets the graph, fills the arrays in then (complete_on_host).
    bool host_ready = true;
    std::vector<int64_t> stub_cols;   // stub: its span of the batch's columns, sources then targets (global ids), and
    int64_t stub_lo = 0;              //       the batch's node offset of the graph -- what completion needs, dropped afterwards
    int64_t max_deg = 0;
    double sb_deg = 0.0;              // size-biased mean CSR degree (sum d^2 / sum d)
    // content fingerprint (graph_fingerprint), set only for graphs of more than 1000 columns: there the LRU key samples the
    // columns, and the device batch pass accepts a cached graph as the one it has just built only if this agrees too
    uint64_t fp_a = 0, fp_b = 0;
    std::mutex plan_mu;
    ugs_plan *plan = nullptr;         // device-resident copy for the handle API, built on first sample()
    std::mutex pre_mu;
    UgsDevPre *devpre = nullptr;      // device CSR left by preprocess_on_device for the FIRST plan assembled from this graph
    int devpre_dev = -1;
    UgsDevPre *take_devpre(int dev) { std::lock_guard<std::mutex> lk(pre_mu); if (!devpre || devpre_dev != dev) return nullptr; UgsDevPre *d = devpre; devpre = nullptr; return d; }
    // root records / viable list of this graph resident in a device's arena (device batch pass: plans of new combinations of
    // known graphs point at them instead of copying them); offsets in elements, -1 = none
    struct DevRoots { int dev; int64_t roots_off, n_roots, via_off, n_via; };
    std::vector<DevRoots> dev_roots;
    ~Graph() {
        if (plan) plan_unref(plan);
        if (devpre) ugs_devpre_free(devpre);
        for (auto &d : dev_roots) arena_release(d.dev, d.roots_off, d.n_roots, d.via_off, d.n_via);
    }
};

// CSR of the symmetrised multigraph, entries in column order (both endpoints of column j, u's row first).
void build_adjacency(Graph &G, const int64_t *src, const int64_t *dst, int64_t E) {
    const int64_t n = G.n;
    G.rowptr.assign((size_t)n + 1, 0);
    for (int64_t j = 0; j < E; ++j) {
        const int64_t u = src[j], v = dst[j];
        if ((uint64_t)u >= (uint64_t)n || (uint64_t)v >= (uint64_t)n) continue;     // silently skipped columns
        ++G.rowptr[(size_t)u + 1];
        ++G.rowptr[(size_t)v + 1];
    }
    for (int64_t r = 0; r < n; ++r) G.rowptr[(size_t)r + 1] += G.rowptr[(size_t)r];
    G.nnz = G.rowptr[(size_t)n];
    G.nbr.resize((size_t)G.nnz);
    G.col.resize((size_t)G.nnz);
    std::vector<int64_t> wr(G.rowptr.begin(), G.rowptr.end() - 1);
    for (int64_t j = 0; j < E; ++j) {
        const int64_t u = src[j], v = dst[j];
        if ((uint64_t)u >= (uint64_t)n || (uint64_t)v >= (uint64_t)n) continue;
        int64_t a = wr[(size_t)u]++;
        G.nbr[(size_t)a] = (int32_t)v; G.col[(size_t)a] = (int32_t)j;
        int64_t b = wr[(size_t)v]++;
        G.nbr[(size_t)b] = (int32_t)u; G.col[(size_t)b] = (int32_t)j;
    }
}

// The reference's "remove the max-degree vertex, then reverse" ordering is the stable ascending sort by
// (CSR degree, vertex id): every vertex is popped from the bucket of its ORIGINAL degree (later, lower-degree
// duplicates are stale when reached), buckets drain high to low and back-to-front.  One counting sort.
void order_by_degree(Graph &G) {
    const int64_t n = G.n;
    G.order.resize((size_t)n);
    G.rank.resize((size_t)n);
    int64_t maxd = 0;
    double s1 = 0, s2 = 0;
    for (int64_t v = 0; v < n; ++v) {
        int64_t d = G.rowptr[(size_t)v + 1] - G.rowptr[(size_t)v];
        maxd = std::max(maxd, d);
        s1 += (double)d; s2 += (double)d * (double)d;
    }
    G.max_deg = maxd;
    G.sb_deg = s1 > 0 ? s2 / s1 : 0.0;
    std::vector<int64_t> start((size_t)maxd + 2, 0);
    for (int64_t v = 0; v < n; ++v) ++start[(size_t)(G.rowptr[(size_t)v + 1] - G.rowptr[(size_t)v]) + 1];
    for (int64_t d = 0; d <= maxd; ++d) start[(size_t)d + 1] += start[(size_t)d];
    for (int64_t v = 0; v < n; ++v) {
        int64_t d = G.rowptr[(size_t)v + 1] - G.rowptr[(size_t)v];
        int64_t pos = start[(size_t)d]++;
        G.order[(size_t)pos] = (int32_t)v;
        G.rank[(size_t)v] = (int32_t)pos;
    }
}

// Vose alias table, stacks filled in ascending index; order-sensitive IEEE arithmetic kept exactly
// (p = w*n/sum; p[l] = (p[l] + p[s]) - 1.0).
void build_alias(Graph &G) {
    const int n = (int)G.n;
    G.prob.assign((size_t)n, 0.0);
    G.alias.assign((size_t)n, 0);
    if (n == 0) return;
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += G.weight[(size_t)i];
    const double denom = total > 0 ? total : 1.0;
    std::vector<double> p((size_t)n);
    std::vector<int32_t> lo, hi;
    lo.reserve((size_t)n); hi.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        p[(size_t)i] = G.weight[(size_t)i] * n / denom;
        (p[(size_t)i] < 1.0 ? lo : hi).push_back(i);
    }
    while (!lo.empty() && !hi.empty()) {
        const int32_t s = lo.back(); lo.pop_back();
        const int32_t l = hi.back();
        G.prob[(size_t)s] = p[(size_t)s];
        G.alias[(size_t)s] = l;
        p[(size_t)l] = (p[(size_t)l] + p[(size_t)s]) - 1.0;
        if (p[(size_t)l] < 1.0) { hi.pop_back(); lo.push_back(l); }
    }
    for (int32_t i : hi) G.prob[(size_t)i] = 1.0;
    for (int32_t i : lo) G.prob[(size_t)i] = 1.0;
}

// suffix degrees and k-reachability of every root inside its suffix graph (host form; ugs_preproc.hip is the device form)
void root_stats_host(Graph &G, int k) {
    const int n = (int)G.n;
    G.sdeg.assign((size_t)n, 0);
    for (int vi = 0; vi < n; ++vi) {
        const int32_t v = G.order[(size_t)vi];
        int32_t c = 0;
        for (int64_t p = G.rowptr[(size_t)v]; p < G.rowptr[(size_t)v + 1]; ++p) c += G.rank[(size_t)G.nbr[(size_t)p]] >= vi;
        G.sdeg[(size_t)vi] = c;
    }
    G.reach.assign((size_t)n, 0);
    std::vector<int32_t> mark((size_t)n, -1), reached;
    reached.reserve((size_t)std::max(k, 1) + 1);
    for (int vi = 0; vi < n; ++vi) {
        reached.clear();
        reached.push_back(G.order[(size_t)vi]);
        mark[(size_t)reached[0]] = vi;
        for (size_t h = 0; h < reached.size() && (int)reached.size() < k; ++h) {
            const int32_t u = reached[h];
            for (int64_t p = G.rowptr[(size_t)u]; p < G.rowptr[(size_t)u + 1] && (int)reached.size() < k; ++p) {
                const int32_t w = G.nbr[(size_t)p];
                if (G.rank[(size_t)w] < vi || mark[(size_t)w] == vi) continue;
                mark[(size_t)w] = vi;
                reached.push_back(w);
            }
        }
        G.reach[(size_t)vi] = (int)reached.size() >= k;
    }
}

// bucket weights d^(k-1), Z (summed in order position order: the floating-point result depends on it), alias table
void weigh_roots(Graph &G, int k) {
    const int n = (int)G.n;
    G.weight.assign((size_t)n, 0.0);
    G.Z = 0.0;
    G.nonzero = 0;
    for (int vi = 0; vi < n; ++vi) {
        if (G.reach[(size_t)vi]) {
            const double d = (double)std::max<int32_t>(1, G.sdeg[(size_t)vi]);
            double b = 1.0;
            for (int t = 1; t < k; ++t) b *= d;
            G.weight[(size_t)vi] = b;
            G.Z += b;
            if (b > 0.0) ++G.nonzero;
        }
    }
    std::vector<uint8_t>().swap(G.reach);
    if (G.Z > 0.0) build_alias(G); else { G.prob.assign((size_t)n, 0.0); G.alias.assign((size_t)n, 0); }
    // relaxation levels of the root draw
    G.viable.clear();
    if (G.nonzero > 0) G.level = 0;
    else {
        G.level = 1;
        for (int vi = 0; vi < n; ++vi) if (G.sdeg[(size_t)vi] > 0) G.viable.push_back(vi);
        if (G.viable.empty()) { G.level = 2; for (int vi = 0; vi < n; ++vi) G.viable.push_back(vi); }
    }
    G.n_viable = (int64_t)G.viable.size();
    if (debug_on()) std::fprintf(stderr, "[UGS PREPROC] n=%d k=%d Z=%.2e viable=%d/%d\n", n, k, G.Z, G.nonzero, n);
}

// arrays of a stub (see Graph::host_ready) from the graph's columns, with the k it was preprocessed for: the same values the
// device computed (both equal the reference's), now on the host as well
void complete_on_host(Graph &G) {
    std::lock_guard<std::mutex> lk(G.pre_mu);
    if (G.host_ready) return;
    const size_t span = G.stub_cols.size() / 2;
    std::vector<int64_t> ru, rv;
    ru.reserve(span); rv.reserve(span);
    for (size_t j = 0; j < span; ++j) {                                  // the graph's columns: both endpoints inside its node range
        const int64_t u = G.stub_cols[j] - G.stub_lo, v = G.stub_cols[span + j] - G.stub_lo;
        if ((uint64_t)u < (uint64_t)G.n && (uint64_t)v < (uint64_t)G.n) { ru.push_back(u); rv.push_back(v); }
    }
    build_adjacency(G, ru.data(), rv.data(), (int64_t)ru.size());
    order_by_degree(G);
    root_stats_host(G, G.k_built);
    weigh_roots(G, G.k_built);
    std::vector<int64_t>().swap(G.stub_cols);
    G.host_ready = true;
}

// What the large form of ugs_bp_build computes for a graph of more than 1000 columns (ugs_device.h: ugs_fp_add), in plain C++:
// covers n, the number of columns and every renumbered column with its position.
void graph_fingerprint(const int64_t *u, const int64_t *v, int64_t cols, int64_t n, uint64_t &fa, uint64_t &fb) {
    unsigned long long a, b;
    ugs_fp_seed((unsigned long long)n, (unsigned long long)cols, a, b);
    for (int64_t t = 0; t < cols; ++t) ugs_fp_add((unsigned long long)t, (unsigned long long)u[t], (unsigned long long)v[t], a, b);
    fa = a; fb = b;
}

int preprocess_on_device(Graph &G, const int64_t *src, const int64_t *dst, int64_t E, int k, bool &done);   // below, after the device helpers

// which path preprocessed / assembled what (ugs_preproc_stats): graphs through ugs_preproc.hip, graphs through the host stages of
// make_graph, plan pieces handed to ugs_devpre_assemble
std::atomic<int64_t> g_pre_device_graphs{0}, g_pre_host_graphs{0}, g_pre_device_pieces{0};

int make_graph(const int64_t *src, const int64_t *dst, int64_t E, int64_t n, int k, std::shared_ptr<Graph> &out) {
    if (n < 0) return fail(UGS_E_BAD_ARG, "num_nodes must be >= 0");
    if (n >= ((int64_t)1 << 30) - 1 || E >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "graph too large: num_nodes must be < 2^30 - 1 and columns < 2^31 - 1");
    auto G = std::make_shared<Graph>();
    G->n = n;
    G->k_built = k;
    if (E > UGS_BATCH_PASS_MAX_COLS) graph_fingerprint(src, dst, E, n, G->fp_a, G->fp_b);
    bool on_device = false;
    if (int rc = preprocess_on_device(*G, src, dst, E, k, on_device)) return rc;
    if (!on_device) {
        Lap lap;
        g_pre_host_graphs.fetch_add(1);
        build_adjacency(*G, src, dst, E);
        if (G->nnz >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "graph too large: CSR entries must be < 2^31 - 1");
        const double t_csr = lap();
        order_by_degree(*G);
        const double t_order = lap();
        root_stats_host(*G, k);
        if (debug_on() && E >= ((int64_t)1 << 21))
            std::fprintf(stderr, "[UGS PREPROC] n=%lld columns=%lld on the host: CSR %.3fs, degree order %.3fs, suffix degrees+reachability %.3fs\n",
                         (long long)n, (long long)E, t_csr, t_order, lap());
    }
    Lap lap;
    weigh_roots(*G, k);
    if (debug_on() && E >= ((int64_t)1 << 21)) std::fprintf(stderr, "[UGS PREPROC] weights, Z, alias table (host) %.3fs\n", lap());
    out = std::move(G);
    return UGS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// handle registry (monotonically increasing int64 handles from 1)
// ---------------------------------------------------------------------------------------------------------------
// The process-wide containers below are heap objects that are never destroyed: at process exit no destructor of this library
// runs (a Graph's destructor releases device plans into the scratch pool and calls the HIP runtime, neither of which may
// still exist during static destruction).
std::mutex g_reg_mu;
std::unordered_map<int64_t, std::shared_ptr<Graph>> &g_reg = *new std::unordered_map<int64_t, std::shared_ptr<Graph>>();
int64_t g_next_handle = 1;

std::shared_ptr<Graph> lookup(int64_t h) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_reg.find(h);
    return it == g_reg.end() ? nullptr : it->second;
}
int64_t enroll(std::shared_ptr<Graph> g) {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    int64_t h = g_next_handle++;
    g_reg[h] = std::move(g);
    return h;
}
void drop(int64_t h) { std::lock_guard<std::mutex> lk(g_reg_mu); g_reg.erase(h); }

// ---------------------------------------------------------------------------------------------------------------
// batch LRU: graph hash -> handle.  Capacity from UGS_CACHE_SIZE (default 1000); capacity 0 never evicts.
// The key deliberately matches the reference's (FNV-1a over n, #cols and (strided) renumbered columns, NOT k), so
// that the same call history produces the same reuse -- including reuse of weights built for another k.
// ---------------------------------------------------------------------------------------------------------------
struct Lru {
    size_t capacity = 1000;
    std::list<std::pair<uint64_t, int64_t>> items;     // front = most recent
    std::unordered_map<uint64_t, std::list<std::pair<uint64_t, int64_t>>::iterator> index;
    int64_t hits = 0, misses = 0;
    bool get(uint64_t key, int64_t &val) {
        auto it = index.find(key);
        if (it == index.end()) return false;
        items.splice(items.begin(), items, it->second);
        val = it->second->second;
        return true;
    }
    bool put(uint64_t key, int64_t val, int64_t &evicted) {   // true if something was evicted
        auto it = index.find(key);
        if (it != index.end()) { it->second->second = val; items.splice(items.begin(), items, it->second); return false; }
        bool ev = false;
        if (capacity > 0 && items.size() >= capacity) {
            evicted = items.back().second;
            index.erase(items.back().first);
            items.pop_back();
            ev = true;
        }
        items.emplace_front(key, val);
        index[key] = items.begin();
        return ev;
    }
    void erase(uint64_t key) {
        auto it = index.find(key);
        if (it == index.end()) return;
        items.erase(it->second);
        index.erase(it);
    }
};
std::mutex g_lru_mu;
Lru *g_lru = nullptr;
Lru &lru() {   // call with g_lru_mu held
    if (!g_lru) {
        g_lru = new Lru();
        if (const char *e = std::getenv("UGS_CACHE_SIZE")) g_lru->capacity = (size_t)std::atoi(e);
        if (debug_on()) std::fprintf(stderr, "[UGS INFO] Preprocessing cache initialized: size=%zu (set UGS_CACHE_SIZE to change)\n", g_lru->capacity);
    }
    return *g_lru;
}

uint64_t graph_key(const int64_t *u, const int64_t *v, int64_t cols, int64_t n) {
    const uint64_t prime = 1099511628211ull;
    uint64_t h = 14695981039346656037ull;
    h = (h ^ (uint64_t)n) * prime;
    h = (h ^ (uint64_t)cols) * prime;
    const int64_t step = cols > 1000 ? cols / 500 : 1;
    for (int64_t j = 0; j < cols; j += step) { h = (h ^ (uint64_t)u[j]) * prime; h = (h ^ (uint64_t)v[j]) * prime; }
    return h;
}

// ---------------------------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------------------------
struct DeviceCtx { int id = -1; int cus = 256; hipStream_t stream = nullptr; };
std::mutex g_dev_mu;
std::map<int, DeviceCtx> &g_devs = *new std::map<int, DeviceCtx>();
thread_local int t_device = -1;
thread_local hipStream_t t_job_stream = nullptr;    // ugs_set_stream: stream of the calling thread's jobs (NULL: the library's own)
thread_local bool t_job_stream_set = false;

int device_ctx(DeviceCtx &out) {
    int dev = t_device;
    if (dev < 0) {
        int cnt = 0;
        hipError_t e = hipGetDeviceCount(&cnt);
        if (e != hipSuccess || cnt <= 0) return fail(UGS_E_NO_DEVICE, "no usable HIP device: this sampler has no CPU path (hipGetDeviceCount: " + std::string(hipGetErrorString(e)) + ")");
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    HIP_TRY(hipSetDevice(dev));
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = g_devs.find(dev);
    if (it == g_devs.end()) {
        DeviceCtx c;
        c.id = dev;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) c.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        it = g_devs.emplace(dev, c).first;
    }
    out = it->second;
    if (t_job_stream_set) out.stream = t_job_stream;
    return UGS_OK;
}

}  // namespace
int ugs_internal_ctx(int *device, hipStream_t *stream) {
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (device) *device = dc.id;
    if (stream) *stream = dc.stream;
    return UGS_OK;
}
namespace {

// grow-only device scratch pool (per process): avoids hipMalloc/hipFree on every call
struct PoolBuf { void *p = nullptr; size_t bytes = 0; int dev = -1; bool owned = true; /* false: a piece of a slab, never hipFree'd on its own */ };
std::mutex g_pool_mu;
std::vector<PoolBuf> &g_pool_free = *new std::vector<PoolBuf>();
int pool_get(size_t bytes, int dev, PoolBuf &out) {
    if (bytes < 256) bytes = 256;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        int best = -1;
        for (int i = 0; i < (int)g_pool_free.size(); ++i)
            if (g_pool_free[(size_t)i].dev == dev && g_pool_free[(size_t)i].bytes >= bytes &&
                (best < 0 || g_pool_free[(size_t)i].bytes < g_pool_free[(size_t)best].bytes)) best = i;
        if (best >= 0 && g_pool_free[(size_t)best].bytes <= 4 * bytes + (1u << 20)) {
            out = g_pool_free[(size_t)best];
            g_pool_free.erase(g_pool_free.begin() + best);
            return UGS_OK;
        }
    }
    // Small requests (the plan of a mini-batch, per-call scratch) come in a slab of 16 one-megabyte pieces: a fresh hipMalloc per new plan
    // costs tens of microseconds -- up to 0.1 ms with a multi-gigabyte plan resident -- and the plan cache hands buffers back only once
    // its 64 slots are full, so without this the first 64 new mini-batches of a process each pay it.
    if (bytes <= ((size_t)1 << 20)) {
        const size_t piece = bytes <= ((size_t)64 << 10) ? (size_t)64 << 10 : (size_t)1 << 20;    // two classes: counters and lists / plans
        const int n = piece == ((size_t)1 << 20) ? 16 : 64;
        void *slab = nullptr;
        if (hipMalloc(&slab, (size_t)n * piece) == hipSuccess) {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            for (int i = 1; i < n; ++i) g_pool_free.push_back(PoolBuf{static_cast<char *>(slab) + (size_t)i * piece, piece, dev, false});
            out.p = slab; out.bytes = piece; out.dev = dev; out.owned = false;       // (the slab itself is never freed: 4 or 16 MB)
            return UGS_OK;
        }
        (void)hipGetLastError();
    }
    size_t rounded = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, rounded);
    if (e != hipSuccess) {   // drop the pool and retry once
        std::vector<PoolBuf> victims;
        { std::lock_guard<std::mutex> lk(g_pool_mu); victims.swap(g_pool_free); }
        for (auto &b : victims) if (b.owned) (void)hipFree(b.p);      // (pieces of a slab are dropped, their slab stays)
        e = hipMalloc(&p, rounded);
        if (e != hipSuccess) return fail_hip(e, "hipMalloc");
    }
    out.p = p; out.bytes = rounded; out.dev = dev; out.owned = true;
    return UGS_OK;
}
void pool_put(PoolBuf &b) {
    if (!b.p) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_free.push_back(b);
    b = PoolBuf();
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------------------------------------------
struct TierChoice { int first = UGS_TIER_S; int second = -1 /* LDS tier that redoes the rows the first one hands on */; bool third_G = false; int64_t bound = 0;
                    bool small = false /* tier S in its 32-candidate form */; bool wide = false /* tier S may run with 16 lanes per walk */; };

struct ugs_plan {
    int device = -1, cus = 256;
    int64_t G = 0, nverts = 0, nnz = 0;
    void *blob = nullptr;                 // one device allocation holding every array of the plan
    size_t blob_bytes = 0;
    PoolBuf blob_buf;                     // small plans borrow their allocation from the scratch pool
    UgsPlanDev dev{};
    // per-graph statistics used to pick the walk tier for a given k
    std::vector<int64_t> g_n, g_maxdeg;
    std::vector<double> g_sbdeg;
    std::vector<int> g_level;
    std::mutex mu;
    std::map<int, TierChoice> tiers;
    std::atomic<int> refs{1};
    uint64_t cache_key = 0;
    bool cached = false;
    // lazily grown scratch owned by the plan (serialised by `mu` per call)
    // invariant: what a walk leaves here is read only by kernels launched under the same hold of `mu`, or after the stg_* check below
    PoolBuf counts, ovf1, ovf2, ovfcnt, scantmp, gws;
    // edges staged by the last walk (UgsWalkArgs::stage) and the call they belong to: a fill of exactly those rows into/from
    // the same nodes buffer expands them; any other fill reads the adjacency rows again
    PoolBuf stage, ulist, work;   // work: 3 x u64 next-item counters (one per walk launch of a call)
    // scan folded into the fill (ugs_plan_step, ugs_fill_scan): the walk kernel's sums of 8 consecutive rows
    PoolBuf tiles;
    // job path: the scan kernel hands the edge total to the host through 16 bytes of pinned memory (total, epoch word) and the host
    // polls the word instead of copying the total back behind a stream wait (wait_signal)
    char *pin_slot = nullptr;
    uint32_t pin_epoch = 0;
    // stream order between calls: a plan's scratch is reused by every call, so a call on another stream than the previous one
    // first waits (on the device) for that call's last kernel
    hipEvent_t last_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
    PoolBuf prow;                         // padded rows (ugs_device.h), built on the device by the first walk in a one-walk-per-wave tier
    std::atomic<size_t> prow_bytes{0};    // their size, readable by the plan cache without this plan's mutex
    bool prow_pooled = false, prow_failed = false;
    size_t prow_asked = 0;                // bytes asked for (rows + table): what ugs_plan_info reports, as blob_bytes is the bytes asked for
    const uint8_t *ord1 = nullptr;        // first-pick table (UgsWalkArgs::ord1): the tail of the padded rows' allocation, 64 bytes per vertex
    int walk_share = 100;                 // ugs_plan_set_walk_share
    bool stg_valid = false;
    const void *stg_nodes = nullptr;
    int64_t stg_row_begin = 0, stg_row_count = 0;
    int stg_m = 0, stg_k = 0;
    int64_t gws_groups = 0, gws_words = 0;
    int gcap = 0, ghs = 0, gbcap = 0, gpcap = 0;
    std::vector<std::shared_ptr<void>> keep;   // device-built plans point into their graphs' arena entries: the graphs live as long as the plan
    ugs_plan *twin_of = nullptr;               // ugs_plan_twin: the plan whose device arrays this one shares (it holds a reference)
    UgsLaunchInfo last_walk{nullptr, 0, 0, 0};
    UgsLaunchInfo last_fill{nullptr, 0, 0, 0};
    int64_t last_overflow = 0;
    bool handle_api = false;
    // optional per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline figure)
    bool timing = false;
    struct EvPair { hipEvent_t a, b; int kind; };     // kind 0 = first-tier walk kernel, 1 = overflow tiers + scan, 2 = fill kernel
    std::vector<EvPair> events;
};

namespace {

struct PlanPiece {                 // one graph of a plan
    std::shared_ptr<Graph> g;      // null for degenerate graphs
    int64_t lo = 0;
    const int64_t *colmap = nullptr;   // batch column of each of the graph's columns (null: identity)
    int64_t ncols = 0;                 // entries of colmap
};

size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Large graphs: the O(nnz) preprocessing stages on the GPU (ugs_preproc.hip).  The degree order stays on
// the host (O(n)); the outcome is bit-identical to the host path.  UGS_DEVICE_PREPROC=0 never, =1 always (testing aid);
// by default graphs with >= 2^21 columns when a device is present and has room.  `done` = false -> caller runs the host path.
int preprocess_on_device(Graph &G, const int64_t *src, const int64_t *dst, int64_t E, int k, bool &done) {
    done = false;
    const char *env = std::getenv("UGS_DEVICE_PREPROC");
    if (env && env[0] == '0') return UGS_OK;
    const bool forced = env && env[0] == '1';
    if (G.n < 1 || E < 1 || E >= ((int64_t)1 << 30)) return UGS_OK;
    if (k > UGS_KMAX) return UGS_OK;       // pre_roots keeps the <= k reached vertices in UGS_KMAX private slots; the host form has no bound on k
    if (!forced && E < ((int64_t)1 << 21)) return UGS_OK;
    DeviceCtx dc;
    {
        const std::string keep = t_err;
        if (device_ctx(dc) != UGS_OK) { t_err = keep; return UGS_OK; }       // no device: create_preproc still works on the host
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || ugs_devpre_bytes(G.n, E) > free_b / 2) return UGS_OK;
    UgsDevPre *d = nullptr;
    struct Guard { UgsDevPre *&d; ~Guard() { ugs_devpre_free(d); } } guard{d};
    Lap lap;
    G.rowptr.assign((size_t)G.n + 1, 0);
    HIP_TRY(ugs_devpre_csr(&d, src, dst, E, G.n, dc.stream, G.rowptr.data(), &G.nnz));
    if (G.nnz >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "graph too large: CSR entries must be < 2^31 - 1");
    const double t_csr = lap();
    order_by_degree(G);
    const double t_order = lap();
    G.sdeg.assign((size_t)G.n, 0);
    G.reach.assign((size_t)G.n, 0);
    HIP_TRY(ugs_devpre_roots(d, G.order.data(), G.rank.data(), k, G.sdeg.data(), G.reach.data()));
    const double t_roots = lap();
    G.nbr.resize((size_t)G.nnz);
    G.col.resize((size_t)G.nnz);
    HIP_TRY(ugs_devpre_download(d, G.nbr.data(), G.col.data()));
    if (debug_on())
        std::fprintf(stderr, "[UGS PREPROC] n=%lld columns=%lld on the device: upload+CSR %.3fs, degree order (host) %.3fs, suffix degrees+reachability %.3fs, "
                     "CSR download %.3fs\n", (long long)G.n, (long long)E, t_csr, t_order, t_roots, lap());
    ugs_devpre_trim(d);
    { std::lock_guard<std::mutex> lk(G.pre_mu); G.devpre = d; G.devpre_dev = dc.id; d = nullptr; }
    g_pre_device_graphs.fetch_add(1);
    done = true;
    return UGS_OK;
}

int assemble_plan(const std::vector<PlanPiece> &pieces, const DeviceCtx &dc, ugs_plan *plan) {
    const int64_t G = (int64_t)pieces.size();
    int64_t nv = 0, nnz = 0, nrows = 0, nviable = 0;
    for (auto &pc : pieces) if (pc.g) { nv += pc.g->n; nnz += pc.g->nnz; nrows += pc.g->n + 1; if (pc.g->level > 0) nviable += (int64_t)pc.g->viable.size(); }
    if (nnz >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "plan too large: total CSR entries must be < 2^31 - 1");
    size_t off_desc = 0;
    size_t off_row = align_up(off_desc + (size_t)std::max<int64_t>(G, 1) * sizeof(UgsGraphDesc));
    size_t off_adj = align_up(off_row + (size_t)std::max<int64_t>(nrows, 1) * sizeof(int64_t));
    size_t off_col = align_up(off_adj + (size_t)std::max<int64_t>(nnz, 1) * sizeof(int2));
    size_t off_root = align_up(off_col + (size_t)std::max<int64_t>(nnz, 1) * sizeof(int2));
    size_t off_via = align_up(off_root + (size_t)std::max<int64_t>(nv, 1) * sizeof(UgsRootRec));
    size_t total = align_up(off_via + (size_t)std::max<int64_t>(nviable, 1) * sizeof(int2));
    // Graphs preprocessed on this device still hold their CSR in HBM (Graph::devpre): their adjacency arrays are written by
    // a kernel and never cross the bus.  Without such a piece (every batch of small graphs) the plan is ONE host blob, one copy.
    std::vector<UgsDevPre *> dpre((size_t)G, nullptr);
    bool split = false;
    for (int64_t gi = 0; gi < G; ++gi)
        if (pieces[(size_t)gi].g && (dpre[(size_t)gi] = pieces[(size_t)gi].g->take_devpre(dc.id))) split = true;
    struct Owned { std::vector<UgsDevPre *> &v; ~Owned() { for (auto *d : v) ugs_devpre_free(d); } } owned{dpre};
    std::vector<char> host(split ? off_adj : total, 0);           // split: head = descriptors + row pointer
    std::vector<char> tail(split ? total - off_root : 0, 0);      // split: tail = root records + viable lists
    auto *desc = reinterpret_cast<UgsGraphDesc *>(host.data() + off_desc);
    auto *rowp = reinterpret_cast<int64_t *>(host.data() + off_row);
    auto *adj = split ? nullptr : reinterpret_cast<int2 *>(host.data() + off_adj);
    auto *adjf = split ? nullptr : reinterpret_cast<int2 *>(host.data() + off_col);
    char *tail_base = split ? tail.data() - off_root : host.data();
    auto *roots = reinterpret_cast<UgsRootRec *>(tail_base + off_root);
    auto *via = reinterpret_cast<int2 *>(tail_base + off_via);
    void *dptr = nullptr;
    if (total <= ((size_t)64 << 20)) {      // batches of small graphs come and go with every shuffled mini-batch: pooled
        if (int rc = pool_get(total, dc.id, plan->blob_buf)) return rc;
        dptr = plan->blob_buf.p;
    } else {
        HIP_TRY(hipMalloc(&dptr, total));
    }
    auto give_back = [&] { if (plan->blob_buf.p) { pool_put(plan->blob_buf); plan->blob_buf = PoolBuf(); } else (void)hipFree(dptr); };
    char *base = static_cast<char *>(dptr);
    auto fill_adj = [](const PlanPiece &pc, int2 *a, int2 *af) {
        const Graph &g = *pc.g;
        for (int64_t p = 0; p < g.nnz; ++p) {
            const int32_t w = g.nbr[(size_t)p];
            a[p] = make_int2(w, g.rank[(size_t)w]);
            const int32_t c = g.col[(size_t)p];
            af[p] = make_int2(w, pc.colmap ? (int32_t)pc.colmap[c] : c);
        }
    };
    int64_t rb = 0, vb = 0, ab = 0, vib = 0;
    plan->g_n.resize((size_t)G); plan->g_maxdeg.resize((size_t)G); plan->g_sbdeg.resize((size_t)G); plan->g_level.resize((size_t)G);
    std::vector<int2> tmp_a, tmp_f;
    for (int64_t gi = 0; gi < G; ++gi) {
        const PlanPiece &pc = pieces[(size_t)gi];
        UgsGraphDesc &d = desc[gi];
        d.node_lo = pc.lo; d.rbase = rb; d.vbase = vb; d.viable_base = vib; d.pad = 0;
        if (!pc.g) { d.n = 0; d.level = -1; d.n_viable = 0; plan->g_n[(size_t)gi] = 0; plan->g_maxdeg[(size_t)gi] = 0; plan->g_sbdeg[(size_t)gi] = 0; plan->g_level[(size_t)gi] = -1; continue; }
        const Graph &g = *pc.g;
        d.n = (int32_t)g.n; d.level = g.level; d.n_viable = (int32_t)g.viable.size();
        plan->g_n[(size_t)gi] = g.n; plan->g_maxdeg[(size_t)gi] = g.max_deg; plan->g_sbdeg[(size_t)gi] = g.sb_deg; plan->g_level[(size_t)gi] = g.level;
        for (int64_t r = 0; r <= g.n; ++r) rowp[rb + r] = ab + g.rowptr[(size_t)r];
        if (!split) fill_adj(pc, adj + ab, adjf + ab);
        else {
            int2 *d_adj = reinterpret_cast<int2 *>(base + off_adj) + ab, *d_adjf = reinterpret_cast<int2 *>(base + off_col) + ab;
            hipError_t e = hipSuccess;
            if (UgsDevPre *dp = dpre[(size_t)gi]) {
                const int64_t *cm = pc.colmap;
                if (cm) { bool ident = true; for (int64_t c = 0; c < pc.ncols && ident; ++c) ident = cm[c] == c; if (ident) cm = nullptr; }
                e = ugs_devpre_assemble(dp, cm, pc.ncols, d_adj, d_adjf, dc.stream);
                if (e == hipSuccess) g_pre_device_pieces.fetch_add(1);
            } else if (g.nnz > 0) {
                tmp_a.resize((size_t)g.nnz); tmp_f.resize((size_t)g.nnz);
                fill_adj(pc, tmp_a.data(), tmp_f.data());
                e = hipMemcpy(d_adj, tmp_a.data(), (size_t)g.nnz * sizeof(int2), hipMemcpyHostToDevice);
                if (e == hipSuccess) e = hipMemcpy(d_adjf, tmp_f.data(), (size_t)g.nnz * sizeof(int2), hipMemcpyHostToDevice);
            }
            if (e != hipSuccess) { give_back(); return fail_hip(e, "plan adjacency"); }
        }
        if (g.level == 0)
            for (int64_t vi = 0; vi < g.n; ++vi) {
                UgsRootRec &r = roots[vb + vi];
                r.prob = g.prob[(size_t)vi]; r.alias = g.alias[(size_t)vi];
                r.v_self = g.order[(size_t)vi]; r.v_alias = g.order[(size_t)g.alias[(size_t)vi]]; r.pad = 0;
            }
        else
            for (size_t t = 0; t < g.viable.size(); ++t) via[vib + (int64_t)t] = make_int2(g.viable[t], g.order[(size_t)g.viable[t]]);
        rb += g.n + 1; vb += g.n; ab += g.nnz; if (g.level > 0) vib += (int64_t)g.viable.size();
    }
    hipError_t e = hipMemcpy(dptr, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && split) e = hipMemcpy(base + off_root, tail.data(), tail.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { give_back(); return fail_hip(e, "hipMemcpy(plan)"); }
    plan->device = dc.id; plan->cus = dc.cus;
    plan->G = G; plan->nverts = nv; plan->nnz = nnz;
    plan->blob = dptr; plan->blob_bytes = total;
    plan->dev.graphs = reinterpret_cast<const UgsGraphDesc *>(base + off_desc);
    plan->dev.rowptr = reinterpret_cast<const int64_t *>(base + off_row);
    plan->dev.adj = reinterpret_cast<const int2 *>(base + off_adj);
    plan->dev.adjf = reinterpret_cast<const int2 *>(base + off_col);
    plan->dev.roots = reinterpret_cast<const UgsRootRec *>(base + off_root);
    plan->dev.viable = reinterpret_cast<const int2 *>(base + off_via);
    plan->dev.num_graphs = G;
    return UGS_OK;
}

hipError_t ev_begin(ugs_plan *p, int kind, hipStream_t s) {
    if (!p->timing) return hipSuccess;
    ugs_plan::EvPair e{nullptr, nullptr, kind};
    hipError_t r = hipEventCreate(&e.a);
    if (r == hipSuccess) r = hipEventCreate(&e.b);
    if (r == hipSuccess) r = hipEventRecord(e.a, s);
    p->events.push_back(e);
    return r;
}
hipError_t ev_end(ugs_plan *p, hipStream_t s) {
    if (!p->timing || p->events.empty()) return hipSuccess;
    return hipEventRecord(p->events.back().b, s);
}
void ev_clear(ugs_plan *p) {
    for (auto &e : p->events) { if (e.a) (void)hipEventDestroy(e.a); if (e.b) (void)hipEventDestroy(e.b); }
    p->events.clear();
}

void destroy_plan(ugs_plan *p) {
    if (!p) return;
    if (p->device >= 0 && hipSetDevice(p->device) == hipSuccess) (void)hipDeviceSynchronize();   // kernels may still read the plan
    ev_clear(p);
    if (p->last_ev) (void)hipEventDestroy(p->last_ev);
    if (p->blob_buf.p) pool_put(p->blob_buf); else if (p->blob) (void)hipFree(p->blob);
    pool_put(p->counts); pool_put(p->ovf1); pool_put(p->ovf2); pool_put(p->ovfcnt); pool_put(p->scantmp);
    pool_put(p->stage); pool_put(p->ulist); pool_put(p->work); pool_put(p->tiles);
    pin_slot_put(p->pin_slot);
    if (p->prow.p) { if (p->prow_pooled) pool_put(p->prow); else (void)hipFree(p->prow.p); p->prow = PoolBuf(); p->ord1 = nullptr; }
    if (p->gws.p) { (void)hipFree(p->gws.p); p->gws = PoolBuf(); }
    ugs_plan *owner = p->twin_of;
    delete p;
    if (owner && owner->refs.fetch_sub(1) == 1) destroy_plan(owner);
}
}  // namespace
namespace { void plan_unref(ugs_plan *p) { if (p && p->refs.fetch_sub(1) == 1) destroy_plan(p); } }
namespace {

// plan cache of batches (small LRU; a hit skips assembly + upload)
std::mutex g_pc_mu;
std::list<ugs_plan *> &g_plan_cache = *new std::list<ugs_plan *>();     // front = most recent
size_t g_plan_cache_cap = 64;
size_t g_plan_cache_bytes_cap = (size_t)8 << 30;

ugs_plan *plan_cache_get(uint64_t key, int dev) {
    std::lock_guard<std::mutex> lk(g_pc_mu);
    for (auto it = g_plan_cache.begin(); it != g_plan_cache.end(); ++it)
        if ((*it)->cache_key == key && (*it)->device == dev) {
            ugs_plan *p = *it;
            g_plan_cache.splice(g_plan_cache.begin(), g_plan_cache, it);
            p->refs.fetch_add(1);
            return p;
        }
    return nullptr;
}
void plan_cache_put(ugs_plan *p) {
    std::vector<ugs_plan *> victims;
    {
        std::lock_guard<std::mutex> lk(g_pc_mu);
        p->refs.fetch_add(1);
        p->cached = true;
        g_plan_cache.push_front(p);
        size_t bytes = 0;
        for (auto *q : g_plan_cache) bytes += q->blob_bytes + q->prow_bytes.load();
        while (g_plan_cache.size() > g_plan_cache_cap || (bytes > g_plan_cache_bytes_cap && g_plan_cache.size() > 1)) {
            ugs_plan *v = g_plan_cache.back();
            g_plan_cache.pop_back();
            bytes -= v->blob_bytes + v->prow_bytes.load();
            victims.push_back(v);
        }
    }
    for (auto *v : victims) plan_unref(v);
}
void plan_cache_trim() {      // after a cached plan grew (padded rows built lazily): apply the byte cap again
    std::vector<ugs_plan *> victims;
    {
        std::lock_guard<std::mutex> lk(g_pc_mu);
        size_t bytes = 0;
        for (auto *q : g_plan_cache) bytes += q->blob_bytes + q->prow_bytes.load();
        while (bytes > g_plan_cache_bytes_cap && g_plan_cache.size() > 1) {
            ugs_plan *v = g_plan_cache.back();
            g_plan_cache.pop_back();
            bytes -= v->blob_bytes + v->prow_bytes.load();
            victims.push_back(v);
        }
    }
    for (auto *v : victims) plan_unref(v);
}
void plan_cache_clear() {
    std::vector<ugs_plan *> victims;
    { std::lock_guard<std::mutex> lk(g_pc_mu); victims.assign(g_plan_cache.begin(), g_plan_cache.end()); g_plan_cache.clear(); }
    for (auto *v : victims) plan_unref(v);
}

// ---------------------------------------------------------------------------------------------------------------
// Repeated batches.  The reference interface hands the whole batch over on every call, and the reference (like the general
// path below) walks every column of it to slice, renumber and hash the graphs before it finds its preprocessing in the LRU.
// A training loop calls with the SAME batch tensors again and again (gps/experiment.py:882-883, fixed seed), so calls are
// first matched as a whole: a 128-bit content hash of (edge_index rows, ptr) -- two independent 64-bit multiply-fold lanes
// over every byte, one pass at memory speed -- names the batch; a hit replays exactly what the general path would do to the
// LRU (one lookup per graph, in graph order: same recency order, same hit counters) and, if every graph is still cached under
// the same handle and the plan is still in the plan cache, returns that plan.  Anything else falls through to the general
// path.  Observable behaviour is that of the general path; the cost drops from several passes over the columns with
// per-column searches and copies (0.24 s per call on the 20M-column graph) to one hashing pass.
// ---------------------------------------------------------------------------------------------------------------
struct Hash128 { uint64_t a, b; bool operator==(const Hash128 &o) const { return a == o.a && b == o.b; } };
inline uint64_t mum(uint64_t x, uint64_t y) { const __uint128_t r = (__uint128_t)x * y; return (uint64_t)r ^ (uint64_t)(r >> 64); }
void hash_words(const int64_t *p, int64_t n, Hash128 &h) {
    const uint64_t K0 = 0xa0761d6478bd642full, K1 = 0xe7037ed1a0b428dbull, K2 = 0x8ebc6af09c88c6e3ull, K3 = 0x589965cc75374cc3ull;
    uint64_t a0 = h.a, a1 = h.a ^ K2, b0 = h.b, b1 = h.b ^ K3;
    int64_t i = 0;
    for (; i + 4 <= n; i += 4) {      // two accumulators per lane: the multiplies of consecutive groups overlap
        const uint64_t x0 = (uint64_t)p[i], x1 = (uint64_t)p[i + 1], x2 = (uint64_t)p[i + 2], x3 = (uint64_t)p[i + 3];
        a0 = mum(x0 ^ K0, x1 ^ a0); a1 = mum(x2 ^ K0, x3 ^ a1);
        b0 = mum(x1 ^ K1, x0 ^ b0); b1 = mum(x3 ^ K1, x2 ^ b1);
    }
    for (; i < n; ++i) { a0 = mum((uint64_t)p[i] ^ K0, a0 ^ K2); b0 = mum((uint64_t)p[i] ^ K1, b0 ^ K3); }
    h.a = mum(a0 ^ K1, a1 ^ (uint64_t)n); h.b = mum(b0 ^ K0, b1 ^ (uint64_t)n);
}
// Equality of two batches is decided by their 128-bit content hash -- probabilistic, and the multiply-fold lanes are not
// collision-resistant against crafted input -- plus a WITNESS of 32 words read back from fixed places of the batch (first, last and
// evenly strided columns of both rows and the ends of ptr): a false match would need a hash collision between two batches that also
// agree in those words.
struct Witness {
    int64_t w[32];
    bool operator==(const Witness &o) const { return std::memcmp(w, o.w, sizeof(w)) == 0; }
};
Witness batch_witness(const int64_t *src, const int64_t *dst, int64_t E, const int64_t *ptr, int64_t G) {
    Witness x{};
    for (int i = 0; i < 14; ++i) {
        const int64_t j = E > 0 ? (int64_t)((__int128)i * (E - 1) / 13) : 0;
        x.w[i] = E > 0 ? src[j] : 0;
        x.w[14 + i] = E > 0 ? dst[j] : 0;
    }
    x.w[28] = ptr[0]; x.w[29] = ptr[G]; x.w[30] = ptr[G / 2]; x.w[31] = E ^ (G << 40);
    return x;
}
struct BatchEntry {
    Hash128 h; int64_t E, G; int k, dev;
    uint64_t plan_key;
    std::vector<std::pair<uint64_t, int64_t>> graphs;     // (LRU key, handle) of every non-degenerate graph, in graph order
    Witness wit;
};
std::mutex g_bi_mu;
std::list<BatchEntry> &g_batch_index = *new std::list<BatchEntry>();   // front = most recent, at most as many as cached plans
void batch_index_clear() { std::lock_guard<std::mutex> lk(g_bi_mu); g_batch_index.clear(); }
// The plan a batch PROBABLY maps to, from the 32 sampled words alone (no pass over the columns, no LRU effect): the streamed call
// starts its walks on it while the real lookup -- content hash, LRU replay -- runs, and keeps them only if that lookup names the same plan.
ugs_plan *peek_batch_plan(const int64_t *src, const int64_t *dst, int64_t E, const int64_t *ptr, int64_t G, int k, int dev) {
    const Witness wit = batch_witness(src, dst, E, ptr, G);
    uint64_t key = 0;
    {
        std::lock_guard<std::mutex> lk(g_bi_mu);
        auto it = g_batch_index.begin();
        for (; it != g_batch_index.end(); ++it)
            if (it->E == E && it->G == G && it->k == k && it->dev == dev && it->wit == wit) { key = it->plan_key; break; }
        if (it == g_batch_index.end()) return nullptr;
    }
    return plan_cache_get(key, dev);
}

// A long array is hashed in chunks of a FIXED size (the value must not depend on the number of threads) by a few helper
// threads; the chunk hashes are then hashed in order.  (20M columns: the hashing pass drops from ~10 ms to ~2 ms of a 20 ms call.)
void hash_array(const int64_t *p, int64_t n, Hash128 &h) {
    constexpr int64_t CH = (int64_t)1 << 20;                                  // words per chunk (8 MB)
    if (n < 4 * CH) { hash_words(p, n, h); return; }
    const int64_t nch = (n + CH - 1) / CH;
    std::vector<Hash128> part((size_t)nch);
    const Hash128 seed = h;
    auto work = [&](int64_t first, int64_t stride) {
        for (int64_t c = first; c < nch; c += stride) {
            Hash128 x{seed.a ^ (0x9e3779b97f4a7c15ull * (uint64_t)(c + 1)), seed.b + (uint64_t)c};
            hash_words(p + c * CH, std::min<int64_t>(CH, n - c * CH), x);
            part[(size_t)c] = x;
        }
    };
    const int64_t hw = (int64_t)std::thread::hardware_concurrency();
    const int64_t T = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nch, 8), hw > 0 ? hw : 1));
    std::vector<std::thread> helpers;
    int64_t started = 1;                                                       // strides taken by a thread: 0 (this one), 1 .. started-1
    try {
        for (int64_t t = 1; t < T; ++t) { helpers.emplace_back(work, t, T); started = t + 1; }
    } catch (...) {}                                                           // std::system_error must not cross the C ABI: this thread does the rest
    work(0, T);
    for (int64_t t = started; t < T; ++t) work(t, T);
    for (auto &th : helpers) th.join();
    static_assert(sizeof(Hash128) == 2 * sizeof(int64_t), "chunk hashes are hashed as words");
    hash_words(reinterpret_cast<const int64_t *>(part.data()), 2 * nch, h);
}

Hash128 batch_hash(const int64_t *src, const int64_t *dst, int64_t E, const int64_t *ptr, int64_t G) {
    Hash128 h{0x2d358dccaa6c78a5ull ^ (uint64_t)E, 0x8bb84b93962eacc9ull ^ (uint64_t)G};
    hash_words(ptr, G + 1, h);
    hash_array(src, E, h);
    hash_array(dst, E, h);
    return h;
}

// the LRU touches of a matched batch; false = some graph is no longer cached under the recorded handle (caller takes the general path)
bool batch_replay(const BatchEntry &e, int64_t &hits) {
    std::lock_guard<std::mutex> lk(g_lru_mu);
    for (auto &kh : e.graphs) {
        int64_t handle = 0;
        if (!lru().get(kh.first, handle) || handle != kh.second) return false;
        ++lru().hits; ++hits;
    }
    return true;
}

// pick the walk tier(s) for k: the candidate set of a walk holds at most min(n-1, (k-1)*max degree) vertices
TierChoice choose_tier(ugs_plan *p, int k) {
    std::lock_guard<std::mutex> lk(p->mu);
    auto it = p->tiers.find(k);
    if (it != p->tiers.end()) return it->second;
    int64_t bound = 0;
    double mean = 0;            // expected candidates at the last step: (k-1) rows of size-biased mean degree
    for (size_t gi = 0; gi < p->g_n.size(); ++gi) {
        if (p->g_level[gi] < 0) continue;
        const int64_t b = std::max<int64_t>(0, std::min<int64_t>(p->g_n[gi] - 1, (int64_t)(k - 1) * p->g_maxdeg[gi]));
        bound = std::max(bound, b);
        mean = std::max(mean, std::min<double>((double)b, (double)(k - 1) * p->g_sbdeg[gi]));
    }
    TierChoice t;
    t.bound = bound;
    // First tier.  8 lanes per walk only with a safety margin (a handed-on walk of a small graph is redone with a whole wave).
    // Among the 64-lane tiers the smaller one pays as long as most walks fit: measured on ER degree 40, k = 12 (mean 451),
    // starting in the 448 tier hands 1.4 % of the rows on and runs at 47.8 M/s against 33.4 M/s when everything starts in
    // the 1024 tier; k = 10 (mean 369): 68 against 43 M/s.
    t.first = UGS_TIER_L;
    if (1.3 * mean + 16.0 <= UGS_TIER_CAP[UGS_TIER_S] || bound <= UGS_TIER_CAP[UGS_TIER_S]) t.first = UGS_TIER_S;
    else
        for (int tier = UGS_TIER_M; tier < UGS_TIER_L; ++tier)
            if (mean <= 1.05 * UGS_TIER_CAP[tier] || bound <= UGS_TIER_CAP[tier]) { t.first = tier; break; }
    if (const char *e = std::getenv("UGS_FORCE_TIER")) { int f = std::atoi(e); if (f >= 0 && f < UGS_LDS_TIERS) t.first = f; }
    // A tier hands a walk on when its candidate list would overflow (bound > CAP) OR when its hash-table guard trips:
    // `vertices seen + candidate lanes of the chunk > hash limit`, which is conservative (the lanes need not be new).  A walk
    // has seen at most bound + 1 vertices, so the guard can trip as soon as bound + 1 + lanes-per-walk exceeds the limit --
    // for the 448-candidate tier (limit 448, 64 lanes) already from bound 384.
    auto may_hand_on = [&](int tier) { return bound > UGS_TIER_CAP[tier] || bound + 1 + UGS_TIER_LANES[tier] > UGS_TIER_HASH_LIMIT[tier]; };
    // handed-on rows are redone ONCE by the smallest LDS tier that cannot hand on itself (else the largest), then by the
    // global-memory tier if even that one can
    if (t.first < UGS_TIER_L && may_hand_on(t.first)) {
        t.second = UGS_TIER_L;
        for (int tier = t.first + 1; tier < UGS_TIER_L; ++tier) if (!may_hand_on(tier)) { t.second = tier; break; }
    }
    const int last_lds = t.second >= 0 ? t.second : t.first;
    t.third_G = may_hand_on(last_lds);
    // tier S in its 32-candidate form: only where no walk can outgrow it (candidate bound, and the hash guard: seen vertices + the
    // 8 lanes of a chunk), so that it needs no hand-on chain of its own
    t.small = t.first == UGS_TIER_S && bound <= UGS_SMALL_CAP && bound + 1 + UGS_TIER_LANES[UGS_TIER_S] <= UGS_SMALL_HASH_LIMIT &&
              std::getenv("UGS_NO_SMALL_TIER") == nullptr;
    // tier S with 16 lanes per walk (UGS_WIDE_LANES; plan_walk_impl takes it for launches that fit the GPU at once): only where no walk
    // can be handed on with 16-lane chunks either
    t.wide = t.first == UGS_TIER_S && (t.small ? bound + 1 + UGS_WIDE_LANES <= UGS_SMALL_HASH_LIMIT
                                               : bound <= UGS_TIER_CAP[UGS_TIER_S] && bound + 1 + UGS_WIDE_LANES <= UGS_TIER_HASH_LIMIT[UGS_TIER_S]);
    p->tiers[k] = t;
    return t;
}

// Column j belongs to graph g iff both endpoints lie in [ptr[g], ptr[g+1]) (the reference lets every graph scan every
// column, src/ugs_sampler_batch_extension.cpp:41-75; with a monotone ptr the node ranges are disjoint and one pass with a
// binary search gives the same per-graph lists, in column order).
void assign_columns(const int64_t *src, const int64_t *dst, int64_t E, const int64_t *ptr, int64_t G,
                    std::vector<int64_t> &cstart, std::vector<int64_t> &cols_of) {
    cstart.assign((size_t)G + 1, 0);
    cols_of.clear();
    bool monotone = true;
    for (int64_t g = 0; g < G; ++g) if (ptr[g + 1] < ptr[g]) { monotone = false; break; }
    if (monotone) {
        std::vector<int32_t> owner((size_t)E, -1);
        for (int64_t j = 0; j < E; ++j) {
            const int64_t u = src[j], v = dst[j];
            if (G == 0 || u < ptr[0] || u >= ptr[G]) continue;
            const int64_t g = (std::upper_bound(ptr, ptr + G + 1, u) - ptr) - 1;    // last g with ptr[g] <= u
            if (g < 0 || g >= G || !(u >= ptr[g] && u < ptr[g + 1])) continue;
            if (v >= ptr[g] && v < ptr[g + 1]) { owner[(size_t)j] = (int32_t)g; ++cstart[(size_t)g + 1]; }
        }
        for (int64_t g = 0; g < G; ++g) cstart[(size_t)g + 1] += cstart[(size_t)g];
        cols_of.resize((size_t)cstart[(size_t)G]);
        std::vector<int64_t> wr(cstart.begin(), cstart.end() - 1);
        for (int64_t j = 0; j < E; ++j) if (owner[(size_t)j] >= 0) cols_of[(size_t)wr[(size_t)owner[(size_t)j]]++] = j;
    } else {   // arbitrary ptr: every graph scans every column, like the reference
        for (int64_t g = 0; g < G; ++g) {
            const int64_t lo = ptr[g], hi = ptr[g + 1];
            for (int64_t j = 0; j < E; ++j) if (src[j] >= lo && src[j] < hi && dst[j] >= lo && dst[j] < hi) cols_of.push_back(j);
            cstart[(size_t)g + 1] = (int64_t)cols_of.size();
        }
    }
}

// Padded rows for the one-walk-per-wave tiers (ugs_device.h): 2^shift entries per vertex, sized so that the rows a walk visits
// (degree ~ the size-biased mean) fit their block with three standard deviations to spare; longer rows continue in adj[].
// Built by a kernel from the plan's own CSR, once.  UGS_NO_PROW=1 keeps the row-pointer path (A/B measurements, tests of both).
// Call with plan->mu held.  Failure to allocate is not an error: the walk then reads rows through the row pointer.
int ensure_prow(ugs_plan *plan, hipStream_t s) {
    if (plan->dev.prow || plan->prow_failed || plan->nverts <= 0) return UGS_OK;
    if (const char *e = std::getenv("UGS_NO_PROW")) if (e[0] == '1') return UGS_OK;
    double sb = 0;
    for (double x : plan->g_sbdeg) sb = std::max(sb, x);
    int shift = 3;
    while (shift < 6 && (double)((1 << shift) - 1) < sb + 3.0 * std::sqrt(sb) + 1.0) ++shift;
    if (const char *e = std::getenv("UGS_PROW_SHIFT")) { const int f = std::atoi(e); if (f >= 3 && f <= 6) shift = f; }
    const size_t row_bytes = ((size_t)plan->nverts << shift) * sizeof(int2);
    if (row_bytes >= ((size_t)1 << 32)) { plan->prow_failed = true; return UGS_OK; }   // the walk kernels address a block by a 32-bit byte offset
    // First-pick table (ugs_device.h, UgsWalkArgs::ord1) behind the rows, in the same allocation: it lives and dies with them, is
    // shared with them (ugs_plan_twin, captured steps) and counts with them in ugs_plan_info and against the plan cache's bytes.
    // Only the launch-uniform walk reads it, and that walk serves plans of one graph.  UGS_NO_FIRST_PICK_TABLE=1: neither built nor used.
    const bool want_ord1 = plan->G == 1 && !plan->g_level.empty() && plan->g_level[0] >= 0 && plan->nverts < ((int64_t)1 << 26) &&
                           !env_is_one("UGS_NO_FIRST_PICK_TABLE");
    const size_t bytes = row_bytes + (want_ord1 ? (size_t)plan->nverts * UGS_ORD1_BYTES : 0);
    if (bytes <= ((size_t)64 << 20)) {
        const std::string keep = t_err;
        if (pool_get(bytes, plan->device, plan->prow) != UGS_OK) { t_err = keep; plan->prow_failed = true; return UGS_OK; }
        plan->prow_pooled = true;
    } else {
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); plan->prow_failed = true; return UGS_OK; }
        plan->prow.p = p; plan->prow.bytes = bytes; plan->prow.dev = plan->device;
    }
    HIP_TRY(ugs_launch_build_prow(plan->dev, plan->nverts, static_cast<int2 *>(plan->prow.p), shift, plan->cus, s));
    plan->dev.prow = static_cast<const int2 *>(plan->prow.p);
    plan->dev.prow_shift = shift;
    // entries fetched together with the header: whole 128-byte lines (16 entries) covering the typical visited row; a row that
    // reaches further costs one more (dependent) load of the block's remaining lines
    int first = (int)std::ceil((sb + 0.5 * std::sqrt(sb) + 1.0) / 16.0) * 16;
    if (const char *e = std::getenv("UGS_PROW_FIRST")) { const int f = std::atoi(e); if (f >= 1) first = f; }
    plan->dev.prow_first = std::max(1, std::min(first, 1 << shift));
    if (want_ord1) {                            // behind the rows' build on the same stream: its kernel reads them
        uint8_t *o = static_cast<uint8_t *>(plan->prow.p) + row_bytes;
        HIP_TRY(hipMemsetAsync(o, 0, (size_t)plan->nverts * UGS_ORD1_BYTES, s));
        HIP_TRY(ugs_launch_build_ord1(plan->dev, plan->nverts, o, nullptr, plan->cus, s));
        plan->ord1 = o;
    }
    HIP_TRY(hipStreamSynchronize(s));          // once per plan: later calls may come on other streams
    plan->prow_bytes.store(plan->prow.bytes);
    plan->prow_asked = bytes;
    if (plan->cached) plan_cache_trim();        // the cache admitted the plan without these bytes: apply its byte cap again
    return UGS_OK;
}

// plan scratch, grown on demand.  The old buffer goes back to the process-wide pool, where any stream may pick it up: the
// plan's last call has to be over first (rare: sizes settle after the first calls).
int ensure(PoolBuf &b, size_t bytes, int dev, ugs_plan *plan) {
    if (b.p && b.bytes >= bytes) return UGS_OK;
    if (b.p && plan && plan->last_valid) HIP_TRY(hipEventSynchronize(plan->last_ev));     // the event, not the caller's stream handle (which may be gone)
    pool_put(b);
    return pool_get(bytes, dev, b);
}

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
// call with plan->mu held, before the first / after the last kernel of a call on stream s
int plan_enter(ugs_plan *plan, hipStream_t s) {
    if (plan->last_valid && plan->last_stream != s && !capturing(s)) HIP_TRY(hipStreamWaitEvent(s, plan->last_ev, 0));
    return UGS_OK;
}
int plan_leave(ugs_plan *plan, hipStream_t s) {
    if (capturing(s)) return UGS_OK;
    if (!plan->last_ev) HIP_TRY(hipEventCreateWithFlags(&plan->last_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(plan->last_ev, s));
    plan->last_stream = s; plan->last_valid = true;
    return UGS_OK;
}


// ---------------------------------------------------------------------------------------------------------------
// Device batch pass (batches of small graphs; kernels: ugs_batch.hip).
//
// A call with a batch that was not seen before as a whole -- in a training loop: every shuffled mini-batch, a new combination
// of graphs the LRU already knows -- no longer walks the columns on the host.  edge_index and ptr are uploaded, one device pass
// slices the batch, computes every graph's LRU key (the reference's FNV-1a, include/cache.hpp:81-109) and writes the plan's
// rowptr / adj / adjf straight into HBM in the reference's CSR order (src/preproc.cpp:32-86); 36 bytes per graph come back.
// The host replays the LRU on those keys (same lookups, same order, same eviction as the general path) and points every
// graph's descriptor at the root records its cached preprocessing keeps in the device's arena.  Only a graph the LRU does not
// know is sliced and preprocessed on the host (its column span comes back with its key), once.
//
// Applicable when ptr is non-decreasing (disjoint node ranges) and every graph has at most UGS_BATCH_PASS_MAX_N vertices and
// at most as many columns as the limit in force: UGS_BATCH_PASS_MAX_COLS (1000) unless the caller has raised it, up to
// UGS_BATCH_PASS_COLS_CEIL (ugs_set_batch_pass_max_cols, or UGS_BATCH_PASS_MAX_COLS in the environment).  Up to 1000 columns
// the key covers a graph's whole content, so a cached graph with the same key has exactly the CSR the pass has just built.
// Beyond, the reference's key samples the columns (include/cache.hpp:100-107): two different graphs can share a key, and the
// reference then samples from the CACHED graph.  The large form of the pass computes that strided key and, beside it, a
// 128-bit fingerprint of the whole content; a cached graph is accepted only if n, nnz and the fingerprint all agree with what
// the pass has built -- then it IS that graph -- and anything else sends the batch to the general path below, which does what
// the reference does.  With the limit at its default a batch holding such a graph takes the general path, as it always did.
// UGS_DEVICE_BATCH=0 switches the pass off, =1 forces it wherever it applies (see device_batch_mode).
// ---------------------------------------------------------------------------------------------------------------
struct RootArena {
    UgsRootRec *roots = nullptr; int64_t roots_cap = 0, roots_used = 0;
    int2 *via = nullptr; int64_t via_cap = 0, via_used = 0;
    std::map<int64_t, std::vector<int64_t>> free_roots, free_via;      // exact-size reuse of released entries
    void *pinned = nullptr; size_t pinned_bytes = 0;                    // staging: the batch going up, the keys coming back, two descriptor slots
    hipEvent_t desc_ev[2] = {nullptr, nullptr}; int desc_slot = 0;
    unsigned long long *d_bump = nullptr;                               // device counter handing out CSR space to the graphs of a pass (never reset)
    unsigned long long bump_host = 0;                                   // its value before the next pass
    unsigned long long done_host = 0;                                   // likewise the blocks-done counter (d_bump + 1) behind the kernels' completion signal
    uint32_t epoch = 0;                                                 // names a pass: written to the flag word by a graph beyond the limits
    std::mutex call_mu;                                                 // one device pass at a time per device (shared staging)
};
std::mutex g_arena_mu;
std::map<int, RootArena *> &g_arenas = *new std::map<int, RootArena *>();
constexpr int64_t kArenaRoots = (int64_t)2 << 20, kArenaVia = (int64_t)1 << 20;     // 48 MB of root records + 8 MB of viable entries per device

RootArena *arena_of(int dev) {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    auto it = g_arenas.find(dev);
    if (it != g_arenas.end()) return it->second;
    auto *a = new RootArena();
    if (hipMalloc(reinterpret_cast<void **>(&a->roots), (size_t)kArenaRoots * sizeof(UgsRootRec)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&a->via), (size_t)kArenaVia * sizeof(int2)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&a->d_bump), 256) != hipSuccess || hipMemset(a->d_bump, 0, 256) != hipSuccess) {
        (void)hipGetLastError();
        if (a->roots) (void)hipFree(a->roots);
        delete a;
        g_arenas[dev] = nullptr;                                        // no arena on this device: the general path serves every call
        return nullptr;
    }
    a->roots_cap = kArenaRoots; a->via_cap = kArenaVia;
    g_arenas[dev] = a;
    return a;
}
int64_t arena_take(std::map<int64_t, std::vector<int64_t>> &fl, int64_t &used, int64_t cap, int64_t n) {   // g_arena_mu held
    if (n <= 0) return 0;
    auto it = fl.find(n);
    if (it != fl.end() && !it->second.empty()) { const int64_t off = it->second.back(); it->second.pop_back(); return off; }
    if (used + n > cap) return -1;
    const int64_t off = used;
    used += n;
    return off;
}
void arena_release(int dev, int64_t roots_off, int64_t n_roots, int64_t via_off, int64_t n_via) {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    auto it = g_arenas.find(dev);
    if (it == g_arenas.end() || !it->second) return;
    if (n_roots > 0 && roots_off >= 0) it->second->free_roots[n_roots].push_back(roots_off);
    if (n_via > 0 && via_off >= 0) it->second->free_via[n_via].push_back(via_off);
}
// the graph's root records (level 0) or viable list (levels 1, 2) in the device's arena; uploaded once per graph and device
int graph_dev_roots(Graph &g, int dev, RootArena *ar, hipStream_t s, Graph::DevRoots &out) {
    std::lock_guard<std::mutex> lk(g.pre_mu);
    for (auto &d : g.dev_roots) if (d.dev == dev) { out = d; return UGS_OK; }
    if (!g.host_ready) return UGS_E_UNSUPPORTED;                        // a stub of another device's pass: the general path completes it first
    Graph::DevRoots d{dev, -1, 0, -1, 0};
    if (g.level == 0) d.n_roots = g.n; else d.n_via = (int64_t)g.viable.size();
    {
        std::lock_guard<std::mutex> lk2(g_arena_mu);
        d.roots_off = arena_take(ar->free_roots, ar->roots_used, ar->roots_cap, d.n_roots);
        d.via_off = arena_take(ar->free_via, ar->via_used, ar->via_cap, d.n_via);
    }
    if (d.roots_off < 0 || d.via_off < 0) {
        if (d.roots_off >= 0 || d.via_off >= 0) arena_release(dev, d.roots_off, d.n_roots, d.via_off, d.n_via);
        return UGS_E_UNSUPPORTED;                                       // arena full: not an error, the caller takes the general path
    }
    if (g.level == 0 && g.n > 0) {
        std::vector<UgsRootRec> rec((size_t)g.n);
        for (int64_t vi = 0; vi < g.n; ++vi) {
            UgsRootRec &r = rec[(size_t)vi];
            r.prob = g.prob[(size_t)vi]; r.alias = g.alias[(size_t)vi];
            r.v_self = g.order[(size_t)vi]; r.v_alias = g.order[(size_t)g.alias[(size_t)vi]]; r.pad = 0;
        }
        HIP_TRY(hipMemcpyAsync(ar->roots + d.roots_off, rec.data(), rec.size() * sizeof(UgsRootRec), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));                               // `rec` is pageable and goes out of scope
    } else if (g.level > 0 && !g.viable.empty()) {
        std::vector<int2> v(g.viable.size());
        for (size_t t = 0; t < g.viable.size(); ++t) v[t] = make_int2(g.viable[t], g.order[(size_t)g.viable[t]]);
        HIP_TRY(hipMemcpyAsync(ar->via + d.via_off, v.data(), v.size() * sizeof(int2), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    g.dev_roots.push_back(d);
    out = d;
    return UGS_OK;
}

// UGS_DEVICE_BATCH: 0 = never, 1 = whenever applicable, unset = whenever applicable and the batch has at least
// kBatchPassMinCols columns.  The chain upload -> kernel -> keys back costs ~20 us of latencies whatever the size (round 4: the host
// polls the kernel's completion word instead of waiting on the stream, -5 us).  Measured with the two paths taking turns call by call
// (tools/batch_pass_probe.py, medians of 55 calls each, host-visible / device outputs): 4672 columns (PROTEINS-shaped) 0.261 / 0.175
// against 0.279 / 0.187 ms for the host's own pass + plan assembly: the pass wins; ~1200 columns (QM9- / MUTAG-shaped batches of 32
// graphs) 0.772 / 0.193 against 0.742 / 0.177 ms and 0.134 / 0.135 against 0.118 / 0.119 ms: it still loses ~16 us.  (Sequential
// measurements -- first one path, then the other -- had shown a tie there: the order of the two had favoured the second.)
constexpr int64_t kBatchPassMinCols = 2048;
int device_batch_mode() {
    const char *e = std::getenv("UGS_DEVICE_BATCH");
    if (e && e[0] == '0') return 0;
    if (e && e[0] == '1') return 1;
    return 2;
}

constexpr int kBatchNotApplicable = 1;      // positive: not an error code of the C ABI

// 64-byte slots of pinned host memory, handed out from slabs that live as long as the process
std::mutex g_pin_mu;
std::vector<char *> &g_pin_free = *new std::vector<char *>();
char *pin_slot_get() {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (g_pin_free.empty()) {
        void *slab = nullptr;
        if (hipHostMalloc(&slab, 64 * 256, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        std::memset(slab, 0, 64 * 256);
        for (int i = 255; i >= 0; --i) g_pin_free.push_back(static_cast<char *>(slab) + 64 * i);
    }
    char *p = g_pin_free.back();
    g_pin_free.pop_back();
    std::memset(p, 0, 64);                      // whatever the slot's last owner's kernels wrote (they are long over)
    return p;
}
std::atomic<uint32_t> g_pin_epoch{0};           // one sequence for all plans: a slot changes hands, its signal values never repeat
void pin_slot_put(char *p) { if (p) { std::lock_guard<std::mutex> lk(g_pin_mu); g_pin_free.push_back(p); } }

// Wait for a kernel that signals its end by writing `want` to a word in pinned host memory (ugs_batch.hip: bp_signal_done): polling the
// word returns ~5 us earlier than hipStreamSynchronize on this stack (tools/sync_probe.hip: 5.9 against 10.9 us for an empty kernel).
// The budget bounds the spin: a kernel that faulted never signals, and the stream wait behind the spin reports its error.
hipError_t wait_signal(const volatile uint32_t *word, uint32_t want, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        if (*word == want) { std::atomic_thread_fence(std::memory_order_acquire); return hipSuccess; }
        if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
    }
    return hipStreamSynchronize(s);
}
std::atomic<int64_t> g_bp_plans{0}, g_bp_fallbacks{0};     // plans built by the device pass / calls it handed to the general path

// Columns per graph up to which the pass applies: process-wide, read once per call (a call in flight keeps what it started with).
// First use takes UGS_BATCH_PASS_MAX_COLS from the environment; out of range = ignored.
std::atomic<int64_t> g_bp_max_cols{UGS_BATCH_PASS_MAX_COLS};
int64_t batch_pass_max_cols() {
    static std::once_flag once;
    std::call_once(once, [] {
        const char *e = std::getenv("UGS_BATCH_PASS_MAX_COLS");
        if (!e || !*e) return;
        char *end = nullptr;
        const long long v = std::strtoll(e, &end, 10);
        if (end && *end == 0 && v >= UGS_BATCH_PASS_MAX_COLS && v <= UGS_BATCH_PASS_COLS_CEIL) g_bp_max_cols.store(v);
        else if (debug_on()) std::fprintf(stderr, "[UGS INFO] UGS_BATCH_PASS_MAX_COLS=%s ignored: must be %d ... %d\n", e, UGS_BATCH_PASS_MAX_COLS, UGS_BATCH_PASS_COLS_CEIL);
    });
    return g_bp_max_cols.load();
}

// Returns UGS_OK with *plan_out set, kBatchNotApplicable (the caller takes the general path; the LRU has not been touched, or
// its counters have been put back), or an error.
int device_batch_plan(const int64_t *src, const int64_t *dst, int64_t E, const int64_t *ptr, int64_t G, int k, const DeviceCtx &dc,
                      bool have_hash, const Hash128 &bh, ugs_plan **plan_out, std::vector<std::pair<uint64_t, int64_t>> &touched) {
    if (G <= 0 || E <= 0 || G > ((int64_t)1 << 20) || E >= ((int64_t)1 << 24)) return kBatchNotApplicable;
    RootArena *ar = arena_of(dc.id);
    if (!ar) return kBatchNotApplicable;
    const int64_t max_cols = batch_pass_max_cols();                     // the limit in force for this call
    std::lock_guard<std::mutex> call_lk(ar->call_mu);
    // pinned staging, one buffer: [src E | dst E | ptr G+1 | rstart G] goes up in ONE copy, [keys G | fingerprints 2G | cnt G | jminc G |
    // jmax G | flag] comes back in one, two descriptor slots go up behind the LRU replay
    const size_t up_words = (size_t)(2 * E + 2 * G + 1), back_bytes = UGS_BP_BACK_BYTES(G), desc_bytes = (size_t)G * sizeof(UgsGraphDesc);
    const size_t miss_bytes = (size_t)G * (sizeof(UgsBpMissIn) + sizeof(UgsBpMissOut)) + 16;
    const size_t st_back = align_up(up_words * 8), st_desc = align_up(st_back + back_bytes), st_miss = align_up(st_desc + 2 * align_up(desc_bytes)),
                 st_total = align_up(st_miss + miss_bytes);
    // the staging's layout depends on this call's E and G: a descriptor copy of an earlier call (asynchronous, from a region placed by
    // ITS sizes) must be over before anything here is written.  Normally long done.
    for (auto &ev : ar->desc_ev) if (ev) (void)hipEventSynchronize(ev);
    if (ar->pinned_bytes < st_total) {
        if (ar->pinned) { for (auto &ev : ar->desc_ev) if (ev) (void)hipEventSynchronize(ev); (void)hipHostFree(ar->pinned); }
        ar->pinned = nullptr; ar->pinned_bytes = 0;
        const size_t want = std::max<size_t>(st_total * 2, 1 << 18);
        if (hipHostMalloc(&ar->pinned, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return kBatchNotApplicable; }
        ar->pinned_bytes = want;
        std::memset(ar->pinned, 0, want);
    }
    auto *hostv = static_cast<int64_t *>(ar->pinned);                   // src | dst | ptr | rstart
    int64_t *h_ptr = hostv + 2 * E, *h_rstart = h_ptr + (G + 1);
    int64_t rows_total = 0, nv = 0;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = ptr[g + 1] - ptr[g];
        if (n < 0 || n > UGS_BATCH_PASS_MAX_N) return kBatchNotApplicable;      // non-monotone ptr, or a large graph
        h_rstart[g] = rows_total;
        if (n > 0 && n >= k) { rows_total += n + 1; nv += n; }
    }
    std::memcpy(hostv, src, (size_t)E * 8);
    std::memcpy(hostv + E, dst, (size_t)E * 8);
    std::memcpy(h_ptr, ptr, (size_t)(G + 1) * sizeof(int64_t));
    // ---- one device allocation: the plan's arrays, then the pass's inputs and scratch -------------------------------------------
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + std::max<size_t>(bytes, 8)); return o; };
    const size_t o_desc = take(desc_bytes), o_row = take((size_t)rows_total * sizeof(int64_t));
    const size_t o_adj = take((size_t)2 * E * sizeof(int2)), o_adjf = take((size_t)2 * E * sizeof(int2));
    const bool fused = G * E <= ugs_batch_pass_fused_work();
    const size_t o_vrank = take((size_t)rows_total * sizeof(int32_t));
    const size_t o_up = take(up_words * 8), o_owner = take(fused ? 8 : (size_t)E * 4), o_cnt = take(fused ? 8 : (size_t)G * 12);
    auto *p = new ugs_plan();
    if (int rc = pool_get(off, dc.id, p->blob_buf)) { delete p; return rc; }
    char *base = static_cast<char *>(p->blob_buf.p);
    auto bail = [&](int rc) { pool_put(p->blob_buf); delete p; return rc; };
    hipStream_t s = dc.stream;
    Lap lap;
    auto *d_src = reinterpret_cast<int64_t *>(base + o_up), *d_dst = d_src + E, *d_ptr = d_dst + E;
    // what comes back is written by the kernel straight into the pinned staging (keys[G] u64 | fp[2G] u64 | cnt[G] | jminc[G] | jmax[G] | flag): no
    // copy command behind the kernel, the host waits for the stream only
    char *h_back = static_cast<char *>(ar->pinned) + st_back;
    const uint32_t epoch = ++ar->epoch ? ar->epoch : ++ar->epoch;       // never 0
    *reinterpret_cast<volatile uint32_t *>(h_back + UGS_BP_BACK_FLAG(G)) = 0u;
    *reinterpret_cast<volatile uint32_t *>(h_back + UGS_BP_BACK_FLAG(G) + 4) = 0u;     // the completion word: the staging's layout moves with E and G, so the
                                                                                   // word may hold anything an earlier call left there -- e.g. a column count equal to this epoch
    hipError_t e = hipMemcpyAsync(d_src, hostv, up_words * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = ugs_launch_batch_pass(d_src, d_dst, E, d_ptr, G, k, reinterpret_cast<int32_t *>(base + o_owner), reinterpret_cast<uint32_t *>(base + o_cnt),
                                                   d_ptr + (G + 1), reinterpret_cast<int64_t *>(base + o_row), reinterpret_cast<int2 *>(base + o_adj),
                                                   reinterpret_cast<int2 *>(base + o_adjf), reinterpret_cast<int32_t *>(base + o_vrank), ar->d_bump, ar->bump_host,
                                                   epoch, h_back, ar->d_bump + 1, ar->done_host, max_cols, s);
    if (e == hipSuccess) e = wait_signal(reinterpret_cast<volatile uint32_t *>(h_back + UGS_BP_BACK_FLAG(G) + 4), epoch, s);
    if (e != hipSuccess) {       // the counters' values are unknown now: start again from zero
        (void)hipDeviceSynchronize();
        (void)hipMemset(ar->d_bump, 0, 16); ar->bump_host = 0; ar->done_host = 0;
        return bail(fail_hip(e, "device batch pass"));
    }
    ar->done_host += (unsigned long long)G;
    const double t_pass = lap();
    const auto *h_keys = reinterpret_cast<const unsigned long long *>(h_back);
    const auto *h_fp = h_keys + G;                                      // two words per graph, written for graphs of more than 1000 columns only
    const auto *h_cnt = reinterpret_cast<const uint32_t *>(h_back + UGS_BP_BACK_CNT(G)), *h_jminc = h_cnt + G, *h_jmax = h_jminc + G;
    // Is the cached graph `c` the graph the pass has just built as graph g?  Up to 1000 columns the key covers the content (n and nnz
    // guard a 64-bit collision); above, the key samples the columns and the fingerprint decides.
    auto same_graph = [&](const Graph &c, int64_t g, int64_t n) {
        if (c.n != n || c.nnz != 2 * (int64_t)h_cnt[g]) return false;
        return h_cnt[g] <= (uint32_t)UGS_BATCH_PASS_MAX_COLS || (c.fp_a == (uint64_t)h_fp[2 * g] && c.fp_b == (uint64_t)h_fp[2 * g + 1]);
    };
    {   // the counter moved by twice the columns of the graphs that got as far as their allocation: re-derive it from what came back
        unsigned long long used = 0;
        for (int64_t g = 0; g < G; ++g) used += 2ull * h_cnt[g];
        if (h_jmax[G] == epoch) {                                        // a graph beyond the limits of the pass: which blocks allocated is not known
            (void)hipStreamSynchronize(s);                              // the signal came from the last block's thread 0: let the kernel retire before its counter is rewritten
            (void)hipMemset(ar->d_bump, 0, 8); ar->bump_host = 0;
            return bail(kBatchNotApplicable);
        }
        ar->bump_host += used;
    }
    // ---- the LRU replay on G keys: the same lookups, in graph order, as the general path ----------------------------------------
    const int slot = ar->desc_slot ^= 1;                                 // the copy of the call before last on this device is long over; wait if not
    if (!ar->desc_ev[slot]) { if (hipEventCreateWithFlags(&ar->desc_ev[slot], hipEventDisableTiming) != hipSuccess) return bail(fail(UGS_E_HIP, "hipEventCreate")); }
    else (void)hipEventSynchronize(ar->desc_ev[slot]);
    UgsGraphDesc *desc = reinterpret_cast<UgsGraphDesc *>(static_cast<char *>(ar->pinned) + st_desc + (size_t)slot * align_up(desc_bytes));
    std::vector<int64_t> evicted, ru, rv;
    std::vector<std::shared_ptr<Graph>> graphs((size_t)G);
    int64_t hits = 0, misses = 0, owned_cols = 0;
    p->g_n.assign((size_t)G, 0); p->g_maxdeg.assign((size_t)G, 0); p->g_sbdeg.assign((size_t)G, 0.0); p->g_level.assign((size_t)G, -1);
    touched.clear();
    // Graphs the LRU does not know (cold path).  Up to UGS_BATCH_ROOTS_MAX_N vertices the rest of their preprocessing runs on the
    // device as well (ugs_bp_roots, one launch for all of them behind this loop): the graph exists on the host as a stub.
    // UGS_DEVICE_COLD=0 keeps the host preprocessing (A/B, tests of both).
    struct Pending { int64_t g; std::shared_ptr<Graph> gr; uint64_t key; int64_t handle; int64_t roots_off, via_off; };
    std::vector<Pending> pend;
    std::vector<int32_t> pend_of((size_t)G, -1);
    std::vector<std::pair<uint64_t, int64_t>> inserted;                  // (key, handle) this call has put into the LRU
    const bool cold_on_device = [] { const char *e = std::getenv("UGS_DEVICE_COLD"); return !(e && e[0] == '0'); }();
    auto give_up = [&] {                                                // put the LRU back as it was: the general path repeats the lookups (same final recency order)
        {
            std::lock_guard<std::mutex> lk(g_lru_mu);
            lru().hits -= hits; lru().misses -= misses;
            if (evicted.empty()) for (auto &kv : inserted) lru().erase(kv.first);      // (an eviction cannot be undone: then the entries stay, as before)
        }
        if (evicted.empty()) for (auto &kv : inserted) drop(kv.second);
        for (auto &pd : pend) arena_release(dc.id, pd.roots_off, pd.gr->n, pd.via_off, pd.gr->n);
        for (int64_t h : evicted) drop(h);
        return bail(kBatchNotApplicable);
    };
    for (int64_t g = 0; g < G; ++g) {
        UgsGraphDesc &d = desc[(size_t)g];
        const int64_t lo = ptr[g], n = ptr[g + 1] - lo;
        d.node_lo = lo; d.rbase = h_rstart[g]; d.vbase = 0; d.viable_base = 0; d.n = 0; d.level = -1; d.n_viable = 0; d.pad = 0;
        if (n <= 0 || n < k) continue;                                   // degenerate: m rows of -1 (never looked up: reference :132-143)
        owned_cols += h_cnt[g];
        const uint64_t key = (uint64_t)h_keys[g];
        int64_t handle = 0;
        bool hit;
        {
            std::lock_guard<std::mutex> lk(g_lru_mu);
            hit = lru().get(key, handle);
            if (hit) ++lru().hits; else ++lru().misses;
        }
        std::shared_ptr<Graph> gr = hit ? lookup(handle) : nullptr;
        if (hit) ++hits; else ++misses;
        if (!gr && cold_on_device && n <= UGS_BATCH_ROOTS_MAX_N) {       // unknown graph: a stub now, its root records by the launch behind this loop
            int64_t ro, vo;
            {
                std::lock_guard<std::mutex> lk2(g_arena_mu);
                ro = arena_take(ar->free_roots, ar->roots_used, ar->roots_cap, n);
                vo = arena_take(ar->free_via, ar->via_used, ar->via_cap, n);
            }
            if (ro < 0 || vo < 0) {
                arena_release(dc.id, ro, ro >= 0 ? n : 0, vo, vo >= 0 ? n : 0);
                return give_up();                                        // arena full: the general path serves this batch
            }
            gr = std::make_shared<Graph>();
            gr->n = n; gr->nnz = 2 * (int64_t)h_cnt[g]; gr->k_built = k; gr->host_ready = false; gr->stub_lo = lo;
            if (h_cnt[g] > (uint32_t)UGS_BATCH_PASS_MAX_COLS) { gr->fp_a = (uint64_t)h_fp[2 * g]; gr->fp_b = (uint64_t)h_fp[2 * g + 1]; }
            if (h_cnt[g]) {                                              // its span of the columns, kept until some host path needs the arrays
                const int64_t j0 = (int64_t)(0xFFFFFFFFu - h_jminc[g]), j1 = (int64_t)h_jmax[g] + 1;
                gr->stub_cols.resize((size_t)(2 * (j1 - j0)));
                std::memcpy(gr->stub_cols.data(), src + j0, (size_t)(j1 - j0) * 8);
                std::memcpy(gr->stub_cols.data() + (j1 - j0), dst + j0, (size_t)(j1 - j0) * 8);
            }
            handle = enroll(gr);
            {
                int64_t ev = 0;
                std::lock_guard<std::mutex> lk(g_lru_mu);
                if (lru().put(key, handle, ev)) evicted.push_back(ev);
            }
            inserted.emplace_back(key, handle);
            pend_of[(size_t)g] = (int32_t)pend.size();
            pend.push_back(Pending{g, gr, key, handle, ro, vo});
            touched.emplace_back(key, handle);
            graphs[(size_t)g] = gr;
            continue;
        }
        if (gr && !gr->host_ready) {                                     // a stub: of this very call (a repeated graph), or of an earlier one
            bool mine = false;
            for (size_t i = 0; i < pend.size() && !mine; ++i) if (pend[i].gr.get() == gr.get()) { pend_of[(size_t)g] = (int32_t)i; mine = true; }
            if (mine) {
                if (!same_graph(*gr, g, n)) return give_up();             // (above 1000 columns: two graphs of this batch sharing a strided key)
                touched.emplace_back(key, handle);
                graphs[(size_t)g] = gr;
                continue;
            }
        }
        if (!gr) {                                                       // unknown graph: sliced and preprocessed on the host, once
            ru.clear(); rv.clear();
            if (h_cnt[g]) for (int64_t j = (int64_t)(0xFFFFFFFFu - h_jminc[g]); j <= (int64_t)h_jmax[g]; ++j) {
                const int64_t u = src[j], v = dst[j];
                if (u >= lo && u < lo + n && v >= lo && v < lo + n) { ru.push_back(u - lo); rv.push_back(v - lo); }
            }
            if ((int64_t)ru.size() != (int64_t)h_cnt[g]) return give_up();
            if (int rc = make_graph(ru.data(), rv.data(), (int64_t)ru.size(), n, k, gr)) { give_up(); return rc; }
            handle = enroll(gr);
            int64_t ev = 0;
            std::lock_guard<std::mutex> lk(g_lru_mu);
            if (lru().put(key, handle, ev)) evicted.push_back(ev);
            inserted.emplace_back(key, handle);
        }
        if (!same_graph(*gr, g, n)) return give_up();                    // a key collision (64-bit, or of the strided key): let the general path do what the reference does
        Graph::DevRoots dr{};
        if (int rc = graph_dev_roots(*gr, dc.id, ar, s, dr)) { if (rc == UGS_E_UNSUPPORTED) return give_up(); give_up(); return rc; }
        d.n = (int32_t)n; d.level = gr->level; d.n_viable = (int32_t)gr->n_viable;
        d.vbase = gr->level == 0 ? dr.roots_off : 0; d.viable_base = gr->level > 0 ? dr.via_off : 0;
        p->g_n[(size_t)g] = n; p->g_maxdeg[(size_t)g] = gr->max_deg; p->g_sbdeg[(size_t)g] = gr->sb_deg; p->g_level[(size_t)g] = gr->level;
        touched.emplace_back(key, handle);
        graphs[(size_t)g] = gr;
    }
    if (!pend.empty()) {                                                 // ---- the unknown graphs: root records on the device, 32 bytes each back
        auto *h_in = reinterpret_cast<UgsBpMissIn *>(static_cast<char *>(ar->pinned) + st_miss);
        auto *h_out = reinterpret_cast<UgsBpMissOut *>(h_in + G);
        for (size_t i = 0; i < pend.size(); ++i) h_in[i] = UgsBpMissIn{(int32_t)pend[i].g, 0, pend[i].roots_off, pend[i].via_off};
        auto *h_rdone = reinterpret_cast<uint32_t *>(h_out + G);
        *reinterpret_cast<volatile uint32_t *>(h_rdone) = 0u;
        e = ugs_launch_batch_roots(d_ptr, d_ptr + (G + 1), reinterpret_cast<const int64_t *>(base + o_row), reinterpret_cast<const int2 *>(base + o_adj),
                                   reinterpret_cast<const int32_t *>(base + o_vrank), h_in, h_out, (int64_t)pend.size(), k, ar->roots, ar->via,
                                   ar->d_bump + 1, ar->done_host, h_rdone, epoch, max_cols, s);
        if (e == hipSuccess) e = wait_signal(h_rdone, epoch, s);
        if (e != hipSuccess) {
            (void)hipDeviceSynchronize();
            (void)hipMemset(ar->d_bump, 0, 16); ar->bump_host = 0; ar->done_host = 0;
            give_up();
            return fail_hip(e, "device batch pass: root records");
        }
        ar->done_host += (unsigned long long)pend.size();
        for (size_t i = 0; i < pend.size(); ++i) {
            Graph &gg = *pend[i].gr;
            const UgsBpMissOut &o = h_out[i];
            const int64_t n = gg.n;
            std::lock_guard<std::mutex> lk(gg.pre_mu);
            if (!gg.host_ready) {                                        // (a host path that met the stub meanwhile has filled in the same values)
                gg.level = o.level; gg.n_viable = o.n_viable; gg.nonzero = o.nonzero; gg.Z = o.Z; gg.max_deg = o.max_deg; gg.sb_deg = o.sb_deg;
            }
            if (o.level == 0) { gg.dev_roots.push_back(Graph::DevRoots{dc.id, pend[i].roots_off, n, -1, 0}); arena_release(dc.id, -1, 0, pend[i].via_off, n); }
            else { gg.dev_roots.push_back(Graph::DevRoots{dc.id, -1, 0, pend[i].via_off, n}); arena_release(dc.id, pend[i].roots_off, n, -1, 0); }
        }
        for (int64_t g = 0; g < G; ++g) {
            if (pend_of[(size_t)g] < 0) continue;
            const Pending &pd = pend[(size_t)pend_of[(size_t)g]];
            const Graph &gg = *pd.gr;
            UgsGraphDesc &d = desc[(size_t)g];
            d.n = (int32_t)gg.n; d.level = gg.level; d.n_viable = (int32_t)gg.n_viable;
            d.vbase = gg.level == 0 ? pd.roots_off : 0; d.viable_base = gg.level > 0 ? pd.via_off : 0;
            p->g_n[(size_t)g] = gg.n; p->g_maxdeg[(size_t)g] = gg.max_deg; p->g_sbdeg[(size_t)g] = gg.sb_deg; p->g_level[(size_t)g] = gg.level;
        }
        pend.clear();
    }
    for (int64_t h : evicted) drop(h);                                   // only evicted handles are destroyed; cached ones live on
    evicted.clear();
    if (debug_on()) {
        std::lock_guard<std::mutex> lk(g_lru_mu);
        std::fprintf(stderr, "[UGS CACHE] hits=%lld misses=%lld cache_size=%zu\n", (long long)hits, (long long)misses, lru().items.size());
    }
    const double t_lru = lap();
    e = hipMemcpyAsync(base + o_desc, desc, desc_bytes, hipMemcpyHostToDevice, s);      // pinned source: truly asynchronous; the plan's first
    if (e == hipSuccess) e = hipEventRecord(ar->desc_ev[slot], s);                        // walk is ordered behind it on the plan (plan_enter)
    if (e != hipSuccess) return bail(fail_hip(e, "plan descriptors"));
    if (int rc = plan_leave(p, s)) return bail(rc);                      // a first call on another stream waits for the descriptors (plan_enter)
    if (std::getenv("UGS_BP_TRACE"))
        std::fprintf(stderr, "[UGS BATCH PASS] G=%lld E=%lld: upload + pass + keys back %.1f us, LRU replay + arena %.1f us, descriptors %.1f us\n",
                     (long long)G, (long long)E, t_pass * 1e6, t_lru * 1e6, lap() * 1e6);
    for (auto &gr : graphs) if (gr) p->keep.push_back(gr);
    p->device = dc.id; p->cus = dc.cus;
    p->G = G; p->nverts = nv; p->nnz = 2 * owned_cols;
    p->blob = base; p->blob_bytes = off;
    p->dev.graphs = reinterpret_cast<const UgsGraphDesc *>(base + o_desc);
    p->dev.rowptr = reinterpret_cast<const int64_t *>(base + o_row);
    p->dev.adj = reinterpret_cast<const int2 *>(base + o_adj);
    p->dev.adjf = reinterpret_cast<const int2 *>(base + o_adjf);
    p->dev.roots = ar->roots;
    p->dev.viable = ar->via;
    p->dev.num_graphs = G;
    p->prow_failed = true;                       // vbase indexes the arena, not a per-plan vertex range: these plans read rows through rowptr
    if (have_hash) {
        p->cache_key = mum(bh.a ^ 0x6a09e667f3bcc909ull, bh.b ^ (uint64_t)k) ^ 0xd6e8feb86659fd93ull;
        plan_cache_put(p);
    }
    *plan_out = p;
    return UGS_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
extern "C" {

const char *ugs_last_error(void) { return t_err.c_str(); }
const char *ugs_version(void) { return "ugs-mi355 0.1 (gfx950)"; }

int ugs_device_count(int *count) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) { if (count) *count = 0; return fail(UGS_E_NO_DEVICE, std::string("no usable HIP device: ") + hipGetErrorString(e)); }
    if (count) *count = c;
    return UGS_OK;
}

int ugs_set_device(int device) {
    int c = 0;
    if (int rc = ugs_device_count(&c)) return rc;
    if (device < 0 || device >= c) return fail(UGS_E_BAD_ARG, "device index out of range");
    t_device = device;
    HIP_TRY(hipSetDevice(device));
    return UGS_OK;
}

int ugs_set_stream(void *stream, int use) {
    t_job_stream = static_cast<hipStream_t>(stream);
    t_job_stream_set = use != 0;
    return UGS_OK;
}

int ugs_create_preproc(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, int64_t num_nodes, int k, int64_t *handle_out) {
    if (!handle_out || (num_cols > 0 && !edge_index) || num_cols < 0) return fail(UGS_E_BAD_ARG, "bad arguments to create_preproc");
    std::shared_ptr<Graph> g;
    if (int rc = make_graph(edge_index, edge_index + row_stride, num_cols, num_nodes, k, g)) return rc;
    *handle_out = enroll(std::move(g));
    return UGS_OK;
}

int ugs_destroy_preproc(int64_t handle) { drop(handle); return UGS_OK; }

int ugs_has_graphlets(int64_t handle, int *out) {
    auto g = lookup(handle);
    if (out) *out = (g && g->Z > 0.0) ? 1 : 0;
    return UGS_OK;
}

int ugs_get_preproc_info(int64_t handle, int *found, int64_t *num_nodes, int64_t *num_edges_stored, double *Z, int *bucket_count_nonzero) {
    auto g = lookup(handle);
    if (found) *found = g ? 1 : 0;
    if (!g) return UGS_OK;
    if (num_nodes) *num_nodes = g->n;
    if (num_edges_stored) *num_edges_stored = g->nnz;
    if (Z) *Z = g->Z;
    if (bucket_count_nonzero) *bucket_count_nonzero = g->nonzero;
    return UGS_OK;
}

int ugs_preproc_dump(int64_t handle, int64_t *indptr, int32_t *indices, int32_t *edge_col, int32_t *order, int32_t *index_of,
                     int32_t *suffix_deg, double *bucket_b, double *prob, int32_t *alias) {
    auto g = lookup(handle);
    if (!g) return fail(UGS_E_INVALID_HANDLE, "Invalid preproc handle");
    if (!g->host_ready) complete_on_host(*g);
    const size_t n = (size_t)g->n, nnz = (size_t)g->nnz;
    if (indptr) std::memcpy(indptr, g->rowptr.data(), (n + 1) * sizeof(int64_t));
    if (indices && nnz) std::memcpy(indices, g->nbr.data(), nnz * sizeof(int32_t));
    if (edge_col && nnz) std::memcpy(edge_col, g->col.data(), nnz * sizeof(int32_t));
    if (order && n) std::memcpy(order, g->order.data(), n * sizeof(int32_t));
    if (index_of && n) std::memcpy(index_of, g->rank.data(), n * sizeof(int32_t));
    if (suffix_deg && n) std::memcpy(suffix_deg, g->sdeg.data(), n * sizeof(int32_t));
    if (bucket_b && n) std::memcpy(bucket_b, g->weight.data(), n * sizeof(double));
    if (prob && n) std::memcpy(prob, g->prob.data(), n * sizeof(double));
    if (alias && n) std::memcpy(alias, g->alias.data(), n * sizeof(int32_t));
    return UGS_OK;
}

int ugs_cache_clear(void) {
    {
        std::lock_guard<std::mutex> lk(g_lru_mu);
        Lru &c = lru();
        for (auto &kv : c.items) drop(kv.second);
        c.items.clear(); c.index.clear(); c.hits = c.misses = 0;
    }
    plan_cache_clear();
    batch_index_clear();
    return UGS_OK;
}

int ugs_set_batch_pass_max_cols(int64_t cols, int64_t *previous_out) {
    const int64_t cur = batch_pass_max_cols();                          // the environment's value first, so that it cannot overwrite this one later
    if (cols < UGS_BATCH_PASS_MAX_COLS || cols > UGS_BATCH_PASS_COLS_CEIL)
        return fail(UGS_E_BAD_ARG, "batch pass column limit must be " + std::to_string(UGS_BATCH_PASS_MAX_COLS) + " ... " + std::to_string(UGS_BATCH_PASS_COLS_CEIL) +
                                       " (got " + std::to_string(cols) + ", still " + std::to_string(cur) + ")");
    const int64_t prev = g_bp_max_cols.exchange(cols);
    if (previous_out) *previous_out = prev;
    return UGS_OK;
}
int64_t ugs_batch_pass_max_cols(void) { return batch_pass_max_cols(); }

int ugs_batch_pass_stats(int64_t *device_plans, int64_t *general_path) {
    if (device_plans) *device_plans = g_bp_plans.load();
    if (general_path) *general_path = g_bp_fallbacks.load();
    return UGS_OK;
}

int ugs_preproc_stats(int64_t *device_graphs, int64_t *host_graphs, int64_t *device_pieces) {
    if (device_graphs) *device_graphs = g_pre_device_graphs.load();
    if (host_graphs) *host_graphs = g_pre_host_graphs.load();
    if (device_pieces) *device_pieces = g_pre_device_pieces.load();
    return UGS_OK;
}

int ugs_cache_stats(int64_t *size, int64_t *hits, int64_t *misses) {
    std::lock_guard<std::mutex> lk(g_lru_mu);
    Lru &c = lru();
    if (size) *size = (int64_t)c.items.size();
    if (hits) *hits = c.hits;
    if (misses) *misses = c.misses;
    return UGS_OK;
}

// ---- plans ------------------------------------------------------------------------------------------------------
int ugs_plan_create_handle(int64_t handle, ugs_plan **plan_out) {
    if (!plan_out) return fail(UGS_E_BAD_ARG, "plan_out is null");
    auto g = lookup(handle);
    if (!g) return fail(UGS_E_INVALID_HANDLE, "Invalid preproc handle");
    if (!g->host_ready) complete_on_host(*g);
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    std::lock_guard<std::mutex> lk(g->plan_mu);
    if (g->plan && g->plan->device == dc.id) { g->plan->refs.fetch_add(1); *plan_out = g->plan; return UGS_OK; }
    auto *p = new ugs_plan();
    p->handle_api = true;
    std::vector<PlanPiece> pieces(1);
    pieces[0].g = g;                       // note: the plan keeps the Graph alive only through its arrays on the device
    if (int rc = assemble_plan(pieces, dc, p)) { delete p; return rc; }
    if (!g->plan) { g->plan = p; p->refs.fetch_add(1); }
    *plan_out = p;
    return UGS_OK;
}

int ugs_plan_create_batch(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                          int k, ugs_plan **plan_out) {
    if (!plan_out || !ptr || num_graphs < 0 || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    if (num_cols >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: columns must be < 2^31 - 1");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    const int64_t G = num_graphs, E = num_cols;
    const int64_t *src = edge_index, *dst = edge_index + row_stride;
    // the batch as a whole: seen before, and everything it needs still cached?
    const bool use_index = std::getenv("UGS_NO_BATCH_INDEX") == nullptr;
    Hash128 bh{0, 0};
    Witness wit{};
    if (use_index) {
        bh = batch_hash(src, dst, E, ptr, G);
        wit = batch_witness(src, dst, E, ptr, G);
        BatchEntry found;
        bool have = false;
        {
            std::lock_guard<std::mutex> lk(g_bi_mu);
            for (auto it = g_batch_index.begin(); it != g_batch_index.end(); ++it)
                if (it->h == bh && it->E == E && it->G == G && it->k == k && it->dev == dc.id && it->wit == wit) {
                    g_batch_index.splice(g_batch_index.begin(), g_batch_index, it);
                    found = *it; have = true;
                    break;
                }
        }
        if (have) {
            int64_t hits = 0;
            if (batch_replay(found, hits)) {
                if (ugs_plan *cached = plan_cache_get(found.plan_key, dc.id)) {
                    if (debug_on()) {
                        std::lock_guard<std::mutex> lk(g_lru_mu);
                        std::fprintf(stderr, "[UGS CACHE] hits=%lld misses=0 cache_size=%zu\n", (long long)hits, lru().items.size());
                    }
                    *plan_out = cached;
                    return UGS_OK;
                }
            }
            // fall through: the general path repeats the lookups (same final recency order); undo the hits counted above
            std::lock_guard<std::mutex> lk(g_lru_mu);
            lru().hits -= hits;
        }
    }
    const int bp_mode = device_batch_mode();
    // A workload the pass cannot take (a graph beyond its limits in every batch, a full arena) would pay upload + pass + wait before
    // every general-path call: after three refusals in a row the default mode leaves the pass alone for the next 64 calls.
    static std::atomic<int> bp_refused{0}, bp_pause{0};
    const bool bp_paused = bp_mode == 2 && bp_pause.load() > 0 && bp_pause.fetch_sub(1) > 0;
    if (!bp_paused && (bp_mode == 1 || (bp_mode == 2 && E >= kBatchPassMinCols))) {   // batches of small graphs: slicing, keys and CSR on the device
        std::vector<std::pair<uint64_t, int64_t>> touched_d;
        ugs_plan *dp = nullptr;
        const int rc = device_batch_plan(src, dst, E, ptr, G, k, dc, use_index, bh, &dp, touched_d);
        if (rc == UGS_OK) {
            bp_refused.store(0);
            g_bp_plans.fetch_add(1);
            if (use_index) {
                std::lock_guard<std::mutex> lk(g_bi_mu);
                for (auto it = g_batch_index.begin(); it != g_batch_index.end(); ++it)
                    if (it->h == bh && it->E == E && it->G == G && it->k == k && it->dev == dc.id) { g_batch_index.erase(it); break; }
                g_batch_index.push_front(BatchEntry{bh, E, G, k, dc.id, dp->cache_key, std::move(touched_d), wit});
                while (g_batch_index.size() > g_plan_cache_cap) g_batch_index.pop_back();
            }
            *plan_out = dp;
            return UGS_OK;
        }
        if (rc != kBatchNotApplicable) return rc;
        g_bp_fallbacks.fetch_add(1);
        if (bp_refused.fetch_add(1) + 1 >= 3) { bp_refused.store(0); bp_pause.store(64); }
    }
    std::vector<int64_t> cstart, cols_of;                      // per-graph column lists, concatenated
    Lap lap;
    assign_columns(src, dst, E, ptr, G, cstart, cols_of);
    const double t_assign = lap();
    // --- per graph: renumber, hash, LRU lookup / preprocessing ------------------------------------------------------
    std::vector<PlanPiece> pieces((size_t)G);
    std::vector<std::pair<uint64_t, int64_t>> touched;          // (LRU key, handle) per non-degenerate graph, for the batch index
    std::vector<int64_t> ru, rv, evicted;
    uint64_t pkey = 14695981039346656037ull;
    const uint64_t prime = 1099511628211ull;
    auto mix = [&](uint64_t x) { pkey = (pkey ^ x) * prime; };
    mix((uint64_t)G);
    int64_t hits = 0, misses = 0;
    for (int64_t g = 0; g < G; ++g) {
        PlanPiece &pc = pieces[(size_t)g];
        const int64_t lo = ptr[g], hi = ptr[g + 1], n = hi - lo;
        pc.lo = lo;
        mix((uint64_t)lo);
        if (n <= 0 || n < k) { mix(0x9e3779b97f4a7c15ull); continue; }        // degenerate: m rows of -1
        const int64_t c0 = cstart[(size_t)g], cn = cstart[(size_t)g + 1] - c0;
        ru.resize((size_t)cn); rv.resize((size_t)cn);
        for (int64_t t = 0; t < cn; ++t) { const int64_t j = cols_of[(size_t)(c0 + t)]; ru[(size_t)t] = src[j] - lo; rv[(size_t)t] = dst[j] - lo; }
        const uint64_t key = graph_key(ru.data(), rv.data(), cn, n);
        int64_t handle = 0;
        bool hit;
        {
            std::lock_guard<std::mutex> lk(g_lru_mu);
            hit = lru().get(key, handle);
            if (hit) ++lru().hits; else ++lru().misses;
        }
        std::shared_ptr<Graph> gr = hit ? lookup(handle) : nullptr;
        if (!gr) {
            if (int rc = make_graph(ru.data(), rv.data(), cn, n, k, gr)) return rc;
            handle = enroll(gr);
            int64_t ev = 0;
            std::lock_guard<std::mutex> lk(g_lru_mu);
            if (lru().put(key, handle, ev)) evicted.push_back(ev);
            ++misses;
        } else {
            ++hits;
            if (!gr->host_ready) complete_on_host(*gr);
        }
        pc.g = gr;
        touched.emplace_back(key, handle);
        pc.colmap = cols_of.data() + c0;
        pc.ncols = cn;
        mix((uint64_t)handle); mix((uint64_t)cn);
        for (int64_t t = 0; t < cn; ++t) mix((uint64_t)cols_of[(size_t)(c0 + t)]);
    }
    for (int64_t h : evicted) drop(h);          // only evicted handles are destroyed; cached ones live on
    if (debug_on()) {
        std::lock_guard<std::mutex> lk(g_lru_mu);
        std::fprintf(stderr, "[UGS CACHE] hits=%lld misses=%lld cache_size=%zu\n", (long long)hits, (long long)misses, lru().items.size());
    }
    auto remember = [&] {
        if (!use_index) return;
        std::lock_guard<std::mutex> lk(g_bi_mu);
        for (auto it = g_batch_index.begin(); it != g_batch_index.end(); ++it)
            if (it->h == bh && it->E == E && it->G == G && it->k == k && it->dev == dc.id) { g_batch_index.erase(it); break; }
        g_batch_index.push_front(BatchEntry{bh, E, G, k, dc.id, pkey, std::move(touched), wit});
        while (g_batch_index.size() > g_plan_cache_cap) g_batch_index.pop_back();
    };
    if (ugs_plan *cached = plan_cache_get(pkey, dc.id)) { remember(); *plan_out = cached; return UGS_OK; }
    const double t_graphs = lap();
    auto *p = new ugs_plan();
    p->cache_key = pkey;
    if (int rc = assemble_plan(pieces, dc, p)) { delete p; return rc; }
    if (debug_on() && E >= ((int64_t)1 << 21))
        std::fprintf(stderr, "[UGS PLAN] columns -> graphs %.3fs, renumber + hash + preprocessing %.3fs, assemble + upload %.3fs\n", t_assign, t_graphs, lap());
    plan_cache_put(p);
    remember();
    *plan_out = p;
    return UGS_OK;
}

int ugs_plan_release(ugs_plan *plan) { plan_unref(plan); return UGS_OK; }

int ugs_plan_graph_roots(ugs_plan *plan, int64_t graph, int64_t capacity, int32_t *level, int32_t *num_nodes, int32_t *num_viable, double *prob,
                         int32_t *alias, int32_t *v_self, int32_t *v_alias, int32_t *viable_vi, int32_t *viable_v) {
    if (!plan || graph < 0 || graph >= plan->G) return fail(UGS_E_BAD_ARG, "graph index outside the plan");
    HIP_TRY(hipSetDevice(plan->device));
    UgsGraphDesc d{};
    {
        std::lock_guard<std::mutex> lk(plan->mu);
        if (plan->last_valid) HIP_TRY(hipEventSynchronize(plan->last_ev));
        HIP_TRY(hipMemcpy(&d, plan->dev.graphs + graph, sizeof(d), hipMemcpyDeviceToHost));
    }
    if (level) *level = d.level;
    if (num_nodes) *num_nodes = d.n;
    if (num_viable) *num_viable = d.n_viable;
    if (d.level == 0 && d.n > 0 && (prob || alias || v_self || v_alias)) {
        if (capacity < d.n) return fail(UGS_E_BAD_ARG, "capacity below the graph's vertex count");
        std::vector<UgsRootRec> rec((size_t)d.n);
        HIP_TRY(hipMemcpy(rec.data(), plan->dev.roots + d.vbase, rec.size() * sizeof(UgsRootRec), hipMemcpyDeviceToHost));
        for (int32_t vi = 0; vi < d.n; ++vi) {
            if (prob) prob[vi] = rec[(size_t)vi].prob;
            if (alias) alias[vi] = rec[(size_t)vi].alias;
            if (v_self) v_self[vi] = rec[(size_t)vi].v_self;
            if (v_alias) v_alias[vi] = rec[(size_t)vi].v_alias;
        }
    } else if (d.level > 0 && d.n_viable > 0 && (viable_vi || viable_v)) {
        if (capacity < d.n_viable) return fail(UGS_E_BAD_ARG, "capacity below the viable list's length");
        std::vector<int2> v((size_t)d.n_viable);
        HIP_TRY(hipMemcpy(v.data(), plan->dev.viable + d.viable_base, v.size() * sizeof(int2), hipMemcpyDeviceToHost));
        for (int32_t t = 0; t < d.n_viable; ++t) { if (viable_vi) viable_vi[t] = v[(size_t)t].x; if (viable_v) viable_v[t] = v[(size_t)t].y; }
    }
    return UGS_OK;
}

int ugs_plan_graph_csr(ugs_plan *plan, int64_t graph, int64_t node_capacity, int64_t entry_capacity, int32_t *num_nodes, int64_t *num_entries,
                       int64_t *rowptr, int32_t *nbr, int32_t *nbr_rank, int32_t *nbr_f, int32_t *nbr_col) {
    if (!plan || graph < 0 || graph >= plan->G) return fail(UGS_E_BAD_ARG, "graph index outside the plan");
    HIP_TRY(hipSetDevice(plan->device));
    UgsGraphDesc d{};
    {
        std::lock_guard<std::mutex> lk(plan->mu);
        if (plan->last_valid) HIP_TRY(hipEventSynchronize(plan->last_ev));
        HIP_TRY(hipMemcpy(&d, plan->dev.graphs + graph, sizeof(d), hipMemcpyDeviceToHost));
    }
    if (d.level < 0 || d.n <= 0) { if (num_nodes) *num_nodes = 0; if (num_entries) *num_entries = 0; return UGS_OK; }
    std::vector<int64_t> rp((size_t)d.n + 1);
    HIP_TRY(hipMemcpy(rp.data(), plan->dev.rowptr + d.rbase, rp.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t nnz = rp[(size_t)d.n] - rp[0];
    if (num_nodes) *num_nodes = d.n;
    if (num_entries) *num_entries = nnz;
    if (rowptr) {
        if (node_capacity < d.n) return fail(UGS_E_BAD_ARG, "capacity below the graph's vertex count");
        for (int32_t x = 0; x <= d.n; ++x) rowptr[x] = rp[(size_t)x] - rp[0];
    }
    if (nnz > 0 && (nbr || nbr_rank || nbr_f || nbr_col)) {
        if (entry_capacity < nnz) return fail(UGS_E_BAD_ARG, "capacity below the graph's entry count");
        std::vector<int2> a((size_t)nnz), f((size_t)nnz);
        HIP_TRY(hipMemcpy(a.data(), plan->dev.adj + rp[0], a.size() * sizeof(int2), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(f.data(), plan->dev.adjf + rp[0], f.size() * sizeof(int2), hipMemcpyDeviceToHost));
        for (int64_t e = 0; e < nnz; ++e) {
            if (nbr) nbr[e] = a[(size_t)e].x;
            if (nbr_rank) nbr_rank[e] = a[(size_t)e].y;
            if (nbr_f) nbr_f[e] = f[(size_t)e].x;
            if (nbr_col) nbr_col[e] = f[(size_t)e].y;
        }
    }
    return UGS_OK;
}

int ugs_plan_info(const ugs_plan *plan, int k, int64_t *num_graphs, int64_t *num_vertices, int64_t *nnz, int64_t *device_bytes, int *tier) {
    if (!plan) return fail(UGS_E_BAD_ARG, "plan is null");
    if (num_graphs) *num_graphs = plan->G;
    if (num_vertices) *num_vertices = plan->nverts;
    if (nnz) *nnz = plan->nnz;
    if (device_bytes) *device_bytes = (int64_t)(plan->blob_bytes + plan->prow_asked);
    if (tier) *tier = choose_tier(const_cast<ugs_plan *>(plan), k).first;
    return UGS_OK;
}

int ugs_plan_first_pick_table(ugs_plan *plan, int64_t capacity, int64_t *num_vertices, int32_t *c1, uint8_t *ord1) {
    if (!plan || !num_vertices) return fail(UGS_E_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(plan->device));
    std::lock_guard<std::mutex> lk(plan->mu);
    *num_vertices = plan->ord1 ? plan->nverts : 0;
    if (!plan->ord1 || (!c1 && !ord1)) return UGS_OK;
    if (capacity < plan->nverts) return fail(UGS_E_BAD_ARG, "capacity below the plan's vertices");
    const size_t nv = (size_t)plan->nverts;
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (ord1) HIP_TRY(hipMemcpy(ord1, plan->ord1, nv * UGS_ORD1_BYTES, hipMemcpyDeviceToHost));       // the table the walks read
    if (c1) {                                   // the candidate counts are not kept: the build kernel once more, into scratch
        void *tmp = nullptr;
        HIP_TRY(hipMalloc(&tmp, nv * (UGS_ORD1_BYTES + sizeof(int32_t))));
        uint8_t *o = static_cast<uint8_t *>(tmp);
        int32_t *c = reinterpret_cast<int32_t *>(o + nv * UGS_ORD1_BYTES);
        hipError_t e = hipMemsetAsync(tmp, 0, nv * (UGS_ORD1_BYTES + sizeof(int32_t)), dc.stream);
        if (e == hipSuccess) e = ugs_launch_build_ord1(plan->dev, plan->nverts, o, c, plan->cus, dc.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
        if (e == hipSuccess) e = hipMemcpy(c1, c, nv * sizeof(int32_t), hipMemcpyDeviceToHost);
        (void)hipFree(tmp);
        if (e != hipSuccess) return fail_hip(e, "first-pick table read-back");
    }
    return UGS_OK;
}

static int plan_walk_impl(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed, const uint64_t *d_seed_ptr,
                          const uint64_t *d_seeds, int64_t row_begin, int64_t row_count, void *stream, int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *total_edges_host,
                          bool *defer_scan = nullptr, bool poll_total = false);
static int plan_walk_locked(ugs_plan *plan, const TierChoice &tc, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed,
                            const uint64_t *d_seed_ptr, const uint64_t *d_seeds, int64_t row_begin, int64_t row_count, hipStream_t s, int64_t *d_nodes, int64_t *d_edge_ptr,
                            int64_t *total_edges_host, bool *defer_scan, bool poll_total);


int ugs_plan_walk(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed, int64_t row_begin,
                  int64_t row_count, void *stream, int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *total_edges_host) {
    return plan_walk_impl(plan, m_per_graph, k, mode, extra_node_offset, seed, nullptr, nullptr, row_begin, row_count, stream, d_nodes, d_edge_ptr, total_edges_host);
}

// the argument checks of a walk; its device made current
static int walk_check(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t row_begin, int64_t row_count, const int64_t *d_nodes,
                      const int64_t *d_edge_ptr) {
    if (!plan) return fail(UGS_E_BAD_ARG, "plan is null");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0 || row_begin < 0 || row_count < 0 || row_begin + row_count > plan->G * (int64_t)m_per_graph)
        return fail(UGS_E_BAD_ARG, "row range outside [0, num_graphs * m_per_graph)");
    if (row_count > 0 && (!d_nodes || !d_edge_ptr)) return fail(UGS_E_BAD_ARG, "null output pointer");
    HIP_TRY(hipSetDevice(plan->device));
    return UGS_OK;
}

// defer_scan (ugs_plan_step): where the fill kernel can turn the counts into edge_ptr itself -- first tier S (rows are filled from
// their adjacency, nothing is staged), no capture in progress -- the scan launch is left out and *defer_scan set.  The caller then
// launches that fill without letting go of plan->mu in between (plan_walk_locked).
static int plan_walk_impl(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed, const uint64_t *d_seed_ptr,
                          const uint64_t *d_seeds, int64_t row_begin, int64_t row_count, void *stream, int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *total_edges_host,
                          bool *defer_scan, bool poll_total) {
    if (defer_scan) *defer_scan = false;
    if (int rc = walk_check(plan, m_per_graph, k, mode, row_begin, row_count, d_nodes, d_edge_ptr)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (row_count == 0) {
        if (d_edge_ptr) HIP_TRY(hipMemsetAsync(d_edge_ptr, 0, sizeof(int64_t), s));
        if (total_edges_host) { HIP_TRY(hipStreamSynchronize(s)); *total_edges_host = 0; }
        return UGS_OK;
    }
    const TierChoice tc = choose_tier(plan, k);
    std::lock_guard<std::mutex> lk(plan->mu);
    return plan_walk_locked(plan, tc, m_per_graph, k, mode, extra_node_offset, seed, d_seed_ptr, d_seeds, row_begin, row_count, s, d_nodes, d_edge_ptr,
                            total_edges_host, defer_scan, poll_total);
}

// The walk of rows [row_begin, row_begin + row_count), row_count > 0, arguments checked (walk_check).  Call with plan->mu held and
// tc = choose_tier(plan, k) taken before the lock (choose_tier takes mu itself).  With *defer_scan set on return the plan's counts
// and 8-row sums are this walk's only while the caller keeps holding mu: a fill that scans them is launched before it lets go.
static int plan_walk_locked(ugs_plan *plan, const TierChoice &tc, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed,
                            const uint64_t *d_seed_ptr, const uint64_t *d_seeds, int64_t row_begin, int64_t row_count, hipStream_t s, int64_t *d_nodes, int64_t *d_edge_ptr,
                            int64_t *total_edges_host, bool *defer_scan, bool poll_total) {
    if (defer_scan) *defer_scan = false;
    if (int rc = plan_enter(plan, s)) return rc;
    plan->stg_valid = false;                    // before any scratch is regrown: a walk that fails below leaves no staging record behind
    if (int rc = ensure(plan->counts, (size_t)row_count * sizeof(uint32_t), plan->device, plan)) return rc;
    if (int rc = ensure(plan->scantmp, (size_t)ugs_scan_tmp_words(row_count) * sizeof(int64_t), plan->device, plan)) return rc;
    if (int rc = ensure(plan->ovfcnt, 4 * sizeof(uint32_t), plan->device, plan)) return rc;
    const bool may_overflow = tc.second >= 0 || tc.third_G;
    if (may_overflow) {
        if (int rc = ensure(plan->ovf1, (size_t)row_count * sizeof(int64_t), plan->device, plan)) return rc;
        if (int rc = ensure(plan->ovf2, (size_t)row_count * sizeof(int64_t), plan->device, plan)) return rc;
    }
    // edge staging by the walk (tiers with one walk per wave): 512 bytes of scratch per row, bounded
    const int64_t stage_max = [] { const char *e = std::getenv("UGS_STAGE_MAX_MB"); return (int64_t)(e ? std::atoll(e) : 4096) << 20; }();   // read per call (tests toggle it)
    const bool stg = tc.first != UGS_TIER_S && row_count * (int64_t)(UGS_STAGE_ITEMS * sizeof(uint2)) <= stage_max;
    if (stg) {
        if (int rc = ensure(plan->stage, (size_t)row_count * UGS_STAGE_ITEMS * sizeof(uint2), plan->device, plan)) return rc;
        if (int rc = ensure(plan->ulist, (size_t)row_count * sizeof(int64_t), plan->device, plan)) return rc;
    }
    if (may_overflow || stg) HIP_TRY(hipMemsetAsync(plan->ovfcnt.p, 0, 4 * sizeof(uint32_t), s));   // nothing else reads the counters
    // dynamic work distribution pays when a launch has many more walks than resident groups (its counter costs one memset)
    const bool dyn = row_count > (int64_t)plan->cus * (tc.first == UGS_TIER_S ? 1024 : 64) && std::getenv("UGS_STATIC_SPLIT") == nullptr;
    if (dyn) {
        if (int rc = ensure(plan->work, 4 * sizeof(unsigned long long), plan->device, plan)) return rc;
        HIP_TRY(hipMemsetAsync(plan->work.p, 0, 4 * sizeof(unsigned long long), s));
    }
    if ((tc.first != UGS_TIER_S && tc.first != UGS_TIER_G) || tc.second >= 0)
        if (int rc = ensure_prow(plan, s)) return rc;
    uint32_t *cnt = static_cast<uint32_t *>(plan->ovfcnt.p);
    UgsWalkArgs a{};
    a.plan = plan->dev;
    a.m = m_per_graph; a.k = k; a.mode = mode;
    a.extra_node_off = extra_node_offset;
    a.seed64 = (uint64_t)(int64_t)seed;
    a.seed_ptr = d_seed_ptr;
    a.seeds = d_seeds;
    a.ord1 = env_is_one("UGS_NO_FIRST_PICK_TABLE") ? nullptr : plan->ord1;     // (read per call: tests and A/Bs toggle it)
    a.row_begin = row_begin; a.row_count = row_count;
    a.nodes = d_nodes;
    a.counts = static_cast<uint32_t *>(plan->counts.p);
    a.in_list = nullptr; a.in_count = nullptr;
    a.ovf_list = static_cast<int64_t *>(plan->ovf1.p);
    a.ovf_count = cnt + 0;
    if (stg) {
        a.stage = static_cast<uint2 *>(plan->stage.p);
        a.ulist = static_cast<int64_t *>(plan->ulist.p); a.ucount = cnt + 3;
        plan->stg_valid = true; plan->stg_nodes = d_nodes; plan->stg_row_begin = row_begin; plan->stg_row_count = row_count;
        plan->stg_m = m_per_graph; plan->stg_k = k;
    }
    a.work_next = dyn ? static_cast<unsigned long long *>(plan->work.p) + 0 : nullptr;
    if (tc.small) a.pad = UGS_SMALL_CAP;
    if (tc.wide && !dyn && std::getenv("UGS_NO_WIDE_TIER") == nullptr /* read per call: tests and A/Bs toggle it */ && row_count <= (int64_t)plan->cus * 3 /* blocks per CU, UGS_BLOCKS_S */ * UGS_WIDE_LANES) a.pad |= UGS_WIDE_LANES;       // (UGS_SMALL_CAP | UGS_WIDE_LANES: both)
    // ugs_plan_step: the fill kernel can turn the counts into edge_ptr itself when the walk leaves the sums of 8 rows beside them --
    // 8-lane tier, rows taken by index (static split), no walk handed on, no capture in progress, a row count the fill's blocks can
    // add up in a few dozen loads per thread
    const bool defer = defer_scan && tc.first == UGS_TIER_S && !may_overflow && !dyn && row_count <= 131072 && !capturing(s) &&
                       std::getenv("UGS_NO_FUSED_SCAN") == nullptr;
    if (defer) {
        if (int rc = ensure(plan->tiles, std::max<size_t>((size_t)((row_count + 7) / 8) * sizeof(uint32_t), 4096), plan->device, plan)) return rc;
        a.wsum = static_cast<uint32_t *>(plan->tiles.p);
    }
    HIP_TRY(ev_begin(plan, 0, s));
    HIP_TRY(ugs_launch_walk(a, tc.first, plan->cus, plan->walk_share, s, &plan->last_walk));
    HIP_TRY(ev_end(plan, s));
    HIP_TRY(ev_begin(plan, 1, s));
    int last = 0;   // index of the counter holding rows that nobody processed
    if (tc.second >= 0) {
        a.in_list = static_cast<const int64_t *>(plan->ovf1.p); a.in_count = cnt + 0;
        a.ovf_list = static_cast<int64_t *>(plan->ovf2.p); a.ovf_count = cnt + 1;
        a.work_next = dyn ? static_cast<unsigned long long *>(plan->work.p) + 1 : nullptr;
        HIP_TRY(ugs_launch_walk(a, tc.second, plan->cus, plan->walk_share, s, nullptr));
        last = 1;
    }
    if (tc.third_G) {
        if (!plan->gws.p) {
            int idx = 0;
            const int64_t gcap = std::max<int64_t>(tc.bound, 1);
            const uint32_t gb = ugs_chain_at_least(gcap, &idx);
            if (!gb) return fail(UGS_E_UNSUPPORTED, "candidate-set bound too large");
            const int64_t prev = std::max<int64_t>(ugs_ord_words(idx), 4);            // orders of every stage below the last one
            int64_t hs = 128;
            while (hs < 2 * (gcap + 65 + 1)) hs <<= 1;
            const int64_t words = ugs_global_ws_words(gcap, gb, prev, hs);
            int64_t groups = std::min<int64_t>(256, std::max<int64_t>(1, ((int64_t)4 << 30) / (words * 4)));
            if (words * 4 > ((int64_t)16 << 30)) return fail(UGS_E_UNSUPPORTED, "candidate-set bound too large for the global-memory workspace");
            void *w = nullptr;
            HIP_TRY(hipMalloc(&w, (size_t)(words * groups) * sizeof(uint32_t)));
            plan->gws.p = w; plan->gws.bytes = (size_t)(words * groups) * 4; plan->gws.dev = plan->device;
            plan->gws_groups = groups; plan->gws_words = words;
            plan->gcap = (int)gcap; plan->gbcap = (int)gb; plan->gpcap = (int)prev; plan->ghs = (int)hs;
        }
        a.in_list = static_cast<const int64_t *>(last == 0 ? plan->ovf1.p : plan->ovf2.p); a.in_count = cnt + last;
        a.ovf_list = static_cast<int64_t *>(last == 0 ? plan->ovf2.p : plan->ovf1.p); a.ovf_count = cnt + 2;
        a.gws = static_cast<uint32_t *>(plan->gws.p);
        a.gws_words_per_group = plan->gws_words; a.gws_groups = plan->gws_groups;
        a.gcap = plan->gcap; a.ghs = plan->ghs; a.gbcap = plan->gbcap; a.gpcap = plan->gpcap;
        a.work_next = nullptr;              // the global tier keeps one walk per workspace slice, static
        HIP_TRY(ugs_launch_walk(a, UGS_TIER_G, plan->cus, plan->walk_share, s, nullptr));
        last = 2;
    }
    // the library's own jobs (poll_total): the scan kernel hands the total to the host and the host polls for it -- the caller of the job
    // API gets its outputs from later operations on the same stream, so nothing else needs the stream to be idle here.  Not while rows
    // may have been handed on (the overflow counters are read back with the total) and not under UGS_DEBUG.
    bool polled = false;
    if (poll_total && total_edges_host && !may_overflow && !debug_on() && !capturing(s) && !defer) {
        if (!plan->pin_slot) plan->pin_slot = pin_slot_get();
        polled = plan->pin_slot != nullptr;
    }
    if (defer) *defer_scan = true;
    else if (polled) {
        uint32_t ep = g_pin_epoch.fetch_add(1) + 1;
        if (ep == 0) ep = g_pin_epoch.fetch_add(1) + 1;
        plan->pin_epoch = ep;
        HIP_TRY(ugs_launch_scan(static_cast<const uint32_t *>(plan->counts.p), row_count, d_edge_ptr, static_cast<int64_t *>(plan->scantmp.p), s,
                                reinterpret_cast<int64_t *>(plan->pin_slot), reinterpret_cast<uint32_t *>(plan->pin_slot + 8), ep));
    } else HIP_TRY(ugs_launch_scan(static_cast<const uint32_t *>(plan->counts.p), row_count, d_edge_ptr, static_cast<int64_t *>(plan->scantmp.p), s));
    HIP_TRY(ev_end(plan, s));
    if (int rc = plan_leave(plan, s)) return rc;
    if (defer) return UGS_OK;                   // the caller's fill kernel scans (and, for the library's jobs, reports the total)
    if (polled) {
        HIP_TRY(wait_signal(reinterpret_cast<volatile uint32_t *>(plan->pin_slot + 8), plan->pin_epoch, s));
        *total_edges_host = *reinterpret_cast<volatile int64_t *>(plan->pin_slot);
        plan->last_overflow = 0;
        return UGS_OK;
    }
    if (total_edges_host) {
        uint32_t h[4] = {0, 0, 0, 0};
        int64_t tot = 0;
        HIP_TRY(hipMemcpyAsync(&tot, d_edge_ptr + row_count, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        if (may_overflow) HIP_TRY(hipMemcpyAsync(h, plan->ovfcnt.p, sizeof(h), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *total_edges_host = tot;
        plan->last_overflow = h[0];
        const bool handled = may_overflow;
        if ((!handled && h[0] != 0) || (handled && h[last] != 0))
            return fail(UGS_E_HIP, "internal error: walk rows left unprocessed after the last tier");
        if (debug_on()) std::fprintf(stderr, "[UGS SAMPLE] rows=%lld k=%d tier=%d overflow=%u/%u/%u edges=%lld\n", (long long)row_count, k, tc.first, h[0], h[1], h[2], (long long)tot);
    }
    return UGS_OK;
}

int ugs_plan_fill(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int64_t row_begin, int64_t row_count,
                  void *stream, const int64_t *d_nodes, const int64_t *d_edge_ptr, int64_t *d_edge_index, int64_t ld, int64_t *d_edge_src) {
    if (!plan) return fail(UGS_E_BAD_ARG, "plan is null");
    if (k < 1 || k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k outside [1, 32]");
    if (mode < 0 || mode > UGS_FILL_BATCH) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (row_count <= 0) return UGS_OK;
    HIP_TRY(hipSetDevice(plan->device));
    UgsFillArgs a{};
    a.plan = plan->dev;
    a.m = m_per_graph; a.k = k; a.mode = mode;
    a.extra_node_off = extra_node_offset;
    a.row_begin = row_begin; a.row_count = row_count;
    a.nodes = d_nodes; a.edge_ptr = d_edge_ptr;
    a.edge_index = d_edge_index; a.ld = ld; a.edge_src = d_edge_src;
    const TierChoice tc = choose_tier(plan, k);
    std::lock_guard<std::mutex> lk(plan->mu);
    if (plan->stg_valid && plan->stg_nodes == d_nodes && plan->stg_row_begin == row_begin && plan->stg_row_count == row_count &&
        plan->stg_m == m_per_graph && plan->stg_k == k) {
        a.stage = static_cast<const uint2 *>(plan->stage.p); a.counts = static_cast<const uint32_t *>(plan->counts.p);
        a.ulist = static_cast<const int64_t *>(plan->ulist.p); a.ucount = static_cast<const uint32_t *>(plan->ovfcnt.p) + 3;
    }
    if (int rc = plan_enter(plan, static_cast<hipStream_t>(stream))) return rc;
    HIP_TRY(ev_begin(plan, 2, static_cast<hipStream_t>(stream)));
    HIP_TRY(ugs_launch_fill(a, tc.first != UGS_TIER_S, plan->cus, static_cast<hipStream_t>(stream), &plan->last_fill));
    HIP_TRY(ev_end(plan, static_cast<hipStream_t>(stream)));
    return plan_leave(plan, static_cast<hipStream_t>(stream));
}

int ugs_plan_step(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed, int64_t row_begin, int64_t row_count,
                  void *stream, int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *d_edge_index, int64_t ld, int64_t *d_edge_src) {
    if (int rc = walk_check(plan, m_per_graph, k, mode, row_begin, row_count, d_nodes, d_edge_ptr)) return rc;
    if (row_count == 0)                         // edge_ptr[0] = 0, nothing to fill
        return plan_walk_impl(plan, m_per_graph, k, mode, extra_node_offset, seed, nullptr, nullptr, row_begin, row_count, stream, d_nodes, d_edge_ptr, nullptr);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const TierChoice tc = choose_tier(plan, k);
    // one hold of mu from the walk to the fill: the fused fill scans the counts and 8-row sums the walk leaves in the plan's scratch,
    // which another caller's walk on this plan would overwrite in between
    std::unique_lock<std::mutex> lk(plan->mu);
    bool deferred = false;
    if (int rc = plan_walk_locked(plan, tc, m_per_graph, k, mode, extra_node_offset, seed, nullptr, nullptr, row_begin, row_count, s, d_nodes, d_edge_ptr,
                                  nullptr, &deferred, false)) return rc;
    if (!deferred) {                            // the scan ran: the fill reads the plan's scratch only through the staging check
        lk.unlock();
        return ugs_plan_fill(plan, m_per_graph, k, mode, extra_node_offset, row_begin, row_count, stream, d_nodes, d_edge_ptr, d_edge_index, ld, d_edge_src);
    }
    if (int rc = plan_enter(plan, s)) return rc;
    UgsFillArgs a{};
    a.plan = plan->dev;
    a.m = m_per_graph; a.k = k; a.mode = mode;
    a.extra_node_off = extra_node_offset;
    a.row_begin = row_begin; a.row_count = row_count;
    a.nodes = d_nodes; a.edge_ptr = d_edge_ptr; a.edge_ptr_out = d_edge_ptr;
    a.edge_index = d_edge_index; a.ld = ld; a.edge_src = d_edge_src;
    a.counts = static_cast<const uint32_t *>(plan->counts.p);
    a.wsum = static_cast<const uint32_t *>(plan->tiles.p);
    HIP_TRY(ev_begin(plan, 2, s));
    HIP_TRY(ugs_launch_fill_scan(a, plan->cus, s, &plan->last_fill));
    HIP_TRY(ev_end(plan, s));
    return plan_leave(plan, s);
}

// ---- a step captured as a HIP graph (include/ugs_mi355.h) -----------------------------------------------------------------
struct ugs_graph {
    ugs_plan *owner = nullptr;       // keeps the device arrays alive
    ugs_plan *shadow = nullptr;      // the same device arrays with PRIVATE scratch: the graph bakes scratch pointers in, and the
                                     // owner's scratch may be regrown by later calls
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraphNode_t seed_node = nullptr;
    hipStream_t cs = nullptr;
    uint64_t *h_seeds = nullptr;     // pinned ring: a replay's seed must stay put until its upload node has run
    uint64_t *d_seed = nullptr;
    int slot = 0, device = -1;
};
static const int kSeedRing = 256;

int ugs_plan_graph_destroy(ugs_graph *g) {
    if (!g) return UGS_OK;
    if (g->device >= 0 && hipSetDevice(g->device) == hipSuccess) (void)hipDeviceSynchronize();
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    if (g->cs) (void)hipStreamDestroy(g->cs);
    if (g->h_seeds) (void)hipHostFree(g->h_seeds);
    if (g->d_seed) (void)hipFree(g->d_seed);
    if (g->shadow) plan_unref(g->shadow);
    if (g->owner) plan_unref(g->owner);
    delete g;
    return UGS_OK;
}

int ugs_plan_graph_create(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int64_t row_begin, int64_t row_count,
                          int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *d_edge_index, int64_t ld, int64_t *d_edge_src, ugs_graph **graph_out) {
    if (!plan || !graph_out) return fail(UGS_E_BAD_ARG, "null argument");
    if (row_count <= 0 || !d_nodes || !d_edge_ptr || !d_edge_index || !d_edge_src || ld <= 0) return fail(UGS_E_BAD_ARG, "a captured step needs rows and all four output buffers");
    HIP_TRY(hipSetDevice(plan->device));
    auto *g = new ugs_graph();
    g->device = plan->device;
    plan->refs.fetch_add(1);
    g->owner = plan;
    {   // the padded rows belong to the OWNER (one copy, counted against the plan cache): build them before the shadow copies `dev`
        const TierChoice tc0 = choose_tier(plan, k);
        std::lock_guard<std::mutex> lk(plan->mu);
        if ((tc0.first != UGS_TIER_S && tc0.first != UGS_TIER_G) || tc0.second >= 0) {
            DeviceCtx dc0;
            if (int rc = device_ctx(dc0)) { plan_unref(plan); delete g; return rc; }
            if (int rc = ensure_prow(plan, dc0.stream)) { plan_unref(plan); delete g; return rc; }
        }
    }
    auto *sh = new ugs_plan();
    sh->device = plan->device; sh->cus = plan->cus; sh->G = plan->G; sh->nverts = plan->nverts; sh->nnz = plan->nnz;
    {
        std::lock_guard<std::mutex> lk(plan->mu);
        sh->dev = plan->dev;         // device arrays shared, not owned (blob stays null)
        sh->ord1 = plan->ord1;
    }
    sh->prow_failed = true;          // never a private copy of the padded rows: the owner's, or the row-pointer path
    sh->g_n = plan->g_n; sh->g_maxdeg = plan->g_maxdeg; sh->g_sbdeg = plan->g_sbdeg; sh->g_level = plan->g_level;
    sh->walk_share = plan->walk_share;
    g->shadow = sh;
    auto bail = [&](int rc) { ugs_plan_graph_destroy(g); return rc; };
    hipError_t e = hipStreamCreateWithFlags(&g->cs, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&g->h_seeds), kSeedRing * sizeof(uint64_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&g->d_seed), sizeof(uint64_t));
    if (e != hipSuccess) return bail(fail_hip(e, "graph resources"));
    g->h_seeds[0] = 0;
    // 1. an ordinary step: every scratch buffer of the shadow plan gets its final size before anything is captured
    if (int rc = plan_walk_impl(sh, m_per_graph, k, mode, extra_node_offset, 0, nullptr, nullptr, row_begin, row_count, g->cs, d_nodes, d_edge_ptr, nullptr)) return bail(rc);
    if (int rc = ugs_plan_fill(sh, m_per_graph, k, mode, extra_node_offset, row_begin, row_count, g->cs, d_nodes, d_edge_ptr, d_edge_index, ld, d_edge_src)) return bail(rc);
    e = hipStreamSynchronize(g->cs);
    if (e != hipSuccess) return bail(fail_hip(e, "graph warm-up"));
    // 2. the same step captured, reading its seed from d_seed
    e = hipStreamBeginCapture(g->cs, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return bail(fail_hip(e, "hipStreamBeginCapture"));
    int rc = plan_walk_impl(sh, m_per_graph, k, mode, extra_node_offset, 0, g->d_seed, nullptr, row_begin, row_count, g->cs, d_nodes, d_edge_ptr, nullptr);
    if (!rc) rc = ugs_plan_fill(sh, m_per_graph, k, mode, extra_node_offset, row_begin, row_count, g->cs, d_nodes, d_edge_ptr, d_edge_index, ld, d_edge_src);
    e = hipStreamEndCapture(g->cs, &g->graph);
    if (rc) return bail(rc);
    if (e != hipSuccess || !g->graph) return bail(fail_hip(e, "hipStreamEndCapture"));
    // 3. the seed upload as an explicit root node every captured root depends on (its source slot is re-pointed per replay)
    size_t nroots = 0;
    e = hipGraphGetRootNodes(g->graph, nullptr, &nroots);
    std::vector<hipGraphNode_t> roots(nroots);
    if (e == hipSuccess && nroots) e = hipGraphGetRootNodes(g->graph, roots.data(), &nroots);
    const bool static_seed = std::getenv("UGS_GRAPH_STATIC") != nullptr;   // measurement aid: replay without the seed upload
    if (e == hipSuccess && !static_seed) e = hipGraphAddMemcpyNode1D(&g->seed_node, g->graph, nullptr, 0, g->d_seed, g->h_seeds, sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && nroots && !static_seed) {
        std::vector<hipGraphNode_t> from(nroots, g->seed_node);
        e = hipGraphAddDependencies(g->graph, from.data(), roots.data(), nroots);
    }
    if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) return bail(fail_hip(e, "building the graph"));
    *graph_out = g;
    return UGS_OK;
}

// A second plan over the SAME device arrays with scratch of its own: calls on a plan are serialised through its scratch (one
// stream at a time), so a caller that wants two steps in flight -- the next batch's walk filling the tail of this one's, on
// another stream -- samples them through a plan and its twin alternately.
int ugs_plan_twin(ugs_plan *plan, int k, ugs_plan **twin_out) {
    if (!plan || !twin_out) return fail(UGS_E_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(plan->device));
    {   // the padded rows belong to the owner: build them before the twin copies `dev`
        const TierChoice tc0 = choose_tier(plan, k);
        std::lock_guard<std::mutex> lk(plan->mu);
        if ((tc0.first != UGS_TIER_S && tc0.first != UGS_TIER_G) || tc0.second >= 0) {
            DeviceCtx dc0;
            if (int rc = device_ctx(dc0)) return rc;
            if (int rc = ensure_prow(plan, dc0.stream)) return rc;
        }
    }
    auto *sh = new ugs_plan();
    sh->device = plan->device; sh->cus = plan->cus; sh->G = plan->G; sh->nverts = plan->nverts; sh->nnz = plan->nnz;
    {
        std::lock_guard<std::mutex> lk(plan->mu);
        // The twin shares the owner's device arrays but not its ordering state.  A device-built plan's graph descriptors go up by a
        // truly asynchronous copy whose only guard is the owner's recorded event (plan_leave): whatever the owner still has in
        // flight is waited for here, once, so that the twin's first walk on any stream reads finished arrays.
        if (plan->last_valid) {
            const hipError_t e = hipEventSynchronize(plan->last_ev);
            if (e != hipSuccess) { delete sh; return fail(UGS_E_HIP, hipGetErrorString(e)); }
        }
        sh->dev = plan->dev;
        sh->ord1 = plan->ord1;
        sh->walk_share = plan->walk_share;
    }
    sh->g_n = plan->g_n; sh->g_maxdeg = plan->g_maxdeg; sh->g_sbdeg = plan->g_sbdeg; sh->g_level = plan->g_level;
    sh->handle_api = plan->handle_api;
    sh->prow_failed = true;
    plan->refs.fetch_add(1);
    sh->twin_of = plan;
    *twin_out = sh;
    return UGS_OK;
}

int ugs_plan_graph_launch(ugs_graph *g, int seed, void *stream) {
    if (!g || !g->exec) return fail(UGS_E_BAD_ARG, "graph is null");
    HIP_TRY(hipSetDevice(g->device));
    g->slot = (g->slot + 1) % kSeedRing;
    g->h_seeds[g->slot] = (uint64_t)(int64_t)seed;
    if (g->seed_node) HIP_TRY(hipGraphExecMemcpyNodeSetParams1D(g->exec, g->seed_node, g->d_seed, g->h_seeds + g->slot, sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipGraphLaunch(g->exec, static_cast<hipStream_t>(stream)));
    return UGS_OK;
}

// ---- collation of a sharded batch (multi-GPU path; include/ugs_mi355.h: wire format) -------------------------------------------
int ugs_collate_layout(int k, int node_bytes, int eidx_bytes, int esrc_bytes, int64_t rows_cap, int64_t edge_cap, int64_t *section_off4,
                       int64_t *msg_bytes) {
    if (k < 1 || rows_cap < 0 || edge_cap < 0 || !section_off4 || !msg_bytes) return fail(UGS_E_BAD_ARG, "bad arguments to collate_layout");
    if ((node_bytes != 4 && node_bytes != 8) || (eidx_bytes != 1 && eidx_bytes != 4 && eidx_bytes != 8) || (esrc_bytes != 4 && esrc_bytes != 8))
        return fail(UGS_E_BAD_ARG, "wire widths: nodes 4|8, edge_index 1|4|8, edge_src 4|8 bytes");
    auto up = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
    int64_t off = 16;                                            // header: rows, edge entries (2 x int64)
    section_off4[0] = off; off = up(off + rows_cap * k * node_bytes);
    section_off4[1] = off; off = up(off + (rows_cap + 1) * 4);
    section_off4[2] = off; off = up(off + 2 * edge_cap * eidx_bytes);
    section_off4[3] = off; off = up(off + edge_cap * esrc_bytes);
    *msg_bytes = off;
    return UGS_OK;
}

int ugs_collate_unpack(const void *d_msgs, int world, const int64_t *row_off, int k, int node_bytes, int eidx_bytes, int esrc_bytes,
                       int64_t rows_cap, int64_t edge_cap, int64_t *d_nodes, int64_t *d_edge_index, int64_t ld, int64_t *d_edge_ptr,
                       int64_t *d_edge_src, int64_t *d_max_total, void *stream) {
    if (!d_msgs || !row_off || world < 1 || world > UGS_COLLATE_MAX_WORLD) return fail(UGS_E_BAD_ARG, "collate: 1 <= world <= 64 messages expected");
    int64_t so[4], mb = 0;
    if (int rc = ugs_collate_layout(k, node_bytes, eidx_bytes, esrc_bytes, rows_cap, edge_cap, so, &mb)) return rc;
    for (int r = 0; r < world; ++r)
        if (row_off[r + 1] < row_off[r] || row_off[r + 1] - row_off[r] > rows_cap) return fail(UGS_E_BAD_ARG, "collate: a rank's row range exceeds rows_cap");
    const bool empty = row_off[world] == row_off[0];             // a batch without rows has no node entries: d_nodes may be null (an empty device tensor's pointer is)
    if ((!d_nodes && !empty) || !d_edge_ptr || (edge_cap > 0 && !empty && (!d_edge_index || !d_edge_src))) return fail(UGS_E_BAD_ARG, "null output pointer");
    if (empty) {                                                 // no rows, hence no edge entries: nothing to launch, edge_ptr is its one closing word
        HIP_TRY(hipMemsetAsync(d_edge_ptr + row_off[world], 0, sizeof(int64_t), static_cast<hipStream_t>(stream)));
        return UGS_OK;
    }
    HIP_TRY(ugs_launch_collate_unpack(d_msgs, world, mb, row_off, k, node_bytes, eidx_bytes, esrc_bytes, rows_cap, edge_cap, so, d_nodes,
                                      d_edge_index, ld, d_edge_ptr, d_edge_src, d_max_total, static_cast<hipStream_t>(stream)));
    return UGS_OK;
}

int ugs_plan_set_walk_share(ugs_plan *plan, int percent) {
    if (!plan || percent < 1 || percent > 100) return fail(UGS_E_BAD_ARG, "walk share: a plan and 1..100 percent");
    std::lock_guard<std::mutex> lk(plan->mu);
    plan->walk_share = percent;
    return UGS_OK;
}

int ugs_plan_set_timing(ugs_plan *plan, int on) {
    if (!plan) return fail(UGS_E_BAD_ARG, "plan is null");
    std::lock_guard<std::mutex> lk(plan->mu);
    ev_clear(plan);
    plan->timing = on != 0;
    return UGS_OK;
}

int ugs_plan_get_timing(ugs_plan *plan, double *ms_sum3, int64_t *launches3) {
    if (!plan || !ms_sum3 || !launches3) return fail(UGS_E_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(plan->mu);
    for (int i = 0; i < 3; ++i) { ms_sum3[i] = 0.0; launches3[i] = 0; }
    for (auto &e : plan->events) {
        HIP_TRY(hipEventSynchronize(e.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
        ms_sum3[e.kind] += (double)ms;
        launches3[e.kind] += 1;
    }
    ev_clear(plan);
    return UGS_OK;
}

int ugs_plan_last_launch(const ugs_plan *plan, char *name_buf, int name_buf_len, int *grid, int *block, int *lds_bytes, int64_t *overflow_rows) {
    if (!plan) return fail(UGS_E_BAD_ARG, "plan is null");
    if (name_buf && name_buf_len > 0) { std::snprintf(name_buf, (size_t)name_buf_len, "%s", plan->last_walk.name ? plan->last_walk.name : ""); }
    if (grid) *grid = plan->last_walk.grid;
    if (block) *block = plan->last_walk.block;
    if (lds_bytes) *lds_bytes = plan->last_walk.lds_bytes;
    if (overflow_rows) *overflow_rows = plan->last_overflow;
    return UGS_OK;
}

int ugs_plan_last_fill(const ugs_plan *plan, char *name_buf, int name_buf_len, int *grid, int *block) {
    if (!plan) return fail(UGS_E_BAD_ARG, "plan is null");
    if (name_buf && name_buf_len > 0) { std::snprintf(name_buf, (size_t)name_buf_len, "%s", plan->last_fill.name ? plan->last_fill.name : ""); }
    if (grid) *grid = plan->last_fill.grid;
    if (block) *block = plan->last_fill.block;
    return UGS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// jobs: the two-phase host-facing API (begin = walks + counts, finish = fill + copy-out)
// ---------------------------------------------------------------------------------------------------------------
// What fills a side sampler's edge outputs at finish: edge_index [2, ld] and edge_src [ld] on the device, on the job's stream.
using JobFill = std::function<hipError_t(int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s)>;
enum { UGS_JOB_UGS = 0, UGS_JOB_EPS, UGS_JOB_UNIFORM, UGS_JOB_RWR, UGS_JOB_UNIFORM_ENUM, UGS_JOB_UNIFORM_POP };

struct ugs_job {
    ugs_plan *plan = nullptr;          // ugs jobs only
    DeviceCtx dc;
    int kind = UGS_JOB_UGS;            // which begin made it: the samplers' own *_finish take no other's job
    int m = 0, k = 0, mode = 0;
    int64_t extra = 0, rows = 0, total = 0, G = 0;
    PoolBuf nodes;                     // nodes [rows, k] and, right behind it, edge_ptr [rows + 1]: one buffer, so that a caller whose
    int64_t *d_eptr = nullptr;         // output tensors are adjacent too gets both with one copy
    // batches of small graphs: begin ran walk + fill as one step (scan folded into the fill) into this staging -- edge_index [2, total]
    // and edge_src [total] laid out for the total the kernel found -- and finish only copies out
    bool packed_ok = false;
    // ugs_sample_graphs_begin: the per-graph seed bases, widened; uploaded on the job's stream to the end of `nodes` (begin_common)
    std::vector<uint64_t> seeds;
    // the side samplers (epsilon_uniform, uniform, rwr): the call's device arrays -- inputs, then the scratch of
    // every stage -- in one pooled blob (hipMalloc/hipFree per call cost milliseconds once the process holds large plans), and the fill
    // that finish runs from them.  The hook holds the sampler's call struct by value; empty: the job fills through its plan.
    PoolBuf blob;
    JobFill fill;
    // a job whose begin reports its own row count (ugs_uniform_enumerate_begin): its sample_ptr [G + 1], rows = sample_ptr[G];
    // empty: rows = G m and sample_ptr = g m
    std::vector<int64_t> sample_ptr;
};

namespace {
std::atomic<int64_t> g_spec_kept{0}, g_spec_wrong{0};              // large calls whose early start stood / was thrown away
std::atomic<int64_t> g_packed_staged{0}, g_packed_refused{0};      // packed steps whose total fitted the staging / that the kernel refused
void free_job(ugs_job *j) {
    if (!j) return;
    pool_put(j->nodes);
    pool_put(j->blob);
    plan_unref(j->plan);
    delete j;
}
int hand_out(ugs_job *j, ugs_job **job_out, int64_t *total_out) {
    *job_out = j;
    if (total_out) *total_out = j->total;
    return UGS_OK;
}

// second launch of a job's step (see begin_common): ugs_fill_scan into the job's staging, total through the pinned slot of the plan.
// Call with plan->mu held since the walk whose counts and 8-row sums it scans.
int packed_fill_locked(ugs_job *j, int64_t cap3) {
    ugs_plan *plan = j->plan;
    hipStream_t s = j->dc.stream;
    int64_t *stg = static_cast<int64_t *>(j->nodes.p) + (j->rows * j->k + j->rows + 1);       // (begin_common sized the buffer for it)
    if (int rc = plan_enter(plan, s)) return rc;
    if (!plan->pin_slot) plan->pin_slot = pin_slot_get();
    UgsFillArgs a{};
    a.plan = plan->dev;
    a.m = j->m; a.k = j->k; a.mode = j->mode;
    a.extra_node_off = j->extra;
    a.row_begin = 0; a.row_count = j->rows;
    a.nodes = static_cast<const int64_t *>(j->nodes.p); a.edge_ptr = j->d_eptr; a.edge_ptr_out = j->d_eptr;
    a.edge_index = stg; a.ld = 0; a.edge_src = nullptr;                                       // set by the kernel (packed_cap)
    a.packed_cap = cap3;
    a.counts = static_cast<const uint32_t *>(plan->counts.p);
    a.wsum = static_cast<const uint32_t *>(plan->tiles.p);
    const bool poll = plan->pin_slot != nullptr;
    if (poll) {
        uint32_t ep = g_pin_epoch.fetch_add(1) + 1;
        if (ep == 0) ep = g_pin_epoch.fetch_add(1) + 1;
        plan->pin_epoch = ep;
        a.h_total = reinterpret_cast<int64_t *>(plan->pin_slot); a.h_flag = reinterpret_cast<uint32_t *>(plan->pin_slot + 8); a.epoch = ep;
    }
    HIP_TRY(ev_begin(plan, 2, s));
    HIP_TRY(ugs_launch_fill_scan(a, plan->cus, s, &plan->last_fill));
    HIP_TRY(ev_end(plan, s));
    if (int rc = plan_leave(plan, s)) return rc;
    if (poll) {
        HIP_TRY(wait_signal(reinterpret_cast<volatile uint32_t *>(plan->pin_slot + 8), plan->pin_epoch, s));
        j->total = *reinterpret_cast<volatile int64_t *>(plan->pin_slot);
    } else {
        int64_t tot = 0;
        HIP_TRY(hipMemcpyAsync(&tot, j->d_eptr + j->rows, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        j->total = tot;
    }
    plan->last_overflow = 0;
    j->packed_ok = 3 * j->total <= cap3;
    (j->packed_ok ? g_packed_staged : g_packed_refused).fetch_add(1);
    return UGS_OK;
}

// seeds (ugs_sample_graphs_begin): plan->G per-graph seeds that replace `seed`; nullptr: one seed for the call
int begin_common(ugs_plan *plan, int m, int k, int mode, int64_t extra, int seed, ugs_job **job_out, int64_t *total_out,
                 const int32_t *seeds = nullptr) {
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) { plan_unref(plan); return rc; }
    auto *j = new ugs_job();
    j->plan = plan; j->dc = dc; j->m = m; j->k = k; j->mode = mode; j->extra = extra;
    j->G = plan->G;
    j->rows = plan->G * (int64_t)m;
    // (a job that may run the packed step keeps its edge staging right behind nodes and edge_ptr: all four outputs leave in ONE copy when
    // the caller's tensors are adjacent too, as the Python shim's are)
    const int64_t node_words = j->rows * k + j->rows + 1;
    const int64_t cap3_want = 3 * j->rows * 2 * (int64_t)k * (int64_t)(k - 1);
    const TierChoice tc0 = choose_tier(plan, k);
    const bool may_pack = k >= 2 && j->rows > 0 && j->rows <= 131072 && tc0.first == UGS_TIER_S && tc0.second < 0 && !tc0.third_G &&
                          cap3_want * (int64_t)sizeof(int64_t) <= ((int64_t)192 << 20) && !debug_on() && std::getenv("UGS_NO_PACKED_STEP") == nullptr;
    const int64_t out_words = node_words + (may_pack ? cap3_want : 0);          // the seed table, if any, lies behind everything finish copies
    const int64_t seed_words = seeds ? plan->G : 0;
    int rc = pool_get((size_t)(out_words + seed_words) * sizeof(int64_t), dc.id, j->nodes);
    const uint64_t *d_seeds = nullptr;
    if (!rc && seed_words > 0) {
        j->seeds.resize((size_t)seed_words);
        for (int64_t g = 0; g < seed_words; ++g) j->seeds[(size_t)g] = (uint64_t)(int64_t)seeds[g];
        uint64_t *d = reinterpret_cast<uint64_t *>(static_cast<int64_t *>(j->nodes.p) + out_words);
        if (hipError_t e = hipMemcpyAsync(d, j->seeds.data(), (size_t)seed_words * sizeof(uint64_t), hipMemcpyHostToDevice, dc.stream); e != hipSuccess)
            rc = fail_hip(e, "hipMemcpyAsync(seeds)");
        d_seeds = d;
    }
    if (!rc) {
        j->d_eptr = static_cast<int64_t *>(j->nodes.p) + j->rows * k;
        // Small batches: every ordered pair of a row's vertices, twice (both directions of a PyG edge are columns, and each column is
        // symmetrised), bounds the edge entries -- if a staging of that size is affordable the step runs here in two launches, the total
        // comes from the fill kernel's first block, and the caller allocates while the rows are being filled.  Repeated columns can
        // exceed the bound: the kernel then writes nothing and finish fills the ordinary way.
        const int64_t cap3 = cap3_want;
        const bool want_packed = may_pack;
        int64_t *d_nodes = static_cast<int64_t *>(j->nodes.p);
        if (want_packed) {                          // (rows > 0) one hold of mu from the walk to the fill that scans its counts and sums
            rc = walk_check(plan, m, k, mode, 0, j->rows, d_nodes, j->d_eptr);
            if (!rc) {
                std::lock_guard<std::mutex> lk(plan->mu);
                bool deferred = false;
                rc = plan_walk_locked(plan, tc0, m, k, mode, extra, seed, nullptr, d_seeds, 0, j->rows, dc.stream, d_nodes, j->d_eptr, &j->total, &deferred, true);
                if (!rc && deferred) rc = packed_fill_locked(j, cap3);
            }
        } else {
            rc = plan_walk_impl(plan, m, k, mode, extra, seed, nullptr, d_seeds, 0, j->rows, dc.stream, d_nodes, j->d_eptr, &j->total, nullptr, true);
        }
    }
    if (rc) { free_job(j); return rc; }
    return hand_out(j, job_out, total_out);
}

int finish_common(ugs_job *j, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr, int64_t *edge_src, int dst_is_device) {
    hipStream_t s = j->dc.stream;
    const int64_t rows = j->rows, k = j->k, tot = j->total;
    int rc = UGS_OK;
    PoolBuf e_idx;                     // host outputs: edge_index [2, tot] and edge_src [tot] staged in ONE device buffer
    auto body = [&]() -> int {
        HIP_TRY(hipSetDevice(j->dc.id));
        int64_t *d_ei = edge_index, *d_es = edge_src;
        const bool packed = j->packed_ok && tot > 0;                // the step already ran (begin_common): copy out of its staging
        if (packed) { d_ei = static_cast<int64_t *>(j->nodes.p) + (rows * k + rows + 1); d_es = d_ei + 2 * tot; }
        else if (!dst_is_device && tot > 0) {
            if (int r = pool_get((size_t)(3 * tot) * sizeof(int64_t), j->dc.id, e_idx)) return r;
            d_ei = static_cast<int64_t *>(e_idx.p); d_es = d_ei + 2 * tot;
        }
        if (tot > 0 && !packed) {                                   // (a side sampler's job is never packed)
            if (!d_ei || !d_es) return fail(UGS_E_BAD_ARG, "null edge output pointer");
            if (j->fill) HIP_TRY(j->fill(d_ei, d_es, tot, s));
            else if (int r = ugs_plan_fill(j->plan, j->m, j->k, j->mode, j->extra, 0, rows, s, static_cast<const int64_t *>(j->nodes.p),
                                           j->d_eptr, d_ei, tot, d_es)) return r;
        }
        const hipMemcpyKind kind = dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        // adjacent outputs (the Python shim carves its tensors out of one allocation) travel in one copy each -- or all in one
        if (packed && edge_ptr == nodes + rows * k && edge_index == edge_ptr + rows + 1 && edge_src == edge_index + 2 * tot) {
            // (the same copy through a kernel storing to the pinned tensors was measured: 103 against 96 us for the 2.3 MB of the
            // PROTEINS-shaped call -- the DMA copy stays)
            HIP_TRY(hipMemcpyAsync(nodes, j->nodes.p, (size_t)(rows * k + rows + 1 + 3 * tot) * sizeof(int64_t), kind, s));
        } else {
        if (edge_ptr == nodes + rows * k) {
            HIP_TRY(hipMemcpyAsync(nodes, j->nodes.p, (size_t)(rows * k + rows + 1) * sizeof(int64_t), kind, s));
        } else {
            if (rows * k > 0) HIP_TRY(hipMemcpyAsync(nodes, j->nodes.p, (size_t)(rows * k) * sizeof(int64_t), kind, s));
            HIP_TRY(hipMemcpyAsync(edge_ptr, j->d_eptr, (size_t)(rows + 1) * sizeof(int64_t), kind, s));
        }
        if ((!dst_is_device || packed) && tot > 0) {
            if (!edge_index || !edge_src) return fail(UGS_E_BAD_ARG, "null edge output pointer");
            if (edge_src == edge_index + 2 * tot) {
                HIP_TRY(hipMemcpyAsync(edge_index, d_ei, (size_t)(3 * tot) * sizeof(int64_t), kind, s));
            } else {
                HIP_TRY(hipMemcpyAsync(edge_index, d_ei, (size_t)(2 * tot) * sizeof(int64_t), kind, s));
                HIP_TRY(hipMemcpyAsync(edge_src, d_es, (size_t)tot * sizeof(int64_t), kind, s));
            }
        }
        }
        if (sample_ptr) {
            std::vector<int64_t> sp((size_t)j->G + 1);
            for (int64_t g = 0; g <= j->G; ++g) sp[(size_t)g] = j->sample_ptr.empty() ? g * (int64_t)j->m : j->sample_ptr[(size_t)g];
            if (dst_is_device) HIP_TRY(hipMemcpy(sample_ptr, sp.data(), sp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            else std::memcpy(sample_ptr, sp.data(), sp.size() * sizeof(int64_t));
        }
        HIP_TRY(hipStreamSynchronize(s));
        return UGS_OK;
    };
    rc = body();
    pool_put(e_idx);
    free_job(j);
    return rc;
}

// ---- what the begins of the side samplers share (eps_begin, uniform_begin, rwr_begin below) ----
// Layout of a job's blob: pieces in the order they are taken, each at a multiple of 256 bytes.  The inputs come first, so that they
// go up in one copy of in_bytes; the scratch of every stage follows.
struct BlobLayout {
    size_t off = 0, in_bytes = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align_up(off + std::max<size_t>(bytes, 8)); return o; }
    void end_inputs() { in_bytes = off; }
};

// The inputs of a sampler that reads the batch itself: both edge rows, ptr, one descriptor per graph and (sample_graphs) the seeds.
struct BatchInputs {
    size_t src, dst, ptr, desc, seeds;
    BatchInputs(BlobLayout &L, int64_t E, int64_t G, size_t desc_bytes, bool per_graph)
        : src(L.take((size_t)E * 8)), dst(L.take((size_t)E * 8)), ptr(L.take((size_t)(G + 1) * 8)), desc(L.take((size_t)G * desc_bytes)),
          seeds(L.take(per_graph ? (size_t)G * 8 : 0)) {}
    void stage(char *host, const int64_t *edge_index, int64_t row_stride, int64_t E, const int64_t *ptr_in, int64_t G, const void *descs,
               size_t desc_bytes, const uint64_t *seeds_in) const {
        for (int64_t e = 0; e < E; ++e) {
            reinterpret_cast<int64_t *>(host + src)[e] = edge_index[e];
            reinterpret_cast<int64_t *>(host + dst)[e] = edge_index[row_stride + e];
        }
        std::memcpy(host + ptr, ptr_in, (size_t)(G + 1) * 8);
        if (G > 0) std::memcpy(host + desc, descs, (size_t)G * desc_bytes);
        if (seeds_in && G > 0) std::memcpy(host + seeds, seeds_in, (size_t)G * 8);
    }
};

// The ptr scan of such a sampler.  ptr must not decrease.  `each(g, n, why)` writes graph g's descriptor and says whether the sampler
// cannot take the graph, leaving the refusal's text in `why`: sample_batch refuses the call with it, sample_graphs lets the graph fail
// alone (too_big[g] = 1: m rows of -1, no draws).
template <class Each>
int scan_ptr(const int64_t *ptr, int64_t G, bool per_graph, std::vector<int32_t> &too_big, Each each) {
    too_big.assign(per_graph ? (size_t)G : 0, 0);
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = ptr[g + 1] - ptr[g];
        if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
        std::string why;
        if (!each(g, n, why)) continue;
        if (!per_graph) return fail(UGS_E_UNSUPPORTED, why);
        too_big[(size_t)g] = 1;
    }
    return UGS_OK;
}

// nodes [rows, k] with edge_ptr [rows + 1] right behind it, and `extra_bytes` of the sampler's own behind both (finish copies none of
// them out).  On failure the job is gone.
int side_job_rows(ugs_job *j, int64_t rows, size_t extra_bytes = 0) {
    j->rows = rows;
    if (int rc = pool_get((size_t)(rows * j->k + rows + 1) * sizeof(int64_t) + extra_bytes, j->dc.id, j->nodes)) { free_job(j); return rc; }
    j->d_eptr = static_cast<int64_t *>(j->nodes.p) + rows * j->k;
    return UGS_OK;
}

// The job of a side sampler: its parameters, its blob, and the G m rows of side_job_rows.  rows_later: the begin learns its row count
// from the device (enumeration) and calls side_job_rows itself, or never has rows (counting).
int side_job(const DeviceCtx &dc, int kind, int64_t G, int m, int k, int mode, size_t blob_bytes, ugs_job **out, bool rows_later = false) {
    auto *j = new ugs_job();
    j->dc = dc; j->kind = kind; j->m = m; j->k = k; j->mode = mode; j->G = G;
    if (int rc = pool_get(blob_bytes, dc.id, j->blob)) { free_job(j); return rc; }
    if (!rows_later) if (int rc = side_job_rows(j, G * (int64_t)m)) return rc;
    *out = j;
    return UGS_OK;
}

// The end of such a begin.  `e` is the outcome of everything the sampler has queued on the job's stream since side_job (upload, kernels,
// read-backs of its own): the total follows them to the host, the stream is drained, and a HIP error of any of it is reported as
// `what`.  On failure the job is gone.
int side_job_total(ugs_job *j, hipError_t e, const char *what) {
    if (e == hipSuccess) e = hipMemcpyAsync(&j->total, j->d_eptr + j->rows, sizeof(int64_t), hipMemcpyDeviceToHost, j->dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(j->dc.stream);
    if (e == hipSuccess) return UGS_OK;
    free_job(j);
    return fail_hip(e, what);
}
}  // namespace

extern "C" {

int ugs_sample_begin(int64_t handle, int m_per_graph, int k, int edge_mode, int64_t base_offset, int seed, ugs_job **job_out, int64_t *total_edges_out) {
    if (!job_out) return fail(UGS_E_BAD_ARG, "job_out is null");
    if (edge_mode < 0 || edge_mode > 2) return fail(UGS_E_BAD_MODE, "edge_mode must be one of: 'local', 'flat', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    auto g = lookup(handle);
    if (!g) return fail(UGS_E_INVALID_HANDLE, "Invalid preproc handle");
    if (g->n == 0) return fail(UGS_E_NO_ROOTS, "No viable roots available");
    ugs_plan *plan = nullptr;
    if (int rc = ugs_plan_create_handle(handle, &plan)) return rc;
    return begin_common(plan, m_per_graph, k, edge_mode, edge_mode == UGS_EDGE_GLOBAL ? base_offset : 0, seed, job_out, total_edges_out);
}

int ugs_sample_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *edge_src, int dst_is_device) {
    if (!job) return fail(UGS_E_BAD_ARG, "job is null");
    return finish_common(job, nodes, edge_index, edge_ptr, nullptr, edge_src, dst_is_device);
}

int ugs_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                           int m_per_graph, int k, int mode, int seed, ugs_job **job_out, int64_t *total_edges_out) {
    if (!job_out) return fail(UGS_E_BAD_ARG, "job_out is null");
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    ugs_plan *plan = nullptr;
    // Large batches start early, like ugs_sample_batch_stream below: the walks begin on the plan the batch's sampled words point at while
    // the lookup (content hash over every column: ~3 ms for 20 M columns) runs on a helper thread; kept only if it names the same plan.
    ugs_plan *guess = nullptr;
    DeviceCtx dc;
    const int64_t spec_min_cols = [] { const char *e = std::getenv("UGS_SPEC_MIN_COLS"); return e ? (int64_t)std::atoll(e) : (int64_t)1 << 21; }();   // (tests lower it)
    if (num_cols >= spec_min_cols && ptr && edge_index && num_graphs > 0 && m_per_graph > 0 && !debug_on() &&
        std::getenv("UGS_NO_SPECULATION") == nullptr && std::getenv("UGS_NO_BATCH_INDEX") == nullptr && device_ctx(dc) == UGS_OK)
        guess = peek_batch_plan(edge_index, edge_index + row_stride, num_cols, ptr, num_graphs, k, dc.id);
    if (guess) {
        int lookup_rc = UGS_OK;
        std::string lookup_err;
        const int dev_tl = t_device; const hipStream_t st_tl = t_job_stream; const bool set_tl = t_job_stream_set;
        std::thread lookup_thread;
        try {
            lookup_thread = std::thread([&, dev_tl, st_tl, set_tl] {
                t_device = dev_tl >= 0 ? dev_tl : dc.id; t_job_stream = st_tl; t_job_stream_set = set_tl;
                lookup_rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan);
                if (lookup_rc != UGS_OK) lookup_err = t_err;
            });
        } catch (...) { plan_unref(guess); guess = nullptr; }          // no thread to be had: look up first, as without a guess
        if (!guess) {
            if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
            return begin_common(plan, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);
        }
        *job_out = nullptr;
        const int rc = begin_common(guess, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);   // (owns the guess's reference)
        lookup_thread.join();
        if (lookup_rc != UGS_OK) { if (rc == UGS_OK) { free_job(*job_out); *job_out = nullptr; } return fail(lookup_rc, lookup_err); }
        if (plan == guess) { plan_unref(plan); g_spec_kept.fetch_add(1); return rc; }
        if (rc == UGS_OK) { free_job(*job_out); *job_out = nullptr; }                       // a different batch after all: once more, on its plan
        g_spec_wrong.fetch_add(1);
        return begin_common(plan, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);
    }
    if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
    return begin_common(plan, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);
}

// sample_batch with one seed per graph: the same plan lookup (LRU replay, device batch pass) and the same job; the seeds go to the
// device with the job (begin_common).  No early start: presample chunks are far below its threshold.
int ugs_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                            int m_per_graph, int k, int mode, const int32_t *seeds, ugs_job **job_out, int64_t *total_edges_out) {
    if (!job_out) return fail(UGS_E_BAD_ARG, "job_out is null");
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (num_graphs > 0 && !seeds) return fail(UGS_E_BAD_ARG, "sample_graphs needs one seed per graph");
    ugs_plan *plan = nullptr;
    if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
    return begin_common(plan, m_per_graph, k, mode, 0, 0, job_out, total_edges_out, num_graphs > 0 ? seeds : nullptr);
}

int ugs_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                            int64_t *edge_src_global, int dst_is_device) {
    if (!job) return fail(UGS_E_BAD_ARG, "job is null");
    return finish_common(job, nodes, edge_index, edge_ptr, sample_ptr, edge_src_global, dst_is_device);
}

int ugs_job_cancel(ugs_job *job) { free_job(job); return UGS_OK; }

// ---- the whole sample_batch call with the copy-out running BESIDE the walks (large host-visible calls) ------------------------------
// The two-phase call is walk (all rows) -> total -> caller allocates -> fill -> copy out: for a million rows the 400 MB of int64
// results cross PCIe for longer than the walks take, one after the other.  Here the caller hands over its buffers up front (edge
// buffers by a capacity it expects, e.g. the previous call's total plus a margin), the rows go through walk / scan / fill in chunks on
// the job stream, and every finished chunk leaves on a second stream while the next one walks.  Row 1 of edge_index [2, total] starts
// at `total`, known with the last chunk only: that half is kept in the device staging and leaves at the end.
namespace {
std::mutex g_copy_mu;
std::map<int, hipStream_t> &g_copy_streams = *new std::map<int, hipStream_t>();
int copy_stream(int dev, hipStream_t &out) {
    std::lock_guard<std::mutex> lk(g_copy_mu);
    auto it = g_copy_streams.find(dev);
    if (it == g_copy_streams.end()) {
        hipStream_t c = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
        it = g_copy_streams.emplace(dev, c).first;
    }
    out = it->second;
    return UGS_OK;
}

// One streamed call: parameters, the caller's (pinned host) buffers, and the device staging that outlives a thrown-away early start.
struct StreamCall {
    DeviceCtx dc;
    int64_t G = 0, extra = 0, cap = 0;
    int m = 0, k = 0, mode = 0, seed = 0;
    int64_t *nodes = nullptr, *edge_index = nullptr, *edge_ptr = nullptr, *sample_ptr = nullptr, *edge_src = nullptr, *total_out = nullptr;
    hipStream_t cs = nullptr;
    PoolBuf d_nodes_b, d_eptr_b, d_loc_b, d_edges_b;
    std::vector<hipEvent_t> evs;
    void release() {
        for (hipEvent_t ev : evs) (void)hipEventDestroy(ev);
        evs.clear();
        pool_put(d_nodes_b); pool_put(d_eptr_b); pool_put(d_loc_b); pool_put(d_edges_b);
    }
};

int stream_rows(ugs_plan *plan, StreamCall &c) {
    const int64_t rows = c.G * (int64_t)c.m, cap = c.cap;
    const int k = c.k;
    int64_t chunk = (rows + 7) / 8;                                   // eight chunks: the first copy starts after an eighth of the walks
    if (chunk < 65536) chunk = 65536;
    if (const char *e = std::getenv("UGS_STREAM_CHUNK_ROWS")) { const int64_t v = std::atoll(e); if (v > 0) chunk = v; }   // (tests: many chunks of a small call)
    const int64_t nchunks = rows > 0 ? (rows + chunk - 1) / chunk : 0;
    hipStream_t s = c.dc.stream;
    int64_t base = 0;
    HIP_TRY(hipSetDevice(c.dc.id));
    if (int rc = copy_stream(c.dc.id, c.cs)) return rc;
    hipStream_t cs = c.cs;
    if (c.sample_ptr) for (int64_t g = 0; g <= c.G; ++g) c.sample_ptr[g] = g * (int64_t)c.m;
    if (rows == 0) { c.edge_ptr[0] = 0; *c.total_out = 0; return UGS_OK; }
    if (!c.d_nodes_b.p) if (int rc = pool_get((size_t)(rows * k) * sizeof(int64_t), c.dc.id, c.d_nodes_b)) return rc;
    if (!c.d_eptr_b.p) if (int rc = pool_get((size_t)(rows + 1) * sizeof(int64_t), c.dc.id, c.d_eptr_b)) return rc;
    if (!c.d_loc_b.p) if (int rc = pool_get((size_t)(chunk + 1) * sizeof(int64_t), c.dc.id, c.d_loc_b)) return rc;
    if (cap > 0 && !c.d_edges_b.p) if (int rc = pool_get((size_t)(3 * cap) * sizeof(int64_t), c.dc.id, c.d_edges_b)) return rc;
    int64_t *d_nodes = static_cast<int64_t *>(c.d_nodes_b.p), *d_eptr = static_cast<int64_t *>(c.d_eptr_b.p), *d_loc = static_cast<int64_t *>(c.d_loc_b.p);
    int64_t *d_ei = static_cast<int64_t *>(c.d_edges_b.p), *d_es = d_ei ? d_ei + 2 * cap : nullptr;
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        const int64_t r0 = ch * chunk, rc_rows = std::min(chunk, rows - r0);
        const bool last = ch + 1 == nchunks;
        int64_t tot = 0;
        if (int rc = plan_walk_impl(plan, c.m, k, c.mode, c.extra, c.seed, nullptr, nullptr, r0, rc_rows, s, d_nodes + r0 * k, d_loc, &tot, nullptr, true)) return rc;
        if (base + tot > cap) { *c.total_out = base + tot; return fail(UGS_E_CAPACITY, "edge_capacity too small for this call's edge entries"); }
        if (tot > 0)
            if (int rc = ugs_plan_fill(plan, c.m, k, c.mode, c.extra, r0, rc_rows, s, d_nodes + r0 * k, d_loc, d_ei + base, cap, d_es + base)) return rc;
        HIP_TRY(ugs_launch_rebase_edge_ptr(d_loc, d_eptr + r0, rc_rows + (last ? 1 : 0), base, s));
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c.evs.push_back(ev);
        HIP_TRY(hipEventRecord(ev, s));
        HIP_TRY(hipStreamWaitEvent(cs, ev, 0));
        HIP_TRY(hipMemcpyAsync(c.nodes + r0 * k, d_nodes + r0 * k, (size_t)(rc_rows * k) * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipMemcpyAsync(c.edge_ptr + r0, d_eptr + r0, (size_t)(rc_rows + (last ? 1 : 0)) * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
        if (tot > 0) {
            HIP_TRY(hipMemcpyAsync(c.edge_index + base, d_ei + base, (size_t)tot * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
            HIP_TRY(hipMemcpyAsync(c.edge_src + base, d_es + base, (size_t)tot * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
        }
        base += tot;
    }
    // row 1 of edge_index: its place in the caller's [2, total] is known now (the last chunk's event orders it behind every fill)
    if (base > 0) HIP_TRY(hipMemcpyAsync(c.edge_index + base, d_ei + cap, (size_t)base * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    *c.total_out = base;
    return UGS_OK;
}
}  // namespace

int ugs_stream_stats(int64_t *early_starts_kept, int64_t *early_starts_discarded) {
    if (early_starts_kept) *early_starts_kept = g_spec_kept.load();
    if (early_starts_discarded) *early_starts_discarded = g_spec_wrong.load();
    return UGS_OK;
}

int ugs_step_stats(int64_t *packed_staged, int64_t *packed_refused) {
    if (packed_staged) *packed_staged = g_packed_staged.load();
    if (packed_refused) *packed_refused = g_packed_refused.load();
    return UGS_OK;
}

int ugs_sample_batch_stream(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                            int m_per_graph, int k, int mode, int seed, int64_t edge_capacity, int64_t *nodes, int64_t *edge_index_out,
                            int64_t *edge_ptr, int64_t *sample_ptr, int64_t *edge_src_global, int64_t *total_edges_out) {
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (edge_capacity < 0 || !edge_ptr || !total_edges_out) return fail(UGS_E_BAD_ARG, "null output pointer or negative edge_capacity");
    if (!ptr || num_graphs < 0 || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    const int64_t G = num_graphs, rows = G * (int64_t)m_per_graph, cap = edge_capacity;
    if (rows > 0 && (!nodes || (cap > 0 && (!edge_index_out || !edge_src_global)))) return fail(UGS_E_BAD_ARG, "null output pointer");
    // The real lookup reads every column (content hash: ~3 ms for 20 M columns).  A batch whose sampled words match a remembered one
    // starts on that batch's plan at once, the lookup runs beside it on a helper thread, and the results stand only if the lookup
    // returns the same plan; otherwise the streams are drained and the call runs again on the right one.
    ugs_plan *plan = nullptr, *guess = nullptr;
    if (rows > 0 && !debug_on() && std::getenv("UGS_NO_SPECULATION") == nullptr && std::getenv("UGS_NO_BATCH_INDEX") == nullptr)
        guess = peek_batch_plan(edge_index, edge_index + row_stride, num_cols, ptr, G, k, dc.id);
    std::thread lookup_thread;
    int lookup_rc = UGS_OK;
    std::string lookup_err;
    if (guess) {
        const int dev_tl = t_device; const hipStream_t st_tl = t_job_stream; const bool set_tl = t_job_stream_set;
        try {
            lookup_thread = std::thread([&, dev_tl, st_tl, set_tl] {
                t_device = dev_tl >= 0 ? dev_tl : dc.id; t_job_stream = st_tl; t_job_stream_set = set_tl;
                lookup_rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan);
                if (lookup_rc != UGS_OK) lookup_err = t_err;
            });
        } catch (...) { plan_unref(guess); guess = nullptr; }          // no thread to be had: look up first, as without a guess
    }
    if (!guess) if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
    StreamCall sc;
    sc.dc = dc; sc.G = G; sc.m = m_per_graph; sc.k = k; sc.mode = mode; sc.extra = 0; sc.seed = seed; sc.cap = cap;
    sc.nodes = nodes; sc.edge_index = edge_index_out; sc.edge_ptr = edge_ptr; sc.sample_ptr = sample_ptr; sc.edge_src = edge_src_global;
    sc.total_out = total_edges_out;
    hipStream_t s = dc.stream;
    auto body = [&](ugs_plan *p) { return stream_rows(p, sc); };
    auto drain = [&] { if (sc.cs) (void)hipStreamSynchronize(sc.cs); (void)hipStreamSynchronize(s); };
    int rc = UGS_OK;
    if (guess) {
        std::string guess_err;
        rc = body(guess);
        if (rc != UGS_OK) guess_err = t_err;
        lookup_thread.join();
        if (lookup_rc != UGS_OK) { drain(); rc = fail(lookup_rc, lookup_err); }             // the call's own error (what the two-phase call reports)
        else if (plan != guess) { drain(); g_spec_wrong.fetch_add(1); rc = body(plan); }      // a different batch after all: once more, on its plan
        else if (rc != UGS_OK) rc = fail(rc, guess_err);
        else g_spec_kept.fetch_add(1);
        plan_unref(guess);
    } else rc = body(plan);
    if (rc != UGS_OK) drain();                                      // nothing may still read the pool buffers
    sc.release();
    if (plan) plan_unref(plan);
    return rc;
}

/* sample() of the handle API (reference src/sampler.cpp:91-290) the same way: rows in chunks, copy-out beside the walks. */
int ugs_sample_stream(int64_t handle, int m_per_graph, int k, int edge_mode, int64_t base_offset, int seed, int64_t edge_capacity,
                      int64_t *nodes, int64_t *edge_index_out, int64_t *edge_ptr, int64_t *edge_src, int64_t *total_edges_out) {
    if (edge_mode < 0 || edge_mode > 2) return fail(UGS_E_BAD_MODE, "edge_mode must be one of: 'local', 'flat', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (edge_capacity < 0 || !edge_ptr || !total_edges_out) return fail(UGS_E_BAD_ARG, "null output pointer or negative edge_capacity");
    if (m_per_graph > 0 && (!nodes || (edge_capacity > 0 && (!edge_index_out || !edge_src)))) return fail(UGS_E_BAD_ARG, "null output pointer");
    auto g = lookup(handle);
    if (!g) return fail(UGS_E_INVALID_HANDLE, "Invalid preproc handle");
    if (g->n == 0) return fail(UGS_E_NO_ROOTS, "No viable roots available");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    ugs_plan *plan = nullptr;
    if (int rc = ugs_plan_create_handle(handle, &plan)) return rc;
    StreamCall sc;
    if (int rc = device_ctx(sc.dc)) { plan_unref(plan); return rc; }
    sc.G = plan->G; sc.m = m_per_graph; sc.k = k; sc.mode = edge_mode; sc.extra = edge_mode == UGS_EDGE_GLOBAL ? base_offset : 0; sc.seed = seed;
    sc.cap = edge_capacity;
    sc.nodes = nodes; sc.edge_index = edge_index_out; sc.edge_ptr = edge_ptr; sc.sample_ptr = nullptr; sc.edge_src = edge_src;
    sc.total_out = total_edges_out;
    const int rc = stream_rows(plan, sc);
    if (rc != UGS_OK) { if (sc.cs) (void)hipStreamSynchronize(sc.cs); (void)hipStreamSynchronize(sc.dc.stream); }
    sc.release();
    plan_unref(plan);
    return rc;
}

// ---- epsilon_uniform_sampler.sample_batch (reference src/samplers/epsilon_uniform_sampler/src/epsilon_uniform_sampler.cpp) ----
// Body of ugs_eps_sample_batch_begin (seeds == nullptr: `seed` keys every row) and ugs_eps_sample_graphs_begin (seeds: one per graph,
// uploaded in the adjacency blob).
static int eps_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                     int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds, double epsilon, ugs_job **job_out,
                     int64_t *total_edges_out) {
    if (!job_out || !ptr || num_graphs < 0 || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    if (!(epsilon > 0.0 && epsilon <= 1.0)) return fail(UGS_E_BAD_ARG, "epsilon must be in (0, 1]");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (num_cols >= ((int64_t)1 << 30)) return fail(UGS_E_UNSUPPORTED, "batch too large: columns must be < 2^30");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    const int64_t G = num_graphs, E = num_cols;
    const int64_t *src = edge_index, *dst = edge_index + row_stride;
    std::vector<int64_t> cstart, cols_of;
    assign_columns(src, dst, E, ptr, G, cstart, cols_of);
    // adjacency lists in the reference's push_back order (:152-176): column order, source row then destination row
    int64_t nrows = 0, nnz = 2 * (int64_t)cols_of.size();
    for (int64_t g = 0; g < G; ++g) nrows += std::max<int64_t>(ptr[g + 1] - ptr[g], 0) + 1;
    if (nnz >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large");
    const int64_t rows = G * (int64_t)m_per_graph;
    BlobLayout L;
    const size_t off_desc = L.take((size_t)G * sizeof(UgsGraphDesc)), off_row = L.take((size_t)nrows * sizeof(int64_t)),
                 off_nbr = L.take((size_t)nnz * sizeof(int32_t)), off_ecs = L.take((size_t)nnz * sizeof(int32_t)),
                 off_seeds = L.take(seeds ? (size_t)G * sizeof(uint64_t) : 0);
    L.end_inputs();
    const size_t off_counts = L.take((size_t)rows * sizeof(uint32_t)), off_st = L.take((size_t)ugs_scan_tmp_words(rows) * sizeof(int64_t));
    std::vector<char> host(L.in_bytes, 0);
    if (seeds && G > 0) std::memcpy(host.data() + off_seeds, seeds, (size_t)G * sizeof(uint64_t));
    auto *desc = reinterpret_cast<UgsGraphDesc *>(host.data() + off_desc);
    auto *rowp = reinterpret_cast<int64_t *>(host.data() + off_row);
    auto *nbr = reinterpret_cast<int32_t *>(host.data() + off_nbr);
    auto *ecs = reinterpret_cast<int32_t *>(host.data() + off_ecs);
    int64_t rb = 0, ab = 0;
    std::vector<int64_t> wr;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t lo = ptr[g], n = std::max<int64_t>(ptr[g + 1] - ptr[g], 0);
        if (n >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "graph too large");
        UgsGraphDesc &d = desc[g];
        d.node_lo = lo; d.rbase = rb; d.vbase = 0; d.viable_base = 0; d.n = (int32_t)n; d.level = 0; d.n_viable = 0; d.pad = 0;
        const int64_t c0 = cstart[(size_t)g], cn = cstart[(size_t)g + 1] - c0;
        for (int64_t r = 0; r <= n; ++r) rowp[rb + r] = 0;
        for (int64_t t = 0; t < cn; ++t) { const int64_t j = cols_of[(size_t)(c0 + t)]; ++rowp[rb + (src[j] - lo) + 1]; ++rowp[rb + (dst[j] - lo) + 1]; }
        for (int64_t r = 0; r < n; ++r) rowp[rb + r + 1] += rowp[rb + r];
        wr.assign(rowp + rb, rowp + rb + n);
        for (int64_t t = 0; t < cn; ++t) {
            const int64_t j = cols_of[(size_t)(c0 + t)], u = src[j] - lo, v = dst[j] - lo;
            int64_t a = ab + wr[(size_t)u]++; nbr[a] = (int32_t)v; ecs[a] = (int32_t)(2 * j);
            int64_t b = ab + wr[(size_t)v]++; nbr[b] = (int32_t)u; ecs[b] = (int32_t)(2 * j + 1);
        }
        for (int64_t r = 0; r <= n; ++r) rowp[rb + r] += ab;
        rb += n + 1; ab += 2 * cn;
    }
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, UGS_JOB_EPS, G, m_per_graph, k, mode, L.off, &j)) return rc;
    char *base = static_cast<char *>(j->blob.p);
    UgsEpsLaunch l{};
    l.graphs = reinterpret_cast<const UgsGraphDesc *>(base + off_desc);
    l.rowptr = reinterpret_cast<const int64_t *>(base + off_row);
    l.nbr = reinterpret_cast<const int32_t *>(base + off_nbr);
    l.ecs = reinterpret_cast<const int32_t *>(base + off_ecs);
    l.num_graphs = G; l.m = m_per_graph; l.k = k; l.mode = mode;
    l.max_attempts = std::max(10, (int)(10.0 / epsilon));
    l.seed = seed; l.seeds = seeds ? reinterpret_cast<const uint64_t *>(base + off_seeds) : nullptr;
    l.epsilon = epsilon; l.rows = rows;
    l.nodes = static_cast<int64_t *>(j->nodes.p); l.counts = reinterpret_cast<uint32_t *>(base + off_counts);
    hipError_t e = hipMemcpyAsync(base, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_eps_launch(l, 0, dc.cus, dc.stream);
    if (e == hipSuccess) e = ugs_launch_scan(l.counts, rows, j->d_eptr, reinterpret_cast<int64_t *>(base + off_st), dc.stream);
    if (int rc = side_job_total(j, e, "epsilon walk")) return rc;
    j->fill = [l, d_eptr = j->d_eptr, cus = dc.cus](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
        UgsEpsLaunch f = l;
        f.edge_ptr = d_eptr; f.edge_index = edge_index; f.edge_src = edge_src; f.ld = ld;
        return ugs_eps_launch(f, 1, cus, s);
    };
    return hand_out(j, job_out, total_edges_out);
}

int ugs_eps_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                               int m_per_graph, int k, int mode, uint64_t seed, double epsilon, ugs_job **job_out, int64_t *total_edges_out) {
    return eps_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, seed, nullptr, epsilon, job_out, total_edges_out);
}

// ---- epsilon_uniform_sampler.sample_graphs: one seed per graph (the law is stated in include/ugs_mi355.h) ----
int ugs_eps_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                                int m_per_graph, int k, int mode, const uint64_t *seeds, double epsilon, int32_t *graph_status,
                                ugs_job **job_out, int64_t *total_edges_out) {
    if (num_graphs > 0 && !seeds) return fail(UGS_E_BAD_ARG, "sample_graphs needs one seed per graph");
    const int rc = eps_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, 0, seeds, epsilon, job_out, total_edges_out);
    if (rc == UGS_OK && graph_status) std::fill(graph_status, graph_status + num_graphs, 0);   // no graph of this sampler fails alone
    return rc;
}

int ugs_eps_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                int64_t *edge_src, int dst_is_device) {
    if (!job || job->kind != UGS_JOB_EPS) return fail(UGS_E_BAD_ARG, "not an epsilon job");
    return finish_common(job, nodes, edge_index, edge_ptr, sample_ptr, edge_src, dst_is_device);
}

// ---- uniform_sampler.sample_batch (reference src/samplers/uniform_sampler/src/uniform_sampler.cpp) ----
// Vertices per graph up to which the sampler enumerates (64: masks only; above: the wide form) and up to which a graph takes the
// mask form (testing aid).  Process-wide; a call reads both once.  First use takes UGS_UNIFORM_MAX_VERTICES from the environment.
static std::mutex g_uni_limit_mu;
static int g_uni_max_vertices = 64, g_uni_mask_vertices = 64;
static void uniform_limits(int *max_vertices, int *mask_vertices) {
    static std::once_flag once;
    std::call_once(once, [] {
        const char *e = std::getenv("UGS_UNIFORM_MAX_VERTICES");
        if (!e || !*e) return;
        char *end = nullptr;
        const long long v = std::strtoll(e, &end, 10);
        if (end && *end == 0 && v >= 64 && v <= UGS_UNI_WIDE_MAX_N) g_uni_max_vertices = (int)v;
        else if (debug_on()) std::fprintf(stderr, "[UGS INFO] UGS_UNIFORM_MAX_VERTICES=%s ignored: must be 64 ... %d\n", e, UGS_UNI_WIDE_MAX_N);
    });
    std::lock_guard<std::mutex> lk(g_uni_limit_mu);
    if (max_vertices) *max_vertices = g_uni_max_vertices;
    if (mask_vertices) *mask_vertices = g_uni_mask_vertices;
}

int ugs_uniform_set_max_vertices(int n, int *previous) {
    int cur = 0;
    uniform_limits(&cur, nullptr);                                      // the environment's value first, so that it cannot overwrite this one later
    if (n < 64 || n > UGS_UNI_WIDE_MAX_N)
        return fail(UGS_E_BAD_ARG, "uniform_sampler vertex limit must be 64 ... " + std::to_string(UGS_UNI_WIDE_MAX_N) + " (got " + std::to_string(n) +
                                       ", still " + std::to_string(cur) + ")");
    std::lock_guard<std::mutex> lk(g_uni_limit_mu);
    if (previous) *previous = g_uni_max_vertices;
    g_uni_max_vertices = n;
    return UGS_OK;
}
int ugs_uniform_max_vertices(void) {
    int cur = 0;
    uniform_limits(&cur, nullptr);
    return cur;
}
int ugs_uniform_set_mask_vertices(int n, int *previous) {
    int cur = 0;
    uniform_limits(nullptr, &cur);
    if (n < 0 || n > 64)
        return fail(UGS_E_BAD_ARG, "uniform_sampler mask threshold must be 0 ... 64 (got " + std::to_string(n) + ", still " + std::to_string(cur) + ")");
    std::lock_guard<std::mutex> lk(g_uni_limit_mu);
    if (previous) *previous = g_uni_mask_vertices;
    g_uni_mask_vertices = n;
    return UGS_OK;
}

// seeds == nullptr: sample_batch, one generator for the call; otherwise sample_graphs: graph g draws from seeds[g], and a graph whose
// one-graph call would be refused (more vertices than the limit in force or than its k allows, |S_g| past the budget) fails alone,
// graph_status[g] = 1.
// what = UNI_ENUMERATE / UNI_COUNT (ugs_uniform_enumerate_begin / ugs_uniform_count_graphs): no generator and no draws; `cap` (max_rows /
// limit) takes the budget's place, per graph as in sample_graphs, graph_status[g] = 1 for a size refusal and 2 for a graph past cap.
// UNI_ENUMERATE: m_per_graph = 0, one row per set, *rows_out = their number.  UNI_COUNT: no job; counts_out[g] = |S_g|, -1 where refused.
// UNI_POPULATE (ugs_uniform_population_add): UNI_ENUMERATE up to its first read-back; `populate` then takes the sorted keys, and no job
// is handed out.
// UNI_DISTINCT (ugs_uniform_distinct_begin): UNI_SAMPLE with per-graph seeds and uni_draw_distinct for the draws; valid_out[g] =
// min(m, |S_g|) from the per-graph counts that come back with the status words.
enum { UNI_SAMPLE = 0, UNI_ENUMERATE, UNI_COUNT, UNI_POPULATE, UNI_DISTINCT };
using UniPopulate = std::function<int(const UgsUniCall &c, const UgsUniWide &w, const std::vector<UgsUniGraph> &gd, const std::vector<int64_t> &gsize,
                                      const int32_t *graph_status, const DeviceCtx &dc)>;
static int uniform_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                         int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds, int32_t *graph_status,
                         ugs_job **job_out, int64_t *total_edges_out, int what = UNI_SAMPLE, int64_t cap = UGS_UNI_BUDGET,
                         int64_t *rows_out = nullptr, int64_t *counts_out = nullptr, const UniPopulate *populate = nullptr,
                         int64_t *valid_out = nullptr) {
    if ((!job_out && what != UNI_COUNT && what != UNI_POPULATE) || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index))
        return fail(UGS_E_BAD_ARG, what == UNI_DISTINCT ? "bad arguments to sample_distinct" : "bad arguments to sample_batch");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    const bool per_graph = seeds != nullptr || what != UNI_SAMPLE;
    if (per_graph && num_graphs >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 2^31 - 1");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 0) return fail(UGS_E_BAD_ARG, "k must be >= 0");
    if (num_cols >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: columns must be < 2^31 - 1");
    const int64_t G = num_graphs, E = num_cols;
    int max_vertices = 64, mask_vertices = 64;                          // the limits in force for this call
    uniform_limits(&max_vertices, &mask_vertices);
    std::vector<UgsUniGraph> gd((size_t)G);
    std::vector<int32_t> too_big;
    int64_t nv = 0, nv_wide = 0, adj_words = 0;
    if (int rc = scan_ptr(ptr, G, per_graph, too_big, [&](int64_t g, int64_t n, std::string &why) {
            const bool wanted = k >= 1 && n >= k;
            int b = 1;                                                  // field width of the wide key: bit length of n - 1
            while (b < 62 && ((int64_t)1 << b) < n) ++b;
            const bool key_fits = k <= UGS_UNI_WIDE_MAX_K && (int64_t)k * b <= 64;
            const bool over = wanted && n > 64 && (n > max_vertices || !key_fits);
            if (over)
                why = "uniform_sampler: graph " + std::to_string(g) + " has " + std::to_string(n) +
                      (n > max_vertices ? " vertices; graphs of more than " + std::to_string(max_vertices) + " vertices (and at least k) are not supported"
                                        : " vertices; a graph of more than 64 vertices (limit in force: " + std::to_string(max_vertices) +
                                              ") needs k <= 8 and k * b <= 64, b = the bit length of n - 1 (here k = " + std::to_string(k) +
                                              ", b = " + std::to_string(b) + ")");
            UgsUniGraph &d = gd[(size_t)g];
            d.lo = ptr[g]; d.n = (int32_t)std::min<int64_t>(n, INT32_MAX); d.vbase = 0;
            d.enumerable = !wanted || over ? 0 : n > 64 || (n > mask_vertices && key_fits) ? 2 : 1;
            if (d.enumerable == 1) { d.vbase = nv; nv += n; }
            if (d.enumerable == 2) nv_wide += n;
            return over;
        })) return rc;
    // the enumerated vertices: the mask graphs' first, the wide graphs' after them
    const int64_t nv_mask = nv;
    std::vector<int64_t> wbase(nv_wide > 0 ? (size_t)G : 0, -1);
    for (int64_t g = 0; nv_wide > 0 && g < G; ++g) {
        UgsUniGraph &d = gd[(size_t)g];
        if (d.enumerable != 2) continue;
        d.vbase = nv; nv += d.n;
        wbase[(size_t)g] = adj_words; adj_words += (int64_t)d.n * ((d.n + 63) / 64);
    }
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    const bool sampling = what == UNI_SAMPLE || what == UNI_DISTINCT, counting = what == UNI_COUNT;
    const int64_t rows = G * (int64_t)m_per_graph, items = nv * 64, budget = nv > 0 ? cap : 0;   // (enumerate: m = 0, its rows come later)
    const int64_t keys = counting ? 0 : budget;                         // counting stores no keys and scans nothing
    // one blob: inputs first (uploaded in one copy), then the scratch of every stage
    BlobLayout L;
    auto take = [&](size_t bytes) { return L.take(bytes); };
    const BatchInputs in(L, E, G, sizeof(UgsUniGraph), seeds != nullptr);
    const bool wide = nv_wide > 0;                                      // a call without wide graphs allocates nothing for them
    const size_t o_vg = take((size_t)nv * 4), o_wb = wide ? take((size_t)G * 8) : 0;
    L.end_inputs();
    const size_t o_wadj = wide ? take((size_t)adj_words * 8) : 0, o_wp = wide ? take((size_t)E * 4) : 0,
                 o_gzm = wide && sampling ? take((size_t)G * 8) : 0, o_rk = wide && sampling ? take((size_t)rows * 8) : 0;
    const size_t o_gc = take(per_graph ? (size_t)G * 8 : 0);
    const size_t cub_bytes = counting ? ugs_uniform_cub_bytes(E, 0, 0) : ugs_uniform_cub_bytes(E, nv, budget);
    const size_t o_cub = take(cub_bytes), o_ck = take((size_t)E * 4), o_ck2 = take((size_t)E * 4), o_cv = take((size_t)E * 4),
                 o_cv2 = take((size_t)E * 4), o_cst = take((size_t)(G + 1) * 8), o_bp = take((size_t)E * 2), o_adj = take((size_t)nv * 8),
                 o_ic = take((size_t)items * 4), o_status = take(4 * 8);
    // (enumerate scans the edge counts of up to `budget` rows)
    const size_t o_io = counting ? 0 : take((size_t)(items + 1) * 8),
                 o_st = counting ? 0 : take((size_t)ugs_scan_tmp_words(std::max(items, sampling ? rows : budget)) * 8),
                 o_sl = counting ? 0 : take((size_t)nv * 4), o_sh = counting ? 0 : take((size_t)nv * 4),
                 o_ka = counting ? 0 : take((size_t)keys * 8), o_kb = counting ? 0 : take((size_t)keys * 8),
                 o_gs = counting ? 0 : take((size_t)G * 8), o_gz = counting ? 0 : take((size_t)G * 8);
    const size_t o_np = sampling ? take((size_t)G * 4) : 0, o_nl = sampling ? take((size_t)G * 4) : 0, o_dr = sampling ? take((size_t)rows * 4) : 0,
                 o_rm = sampling ? take((size_t)rows * 8) : 0, o_ec = sampling ? take((size_t)rows * 4) : 0;
    const size_t o_sp = what == UNI_ENUMERATE ? take((size_t)(G + 1) * 8) : 0;
    std::vector<char> host(L.in_bytes, 0);
    in.stage(host.data(), edge_index, row_stride, E, ptr, G, gd.data(), sizeof(UgsUniGraph), seeds);
    if (wide) std::memcpy(host.data() + o_wb, wbase.data(), (size_t)G * 8);
    auto *vg = reinterpret_cast<int32_t *>(host.data() + o_vg);
    for (int64_t g = 0; g < G; ++g)
        if (gd[(size_t)g].enumerable) for (int32_t v = 0; v < gd[(size_t)g].n; ++v) vg[gd[(size_t)g].vbase + v] = (int32_t)g;
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, sampling ? UGS_JOB_UNIFORM : UGS_JOB_UNIFORM_ENUM, G, m_per_graph, k, mode, L.off, &j, !sampling)) return rc;
    auto bail = [&](int rc) { free_job(j); return rc; };
    char *b = static_cast<char *>(j->blob.p);
    UgsUniCall c{};
    c.G = G; c.E = E; c.nv = nv; c.rows = rows; c.budget = budget; c.m = m_per_graph; c.k = k; c.mode = mode; c.seed = seed;
    c.seeds = seeds ? reinterpret_cast<const uint64_t *>(b + in.seeds) : nullptr;
    c.per_graph = per_graph ? 1 : 0;
    c.distinct = what == UNI_DISTINCT ? 1 : 0;
    c.gcount = per_graph ? reinterpret_cast<int64_t *>(b + o_gc) : nullptr;
    c.src = reinterpret_cast<const int64_t *>(b + in.src); c.dst = reinterpret_cast<const int64_t *>(b + in.dst);
    c.ptr = reinterpret_cast<const int64_t *>(b + in.ptr); c.graphs = reinterpret_cast<const UgsUniGraph *>(b + in.desc);
    c.vgraph = reinterpret_cast<const int32_t *>(b + o_vg);
    c.cub_tmp = b + o_cub; c.cub_bytes = cub_bytes;
    c.ckey = reinterpret_cast<uint32_t *>(b + o_ck); c.ckey2 = reinterpret_cast<uint32_t *>(b + o_ck2);
    c.cval = reinterpret_cast<int32_t *>(b + o_cv); c.cval2 = reinterpret_cast<int32_t *>(b + o_cv2);
    c.cstart = reinterpret_cast<int64_t *>(b + o_cst); c.bpair = reinterpret_cast<uint16_t *>(b + o_bp);
    c.adj = reinterpret_cast<uint64_t *>(b + o_adj); c.icount = reinterpret_cast<uint32_t *>(b + o_ic);
    c.ioff = reinterpret_cast<int64_t *>(b + o_io); c.scan_tmp = reinterpret_cast<int64_t *>(b + o_st);
    c.seg_lo = reinterpret_cast<int32_t *>(b + o_sl); c.seg_hi = reinterpret_cast<int32_t *>(b + o_sh);
    c.keys_a = reinterpret_cast<uint64_t *>(b + o_ka); c.keys_b = reinterpret_cast<uint64_t *>(b + o_kb);
    c.gstart = reinterpret_cast<int64_t *>(b + o_gs); c.gsize = reinterpret_cast<int64_t *>(b + o_gz);
    c.nepos = reinterpret_cast<int32_t *>(b + o_np); c.ne_list = reinterpret_cast<int32_t *>(b + o_nl);
    c.draws = reinterpret_cast<int32_t *>(b + o_dr); c.rowmask = reinterpret_cast<uint64_t *>(b + o_rm);
    c.ecount = reinterpret_cast<uint32_t *>(b + o_ec); c.status = reinterpret_cast<int64_t *>(b + o_status);
    if (sampling) { c.nodes = static_cast<int64_t *>(j->nodes.p); c.edge_ptr = j->d_eptr; }
    UgsUniWide w{};
    w.nv_mask = nv_mask; w.adj_words = adj_words;
    if (wide) {
        w.wbase = reinterpret_cast<const int64_t *>(b + o_wb); w.wadj = reinterpret_cast<uint64_t *>(b + o_wadj);
        w.wpair = reinterpret_cast<uint32_t *>(b + o_wp); w.gsize_mask = reinterpret_cast<int64_t *>(b + o_gzm);
        w.rowkey = reinterpret_cast<uint64_t *>(b + o_rk);
    }
    int64_t status[4] = {0, 0, 0, 0};
    std::vector<int64_t> gcount(per_graph && nv > 0 ? (size_t)G : 0, 0);   // per-graph subset counts: read back once, with the total
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (!sampling) {
        // the count pass (count: nothing else; enumerate: through the sorts), then the first read-back: the graphs' counts and sizes
        std::vector<int64_t> gsize(!counting && nv > 0 ? (size_t)G : 0, 0);
        if (e == hipSuccess) e = counting ? ugs_uniform_count(c, w, dc.stream) : ugs_uniform_enum_keys(c, w, dc.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(status, c.status, sizeof(status), hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess && !gcount.empty()) e = hipMemcpyAsync(gcount.data(), c.gcount, (size_t)G * 8, hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess && !gsize.empty()) e = hipMemcpyAsync(gsize.data(), c.gsize, (size_t)G * 8, hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
        if (e != hipSuccess) return bail(fail_hip(e, "uniform_sampler pipeline"));
        for (int64_t g = 0; g < G; ++g) {
            const bool past = !gcount.empty() && gd[(size_t)g].enumerable && gcount[(size_t)g] > budget;
            graph_status[g] = too_big[(size_t)g] ? 1 : past ? 2 : 0;
            if (counting) counts_out[g] = graph_status[g] ? -1 : gcount.empty() ? 0 : gcount[(size_t)g];
        }
        if (counting) return bail(UGS_OK);
        if (status[1])
            return bail(fail(UGS_E_UNSUPPORTED, "uniform_sampler: the call's graphs together have " + std::to_string(status[0]) +
                                                " connected k-subsets, more than max_rows = " + std::to_string(cap) + "; split the call"));
        if (what == UNI_POPULATE) return bail((*populate)(c, w, gd, gsize, graph_status, dc));
        // sample_ptr: the sizes scanned in batch order (the keys lie in the order of the enumerated vertices, mask graphs first)
        j->sample_ptr.assign((size_t)G + 1, 0);
        for (int64_t g = 0; g < G; ++g) j->sample_ptr[(size_t)g + 1] = j->sample_ptr[(size_t)g] + (gsize.empty() ? 0 : gsize[(size_t)g]);
        const int64_t R = j->sample_ptr[(size_t)G];
        if (int rc = side_job_rows(j, R, (size_t)R * 4)) return rc;    // nodes and edge_ptr by R, the per-row edge counts behind them
        c.rows = R; c.nodes = static_cast<int64_t *>(j->nodes.p); c.edge_ptr = j->d_eptr;
        c.ecount = reinterpret_cast<uint32_t *>(j->d_eptr + R + 1);
        c.sptr = reinterpret_cast<const int64_t *>(b + o_sp);
        e = hipMemcpyAsync(b + o_sp, j->sample_ptr.data(), (size_t)(G + 1) * 8, hipMemcpyHostToDevice, dc.stream);
        if (e == hipSuccess) e = ugs_uniform_enum_rows(c, w, dc.stream);
        if (int rc = side_job_total(j, e, "uniform_sampler enumeration")) return rc;    // the second read-back: the edge total
        if (rows_out) *rows_out = R;
        j->fill = [c, w](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) { return ugs_uniform_enum_fill(c, w, edge_index, edge_src, ld, s); };
        return hand_out(j, job_out, total_edges_out);
    }
    if (e == hipSuccess) e = ugs_uniform_begin(c, w, dc.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(status, c.status, sizeof(status), hipMemcpyDeviceToHost, dc.stream);
    if (e == hipSuccess && !gcount.empty()) e = hipMemcpyAsync(gcount.data(), c.gcount, (size_t)G * 8, hipMemcpyDeviceToHost, dc.stream);
    if (int rc = side_job_total(j, e, "uniform_sampler pipeline")) return rc;
    if (status[1] && per_graph)
        return bail(fail(UGS_E_UNSUPPORTED, "uniform_sampler: the call's graphs together have " + std::to_string(status[0]) +
                                            " connected k-subsets, more than the device budget of " + std::to_string(budget) +
                                            "; split the call"));
    if (status[1])
        return bail(fail(UGS_E_UNSUPPORTED, "uniform_sampler: the batch has more than " + std::to_string(budget) +
                                            " connected k-subsets (the device budget; " + std::to_string(status[0]) + " counted before stopping)"));
    for (int64_t g = 0; per_graph && g < G; ++g)
        graph_status[g] = too_big[(size_t)g] || (!gcount.empty() && gd[(size_t)g].enumerable && gcount[(size_t)g] > budget) ? 1 : 0;
    for (int64_t g = 0; valid_out && g < G; ++g)                        // a healthy graph's count is its |S_g|
        valid_out[g] = graph_status[g] || gcount.empty() || !gd[(size_t)g].enumerable ? 0 : std::min<int64_t>(m_per_graph, gcount[(size_t)g]);
    j->fill = [c, w](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) { return ugs_uniform_fill(c, w, edge_index, edge_src, ld, s); };
    return hand_out(j, job_out, total_edges_out);
}

int ugs_uniform_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                                   int m_per_graph, int k, int mode, uint64_t seed, ugs_job **job_out, int64_t *total_edges_out) {
    return uniform_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, seed, nullptr, nullptr, job_out,
                         total_edges_out);
}

int ugs_uniform_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                                    int64_t num_graphs, int m_per_graph, int k, int mode, const uint64_t *seeds, int32_t *graph_status,
                                    ugs_job **job_out, int64_t *total_edges_out) {
    if (num_graphs > 0 && (!seeds || !graph_status)) return fail(UGS_E_BAD_ARG, "sample_graphs needs seeds and graph_status");
    static const uint64_t no_graphs = 0;                                // num_graphs == 0 still takes the per-graph path
    int32_t no_status = 0;
    return uniform_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, 0, seeds ? seeds : &no_graphs,
                         graph_status ? graph_status : &no_status, job_out, total_edges_out);
}

// ---- uniform_sampler.sample_distinct: m distinct sets per graph, the whole population when it has at most m (the law is stated in
//      include/ugs_mi355.h).  The checks that are this call's own, for both begins, before any device work. ----
static int distinct_checks(int64_t num_graphs, int m_per_graph, const uint64_t *seeds, const int32_t *graph_status, const int64_t *valid_out) {
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (m_per_graph > UGS_UNI_DISTINCT_MAX_M)
        return fail(UGS_E_UNSUPPORTED, "uniform_sampler sample_distinct: m_per_graph must be <= " + std::to_string(UGS_UNI_DISTINCT_MAX_M) +
                                           " (got " + std::to_string(m_per_graph) + "): a graph's draws are resolved in one workgroup's LDS");
    if (num_graphs > 0 && (!seeds || !graph_status || !valid_out)) return fail(UGS_E_BAD_ARG, "sample_distinct needs seeds, graph_status and valid");
    return UGS_OK;
}

int ugs_uniform_distinct_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                               int m_per_graph, int k, int mode, const uint64_t *seeds, int32_t *graph_status, int64_t *valid_out,
                               ugs_job **job_out, int64_t *total_edges_out) {
    if (int rc = distinct_checks(num_graphs, m_per_graph, seeds, graph_status, valid_out)) return rc;
    static const uint64_t no_graphs = 0;                                // num_graphs <= 0: nothing is read or written through these
    int32_t no_status = 0;
    return uniform_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, 0, seeds ? seeds : &no_graphs,
                         graph_status ? graph_status : &no_status, job_out, total_edges_out, UNI_DISTINCT, UGS_UNI_BUDGET, nullptr, nullptr,
                         nullptr, valid_out);
}

int ugs_uniform_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                    int64_t *edge_src, int dst_is_device) {
    if (!job || job->kind != UGS_JOB_UNIFORM) return fail(UGS_E_BAD_ARG, "not a uniform_sampler job");
    return finish_common(job, nodes, edge_index, edge_ptr, sample_ptr, edge_src, dst_is_device);
}

// ---- uniform_sampler.count_graphs / enumerate_graphs: the population the sampler draws from (the law is stated in include/ugs_mi355.h) ----
int ugs_uniform_count_graphs(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int k,
                             int64_t limit, int64_t *counts_out, int32_t *graph_status) {
    if (limit < 1 || limit > ((int64_t)1 << 32)) return fail(UGS_E_BAD_ARG, "limit must be 1 ... 2^32 (got " + std::to_string(limit) + ")");
    if (num_graphs > 0 && (!counts_out || !graph_status)) return fail(UGS_E_BAD_ARG, "count_graphs needs counts_out and graph_status");
    return uniform_begin(edge_index, row_stride, num_cols, ptr, num_graphs, 0, k, 0, 0, nullptr, graph_status, nullptr, nullptr, UNI_COUNT, limit,
                         nullptr, counts_out);
}

int ugs_uniform_enumerate_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int k,
                                int mode, int64_t max_rows, int32_t *graph_status, ugs_job **job_out, int64_t *total_rows_out,
                                int64_t *total_edges_out) {
    if (max_rows < 1 || max_rows > UGS_UNI_BUDGET) return fail(UGS_E_BAD_ARG, "max_rows must be 1 ... 2^25 (got " + std::to_string(max_rows) + ")");
    if (num_graphs > 0 && !graph_status) return fail(UGS_E_BAD_ARG, "enumerate_graphs needs graph_status");
    if (!total_rows_out) return fail(UGS_E_BAD_ARG, "total_rows_out is null");
    return uniform_begin(edge_index, row_stride, num_cols, ptr, num_graphs, 0, k, mode, 0, nullptr, graph_status, job_out, total_edges_out,
                         UNI_ENUMERATE, max_rows, total_rows_out);
}

int ugs_uniform_enumerate_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr, int64_t *edge_src,
                                 int dst_is_device) {
    if (!job || job->kind != UGS_JOB_UNIFORM_ENUM) return fail(UGS_E_BAD_ARG, "not a uniform_sampler enumeration job");
    return finish_common(job, nodes, edge_index, edge_ptr, sample_ptr, edge_src, dst_is_device);
}

// ---- uniform_sampler.PopulationCache: every graph enumerated once, sample calls served from the stored keys (the law is stated in
//      include/ugs_mi355.h at ugs_uniform_population_create) ----
namespace {
struct PopSlot {
    const uint64_t *keys = nullptr;   // in a block of the population; nullptr: S_g is empty or the graph failed
    int64_t size = 0;                 // |S_g|; -1: the graph failed at add time
    uint64_t fp = 0;                  // fingerprint of its adjacency (ugs_device.h)
    int32_t n = 0, form = 0, b = 0;   // vertices; 1: mask keys, 2: wide keys of b-bit fields, 0: not enumerated
    const int32_t *cls = nullptr;     // WL population: the class index of each key, in the block beside the keys' (nullptr: no keys)
    uint64_t lfp = 0;                 // WL population: fingerprint of its loop vertices (ugs_device.h)
};
struct PopBlock { uint64_t *p = nullptr; int64_t cap = 0, used = 0; int32_t *c = nullptr; /* WL population: a class index per key */ };
struct PopDevMem {                    // device memory that goes with its last holder (a population's class table, an id array)
    void *p = nullptr;
    ~PopDevMem() { if (p) (void)hipFree(p); }
};
struct PopDigestHash { size_t operator()(const std::array<uint64_t, 2> &d) const { return (size_t)(d[0] ^ (d[1] * 0x9E3779B97F4A7C15ull)); } };
struct PopIdCache { uint64_t token = 0; int64_t classes = 0; std::shared_ptr<PopDevMem> ids; };
// Blocks are never moved or freed before the population dies, slots are only appended: what a job has read stays valid through any add.
struct PopState {
    int k = 0, dev = -1;
    int64_t block_keys = 0, keys = 0, bytes = 0;
    int cur = -1;                     // the block of block_keys keys that takes the next small graph
    std::shared_mutex mu;             // adds: exclusive; sample begins, sizes, info: shared
    std::deque<PopSlot> slots;
    std::vector<PopBlock> blocks;
    // WL class indices (ugs_uniform_population_create_wl; wl_iter < 0: a plain population).  The class table is written by adds only
    // (mu exclusive); a grown table is a new device array, the old one goes with the last job that read it.
    int wl_iter = -1, wl_labeled = -1;                        // labelling of the adds so far: -1 none yet, 0 degrees, 1 given labels
    int64_t wl_rows = 0, wl_tab_bytes = 0;                    // rows hashed; bytes of the device class table
    std::vector<std::array<uint64_t, 2>> classes;             // the distinct digests in class order
    std::unordered_map<std::array<uint64_t, 2>, int32_t, PopDigestHash> class_of;
    std::shared_ptr<PopDevMem> class_tab;                     // `classes` on the device, [C, 2] uint64, and C zero status words behind it
    int64_t class_tab_rows = 0;
    std::mutex wl_mu;                                         // the id arrays, one per vocabulary seen (sample begins hold mu shared)
    std::vector<PopIdCache> id_caches;
    ~PopState() { for (PopBlock &b : blocks) { (void)hipFree(b.p); if (b.c) (void)hipFree(b.c); } }
    // room for n keys, contiguous in one block (mu held exclusively); a WL population has n class indices beside them
    int take(int64_t n, uint64_t **out, int32_t **cls_out = nullptr) {
        const bool own = n > block_keys;
        if (own || cur < 0 || blocks[(size_t)cur].cap - blocks[(size_t)cur].used < n) {
            PopBlock b;
            b.cap = own ? n : block_keys;
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b.p), (size_t)b.cap * sizeof(uint64_t)));
            if (wl_iter >= 0) {
                if (hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.c), (size_t)b.cap * sizeof(int32_t)); e != hipSuccess) {
                    (void)hipFree(b.p);
                    return fail_hip(e, "hipMalloc");
                }
                bytes += b.cap * (int64_t)sizeof(int32_t);
            }
            blocks.push_back(b);
            bytes += b.cap * (int64_t)sizeof(uint64_t);
            if (own) { blocks.back().used = n; *out = b.p; if (cls_out) *cls_out = b.c; return UGS_OK; }
            cur = (int)blocks.size() - 1;
        }
        PopBlock &b = blocks[(size_t)cur];
        *out = b.p + b.used;
        if (cls_out) *cls_out = b.c ? b.c + b.used : nullptr;
        b.used += n;
        return UGS_OK;
    }
};
}  // namespace
struct ugs_uniform_population { std::shared_ptr<PopState> st; };

int ugs_uniform_population_create(int k, int64_t block_keys, ugs_uniform_population **pop_out) {
    if (!pop_out) return fail(UGS_E_BAD_ARG, "pop_out is null");
    if (k < 0) return fail(UGS_E_BAD_ARG, "k must be >= 0");
    if (block_keys < 1 || block_keys > ((int64_t)1 << 28))
        return fail(UGS_E_BAD_ARG, "block_keys must be 1 ... 2^28 (got " + std::to_string(block_keys) + ")");
    auto *p = new ugs_uniform_population();
    p->st = std::make_shared<PopState>();
    p->st->k = k; p->st->block_keys = block_keys;
    *pop_out = p;
    return UGS_OK;
}

int ugs_uniform_population_create_wl(int k, int64_t block_keys, int iterations, ugs_uniform_population **pop_out) {
    if (iterations < 0 || iterations > 8)                               // ugs_wl_hash's range (UGS_WL_MAX_ITER)
        return fail(UGS_E_UNSUPPORTED, "population: 0 <= wl iterations <= 8 (got " + std::to_string(iterations) + ")");
    if (k < 1 || k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "population: WL class indices need 1 <= k <= 32 (got " + std::to_string(k) + ")");
    if (int rc = ugs_uniform_population_create(k, block_keys, pop_out)) return rc;
    (*pop_out)->st->wl_iter = iterations;
    return UGS_OK;
}

int ugs_uniform_population_destroy(ugs_uniform_population *pop) {
    delete pop;                                                          // the storage goes with the last job that samples from it
    return UGS_OK;
}

// The WL stage of an add (mu held exclusively; c, w: the call behind enum_keys and ugs_uniform_pop_store).  The stored members are
// written out as the rows of mode "sample" with their edges -- enum_rows / enum_fill over a window of the call's sample_ptr, shifted so
// that the window's first row is row 0 -- and hashed by ugs_wl_hash / ugs_wl_hash_labeled, chunk after chunk; the digests come back
// to the host, which numbers the distinct ones, and the class indices go beside the keys.  Scratch per chunk: at most
// POP_WL_CHUNK_ROWS rows (nodes 8 k, edge_ptr 8, count 4, digest 16, status 4 bytes each: 17 MiB at k = 32) and POP_WL_CHUNK_EDGES edge
// entries of 24 bytes (192 MiB); a chunk with more entries is halved until it fits or is one row.
constexpr int64_t POP_WL_CHUNK_ROWS = (int64_t)1 << 16, POP_WL_CHUNK_EDGES = (int64_t)1 << 23;
static int population_wl_classes(PopState &st, const UgsUniCall &c, const UgsUniWide &w, const std::vector<int64_t> &size,
                                 const std::vector<int32_t *> &dcls, const int64_t *d_labels, int64_t num_labels, const DeviceCtx &dc) {
    const int64_t G = c.G;
    const int k = c.k;
    std::vector<int64_t> sptr((size_t)G + 1, 0), shifted((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; ++g) sptr[(size_t)g + 1] = sptr[(size_t)g] + size[(size_t)g];
    const int64_t R = sptr[(size_t)G];
    if (R == 0) return UGS_OK;
    const int64_t cap = std::min(R, POP_WL_CHUNK_ROWS);
    PoolBuf rb, eb;
    if (int rc = pool_get((size_t)cap * ((size_t)k * 8 + 8 + 16 + 4 + 4) + (size_t)(G + 2) * 8, dc.id, rb)) return rc;
    auto done = [&](int rc) { pool_put(rb); pool_put(eb); return rc; };
    int64_t *d_nodes = static_cast<int64_t *>(rb.p), *d_eptr = d_nodes + cap * k, *d_sptr = d_eptr + cap + 1;
    uint64_t *d_dig = reinterpret_cast<uint64_t *>(d_sptr + G + 1);
    uint32_t *d_ec = reinterpret_cast<uint32_t *>(d_dig + 2 * cap);
    int32_t *d_st = reinterpret_cast<int32_t *>(d_ec + cap);
    std::vector<int32_t> cls((size_t)R), hs((size_t)cap);
    std::vector<uint64_t> hd((size_t)cap * 2);
    hipStream_t s = dc.stream;
    for (int64_t r0 = 0, n = cap; r0 < R; r0 += n) {
        n = std::min(n, R - r0);
        UgsUniCall cc = c;
        int64_t total = 0;
        for (;;) {
            for (int64_t g = 0; g <= G; ++g) shifted[(size_t)g] = sptr[(size_t)g] - r0;
            cc.rows = n; cc.mode = 0; cc.sptr = d_sptr; cc.nodes = d_nodes; cc.edge_ptr = d_eptr; cc.ecount = d_ec;
            hipError_t e = hipMemcpyAsync(d_sptr, shifted.data(), (size_t)(G + 1) * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = ugs_uniform_enum_rows(cc, w, s);
            if (e == hipSuccess) e = hipMemcpyAsync(&total, d_eptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return done(fail_hip(e, "uniform_sampler population add (rows of the WL stage)"));
            if (total <= POP_WL_CHUNK_EDGES || n == 1) break;
            n = (n + 1) / 2;
        }
        const int64_t ld = std::max<int64_t>(total, 1);
        if (eb.bytes < (size_t)ld * 24) {
            pool_put(eb);
            if (int rc = pool_get((size_t)ld * 24, dc.id, eb)) return done(rc);
        }
        int64_t *d_ei = static_cast<int64_t *>(eb.p);
        if (hipError_t e = ugs_uniform_enum_fill(cc, w, d_ei, d_ei + 2 * ld, ld, s); e != hipSuccess)
            return done(fail_hip(e, "uniform_sampler population add (edges of the WL stage)"));
        if (int rc = d_labels ? ugs_wl_hash_labeled(d_nodes, d_ei, ld, total, d_eptr, n, k, st.wl_iter, d_labels, num_labels, d_dig, d_st)
                              : ugs_wl_hash(d_nodes, d_ei, ld, total, d_eptr, n, k, st.wl_iter, d_dig, d_st)) return done(rc);
        hipError_t e = hipMemcpyAsync(hd.data(), d_dig, (size_t)n * 16, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hs.data(), d_st, (size_t)n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return done(fail_hip(e, "uniform_sampler population add (digests of the WL stage)"));
        for (int64_t i = 0; i < n; ++i) {
            int32_t id = -1;                                             // no digest (status 3: a start label outside [0, 2^32))
            if (hs[(size_t)i] == 0) {
                const std::array<uint64_t, 2> d{hd[(size_t)i * 2], hd[(size_t)i * 2 + 1]};
                auto it = st.class_of.find(d);
                if (it == st.class_of.end()) {
                    it = st.class_of.emplace(d, (int32_t)st.classes.size()).first;
                    st.classes.push_back(d);
                }
                id = it->second;
            }
            cls[(size_t)(r0 + i)] = id;
        }
    }
    // the class indices beside the keys: graphs that lie one behind the other in a block go in one copy
    for (int64_t g = 0; g < G;) {
        if (size[(size_t)g] == 0) { ++g; continue; }
        int64_t h = g, len = 0;
        while (h < G && (size[(size_t)h] == 0 || dcls[(size_t)h] == dcls[(size_t)g] + len)) len += size[(size_t)h++];
        if (hipError_t e = hipMemcpy(dcls[(size_t)g], cls.data() + sptr[(size_t)g], (size_t)len * 4, hipMemcpyHostToDevice); e != hipSuccess)
            return done(fail_hip(e, "uniform_sampler population add (class indices)"));
        g = h;
    }
    // the class table on the device, for the id arrays of the sample calls: a new array when it has grown
    const int64_t C = (int64_t)st.classes.size();
    if (C > st.class_tab_rows) {
        auto tab = std::make_shared<PopDevMem>();
        hipError_t e = hipMalloc(&tab->p, (size_t)C * 20);
        if (e == hipSuccess) e = hipMemcpy(tab->p, st.classes.data(), (size_t)C * 16, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemsetAsync(static_cast<char *>(tab->p) + (size_t)C * 16, 0, (size_t)C * 4, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return done(fail_hip(e, "uniform_sampler population add (class table)"));
        st.bytes += C * 20 - st.wl_tab_bytes;
        st.wl_tab_bytes = C * 20;
        st.class_tab = tab; st.class_tab_rows = C;
    }
    st.wl_rows += R;
    return done(UGS_OK);
}

// d_labels (device, int64 [num_labels], one per vertex of the call) or nullptr: the start labels of a WL population's digests
static int population_add(ugs_uniform_population *pop, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                          int64_t num_graphs, int64_t max_rows, const int64_t *d_labels, int64_t num_labels, int64_t *slots_out,
                          int32_t *graph_status) {
    if (!pop) return fail(UGS_E_BAD_ARG, "population is null");
    if (max_rows < 1 || max_rows > UGS_UNI_BUDGET) return fail(UGS_E_BAD_ARG, "max_rows must be 1 ... 2^25 (got " + std::to_string(max_rows) + ")");
    if (num_graphs > 0 && (!slots_out || !graph_status)) return fail(UGS_E_BAD_ARG, "population add needs slots_out and graph_status");
    PopState &st = *pop->st;
    const int64_t G = num_graphs;
    const bool wl = st.wl_iter >= 0;                                     // (fixed at creation)
    const int labeled = d_labels ? 1 : 0;
    static const char *const mixed = "uniform_sampler population: every add of a WL population uses the same labelling (degrees, or given labels)";
    if (d_labels && !wl) return fail(UGS_E_BAD_ARG, "uniform_sampler population: labels given to a population created without WL iterations");
    if (d_labels && ptr && G > 0 && num_labels != ptr[G])
        return fail(UGS_E_BAD_ARG, "uniform_sampler population: " + std::to_string(num_labels) + " labels for " + std::to_string(ptr[G]) + " vertices");
    if (d_labels && ptr && ptr[0] != 0) return fail(UGS_E_BAD_ARG, "uniform_sampler population: an add with labels needs ptr[0] = 0");
    if (wl) {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        if (G > 0 && st.wl_labeled >= 0 && st.wl_labeled != labeled) return fail(UGS_E_BAD_ARG, mixed);
    }
    const UniPopulate store = [&](const UgsUniCall &c, const UgsUniWide &w, const std::vector<UgsUniGraph> &gd, const std::vector<int64_t> &gsize,
                                  const int32_t *status, const DeviceCtx &dc) -> int {
        std::unique_lock<std::shared_mutex> lk(st.mu);
        if (st.dev >= 0 && st.dev != dc.id)
            return fail(UGS_E_BAD_ARG, "the population lives on device " + std::to_string(st.dev) + ", this add runs on device " + std::to_string(dc.id));
        st.dev = dc.id;
        // host side of the copy: per graph the destination of its keys, then the fingerprints come back
        std::vector<uint64_t *> dst((size_t)G, nullptr);
        std::vector<int32_t *> dcls((size_t)G, nullptr);
        std::vector<int64_t> size((size_t)G, 0);
        for (int64_t g = 0; g < G; ++g) {
            const int64_t sz = status[g] || gsize.empty() ? 0 : gsize[(size_t)g];
            if (sz > 0) if (int rc = st.take(sz, &dst[(size_t)g], wl ? &dcls[(size_t)g] : nullptr)) return rc;
            size[(size_t)g] = sz;
        }
        PoolBuf tab;                                                     // dst [G], the fingerprints [G] and the loop fingerprints [G]
        if (int rc = pool_get((size_t)G * 24, dc.id, tab)) return rc;
        auto **d_dst = static_cast<uint64_t **>(tab.p);
        auto *d_fp = reinterpret_cast<uint64_t *>(d_dst + G);
        std::vector<uint64_t> fp((size_t)G * 2, 0);
        hipError_t e = hipMemcpyAsync(d_dst, dst.data(), (size_t)G * 8, hipMemcpyHostToDevice, dc.stream);
        if (e == hipSuccess) e = ugs_uniform_pop_store(c, w, d_dst, d_fp, dc.stream);
        if (e == hipSuccess && wl) e = ugs_uniform_pop_loops(c, nullptr, d_fp + G, dc.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(fp.data(), d_fp, (size_t)G * (wl ? 16 : 8), hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
        pool_put(tab);
        if (e != hipSuccess) return fail_hip(e, "uniform_sampler population add");
        if (wl) {
            if (st.wl_labeled >= 0 && st.wl_labeled != labeled) return fail(UGS_E_BAD_ARG, mixed);
            if (int rc = population_wl_classes(st, c, w, size, dcls, d_labels, num_labels, dc)) return rc;
            if (ptr[G] > ptr[0]) st.wl_labeled = labeled;                // (an add without vertices fixes nothing)
        }
        for (int64_t g = 0; g < G; ++g) {
            PopSlot s;
            const UgsUniGraph &d = gd[(size_t)g];
            s.n = d.n;
            if (status[g]) s.size = -1;
            else {
                s.form = d.enumerable; s.fp = fp[(size_t)g];
                s.size = gsize.empty() ? 0 : gsize[(size_t)g];
                s.keys = dst[(size_t)g];
                s.cls = dcls[(size_t)g]; s.lfp = fp[(size_t)(G + g)];
                int b = 1;
                while (b < 16 && (1 << b) < d.n) ++b;
                s.b = b;
                st.keys += s.size;
            }
            slots_out[g] = (int64_t)st.slots.size();
            st.slots.push_back(s);
        }
        return UGS_OK;
    };
    if (G == 0) return UGS_OK;
    return uniform_begin(edge_index, row_stride, num_cols, ptr, G, 0, st.k, 0, 0, nullptr, graph_status, nullptr, nullptr, UNI_POPULATE, max_rows,
                         nullptr, nullptr, &store);
}

int ugs_uniform_population_add(ugs_uniform_population *pop, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                               int64_t num_graphs, int64_t max_rows, int64_t *slots_out, int32_t *graph_status) {
    return population_add(pop, edge_index, row_stride, num_cols, ptr, num_graphs, max_rows, nullptr, 0, slots_out, graph_status);
}

int ugs_uniform_population_add_wl(ugs_uniform_population *pop, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                                  int64_t num_graphs, int64_t max_rows, const int64_t *d_labels, int64_t num_labels, int64_t *slots_out,
                                  int32_t *graph_status) {
    if (pop && pop->st->wl_iter < 0) return fail(UGS_E_BAD_ARG, "uniform_sampler population: created without WL iterations");
    return population_add(pop, edge_index, row_stride, num_cols, ptr, num_graphs, max_rows, d_labels, num_labels, slots_out, graph_status);
}

int ugs_uniform_population_wl_stats(ugs_uniform_population *pop, int64_t *classes_out, int64_t *rows_hashed_out) {
    if (!pop) return fail(UGS_E_BAD_ARG, "population is null");
    PopState &st = *pop->st;
    std::shared_lock<std::shared_mutex> lk(st.mu);
    if (classes_out) *classes_out = (int64_t)st.classes.size();
    if (rows_hashed_out) *rows_hashed_out = st.wl_rows;
    return UGS_OK;
}

int ugs_uniform_population_wl_digests(ugs_uniform_population *pop, int64_t capacity, uint64_t *digest_out, int64_t *count_out) {
    if (!pop || !count_out || capacity < 0 || (capacity > 0 && !digest_out)) return fail(UGS_E_BAD_ARG, "bad arguments to population wl_digests");
    PopState &st = *pop->st;
    std::shared_lock<std::shared_mutex> lk(st.mu);
    if (st.wl_iter < 0) return fail(UGS_E_BAD_ARG, "uniform_sampler population: created without WL iterations");
    *count_out = (int64_t)st.classes.size();
    if (capacity < *count_out) return UGS_OK;                            // (the caller asks again with room for count)
    std::vector<std::array<uint64_t, 2>> d = st.classes;
    std::sort(d.begin(), d.end());
    if (!d.empty()) std::memcpy(digest_out, d.data(), d.size() * 16);
    return UGS_OK;
}

int ugs_uniform_population_sizes(ugs_uniform_population *pop, const int64_t *slots, int64_t num_graphs, int64_t *sizes_out) {
    if (!pop || (num_graphs > 0 && (!slots || !sizes_out))) return fail(UGS_E_BAD_ARG, "bad arguments to population sizes");
    PopState &st = *pop->st;
    std::shared_lock<std::shared_mutex> lk(st.mu);
    for (int64_t g = 0; g < num_graphs; ++g) {
        if (slots[g] < 0 || slots[g] >= (int64_t)st.slots.size()) return fail(UGS_E_BAD_ARG, "unknown population slot " + std::to_string(slots[g]));
        sizes_out[g] = st.slots[(size_t)slots[g]].size;
    }
    return UGS_OK;
}

int ugs_uniform_population_info(ugs_uniform_population *pop, int64_t *slots_out, int64_t *keys_out, int64_t *bytes_out, int64_t *blocks_out) {
    if (!pop) return fail(UGS_E_BAD_ARG, "population is null");
    PopState &st = *pop->st;
    std::shared_lock<std::shared_mutex> lk(st.mu);
    if (slots_out) *slots_out = (int64_t)st.slots.size();
    if (keys_out) *keys_out = st.keys;
    if (bytes_out) *bytes_out = st.bytes;
    if (blocks_out) *blocks_out = (int64_t)st.blocks.size();
    return UGS_OK;
}

// valid_out != nullptr: the distinct call (ugs_uniform_population_distinct_begin) -- uni_draw_distinct draws, valid_out[g] = min(m, |S_g|)
// from the slots
// wl != nullptr (ugs_uniform_population_sample_wl_begin / _distinct_wl_begin): the vocabulary ids of the rows' WL classes as well
struct PopWlArgs { const uint64_t *d_keys; const int64_t *d_ids; int64_t vocab_size, unknown_id; uint64_t token; int64_t *d_ids_out; };
static int population_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                            int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, uint64_t seed,
                            const uint64_t *seeds, int check, int32_t *graph_status, int64_t *valid_out, ugs_job **job_out,
                            int64_t *total_edges_out, const PopWlArgs *wl = nullptr) {
    if (!pop || !job_out || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index))
        return fail(UGS_E_BAD_ARG, valid_out ? "bad arguments to sample_distinct" : "bad arguments to sample_batch");
    if (wl && pop->st->wl_iter < 0) return fail(UGS_E_BAD_ARG, "uniform_sampler population: created without WL iterations, it holds no class indices");
    if (wl && (wl->vocab_size < 0 || (wl->vocab_size > 0 && (!wl->d_keys || !wl->d_ids)) || (num_graphs > 0 && m_per_graph > 0 && !wl->d_ids_out)))
        return fail(UGS_E_BAD_ARG, "uniform_sampler population: bad vocabulary arguments");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !slots) return fail(UGS_E_BAD_ARG, "population sample needs one slot per graph");
    if (seeds && num_graphs > 0 && !graph_status) return fail(UGS_E_BAD_ARG, "sample_graphs needs seeds and graph_status");
    if (num_graphs >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 2^31 - 1");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (num_cols >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: columns must be < 2^31 - 1");
    const std::shared_ptr<PopState> stp = pop->st;
    PopState &st = *stp;
    const int64_t G = num_graphs, E = num_cols;
    const int k = st.k;
    // the slots of the batch, read under the shared lock; everything they point at outlives the job
    std::vector<UgsPopGraph> pg((size_t)G);
    std::vector<UgsUniGraph> gd((size_t)G);
    std::vector<int64_t> gsize((size_t)G, 0), wbase;
    std::vector<const int32_t *> gcls(wl ? (size_t)G : 0, nullptr);
    std::vector<uint64_t> glfp(wl ? (size_t)G : 0, 0);
    int64_t nv = 0, nv_wide = 0, adj_words = 0;
    bool any_wide = false;
    int pop_dev = -1;
    {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        pop_dev = st.dev;
        for (int64_t g = 0; g < G; ++g) {
            if (slots[g] < 0 || slots[g] >= (int64_t)st.slots.size()) return fail(UGS_E_BAD_ARG, "unknown population slot " + std::to_string(slots[g]));
            const PopSlot &s = st.slots[(size_t)slots[g]];
            const int64_t n = ptr[g + 1] - ptr[g];
            if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
            if (n != s.n)
                return fail(UGS_E_BAD_ARG, "uniform_sampler population: graph " + std::to_string(g) + " of the batch has " + std::to_string(n) +
                                               " vertices, the graph added in its place has " + std::to_string(s.n));
            if (s.size < 0 && !seeds)
                return fail(UGS_E_UNSUPPORTED, "uniform_sampler population: graph " + std::to_string(g) +
                                                   " of the batch failed when it was added (its size or its number of connected k-subsets)");
            if (graph_status) graph_status[g] = s.size < 0 ? 1 : 0;
            UgsPopGraph &d = pg[(size_t)g];
            d.keys = s.keys; d.lo = ptr[g]; d.fp = s.fp; d.n = s.n; d.form = s.size < 0 ? 0 : s.form; d.b = s.b;
            gsize[(size_t)g] = s.size > 0 ? s.size : 0;
            if (wl) { gcls[(size_t)g] = s.cls; glfp[(size_t)g] = s.lfp; }
            if (valid_out) valid_out[g] = std::min<int64_t>(m_per_graph, gsize[(size_t)g]);
            any_wide = any_wide || (d.form == 2 && s.size > 0);
            UgsUniGraph &u = gd[(size_t)g];
            u.lo = ptr[g]; u.n = s.n; u.vbase = 0; u.enumerable = d.form;
            if (d.form == 1) { u.vbase = nv; nv += s.n; }
            if (d.form == 2) nv_wide += s.n;
        }
    }
    const int64_t nv_mask = nv;
    const bool wide = check && nv_wide > 0;                              // only the check builds bitmaps
    if (wide) wbase.assign((size_t)G, -1);
    for (int64_t g = 0; g < G; ++g) {
        UgsUniGraph &u = gd[(size_t)g];
        if (u.enumerable != 2) continue;
        u.vbase = nv; nv += u.n;
        if (wide) { wbase[(size_t)g] = adj_words; adj_words += (int64_t)u.n * ((u.n + 63) / 64); }
    }
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (pop_dev >= 0 && pop_dev != dc.id)
        return fail(UGS_E_BAD_ARG, "the population lives on device " + std::to_string(pop_dev) + ", this call runs on device " + std::to_string(dc.id));
    const int64_t rows = G * (int64_t)m_per_graph;
    // the vocabulary ids of the classes: kept per vocabulary, made again (ugs_wl_lookup over the class table) when the table has grown
    std::shared_ptr<PopDevMem> class_ids;
    if (wl) {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        std::lock_guard<std::mutex> lk2(st.wl_mu);
        const int64_t C = st.class_tab_rows;
        auto it = std::find_if(st.id_caches.begin(), st.id_caches.end(), [&](const PopIdCache &x) { return x.token == wl->token; });
        if (it != st.id_caches.end() && it->classes == C) class_ids = it->ids;
        else {
            class_ids = std::make_shared<PopDevMem>();
            HIP_TRY(hipMalloc(&class_ids->p, (size_t)std::max<int64_t>(C, 1) * 8));
            if (C > 0) {
                const auto *tab = static_cast<const uint64_t *>(st.class_tab->p);
                if (int rc = ugs_wl_lookup(tab, reinterpret_cast<const int32_t *>(tab + 2 * C), C, wl->d_keys, wl->d_ids, wl->vocab_size, wl->unknown_id,
                                           static_cast<int64_t *>(class_ids->p))) return rc;
                HIP_TRY(hipStreamSynchronize(dc.stream));                // another thread's stream may read it next
            }
            if (it != st.id_caches.end()) st.id_caches.erase(it);
            if (st.id_caches.size() >= 8) st.id_caches.erase(st.id_caches.begin());
            st.id_caches.push_back(PopIdCache{wl->token, C, class_ids});
        }
    }
    BlobLayout L;
    auto take = [&](size_t bytes) { return L.take(bytes); };
    const BatchInputs in(L, E, G, sizeof(UgsUniGraph), seeds != nullptr);
    const size_t o_pg = take((size_t)G * sizeof(UgsPopGraph)), o_gz = take((size_t)G * 8), o_wb = wide ? take((size_t)G * 8) : 0;
    const size_t o_cls = wl ? take((size_t)G * 8) : 0, o_lfp = wl ? take((size_t)G * 8) : 0;
    L.end_inputs();
    const size_t cub_bytes = ugs_uniform_cub_bytes(E, 0, 0);
    const size_t o_cub = take(cub_bytes), o_ck = take((size_t)E * 4), o_ck2 = take((size_t)E * 4), o_cv = take((size_t)E * 4),
                 o_cv2 = take((size_t)E * 4), o_cst = take((size_t)(G + 1) * 8), o_pair = take((size_t)E * 4), o_status = take(4 * 8),
                 o_np = take((size_t)G * 4), o_nl = take((size_t)G * 4), o_dr = take((size_t)rows * 4), o_rk = take((size_t)rows * 8),
                 o_ec = take((size_t)rows * 4), o_st = take((size_t)ugs_scan_tmp_words(rows) * 8);
    const size_t o_bp = check ? take((size_t)E * 2) : 0, o_adj = check ? take((size_t)nv * 8) : 0, o_wadj = wide ? take((size_t)adj_words * 8) : 0;
    std::vector<char> host(L.in_bytes, 0);
    in.stage(host.data(), edge_index, row_stride, E, ptr, G, gd.data(), sizeof(UgsUniGraph), seeds);
    if (G > 0) std::memcpy(host.data() + o_pg, pg.data(), (size_t)G * sizeof(UgsPopGraph));
    if (G > 0) std::memcpy(host.data() + o_gz, gsize.data(), (size_t)G * 8);
    if (wide) std::memcpy(host.data() + o_wb, wbase.data(), (size_t)G * 8);
    if (wl && G > 0) std::memcpy(host.data() + o_cls, gcls.data(), (size_t)G * 8);
    if (wl && G > 0) std::memcpy(host.data() + o_lfp, glfp.data(), (size_t)G * 8);
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, UGS_JOB_UNIFORM_POP, G, m_per_graph, k, mode, L.off, &j)) return rc;
    char *b = static_cast<char *>(j->blob.p);
    UgsPopCall p{};
    UgsUniCall &c = p.c;
    c.G = G; c.E = E; c.nv = check ? nv : 0; c.rows = rows; c.m = m_per_graph; c.k = k; c.mode = mode; c.seed = seed;
    c.seeds = seeds ? reinterpret_cast<const uint64_t *>(b + in.seeds) : nullptr;
    c.distinct = valid_out ? 1 : 0;
    c.src = reinterpret_cast<const int64_t *>(b + in.src); c.dst = reinterpret_cast<const int64_t *>(b + in.dst);
    c.ptr = reinterpret_cast<const int64_t *>(b + in.ptr); c.graphs = reinterpret_cast<const UgsUniGraph *>(b + in.desc);
    c.cub_tmp = b + o_cub; c.cub_bytes = cub_bytes;
    c.ckey = reinterpret_cast<uint32_t *>(b + o_ck); c.ckey2 = reinterpret_cast<uint32_t *>(b + o_ck2);
    c.cval = reinterpret_cast<int32_t *>(b + o_cv); c.cval2 = reinterpret_cast<int32_t *>(b + o_cv2);
    c.cstart = reinterpret_cast<int64_t *>(b + o_cst); c.status = reinterpret_cast<int64_t *>(b + o_status);
    c.gsize = reinterpret_cast<int64_t *>(b + o_gz);
    c.nepos = reinterpret_cast<int32_t *>(b + o_np); c.ne_list = reinterpret_cast<int32_t *>(b + o_nl);
    c.draws = reinterpret_cast<int32_t *>(b + o_dr); c.ecount = reinterpret_cast<uint32_t *>(b + o_ec);
    c.scan_tmp = reinterpret_cast<int64_t *>(b + o_st);
    c.nodes = static_cast<int64_t *>(j->nodes.p); c.edge_ptr = j->d_eptr;
    p.pg = reinterpret_cast<const UgsPopGraph *>(b + o_pg);
    p.pair = reinterpret_cast<uint32_t *>(b + o_pair); p.rowkey = reinterpret_cast<uint64_t *>(b + o_rk);
    p.check = check ? 1 : 0; p.any_wide = any_wide ? 1 : 0;
    p.w.nv_mask = check ? nv_mask : 0; p.w.adj_words = adj_words;
    if (check) {
        c.bpair = reinterpret_cast<uint16_t *>(b + o_bp); c.adj = reinterpret_cast<uint64_t *>(b + o_adj);
    }
    if (wide) {
        p.w.wbase = reinterpret_cast<const int64_t *>(b + o_wb); p.w.wadj = reinterpret_cast<uint64_t *>(b + o_wadj);
        p.w.wpair = p.pair;                                              // uni_wadj writes the wide columns' pairs again, the same values
    }
    int64_t status[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_uniform_pop_begin(p, dc.stream);
    if (e == hipSuccess && wl) {
        UgsPopWl q{};
        q.cls = reinterpret_cast<const int32_t *const *>(b + o_cls); q.lfp = reinterpret_cast<const uint64_t *>(b + o_lfp);
        q.id_of_class = static_cast<const int64_t *>(class_ids->p); q.unknown_id = wl->unknown_id; q.ids_out = wl->d_ids_out;
        e = ugs_uniform_pop_wl(p, q, dc.stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(status, c.status, sizeof(status), hipMemcpyDeviceToHost, dc.stream);
    if (int rc = side_job_total(j, e, "uniform_sampler population pipeline")) return rc;
    if (status[2] || status[3]) {                                        // (status[3]: the loop vertices, compared only with wl)
        free_job(j);
        return fail(UGS_E_BAD_ARG, "uniform_sampler population: graph " + std::to_string(G - std::max(status[2], status[3])) +
                                       (status[2] >= status[3] ? " of the batch does not have the adjacency of the graph added in its place"
                                                               : " of the batch does not have the loop vertices of the graph added in its place"));
    }
    j->fill = [p, stp, class_ids](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) { return ugs_uniform_pop_fill(p, edge_index, edge_src, ld, s); };
    return hand_out(j, job_out, total_edges_out);
}

int ugs_uniform_population_sample_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                                        int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, uint64_t seed,
                                        const uint64_t *seeds, int check, int32_t *graph_status, ugs_job **job_out, int64_t *total_edges_out) {
    return population_begin(pop, slots, edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, mode, seed, seeds, check, graph_status,
                            nullptr, job_out, total_edges_out);
}

int ugs_uniform_population_distinct_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                                          int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode,
                                          const uint64_t *seeds, int check, int32_t *graph_status, int64_t *valid_out, ugs_job **job_out,
                                          int64_t *total_edges_out) {
    if (int rc = distinct_checks(num_graphs, m_per_graph, seeds, graph_status, valid_out)) return rc;
    static const uint64_t no_graphs = 0;
    int64_t no_valid = 0;
    return population_begin(pop, slots, edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, mode, 0, seeds ? seeds : &no_graphs,
                            check, graph_status, valid_out ? valid_out : &no_valid, job_out, total_edges_out);
}

int ugs_uniform_population_sample_wl_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                                           int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, uint64_t seed,
                                           const uint64_t *seeds, int check, int32_t *graph_status, const uint64_t *d_vocab_keys,
                                           const int64_t *d_vocab_ids, int64_t vocab_size, int64_t unknown_id, uint64_t vocab_token,
                                           int64_t *d_wl_ids_out, ugs_job **job_out, int64_t *total_edges_out) {
    const PopWlArgs wl{d_vocab_keys, d_vocab_ids, vocab_size, unknown_id, vocab_token, d_wl_ids_out};
    return population_begin(pop, slots, edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, mode, seed, seeds, check, graph_status,
                            nullptr, job_out, total_edges_out, &wl);
}

int ugs_uniform_population_distinct_wl_begin(ugs_uniform_population *pop, const int64_t *slots, const int64_t *edge_index, int64_t row_stride,
                                             int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode,
                                             const uint64_t *seeds, int check, int32_t *graph_status, int64_t *valid_out,
                                             const uint64_t *d_vocab_keys, const int64_t *d_vocab_ids, int64_t vocab_size, int64_t unknown_id,
                                             uint64_t vocab_token, int64_t *d_wl_ids_out, ugs_job **job_out, int64_t *total_edges_out) {
    if (int rc = distinct_checks(num_graphs, m_per_graph, seeds, graph_status, valid_out)) return rc;
    static const uint64_t no_graphs = 0;
    int64_t no_valid = 0;
    const PopWlArgs wl{d_vocab_keys, d_vocab_ids, vocab_size, unknown_id, vocab_token, d_wl_ids_out};
    return population_begin(pop, slots, edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, mode, 0, seeds ? seeds : &no_graphs,
                            check, graph_status, valid_out ? valid_out : &no_valid, job_out, total_edges_out, &wl);
}

int ugs_uniform_population_sample_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                         int64_t *edge_src, int dst_is_device) {
    if (!job || job->kind != UGS_JOB_UNIFORM_POP) return fail(UGS_E_BAD_ARG, "not a uniform_sampler population job");
    return finish_common(job, nodes, edge_index, edge_ptr, sample_ptr, edge_src, dst_is_device);
}

// ---- rwr_sampler.sample_batch (reference src/samplers/rwr_sampler/src/rwr_sampler.cpp, one OpenMP thread) ----
// seeds == nullptr: sample_batch, graph g seeded with seed + g; otherwise sample_graphs: graph g seeded with seeds[g], and a graph
// whose one-graph call would be refused (n >= k and 10 n k > INT_MAX) fails alone, graph_status[g] = 1.
// row_streams: one generator per row (ugs_rwr_sample_rows_begin) in place of one per graph.
static int rwr_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                     int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds, int32_t *graph_status, double p_restart,
                     ugs_job **job_out, int64_t *total_edges_out, bool row_streams = false) {
    const bool per_graph = seeds != nullptr;
    if (!job_out || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (!(p_restart >= 0.0 && p_restart <= 1.0)) return fail(UGS_E_BAD_ARG, "p_restart in [0,1]");
    if (k > UGS_RWR_KMAX) return fail(UGS_E_UNSUPPORTED, "rwr_sampler: k must be <= " + std::to_string(UGS_RWR_KMAX));
    if (num_cols >= ((int64_t)1 << 30)) return fail(UGS_E_UNSUPPORTED, "batch too large: columns must be < 2^30");
    const int64_t G = num_graphs, E = num_cols;
    if (per_graph && G >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 2^31 - 1");
    std::vector<UgsRwrGraph> gd((size_t)G);
    std::vector<int32_t> too_big;
    if (int rc = scan_ptr(ptr, G, per_graph, too_big, [&](int64_t g, int64_t n, std::string &why) {
            const bool over = n >= k && n > (int64_t)INT32_MAX / (10 * (int64_t)k);
            if (over) why = "rwr_sampler: graph " + std::to_string(g) + " has " + std::to_string(n) + " vertices; 10 n k must fit the reference's int iteration limit";
            UgsRwrGraph &d = gd[(size_t)g];
            d.lo = ptr[g]; d.vbase = ptr[g] - ptr[0]; d.n = (int32_t)std::min<int64_t>(n, INT32_MAX);
            d.T = n >= k && !over ? (int32_t)(n * k * 10) : 0;          // (T = 0: m rows of -1 and no draws)
            return over;
        })) return rc;
    const int64_t NV = G > 0 ? ptr[G] - ptr[0] : 0;
    if (NV >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: vertices must be < 2^31 - 1");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    const int64_t rows = G * (int64_t)m_per_graph;
    // one blob: inputs first (uploaded in one copy), then the scratch of every stage
    BlobLayout L;
    auto take = [&](size_t bytes) { return L.take(bytes); };
    const BatchInputs in(L, E, G, sizeof(UgsRwrGraph), per_graph);
    L.end_inputs();
    const size_t cub_bytes = ugs_rwr_cub_bytes(E);
    const size_t o_cub = take(cub_bytes), o_hk = take((size_t)E * 8), o_hk2 = take((size_t)E * 8), o_hv = take((size_t)E * 8),
                 o_hv2 = take((size_t)E * 8), o_rs = take((size_t)(NV + 1) * 4), o_par = take((size_t)NV * 4), o_cs = take((size_t)NV * 4),
                 o_dm = take((size_t)NV), o_rst = take((size_t)rows * 8), o_ec = take((size_t)rows * 4),
                 o_st = take((size_t)ugs_scan_tmp_words(rows) * 8);
    std::vector<char> host(L.in_bytes, 0);
    in.stage(host.data(), edge_index, row_stride, E, ptr, G, gd.data(), sizeof(UgsRwrGraph), per_graph ? seeds : nullptr);
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, UGS_JOB_RWR, G, m_per_graph, k, mode, L.off, &j)) return rc;
    char *b = static_cast<char *>(j->blob.p);
    UgsRwrCall c{};
    c.G = G; c.E = E; c.NV = NV; c.rows = rows; c.m = m_per_graph; c.k = k; c.mode = mode; c.seed = seed; c.p = p_restart;
    c.seeds = per_graph ? reinterpret_cast<const uint64_t *>(b + in.seeds) : nullptr;
    // speculation window: room for about 16 draws per wanted walk, 1 to 4 offsets per lane
    c.spec = (int32_t)std::min<int64_t>(4, std::max<int64_t>(1, ((int64_t)m_per_graph * 16 + 255) / 256));
    c.src = reinterpret_cast<const int64_t *>(b + in.src); c.dst = reinterpret_cast<const int64_t *>(b + in.dst);
    c.ptr = reinterpret_cast<const int64_t *>(b + in.ptr); c.graphs = reinterpret_cast<const UgsRwrGraph *>(b + in.desc);
    c.cub_tmp = b + o_cub; c.cub_bytes = cub_bytes;
    c.hkey = reinterpret_cast<uint32_t *>(b + o_hk); c.hkey2 = reinterpret_cast<uint32_t *>(b + o_hk2);
    c.hval = reinterpret_cast<int32_t *>(b + o_hv); c.hval2 = reinterpret_cast<int32_t *>(b + o_hv2);
    c.rs = reinterpret_cast<int32_t *>(b + o_rs); c.parent = reinterpret_cast<int32_t *>(b + o_par);
    c.csize = reinterpret_cast<int32_t *>(b + o_cs); c.doomed = reinterpret_cast<uint8_t *>(b + o_dm);
    c.rstart = reinterpret_cast<int64_t *>(b + o_rst); c.ecount = reinterpret_cast<uint32_t *>(b + o_ec);
    c.scan_tmp = reinterpret_cast<int64_t *>(b + o_st);
    c.nodes = static_cast<int64_t *>(j->nodes.p); c.edge_ptr = j->d_eptr;
    if (row_streams) {
        // half-edges inside each graph, as rwr_halfedges keeps them: they size the walk kernel's LDS.  Columns mostly follow their graphs.
        std::vector<int64_t> half((size_t)G, 0);
        int64_t g = 0;
        for (int64_t x = 0; x < E && G > 0; ++x) {
            const int64_t u = edge_index[x], v = edge_index[row_stride + x];
            if (!(ptr[g] <= u && u < ptr[g + 1])) g = std::min<int64_t>(std::upper_bound(ptr + 1, ptr + G + 1, u) - (ptr + 1), G - 1);
            if (ptr[g] <= u && u < ptr[g + 1] && ptr[g] <= v && v < ptr[g + 1]) half[(size_t)g] += 2;
        }
        ugs_rwr_row_streams(c, gd.data(), half.data());
    }
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_rwr_begin(c, dc.stream);
    if (int rc = side_job_total(j, e, "rwr_sampler pipeline")) return rc;
    for (int64_t g = 0; per_graph && g < G; ++g) graph_status[g] = too_big[(size_t)g];
    j->fill = [c](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) { return ugs_rwr_fill(c, edge_index, edge_src, ld, s); };
    return hand_out(j, job_out, total_edges_out);
}

int ugs_rwr_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                               int m_per_graph, int k, int mode, uint64_t seed, double p_restart, ugs_job **job_out,
                               int64_t *total_edges_out) {
    return rwr_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, seed, nullptr, nullptr, p_restart, job_out,
                     total_edges_out);
}

int ugs_rwr_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                                int m_per_graph, int k, int mode, const uint64_t *seeds, double p_restart, int32_t *graph_status,
                                ugs_job **job_out, int64_t *total_edges_out) {
    if (num_graphs > 0 && (!seeds || !graph_status)) return fail(UGS_E_BAD_ARG, "sample_graphs needs seeds and graph_status");
    static const uint64_t no_graphs = 0;                                // num_graphs == 0 still takes the per-graph path
    int32_t no_status = 0;
    return rwr_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, 0, seeds ? seeds : &no_graphs,
                     graph_status ? graph_status : &no_status, p_restart, job_out, total_edges_out);
}

int ugs_rwr_sample_rows_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                              int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds, double p_restart,
                              int32_t *graph_status, ugs_job **job_out, int64_t *total_edges_out) {
    static const uint64_t no_graphs = 0;                                // no graphs, no seeds: graph_status alone asks for the per-graph form
    if (!seeds && num_graphs == 0 && graph_status) seeds = &no_graphs;
    if (!seeds) {
        if (graph_status) return fail(UGS_E_BAD_ARG, "sample_rows without seeds takes no graph_status");
        return rwr_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, seed, nullptr, nullptr, p_restart, job_out,
                         total_edges_out, true);
    }
    if (!graph_status) return fail(UGS_E_BAD_ARG, "sample_rows with seeds needs graph_status");
    return rwr_begin(edge_index, row_stride, num_cols, ptr, num_graphs, m_per_graph, k, mode, 0, seeds, graph_status, p_restart, job_out,
                     total_edges_out, true);
}

int ugs_rwr_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                                int64_t *edge_src, int dst_is_device) {
    if (!job || job->kind != UGS_JOB_RWR) return fail(UGS_E_BAD_ARG, "not an rwr_sampler job");
    return finish_common(job, nodes, edge_index, edge_ptr, sample_ptr, edge_src, dst_is_device);
}

// ---- rwr_sampler.GraphCache: the CSR of every dataset graph built once and kept on the device; a sample call over any batch of
//      added graphs runs only the walks, the scan and the fill (the contract stands in include/ugs_mi355.h at
//      ugs_rwr_cache_sample_begin; layout and generations: DESIGN.md section 11.2) ----
namespace {
struct RwrSlot {
    int64_t vbase = 0, col0 = -1, cols = 0;   // vertex offset in the store's rs / doomed; first stored column (-1: none); columns E_g
    int32_t n = 0;
    bool failed = false;                      // n >= k and 10 n k > INT_MAX: no storage, never walked
};
// One generation of the storage.  Growth makes a new one and copies; a job's fill hook holds the one it walked on.
struct RwrGen {
    int32_t *rs = nullptr, *tg = nullptr;
    uint8_t *doomed = nullptr;
    int2 *cols = nullptr;
    int64_t cap_v = 0, cap_h = 0, cap_c = 0;  // entries of rs / doomed, of tg, of cols
    ~RwrGen() { (void)hipFree(rs); (void)hipFree(tg); (void)hipFree(doomed); (void)hipFree(cols); }
    int64_t bytes() const { return cap_v * 5 + cap_h * 4 + cap_c * 8; }
    int alloc(int64_t v, int64_t h, int64_t c) {
        cap_v = std::max<int64_t>(v, 1); cap_h = std::max<int64_t>(h, 1); cap_c = std::max<int64_t>(c, 1);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&rs), (size_t)cap_v * 4));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&doomed), (size_t)cap_v));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&tg), (size_t)cap_h * 4));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cols), (size_t)cap_c * 8));
        return UGS_OK;
    }
};
struct RwrCacheState {
    int k = 0, dev = -1;
    int64_t reserve_v = 0, reserve_c = 0;
    std::mutex add_mu;                        // adds, one at a time, from the build to the publication
    std::shared_mutex mu;                     // what a sample begin reads: slots and gen (exclusive only to publish an add)
    std::deque<RwrSlot> slots;
    std::shared_ptr<RwrGen> gen;
    int64_t used_v = 0, used_h = 0, used_c = 0, generations = 0;
};
bool rwr_over(int64_t n, int k) { return n >= k && n > (int64_t)INT32_MAX / (10 * (int64_t)k); }
}  // namespace
struct ugs_rwr_cache { std::shared_ptr<RwrCacheState> st; };

int ugs_rwr_cache_create(int k, int64_t reserve_vertices, int64_t reserve_columns, ugs_rwr_cache **cache_out) {
    if (!cache_out) return fail(UGS_E_BAD_ARG, "cache_out is null");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_RWR_KMAX) return fail(UGS_E_UNSUPPORTED, "rwr_sampler: k must be <= " + std::to_string(UGS_RWR_KMAX));
    if (reserve_vertices < 0 || reserve_vertices >= (int64_t)INT32_MAX || reserve_columns < 0 || reserve_columns >= ((int64_t)1 << 30))
        return fail(UGS_E_BAD_ARG, "reserve must be 0 ... 2^31 - 2 vertices and 0 ... 2^30 - 1 columns");
    auto *c = new ugs_rwr_cache();
    c->st = std::make_shared<RwrCacheState>();
    c->st->k = k; c->st->reserve_v = reserve_vertices; c->st->reserve_c = reserve_columns;
    *cache_out = c;
    return UGS_OK;
}

int ugs_rwr_cache_destroy(ugs_rwr_cache *cache) {
    delete cache;                                                        // a generation goes with the last job that walked on it
    return UGS_OK;
}

int ugs_rwr_cache_info(ugs_rwr_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *half_edges_out, int64_t *bytes_out,
                       int64_t *generations_out) {
    if (!cache) return fail(UGS_E_BAD_ARG, "cache is null");
    RwrCacheState &st = *cache->st;
    std::shared_lock<std::shared_mutex> lk(st.mu);
    if (graphs_out) *graphs_out = (int64_t)st.slots.size();
    if (vertices_out) *vertices_out = st.used_v;
    if (half_edges_out) *half_edges_out = st.used_h;
    if (bytes_out) *bytes_out = st.gen ? st.gen->bytes() : 0;
    if (generations_out) *generations_out = st.generations;
    return UGS_OK;
}

int ugs_rwr_cache_add(ugs_rwr_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                      int64_t num_graphs, int64_t *slots_out, int32_t *status_out) {
    if (!cache || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to rwr cache add");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && (!slots_out || !status_out)) return fail(UGS_E_BAD_ARG, "rwr cache add needs slots_out and status_out");
    if (num_cols >= ((int64_t)1 << 30)) return fail(UGS_E_UNSUPPORTED, "add too large: columns must be < 2^30");
    RwrCacheState &st = *cache->st;
    const int64_t G = num_graphs, E_in = num_cols;
    const int k = st.k;
    if (G == 0) {
        if (E_in > 0) return fail(UGS_E_BAD_ARG, "rwr cache add: columns without a graph");
        return UGS_OK;
    }
    // The batch as it is stored: a failed graph keeps its slot and its column count but neither vertices nor columns.  Columns
    // must come graph by graph, in the order of the graphs, both endpoints inside the graph: that order is what a batch is
    // compared with, and a column that left its graph could fall into a neighbour's range once the graph stands in a batch.
    std::vector<RwrSlot> fresh((size_t)G);
    std::vector<int64_t> cptr((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = ptr[g + 1] - ptr[g];
        if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
        RwrSlot &s = fresh[(size_t)g];
        s.n = (int32_t)std::min<int64_t>(n, INT32_MAX);
        s.failed = rwr_over(n, k);
        cptr[(size_t)g + 1] = cptr[(size_t)g] + (s.failed ? 0 : n);
    }
    const int64_t NV = cptr[(size_t)G];
    if (NV >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "add too large: vertices must be < 2^31 - 1");
    std::vector<int64_t> src, dst;
    src.reserve((size_t)E_in); dst.reserve((size_t)E_in);
    {
        int64_t g = 0;
        for (int64_t x = 0; x < E_in; ++x) {
            const int64_t u = edge_index[x], v = edge_index[row_stride + x];
            while (g < G && !(ptr[g] <= u && u < ptr[g + 1])) ++g;
            if (g >= G || !(ptr[g] <= v && v < ptr[g + 1]))
                return fail(UGS_E_BAD_ARG, "rwr cache add: column " + std::to_string(x) + " is not inside one graph, or the columns are not in the order of the graphs");
            RwrSlot &s = fresh[(size_t)g];
            ++s.cols;
            if (s.failed) continue;
            src.push_back(u - ptr[g] + cptr[(size_t)g]);
            dst.push_back(v - ptr[g] + cptr[(size_t)g]);
        }
    }
    const int64_t E = (int64_t)src.size();
    std::lock_guard<std::mutex> add_lk(st.add_mu);                       // (only adds write used_* and gen: reading them here needs no more)
    if (st.used_h + 2 * E >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "rwr cache: the half-edges of all added graphs must stay below 2^31 (row starts are 32-bit offsets)");
    if (st.used_v + NV + 1 >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "rwr cache: vertices plus adds must stay below 2^31");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (st.dev >= 0 && st.dev != dc.id)
        return fail(UGS_E_BAD_ARG, "the rwr cache lives on device " + std::to_string(st.dev) + ", this add runs on device " + std::to_string(dc.id));
    // the build's blob: the compact batch first (one copy), then the scratch of rwr_init ... rwr_rowstart
    BlobLayout L;
    auto take = [&](size_t bytes) { return L.take(bytes); };
    const size_t o_src = take((size_t)E * 8), o_dst = take((size_t)E * 8), o_ptr = take((size_t)(G + 1) * 8);
    L.end_inputs();
    const size_t cub_bytes = ugs_rwr_cub_bytes(E);
    const size_t o_cub = take(cub_bytes), o_hk = take((size_t)E * 8), o_hk2 = take((size_t)E * 8), o_hv = take((size_t)E * 8),
                 o_hv2 = take((size_t)E * 8), o_rs = take((size_t)(NV + 1) * 4), o_par = take((size_t)NV * 4), o_cs = take((size_t)NV * 4),
                 o_dm = take((size_t)NV);
    std::vector<char> host(L.in_bytes, 0);
    if (E > 0) { std::memcpy(host.data() + o_src, src.data(), (size_t)E * 8); std::memcpy(host.data() + o_dst, dst.data(), (size_t)E * 8); }
    std::memcpy(host.data() + o_ptr, cptr.data(), (size_t)(G + 1) * 8);
    // room in the store: this generation, or a new one of at least twice the size with everything held so far copied over
    std::shared_ptr<RwrGen> gen = st.gen;
    const int64_t need_v = st.used_v + NV + 1, need_h = st.used_h + 2 * E, need_c = st.used_c + E;
    const bool grow = !gen || need_v > gen->cap_v || need_h > gen->cap_h || need_c > gen->cap_c;
    if (grow) {
        auto room = [](int64_t need, int64_t have, int64_t reserve) { return need <= have ? have : std::max({need, 2 * have, reserve}); };
        const std::shared_ptr<RwrGen> old = gen;
        gen = std::make_shared<RwrGen>();
        HIP_TRY(hipSetDevice(dc.id));
        if (int rc = gen->alloc(room(need_v, old ? old->cap_v : 0, st.reserve_v), room(need_h, old ? old->cap_h : 0, 2 * st.reserve_c),
                                room(need_c, old ? old->cap_c : 0, st.reserve_c))) return rc;
        if (old) {
            if (st.used_v > 0) {
                HIP_TRY(hipMemcpyAsync(gen->rs, old->rs, (size_t)st.used_v * 4, hipMemcpyDeviceToDevice, dc.stream));
                HIP_TRY(hipMemcpyAsync(gen->doomed, old->doomed, (size_t)st.used_v, hipMemcpyDeviceToDevice, dc.stream));
            }
            if (st.used_h > 0) HIP_TRY(hipMemcpyAsync(gen->tg, old->tg, (size_t)st.used_h * 4, hipMemcpyDeviceToDevice, dc.stream));
            if (st.used_c > 0) HIP_TRY(hipMemcpyAsync(gen->cols, old->cols, (size_t)st.used_c * 8, hipMemcpyDeviceToDevice, dc.stream));
        }
    }
    PoolBuf blob;
    if (int rc = pool_get(L.off, dc.id, blob)) return rc;
    char *b = static_cast<char *>(blob.p);
    UgsRwrCall c{};
    c.G = G; c.E = E; c.NV = NV; c.k = k;
    c.src = reinterpret_cast<const int64_t *>(b + o_src); c.dst = reinterpret_cast<const int64_t *>(b + o_dst);
    c.ptr = reinterpret_cast<const int64_t *>(b + o_ptr);
    c.cub_tmp = b + o_cub; c.cub_bytes = cub_bytes;
    c.hkey = reinterpret_cast<uint32_t *>(b + o_hk); c.hkey2 = reinterpret_cast<uint32_t *>(b + o_hk2);
    c.hval = reinterpret_cast<int32_t *>(b + o_hv); c.hval2 = reinterpret_cast<int32_t *>(b + o_hv2);
    c.rs = reinterpret_cast<int32_t *>(b + o_rs); c.parent = reinterpret_cast<int32_t *>(b + o_par);
    c.csize = reinterpret_cast<int32_t *>(b + o_cs); c.doomed = reinterpret_cast<uint8_t *>(b + o_dm);
    UgsRwrStore w{};
    w.rs = gen->rs; w.tg = gen->tg; w.doomed = gen->doomed; w.cols = gen->cols;
    w.rs_base = st.used_v; w.tg_base = st.used_h; w.col_base = st.used_c;
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_rwr_build(c, dc.stream);
    if (e == hipSuccess) e = ugs_rwr_store_append(c, w, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    pool_put(blob);
    if (e != hipSuccess) return fail_hip(e, "rwr_sampler cache add");     // (a new generation is dropped: the cache is as it was)
    int64_t col = st.used_c;
    std::unique_lock<std::shared_mutex> lk(st.mu);
    st.dev = dc.id;
    if (grow) { st.gen = gen; ++st.generations; }
    for (int64_t g = 0; g < G; ++g) {
        RwrSlot &s = fresh[(size_t)g];
        s.vbase = st.used_v + cptr[(size_t)g];
        if (!s.failed) { s.col0 = col; col += s.cols; }
        slots_out[g] = (int64_t)st.slots.size();
        status_out[g] = s.failed ? 1 : 0;
        st.slots.push_back(s);
    }
    st.used_v = need_v; st.used_h = need_h; st.used_c = need_c;
    return UGS_OK;
}

int ugs_rwr_cache_sample_begin(ugs_rwr_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                               const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, uint64_t seed, const uint64_t *seeds,
                               double p_restart, int row_streams, int check, int32_t *graph_status, ugs_job **job_out,
                               int64_t *total_edges_out) {
    if (!cache || !job_out || !ptr) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !slots) return fail(UGS_E_BAD_ARG, "rwr cache sample needs one slot per graph");
    if (check && (num_cols < 0 || (num_cols > 0 && !edge_index))) return fail(UGS_E_BAD_ARG, "the check needs the batch's edge_index");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (!(p_restart >= 0.0 && p_restart <= 1.0)) return fail(UGS_E_BAD_ARG, "p_restart in [0,1]");
    static const uint64_t no_graphs = 0;                                // no graphs, no seeds: graph_status alone asks for the per-graph form
    if (!seeds && num_graphs == 0 && graph_status) seeds = &no_graphs;
    const bool per_graph = seeds != nullptr;
    if (per_graph && num_graphs > 0 && !graph_status) return fail(UGS_E_BAD_ARG, "sample_graphs needs seeds and graph_status");
    if (!per_graph && graph_status) return fail(UGS_E_BAD_ARG, "graph_status goes with seeds");
    if (num_graphs >= (int64_t)0x7f7f7f7f) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 0x7f7f7f7f");   // (first_bad starts there)
    const std::shared_ptr<RwrCacheState> stp = cache->st;
    RwrCacheState &st = *stp;
    const int64_t G = num_graphs;
    const int k = st.k;
    const bool have_cols = edge_index != nullptr;                        // check == 0 and no edge_index: num_cols says nothing
    const bool checked = check != 0;
    std::vector<UgsRwrGraph> gd((size_t)G);
    std::vector<int64_t> coff((size_t)G + 1, 0), col0((size_t)G, -1), half((size_t)G, 0);
    std::vector<int32_t> status((size_t)G, 0);
    std::shared_ptr<RwrGen> gen;
    int cache_dev = -1;
    {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        gen = st.gen;
        cache_dev = st.dev;
        for (int64_t g = 0; g < G; ++g) {
            if (slots[g] < 0 || slots[g] >= (int64_t)st.slots.size()) return fail(UGS_E_BAD_ARG, "unknown rwr cache slot " + std::to_string(slots[g]));
            const RwrSlot &s = st.slots[(size_t)slots[g]];
            const int64_t n = ptr[g + 1] - ptr[g];
            if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
            if (n != s.n)
                return fail(UGS_E_BAD_ARG, "rwr_sampler cache: graph " + std::to_string(g) + " of the batch has " + std::to_string(n) +
                                               " vertices, the graph added in its place has " + std::to_string(s.n));
            if (s.failed && !per_graph)                                 // (rwr_begin's text for the same graph)
                return fail(UGS_E_UNSUPPORTED, "rwr_sampler: graph " + std::to_string(g) + " has " + std::to_string(n) +
                                                   " vertices; 10 n k must fit the reference's int iteration limit");
            status[(size_t)g] = s.failed ? 1 : 0;
            UgsRwrGraph &d = gd[(size_t)g];
            d.lo = ptr[g]; d.vbase = s.vbase; d.n = s.n;
            d.T = n >= k && !s.failed ? (int32_t)(n * k * 10) : 0;      // (T = 0: m rows of -1 and no draws)
            coff[(size_t)g + 1] = coff[(size_t)g] + s.cols;
            col0[(size_t)g] = s.col0;
            half[(size_t)g] = s.failed ? 0 : 2 * s.cols;
        }
    }
    const int64_t E = coff[(size_t)G];
    if ((checked || have_cols) && num_cols != E)
        return fail(UGS_E_BAD_ARG, "rwr_sampler cache: the batch has " + std::to_string(num_cols) + " columns, the added graphs have " + std::to_string(E));
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (cache_dev >= 0 && cache_dev != dc.id)
        return fail(UGS_E_BAD_ARG, "the rwr cache lives on device " + std::to_string(cache_dev) + ", this call runs on device " + std::to_string(dc.id));
    const int64_t rows = G * (int64_t)m_per_graph;
    const int64_t Ec = checked ? E : 0;                                  // columns that go up: none without the check
    // one blob: descriptors, seeds and (check) the batch's columns go up in one copy; then the walks' scratch.  No half-edge arrays.
    BlobLayout L;
    auto take = [&](size_t bytes) { return L.take(bytes); };
    const size_t o_desc = take((size_t)G * sizeof(UgsRwrGraph)), o_seeds = take(per_graph ? (size_t)G * 8 : 0),
                 o_coff = take(checked ? (size_t)(G + 1) * 8 : 0), o_col0 = take(checked ? (size_t)G * 8 : 0), o_src = take((size_t)Ec * 8),
                 o_dst = take((size_t)Ec * 8);
    L.end_inputs();
    const size_t o_rst = take((size_t)rows * 8), o_ec = take((size_t)rows * 4), o_st = take((size_t)ugs_scan_tmp_words(rows) * 8);
    std::vector<char> host(L.in_bytes, 0);
    if (G > 0) std::memcpy(host.data() + o_desc, gd.data(), (size_t)G * sizeof(UgsRwrGraph));
    if (per_graph && G > 0) std::memcpy(host.data() + o_seeds, seeds, (size_t)G * 8);
    if (checked) {
        std::memcpy(host.data() + o_coff, coff.data(), (size_t)(G + 1) * 8);
        if (G > 0) std::memcpy(host.data() + o_col0, col0.data(), (size_t)G * 8);
        if (Ec > 0) {
            std::memcpy(host.data() + o_src, edge_index, (size_t)Ec * 8);
            std::memcpy(host.data() + o_dst, edge_index + row_stride, (size_t)Ec * 8);
        }
    }
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, UGS_JOB_RWR, G, m_per_graph, k, mode, L.off, &j, true)) return rc;
    if (int rc = side_job_rows(j, rows, 8)) return rc;                   // first_bad right behind the edge total: one read-back for both
    char *b = static_cast<char *>(j->blob.p);
    UgsRwrCall c{};
    c.G = G; c.rows = rows; c.m = m_per_graph; c.k = k; c.mode = mode; c.seed = seed; c.p = p_restart;
    c.seeds = per_graph ? reinterpret_cast<const uint64_t *>(b + o_seeds) : nullptr;
    c.spec = (int32_t)std::min<int64_t>(4, std::max<int64_t>(1, ((int64_t)m_per_graph * 16 + 255) / 256));
    c.graphs = reinterpret_cast<const UgsRwrGraph *>(b + o_desc);
    if (gen) { c.rs = gen->rs; c.hval2 = gen->tg; c.doomed = gen->doomed; }
    c.rstart = reinterpret_cast<int64_t *>(b + o_rst); c.ecount = reinterpret_cast<uint32_t *>(b + o_ec);
    c.scan_tmp = reinterpret_cast<int64_t *>(b + o_st);
    c.nodes = static_cast<int64_t *>(j->nodes.p); c.edge_ptr = j->d_eptr;
    if (row_streams) ugs_rwr_row_streams(c, gd.data(), half.data());
    int64_t back[2] = {0, 0};                                            // the edge total, and the check's first_bad in the low word behind it
    int32_t *d_bad = reinterpret_cast<int32_t *>(j->d_eptr + rows + 1);
    const bool run_check = checked && Ec > 0 && gen;
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess && run_check) e = hipMemsetAsync(d_bad, 0x7f, 8, dc.stream);        // above every g
    if (e == hipSuccess) e = ugs_rwr_walks(c, dc.stream);
    if (e == hipSuccess && run_check) {
        UgsRwrCheck q{};
        q.E = Ec; q.G = G;
        q.src = reinterpret_cast<const int64_t *>(b + o_src); q.dst = reinterpret_cast<const int64_t *>(b + o_dst);
        q.graphs = c.graphs;
        q.coff = reinterpret_cast<const int64_t *>(b + o_coff); q.col0 = reinterpret_cast<const int64_t *>(b + o_col0);
        q.cols = gen->cols; q.first_bad = d_bad;
        e = ugs_rwr_store_check(q, dc.stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(back, j->d_eptr + rows, run_check ? 16 : 8, hipMemcpyDeviceToHost, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e != hipSuccess) { free_job(j); return fail_hip(e, "rwr_sampler cache pipeline"); }
    j->total = back[0];
    if (run_check) {
        const int64_t bad = (int64_t)(int32_t)(back[1] & 0xffffffff);
        if (bad < G) {
            free_job(j);
            return fail(UGS_E_BAD_ARG, "rwr_sampler cache: graph " + std::to_string(bad) + " of the batch differs from the graph added in its place");
        }
    }
    for (int64_t g = 0; per_graph && g < G; ++g) graph_status[g] = status[(size_t)g];
    // the hook holds the generation the walks read: an add that regrows the store leaves this job its buffers
    j->fill = [c, gen](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) { return ugs_rwr_fill(c, edge_index, edge_src, ld, s); };
    return hand_out(j, job_out, total_edges_out);
}

}  // extern "C"

