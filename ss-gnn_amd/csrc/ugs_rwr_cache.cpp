// ugs_rwr_cache.cpp -- host side of rwr_sampler.GraphCache in libugs_mi355.so: the CSR of every dataset graph built once
// (ugs_rwr_build + ugs_rwr_store_append in ugs_rwr.hip) and kept on the device; a sample call over any batch of added graphs runs
// only the walks, the scan and the fill.
//
// Behavioural contract: rwr_begin (ugs_side_rwr.cpp) on the collated batch; the law stands in include/ugs_mi355.h at
// ugs_rwr_cache_sample_begin.  The store, the cache state and its locking, the front halves of the add and of the begin and the
// check's inputs are the dataset caches' (ugs_cache_common.cpp; ugs_host_internal.h); the job is the job
// path's (ugs_jobs.cpp).  What is this cache's own -- failed graphs, layout: DESIGN.md section 11.2.
#include "ugs_host_internal.h"

#include <deque>

using namespace ugs_host;

namespace {
struct RwrSlot {
    int64_t vbase = 0, col0 = -1, cols = 0;   // vertex offset in the store's rs / doomed; first stored column (-1: none); columns E_g
    int32_t n = 0;
    bool failed = false;                      // n >= k and 10 n k > INT_MAX: no storage, never walked
};
// The store: rs and doomed per vertex (plus one entry per add), tg per half-edge, cols per column.
enum { RS, DOOMED, TG, COLS };
enum { GV, GH, GC };
const StoreShape RWR_SHAPE = {4, 3, {{4, GV}, {1, GV}, {4, GH}, {8, GC}}};
const char *const NAME = "rwr cache";
struct RwrCacheState : CacheState {
    int k = 0;
    std::deque<RwrSlot> slots;
    RwrCacheState() : CacheState(RWR_SHAPE, NAME, "rwr_sampler", GV, GH) {}
};
bool rwr_over(int64_t n, int k) { return n >= k && n > (int64_t)INT32_MAX / (10 * (int64_t)k); }
}  // namespace
struct ugs_rwr_cache { std::shared_ptr<RwrCacheState> st; };

extern "C" {

int ugs_rwr_cache_create(int k, int64_t reserve_vertices, int64_t reserve_columns, ugs_rwr_cache **cache_out) {
    if (!cache_out) return fail(UGS_E_BAD_ARG, "cache_out is null");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_RWR_KMAX) return fail(UGS_E_UNSUPPORTED, "rwr_sampler: k must be <= " + std::to_string(UGS_RWR_KMAX));
    if (int rc = cache_reserve_check(reserve_vertices, reserve_columns)) return rc;
    auto *c = new ugs_rwr_cache();
    c->st = std::make_shared<RwrCacheState>();
    c->st->k = k;
    c->st->reserve[GV] = reserve_vertices; c->st->reserve[GH] = 2 * reserve_columns; c->st->reserve[GC] = reserve_columns;
    *cache_out = c;
    return UGS_OK;
}

int ugs_rwr_cache_destroy(ugs_rwr_cache *cache) {
    delete cache;                                                        // a generation goes with the last job that walked on it
    return UGS_OK;
}

int ugs_rwr_cache_info(ugs_rwr_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *half_edges_out, int64_t *bytes_out,
                       int64_t *generations_out) {
    return cache_info(cache ? cache->st.get() : nullptr, graphs_out, vertices_out, half_edges_out, bytes_out, generations_out);
}

int ugs_rwr_cache_add(ugs_rwr_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                      int64_t num_graphs, int64_t *slots_out, int32_t *status_out) {
    if (int rc = cache_add_args(NAME, cache, edge_index, num_cols, ptr, num_graphs, slots_out && status_out, "slots_out and status_out",
                                (int64_t)1 << 30, "2^30")) return rc;
    const int64_t G = num_graphs;
    if (G == 0) return UGS_OK;
    RwrCacheState &st = *cache->st;
    const int k = st.k;
    // The batch as it is stored: a failed graph keeps its slot and its column count but neither vertices nor columns.
    std::vector<RwrSlot> fresh((size_t)G);
    std::vector<int64_t> vptr((size_t)G + 1, 0), cptr;
    std::vector<int32_t> none;
    if (int rc = scan_ptr(ptr, G, false, none, [&](int64_t g, int64_t n, std::string &) {
            RwrSlot &s = fresh[(size_t)g];
            s.n = (int32_t)std::min<int64_t>(n, INT32_MAX);
            s.failed = rwr_over(n, k);
            vptr[(size_t)g + 1] = vptr[(size_t)g] + (s.failed ? 0 : n);
            return false;
        })) return rc;
    const int64_t NV = vptr[(size_t)G];
    if (NV >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "add too large: vertices must be < 2^31 - 1");
    std::vector<int64_t> src, dst;
    src.reserve((size_t)num_cols); dst.reserve((size_t)num_cols);
    if (int rc = cache_walk_columns(NAME, edge_index, row_stride, num_cols, ptr, G, cptr, [&](int64_t, int64_t g, int64_t u, int64_t v) {
            if (fresh[(size_t)g].failed) return;
            src.push_back(u + vptr[(size_t)g]);
            dst.push_back(v + vptr[(size_t)g]);
        })) return rc;
    const int64_t E = (int64_t)src.size();
    std::lock_guard<std::mutex> add_lk(st.add_mu);
    if (st.used[GH] + 2 * E >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "rwr cache: the half-edges of all added graphs must stay below 2^31 (row starts are 32-bit offsets)");
    if (st.used[GV] + NV + 1 >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "rwr cache: vertices plus adds must stay below 2^31");
    CacheAdd a;
    if (int rc = cache_add_device(st, a)) return rc;
    const DeviceCtx &dc = a.dc;
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
    std::memcpy(host.data() + o_ptr, vptr.data(), (size_t)(G + 1) * 8);
    a.need[GV] = st.used[GV] + NV + 1; a.need[GH] = st.used[GH] + 2 * E; a.need[GC] = st.used[GC] + E;
    if (int rc = cache_room(st, a)) return rc;
    const StoreGen &gen = *a.gen;
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
    w.rs = gen.at<int32_t>(RS); w.tg = gen.at<int32_t>(TG); w.doomed = gen.at<uint8_t>(DOOMED); w.cols = gen.at<int2>(COLS);
    w.rs_base = st.used[GV]; w.tg_base = st.used[GH]; w.col_base = st.used[GC];
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_rwr_build(c, dc.stream);
    if (e == hipSuccess) e = ugs_rwr_store_append(c, w, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    pool_put(blob);
    if (e != hipSuccess) return fail_hip(e, "rwr_sampler cache add");     // (a new generation is dropped: the cache is as it was)
    cache_publish(st, a, G, [&] {
        int64_t col = st.used[GC];
        for (int64_t g = 0; g < G; ++g) {
            RwrSlot &s = fresh[(size_t)g];
            s.cols = cptr[(size_t)g + 1] - cptr[(size_t)g];
            s.vbase = st.used[GV] + vptr[(size_t)g];
            if (!s.failed) { s.col0 = col; col += s.cols; }
            slots_out[g] = (int64_t)st.slots.size();
            status_out[g] = s.failed ? 1 : 0;
            st.slots.push_back(s);
        }
    });
    return UGS_OK;
}

int ugs_rwr_cache_sample_begin(ugs_rwr_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                               const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, uint64_t seed, const uint64_t *seeds,
                               double p_restart, int row_streams, int check, int32_t *graph_status, ugs_job **job_out,
                               int64_t *total_edges_out) {
    if (int rc = cache_begin_args(NAME, cache && job_out && ptr, slots, edge_index, num_cols, num_graphs, check)) return rc;
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (!(p_restart >= 0.0 && p_restart <= 1.0)) return fail(UGS_E_BAD_ARG, "p_restart in [0,1]");
    static const uint64_t no_graphs = 0;                                // no graphs, no seeds: graph_status alone asks for the per-graph form
    if (!seeds && num_graphs == 0 && graph_status) seeds = &no_graphs;
    const bool per_graph = seeds != nullptr;
    if (per_graph && num_graphs > 0 && !graph_status) return fail(UGS_E_BAD_ARG, "sample_graphs needs seeds and graph_status");
    if (!per_graph && graph_status) return fail(UGS_E_BAD_ARG, "graph_status goes with seeds");
    const std::shared_ptr<RwrCacheState> stp = cache->st;
    RwrCacheState &st = *stp;
    const int64_t G = num_graphs;
    const int k = st.k;
    const bool have_cols = edge_index != nullptr;                        // check == 0 and no edge_index: num_cols says nothing
    const bool checked = check != 0;
    std::vector<UgsRwrGraph> gd((size_t)G);
    std::vector<int64_t> half((size_t)G, 0);
    std::vector<int32_t> status((size_t)G, 0);
    CacheBatch cb;
    if (int rc = cache_scan_slots(st, st.slots, slots, ptr, G, cb, [&](int64_t g, const RwrSlot &s, int64_t n) {
            if (s.failed && !per_graph)                                 // (rwr_begin's text for the same graph)
                return fail(UGS_E_UNSUPPORTED, "rwr_sampler: graph " + std::to_string(g) + " has " + std::to_string(n) +
                                                   " vertices; 10 n k must fit the reference's int iteration limit");
            status[(size_t)g] = s.failed ? 1 : 0;
            UgsRwrGraph &d = gd[(size_t)g];
            d.lo = ptr[g]; d.vbase = s.vbase; d.n = s.n;
            d.T = n >= k && !s.failed ? (int32_t)(n * k * 10) : 0;      // (T = 0: m rows of -1 and no draws)
            half[(size_t)g] = s.failed ? 0 : 2 * s.cols;
            return (int)UGS_OK;
        })) return rc;
    DeviceCtx dc;
    if (int rc = cache_begin_device(st, cb, checked || have_cols, num_cols, dc)) return rc;
    const StoreGen *gen = cb.gen.get();
    const int64_t E = cb.E, rows = G * (int64_t)m_per_graph;
    const int64_t Ec = checked ? E : 0;                                  // columns that go up: none without the check
    // one blob: descriptors, seeds and (check) coff, col0 and the batch's columns go up in one copy; then the walks' scratch.
    // No half-edge arrays.
    BlobLayout L;
    auto take = [&](size_t bytes) { return L.take(bytes); };
    const size_t o_desc = take((size_t)G * sizeof(UgsRwrGraph)), o_seeds = take(per_graph ? (size_t)G * 8 : 0);
    const CheckInputs in(L, G, Ec, checked, false, checked);             // (the descriptors hold lo)
    L.end_inputs();
    const size_t o_rst = take((size_t)rows * 8), o_ec = take((size_t)rows * 4), o_st = take((size_t)ugs_scan_tmp_words(rows) * 8);
    std::vector<char> host(L.in_bytes, 0);
    if (G > 0) std::memcpy(host.data() + o_desc, gd.data(), (size_t)G * sizeof(UgsRwrGraph));
    if (per_graph && G > 0) std::memcpy(host.data() + o_seeds, seeds, (size_t)G * 8);
    in.stage(host.data(), cb, ptr, G, edge_index, row_stride);
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, UGS_JOB_RWR, G, m_per_graph, k, mode, L.off, &j, true)) return rc;
    if (int rc = side_job_rows(j, rows, 8)) return rc;                   // first_bad right behind the edge total: one read-back for both
    char *b = static_cast<char *>(j->blob.p);
    UgsRwrCall c{};
    c.G = G; c.rows = rows; c.m = m_per_graph; c.k = k; c.mode = mode; c.seed = seed; c.p = p_restart;
    c.seeds = per_graph ? reinterpret_cast<const uint64_t *>(b + o_seeds) : nullptr;
    c.spec = (int32_t)std::min<int64_t>(4, std::max<int64_t>(1, ((int64_t)m_per_graph * 16 + 255) / 256));
    c.graphs = reinterpret_cast<const UgsRwrGraph *>(b + o_desc);
    if (gen) { c.rs = gen->at<int32_t>(RS); c.hval2 = gen->at<int32_t>(TG); c.doomed = gen->at<uint8_t>(DOOMED); }
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
        q.src = reinterpret_cast<const int64_t *>(b + in.src); q.dst = reinterpret_cast<const int64_t *>(b + in.dst);
        q.graphs = c.graphs;
        q.coff = reinterpret_cast<const int64_t *>(b + in.coff); q.col0 = reinterpret_cast<const int64_t *>(b + in.col0);
        q.cols = gen->at<int2>(COLS); q.first_bad = d_bad;
        e = ugs_rwr_store_check(q, dc.stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(back, j->d_eptr + rows, run_check ? 16 : 8, hipMemcpyDeviceToHost, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e != hipSuccess) { free_job(j); return fail_hip(e, "rwr_sampler cache pipeline"); }
    j->total = back[0];
    if (run_check)
        if (int rc = cache_check_verdict(st, back[1], G)) { free_job(j); return rc; }
    for (int64_t g = 0; per_graph && g < G; ++g) graph_status[g] = status[(size_t)g];
    // the hook holds the generation the walks read: an add that regrows the store leaves this job its buffers
    j->fill = [c, keep = cb.gen](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) { return ugs_rwr_fill(c, edge_index, edge_src, ld, s); };
    return hand_out(j, job_out, total_edges_out);
}

}  // extern "C"
