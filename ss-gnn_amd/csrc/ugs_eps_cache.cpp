// ugs_eps_cache.cpp -- host side of epsilon_uniform_sampler.GraphCache in libugs_mi355.so: the adjacency lists of every dataset graph
// built once, on the device (ugs_eps_build in ugs_eps.hip), and kept there as one "batch of all added graphs"; a cached call over any
// batch of added graphs builds one descriptor per graph, O(G) on the host, and runs the walk, scan and fill kernels of the uncached
// call on them.  The adjacency depends on neither k nor epsilon, so both are arguments of the call and one cache serves every value.
//
// Behavioural contract: ugs_eps_sample_batch_begin / ugs_eps_sample_graphs_begin (ugs_side_eps.cpp) on the collated batch; the law is
// stated in include/ugs_mi355.h at ugs_eps_cache_sample_begin.  The job and the pieces the begin is built from are the job path's
// (ugs_jobs.cpp; ugs_host_internal.h); the check is ugs_store_check of ugs_store.hip.  The store, the cache
// state and its locking, the front halves of the add and of the begin and the check's inputs are the dataset caches'
// (ugs_cache_common.cpp).  What is this cache's own -- layout, the build kernel, graph_csr: DESIGN.md section 16.
#include "ugs_host_internal.h"

#include <deque>

using namespace ugs_host;

namespace {
// What the host keeps of an added graph: its place in the store.
struct EpsSlot {
    int64_t n = 0, cols = 0;                  // vertices as added, columns
    int64_t rbase = 0, abase = 0, col0 = 0;   // first rowptr entry, first nbr / ecs entry, first stored column
};
// The store: rowptr per vertex (plus one entry per graph), nbr and ecs per half-edge, cols per column.
enum { ROWPTR, NBR, ECS, COLS };
enum { GR, GH, GC };
const StoreShape EPS_SHAPE = {4, 3, {{8, GR}, {4, GH}, {4, GH}, {8, GC}}};
const char *const NAME = "eps cache";
struct EpsCacheState : CacheState {
    std::deque<EpsSlot> slots;
    EpsCacheState() : CacheState(EPS_SHAPE, NAME, "epsilon_uniform_sampler", GR, GH) {}
};
}  // namespace
struct ugs_eps_cache { std::shared_ptr<EpsCacheState> st; };

extern "C" {

int ugs_eps_cache_create(int64_t reserve_vertices, int64_t reserve_columns, ugs_eps_cache **cache_out) {
    if (!cache_out) return fail(UGS_E_BAD_ARG, "cache_out is null");
    if (int rc = cache_reserve_check(reserve_vertices, reserve_columns)) return rc;
    auto *c = new ugs_eps_cache();
    c->st = std::make_shared<EpsCacheState>();
    c->st->reserve[GR] = reserve_vertices; c->st->reserve[GH] = 2 * reserve_columns; c->st->reserve[GC] = reserve_columns;
    *cache_out = c;
    return UGS_OK;
}

int ugs_eps_cache_destroy(ugs_eps_cache *cache) {
    delete cache;                                                        // a generation goes with the last job that walked on it
    return UGS_OK;
}

int ugs_eps_cache_info(ugs_eps_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *half_edges_out, int64_t *bytes_out,
                       int64_t *generations_out) {
    return cache_info(cache ? cache->st.get() : nullptr, graphs_out, vertices_out, half_edges_out, bytes_out, generations_out);
}

int ugs_eps_cache_add(ugs_eps_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                      int64_t num_graphs, int64_t *slots_out) {
    if (int rc = cache_add_args(NAME, cache, edge_index, num_cols, ptr, num_graphs, slots_out, "slots_out", (int64_t)1 << 30, "2^30")) return rc;
    const int64_t G = num_graphs, E = num_cols;
    if (G == 0) return UGS_OK;
    EpsCacheState &st = *cache->st;
    std::vector<EpsSlot> fresh((size_t)G);
    std::vector<int64_t> vptr((size_t)G + 1, 0), cptr;
    std::vector<int32_t> none;
    if (int rc = scan_ptr(ptr, G, false, none, [&](int64_t g, int64_t n, std::string &why) {
            if (n >= (int64_t)INT32_MAX) why = "graph too large";       // (eps_begin's text)
            fresh[(size_t)g].n = n;
            vptr[(size_t)g + 1] = vptr[(size_t)g] + n;
            return !why.empty();
        })) return rc;
    const int64_t NV = vptr[(size_t)G], n_rows = NV + G;
    if (n_rows >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "add too large: vertices plus graphs must be < 2^31 - 1");
    std::vector<int2> local((size_t)E);                                  // the add's columns as the store keeps them: pairs of local ids
    if (int rc = cache_walk_columns(NAME, edge_index, row_stride, E, ptr, G, cptr, [&](int64_t x, int64_t, int64_t u, int64_t v) {
            local[(size_t)x] = make_int2((int32_t)u, (int32_t)v);
        })) return rc;
    for (int64_t g = 0; g < G; ++g) fresh[(size_t)g].cols = cptr[(size_t)g + 1] - cptr[(size_t)g];
    std::lock_guard<std::mutex> add_lk(st.add_mu);
    if (st.used[GH] + 2 * E >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "eps cache: the half-edges of all added graphs must stay below 2^31");
    if (st.used[GR] + n_rows >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "eps cache: vertices plus graphs of all adds must stay below 2^31");
    CacheAdd a;
    if (int rc = cache_add_device(st, a)) return rc;
    const DeviceCtx &dc = a.dc;
    // the build's blob: the two prefix arrays (one copy), then one cursor per vertex.  The columns go straight into the store.
    BlobLayout L;
    const size_t o_vptr = L.take((size_t)(G + 1) * 8), o_cptr = L.take((size_t)(G + 1) * 8);
    L.end_inputs();
    const size_t o_cur = L.take((size_t)NV * 4);
    std::vector<char> host(L.in_bytes, 0);
    std::memcpy(host.data() + o_vptr, vptr.data(), (size_t)(G + 1) * 8);
    std::memcpy(host.data() + o_cptr, cptr.data(), (size_t)(G + 1) * 8);
    a.need[GR] = st.used[GR] + n_rows; a.need[GH] = st.used[GH] + 2 * E; a.need[GC] = st.used[GC] + E;
    if (int rc = cache_room(st, a)) return rc;
    const StoreGen &gen = *a.gen;
    PoolBuf blob;
    if (int rc = pool_get(L.off, dc.id, blob)) return rc;
    char *b = static_cast<char *>(blob.p);
    UgsEpsBuild w{};
    w.G = G;
    w.vptr = reinterpret_cast<const int64_t *>(b + o_vptr); w.cptr = reinterpret_cast<const int64_t *>(b + o_cptr);
    w.cursor = reinterpret_cast<int32_t *>(b + o_cur);
    w.rowptr = gen.at<int64_t>(ROWPTR); w.nbr = gen.at<int32_t>(NBR); w.ecs = gen.at<int32_t>(ECS); w.cols = gen.at<int2>(COLS);
    w.row_base = st.used[GR]; w.adj_base = st.used[GH]; w.col_base = st.used[GC];
    // (beyond what is published nothing reads: the columns land in the store, the kernel reads them there and writes behind used_*)
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(gen.at<int2>(COLS) + st.used[GC], local.data(), (size_t)E * 8, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_eps_build(w, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    pool_put(blob);
    if (e != hipSuccess) return fail_hip(e, "epsilon_uniform_sampler cache add");   // (a new generation is dropped: the cache is as it was)
    cache_publish(st, a, G, [&] {
        for (int64_t g = 0; g < G; ++g) {
            EpsSlot &s = fresh[(size_t)g];
            s.rbase = st.used[GR] + vptr[(size_t)g] + g;
            s.abase = st.used[GH] + 2 * cptr[(size_t)g];
            s.col0 = st.used[GC] + cptr[(size_t)g];
            slots_out[g] = (int64_t)st.slots.size();
            st.slots.push_back(s);
        }
    });
    return UGS_OK;
}

int ugs_eps_cache_graph_csr(ugs_eps_cache *cache, int64_t slot, int64_t node_capacity, int64_t entry_capacity, int64_t *num_nodes,
                            int64_t *num_entries, int64_t *rowptr, int32_t *nbr, int32_t *ecs) {
    if (!cache) return fail(UGS_E_BAD_ARG, "cache is null");
    EpsCacheState &st = *cache->st;
    EpsSlot s;
    std::shared_ptr<StoreGen> gen;
    int dev = -1;
    {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        if (slot < 0 || slot >= (int64_t)st.slots.size()) return fail(UGS_E_BAD_ARG, "unknown eps cache slot " + std::to_string(slot));
        s = st.slots[(size_t)slot];
        gen = st.gen;
        dev = st.dev;
    }
    const int64_t nnz = 2 * s.cols;
    if (num_nodes) *num_nodes = s.n;
    if (num_entries) *num_entries = nnz;
    if ((rowptr && node_capacity < s.n) || ((nbr || ecs) && entry_capacity < nnz)) return fail(UGS_E_CAPACITY, "eps cache graph csr: capacity too small");
    HIP_TRY(hipSetDevice(dev));
    if (rowptr) {
        HIP_TRY(hipMemcpy(rowptr, gen->at<int64_t>(ROWPTR) + s.rbase, (size_t)(s.n + 1) * 8, hipMemcpyDeviceToHost));
        for (int64_t r = 0; r <= s.n; ++r) rowptr[r] -= s.abase;
    }
    if (nbr && nnz > 0) HIP_TRY(hipMemcpy(nbr, gen->at<int32_t>(NBR) + s.abase, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    if (ecs && nnz > 0) HIP_TRY(hipMemcpy(ecs, gen->at<int32_t>(ECS) + s.abase, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    return UGS_OK;
}

int ugs_eps_cache_sample_begin(ugs_eps_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                               const int64_t *ptr, int64_t num_graphs, int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds,
                               double epsilon, int check, int32_t *graph_status, ugs_job **job_out, int64_t *total_edges_out) {
    if (int rc = cache_begin_args(NAME, cache && job_out && ptr, slots, edge_index, num_cols, num_graphs, check)) return rc;
    if (!(epsilon > 0.0 && epsilon <= 1.0)) return fail(UGS_E_BAD_ARG, "epsilon must be in (0, 1]");      // (eps_begin's checks and texts)
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    const std::shared_ptr<EpsCacheState> stp = cache->st;
    EpsCacheState &st = *stp;
    const int64_t G = num_graphs;
    const bool have_cols = edge_index != nullptr;                        // check == 0 and no edge_index: num_cols says nothing
    const bool checked = check != 0;
    // O(G): one descriptor per graph from its slot and the prefix sums of the column counts
    std::vector<UgsGraphDesc> gd((size_t)G);
    CacheBatch cb;
    if (int rc = cache_scan_slots(st, st.slots, slots, ptr, G, cb, [&](int64_t g, const EpsSlot &s, int64_t) {
            UgsGraphDesc &d = gd[(size_t)g];
            d.node_lo = ptr[g]; d.rbase = s.rbase; d.vbase = 0; d.viable_base = 0; d.n = (int32_t)s.n; d.level = 0; d.n_viable = 0; d.pad = 0;
            return (int)UGS_OK;
        })) return rc;
    DeviceCtx dc;
    if (int rc = cache_begin_device(st, cb, checked || have_cols, num_cols, dc)) return rc;
    const StoreGen *gen = cb.gen.get();
    const int64_t E = cb.E;
    const int64_t rows = G * (int64_t)m_per_graph;
    const bool run_check = checked && E > 0 && gen;
    const int64_t Ec = run_check ? E : 0;                                // columns that go up: none without the check
    // one blob: descriptors, coff, seeds and (check) ptr, col0 and the batch's columns go up in one copy; then the walks' scratch.
    // No adjacency arrays.
    BlobLayout L;
    const size_t o_desc = L.take((size_t)G * sizeof(UgsGraphDesc)), o_seeds = L.take(seeds ? (size_t)G * 8 : 0);
    const CheckInputs in(L, G, Ec, true, run_check, run_check);          // (coff goes up with or without the check: it is the rows' col_base)
    L.end_inputs();
    const size_t o_counts = L.take((size_t)rows * sizeof(uint32_t)), o_st = L.take((size_t)ugs_scan_tmp_words(rows) * sizeof(int64_t));
    std::vector<char> host(L.in_bytes, 0);
    if (G > 0) std::memcpy(host.data() + o_desc, gd.data(), (size_t)G * sizeof(UgsGraphDesc));
    if (seeds && G > 0) std::memcpy(host.data() + o_seeds, seeds, (size_t)G * 8);
    in.stage(host.data(), cb, ptr, G, edge_index, row_stride);
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, UGS_JOB_EPS, G, m_per_graph, k, mode, L.off, &j, true)) return rc;
    if (int rc = side_job_rows(j, rows, 8)) return rc;                   // first_bad right behind the edge total: one read-back for both
    char *b = static_cast<char *>(j->blob.p);
    UgsEpsLaunch l{};
    l.graphs = reinterpret_cast<const UgsGraphDesc *>(b + o_desc);
    if (gen) { l.rowptr = gen->at<int64_t>(ROWPTR); l.nbr = gen->at<int32_t>(NBR); l.ecs = gen->at<int32_t>(ECS); }
    l.num_graphs = G; l.m = m_per_graph; l.k = k; l.mode = mode;
    l.max_attempts = std::max(10, (int)(10.0 / epsilon));
    l.seed = seed; l.seeds = seeds ? reinterpret_cast<const uint64_t *>(b + o_seeds) : nullptr;
    l.epsilon = epsilon; l.rows = rows;
    l.nodes = static_cast<int64_t *>(j->nodes.p); l.counts = reinterpret_cast<uint32_t *>(b + o_counts);
    l.col_base = reinterpret_cast<const int64_t *>(b + in.coff);          // the rows hold columns local to their graph
    int64_t back[2] = {0, 0};                                            // the edge total, and the check's first_bad in the low word behind it
    int32_t *d_bad = reinterpret_cast<int32_t *>(j->d_eptr + rows + 1);
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess && run_check) e = hipMemsetAsync(d_bad, 0x7f, 8, dc.stream);        // above every g
    if (e == hipSuccess) e = ugs_eps_launch(l, 0, dc.cus, dc.stream);
    if (e == hipSuccess) e = ugs_launch_scan(l.counts, rows, j->d_eptr, reinterpret_cast<int64_t *>(b + o_st), dc.stream);
    if (e == hipSuccess && run_check) {
        UgsStoreCheck q{};
        q.E = Ec; q.G = G;
        q.src = reinterpret_cast<const int64_t *>(b + in.src); q.dst = reinterpret_cast<const int64_t *>(b + in.dst);
        q.lo = reinterpret_cast<const int64_t *>(b + in.lo); q.coff = l.col_base; q.col0 = reinterpret_cast<const int64_t *>(b + in.col0);
        q.cols = gen->at<int2>(COLS); q.first_bad = d_bad;
        e = ugs_store_check(q, dc.stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(back, j->d_eptr + rows, run_check ? 16 : 8, hipMemcpyDeviceToHost, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e != hipSuccess) { free_job(j); return fail_hip(e, "epsilon_uniform_sampler cache pipeline"); }
    j->total = back[0];
    if (run_check)
        if (int rc = cache_check_verdict(st, back[1], G)) { free_job(j); return rc; }
    if (seeds && graph_status) std::fill(graph_status, graph_status + G, 0);       // no graph of this sampler fails alone
    // the hook holds the generation the walks read: an add that regrows the store leaves this job its buffers
    j->fill = [l, keep = cb.gen, d_eptr = j->d_eptr, cus = dc.cus](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
        UgsEpsLaunch f = l;
        f.edge_ptr = d_eptr; f.edge_index = edge_index; f.edge_src = edge_src; f.ld = ld;
        return ugs_eps_launch(f, 1, cus, s);
    };
    return hand_out(j, job_out, total_edges_out);
}

}  // extern "C"
