// ugs_graph_cache.cpp -- host side of ugs_sampler.GraphCache in libugs_mi355.so: every dataset graph preprocessed once at the
// cache's k and kept on the device as one "plan of all added graphs"; a cached call over any batch of added graphs builds one
// descriptor per graph, O(G) on the host, and runs the walk, scan and fill kernels of the uncached call on them.
//
// Behavioural contract: the reference `ugs_sampler`'s sample_batch (src/ugs_sampler_batch_extension.cpp:41-299) on the collated batch
// with an empty preprocessing cache; the law is stated in include/ugs_mi355.h at ugs_graph_cache_sample_begin.  Preprocessing, plans,
// walks and fills come from ugs_host.cpp and the job from ugs_jobs.cpp, through ugs_host_internal.h; the store's own three kernels are
// in ugs_store.hip.  The store, the cache state and its locking, the front halves of the add and of the begin and the check's inputs
// are the dataset caches' (ugs_cache_common.cpp).  What is this cache's own -- preprocessing outside the LRU,
// degenerate graphs, the view plan, the rebase of edge_src, last_launch: DESIGN.md section 15.
#include "ugs_host_internal.h"

#include <cstdio>
#include <deque>

using namespace ugs_host;

namespace {
// What the host keeps of an added graph: its place in the store and what choose_tier needs of it.
struct UgsSlot {
    int64_t n = 0, nnz = 0, cols = 0;                      // vertices as added (also of a degenerate graph), CSR entries, columns
    int64_t rbase = 0, vbase = 0, viable_base = 0, col0 = 0;   // first rowptr entry, root record, viable entry, stored column
    int32_t level = -1, n_viable = 0;                      // level -1: degenerate (n <= 0 or n < k), m rows of -1, nothing stored but columns
    int64_t max_deg = 0;
    double sb_deg = 0.0;
};
// The store: the arrays of a plan of all added graphs (rowptr, adj and adjf, root records, viable lists) and the columns.
enum { ROWPTR, ADJ, ADJF, ROOTS, VIABLE, COLS };
enum { GR, GA, GV, GW, GC };
const StoreShape UGS_SHAPE = {6, 5, {{8, GR}, {8, GA}, {8, GA}, {sizeof(UgsRootRec), GV}, {8, GW}, {8, GC}}};
const char *const NAME = "graph cache";
struct UgsCacheState : CacheState {
    int k = 0;
    std::deque<UgsSlot> slots;
    UgsCacheState() : CacheState(UGS_SHAPE, NAME, "ugs_sampler", GV, GA) {}
};
// ugs_graph_cache_last_launch: the calling thread's last cached call
thread_local const void *t_last_cache = nullptr;
thread_local const char *t_last_walk = nullptr, *t_last_fill = nullptr;
}  // namespace
struct ugs_graph_cache { std::shared_ptr<UgsCacheState> st; };

extern "C" {

int ugs_graph_cache_create(int k, int64_t reserve_vertices, int64_t reserve_columns, ugs_graph_cache **cache_out) {
    if (!cache_out) return fail(UGS_E_BAD_ARG, "cache_out is null");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (int rc = cache_reserve_check(reserve_vertices, reserve_columns)) return rc;
    auto *c = new ugs_graph_cache();
    c->st = std::make_shared<UgsCacheState>();
    c->st->k = k;
    int64_t *r = c->st->reserve;
    r[GR] = reserve_vertices + reserve_vertices / 4; r[GA] = 2 * reserve_columns; r[GV] = reserve_vertices; r[GW] = 0; r[GC] = reserve_columns;
    *cache_out = c;
    return UGS_OK;
}

int ugs_graph_cache_destroy(ugs_graph_cache *cache) {
    delete cache;                                                        // a generation goes with the last job that walks on it
    return UGS_OK;
}

int ugs_graph_cache_info(ugs_graph_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *entries_out, int64_t *bytes_out,
                         int64_t *generations_out) {
    return cache_info(cache ? cache->st.get() : nullptr, graphs_out, vertices_out, entries_out, bytes_out, generations_out);
}

int ugs_graph_cache_last_launch(ugs_graph_cache *cache, char *walk_buf, int walk_buf_len, char *fill_buf, int fill_buf_len) {
    if (!cache) return fail(UGS_E_BAD_ARG, "cache is null");
    const bool mine = t_last_cache == cache->st.get();
    if (walk_buf && walk_buf_len > 0) std::snprintf(walk_buf, (size_t)walk_buf_len, "%s", mine && t_last_walk ? t_last_walk : "");
    if (fill_buf && fill_buf_len > 0) std::snprintf(fill_buf, (size_t)fill_buf_len, "%s", mine && t_last_fill ? t_last_fill : "");
    return UGS_OK;
}

int ugs_graph_cache_add(ugs_graph_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                        int64_t num_graphs, int64_t *slots_out) {
    if (int rc = cache_add_args(NAME, cache, edge_index, num_cols, ptr, num_graphs, slots_out, "slots_out", (int64_t)INT32_MAX, "2^31 - 1")) return rc;
    const int64_t G = num_graphs, E = num_cols;
    if (G == 0) return UGS_OK;
    UgsCacheState &st = *cache->st;
    const int k = st.k;
    std::vector<UgsSlot> fresh((size_t)G);
    std::vector<int64_t> cu((size_t)E), cv((size_t)E), cptr;
    std::vector<int32_t> none;
    if (int rc = scan_ptr(ptr, G, false, none, [&](int64_t g, int64_t n, std::string &why) {
            fresh[(size_t)g].n = n;
            if (n >= ((int64_t)1 << 30) - 1) why = "graph too large: num_nodes must be < 2^30 - 1";
            return !why.empty();
        })) return rc;
    if (int rc = cache_walk_columns(NAME, edge_index, row_stride, E, ptr, G, cptr, [&](int64_t x, int64_t, int64_t u, int64_t v) {
            cu[(size_t)x] = u; cv[(size_t)x] = v;
        })) return rc;
    for (int64_t g = 0; g < G; ++g) fresh[(size_t)g].cols = cptr[(size_t)g + 1] - cptr[(size_t)g];
    // Preprocessing at the cache's k, by the host stages every uncached miss goes through -- outside the registry, the LRU, the plan
    // cache and the batch index.  A graph of fewer than k vertices is degenerate, as in a batch plan: a slot, its columns, no arrays.
    std::vector<std::shared_ptr<Graph>> graphs((size_t)G);
    int64_t n_rows = 0, nnz = 0, n_roots = 0, n_via = 0;
    for (int64_t g = 0; g < G; ++g) {
        UgsSlot &s = fresh[(size_t)g];
        if (s.n <= 0 || s.n < k) continue;
        std::shared_ptr<Graph> &gr = graphs[(size_t)g];
        if (int rc = graph_outside_lru(cu.data() + cptr[(size_t)g], cv.data() + cptr[(size_t)g], s.cols, s.n, k, gr)) return rc;
        s.nnz = gr->nnz; s.level = gr->level; s.n_viable = gr->level > 0 ? (int32_t)gr->viable.size() : 0;
        s.max_deg = gr->max_deg; s.sb_deg = gr->sb_deg;
        s.rbase = n_rows; s.vbase = n_roots; s.viable_base = n_via;     // inside the chunk, as assemble_plan lays its pieces out
        n_rows += s.n + 1; n_roots += s.n; nnz += s.nnz; n_via += s.n_viable;
    }
    std::lock_guard<std::mutex> add_lk(st.add_mu);
    if (st.used[GA] + nnz >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "graph cache: the CSR entries of all added graphs must stay below 2^31 - 1");
    if (st.used[GC] + E >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "graph cache: the columns of all added graphs must stay below 2^31 - 1");
    CacheAdd add;
    if (int rc = cache_add_device(st, add)) return rc;
    const DeviceCtx &dc = add.dc;
    // the chunk as a plan of its own (pooled; uploaded before plan_of_graphs returns), and its columns beside it
    ugs_plan *chunk = new ugs_plan();
    chunk->view = true;                                                  // (never shared: nothing but this add's stream reads it)
    struct Drop { ugs_plan *p; PoolBuf cols; ~Drop() { pool_put(cols); plan_unref(p); } } drop{chunk, PoolBuf()};
    if (int rc = plan_of_graphs(graphs, dc, chunk)) return rc;
    if (int rc = pool_get((size_t)std::max<int64_t>(2 * E, 1) * 8, dc.id, drop.cols)) return rc;
    int64_t *d_cu = static_cast<int64_t *>(drop.cols.p), *d_cv = d_cu + E;
    add.need[GR] = st.used[GR] + n_rows; add.need[GA] = st.used[GA] + nnz; add.need[GV] = st.used[GV] + n_roots; add.need[GW] = st.used[GW] + n_via;
    add.need[GC] = st.used[GC] + E;
    if (int rc = cache_room(st, add)) return rc;
    const StoreGen &gen = *add.gen;
    UgsStoreAppend a{};
    a.rowptr = chunk->dev.rowptr; a.adj = chunk->dev.adj; a.adjf = chunk->dev.adjf; a.roots = chunk->dev.roots; a.viable = chunk->dev.viable;
    a.col_u = d_cu; a.col_v = d_cv;
    a.n_rowptr = n_rows; a.nnz = nnz; a.n_roots = n_roots; a.n_viable = n_via; a.n_cols = E;
    a.s_rowptr = gen.at<int64_t>(ROWPTR); a.s_adj = gen.at<int2>(ADJ); a.s_adjf = gen.at<int2>(ADJF); a.s_roots = gen.at<UgsRootRec>(ROOTS);
    a.s_viable = gen.at<int2>(VIABLE); a.s_cols = gen.at<int2>(COLS);
    a.row_base = st.used[GR]; a.adj_base = st.used[GA]; a.root_base = st.used[GV]; a.via_base = st.used[GW]; a.col_base = st.used[GC];
    hipError_t e = hipSuccess;
    if (E > 0) e = hipMemcpyAsync(d_cu, cu.data(), (size_t)E * 8, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(d_cv, cv.data(), (size_t)E * 8, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_store_append(a, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e != hipSuccess) return fail_hip(e, "graph cache add");          // (a new generation is dropped: the cache is as it was)
    cache_publish(st, add, G, [&] {
        for (int64_t g = 0; g < G; ++g) {
            UgsSlot &s = fresh[(size_t)g];
            s.rbase += st.used[GR]; s.vbase += st.used[GV]; s.viable_base += st.used[GW];
            s.col0 = st.used[GC] + cptr[(size_t)g];
            slots_out[g] = (int64_t)st.slots.size();
            st.slots.push_back(s);
        }
    });
    return UGS_OK;
}

int ugs_graph_cache_sample_begin(ugs_graph_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                                 const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, int seed, const int32_t *seeds, int check,
                                 ugs_job **job_out, int64_t *total_edges_out) {
    if (int rc = cache_begin_args(NAME, cache && job_out && ptr, slots, edge_index, num_cols, num_graphs, check)) return rc;
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    const std::shared_ptr<UgsCacheState> stp = cache->st;
    UgsCacheState &st = *stp;
    const int64_t G = num_graphs;
    const int k = st.k;
    const bool checked = check != 0, have_cols = edge_index != nullptr;
    // O(G): one descriptor per graph from its slot, the prefix sums of the column counts, and what choose_tier reads
    std::vector<UgsGraphDesc> gd((size_t)G);
    ugs_plan *plan = new ugs_plan();
    plan->view = true;
    plan->prow_failed = true;                                            // no padded rows for the store: 64-lane tiers read rows through rowptr
    struct Unref { ugs_plan *p; ~Unref() { plan_unref(p); } } unref{plan};   // (begin_common takes the reference over: p is cleared before)
    plan->g_n.resize((size_t)G); plan->g_maxdeg.resize((size_t)G); plan->g_sbdeg.resize((size_t)G); plan->g_level.resize((size_t)G);
    CacheBatch cb;
    if (int rc = cache_scan_slots(st, st.slots, slots, ptr, G, cb, [&](int64_t g, const UgsSlot &s, int64_t) {
            UgsGraphDesc &d = gd[(size_t)g];
            const bool live = s.level >= 0;
            d.node_lo = ptr[g]; d.rbase = s.rbase; d.vbase = s.vbase; d.viable_base = s.viable_base;
            d.n = live ? (int32_t)s.n : 0; d.level = s.level; d.n_viable = s.n_viable; d.pad = 0;
            plan->g_n[(size_t)g] = live ? s.n : 0; plan->g_maxdeg[(size_t)g] = s.max_deg; plan->g_sbdeg[(size_t)g] = s.sb_deg; plan->g_level[(size_t)g] = s.level;
            plan->nverts += live ? s.n : 0; plan->nnz += s.nnz;
            return (int)UGS_OK;
        })) return rc;
    DeviceCtx dc;
    if (int rc = cache_begin_device(st, cb, checked || have_cols, num_cols, dc)) return rc;
    const StoreGen *gen = cb.gen.get();
    const std::vector<int64_t> &coff = cb.coff;
    const int64_t E = cb.E;
    const int64_t rows = G * (int64_t)m_per_graph;
    const bool run_check = checked && E > 0 && gen;
    const int64_t Ec = run_check ? E : 0;                                // columns that go up: none without the check
    // the view plan's blob: descriptors, coff and (check) ptr, col0 and the batch's columns go up in one copy; first_bad behind them
    BlobLayout L;
    const size_t o_desc = L.take((size_t)G * sizeof(UgsGraphDesc));
    const CheckInputs in(L, G, Ec, true, run_check, run_check);          // (coff goes up with or without the check: the rebase reads it)
    L.end_inputs();
    const size_t o_bad = L.take(8);
    std::vector<char> host(L.in_bytes, 0);
    if (G > 0) std::memcpy(host.data() + o_desc, gd.data(), (size_t)G * sizeof(UgsGraphDesc));
    in.stage(host.data(), cb, ptr, G, edge_index, row_stride);
    if (int rc = pool_get(L.off, dc.id, plan->blob_buf)) return rc;
    char *b = static_cast<char *>(plan->blob_buf.p);
    plan->device = dc.id; plan->cus = dc.cus; plan->G = G;
    plan->blob = b; plan->blob_bytes = L.off;
    plan->dev.graphs = reinterpret_cast<const UgsGraphDesc *>(b + o_desc);
    if (gen) {
        plan->dev.rowptr = gen->at<int64_t>(ROWPTR); plan->dev.adj = gen->at<int2>(ADJ); plan->dev.adjf = gen->at<int2>(ADJF);
        plan->dev.roots = gen->at<UgsRootRec>(ROOTS); plan->dev.viable = gen->at<int2>(VIABLE);
        plan->keep.push_back(cb.gen);                                      // an add that regrows the store leaves this job its buffers
    }
    plan->dev.num_graphs = G;
    const int64_t *d_coff = reinterpret_cast<const int64_t *>(b + in.coff);
    int32_t *d_bad = reinterpret_cast<int32_t *>(b + o_bad);
    // first_bad travels to a pinned word behind the check, ahead of the walks on the same stream: it is there when the edge total is
    char *pin = run_check ? pin_slot_get() : nullptr;
    struct PinBack { char *p; ~PinBack() { pin_slot_put(p); } } pin_back{pin};
    if (pin) std::memset(pin, 0xff, 4);                                  // -1: not written yet
    HIP_TRY(hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream));
    if (run_check) {
        HIP_TRY(hipMemsetAsync(d_bad, 0x7f, 8, dc.stream));              // above every g
        UgsStoreCheck q{};
        q.E = Ec; q.G = G;
        q.src = reinterpret_cast<const int64_t *>(b + in.src); q.dst = reinterpret_cast<const int64_t *>(b + in.dst);
        q.lo = reinterpret_cast<const int64_t *>(b + in.lo); q.coff = d_coff; q.col0 = reinterpret_cast<const int64_t *>(b + in.col0);
        q.cols = gen->at<int2>(COLS); q.first_bad = d_bad;
        HIP_TRY(ugs_store_check(q, dc.stream));
        if (pin) HIP_TRY(hipMemcpyAsync(pin, d_bad, 4, hipMemcpyDeviceToHost, dc.stream));
    }
    // the job: walk and scan (and, for batches of small graphs, the packed step) exactly as on a batch plan
    unref.p = nullptr;
    ugs_job *j = nullptr;
    int rc = begin_common(plan, m_per_graph, k, mode, 0, seed, &j, nullptr, G > 0 ? seeds : nullptr);
    if (rc != UGS_OK) { (void)hipStreamSynchronize(dc.stream); return rc; }      // (the upload's source is this call's)
    if (run_check) {
        int32_t bad = 0x7f7f7f7f;
        hipError_t e = hipSuccess;
        if (pin) {                                                       // (the total is known: everything queued ahead of the walks is over)
            std::memcpy(&bad, pin, 4);
            if (bad == -1) { e = hipStreamSynchronize(dc.stream); std::memcpy(&bad, pin, 4); }
        }
        else { e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, dc.stream); if (e == hipSuccess) e = hipStreamSynchronize(dc.stream); }
        if (e != hipSuccess) { free_job(j); return fail_hip(e, "graph cache check"); }
        if (int refused = cache_check_verdict(st, bad, G)) {
            (void)hipStreamSynchronize(dc.stream);
            free_job(j);
            return refused;
        }
    }
    // edge_src: the store's columns are local to their graph; coff[g] makes them the batch's
    t_last_cache = stp.get(); t_last_walk = plan->last_walk.name; t_last_fill = plan->last_fill.name;
    const bool shift = G > 1 && coff[(size_t)G - 1] > 0 && rows > 0;
    const void *who = stp.get();
    // (the kernel reads coff in the plan's blob: the plan's last-kernel event moves behind it, so that the plan outlives it)
    auto rebase = [plan](const int64_t *edge_ptr, int64_t *edge_src, const int64_t *cf, int64_t nrows, int m, hipStream_t s) {
        hipError_t e = ugs_store_rebase_src(edge_ptr, edge_src, cf, nrows, m, s);
        std::lock_guard<std::mutex> lk(plan->mu);
        if (e == hipSuccess && plan_leave(plan, s) != UGS_OK) e = hipErrorUnknown;
        return e;
    };
    if (j->packed_ok && j->total > 0) {
        int64_t *d_es = static_cast<int64_t *>(j->nodes.p) + (rows * k + rows + 1) + 2 * j->total;
        if (shift)
            if (hipError_t e = rebase(j->d_eptr, d_es, d_coff, rows, m_per_graph, dc.stream); e != hipSuccess) { free_job(j); return fail_hip(e, "ugs_store_rebase_src"); }
    } else {
        const int64_t *d_eptr = j->d_eptr;
        const int m = m_per_graph;
        j->after_fill = [plan, who, shift, d_eptr, d_coff, rows, m, rebase](int64_t *edge_src, hipStream_t s) {
            if (t_last_cache == who) t_last_fill = plan->last_fill.name;
            return shift ? rebase(d_eptr, edge_src, d_coff, rows, m, s) : hipSuccess;
        };
    }
    return hand_out(j, job_out, total_edges_out);
}

}  // extern "C"
