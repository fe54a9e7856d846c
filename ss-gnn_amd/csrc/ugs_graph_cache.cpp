// ugs_graph_cache.cpp -- host side of ugs_sampler.GraphCache in libugs_mi355.so: every dataset graph preprocessed once at the
// cache's k and kept on the device as one "plan of all added graphs"; a cached call over any batch of added graphs builds one
// descriptor per graph, O(G) on the host, and runs the walk, scan and fill kernels of the uncached call on them.
//
// Behavioural contract: the reference `ugs_sampler`'s sample_batch (src/ugs_sampler_batch_extension.cpp:41-299) on the collated batch
// with an empty preprocessing cache; the law is stated in include/ugs_mi355.h at ugs_graph_cache_sample_begin.  Preprocessing, plans,
// walks and fills come from ugs_host.cpp and the job from ugs_jobs.cpp, through ugs_host_internal.h; the store's own three kernels are
// in ugs_store.hip.  Layout, generations and the cached call: DESIGN.md section 15.
#include "ugs_host_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

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
// One generation of the storage.  Growth makes a new one and copies; a job's view plan holds the one it walks on.
struct UgsGen {
    int64_t *rowptr = nullptr;
    int2 *adj = nullptr, *adjf = nullptr, *viable = nullptr, *cols = nullptr;
    UgsRootRec *roots = nullptr;
    int64_t cap_r = 0, cap_a = 0, cap_v = 0, cap_w = 0, cap_c = 0;   // entries of rowptr, of adj / adjf, of roots, of viable, of cols
    ~UgsGen() { (void)hipFree(rowptr); (void)hipFree(adj); (void)hipFree(adjf); (void)hipFree(roots); (void)hipFree(viable); (void)hipFree(cols); }
    int64_t bytes() const { return cap_r * 8 + cap_a * 16 + cap_v * (int64_t)sizeof(UgsRootRec) + cap_w * 8 + cap_c * 8; }
    int alloc(int64_t r, int64_t a, int64_t v, int64_t w, int64_t c) {
        cap_r = std::max<int64_t>(r, 1); cap_a = std::max<int64_t>(a, 1); cap_v = std::max<int64_t>(v, 1); cap_w = std::max<int64_t>(w, 1);
        cap_c = std::max<int64_t>(c, 1);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&rowptr), (size_t)cap_r * 8));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&adj), (size_t)cap_a * 8));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&adjf), (size_t)cap_a * 8));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&roots), (size_t)cap_v * sizeof(UgsRootRec)));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&viable), (size_t)cap_w * 8));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cols), (size_t)cap_c * 8));
        return UGS_OK;
    }
};
struct UgsCacheState {
    int k = 0, dev = -1;
    int64_t reserve_v = 0, reserve_c = 0;
    std::mutex add_mu;                        // adds, one at a time, from the preprocessing to the publication
    std::shared_mutex mu;                     // what a sample begin reads: slots and gen (exclusive only to publish an add)
    std::deque<UgsSlot> slots;
    std::shared_ptr<UgsGen> gen;
    int64_t used_r = 0, used_a = 0, used_v = 0, used_w = 0, used_c = 0, generations = 0;
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
    if (reserve_vertices < 0 || reserve_vertices >= (int64_t)INT32_MAX || reserve_columns < 0 || reserve_columns >= ((int64_t)1 << 30))
        return fail(UGS_E_BAD_ARG, "reserve must be 0 ... 2^31 - 2 vertices and 0 ... 2^30 - 1 columns");
    auto *c = new ugs_graph_cache();
    c->st = std::make_shared<UgsCacheState>();
    c->st->k = k; c->st->reserve_v = reserve_vertices; c->st->reserve_c = reserve_columns;
    *cache_out = c;
    return UGS_OK;
}

int ugs_graph_cache_destroy(ugs_graph_cache *cache) {
    delete cache;                                                        // a generation goes with the last job that walks on it
    return UGS_OK;
}

int ugs_graph_cache_info(ugs_graph_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *entries_out, int64_t *bytes_out,
                         int64_t *generations_out) {
    if (!cache) return fail(UGS_E_BAD_ARG, "cache is null");
    UgsCacheState &st = *cache->st;
    std::shared_lock<std::shared_mutex> lk(st.mu);
    if (graphs_out) *graphs_out = (int64_t)st.slots.size();
    if (vertices_out) *vertices_out = st.used_v;
    if (entries_out) *entries_out = st.used_a;
    if (bytes_out) *bytes_out = st.gen ? st.gen->bytes() : 0;
    if (generations_out) *generations_out = st.generations;
    return UGS_OK;
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
    if (!cache || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to graph cache add");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !slots_out) return fail(UGS_E_BAD_ARG, "graph cache add needs slots_out");
    if (num_cols >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "add too large: columns must be < 2^31 - 1");
    UgsCacheState &st = *cache->st;
    const int64_t G = num_graphs, E = num_cols;
    const int k = st.k;
    if (G == 0) {
        if (E > 0) return fail(UGS_E_BAD_ARG, "graph cache add: columns without a graph");
        return UGS_OK;
    }
    // Columns must come graph by graph, in the order of the graphs, both endpoints inside the graph: that order is what a batch is
    // compared with, and a column that left its graph could fall into a neighbour's range once the graph stands in a batch.
    std::vector<UgsSlot> fresh((size_t)G);
    std::vector<int64_t> cu((size_t)E), cv((size_t)E), cptr((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = ptr[g + 1] - ptr[g];
        if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
        if (n >= ((int64_t)1 << 30) - 1) return fail(UGS_E_UNSUPPORTED, "graph too large: num_nodes must be < 2^30 - 1");
        fresh[(size_t)g].n = n;
    }
    {
        int64_t g = 0;
        for (int64_t x = 0; x < E; ++x) {
            const int64_t u = edge_index[x], v = edge_index[row_stride + x];
            while (g < G && !(ptr[g] <= u && u < ptr[g + 1])) ++g;
            if (g >= G || !(ptr[g] <= v && v < ptr[g + 1]))
                return fail(UGS_E_BAD_ARG, "graph cache add: column " + std::to_string(x) + " is not inside one graph, or the columns are not in the order of the graphs");
            ++fresh[(size_t)g].cols;
            cu[(size_t)x] = u - ptr[g]; cv[(size_t)x] = v - ptr[g];
        }
    }
    for (int64_t g = 0; g < G; ++g) cptr[(size_t)g + 1] = cptr[(size_t)g] + fresh[(size_t)g].cols;
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
    std::lock_guard<std::mutex> add_lk(st.add_mu);                       // (only adds write used_* and gen: reading them here needs no more)
    if (st.used_a + nnz >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "graph cache: the CSR entries of all added graphs must stay below 2^31 - 1");
    if (st.used_c + E >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "graph cache: the columns of all added graphs must stay below 2^31 - 1");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (st.dev >= 0 && st.dev != dc.id)
        return fail(UGS_E_BAD_ARG, "the graph cache lives on device " + std::to_string(st.dev) + ", this add runs on device " + std::to_string(dc.id));
    HIP_TRY(hipSetDevice(dc.id));
    // the chunk as a plan of its own (pooled; uploaded before plan_of_graphs returns), and its columns beside it
    ugs_plan *chunk = new ugs_plan();
    chunk->view = true;                                                  // (never shared: nothing but this add's stream reads it)
    struct Drop { ugs_plan *p; PoolBuf cols; ~Drop() { pool_put(cols); plan_unref(p); } } drop{chunk, PoolBuf()};
    if (int rc = plan_of_graphs(graphs, dc, chunk)) return rc;
    if (int rc = pool_get((size_t)std::max<int64_t>(2 * E, 1) * 8, dc.id, drop.cols)) return rc;
    int64_t *d_cu = static_cast<int64_t *>(drop.cols.p), *d_cv = d_cu + E;
    // room in the store: this generation, or a new one of at least twice the size with everything held so far copied over
    std::shared_ptr<UgsGen> gen = st.gen;
    const int64_t need_r = st.used_r + n_rows, need_a = st.used_a + nnz, need_v = st.used_v + n_roots, need_w = st.used_w + n_via, need_c = st.used_c + E;
    const bool grow = !gen || need_r > gen->cap_r || need_a > gen->cap_a || need_v > gen->cap_v || need_w > gen->cap_w || need_c > gen->cap_c;
    if (grow) {
        auto room = [](int64_t need, int64_t have, int64_t reserve) { return need <= have ? have : std::max({need, 2 * have, reserve}); };
        const std::shared_ptr<UgsGen> old = gen;
        gen = std::make_shared<UgsGen>();
        if (int rc = gen->alloc(room(need_r, old ? old->cap_r : 0, st.reserve_v + st.reserve_v / 4), room(need_a, old ? old->cap_a : 0, 2 * st.reserve_c),
                                room(need_v, old ? old->cap_v : 0, st.reserve_v), room(need_w, old ? old->cap_w : 0, 0),
                                room(need_c, old ? old->cap_c : 0, st.reserve_c))) return rc;
        if (old) {
            if (st.used_r > 0) HIP_TRY(hipMemcpyAsync(gen->rowptr, old->rowptr, (size_t)st.used_r * 8, hipMemcpyDeviceToDevice, dc.stream));
            if (st.used_a > 0) {
                HIP_TRY(hipMemcpyAsync(gen->adj, old->adj, (size_t)st.used_a * 8, hipMemcpyDeviceToDevice, dc.stream));
                HIP_TRY(hipMemcpyAsync(gen->adjf, old->adjf, (size_t)st.used_a * 8, hipMemcpyDeviceToDevice, dc.stream));
            }
            if (st.used_v > 0) HIP_TRY(hipMemcpyAsync(gen->roots, old->roots, (size_t)st.used_v * sizeof(UgsRootRec), hipMemcpyDeviceToDevice, dc.stream));
            if (st.used_w > 0) HIP_TRY(hipMemcpyAsync(gen->viable, old->viable, (size_t)st.used_w * 8, hipMemcpyDeviceToDevice, dc.stream));
            if (st.used_c > 0) HIP_TRY(hipMemcpyAsync(gen->cols, old->cols, (size_t)st.used_c * 8, hipMemcpyDeviceToDevice, dc.stream));
        }
    }
    UgsStoreAppend a{};
    a.rowptr = chunk->dev.rowptr; a.adj = chunk->dev.adj; a.adjf = chunk->dev.adjf; a.roots = chunk->dev.roots; a.viable = chunk->dev.viable;
    a.col_u = d_cu; a.col_v = d_cv;
    a.n_rowptr = n_rows; a.nnz = nnz; a.n_roots = n_roots; a.n_viable = n_via; a.n_cols = E;
    a.s_rowptr = gen->rowptr; a.s_adj = gen->adj; a.s_adjf = gen->adjf; a.s_roots = gen->roots; a.s_viable = gen->viable; a.s_cols = gen->cols;
    a.row_base = st.used_r; a.adj_base = st.used_a; a.root_base = st.used_v; a.via_base = st.used_w; a.col_base = st.used_c;
    hipError_t e = hipSuccess;
    if (E > 0) e = hipMemcpyAsync(d_cu, cu.data(), (size_t)E * 8, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(d_cv, cv.data(), (size_t)E * 8, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_store_append(a, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e != hipSuccess) return fail_hip(e, "graph cache add");          // (a new generation is dropped: the cache is as it was)
    std::unique_lock<std::shared_mutex> lk(st.mu);
    st.dev = dc.id;
    if (grow) { st.gen = gen; ++st.generations; }
    for (int64_t g = 0; g < G; ++g) {
        UgsSlot &s = fresh[(size_t)g];
        s.rbase += st.used_r; s.vbase += st.used_v; s.viable_base += st.used_w;
        s.col0 = st.used_c + cptr[(size_t)g];
        slots_out[g] = (int64_t)st.slots.size();
        st.slots.push_back(s);
    }
    st.used_r = need_r; st.used_a = need_a; st.used_v = need_v; st.used_w = need_w; st.used_c = need_c;
    return UGS_OK;
}

int ugs_graph_cache_sample_begin(ugs_graph_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                                 const int64_t *ptr, int64_t num_graphs, int m_per_graph, int mode, int seed, const int32_t *seeds, int check,
                                 ugs_job **job_out, int64_t *total_edges_out) {
    if (!cache || !job_out || !ptr) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !slots) return fail(UGS_E_BAD_ARG, "graph cache sample needs one slot per graph");
    if (check && (num_cols < 0 || (num_cols > 0 && !edge_index))) return fail(UGS_E_BAD_ARG, "the check needs the batch's edge_index");
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (num_graphs >= (int64_t)0x7f7f7f7f) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 0x7f7f7f7f");   // (first_bad starts there)
    const std::shared_ptr<UgsCacheState> stp = cache->st;
    UgsCacheState &st = *stp;
    const int64_t G = num_graphs;
    const int k = st.k;
    const bool checked = check != 0, have_cols = edge_index != nullptr;
    // O(G): one descriptor per graph from its slot, the prefix sums of the column counts, and what choose_tier reads
    std::vector<UgsGraphDesc> gd((size_t)G);
    std::vector<int64_t> coff((size_t)G + 1, 0), col0((size_t)G, 0);
    ugs_plan *plan = new ugs_plan();
    plan->view = true;
    plan->prow_failed = true;                                            // no padded rows for the store: 64-lane tiers read rows through rowptr
    struct Unref { ugs_plan *p; ~Unref() { plan_unref(p); } } unref{plan};   // (begin_common takes the reference over: p is cleared before)
    plan->g_n.resize((size_t)G); plan->g_maxdeg.resize((size_t)G); plan->g_sbdeg.resize((size_t)G); plan->g_level.resize((size_t)G);
    std::shared_ptr<UgsGen> gen;
    int cache_dev = -1;
    {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        gen = st.gen;
        cache_dev = st.dev;
        for (int64_t g = 0; g < G; ++g) {
            if (slots[g] < 0 || slots[g] >= (int64_t)st.slots.size()) return fail(UGS_E_BAD_ARG, "unknown graph cache slot " + std::to_string(slots[g]));
            const UgsSlot &s = st.slots[(size_t)slots[g]];
            const int64_t n = ptr[g + 1] - ptr[g];
            if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
            if (n != s.n)
                return fail(UGS_E_BAD_ARG, "ugs_sampler cache: graph " + std::to_string(g) + " of the batch has " + std::to_string(n) +
                                               " vertices, the graph added in its place has " + std::to_string(s.n));
            UgsGraphDesc &d = gd[(size_t)g];
            const bool live = s.level >= 0;
            d.node_lo = ptr[g]; d.rbase = s.rbase; d.vbase = s.vbase; d.viable_base = s.viable_base;
            d.n = live ? (int32_t)s.n : 0; d.level = s.level; d.n_viable = s.n_viable; d.pad = 0;
            plan->g_n[(size_t)g] = live ? s.n : 0; plan->g_maxdeg[(size_t)g] = s.max_deg; plan->g_sbdeg[(size_t)g] = s.sb_deg; plan->g_level[(size_t)g] = s.level;
            plan->nverts += live ? s.n : 0; plan->nnz += s.nnz;
            coff[(size_t)g + 1] = coff[(size_t)g] + s.cols;
            col0[(size_t)g] = s.col0;
        }
    }
    const int64_t E = coff[(size_t)G];
    if ((checked || have_cols) && num_cols != E)
        return fail(UGS_E_BAD_ARG, "ugs_sampler cache: the batch has " + std::to_string(num_cols) + " columns, the added graphs have " + std::to_string(E));
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (cache_dev >= 0 && cache_dev != dc.id)
        return fail(UGS_E_BAD_ARG, "the graph cache lives on device " + std::to_string(cache_dev) + ", this call runs on device " + std::to_string(dc.id));
    HIP_TRY(hipSetDevice(dc.id));
    const int64_t rows = G * (int64_t)m_per_graph;
    const bool run_check = checked && E > 0 && gen;
    const int64_t Ec = run_check ? E : 0;                                // columns that go up: none without the check
    // the view plan's blob: descriptors, coff and (check) ptr, col0 and the batch's columns go up in one copy; first_bad behind them
    BlobLayout L;
    const size_t o_desc = L.take((size_t)G * sizeof(UgsGraphDesc)), o_coff = L.take((size_t)(G + 1) * 8), o_lo = L.take(run_check ? (size_t)G * 8 : 0),
                 o_col0 = L.take(run_check ? (size_t)G * 8 : 0), o_src = L.take((size_t)Ec * 8), o_dst = L.take((size_t)Ec * 8);
    L.end_inputs();
    const size_t o_bad = L.take(8);
    std::vector<char> host(L.in_bytes, 0);
    if (G > 0) std::memcpy(host.data() + o_desc, gd.data(), (size_t)G * sizeof(UgsGraphDesc));
    std::memcpy(host.data() + o_coff, coff.data(), (size_t)(G + 1) * 8);
    if (run_check) {
        std::memcpy(host.data() + o_lo, ptr, (size_t)G * 8);
        std::memcpy(host.data() + o_col0, col0.data(), (size_t)G * 8);
        std::memcpy(host.data() + o_src, edge_index, (size_t)Ec * 8);
        std::memcpy(host.data() + o_dst, edge_index + row_stride, (size_t)Ec * 8);
    }
    if (int rc = pool_get(L.off, dc.id, plan->blob_buf)) return rc;
    char *b = static_cast<char *>(plan->blob_buf.p);
    plan->device = dc.id; plan->cus = dc.cus; plan->G = G;
    plan->blob = b; plan->blob_bytes = L.off;
    plan->dev.graphs = reinterpret_cast<const UgsGraphDesc *>(b + o_desc);
    if (gen) {
        plan->dev.rowptr = gen->rowptr; plan->dev.adj = gen->adj; plan->dev.adjf = gen->adjf; plan->dev.roots = gen->roots; plan->dev.viable = gen->viable;
        plan->keep.push_back(gen);                                       // an add that regrows the store leaves this job its buffers
    }
    plan->dev.num_graphs = G;
    const int64_t *d_coff = reinterpret_cast<const int64_t *>(b + o_coff);
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
        q.src = reinterpret_cast<const int64_t *>(b + o_src); q.dst = reinterpret_cast<const int64_t *>(b + o_dst);
        q.lo = reinterpret_cast<const int64_t *>(b + o_lo); q.coff = d_coff; q.col0 = reinterpret_cast<const int64_t *>(b + o_col0);
        q.cols = gen->cols; q.first_bad = d_bad;
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
        if ((int64_t)bad < G) {
            (void)hipStreamSynchronize(dc.stream);
            free_job(j);
            return fail(UGS_E_BAD_ARG, "ugs_sampler cache: graph " + std::to_string(bad) + " of the batch differs from the graph added in its place");
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
