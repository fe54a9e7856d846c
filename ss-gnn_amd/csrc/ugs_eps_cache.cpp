// ugs_eps_cache.cpp -- host side of epsilon_uniform_sampler.GraphCache in libugs_mi355.so: the adjacency lists of every dataset graph
// built once, on the device (ugs_eps_build in ugs_eps.hip), and kept there as one "batch of all added graphs"; a cached call over any
// batch of added graphs builds one descriptor per graph, O(G) on the host, and runs the walk, scan and fill kernels of the uncached
// call on them.  The adjacency depends on neither k nor epsilon, so both are arguments of the call and one cache serves every value.
//
// Behavioural contract: ugs_eps_sample_batch_begin / ugs_eps_sample_graphs_begin (ugs_side_eps.cpp) on the collated batch; the law is
// stated in include/ugs_mi355.h at ugs_eps_cache_sample_begin.  The job and the pieces the begin is built from are the job path's
// (ugs_jobs.cpp; ugs_host_internal.h); the check is ugs_store_check of ugs_store.hip.  Layout, the build kernel
// and generations: DESIGN.md section 16.  Modelled on the rwr cache in ugs_side_rwr.cpp and on ugs_graph_cache.cpp.
#include "ugs_host_internal.h"

#include <algorithm>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

using namespace ugs_host;

namespace {
// What the host keeps of an added graph: its place in the store.
struct EpsSlot {
    int64_t n = 0, cols = 0;                  // vertices as added, columns
    int64_t rbase = 0, abase = 0, col0 = 0;   // first rowptr entry, first nbr / ecs entry, first stored column
};
// One generation of the storage.  Growth makes a new one and copies; a job's fill hook holds the one it walked on.
struct EpsGen {
    int64_t *rowptr = nullptr;
    int32_t *nbr = nullptr, *ecs = nullptr;
    int2 *cols = nullptr;
    int64_t cap_r = 0, cap_h = 0, cap_c = 0;  // entries of rowptr, of nbr / ecs, of cols
    ~EpsGen() { (void)hipFree(rowptr); (void)hipFree(nbr); (void)hipFree(ecs); (void)hipFree(cols); }
    int64_t bytes() const { return cap_r * 8 + cap_h * 8 + cap_c * 8; }
    int alloc(int64_t r, int64_t h, int64_t c) {
        cap_r = std::max<int64_t>(r, 1); cap_h = std::max<int64_t>(h, 1); cap_c = std::max<int64_t>(c, 1);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&rowptr), (size_t)cap_r * 8));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&nbr), (size_t)cap_h * 4));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ecs), (size_t)cap_h * 4));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cols), (size_t)cap_c * 8));
        return UGS_OK;
    }
};
struct EpsCacheState {
    int dev = -1;
    int64_t reserve_v = 0, reserve_c = 0;
    std::mutex add_mu;                        // adds, one at a time, from the build to the publication
    std::shared_mutex mu;                     // what a sample begin reads: slots and gen (exclusive only to publish an add)
    std::deque<EpsSlot> slots;
    std::shared_ptr<EpsGen> gen;
    int64_t used_r = 0, used_h = 0, used_c = 0, generations = 0;
};
}  // namespace
struct ugs_eps_cache { std::shared_ptr<EpsCacheState> st; };

extern "C" {

int ugs_eps_cache_create(int64_t reserve_vertices, int64_t reserve_columns, ugs_eps_cache **cache_out) {
    if (!cache_out) return fail(UGS_E_BAD_ARG, "cache_out is null");
    if (reserve_vertices < 0 || reserve_vertices >= (int64_t)INT32_MAX || reserve_columns < 0 || reserve_columns >= ((int64_t)1 << 30))
        return fail(UGS_E_BAD_ARG, "reserve must be 0 ... 2^31 - 2 vertices and 0 ... 2^30 - 1 columns");
    auto *c = new ugs_eps_cache();
    c->st = std::make_shared<EpsCacheState>();
    c->st->reserve_v = reserve_vertices; c->st->reserve_c = reserve_columns;
    *cache_out = c;
    return UGS_OK;
}

int ugs_eps_cache_destroy(ugs_eps_cache *cache) {
    delete cache;                                                        // a generation goes with the last job that walked on it
    return UGS_OK;
}

int ugs_eps_cache_info(ugs_eps_cache *cache, int64_t *graphs_out, int64_t *vertices_out, int64_t *half_edges_out, int64_t *bytes_out,
                       int64_t *generations_out) {
    if (!cache) return fail(UGS_E_BAD_ARG, "cache is null");
    EpsCacheState &st = *cache->st;
    std::shared_lock<std::shared_mutex> lk(st.mu);
    if (graphs_out) *graphs_out = (int64_t)st.slots.size();
    if (vertices_out) *vertices_out = st.used_r;
    if (half_edges_out) *half_edges_out = st.used_h;
    if (bytes_out) *bytes_out = st.gen ? st.gen->bytes() : 0;
    if (generations_out) *generations_out = st.generations;
    return UGS_OK;
}

int ugs_eps_cache_add(ugs_eps_cache *cache, const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr,
                      int64_t num_graphs, int64_t *slots_out) {
    if (!cache || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to eps cache add");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !slots_out) return fail(UGS_E_BAD_ARG, "eps cache add needs slots_out");
    if (num_cols >= ((int64_t)1 << 30)) return fail(UGS_E_UNSUPPORTED, "add too large: columns must be < 2^30");
    EpsCacheState &st = *cache->st;
    const int64_t G = num_graphs, E = num_cols;
    if (G == 0) {
        if (E > 0) return fail(UGS_E_BAD_ARG, "eps cache add: columns without a graph");
        return UGS_OK;
    }
    // Columns must come graph by graph, in the order of the graphs, both endpoints inside the graph: that order is what a batch is
    // compared with, and a column that left its graph could fall into a neighbour's range once the graph stands in a batch.
    std::vector<EpsSlot> fresh((size_t)G);
    std::vector<int64_t> vptr((size_t)G + 1, 0), cptr((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = ptr[g + 1] - ptr[g];
        if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
        if (n >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "graph too large");       // (eps_begin's text)
        fresh[(size_t)g].n = n;
        vptr[(size_t)g + 1] = vptr[(size_t)g] + n;
    }
    const int64_t NV = vptr[(size_t)G], n_rows = NV + G;
    if (n_rows >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "add too large: vertices plus graphs must be < 2^31 - 1");
    std::vector<int2> local((size_t)E);                                  // the add's columns as the store keeps them: pairs of local ids
    {
        int64_t g = 0;
        for (int64_t x = 0; x < E; ++x) {
            const int64_t u = edge_index[x], v = edge_index[row_stride + x];
            while (g < G && !(ptr[g] <= u && u < ptr[g + 1])) ++g;
            if (g >= G || !(ptr[g] <= v && v < ptr[g + 1]))
                return fail(UGS_E_BAD_ARG, "eps cache add: column " + std::to_string(x) + " is not inside one graph, or the columns are not in the order of the graphs");
            ++fresh[(size_t)g].cols;
            local[(size_t)x] = make_int2((int32_t)(u - ptr[g]), (int32_t)(v - ptr[g]));
        }
    }
    for (int64_t g = 0; g < G; ++g) cptr[(size_t)g + 1] = cptr[(size_t)g] + fresh[(size_t)g].cols;
    std::lock_guard<std::mutex> add_lk(st.add_mu);                       // (only adds write used_* and gen: reading them here needs no more)
    if (st.used_h + 2 * E >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "eps cache: the half-edges of all added graphs must stay below 2^31");
    if (st.used_r + n_rows >= (int64_t)INT32_MAX)
        return fail(UGS_E_UNSUPPORTED, "eps cache: vertices plus graphs of all adds must stay below 2^31");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (st.dev >= 0 && st.dev != dc.id)
        return fail(UGS_E_BAD_ARG, "the eps cache lives on device " + std::to_string(st.dev) + ", this add runs on device " + std::to_string(dc.id));
    HIP_TRY(hipSetDevice(dc.id));
    // the build's blob: the two prefix arrays (one copy), then one cursor per vertex.  The columns go straight into the store.
    BlobLayout L;
    const size_t o_vptr = L.take((size_t)(G + 1) * 8), o_cptr = L.take((size_t)(G + 1) * 8);
    L.end_inputs();
    const size_t o_cur = L.take((size_t)NV * 4);
    std::vector<char> host(L.in_bytes, 0);
    std::memcpy(host.data() + o_vptr, vptr.data(), (size_t)(G + 1) * 8);
    std::memcpy(host.data() + o_cptr, cptr.data(), (size_t)(G + 1) * 8);
    // room in the store: this generation, or a new one of at least twice the size with everything held so far copied over
    std::shared_ptr<EpsGen> gen = st.gen;
    const int64_t need_r = st.used_r + n_rows, need_h = st.used_h + 2 * E, need_c = st.used_c + E;
    const bool grow = !gen || need_r > gen->cap_r || need_h > gen->cap_h || need_c > gen->cap_c;
    if (grow) {
        auto room = [](int64_t need, int64_t have, int64_t reserve) { return need <= have ? have : std::max({need, 2 * have, reserve}); };
        const std::shared_ptr<EpsGen> old = gen;
        gen = std::make_shared<EpsGen>();
        if (int rc = gen->alloc(room(need_r, old ? old->cap_r : 0, st.reserve_v), room(need_h, old ? old->cap_h : 0, 2 * st.reserve_c),
                                room(need_c, old ? old->cap_c : 0, st.reserve_c))) return rc;
        if (old) {
            if (st.used_r > 0) HIP_TRY(hipMemcpyAsync(gen->rowptr, old->rowptr, (size_t)st.used_r * 8, hipMemcpyDeviceToDevice, dc.stream));
            if (st.used_h > 0) {
                HIP_TRY(hipMemcpyAsync(gen->nbr, old->nbr, (size_t)st.used_h * 4, hipMemcpyDeviceToDevice, dc.stream));
                HIP_TRY(hipMemcpyAsync(gen->ecs, old->ecs, (size_t)st.used_h * 4, hipMemcpyDeviceToDevice, dc.stream));
            }
            if (st.used_c > 0) HIP_TRY(hipMemcpyAsync(gen->cols, old->cols, (size_t)st.used_c * 8, hipMemcpyDeviceToDevice, dc.stream));
        }
    }
    PoolBuf blob;
    if (int rc = pool_get(L.off, dc.id, blob)) return rc;
    char *b = static_cast<char *>(blob.p);
    UgsEpsBuild w{};
    w.G = G;
    w.vptr = reinterpret_cast<const int64_t *>(b + o_vptr); w.cptr = reinterpret_cast<const int64_t *>(b + o_cptr);
    w.cursor = reinterpret_cast<int32_t *>(b + o_cur);
    w.rowptr = gen->rowptr; w.nbr = gen->nbr; w.ecs = gen->ecs; w.cols = gen->cols;
    w.row_base = st.used_r; w.adj_base = st.used_h; w.col_base = st.used_c;
    // (beyond what is published nothing reads: the columns land in the store, the kernel reads them there and writes behind used_*)
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess && E > 0) e = hipMemcpyAsync(gen->cols + st.used_c, local.data(), (size_t)E * 8, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess) e = ugs_eps_build(w, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    pool_put(blob);
    if (e != hipSuccess) return fail_hip(e, "epsilon_uniform_sampler cache add");   // (a new generation is dropped: the cache is as it was)
    std::unique_lock<std::shared_mutex> lk(st.mu);
    st.dev = dc.id;
    if (grow) { st.gen = gen; ++st.generations; }
    for (int64_t g = 0; g < G; ++g) {
        EpsSlot &s = fresh[(size_t)g];
        s.rbase = st.used_r + vptr[(size_t)g] + g;
        s.abase = st.used_h + 2 * cptr[(size_t)g];
        s.col0 = st.used_c + cptr[(size_t)g];
        slots_out[g] = (int64_t)st.slots.size();
        st.slots.push_back(s);
    }
    st.used_r = need_r; st.used_h = need_h; st.used_c = need_c;
    return UGS_OK;
}

int ugs_eps_cache_graph_csr(ugs_eps_cache *cache, int64_t slot, int64_t node_capacity, int64_t entry_capacity, int64_t *num_nodes,
                            int64_t *num_entries, int64_t *rowptr, int32_t *nbr, int32_t *ecs) {
    if (!cache) return fail(UGS_E_BAD_ARG, "cache is null");
    EpsCacheState &st = *cache->st;
    EpsSlot s;
    std::shared_ptr<EpsGen> gen;
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
        HIP_TRY(hipMemcpy(rowptr, gen->rowptr + s.rbase, (size_t)(s.n + 1) * 8, hipMemcpyDeviceToHost));
        for (int64_t r = 0; r <= s.n; ++r) rowptr[r] -= s.abase;
    }
    if (nbr && nnz > 0) HIP_TRY(hipMemcpy(nbr, gen->nbr + s.abase, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    if (ecs && nnz > 0) HIP_TRY(hipMemcpy(ecs, gen->ecs + s.abase, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    return UGS_OK;
}

int ugs_eps_cache_sample_begin(ugs_eps_cache *cache, const int64_t *slots, const int64_t *edge_index, int64_t row_stride, int64_t num_cols,
                               const int64_t *ptr, int64_t num_graphs, int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds,
                               double epsilon, int check, int32_t *graph_status, ugs_job **job_out, int64_t *total_edges_out) {
    if (!cache || !job_out || !ptr) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !slots) return fail(UGS_E_BAD_ARG, "eps cache sample needs one slot per graph");
    if (check && (num_cols < 0 || (num_cols > 0 && !edge_index))) return fail(UGS_E_BAD_ARG, "the check needs the batch's edge_index");
    if (!(epsilon > 0.0 && epsilon <= 1.0)) return fail(UGS_E_BAD_ARG, "epsilon must be in (0, 1]");      // (eps_begin's checks and texts)
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (num_graphs >= (int64_t)0x7f7f7f7f) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 0x7f7f7f7f");   // (first_bad starts there)
    const std::shared_ptr<EpsCacheState> stp = cache->st;
    EpsCacheState &st = *stp;
    const int64_t G = num_graphs;
    const bool have_cols = edge_index != nullptr;                        // check == 0 and no edge_index: num_cols says nothing
    const bool checked = check != 0;
    // O(G): one descriptor per graph from its slot and the prefix sums of the column counts
    std::vector<UgsGraphDesc> gd((size_t)G);
    std::vector<int64_t> coff((size_t)G + 1, 0), col0((size_t)G, 0);
    std::shared_ptr<EpsGen> gen;
    int cache_dev = -1;
    {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        gen = st.gen;
        cache_dev = st.dev;
        for (int64_t g = 0; g < G; ++g) {
            if (slots[g] < 0 || slots[g] >= (int64_t)st.slots.size()) return fail(UGS_E_BAD_ARG, "unknown eps cache slot " + std::to_string(slots[g]));
            const EpsSlot &s = st.slots[(size_t)slots[g]];
            const int64_t n = ptr[g + 1] - ptr[g];
            if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
            if (n != s.n)
                return fail(UGS_E_BAD_ARG, "epsilon_uniform_sampler cache: graph " + std::to_string(g) + " of the batch has " + std::to_string(n) +
                                               " vertices, the graph added in its place has " + std::to_string(s.n));
            UgsGraphDesc &d = gd[(size_t)g];
            d.node_lo = ptr[g]; d.rbase = s.rbase; d.vbase = 0; d.viable_base = 0; d.n = (int32_t)s.n; d.level = 0; d.n_viable = 0; d.pad = 0;
            coff[(size_t)g + 1] = coff[(size_t)g] + s.cols;
            col0[(size_t)g] = s.col0;
        }
    }
    const int64_t E = coff[(size_t)G];
    if ((checked || have_cols) && num_cols != E)
        return fail(UGS_E_BAD_ARG, "epsilon_uniform_sampler cache: the batch has " + std::to_string(num_cols) + " columns, the added graphs have " + std::to_string(E));
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    if (cache_dev >= 0 && cache_dev != dc.id)
        return fail(UGS_E_BAD_ARG, "the eps cache lives on device " + std::to_string(cache_dev) + ", this call runs on device " + std::to_string(dc.id));
    const int64_t rows = G * (int64_t)m_per_graph;
    const bool run_check = checked && E > 0 && gen;
    const int64_t Ec = run_check ? E : 0;                                // columns that go up: none without the check
    // one blob: descriptors, coff, seeds and (check) ptr, col0 and the batch's columns go up in one copy; then the walks' scratch.
    // No adjacency arrays.
    BlobLayout L;
    const size_t o_desc = L.take((size_t)G * sizeof(UgsGraphDesc)), o_coff = L.take((size_t)(G + 1) * 8), o_seeds = L.take(seeds ? (size_t)G * 8 : 0),
                 o_lo = L.take(run_check ? (size_t)G * 8 : 0), o_col0 = L.take(run_check ? (size_t)G * 8 : 0), o_src = L.take((size_t)Ec * 8),
                 o_dst = L.take((size_t)Ec * 8);
    L.end_inputs();
    const size_t o_counts = L.take((size_t)rows * sizeof(uint32_t)), o_st = L.take((size_t)ugs_scan_tmp_words(rows) * sizeof(int64_t));
    std::vector<char> host(L.in_bytes, 0);
    if (G > 0) std::memcpy(host.data() + o_desc, gd.data(), (size_t)G * sizeof(UgsGraphDesc));
    std::memcpy(host.data() + o_coff, coff.data(), (size_t)(G + 1) * 8);
    if (seeds && G > 0) std::memcpy(host.data() + o_seeds, seeds, (size_t)G * 8);
    if (run_check) {
        std::memcpy(host.data() + o_lo, ptr, (size_t)G * 8);
        std::memcpy(host.data() + o_col0, col0.data(), (size_t)G * 8);
        std::memcpy(host.data() + o_src, edge_index, (size_t)Ec * 8);
        std::memcpy(host.data() + o_dst, edge_index + row_stride, (size_t)Ec * 8);
    }
    ugs_job *j = nullptr;
    if (int rc = side_job(dc, UGS_JOB_EPS, G, m_per_graph, k, mode, L.off, &j, true)) return rc;
    if (int rc = side_job_rows(j, rows, 8)) return rc;                   // first_bad right behind the edge total: one read-back for both
    char *b = static_cast<char *>(j->blob.p);
    UgsEpsLaunch l{};
    l.graphs = reinterpret_cast<const UgsGraphDesc *>(b + o_desc);
    if (gen) { l.rowptr = gen->rowptr; l.nbr = gen->nbr; l.ecs = gen->ecs; }
    l.num_graphs = G; l.m = m_per_graph; l.k = k; l.mode = mode;
    l.max_attempts = std::max(10, (int)(10.0 / epsilon));
    l.seed = seed; l.seeds = seeds ? reinterpret_cast<const uint64_t *>(b + o_seeds) : nullptr;
    l.epsilon = epsilon; l.rows = rows;
    l.nodes = static_cast<int64_t *>(j->nodes.p); l.counts = reinterpret_cast<uint32_t *>(b + o_counts);
    l.col_base = reinterpret_cast<const int64_t *>(b + o_coff);          // the rows hold columns local to their graph
    int64_t back[2] = {0, 0};                                            // the edge total, and the check's first_bad in the low word behind it
    int32_t *d_bad = reinterpret_cast<int32_t *>(j->d_eptr + rows + 1);
    hipError_t e = hipMemcpyAsync(b, host.data(), L.in_bytes, hipMemcpyHostToDevice, dc.stream);
    if (e == hipSuccess && run_check) e = hipMemsetAsync(d_bad, 0x7f, 8, dc.stream);        // above every g
    if (e == hipSuccess) e = ugs_eps_launch(l, 0, dc.cus, dc.stream);
    if (e == hipSuccess) e = ugs_launch_scan(l.counts, rows, j->d_eptr, reinterpret_cast<int64_t *>(b + o_st), dc.stream);
    if (e == hipSuccess && run_check) {
        UgsStoreCheck q{};
        q.E = Ec; q.G = G;
        q.src = reinterpret_cast<const int64_t *>(b + o_src); q.dst = reinterpret_cast<const int64_t *>(b + o_dst);
        q.lo = reinterpret_cast<const int64_t *>(b + o_lo); q.coff = l.col_base; q.col0 = reinterpret_cast<const int64_t *>(b + o_col0);
        q.cols = gen->cols; q.first_bad = d_bad;
        e = ugs_store_check(q, dc.stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(back, j->d_eptr + rows, run_check ? 16 : 8, hipMemcpyDeviceToHost, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e != hipSuccess) { free_job(j); return fail_hip(e, "epsilon_uniform_sampler cache pipeline"); }
    j->total = back[0];
    if (run_check) {
        const int64_t bad = (int64_t)(int32_t)(back[1] & 0xffffffff);
        if (bad < G) {
            free_job(j);
            return fail(UGS_E_BAD_ARG, "epsilon_uniform_sampler cache: graph " + std::to_string(bad) + " of the batch differs from the graph added in its place");
        }
    }
    if (seeds && graph_status) std::fill(graph_status, graph_status + G, 0);       // no graph of this sampler fails alone
    // the hook holds the generation the walks read: an add that regrows the store leaves this job its buffers
    j->fill = [l, gen, d_eptr = j->d_eptr, cus = dc.cus](int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s) {
        UgsEpsLaunch f = l;
        f.edge_ptr = d_eptr; f.edge_index = edge_index; f.edge_src = edge_src; f.ld = ld;
        return ugs_eps_launch(f, 1, cus, s);
    };
    return hand_out(j, job_out, total_edges_out);
}

}  // extern "C"
