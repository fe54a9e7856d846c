// ugs_side_rwr.cpp -- host side of rwr_sampler in libugs_mi355.so: rwr_begin (sample_batch, sample_graphs and sample_rows are its
// modes) over the kernels of ugs_rwr.hip, and GraphCache: the dataset's CSRs built once and kept on the device.
//
// Behavioural contract: the reference `rwr_sampler`
// (AniruddhaMandal/SS-GNN src/samplers/rwr_sampler/src/rwr_sampler.cpp, one OpenMP thread); the laws of the entries the reference
// does not have are stated in include/ugs_mi355.h.  The job it hands out and the pieces its begins are built from are the job
// path's (ugs_jobs.cpp; ugs_host_internal.h).
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

extern "C" {

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
