// ugs_side_rwr.cpp -- host side of rwr_sampler in libugs_mi355.so: rwr_begin (sample_batch, sample_graphs and sample_rows are its
// modes) over the kernels of ugs_rwr.hip.  (rwr_sampler.GraphCache is in ugs_rwr_cache.cpp.)
//
// Behavioural contract: the reference `rwr_sampler`
// (AniruddhaMandal/SS-GNN src/samplers/rwr_sampler/src/rwr_sampler.cpp, one OpenMP thread); the laws of the entries the reference
// does not have are stated in include/ugs_mi355.h.  The job it hands out and the pieces its begins are built from are the job
// path's (ugs_jobs.cpp; ugs_host_internal.h).
#include "ugs_host_internal.h"

#include <algorithm>
#include <cstring>
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

}  // extern "C"
