// ugs_side_eps.cpp -- host side of epsilon_uniform_sampler in libugs_mi355.so: eps_begin, which builds the batch's adjacency lists
// and queues the walks of ugs_eps.hip, and the C ABI of ugs_eps_sample_batch_* / ugs_eps_sample_graphs_begin.
//
// Behavioural contract: the reference `epsilon_uniform_sampler`
// (AniruddhaMandal/SS-GNN src/samplers/epsilon_uniform_sampler/src/epsilon_uniform_sampler.cpp).  The job it hands out and the pieces
// its begin is built from are the job path's (ugs_jobs.cpp; ugs_host_internal.h).
#include "ugs_host_internal.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace ugs_host;

extern "C" {

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

}  // extern "C"
