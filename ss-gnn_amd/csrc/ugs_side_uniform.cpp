// ugs_side_uniform.cpp -- host side of uniform_sampler in libugs_mi355.so: the vertex limits, uniform_begin (sample_batch,
// sample_graphs, sample_distinct, count_graphs and enumerate_graphs are its modes) over the kernels of ugs_uniform.hip, and
// PopulationCache with its WL class indices (ugs_wl.hip): every graph enumerated once, sample calls served from the stored keys.
//
// Behavioural contract: the reference `uniform_sampler`
// (AniruddhaMandal/SS-GNN src/samplers/uniform_sampler/src/uniform_sampler.cpp); the laws of the entries the reference does not have
// are stated in include/ugs_mi355.h.  The job it hands out and the pieces its begins are built from are the job path's (ugs_jobs.cpp;
// ugs_host_internal.h).
#include "ugs_host_internal.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

using namespace ugs_host;

extern "C" {

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
// UNI_CENSUS (ugs_graphlet_census): UNI_COUNT with the census pass in the count pass's place; `census` names the tables and the
// device counts, counts_out may be null.
// UNI_VCENSUS (ugs_graphlet_vertex_census): UNI_CENSUS with the vertex census pass; `vcensus` names the tables and the device rows,
// its N is set here, ptr[G], once ptr is known to be sound.
enum { UNI_SAMPLE = 0, UNI_ENUMERATE, UNI_COUNT, UNI_POPULATE, UNI_DISTINCT, UNI_CENSUS, UNI_VCENSUS };
using UniPopulate = std::function<int(const UgsUniCall &c, const UgsUniWide &w, const std::vector<UgsUniGraph> &gd, const std::vector<int64_t> &gsize,
                                      const int32_t *graph_status, const DeviceCtx &dc)>;
static int uniform_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                         int m_per_graph, int k, int mode, uint64_t seed, const uint64_t *seeds, int32_t *graph_status,
                         ugs_job **job_out, int64_t *total_edges_out, int what = UNI_SAMPLE, int64_t cap = UGS_UNI_BUDGET,
                         int64_t *rows_out = nullptr, int64_t *counts_out = nullptr, const UniPopulate *populate = nullptr,
                         int64_t *valid_out = nullptr, const UgsCensus *census = nullptr, const UgsVertexCensus *vcensus = nullptr) {
    if ((!job_out && what != UNI_COUNT && what != UNI_POPULATE && what != UNI_CENSUS && what != UNI_VCENSUS) || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index))
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
    const bool sampling = what == UNI_SAMPLE || what == UNI_DISTINCT, counting = what == UNI_COUNT || what == UNI_CENSUS || what == UNI_VCENSUS;
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
        UgsVertexCensus vz{};
        if (what == UNI_VCENSUS) { vz = *vcensus; vz.N = ptr[G]; }      // scan_ptr: non-decreasing, and the entry refused ptr[0] < 0
        if (e == hipSuccess)
            e = what == UNI_CENSUS    ? ugs_uniform_census(c, w, *census, dc.stream)
                : what == UNI_VCENSUS ? ugs_uniform_vertex_census(c, w, vz, dc.stream)
                : counting            ? ugs_uniform_count(c, w, dc.stream)
                                      : ugs_uniform_enum_keys(c, w, dc.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(status, c.status, sizeof(status), hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess && !gcount.empty()) e = hipMemcpyAsync(gcount.data(), c.gcount, (size_t)G * 8, hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess && !gsize.empty()) e = hipMemcpyAsync(gsize.data(), c.gsize, (size_t)G * 8, hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
        if (e != hipSuccess) return bail(fail_hip(e, "uniform_sampler pipeline"));
        for (int64_t g = 0; g < G; ++g) {
            const bool past = !gcount.empty() && gd[(size_t)g].enumerable && gcount[(size_t)g] > budget;
            graph_status[g] = too_big[(size_t)g] ? 1 : past ? 2 : 0;
            if (counting && counts_out) counts_out[g] = graph_status[g] ? -1 : gcount.empty() ? 0 : gcount[(size_t)g];
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

// ---- ugs_sampler.graphlets.census: the exact k-graphlet histogram of every graph, no set stored (the law is stated in include/ugs_mi355.h) ----
int ugs_graphlet_census(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int k,
                        int64_t limit, const int64_t *d_keys, int64_t num_keys, const uint16_t *d_code_col, int64_t *d_counts_out,
                        int32_t *graph_status) {
    if (k < 1 || k > 8) return fail(UGS_E_UNSUPPORTED, "graphlet_census: 1 <= k <= 8");
    if (limit < 1 || limit > ((int64_t)1 << 32)) return fail(UGS_E_BAD_ARG, "limit must be 1 ... 2^32 (got " + std::to_string(limit) + ")");
    if (!d_keys || num_keys < 1 || num_keys >= 0xFFFF) return fail(UGS_E_BAD_ARG, "graphlet_census needs the keys of its columns, 1 ... 65534 of them");
    if ((k < 8) != (d_code_col != nullptr)) return fail(UGS_E_BAD_ARG, "graphlet_census takes the code table for k <= 7 and none for k = 8");
    if (num_graphs > 0 && (!d_counts_out || !graph_status)) return fail(UGS_E_BAD_ARG, "graphlet_census needs counts_out and graph_status");
    UgsCensus z{};
    z.code_col = d_code_col; z.keys = d_keys; z.W = num_keys; z.counts = reinterpret_cast<unsigned long long *>(d_counts_out);
    return uniform_begin(edge_index, row_stride, num_cols, ptr, num_graphs, 0, k, 0, 0, nullptr, graph_status, nullptr, nullptr, UNI_CENSUS, limit,
                         nullptr, nullptr, nullptr, nullptr, &z);
}

// ---- ugs_sampler.graphlets.vertex_census: the exact k-graphlet degree vector of every vertex, no set stored (the law is stated in
//      include/ugs_mi355.h) ----
int ugs_graphlet_vertex_census(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs, int k,
                               int64_t limit, int64_t num_keys, const int64_t *d_obase, int64_t num_orbits, const uint32_t *d_table,
                               int64_t *d_gdv_out, int32_t *graph_status) {
    if (k < 1 || k > 7)
        return fail(UGS_E_UNSUPPORTED, "graphlet_vertex_census: 1 <= k <= 7 (k = 8 would be 72 489 columns a vertex and a canonical search a set)");
    if (limit < 1 || limit > ((int64_t)1 << 32)) return fail(UGS_E_BAD_ARG, "limit must be 1 ... 2^32 (got " + std::to_string(limit) + ")");
    if (!d_obase || !d_table || num_keys < 1 || num_keys > 1024 || num_orbits < num_keys || num_orbits > 7 * num_keys)
        return fail(UGS_E_BAD_ARG, "graphlet_vertex_census needs the orbit bases of its classes (1 ... 1024 of them), the number of columns and the table");
    if (num_graphs > 0 && !graph_status) return fail(UGS_E_BAD_ARG, "graphlet_vertex_census needs graph_status");
    if (ptr && num_graphs >= 0 && ptr[0] < 0) return fail(UGS_E_BAD_ARG, "ptr[0] must be >= 0");
    if (ptr && num_graphs >= 0 && ptr[num_graphs] > 0 && !d_gdv_out) return fail(UGS_E_BAD_ARG, "graphlet_vertex_census needs gdv_out");
    UgsVertexCensus z{};
    z.table = d_table; z.obase = d_obase; z.W = num_keys; z.O = num_orbits; z.gdv = reinterpret_cast<unsigned long long *>(d_gdv_out);
    return uniform_begin(edge_index, row_stride, num_cols, ptr, num_graphs, 0, k, 0, 0, nullptr, graph_status, nullptr, nullptr, UNI_VCENSUS, limit,
                         nullptr, nullptr, nullptr, nullptr, nullptr, &z);
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

}  // extern "C"
