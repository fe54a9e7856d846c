// ugs_census_csr.cpp -- host side of the CSR form of the graphlet censuses: ugs_graphlet_census_csr and ugs_graphlet_vertex_census_csr in
// include/ugs_mi355.h, which states the law; kernels: ugs_census_csr.hip; DESIGN.md section 19.5.  Argument checks, the call's scratch
// (the graphs' counters and the validation word) from the pool, launches and the two read-backs: nothing else.
#include "ugs_host_internal.h"
#include "ugs_census_csr.h"
#include "ugs_graphlet_common.h"

#include <string>
#include <vector>

namespace {

// the checks both entries share, in the order the header states them: k, limit, the form's limits, then the pointers
int csr_args(const char *name, const int64_t *d_ptr, int64_t G, const int64_t *d_rowptr, const int32_t *d_col, int64_t N, int64_t M, int k,
             int64_t limit, const int32_t *graph_status) {
    const std::string who(name);
    if (k < 1 || k > 8) return fail(UGS_E_UNSUPPORTED, who + ": 1 <= k <= 8");
    if (k == 8) return fail(UGS_E_UNSUPPORTED, who + ": 1 <= k <= 7 in the CSR form (a raw code of 28 bits has no table)");
    if (limit < 1 || limit > ((int64_t)1 << 62)) return fail(UGS_E_BAD_ARG, "limit must be 1 ... 2^62 (got " + std::to_string(limit) + ")");
    if (N >= ((int64_t)1 << 31)) return fail(UGS_E_UNSUPPORTED, who + ": vertices must be < 2^31");
    if (M > (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, who + ": CSR entries must be <= 2^31 - 1");
    if (G >= (int64_t)INT32_MAX) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 2^31 - 1");
    if (G < 0 || N < 0 || M < 0) return fail(UGS_E_BAD_ARG, who + ": negative size");
    if (!d_ptr || !d_rowptr || (M > 0 && !d_col)) return fail(UGS_E_BAD_ARG, who + " needs ptr, rowptr and col");
    if (G > 0 && !graph_status) return fail(UGS_E_BAD_ARG, who + " needs graph_status");
    return UGS_OK;
}

// zero the output, validate, run `pass`, read the graphs' counts back: graph_status[g] = 2 for a graph past the limit; `clear` runs
// only where there is such a graph
template <class Pass, class Clear>
int csr_run(const char *name, UgsCsrCall c, void *d_out, size_t out_bytes, int32_t *graph_status, Pass pass, Clear clear) {
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    PoolBuf scratch;
    const size_t flag_at = align_up((size_t)std::max<int64_t>(c.G, 1) * 8);
    if (int rc = pool_get(flag_at + 8, dc.id, scratch)) return rc;
    c.gcount = static_cast<unsigned long long *>(scratch.p);
    c.flag = reinterpret_cast<int32_t *>(static_cast<char *>(scratch.p) + flag_at);
    int32_t flag = 0;
    std::vector<unsigned long long> gcount((size_t)c.G, 0);
    hipError_t e = hipMemsetAsync(scratch.p, 0, flag_at + 8, dc.stream);
    if (e == hipSuccess && out_bytes > 0) e = hipMemsetAsync(d_out, 0, out_bytes, dc.stream);
    if (e == hipSuccess) e = ugs_census_csr_validate(c, dc.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, c.flag, sizeof(flag), hipMemcpyDeviceToHost, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e == hipSuccess && !flag) {
        e = pass(c, dc.stream);
        if (e == hipSuccess && c.G > 0) e = hipMemcpyAsync(gcount.data(), c.gcount, (size_t)c.G * 8, hipMemcpyDeviceToHost, dc.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
        bool failed = false;
        for (int64_t g = 0; g < c.G; ++g) failed = failed || gcount[(size_t)g] > c.budget;
        if (e == hipSuccess && failed) {
            e = clear(c, dc.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
        }
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(dc.stream);
        pool_put(scratch);
        return fail_hip(e, name);
    }
    pool_put(scratch);
    if (flag)
        return fail(UGS_E_BAD_ARG, std::string(name) + ": ptr must be non-decreasing from ptr[0] >= 0 to the number of vertices, rowptr non-decreasing "
                                   "from 0 to the number of entries, and every row strictly ascending, inside its vertex's graph, without "
                                   "the vertex itself and symmetric");
    for (int64_t g = 0; g < c.G; ++g) graph_status[g] = gcount[(size_t)g] > c.budget ? 2 : 0;
    return UGS_OK;
}

}  // namespace

extern "C" {

int ugs_graphlet_census_csr(const int64_t *d_ptr, int64_t num_graphs, const int64_t *d_rowptr, const int32_t *d_col, int64_t num_vertices,
                            int64_t num_entries, int k, int64_t limit, const int64_t *d_keys, int64_t num_keys, const uint16_t *d_code_col,
                            int64_t *d_counts_out, int32_t *graph_status) {
    if (int rc = csr_args("graphlet_census_csr", d_ptr, num_graphs, d_rowptr, d_col, num_vertices, num_entries, k, limit, graph_status)) return rc;
    if (!d_keys || num_keys < 1 || num_keys >= 0xFFFF || !d_code_col)
        return fail(UGS_E_BAD_ARG, "graphlet_census_csr needs the keys of its columns, 1 ... 65534 of them, and the code table");
    if (num_graphs > 0 && !d_counts_out) return fail(UGS_E_BAD_ARG, "graphlet_census_csr needs counts_out");
    UgsCsrCall c{};
    c.ptr = d_ptr; c.rowptr = d_rowptr; c.col = d_col; c.G = num_graphs; c.N = num_vertices; c.M = num_entries; c.k = k;
    c.budget = (unsigned long long)limit;
    UgsCensus z{};
    z.code_col = d_code_col; z.keys = d_keys; z.W = num_keys; z.counts = reinterpret_cast<unsigned long long *>(d_counts_out);
    return csr_run("graphlet_census_csr", c, d_counts_out, (size_t)num_graphs * (size_t)num_keys * 8, graph_status,
                   [&](const UgsCsrCall &call, hipStream_t s) { return ugs_census_csr_census(call, z, s); },
                   [&](const UgsCsrCall &call, hipStream_t s) { return ugs_census_csr_census_clear(call, z, s); });
}

int ugs_graphlet_vertex_census_csr(const int64_t *d_ptr, int64_t num_graphs, const int64_t *d_rowptr, const int32_t *d_col,
                                   int64_t num_vertices, int64_t num_entries, int k, int64_t limit, int64_t num_keys, const int64_t *d_obase,
                                   int64_t num_orbits, const uint32_t *d_table, int64_t *d_gdv_out, int32_t *graph_status) {
    if (int rc = csr_args("graphlet_vertex_census_csr", d_ptr, num_graphs, d_rowptr, d_col, num_vertices, num_entries, k, limit, graph_status))
        return rc;
    if (!d_obase || !d_table || num_keys < 1 || num_keys > 1024 || num_orbits < num_keys || num_orbits > 7 * num_keys)
        return fail(UGS_E_BAD_ARG, "graphlet_vertex_census_csr needs the orbit bases of its classes (1 ... 1024 of them), the number of columns and the table");
    if (num_vertices > 0 && !d_gdv_out) return fail(UGS_E_BAD_ARG, "graphlet_vertex_census_csr needs gdv_out");
    UgsCsrCall c{};
    c.ptr = d_ptr; c.rowptr = d_rowptr; c.col = d_col; c.G = num_graphs; c.N = num_vertices; c.M = num_entries; c.k = k;
    c.budget = (unsigned long long)limit;
    UgsVertexCensus z{};
    z.table = d_table; z.obase = d_obase; z.W = num_keys; z.O = num_orbits; z.N = num_vertices; z.gdv = reinterpret_cast<unsigned long long *>(d_gdv_out);
    return csr_run("graphlet_vertex_census_csr", c, d_gdv_out, (size_t)num_vertices * (size_t)num_orbits * 8, graph_status,
                   [&](const UgsCsrCall &call, hipStream_t s) { return ugs_census_csr_vertex(call, z, s); },
                   [&](const UgsCsrCall &call, hipStream_t s) { return ugs_census_csr_vertex_clear(call, z, s); });
}

}  // extern "C"
