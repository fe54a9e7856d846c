// ugs_rows.cpp -- host side of ugs_sampler.rows.unique_rows (C ABI: ugs_rows_unique_begin / _finish / ugs_rows_last_launch in
// include/ugs_mi355.h, which states the law; kernels: ugs_rows.hip).  A job of the job path: the calling
// thread's device and stream, a blob from the scratch pool, ugs_job_cancel.
#include "ugs_host_internal.h"

#include <cstdio>
#include <string>

using namespace ugs_host;

namespace {
thread_local const char *t_rows_form = "none";

// Turns the status words of a refused call into its message.
int rows_refusal(const UgsRowsBack &b, int bits) {
    if (b.st[UGS_ROWS_ST_PTR] != UGS_ROWS_NONE) {
        const int64_t i = b.st[UGS_ROWS_ST_PTR] >> 2;
        const int which = (int)(b.st[UGS_ROWS_ST_PTR] & 3);
        const char *name = which == 0 ? "sample_ptr" : which == 1 ? "edge_ptr" : "ptr";
        return fail(UGS_E_BAD_ARG, std::string("unique_rows: ") + name + " must start at 0, must not decrease and must end at the number of " +
                                       (which == 0 ? "rows" : which == 1 ? "edge entries" : "vertices") + " (index " + std::to_string(i) + ")");
    }
    if (b.st[UGS_ROWS_ST_GRAPH] != UGS_ROWS_NONE) {
        const int64_t g = b.st[UGS_ROWS_ST_GRAPH] >> 1;
        if ((b.st[UGS_ROWS_ST_GRAPH] & 1) == 0)
            return fail(UGS_E_UNSUPPORTED, "unique_rows: graph " + std::to_string(g) + " has more than " + std::to_string(UGS_ROWS_MAX_PER_GRAPH) + " rows");
        return fail(UGS_E_UNSUPPORTED, "unique_rows: graph " + std::to_string(g) + " has more than " + std::to_string(((int64_t)1 << bits) - 1) +
                                           " vertices, the most a " + std::to_string(bits) + "-bit key field holds at this k");
    }
    return fail(UGS_E_BAD_ARG, "unique_rows: row " + std::to_string(b.st[UGS_ROWS_ST_ENTRY]) + " has an entry below -1 or outside its graph");
}
}  // namespace

extern "C" {

int ugs_rows_unique_begin(const int64_t *d_nodes, int k, int64_t num_rows, const int64_t *d_edge_ptr, int64_t num_edges,
                          const int64_t *d_sample_ptr, int64_t num_graphs, const int64_t *d_ptr, int by, ugs_job **job_out,
                          int64_t *unique_rows_out, int64_t *unique_edges_out) {
    t_rows_form = "none";
    if (!job_out || !unique_rows_out || !unique_edges_out) return fail(UGS_E_BAD_ARG, "unique_rows: null output pointer");
    if (by != 0 && by != 1) return fail(UGS_E_BAD_ARG, "unique_rows: by must be 0 (sequence) or 1 (set)");
    if (k < 1 || k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "unique_rows: 1 <= k <= 32");
    const int64_t R = num_rows, G = num_graphs, Es = num_edges;
    if (R < 0 || G < 0 || Es < 0) return fail(UGS_E_BAD_ARG, "unique_rows: num_rows, num_graphs and num_edges must be >= 0");
    if (R >= ((int64_t)1 << 31) || G >= ((int64_t)1 << 31)) return fail(UGS_E_UNSUPPORTED, "unique_rows: rows and graphs must be < 2^31");
    if (!d_edge_ptr || !d_sample_ptr || !d_ptr || (R > 0 && !d_nodes)) return fail(UGS_E_BAD_ARG, "unique_rows: null input pointer");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;

    auto call = std::make_shared<UgsRowsCall>();
    UgsRowsCall &c = *call;
    c.nodes = d_nodes; c.edge_ptr = d_edge_ptr; c.sample_ptr = d_sample_ptr; c.ptr = d_ptr;
    c.R = R; c.G = G; c.Es = Es; c.k = k; c.by = by; c.bits = std::min(31, 128 / k);
    BlobLayout L;
    const size_t o_status = L.take(UGS_ROWS_ST_WORDS * 8), o_back = L.take(sizeof(UgsRowsBack)), o_nbig = L.take(4 * 4);
    const size_t o_keys = L.take((size_t)R * 16), o_rowg = L.take((size_t)R * 4), o_rep = L.take((size_t)R * 4), o_lrank = L.take((size_t)R * 4);
    const size_t o_cnt = L.take((size_t)R * 4), o_eoff = L.take((size_t)R * 8), o_ug = L.take((size_t)G * 8), o_eg = L.take((size_t)G * 8);
    const size_t o_ubase = L.take((size_t)(G + 1) * 8), o_ebase = L.take((size_t)(G + 1) * 8), o_big = L.take((size_t)G * 3 * 4);

    auto *j = new ugs_job();
    j->dc = dc; j->kind = UGS_JOB_ROWS; j->k = k; j->G = G; j->rows = R;
    if (int rc = pool_get(L.off, dc.id, j->blob)) { free_job(j); return rc; }
    char *base = static_cast<char *>(j->blob.p);
    c.status = reinterpret_cast<int64_t *>(base + o_status); c.back = reinterpret_cast<UgsRowsBack *>(base + o_back);
    c.nbig = reinterpret_cast<int32_t *>(base + o_nbig); c.keys = reinterpret_cast<uint4 *>(base + o_keys);
    c.rowg = reinterpret_cast<int32_t *>(base + o_rowg); c.rep = reinterpret_cast<int32_t *>(base + o_rep);
    c.lrank = reinterpret_cast<int32_t *>(base + o_lrank); c.cnt = reinterpret_cast<int32_t *>(base + o_cnt);
    c.eoff = reinterpret_cast<int64_t *>(base + o_eoff); c.ug = reinterpret_cast<int64_t *>(base + o_ug); c.eg = reinterpret_cast<int64_t *>(base + o_eg);
    c.ubase = reinterpret_cast<int64_t *>(base + o_ubase); c.ebase = reinterpret_cast<int64_t *>(base + o_ebase);
    c.big = reinterpret_cast<int32_t *>(base + o_big);

    UgsRowsBack back{};
    hipError_t e = ugs_rows_dedup(c, dc.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&back, c.back, sizeof(back), hipMemcpyDeviceToHost, dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dc.stream);
    if (e != hipSuccess) { free_job(j); return fail_hip(e, "unique_rows (begin)"); }
    for (int i = 0; i < UGS_ROWS_ST_WORDS - 1; ++i)
        if (back.st[i] != UGS_ROWS_NONE) { free_job(j); return rows_refusal(back, c.bits); }
    t_rows_form = back.big > 0 ? (back.small > 0 ? "wave+workgroup" : "workgroup") : back.small > 0 ? "wave" : "none";
    j->rows_call = call;
    j->rows_kept = back.U;
    j->total = back.Eu;
    *unique_rows_out = back.U;
    return hand_out(j, job_out, unique_edges_out);
}

int ugs_rows_unique_finish(ugs_job *job, int64_t *d_nodes_u, const int64_t *d_edge_index_in, int64_t in_stride, const int64_t *d_edge_src_in,
                           int64_t *d_edge_index_u, int64_t ld, int64_t *d_edge_ptr_u, int64_t *d_sample_ptr_u, int64_t *d_edge_src_u,
                           int64_t *d_count, int64_t *d_inverse) {
    if (!job || job->kind != UGS_JOB_ROWS) return fail(UGS_E_BAD_ARG, "not a unique_rows job");
    const UgsRowsCall &c = *static_cast<const UgsRowsCall *>(job->rows_call.get());
    const int64_t U = job->rows_kept, Eu = job->total;
    auto body = [&]() -> int {
        if (!d_edge_ptr_u || !d_sample_ptr_u || (c.R > 0 && !d_inverse) || (U > 0 && (!d_nodes_u || !d_count)))
            return fail(UGS_E_BAD_ARG, "unique_rows: null output pointer");
        if (Eu > 0 && (!d_edge_index_in || !d_edge_index_u || ld < Eu || in_stride < c.Es))
            return fail(UGS_E_BAD_ARG, "unique_rows: edge_index pointers, in_stride >= the input's edge entries and ld >= the result's are needed");
        if ((d_edge_src_in == nullptr) != (d_edge_src_u == nullptr) && Eu > 0)
            return fail(UGS_E_BAD_ARG, "unique_rows: edge_src goes in and out together, or not at all");
        HIP_TRY(hipSetDevice(job->dc.id));
        UgsRowsOut o{};
        o.edge_index_in = d_edge_index_in; o.in_stride = in_stride; o.edge_src_in = d_edge_src_in;
        o.nodes_u = d_nodes_u; o.edge_index_u = d_edge_index_u; o.edge_ptr_u = d_edge_ptr_u; o.sample_ptr_u = d_sample_ptr_u;
        o.edge_src_u = d_edge_src_in ? d_edge_src_u : nullptr; o.count = d_count; o.inverse = d_inverse; o.ld = ld;
        HIP_TRY(ugs_rows_compact(c, o, U, Eu, job->dc.stream));
        HIP_TRY(hipStreamSynchronize(job->dc.stream));          // the blob goes back to the pool, which knows no streams
        return UGS_OK;
    };
    const int rc = body();
    free_job(job);
    return rc;
}

int ugs_rows_last_launch(char *buf, int buf_len) {
    if (!buf || buf_len <= 0) return fail(UGS_E_BAD_ARG, "null name buffer");
    std::snprintf(buf, (size_t)buf_len, "%s", t_rows_form);
    return UGS_OK;
}

}  // extern "C"
