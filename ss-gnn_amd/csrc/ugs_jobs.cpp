// ugs_jobs.cpp -- the job path of libugs_mi355.so: ugs_job, the packed step, begin_common / finish_common, the skeleton every side
// sampler's begin is built from (side_job, side_job_rows, side_job_total), the C ABI of ugs_sample_* /
// ugs_sample_batch_* / ugs_sample_graphs_begin / ugs_job_cancel, and the streamed call with its copy streams and counters.
//
// Behavioural contract: the reference `ugs_sampler`'s sample() (src/sampler.cpp:91-290) and its batch wrapper
// (src/ugs_sampler_batch_extension.cpp:41-299); plans, walks and fills come from ugs_host.cpp through ugs_host_internal.h.
#include "ugs_host_internal.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace ugs_host;

// ---------------------------------------------------------------------------------------------------------------
// jobs: the two-phase host-facing API (begin = walks + counts, finish = fill + copy-out)
// ---------------------------------------------------------------------------------------------------------------
namespace {
std::atomic<int64_t> g_spec_kept{0}, g_spec_wrong{0};              // large calls whose early start stood / was thrown away
std::atomic<int64_t> g_packed_staged{0}, g_packed_refused{0};      // packed steps whose total fitted the staging / that the kernel refused
}  // namespace
namespace ugs_host __attribute__((visibility("hidden"))) {
void free_job(ugs_job *j) {
    if (!j) return;
    pool_put(j->nodes);
    pool_put(j->blob);
    plan_unref(j->plan);
    delete j;
}
int hand_out(ugs_job *j, ugs_job **job_out, int64_t *total_out) {
    *job_out = j;
    if (total_out) *total_out = j->total;
    return UGS_OK;
}
}  // namespace ugs_host

namespace {
// second launch of a job's step (see begin_common): ugs_fill_scan into the job's staging, total through the pinned slot of the plan.
// Call with plan->mu held since the walk whose counts and 8-row sums it scans.
int packed_fill_locked(ugs_job *j, int64_t cap3) {
    ugs_plan *plan = j->plan;
    hipStream_t s = j->dc.stream;
    int64_t *stg = static_cast<int64_t *>(j->nodes.p) + (j->rows * j->k + j->rows + 1);       // (begin_common sized the buffer for it)
    if (int rc = plan_enter(plan, s)) return rc;
    if (!plan->pin_slot) plan->pin_slot = pin_slot_get();
    UgsFillArgs a{};
    a.plan = plan->dev;
    a.m = j->m; a.k = j->k; a.mode = j->mode;
    a.extra_node_off = j->extra;
    a.row_begin = 0; a.row_count = j->rows;
    a.nodes = static_cast<const int64_t *>(j->nodes.p); a.edge_ptr = j->d_eptr; a.edge_ptr_out = j->d_eptr;
    a.edge_index = stg; a.ld = 0; a.edge_src = nullptr;                                       // set by the kernel (packed_cap)
    a.packed_cap = cap3;
    a.counts = static_cast<const uint32_t *>(plan->counts.p);
    a.wsum = static_cast<const uint32_t *>(plan->tiles.p);
    const bool poll = plan->pin_slot != nullptr;
    if (poll) {
        uint32_t ep = g_pin_epoch.fetch_add(1) + 1;
        if (ep == 0) ep = g_pin_epoch.fetch_add(1) + 1;
        plan->pin_epoch = ep;
        a.h_total = reinterpret_cast<int64_t *>(plan->pin_slot); a.h_flag = reinterpret_cast<uint32_t *>(plan->pin_slot + 8); a.epoch = ep;
    }
    HIP_TRY(ev_begin(plan, 2, s));
    HIP_TRY(ugs_launch_fill_scan(a, plan->cus, s, &plan->last_fill));
    HIP_TRY(ev_end(plan, s));
    if (int rc = plan_leave(plan, s)) return rc;
    if (poll) {
        HIP_TRY(wait_signal(reinterpret_cast<volatile uint32_t *>(plan->pin_slot + 8), plan->pin_epoch, s));
        j->total = *reinterpret_cast<volatile int64_t *>(plan->pin_slot);
    } else {
        int64_t tot = 0;
        HIP_TRY(hipMemcpyAsync(&tot, j->d_eptr + j->rows, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        j->total = tot;
    }
    plan->last_overflow = 0;
    j->packed_ok = 3 * j->total <= cap3;
    (j->packed_ok ? g_packed_staged : g_packed_refused).fetch_add(1);
    return UGS_OK;
}
}  // namespace

namespace ugs_host __attribute__((visibility("hidden"))) {
// seeds (ugs_sample_graphs_begin): plan->G per-graph seeds that replace `seed`; nullptr: one seed for the call
int begin_common(ugs_plan *plan, int m, int k, int mode, int64_t extra, int seed, ugs_job **job_out, int64_t *total_out,
                 const int32_t *seeds) {
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) { plan_unref(plan); return rc; }
    auto *j = new ugs_job();
    j->plan = plan; j->dc = dc; j->m = m; j->k = k; j->mode = mode; j->extra = extra;
    j->G = plan->G;
    j->rows = plan->G * (int64_t)m;
    // (a job that may run the packed step keeps its edge staging right behind nodes and edge_ptr: all four outputs leave in ONE copy when
    // the caller's tensors are adjacent too, as the Python shim's are)
    const int64_t node_words = j->rows * k + j->rows + 1;
    const int64_t cap3_want = 3 * j->rows * 2 * (int64_t)k * (int64_t)(k - 1);
    const TierChoice tc0 = choose_tier(plan, k);
    const bool may_pack = k >= 2 && j->rows > 0 && j->rows <= 131072 && tc0.first == UGS_TIER_S && tc0.second < 0 && !tc0.third_G &&
                          cap3_want * (int64_t)sizeof(int64_t) <= ((int64_t)192 << 20) && !debug_on() && std::getenv("UGS_NO_PACKED_STEP") == nullptr;
    const int64_t out_words = node_words + (may_pack ? cap3_want : 0);          // the seed table, if any, lies behind everything finish copies
    const int64_t seed_words = seeds ? plan->G : 0;
    int rc = pool_get((size_t)(out_words + seed_words) * sizeof(int64_t), dc.id, j->nodes);
    const uint64_t *d_seeds = nullptr;
    if (!rc && seed_words > 0) {
        j->seeds.resize((size_t)seed_words);
        for (int64_t g = 0; g < seed_words; ++g) j->seeds[(size_t)g] = (uint64_t)(int64_t)seeds[g];
        uint64_t *d = reinterpret_cast<uint64_t *>(static_cast<int64_t *>(j->nodes.p) + out_words);
        if (hipError_t e = hipMemcpyAsync(d, j->seeds.data(), (size_t)seed_words * sizeof(uint64_t), hipMemcpyHostToDevice, dc.stream); e != hipSuccess)
            rc = fail_hip(e, "hipMemcpyAsync(seeds)");
        d_seeds = d;
    }
    if (!rc) {
        j->d_eptr = static_cast<int64_t *>(j->nodes.p) + j->rows * k;
        // Small batches: every ordered pair of a row's vertices, twice (both directions of a PyG edge are columns, and each column is
        // symmetrised), bounds the edge entries -- if a staging of that size is affordable the step runs here in two launches, the total
        // comes from the fill kernel's first block, and the caller allocates while the rows are being filled.  Repeated columns can
        // exceed the bound: the kernel then writes nothing and finish fills the ordinary way.
        const int64_t cap3 = cap3_want;
        const bool want_packed = may_pack;
        int64_t *d_nodes = static_cast<int64_t *>(j->nodes.p);
        if (want_packed) {                          // (rows > 0) one hold of mu from the walk to the fill that scans its counts and sums
            rc = walk_check(plan, m, k, mode, 0, j->rows, d_nodes, j->d_eptr);
            if (!rc) {
                std::lock_guard<std::mutex> lk(plan->mu);
                bool deferred = false;
                rc = plan_walk_locked(plan, tc0, m, k, mode, extra, seed, nullptr, d_seeds, 0, j->rows, dc.stream, d_nodes, j->d_eptr, &j->total, &deferred, true);
                if (!rc && deferred) rc = packed_fill_locked(j, cap3);
            }
        } else {
            rc = plan_walk_impl(plan, m, k, mode, extra, seed, nullptr, d_seeds, 0, j->rows, dc.stream, d_nodes, j->d_eptr, &j->total, nullptr, true);
        }
    }
    if (rc) { free_job(j); return rc; }
    return hand_out(j, job_out, total_out);
}

int finish_common(ugs_job *j, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr, int64_t *edge_src, int dst_is_device) {
    hipStream_t s = j->dc.stream;
    const int64_t rows = j->rows, k = j->k, tot = j->total;
    int rc = UGS_OK;
    PoolBuf e_idx;                     // host outputs: edge_index [2, tot] and edge_src [tot] staged in ONE device buffer
    auto body = [&]() -> int {
        HIP_TRY(hipSetDevice(j->dc.id));
        int64_t *d_ei = edge_index, *d_es = edge_src;
        const bool packed = j->packed_ok && tot > 0;                // the step already ran (begin_common): copy out of its staging
        if (packed) { d_ei = static_cast<int64_t *>(j->nodes.p) + (rows * k + rows + 1); d_es = d_ei + 2 * tot; }
        else if (!dst_is_device && tot > 0) {
            if (int r = pool_get((size_t)(3 * tot) * sizeof(int64_t), j->dc.id, e_idx)) return r;
            d_ei = static_cast<int64_t *>(e_idx.p); d_es = d_ei + 2 * tot;
        }
        if (tot > 0 && !packed) {                                   // (a side sampler's job is never packed)
            if (!d_ei || !d_es) return fail(UGS_E_BAD_ARG, "null edge output pointer");
            if (j->fill) HIP_TRY(j->fill(d_ei, d_es, tot, s));
            else if (int r = ugs_plan_fill(j->plan, j->m, j->k, j->mode, j->extra, 0, rows, s, static_cast<const int64_t *>(j->nodes.p),
                                           j->d_eptr, d_ei, tot, d_es)) return r;
            if (j->after_fill) HIP_TRY(j->after_fill(d_es, s));
        }
        const hipMemcpyKind kind = dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        // adjacent outputs (the Python shim carves its tensors out of one allocation) travel in one copy each -- or all in one
        if (packed && edge_ptr == nodes + rows * k && edge_index == edge_ptr + rows + 1 && edge_src == edge_index + 2 * tot) {
            // (the same copy through a kernel storing to the pinned tensors was measured: 103 against 96 us for the 2.3 MB of the
            // PROTEINS-shaped call -- the DMA copy stays)
            HIP_TRY(hipMemcpyAsync(nodes, j->nodes.p, (size_t)(rows * k + rows + 1 + 3 * tot) * sizeof(int64_t), kind, s));
        } else {
        if (edge_ptr == nodes + rows * k) {
            HIP_TRY(hipMemcpyAsync(nodes, j->nodes.p, (size_t)(rows * k + rows + 1) * sizeof(int64_t), kind, s));
        } else {
            if (rows * k > 0) HIP_TRY(hipMemcpyAsync(nodes, j->nodes.p, (size_t)(rows * k) * sizeof(int64_t), kind, s));
            HIP_TRY(hipMemcpyAsync(edge_ptr, j->d_eptr, (size_t)(rows + 1) * sizeof(int64_t), kind, s));
        }
        if ((!dst_is_device || packed) && tot > 0) {
            if (!edge_index || !edge_src) return fail(UGS_E_BAD_ARG, "null edge output pointer");
            if (edge_src == edge_index + 2 * tot) {
                HIP_TRY(hipMemcpyAsync(edge_index, d_ei, (size_t)(3 * tot) * sizeof(int64_t), kind, s));
            } else {
                HIP_TRY(hipMemcpyAsync(edge_index, d_ei, (size_t)(2 * tot) * sizeof(int64_t), kind, s));
                HIP_TRY(hipMemcpyAsync(edge_src, d_es, (size_t)tot * sizeof(int64_t), kind, s));
            }
        }
        }
        if (sample_ptr) {
            std::vector<int64_t> sp((size_t)j->G + 1);
            for (int64_t g = 0; g <= j->G; ++g) sp[(size_t)g] = j->sample_ptr.empty() ? g * (int64_t)j->m : j->sample_ptr[(size_t)g];
            if (dst_is_device) HIP_TRY(hipMemcpy(sample_ptr, sp.data(), sp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            else std::memcpy(sample_ptr, sp.data(), sp.size() * sizeof(int64_t));
        }
        HIP_TRY(hipStreamSynchronize(s));
        return UGS_OK;
    };
    rc = body();
    pool_put(e_idx);
    free_job(j);
    return rc;
}

// nodes [rows, k] with edge_ptr [rows + 1] right behind it, and `extra_bytes` of the sampler's own behind both (finish copies none of
// them out).  On failure the job is gone.
int side_job_rows(ugs_job *j, int64_t rows, size_t extra_bytes) {
    j->rows = rows;
    if (int rc = pool_get((size_t)(rows * j->k + rows + 1) * sizeof(int64_t) + extra_bytes, j->dc.id, j->nodes)) { free_job(j); return rc; }
    j->d_eptr = static_cast<int64_t *>(j->nodes.p) + rows * j->k;
    return UGS_OK;
}

// The job of a side sampler: its parameters, its blob, and the G m rows of side_job_rows.  rows_later: the begin learns its row count
// from the device (enumeration) and calls side_job_rows itself, or never has rows (counting).
int side_job(const DeviceCtx &dc, int kind, int64_t G, int m, int k, int mode, size_t blob_bytes, ugs_job **out, bool rows_later) {
    auto *j = new ugs_job();
    j->dc = dc; j->kind = kind; j->m = m; j->k = k; j->mode = mode; j->G = G;
    if (int rc = pool_get(blob_bytes, dc.id, j->blob)) { free_job(j); return rc; }
    if (!rows_later) if (int rc = side_job_rows(j, G * (int64_t)m)) return rc;
    *out = j;
    return UGS_OK;
}

// The end of such a begin.  `e` is the outcome of everything the sampler has queued on the job's stream since side_job (upload, kernels,
// read-backs of its own): the total follows them to the host, the stream is drained, and a HIP error of any of it is reported as
// `what`.  On failure the job is gone.
int side_job_total(ugs_job *j, hipError_t e, const char *what) {
    if (e == hipSuccess) e = hipMemcpyAsync(&j->total, j->d_eptr + j->rows, sizeof(int64_t), hipMemcpyDeviceToHost, j->dc.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(j->dc.stream);
    if (e == hipSuccess) return UGS_OK;
    free_job(j);
    return fail_hip(e, what);
}
}  // namespace ugs_host

extern "C" {

int ugs_sample_begin(int64_t handle, int m_per_graph, int k, int edge_mode, int64_t base_offset, int seed, ugs_job **job_out, int64_t *total_edges_out) {
    if (!job_out) return fail(UGS_E_BAD_ARG, "job_out is null");
    if (edge_mode < 0 || edge_mode > 2) return fail(UGS_E_BAD_MODE, "edge_mode must be one of: 'local', 'flat', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    auto g = lookup(handle);
    if (!g) return fail(UGS_E_INVALID_HANDLE, "Invalid preproc handle");
    if (g->n == 0) return fail(UGS_E_NO_ROOTS, "No viable roots available");
    ugs_plan *plan = nullptr;
    if (int rc = ugs_plan_create_handle(handle, &plan)) return rc;
    return begin_common(plan, m_per_graph, k, edge_mode, edge_mode == UGS_EDGE_GLOBAL ? base_offset : 0, seed, job_out, total_edges_out);
}

int ugs_sample_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *edge_src, int dst_is_device) {
    if (!job) return fail(UGS_E_BAD_ARG, "job is null");
    if (job->kind == UGS_JOB_ROWS) return fail(UGS_E_BAD_ARG, "a unique_rows job is no sampler's: ugs_rows_unique_finish completes it");
    return finish_common(job, nodes, edge_index, edge_ptr, nullptr, edge_src, dst_is_device);
}

int ugs_sample_batch_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                           int m_per_graph, int k, int mode, int seed, ugs_job **job_out, int64_t *total_edges_out) {
    if (!job_out) return fail(UGS_E_BAD_ARG, "job_out is null");
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    ugs_plan *plan = nullptr;
    // Large batches start early, like ugs_sample_batch_stream below: the walks begin on the plan the batch's sampled words point at while
    // the lookup (content hash over every column: ~3 ms for 20 M columns) runs on a helper thread; kept only if it names the same plan.
    ugs_plan *guess = nullptr;
    DeviceCtx dc;
    const int64_t spec_min_cols = [] { const char *e = std::getenv("UGS_SPEC_MIN_COLS"); return e ? (int64_t)std::atoll(e) : (int64_t)1 << 21; }();   // (tests lower it)
    if (num_cols >= spec_min_cols && ptr && edge_index && num_graphs > 0 && m_per_graph > 0 && !debug_on() &&
        std::getenv("UGS_NO_SPECULATION") == nullptr && std::getenv("UGS_NO_BATCH_INDEX") == nullptr && device_ctx(dc) == UGS_OK)
        guess = peek_batch_plan(edge_index, edge_index + row_stride, num_cols, ptr, num_graphs, k, dc.id);
    if (guess) {
        int lookup_rc = UGS_OK;
        std::string lookup_err;
        const int dev_tl = t_device; const hipStream_t st_tl = t_job_stream; const bool set_tl = t_job_stream_set;
        std::thread lookup_thread;
        try {
            lookup_thread = std::thread([&, dev_tl, st_tl, set_tl] {
                t_device = dev_tl >= 0 ? dev_tl : dc.id; t_job_stream = st_tl; t_job_stream_set = set_tl;
                lookup_rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan);
                if (lookup_rc != UGS_OK) lookup_err = t_err;
            });
        } catch (...) { plan_unref(guess); guess = nullptr; }          // no thread to be had: look up first, as without a guess
        if (!guess) {
            if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
            return begin_common(plan, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);
        }
        *job_out = nullptr;
        const int rc = begin_common(guess, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);   // (owns the guess's reference)
        lookup_thread.join();
        if (lookup_rc != UGS_OK) { if (rc == UGS_OK) { free_job(*job_out); *job_out = nullptr; } return fail(lookup_rc, lookup_err); }
        if (plan == guess) { plan_unref(plan); g_spec_kept.fetch_add(1); return rc; }
        if (rc == UGS_OK) { free_job(*job_out); *job_out = nullptr; }                       // a different batch after all: once more, on its plan
        g_spec_wrong.fetch_add(1);
        return begin_common(plan, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);
    }
    if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
    return begin_common(plan, m_per_graph, k, mode, 0, seed, job_out, total_edges_out);
}

// sample_batch with one seed per graph: the same plan lookup (LRU replay, device batch pass) and the same job; the seeds go to the
// device with the job (begin_common).  No early start: presample chunks are far below its threshold.
int ugs_sample_graphs_begin(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                            int m_per_graph, int k, int mode, const int32_t *seeds, ugs_job **job_out, int64_t *total_edges_out) {
    if (!job_out) return fail(UGS_E_BAD_ARG, "job_out is null");
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (num_graphs > 0 && !seeds) return fail(UGS_E_BAD_ARG, "sample_graphs needs one seed per graph");
    ugs_plan *plan = nullptr;
    if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
    return begin_common(plan, m_per_graph, k, mode, 0, 0, job_out, total_edges_out, num_graphs > 0 ? seeds : nullptr);
}

int ugs_sample_batch_finish(ugs_job *job, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr,
                            int64_t *edge_src_global, int dst_is_device) {
    if (!job) return fail(UGS_E_BAD_ARG, "job is null");
    if (job->kind == UGS_JOB_ROWS) return fail(UGS_E_BAD_ARG, "a unique_rows job is no sampler's: ugs_rows_unique_finish completes it");
    return finish_common(job, nodes, edge_index, edge_ptr, sample_ptr, edge_src_global, dst_is_device);
}

int ugs_job_cancel(ugs_job *job) { free_job(job); return UGS_OK; }

// ---- the whole sample_batch call with the copy-out running BESIDE the walks (large host-visible calls) ------------------------------
// The two-phase call is walk (all rows) -> total -> caller allocates -> fill -> copy out: for a million rows the 400 MB of int64
// results cross PCIe for longer than the walks take, one after the other.  Here the caller hands over its buffers up front (edge
// buffers by a capacity it expects, e.g. the previous call's total plus a margin), the rows go through walk / scan / fill in chunks on
// the job stream, and every finished chunk leaves on a second stream while the next one walks.  Row 1 of edge_index [2, total] starts
// at `total`, known with the last chunk only: that half is kept in the device staging and leaves at the end.
namespace {
std::mutex g_copy_mu;
std::map<int, hipStream_t> &g_copy_streams = *new std::map<int, hipStream_t>();
int copy_stream(int dev, hipStream_t &out) {
    std::lock_guard<std::mutex> lk(g_copy_mu);
    auto it = g_copy_streams.find(dev);
    if (it == g_copy_streams.end()) {
        hipStream_t c = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
        it = g_copy_streams.emplace(dev, c).first;
    }
    out = it->second;
    return UGS_OK;
}

// One streamed call: parameters, the caller's (pinned host) buffers, and the device staging that outlives a thrown-away early start.
struct StreamCall {
    DeviceCtx dc;
    int64_t G = 0, extra = 0, cap = 0;
    int m = 0, k = 0, mode = 0, seed = 0;
    int64_t *nodes = nullptr, *edge_index = nullptr, *edge_ptr = nullptr, *sample_ptr = nullptr, *edge_src = nullptr, *total_out = nullptr;
    hipStream_t cs = nullptr;
    PoolBuf d_nodes_b, d_eptr_b, d_loc_b, d_edges_b;
    std::vector<hipEvent_t> evs;
    void release() {
        for (hipEvent_t ev : evs) (void)hipEventDestroy(ev);
        evs.clear();
        pool_put(d_nodes_b); pool_put(d_eptr_b); pool_put(d_loc_b); pool_put(d_edges_b);
    }
};

int stream_rows(ugs_plan *plan, StreamCall &c) {
    const int64_t rows = c.G * (int64_t)c.m, cap = c.cap;
    const int k = c.k;
    int64_t chunk = (rows + 7) / 8;                                   // eight chunks: the first copy starts after an eighth of the walks
    if (chunk < 65536) chunk = 65536;
    if (const char *e = std::getenv("UGS_STREAM_CHUNK_ROWS")) { const int64_t v = std::atoll(e); if (v > 0) chunk = v; }   // (tests: many chunks of a small call)
    const int64_t nchunks = rows > 0 ? (rows + chunk - 1) / chunk : 0;
    hipStream_t s = c.dc.stream;
    int64_t base = 0;
    HIP_TRY(hipSetDevice(c.dc.id));
    if (int rc = copy_stream(c.dc.id, c.cs)) return rc;
    hipStream_t cs = c.cs;
    if (c.sample_ptr) for (int64_t g = 0; g <= c.G; ++g) c.sample_ptr[g] = g * (int64_t)c.m;
    if (rows == 0) { c.edge_ptr[0] = 0; *c.total_out = 0; return UGS_OK; }
    if (!c.d_nodes_b.p) if (int rc = pool_get((size_t)(rows * k) * sizeof(int64_t), c.dc.id, c.d_nodes_b)) return rc;
    if (!c.d_eptr_b.p) if (int rc = pool_get((size_t)(rows + 1) * sizeof(int64_t), c.dc.id, c.d_eptr_b)) return rc;
    if (!c.d_loc_b.p) if (int rc = pool_get((size_t)(chunk + 1) * sizeof(int64_t), c.dc.id, c.d_loc_b)) return rc;
    if (cap > 0 && !c.d_edges_b.p) if (int rc = pool_get((size_t)(3 * cap) * sizeof(int64_t), c.dc.id, c.d_edges_b)) return rc;
    int64_t *d_nodes = static_cast<int64_t *>(c.d_nodes_b.p), *d_eptr = static_cast<int64_t *>(c.d_eptr_b.p), *d_loc = static_cast<int64_t *>(c.d_loc_b.p);
    int64_t *d_ei = static_cast<int64_t *>(c.d_edges_b.p), *d_es = d_ei ? d_ei + 2 * cap : nullptr;
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        const int64_t r0 = ch * chunk, rc_rows = std::min(chunk, rows - r0);
        const bool last = ch + 1 == nchunks;
        int64_t tot = 0;
        if (int rc = plan_walk_impl(plan, c.m, k, c.mode, c.extra, c.seed, nullptr, nullptr, r0, rc_rows, s, d_nodes + r0 * k, d_loc, &tot, nullptr, true)) return rc;
        if (base + tot > cap) { *c.total_out = base + tot; return fail(UGS_E_CAPACITY, "edge_capacity too small for this call's edge entries"); }
        if (tot > 0)
            if (int rc = ugs_plan_fill(plan, c.m, k, c.mode, c.extra, r0, rc_rows, s, d_nodes + r0 * k, d_loc, d_ei + base, cap, d_es + base)) return rc;
        HIP_TRY(ugs_launch_rebase_edge_ptr(d_loc, d_eptr + r0, rc_rows + (last ? 1 : 0), base, s));
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c.evs.push_back(ev);
        HIP_TRY(hipEventRecord(ev, s));
        HIP_TRY(hipStreamWaitEvent(cs, ev, 0));
        HIP_TRY(hipMemcpyAsync(c.nodes + r0 * k, d_nodes + r0 * k, (size_t)(rc_rows * k) * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipMemcpyAsync(c.edge_ptr + r0, d_eptr + r0, (size_t)(rc_rows + (last ? 1 : 0)) * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
        if (tot > 0) {
            HIP_TRY(hipMemcpyAsync(c.edge_index + base, d_ei + base, (size_t)tot * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
            HIP_TRY(hipMemcpyAsync(c.edge_src + base, d_es + base, (size_t)tot * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
        }
        base += tot;
    }
    // row 1 of edge_index: its place in the caller's [2, total] is known now (the last chunk's event orders it behind every fill)
    if (base > 0) HIP_TRY(hipMemcpyAsync(c.edge_index + base, d_ei + cap, (size_t)base * sizeof(int64_t), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    *c.total_out = base;
    return UGS_OK;
}
}  // namespace

int ugs_stream_stats(int64_t *early_starts_kept, int64_t *early_starts_discarded) {
    if (early_starts_kept) *early_starts_kept = g_spec_kept.load();
    if (early_starts_discarded) *early_starts_discarded = g_spec_wrong.load();
    return UGS_OK;
}

int ugs_step_stats(int64_t *packed_staged, int64_t *packed_refused) {
    if (packed_staged) *packed_staged = g_packed_staged.load();
    if (packed_refused) *packed_refused = g_packed_refused.load();
    return UGS_OK;
}

int ugs_sample_batch_stream(const int64_t *edge_index, int64_t row_stride, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                            int m_per_graph, int k, int mode, int seed, int64_t edge_capacity, int64_t *nodes, int64_t *edge_index_out,
                            int64_t *edge_ptr, int64_t *sample_ptr, int64_t *edge_src_global, int64_t *total_edges_out) {
    if (mode < 0 || mode > 2) return fail(UGS_E_BAD_MODE, "mode must be one of: 'sample', 'graph', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    if (edge_capacity < 0 || !edge_ptr || !total_edges_out) return fail(UGS_E_BAD_ARG, "null output pointer or negative edge_capacity");
    if (!ptr || num_graphs < 0 || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    DeviceCtx dc;
    if (int rc = device_ctx(dc)) return rc;
    const int64_t G = num_graphs, rows = G * (int64_t)m_per_graph, cap = edge_capacity;
    if (rows > 0 && (!nodes || (cap > 0 && (!edge_index_out || !edge_src_global)))) return fail(UGS_E_BAD_ARG, "null output pointer");
    // The real lookup reads every column (content hash: ~3 ms for 20 M columns).  A batch whose sampled words match a remembered one
    // starts on that batch's plan at once, the lookup runs beside it on a helper thread, and the results stand only if the lookup
    // returns the same plan; otherwise the streams are drained and the call runs again on the right one.
    ugs_plan *plan = nullptr, *guess = nullptr;
    if (rows > 0 && !debug_on() && std::getenv("UGS_NO_SPECULATION") == nullptr && std::getenv("UGS_NO_BATCH_INDEX") == nullptr)
        guess = peek_batch_plan(edge_index, edge_index + row_stride, num_cols, ptr, G, k, dc.id);
    std::thread lookup_thread;
    int lookup_rc = UGS_OK;
    std::string lookup_err;
    if (guess) {
        const int dev_tl = t_device; const hipStream_t st_tl = t_job_stream; const bool set_tl = t_job_stream_set;
        try {
            lookup_thread = std::thread([&, dev_tl, st_tl, set_tl] {
                t_device = dev_tl >= 0 ? dev_tl : dc.id; t_job_stream = st_tl; t_job_stream_set = set_tl;
                lookup_rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan);
                if (lookup_rc != UGS_OK) lookup_err = t_err;
            });
        } catch (...) { plan_unref(guess); guess = nullptr; }          // no thread to be had: look up first, as without a guess
    }
    if (!guess) if (int rc = ugs_plan_create_batch(edge_index, row_stride, num_cols, ptr, num_graphs, k, &plan)) return rc;
    StreamCall sc;
    sc.dc = dc; sc.G = G; sc.m = m_per_graph; sc.k = k; sc.mode = mode; sc.extra = 0; sc.seed = seed; sc.cap = cap;
    sc.nodes = nodes; sc.edge_index = edge_index_out; sc.edge_ptr = edge_ptr; sc.sample_ptr = sample_ptr; sc.edge_src = edge_src_global;
    sc.total_out = total_edges_out;
    hipStream_t s = dc.stream;
    auto body = [&](ugs_plan *p) { return stream_rows(p, sc); };
    auto drain = [&] { if (sc.cs) (void)hipStreamSynchronize(sc.cs); (void)hipStreamSynchronize(s); };
    int rc = UGS_OK;
    if (guess) {
        std::string guess_err;
        rc = body(guess);
        if (rc != UGS_OK) guess_err = t_err;
        lookup_thread.join();
        if (lookup_rc != UGS_OK) { drain(); rc = fail(lookup_rc, lookup_err); }             // the call's own error (what the two-phase call reports)
        else if (plan != guess) { drain(); g_spec_wrong.fetch_add(1); rc = body(plan); }      // a different batch after all: once more, on its plan
        else if (rc != UGS_OK) rc = fail(rc, guess_err);
        else g_spec_kept.fetch_add(1);
        plan_unref(guess);
    } else rc = body(plan);
    if (rc != UGS_OK) drain();                                      // nothing may still read the pool buffers
    sc.release();
    if (plan) plan_unref(plan);
    return rc;
}

/* sample() of the handle API (reference src/sampler.cpp:91-290) the same way: rows in chunks, copy-out beside the walks. */
int ugs_sample_stream(int64_t handle, int m_per_graph, int k, int edge_mode, int64_t base_offset, int seed, int64_t edge_capacity,
                      int64_t *nodes, int64_t *edge_index_out, int64_t *edge_ptr, int64_t *edge_src, int64_t *total_edges_out) {
    if (edge_mode < 0 || edge_mode > 2) return fail(UGS_E_BAD_MODE, "edge_mode must be one of: 'local', 'flat', 'global'");
    if (m_per_graph < 0) return fail(UGS_E_BAD_ARG, "m_per_graph must be >= 0");
    if (edge_capacity < 0 || !edge_ptr || !total_edges_out) return fail(UGS_E_BAD_ARG, "null output pointer or negative edge_capacity");
    if (m_per_graph > 0 && (!nodes || (edge_capacity > 0 && (!edge_index_out || !edge_src)))) return fail(UGS_E_BAD_ARG, "null output pointer");
    auto g = lookup(handle);
    if (!g) return fail(UGS_E_INVALID_HANDLE, "Invalid preproc handle");
    if (g->n == 0) return fail(UGS_E_NO_ROOTS, "No viable roots available");
    if (k < 1) return fail(UGS_E_BAD_ARG, "k must be >= 1");
    if (k > UGS_KMAX) return fail(UGS_E_UNSUPPORTED, "k > 32 is not supported by the HIP sampler");
    ugs_plan *plan = nullptr;
    if (int rc = ugs_plan_create_handle(handle, &plan)) return rc;
    StreamCall sc;
    if (int rc = device_ctx(sc.dc)) { plan_unref(plan); return rc; }
    sc.G = plan->G; sc.m = m_per_graph; sc.k = k; sc.mode = edge_mode; sc.extra = edge_mode == UGS_EDGE_GLOBAL ? base_offset : 0; sc.seed = seed;
    sc.cap = edge_capacity;
    sc.nodes = nodes; sc.edge_index = edge_index_out; sc.edge_ptr = edge_ptr; sc.sample_ptr = nullptr; sc.edge_src = edge_src;
    sc.total_out = total_edges_out;
    const int rc = stream_rows(plan, sc);
    if (rc != UGS_OK) { if (sc.cs) (void)hipStreamSynchronize(sc.cs); (void)hipStreamSynchronize(sc.dc.stream); }
    sc.release();
    plan_unref(plan);
    return rc;
}

}  // extern "C"
