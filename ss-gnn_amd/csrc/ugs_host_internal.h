// ugs_host_internal.h -- what the host translation units of libugs_mi355.so share: ugs_host.cpp (preprocessing, registry, LRU, plans,
// batch index, device batch pass), ugs_jobs.cpp (the two-phase job path and the streamed call), one ugs_side_<name>.cpp per side
// sampler, ugs_graph_cache.cpp (ugs_sampler.GraphCache) and ugs_eps_cache.cpp (epsilon_uniform_sampler.GraphCache).  Not part of the C ABI (that is include/ugs_mi355.h) and not for the .hip files (they share ugs_device.h).
//
// Declarations only: every global and every thread_local is defined in exactly one .cpp -- ugs_host.cpp, except the job-path section
// at the end, which ugs_jobs.cpp owns.  Everything sits in namespace ugs_host with hidden visibility, so nothing here is exported
// (the block a .cpp defines these in repeats the attribute: a definition does not take it over from its declaration);
// the two opaque types of the C ABI, ugs_plan and ugs_job, stay at global scope.
#pragma once
#include "../../include/ugs_mi355.h"
#include "ugs_device.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

struct ugs_plan;
struct ugs_job;

namespace ugs_host __attribute__((visibility("hidden"))) {

// ---- error reporting: the thread's message (ugs_last_error) and the code that goes with it ----
extern thread_local std::string t_err;
int fail(int code, const std::string &msg);
int fail_hip(hipError_t e, const char *what);
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail_hip(e_, #expr); } while (0)
bool debug_on();
bool env_is_one(const char *name);

// ---- per-graph preprocessing result and the handle registry ----
void plan_unref(ugs_plan *p);
void arena_release(int dev, int64_t roots_off, int64_t n_roots, int64_t via_off, int64_t n_via);
void pin_slot_put(char *p);
struct Graph {
    int64_t n = 0, nnz = 0;
    int k_built = 0;
    std::vector<int64_t> rowptr;      // n+1, 0-based
    std::vector<int32_t> nbr, col;    // CSR neighbours and source column of each entry
    std::vector<int32_t> order, rank; // order[vi] = vertex, rank[vertex] = vi
    std::vector<int32_t> sdeg;        // suffix degree per order position
    std::vector<uint8_t> reach;       // scratch: root reaches k vertices inside its suffix graph
    std::vector<double> weight;       // bucket weight per order position
    std::vector<double> prob;         // alias table (only if Z > 0)
    std::vector<int32_t> alias;
    double Z = 0.0;
    int nonzero = 0;
    int level = 0;                    // relaxation level of the root draw
    std::vector<int32_t> viable;      // order positions for levels 1, 2
    int64_t n_viable = 0;             // their number (a graph preprocessed by the device batch pass has only this)
    // A graph the device batch pass preprocessed (cold path, ugs_bp_roots) exists on the host as a STUB: n, nnz, level, Z, the degree
    // statistics and its root records in a device's arena -- no arrays.  The general path, which has the graph's columns at hand
    // whenever it meets the graph, fills the arrays in then (complete_on_host).
    bool host_ready = true;
    std::vector<int64_t> stub_cols;   // stub: its span of the batch's columns, sources then targets (global ids), and
    int64_t stub_lo = 0;              //       the batch's node offset of the graph -- what completion needs, dropped afterwards
    int64_t max_deg = 0;
    double sb_deg = 0.0;              // size-biased mean CSR degree (sum d^2 / sum d)
    // content fingerprint (graph_fingerprint), set only for graphs of more than 1000 columns: there the LRU key samples the
    // columns, and the device batch pass accepts a cached graph as the one it has just built only if this agrees too
    uint64_t fp_a = 0, fp_b = 0;
    std::mutex plan_mu;
    ugs_plan *plan = nullptr;         // device-resident copy for the handle API, built on first sample()
    std::mutex pre_mu;
    UgsDevPre *devpre = nullptr;      // device CSR left by preprocess_on_device for the FIRST plan assembled from this graph
    int devpre_dev = -1;
    UgsDevPre *take_devpre(int dev) { std::lock_guard<std::mutex> lk(pre_mu); if (!devpre || devpre_dev != dev) return nullptr; UgsDevPre *d = devpre; devpre = nullptr; return d; }
    // root records / viable list of this graph resident in a device's arena (device batch pass: plans of new combinations of
    // known graphs point at them instead of copying them); offsets in elements, -1 = none
    struct DevRoots { int dev; int64_t roots_off, n_roots, via_off, n_via; };
    std::vector<DevRoots> dev_roots;
    ~Graph() {
        if (plan) plan_unref(plan);
        if (devpre) ugs_devpre_free(devpre);
        for (auto &d : dev_roots) arena_release(d.dev, d.roots_off, d.n_roots, d.via_off, d.n_via);
    }
};
std::shared_ptr<Graph> lookup(int64_t h);

// ---- the calling thread's device and stream (ugs_set_device, ugs_set_stream) ----
struct DeviceCtx { int id = -1; int cus = 256; hipStream_t stream = nullptr; };
// Declared constant-initialised, so that the other files read them directly: without it every access first tests the address of the
// variable's init function, which these three do not have -- and in a shared object the address of an absent hidden function does not
// test as null (it is the load address), so the access would call it.  (t_err has an init function, defined next to it.)
#define UGS_TLS_CONST __attribute__((require_constant_initialization))
extern thread_local int t_device UGS_TLS_CONST;
extern thread_local hipStream_t t_job_stream UGS_TLS_CONST;
extern thread_local bool t_job_stream_set UGS_TLS_CONST;
int device_ctx(DeviceCtx &out);

// ---- the grow-only device scratch pool ----
struct PoolBuf { void *p = nullptr; size_t bytes = 0; int dev = -1; bool owned = true; /* false: a piece of a slab, never hipFree'd on its own */ };
int pool_get(size_t bytes, int dev, PoolBuf &out);
void pool_put(PoolBuf &b);
size_t align_up(size_t x, size_t a = 256);

}  // namespace ugs_host
using namespace ugs_host;       // the C-ABI types below, like every host translation unit, name the shared types unqualified

// ---- plans: the opaque type of the C ABI, at global scope with the tier choice it caches ----
struct TierChoice { int first = UGS_TIER_S; int second = -1 /* LDS tier that redoes the rows the first one hands on */; bool third_G = false; int64_t bound = 0;
                    bool small = false /* tier S in its 32-candidate form */; bool wide = false /* tier S may run with 16 lanes per walk */; };

struct ugs_plan {
    int device = -1, cus = 256;
    int64_t G = 0, nverts = 0, nnz = 0;
    void *blob = nullptr;                 // one device allocation holding every array of the plan
    size_t blob_bytes = 0;
    PoolBuf blob_buf;                     // small plans borrow their allocation from the scratch pool
    UgsPlanDev dev{};
    // per-graph statistics used to pick the walk tier for a given k
    std::vector<int64_t> g_n, g_maxdeg;
    std::vector<double> g_sbdeg;
    std::vector<int> g_level;
    std::mutex mu;
    std::map<int, TierChoice> tiers;
    std::atomic<int> refs{1};
    uint64_t cache_key = 0;
    bool cached = false;
    // lazily grown scratch owned by the plan (serialised by `mu` per call)
    // invariant: what a walk leaves here is read only by kernels launched under the same hold of `mu`, or after the stg_* check below
    PoolBuf counts, ovf1, ovf2, ovfcnt, scantmp, gws;
    // edges staged by the last walk (UgsWalkArgs::stage) and the call they belong to: a fill of exactly those rows into/from
    // the same nodes buffer expands them; any other fill reads the adjacency rows again
    PoolBuf stage, ulist, work;   // work: 3 x u64 next-item counters (one per walk launch of a call)
    // scan folded into the fill (ugs_plan_step, ugs_fill_scan): the walk kernel's sums of 8 consecutive rows
    PoolBuf tiles;
    // job path: the scan kernel hands the edge total to the host through 16 bytes of pinned memory (total, epoch word) and the host
    // polls the word instead of copying the total back behind a stream wait (wait_signal)
    char *pin_slot = nullptr;
    uint32_t pin_epoch = 0;
    // stream order between calls: a plan's scratch is reused by every call, so a call on another stream than the previous one
    // first waits (on the device) for that call's last kernel
    hipEvent_t last_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool last_valid = false;
    PoolBuf prow;                         // padded rows (ugs_device.h), built on the device by the first walk in a one-walk-per-wave tier
    std::atomic<size_t> prow_bytes{0};    // their size, readable by the plan cache without this plan's mutex
    bool prow_pooled = false, prow_failed = false;
    size_t prow_asked = 0;                // bytes asked for (rows + table): what ugs_plan_info reports, as blob_bytes is the bytes asked for
    const uint8_t *ord1 = nullptr;        // first-pick table (UgsWalkArgs::ord1): the tail of the padded rows' allocation, 64 bytes per vertex
    int walk_share = 100;                 // ugs_plan_set_walk_share
    bool stg_valid = false;
    const void *stg_nodes = nullptr;
    int64_t stg_row_begin = 0, stg_row_count = 0;
    int stg_m = 0, stg_k = 0;
    int64_t gws_groups = 0, gws_words = 0;
    int gcap = 0, ghs = 0, gbcap = 0, gpcap = 0;
    std::vector<std::shared_ptr<void>> keep;   // device-built plans point into their graphs' arena entries: the graphs live as long as the plan
    ugs_plan *twin_of = nullptr;               // ugs_plan_twin: the plan whose device arrays this one shares (it holds a reference)
    UgsLaunchInfo last_walk{nullptr, 0, 0, 0};
    UgsLaunchInfo last_fill{nullptr, 0, 0, 0};
    int64_t last_overflow = 0;
    bool handle_api = false;
    // optional per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline figure)
    bool timing = false;
    struct EvPair { hipEvent_t a, b; int kind; };     // kind 0 = first-tier walk kernel, 1 = overflow tiers + scan, 2 = fill kernel
    std::vector<EvPair> events;
    // a view plan (ugs_graph_cache.cpp): one cached call's descriptors over the store's arrays, which `keep` holds.  It is never shared
    // and dies with its job, so destroying it waits for its own last kernel (last_ev) instead of the whole device.
    bool view = false;
};

namespace ugs_host __attribute__((visibility("hidden"))) {

// ---- what the job path needs of a plan (all defined in ugs_host.cpp) ----
TierChoice choose_tier(ugs_plan *p, int k);
// ugs_graph_cache.cpp: a graph preprocessed at k that no registry, LRU or batch index learns of, and a chunk of such graphs
// (nullptr: degenerate, n <= 0 or n < k) laid out as one plan -- node_lo 0 and columns local to each graph -- that no cache holds
int graph_outside_lru(const int64_t *src, const int64_t *dst, int64_t E, int64_t n, int k, std::shared_ptr<Graph> &out);
int plan_of_graphs(const std::vector<std::shared_ptr<Graph>> &graphs, const DeviceCtx &dc, ugs_plan *plan);
int plan_enter(ugs_plan *plan, hipStream_t s);
int plan_leave(ugs_plan *plan, hipStream_t s);
hipError_t ev_begin(ugs_plan *p, int kind, hipStream_t s);
hipError_t ev_end(ugs_plan *p, hipStream_t s);
char *pin_slot_get();
hipError_t wait_signal(const volatile uint32_t *word, uint32_t want, hipStream_t s);
extern std::atomic<uint32_t> g_pin_epoch;
ugs_plan *peek_batch_plan(const int64_t *src, const int64_t *dst, int64_t E, const int64_t *ptr, int64_t G, int k, int dev);
void assign_columns(const int64_t *src, const int64_t *dst, int64_t E, const int64_t *ptr, int64_t G,
                    std::vector<int64_t> &cstart, std::vector<int64_t> &cols_of);
int walk_check(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t row_begin, int64_t row_count, const int64_t *d_nodes,
               const int64_t *d_edge_ptr);
int plan_walk_impl(ugs_plan *plan, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed, const uint64_t *d_seed_ptr,
                          const uint64_t *d_seeds, int64_t row_begin, int64_t row_count, void *stream, int64_t *d_nodes, int64_t *d_edge_ptr, int64_t *total_edges_host,
                          bool *defer_scan = nullptr, bool poll_total = false);
int plan_walk_locked(ugs_plan *plan, const TierChoice &tc, int m_per_graph, int k, int mode, int64_t extra_node_offset, int seed,
                            const uint64_t *d_seed_ptr, const uint64_t *d_seeds, int64_t row_begin, int64_t row_count, hipStream_t s, int64_t *d_nodes, int64_t *d_edge_ptr,
                            int64_t *total_edges_host, bool *defer_scan, bool poll_total);

// ---------------------------------------------------------------------------------------------------------------
// The job path (defined in ugs_jobs.cpp) and the contract between it and a side sampler: DESIGN.md section 14.
// A sampler's begin lays its blob out (BlobLayout, BatchInputs, scan_ptr), takes a job (side_job, side_job_rows), queues its work,
// ends with side_job_total and hand_out, and leaves a JobFill for finish_common.
// ---------------------------------------------------------------------------------------------------------------
// What fills a side sampler's edge outputs at finish: edge_index [2, ld] and edge_src [ld] on the device, on the job's stream.
using JobFill = std::function<hipError_t(int64_t *edge_index, int64_t *edge_src, int64_t ld, hipStream_t s)>;
enum { UGS_JOB_UGS = 0, UGS_JOB_EPS, UGS_JOB_UNIFORM, UGS_JOB_RWR, UGS_JOB_UNIFORM_ENUM, UGS_JOB_UNIFORM_POP };

}  // namespace ugs_host

struct ugs_job {
    ugs_plan *plan = nullptr;          // ugs jobs only
    DeviceCtx dc;
    int kind = UGS_JOB_UGS;            // which begin made it: the samplers' own *_finish take no other's job
    int m = 0, k = 0, mode = 0;
    int64_t extra = 0, rows = 0, total = 0, G = 0;
    PoolBuf nodes;                     // nodes [rows, k] and, right behind it, edge_ptr [rows + 1]: one buffer, so that a caller whose
    int64_t *d_eptr = nullptr;         // output tensors are adjacent too gets both with one copy
    // batches of small graphs: begin ran walk + fill as one step (scan folded into the fill) into this staging -- edge_index [2, total]
    // and edge_src [total] laid out for the total the kernel found -- and finish only copies out
    bool packed_ok = false;
    // ugs_sample_graphs_begin: the per-graph seed bases, widened; uploaded on the job's stream to the end of `nodes` (begin_common)
    std::vector<uint64_t> seeds;
    // the side samplers (epsilon_uniform, uniform, rwr): the call's device arrays -- inputs, then the scratch of
    // every stage -- in one pooled blob (hipMalloc/hipFree per call cost milliseconds once the process holds large plans), and the fill
    // that finish runs from them.  The hook holds the sampler's call struct by value; empty: the job fills through its plan.
    PoolBuf blob;
    JobFill fill;
    // a job on a view plan (ugs_graph_cache.cpp): runs behind the plan's own fill at finish, on the job's stream -- edge_src from
    // columns local to each graph to batch columns (a packed step had it at begin)
    std::function<hipError_t(int64_t *edge_src, hipStream_t s)> after_fill;
    // a job whose begin reports its own row count (ugs_uniform_enumerate_begin): its sample_ptr [G + 1], rows = sample_ptr[G];
    // empty: rows = G m and sample_ptr = g m
    std::vector<int64_t> sample_ptr;
};

namespace ugs_host __attribute__((visibility("hidden"))) {

void free_job(ugs_job *j);
int hand_out(ugs_job *j, ugs_job **job_out, int64_t *total_out);
int begin_common(ugs_plan *plan, int m, int k, int mode, int64_t extra, int seed, ugs_job **job_out, int64_t *total_out,
                 const int32_t *seeds = nullptr);
int finish_common(ugs_job *j, int64_t *nodes, int64_t *edge_index, int64_t *edge_ptr, int64_t *sample_ptr, int64_t *edge_src, int dst_is_device);
int side_job_rows(ugs_job *j, int64_t rows, size_t extra_bytes = 0);
int side_job(const DeviceCtx &dc, int kind, int64_t G, int m, int k, int mode, size_t blob_bytes, ugs_job **out, bool rows_later = false);
int side_job_total(ugs_job *j, hipError_t e, const char *what);

// ---- what the begins of the side samplers share (eps_begin, uniform_begin, rwr_begin in ugs_side_*.cpp) ----
// Layout of a job's blob: pieces in the order they are taken, each at a multiple of 256 bytes.  The inputs come first, so that they
// go up in one copy of in_bytes; the scratch of every stage follows.
struct BlobLayout {
    size_t off = 0, in_bytes = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align_up(off + std::max<size_t>(bytes, 8)); return o; }
    void end_inputs() { in_bytes = off; }
};

// The inputs of a sampler that reads the batch itself: both edge rows, ptr, one descriptor per graph and (sample_graphs) the seeds.
struct BatchInputs {
    size_t src, dst, ptr, desc, seeds;
    BatchInputs(BlobLayout &L, int64_t E, int64_t G, size_t desc_bytes, bool per_graph)
        : src(L.take((size_t)E * 8)), dst(L.take((size_t)E * 8)), ptr(L.take((size_t)(G + 1) * 8)), desc(L.take((size_t)G * desc_bytes)),
          seeds(L.take(per_graph ? (size_t)G * 8 : 0)) {}
    void stage(char *host, const int64_t *edge_index, int64_t row_stride, int64_t E, const int64_t *ptr_in, int64_t G, const void *descs,
               size_t desc_bytes, const uint64_t *seeds_in) const {
        for (int64_t e = 0; e < E; ++e) {
            reinterpret_cast<int64_t *>(host + src)[e] = edge_index[e];
            reinterpret_cast<int64_t *>(host + dst)[e] = edge_index[row_stride + e];
        }
        std::memcpy(host + ptr, ptr_in, (size_t)(G + 1) * 8);
        if (G > 0) std::memcpy(host + desc, descs, (size_t)G * desc_bytes);
        if (seeds_in && G > 0) std::memcpy(host + seeds, seeds_in, (size_t)G * 8);
    }
};

// The ptr scan of such a sampler.  ptr must not decrease.  `each(g, n, why)` writes graph g's descriptor and says whether the sampler
// cannot take the graph, leaving the refusal's text in `why`: sample_batch refuses the call with it, sample_graphs lets the graph fail
// alone (too_big[g] = 1: m rows of -1, no draws).
template <class Each>
int scan_ptr(const int64_t *ptr, int64_t G, bool per_graph, std::vector<int32_t> &too_big, Each each) {
    too_big.assign(per_graph ? (size_t)G : 0, 0);
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = ptr[g + 1] - ptr[g];
        if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
        std::string why;
        if (!each(g, n, why)) continue;
        if (!per_graph) return fail(UGS_E_UNSUPPORTED, why);
        too_big[(size_t)g] = 1;
    }
    return UGS_OK;
}

}  // namespace ugs_host
