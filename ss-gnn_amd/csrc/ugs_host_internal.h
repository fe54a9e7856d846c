// ugs_host_internal.h -- what the host translation units of libugs_mi355.so share: ugs_host.cpp (preprocessing, registry, LRU, plans,
// batch index, device batch pass), ugs_jobs.cpp (the two-phase job path and the streamed call), one ugs_side_<name>.cpp per side
// sampler, one file per dataset cache -- ugs_rwr_cache.cpp (rwr_sampler.GraphCache), ugs_graph_cache.cpp (ugs_sampler.GraphCache),
// ugs_eps_cache.cpp (epsilon_uniform_sampler.GraphCache) -- and ugs_cache_common.cpp (what those three share).  Not part of the
// C ABI (that is include/ugs_mi355.h) and not for the .hip files (they share ugs_device.h).
//
// Declarations and templates only: every global and every thread_local is defined in exactly one .cpp -- ugs_host.cpp, except the
// job-path section, which ugs_jobs.cpp owns, and the caches' section at the end, which ugs_cache_common.cpp owns.
// Everything sits in namespace ugs_host with hidden visibility, so nothing here is exported
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
#include <shared_mutex>
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
enum { UGS_JOB_UGS = 0, UGS_JOB_EPS, UGS_JOB_UNIFORM, UGS_JOB_RWR, UGS_JOB_UNIFORM_ENUM, UGS_JOB_UNIFORM_POP, UGS_JOB_ROWS };

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
    // ugs_rows_unique_begin (ugs_rows.cpp): no sampler's job -- the call's arrays (UgsRowsCall over `blob` and the caller's inputs) and
    // the number of kept rows; `rows` is R and `total` is Eu
    std::shared_ptr<void> rows_call;
    int64_t rows_kept = 0;
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

// ---- what the dataset caches share (rwr_sampler, ugs_sampler and epsilon_uniform_sampler GraphCache: ugs_rwr_cache.cpp,
//      ugs_graph_cache.cpp, ugs_eps_cache.cpp; defined in ugs_cache_common.cpp) ----
// A cache's device storage is a short fixed list of arrays, stated as data.  Arrays of one capacity group hold the same number of
// entries and grow together (rwr: rs and doomed; ugs: adj and adjf; eps: nbr and ecs).
constexpr int STORE_MAX = 6;
struct StoreArray { size_t elem; int group; };
struct StoreShape { int arrays, groups; StoreArray a[STORE_MAX]; };

// One generation of the storage.  Growth makes a new one and copies; a job holds the one it walks on for as long as it lives.
struct StoreGen {
    const StoreShape &shape;
    void *p[STORE_MAX] = {};
    int64_t cap[STORE_MAX] = {};              // entries per group, each at least 1
    explicit StoreGen(const StoreShape &s) : shape(s) {}
    StoreGen(const StoreGen &) = delete;
    ~StoreGen();
    int64_t bytes() const;
    template <class T> T *at(int array) const { return static_cast<T *>(p[array]); }
};

// The state every cache has; a cache derives its own from it and adds its slots (a deque whose entries have n, cols and col0).
// The locking, the same for all three: adds run one at a time under add_mu, from the build to the publication, and only they write
// used, gen and dev, so an add reads them under add_mu alone.  An add publishes under the exclusive `mu`, only after its stream has
// synchronised, and a failed add publishes nothing: the cache is as it was.  A begin copies `gen` and reads the slots under the
// shared `mu`, and its job keeps the generation alive (plan->keep for ugs, the fill hook's capture for rwr and eps).
struct CacheState {
    const StoreShape &shape;
    const char *name, *sampler;               // "rwr cache" in the add's refusals and the device check, "rwr_sampler" in the begin's
    int info_vertices, info_entries;          // the groups whose fill info reports as vertices and as half-edges / CSR entries
    int dev = -1;
    int64_t reserve[STORE_MAX] = {};          // per group: the least a first allocation takes
    std::mutex add_mu;
    std::shared_mutex mu;
    std::shared_ptr<StoreGen> gen;
    int64_t used[STORE_MAX] = {}, graphs = 0, generations = 0;
    CacheState(const StoreShape &s, const char *name_, const char *sampler_, int info_v, int info_e)
        : shape(s), name(name_), sampler(sampler_), info_vertices(info_v), info_entries(info_e) {}
};
int cache_reserve_check(int64_t reserve_vertices, int64_t reserve_columns);
int cache_info(CacheState *st, int64_t *graphs_out, int64_t *vertices_out, int64_t *entries_out, int64_t *bytes_out, int64_t *generations_out);

// An add between its front half and its publication.
struct CacheAdd {
    DeviceCtx dc;
    std::shared_ptr<StoreGen> gen;            // where the build writes, behind `used`: the current generation or (grow) a new one
    bool grow = false;
    int64_t need[STORE_MAX] = {};             // per group: the entries used once the add is published
};
// The add's front half.  cache_add_args: the argument checks (`outs`: the outputs the cache fills for G > 0 are there); G == 0 adds
// nothing and is no error unless it brings columns.  The ptr scan is scan_ptr.  cache_walk_columns hands column x to
// each(x, g, u - ptr[g], v - ptr[g]) and leaves the prefix sums of the columns per graph in cptr [G + 1]: columns must come graph by
// graph, in the order of the graphs, both endpoints inside the graph -- that order is what a batch is compared with, and a column
// that left its graph could fall into a neighbour's range once the graph stands in a batch.  cache_add_device (under add_mu, behind
// the cache's own 2^31 guards): the calling thread's device, which must be the cache's.
int cache_add_args(const char *name, bool have_cache, const int64_t *edge_index, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                   bool outs, const char *outs_text, int64_t cols_limit, const char *cols_limit_text);
template <class Each>
int cache_walk_columns(const char *name, const int64_t *edge_index, int64_t row_stride, int64_t E, const int64_t *ptr, int64_t G,
                       std::vector<int64_t> &cptr, Each each) {
    cptr.assign((size_t)G + 1, 0);
    int64_t g = 0;
    for (int64_t x = 0; x < E; ++x) {
        const int64_t u = edge_index[x], v = edge_index[row_stride + x];
        while (g < G && !(ptr[g] <= u && u < ptr[g + 1])) ++g;
        if (g >= G || !(ptr[g] <= v && v < ptr[g + 1]))
            return fail(UGS_E_BAD_ARG, std::string(name) + " add: column " + std::to_string(x) + " is not inside one graph, or the columns are not in the order of the graphs");
        ++cptr[(size_t)g + 1];
        each(x, g, u - ptr[g], v - ptr[g]);
    }
    for (int64_t h = 0; h < G; ++h) cptr[(size_t)h + 1] += cptr[(size_t)h];
    return UGS_OK;
}
int cache_add_device(const CacheState &st, CacheAdd &a);
// Room for a.need: the current generation, or a new one -- per group max(need, twice what there was, the reserve) entries, at least
// 1 -- with the copies of everything held so far (used * elem bytes of every array) queued on the add's stream.
int cache_room(const CacheState &st, CacheAdd &a);
// The publication, behind the stream's synchronisation: push() appends the cache's slots, placed from st.used as it still is.
template <class Push>
void cache_publish(CacheState &st, const CacheAdd &a, int64_t G, Push push) {
    std::unique_lock<std::shared_mutex> lk(st.mu);
    push();
    st.dev = a.dc.id;
    if (a.grow) { st.gen = a.gen; ++st.generations; }
    std::copy(a.need, a.need + st.shape.groups, st.used);
    st.graphs += G;
}

// What a begin takes from the cache under the shared lock: the generation, and per graph of the batch the prefix sums of the column
// counts and the first stored column (E = coff[G]).
struct CacheBatch {
    std::shared_ptr<StoreGen> gen;
    int dev = -1;
    std::vector<int64_t> coff, col0;
    int64_t E = 0;
};
// The begin's front half.  cache_begin_args: the argument checks all three share; the cache's own follow it.  cache_scan_slots:
// every slot known, ptr non-decreasing, every graph of the batch as large as the graph added in its place; each(g, slot, n) writes
// the cache's descriptor and may refuse the graph (its return, UGS_OK to go on).  cache_begin_device: the column total, if the
// batch's columns are at hand (`compare`), and the calling thread's device, which must be the cache's.
int cache_begin_args(const char *name, bool have_args, const int64_t *slots, const int64_t *edge_index, int64_t num_cols, int64_t num_graphs, int check);
template <class Slots, class Each>
int cache_scan_slots(CacheState &st, const Slots &all, const int64_t *slots, const int64_t *ptr, int64_t G, CacheBatch &cb, Each each) {
    if (G >= (int64_t)0x7f7f7f7f) return fail(UGS_E_UNSUPPORTED, "batch too large: graphs must be < 0x7f7f7f7f");   // (first_bad starts there)
    cb.coff.assign((size_t)G + 1, 0); cb.col0.assign((size_t)G, 0);
    std::shared_lock<std::shared_mutex> lk(st.mu);
    cb.gen = st.gen;
    cb.dev = st.dev;
    for (int64_t g = 0; g < G; ++g) {
        if (slots[g] < 0 || slots[g] >= (int64_t)all.size()) return fail(UGS_E_BAD_ARG, std::string("unknown ") + st.name + " slot " + std::to_string(slots[g]));
        const auto &s = all[(size_t)slots[g]];
        const int64_t n = ptr[g + 1] - ptr[g];
        if (n < 0) return fail(UGS_E_BAD_ARG, "ptr must be non-decreasing (graph " + std::to_string(g) + ")");
        if (n != s.n)
            return fail(UGS_E_BAD_ARG, std::string(st.sampler) + " cache: graph " + std::to_string(g) + " of the batch has " + std::to_string(n) +
                                           " vertices, the graph added in its place has " + std::to_string(s.n));
        if (int rc = each(g, s, n)) return rc;
        cb.coff[(size_t)g + 1] = cb.coff[(size_t)g] + s.cols;
        cb.col0[(size_t)g] = s.col0;
    }
    cb.E = cb.coff[(size_t)G];
    return UGS_OK;
}
int cache_begin_device(const CacheState &st, const CacheBatch &cb, bool compare, int64_t num_cols, DeviceCtx &dc);

// The inputs of the check of a cached call (ugs_store_check, ugs_rwr_store_check), as pieces of the call's blob: coff [G + 1],
// lo [G] (the batch's ptr), col0 [G] and both rows of the batch's Ec columns.  A piece goes up only where its flag says so; each
// cache fills its own kernel struct from the offsets.  cache_check_verdict turns the word the check leaves (first_bad, 0x7f7f7f7f
// where the host set it: above every g) into the refusal.
struct CheckInputs {
    size_t coff, lo, col0, src, dst;
    bool coff_up, lo_up, col0_up;
    int64_t Ec;
    CheckInputs(BlobLayout &L, int64_t G, int64_t Ec_, bool coff_up_, bool lo_up_, bool col0_up_)
        : coff(L.take(coff_up_ ? (size_t)(G + 1) * 8 : 0)), lo(L.take(lo_up_ ? (size_t)G * 8 : 0)), col0(L.take(col0_up_ ? (size_t)G * 8 : 0)),
          src(L.take((size_t)Ec_ * 8)), dst(L.take((size_t)Ec_ * 8)), coff_up(coff_up_), lo_up(lo_up_), col0_up(col0_up_), Ec(Ec_) {}
    void stage(char *host, const CacheBatch &cb, const int64_t *ptr, int64_t G, const int64_t *edge_index, int64_t row_stride) const;
};
int cache_check_verdict(const CacheState &st, int64_t word, int64_t G);

}  // namespace ugs_host
