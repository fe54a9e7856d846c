// ugs_cache_common.cpp -- what the three dataset caches of libugs_mi355.so share on the host (ugs_rwr_cache.cpp, ugs_graph_cache.cpp,
// ugs_eps_cache.cpp): a generation of device storage described by data and how it grows, the common cache state with create's reserve
// check and info, the front halves of the add and of the sample begin, and the inputs and the verdict of the batch check.
// Declared, with the templates that take a cache's callbacks, in ugs_host_internal.h; DESIGN.md section 17.
#include "ugs_host_internal.h"

namespace ugs_host __attribute__((visibility("hidden"))) {

// ---- generations ----
StoreGen::~StoreGen() { for (int i = 0; i < shape.arrays; ++i) (void)hipFree(p[i]); }

int64_t StoreGen::bytes() const {
    int64_t b = 0;
    for (int i = 0; i < shape.arrays; ++i) b += cap[shape.a[i].group] * (int64_t)shape.a[i].elem;
    return b;
}

int cache_room(const CacheState &st, CacheAdd &a) {
    const StoreShape &sh = st.shape;
    a.gen = st.gen;
    a.grow = !a.gen;
    for (int g = 0; g < sh.groups && !a.grow; ++g) a.grow = a.need[g] > a.gen->cap[g];
    if (!a.grow) return UGS_OK;
    auto room = [](int64_t need, int64_t have, int64_t reserve) { return need <= have ? have : std::max({need, 2 * have, reserve}); };
    const std::shared_ptr<StoreGen> old = a.gen;
    a.gen = std::make_shared<StoreGen>(sh);
    for (int g = 0; g < sh.groups; ++g) a.gen->cap[g] = std::max<int64_t>(room(a.need[g], old ? old->cap[g] : 0, st.reserve[g]), 1);
    for (int i = 0; i < sh.arrays; ++i) HIP_TRY(hipMalloc(&a.gen->p[i], (size_t)a.gen->cap[sh.a[i].group] * sh.a[i].elem));
    for (int i = 0; old && i < sh.arrays; ++i)
        if (const int64_t used = st.used[sh.a[i].group]; used > 0)
            HIP_TRY(hipMemcpyAsync(a.gen->p[i], old->p[i], (size_t)used * sh.a[i].elem, hipMemcpyDeviceToDevice, a.dc.stream));
    return UGS_OK;
}

// ---- create and info ----
int cache_reserve_check(int64_t reserve_vertices, int64_t reserve_columns) {
    if (reserve_vertices < 0 || reserve_vertices >= (int64_t)INT32_MAX || reserve_columns < 0 || reserve_columns >= ((int64_t)1 << 30))
        return fail(UGS_E_BAD_ARG, "reserve must be 0 ... 2^31 - 2 vertices and 0 ... 2^30 - 1 columns");
    return UGS_OK;
}

int cache_info(CacheState *st, int64_t *graphs_out, int64_t *vertices_out, int64_t *entries_out, int64_t *bytes_out, int64_t *generations_out) {
    if (!st) return fail(UGS_E_BAD_ARG, "cache is null");
    std::shared_lock<std::shared_mutex> lk(st->mu);
    if (graphs_out) *graphs_out = st->graphs;
    if (vertices_out) *vertices_out = st->used[st->info_vertices];
    if (entries_out) *entries_out = st->used[st->info_entries];
    if (bytes_out) *bytes_out = st->gen ? st->gen->bytes() : 0;
    if (generations_out) *generations_out = st->generations;
    return UGS_OK;
}

// ---- the calling thread's device, which must be the cache's (what: "add" or "call") ----
static int cache_device(const char *name, int cache_dev, const char *what, DeviceCtx &dc) {
    if (int rc = device_ctx(dc)) return rc;
    if (cache_dev >= 0 && cache_dev != dc.id)
        return fail(UGS_E_BAD_ARG, std::string("the ") + name + " lives on device " + std::to_string(cache_dev) + ", this " + what + " runs on device " + std::to_string(dc.id));
    return UGS_OK;
}

// ---- the add's front half ----
int cache_add_args(const char *name, bool have_cache, const int64_t *edge_index, int64_t num_cols, const int64_t *ptr, int64_t num_graphs,
                   bool outs, const char *outs_text, int64_t cols_limit, const char *cols_limit_text) {
    const std::string nm(name);
    if (!have_cache || !ptr || num_cols < 0 || (num_cols > 0 && !edge_index)) return fail(UGS_E_BAD_ARG, "bad arguments to " + nm + " add");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !outs) return fail(UGS_E_BAD_ARG, nm + " add needs " + outs_text);
    if (num_cols >= cols_limit) return fail(UGS_E_UNSUPPORTED, std::string("add too large: columns must be < ") + cols_limit_text);
    if (num_graphs == 0 && num_cols > 0) return fail(UGS_E_BAD_ARG, nm + " add: columns without a graph");
    return UGS_OK;
}

int cache_add_device(const CacheState &st, CacheAdd &a) { return cache_device(st.name, st.dev, "add", a.dc); }

// ---- the begin's front half ----
int cache_begin_args(const char *name, bool have_args, const int64_t *slots, const int64_t *edge_index, int64_t num_cols, int64_t num_graphs, int check) {
    if (!have_args) return fail(UGS_E_BAD_ARG, "bad arguments to sample_batch");
    if (num_graphs < 0) return fail(UGS_E_BAD_ARG, "ptr must hold at least one entry");
    if (num_graphs > 0 && !slots) return fail(UGS_E_BAD_ARG, std::string(name) + " sample needs one slot per graph");
    if (check && (num_cols < 0 || (num_cols > 0 && !edge_index))) return fail(UGS_E_BAD_ARG, "the check needs the batch's edge_index");
    return UGS_OK;
}

int cache_begin_device(const CacheState &st, const CacheBatch &cb, bool compare, int64_t num_cols, DeviceCtx &dc) {
    if (compare && num_cols != cb.E)
        return fail(UGS_E_BAD_ARG, std::string(st.sampler) + " cache: the batch has " + std::to_string(num_cols) + " columns, the added graphs have " + std::to_string(cb.E));
    return cache_device(st.name, cb.dev, "call", dc);
}

// ---- the check ----
void CheckInputs::stage(char *host, const CacheBatch &cb, const int64_t *ptr, int64_t G, const int64_t *edge_index, int64_t row_stride) const {
    if (coff_up) std::memcpy(host + coff, cb.coff.data(), (size_t)(G + 1) * 8);
    if (lo_up && G > 0) std::memcpy(host + lo, ptr, (size_t)G * 8);
    if (col0_up && G > 0) std::memcpy(host + col0, cb.col0.data(), (size_t)G * 8);
    if (Ec > 0) {
        std::memcpy(host + src, edge_index, (size_t)Ec * 8);
        std::memcpy(host + dst, edge_index + row_stride, (size_t)Ec * 8);
    }
}

int cache_check_verdict(const CacheState &st, int64_t word, int64_t G) {
    const int64_t bad = (int64_t)(int32_t)(word & 0xffffffff);
    if (bad < G) return fail(UGS_E_BAD_ARG, std::string(st.sampler) + " cache: graph " + std::to_string(bad) + " of the batch differs from the graph added in its place");
    return UGS_OK;
}

}  // namespace ugs_host
