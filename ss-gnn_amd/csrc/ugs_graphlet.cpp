// ugs_graphlet.cpp -- host side of ugs_sampler.graphlets (C ABI: ugs_graphlet_canon_code / ugs_graphlet_table and, for the orbits,
// ugs_graphlet_rooted_codes / ugs_graphlet_orbit_counts, for node-labelled graphs ugs_graphlet_labelled_code and, for the vertex
// census, ugs_graphlet_vertex_census_entry in include/ugs_mi355.h, which states the laws; kernels: ugs_graphlet.hip; the search all
// share: ugs_graphlet_common.h).
// No device work here: the table of all graphs on n vertices, and their orbit counts, are built on the host, once per process and n.
#include "ugs_host_internal.h"
#include "ugs_graphlet_common.h"

#include <algorithm>
#include <mutex>
#include <vector>

using namespace ugs_host;

namespace {

struct HostStack {
    uint64_t w[UGS_GL_KMAX];
    void put(int level, uint64_t v) { w[level] = v; }
    uint64_t get(int level) const { return w[level]; }
};

uint32_t canon_code(uint32_t code, int n, uint32_t *stats = nullptr) {
    HostStack st;
    return ugs_gl::canon(ugs_gl::adj_of_code(code, n), n, st, stats);
}

// The rooted codes of the n vertices, and how many distinct ones there are: the number of orbits.
int rooted_codes(uint32_t code, int n, uint32_t *out) {
    HostStack st;
    const uint64_t adj = ugs_gl::adj_of_code(code, n);
    int distinct = 0;
    for (int v = 0; v < n; ++v) {
        out[v] = ugs_gl::rooted(adj, n, v, st);
        distinct += std::find(out, out + v, out[v]) == out + v;
    }
    return distinct;
}

std::mutex g_table_mu;
std::vector<uint32_t> g_codes[UGS_GL_KMAX + 1];       // [n]: canonical codes of all graphs on n vertices, ascending; empty = not built
std::vector<int64_t> g_orbits[UGS_GL_KMAX + 1];       // [n]: the number of orbits of each of them; empty = not built
std::vector<int64_t> g_connected[UGS_GL_KMAX + 1];    // [n]: the keys of the connected ones among them, ascending; empty = not built

// Every graph on n vertices is a graph on n - 1 vertices plus a last vertex, and the last vertex's column is the top n - 1 bits: all
// (n-1)-classes times all 2^(n-1) neighbour sets reach every n-class.  Called with the mutex held.
const std::vector<uint32_t> &codes_of(int n) {
    std::vector<uint32_t> &out = g_codes[n];
    if (!out.empty()) return out;
    if (n == 1) { out.push_back(0); return out; }
    const std::vector<uint32_t> &below = codes_of(n - 1);
    const int lo = ugs_gl::tri(n - 1);
    std::vector<uint32_t> all;
    all.reserve(below.size() << (n - 1));
    for (uint32_t c : below)
        for (uint32_t s = 0; s < (1u << (n - 1)); ++s) all.push_back(canon_code(c | (s << lo), n));
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    out.swap(all);
    return out;
}

}  // namespace

extern "C" {

int ugs_graphlet_canon_code(uint32_t code, int n, uint32_t *out) {
    if (n < 1 || n > UGS_GL_KMAX) return fail(UGS_E_UNSUPPORTED, "graphlet_canon_code: 1 <= n <= 8");
    if (!out) return fail(UGS_E_BAD_ARG, "graphlet_canon_code: null output pointer");
    if ((uint64_t)code >> ugs_gl::tri(n)) return fail(UGS_E_BAD_ARG, "graphlet_canon_code: the code has bits above n(n-1)/2");
    *out = canon_code(code, n);
    return UGS_OK;
}

int ugs_graphlet_search_stats(uint32_t code, int n, uint32_t *leaves_out, uint32_t *nodes_out) {
    if (n < 1 || n > UGS_GL_KMAX) return fail(UGS_E_UNSUPPORTED, "graphlet_search_stats: 1 <= n <= 8");
    if (!leaves_out || !nodes_out) return fail(UGS_E_BAD_ARG, "graphlet_search_stats: null output pointer");
    if ((uint64_t)code >> ugs_gl::tri(n)) return fail(UGS_E_BAD_ARG, "graphlet_search_stats: the code has bits above n(n-1)/2");
    uint32_t stats[2] = {0, 0};
    canon_code(code, n, stats);
    *leaves_out = stats[0];
    *nodes_out = stats[1];
    return UGS_OK;
}

int ugs_graphlet_table(int n, int64_t *keys_out, int64_t capacity, int64_t *count_out) {
    if (n < 1 || n > UGS_GL_KMAX) return fail(UGS_E_UNSUPPORTED, "graphlet_table: 1 <= n <= 8");
    if (!count_out || capacity < 0 || (capacity > 0 && !keys_out)) return fail(UGS_E_BAD_ARG, "graphlet_table: count_out, and keys_out for capacity > 0, are needed");
    std::lock_guard<std::mutex> lock(g_table_mu);
    const std::vector<uint32_t> &codes = codes_of(n);
    *count_out = (int64_t)codes.size();
    if (capacity >= (int64_t)codes.size())
        for (size_t i = 0; i < codes.size(); ++i) keys_out[i] = ((int64_t)n << 28) | (int64_t)codes[i];
    return UGS_OK;
}

int ugs_graphlet_rooted_codes(uint32_t code, int n, uint32_t *out) {
    if (n < 1 || n > UGS_GL_KMAX) return fail(UGS_E_UNSUPPORTED, "graphlet_rooted_codes: 1 <= n <= 8");
    if (!out) return fail(UGS_E_BAD_ARG, "graphlet_rooted_codes: null output pointer");
    if ((uint64_t)code >> ugs_gl::tri(n)) return fail(UGS_E_BAD_ARG, "graphlet_rooted_codes: the code has bits above n(n-1)/2");
    rooted_codes(code, n, out);
    for (int v = n; v < UGS_GL_KMAX; ++v) out[v] = 0xffffffffu;
    return UGS_OK;
}

int ugs_graphlet_orbit_counts(int n, int64_t *counts_out, int64_t capacity, int64_t *count_out) {
    if (n < 1 || n > UGS_GL_KMAX) return fail(UGS_E_UNSUPPORTED, "graphlet_orbit_counts: 1 <= n <= 8");
    if (!count_out || capacity < 0 || (capacity > 0 && !counts_out)) return fail(UGS_E_BAD_ARG, "graphlet_orbit_counts: count_out, and counts_out for capacity > 0, are needed");
    std::lock_guard<std::mutex> lock(g_table_mu);
    const std::vector<uint32_t> &codes = codes_of(n);
    std::vector<int64_t> &orbits = g_orbits[n];
    if (orbits.empty()) {
        uint32_t rooted[UGS_GL_KMAX];
        orbits.reserve(codes.size());
        for (uint32_t c : codes) orbits.push_back(rooted_codes(c, n, rooted));
    }
    *count_out = (int64_t)orbits.size();
    if (capacity >= (int64_t)orbits.size()) std::copy(orbits.begin(), orbits.end(), counts_out);
    return UGS_OK;
}

int ugs_graphlet_vertex_census_entry(uint32_t code, int n, uint32_t *out) {
    if (n < 1 || n >= UGS_GL_KMAX) return fail(UGS_E_UNSUPPORTED, "graphlet_vertex_census_entry: 1 <= n <= 7");
    if (!out) return fail(UGS_E_BAD_ARG, "graphlet_vertex_census_entry: null output pointer");
    if ((uint64_t)code >> ugs_gl::tri(n)) return fail(UGS_E_BAD_ARG, "graphlet_vertex_census_entry: the code has bits above n(n-1)/2");
    const int64_t *keys;
    int64_t num_keys;
    {
        std::lock_guard<std::mutex> lock(g_table_mu);
        std::vector<int64_t> &conn = g_connected[n];  // never changed once built: read below without the lock
        if (conn.empty())
            for (uint32_t c : codes_of(n))
                if (ugs_gl::connected(ugs_gl::adj_of_code(c, n), n)) conn.push_back(((int64_t)n << 28) | (int64_t)c);
        keys = conn.data();
        num_keys = (int64_t)conn.size();
    }
    HostStack st;
    *out = ugs_gl::vertex_entry(code, n, keys, num_keys, st);
    return UGS_OK;
}

int ugs_graphlet_labelled_code(uint32_t code, int n, const int32_t *labels, int64_t *key_out, uint32_t *rooted_out) {
    if (n < 1 || n > UGS_GL_KMAX) return fail(UGS_E_UNSUPPORTED, "graphlet_labelled_code: 1 <= n <= 8");
    if (!labels || !key_out) return fail(UGS_E_BAD_ARG, "graphlet_labelled_code: null labels or key pointer");
    if ((uint64_t)code >> ugs_gl::tri(n)) return fail(UGS_E_BAD_ARG, "graphlet_labelled_code: the code has bits above n(n-1)/2");
    int lab[UGS_GL_KMAX];
    for (int v = 0; v < n; ++v) {
        if (labels[v] < 0 || labels[v] >= 4096) return fail(UGS_E_BAD_ARG, "graphlet_labelled_code: labels lie in [0, 4096)");
        lab[v] = labels[v];
    }
    HostStack st;
    const uint64_t adj = ugs_gl::adj_of_code(code, n);
    const uint64_t cells = ugs_gl::label_cells(lab, n);
    const uint64_t canon = ugs_gl::canon_cells(adj, cells, n, st);
    std::sort(lab, lab + n);
    uint64_t hi = ((uint64_t)n << 60) | (canon << 32), lo = 0;       // K = n 2^124 + code 2^96 + sum L[p] 2^(12 p)
    for (int p = 0; p < n; ++p) {
        const int at = 12 * p;
        if (at < 64) lo |= (uint64_t)lab[p] << at;                   // L[5] straddles the words: its high 8 bits fall off here
        if (at + 12 > 64) hi |= at >= 64 ? (uint64_t)lab[p] << (at - 64) : (uint64_t)lab[p] >> (64 - at);
    }
    key_out[0] = (int64_t)hi;
    key_out[1] = (int64_t)lo;
    if (rooted_out) {
        for (int v = 0; v < n; ++v) rooted_out[v] = ugs_gl::rooted_cells(adj, cells, n, v, st);
        for (int v = n; v < UGS_GL_KMAX; ++v) rooted_out[v] = 0xffffffffu;
    }
    return UGS_OK;
}

}  // extern "C"
