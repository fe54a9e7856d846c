// graphlet_vertex_table_sweep.cpp -- a stand-alone sweep of ugs_graphlet_vertex_census_entry (csrc/ugs_graphlet.cpp; the code path of
// the device table of graphlets.vertex_census) for a sanitizer build on the CPU: every raw code of n = 1 .. 7 vertices, each entry
// cross-checked against ugs_graphlet_rooted_codes and ugs_graphlet_canon_code.  No device work.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//         tools/graphlet_vertex_table_sweep.cpp -o graphlet_vertex_table_sweep && ./graphlet_vertex_table_sweep
#include "../ss-gnn_amd/csrc/ugs_graphlet.cpp"

#include <cstdio>

int ugs_host::fail(int code, const std::string &msg) {
    std::fprintf(stderr, "refused (%d): %s\n", code, msg.c_str());
    return code;
}

int main() {
    long entries = 0, connected = 0, orbits_seen = 0;
    for (int n = 1; n < UGS_GL_KMAX; ++n) {
        int64_t count = 0;
        if (ugs_graphlet_table(n, nullptr, 0, &count)) return 1;
        std::vector<int64_t> keys((size_t)count), orbit_count((size_t)count);
        if (ugs_graphlet_table(n, keys.data(), count, &count)) return 1;
        if (ugs_graphlet_orbit_counts(n, orbit_count.data(), count, &count)) return 1;
        std::vector<int64_t> conn;                               // the columns: the connected keys, ascending
        std::vector<int64_t> conn_orbits;
        for (int64_t i = 0; i < count; ++i)
            if (ugs_gl::connected(ugs_gl::adj_of_code((uint32_t)keys[(size_t)i] & ((1u << 28) - 1u), n), n)) {
                conn.push_back(keys[(size_t)i]);
                conn_orbits.push_back(orbit_count[(size_t)i]);
            }
        std::vector<char> hit(conn.size(), 0);
        const uint32_t codes = 1u << ugs_gl::tri(n);
        for (uint32_t code = 0; code < codes; ++code) {
            uint32_t entry = 0, canon = 0, rooted[UGS_GL_KMAX];
            if (ugs_graphlet_vertex_census_entry(code, n, &entry)) return 1;
            if (ugs_graphlet_canon_code(code, n, &canon)) return 1;
            if (ugs_graphlet_rooted_codes(code, n, rooted)) return 1;
            ++entries;
            const bool is_conn = ugs_gl::connected(ugs_gl::adj_of_code(code, n), n);
            if ((entry == ugs_gl::VERTEX_NONE) == is_conn) return 2;              // the mark is exactly "not connected"
            if (!is_conn) continue;
            ++connected;
            if (entry >> (ugs_gl::VERTEX_COL_BITS + ugs_gl::VERTEX_ORB_BITS * n)) return 3;   // nothing above the n position fields
            const uint32_t col = ugs_gl::vertex_col(entry);
            if (col >= conn.size() || conn[col] != (((int64_t)n << 28) | (int64_t)canon)) return 4;
            hit[col] = 1;
            int distinct = 0;
            for (int p = 0; p < n; ++p) {
                int below = 0;
                bool first = true;
                for (int q = 0; q < n; ++q) {
                    bool counted = rooted[q] < rooted[p];
                    for (int i = 0; i < q; ++i) counted = counted && rooted[i] != rooted[q];
                    below += counted;
                    if (q < p && rooted[q] == rooted[p]) first = false;
                }
                distinct += first;
                if ((int)ugs_gl::vertex_local(entry, p) != below) return 5;       // the local index of every position
                if (below >= conn_orbits[col]) return 6;                          // inside the class's orbits
            }
            if (distinct != conn_orbits[col]) return 7;
            orbits_seen += distinct;
        }
        for (char h : hit)
            if (!h) return 8;                                    // every column is some code's
        uint32_t out = 0;
        if (ugs_graphlet_vertex_census_entry(codes, n, &out) != UGS_E_BAD_ARG) return 9;   // a bit above n (n - 1) / 2
    }
    uint32_t out = 0;
    if (ugs_graphlet_vertex_census_entry(0, 8, &out) != UGS_E_UNSUPPORTED || ugs_graphlet_vertex_census_entry(0, 0, &out) != UGS_E_UNSUPPORTED) return 10;
    if (ugs_graphlet_vertex_census_entry(0, 3, nullptr) != UGS_E_BAD_ARG) return 11;
    std::printf("graphlet_vertex_table_sweep: %ld entries, %ld of connected graphs, %ld orbits met, clean\n", entries, connected, orbits_seen);
    return 0;
}
