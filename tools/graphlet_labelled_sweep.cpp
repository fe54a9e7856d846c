// graphlet_labelled_sweep.cpp -- a stand-alone sweep of ugs_graphlet_labelled_code (csrc/ugs_graphlet.cpp) for a sanitizer build on the
// CPU: every class of n = 1 .. 8 under a few labellings, the facts a wrong read or write would break checked on the way.  No device work.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//         tools/graphlet_labelled_sweep.cpp -o graphlet_labelled_sweep && ./graphlet_labelled_sweep
#include "../ss-gnn_amd/csrc/ugs_graphlet.cpp"

#include <cstdio>

int ugs_host::fail(int code, const std::string &msg) {
    std::fprintf(stderr, "refused (%d): %s\n", code, msg.c_str());
    return code;
}

int main() {
    long searches = 0, split = 0;
    for (int n = 1; n <= UGS_GL_KMAX; ++n) {
        int64_t count = 0;
        if (ugs_graphlet_table(n, nullptr, 0, &count)) return 1;
        std::vector<int64_t> keys((size_t)count);
        if (ugs_graphlet_table(n, keys.data(), count, &count)) return 1;
        for (int64_t key : keys) {
            const uint32_t code = (uint32_t)key & ((1u << 28) - 1u);
            uint32_t plain[UGS_GL_KMAX];
            if (ugs_graphlet_rooted_codes(code, n, plain)) return 1;
            // constant; two labels by parity and by half; three labels; all distinct, descending; the widest label everywhere
            const int32_t labellings[6][UGS_GL_KMAX] = {{5, 5, 5, 5, 5, 5, 5, 5},       {0, 1, 0, 1, 0, 1, 0, 1},
                                                        {7, 7, 7, 7, 2, 2, 2, 2},       {1, 0, 2, 1, 0, 2, 1, 0},
                                                        {80, 70, 60, 50, 40, 30, 20, 10}, {4095, 4095, 4095, 4095, 4095, 4095, 4095, 4095}};
            for (int l = 0; l < 6; ++l) {
                int64_t words[2] = {0, 0}, again[2] = {0, 0};
                uint32_t rooted[UGS_GL_KMAX];
                if (ugs_graphlet_labelled_code(code, n, labellings[l], words, rooted)) return 1;
                if (ugs_graphlet_labelled_code(code, n, labellings[l], again, nullptr)) return 1;
                searches += n + 2;
                if (words[0] != again[0] || words[1] != again[1]) return 2;
                const uint32_t canon = (uint32_t)((uint64_t)words[0] >> 32) & ((1u << 28) - 1u);
                if ((int)((uint64_t)words[0] >> 60) != n) return 3;
                int top = 0;
                for (int v = 0; v < n; ++v) top = std::max(top, (int)labellings[l][v]);
                uint32_t least = 1u << 28;
                for (int v = 0; v < n; ++v)
                    if (labellings[l][v] == top) least = std::min(least, rooted[v]);
                if (least != canon) return 4;                    // the canonical code is the smallest rooted code of the largest label
                for (int v = n; v < UGS_GL_KMAX; ++v)
                    if (rooted[v] != 0xffffffffu) return 5;
                if (l == 0 || l == 5) {
                    for (int v = 0; v < n; ++v)
                        if (rooted[v] != plain[v]) return 6;     // constant labels: the unlabelled rooted codes
                    if (canon != code) return 7;                 // and the class's own code
                } else {
                    for (int v = 0; v < n; ++v)
                        for (int w = 0; w < v; ++w)              // labels only ever split an orbit
                            if (labellings[l][v] == labellings[l][w] && rooted[v] == rooted[w] && plain[v] != plain[w]) return 8;
                    for (int v = 0; v < n; ++v)
                        for (int w = 0; w < v; ++w) split += plain[v] == plain[w] && labellings[l][v] != labellings[l][w];
                }
            }
        }
    }
    std::printf("graphlet_labelled_sweep: %ld searches, %ld vertex pairs of one orbit split by their labels, clean\n", searches, split);
    return 0;
}
