// counter_probe.hip -- diagnostic only: what a trip to the walk kernel's work counter costs.  The dynamic work loop
// of ugs_walk_lds asks one 8-byte word in device memory for its rows, atomicAdd with return, lane 0 of a wave, the next request
// only after the answer.  This program does the same and nothing else: CUs x 20 one-wave blocks (the residency of the 448-candidate
// tier), lane 0 of every wave N dependent atomicAdd-with-return.
//   saturated   every wave on ONE word: wall time / trips of all waves = the service time of a same-address trip
//   unloaded    one wave alone: wall time / N = the round trip with nobody else asking
//   W words     the waves spread over W words in separate 128-byte lines (wave w asks word w % W): does the service scale?
// build: hipcc --offload-arch=gfx950 -O2 tools/counter_probe.hip -o ab/counter_probe ; run once on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <algorithm>
#include <vector>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)
constexpr int kLineWords = 16;                    // 128 bytes of 8-byte words
constexpr int kMaxWords = 32;
__global__ __launch_bounds__(64) void k_trips(unsigned long long *words, int nwords, int n, unsigned long long *sink) {
    if (threadIdx.x != 0) return;
    unsigned long long *p = words + (size_t)(blockIdx.x % (unsigned)nwords) * kLineWords;      // nwords <= kMaxWords: inside the buffer
    unsigned long long v = 0ull;
    for (int i = 0; i < n; ++i) v = atomicAdd(p, 1ull + (v >> 63));                            // the next request needs this answer
    sink[blockIdx.x] = v;
}
static double run(unsigned long long *words, unsigned long long *sink, int blocks, int nwords, int n) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 4; ++rep) {           // the first repetition warms up and is dropped
        CHECK(hipMemset(words, 0, (size_t)kMaxWords * kLineWords * 8));
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_trips, dim3(blocks), dim3(64), 0, 0, words, nwords, n, sink);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float t = 0.f; CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    return ms[1] * 1e6;                            // median, ns
}
int main() {
    hipDeviceProp_t pr; CHECK(hipGetDeviceProperties(&pr, 0));
    const int cus = pr.multiProcessorCount, waves = cus * 20;
    unsigned long long *words, *sink;
    CHECK(hipMalloc((void **)&words, (size_t)kMaxWords * kLineWords * 8));
    CHECK(hipMalloc((void **)&sink, (size_t)waves * 8));
    std::printf("%s %s, %d CUs, %d one-wave blocks\n", pr.name, pr.gcnArchName, cus, waves);
    const int n_one = 20000, n_all = 2000;
    const double one = run(words, sink, 1, 1, n_one);
    std::printf("unloaded   1 wave, 1 word, %d trips: %.1f ns per trip (round trip)\n", n_one, one / n_one);
    for (int w : {1, 4, 8, 16, 32}) {
        const double t = run(words, sink, waves, w, n_all);
        const double trips = (double)waves * n_all;
        std::printf("saturated  %d waves, %2d word%s, %d trips each: %.2f ns per trip device-wide (%.1f M trips/s), %.2f us as a wave sees one\n",
                    waves, w, w == 1 ? " " : "s", n_all, t / trips, trips / t * 1e3, t / n_all * 1e-3);
    }
    CHECK(hipFree(words)); CHECK(hipFree(sink));
    return 0;
}
