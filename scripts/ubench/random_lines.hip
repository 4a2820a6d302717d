// random_lines: the read rate of uniformly random, 128-byte-aligned 128-byte lines from a table of a given size -- the
// access an FM-index LF step makes (one line per range end).  Every lane reads whole lines (8 x 16 B) at indices from
// a per-lane hash stream, LINES_PER_LANE of them, independent of each other (no pointer chase), and folds them into one
// word so that nothing is dead.  Prints one JSON line per table size.
//   hipcc --offload-arch=gfx950 -O3 -o random_lines random_lines.hip && ./random_lines 1572864 31457280
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                                \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

constexpr int LINES_PER_LANE = 256;

__global__ __launch_bounds__(256) void read_lines(const uint4 *__restrict__ table, uint64_t nlines, uint32_t seed, uint32_t *__restrict__ out)
{
    const uint64_t gid = blockIdx.x * 256ull + threadIdx.x;
    uint32_t x = (uint32_t)gid * 0x9E3779B9u ^ seed, acc = 0;
    for (int k = 0; k < LINES_PER_LANE; ++k) {
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
        const uint4 *p = table + (uint64_t)(x % nlines) * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint4 v = p[q];
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    }
    out[gid] = acc;
}

int main(int argc, char **argv)
{
    const int blocks = 256 * 32; // 256 CUs x 8 workgroups of 4 waves
    uint32_t *d_out;
    CHECK(hipMalloc(&d_out, blocks * 256 * sizeof(uint32_t)));
    for (int a = 1; a < argc; ++a) {
        const uint64_t bytes = strtoull(argv[a], nullptr, 10) & ~127ull, nlines = bytes / 128;
        uint4 *d_table;
        CHECK(hipMalloc(&d_table, bytes));
        CHECK(hipMemset(d_table, 0x5A, bytes));
        hipEvent_t e0, e1;
        CHECK(hipEventCreate(&e0));
        CHECK(hipEventCreate(&e1));
        for (int w = 0; w < 3; ++w)
            hipLaunchKernelGGL(read_lines, dim3(blocks), dim3(256), 0, 0, d_table, nlines, 7u + w, d_out);
        CHECK(hipDeviceSynchronize());
        std::vector<float> ms;
        for (int r = 0; r < 10; ++r) {
            CHECK(hipEventRecord(e0));
            hipLaunchKernelGGL(read_lines, dim3(blocks), dim3(256), 0, 0, d_table, nlines, 100u + r, d_out);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float t;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            ms.push_back(t);
        }
        float best = ms[0], sum = 0;
        for (float t : ms) {
            best = t < best ? t : best;
            sum += t;
        }
        const double lines = (double)blocks * 256 * LINES_PER_LANE;
        printf("{\"table_bytes\": %llu, \"lines\": %.0f, \"best_ms\": %.4f, \"mean_ms\": %.4f, \"lines_per_s\": %.4e, "
               "\"GB_per_s\": %.1f}\n",
               (unsigned long long)bytes, lines, best, sum / ms.size(), lines / (best * 1e-3), lines * 128 / (best * 1e-3) / 1e9);
        CHECK(hipFree(d_table));
        CHECK(hipEventDestroy(e0));
        CHECK(hipEventDestroy(e1));
    }
    CHECK(hipFree(d_out));
    return 0;
}
