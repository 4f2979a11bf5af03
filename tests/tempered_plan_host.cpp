// The launch arithmetic of k_temper (enstop_amd/csrc/plsa_tempered_plan.hpp) on a CPU; tests/test_tempered_plan_host.py builds
// this with the sanitizers and feeds the cases.
//
// stdin, one call per line; stdout, one line of results per call:
//     temper n4 grid_cap -> grid threads stride starts_ok counted walked
// n4: float4s of the table.  threads = grid * block.  starts_ok: the first indices of the threads, in launch order, are
// 0, 1, ..., threads - 1.  counted: sum over the threads of the float4s each one's loop visits (closed form per thread).
// walked: the kernel's loop run literally for every thread over a bitmap of n4 places taken from the heap -- 1 when every
// place was visited exactly once and none outside, 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../enstop_amd/csrc/plsa_tempered_plan.hpp"

namespace plan = plsa::plan;

int main() {
    char name[32];
    long long n4, cap;
    while (std::scanf("%31s %lld %lld", name, &n4, &cap) == 3) {
        if (std::strcmp(name, "temper")) { std::fprintf(stderr, "unknown call: %s\n", name); return 2; }
        const int grid = plan::temper_grid(n4, (int)cap);
        const int64_t threads = (int64_t)grid * plan::TEMPER_BLOCK, stride = plan::temper_stride((unsigned)grid);
        const size_t words = (size_t)((n4 + 63) / 64);
        std::unique_ptr<uint64_t[]> seen(new uint64_t[words]());      // exactly the places of the table
        bool starts_ok = true, once = true;
        int64_t counted = 0, expect = 0;
        for (int b = 0; b < grid; ++b)
            for (int l = 0; l < plan::TEMPER_BLOCK; ++l, ++expect) {
                const int64_t first = plan::temper_first((unsigned)b, (unsigned)l);
                starts_ok = starts_ok && first == expect;
                if (first < n4) counted += (n4 - 1 - first) / stride + 1;
            }
        // the kernel's loop, `for (i = first; i < n4; i += stride)` of every thread, with the trips as the outer loop (trip j
        // of all threads before trip j + 1: the same visits, in the order the memory lies)
        for (int64_t trip = 0; trip * stride < n4; ++trip)
            for (int b = 0; b < grid; ++b)
                for (int l = 0; l < plan::TEMPER_BLOCK; ++l) {
                    const int64_t i = plan::temper_first((unsigned)b, (unsigned)l) + trip * stride;
                    if (!(i < n4)) continue;
                    uint64_t &w = seen[(size_t)(i >> 6)];
                    const uint64_t bit = 1ull << (i & 63);
                    once = once && !(w & bit);
                    w |= bit;
                }
        for (size_t w = 0; w < words && once; ++w) {
            const int64_t left = n4 - (int64_t)w * 64;
            once = seen[w] == (left >= 64 ? ~0ull : (1ull << left) - 1);
        }
        std::printf("%d %lld %lld %d %lld %d\n", grid, (long long)threads, (long long)stride, starts_ok ? 1 : 0,
                    (long long)counted, once ? 1 : 0);
    }
    return 0;
}
