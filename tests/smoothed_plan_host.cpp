// The launch arithmetic of the smoothed-EM kernels (enstop_amd/csrc/plsa_smoothed_plan.hpp) on a CPU;
// tests/test_smoothed_plan_host.py builds this with the sanitizers and feeds the cases.
//
// stdin, one call per line; stdout, one line of results per call:
//     smooth rows kq k grid_cap -> grid threads stride starts_ok walked pos_ok mask_ok
//     prior  rows kq k 0        -> slabs threads 256 cut_ok walked pos_ok mask_ok
// A table is [rows, 4 kq] float32: rows * kq float4s.  smooth: the loop of k_smooth_rows / k_smooth_topics run literally for
// every thread of the grid the plan gives -- batches of four strides with the positions advanced by smooth_advance, then the
// remainder -- over a bitmap of the table's float4s taken from the heap.  prior: the loop of k_log_prior for every thread of
// every slab.  walked: every place was visited exactly once and none outside.  pos_ok: at every visit the walked position was
// (i / kq, i % kq).  mask_ok: at every visit bit j of the pad mask was (4 q + j < k).  starts_ok: the first indices of the
// threads, in launch order, are 0, 1, ...  cut_ok: the slabs' row ranges are consecutive and cover [0, rows).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../enstop_amd/csrc/plsa_smoothed_plan.hpp"

namespace plan = plsa::plan;

struct Walk {
    int64_t n4;
    int kq, k;
    std::unique_ptr<uint64_t[]> seen;
    bool once = true, pos_ok = true, mask_ok = true;
    Walk(int64_t n4_, int kq_, int k_) : n4(n4_), kq(kq_), k(k_), seen(new uint64_t[(size_t)((n4_ + 63) / 64)]()) {}
    void visit(int64_t i, const plan::SmoothPos &p) {
        if (i < 0 || i >= n4) { once = false; return; }
        uint64_t &w = seen[(size_t)(i >> 6)];
        const uint64_t bit = 1ull << (i & 63);
        once = once && !(w & bit);
        w |= bit;
        pos_ok = pos_ok && p.row == i / kq && p.q == (int)(i % kq);
        unsigned want = 0;
        for (int j = 0; j < 4; ++j)
            if (4 * (int)(i % kq) + j < k) want |= 1u << j;
        mask_ok = mask_ok && plan::smooth_pad_mask(p.q, k) == want;
    }
    bool all() {
        const size_t words = (size_t)((n4 + 63) / 64);
        for (size_t w = 0; w < words && once; ++w) {
            const int64_t left = n4 - (int64_t)w * 64;
            once = seen[w] == (left >= 64 ? ~0ull : (1ull << left) - 1);
        }
        return once;
    }
};

int main() {
    char name[32];
    long long rows, kq, k, cap;
    while (std::scanf("%31s %lld %lld %lld %lld", name, &rows, &kq, &k, &cap) == 5) {
        const int64_t n4 = rows * kq;
        Walk walk(n4, (int)kq, (int)k);
        if (!std::strcmp(name, "smooth")) {
            const int grid = plan::smooth_grid(n4, (int)cap);
            const int64_t stride = plan::smooth_stride((unsigned)grid);
            const plan::SmoothStep step = plan::smooth_step(stride, (int)kq);
            bool starts_ok = true;
            int64_t expect = 0;
            for (int b = 0; b < grid; ++b)
                for (int l = 0; l < plan::SMOOTH_BLOCK; ++l, ++expect) {
                    int64_t i = plan::smooth_first((unsigned)b, (unsigned)l);
                    starts_ok = starts_ok && i == expect;
                    plan::SmoothPos p0 = plan::smooth_pos(i, (int)kq);
                    for (; i + 3 * stride < n4; i += 4 * stride) {
                        const plan::SmoothPos p1 = plan::smooth_advance(p0, step, (int)kq), p2 = plan::smooth_advance(p1, step, (int)kq),
                                              p3 = plan::smooth_advance(p2, step, (int)kq);
                        walk.visit(i, p0); walk.visit(i + stride, p1); walk.visit(i + 2 * stride, p2); walk.visit(i + 3 * stride, p3);
                        p0 = plan::smooth_advance(p3, step, (int)kq);
                    }
                    for (; i < n4; i += stride) {
                        walk.visit(i, p0);
                        p0 = plan::smooth_advance(p0, step, (int)kq);
                    }
                }
            const bool walked = walk.all();
            std::printf("%d %lld %lld %d %d %d %d\n", grid, (long long)grid * plan::SMOOTH_BLOCK, (long long)stride, starts_ok ? 1 : 0,
                        walked ? 1 : 0, walk.pos_ok ? 1 : 0, walk.mask_ok ? 1 : 0);
        } else if (!std::strcmp(name, "prior")) {
            const int slabs = plan::prior_grid(rows);
            const plan::SmoothStep step = plan::smooth_step(plan::SMOOTH_BLOCK, (int)kq);
            bool cut_ok = true;
            int64_t next = 0;
            for (int s = 0; s < slabs; ++s) {
                const int64_t first = plan::prior_rows_first(rows, (unsigned)slabs, (unsigned)s);
                const int64_t last = plan::prior_rows_last(rows, (unsigned)slabs, (unsigned)s);
                if (first < last) { cut_ok = cut_ok && first == next; next = last; }
                for (int l = 0; l < plan::SMOOTH_BLOCK; ++l) {
                    const int64_t end = last * kq;
                    int64_t i = first * kq + l;
                    plan::SmoothPos p = plan::smooth_pos(i, (int)kq);
                    for (; i < end; i += plan::SMOOTH_BLOCK) {
                        walk.visit(i, p);
                        p = plan::smooth_advance(p, step, (int)kq);
                    }
                }
            }
            cut_ok = cut_ok && next == rows;
            const bool walked = walk.all();
            std::printf("%d %lld %d %d %d %d %d\n", slabs, (long long)slabs * plan::SMOOTH_BLOCK, plan::SMOOTH_BLOCK, cut_ok ? 1 : 0,
                        walked ? 1 : 0, walk.pos_ok ? 1 : 0, walk.mask_ok ? 1 : 0);
        } else {
            std::fprintf(stderr, "unknown call: %s\n", name);
            return 2;
        }
    }
    return 0;
}
