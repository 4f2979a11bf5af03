// The launch arithmetic of the LDA kernels (enstop_amd/csrc/plsa_lda_plan.hpp) on a CPU: the header is free of HIP.  Reads cases
// "kind rows kq k cap" from standard input and walks the kernels' own loops for every thread of the grid the plan gives.
//   stream: k_lda_tables / k_lda_rows / k_lda_topics over rows * kq float4s.  Prints
//           grid threads visited_once(0/1) positions_ok(0/1) masks_ok(0/1)
//   rowsum: k_lda_rowsum / k_lda_wordmax, one group of lanes per row.  Prints
//           grid lanes groups visited_once(0/1) order_ok(0/1)       (order: lane l takes the quarters l, l + lanes, ... ascending)
//   slabs:  k_lda_bound / k_lda_topic_partial / k_lda_shift_sum over `rows` rows, k_lda_topic_sums over 4 kq topics.  Prints
//           slabs topic_grid shift_slabs cut_ok(0/1)       (cut: both slab counts cut the rows into consecutive ranges)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../enstop_amd/csrc/plsa_lda_plan.hpp"

namespace plan = plsa::plan;

static void stream(int64_t rows, int kq, int k, int cap) {
    const int64_t n4 = rows * kq;
    const int grid = plan::lda_grid(n4, cap);
    std::vector<uint8_t> seen((size_t)n4, 0);
    bool once = true, pos_ok = true, mask_ok = true;
    const int64_t stride = plan::smooth_stride((unsigned)grid);
    const plan::SmoothStep step = plan::smooth_step(stride, kq);
    for (int b = 0; b < grid; ++b)
        for (int t = 0; t < plan::LDA_BLOCK; ++t) {
            int64_t i = plan::smooth_first((unsigned)b, (unsigned)t);
            plan::SmoothPos p = plan::smooth_pos(i, kq);
            for (; i < n4; i += stride) {
                if (seen[(size_t)i]++) once = false;
                if (p.row != i / kq || p.q != (int)(i % kq)) pos_ok = false;
                unsigned want = 0;
                for (int j = 0; j < 4; ++j) if (4 * p.q + j < k) want |= 1u << j;
                if (plan::smooth_pad_mask(p.q, k) != want) mask_ok = false;
                p = plan::smooth_advance(p, step, kq);
            }
        }
    for (int64_t i = 0; i < n4; ++i) if (seen[(size_t)i] != 1) once = false;
    std::printf("%d %lld %d %d %d\n", grid, (long long)grid * plan::LDA_BLOCK, once ? 1 : 0, pos_ok ? 1 : 0, mask_ok ? 1 : 0);
}

static void rowsum(int64_t rows, int kq, int cap) {
    const int lanes = plan::lda_row_lanes(kq), groups = plan::lda_row_groups(lanes);
    const int grid = plan::lda_rowsum_grid(rows, kq, cap);
    std::vector<uint8_t> seen((size_t)(rows * kq), 0);
    bool once = true, order_ok = true;
    const int64_t stride = plan::lda_row_stride((unsigned)grid, lanes);
    for (int b = 0; b < grid; ++b)
        for (int t = 0; t < plan::LDA_BLOCK; ++t) {
            const int lane = t % lanes, group = t / lanes;
            if ((t - lane) / plan::LDA_WAVE != (t - lane + lanes - 1) / plan::LDA_WAVE) order_ok = false;   // a group never leaves its wavefront
            for (int64_t row = plan::lda_row_first((unsigned)b, group, lanes); row < rows; row += stride) {
                int last = -1;
                for (int q = lane; q < kq; q += lanes) {
                    if (seen[(size_t)(row * kq + q)]++) once = false;
                    if (q <= last) order_ok = false;
                    last = q;
                }
            }
        }
    for (size_t i = 0; i < seen.size(); ++i) if (seen[i] != 1) once = false;
    std::printf("%d %d %d %d %d\n", grid, lanes, groups, once ? 1 : 0, order_ok ? 1 : 0);
}

static void slabs(int64_t rows, int kq) {
    const int counts[2] = {plan::lda_bound_grid(rows), plan::lda_shift_grid(rows)};
    bool cut_ok = true;
    for (int n : counts) {
        int64_t next = 0;
        for (int s = 0; s < n; ++s) {
            const int64_t first = plan::prior_rows_first(rows, (unsigned)n, (unsigned)s), last = plan::prior_rows_last(rows, (unsigned)n, (unsigned)s);
            if (last > first) {
                if (first != next) cut_ok = false;
                next = last;
            }
        }
        if (next != rows) cut_ok = false;
    }
    std::printf("%d %d %d %d\n", counts[0], plan::lda_topic_grid(4 * kq), counts[1], cut_ok ? 1 : 0);
}

int main() {
    char kind[16];
    long long rows;
    int kq, k, cap;
    while (std::scanf("%15s %lld %d %d %d", kind, &rows, &kq, &k, &cap) == 5) {
        if (!std::strcmp(kind, "stream")) stream(rows, kq, k, cap);
        else if (!std::strcmp(kind, "rowsum")) rowsum(rows, kq, cap);
        else if (!std::strcmp(kind, "slabs")) slabs(rows, kq);
        else return 2;
    }
    return 0;
}
