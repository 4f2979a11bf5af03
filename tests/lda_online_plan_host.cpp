// The launch arithmetic of k_lda_online_blend (enstop_amd/csrc/plsa_lda_online_kernels.hpp: the geometry of plsa_online_plan.hpp,
// the pad mask of plsa_smoothed_plan.hpp) beside that of k_lda_topic_partial (plsa_lda_plan.hpp), whose slab partials it
// replaces, on a CPU; tests/test_lda_online_plan_host.py builds this with the sanitizers and feeds the cases.
//
// stdin, one call per line; stdout, one line of results per call:
//     blend m kp k -> grid n4 walked slabs_same strands_same mask_ok
// A table is [m, kp] float32: n4 = m * kp / 4 float4s.  grid: workgroups (= slabs).  walked: the kernel's loops -- four rows in
// flight, then the rest -- run literally for every thread of every workgroup over a bitmap of n4 places taken from the heap:
// 1 when every place was visited exactly once, by one lane, and none outside.  slabs_same: blend_grid(m) == lda_bound_grid(m),
// and every slab's blend_rows_first / blend_rows_last are prior_rows_first / prior_rows_last.  strands_same: for every slab,
// every column z and every strand r of its sweep, the rows the owning blend lane visits are, in order, the rows
// k_lda_topic_partial's thread (z - zb) + r * span adds (w = first + r, + rpp, ... below last), and the place a lane leaves its
// strand sum in the workgroup's array is the place that kernel's second half reads for (z, r).  mask_ok: bit j of the lane's
// pad mask is set exactly when column 4 q + j < k, for every active lane.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../enstop_amd/csrc/plsa_lda_plan.hpp"
#include "../enstop_amd/csrc/plsa_online_plan.hpp"

namespace plan = plsa::plan;

int main() {
    char name[32];
    long long m, kp, k;
    while (std::scanf("%31s %lld %lld %lld", name, &m, &kp, &k) == 4) {
        if (std::strcmp(name, "blend")) { std::fprintf(stderr, "unknown call: %s\n", name); return 2; }
        if (kp <= 0 || kp % 4 || kp > plan::BLEND_MAX_KP || k < 1 || k > kp) { std::fprintf(stderr, "bad kp / k\n"); return 2; }
        const int grid = plan::blend_grid(m);
        const int kq = (int)kp / 4;
        const int64_t n4 = (int64_t)m * kq;
        const size_t words = (size_t)((n4 + 63) / 64);
        std::unique_ptr<uint64_t[]> seen(new uint64_t[words]());      // exactly the places of the table
        bool once = true, slabs_same = grid == plan::lda_bound_grid(m), strands_same = true, mask_ok = true;
        // the lane that owns (float4 column, strand), or -1
        std::vector<int> owner((size_t)kq * 256, -1);
        for (unsigned t = 0; t < (unsigned)plan::BLEND_BLOCK; ++t) {
            const plan::BlendLane l = plan::blend_lane((int)kp, t);
            if (!l.active) continue;
            int &o = owner[(size_t)l.q * 256 + l.strand];
            once = once && o < 0;
            o = (int)t;
            const unsigned mask = plan::smooth_pad_mask(l.q, (int)k);
            for (int j = 0; j < 4; ++j) mask_ok = mask_ok && (((mask >> j) & 1u) != 0) == (4 * l.q + j < k);
            mask_ok = mask_ok && mask < 16u;
        }
        for (int b = 0; b < grid; ++b) {
            const int64_t first_row = plan::blend_rows_first(m, (unsigned)grid, (unsigned)b);
            const int64_t last_row = plan::blend_rows_last(m, (unsigned)grid, (unsigned)b);
            slabs_same = slabs_same && first_row == plan::prior_rows_first(m, (unsigned)grid, (unsigned)b) &&
                         last_row == plan::prior_rows_last(m, (unsigned)grid, (unsigned)b);
            for (unsigned t = 0; t < (unsigned)plan::BLEND_BLOCK; ++t) {
                const plan::BlendLane l = plan::blend_lane((int)kp, t);
                if (!l.active) continue;
                const int64_t end = plan::blend_end(last_row, kq), stride = plan::blend_stride(kq, l);
                int64_t i = plan::blend_first(first_row, kq, l);
                auto visit = [&](int64_t at) {
                    if (at < 0 || at >= n4) { once = false; return; }
                    uint64_t &w = seen[(size_t)(at >> 6)];
                    const uint64_t bit = 1ull << (at & 63);
                    once = once && !(w & bit);
                    w |= bit;
                };
                // the kernel's two loops
                for (; i + 3 * stride < end; i += 4 * stride) { visit(i); visit(i + stride); visit(i + 2 * stride); visit(i + 3 * stride); }
                for (; i < end; i += stride) visit(i);
            }
            // k_lda_topic_partial's loops for this slab, column by column and strand by strand, beside the owning lane's
            for (int zb = 0; zb < kp && strands_same; zb += 256) {
                const int span = (int)kp - zb < 256 ? (int)kp - zb : 256, rpp = 256 / span;
                for (int thread = 0; thread < 256 && strands_same; ++thread) {
                    const int z = zb + thread % span, ro = thread / span;
                    if (ro >= rpp) continue;
                    const int t = owner[(size_t)(z / 4) * 256 + ro];
                    if (t < 0) { strands_same = false; break; }
                    const plan::BlendLane l = plan::blend_lane((int)kp, (unsigned)t);
                    // where the lane leaves the sum of column z and where the second half reads strand ro of column z
                    const int left = l.strand * l.span + 4 * (l.q - l.sweep * 64) + z % 4, read = ro * span + z - zb;
                    strands_same = strands_same && l.sweep == zb / 256 && l.q == z / 4 && l.strand == ro && left == read && left < 256;
                    const int64_t end = plan::blend_end(last_row, kq), stride = plan::blend_stride(kq, l);
                    int64_t i = plan::blend_first(first_row, kq, l);
                    for (int64_t w = first_row + ro; w < last_row; w += rpp, i += stride)
                        strands_same = strands_same && i < end && i == w * kq + z / 4;
                    strands_same = strands_same && i >= end;          // the lane visits no row beyond them
                }
            }
        }
        for (size_t w = 0; w < words && once; ++w) {
            const int64_t left = n4 - (int64_t)w * 64;
            once = seen[w] == (left >= 64 ? ~0ull : (1ull << left) - 1);
        }
        std::printf("%d %lld %d %d %d %d\n", grid, (long long)n4, once ? 1 : 0, slabs_same ? 1 : 0, strands_same ? 1 : 0,
                    mask_ok ? 1 : 0);
    }
    return 0;
}
