// The launch arithmetic of enstop_amd/csrc/plsa_launch_plan.hpp on a CPU (tests/test_launch_plan_host.py builds this with the
// sanitizers, feeds the cases and compares with values that come from elsewhere).
//
// stdin, one call per line; stdout, one line of results per call:
//     lane_shape k chunks_per_lane row_shape_8x2            -> kp lpn ch row_lpn row_ch
//     row_items n nnz cus row_lpn ritems_mode rseg_override -> use seg
//     col_item_len nnz cus lpn seg_override                 -> seg
//     order_band kp knob                                    -> documents per band
//     grid_for work per_block cap                           -> grid
//     row_pass n n_ritems items row_lpn grid_cap xcd_rows   -> grid reduce_grid
//     col_pass n_items m lpn n_heavy grid_cap               -> n_chunks reduce_grid norm_blocks
//     xcd_split knob n_chunks n kp                          -> 0 | 1
//     balance n_chunks frac[0..9) (hex floats)              -> lo[0..9) split_grid unsplit_grid
//     table_is_wide rows kp force                           -> 0 | 1
//     sort_bits count                                       -> bits
//     order_key n band                                      -> len_bits key_bits
//     e_item_len lpn override                               -> entries per piece
//     packed_ok nnz id_range escaped                        -> 0 | 1
//     xcd_times grid stamps[0..grid]                        -> us[0..8) spread (hex floats)
//     balance_step frac[0..9) us[0..8) (hex floats)         -> next frac[0..9) (hex floats)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../enstop_amd/csrc/plsa_launch_plan.hpp"

namespace plan = plsa::plan;

int main() {
    char name[32];
    long long a, b, c, d, e, f;
    while (std::scanf("%31s", name) == 1) {
        auto args = [&](int count) {
            long long *v[6] = {&a, &b, &c, &d, &e, &f};
            for (int i = 0; i < count; ++i)
                if (std::scanf("%lld", v[i]) != 1) { std::fprintf(stderr, "bad case: %s\n", name); std::abort(); }
        };
        if (!std::strcmp(name, "lane_shape")) {
            args(3);
            const plan::LaneShape s = plan::lane_shape((int)a, (int)b, c != 0);
            std::printf("%d %d %d %d %d\n", s.kp, s.lpn, s.ch, s.row_lpn, s.row_ch);
        } else if (!std::strcmp(name, "row_items")) {
            args(6);
            const plan::RowItems r = plan::row_items(a, b, (int)c, (int)d, (int)e, (int)f);
            std::printf("%d %d\n", r.use ? 1 : 0, r.seg);
        } else if (!std::strcmp(name, "col_item_len")) {
            args(4);
            std::printf("%d\n", plan::col_item_len(a, (int)b, (int)c, (int)d));
        } else if (!std::strcmp(name, "order_band")) {
            args(2);
            std::printf("%d\n", plan::order_band((int)a, (int)b));
        } else if (!std::strcmp(name, "grid_for")) {
            args(3);
            std::printf("%d\n", plan::grid_for(a, (int)b, (int)c));
        } else if (!std::strcmp(name, "row_pass")) {
            args(6);
            const plan::RowPass r = plan::row_pass(a, b, c != 0, (int)d, (int)e, f != 0);
            std::printf("%d %d\n", r.grid, r.reduce_grid);
        } else if (!std::strcmp(name, "col_pass")) {
            args(5);
            const plan::ColPass p = plan::col_pass(a, b, (int)c, (int)d, (int)e);
            std::printf("%d %d %d\n", p.n_chunks, p.reduce_grid, p.norm_blocks);
        } else if (!std::strcmp(name, "xcd_split")) {
            args(4);
            std::printf("%d\n", plan::xcd_split(a != 0, (int)b, c, (int)d) ? 1 : 0);
        } else if (!std::strcmp(name, "balance")) {
            args(1);
            // exactly nine places each, from the heap: a step past them is the address sanitizer's to see
            std::unique_ptr<double[]> frac(new double[9]);
            std::unique_ptr<int[]> lo(new int[9]);
            for (int x = 0; x < 9; ++x) {
                char text[64];
                if (std::scanf("%63s", text) != 1) { std::fprintf(stderr, "bad case: balance\n"); std::abort(); }
                frac[x] = std::strtod(text, nullptr);
            }
            plan::balance_lo(frac.get(), (int)a, lo.get());
            for (int x = 0; x < 9; ++x) std::printf("%d ", lo[x]);
            std::printf("%d %d\n", plan::col_grid(lo.get(), (int)a, true), plan::col_grid(lo.get(), (int)a, false));
        } else if (!std::strcmp(name, "sort_bits")) {
            args(1);
            std::printf("%d\n", plan::sort_bits(a));
        } else if (!std::strcmp(name, "order_key")) {
            args(2);
            const plan::OrderKey k = plan::order_key(a, (int)b);
            std::printf("%d %d\n", k.len_bits, k.key_bits);
        } else if (!std::strcmp(name, "e_item_len")) {
            args(2);
            std::printf("%d\n", plan::e_item_len((int)a, (int)b));
        } else if (!std::strcmp(name, "packed_ok")) {
            args(3);
            std::printf("%d\n", plan::packed_ok(a, b, (uint64_t)c) ? 1 : 0);
        } else if (!std::strcmp(name, "xcd_times")) {
            args(1);
            // exactly grid + 1 stamps, from the heap
            std::unique_ptr<unsigned long long[]> stamps(new unsigned long long[(size_t)a + 1]);
            for (long long i = 0; i <= a; ++i)
                if (std::scanf("%llu", &stamps[(size_t)i]) != 1) { std::fprintf(stderr, "bad case: xcd_times\n"); std::abort(); }
            const plan::XcdTimes t = plan::xcd_times(stamps.get(), (int)a);
            for (int x = 0; x < 8; ++x) std::printf("%a ", t.us[x]);
            std::printf("%a\n", t.spread);
        } else if (!std::strcmp(name, "balance_step")) {
            std::unique_ptr<double[]> frac(new double[9]), us(new double[8]), next(new double[9]);
            for (int x = 0; x < 17; ++x) {
                char text[64];
                if (std::scanf("%63s", text) != 1) { std::fprintf(stderr, "bad case: balance_step\n"); std::abort(); }
                (x < 9 ? frac[x] : us[x - 9]) = std::strtod(text, nullptr);
            }
            plan::balance_step(frac.get(), us.get(), next.get());
            for (int x = 0; x < 9; ++x) std::printf("%a%c", next[x], x < 8 ? ' ' : '\n');
        } else if (!std::strcmp(name, "table_is_wide")) {
            args(3);
            std::printf("%d\n", plan::table_is_wide(a, (int)b, c != 0) ? 1 : 0);
        } else {
            std::fprintf(stderr, "unknown call: %s\n", name);
            return 2;
        }
    }
    return 0;
}
