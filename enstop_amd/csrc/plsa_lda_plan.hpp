// plsa_lda_plan.hpp -- the launch arithmetic of the kernels of variational Bayes LDA (plsa_lda_kernels.hpp), free of HIP like
// plsa_smoothed_plan.hpp, on which it stands: plain values in, plain values out.  The kernels take their indices from here,
// the host takes the grids from here, and tests/lda_plan_host.cpp walks the same functions on a CPU.
//
// Tables are the tables of plsa_smoothed_plan.hpp: [rows, kp] float32, kq = kp / 4 float4s ("quarters") per row, n4 = rows * kq
// float4s counted in 64 bits, the topics 4 q .. 4 q + 3 of quarter q live where smooth_pad_mask says so.
//
// k_lda_tables, k_lda_rows, k_lda_topics: the grid-stride walk of k_smooth_rows (smooth_first, smooth_stride, smooth_pos,
// smooth_advance) on lda_grid(n4, grid_cap) workgroups -- every float4 once, whatever the cap.
//
// k_lda_rowsum, k_lda_wordmax: one float64 sum (one maximum) per row.  A row is summed by a group of lda_row_lanes(kq) lanes, the smallest power of two
// that is >= kq and at most 64 (a group never leaves its wavefront): lane l adds the quarters l, l + lanes, ... in that
// order, each quarter x + y + z + w, and the lanes' sums are added by a butterfly over the group.  The order is a function of
// kq alone.  A workgroup holds 256 / lanes groups; group g of workgroup b sums the rows b * groups + g, + grid * groups, ...
//
// k_lda_topic_sums: a workgroup holds 256 / LDA_TOPIC_LANES topics; lane l of a topic adds its slab partials l, l + 16, ... in
// that order, and the 16 lane sums are added in lane order: an order that depends on the number of partials alone.
//
// k_lda_bound, k_lda_topic_partial: the slabs of k_log_prior (prior_grid, prior_rows_first, prior_rows_last) over the rows of
// their table: never a function of the grid cap.  k_lda_shift_sum: the same cut of the documents into lda_shift_grid(n) slabs,
// LDA_SHIFT_SLABS at the most -- it walks the corpus' entries, not a table, and 256 workgroups leave the chip idle there.
#pragma once

#include "plsa_smoothed_plan.hpp"

namespace plsa {
namespace plan {

constexpr int LDA_BLOCK = SMOOTH_BLOCK;
constexpr int LDA_WAVE = 64;
constexpr int LDA_TOPIC_LANES = 16;
constexpr int LDA_SHIFT_SLABS = 4096;

inline int lda_grid(int64_t n4, int grid_cap) { return smooth_grid(n4, grid_cap); }
inline int lda_bound_grid(int64_t rows) { return prior_grid(rows); }
inline int lda_topic_grid(int kp) { return std::max(1, (kp * LDA_TOPIC_LANES + LDA_BLOCK - 1) / LDA_BLOCK); }
inline int lda_shift_grid(int64_t rows) { return (int)std::min<int64_t>(LDA_SHIFT_SLABS, std::max<int64_t>(rows, 1)); }

#if defined(__HIPCC__)
#define PLSA_LDA_PLAN_HD __host__ __device__
#else
#define PLSA_LDA_PLAN_HD
#endif

// lanes that sum one row of kq quarters: the smallest power of two >= kq, at most one wavefront
PLSA_LDA_PLAN_HD inline int lda_row_lanes(int kq) {
    int lanes = 1;
    while (lanes < kq && lanes < LDA_WAVE) lanes *= 2;
    return lanes;
}
PLSA_LDA_PLAN_HD inline int lda_row_groups(int lanes) { return LDA_BLOCK / lanes; }
// first row of group `group` of workgroup `block`, and the distance to its next one
PLSA_LDA_PLAN_HD inline int64_t lda_row_first(unsigned block, int group, int lanes) {
    return (int64_t)block * lda_row_groups(lanes) + group;
}
PLSA_LDA_PLAN_HD inline int64_t lda_row_stride(unsigned grid, int lanes) { return (int64_t)grid * lda_row_groups(lanes); }
#undef PLSA_LDA_PLAN_HD

// workgroups of k_lda_rowsum: one group per row, one workgroup at least, the cap at most
inline int lda_rowsum_grid(int64_t rows, int kq, int grid_cap) {
    const int groups = lda_row_groups(lda_row_lanes(kq));
    int64_t need = (rows + groups - 1) / groups;
    if (need < 1) need = 1;
    return (int)std::min<int64_t>(need, std::max(1, grid_cap));
}

}  // namespace plan
}  // namespace plsa
