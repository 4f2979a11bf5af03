// plsa_online_plan.hpp -- the launch arithmetic of k_online_blend (plsa_online_kernels.hpp), free of HIP like
// plsa_tempered_plan.hpp: plain values in, plain values out.  The kernel takes its lane, its first index, its stride and its
// bound from here, the host takes the grid from here, and tests/online_plan_host.cpp walks the same functions on a CPU.
//
// A table is [m, kp] float32 with kp a multiple of 4 and at most 1024, so a row is kq = kp / 4 float4s and the table
// n4 = m * kq of them, counted in 64 bits.  The blend also leaves the float64 column sums of what it writes, slab by slab, in
// the order colsum_slab_body (plsa_kernels.hpp) adds them, so its work is cut the way that body cuts it:
//   slab s of n_slabs = min(256, max(m, 1)) owns the rows [s * per, min(m, (s + 1) * per)), per = ceil(m / n_slabs);
//   the columns go in sweeps of 256: sweep v covers the columns [256 v, 256 v + span), span = min(256, kp - 256 v), and adds
//   rpp = 256 / span interleaved strands of rows (strand r: the slab's rows first + r, first + r + rpp, ...);
//   there a thread owns one column of one strand; here a lane owns FOUR adjacent columns of one strand (one float4 per row),
//   so a sweep has (span / 4) * rpp <= 64 lanes: wave v of the 256-thread workgroup runs sweep v.
// Lane (v, item): float4 column q = 64 v + item % (span / 4) of the row, strand r = item / (span / 4).  It visits the float4s
// (first + r) * kq + q, stepping rpp * kq, below last * kq: every float4 of the slab once, every strand in row order.
#pragma once

#include <algorithm>
#include <cstdint>

namespace plsa {
namespace plan {

constexpr int BLEND_BLOCK = 256;
constexpr int BLEND_SLABS = 256;       // = NORM_BLOCKS of plsa_kernels.hpp (asserted where both are visible)
constexpr int BLEND_MAX_KP = 1024;     // four sweeps, one per wave of the workgroup

// workgroups = slabs for a table of m rows, at least one (an empty table is a launch that does nothing)
inline int blend_grid(int64_t m) { return (int)std::min<int64_t>(BLEND_SLABS, std::max<int64_t>(m, 1)); }

#if defined(__HIPCC__)
#define PLSA_ONLINE_HD __host__ __device__
#else
#define PLSA_ONLINE_HD
#endif

struct BlendLane {
    int active;     // 0: the lane owns nothing (its sweep does not exist, or has fewer lanes)
    int sweep;      // which 256 columns
    int span, rpp;  // columns of the sweep, strands of rows
    int q;          // float4 column of the row, 0 .. kq - 1
    int strand;     // 0 .. rpp - 1
};

PLSA_ONLINE_HD inline BlendLane blend_lane(int kp, unsigned thread) {
    BlendLane l = {0, (int)(thread / 64), 0, 0, 0, 0};
    const int zb = l.sweep * 256, item = (int)(thread % 64);
    if (zb >= kp) return l;
    l.span = kp - zb < 256 ? kp - zb : 256;
    l.rpp = 256 / l.span;
    const int sq = l.span / 4;
    if (item >= sq * l.rpp) return l;
    l.active = 1;
    l.q = zb / 4 + item % sq;
    l.strand = item / sq;
    return l;
}

// rows [first, last) of slab `slab` (last <= first: none)
PLSA_ONLINE_HD inline int64_t blend_rows_first(int64_t m, unsigned n_slabs, unsigned slab) {
    return (int64_t)slab * ((m + n_slabs - 1) / n_slabs);
}
PLSA_ONLINE_HD inline int64_t blend_rows_last(int64_t m, unsigned n_slabs, unsigned slab) {
    const int64_t per = (m + n_slabs - 1) / n_slabs, last = (int64_t)slab * per + per;
    return last < m ? last : m;
}

// the lane's loop over float4 indices: for (i = first; i < end; i += stride)
PLSA_ONLINE_HD inline int64_t blend_first(int64_t row_first, int kq, const BlendLane &l) { return (row_first + l.strand) * kq + l.q; }
PLSA_ONLINE_HD inline int64_t blend_stride(int kq, const BlendLane &l) { return (int64_t)l.rpp * kq; }
PLSA_ONLINE_HD inline int64_t blend_end(int64_t row_last, int kq) { return row_last * kq; }
#undef PLSA_ONLINE_HD

}  // namespace plan
}  // namespace plsa
