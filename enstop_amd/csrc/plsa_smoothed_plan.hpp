// plsa_smoothed_plan.hpp -- the launch arithmetic of the three kernels of smoothed (MAP) EM (plsa_smoothed_kernels.hpp), free
// of HIP like plsa_tempered_plan.hpp: plain values in, plain values out.  The kernels take their first index, their stride,
// their positions and their pad masks from here, the host takes the grids from here, and tests/smoothed_plan_host.cpp walks
// the same functions on a CPU.
//
// A table is [rows, kp] float32 with kp a multiple of 4, so a row is kq = kp / 4 float4s ("quarters" 0 .. kq - 1) and the
// table n4 = rows * kq of them, counted in 64 bits: a table of 2^31 floats and more is legal.
//
// k_smooth_rows, k_smooth_topics: thread t of the launch (t = block * 256 + lane, T = grid * 256 threads) handles the float4s
// t, t + T, t + 2T, ... below n4 -- the residue classes modulo T, each float4 once.  A float4 index i sits in row i / kq at
// quarter i % kq; a lane divides once (smooth_pos) and then walks: a step of T float4s is T / kq rows and T % kq quarters,
// with one carry (smooth_advance).  Quarter q holds the topics 4 q .. 4 q + 3; of those, the ones below k are live (bit j of
// smooth_pad_mask: topic 4 q + j < k), the rest are padding and stay exactly 0.
//
// k_log_prior: a fixed number of slabs of whole rows, each owning one float64 partial -- slab s of
// n_slabs = min(256, max(rows, 1)) owns the rows [s * per, min(rows, (s + 1) * per)), per = ceil(rows / n_slabs), the cut of
// k_colsum_partial.  Thread t of the slab's workgroup handles the slab's float4s t, t + 256, ...: the grid is the slab count
// whatever the context's grid cap is, so the partials, and the sum k_ll_final forms of them, do not depend on it.
#pragma once

#include <algorithm>
#include <cstdint>

namespace plsa {
namespace plan {

constexpr int SMOOTH_BLOCK = 256;
constexpr int PRIOR_SLABS = 256;       // = NORM_BLOCKS of plsa_kernels.hpp (asserted where both are visible)

// workgroups for n4 float4s, at least one (an empty table is a launch that does nothing), at most grid_cap
inline int smooth_grid(int64_t n4, int grid_cap) {
    int64_t need = (n4 + SMOOTH_BLOCK - 1) / SMOOTH_BLOCK;
    if (need < 1) need = 1;
    return (int)std::min<int64_t>(need, std::max(1, grid_cap));
}

// workgroups = slabs of k_log_prior for a table of `rows` rows, at least one
inline int prior_grid(int64_t rows) { return (int)std::min<int64_t>(PRIOR_SLABS, std::max<int64_t>(rows, 1)); }

#if defined(__HIPCC__)
#define PLSA_SMOOTH_HD __host__ __device__
#else
#define PLSA_SMOOTH_HD
#endif

PLSA_SMOOTH_HD inline int64_t smooth_first(unsigned block, unsigned lane) { return (int64_t)block * SMOOTH_BLOCK + lane; }
PLSA_SMOOTH_HD inline int64_t smooth_stride(unsigned grid) { return (int64_t)grid * SMOOTH_BLOCK; }

struct SmoothPos {
    int64_t row;    // i / kq
    int q;          // i % kq
};
struct SmoothStep {
    int64_t rows;   // stride / kq
    int q;          // stride % kq
};

PLSA_SMOOTH_HD inline SmoothPos smooth_pos(int64_t i, int kq) {
    const int64_t row = i / kq;
    return SmoothPos{row, (int)(i - row * kq)};
}
PLSA_SMOOTH_HD inline SmoothStep smooth_step(int64_t stride, int kq) {
    const int64_t rows = stride / kq;
    return SmoothStep{rows, (int)(stride - rows * kq)};
}
// the position `s` further on: p.q and s.q are both below kq, so one carry is all there can be
PLSA_SMOOTH_HD inline SmoothPos smooth_advance(const SmoothPos &p, const SmoothStep &s, int kq) {
    SmoothPos r{p.row + s.rows, p.q + s.q};
    if (r.q >= kq) { r.q -= kq; ++r.row; }
    return r;
}

// bit j set: topic 4 q + j is one of the k real topics
PLSA_SMOOTH_HD inline unsigned smooth_pad_mask(int q, int k) {
    int live = k - 4 * q;
    live = live < 0 ? 0 : (live > 4 ? 4 : live);
    return (1u << live) - 1u;
}

// rows [first, last) of slab `slab` of k_log_prior (last <= first: none)
PLSA_SMOOTH_HD inline int64_t prior_rows_first(int64_t rows, unsigned n_slabs, unsigned slab) {
    return (int64_t)slab * ((rows + n_slabs - 1) / n_slabs);
}
PLSA_SMOOTH_HD inline int64_t prior_rows_last(int64_t rows, unsigned n_slabs, unsigned slab) {
    const int64_t per = (rows + n_slabs - 1) / n_slabs, last = (int64_t)slab * per + per;
    return last < rows ? last : rows;
}
#undef PLSA_SMOOTH_HD

}  // namespace plan
}  // namespace plsa
