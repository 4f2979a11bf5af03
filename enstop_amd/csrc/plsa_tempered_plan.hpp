// plsa_tempered_plan.hpp -- the launch arithmetic of k_temper (plsa_tempered_kernels.hpp), free of HIP like
// plsa_launch_plan.hpp: plain values in, plain values out.  The kernel takes its first index and its stride from here, the
// host takes the grid from here, and tests/tempered_plan_host.cpp walks the same three functions on a CPU.
//
// A table is [rows, kp] float32 with kp a multiple of 4, so it is n4 = rows * kp / 4 float4s, counted in 64 bits: a table of
// 2^31 floats and more is legal (the wide passes gather from such tables).  Thread t of the launch (t = block * 256 + lane,
// T = grid * 256 threads) handles the float4s t, t + T, t + 2T, ... below n4: the residue classes modulo T, each float4 once.
#pragma once

#include <algorithm>
#include <cstdint>

namespace plsa {
namespace plan {

constexpr int TEMPER_BLOCK = 256;

// workgroups for n4 float4s, at least one (an empty table is a launch that does nothing), at most grid_cap
inline int temper_grid(int64_t n4, int grid_cap) {
    int64_t need = (n4 + TEMPER_BLOCK - 1) / TEMPER_BLOCK;
    if (need < 1) need = 1;
    return (int)std::min<int64_t>(need, std::max(1, grid_cap));
}

#if defined(__HIPCC__)
#define PLSA_TEMPER_HD __host__ __device__
#else
#define PLSA_TEMPER_HD
#endif
PLSA_TEMPER_HD inline int64_t temper_first(unsigned block, unsigned lane) { return (int64_t)block * TEMPER_BLOCK + lane; }
PLSA_TEMPER_HD inline int64_t temper_stride(unsigned grid) { return (int64_t)grid * TEMPER_BLOCK; }
#undef PLSA_TEMPER_HD

}  // namespace plan
}  // namespace plsa
