// plsa_tempered_kernels.hpp -- the one kernel of tempered EM (include/plsa_hip_tempered.h).
//
// The tempered responsibility P_beta(z|d,w) ~ (P(z|d) P(w|z))^beta factorises into P(z|d)^beta * P(w|z)^beta, so a tempered
// iteration is the ordinary fused iteration on two side tables that hold the factors raised to the power beta: k (n + m)
// powers per iteration here instead of 2 nnz k inside the passes, which stay as they are.
#pragma once

#include "plsa_tempered_plan.hpp"

namespace plsa {

// x^beta, rounded once: the float64 pow is good to a few float64 ulp, so the float32 it rounds to is within 1 float32 ulp of
// float32(pow of the exact arithmetic) -- and of any other float64 pow of that quality.  Exact zeros (and the pad columns
// k..kp, which are zeros) stay exact zeros; a negative or NaN entry, which no factor holds, gives 0 as well.  Denormal
// inputs and results are kept: the conversions honour the float32 denormal mode the library is built with.
__device__ __forceinline__ float temper_one(float x, double beta) { return x > 0.f ? (float)pow((double)x, beta) : 0.f; }

// out[i] = in[i]^beta over a [rows, kp] float32 table seen as n4 float4s; grid-stride, geometry from plan::temper_*
__global__ __launch_bounds__(256) void k_temper(const float4 *__restrict__ in, float4 *__restrict__ out, long long n4, double beta) {
    const long long stride = plan::temper_stride(gridDim.x);
    for (long long i = plan::temper_first(blockIdx.x, threadIdx.x); i < n4; i += stride) {
        float4 v = in[i];
        v.x = temper_one(v.x, beta);
        v.y = temper_one(v.y, beta);
        v.z = temper_one(v.z, beta);
        v.w = temper_one(v.w, beta);
        out[i] = v;
    }
}

}  // namespace plsa
