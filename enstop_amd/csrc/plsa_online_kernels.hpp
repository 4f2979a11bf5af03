// plsa_online_kernels.hpp -- the one kernel of online (stepwise) EM (include/plsa_hip_online.h).
//
// The global update of a step blends the block's un-normalised P(w|z) sums into the running statistic and normalises the
// result: S' = b * Vacc + a * S, norm[z] = sum_w S'[w, z], V' = S' / norm.  k_online_blend does the first two parts in one
// sweep over S and Vacc (3 m kp 4 bytes: two reads, one write): it writes S' in place and the per-slab float64 column sums of
// S' in the layout, and with the additions, of k_colsum_partial over S' -- so k_colsum_final and k_v_normalise follow
// unchanged, and a step at a = 0, b = 1 leaves the bits of plsa_em_finish.
#pragma once

#include "plsa_online_plan.hpp"

namespace plsa {

static_assert(plan::BLEND_SLABS == NORM_BLOCKS, "the blend's slabs are the slabs of k_colsum_partial");

// one rounding for a * s, one for the fused multiply-add: round32(b * acc + round32(a * s))
__device__ __forceinline__ float blend_one(float s, float acc, float a, float b) { return fmaf(b, acc, __fmul_rn(a, s)); }

__device__ __forceinline__ float4 blend_four(const float4 &s, const float4 &acc, float a, float b, float4 &sum) {
    float4 r;
    r.x = blend_one(s.x, acc.x, a, b);
    r.y = blend_one(s.y, acc.y, a, b);
    r.z = blend_one(s.z, acc.z, a, b);
    r.w = blend_one(s.w, acc.w, a, b);
    sum.x += r.x; sum.y += r.y; sum.z += r.z; sum.w += r.w;      // the strand's float32 sum, in row order
    return r;
}

// S [m, kp] <- b * acc + a * S, and partials [gridDim.x, kp] <- float64 column sums of the new S per slab; one workgroup per
// slab, geometry from plan::blend_*.  S is read and written through the same pointer (each float4 by one lane only).
__global__ __launch_bounds__(256) void k_online_blend(float4 *S, const float4 *__restrict__ acc, long long m, int kp, float a,
                                                      float b, double *__restrict__ partials) {
    __shared__ double sred[plan::BLEND_MAX_KP / 256][256];
    const int kq = kp / 4;
    const plan::BlendLane lane = plan::blend_lane(kp, threadIdx.x);
    if (lane.active) {
        const long long end = plan::blend_end(plan::blend_rows_last(m, gridDim.x, blockIdx.x), kq);
        const long long stride = plan::blend_stride(kq, lane);
        long long i = plan::blend_first(plan::blend_rows_first(m, gridDim.x, blockIdx.x), kq, lane);
        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
        // four rows in flight: the loads of a batch are issued before its first store (S may not be declared restrict)
        for (; i + 3 * stride < end; i += 4 * stride) {
            const float4 s0 = S[i], s1 = S[i + stride], s2 = S[i + 2 * stride], s3 = S[i + 3 * stride];
            const float4 v0 = acc[i], v1 = acc[i + stride], v2 = acc[i + 2 * stride], v3 = acc[i + 3 * stride];
            S[i] = blend_four(s0, v0, a, b, sum);
            S[i + stride] = blend_four(s1, v1, a, b, sum);
            S[i + 2 * stride] = blend_four(s2, v2, a, b, sum);
            S[i + 3 * stride] = blend_four(s3, v3, a, b, sum);
        }
        for (; i < end; i += stride) S[i] = blend_four(S[i], acc[i], a, b, sum);
        double *row = &sred[lane.sweep][lane.strand * lane.span + 4 * (lane.q - lane.sweep * 64)];
        row[0] = (double)sum.x; row[1] = (double)sum.y; row[2] = (double)sum.z; row[3] = (double)sum.w;
    }
    __syncthreads();
    // the strands of a column, added in strand order (colsum_slab_body's second half)
    for (int z = threadIdx.x; z < kp; z += 256) {
        const int sweep = z / 256, zb = sweep * 256;
        const int span = min(256, kp - zb), rpp = 256 / span;
        double tot = 0.0;
        for (int r = 0; r < rpp; ++r) tot += sred[sweep][r * span + z - zb];
        partials[(long long)blockIdx.x * kp + z] = tot;
    }
}

}  // namespace plsa
