// plsa_lda_online_kernels.hpp -- the one kernel of online variational Bayes LDA (enstop_amd/include/plsa_hip_lda_online.h,
// DESIGN.md section 21).
//
// The global update of a step blends the block's raw counts into lambda and forms the tables of the result:
// lambda' = b * Vacc + (a * lambda + c) over the topics below k, 0 at the pads, then S_z = sum_w lambda'[w, z] and the table B.
// k_lda_online_blend does the blend and the first half of the sums in one sweep over lambda and Vacc (3 m kp 4 bytes: two
// reads, one write): it writes lambda' in place and the per-slab float64 column sums of lambda' in the layout, and with the
// additions, of k_lda_topic_partial over lambda' -- so k_lda_topic_sums, k_lda_wordmax and k_lda_tables follow unchanged, the
// sweep of k_lda_topic_partial is never launched, and a step at a = 0, b = 1 leaves the bits of an iteration of plsa_lda_fit.
//
// The geometry is k_online_blend's (plan::blend_*, plsa_online_plan.hpp): one workgroup per slab, a lane owns four adjacent
// columns of one strand of the slab's rows.  Its slabs are the slabs of k_lda_topic_partial (plan::prior_rows_*, the same
// cut) and its strands are that kernel's: tests/lda_online_plan_host.cpp walks both on a CPU.
#pragma once

#include "plsa_lda_plan.hpp"
#include "plsa_online_plan.hpp"

namespace plsa {

static_assert(plan::BLEND_SLABS == plan::PRIOR_SLABS && plan::BLEND_BLOCK == plan::LDA_BLOCK,
              "the blend's slabs are the slabs of k_lda_topic_partial");

// one rounding for a * lam + c, one for the second fused multiply-add: round32(b * acc + round32(a * lam + c))
__device__ __forceinline__ float lda_blend_one(float lam, float acc, float a, float b, float c) { return fmaf(b, acc, fmaf(a, lam, c)); }

// the live topics of one quarter blended, the pads exact 0; the strand's float64 sums, in row order
__device__ __forceinline__ float4 lda_blend_four(const float4 &lam, const float4 &acc, float a, float b, float c, unsigned mask,
                                                 double &s0, double &s1, double &s2, double &s3) {
    float4 r;
    r.x = (mask & 1u) ? lda_blend_one(lam.x, acc.x, a, b, c) : 0.f;
    r.y = (mask & 2u) ? lda_blend_one(lam.y, acc.y, a, b, c) : 0.f;
    r.z = (mask & 4u) ? lda_blend_one(lam.z, acc.z, a, b, c) : 0.f;
    r.w = (mask & 8u) ? lda_blend_one(lam.w, acc.w, a, b, c) : 0.f;
    s0 += (double)r.x; s1 += (double)r.y; s2 += (double)r.z; s3 += (double)r.w;
    return r;
}

// L [m, kp] <- b * acc + (a * L + c) over the topics below k (0 at the pads), and partials [gridDim.x, kp] <- float64 column
// sums of the new L per slab; one workgroup per slab, geometry from plan::blend_*.  L is read and written through the same
// pointer (each float4 by one lane only).
__global__ __launch_bounds__(256) void k_lda_online_blend(float4 *L, const float4 *__restrict__ acc, long long m, int kp, int k,
                                                          float a, float b, float c, double *__restrict__ partials) {
    __shared__ double sred[plan::BLEND_MAX_KP / 256][256];
    const int kq = kp / 4;
    const plan::BlendLane lane = plan::blend_lane(kp, threadIdx.x);
    if (lane.active) {
        const long long end = plan::blend_end(plan::blend_rows_last(m, gridDim.x, blockIdx.x), kq);
        const long long stride = plan::blend_stride(kq, lane);
        long long i = plan::blend_first(plan::blend_rows_first(m, gridDim.x, blockIdx.x), kq, lane);
        const unsigned mask = plan::smooth_pad_mask(lane.q, k);      // a lane stays in its quarter
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        // four rows in flight: the loads of a batch are issued before its first store (L may not be declared restrict)
        for (; i + 3 * stride < end; i += 4 * stride) {
            const float4 l0 = L[i], l1 = L[i + stride], l2 = L[i + 2 * stride], l3 = L[i + 3 * stride];
            const float4 v0 = acc[i], v1 = acc[i + stride], v2 = acc[i + 2 * stride], v3 = acc[i + 3 * stride];
            L[i] = lda_blend_four(l0, v0, a, b, c, mask, s0, s1, s2, s3);
            L[i + stride] = lda_blend_four(l1, v1, a, b, c, mask, s0, s1, s2, s3);
            L[i + 2 * stride] = lda_blend_four(l2, v2, a, b, c, mask, s0, s1, s2, s3);
            L[i + 3 * stride] = lda_blend_four(l3, v3, a, b, c, mask, s0, s1, s2, s3);
        }
        for (; i < end; i += stride) L[i] = lda_blend_four(L[i], acc[i], a, b, c, mask, s0, s1, s2, s3);
        double *row = &sred[lane.sweep][lane.strand * lane.span + 4 * (lane.q - lane.sweep * 64)];
        row[0] = s0; row[1] = s1; row[2] = s2; row[3] = s3;
    }
    __syncthreads();
    // the strands of a column, added in strand order (k_lda_topic_partial's second half)
    for (int z = threadIdx.x; z < kp; z += 256) {
        const int sweep = z / 256, zb = sweep * 256;
        const int span = min(256, kp - zb), rpp = 256 / span;
        double tot = 0.0;
        for (int r = 0; r < rpp; ++r) tot += sred[sweep][r * span + z - zb];
        partials[(long long)blockIdx.x * kp + z] = tot;
    }
}

}  // namespace plsa
