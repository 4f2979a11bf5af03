// plsa_smoothed_kernels.hpp -- the three kernels of smoothed (MAP) EM (plsa_hip_diag.h: plsa_fit_smoothed, plsa_refit_smoothed,
// plsa_log_posterior).
//
// A smoothed M-step adds a pseudo-count to every expected count before it is normalised:
//     P(z|d) = (n_dz + a) / (N_d + k a)            P(w|z) = (n_wz + b) / (N_z + m b)
// The fused passes stay as they are.  The document pass leaves u = n_dz / N_d in P(z|d) and N_d in norm_pdz, so
// k_smooth_rows turns u into (u N_d + a) / (N_d + k a) in place; the column pass leaves n_wz in Vacc and the norm kernels N_z
// in norm_pwz, so k_smooth_topics writes (Vacc + b) / (N_z + m b) -- the sum over w of the new numerators IS N_z + m b, no
// second sweep forms it.  k_log_prior sums the log-prior terms of one table in float64.  All three stream float4s (16-byte
// loads and stores, several rows in flight per lane, no atomics); the padding topics k .. kp - 1 stay exactly 0.
#pragma once

#include "plsa_smoothed_plan.hpp"

namespace plsa {

static_assert(plan::PRIOR_SLABS == NORM_BLOCKS, "the prior's slabs are the slabs of k_colsum_partial");

// (u N_d + a) / (N_d + k a) for the live topics of one quarter: one fused multiply-add, one sum, one division, each rounded
// once.  An empty document (N_d = 0, u = 0) gets a / (k a), the prior mean.
__device__ __forceinline__ float4 smooth_row_four(const float4 &u, float nd, float a, float ka, unsigned mask) {
    const float den = nd + ka;
    float4 r;
    r.x = (mask & 1u) ? fmaf(u.x, nd, a) / den : 0.f;
    r.y = (mask & 2u) ? fmaf(u.y, nd, a) / den : 0.f;
    r.z = (mask & 4u) ? fmaf(u.z, nd, a) / den : 0.f;
    r.w = (mask & 8u) ? fmaf(u.w, nd, a) / den : 0.f;
    return r;
}

// U [rows, 4 kq] <- (U * norm_pdz[row] + a) / (norm_pdz[row] + ka) in place over the topics below k (a > 0; ka = (float)(k a),
// formed once on the host); grid-stride, geometry from plan::smooth_*.  U is read and written through the same pointer, each
// float4 by one lane only.
__global__ __launch_bounds__(256) void k_smooth_rows(float4 *U, const float *__restrict__ norm_pdz, long long n4, int kq, int k,
                                                     float a, float ka) {
    const long long stride = plan::smooth_stride(gridDim.x);
    const plan::SmoothStep step = plan::smooth_step(stride, kq);
    long long i = plan::smooth_first(blockIdx.x, threadIdx.x);
    plan::SmoothPos p0 = plan::smooth_pos(i, kq);
    // four rows in flight: the loads of a batch are issued before its first store
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const plan::SmoothPos p1 = plan::smooth_advance(p0, step, kq), p2 = plan::smooth_advance(p1, step, kq),
                              p3 = plan::smooth_advance(p2, step, kq);
        const float4 u0 = U[i], u1 = U[i + stride], u2 = U[i + 2 * stride], u3 = U[i + 3 * stride];
        const float n0 = norm_pdz[p0.row], n1 = norm_pdz[p1.row], n2 = norm_pdz[p2.row], n3 = norm_pdz[p3.row];
        U[i] = smooth_row_four(u0, n0, a, ka, plan::smooth_pad_mask(p0.q, k));
        U[i + stride] = smooth_row_four(u1, n1, a, ka, plan::smooth_pad_mask(p1.q, k));
        U[i + 2 * stride] = smooth_row_four(u2, n2, a, ka, plan::smooth_pad_mask(p2.q, k));
        U[i + 3 * stride] = smooth_row_four(u3, n3, a, ka, plan::smooth_pad_mask(p3.q, k));
        p0 = plan::smooth_advance(p3, step, kq);
    }
    for (; i < n4; i += stride) {
        U[i] = smooth_row_four(U[i], norm_pdz[p0.row], a, ka, plan::smooth_pad_mask(p0.q, k));
        p0 = plan::smooth_advance(p0, step, kq);
    }
}

__device__ __forceinline__ float4 smooth_topic_four(const float4 &acc, const float4 &den, float b, unsigned mask) {
    float4 r;
    r.x = (mask & 1u) ? (acc.x + b) / den.x : 0.f;
    r.y = (mask & 2u) ? (acc.y + b) / den.y : 0.f;
    r.z = (mask & 4u) ? (acc.z + b) / den.z : 0.f;
    r.w = (mask & 8u) ? (acc.w + b) / den.w : 0.f;
    return r;
}

// Vt_out [m, 4 kq] <- (Vacc + b) / den over the topics below k, den[z] = (float)((double)norm_pwz[z] + mb), mb = (double)m * b
// formed once on the host (b > 0, so den > 0); every workgroup forms den into LDS before its stride loop, the way
// k_v_normalise keeps its norms.  Dynamic LDS: 4 kq floats.
__global__ __launch_bounds__(256) void k_smooth_topics(const float4 *__restrict__ Vacc, float4 *__restrict__ Vt_out, long long n4,
                                                       int kq, int k, const float *__restrict__ norm_pwz, float b, double mb) {
    extern __shared__ __attribute__((aligned(16))) float sden[];   // [4 kq]
    for (int z = threadIdx.x; z < 4 * kq; z += 256) sden[z] = z < k ? (float)((double)norm_pwz[z] + mb) : 1.f;
    __syncthreads();
    const float4 *den4 = reinterpret_cast<const float4 *>(sden);
    const long long stride = plan::smooth_stride(gridDim.x);
    const plan::SmoothStep step = plan::smooth_step(stride, kq);
    long long i = plan::smooth_first(blockIdx.x, threadIdx.x);
    plan::SmoothPos p0 = plan::smooth_pos(i, kq);
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const plan::SmoothPos p1 = plan::smooth_advance(p0, step, kq), p2 = plan::smooth_advance(p1, step, kq),
                              p3 = plan::smooth_advance(p2, step, kq);
        const float4 v0 = Vacc[i], v1 = Vacc[i + stride], v2 = Vacc[i + 2 * stride], v3 = Vacc[i + 3 * stride];
        Vt_out[i] = smooth_topic_four(v0, den4[p0.q], b, plan::smooth_pad_mask(p0.q, k));
        Vt_out[i + stride] = smooth_topic_four(v1, den4[p1.q], b, plan::smooth_pad_mask(p1.q, k));
        Vt_out[i + 2 * stride] = smooth_topic_four(v2, den4[p2.q], b, plan::smooth_pad_mask(p2.q, k));
        Vt_out[i + 3 * stride] = smooth_topic_four(v3, den4[p3.q], b, plan::smooth_pad_mask(p3.q, k));
        p0 = plan::smooth_advance(p3, step, kq);
    }
    for (; i < n4; i += stride) {
        Vt_out[i] = smooth_topic_four(Vacc[i], den4[p0.q], b, plan::smooth_pad_mask(p0.q, k));
        p0 = plan::smooth_advance(p0, step, kq);
    }
}

// coef * w * log(x) of the live entries of one quarter, added to s one after the other.  An entry equal to 0 adds nothing
// (nor does a negative one or a NaN, which no factor holds): EM never produces a zero under a positive pseudo-count, it can
// only stand in starting factors the caller supplied, and there the objective reports the rest of the table instead of -inf.
__device__ __forceinline__ void log_prior_four(const float4 &x, double cw, unsigned mask, double &s) {
    if ((mask & 1u) && x.x > 0.f) s += cw * log((double)x.x);
    if ((mask & 2u) && x.y > 0.f) s += cw * log((double)x.y);
    if ((mask & 4u) && x.z > 0.f) s += cw * log((double)x.z);
    if ((mask & 8u) && x.w > 0.f) s += cw * log((double)x.w);
}

// partials[slab] = float64 sum of coef * w[row] * log((double)T[row, z]) over the slab's rows and z < k (w == nullptr: 1).
// One workgroup per slab (plan::prior_grid(rows) of them, never the grid cap), thread t the slab's float4s t, t + 256, ...;
// the 256 thread sums are added by a fixed tree.  k_ll_final adds the partials in order.
__global__ __launch_bounds__(256) void k_log_prior(const float4 *__restrict__ T, long long rows, int kq, int k,
                                                   const float *__restrict__ w, double coef, double *__restrict__ partials) {
    __shared__ double red[256];
    const long long end = plan::prior_rows_last(rows, gridDim.x, blockIdx.x) * kq;
    long long i = plan::prior_rows_first(rows, gridDim.x, blockIdx.x) * kq + threadIdx.x;
    const plan::SmoothStep step = plan::smooth_step(plan::SMOOTH_BLOCK, kq);
    plan::SmoothPos p = plan::smooth_pos(i, kq);
    double s = 0.0;
    for (; i < end; i += plan::SMOOTH_BLOCK) {
        const double cw = w ? coef * (double)w[p.row] : coef;
        log_prior_four(T[i], cw, plan::smooth_pad_mask(p.q, k), s);
        p = plan::smooth_advance(p, step, kq);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

}  // namespace plsa
