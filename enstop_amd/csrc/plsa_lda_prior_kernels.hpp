// plsa_lda_prior_kernels.hpp -- the kernels of LDA's learned priors (include/plsa_hip_lda_priors.h).
//
// A prior update needs the sums T_z = sum_d (psi(gamma_dz) - psi(S_d)) and sum_w (psi(lambda_zw) - psi(S_z)) of the state in
// force: k_lda_logmean streams a table once and leaves one float64 partial per slab and topic, k_lda_logmean_sums adds them in
// a fixed order; the Newton iterations run on the host (plsa_lda_prior_math.hpp).  With a vector prior the document side of an
// iteration is k_lda_rows_v (gamma = u N_d + alpha_z) and the document side of the bound k_lda_bound_v ((alpha_z - x) where
// k_lda_bound has (prior - x)).  The geometry is plsa_lda_prior_plan.hpp's; the pads k .. kp - 1 stay exact 0.
#pragma once

#include "plsa_lda_kernels.hpp"
#include "plsa_lda_prior_plan.hpp"

namespace plsa {

// partials[slab, z] = float64 sum over the slab's rows r of psi(T[r, z]) - psi_S, T [rows, kp] float32, over the entries
// k_lda_bound counts as live (a positive entry of a row -- BY_ROW -- or of a topic with a positive sum S); psi_S is per row
// (gamma, from k_lda_rowsum) or per topic (lambda, from k_lda_topic_sums).  The pads get 0.  The thread layout of
// k_lda_topic_partial: thread t owns topic zb + t % span and a strand of the slab's rows, the strands of a topic are added
// in strand order.  One workgroup per slab (plan::lda_logmean_grid(rows)), never the grid cap.
template <bool BY_ROW>
__global__ __launch_bounds__(256) void k_lda_logmean(const float *__restrict__ T, long long rows, int kp, int k,
                                                     const double *__restrict__ S, const double *__restrict__ psi_S,
                                                     double *__restrict__ partials) {
    __shared__ double sred[256];
    const long long r0 = plan::prior_rows_first(rows, gridDim.x, blockIdx.x), r1 = plan::prior_rows_last(rows, gridDim.x, blockIdx.x);
    for (int zb = 0; zb < kp; zb += plan::LDA_BLOCK) {
        const int span = plan::logmean_span(kp, zb), strands = plan::logmean_strands(span);
        const int z = zb + (int)threadIdx.x % span, strand = (int)threadIdx.x / span;
        double s = 0.0;
        if (strand < strands && z < k) {
            if (BY_ROW) {
                for (long long r = r0 + strand; r < r1; r += strands) {
                    const float x = T[r * kp + z];
                    if (x > 0.f && S[r] > 0.0) s += lda::digamma((double)x) - psi_S[r];
                }
            } else if (S[z] > 0.0) {
                const double ps = psi_S[z];
                for (long long r = r0 + strand; r < r1; r += strands) {
                    const float x = T[r * kp + z];
                    if (x > 0.f) s += lda::digamma((double)x) - ps;
                }
            }
        }
        sred[threadIdx.x] = s;
        __syncthreads();
        if ((int)threadIdx.x < span) {
            double tot = 0.0;
            for (int r = 0; r < strands; ++r) tot += sred[r * span + threadIdx.x];
            partials[(long long)blockIdx.x * kp + zb + threadIdx.x] = tot;
        }
        __syncthreads();
    }
}

// out[z] = the sum of the slab partials of topic z ([n_partials, kp] float64), 0 at the pads: the lanes of k_lda_topic_sums,
// without its psi and without its clamp (the sums are negative).  Lane l of a topic owns the partials l, l + 16, ...; with up to
// 4 096 of them it keeps LOGMEAN_CHAINS sums going, its j-th partial into sum j % LOGMEAN_CHAINS, so that as many loads are in
// flight (one chain of 256 dependent additions waited for every load: 0.066 ms a launch, whatever the shape), and adds the
// sums in their order: an order that depends on the number of partials alone.
__global__ __launch_bounds__(256) void k_lda_logmean_sums(const double *__restrict__ partials, int n_partials, int kp, int k,
                                                          double *__restrict__ out) {
    __shared__ double sred[256];
    constexpr int TOPICS = plan::LDA_BLOCK / plan::LDA_TOPIC_LANES, CHAINS = plan::LOGMEAN_CHAINS;
    const int z = (int)blockIdx.x * TOPICS + (int)threadIdx.x % TOPICS, lane = (int)threadIdx.x / TOPICS;
    double s = 0.0;
    if (z < k) {
        double chain[CHAINS];
#pragma unroll
        for (int u = 0; u < CHAINS; ++u) chain[u] = 0.0;
        int b = lane;
        for (; b + (CHAINS - 1) * plan::LDA_TOPIC_LANES < n_partials; b += CHAINS * plan::LDA_TOPIC_LANES) {
            double x[CHAINS];
#pragma unroll
            for (int u = 0; u < CHAINS; ++u) x[u] = partials[(long long)(b + u * plan::LDA_TOPIC_LANES) * kp + z];
#pragma unroll
            for (int u = 0; u < CHAINS; ++u) chain[u] += x[u];
        }
#pragma unroll
        for (int u = 0; u < CHAINS; ++u, b += plan::LDA_TOPIC_LANES)
            if (b < n_partials) chain[u] += partials[(long long)b * kp + z];
#pragma unroll
        for (int u = 0; u < CHAINS; ++u) s += chain[u];
    }
    sred[threadIdx.x] = s;
    __syncthreads();
    if (lane == 0 && z < kp) {
        double tot = 0.0;
        for (int l = 0; l < plan::LDA_TOPIC_LANES; ++l) tot += sred[l * TOPICS + threadIdx.x];
        out[z] = tot;
    }
}

// u N_d + alpha_z for the live topics of one quarter; an empty document (N_d = 0, u = 0) gets alpha
__device__ __forceinline__ float4 lda_row_four_v(const float4 &u, float nd, const float4 &alpha, unsigned mask) {
    float4 r;
    r.x = (mask & 1u) ? fmaf(u.x, nd, alpha.x) : 0.f;
    r.y = (mask & 2u) ? fmaf(u.y, nd, alpha.y) : 0.f;
    r.z = (mask & 4u) ? fmaf(u.z, nd, alpha.z) : 0.f;
    r.w = (mask & 8u) ? fmaf(u.w, nd, alpha.w) : 0.f;
    return r;
}

// U [rows, 4 kq] <- U * norm_pdz[row] + alpha[z] in place over the topics below k: k_lda_rows with the prior of topic z in
// alpha [4 kq] float32, one float4 of it per quarter
__global__ __launch_bounds__(256) void k_lda_rows_v(float4 *U, const float *__restrict__ norm_pdz, long long n4, int kq, int k,
                                                    const float4 *__restrict__ alpha) {
    const long long stride = plan::smooth_stride(gridDim.x);
    const plan::SmoothStep step = plan::smooth_step(stride, kq);
    long long i = plan::smooth_first(blockIdx.x, threadIdx.x);
    plan::SmoothPos p0 = plan::smooth_pos(i, kq);
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const plan::SmoothPos p1 = plan::smooth_advance(p0, step, kq), p2 = plan::smooth_advance(p1, step, kq),
                              p3 = plan::smooth_advance(p2, step, kq);
        const float4 u0 = U[i], u1 = U[i + stride], u2 = U[i + 2 * stride], u3 = U[i + 3 * stride];
        const float n0 = norm_pdz[p0.row], n1 = norm_pdz[p1.row], n2 = norm_pdz[p2.row], n3 = norm_pdz[p3.row];
        U[i] = lda_row_four_v(u0, n0, alpha[p0.q], plan::smooth_pad_mask(p0.q, k));
        U[i + stride] = lda_row_four_v(u1, n1, alpha[p1.q], plan::smooth_pad_mask(p1.q, k));
        U[i + 2 * stride] = lda_row_four_v(u2, n2, alpha[p2.q], plan::smooth_pad_mask(p2.q, k));
        U[i + 3 * stride] = lda_row_four_v(u3, n3, alpha[p3.q], plan::smooth_pad_mask(p3.q, k));
        p0 = plan::smooth_advance(p3, step, kq);
    }
    for (; i < n4; i += stride) {
        U[i] = lda_row_four_v(U[i], norm_pdz[p0.row], alpha[p0.q], plan::smooth_pad_mask(p0.q, k));
        p0 = plan::smooth_advance(p0, step, kq);
    }
}

// the document side of k_lda_bound with the prior of topic z in alpha [4 kq] float64: per live entry
// lgamma(x) + (alpha_z - x) (psi(x) - psi(S_d)), -lgamma(S_d) once per row; the slabs, the walk and the tree of k_lda_bound
__global__ __launch_bounds__(256) void k_lda_bound_v(const float4 *__restrict__ T, long long rows, int kq, int k,
                                                     const double *__restrict__ alpha, const double *__restrict__ S,
                                                     const double *__restrict__ psi_S, double *__restrict__ partials) {
    __shared__ double red[256];
    const long long end = plan::prior_rows_last(rows, gridDim.x, blockIdx.x) * kq;
    long long i = plan::prior_rows_first(rows, gridDim.x, blockIdx.x) * kq + threadIdx.x;
    const plan::SmoothStep step = plan::smooth_step(plan::LDA_BLOCK, kq);
    plan::SmoothPos p = plan::smooth_pos(i, kq);
    double s = 0.0;
    for (; i < end; i += plan::LDA_BLOCK) {
        const float4 x = T[i];
        const unsigned mask = plan::smooth_pad_mask(p.q, k);
        const double sr = S[p.row], ps = psi_S[p.row];
        const bool live = sr > 0.0;
        const int z = 4 * p.q;
        if (p.q == 0 && live) s -= lgamma(sr);
        lda_bound_entry(x.x, alpha[z], ps, live && (mask & 1u), s);
        lda_bound_entry(x.y, alpha[z + 1], ps, live && (mask & 2u), s);
        lda_bound_entry(x.z, alpha[z + 2], ps, live && (mask & 4u), s);
        lda_bound_entry(x.w, alpha[z + 3], ps, live && (mask & 8u), s);
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
