// plsa_lda_kernels.hpp -- the kernels of variational Bayes LDA (include/plsa_hip_diag.h).
//
// The state is gamma [n, kp] (in the place of P(z|d)) and lambda [m, kp] (in the place of P(w|z), word-major).  With
//     A_dz = exp(psi(gamma_dz) - psi(S_d)), S_d = sum_z gamma_dz        B_zw = exp(psi(lambda_zw) - psi(S_z)), S_z = sum_w lambda_zw
// the optimal responsibilities are phi_dwz ~ A_dz B_zw, and the fused passes compute the two expected-count sums of any pair
// of non-negative tables -- and phi does not change when a document's row of A or a word's row of B is scaled.  So an iteration
// forms the tables with the largest entry of every such row scaled to 1 (k_lda_rowsum / k_lda_topic_sums / k_lda_wordmax,
// k_lda_tables: float32 holds exp(-87) at the least, and psi(0.01) is -100), runs the passes on them, and adds the priors
// behind the passes: the document pass leaves u = n_dz / N_d and N_d, k_lda_rows writes
// gamma = u N_d + alpha in place; the column pass leaves n_wz in Vacc, k_lda_topics writes lambda = Vacc + eta.  k_lda_bound
// sums the Dirichlet part of the bound of one table in float64.  The streaming kernels move float4s (16-byte loads and
// stores, four rows in flight per lane, grid-stride, no atomics); the padding topics k .. kp - 1 are written as exact 0.
#pragma once

#include "plsa_lda_math.hpp"
#include "plsa_lda_plan.hpp"

namespace plsa {

static_assert(plan::LDA_BLOCK == 256 && plan::PRIOR_SLABS == NORM_BLOCKS, "the slabs of k_lda_bound are the slabs of k_colsum_partial");

// S[row] = float64 sum of the live float32 entries of row `row` of T [rows, 4 kq], psi_S[row] = digamma(S[row]) and
// shift[row] = digamma(largest entry) - psi_S[row], the logarithm of the row's largest table entry (digamma is increasing);
// the order of the additions is plan::lda_row_lanes' (a function of kq alone).  A row without a positive sum gets 0, 0, 0: its
// table entries are 0 (k_lda_tables), its bound terms are left out (k_lda_bound).
__global__ __launch_bounds__(256) void k_lda_rowsum(const float4 *__restrict__ T, long long rows, int kq, int k, int lanes,
                                                    double *__restrict__ S, double *__restrict__ psi_S, double *__restrict__ shift) {
    const int lane = (int)threadIdx.x % lanes, group = (int)threadIdx.x / lanes;
    const long long stride = plan::lda_row_stride(gridDim.x, lanes);
    for (long long row = plan::lda_row_first(blockIdx.x, group, lanes); row < rows; row += stride) {
        double s = 0.0;
        float top = 0.f;
        for (int q = lane; q < kq; q += lanes) {
            const float4 x = T[row * kq + q];
            const unsigned mask = plan::smooth_pad_mask(q, k);
            double t = (mask & 1u) ? (double)x.x : 0.0;
            if (mask & 2u) t += (double)x.y;
            if (mask & 4u) t += (double)x.z;
            if (mask & 8u) t += (double)x.w;
            s += t;
            if (mask & 1u) top = fmaxf(top, x.x);
            if (mask & 2u) top = fmaxf(top, x.y);
            if (mask & 4u) top = fmaxf(top, x.z);
            if (mask & 8u) top = fmaxf(top, x.w);
        }
        // butterfly over the group: every lane ends with the same sum (an IEEE addition commutes) and the same maximum
        for (int off = lanes / 2; off > 0; off >>= 1) {
            s += __shfl_xor(s, off, lanes);
            top = fmaxf(top, __shfl_xor(top, off, lanes));
        }
        if (lane == 0) {
            const bool live = s > 0.0 && top > 0.f;
            const double ps = live ? lda::digamma(s) : 0.0;
            S[row] = live ? s : 0.0;
            psi_S[row] = ps;
            shift[row] = live ? lda::digamma((double)top) - ps : 0.0;
        }
    }
}

// shift[w] = max over the live topics z of psi(T[w, z]) - psi_S[z], the logarithm of word w's largest table entry, T [rows, 4 kq]
// word-major; a row without a positive entry under a live topic gets 0.  The lanes and groups of k_lda_rowsum.
__global__ __launch_bounds__(256) void k_lda_wordmax(const float4 *__restrict__ T, long long rows, int kq, int k, int lanes,
                                                     const double *__restrict__ S, const double *__restrict__ psi_S,
                                                     double *__restrict__ shift) {
    const int lane = (int)threadIdx.x % lanes, group = (int)threadIdx.x / lanes;
    const long long stride = plan::lda_row_stride(gridDim.x, lanes);
    for (long long row = plan::lda_row_first(blockIdx.x, group, lanes); row < rows; row += stride) {
        double top = -INFINITY;
        for (int q = lane; q < kq; q += lanes) {
            const float4 x = T[row * kq + q];
            const unsigned mask = plan::smooth_pad_mask(q, k);
            const int z = 4 * q;
            if ((mask & 1u) && x.x > 0.f && S[z] > 0.0) top = fmax(top, lda::digamma((double)x.x) - psi_S[z]);
            if ((mask & 2u) && x.y > 0.f && S[z + 1] > 0.0) top = fmax(top, lda::digamma((double)x.y) - psi_S[z + 1]);
            if ((mask & 4u) && x.z > 0.f && S[z + 2] > 0.0) top = fmax(top, lda::digamma((double)x.z) - psi_S[z + 2]);
            if ((mask & 8u) && x.w > 0.f && S[z + 3] > 0.0) top = fmax(top, lda::digamma((double)x.w) - psi_S[z + 3]);
        }
        for (int off = lanes / 2; off > 0; off >>= 1) top = fmax(top, __shfl_xor(top, off, lanes));
        if (lane == 0) shift[row] = top > -INFINITY ? top : 0.0;
    }
}

// partials[slab, z] = float64 sum of T[w, z] over the slab's rows w, T [rows, kp] float32: the slabs and the thread layout of
// k_colsum_partial (thread t owns topic t % span and the rows t / span, + 256 / span, ... of the slab; the strands of a topic
// are added in strand order), with float64 strands -- a float32 strand of L entries would put (L - 1) 2^-24 into S_z, and so
// into every entry of topic z's table row.  One workgroup per slab (plan::lda_bound_grid(rows)), never the grid cap.
__global__ __launch_bounds__(256) void k_lda_topic_partial(const float *__restrict__ T, long long rows, int kp,
                                                           double *__restrict__ partials) {
    __shared__ double sred[256];
    const long long r0 = plan::prior_rows_first(rows, gridDim.x, blockIdx.x), r1 = plan::prior_rows_last(rows, gridDim.x, blockIdx.x);
    for (int zb = 0; zb < kp; zb += 256) {
        const int span = min(256, kp - zb), rpp = 256 / span;
        const int z = zb + (int)threadIdx.x % span, ro = (int)threadIdx.x / span;
        double s = 0.0;
        if (ro < rpp)
            for (long long w = r0 + ro; w < r1; w += rpp) s += (double)T[w * kp + z];
        sred[threadIdx.x] = s;
        __syncthreads();
        if ((int)threadIdx.x < span) {
            double tot = 0.0;
            for (int r = 0; r < rpp; ++r) tot += sred[r * span + threadIdx.x];
            partials[(long long)blockIdx.x * kp + zb + threadIdx.x] = tot;
        }
        __syncthreads();
    }
}

// S[z] = the sum of the slab partials of topic z ([n_partials, kp] float64), psi_S[z] = digamma(S[z]); the pads and a topic
// without a positive sum get 0, 0.  A workgroup holds 16 topics (thread t: topic t % 16 of them, so neighbours read neighbours)
// and 16 lanes per topic: lane l = t / 16 adds the partials l, l + 16, ... in that order, the lane sums are added in lane order.
__global__ __launch_bounds__(256) void k_lda_topic_sums(const double *__restrict__ partials, int n_partials, int kp, int k,
                                                        double *__restrict__ S, double *__restrict__ psi_S) {
    __shared__ double sred[256];
    constexpr int TOPICS = plan::LDA_BLOCK / plan::LDA_TOPIC_LANES;
    const int z = (int)blockIdx.x * TOPICS + (int)threadIdx.x % TOPICS, lane = (int)threadIdx.x / TOPICS;
    double s = 0.0;
    if (z < k)
        for (int b = lane; b < n_partials; b += plan::LDA_TOPIC_LANES) s += partials[(long long)b * kp + z];
    sred[threadIdx.x] = s;
    __syncthreads();
    if (lane == 0 && z < kp) {
        double tot = 0.0;
        for (int l = 0; l < plan::LDA_TOPIC_LANES; ++l) tot += sred[l * TOPICS + threadIdx.x];
        const bool live = tot > 0.0;
        S[z] = live ? tot : 0.0;
        psi_S[z] = live ? lda::digamma(tot) : 0.0;
    }
}

// (float)exp(psi(x) - off) of one entry, off = psi_S + the row's shift: evaluated in float64, rounded to float32 once.  x <= 0 (a
// starting value the caller supplied; no update leaves one under a positive prior) and an entry of a row without a sum give 0.
__device__ __forceinline__ float lda_entry(float x, double off, bool live) {
    return live && x > 0.f ? (float)lda::exp_digamma_diff((double)x, off) : 0.f;
}

template <bool BY_ROW>
__device__ __forceinline__ float4 lda_table_four(const float4 &x, const plan::SmoothPos &p, int k, const double *__restrict__ S,
                                                 const double *__restrict__ psi_S, const double *__restrict__ shift) {
    const unsigned mask = plan::smooth_pad_mask(p.q, k);
    const double sh = shift ? shift[p.row] : 0.0;
    float4 r;
    if (BY_ROW) {
        const bool live = S[p.row] > 0.0;
        const double off = psi_S[p.row] + sh;
        r.x = lda_entry(x.x, off, live && (mask & 1u));
        r.y = lda_entry(x.y, off, live && (mask & 2u));
        r.z = lda_entry(x.z, off, live && (mask & 4u));
        r.w = lda_entry(x.w, off, live && (mask & 8u));
    } else {
        // a quarter's four topics: 4 q + 3 < kp, and S, psi_S hold kp entries (0 at the pads)
        const int z = 4 * p.q;
        r.x = lda_entry(x.x, psi_S[z] + sh, (mask & 1u) && S[z] > 0.0);
        r.y = lda_entry(x.y, psi_S[z + 1] + sh, (mask & 2u) && S[z + 1] > 0.0);
        r.z = lda_entry(x.z, psi_S[z + 2] + sh, (mask & 4u) && S[z + 2] > 0.0);
        r.w = lda_entry(x.w, psi_S[z + 3] + sh, (mask & 8u) && S[z + 3] > 0.0);
    }
    return r;
}

// out [rows, 4 kq] <- exp(psi(T) - psi(S) - shift[row]) over the topics below k, 0 at the pads.  BY_ROW: S, psi_S are per row
// (gamma, from k_lda_rowsum); otherwise per topic (lambda, from k_lda_topic_sums).  shift (per row of T; nullptr: none) is the
// logarithm of the row's largest entry, so the largest entry of every row is 1 and nothing but what is negligible beside it
// can leave the float32 range.  Grid-stride, geometry from plan::smooth_*.
template <bool BY_ROW>
__global__ __launch_bounds__(256) void k_lda_tables(const float4 *__restrict__ T, float4 *__restrict__ out, long long n4, int kq,
                                                    int k, const double *__restrict__ S, const double *__restrict__ psi_S,
                                                    const double *__restrict__ shift) {
    const long long stride = plan::smooth_stride(gridDim.x);
    const plan::SmoothStep step = plan::smooth_step(stride, kq);
    long long i = plan::smooth_first(blockIdx.x, threadIdx.x);
    plan::SmoothPos p0 = plan::smooth_pos(i, kq);
    // four rows in flight: the loads of a batch are issued before its first store
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const plan::SmoothPos p1 = plan::smooth_advance(p0, step, kq), p2 = plan::smooth_advance(p1, step, kq),
                              p3 = plan::smooth_advance(p2, step, kq);
        const float4 x0 = T[i], x1 = T[i + stride], x2 = T[i + 2 * stride], x3 = T[i + 3 * stride];
        out[i] = lda_table_four<BY_ROW>(x0, p0, k, S, psi_S, shift);
        out[i + stride] = lda_table_four<BY_ROW>(x1, p1, k, S, psi_S, shift);
        out[i + 2 * stride] = lda_table_four<BY_ROW>(x2, p2, k, S, psi_S, shift);
        out[i + 3 * stride] = lda_table_four<BY_ROW>(x3, p3, k, S, psi_S, shift);
        p0 = plan::smooth_advance(p3, step, kq);
    }
    for (; i < n4; i += stride) {
        out[i] = lda_table_four<BY_ROW>(T[i], p0, k, S, psi_S, shift);
        p0 = plan::smooth_advance(p0, step, kq);
    }
}

// u N_d + alpha for the live topics of one quarter: one fused multiply-add.  An empty document (N_d = 0, u = 0) gets alpha.
__device__ __forceinline__ float4 lda_row_four(const float4 &u, float nd, float alpha, unsigned mask) {
    float4 r;
    r.x = (mask & 1u) ? fmaf(u.x, nd, alpha) : 0.f;
    r.y = (mask & 2u) ? fmaf(u.y, nd, alpha) : 0.f;
    r.z = (mask & 4u) ? fmaf(u.z, nd, alpha) : 0.f;
    r.w = (mask & 8u) ? fmaf(u.w, nd, alpha) : 0.f;
    return r;
}

// U [rows, 4 kq] <- U * norm_pdz[row] + alpha in place over the topics below k: gamma behind a document pass.  U is read and
// written through the same pointer, each float4 by one lane only.
__global__ __launch_bounds__(256) void k_lda_rows(float4 *U, const float *__restrict__ norm_pdz, long long n4, int kq, int k,
                                                  float alpha) {
    const long long stride = plan::smooth_stride(gridDim.x);
    const plan::SmoothStep step = plan::smooth_step(stride, kq);
    long long i = plan::smooth_first(blockIdx.x, threadIdx.x);
    plan::SmoothPos p0 = plan::smooth_pos(i, kq);
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const plan::SmoothPos p1 = plan::smooth_advance(p0, step, kq), p2 = plan::smooth_advance(p1, step, kq),
                              p3 = plan::smooth_advance(p2, step, kq);
        const float4 u0 = U[i], u1 = U[i + stride], u2 = U[i + 2 * stride], u3 = U[i + 3 * stride];
        const float n0 = norm_pdz[p0.row], n1 = norm_pdz[p1.row], n2 = norm_pdz[p2.row], n3 = norm_pdz[p3.row];
        U[i] = lda_row_four(u0, n0, alpha, plan::smooth_pad_mask(p0.q, k));
        U[i + stride] = lda_row_four(u1, n1, alpha, plan::smooth_pad_mask(p1.q, k));
        U[i + 2 * stride] = lda_row_four(u2, n2, alpha, plan::smooth_pad_mask(p2.q, k));
        U[i + 3 * stride] = lda_row_four(u3, n3, alpha, plan::smooth_pad_mask(p3.q, k));
        p0 = plan::smooth_advance(p3, step, kq);
    }
    for (; i < n4; i += stride) {
        U[i] = lda_row_four(U[i], norm_pdz[p0.row], alpha, plan::smooth_pad_mask(p0.q, k));
        p0 = plan::smooth_advance(p0, step, kq);
    }
}

__device__ __forceinline__ float4 lda_topic_four(const float4 &acc, float eta, unsigned mask) {
    float4 r;
    r.x = (mask & 1u) ? acc.x + eta : 0.f;
    r.y = (mask & 2u) ? acc.y + eta : 0.f;
    r.z = (mask & 4u) ? acc.z + eta : 0.f;
    r.w = (mask & 8u) ? acc.w + eta : 0.f;
    return r;
}

// Vt_out [m, 4 kq] <- Vacc + eta over the topics below k: lambda behind run_col_pass(parts 3)
__global__ __launch_bounds__(256) void k_lda_topics(const float4 *__restrict__ Vacc, float4 *__restrict__ Vt_out, long long n4,
                                                    int kq, int k, float eta) {
    const long long stride = plan::smooth_stride(gridDim.x);
    const plan::SmoothStep step = plan::smooth_step(stride, kq);
    long long i = plan::smooth_first(blockIdx.x, threadIdx.x);
    plan::SmoothPos p0 = plan::smooth_pos(i, kq);
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const plan::SmoothPos p1 = plan::smooth_advance(p0, step, kq), p2 = plan::smooth_advance(p1, step, kq),
                              p3 = plan::smooth_advance(p2, step, kq);
        const float4 v0 = Vacc[i], v1 = Vacc[i + stride], v2 = Vacc[i + 2 * stride], v3 = Vacc[i + 3 * stride];
        Vt_out[i] = lda_topic_four(v0, eta, plan::smooth_pad_mask(p0.q, k));
        Vt_out[i + stride] = lda_topic_four(v1, eta, plan::smooth_pad_mask(p1.q, k));
        Vt_out[i + 2 * stride] = lda_topic_four(v2, eta, plan::smooth_pad_mask(p2.q, k));
        Vt_out[i + 3 * stride] = lda_topic_four(v3, eta, plan::smooth_pad_mask(p3.q, k));
        p0 = plan::smooth_advance(p3, step, kq);
    }
    for (; i < n4; i += stride) {
        Vt_out[i] = lda_topic_four(Vacc[i], eta, plan::smooth_pad_mask(p0.q, k));
        p0 = plan::smooth_advance(p0, step, kq);
    }
}

// lgamma(x) + (prior - x) (psi(x) - psi_S) of one entry, added to s; x <= 0 and an entry of a row without a sum add nothing
__device__ __forceinline__ void lda_bound_entry(float x, double prior, double psi_s, bool live, double &s) {
    if (live && x > 0.f) {
        const double xd = (double)x;
        s += lgamma(xd) + (prior - xd) * (lda::digamma(xd) - psi_s);
    }
}

// partials[slab] = float64 sum over the slab's rows of the Dirichlet part of the bound of T [rows, 4 kq]: per live entry
// lgamma(x) + (prior - x) (psi(x) - psi(S)), and -lgamma(S) once per row (BY_ROW: added by the lane that holds the row's
// quarter 0) or once per topic (added in slab 0 by thread z % 256).  One workgroup per slab (plan::lda_bound_grid(rows) of
// them, never the grid cap), thread t the slab's float4s t, t + 256, ...; the 256 thread sums are added by a fixed tree.
// k_ll_final adds the partials in order.
template <bool BY_ROW>
__global__ __launch_bounds__(256) void k_lda_bound(const float4 *__restrict__ T, long long rows, int kq, int k, double prior,
                                                   const double *__restrict__ S, const double *__restrict__ psi_S,
                                                   double *__restrict__ partials) {
    __shared__ double red[256];
    const long long end = plan::prior_rows_last(rows, gridDim.x, blockIdx.x) * kq;
    long long i = plan::prior_rows_first(rows, gridDim.x, blockIdx.x) * kq + threadIdx.x;
    const plan::SmoothStep step = plan::smooth_step(plan::LDA_BLOCK, kq);
    plan::SmoothPos p = plan::smooth_pos(i, kq);
    double s = 0.0;
    for (; i < end; i += plan::LDA_BLOCK) {
        const float4 x = T[i];
        const unsigned mask = plan::smooth_pad_mask(p.q, k);
        if (BY_ROW) {
            const double sr = S[p.row], ps = psi_S[p.row];
            const bool live = sr > 0.0;
            if (p.q == 0 && live) s -= lgamma(sr);
            lda_bound_entry(x.x, prior, ps, live && (mask & 1u), s);
            lda_bound_entry(x.y, prior, ps, live && (mask & 2u), s);
            lda_bound_entry(x.z, prior, ps, live && (mask & 4u), s);
            lda_bound_entry(x.w, prior, ps, live && (mask & 8u), s);
        } else {
            const int z = 4 * p.q;
            lda_bound_entry(x.x, prior, psi_S[z], (mask & 1u) && S[z] > 0.0, s);
            lda_bound_entry(x.y, prior, psi_S[z + 1], (mask & 2u) && S[z + 1] > 0.0, s);
            lda_bound_entry(x.z, prior, psi_S[z + 2], (mask & 4u) && S[z + 2] > 0.0, s);
            lda_bound_entry(x.w, prior, psi_S[z + 3], (mask & 8u) && S[z + 3] > 0.0, s);
        }
        p = plan::smooth_advance(p, step, kq);
    }
    if (!BY_ROW && blockIdx.x == 0)
        for (int z = threadIdx.x; z < k; z += plan::LDA_BLOCK)
            if (S[z] > 0.0) s -= lgamma(S[z]);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// partials[slab] = float64 sum of x_dw (shift_row[d] + shift_word[w]) over the entries of the slab's documents: what the scaled
// tables take out of sum x_dw log sum_z A_dz B_zw.  plan::lda_shift_grid(rows) slabs of documents, cut like k_lda_bound's; thread t the slab's entries
// t, t + 256, ... of the CSR arrays; a fixed tree; k_ll_final adds the partials in order.
__global__ __launch_bounds__(256) void k_lda_shift_sum(const int *__restrict__ indptr, const int *__restrict__ col,
                                                       const float *__restrict__ val, long long rows,
                                                       const double *__restrict__ shift_row, const double *__restrict__ shift_word,
                                                       double *__restrict__ partials) {
    __shared__ double red[256];
    const long long r0 = plan::prior_rows_first(rows, gridDim.x, blockIdx.x), r1 = plan::prior_rows_last(rows, gridDim.x, blockIdx.x);
    double s = 0.0;
    if (r0 < r1) {
        // the slab's entries, and the row of the first one this thread visits; rows are found by walking indptr forward
        const long long e1 = indptr[r1];
        long long row = r0;
        for (long long e = (long long)indptr[r0] + threadIdx.x; e < e1; e += plan::LDA_BLOCK) {
            while (indptr[row + 1] <= e) ++row;          // (e < e1 = indptr[r1]: row stays below r1)
            const float x = val[e];
            if (x > 0.f) s += (double)x * (shift_row[row] + shift_word[col[e]]);
        }
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
