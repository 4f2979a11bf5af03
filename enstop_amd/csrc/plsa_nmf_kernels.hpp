// plsa_nmf_kernels.hpp -- Kullback-Leibler NMF by multiplicative updates on the structures of the fused EM passes.
//
// The arithmetic is scikit-learn's _fit_multiplicative_update for sparse X, beta_loss = 1, gamma = 1, no regularisation
// (sklearn/decomposition/_nmf.py), one half-iteration per kernel family:
//
//   W[d,:] <- W[d,:] * ( sum_{w in d} x_dw / (WH)_dw * H[:,w] ) / H_sum         _multiplicative_update_w
//   H[:,w] <- H[:,w] * ( sum_{d in w} x_dw / (WH)_dw * W[d,:] ) / W_sum         _multiplicative_update_h (reads the NEW W)
//
// W lives where P(z|d) lives (U, [n, kp]), H where P(w|z) lives (Vt, word-major [m, kp]).  (WH)_dw is a group sum, clamped
// to EPS32 before the quotient; the quotient is formed once, in the lane that loaded the entry.  Every product-and-add is
// an explicit fma and contraction is off around them: the packed and the two-array instantiation, the narrow and the WIDE
// one, a lone pass and the in-kernel repetition of the combined pass all execute the same operations on the same values.
// Nothing here uses float atomics; every sum has a fixed order.
#pragma once

#include "plsa_kernels.hpp"

namespace plsa {

constexpr float NMF_EPS32 = 1.1920928955078125e-07f;    // np.finfo(np.float32).eps
constexpr float NMF_EPS64 = 2.220446049250313e-16f;     // np.finfo(np.float64).eps = 2^-52, exact in float32

// lane-partial of the dot product of two k-vectors (chunks outside the row are zero in `a`)
template <int CH>
__device__ __forceinline__ float nmf_dot(const float4 (&a)[CH], const float4 (&b)[CH]) {
#pragma clang fp contract(off)
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        p = __builtin_fmaf(a[j].x, b[j].x, p); p = __builtin_fmaf(a[j].y, b[j].y, p);
        p = __builtin_fmaf(a[j].z, b[j].z, p); p = __builtin_fmaf(a[j].w, b[j].w, p);
    }
    return p;
}

template <int CH>
__device__ __forceinline__ void nmf_axpy(float4 (&acc)[CH], float q, const float4 (&r)[CH]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        acc[j].x = __builtin_fmaf(q, r[j].x, acc[j].x); acc[j].y = __builtin_fmaf(q, r[j].y, acc[j].y);
        acc[j].z = __builtin_fmaf(q, r[j].z, acc[j].z); acc[j].w = __builtin_fmaf(q, r[j].w, acc[j].w);
    }
}

// x / (WH) with scikit-learn's guard: WH_data[WH_data < EPSILON] = EPSILON (true division)
__device__ __forceinline__ float nmf_quotient(float x, float wh) {
#pragma clang fp contract(off)
    return x / (wh < NMF_EPS32 ? NMF_EPS32 : wh);
}

// factor * (numerator / sum): numerator /= denominator; W *= delta_W (in that order)
__device__ __forceinline__ float4 nmf_scale(const float4 &f, const float4 &num, const float4 &den) {
#pragma clang fp contract(off)
    return make_float4(f.x * (num.x / den.x), f.y * (num.y / den.y), f.z * (num.z / den.z), f.w * (num.w / den.w));
}

// UN entries of a stream piece against the owner's k-vector `own` (W row in the document pass, H row in the column
// pass): gathers UN rows of `table`, forms x / max(own . row, EPS32) in the lane that loaded the entry (lane s0 + q holds
// entry q of the batch) and adds quotient * row.  Lanes past the end of the piece hold (id 0, count 0): exact zeros.
template <class S, int UN>
__device__ __forceinline__ void nmf_batch(int s0, int id_l, float x_l, int li, int kp, const float *table,
                                          const float4 (&own)[S::CH], float4 (&acc)[S::CH]) {
    constexpr int LPN = S::LPN, CH = S::CH;
    float4 a[UN][CH];
#pragma unroll
    for (int q = 0; q < UN; ++q) gather_row<S>(table, __shfl(id_l, s0 + q, LPN), li, kp, a[q]);
    float mine = 1.f;
#pragma unroll
    for (int q = 0; q < UN; ++q) {
        const float wh = group_sum<LPN>(nmf_dot<CH>(own, a[q]));
        mine = (li == s0 + q) ? wh : mine;
    }
    const float q_mine = nmf_quotient(x_l, mine);
#pragma unroll
    for (int q = 0; q < UN; ++q) nmf_axpy<CH>(acc, __shfl(q_mine, s0 + q, LPN), a[q]);
}

// one sweep over the entries [j0, j1) of a stream (CSR piece of a document, CSC piece of a column item); sbase: the owner's
// first word in a packed stream (plsa_kernels.hpp: EntryCursor)
template <class S, int UN>
__device__ __forceinline__ void nmf_sweep(const int *__restrict__ ids, const float *__restrict__ vals, int sbase, int j0, int j1,
                                          int li, int kp, const float *table, const float4 (&own)[S::CH],
                                          float4 (&acc)[S::CH]) {
    constexpr int LPN = S::LPN;
    EntryCursor<S> es;
    es.open(ids, vals, sbase, j0, j1, li);
    for (int jb = j0; jb < j1; jb += LPN) {
        int id_l;
        float x_l;
        es.take(ids, vals, jb, j1, li, id_l, x_l);
        const int cnt = min(LPN, j1 - jb);
        int s0 = 0;
        for (; s0 + UN <= cnt; s0 += UN) nmf_batch<S, UN>(s0, id_l, x_l, li, kp, table, own, acc);
        constexpr int TAIL = (UN >= 2 && LPN >= 2) ? 2 : 1;      // short pieces must not pay for UN padded gathers
        for (; s0 < cnt; s0 += TAIL) nmf_batch<S, TAIL>(s0, id_l, x_l, li, kp, table, own, acc);
    }
}

// ------------------------------------------------------------------------------------------------
// k_nmf_row_pass: _multiplicative_update_w.  A group owns a document (visited through row_order) or, in row-item mode
// (ritem_row != nullptr), one item of a document; the W row sits in registers, rows of H (Vt) are gathered.
//   documents: the accumulator is multiplied by W / H_sum and the row is written once, IN PLACE (no other group reads
//     it).  `iters` > 1 repeats the update on the row in registers: between two H updates iteration i + 1 of a document
//     reads only what iteration i of the same document wrote, so a fit with H fixed runs the iterations between two
//     stopping tests in one launch (the combined pass).  The repetition executes the code of a lone pass.
//   row items: un-scaled partial rows, k_nmf_row_reduce adds them in item order and applies the update (iters == 1).
// h_sum: sum_w H[z,w], zeros replaced by EPS32 (k_nmf_colsum_final).
// ------------------------------------------------------------------------------------------------
template <class S>
__global__ __launch_bounds__(256) void k_nmf_row_pass(const int *__restrict__ indptr, const int *__restrict__ colidx,
                                                      const float *__restrict__ vals, const int *__restrict__ sblk, int n,
                                                      const int *__restrict__ row_order, float *W,
                                                      const float *__restrict__ Vt, const float *__restrict__ h_sum,
                                                      int kp_rt, int iters, const int *__restrict__ ritem_row,
                                                      const int *__restrict__ ritem_start, int rseg, i64 n_ritems,
                                                      float *__restrict__ rpartial) {
    constexpr int LPN = S::LPN, CH = S::CH;
    constexpr int GPB = 256 / LPN;
    const int kp = S::kp(kp_rt);
    const int li = threadIdx.x % LPN;
    const int gid = threadIdx.x / LPN;
    const bool items = ritem_row != nullptr;
    const i64 n_work = items ? n_ritems : (i64)n;
    float4 hs[CH];
    load_row<S, false>(h_sum, li, kp, hs);
    for (i64 r = (i64)blockIdx.x * GPB + gid; r < n_work; r += (i64)gridDim.x * GPB) {
        const int d = items ? ritem_row[r] : (row_order ? row_order[r] : (int)r);
        const int j0 = items ? ritem_start[r] : indptr[d];
        const int j1 = items ? min(j0 + rseg, indptr[d + 1]) : indptr[d + 1];
        float4 w[CH], acc[CH];
        load_row<S, true>(W + (i64)d * kp, li, kp, w);
        const int sbase = S::PACKED ? (items ? (int)r * row_item_slot<LPN>(rseg) : sblk[d] * (4 * LPN)) : 0;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int j = 0; j < CH; ++j) acc[j] = zero4();
            nmf_sweep<S, S::UNR>(colidx, vals, sbase, j0, j1, li, kp, Vt, w, acc);
            if (items) break;
#pragma unroll
            for (int j = 0; j < CH; ++j) w[j] = S::ok(li, j, kp) ? nmf_scale(w[j], acc[j], hs[j]) : zero4();
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            if (!S::ok(li, j, kp)) continue;
            if (items) st4(rpartial + r * kp + S::c4(li, j), acc[j]);
            else st4(W + (i64)d * kp + S::c4(li, j), w[j]);
        }
    }
}

// the tail of k_nmf_row_pass in row-item mode: item partials of a document in item order, then W * (sum / H_sum), in place
template <class S>
__global__ __launch_bounds__(256) void k_nmf_row_reduce(const int *__restrict__ ritem_first, int n,
                                                        const float *__restrict__ rpartial, float *W,
                                                        const float *__restrict__ h_sum, int kp_rt) {
    constexpr int LPN = S::LPN, CH = S::CH;
    constexpr int GPB = 256 / LPN;
    const int kp = S::kp(kp_rt);
    const int li = threadIdx.x % LPN;
    const int gid = threadIdx.x / LPN;
    float4 hs[CH];
    load_row<S, false>(h_sum, li, kp, hs);
    for (i64 d = (i64)blockIdx.x * GPB + gid; d < n; d += (i64)gridDim.x * GPB) {
        const int i0 = ritem_first[d], i1 = ritem_first[d + 1];
        float4 acc[CH], w[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[j] = zero4();
        for (int it = i0; it < i1; ++it) {
            float4 p[CH];
            load_row<S, true>(rpartial + (i64)it * kp, li, kp, p);
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                acc[j].x += p[j].x; acc[j].y += p[j].y; acc[j].z += p[j].z; acc[j].w += p[j].w;
            }
        }
        load_row<S, true>(W + d * kp, li, kp, w);
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (S::ok(li, j, kp)) st4(W + d * kp + S::c4(li, j), nmf_scale(w[j], acc[j], hs[j]));
    }
}

// ------------------------------------------------------------------------------------------------
// k_nmf_col_pass: the numerator of _multiplicative_update_h.  A group owns a column item (item_rec: the visiting-order
// records of the EM column pass), the H row sits in registers, rows of the NEW W are gathered; one partial k-vector per
// item.  The per-column sums of the partials are k_col_reduce's (fixed item order), k_nmf_h_finish applies the update.
// ------------------------------------------------------------------------------------------------
template <class S>
__global__ __launch_bounds__(256) void k_nmf_col_pass(const int4 *__restrict__ item_rec, i64 n_items,
                                                      const int *__restrict__ csc_row, const float *__restrict__ csc_val,
                                                      int slot, const float *__restrict__ W, const float *__restrict__ Vt,
                                                      float *__restrict__ partial, int kp_rt) {
    constexpr int LPN = S::LPN, CH = S::CH;
    constexpr int GPB = 256 / LPN;
    const int kp = S::kp(kp_rt);
    const int li = threadIdx.x % LPN;
    const int gid = threadIdx.x / LPN;
    for (i64 io = (i64)blockIdx.x * GPB + gid; io < n_items; io += (i64)gridDim.x * GPB) {
        const int4 rec = item_rec[io];
        float4 h[CH], acc[CH];
        load_row<S, true>(Vt + (i64)rec.x * kp, li, kp, h);
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[j] = zero4();
        nmf_sweep<S, S::UNR_COL>(csc_row, csc_val, S::PACKED ? rec.w * slot : 0, rec.y, rec.z, li, kp, W, h, acc);
#pragma unroll
        for (int j = 0; j < CH; ++j)
            if (S::ok(li, j, kp)) st4(partial + (i64)rec.w * kp + S::c4(li, j), acc[j]);
    }
}

// H[w,:] <- H[w,:] * (numerator[w,:] / W_sum), then H[H < float64 eps] = 0 (_fit_multiplicative_update), in place.
// w_sum: sum_d W[d,z], zeros replaced by 1.
__global__ __launch_bounds__(256) void k_nmf_h_finish(const float *__restrict__ num, float *Vt, i64 m, int kp,
                                                      const float *__restrict__ w_sum) {
    extern __shared__ float s_wsum[];  // [kp]
    for (int z = threadIdx.x; z < kp; z += 256) s_wsum[z] = w_sum[z];
    __syncthreads();
    const i64 total4 = m * kp / 4;
    const int kq = kp / 4;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total4; i += (i64)gridDim.x * 256) {
        const int z4 = (int)(i % kq) * 4;
        float4 o = nmf_scale(ld4(Vt + i * 4), ld4(num + i * 4), make_float4(s_wsum[z4], s_wsum[z4 + 1], s_wsum[z4 + 2], s_wsum[z4 + 3]));
        o.x = o.x < NMF_EPS64 ? 0.f : o.x; o.y = o.y < NMF_EPS64 ? 0.f : o.y;
        o.z = o.z < NMF_EPS64 ? 0.f : o.z; o.w = o.w < NMF_EPS64 ? 0.f : o.w;
        st4(Vt + i * 4, o);
    }
}

// ------------------------------------------------------------------------------------------------
// H_sum (over the m rows of Vt) and W_sum (over the n rows of U): float64, fixed order -- the only sums of an iteration
// whose length is not bounded by a row or a column.
//   k_nmf_colsum_partial : block b adds a contiguous slab of rows (thread layout of colsum_slab_body, float64 strands)
//   k_nmf_colsum_final   : adds the slab sums in slab order -> raw (float64: the objective's W_sum . H_sum) and guarded
//                          (float32, zeros replaced by `if_zero`: EPS32 for H_sum, 1 for W_sum)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nmf_colsum_partial(const float *__restrict__ A, i64 rows, int kp,
                                                            double *__restrict__ partials) {
    __shared__ double sred[256];
    const i64 per = (rows + gridDim.x - 1) / gridDim.x;
    const i64 r0 = (i64)blockIdx.x * per, r1 = min(rows, r0 + per);
    for (int zb = 0; zb < kp; zb += 256) {
        const int span = min(256, kp - zb);
        const int rpp = 256 / span;
        const int z = zb + (int)threadIdx.x % span;
        const int ro = (int)threadIdx.x / span;
        double s = 0.0;
        if (ro < rpp)
            for (i64 r = r0 + ro; r < r1; r += rpp) s += (double)A[r * kp + z];
        sred[threadIdx.x] = (ro < rpp) ? s : 0.0;
        __syncthreads();
        if ((int)threadIdx.x < span) {
            double tot = 0.0;
            for (int r = 0; r < rpp; ++r) tot += sred[r * span + threadIdx.x];
            partials[(i64)blockIdx.x * kp + zb + threadIdx.x] = tot;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_nmf_colsum_final(const double *__restrict__ partials, int n_partials, int kp,
                                                          double *__restrict__ raw, float *__restrict__ guarded,
                                                          float if_zero) {
    for (int z = threadIdx.x; z < kp; z += 256) {
        double t = 0.0;
        for (int b = 0; b < n_partials; ++b) t += partials[(i64)b * kp + z];
        raw[z] = t;
        const float f = (float)t;
        guarded[z] = f == 0.f ? if_zero : f;
    }
}

// ------------------------------------------------------------------------------------------------
// The objective, _beta_divergence(X, W, H, 1, square_root=True): per workgroup the float64 sums of x log(x / max(WH, EPS32))
// and of x over the stored entries with x > EPS32 (document-owned, the traversal of k_loglik; the logarithm is taken in
// float64, in the lane that loaded the entry), then
//   D = sum x log(x / wh) + W_sum . H_sum - sum x,   out[0] = sqrt(2 max(D, 0)), out[1] = D.
// ------------------------------------------------------------------------------------------------
template <class S>
__global__ __launch_bounds__(256) void k_nmf_divergence(const int *__restrict__ indptr, const int *__restrict__ colidx,
                                                        const float *__restrict__ vals, int n,
                                                        const int *__restrict__ row_order, const float *__restrict__ W,
                                                        const float *__restrict__ Vt, int kp_rt,
                                                        double *__restrict__ partials /*[2][gridDim.x]*/) {
    constexpr int LPN = S::LPN, CH = S::CH, UNR = S::UNR;
    constexpr int GPB = 256 / LPN;
    const int kp = S::kp(kp_rt);
    const int li = threadIdx.x % LPN;
    const int gid = threadIdx.x / LPN;
    double s_log = 0.0, s_x = 0.0;
    for (i64 r = (i64)blockIdx.x * GPB + gid; r < n; r += (i64)gridDim.x * GPB) {
        const int d = row_order ? row_order[r] : (int)r;
        const int j0 = indptr[d], j1 = indptr[d + 1];
        float4 w[CH];
        load_row<S, true>(W + (i64)d * kp, li, kp, w);
        for (int jb = j0; jb < j1; jb += LPN) {
            const bool mine_ok = jb + li < j1;
            const int id_l = mine_ok ? ldi(colidx + jb + li) : 0;
            const float x_l = mine_ok ? ldf(vals + jb + li) : 0.f;
            const int cnt = min(LPN, j1 - jb);
            float mine = 1.f;
            for (int s0 = 0; s0 < cnt; s0 += UNR) {
                float4 a[UNR][CH];
#pragma unroll
                for (int q = 0; q < UNR; ++q) gather_row<S>(Vt, __shfl(id_l, s0 + q, LPN), li, kp, a[q]);
#pragma unroll
                for (int q = 0; q < UNR; ++q) {
                    const float wh = group_sum<LPN>(nmf_dot<CH>(w, a[q]));
                    mine = (li == s0 + q) ? wh : mine;
                }
            }
            if (mine_ok && x_l > NMF_EPS32) {
                const double wh = (double)(mine < NMF_EPS32 ? NMF_EPS32 : mine);
                s_log += (double)x_l * log((double)x_l / wh);
                s_x += (double)x_l;
            }
        }
    }
    __shared__ double red[256];
    for (int which = 0; which < 2; ++which) {
        red[threadIdx.x] = which ? s_x : s_log;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[(i64)which * gridDim.x + blockIdx.x] = red[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_nmf_divergence_final(const double *__restrict__ partials, int nb,
                                                              const double *__restrict__ w_sum_raw,
                                                              const double *__restrict__ h_sum_raw, int k,
                                                              double *__restrict__ out /*[2]*/) {
    __shared__ double red[256];
    __shared__ double sums[2];
    for (int which = 0; which < 2; ++which) {
        ll_final_body(partials + (i64)which * nb, nb, sums + which, red);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double wh = 0.0;
        for (int z = 0; z < k; ++z) wh += w_sum_raw[z] * h_sum_raw[z];
        const double D = sums[0] + (wh - sums[1]);
        out[0] = sqrt(2.0 * (D > 0.0 ? D : 0.0));
        out[1] = D;
    }
}

}  // namespace plsa
