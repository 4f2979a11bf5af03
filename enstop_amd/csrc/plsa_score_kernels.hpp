// plsa_score_kernels.hpp -- per-document log-likelihood, token mass and zero-mass token count (include/plsa_hip_score.h).
//
// k_score_rows<S> is k_loglik with its sums kept per document instead of per workgroup: one lane group owns a document,
// forms dot = sum_z P(w|z) P(z|d) for each stored entry exactly as k_loglik does (the same lane shape S, load_row, the same
// chunk order inside a lane, group_sum), and lane 0 of the group adds the entry's terms to three float64 accumulators in the
// document's entry order.  The three sums of a document are written once, by that lane, with ordinary stores: no atomics,
// no reduction across documents.  So a document's values are a function of its own entries, its P(z|d) row, its weight and
// the P(w|z) rows it touches -- not of the grid, of which group visits it, or of the order the documents are visited in.
//
// A long document is one group's serial walk (the trade k_nmf_divergence makes): correct, and slow for a corpus with a
// few very long rows; row items would need a second, ordered reduction per document and are not built for this pass.
#pragma once

#include "plsa_kernels.hpp"

namespace plsa {

// out: [3][n] float64 -- ll, tokens, unscored.  row_order: the visiting order (descending length) or nullptr.
template <class S>
__global__ __launch_bounds__(256, PLSA_WAVES) void k_score_rows(const int *__restrict__ indptr,
                                                                const int *__restrict__ colidx,
                                                                const float *__restrict__ vals, int n,
                                                                const int *__restrict__ row_order,
                                                                const float *__restrict__ U,
                                                                const float *__restrict__ Vt,
                                                                const float *__restrict__ sw, int kp_rt,
                                                                double *__restrict__ out) {
    constexpr int LPN = S::LPN, CH = S::CH, UNR = S::UNR;
    constexpr int GPB = 256 / LPN;
    const int kp = S::kp(kp_rt);
    const int li = threadIdx.x % LPN;
    const int gid = threadIdx.x / LPN;
    for (i64 r = (i64)blockIdx.x * GPB + gid; r < n; r += (i64)gridDim.x * GPB) {
        const int d = row_order ? row_order[r] : (int)r;
        const int j0 = indptr[d], j1 = indptr[d + 1];
        float4 u[CH];
        load_row<S, true, PLSA_NT_STREAMS>(U + (i64)d * kp, li, kp, u);
        const float swd = sw ? sw[d] : 1.0f;
        double ll = 0.0, tokens = 0.0, unscored = 0.0;
        int w_n = (j0 + li < j1) ? ldi(colidx + j0 + li) : 0;
        float x_n = (j0 + li < j1) ? ldf(vals + j0 + li) : 0.f;
        for (int jb = j0; jb < j1; jb += LPN) {
            const int w_l = w_n;
            const float x_l = x_n;
            const int jn = jb + LPN + li;
            w_n = jn < j1 ? ldi(colidx + jn) : 0;
            x_n = jn < j1 ? ldf(vals + jn) : 0.f;
            const int cnt = min(LPN, j1 - jb);
            for (int s0 = 0; s0 < cnt; s0 += UNR) {
                float4 vt[UNR][CH];
                float x[UNR];
#pragma unroll
                for (int q = 0; q < UNR; ++q) {
                    const int w = __shfl(w_l, s0 + q, LPN);
                    x[q] = __shfl(x_l, s0 + q, LPN);
                    load_row<S, false>(Vt + (i64)w * kp, li, kp, vt[q]);
                }
#pragma unroll
                for (int q = 0; q < UNR; ++q) {
                    float part = 0.f;
#pragma unroll
                    for (int j = 0; j < CH; ++j)
                        part += (vt[q][j].x * u[j].x + vt[q][j].y * u[j].y) + (vt[q][j].z * u[j].z + vt[q][j].w * u[j].w);
                    const float dot = group_sum<LPN>(part);
                    if (li == 0 && s0 + q < cnt && x[q] > 0.f) {          // stored zeros (and negatives, NaN) add nothing
                        if (dot > 0.f) {
                            ll += (double)(x[q] * logf(dot) * swd);      // the float32 term of k_loglik
                            tokens += (double)x[q] * (double)swd;
                        } else if (dot == 0.f) {                          // a word the model gives no mass
                            unscored += (double)x[q] * (double)swd;
                        }
                    }
                }
            }
        }
        if (li == 0) {
            out[d] = ll;
            out[(i64)n + d] = tokens;
            out[2 * (i64)n + d] = unscored;
        }
    }
}

}  // namespace plsa
