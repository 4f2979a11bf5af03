/*
 * plsa_hip_nmf.h -- Kullback-Leibler NMF by multiplicative updates in libplsa_hip.so.
 *
 * The reference fits its model="nmf" members with scikit-learn's NMF(beta_loss=1, solver="mu", alpha=0)
 * (enstop/enstop_.py).  These entry points restate that solver -- sklearn/decomposition/_nmf.py, version 1.7, sparse X,
 * gamma = 1, no regularisation -- on the matrix that is ACTIVE on the context (the uploaded corpus or its current bootstrap
 * resample), on the structures the fused EM passes already keep there.  With EPS32 = np.finfo(np.float32).eps:
 *
 *   (WH)_dw < EPS32 -> EPS32 before every quotient x_dw / (WH)_dw     (_special_sparse_dot + the guard of both updates)
 *   W[d,:] <- W[d,:] * (sum_{w in d} x_dw / (WH)_dw * H[:,w]) / H_sum, a zero H_sum[z] read as EPS32
 *   H[:,w] <- H[:,w] * (sum_{d in w} x_dw / (WH)_dw * W[d,:]) / W_sum, a zero W_sum[z] read as 1; then H < 2^-52 -> 0
 *
 * Factors are float32, W [n,k] and H [k,m] row-major on the host.  They share the device buffers of the pLSA factors: a
 * pLSA call after an NMF call starts from its own plsa_set_factors / plsa_init_factors_* and behaves as on a fresh context,
 * and the other way round.  No float atomics: every result is bit-reproducible from run to run and does not depend on
 * what the context did before.
 *
 * Same conventions as plsa_hip.h: status codes (0 = ok), plsa_last_error(ctx), borrowed host arrays, not thread-safe.  A
 * context without a corpus, without NMF factors for the active matrix, or k outside [1, 1024] is a status code: nothing
 * is launched.
 */
#ifndef PLSA_HIP_NMF_H
#define PLSA_HIP_NMF_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The starting point NMF(init="custom") takes: values stored unchanged (neither normalised nor clamped). */
int plsa_nmf_set_factors(plsa_ctx *ctx, const float *W /* [n*k] */, const float *H /* [k*m] */, int64_t n, int64_t m,
                         int32_t k);
/* The current factors, unchanged; either pointer may be NULL. */
int plsa_nmf_get_factors(plsa_ctx *ctx, float *W /* [n*k] */, float *H /* [k*m] */);

/* sklearn.decomposition._nmf._multiplicative_update_w (beta_loss = 1): one W half-iteration, H_sum from the current H. */
int plsa_nmf_update_w(plsa_ctx *ctx);
/* sklearn.decomposition._nmf._multiplicative_update_h (beta_loss = 1) and the H[H < float64 eps] = 0 that
 * _fit_multiplicative_update applies after it: one H half-iteration, reading the current W. */
int plsa_nmf_update_h(plsa_ctx *ctx);

/* sklearn.decomposition._nmf._beta_divergence(X, W, H, 1, square_root=True):
 *   sqrt(2 max(D, 0)),  D = sum_{x > EPS32} x log(x / max(WH, EPS32)) + W_sum . H_sum - sum_{x > EPS32} x
 * over the stored entries, float64 sums in a fixed order. */
int plsa_nmf_divergence(plsa_ctx *ctx, double *sqrt2d);

/* sklearn.decomposition._nmf._fit_multiplicative_update: up to max_iter iterations (W half, then the H half unless
 * update_h == 0).  error_at_init is taken before the first update; when tol > 0 the objective is evaluated every 10
 * iterations and the loop stops when (previous - error) / error_at_init < tol.  *n_iter is the iteration of the stopping
 * test, or max_iter.  errors[0] = error_at_init, errors[i] = the i-th tested error, as far as errors_len allows (errors
 * may be NULL).  The loop runs on the library's side; the host is consulted at the tests only.  max_iter < 1 is a status
 * code. */
int plsa_nmf_fit(plsa_ctx *ctx, int update_h, int max_iter, double tol, int32_t *n_iter, double *errors /* [errors_len] */,
                 int32_t errors_len);

#ifdef __cplusplus
}
#endif
#endif
