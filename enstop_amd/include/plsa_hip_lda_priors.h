/*
 * plsa_hip_lda_priors.h -- variational Bayes LDA in libplsa_hip.so with a vector document-topic prior and with priors that are
 * learned on the way.  The LDA of plsa_hip_diag.h takes two fixed scalars; here alpha is one number per
 * topic (asymmetric: Wallach, Mimno, McCallum 2009), eta stays one number, and either can be re-estimated by maximising the
 * variational bound over it between iterations (Blei, Ng, Jordan 2003, appendix A.4.2).  The reference has no counterpart.
 *
 * The state, the tables, the passes, the scaling and the threshold are those of the LDA section of plsa_hip_diag.h, with
 *
 *   gamma_dz = alpha_z + sum_w x_dw phi_dwz                      lambda_zw = eta + sum_d x_dw phi_dwz
 *
 * and, in the bound, the document constant n [lgamma(sum_z alpha_z) - sum_z lgamma(alpha_z)] and (alpha_z - gamma_dz) where
 * the scalar form has (alpha - gamma_dz).  With every alpha_z equal to one number, gamma and lambda have the bits the scalar
 * entry points leave; the bound agrees within the rounding of its float64 sums (lgamma(sum alpha) is not lgamma(k alpha) to
 * the bit).
 *
 * A prior update.  With gamma fixed the bound depends on alpha through
 *
 *   F(alpha) = n [lgamma(sum_z alpha_z) - sum_z lgamma(alpha_z)] + sum_z alpha_z T_z ,     T_z = sum_d (psi(gamma_dz) - psi(S_d)) ,
 *
 * and with lambda fixed on eta through F(eta) = k [lgamma(m eta) - m lgamma(eta)] + eta T, T = sum_z sum_w (psi(lambda_zw) -
 * psi(S_z)).  Both are concave.  The sums T are formed on the device (k_lda_logmean: float64 slab partials per topic, the slab
 * count a function of the row count alone; k_lda_logmean_sums adds them in a fixed order -- the bits do not depend on the launch
 * geometry), k doubles come back through a page-locked slot, and the host maximises F by Newton's method with the linear-time
 * Hessian.  Every component of a learned prior stays >= 1e-6; an update is kept only if it does not lower F, so no step of a
 * fit lowers the bound.  A prior update from a state close to the random start runs away (all documents look alike there, and
 * the maximising alpha is in the hundreds): prior_start is the burn-in, and callers should not make it small.
 *
 * One stream, no look-ahead buffer set, no hipGraph.  The launch chain of an iteration is the scalar form's with k_lda_rows_v
 * in the place of k_lda_rows; a bound runs k_lda_bound_v on the document side.  The existing entry points run what they ran.
 *
 * There are no sample weights.
 *
 * Each of these is a status code and a message, and launches nothing: a prior component (or eta, where it is read) that is not
 * a finite number > 0 (NaN included); alpha == NULL; prior_start < 1; prior_every < 1; learn outside 0 .. 3; doc_iter < 1;
 * flags without PLSA_FUSED; flags with PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS or PLSA_REFERENCE_LL; a context in
 * reference arithmetic (plsa_set_arithmetic); a context that is a shard of a communicator.
 *
 * The prior vector on the device, the slab partials (8 kp min(4096, rows) bytes) and the page-locked slot belong to the
 * context: kept between calls, freed by plsa_release_scratch and plsa_destroy.
 *
 * Same conventions as plsa_hip.h: status codes (0 = ok), plsa_last_error(ctx), borrowed host arrays, not thread-safe.
 *
 * Where this file lives: the listing of include/ and the plsa_lda names of plsa_hip_diag.h are both pinned by tests, so the
 * header stands in enstop_amd/include/  and moves to include/ when that listing is next opened.
 */
#ifndef PLSA_HIP_LDA_PRIORS_H
#define PLSA_HIP_LDA_PRIORS_H

#include "../../include/plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_iter iterations from the state on the context under the priors alpha [k] and *eta, with the loop of the scalar fit on the
 * bound.  learn: bit 0 re-estimates alpha, bit 1 eta; 0 keeps both fixed.  The priors are updated behind the iterations
 * prior_start, prior_start + prior_every, ... (counted from 1), before the test of the bound that may be due there, which
 * therefore sees the new priors.  A due test is recorded as always; while a prior is learned it cannot stop the loop before
 * the first update has happened.  On return alpha and *eta hold the priors in force at the end.  n_iter, n_iter_per_test,
 * tolerance, doc_iter, thresh, flags, iters_done, bound_trace, n_bound: as in the scalar fit. */
int plsa_lda_prior_fit(plsa_ctx *ctx, double *alpha /* [k] in: start, out: final */, double *eta /* in / out */, int32_t learn,
                       int32_t prior_start, int32_t prior_every, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                       int32_t doc_iter, float thresh, int32_t flags, int32_t *iters_done, float *bound_trace, int32_t *n_bound);

/* The fold-in under a vector prior: gamma alone moves, lambda is never written, nothing is learned. */
int plsa_lda_prior_refit(plsa_ctx *ctx, const double *alpha /* [k] */, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                         int32_t doc_iter, float thresh, int32_t flags, int32_t *iters_done, float *bound_trace,
                         int32_t *n_bound);

/* The bound of the state in force under alpha [k] and eta, float64; with_topics == 0 leaves the topic part out (eta is then
 * not read). */
int plsa_lda_prior_bound(plsa_ctx *ctx, const double *alpha /* [k] */, double eta, int32_t with_topics, double *out);

/* Diagnostic read-back: the sums a prior update would see, t_doc[z] = sum_d (psi(gamma_dz) - psi(S_d)) and
 * t_topic[z] = sum_w (psi(lambda_zw) - psi(S_z)) of the state in force, which stays as it is.  Either pointer may be NULL. */
int plsa_lda_prior_stats(plsa_ctx *ctx, double *t_doc /* [k] or NULL */, double *t_topic /* [k] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PLSA_HIP_LDA_PRIORS_H */
