/*
 * plsa_hip_lda_online.h -- online variational Bayes LDA in libplsa_hip.so (Hoffman, Blei, Bach 2010, algorithm 2; DESIGN.md
 * section 21): the LDA of plsa_hip_diag.h with one global update per block of documents, on a state that outlives its block
 * contexts the way the state of plsa_hip_online.h does.  The reference has no counterpart.
 *
 * A plsa_lda_online state holds lambda [m, kp] float32 (word-major), the table B = exp(psi(lambda) - psi(S_z) - shift_w) formed
 * from it, B's float64 side arrays (S_z and psi(S_z) per topic, the shift per word), the slab partials of the column sums, a
 * step counter t and ONE event.  alpha and eta are fixed scalars.
 *
 * One step on block b -- n_b documents resident on a block context with their own gamma_b:
 *
 *   1. doc_iter - 1 gamma-only rounds and one full round, each a round of the batch fit: A from the block's gamma, the fused
 *      passes with A and THE STATE'S B standing in, gamma <- u N_d + alpha; the last round also leaves the block's raw counts
 *      n_wz in the block context's accumulator.  The block context's own topic table is never read or written.
 *   2. with a = (float)(1 - rho), b = (float)(rho scale), c = (float)(rho eta):
 *          lambda'[w, z] = fmaf(b, n_wz[w, z], fmaf(a, lambda[w, z], c))    for z < k,    exact 0 at the pads k .. kp - 1
 *      (k_lda_online_blend: in place, one sweep, 3 m kp 4 bytes, and the float64 slab sums of lambda' in the layout and the
 *      addition order of the batch fit's own first sweep over lambda, which is therefore never launched).
 *      scale = D / n_b, D the number of documents the corpus has (or is promised to have).
 *   3. B and its side arrays from lambda', by the launches of the batch fit: the S_z of the tables in force have the bits a
 *      fresh context would compute from lambda'.
 *   4. the event is recorded, t += 1.
 *
 * At rho = 1 and scale = 1 a step IS an iteration of plsa_lda_fit on the block, to the bit.
 *
 * Steps and folds on different block contexts are ordered on the device by the state's event: waited for by the block's stream
 * at the start, recorded at the end.  One stream per call, no second stream, no look-ahead buffer set, no hipGraph, no atomics.
 * A step does not wait on the host unless bound_partial is given.
 *
 * Each of these is a status code and a message, launches nothing and leaves the state and the block context as they were:
 * flags without PLSA_FUSED; flags with PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS or PLSA_REFERENCE_LL; a block context in
 * reference arithmetic (plsa_set_arithmetic); a block context that is a shard of a communicator; a block context on another
 * device than the state; a block context whose m, k or kp differ from the state's; a block context without factors; alpha or
 * eta that is not a finite number > 0 (NaN included); doc_iter < 1 (a fold: n_rounds < 0); rho outside (0, 1]; a scale that is
 * not a finite number > 0.
 *
 * The state owns lambda, B, the side arrays and the slab partials: a block context's plsa_release_scratch and plsa_destroy do
 * not free them, and the state survives its block contexts.  It must not outlive its home context.  There are no sample
 * weights; learned and asymmetric priors have no online form yet.
 *
 * Same conventions as plsa_hip.h: status codes (0 = ok), plsa_last_error(ctx) of the context a call was given (the home
 * context for the calls without a block context), borrowed host arrays, not thread-safe.
 *
 * Where this file lives: the listing of include/ is pinned by a test, so the header stands in enstop_amd/include/
 * (INTEGRATION.md section 1m), beside plsa_hip_lda_priors.h.
 */
#ifndef PLSA_HIP_LDA_ONLINE_H
#define PLSA_HIP_LDA_ONLINE_H

#include "../../include/plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plsa_lda_online plsa_lda_online;

/* A state for m words and k topics on the device of `home`, whose stream and staging buffer carry the host copies of lambda.
 * lambda is all 0 until plsa_lda_online_set_lambda. */
int plsa_lda_online_create(plsa_ctx *home, int64_t m, int32_t k, plsa_lda_online **state);

/* Waits for the last step or fold, then frees the state.  NULL is allowed. */
void plsa_lda_online_destroy(plsa_lda_online *state);

/* lambda := lam [k, m] (host, float32), B and the side arrays formed from it, t := 0.  Synchronous. */
int plsa_lda_online_set_lambda(plsa_lda_online *state, const float *lam /* [k, m] */);

/* lambda -> lam [k, m] and the step counter -> *steps, after waiting for the last step or fold.  Either may be NULL. */
int plsa_lda_online_get_lambda(plsa_lda_online *state, float *lam /* [k, m] or NULL */, int64_t *steps /* or NULL */);

/* One step (above) on the block resident on block_ctx.  bound_partial, when given, receives the block's variational bound
 * WITHOUT the topic part -- the likelihood term plus the Dirichlet part of gamma and its constant -- at the gamma the step
 * leaves and the lambda the step started from: what plsa_lda_bound(ctx, alpha, eta, 0, .) returns on a context holding the
 * block, that gamma and that lambda.  It is launched between 1 and 2, so the scalar travels while the update runs; waiting for
 * it is the only host wait of a step. */
int plsa_lda_online_step(plsa_lda_online *state, plsa_ctx *block_ctx, double alpha, double eta, int32_t doc_iter, float thresh,
                         double rho, double scale, int32_t flags, double *bound_partial /* or NULL */);

/* n_rounds gamma-only rounds on the block resident on block_ctx under the state's tables; lambda and t stay. */
int plsa_lda_online_fold(plsa_lda_online *state, plsa_ctx *block_ctx, double alpha, int32_t n_rounds, float thresh,
                         int32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* PLSA_HIP_LDA_ONLINE_H */
