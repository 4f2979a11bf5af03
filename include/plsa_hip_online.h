/*
 * plsa_hip_online.h -- online (stepwise) EM in libplsa_hip.so (Cappe & Moulines 2009; Liang & Klein 2009): P(w|z) is updated
 * after every block of documents from a running sufficient statistic and a decaying step size, instead of once per pass over
 * the corpus.  The reference has no counterpart.
 *
 * State (an opaque plsa_online): the topics V = P(w|z) and the statistic S, both word-major [m, kp] float32 on the device
 * like a context's own topic table (kp: k rounded up to a multiple of 4), a step counter t, and one event.  Host arrays of
 * V and S are [k, m] float32, the layout of plsa_set_factors.
 *
 * One step on a block context (a plsa_ctx holding a block of whole documents with factors set for the same m and k):
 *   1. inner fold-in: inner_iter frozen-topic iterations over the block's rows under the state's V -- the document pass of
 *      the fused plsa_refit; only the block's P(z|d) moves;
 *   2. accumulate: the fused passes of plsa_em_accumulate under the state's V; the block's P(z|d) rows are then final and its
 *      accumulator holds the block's un-normalised P(w|z) sums Vacc; ll_partial, when asked for, is the log-likelihood of the
 *      block under the factors the accumulate started from;
 *   3. global update: S' = fmaf(b, Vacc, a * S) in float32 with a = (float)(1 - rho) and b = (float)(rho * scale), both
 *      rounded once on the host; norm[z] = the float64 fixed-order column sum of S' (the slab order of plsa_em_finish's
 *      norm), rounded to float32; V' = S' / norm where the norm is positive, as plsa_em_finish divides.  The pad columns
 *      k .. kp stay zero in both.
 * The state's V stands in the place the block's passes read for the length of the chain; the block's own topic table is not
 * copied, read or written.  With rho = 1, scale = 1 and a finite S, a step with inner_iter = 0 leaves in V and in the block's
 * P(z|d) the bits plsa_em_accumulate + plsa_em_finish leave on a context with the same rows and factors.
 *
 * One stream, no look-ahead buffer set, no hipGraph: the launch chain of a step is k_row_pass<fused> (inner_iter + 1 times),
 * k_col_pass<fused>, k_col_reduce, k_online_blend, k_colsum_final and k_v_normalise, in that order on the block context's
 * stream.  Steps and folds on different contexts are ordered on the device by the state's event, which the stream waits for at
 * the start of a call and which is recorded at its end; a step involves no host wait unless ll_partial is asked for (or
 * weights are passed from the host: make them resident with plsa_set_sample_weight instead).
 *
 * Each of these is a status code and a message on the block context, launches nothing and leaves state and factors as they
 * were: flags without PLSA_FUSED; flags with PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS or PLSA_REFERENCE_LL; a context in
 * reference arithmetic (plsa_set_arithmetic) or with a communicator; a block whose m or k differs from the state's, or on
 * another device; rho outside (0, 1] (NaN included); a scale that is not a positive finite number; a negative iteration count.
 *
 * The state owns its tables: plsa_release_scratch and plsa_destroy of a block context leave it valid.  The home context lends
 * its device, its stream and a staging buffer to the host copies of V and S and must outlive the state.
 *
 * Same conventions as plsa_hip.h: status codes (0 = ok), plsa_last_error(ctx), borrowed host arrays, not thread-safe.
 */
#ifndef PLSA_HIP_ONLINE_H
#define PLSA_HIP_ONLINE_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plsa_online plsa_online;

/* A state for m words and k topics on the home context's device; V and S start as zeros, t = 0.  2 * 4 m kp bytes. */
int plsa_online_create(plsa_ctx *home_ctx, int64_t m, int32_t k, plsa_online **state);

/* Waits for the last step, then frees the state. */
void plsa_online_destroy(plsa_online *state);

/* V := the given topics, S := V / k (every entry divided by (float)k in float32), t := 0.  Synchronous. */
int plsa_online_set_topics(plsa_online *state, const float *V /* [k, m] */);

/* The current topics, after every step enqueued so far. */
int plsa_online_get_topics(plsa_online *state, float *V /* [k, m] */);

/* The statistic and the step counter, either may be NULL; plsa_online_statistic_set replaces S alone (V and t stay): tests
 * and warm starts. */
int plsa_online_statistic_get(plsa_online *state, float *S /* [k, m] or NULL */, int64_t *steps /* or NULL */);
int plsa_online_statistic_set(plsa_online *state, const float *S /* [k, m] */);

/* One step as defined above.  sw: document weights of the block, [n] or NULL (NULL: the resident weights, if any), applied
 * as plsa_em_accumulate applies them.  thresh: the E-step threshold of plsa_fit.  flags: PLSA_FUSED.  ll_partial: NULL, or
 * where the block's log-likelihood goes. */
int plsa_online_step(plsa_online *state, plsa_ctx *block_ctx, const float *sw, int32_t inner_iter, float thresh, double rho,
                     double scale, int32_t flags, double *ll_partial);

/* n_iter frozen-topic iterations over the block's rows under the state's V, nothing else: neither V, S nor t change. */
int plsa_online_fold(plsa_online *state, plsa_ctx *block_ctx, const float *sw, int32_t n_iter, float thresh, int32_t flags);

#ifdef __cplusplus
}
#endif
#endif
