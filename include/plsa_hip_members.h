/*
 * plsa_hip_members.h -- batched ensemble members of libplsa_hip.so.
 *
 * The reference fans the bootstrapped fits of an ensemble out over a thread pool and stacks their topics with np.vstack
 * (enstop/enstop_.py:164-231: the fan-out at :209-217, the serial branch at :220-223, the stack order at :225-231).  On
 * one GPU a 20-Newsgroups-sized fit is a chain of short dependent launches that does not fill the device; a BATCH
 * advances B members (same base corpus, different bootstrap resamples and initial factors) through the fused EM
 * schedule together, each kernel of an iteration launched ONCE for all members.
 *
 * Contract: member r's topics, iteration count and log-likelihood trace are, bit for bit, what plsa_bootstrap +
 * plsa_init_factors_mt19937 / plsa_set_factors + plsa_fit give on a context of its own.  The likelihood test
 * (enstop/plsa.py:630-638) is evaluated per member; a member that stops keeps the factors the standalone loop returns
 * and costs no further work.  Calls a batch cannot carry (flags without PLSA_FUSED, PLSA_REFERENCE_SUMS /
 * PLSA_REFERENCE_LL, PLSA_SHARDED, PLSA_GRAPH, timing on, 64-bit gather tables) and members whose kernel instantiation
 * no other member shares run through plsa_fit, one after the other: same results.
 *
 * Same conventions as plsa_hip.h: status codes, plsa_last_error(ctx) of the context the batch was created on, borrowed
 * host arrays.  A batch belongs to its context, shares its streams and its base corpus, and must be destroyed before it.
 * Like the context it is not thread-safe.
 */
#ifndef PLSA_HIP_MEMBERS_H
#define PLSA_HIP_MEMBERS_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plsa_members plsa_members;

enum { PLSA_MEMBERS_MAX = 64 };   /* members per batch: the live set travels to the kernels as one 64-bit word */

/* A batch of `n_members` (1 .. PLSA_MEMBERS_MAX) member slots on `ctx`.  The slots keep their device buffers between
 * fits (successive batches of one ensemble, successive ensembles): create once, prepare + fit many times. */
int plsa_members_create(plsa_ctx *ctx, int32_t n_members, plsa_members **out);
void plsa_members_destroy(plsa_members *batch);

/* How many members of k topics over the corpus resident on `ctx` fit into half of the HBM that is free right now
 * (0 .. PLSA_MEMBERS_MAX): the cap of a batch. */
int plsa_members_capacity(plsa_ctx *ctx, int32_t k, int32_t *max_members);

/* Member `member` := the rows idx[0 .. n_out) of the corpus resident on the batch's context (enstop_.py:86-88; idx == NULL:
 * the corpus itself), with k topics initialised either from the MT19937 state `mt_state_io` ([625]: plsa_init(random)
 * drawn on the device, the advanced state is written back -- plsa_init_factors_mt19937) or, when mt_state_io is NULL,
 * from the host factors U [n_out, k] and V [k, m] (plsa_set_factors). */
int plsa_members_prepare(plsa_members *batch, int32_t member, const int64_t *idx, int64_t n_out, int32_t k,
                         uint32_t *mt_state_io, const float *U, const float *V);

/* plsa_fit for the first `n_active` members (all prepared with the same k), sample weights all one (enstop_.py:91).
 * iters_done[n_active], n_ll[n_active]; ll_trace[n_active * ll_cap] (row r: member r's likelihoods, ll_cap >= n_iter + 2)
 * or NULL.  n_batched (or NULL): how many of the members went through batched launches (the others through plsa_fit). */
int plsa_members_fit(plsa_members *batch, int32_t n_active, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                     float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t ll_cap, int32_t *n_ll,
                     int32_t *n_batched);

/* member's P(w|z) [k, m] to DEVICE memory `dst` (a slot of plsa_stack_reserve: the np.vstack of enstop_.py:225-231) */
int plsa_members_copy_components(plsa_members *batch, int32_t member, void *dst);

/* The member's own context, BORROWED (never plsa_destroy it; it dies with the batch): plsa_get_factors, plsa_active_shape and
 * the reports of plsa_hip_diag.h (plsa_pass_info, plsa_packed_info, plsa_schedule_info) apply to a member through it. */
int plsa_members_context(plsa_members *batch, int32_t member, plsa_ctx **out);

/* How member `member` ran in the last plsa_members_fit: info[0] launch group (-1: plsa_fit), [1] members in that group,
 * [2] row items in use, [3] row item length, [4] chunk rows of the column pass, [5] heavy columns, [6] grid of the document
 * pass (= partials of its fused log-likelihood), [7] grid of its first norm stage (0: one stage). */
int plsa_members_info(plsa_members *batch, int32_t member, int32_t *info /*[8]*/);

/* The float64 log-likelihood behind the member's last likelihood test of the last plsa_members_fit (ll_trace holds it
 * rounded to float32, like the reference's trace): the fixed-order sum of one partial per workgroup of the member's own
 * document-pass grid. */
int plsa_members_last_ll(plsa_members *batch, int32_t member, double *ll);

/* free what the batch holds on the device (slots stay usable: buffers are re-created by the next prepare) */
int plsa_members_release(plsa_members *batch);

#ifdef __cplusplus
}
#endif
#endif
