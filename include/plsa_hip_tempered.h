/*
 * plsa_hip_tempered.h -- tempered EM in libplsa_hip.so (Hofmann 1999 / 2001): EM iterations whose responsibilities are
 * flattened by an exponent 0 < beta <= 1, and one snapshot slot for the factors, so that a host loop can stop on a held-out
 * score (plsa_hip_score.h), go back to the best factors and lower beta.  The reference has no counterpart.
 *
 *   P_beta(z|d,w) = (P(z|d) P(w|z))^beta / sum_z' (P(z'|d) P(w|z'))^beta ,  and  (P(z|d) P(w|z))^beta = P(z|d)^beta P(w|z)^beta .
 *
 * So one tempered iteration is: raise the two factor tables to the power beta, element by element, into two side tables
 * (k (n + m) powers; inside the passes it would be 2 nnz k), then run the ordinary fused iteration with the side tables as
 * its inputs and the ordinary factor buffers as its outputs.  Both fused passes normalise their outputs by the sums they
 * accumulate themselves, so the new P(z|d) and P(w|z) are the tempered M-step's.  The passes are the ones plsa_fit runs.
 *
 * The power: out = x > 0 ? (float)pow((double)x, beta) : 0.  Exact zeros stay exact zeros, the pad columns too; float32
 * denormals are kept on both sides; every entry is within 1 float32 ulp of the correctly rounded x^beta.
 *
 * One stream, no look-ahead buffer set, no hipGraph: the launch chain of an iteration is k_temper (twice),
 * k_row_pass<fused>, k_col_pass<fused> and the column tail, in that order on the context's stream.
 *
 * Same conventions as plsa_hip.h: status codes (0 = ok), plsa_last_error(ctx), borrowed host arrays, not thread-safe.
 */
#ifndef PLSA_HIP_TEMPERED_H
#define PLSA_HIP_TEMPERED_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_iter tempered EM iterations at `beta` from the factors on the context, with plsa_fit's arguments, loop and stop rule:
 * a likelihood of the initial factors, then one after every n_iter_per_test-th iteration, the stop on its relative change
 * against `tolerance` (tolerance = 0 never stops on it).  The call is stateless in beta: nothing of it outlives the call, and
 * no other entry point ever sees a temperature.
 *
 * Every likelihood of the trace is the likelihood of the TRUE factors (a launch of k_loglik, as plsa_log_likelihood), never
 * the tempered dot product the document pass could carry along.
 *
 * beta == 1.0 calls plsa_fit with the same arguments and does nothing else.
 *
 * sw, n_iter, n_iter_per_test, tolerance, thresh, iters_done, ll_trace, n_ll: as in plsa_fit.  flags: PLSA_FUSED is required;
 * PLSA_TRACE_LL, PLSA_SW_LL_ONLY and PLSA_STOP_NO_ZERO_ARM mean what they mean there.
 *
 * Each of these is a status code and a message, and launches nothing: beta outside (0, 1] (NaN included); flags without
 * PLSA_FUSED; flags with PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS or PLSA_REFERENCE_LL; a context in reference
 * arithmetic (plsa_set_arithmetic).
 *
 * The two side tables belong to the context: 4 kp (n + m) bytes, kept between calls, freed by plsa_release_scratch and
 * plsa_destroy. */
int plsa_fit_tempered(plsa_ctx *ctx, const float *sw /* [n] or NULL */, double beta, int32_t n_iter, int32_t n_iter_per_test,
                      double tolerance, float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll);

/* Device-to-device copy of the current P(z|d) and P(w|z) into the context's one snapshot slot (4 kp (n + m) bytes, freed by
 * plsa_release_scratch and plsa_destroy).  A second snapshot replaces the first. */
int plsa_factors_snapshot(plsa_ctx *ctx);

/* The snapshot becomes the current factors again, bit for bit; the slot keeps it.  An error without a snapshot (none taken,
 * or freed by plsa_release_scratch) and when the active matrix's shape or k is no longer the one it was taken for. */
int plsa_factors_restore(plsa_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
