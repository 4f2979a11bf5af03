/*
 * plsa_hip_score.h -- held-out scoring in libplsa_hip.so: per-document log-likelihood of a corpus under the factors
 * that are on the context.
 *
 * The reference returns one scalar for a whole matrix (log_likelihood, enstop/plsa.py:329-386); choosing n_components by
 * held-out perplexity needs that sum per document, and for the held-out half of each document against the P(z|d) that was
 * just folded in on the other half.  plsa_score_rows is the per-document form of that function, with the factors left
 * where plsa_refit put them.
 *
 * For every document d of the scored matrix and every stored entry (d, w) with count x, with
 *   dot = sum_z P(w|z) P(z|d)      formed as plsa_log_likelihood forms it (float32, the same lane shape and order)
 *   sw_d                           the document's weight (1 without weights)
 *
 *   x > 0 and dot > 0 :  ll[d]       += (double)(x * logf(dot) * sw_d)     the float32 term plsa_log_likelihood adds
 *                        tokens[d]   += (double)x * (double)sw_d
 *   x > 0 and dot == 0:  unscored[d] += (double)x * (double)sw_d           a word the model gives no mass: nothing else
 *   otherwise          :  nothing
 *
 * Stored zeros contribute nothing.  This DIFFERS from plsa_log_likelihood, which lets 0 * log 0 through (NaN, like the
 * reference): ll[d] here is finite whenever the factors are, and unscored[d] says how much of the document it leaves out.
 * An empty document gives +0.0 in all three outputs.
 *
 * The sums are float64, taken in the document's entry order by the one lane that owns the document.  No atomics, no sum
 * across documents: a document's three values have the same bits whatever the grid, the order the documents are visited in
 * (PLSA_SORT_ROWS), PLSA_FORCE_WIDE, PLSA_PACKED, PLSA_ROW_ITEMS, and whatever the context did before.
 * plsa_set_arithmetic does NOT affect this entry point: it always runs the default arithmetic described above.
 *
 * Same conventions as plsa_hip.h: status codes (0 = ok), plsa_last_error(ctx), borrowed host arrays, not thread-safe.
 */
#ifndef PLSA_HIP_SCORE_H
#define PLSA_HIP_SCORE_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scores the ACTIVE matrix (indptr = indices = data = NULL, nnz = 0) or ANOTHER matrix given as host CSR arrays.
 *
 * Another matrix has the active matrix's n rows and m columns -- the shapes of the factors; there is no other shape to
 * pass.  indptr has n + 1 entries with indptr[0] == 0 and indptr[n] == nnz, nnz < 2^31, column ids in [0, m), row
 * pointers non-decreasing: the last two are checked on the device by the check plsa_upload_csr runs, and a violation is a
 * status and a message.  The matrix is copied into scratch buffers of the context (4 (n + 1) + 8 nnz bytes, kept between
 * calls, freed by plsa_release_scratch).  It does not replace the resident corpus, does not move the factors and does not
 * invalidate any derived structure, packed stream or P(z|w,d): a fit or refit after the call behaves as if the call had
 * not happened.
 *
 * sw: [n] document weights or NULL -- plsa_log_likelihood's convention: NULL means the weights made resident by
 * plsa_set_sample_weight, or 1 when there are none.
 * ll, tokens, unscored: [n] each; any may be NULL, not all three.
 *
 * Each of these is a status code and launches nothing: no corpus uploaded; factors not set, or set for another n or m;
 * k outside [1, 1024]; only some of indptr / indices / data given, nnz < 0, or indptr[0] != 0 or indptr[n] != nnz;
 * nnz >= 2^31; all three outputs NULL.
 *
 * Runs on the context's stream and returns after its own copies have landed. */
int plsa_score_rows(plsa_ctx *ctx, const int32_t *indptr /* [n+1] or NULL */, const int32_t *indices /* [nnz] or NULL */,
                    const float *data /* [nnz] or NULL */, int64_t nnz, const float *sw /* [n] or NULL */,
                    double *ll /* [n] or NULL */, double *tokens /* [n] or NULL */, double *unscored /* [n] or NULL */);

#ifdef __cplusplus
}
#endif
#endif
